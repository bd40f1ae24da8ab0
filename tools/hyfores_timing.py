"""Time the stored-filter apply and the HyFoReS gain and window sums (csrc/hyfores.hip) against their byte floors.

    python tools/hyfores_timing.py [--shape NPOL,NFREQ,NEW,NEL,NRA ...] [--out profiles/hyfores_timing.json]

Default shapes: 2 pol x 64 freq x 4 ew x 64 el x 2048 RA and 2 x 128 x 4 x 8 x 2048, the stream of
tools/dayenu_hybrid_timing.py (unit noise, weights in 0.5 ... 1.5, eight channel masks over the RA, true DAYENU filters
with tauw 0.4 and epsilon 1e-3).  The filter dataset is written by ``dmm_dayenu_hybrid_save``, the store stream of the
filter task, which is timed in the same session: its rate is the yardstick.  Every entry point is warmed up once at the
same shape and timed with a host clock around work that ends in a device synchronise.

Reported per shape and entry point: seconds, the once-through bytes (``filter``, ``vis`` and ``post`` each read once,
the weights and masks read once, the outputs written once), and the ratio of the time to what those bytes would take at
the store stream's measured rate; the float64 operations of the sums counted from the shapes.  ``apply`` is
``dmm_hybrid_filter_apply`` with ``weight_out`` (its scan of the filter for the sample status and the weights, and its
product); ``apply_cov`` adds ``freq_cov``.  The window's operations are those of the full product over all ``nfreq^2``
pairs; the kernel forms the Gram tiles on and below the diagonal only, ``(ntile + 1) / (2 ntile)`` of them.  For context the float64 NumPy twin's estimate for one (pol, ew) on the same
host, run on the first ``--twin-ra`` RA and scaled to the whole axis.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def time_shape(shape, repeats, twin_ra):
    import numpy as np

    import hyfores_twin as twin
    from dayenu_hybrid_timing import inputs
    from draco_amd import _lib
    from draco_amd.analysis import dayenu, hyforesbandpass
    from draco_amd.device import Context, ptr

    npol, n, new, nel, nra = shape
    ctx = Context.get()
    lib = _lib.lib
    freq, vis, weight = inputs(np, shape)

    def clock(fn):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return time.perf_counter() - t0, r

    def best(fn):
        ts = [clock(fn)[0] for _ in range(repeats + 1)]  # (the first is the warm-up)
        return min(ts[1:])

    vis_d, w_d = ctx.to_device(vis), ctx.to_device(weight)
    flag_d = ctx.empty((n, new, nra), np.uint8)
    _lib.check(lib.dmm_dayenu_hybrid_mask(ctx.handle, npol, n, new, nra, ptr(w_d), ptr(flag_d)))
    masks, index = dayenu._group_rows(np.ascontiguousarray(flag_d.cpu().numpy().reshape(n, new * nra).T))
    bands = dayenu._bands(0.4, 0.0, 1e-3)
    nf, status = dayenu.build_filters(ctx, ctx.to_device(freq), np.repeat(bands[np.newaxis], masks.shape[0], axis=0), masks)
    assert not status.any()
    imat_d = ctx.to_device(index.astype(np.int32))
    filt = ctx.empty((npol, n, n, new, nra), np.float64)
    t_save = best(lambda: _lib.check(lib.dmm_dayenu_hybrid_save(ctx.handle, npol, n, new, nra, ptr(nf), masks.shape[0], ptr(imat_d), 0, ptr(filt))))
    mat_bytes = npol * n * n * new * nra * 8
    rate = mat_bytes / t_save

    post = ctx.empty(vis_d.shape, np.complex64)
    w_out = ctx.empty(w_d.shape, np.float32)
    cov = ctx.empty(filt.shape, np.float64)
    bits = ctx.empty((npol, new, nra), np.int32)
    st = ctx.empty((npol, new, nra), np.uint8)

    def apply(c):
        _lib.check(lib.dmm_hybrid_filter_apply(ctx.handle, npol, n, new, nel, nra, ptr(filt), ptr(vis_d), ptr(w_d), None, None, 0, 0, ptr(post), ptr(w_out), ptr(c), ptr(bits), ptr(st)))

    t_apply = best(lambda: apply(None))
    t_apply_cov = best(lambda: apply(cov))
    assert int((st != _lib.DMM_HFA_OK).sum()) == 0
    del cov
    elm = ctx.to_device(np.ones(nel, dtype=np.uint8))
    pix = ctx.to_device((np.random.default_rng(3).random((npol, n, nel, nra)) < 0.1).astype(np.uint8))
    yn, d = ctx.empty((npol, new, n), np.complex128), ctx.empty((npol, new, n), np.float64)
    win = ctx.empty((npol, new, n, n), np.complex128)
    part = ctx.empty((-(-nra // _lib.DMM_HYFORES_RUN), npol, new, n, n), np.complex128)
    t_gain = best(lambda: _lib.check(lib.dmm_hyfores_gain(ctx.handle, npol, n, new, nel, nra, ptr(vis_d), ptr(post), ptr(w_out), ptr(elm), ptr(pix), ptr(yn), ptr(d))))
    t_window = best(lambda: _lib.check(lib.dmm_hyfores_window(ctx.handle, npol, n, new, nel, nra, ptr(filt), ptr(vis_d), ptr(post), ptr(w_out), ptr(elm), ptr(pix), ptr(part), ptr(win))))
    t_est = best(lambda: hyforesbandpass.estimate(ctx, vis_d, post, w_out, filt, elm, pix))

    # ---- the float64 NumPy twin's estimate for one (pol, ew), on the first RA
    ra = min(twin_ra, nra)
    pv, pw, pf = post[:1, :, :1, :, :ra].cpu().numpy(), w_out[:1, :, :1, :ra].cpu().numpy(), filt[:1, :, :, :1, :ra].cpu().numpy()
    t0 = time.perf_counter()
    twin.estimate(vis[:1, :, :1, :, :ra], pv, pw, pf, np.ones(nel, dtype=bool), pix[:1, :, :, :ra].cpu().numpy().astype(bool))
    t_twin = (time.perf_counter() - t0) * nra / ra

    nsample = npol * new * nra
    small = weight.nbytes + pix.numel()
    by = {
        "apply": mat_bytes + 2 * vis.nbytes + 2 * weight.nbytes,
        "apply_cov": 2 * mat_bytes + 2 * vis.nbytes + 2 * weight.nbytes,
        "gain": 2 * vis.nbytes + small,
        "window": mat_bytes + 2 * vis.nbytes + small + 2 * part.numel() * 16,
    }
    flop = {
        "apply": nsample * (4.0 * n * n * nel + 3.0 * n * n),
        "apply_cov": nsample * (4.0 * n * n * nel + 3.0 * n * n + 3.0 * n * n * (n + 4) / 2),
        "gain": nsample * n * nel * 14.0,
        "window": nsample * n * n * (8.0 * nel + 2),
    }
    ts = {"apply": t_apply, "apply_cov": t_apply_cov, "gain": t_gain, "window": t_window}
    return {
        "shape": {"npol": npol, "nfreq": n, "new": new, "nel": nel, "nra": nra},
        "store_stream": {"entry": "dmm_dayenu_hybrid_save", "s": t_save, "bytes": mat_bytes, "tb_per_s": rate / 1e12},
        "entries": {k: {"s": ts[k], "once_through_bytes": by[k], "tb_per_s": by[k] / ts[k] / 1e12, "time_over_byte_floor": ts[k] / (by[k] / rate), "f64_flop": flop[k],
                        "tflops": flop[k] / ts[k] / 1e12} for k in ts},
        "estimate_gain_window_and_copy_back_s": t_est,
        "numpy_twin_estimate_one_pol_ew_s_extrapolated": t_twin,
        "numpy_twin_ra": ra,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="NPOL,NFREQ,NEW,NEL,NRA (repeatable)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--twin-ra", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    shapes = [tuple(int(x) for x in s.split(",")) for s in args.shape] if args.shape else [(2, 64, 4, 64, 2048), (2, 128, 4, 8, 2048)]
    doc = {"tool": "tools/hyfores_timing.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "cases": []}
    for shape in shapes:
        res = time_shape(shape, args.repeats, args.twin_ra)
        doc["cases"].append(res)
        print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
