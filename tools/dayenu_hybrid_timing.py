"""Time the DAYENU filter of hybrid visibilities and the east-west averages of RADependentWeights, stage by stage.

    python tools/dayenu_hybrid_timing.py [--shape NPOL,NFREQ,NEW,NEL,NRA ...] [--out profiles/dayenu_hybrid_timing.json]
    python tools/dayenu_hybrid_timing.py --merge-stats <rocprofv3 kernel stats csv> --out profiles/dayenu_hybrid_timing.json

Default shapes: 2 pol x 64 freq x 4 ew x 64 el x 2048 RA and 2 x 128 x 4 x 8 x 2048.  The stream carries unit noise and
float32 weights in 0.5 ... 1.5; eight distinct channel masks over the RA (sorted, so that a mask covers a run of RA)
zero 3 % of the weights, the same channels in both polarisations.  The filters are true DAYENU filters (tauw 0.4,
epsilon 1e-3).  Every stage is called as ``DayenuDelayFilterHybridVis`` / ``RADependentWeights`` call it, warmed up
once at the same shape and timed with a host clock around work that ends in a device synchronise; the task as a whole
(apply + save + cov) is timed too.

Reported per shape: seconds per stage (mask with its copy to the host and the grouping, build, apply, save,
covariance, east-west coefficients and scaling, east-west averages); the bytes the streaming stages move and the
float64 operations of the matrix-core stages, counted from the shapes as executed; their rates against 6.1 TB/s (the
read-once stream of DESIGN.md 7k) and the FP64 matrix-core peak (78.6 TFLOP/s); for context the float64 NumPy twin's
time for one (ew, ra) column on the same host.

Operations, n = nfreq, n16 = n rounded up to 16:
  apply        2 n16 n16' per column, n16' = n rounded up to 32 rows, columns = 2 nel + 1 per (pol, ew, ra)
  covariance   per (pol, ew, ra): the 16-row tiles f' <= f of every row f, each 2 x 16 x n16 (about n^3 + 16 n^2; the
               issue's count of the full product is 2 n^3), plus one multiply per 4 x 4 of them to form the A operand
"""

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F64 = 78.6e12
HBM_STREAM = 6.1e12
DF = 0.390625


def inputs(np, shape, seed=11):
    npol, n, new, nel, nra = shape
    rng = np.random.default_rng(seed)
    freq = 600.0 + DF * np.arange(n)
    masks = np.ones((8, n), dtype=bool)
    for m in masks[1:]:
        m[rng.choice(np.arange(1, n - 1), size=max(1, round(0.03 * n * 8 / 7)), replace=False)] = False
    which = np.sort(rng.integers(8, size=(new, nra)), axis=1)
    vis = (rng.standard_normal((npol, n, new, nel, nra), dtype=np.float32) + 1j * rng.standard_normal((npol, n, new, nel, nra), dtype=np.float32)).astype(np.complex64)
    weight = (0.5 + rng.random((npol, n, new, nra), dtype=np.float32)).astype(np.float32)
    weight *= np.moveaxis(masks[which], -1, 0)[np.newaxis].astype(np.float32)
    return freq, vis, weight


def time_shape(shape, repeats):
    import ctypes as C

    import numpy as np
    import torch

    import dayenu_hybrid_twin as twin
    from draco_amd import _lib
    from draco_amd.analysis import dayenu
    from draco_amd.analysis.ringmapmaker import RADependentWeights
    from draco_amd.core import containers
    from draco_amd.device import Context, ptr

    npol, n, new, nel, nra = shape
    ctx = Context.get()
    lib = _lib.lib
    freq, vis, weight = inputs(np, shape)
    cfg = dict(tauw=0.4, epsilon=1e-3, apply_filter=True, save_filter=True, calculate_cov=True)

    def clock(fn):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return time.perf_counter() - t0, r

    def best(fn, prepare=None):
        ts = []
        for i in range(repeats + 1):  # (the first is the warm-up)
            if prepare:
                prepare()
            ts.append(clock(fn)[0])
        return min(ts[1:])

    vis_d, w_d = ctx.to_device(vis), ctx.to_device(weight)
    vis0, w0 = vis_d.clone(), w_d.clone()
    bands = dayenu._bands(cfg["tauw"], 0.0, cfg["epsilon"])
    freq_d = ctx.to_device(freq)
    flag_d = ctx.empty((n, new, nra), np.uint8)
    state = {}

    def mask():
        _lib.check(lib.dmm_dayenu_hybrid_mask(ctx.handle, npol, n, new, nra, ptr(w_d), ptr(flag_d)))
        flags = np.ascontiguousarray(flag_d.cpu().numpy().reshape(n, new * nra).T)
        masks, index = dayenu._group_rows(flags)
        assert index.min() >= 0
        state["masks"], state["imat"] = masks, index.astype(np.int32)

    t_mask = best(mask)
    masks, imat = state["masks"], state["imat"]
    nmat = masks.shape[0]

    def build():
        state["nf"], status = dayenu.build_filters(ctx, freq_d, np.repeat(bands[np.newaxis], nmat, axis=0), masks)
        assert not status.any()

    t_build = best(build)
    nf = state["nf"]
    imat_d = ctx.to_device(imat)
    out = ctx.empty((npol, n, n, new, nra), np.float64)
    cov = ctx.empty((npol, n, n, new, nra), np.float64)
    t_save = best(lambda: _lib.check(lib.dmm_dayenu_hybrid_save(ctx.handle, npol, n, new, nra, ptr(nf), nmat, ptr(imat_d), 0, ptr(out))))
    t_cov = best(lambda: _lib.check(lib.dmm_dayenu_hybrid_cov(ctx.handle, npol, n, new, nra, ptr(nf), nmat, ptr(imat_d), ptr(w_d), 0, ptr(cov))))

    wide_d = ctx.to_device(np.repeat(imat, 2))
    vr = torch.view_as_real(vis_d)

    def apply():
        for pp in range(npol):
            data = dayenu._side(vr[pp], nel, 2 * new * nel * nra, 2 * nra, 1, 2 * nel * nra)
            wside = dayenu._side(w_d[pp], 1, new * nra, 0, 1, nra)
            dayenu.apply_filters(ctx, _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_ITEMS, n, 2 * nra, new, nf, wide_d, None, None, new * (-(-2 * nra // 32)), data, None)
            dayenu.apply_filters(ctx, _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_ITEMS, n, nra, new, nf, imat_d, None, None, new * (-(-nra // 32)), None, wside)

    def restore():
        vis_d.copy_(vis0)
        w_d.copy_(w0)

    t_apply = best(apply, restore)

    # ---- the east-west averages, on the filtered stream
    table_d = ctx.to_device((new - np.arange(new)).astype(np.float64))
    cf, cc, w2 = (ctx.empty((npol, n, new), np.float64) for _ in range(3))
    num = ctx.empty((npol, n), np.float64)
    rw = ctx.to_device(np.ones((npol, n, nra, nel)))
    ring = ctx.empty((npol, n, n, nra), np.float64)

    def coef_scale():
        _lib.check(lib.dmm_ew_coef(ctx.handle, npol, n, new, nra, _lib.DMM_EW_TABLE, ptr(table_d), ptr(w_d), ptr(cf), ptr(cc), ptr(w2), ptr(num)))
        _lib.check(lib.dmm_ew_scale(ctx.handle, npol, n, new, nra, nel, ptr(w_d), ptr(w2), ptr(num), ptr(rw)))

    t_coef = best(coef_scale)
    t_avg = best(lambda: _lib.check(lib.dmm_ew_average(ctx.handle, npol * n * n, n, new, nra, ptr(cf), ptr(out), ptr(ring))))
    del out, cov, ring

    # ---- the two tasks as a whole
    def task_run():
        s = containers.HybridVisStream(pol=np.array(["XX", "YY"])[:npol], freq=freq, ew=new, el=np.linspace(-0.5, 0.5, nel), ra=nra, allocate=False)
        s.attach("vis", vis_d)
        s.attach("vis_weight", w_d)
        t = dayenu.DayenuDelayFilterHybridVis(**cfg)
        t.setup()
        state["stream"] = t.process(s)

    t_task = best(task_run, restore)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "YY"])[:npol], freq=freq, ra=nra, el=np.linspace(-0.5, 0.5, nel), allocate=False)
    rm.attrs["weight_ew"], rm.attrs["exclude_cyl"] = "natural", []
    rm.attach("weight", rw)
    t_radep = best(lambda: RADependentWeights().process(state["stream"], rm))

    # ---- the float64 NumPy twin on one (ew, ra) column
    t0 = time.perf_counter()
    twin.filter_hybrid(freq, vis[:, :, :1, :, :1], weight[:, :, :1, :1], **cfg)
    t_twin = time.perf_counter() - t0

    n16, n32 = -(-n // 16) * 16, -(-n // 32) * 32
    nsample = npol * new * nra
    mat_bytes = npol * n * n * new * nra * 8
    cov_flop = nsample * sum((f // 16 + 1) * 16 for f in range(n)) * n16 * 2.0
    apply_flop = nsample * (2 * nel + 1) * 2.0 * n16 * n32
    apply_bytes = 2 * (vis.nbytes + weight.nbytes)
    avg_bytes = mat_bytes + mat_bytes // new
    return {
        "shape": {"npol": npol, "nfreq": n, "new": new, "nel": nel, "nra": nra},
        "distinct_filters": int(nmat),
        "zero_weight_fraction": float((weight == 0).mean()),
        "stage_s": {"mask": t_mask, "build": t_build, "apply": t_apply, "save": t_save, "covariance": t_cov, "ew_coef_and_scale": t_coef, "ew_average_one_dataset": t_avg},
        "task_s": {"DayenuDelayFilterHybridVis_apply_save_cov": t_task, "RADependentWeights_filter_and_cov": t_radep},
        "save": {"bytes": mat_bytes, "tb_per_s": mat_bytes / t_save / 1e12, "share_of_stream_yardstick": mat_bytes / t_save / HBM_STREAM},
        "ew_average": {"bytes": avg_bytes, "tb_per_s": avg_bytes / t_avg / 1e12, "share_of_stream_yardstick": avg_bytes / t_avg / HBM_STREAM},
        "covariance": {"flop_executed": cov_flop, "flop_full_product": nsample * 2.0 * n**3, "store_bytes": mat_bytes, "tflops_executed": cov_flop / t_cov / 1e12,
                       "share_of_f64_matrix_peak": cov_flop / t_cov / PEAK_F64, "store_tb_per_s": mat_bytes / t_cov / 1e12},
        "apply": {"flop": apply_flop, "bytes": apply_bytes, "tflops": apply_flop / t_apply / 1e12, "share_of_f64_matrix_peak": apply_flop / t_apply / PEAK_F64,
                  "tb_per_s": apply_bytes / t_apply / 1e12},
        "numpy_twin_one_ew_ra_column_s": t_twin,
        "numpy_twin_all_columns_s_extrapolated": t_twin * new * nra,
    }


def merge_stats(path, out):
    """Add the kernels' shares of a rocprofv3 ``--kernel-trace --stats`` run to the JSON at ``out``."""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    name_key = next(k for k in rows[0] if k.lower() == "name")
    dur_key = next(k for k in rows[0] if "total" in k.lower() and "duration" in k.lower())
    calls_key = next(k for k in rows[0] if k.lower() == "calls")
    total = sum(float(r[dur_key]) for r in rows)
    kernels = [{"kernel": r[name_key].split("(")[0], "calls": int(r[calls_key]), "ms": float(r[dur_key]) / 1e6, "share": float(r[dur_key]) / total} for r in rows]
    kernels.sort(key=lambda k: -k["ms"])
    with open(out) as fh:
        doc = json.load(fh)
    doc["kernel_trace"] = {"note": "kernel trace of a run of its own; shares of the summed kernel time", "kernels": kernels}
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="NPOL,NFREQ,NEW,NEL,NRA (repeatable)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return 0

    import torch

    shapes = [tuple(int(x) for x in s.split(",")) for s in args.shape] if args.shape else [(2, 64, 4, 64, 2048), (2, 128, 4, 8, 2048)]
    doc = {"tool": "tools/dayenu_hybrid_timing.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "f64_matrix_peak_flops": PEAK_F64,
           "stream_yardstick_bytes_per_s": HBM_STREAM, "cases": []}
    for shape in shapes:
        res = time_shape(shape, args.repeats)
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
