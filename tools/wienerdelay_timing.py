"""Time the Wiener delay transform of a filtered ring map: the build and the apply at a sub-band-like shape.

    python tools/wienerdelay_timing.py [--shape NPOL,NFREQ,NRA,NEL ...] [--out profiles/wienerdelay_timing.json]
    python tools/wienerdelay_timing.py --merge-stats <rocprofv3 kernel stats csv> --out profiles/wienerdelay_timing.json

Default shapes: 2 pol x 64 freq x 2048 RA x 64 el (a sub-band) and 2 x 128 x 2048 x 8.  The ring map carries a true
DAYENU filter (tauw 0.2, epsilon 1e-3, eight distinct channel masks over the RA), ``C = K diag(var) K^T``, 3 % of the
weights zero, a Hann window and a prior of the order of the noise.  Every timed call is warmed up once at the same
shape and timed with a host clock around work that ends in a device synchronise.

Reported per shape: the build time in all and per pixel; the float64 operations of the stages actually executed
(counted from the shapes below) over that time, against the FP64 matrix-core peak of DESIGN.md (78.6 TFLOP/s); the apply
time and the operator's bytes over it, against the 6.1 TB/s the cross-product kernel reached as the
yardstick of a read-once stream; for context the float64 NumPy twin's time on one (pol, el) column (all RA) on the
same host.  The share of each kernel of the build comes from a kernel trace taken in a run of its own (tracing slows the
host) and is merged with ``--merge-stats``.

Operations per pixel, n = nfreq, N = 2 n, d = ndelay, tiles of 64 and blocks of 32 as executed:
  T = Hb [Re P | Im P]            2 n n N
  Re A, Im A (upper tiles)        2 x 2 n (64^2 x tiles on or above the diagonal)
  Y = (H F)^T, two parts          2 x 2 d n n
  factorisation                   N^3 / 3
  two triangular solves           2 d N^2
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


def build_flops(n, nd):
    N = 2 * n
    tiles = -(-n // 64)
    upper = tiles * (tiles + 1) // 2
    return {"T": 2.0 * n * n * N, "A": 2 * 2.0 * n * min(n * n, 64 * 64 * upper), "Y": 2 * 2.0 * nd * n * n, "factor": N**3 / 3.0, "solve": 2.0 * nd * N * N}


def dayenu_k(np, freq, mask, tauw, epsilon):
    dfreq = freq[:, np.newaxis] - freq[np.newaxis, :]
    cov = np.eye(freq.size) + np.sinc(2.0 * tauw * dfreq) / epsilon
    mm = mask[:, np.newaxis] & mask[np.newaxis, :]
    return np.linalg.pinv(mm * cov, hermitian=True) * mm


def inputs(np, npol, n, nra, nel, seed=7):
    rng = np.random.default_rng(seed)
    freq = 600.0 + DF * np.arange(n)
    masks = np.ones((8, n), dtype=bool)
    for m in masks[1:]:
        m[rng.choice(np.arange(1, n - 1), size=max(1, n // 16), replace=False)] = False
    kk = np.stack([dayenu_k(np, freq, m, 0.2, 1e-3) for m in masks])
    which = np.sort(rng.integers(8, size=nra))
    var = 1.0 + rng.random((npol, n))
    K = np.empty((npol, n, n, nra))
    C = np.empty((npol, n, n, nra))
    for p in range(npol):
        cc = np.einsum("mgf,f,mhf->mgh", kk, var[p], kk)
        K[p] = kk[which].transpose(1, 2, 0)
        C[p] = cc[which].transpose(1, 2, 0)
    w = 0.5 + 1.5 * rng.random((npol, n, nra, nel))
    w[rng.random(w.shape) < 0.03] = 0.0
    w *= masks[which].T[np.newaxis, :, :, np.newaxis]
    dbp = 0.5 + rng.random((1, npol, n, nel))
    m = rng.standard_normal((1, npol, n, nra, nel))
    return freq, K, C, w, dbp, m


def time_shape(shape, repeats, workspace_mib):
    import numpy as np

    import wienerdelay_twin as twin
    from draco_amd.analysis import powerspec as ps
    from draco_amd.core import containers
    from draco_amd.device import Context

    npol, n, nra, nel = shape
    ctx = Context.get()
    freq, K, C, w, dbp, m = inputs(np, npol, n, nra, nel)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "YY"])[:npol], freq=freq, ra=nra, el=np.linspace(-0.5, 0.5, nel))
    rm.map[:], rm.weight[:] = m, w
    for name, val in (("dirty_beam_power", dbp), ("filter", K), ("freq_cov", C)):
        rm.add_dataset(name)
        rm.datasets[name] = containers.Dataset(dev=ctx.to_device(val))
    for name in ("map", "weight"):
        rm.datasets[name].set_device(ctx.to_device(rm.datasets[name].host()))
    task = ps.ConstructWienerDelayTransform(prior_amp=1.0, window="hann", workspace_mib=workspace_mib)
    apply = ps.ApplyWienerDelayTransform()

    def clock(fn):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return time.perf_counter() - t0, r

    _, op = clock(lambda: task.process(rm))  # warm-up at this shape
    t_build = []
    for _ in range(repeats):
        del op
        t, op = clock(lambda: task.process(rm))
        t_build.append(t)
    clock(lambda: apply.process(rm, op))
    t_apply = [clock(lambda: apply.process(rm, op))[0] for _ in range(max(repeats, 3))]
    nd = int(len(op.index_map["delay"]))
    npix = npol * nra * nel
    fl = build_flops(n, nd)
    op_bytes = npix * nd * n * 8
    tb, ta = min(t_build), min(t_apply)

    # the float64 NumPy twin on one (pol, el) column, all RA, on this host
    win = task._get_window(freq)
    _, F, sdiag = twin.constants(freq, win, 1.0, 0.0)
    t0 = time.perf_counter()
    twin.build(K[:1], C[:1], w[:1, :, :, :1], dbp[0, :1, :, :1], F, sdiag, win, ld=False)
    t_twin = time.perf_counter() - t0
    return {
        "shape": {"npol": npol, "nfreq": n, "nra": nra, "nel": nel, "ndelay": nd},
        "pixels": npix,
        "workspace_mib": workspace_mib,
        "operator_bytes": op_bytes,
        "build_s": t_build,
        "build_us_per_pixel": 1e6 * tb / npix,
        "build_flop_per_pixel": fl,
        "build_tflops": sum(fl.values()) * npix / tb / 1e12,
        "build_share_of_f64_matrix_peak": sum(fl.values()) * npix / tb / PEAK_F64,
        "apply_s": t_apply,
        "apply_operator_tb_per_s": op_bytes / ta / 1e12,
        "apply_share_of_read_once_yardstick": op_bytes / ta / HBM_STREAM,
        "numpy_twin_one_pol_el_column_s": t_twin,
        "numpy_twin_us_per_pixel": 1e6 * t_twin / nra,
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
    doc["kernel_trace"] = {"note": "kernel trace of a run of its own (one warm-up and one timed build and apply per shape); shares of the summed kernel time", "kernels": kernels}
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", action="append", help="NPOL,NFREQ,NRA,NEL (repeatable)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workspace-mib", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return 0

    import torch

    shapes = [tuple(int(x) for x in s.split(",")) for s in args.shape] if args.shape else [(2, 64, 2048, 64), (2, 128, 2048, 8)]
    doc = {"tool": "tools/wienerdelay_timing.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "f64_matrix_peak_flops": PEAK_F64,
           "read_once_yardstick_bytes_per_s": HBM_STREAM, "cases": []}
    for shape in shapes:
        res = time_shape(shape, args.repeats, args.workspace_mib)
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
