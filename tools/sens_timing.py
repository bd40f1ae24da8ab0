#!/usr/bin/env python
"""HIP-event timing of `ComputeSystemSensitivity` on one CHIME-like frequency block: a stacked stream of 4 cylinders x 256
feeds x 2 polarisations (2048 inputs, 2 098 176 products, the stack axis of the stand-in telescope's redundancy), 8192
times, `--freqs` frequencies, four distinct columns of input flags, 10 % zero weights.

Timed, each after a warm-up call and as the median of `--windows` windows of `--reps` calls (`process`: a tenth as
many): `process` (the host's index work over the product axis included: the GPU idles while it runs) and `run` (the two
kernels with the tables in hand).
Printed per case: ms per frequency and the rate on the algorithmic bytes, which are one read of the weight cube and one
read of the autocorrelation rows of vis.  Beside them, in the same session: `SiderealRebinner`'s kernel on its CHIME-like
day (`tools/regrid_timing.py --method rebin`: 97 024 rows x 8427 samples onto 1024 bins), a reduction of the same kind,
with the ratio of the two rates; and the wall time of the float64 NumPy twin (`tests/sens_twin.py`) at one frequency of
the same shape, as the CPU figure.  One JSON line per case; `--out` also writes them to a file.

    python tools/sens_timing.py [--freqs 32] [--nt 8192] [--nfeed-cyl 256] [--out profiles/sens_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12


def windows(ctx, fn, nwin, reps):
    fn()
    ctx.sync()
    out = []
    for _ in range(nwin):
        ctx.timer_start()
        for _ in range(reps):
            fn()
        out.append(ctx.timer_stop() / reps)
    return out


def rebin_rate(ctx, args):
    """GB/s of `dmm_rebin` on the day `tools/regrid_timing.py --method rebin` times (12 B per sample in, 18 B per bin out)."""
    import torch

    from draco_amd import _lib
    from draco_amd.util import regrid

    rows, nt, samples = 256 * 379, 8640, 1024
    rng = np.random.default_rng(1)
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    t = np.sort(np.linspace(-0.005, 1.005, nt) + rng.uniform(-0.4, 0.4, nt) * 1.01 / nt)
    t = t[((t < 0.31) | (t > 0.33)) & ((t < 0.70) | (t > 0.705))]
    n = len(t)
    vis = torch.view_as_complex(torch.randn((rows, n, 2), dtype=torch.float32, device=ctx.device, generator=gen))
    w = torch.rand((rows, n), dtype=torch.float32, device=ctx.device, generator=gen) + 0.5
    w *= torch.rand((rows, n), dtype=torch.float32, device=ctx.device, generator=gen) > 0.2
    target = np.linspace(0.0, 1.0, samples, endpoint=False)
    plan = regrid.RebinPlan(ctx, t, target, np.median(np.abs(np.diff(t))), 0.0, target * 360.0)
    ms = windows(ctx, lambda: regrid.rebin(ctx, plan, vis, w, _lib.DMM_REBIN_INVERSE_VARIANCE), args.windows, args.reps)
    med = float(np.median(ms))
    nbytes = rows * (12 * n + 18 * samples)
    ctx.sync()
    return {"case": "rebin", "rows": rows, "nt": n, "samples": samples, "ms": round(med, 3), "GBps": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freqs", type=int, default=32)
    ap.add_argument("--nt", type=int, default=8192)
    ap.add_argument("--ncyl", type=int, default=4)
    ap.add_argument("--nfeed-cyl", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per window of the kernels (a tenth as many of `process`)")
    ap.add_argument("--no-twin", action="store_true", help="skip the float64 NumPy twin (a few GB of host memory at full size)")
    ap.add_argument("--no-rebin", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from draco_amd.analysis.sensitivity import ComputeSystemSensitivity
    from draco_amd.core import containers
    from draco_amd.core.products import TransitTelescope
    from draco_amd.device import Context

    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    t0 = time.perf_counter()
    tel = TransitTelescope(np.linspace(600.0, 601.0, args.freqs), lmax=4, ncyl=args.ncyl, nfeed_cyl=args.nfeed_cyl)
    t_tel = time.perf_counter() - t0
    nf, nt, nstack = args.freqs, args.nt, tel.npairs
    ctx = Context.get()
    gen = torch.Generator(device=ctx.device).manual_seed(2)
    freq = np.zeros(nf, dtype=[("centre", np.float64), ("width", np.float64)])
    freq["centre"], freq["width"] = 800.0 - 0.390625 * np.arange(nf), 0.390625
    ts = containers.TimeStream(freq=freq, time=1.6e9 + 10.0 * np.arange(nt), input=tel.input_index, prod=tel.index_map_prod, stack=tel.index_map_stack,
                               reverse_map_stack=tel.reverse_map_stack, allocate=False)
    vis = torch.view_as_complex(torch.randn((nf, nstack, nt, 2), dtype=torch.float32, device=ctx.device, generator=gen))
    ps = ts.prodstack
    autos = np.flatnonzero(ps["input_a"] == ps["input_b"])
    vis[:, torch.from_numpy(autos).to(ctx.device)] += 100.0
    w = torch.rand((nf, nstack, nt), dtype=torch.float32, device=ctx.device, generator=gen) + 0.5
    w *= torch.rand((nf, nstack, nt), dtype=torch.float32, device=ctx.device, generator=gen) > 0.1
    ts.attach("vis", vis)
    ts.attach("vis_weight", w)
    ts.add_dataset("input_flags")
    flags = np.ones((tel.nfeed, nt), dtype=np.float32)
    flags[3] = 0.0
    flags[100 % tel.nfeed, nt // 4 : nt // 2] = 0.0
    flags[[7, 9], nt // 2 :] = 0.0
    flags[11, 3 * nt // 4 :] = 0.0
    ts.input_flags[:] = flags

    task = ComputeSystemSensitivity()
    task.setup(tel)
    t0 = time.perf_counter()
    tb = task.tables(ts)
    t_tab = time.perf_counter() - t0
    nauto = len(tb["auto_rows"])
    nbytes = nf * nt * (4 * nstack + 8 * nauto)
    shape = {"nfreq": nf, "nstack": nstack, "ntime": nt, "ninput": tel.nfeed, "nprod": len(tel.index_map_prod), "nauto": nauto, "rows_per_pol": np.diff(tb["pol_ptr"]).tolist(),
             "flag_columns": int(tb["cnt"].shape[1]), "algorithmic_GB": round(nbytes / 1e9, 3), "telescope_s": round(t_tel, 1), "tables_s": round(t_tab, 3)}
    sens = {}
    for name, fn, reps in (("run", lambda: task.run(ts, tb), args.reps), ("process", lambda: task.process(ts), max(1, args.reps // 10))):
        ms = windows(ctx, fn, args.windows, reps)
        med = float(np.median(ms))
        sens[name] = nbytes / med / 1e6
        emit(dict({"case": "sens_" + name, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "ms_per_freq": round(med / nf, 4),
                   "GBps": round(sens[name], 1), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4), "hbm_floor_ms": round(nbytes / PEAK * 1e3, 3)}, **shape))
    out = task.run(ts, tb)
    ctx.sync()
    got = {k: out.datasets[k]._dev[0].cpu().numpy() for k in ("measured", "radiometer", "weight")}

    if not args.no_rebin:
        del out
        rb = rebin_rate(ctx, args)
        rb["sens_run_over_rebin"] = round(sens["run"] / rb["GBps"], 3)
        emit(rb)

    if not args.no_twin:
        import sens_twin as twin

        v1, w1 = vis[:1].cpu().numpy(), w[:1].cpu().numpy()
        t0 = time.perf_counter()
        tw = twin.sensitivity(v1, w1, tb)
        wall = time.perf_counter() - t0
        err = max(float(np.nanmax(np.abs(got[k].astype(np.float64) - t[0]) / np.where(t[0] == 0, 1.0, np.abs(t[0])))) for k, t in zip(("measured", "radiometer", "weight"), tw))
        emit({"case": "twin_float64_numpy", "nfreq": 1, "nstack": nstack, "ntime": nt, "wall_s": round(wall, 2), "threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]),
              "gpu_against_twin_rel": err})
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
