#!/usr/bin/env python
"""HIP-event timing of the regridder alone at cfg-3 size (256 frequencies x 379 stack entries = 97 024 rows, 1024
samples out) for nt in {1536, 2048, 4096, 8640} with jittered time stamps, two gaps and 20 % flagged samples, and of one
stacker update.  Per case: a warm-up call, then `--windows` windows of `--reps` calls each; prints the median window,
the spread over windows, GB/s on the algorithmic bytes (input 12 B per sample + output 12 B per grid point; stacker:
read day + state, write state) and the fraction of the 8 TB/s peak.  One JSON line per case.

    python tools/regrid_timing.py [--rows 97024] [--nt 1536 2048 4096 8640] [--workspace-mib 0]

`--method rebin | nearest | linear | cubic` times the rebinner or one of the direct interpolators on the same data
instead (default `band_wiener`: the above).

`--method gp` times the Gaussian-process regridder (`dmm_gp_fill` / `dmm_gp_project` + `dmm_gp_compact` / `dmm_gp_apply`)
on `--freqs` frequencies x rows / freqs stacks, once for every entry of `--gp-masks` (the number of distinct flag
patterns among the frequencies: 1 = every frequency shares one factorisation), split into the three stages with the
float64 FLOP rate of each against the counts of DESIGN.md section 7h, and the band-Wiener regridder on the same data.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def other_method(args):
    """`--method rebin | nearest | linear | cubic`: the same rows, time stamps, flags and windows through `dmm_rebin`
    (inverse-variance weights; bytes: 12 B per sample in, 18 B per bin out -- vis, weight, nsample, effective_ra) or
    `dmm_regrid_interp` (12 B per sample in, 12 B per grid point out; the tap tables are uploaded once, outside the windows)."""
    import torch

    from draco_amd import _lib
    from draco_amd.analysis import sidereal
    from draco_amd.device import Context, ptr
    from draco_amd.util import regrid

    ctx = Context.get()
    rng = np.random.default_rng(1)
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    for nt in args.nt:
        t = np.sort(np.linspace(-0.005, 1.005, nt) + rng.uniform(-0.4, 0.4, nt) * 1.01 / nt)
        t = t[((t < 0.31) | (t > 0.33)) & ((t < 0.70) | (t > 0.705))]
        n = len(t)
        vis = torch.view_as_complex(torch.randn((args.rows, n, 2), dtype=torch.float32, device=ctx.device, generator=gen))
        w = torch.rand((args.rows, n), dtype=torch.float32, device=ctx.device, generator=gen) + 0.5
        w *= torch.rand((args.rows, n), dtype=torch.float32, device=ctx.device, generator=gen) > 0.2
        if args.method == "rebin":
            target = np.linspace(0.0, 1.0, args.samples, endpoint=False)
            plan = regrid.RebinPlan(ctx, t, target, np.median(np.abs(np.diff(t))), 0.0, target * 360.0)
            fn = lambda: regrid.rebin(ctx, plan, vis, w, _lib.DMM_REBIN_INVERSE_VARIANCE)  # noqa: E731
            nbytes = args.rows * (12 * n + 18 * args.samples)
        else:
            task = {"nearest": sidereal.SiderealRegridderNearest, "linear": sidereal.SiderealRegridderLinear, "cubic": sidereal.SiderealRegridderCubic}[args.method](samples=args.samples)
            tap, coeff, bad = task._taps(t, np.arange(args.samples, dtype=np.float64) / args.samples)
            tap_d, coeff_d, bad_d = ctx.to_device(tap, np.int32), ctx.to_device(coeff, np.float64), ctx.to_device(bad, np.uint8)
            ov, ow = ctx.empty((args.rows, args.samples), np.complex64), ctx.empty((args.rows, args.samples), np.float32)
            fn = lambda: _lib.check(_lib.lib.dmm_regrid_interp(ctx.handle, len(tap), ptr(vis), ptr(w), args.rows, n, args.samples, ptr(tap_d), ptr(coeff_d), ptr(bad_d), None, None, None, None, ptr(ov), ptr(ow)))  # noqa: E731
            nbytes = args.rows * 12 * (n + args.samples)
        ms = windows(ctx, fn, args.windows, args.reps)
        med = float(np.median(ms))
        print(json.dumps({"case": args.method, "rows": args.rows, "nt": n, "samples": args.samples, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                          "GBps": round(nbytes / med / 1e6, 1), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4), "hbm_floor_ms": round(nbytes / PEAK * 1e3, 3)}), flush=True)
        ctx.sync()
        del vis, w


def gp_method(args):
    """`--method gp`: see the module docstring.  FLOP counts per distinct mask of order n, band M, nk kept rows: fill 24
    per evaluated entry (n M + n nk entries), projection n M^2 + 4 n M nk, apply 6 per (stack, kept row, sample of its
    span) and frequency."""
    import torch

    from draco_amd.device import Context
    from draco_amd.util import gaussian_process as gp
    from draco_amd.util import regrid

    ctx = Context.get()
    rng = np.random.default_rng(1)
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    kw, pad = 5, 25
    grid = np.arange(-pad, args.samples + pad, dtype=np.float64) / args.samples
    spec = {"name": "matern", "width": kw, "alpha": 1.0, "nu": 2.5, "epsilon": 1e-3}
    nfreq = args.freqs
    nstack = args.rows // nfreq
    for nt in args.nt:
        t = np.sort(np.linspace(-0.005, 1.005, nt) + rng.uniform(-0.4, 0.4, nt) * 1.01 / nt)
        t = t[((t < 0.31) | (t > 0.33)) & ((t < 0.70) | (t > 0.705))]
        n = len(t)
        vis = torch.view_as_complex(torch.randn((nfreq, nstack, n, 2), dtype=torch.float32, device=ctx.device, generator=gen))
        w0 = torch.rand((nfreq, nstack, n), dtype=torch.float32, device=ctx.device, generator=gen) + 0.5
        w0 *= torch.rand((nfreq, nstack, n), dtype=torch.float32, device=ctx.device, generator=gen) > 0.2
        gp.resample_device(ctx, vis[:1, :64].contiguous(), w0[:1, :64].contiguous(), t, grid, 1.7, 1, spec, pad=pad, samples=args.samples)  # warm-up: loads the code
        ctx.sync()
        for nmask in args.gp_masks:
            w = w0.clone()
            for f in range(nfreq):  # frequency f carries flag pattern f % nmask: five samples flagged in every stack
                k = f % nmask
                if k:
                    w[f, :, 100 + 7 * k : 105 + 7 * k] = 0
            runs = []
            for _ in range(args.windows):
                tm, info = {}, {}
                ctx.sync()
                t0 = time.perf_counter()
                gp.resample_device(ctx, vis, w, t, grid, 1.7, 1, spec, pad=pad, samples=args.samples, timings=tm, info=info)
                ctx.sync()
                tm["wall_ms"] = (time.perf_counter() - t0) * 1e3
                runs.append(tm)
            med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
            ng = info["ngroup"]
            fl_fill = 24.0 * sum(a * (m + k) for a, m, k in zip(info["n"], info["M"], info["nk"]))
            fl_proj = float(sum(a * m * m + 4.0 * a * m * k for a, m, k in zip(info["n"], info["M"], info["nk"])))
            fl_apply = 6.0 * nstack * sum(info["span_sum"][g] * info["nfreq_of"][g] for g in range(ng))
            print(json.dumps({"case": "gp", "rows": nfreq * nstack, "nfreq": nfreq, "nstack": nstack, "nt": n, "samples": args.samples, "masks": ng, "M": max(info["M"]), "order": max(info["n"]),
                              "kept_rows": max(info["nk"]), "max_span": max(info["span"]), "windows": args.windows,
                              "fill_ms": round(med["fill_ms"], 3), "project_ms": round(med["project_ms"], 3), "apply_ms": round(med["apply_ms"], 3), "wall_ms": round(med["wall_ms"], 1),
                              "fill_gflop": round(fl_fill / 1e9, 2), "project_gflop": round(fl_proj / 1e9, 2), "apply_gflop": round(fl_apply / 1e9, 2),
                              "fill_gflops": round(fl_fill / med["fill_ms"] / 1e6, 1), "project_gflops": round(fl_proj / med["project_ms"] / 1e6, 1),
                              "apply_gflops": round(fl_apply / med["apply_ms"] / 1e6, 1)}), flush=True)
            del w
        plan = regrid.RegridPlan(ctx, grid, t, kw)
        v2, w2 = vis.reshape(-1, n), w0.reshape(-1, n)
        ms = windows(ctx, lambda: regrid.band_wiener(ctx, plan, v2, w2, 1e-3, pad, args.samples), args.windows, 1)
        print(json.dumps({"case": "regrid", "rows": nfreq * nstack, "nt": n, "samples": args.samples, "ms": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}), flush=True)
        ctx.sync()
        plan.close()
        del vis, w0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256 * 379)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--nt", type=int, nargs="+", default=[1536, 2048, 4096, 8640])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--workspace-mib", type=int, default=0)
    ap.add_argument("--method", choices=["band_wiener", "rebin", "nearest", "linear", "cubic", "gp"], default="band_wiener")
    ap.add_argument("--freqs", type=int, default=256, help="gp: frequencies the rows are split into")
    ap.add_argument("--gp-masks", type=int, nargs="+", default=[1, 256], help="gp: numbers of distinct flag patterns to time")
    args = ap.parse_args()
    if args.method == "gp":
        return gp_method(args)
    if args.method != "band_wiener":
        return other_method(args)

    import torch

    from draco_amd import _lib
    from draco_amd.device import Context, ptr
    from draco_amd.util import regrid

    ctx = Context.get()
    with ctx.options(regrid_workspace_mib=args.workspace_mib):
        rng = np.random.default_rng(1)
        gen = torch.Generator(device=ctx.device).manual_seed(1)
        kw, pad = 5, 25
        grid = np.arange(-pad, args.samples + pad, dtype=np.float64) / args.samples
        for nt in args.nt:
            t = np.sort(np.linspace(-0.005, 1.005, nt) + rng.uniform(-0.4, 0.4, nt) * 1.01 / nt)
            t = t[((t < 0.31) | (t > 0.33)) & ((t < 0.70) | (t > 0.705))]
            n = len(t)
            vis = torch.randn((args.rows, n, 2), dtype=torch.float32, device=ctx.device, generator=gen)
            vis = torch.view_as_complex(vis)
            w = torch.rand((args.rows, n), dtype=torch.float32, device=ctx.device, generator=gen) + 0.5
            w *= torch.rand((args.rows, n), dtype=torch.float32, device=ctx.device, generator=gen) > 0.2
            plan = regrid.RegridPlan(ctx, grid, t, kw)
            ms = windows(ctx, lambda: regrid.band_wiener(ctx, plan, vis, w, 1e-3, pad, args.samples), args.windows, args.reps)
            nbytes = args.rows * 12 * (n + args.samples)
            med = float(np.median(ms))
            print(json.dumps({"case": "regrid", "rows": args.rows, "nt": n, "samples": args.samples, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                              "GBps": round(nbytes / med / 1e6, 1), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4), "hbm_floor_ms": round(nbytes / PEAK * 1e3, 3)}), flush=True)
            ctx.sync()
            plan.close()
            del vis, w
        # one stacker update (inverse variance, with sample variance)
        n = args.rows * args.samples
        dv = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device=ctx.device, generator=gen))
        dw = torch.rand(n, dtype=torch.float32, device=ctx.device, generator=gen)
        sv, sw, ns = ctx.zeros((n,), np.complex64), ctx.zeros((n,), np.float32), ctx.zeros((n,), np.int16)
        sq, var = ctx.zeros((n,), np.float32), ctx.zeros((3, n), np.float32)
        for with_var in (0, 1):
            fn = lambda: _lib.check(_lib.lib.dmm_sidereal_stack_add(ctx.handle, 1, with_var, ptr(dv), ptr(dw), None, ptr(sv), ptr(sw), ptr(ns), ptr(sq), ptr(var), n))  # noqa: E731
            ms = windows(ctx, fn, args.windows, 4)
            nbytes = n * (12 + 2 * 14 + (2 * 16 if with_var else 0))
            med = float(np.median(ms))
            print(json.dumps({"case": "stack_add", "with_variance": with_var, "elements": n, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                              "GBps": round(nbytes / med / 1e6, 1), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4)}), flush=True)


if __name__ == "__main__":
    main()
