#!/usr/bin/env python
"""HIP-event timing of the three kernels of the power-spectrum chain (`csrc/powerspec.hip`) on a ring-map delay cube of
`--pol` polarisations x `--delays` delays x `--ra` RA x `--el` el (default 2 x 128 x 2048 x 512, complex128: 4.3 GB), and
on one cube whose axes are no powers of two (1500 x 500, Bluestein on both).

Timed, each after a warm-up call and as the median of `--windows` windows of `--reps` calls:
  uv_fft2   `dmm_uv_fft2`, the tapered 2-D transform of the whole cube           32 B / cell algorithmic (it moves 64)
  cross     `dmm_ps3d_cross` of the two polarisations of the cube (distinct inputs) 48 B / cell
  cyl_bin   `dmm_ps_cyl_bin` of that cross spectrum into 34 bins, unit weights     16 B / cell (it reads the cells of
            the bins only; the host's table building and the upload are inside the window)
Printed per case: ms, the rate in TB/s on the algorithmic bytes and its share of the 8 TB/s of the HBM.  One JSON line
per case; `--out` also writes them to a file.

    python tools/powerspec_timing.py [--delays 128] [--out profiles/powerspec_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def run_case(ctx, emit, args, npol, ndelay, nra, nel):
    import torch

    from draco_amd import _lib
    from draco_amd.analysis import powerspec as ps
    from draco_amd.device import ptr

    gen = torch.Generator(device=ctx.device).manual_seed(nra + nel)
    cube = torch.view_as_complex(torch.randn((npol, nel, nra, ndelay, 2), dtype=torch.float64, device=ctx.device, generator=gen))
    ra = 10.0 + 0.01 * np.arange(nra)
    dec = 49.3 + 0.01 * (np.arange(nel) - nel / 2)
    w_ra, w_el = (ctx.to_device(np.ascontiguousarray(w)) for w in ps._taper(ra, dec, "tukey-0.5"))
    vis = ctx.empty((npol, ndelay, nra, nel), np.complex128)
    ncell = ndelay * nra * nel
    shape = {"npol": npol, "ndelay": ndelay, "nra": nra, "nel": nel, "cells_per_pol": ncell}

    def report(case, ms, nbytes, **more):
        med = float(np.median(ms))
        emit(dict({"case": case, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "algorithmic_GB": round(nbytes / 1e9, 3),
                   "TBps": round(nbytes / med / 1e9, 3), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4)}, **shape, **more))

    def fft():
        _lib.check(_lib.lib.dmm_uv_fft2(ctx.handle, ptr(cube), npol, nel, nra, ndelay, ptr(w_ra), ptr(w_el), ptr(vis), args.slab_mib))

    report("uv_fft2", windows(ctx, fft, args.windows, args.reps), 32 * npol * ncell, slab_mib=args.slab_mib)
    if npol < 2:
        return
    spec = ctx.empty((1, ndelay, nra, nel), np.complex128)
    v1, v2 = vis[0:1], vis[1:2]

    def cross():
        _lib.check(_lib.lib.dmm_ps3d_cross(ctx.handle, ptr(v1), ptr(v2), 1, 1, ncell, 1.5, ptr(spec)))

    report("cross", windows(ctx, cross, args.windows, args.reps), 48 * ncell)
    # rings of equal width between 10 % and 45 % of the extent of the (u, v) plane; the cells outside belong to no bin
    nbins = 34
    r = np.hypot(*np.meshgrid((np.arange(nel) - nel // 2) / nel, (np.arange(nra) - nra // 2) / nra))
    idx = np.floor((r - 0.1) / (0.35 / nbins)).astype(np.int64)
    binmap = np.ascontiguousarray(np.where((idx >= 0) & (idx < nbins), idx, -1).astype(np.int16))
    o_s, o_w, o_n = ctx.empty((ndelay, nbins), np.complex128), ctx.empty((ndelay, nbins), np.float64), ctx.empty((ndelay, nbins), np.float64)

    def cyl():
        _lib.check(_lib.lib.dmm_ps_cyl_bin(ctx.handle, ptr(spec), None, binmap.ctypes.data, ndelay, nra, nel, nbins, ptr(o_s), ptr(o_w), ptr(o_n)))

    report("cyl_bin", windows(ctx, cyl, args.windows, max(1, args.reps // 2)), 16 * ncell, nbins=nbins, cells_in_bins=int((binmap >= 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pol", type=int, default=2)
    ap.add_argument("--delays", type=int, default=128)
    ap.add_argument("--ra", type=int, default=2048)
    ap.add_argument("--el", type=int, default=512)
    ap.add_argument("--odd-delays", type=int, default=32, help="delays of the 1500 x 500 cube (0: skip it)")
    ap.add_argument("--slab-mib", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from draco_amd.device import Context

    ctx = Context.get()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    run_case(ctx, emit, args, args.pol, args.delays, args.ra, args.el)
    if args.odd_delays:
        run_case(ctx, emit, args, args.pol, args.odd_delays, 1500, 500)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
