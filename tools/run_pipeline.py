#!/usr/bin/env python
"""End-to-end example: sky -> SimulateSidereal -> (noise) -> MModeTransform -> {Dirty, Wiener, ML}MapMaker.

    python tools/run_pipeline.py [--config 1] [--makers dirty wiener ml] [--noise] [--regrid | --rebin | --regrid-gp]

--regrid: the simulated day is first sampled onto irregular time stamps (jitter, a gap, flagged samples) as a TimeStream
and brought back to the RA grid by SiderealRegridder before the m-mode transform.
--rebin: the same TimeStream goes through SiderealRebinner and RebinGradientCorrection instead.
--rfi (with one of the three): bursts are injected into the TimeStream and RFIMask -> ApplyTimeFreqMask run ahead of the regridder.

Mirrors the reference's tutorial pipeline (doc/pipeline_params.yaml:1-35) with this repo's
task classes.  Prints per-task wall time (device synchronised) and a few sanity numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1)
    ap.add_argument("--makers", nargs="*", default=["dirty", "wiener"])
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--regrid", action="store_true", help="go through an irregular TimeStream and SiderealRegridder")
    ap.add_argument("--rebin", action="store_true", help="go through an irregular TimeStream, SiderealRebinner and RebinGradientCorrection")
    ap.add_argument("--regrid-gp", action="store_true", help="go through an irregular TimeStream and SiderealRegridderGP (kernel width 5 from 512 RA samples up, else 2: "
                    "the band-truncated kernel matrix of a short day is not positive definite at width 5)")
    ap.add_argument("--rfi", action="store_true", help="with --regrid / --rebin / --regrid-gp: inject bursts into the TimeStream, then RFIMask and ApplyTimeFreqMask ahead of the regridder")
    ap.add_argument("--nfreq", type=int, default=0, help="override the number of frequencies")
    ap.add_argument("--pool-gb", type=float, default=0.0, help="B pool budget in GB (default: 0.6 of the free HBM)")
    args = ap.parse_args()

    import torch

    from draco_amd.analysis.mapmaker import DirtyMapMaker, MaximumLikelihoodMapMaker, WienerMapMaker
    from draco_amd.analysis.transform import MModeTransform
    from draco_amd.core import containers
    from draco_amd.core.products import SyntheticProvider, TransitTelescope
    from draco_amd.device import Context
    from draco_amd.synthesis.noise import GaussianNoise
    from draco_amd.synthesis.stream import SimulateSidereal
    from draco_amd import workloads as osyn

    cfg = dict(osyn.CONFIGS[args.config])
    if args.nfreq:
        cfg["nfreq"] = args.nfreq
    ctx = Context.get()
    tel = TransitTelescope(osyn.frequencies(cfg["nfreq"]), lmax=cfg["lmax"], ncyl=cfg["ncyl"], nfeed_cyl=cfg["nfeed_cyl"])
    bt = SyntheticProvider(tel, seed=3000 + args.config)
    nside = cfg["nside"]

    # band-limited Gaussian sky with C_l = (l+1)^-2, made on the device through alm2map
    from draco_amd import _lib
    from draco_amd.device import ptr

    gen = torch.Generator(device=ctx.device).manual_seed(4000 + args.config)
    lmax = tel.lmax
    alm = torch.randn((tel.nfreq, 4, lmax + 1, lmax + 1), dtype=torch.complex128, device=ctx.device, generator=gen)
    cl = (torch.arange(lmax + 1, device=ctx.device, dtype=torch.float64) + 1.0) ** -1.0
    alm = alm * cl[None, None, None, :]
    alm[:, :, 0, :] = alm[:, :, 0, :].real.to(torch.complex128)  # m = 0 is real
    alm[:, 1:3, :, :2] = 0
    sky = ctx.empty((tel.nfreq, 4, 12 * nside * nside), np.float64)
    alm = alm.contiguous()
    _lib.check(_lib.lib.dmm_alm2map(ctx.handle, ptr(alm), tel.nfreq, 4, lmax, lmax, nside, ptr(sky)))
    mp = containers.Map(nside=nside, freq=tel.frequencies, allocate=False)
    mp.attach("map", sky)

    report = {"config": args.config, "nfeed": tel.nfeed, "npairs": tel.npairs, "nfreq": tel.nfreq, "lmax": lmax, "nside": nside}

    def timed(name, fn):
        torch.cuda.synchronize()  # device-wide: a map-maker's last alm2map may still be running on the side stream
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        report[name + "_s"] = round(time.perf_counter() - t0, 4)
        print(f"[run_pipeline] {name}: {report[name + '_s']} s", file=sys.stderr, flush=True)
        return out

    pool = int(args.pool_gb * 1e9) if args.pool_gb > 0 else None
    sim = SimulateSidereal(pool_bytes=pool)
    sim.setup(bt)
    timed("SimulateSidereal_first_call(incl. B block allocation)", lambda: sim.process(mp))
    ss = timed("SimulateSidereal", lambda: sim.process(mp))
    if args.noise:
        gn = GaussianNoise(seed=1, ndays=733.0, recv_temp=50.0)
        gn.setup(tel)
        ss = timed("GaussianNoise_host", lambda: gn.process(ss))
    if args.regrid or args.rebin or args.regrid_gp:
        from draco_amd.analysis.sidereal import RebinGradientCorrection, SiderealRebinner, SiderealRegridder, SiderealRegridderGP
        from draco_amd.util import regrid

        nra, lsd, a = ss.vis.shape[-1], 100, 5
        rng = np.random.default_rng(7)
        nt = 2 * nra
        lsds = np.sort(lsd + np.linspace(-0.03, 1.03, nt) + rng.uniform(-0.3, 0.3, nt) * 1.06 / nt)
        lsds = lsds[(lsds < lsd + 0.5) | (lsds > lsd + 0.5 + 2.0 * a / nra)]
        pad = 5 * a
        grid = lsd + np.arange(-pad, nra + pad, dtype=np.float64) / nra
        R = torch.from_numpy(regrid.lanczos_forward_matrix(grid, lsds, a).astype(np.float32)).to(ctx.device)  # [nt, ngrid]
        idx = torch.from_numpy(np.arange(-pad, nra + pad) % nra).to(ctx.device)
        sv = ss.vis.device(ctx)[..., idx]  # the day is periodic
        ts = containers.TimeStream(axes_from=ss, attrs_from=ss, time=tel.lsd_to_unix(lsds), allocate=False)
        ts.attach("vis", torch.complex(sv.real @ R.T, sv.imag @ R.T).contiguous())
        tw = torch.ones(ts.vis.shape, dtype=torch.float32, device=ctx.device)
        tw[..., :: 7] = 0.0
        ts.attach("vis_weight", tw)
        ts.attrs["lsd"] = lsd
        if args.rfi:  # bursts on a few time samples of every product, found on one stack entry and masked in all
            from draco_amd.analysis.flagging import ApplyTimeFreqMask, RFIMask

            tv = ts.vis.device(ctx)
            bursts = rng.choice(len(lsds), size=max(2, len(lsds) // 100), replace=False)
            tv[..., torch.from_numpy(bursts).to(ctx.device)] += 50.0 * tv.abs().mean()
            rfimask = timed("RFIMask", lambda: RFIMask(stack_ind=0).process(ts))
            ts = timed("ApplyTimeFreqMask", lambda: ApplyTimeFreqMask().process(ts, rfimask))
            found = rfimask.mask[:][:, bursts].mean()
            report["rfi_masked_fraction"] = float(rfimask.mask[:].mean())
            report["rfi_bursts_found"] = float(found)
        if args.rebin:
            rb = SiderealRebinner(samples=nra)
            rb.setup(tel)
            timed("SiderealRebinner_first_call", lambda: rb.process(ts))
            sr = timed("SiderealRebinner", lambda: rb.process(ts))
            gc = RebinGradientCorrection()
            gc.setup(sr)  # the day has full coverage: it is its own reference
            sr = timed("RebinGradientCorrection", lambda: gc.process(sr))
        elif args.regrid_gp:
            rg = SiderealRegridderGP(samples=nra, kernel_width=a if nra >= 512 else 2)
            rg.setup(tel)
            timed("SiderealRegridderGP_first_call", lambda: rg.process(ts))
            sr = timed("SiderealRegridderGP", lambda: rg.process(ts))
        else:
            rg = SiderealRegridder(samples=nra, kernel_width=a)
            rg.setup(tel)
            timed("SiderealRegridder_first_call", lambda: rg.process(ts))
            sr = timed("SiderealRegridder", lambda: rg.process(ts))
        ss = sr
    tr = MModeTransform()
    tr.setup(bt)
    mm = timed("MModeTransform", lambda: tr.process(ss))
    makers = {"dirty": DirtyMapMaker, "wiener": WienerMapMaker, "ml": MaximumLikelihoodMapMaker}
    for name in args.makers:
        task = makers[name](nside=nside, pool_bytes=pool)
        task.setup(bt)
        timed(name + "_first_call(incl. B fill)", lambda: task.process(mm))
        out = timed(name, lambda: task.process(mm))
        m = out.map[:]
        report[name + "_map_rms"] = float(np.sqrt((m**2).mean()))
        assert np.all(np.isfinite(m))
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
