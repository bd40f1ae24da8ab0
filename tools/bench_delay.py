"""Time the Wiener-filter delay transform: the whole task and each stage of `csrc/delay.hip`, with device events.

    python tools/bench_delay.py [--out profiles/delay_timing.json] [--nstack 64] [--nra 1024] [--reps 3]

Two inputs at the CHIME shape (1024 channels, real time domain, solve of order 2048): a synthetic sidereal stream
(`nstack` stack entries x `nra` RA samples) and a ring-map slice (1 beam x 2 pol x `nstack / 2` el x `nra` RA).  Each is
warmed up once, then `DelaySpectrumWienerFilter.process` is timed `reps` times between events on the task's stream
(the minimum and the spread are reported).  The stages are timed the same way on one batch of 16 baselines through
the library's entry points.  Reported per baseline: time, and achieved FP64 FLOP/s from the operations the algorithm
needs (projection 2 R K n, factorisation n^3 / 3, the two triangular solves 2 R n^2; R = samples + 1 right-hand sides,
K = 2 x channels, n = order).  For comparison the NumPy twin of the reference's arithmetic runs on this host for
4 baselines of the same stream (labelled as such: another machine's CPU, not a GPU number).
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NFREQ = 1024
DF = 0.390625


def prior(nbase, ndelay):
    import numpy as np

    tau = np.abs(np.arange(ndelay) - ndelay // 2) / (ndelay / 2)
    return np.tile(1000.0 * 10.0 ** (-4.0 * tau) + 3e-3, (nbase, 1))


def timed(ctx, fn, reps):
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--nstack", type=int, default=64)
    ap.add_argument("--nra", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-baselines", type=int, default=4)
    args = ap.parse_args()

    import numpy as np
    import torch

    import delay_twin as twin
    from draco_amd import _lib
    from draco_amd.analysis import delay
    from draco_amd.core import containers
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    nstack, nra = args.nstack, args.nra
    freq = 400.0 + DF * np.arange(NFREQ)
    ndelay = 2 * NFREQ
    res = {"nfreq": NFREQ, "order": ndelay, "nra": nra, "nbase": nstack, "reps": args.reps}

    def dps(nbase):
        d = containers.DelaySpectrum(baseline=nbase, delay=ndelay)
        d.spectrum[:] = prior(nbase, ndelay)
        return d

    gen = torch.Generator(device=ctx.device).manual_seed(7)
    flagged = torch.from_numpy(np.random.default_rng(7).uniform(size=NFREQ) < 0.1).to(ctx.device)

    # ---- the whole task on a stream
    s = containers.SiderealStream(freq=freq, ra=nra, stack=nstack, allocate=False)
    vis = torch.view_as_complex(torch.randn((NFREQ, nstack, nra, 2), device=ctx.device, dtype=torch.float32, generator=gen))
    weight = torch.rand((NFREQ, nstack, nra), device=ctx.device, dtype=torch.float32, generator=gen) + 0.5
    weight[flagged] = 0.0
    s.attach("vis", vis)
    s.attach("vis_weight", weight)
    task = delay.DelaySpectrumWienerFilter(sample_axis="ra")
    task.setup(dps(nstack))
    task.process(s)  # warm-up
    lo, hi = timed(ctx, lambda: task.process(s), args.reps)
    res["stream_ms"] = [lo, hi]
    res["stream_ms_per_baseline"] = lo / nstack

    # ---- the whole task on a ring-map slice
    nel = max(1, nstack // 2)
    rm = containers.RingMap(freq=freq, beam=1, pol=np.array(["XX", "YY"]), ra=nra, el=np.linspace(-1, 1, nel), allocate=False)
    rmap = torch.randn((1, 2, NFREQ, nra, nel), device=ctx.device, dtype=torch.float64, generator=gen)
    rw = torch.rand((2, NFREQ, nra, nel), device=ctx.device, dtype=torch.float64, generator=gen) + 0.5
    rw[:, flagged] = 0.0
    rm.attach("map", rmap)
    rm.attach("weight", rw)
    rtask = delay.DelaySpectrumWienerFilter(dataset="map", sample_axis="ra")
    rtask.setup(dps(2 * nel))
    rtask.process(rm)
    lo, hi = timed(ctx, lambda: rtask.process(rm), args.reps)
    res["ringmap_ms"] = [lo, hi]
    res["ringmap_ms_per_baseline"] = lo / (2 * nel)

    # ---- the stages, one batch of 16 stream baselines
    nb, nrow, K, n = min(16, nstack), nra + 1, 2 * NFREQ, ndelay
    chan_d = ctx.to_device(np.arange(NFREQ, dtype=np.int32))
    coef_d = ctx.to_device(np.asarray(delay._window_coef(np.arange(NFREQ) / (NFREQ + 1), "nuttall") ** 2))
    F = ctx.empty((K, n), np.float64)
    X, Y, G = ctx.empty((nb, nrow, K), np.float64), ctx.empty((nb, nrow, n), np.float64), ctx.empty((nb, n, n), np.float64)
    nzt, status = ctx.empty((nb, nra), np.uint8), ctx.empty((nb,), np.int32)
    si_d = ctx.to_device(delay._shifted_inverse(prior(nb, ndelay), False))
    spec = ctx.empty((nb, nra, ndelay), np.complex128)
    st = vis.stride()
    dv = delay._view(vis, _lib.DMM_DELAY_C64, st[2], st[0], [st[1]])
    wv = delay._view(weight, _lib.DMM_DELAY_F32, st[2], st[0], [st[1]])
    fold = (C.c_int64 * 1)(nstack)
    lib, h = _lib.lib, ctx.handle
    stages = {
        "fourier": lambda: _lib.check(lib.dmm_delay_fourier(h, ndelay, NFREQ, 0, ptr(chan_d), ptr(F))),
        "prepare": lambda: _lib.check(lib.dmm_delay_prepare(h, ndelay, NFREQ, nra, nb, 0, 1, fold, C.byref(dv), C.byref(wv), 0, 1, 1, 0.0, 0.0, 1.0, ptr(coef_d), ptr(chan_d), ptr(X), ptr(nzt), ptr(status))),
        "project": lambda: _lib.check(lib.dmm_delay_project(h, n, NFREQ, nrow, nb, ptr(X), ptr(F), ptr(Y), ptr(status))),
        "solve": lambda: _lib.check(lib.dmm_delay_solve(h, n, 0, nra, nb, ptr(Y), ptr(si_d), ptr(G), ptr(status))),
        "store": lambda: _lib.check(lib.dmm_delay_store(h, ndelay, 0, nra, nrow, nb, ptr(Y), ptr(nzt), ptr(status), ptr(spec), None)),
    }
    flops = {"project": 2.0 * nrow * K * n, "solve": n**3 / 3.0 + 2.0 * nrow * n * n}
    for fn in stages.values():
        fn()  # warm-up, in order
    res["stages"] = {}
    for name in ("fourier", "prepare", "project", "solve", "store"):  # (project refreshes Y before every solve)
        reps = []
        for _ in range(args.reps):
            if name == "solve":
                stages["project"]()
            ctx.timer_start()
            stages[name]()
            reps.append(ctx.timer_stop())
        per = min(reps) / (1 if name == "fourier" else nb)
        r = {"ms_per_baseline" if name != "fourier" else "ms_per_call": per, "ms_spread": [min(reps), max(reps)]}
        if name in flops:
            r["tflops_fp64"] = flops[name] / (per * 1e-3) / 1e12
        res["stages"][name] = r
    res["stage_batch"] = nb
    res["status_nonzero"] = int((status.cpu().numpy() != 0).sum())

    # ---- the NumPy twin on this host, a few baselines of the same stream
    nh = min(args.host_baselines, nstack)
    hv, hw = vis[:, :nh].cpu().numpy().transpose(1, 2, 0), weight[:, :nh].cpu().numpy().transpose(1, 2, 0)
    cfg = dict(time_frac=0.0, freq_frac=0.0, remove_mean=True, weight_boost=1.0, window="nuttall", complex_timedomain=False)
    t0 = time.perf_counter()
    href, _ = twin.evaluate(hv, hw, prior(nh, ndelay), ndelay, np.arange(NFREQ), cfg, "wiener")
    res["host_numpy_twin_s_per_baseline"] = (time.perf_counter() - t0) / nh
    res["host_baselines"] = nh
    res["host_cores"] = len(os.sched_getaffinity(0))
    got = task.process(s).spectrum.device(ctx)[:nh].cpu().numpy()
    res["rel_diff_to_host_twin"] = twin.rel_err(got, href)
    print("DELAY_TIMING " + json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
