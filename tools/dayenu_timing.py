"""Time the DAYENU delay filter: filter build and apply separately, with the context's timer.

    python tools/dayenu_timing.py [--out profiles/dayenu_timing.json]

Two shapes: cfg 3's stream (256 freq x 379 stack x 1024 RA) and a CHIME-like slice (1024 freq x 64 stack x 4096 RA);
every stack entry has its own cutoff, so every matrix is built.  Each shape runs in a child process of its own under a
time limit; the first failure ends the run.  Reported per shape: mask, build and apply times, the apply's achieved FP64
TFLOPS (6 n^2 nra flops per item: 2 n^2 per real data column, two of them per sample, and 2 n^2 per weight column) and
bytes per second (vis and weight read and written once, each filter read once), and the time of the NumPy twin
(`numpy.linalg.pinv` + two matmuls, as the reference does it) on the host for a stated subsample of baselines.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg3": (256, 379, 1024, 8), "chime_slice": (1024, 64, 4096, 2)}  # nfreq, nstack, nra, host baselines
LIMIT_S = 240


def child(name):
    sys.path.insert(0, ROOT)
    import ctypes as C

    import numpy as np
    import torch

    from draco_amd import _lib
    from draco_amd.analysis import dayenu
    from draco_amd.device import Context, ptr

    nfreq, nstack, nra, nhost = SHAPES[name]
    ctx = Context.get()
    rng = np.random.default_rng(5)
    freq = 400.0 + 0.390625 * np.arange(nfreq)
    cuts = 0.1 + 0.15 * np.arange(nstack) / nstack
    vis = torch.view_as_complex(torch.randn((nfreq, nstack, nra, 2), device=ctx.device, dtype=torch.float32))
    weight = torch.rand((nfreq, nstack, nra), device=ctx.device, dtype=torch.float32) + 0.5
    weight[torch.from_numpy(rng.uniform(size=nfreq) < 0.125).to(ctx.device)] = 0.0
    data = dayenu._side(vis, 2 * nra, 2 * nstack * nra, 1, 2 * nra, 0)
    wside = dayenu._side(weight, nra, nstack * nra, 1, nra, 0)
    flag_d = ctx.empty((1, nstack, nfreq), np.uint8)
    res = {"shape": name, "nfreq": nfreq, "nstack": nstack, "nra": nra}

    def timed(fn, reps):
        best = None
        for _ in range(reps):
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop()
            best = ms if best is None else min(best, ms)
        return best

    res["mask_ms"] = timed(lambda: _lib.check(_lib.lib.dmm_dayenu_mask(ctx.handle, 0, 0, nfreq, nstack, 1, C.byref(wside), ptr(flag_d))), 2)
    flags = flag_d.cpu().numpy().reshape(nstack, nfreq)
    bands = np.stack([cuts, np.full(nstack, 1e-12)], axis=-1)[:, None, :]
    freq_d = ctx.to_device(freq)
    nf = ctx.empty((nstack, nfreq, nfreq), np.float64)
    status = [None]

    def build():
        status[0] = dayenu.build_filters(ctx, freq_d, bands, flags, out=nf)[1]

    build()  # (warm-up: scratch allocation)
    t0 = time.perf_counter()
    ctx.timer_start()
    build()
    res["build_ms"] = ctx.timer_stop()
    res["build_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    res["build_failed"] = int(status[0].sum())
    imat = ctx.to_device(np.arange(nstack, dtype=np.int32))
    apply = lambda: dayenu.apply_filters(ctx, 0, 0, nfreq, nstack, 1, nf, imat, None, None, nstack, data, wside)  # noqa: E731
    res["apply_ms"] = timed(apply, 3)
    flops = 6.0 * nfreq * nfreq * nra * nstack
    nbytes = 24.0 * nfreq * nra * nstack + 8.0 * nfreq * nfreq * nstack
    res["apply_tflops_fp64"] = flops / (res["apply_ms"] * 1e-3) / 1e12
    res["apply_gb_per_s"] = nbytes / (res["apply_ms"] * 1e-3) / 1e9
    # the NumPy twin of the same slice on the host, for `nhost` baselines
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dayenu_twin as twin

    hv = (rng.normal(size=(nfreq, nra)) + 1j * rng.normal(size=(nfreq, nra))).astype(np.complex64)
    hw = rng.uniform(0.5, 1.5, size=(nfreq, nra)).astype(np.float32) * flags[0][:, None]
    t0 = time.perf_counter()
    for b in range(nhost):
        twin.filter_item(freq, cuts[b], hv, hw, 1e-12)
    res["host_twin_s_per_baseline"] = (time.perf_counter() - t0) / nhost
    res["host_baselines"] = nhost
    res["host_cores"] = len(os.sched_getaffinity(0))
    res["gpu_s_per_baseline"] = 1e-3 * (res["build_ms"] + res["apply_ms"]) / nstack
    print("DAYENU_TIMING " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return 0
    results = []
    for name in SHAPES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=LIMIT_S)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"{name}: exit status {p.returncode}; stopping")
            return 1
        results += [json.loads(line.split(" ", 1)[1]) for line in p.stdout.splitlines() if line.startswith("DAYENU_TIMING ")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
