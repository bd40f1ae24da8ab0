"""Time the DPSS inpainting: one `DPSSFilterDelayStokesI.process`, whole and split by stage.

    python tools/dpss_timing.py [--stack N] [--out profiles/dpss_timing.json]

Two shapes: cfg 3's stream (256 freq x 758 stack x 1024 RA) and a 1024-channel variant with fewer stack entries (1024
freq x 64 stack x 1024 RA); `--stack N` caps the stack entries of both (the time per column does not depend on them).
The baselines give eight distinct delay cuts, 2 % of the samples are flagged in gaps 1 to 4 wide.  Each shape runs in a
child process of its own under a time limit; the first failure ends the run.  Reported per shape: the wall time of one
`process` (bases cached by a first call on a one-entry stream), the time per column, the modes per cut, and a second,
stage-synchronised run's split between pack, Gram, projection, factorisation (with the solve of the data), variance,
synthesis, PCHIP, gap flag and store, from the context's timer.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg3": (256, 758, 1024), "wide_band": (1024, 64, 1024)}  # nfreq, nstack, nra
LIMIT_S = 500


def child(name, stack_cap):
    sys.path.insert(0, ROOT)
    import types

    import numpy as np
    import scipy.constants
    import torch

    from draco_amd.analysis.interpolate import DPSSFilterDelayStokesI
    from draco_amd.core import containers
    from draco_amd.device import Context

    nfreq, nstack, nra = SHAPES[name]
    nstack = min(nstack, stack_cap) if stack_cap else nstack
    ctx = Context.get()
    freq = 800.0 - 0.390625 * np.arange(nfreq)
    cuts = 0.15 + 0.02 * (np.arange(nstack) % 8)
    stack = np.stack([np.zeros(nstack), cuts * 1e-6 * scipy.constants.c], axis=1)
    gen = torch.Generator(device=ctx.device).manual_seed(7)
    vis = torch.view_as_complex(torch.randn((nfreq, nstack, nra, 2), device=ctx.device, dtype=torch.float32, generator=gen))
    weight = torch.rand((nfreq, nstack, nra), device=ctx.device, dtype=torch.float32, generator=gen) + 0.5
    gap = torch.rand((nfreq, nstack, nra), device=ctx.device, dtype=torch.float32, generator=gen) < 0.008
    for shift in range(3):  # gaps 1 to 4 wide: each start is extended by a random number of channels
        more = gap & (torch.rand(gap.shape, device=ctx.device, generator=gen) < 0.6)
        gap[shift + 1 :] |= more[: nfreq - shift - 1]
    weight[gap] = 0.0
    flagged = float(gap.float().mean())
    del gap

    def stream(ns):
        s = containers.SiderealStream(freq=freq, ra=nra, stack=stack[:ns], allocate=False)
        s.attach("vis", vis[:, :ns].contiguous() if ns != nstack else vis)
        s.attach("vis_weight", weight[:, :ns].contiguous() if ns != nstack else weight)
        return s

    task = DPSSFilterDelayStokesI(halfwidths=[0.1], centres=[0.0], copy=True)
    task.setup(types.SimpleNamespace(lmax=1, mmax=1, frequencies=None))
    t0 = time.perf_counter()
    task.process(stream(min(8, nstack)))  # (the bases: host eigen-decompositions, cached on the task; warm-up)
    ctx.sync()
    res = {"shape": name, "nfreq": nfreq, "nstack": nstack, "nra": nra, "flagged_fraction": flagged, "bases_and_warmup_s": time.perf_counter() - t0,
           "modes": sorted({int(b.k) for b in task._basis_cache.values()}), "columns": nstack * nra}
    s = stream(nstack)
    t0 = time.perf_counter()
    out = task.process(s)
    ctx.sync()
    res["process_s"] = time.perf_counter() - t0
    res["us_per_column"] = 1e6 * res["process_s"] / (nstack * nra)
    assert bool(torch.isfinite(out.weight.device(ctx)).all())
    del out
    task._timings = {}
    t0 = time.perf_counter()
    task.process(s)
    ctx.sync()
    res["staged_process_s"] = time.perf_counter() - t0
    res["stage_ms"] = {k: round(v, 3) for k, v in task._timings.items()}
    total = sum(task._timings.values())
    res["stage_share"] = {k: round(v / total, 4) for k, v in task._timings.items()}
    print("DPSS_TIMING " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--stack", type=int, default=0, help="cap on the stack entries of both shapes (0: the full shapes)")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.stack)
        return 0
    results = []
    for name in SHAPES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--stack", str(args.stack)], capture_output=True, text=True, timeout=LIMIT_S)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print(f"{name}: exit status {p.returncode}; stopping")
            return 1
        results += [json.loads(line.split(" ", 1)[1]) for line in p.stdout.splitlines() if line.startswith("DPSS_TIMING ")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
