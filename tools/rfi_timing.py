"""Time the RFI flagging: `medfilt` alone at both default windows and one default `RFISensitivityMask.process`.

    python tools/rfi_timing.py [--nfreq 1024] [--ntime 8640] [--npol 3] [--out profiles/rfi_timing.txt]

The plane is the radiometer ratio of a day: unit mean, 5 % noise, a few bad channels, broadband bursts and single
spikes, 3 % of the weights zero.  Reported: the time of each moving median (events on the stream), its LDS reads per
output by the kernel's own accounting and the share of the LDS rate that makes; then the task's wall time and the time
per kernel class (every wrapped call synchronised: the sum exceeds the unsynchronised wall time by the launch gaps).

LDS accounting of the median: the selection's reads depend on the data (a column is searched only inside the bracket
its earlier probes left), so they are counted by replaying the kernel's bisection on the host for 48 outputs of the
timed plane; the rank sort reads sf keys per strip sample, (st + T - 1) sf^2 / T per output, whatever the data.  The
bound without brackets, 65 steps of one ceil(log2(sf + 1))-read search in each of the st columns, is printed beside it.
Rates from the microarchitecture guide: 128 B per clock and CU for 8-byte LDS reads, 256 CUs, 2.4 GHz; 6.3 TB/s HBM.
"""

import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LDS_RATE = 256 * 128 * 2.4e9  # bytes per second, 8-byte reads
HBM_RATE = 6.3e12
TILE = 32


def replay_reads(x, keep, f, t, size):
    """(LDS reads, bisection steps) of the kernel's selection for output (f, t): the same brackets, counted."""
    import numpy as np

    hf, ht = size[0] // 2, size[1] // 2
    nf, nt = x.shape
    cols = []
    for c in range(max(t - ht, 0), min(t + ht, nt - 1) + 1):
        r = slice(max(f - hf, 0), min(f + hf, nf - 1) + 1)
        bits = x[r, c][keep[r, c]].view(np.uint64)
        keys = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
        cols.append(sorted(int(k) for k in keys))
    n = sum(len(c) for c in cols)
    if n == 0:
        return 0, 0
    k1 = (n - 1) // 2
    kmin, kmax = min(c[0] for c in cols if c), max(c[-1] for c in cols if c)
    reads = 2 * sum(1 for c in cols if c)  # the first and the last key of every column
    if kmin == kmax:
        return reads, 0
    b = (kmin ^ kmax).bit_length() - 1
    xk = (kmin >> (b + 1)) << (b + 1)
    lo, hi = [0] * len(cols), [len(c) for c in cols]
    clo, chi, steps = 0, n, 0
    for bit in range(b, -1, -1):
        tk = xk | (1 << bit)
        mid = []
        for j, col in enumerate(cols):
            l, ln = lo[j], hi[j] - lo[j]
            while ln > 0:
                half = ln >> 1
                reads += 1
                if col[l + half] < tk:
                    l, ln = l + half + 1, ln - half - 1
                else:
                    ln = half
            mid.append(l)
        c = sum(mid)
        steps += 1
        if c <= k1:
            xk, clo, lo = tk, c, mid
        else:
            chi, hi = c, mid
        if chi - clo == 1:
            break
    return reads + 2, steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--nfreq", type=int, default=1024)
    ap.add_argument("--ntime", type=int, default=8640)
    ap.add_argument("--npol", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from draco_amd.analysis import flagging
    from draco_amd.core import containers
    from draco_amd.device import Context
    from draco_amd.util import filters, rfi

    nf, nt, npol = args.nfreq, args.ntime, args.npol
    ctx = Context.get()
    rng = np.random.default_rng(3)
    ratio = (1.0 + 0.05 * rng.standard_normal((nf, npol, nt), dtype=np.float32)).astype(np.float32)
    ratio[rng.integers(nf, size=8)] += 0.6
    for t in rng.integers(nt - 4, size=6):
        ratio[:, :, t : t + 3] += 0.4
    ratio[rng.uniform(size=ratio.shape) < 2e-4] += 1.0
    weight = np.ones_like(ratio)
    weight[rng.uniform(size=ratio.shape) < 0.03] = 0.0
    lines = [f"RFI timing: {nf} freq x {npol} pol x {nt} time, torch {torch.__version__}"]

    y = ctx.to_device(ratio[:, 0].astype(np.float64))
    flag = ctx.to_device((weight[:, 0] == 0).view(np.uint8))
    for size in ((37, 181), (101, 31)):
        filters.medfilt_device(ctx, y, flag, size)  # warm-up
        ctx.sync()
        ctx.timer_start()
        filters.medfilt_device(ctx, y, flag, size)
        ms = ctx.timer_stop()
        sf, st = size
        x64, keep = ratio[:, 0].astype(np.float64), weight[:, 0] != 0
        picks = [replay_reads(x64, keep, int(rng.integers(nf)), int(rng.integers(nt)), size) for _ in range(48)]
        select = float(np.mean([p[0] for p in picks]))
        steps = float(np.mean([p[1] for p in picks]))
        sort = (st + TILE - 1) * sf * sf / TILE
        bound = 65 * st * math.ceil(math.log2(sf + 1))
        lds = (select + sort) * 8 * nf * nt / (ms * 1e-3)
        hbm = nf * nt * (8 + 8 + 1) / (ms * 1e-3)
        lines.append(f"medfilt {size}: {ms:9.2f} ms  {1e6 * ms / (nf * nt):8.3f} ns/output  LDS reads/output: selection {select:7.0f} in {steps:4.1f} steps "
                     f"(without brackets <= {bound}), sort {sort:6.0f}  => {100 * lds / LDS_RATE:5.1f} % of the LDS rate, {100 * hbm / HBM_RATE:6.3f} % of the HBM rate")

    # ---- the default task, whole and per kernel class
    sens = containers.SystemSensitivity(freq=800.0 - 400.0 / nf * np.arange(nf), pol=np.arange(npol).astype(str), time=1.6e9 + 10.0 * np.arange(nt))
    sens.measured[:], sens.radiometer[:], sens.weight[:] = ratio, 1.0, weight
    for ds in sens.datasets.values():
        ds.set_device(ctx.to_device(ds.host()))
    task = flagging.RFISensitivityMask()
    task.setup()
    ctx.sync()
    t0 = time.perf_counter()
    out = task.process(sens)
    ctx.sync()
    wall = time.perf_counter() - t0
    lines.append(f"RFISensitivityMask (defaults, mask_type combine): {wall:8.3f} s wall, {100 * out.mask[:].mean():.2f} % masked")

    spent = {}

    def timed(name, fn):
        def wrapped(*a, **k):
            ctx.sync()
            t = time.perf_counter()
            r = fn(*a, **k)
            ctx.sync()
            spent[name] = spent.get(name, 0.0) + time.perf_counter() - t
            return r

        return wrapped

    filters.medfilt_device = timed("moving median", filters.medfilt_device)
    filters.quantile_device = timed("row quantile", filters.quantile_device)
    rfi.sumthreshold_device = timed("SumThreshold", rfi.sumthreshold_device)
    rfi.sir_device = timed("SIR", rfi.sir_device)
    for name in ("_absdev", "_nsigma", "_mask_op"):
        setattr(flagging, name, timed("elementwise", getattr(flagging, name)))
    flagging._TVBands.flag = timed("TV fractions", flagging._TVBands.flag)
    t0 = time.perf_counter()
    task.process(sens)
    ctx.sync()
    staged = time.perf_counter() - t0
    lines.append(f"  synchronised per class ({staged:.3f} s wall):")
    for name, s in sorted(spent.items(), key=lambda kv: -kv[1]):
        lines.append(f"    {name:14s} {s:8.3f} s  {100 * s / staged:5.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
