"""Times of the chi-squared mask path on one GPU, device-synchronised, the median of the runs after a warm-up:

* the weighted moving median on one 1024 x 8640 plane at (1, 601), (3, 601) and (101, 31), with the LDS bytes of a block
  and the blocks of a CU that leaves; at (101, 31) and (37, 181) the same plane with 0/1 weights beside ``dmm_rfi_medfilt``;
* ``RFIMaskChisqHighDelay.process`` with its defaults and with ``mask_type="sumthreshold"`` on a stack-collapsed
  ``TimeStream`` of that size, with the share of every stage;
* ``ReduceChisq`` over ``stack`` at 256 x 379 x 1024 complex64, with the bytes per second it achieves on two passes over
  the data and the weights.

    python tools/chisqmask_timing.py --out profiles/chisqmask_timing.json [--small]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from draco_amd import _lib
from draco_amd.analysis import flagging
from draco_amd.analysis.transform import ReduceChisq
from draco_amd.core import containers
from draco_amd.device import Context
from draco_amd.util import filters

HBM = 6.3e12  # bytes / s, the rate DESIGN.md compares streaming kernels with
LDS_CU = 160 * 1024


def timed(fn, reps=4):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return dict(times=ts, median_after_warmup=float(np.median(ts[1:])))


def lds_bytes(size, nf, nt, weighted):
    """What one block of the (weighted) median kernel keeps in LDS, as the entry points size it."""
    strip, tile, sample = (_lib.DMM_RFI_WMED_MAX_STRIP, _lib.DMM_RFI_WMED_TILE, 16) if weighted else (_lib.DMM_RFI_MAX_STRIP, 32, 8)
    rows = min(size[0], nf)
    T = max(1, min(tile, strip // rows - (size[1] - 1)))
    cols = min(T + size[1] - 1, nt)
    return dict(tile=T, lds_bytes=rows * cols * sample + cols * 4, blocks_per_cu=int(LDS_CU // (rows * cols * sample + cols * 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    args = ap.parse_args()
    nf, nt = (64, 700) if args.small else (1024, 8640)
    red = (8, 11, 256) if args.small else (256, 379, 1024)
    ctx = Context.get()
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(17)
    res = dict(plane=[nf, nt], hbm_rate=HBM)

    # ---- the medians
    ndof = torch.randint(40, 200, (nf, nt), generator=gen, device=ctx.device).to(torch.float64)
    lost = torch.rand((nf, nt), generator=gen, device=ctx.device) < 0.1
    w = ndof * ~lost / 2.0
    y = 1.0 + torch.sqrt(1.0 / torch.clamp(w, min=1.0)) * torch.randn((nf, nt), generator=gen, device=ctx.device, dtype=torch.float64)
    for size in ((1, 601), (3, 601), (101, 31)):
        size = filters.check_weighted_size(size, 2)
        r = timed(lambda: filters.moving_weighted_median_device(ctx, y, w, size))
        r.update(lds_bytes(size, nf, nt, True), ns_per_output=1e9 * r["median_after_warmup"] / (nf * nt))
        res[f"wmedfilt_{size[0]}x{size[1]}"] = r
        print(size, r, flush=True)
    keep = (~lost).to(torch.float64)
    flag = lost.to(torch.uint8)
    for size in ((101, 31), (37, 181)):
        a = timed(lambda: filters.moving_weighted_median_device(ctx, y, keep, size))
        b = timed(lambda: filters.medfilt_device(ctx, y, flag, size))
        same = bool(torch.equal(filters.moving_weighted_median_device(ctx, y, keep, size).view(torch.int64), filters.medfilt_device(ctx, y, flag, size).view(torch.int64)))
        res[f"unit_weights_{size[0]}x{size[1]}"] = dict(wmedfilt=a, medfilt=b, ratio=a["median_after_warmup"] / b["median_after_warmup"], bit_equal=same,
                                                        wmedfilt_block=lds_bytes(size, nf, nt, True), medfilt_block=lds_bytes(size, nf, nt, False))
        print(size, res[f"unit_weights_{size[0]}x{size[1]}"], flush=True)

    # ---- the mask task on a stack-collapsed time stream
    ts = containers.TimeStream(freq=800.0 - 0.390625 * np.arange(nf), stack=1, time=1.6e9 + 10.0 * np.arange(nt), allocate=False)
    vis = torch.complex(y.to(torch.float32), torch.zeros_like(y, dtype=torch.float32)).reshape(nf, 1, nt).contiguous()
    ts.attach("vis", vis)
    ts.attach("vis_weight", (2.0 * w).to(torch.float32).reshape(nf, 1, nt).contiguous())
    for mask_type in ("mad", "sumthreshold"):
        task = flagging.RFIMaskChisqHighDelay(mask_type=mask_type)
        task.setup()
        stages = {}

        def staged(name, fn):
            def wrapped(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                stages[name] = stages.get(name, 0.0) + time.perf_counter() - t0
                return out

            return wrapped

        task._collapse = staged("collapse", task._collapse)
        task.mask_1d = staged("mask_1d", task.mask_1d)
        task.mask_2d = staged("mask_2d", task.mask_2d)
        task.mask_2d_sumthreshold = staged("mask_2d_sumthreshold", task.mask_2d_sumthreshold)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            task.process(ts)  # warm-up
            stages.clear()
            out = {}
            r = timed(lambda: out.update(mask=task.process(ts)), reps=3)
        total = sum(r["times"])
        r["stage_share"] = {k: v / total for k, v in stages.items()}
        r["masked_fraction"] = float(out["mask"].mask.device(ctx).float().mean())
        res[f"process_{mask_type}"] = r
        print(mask_type, r, flush=True)

    # ---- ReduceChisq over the stack axis
    a, b, c = red
    st = containers.TimeStream(freq=800.0 - 0.390625 * np.arange(a), stack=b, time=1.6e9 + 10.0 * np.arange(c), allocate=False)
    st.attach("vis", torch.view_as_complex(torch.randn((a, b, c, 2), generator=gen, device=ctx.device, dtype=torch.float32)))
    st.attach("vis_weight", torch.rand((a, b, c), generator=gen, device=ctx.device, dtype=torch.float32) + 0.5)
    task = ReduceChisq(axes=["stack"], dataset="vis")
    r = timed(lambda: task.process(st), reps=6)
    once = a * b * c * (8 + 4)
    r.update(shape=list(red), bytes_two_passes=2 * once, rate=2 * once / r["median_after_warmup"], share_of_hbm=2 * once / r["median_after_warmup"] / HBM,
             rate_if_second_pass_is_cached=once / r["median_after_warmup"])
    res["reduce_chisq"] = r
    print("reduce_chisq", r, flush=True)

    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
