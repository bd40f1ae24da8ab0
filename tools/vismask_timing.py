"""Times of the transient RFI mask from visibilities on one GPU, device-synchronised: one warm-up, then five
repetitions, the median and the range.  The unit is one frequency of about 1800 Stokes-I baselines x 8640 times (a
``pair_rule="halfplane"`` telescope of 4 cylinders x 256 feeds x 2 polarisations: 7159 stack entries, 1790 baselines,
Bluestein at M = 4096).

* every new kernel of ``csrc/vismask.hip`` on that unit, with the bytes it has to move (its model) and the rate that is;
* the two moving medians of ``mad`` on the same plane, for scale;
* ``RFITransientVisMask.process`` on 16 frequencies, device-resident, with the share of every stage.

    python tools/vismask_timing.py --out profiles/vismask_timing.json [--small]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from draco_amd import _lib
from draco_amd.analysis import flagging, transform
from draco_amd.core import containers
from draco_amd.core.products import TransitTelescope
from draco_amd.device import Context, ptr
from draco_amd.util import filters, rfi

HBM = 6.3e12  # bytes / s, the rate DESIGN.md compares streaming kernels with


def timed(fn, reps=5):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return dict(times=ts, median=float(np.median(ts)), range=[float(min(ts)), float(max(ts))])


def with_model(r, nbytes):
    r.update(model_bytes=int(nbytes), rate_tb_s=nbytes / r["median"] / 1e12, share_of_hbm=nbytes / r["median"] / HBM)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a rehearsal at toy sizes")
    args = ap.parse_args()
    ncyl, nfeed, nt, nfreq = (2, 8, 700, 3) if args.small else (4, 256, 8640, 16)
    freq = 400.0 + 0.390625 * np.arange(nfreq)[::-1]
    t0 = time.perf_counter()
    tel = TransitTelescope(freq, lmax=1, ncyl=ncyl, nfeed_cyl=nfeed, npol_feed=2, pair_rule="halfplane", lsd_start=1.5e9)
    ubase, ptr_h, rows_h = transform.stokes_i_table(tel)
    nprod, nbase = len(tel.uniquepairs), len(ubase)
    ctx = Context.get()
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(23)
    res = dict(nprod=nprod, nbase=nbase, nt=nt, nfreq=nfreq, hbm_rate=HBM, telescope_s=time.perf_counter() - t0)
    print(res, flush=True)

    def noise(shape, dtype=torch.float32):
        return torch.randn(shape, generator=gen, device=ctx.device, dtype=dtype)

    # ---- the kernels on one frequency
    vis = torch.complex(1.0 + 0.5 * noise((1, nprod, nt)), 0.5 * noise((1, nprod, nt)))
    vis[0, :, nt // 3 : nt // 3 + 3] += 30.0
    weight = torch.full((1, nprod, nt), 3.0, device=ctx.device)
    weight[:, :, 100:103] = 0.0
    ptr_d, rows_d = ctx.to_device(ptr_h), ctx.to_device(rows_h)
    n = nbase * nt
    r = timed(lambda: transform.stokes_i_device(ctx, vis, weight, ptr_d, rows_d))
    res["stokes_i_sum"] = with_model(r, 12 * (len(rows_h) + nbase) * nt)
    vi, wi = transform.stokes_i_device(ctx, vis, weight, ptr_d, rows_d)
    time_s = 1.6e9 + 10.0 * np.arange(nt)
    ra = np.unwrap(tel.unix_to_lsa(time_s), period=360.0) * np.pi / 180.0
    cut = freq.min() * 1e6 / flagging.RFIVisMask.SPEED_OF_LIGHT * ubase[:, 0].max() / np.cos(np.deg2rad(tel.latitude))
    taps = ctx.to_device(filters.convolution_taps(ra, cut))
    res["ntap"] = int(taps.numel())
    r = timed(lambda: filters.wconv_filter_device(ctx, vi, wi, taps, highpass=True))
    res["wconv_filter"] = with_model(r, (8 + 4 + 16) * n)
    hp = filters.wconv_filter_device(ctx, vi, wi, taps, highpass=True)
    beams = torch.empty((1, nbase, nt), dtype=torch.float64, device=ctx.device)
    r = timed(lambda: _lib.check(_lib.lib.dmm_beam_abs_fft(ctx.handle, ptr(hp), 1, nbase, nt, ptr(beams))))
    res["beam_abs_fft"] = with_model(r, (16 + 8) * n)
    flag = wi.eq(0).all(dim=1, keepdim=True).expand(1, nbase, nt).to(torch.uint8).contiguous()
    for name, size in (("medfilt_base", (1, 101)), ("medfilt_dev", (1, 51))):
        res[name] = with_model(timed(lambda: filters.medfilt_device(ctx, beams, flag, size)), (8 + 1 + 8) * n)
    ratio = flagging._mad_device(ctx, beams, flag, (1, 101), (1, 51))[0]
    info = {}
    r = timed(lambda: rfi.hysteresis_device(ctx, ratio, 2.0, 8.0, info=info))
    r["sweeps"] = info["sweeps"]
    res["rfi_hysteresis"] = with_model(r, (8 + 1 + 1 + 1 + 4 * info["sweeps"]) * n)  # x, the state, the result; two reads and two writes of the state per sweep at most
    flags = rfi.hysteresis_device(ctx, ratio, 2.0, 8.0)
    count = torch.zeros((1, nt), dtype=torch.int32, device=ctx.device)
    r = timed(lambda: _lib.check(_lib.lib.dmm_rfi_beam_count(ctx.handle, ptr(flags), 1, nbase, nt, ptr(count))))
    res["rfi_beam_count"] = with_model(r, n + 8 * nt)
    for k in ("stokes_i_sum", "wconv_filter", "beam_abs_fft", "medfilt_base", "medfilt_dev", "rfi_hysteresis", "rfi_beam_count"):
        print(k, {a: res[k][a] for a in ("median", "range", "rate_tb_s")}, flush=True)
    del vis, weight, vi, wi, hp, beams, ratio, flags, flag

    # ---- the task on nfreq frequencies, with the share of every stage
    stream = containers.TimeStream(freq=freq, stack=nprod, time=time_s, allocate=False)
    v = torch.complex(1.0 + 0.5 * noise((nfreq, nprod, nt)), 0.5 * noise((nfreq, nprod, nt)))
    v[nfreq // 2, :, nt // 3 : nt // 3 + 3] += 30.0
    w = torch.full((nfreq, nprod, nt), 3.0, device=ctx.device)
    w[:, :, 100:103] = 0.0
    stream.attach("vis", v)
    stream.attach("vis_weight", w)
    task = flagging.RFITransientVisMask()
    task.setup(tel)
    stages = {}

    def wrap(owner, name, label):
        orig = getattr(owner, name)

        def inner(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = orig(*a, **k)
            torch.cuda.synchronize()
            stages[label] = stages.get(label, 0.0) + time.perf_counter() - t
            return out

        setattr(owner, name, inner)

    wrap(transform, "stokes_I", "stokes_i")
    wrap(filters, "wconv_filter_device", "highpass")
    wrap(_lib.lib, "dmm_beam_abs_fft", "beam_abs_fft")
    wrap(flagging, "_mad_device", "mad")
    wrap(rfi, "hysteresis_device", "hysteresis")
    wrap(rfi, "sir_device", "sir")
    wrap(_lib.lib, "dmm_rfi_beam_count", "beam_count")
    out = {}

    def run():
        stages.clear()
        out["mask"] = task.process(stream)

    r = timed(run)
    r["stages_last_run"] = dict(stages)
    r["stages_last_run"]["rest"] = r["times"][-1] - sum(stages.values())
    r["masked_fraction"] = float(np.asarray(out["mask"].mask[:]).mean())
    r["per_frequency"] = r["median"] / nfreq
    res["process"] = r
    print("process", r, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
