"""Wall times of the null-filter build (64 distinct filters of order 1024 at 160 and 400 modes) and of one
``DelayFilter.process`` on ``[1024, 256, 2048]`` complex64: device-synchronised, the median of the runs after a warm-up.

    python tools/nullfilter_timing.py [out.json]
"""
import os, sys, time, types, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from draco_amd.util import filters
from draco_amd.device import Context
from draco_amd.core import containers
from draco_amd.analysis.delay import DelayFilter

ctx = Context.get()
DF = 0.390625
res = {}
n = 1024
freq = 600 + DF * np.arange(n)
fd = ctx.to_device(freq)
for cut in (0.1, 0.25):
    K = int(4.0 * np.ptp(freq) * cut + 0.5)
    rng = np.random.default_rng(99)
    masks = rng.uniform(size=(64, n)) > 0.15
    ts = []
    for rep in range(6):
        info = {}
        torch.cuda.synchronize(); t0 = time.perf_counter()
        nf, status, nkeep, sig = filters.build_null_filters(ctx, fd, [cut] * 64, K, masks, None, info=info, workspace_mib=4096)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    res[f"build64_K{K}"] = dict(times=ts, median_after_warmup=float(np.median(ts[1:])), status=int(status.sum()), sweeps=[int(info["sweeps"].min()), int(info["sweeps"].max())],
                                nkeep=[int(nkeep.min()), int(nkeep.max())])
    print(K, res[f"build64_K{K}"], flush=True)
    del nf

# ---- one DelayFilter.process on [1024, 256, 2048] complex64
nstack, nt = 256, 2048
gen = torch.Generator(device=ctx.device); gen.manual_seed(5)
vis = torch.randn((n, nstack, nt, 2), generator=gen, device=ctx.device, dtype=torch.float32)
vis = torch.view_as_complex(vis)
weight = torch.rand((n, nstack, nt), generator=gen, device=ctx.device, dtype=torch.float32) + 0.5
chan = torch.rand((n, nstack), generator=gen, device=ctx.device) < 0.15
weight *= (~chan)[:, :, None]
prod = np.zeros(nstack, dtype=[("input_a", "<u2"), ("input_b", "<u2")]); prod["input_b"] = np.arange(1, nstack + 1)
feedpos = np.zeros((nstack + 1, 2)); feedpos[1:, 1] = np.linspace(0.0, 75.0, nstack)
ss = containers.SiderealStream(freq=freq, ra=nt, prod=prod, input=nstack + 1, allocate=False)
ss.attach("vis", vis); ss.attach("vis_weight", weight)
task = DelayFilter(delay_cut=0.1, za_cut=1.0, workspace_mib=8192)
task.setup(types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None))
cuts = task._cuts(prod)
ts = []
for rep in range(4):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    task.process(ss)
    torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
res["process_1024x256x2048_c64"] = dict(times=ts, median_after_warmup=float(np.median(ts[1:])), cuts=[float(cuts.min()), float(cuts.max())],
                                        num_modes=[int(4 * np.ptp(freq) * cuts.min() + 0.5), int(4 * np.ptp(freq) * cuts.max() + 0.5)], finite=bool(torch.isfinite(torch.view_as_real(ss.vis.device(ctx))).all()))
print(res["process_1024x256x2048_c64"], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
