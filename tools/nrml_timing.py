"""Time the NRML delay power spectrum estimator on a CHIME-like block.

    python tools/nrml_timing.py [--shape NBASE,NRA,NCHAN] [--out profiles/nrml_timing.json]

Default shape: 32 baselines x 1024 RA samples x 512 channels (-> 1022 delays, ``skip_nyquist=False``).  The stream is
a delay spectrum that falls four decades from zero delay plus noise at 0.1, in double precision on the device.  Every
timed call is warmed up once at the same shape and timed with a host clock around work that ends in a device
synchronise.

Reported, each as the median of the repeats with their range: the whole optimisation
(``DelayPowerSpectrumNRML.process`` at the default tolerance) in seconds per baseline and per outer iteration; one
value-and-gradient evaluation of the batch; the Hessian of the batch (P and Q formed by matrix products plus an
element-wise pass) with the float64 operations it executes over its time, against the FP64 matrix-core peak of
DESIGN.md (78.6 TFLOP/s); and for context the float64 NumPy evaluator's time for one value, gradient and Hessian of
one baseline on the same host.

Operations per baseline, n = nchan, N = ndelay, tiles of 64: four real planes over K = 2 n on all T^2 tiles, T = ceil(N /
64): 4 x 2 x 64^2 x 2 n each (16 N^2 n for an N that fills its tiles).
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64 = 78.6e12
DF = 0.390625


def make_stream(np, ctx, nbase, nra, nchan, seed=11):
    from draco_amd.core import containers
    import torch

    N = 2 * (nchan - 1)
    g = torch.Generator(device=ctx.device).manual_seed(seed)
    tau = np.abs(np.fft.fftfreq(N)) * 2
    S = ctx.to_device(100.0 * 10.0 ** (-4.0 * tau**0.8) + 1e-3)
    E = ctx.to_device(np.exp(-2j * np.pi * ((np.arange(nchan)[:, None] * np.arange(N)[None, :]) % N) / N))
    d = torch.randn((nbase * nra, N), dtype=torch.complex128, device=ctx.device, generator=g) * torch.sqrt(S)
    vis = d @ E.T + 0.1 * torch.randn((nbase * nra, nchan), dtype=torch.complex128, device=ctx.device, generator=g)
    vis = vis.reshape(nbase, nra, nchan).permute(2, 0, 1).contiguous()
    weight = torch.full((nchan, nbase, nra), 100.0, dtype=torch.float64, device=ctx.device)
    weight[[nchan // 7, nchan // 3, nchan // 3 + 1]] = 0.0
    ss = containers.SiderealStream(freq=400.0 + DF * np.arange(nchan), ra=nra, stack=nbase, allocate=False)
    for name, t in (("vis", vis), ("vis_weight", weight)):
        ss.datasets[name] = containers.Dataset(dev=t, attrs={"axis": ss._dataset_spec[name]["axes"]})
    return ss, N


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="32,1024,512", help="NBASE,NRA,NCHAN")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workspace-mib", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from draco_amd.analysis import delay, delayopt
    from draco_amd.device import Context

    nbase, nra, nchan = (int(v) for v in args.shape.split(","))
    ctx = Context.get()
    ss, N = make_stream(np, ctx, nbase, nra, nchan)

    def clock(fn):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return time.perf_counter() - t0, r

    task = delay.DelayPowerSpectrumNRML(sample_axis="ra", nsamp=100, skip_nyquist=False, save_samples=True, save_spectrum_mask=True, workspace_mib=args.workspace_mib)

    def stat(ts):
        ts = sorted(ts)
        return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "repeats": len(ts)}

    clock(lambda: task.process(ss))  # warm-up at this shape
    runs = [clock(lambda: task.process(ss)) for _ in range(args.repeats)]
    out = runs[-1][1]
    t_proc = stat([t for t, _ in runs])
    t_all = t_proc["median_s"]
    samples = out.datasets["spectrum_samples"][:]
    iters = (samples.any(axis=2).sum(axis=0) - 1).astype(int)
    flagged = int(out.datasets["spectrum_mask"][:].sum())

    # one batch, as the task builds it, for the evaluations
    delays, channel_ind = task._calculate_delays(ss)
    name, axes, waxes, fold = task._resolve(ss)
    data, weight, data_v, weight_v, fold_n = task._prepare_inputs(ss, ctx, name, axes, waxes, fold)
    T = -(-N // 64)
    flops = nbase * T * T * 4 * 2 * 64 * 64 * 2 * nchan
    (b0, ev), = list(delay.nrml_evaluators(ctx, data_v, weight_v, fold_n, nbase, nra, channel_ind, N, "nuttall", remove_mean=True, time_frac=0.0, freq_frac=0.0, weight_boost=1.0,
                                           workspace_mib=args.workspace_mib))
    live = ev.base == 0
    x0 = np.log(ev.S0.cpu().numpy())
    ev.value_grad(x0, live)  # warm-up
    t_vg = stat([clock(lambda: ev.value_grad(x0, live))[0] for _ in range(args.repeats)])
    ev.hessian(live)
    t_h = stat([clock(lambda: ev.hessian(live))[0] for _ in range(max(args.repeats, 5))])
    res = {"value_grad": t_vg, "hessian": t_h, "hessian_tflops": flops / t_h["median_s"] / 1e12, "hessian_share_of_f64_matrix_peak": flops / t_h["median_s"] / PEAK_F64}
    del ev

    # the float64 NumPy evaluator on one baseline: one value, gradient and Hessian
    d0 = ss.datasets["vis"][:][:, 0, :].T
    w0 = ss.datasets["vis_weight"][:][:, 0, :].mean(axis=1)
    d0 = d0 - d0.mean(axis=0, keepdims=True)
    keep = w0 > 0
    X, MF, Nm, nsamp, S0 = delayopt._model_host(d0[:, keep], N, w0[keep], "nuttall", np.arange(nchan)[keep])
    f = delayopt.AddFunctions([delayopt.LogLikePS(X, MF, Nm, nsamp, bounds=(1e-15, 1e10), device=False), delayopt.GaussianProcessPrior(N, width=5, alpha=1.0, kernel="matern", nu=1.5)])
    x = np.log(S0)
    t0 = time.perf_counter()
    f.value(x), f.gradient(x), f.hessian(x)
    t_numpy = time.perf_counter() - t0

    doc = {
        "tool": "tools/nrml_timing.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "f64_matrix_peak_flops": PEAK_F64,
        "shape": {"nbase": nbase, "nra": nra, "nchan": nchan, "ndelay": N}, "workspace_mib": args.workspace_mib,
        "process": t_proc, "process_s_per_baseline": t_all / nbase, "outer_iterations": iters.tolist(), "process_s_per_outer_iteration": t_all / max(1, int(iters.max())),
        "flagged_baselines": flagged, **res, "numpy_one_baseline_value_gradient_hessian_s": t_numpy,
    }
    print(json.dumps(doc))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
