"""Time the noise-model kernels stage by stage: the pack, factorisation and store of ReconstructVisFreqCov, the gather of
ReconstructVisWeight, the colouring of FreqCorrelatedNoise, and the host draw and upload of its normal variates.

    python tools/noisemodel_timing.py [--shape NPOL,NFREQ,NEW,NNS,NRA] [--out profiles/noisemodel_timing.json]

Default shape: 2 pol x 64 freq x 4 ew x ns 63 x 2048 RA.  The covariances are ``A A^T + 4 I`` with ``A [freq, 3]`` unit
normal per sample, the weights float32 in 0.5 ... 1.5 with 3 % zeros.  Every stage is called as the tasks call it, warmed
up once at the same shape and timed with a host clock around work that ends in a device synchronise.

Reported: seconds per stage, the bytes each stage has to move counted from the shapes (its floor: pack and store take
the covariance once in and once out, of which the kernels move the triangle they need; the colouring is bounded by its
complex64 and float32 outputs, its operands are listed beside them), the rates against 6.1 TB/s (the read-once stream of
DESIGN.md 7k); for one ``(pol, ew)`` slab the host draw (``util.random.complex_normal`` into pinned memory) and the
upload, separately; and ``FreqCorrelatedNoise.process`` as a whole, to show which of the two bounds it.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STREAM = 6.1e12
PEAK_F64_VECTOR = 78.6e12  # (the vector FP64 peak equals the matrix-core one on this part)


def time_shape(shape, repeats):
    import numpy as np
    import torch

    from draco_amd import _lib
    from draco_amd.core import containers
    from draco_amd.device import Context, ptr
    from draco_amd.synthesis.noise import FreqCorrelatedNoise
    from draco_amd.util import random

    npol, n, new, nns, nra = shape
    ctx = Context.get()
    lib = _lib.lib
    dev = ctx.device

    def clock(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return time.perf_counter() - t0

    def best(fn):
        return min([clock(fn) for _ in range(repeats + 1)][1:])  # (the first is the warm-up)

    gen = torch.Generator(device=dev).manual_seed(7)
    A = torch.randn((npol, new, nra, n, 3), generator=gen, device=dev, dtype=torch.float64)
    cov = (A @ A.transpose(-1, -2) + 4.0 * torch.eye(n, device=dev, dtype=torch.float64)).permute(0, 3, 4, 1, 2).contiguous()
    weight = (0.5 + torch.rand((npol, n, new, nra), generator=gen, device=dev, dtype=torch.float32)) * (torch.rand((npol, n, new, nra), generator=gen, device=dev) > 0.03)
    weight = weight.contiguous()
    scale = torch.full((npol, n, n, new), 0.25, device=dev, dtype=torch.float64)
    del A
    total = npol * new * nra
    chunk = min(total, 65535)
    G = ctx.empty((chunk, n, n), np.float64)
    status = ctx.empty((chunk,), np.int32)
    chol = ctx.empty((npol, new, nra, n, n), np.float64)
    wout = ctx.empty((npol, n, new, nra), np.float32)

    def pack():
        _lib.check(lib.dmm_noisemodel_pack(ctx.handle, npol, n, new, nra, 0, chunk, ptr(cov), ptr(scale), ptr(weight), ptr(G), ptr(wout)))

    def factor():
        _lib.check(lib.dmm_noisemodel_factor(ctx.handle, n, chunk, ptr(G), ptr(status)))

    def store():
        _lib.check(lib.dmm_noisemodel_store(ctx.handle, npol, n, new, nra, 0, chunk, ptr(G), ptr(weight), ptr(status), ptr(chol)))

    t_pack = best(pack)
    ts = []
    for _ in range(repeats + 1):  # (the factorisation works in place: pack again before every run)
        pack()
        ts.append(clock(factor))
    t_factor = min(ts[1:])
    assert not bool(status.any())
    t_store = best(store)
    for s0 in range(chunk, total, chunk):  # (the rest of the factors, for the colouring below)
        ns = min(chunk, total - s0)
        _lib.check(lib.dmm_noisemodel_pack(ctx.handle, npol, n, new, nra, s0, ns, ptr(cov), ptr(scale), ptr(weight), ptr(G), ptr(wout)))
        _lib.check(lib.dmm_noisemodel_factor(ctx.handle, n, ns, ptr(G), ptr(status)))
        _lib.check(lib.dmm_noisemodel_store(ctx.handle, npol, n, new, nra, s0, ns, ptr(G), ptr(weight), ptr(status), ptr(chol)))
    ctx.sync()
    del G, cov

    # ---- the gather of ReconstructVisWeight: a telescope's worth of stack entries, three quarters of them taking part
    nstack = 4 * new * nns
    rng = np.random.default_rng(3)
    cell = rng.integers(0, npol * new, size=nstack).astype(np.int32)
    cell[rng.uniform(size=nstack) < 0.25] = -1
    tabs = [ctx.to_device(np.full((npol, n, new), 0.5)), ctx.to_device(cell), ctx.to_device(rng.integers(1, 200, size=nstack).astype(np.float64))]
    wss = ctx.empty((n, nstack, nra), np.float32)
    t_weight = best(lambda: _lib.check(lib.dmm_noisemodel_weight(ctx.handle, npol, n, new, nra, nstack, ptr(weight), *(ptr(t) for t in tabs), ptr(wss))))
    weight_bytes = wss.numel() * 4 + int((cell >= 0).sum()) * n * nra * 4
    del wss

    # ---- one slab of the colouring, its draw and its upload
    red = rng.integers(1, 200, size=(npol, new, nns)).astype(np.int32)
    red_d, isr_d = ctx.to_device(red), ctx.to_device(1.0 / np.sqrt(red))
    vis = ctx.empty((npol, n, new, nns, nra), np.complex64)
    vw = ctx.empty((npol, n, new, nns, nra), np.float32)
    zp = torch.empty((nra, n, nns), dtype=torch.complex64, pin_memory=True)
    z = zp.numpy()
    zd = ctx.empty((nra, n, nns), np.complex64)
    g = np.random.default_rng(5)
    t_draw = min(clock(lambda: random.complex_normal(scale=1.0, out=z, rng=g)) for _ in range(repeats))
    t_upload = best(lambda: zd.copy_(zp, non_blocking=True))
    t_colour = best(lambda: _lib.check(lib.dmm_noise_colour(ctx.handle, npol, n, new, nns, nra, 0, 0, ptr(chol), ptr(zd), ptr(wout), ptr(red_d), ptr(isr_d), ptr(vis), ptr(vw))))
    pc = ctx.to_device(np.arange(npol, dtype=np.int32))
    t_herm = best(lambda: _lib.check(lib.dmm_noise_hermitian(ctx.handle, npol, n, new, nns, nra, ptr(pc), ptr(vis))))
    del vis, vw

    # ---- the task as a whole
    model = containers.FreqNoiseModel(pol=np.array(["XX", "YY", "XY", "YX"])[:npol], freq=600.0 + 0.390625 * np.arange(n), ew=new, ns=nns, ra=nra, allocate=False)
    model.add_dataset("freq_cov")
    model.attach("freq_cov", chol)
    model.attach("weight", wout)
    model.datasets["redundancy"] = containers.Dataset(host=red)
    task = FreqCorrelatedNoise(seed=1)
    t_task = best(lambda: task.process(model))

    mat = npol * new * nra * n * n * 8
    tri = npol * new * nra * n * (n + 1) // 2 * 8
    slab_out = n * nns * nra * 12
    slab_in = nra * n * n * 8 + nra * n * nns * 8
    colour_flop = 2.0 * nra * (2 * nns) * n * (n + 1) / 2

    def rate(b, t):
        return {"bytes": int(b), "tb_per_s": b / t / 1e12, "share_of_stream_yardstick": b / t / HBM_STREAM}

    return {
        "shape": {"npol": npol, "nfreq": n, "new": new, "nns": nns, "nra": nra},
        "samples": total,
        "samples_timed_pack_factor_store": chunk,
        "stage_s": {"pack": t_pack, "factor": t_factor, "store": t_store, "weight_gather": t_weight, "colour_one_slab": t_colour, "hermitian": t_herm,
                    "host_draw_one_slab": t_draw, "upload_one_slab": t_upload},
        "task_s": {"FreqCorrelatedNoise": t_task, "slabs": npol * new, "host_draw_all_slabs": t_draw * npol * new, "colour_all_slabs": t_colour * npol * new},
        "pack": {"floor_once_in_once_out": rate(2 * mat * chunk / total, t_pack), "moved_triangle_in_and_out": rate(2 * tri * chunk / total, t_pack)},
        "factor": {"flop": chunk * n**3 / 3.0, "tflops": chunk * n**3 / 3.0 / t_factor / 1e12, "in_place": rate(2 * tri * chunk / total, t_factor)},
        "store": {"floor_once_in_once_out": rate(2 * mat * chunk / total, t_store), "moved_triangle_in_matrix_out": rate((tri + mat) * chunk / total, t_store)},
        "weight_gather": rate(weight_bytes, t_weight),
        "colour": {"floor_outputs": rate(slab_out, t_colour), "outputs_and_operands": rate(slab_out + slab_in, t_colour), "flop": colour_flop,
                   "tflops": colour_flop / t_colour / 1e12, "share_of_f64_vector_peak": colour_flop / t_colour / PEAK_F64_VECTOR},
        "host_draw": {"complex_normals_per_slab": nra * n * nns, "normals_per_s": nra * n * nns / t_draw, "upload_gb_per_s": nra * n * nns * 8 / t_upload / 1e9},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="2,64,4,63,2048", help="NPOL,NFREQ,NEW,NNS,NRA")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    res = time_shape(tuple(int(x) for x in args.shape.split(",")), args.repeats)
    doc = {"tool": "tools/noisemodel_timing.py", "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "stream_yardstick_bytes_per_s": HBM_STREAM, "cases": [res]}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
