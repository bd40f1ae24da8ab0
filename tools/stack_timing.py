#!/usr/bin/env python
"""Host-clock timing of the source-stacking tasks (`csrc/sourcestack.hip`) on inputs built on the device from a seed: a
ring map of `--pol` x `--freq` x `--ra` x `--el` float64 with weights (default 4 x 64 x 4096 x 1024: 8.6 GB each) and a
catalogue of `--sources` sources (default 200000) uniform over the map and the band.

Timed, each after one warm-up call, `--reps` calls (default 5), the host clock around a synchronised call; median and
range:
  ringmap_beamform  `RingMapBeamForm.process` (pixel search and sort on the host, uploads, `dmm_ringmap_extract`)
  extract_kernel    `dmm_ringmap_extract` alone on the same indices, in pixel order and in catalogue order
  torch_index       `map[0][:, :, ri, ei]` and `weight[:, :, ri, ei]` with the same indices: the baseline of the extract
                    kernel, independent of the code under test (its result is laid out [pol, freq, source])
  source_stack      `SourceStack.process` with `freqside` 20 on the formed beam (host tables and uploads included)
  stack3d           `RingMapStack2D.process` with `num_freq` 20, the other defaults, for the first `--sources3d` sources
  random_subsets    ten `RandomSubset` draws of half the catalogue, each through `SourceStack`
Bytes are those of the traffic models in DESIGN.md 7g: extract 2 datasets x (64 read + 8 written) per element; stack 16
per (source, pol, channel); stack3d 16 per (source, pol, channel in a bin, pixel of the clipped patch).  One JSON line
per case; `--out` also writes them to a file.

    python tools/stack_timing.py [--out profiles/stack_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
NU21 = 1420.40575177
LATITUDE = 49.3


class Telescope:
    latitude = LATITUDE
    lmax = mmax = 1
    frequencies = np.zeros(1)


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pol", type=int, default=4)
    ap.add_argument("--freq", type=int, default=64)
    ap.add_argument("--ra", type=int, default=4096)
    ap.add_argument("--el", type=int, default=1024)
    ap.add_argument("--sources", type=int, default=200000)
    ap.add_argument("--sources3d", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from draco_amd import _lib
    from draco_amd.analysis.beamform import RingMapBeamForm, RingMapStack2D
    from draco_amd.analysis.sourcestack import RandomSubset, SourceStack
    from draco_amd.core import containers
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    npol, nfreq, nra, nel, nsrc = args.pol, args.freq, args.ra, args.el, args.sources
    gen = torch.Generator(device=ctx.device).manual_seed(args.seed)
    rmap = torch.randn((1, npol, nfreq, nra, nel), dtype=torch.float64, device=ctx.device, generator=gen)
    weight = torch.rand((npol, nfreq, nra, nel), dtype=torch.float64, device=ctx.device, generator=gen) + 0.5
    centre = (800.0 - 400.0 / 1024 * np.arange(nfreq)).copy()  # descending, 0.39 MHz channels
    frequency = np.zeros(nfreq, dtype=[("centre", np.float64), ("width", np.float64)])
    frequency["centre"], frequency["width"] = centre, 400.0 / 1024
    el = np.linspace(-0.95, 0.95, nel)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "reXY", "imXY", "YY"][:npol]), freq=frequency, ra=nra, el=el, allocate=False)
    rm.attach("map", rmap)
    rm.attach("weight", weight)

    rng = np.random.default_rng(args.seed)
    cat = containers.SpectroscopicCatalog(object_id=np.arange(nsrc))
    cat["position"]["ra"][:] = rng.uniform(0.0, 360.0, size=nsrc)
    cat["position"]["dec"][:] = LATITUDE + np.degrees(np.arcsin(rng.uniform(el[0], el[-1], size=nsrc)))
    cat["redshift"]["z"][:] = NU21 / rng.uniform(centre.min(), centre.max(), size=nsrc) - 1.0
    cat.attrs["tag"] = "timing"

    lines = []
    shape = {"npol": npol, "nfreq": nfreq, "nra": nra, "nel": nel}

    def emit(case, ms, nbytes=None, **more):
        med = float(np.median(ms))
        rec = dict({"case": case, "ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}, **shape, **more)
        if nbytes is not None:
            rec.update({"model_GB": round(nbytes / 1e9, 3), "TBps": round(nbytes / med / 1e9, 3), "frac_peak": round(nbytes / med * 1e3 / PEAK, 4)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # ---- RingMapBeamForm and its kernel against the torch expression
    bf = RingMapBeamForm()
    bf.setup(Telescope(), rm)
    fb = bf.process(cat)
    n_in = fb.beam.shape[0]
    extract_bytes = 2 * n_in * npol * nfreq * (64 + 8)
    emit("ringmap_beamform", timed(ctx, lambda: bf.process(cat), args.reps), extract_bytes, sources=n_in)
    ra_ind, el_ind, _ = bf._source_ind(cat["position"]["ra"], cat["position"]["dec"])
    order = np.argsort(ra_ind.astype(np.int64) * nel + el_ind, kind="stable").astype(np.int32)
    ri_d, ei_d, or_d = (ctx.to_device(np.ascontiguousarray(x, dtype=np.int32)) for x in (ra_ind, el_ind, order))
    ob, ow = ctx.empty((n_in, npol, nfreq), np.float64), ctx.empty((n_in, npol, nfreq), np.float64)
    m0 = rmap[0]
    for label, od in (("pixel order", or_d), ("catalogue order", None)):
        emit("extract_kernel", timed(ctx, lambda: _lib.check(_lib.lib.dmm_ringmap_extract(ctx.handle, npol, nfreq, nra, nel, ptr(m0), ptr(weight), 0, n_in, ptr(ri_d), ptr(ei_d),
                                                                                            ptr(od), ptr(ob), ptr(ow))), args.reps), extract_bytes, sources=n_in, visit=label)
    ri_t, ei_t = ri_d.long(), ei_d.long()
    emit("torch_index", timed(ctx, lambda: (m0[:, :, ri_t, ei_t], weight[:, :, ri_t, ei_t]), args.reps), extract_bytes, sources=n_in)
    assert torch.equal(m0[:, :, ri_t, ei_t].permute(2, 0, 1), fb.beam._dev)

    # ---- SourceStack
    stk = SourceStack(freqside=20)
    emit("source_stack", timed(ctx, lambda: stk.process(fb), args.reps), 16 * n_in * npol * nfreq, sources=n_in, freqside=20)

    # ---- RingMapStack2D on the first sources of the catalogue
    n3 = min(args.sources3d, nsrc)
    cat3 = containers.SpectroscopicCatalog(object_id=np.arange(n3))
    for name in ("position", "redshift"):
        cat3[name][:] = cat[name][:][:n3]
    cat3.attrs["tag"] = "timing3d"
    s3 = RingMapStack2D(num_freq=20)
    s3.setup(Telescope(), rm)
    ri3, ei3, si3 = bf._source_ind(cat3["position"]["ra"], cat3["position"]["dec"])
    sf3 = NU21 / (1.0 + cat3["redshift"]["z"][si3])
    df = np.median(np.abs(np.diff(centre)))
    edges = (np.arange(-20, 22) - 0.5) * df
    bins = np.digitize(centre[np.newaxis, :] - sf3[:, np.newaxis], edges)
    nchan = ((bins >= 1) & (bins <= 41)).sum(axis=1)
    rows = np.minimum(ei3 + 11, nel) - np.maximum(ei3 - 10, 0)
    emit("stack3d", timed(ctx, lambda: s3.process(cat3), args.reps), 16 * npol * int((nchan * rows * 21).sum()), sources=int(si3.size), num_freq=20, patch="21x21")

    # ---- ten draws of half the catalogue through SourceStack
    sub = RandomSubset(number=10 * (args.reps + 1), size=n_in // 2, seed=args.seed)
    sub.setup(fb)

    def draws():
        for _ in range(10):
            stk.process(sub.process())

    emit("random_subsets", timed(ctx, draws, args.reps), None, draws=10, size=n_in // 2)

    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
