"""Time source beamforming: `BeamFormCat.process` on a synthetic CHIME-like dataset sized to one rank.

    python tools/srcbeam_bench.py [--sources 2000] [--freq 64] [--ra 4096] [--stacks 1700] [--reps 5] [--out FILE]

The dataset: `--freq` local frequencies (400 ... 425 MHz), `--ra` right ascensions, about `--stacks` stacked baselines
for each of XX and YY (4 cylinders 22 m apart, feeds 0.3048 m apart; every stack is one product, so the natural weight
is the mask of the visibility weight), 2 % of the weights zero.  The catalogue is uniform in right ascension and in
declination between 0 and 80 degrees; `timetrack=900`, `polarization="copol"`, natural weighting, an analytic
primary beam evaluated on the host.  After one warm-up `process` (code objects, allocator) the same call is timed
`--reps` times with a host clock around work that ends in a device synchronise; inside, the calls of
`_fast_tools.form` (the inversion of the windows on the host, five small uploads, the kernel, a synchronise: not kernel
time from a trace) and the host-side beam tables are timed the same way.  Reported: the median and the range over the
repetitions of the whole call, of the form calls and of the beam tables, sources per second (whole call), terms per
second of the form calls (a term is one (source, polarisation, frequency, hour-angle sample, baseline)), and the bytes
the form kernel reads from the data per term, computed from the shapes: every (frequency, sample) row that some source of a chunk looks
at is read once per chunk and polarisation, 12 bytes per stack (complex64 visibility, float32 weight).
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Pairs:
    """`feedmap[i, j]` / `feedconj[i, j]` of a telescope whose only products are (reference feed, feed k)."""

    def __init__(self, fn):
        self.fn = fn

    def __getitem__(self, ij):
        import numpy as np

        return self.fn(np.asarray(ij[0]), np.asarray(ij[1]))


class BenchTelescope:
    stack_type = "redundant"
    lmax = mmax = 0
    latitude = 49.3

    def __init__(self, frequencies, ns):
        import numpy as np

        self.frequencies = np.asarray(frequencies, dtype=np.float64)
        self.ns = ns
        k = np.arange(ns)
        # baselines of one polarisation: east 0 / 22 / 44 / 66 m, north -n ... n feed spacings
        per = (ns + 3) // 4
        self.baselines = np.stack([22.0 * (k // per), 0.3048 * ((k % per) - per // 2 + 0.5)], axis=1)
        n = ns + 1
        self.polarisation = np.array(["X"] * n + ["Y"] * n)
        self.beamclass = np.array([0] * n + [1] * n)
        self.feedmap = _Pairs(lambda i, j: (j - i - 1) % ns)
        self.feedconj = _Pairs(lambda i, j: (i != i))

    def lsd_to_unix(self, lsd):
        return 86164.0905 * lsd

    def beam(self, feed, freq, angpos):
        import numpy as np

        phi = angpos[:, 1]
        sig = (0.035 if feed else 0.03) * 600.0 / self.frequencies[freq]
        g = np.exp(-0.5 * (phi / sig) ** 2) * np.sin(angpos[:, 0])
        return np.stack([g * np.exp(0.2j * phi / sig), 0.05 * g * phi / sig], axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sources", type=int, default=2000)
    ap.add_argument("--freq", type=int, default=64)
    ap.add_argument("--ra", type=int, default=4096)
    ap.add_argument("--stacks", type=int, default=1700)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from draco_amd.analysis.beamform import BeamFormCat
    from draco_amd.core import containers
    from draco_amd.device import Context
    from draco_amd.util import _fast_tools

    ctx = Context.get()
    nf, nra, ns = args.freq, args.ra, args.stacks
    freq = 400.0 + 0.390625 * np.arange(nf)
    tel = BenchTelescope(freq, ns)
    n = ns + 1
    prod = np.array([(0, k) for k in range(1, n)] + [(n, n + k) for k in range(1, n)], dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    stack = np.zeros(2 * ns, dtype=[("prod", "<u4"), ("conjugate", "u1")])
    stack["prod"] = np.arange(2 * ns)
    rev = np.zeros(2 * ns, dtype=[("stack", "<u4"), ("conjugate", "u1")])
    rev["stack"] = np.arange(2 * ns)
    ss = containers.SiderealStream(freq=freq, ra=nra, stack=stack, prod=prod, input=np.arange(2 * n), reverse_map_stack=rev, allocate=False)
    ss.attrs["lsd"] = 1
    gen = torch.Generator(device=ctx.device).manual_seed(11)
    vis = torch.view_as_complex(torch.randn((nf, 2 * ns, nra, 2), device=ctx.device, dtype=torch.float32, generator=gen))
    weight = torch.rand((nf, 2 * ns, nra), device=ctx.device, dtype=torch.float32, generator=gen) + 0.5
    weight[torch.rand((nf, 2 * ns, nra), device=ctx.device, generator=gen) < 0.02] = 0.0
    ss.attach("vis", vis)
    ss.attach("vis_weight", weight)
    ss.add_dataset("input_flags")
    ss.input_flags[:] = 1.0
    rng = np.random.default_rng(5)
    cat = containers.SourceCatalog(object_id=np.arange(args.sources))
    cat["position"]["ra"][:] = rng.uniform(0.0, 360.0, size=args.sources)
    cat["position"]["dec"][:] = rng.uniform(0.0, 80.0, size=args.sources)
    cat.attrs["coordinates"] = "CIRS"

    task = BeamFormCat(timetrack=900.0, polarization="copol", weight="natural")
    t0 = time.perf_counter()
    task.setup(tel, ss)
    ctx.sync()
    setup_s = time.perf_counter() - t0
    del vis, weight

    # timers around the two stages (both end in a device synchronise or are pure host work)
    clock = {"form": 0.0, "tables": 0.0, "rows": 0}
    form0, table0 = _fast_tools.form, task._beam_table

    def form(ctx_, visT, ws, u, v, ut, vt, ra_index, *a, **k):
        t = time.perf_counter()
        out = form0(ctx_, visT, ws, u, v, ut, vt, ra_index, *a, **k)
        ctx_.sync()
        clock["form"] += time.perf_counter() - t
        clock["rows"] += int(np.unique(ra_index[ra_index >= 0]).size)
        return out

    def beam_table(dec, ha):
        t = time.perf_counter()
        out = table0(dec, ha)
        clock["tables"] += time.perf_counter() - t
        return out

    _fast_tools.form, task._beam_table = form, beam_table
    out = task.process(cat)  # warm-up
    ctx.sync()
    assert bool(torch.isfinite(out.beam.device(ctx)).all())
    nha = task.nha
    terms = float(args.sources) * task.npol * nf * nha * ns
    runs = []
    for _ in range(args.reps):
        clock.update(form=0.0, tables=0.0, rows=0)
        t0 = time.perf_counter()
        task.process(cat)
        ctx.sync()
        runs.append({"process_s": time.perf_counter() - t0, "form_s": clock["form"], "tables_s": clock["tables"], "rows": clock["rows"]})

    def stat(key):
        x = sorted(r[key] for r in runs)
        return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]}

    res = {
        "sources": args.sources, "nfreq": nf, "nra": nra, "stacks_per_pol": ns, "npol": task.npol, "nha": nha, "reps": args.reps, "setup_s": setup_s, "terms": terms,
        "process_s": stat("process_s"), "form_s": stat("form_s"), "tables_s": stat("tables_s"),
    }
    res["sources_per_s"] = args.sources / res["process_s"]["median"]
    res["terms_per_s_form_calls"] = terms / res["form_s"]["median"]
    res["terms_per_s_form_calls_range"] = [terms / res["form_s"]["max"], terms / res["form_s"]["min"]]
    res["bytes_read_per_term"] = 12.0 * runs[0]["rows"] * nf * ns / terms
    print("SRCBEAM_BENCH " + json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
