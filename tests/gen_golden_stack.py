"""Generate tests/golden/stack.npz by EXECUTING the reference's own ``SourceStack.process``, ``RandomSubset.process``,
``GroupSourceStacks``, ``RingMapBeamForm.process`` and ``RingMapStack2D.process`` from source (through
``oracle._refstub``, unmodified) on small stand-in containers (NumPy arrays with the attributes the tasks touch) and a
one-rank stand-in communicator (``Allgather`` / ``Allreduce`` / ``Bcast`` copy, ``reduce`` returns its argument).  The
``config.enum`` attribute is set on the instances (the stub returns ``None`` for it) and ``nu21`` carries its public
value.  Only arrays are kept.  Run where the reference checkout exists:

    python tests/gen_golden_stack.py

The file holds the inputs once (one ring map with weights and rms, stored as float32 values; two catalogues, one per RA
axis; one formed beam on an irregular frequency axis), and per case the reference's outputs, the truth
(``tests/stack_twin.py`` in long double, rounded to float64), ``e_ref`` (the reference against the truth), ``e_f64`` (the
float64 twin against the truth) for stack and weight, and ``norm`` (the size of what was summed).  The pencil beams of
``RingMapBeamForm`` are asserted here to be bit-equal to ``stack_twin.extract`` at the reference's own pixel indices;
the file keeps the indices.

Asserted here, so that the reference is well determined on the inputs: no source lies within 1 % of a pixel of the
half-pixel cut in RA or el; no ``freq - source_freq`` lies within 1 % of a channel width of a bin edge of any case,
except the one source placed exactly on a channel centre in the case ``s3_tie``, whose edges are whole multiples of
the channel width (exact in float64); the twin's bin membership equals ``np.digitize``'s in the reference.
"""

import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stack_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NRA, NEL, NFREQ = twin.NRA, twin.NEL, twin.NFREQ
TIE_CENTRE = 612.0


class DS(np.ndarray):
    """A dataset: an array with ``attrs`` and the MPIArray attributes of one rank."""

    attrs = None
    local_offset = property(lambda s: (0,) * s.ndim)
    local_shape = property(lambda s: s.shape)
    local_array = property(lambda s: np.asarray(s))


def dataset(arr, axes):
    d = np.array(arr).view(DS)
    d.attrs = {"axis": list(axes)}
    return d


class Comm:
    rank, size = 0, 1

    def Allgather(self, src, dst):
        dst[...] = np.asarray(src).reshape(dst.shape)

    def Allreduce(self, src, dst, op=None):
        dst[...] = src

    def Bcast(self, buf, root=0):
        pass

    def reduce(self, x, op=None, root=0):
        return x


_POS = [("ra", np.float64), ("dec", np.float64)]
_RED = [("z", np.float64), ("z_error", np.float64)]


class RC:
    """A container: axes, attributes and datasets allocated from ``_spec``."""

    _axes = ()
    _spec = {}
    _optional = {}
    distributed = False

    def __init__(self, axes_from=None, attrs_from=None, comm=None, distributed=None, **axes):
        self.index_map, self.attrs, self.comm = {}, {}, Comm()
        if axes_from is not None:
            for ax in self._axes:
                if ax in axes_from.index_map:
                    self.index_map[ax] = axes_from.index_map[ax]
        for ax, val in axes.items():
            self.index_map[ax] = np.asarray(val)
        if attrs_from is not None:
            self.attrs.update(attrs_from.attrs)
        self.datasets = {}
        for name in self._spec:
            self.add_dataset(name)

    def add_dataset(self, name):
        axes, dtype = {**self._spec, **self._optional}[name]
        self.datasets[name] = dataset(np.zeros(tuple(len(self.index_map[a]) for a in axes), dtype=dtype), axes)

    def __getattr__(self, name):
        if name in ("datasets", "index_map"):
            raise AttributeError(name)
        if name in self.datasets:
            return self.datasets[name]
        raise AttributeError(name)

    freq = property(lambda s: s.index_map["freq"]["centre"])
    frequency = property(lambda s: s.index_map["freq"])
    pol = property(lambda s: s.index_map["pol"])

    def __getitem__(self, k):
        return self.datasets[k]

    def __contains__(self, k):
        return k in self.datasets

    def redistribute(self, axis):
        pass


class RingMap(RC):
    _axes = ("beam", "pol", "freq", "ra", "el")
    _optional = {"map": (["beam", "pol", "freq", "ra", "el"], np.float64), "weight": (["pol", "freq", "ra", "el"], np.float64), "rms": (["pol", "freq", "ra"], np.float64)}


class Catalog(RC):
    _axes = ("object_id",)
    _spec = {"position": (["object_id"], _POS), "redshift": (["object_id"], _RED)}


class FormedBeam(RC):
    _axes = ("object_id", "pol", "freq")
    _spec = {"beam": (["object_id", "pol", "freq"], np.float64), "weight": (["object_id", "pol", "freq"], np.float64), "position": (["object_id"], _POS)}
    _optional = {"redshift": (["object_id"], _RED)}


class FrequencyStack(RC):
    _axes = ("freq",)
    _spec = {"stack": (["freq"], np.float64), "weight": (["freq"], np.float64)}


class FrequencyStackByPol(RC):
    _axes = ("pol", "freq")
    _spec = {"stack": (["pol", "freq"], np.float64), "weight": (["pol", "freq"], np.float64)}


class MockFrequencyStack(RC):
    _axes = ("mock", "freq")
    _spec = {"stack": (["mock", "freq"], np.float64), "weight": (["mock", "freq"], np.float64)}


class MockFrequencyStackByPol(RC):
    _axes = ("mock", "pol", "freq")
    _spec = {"stack": (["mock", "pol", "freq"], np.float64), "weight": (["mock", "pol", "freq"], np.float64)}


class Stack3D(RC):
    _axes = ("pol", "delta_ra", "delta_dec", "freq")
    _spec = {"stack": (["pol", "delta_ra", "delta_dec", "freq"], np.float64), "weight": (["pol", "delta_ra", "delta_dec", "freq"], np.float64)}


CONTAINERS = types.SimpleNamespace(FormedBeam=FormedBeam, FrequencyStack=FrequencyStack, FrequencyStackByPol=FrequencyStackByPol, MockFrequencyStack=MockFrequencyStack,
                                   MockFrequencyStackByPol=MockFrequencyStackByPol, Stack3D=Stack3D)


def all_edges(frequency):
    """Every set of bin edges a case digitizes against on this frequency axis: ``{case: edges}``."""
    out = {}
    for name, (src, cfg) in twin.STACK_CASES.items():
        out[name] = (src, twin.stack_bins(frequency[src], cfg["freqside"])[1])
    for name, (src, cfg) in twin.STACK3D_CASES.items():
        full = {**twin.STACK3D_DEFAULTS, **cfg}
        out[name] = (src, twin.stack3d_edges(frequency[src]["centre"], full["num_freq"], full["freq_width"]))
    return out


def edge_margin(freq, width, sfreq, edges):
    """The least ``|freq - sfreq - edge|`` in channel widths, exact zeros aside; and how many exact zeros there are."""
    d = np.abs((freq[np.newaxis, :] - sfreq[:, np.newaxis])[:, :, np.newaxis] - edges[np.newaxis, np.newaxis, :]) / width[np.newaxis, :, np.newaxis]
    return d[d > 0].min(), int((d == 0).sum())


def exact_z(sf):
    """A redshift whose line frequency ``NU21 / (1 + z)`` is exactly ``sf`` in float64."""
    z = twin.NU21 / sf - 1.0
    for _ in range(64):
        got = twin.NU21 / (1.0 + z)
        if got == sf:
            return z
        z = np.nextafter(z, np.inf if got > sf else -np.inf)
    raise AssertionError("no exact redshift found")


def make_inputs():
    rng = np.random.default_rng(20261)
    rmap = rng.normal(size=(4, NFREQ, NRA, NEL)).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, size=(4, NFREQ, NRA, NEL)).astype(np.float32)
    weight[rng.uniform(size=weight.shape) < 0.05] = 0.0
    rms = rng.uniform(0.5, 2.0, size=(4, NFREQ, NRA)).astype(np.float32)
    rms[rng.uniform(size=rms.shape) < 0.05] = 0.0
    el = np.linspace(-0.6, 0.8, NEL)
    dell = el[1] - el[0]
    # offsets of the line frequencies from a channel centre (MHz): clear of every edge of every case
    bad = np.array([0.0, 1.0 / 3.0, 1.0, 5.0 / 3.0])

    def offsets(n):
        out = []
        while len(out) < n:
            o = rng.uniform(-0.8, 0.8)
            if np.abs(np.abs(o) - bad).min() > 0.05:
                out.append(o)
        return np.array(out)

    cats = {}
    for kind, span in (("closed", 360.0), ("clip", 300.0)):
        ra = np.linspace(0.0, span, NRA, endpoint=False)
        dra = ra[1] - ra[0]
        # pixels: the four corners, the first and last RA and el rows, two sources in one pixel, the rest at random
        pix = [(0, 0), (0, NEL - 1), (NRA - 1, 0), (NRA - 1, NEL - 1), (0, 7), (NRA - 1, 12), (9, 0), (20, NEL - 1), (14, 10), (14, 10), (1, 1), (NRA - 2, NEL - 2)]
        while len(pix) < 40:
            pix.append((int(rng.integers(0, NRA)), int(rng.integers(0, NEL))))
        pix = np.array(pix)
        sra = (ra[pix[:, 0]] + rng.uniform(-0.4, 0.4, size=40) * dra) % 360.0
        sel = el[pix[:, 1]] + rng.uniform(-0.4, 0.4, size=40) * dell
        chan = rng.integers(-2, NFREQ + 2, size=40)
        chan[:12] = [0, NFREQ - 1, 1, NFREQ - 2, 6, 6, 3, 9, 5, 7, -2, NFREQ + 1]  # cut by either band edge, outside the band
        sf = 600.0 + 2.0 * chan + offsets(40)
        z = twin.NU21 / sf - 1.0
        z[6] = exact_z(TIE_CENTRE)  # the tie: exactly on a channel centre
        # six sources outside the map: above and below in el, and (on the clipped axis) past the end of the RA axis
        ora = np.array([10.0, 200.0, 100.0, 335.0 if kind == "clip" else 50.0, 330.0 if kind == "clip" else 250.0, 301.0 if kind == "clip" else 120.0])
        oel = np.array([0.9, -0.75, 0.95, 0.12 if kind == "clip" else 0.9, 0.22 if kind == "clip" else -0.7, 0.31 if kind == "clip" else 0.87])
        order = rng.permutation(46)
        ra_all, el_all = np.concatenate([sra, ora])[order], np.concatenate([sel, oel])[order]
        z_all = np.concatenate([z, twin.NU21 / (606.0 + offsets(6)) - 1.0])[order]
        cats[kind] = {"ra": ra_all, "dec": twin.LATITUDE + np.degrees(np.arcsin(el_all)), "z": z_all, "pix": pix, "order": order}
    # a source whose weights are all zero (closed axis): its pixel in the weights, its RA column in the rms
    weight[:, :, 14, 10] = 0.0
    rms[:, :, 20] = 0.0
    # the formed beam on the irregular axis
    irr = twin.irregular_axis()
    nirr = 30
    irr_sf = np.empty(nirr)
    edges = [twin.stack_bins(irr, cfg["freqside"])[1] for src, cfg in twin.STACK_CASES.values() if src == "irregular"]
    for s in range(nirr):
        while True:
            cand = rng.uniform(irr["centre"].min() - 4.0, irr["centre"].max() + 4.0)
            if all(edge_margin(irr["centre"], irr["width"], np.array([cand]), e)[0] > 0.02 for e in edges):
                irr_sf[s] = cand
                break
    ibeam = rng.normal(size=(nirr, 4, irr.size)).astype(np.float32)
    iweight = rng.uniform(0.5, 2.0, size=ibeam.shape).astype(np.float32)
    iweight[rng.uniform(size=iweight.shape) < 0.1] = 0.0
    iweight[4] = 0.0
    return rmap, weight, rms, cats, {"beam": ibeam, "weight": iweight, "z": twin.NU21 / irr_sf - 1.0, "frequency": irr}


def ring_map(name, rmap, weight, rms):
    npol, frequency, ra, el, has_weight = twin.map_axes(name)
    rm = RingMap(beam=np.arange(1), pol=np.array(["XX", "reXY", "imXY", "YY"][:npol]), freq=frequency, ra=ra, el=el)
    rm.add_dataset("map")
    rm.map[:] = rmap[np.newaxis, :npol]
    if has_weight:
        rm.add_dataset("weight")
        rm.weight[:] = weight[:npol]
    else:
        rm.add_dataset("rms")
        rm.rms[:] = rms[:npol]
    rm.attrs["tag"] = "rm_" + name
    return rm


def catalog(cat, tag):
    c = Catalog(object_id=np.arange(len(cat["ra"])))
    c["position"]["ra"], c["position"]["dec"], c["redshift"]["z"] = cat["ra"], cat["dec"], cat["z"]
    c.attrs["tag"] = tag
    return c


def main():
    _refstub.load_reference()
    import importlib

    tasklib = importlib.import_module("caput.pipeline.tasklib")
    tasklib.random = types.SimpleNamespace(RandomTask=type("RandomTask", (), {}))

    class Stop(Exception):
        pass

    from draco.analysis import beamform as bf
    from draco.analysis import sourcestack as ss

    for mod in (bf, ss):
        mod.invert_no_zero = _refstub._invert_no_zero
        mod.NU21 = twin.NU21
        mod.containers = CONTAINERS
    bf.io = types.SimpleNamespace(get_telescope=lambda m: m)
    ss.exceptions = types.SimpleNamespace(PipelineStopIteration=Stop)
    log = logging.getLogger("gen")
    tel = twin.FakeTelescope()

    rmap, weight, rms, cats, irr = make_inputs()
    out = {"map": rmap, "weight": weight, "rms": rms, "irr/beam": irr["beam"], "irr/weight": irr["weight"], "irr/z": irr["z"]}
    for kind, cat in cats.items():
        for k in ("ra", "dec", "z"):
            out[f"cat_{kind}/{k}"] = cat[k]

    # ---- RingMapBeamForm on every ring map
    beams, frequency = {}, {"irregular": irr["frequency"]}
    for name in twin.MAPS:
        rm = ring_map(name, rmap, weight, rms)
        kind = twin.MAPS[name][2]
        task = bf.RingMapBeamForm()
        task.log = log
        task.setup(tel, rm)
        src_ra, src_dec = task._process_catalog(catalog(cats[kind], "cat_" + kind))
        ra_ind, el_ind, src_ind = task._source_ind(src_ra, src_dec)
        fb = task.process(catalog(cats[kind], "cat_" + kind))
        t_ri, t_ei, t_si, margin = twin.source_ind(rm.index_map["ra"], rm.index_map["el"], cats[kind]["ra"], cats[kind]["dec"])
        assert margin > 0.01, margin
        assert np.array_equal(ra_ind, t_ri) and np.array_equal(el_ind, t_ei) and np.array_equal(src_ind, t_si)
        assert src_ind.size == 40 and np.array_equal(np.sort(cats[kind]["order"].argsort()[:40]), src_ind)
        pix = cats[kind]["pix"][cats[kind]["order"][src_ind]]
        assert np.array_equal(pix[:, 0], ra_ind) and np.array_equal(pix[:, 1], el_ind)
        has_weight = twin.MAPS[name][3] == "weight"
        tb, tw = twin.extract(np.asarray(rm.map[0]), np.asarray(rm.weight if has_weight else rm.rms), not has_weight, ra_ind, el_ind)
        assert np.array_equal(np.asarray(fb.beam), tb) and np.array_equal(np.asarray(fb.weight), tw)
        assert np.array_equal(fb.index_map["object_id"], src_ind) and fb.attrs["tag"] == "cat_" + kind
        assert np.array_equal(np.asarray(fb["position"]["ra"]), cats[kind]["ra"][src_ind]) and np.array_equal(np.asarray(fb["redshift"]["z"]), cats[kind]["z"][src_ind])
        out[f"bf/{name}/ra_ind"], out[f"bf/{name}/el_ind"], out[f"bf/{name}/src_ind"] = ra_ind.astype(np.int32), el_ind.astype(np.int32), src_ind.astype(np.int32)
        beams[name], frequency[name] = fb, rm.index_map["freq"]
        print(f"{name:14s} {src_ind.size} of {len(cats[kind]['ra'])} sources inside, margin {margin:.3f} pixel, zero-weight rows {int((tw.sum(axis=(1, 2)) == 0).sum())}")
    fbi = FormedBeam(object_id=np.arange(len(irr["z"])), pol=np.array(["XX", "reXY", "imXY", "YY"]), freq=irr["frequency"])
    fbi.beam[:], fbi.weight[:] = irr["beam"], irr["weight"]
    fbi.add_dataset("redshift")
    fbi["redshift"]["z"] = irr["z"]
    fbi.attrs["tag"] = "irr"
    beams["irregular"] = fbi

    # ---- every frequency offset is clear of every edge
    for case, (src, edges) in all_edges(frequency).items():
        fm = frequency[src]
        sfreq = twin.NU21 / (1.0 + np.asarray(beams[src]["redshift"]["z"]))
        margin, ties = edge_margin(fm["centre"], fm["width"], sfreq, edges)
        assert margin > 0.01, (case, margin)
        assert ties == (4 if case == "s3_tie" else 0), (case, ties)

    # ---- SourceStack
    for name, (src, cfg) in twin.STACK_CASES.items():
        full = {**twin.STACK_DEFAULTS, **cfg}
        task = ss.SourceStack()
        task.log = log
        for k, v in full.items():
            setattr(task, k, v)
        fb = beams[src]
        res = task.process(fb)
        assert type(res) is (FrequencyStackByPol if len(fb.pol) > 1 else FrequencyStack)
        args = (np.asarray(fb.beam), np.asarray(fb.weight), fb.frequency, np.asarray(fb["redshift"]["z"]))
        truth = twin.source_stack(*args, **full, dtype=np.longdouble)
        f64 = twin.source_stack(*args, **full, dtype=np.float64)
        # the reference's own membership expression
        ref_idx = np.digitize(fb.freq[np.newaxis, :] - (twin.NU21 / (args[3] + 1.0))[:, np.newaxis], twin.stack_bins(fb.frequency, full["freqside"])[1]) - 1
        live = truth["index"] >= 0
        assert np.array_equal(ref_idx[live], truth["index"][live])
        assert np.array_equal(np.asarray(res.index_map["freq"]["centre"]), truth["axis"]["centre"])
        rs, rw = np.asarray(res.stack).reshape(truth["stack"].shape), np.asarray(res.weight).reshape(truth["stack"].shape)
        rec = record(rs, rw, truth, f64)
        rec["index"] = truth["index"].astype(np.int8)
        rec["axis_centre"], rec["axis_width"] = truth["axis"]["centre"], truth["axis"]["width"]
        report(name, rec, f"stacked {int((truth['index'] >= 0).any(axis=1).sum())} of {len(args[3])}")
        for k, v in rec.items():
            out[f"ss/{name}/{k}"] = v

    # ---- RingMapStack2D
    for name, (src, cfg) in twin.STACK3D_CASES.items():
        full = {**twin.STACK3D_DEFAULTS, **cfg}
        rm = ring_map(src, rmap, weight, rms)
        kind = twin.MAPS[src][2]
        task = bf.RingMapStack2D()
        task.log, task.comm = log, Comm()
        for k, v in full.items():
            setattr(task, k, v)
        task.setup(tel, rm)
        res = task.process(catalog(cats[kind], "cat_" + kind))
        assert res.attrs["tag"] == "cat_" + kind
        has_weight = twin.MAPS[src][3] == "weight"
        ri, ei, si = (out[f"bf/{src}/{k}"] for k in ("ra_ind", "el_ind", "src_ind"))
        args = (np.asarray(rm.map[0]), np.asarray(rm.weight if has_weight else rm.rms), not has_weight, rm.freq, rm.index_map["ra"], rm.index_map["el"], ri, ei, cats[kind]["z"][si])
        truth = twin.stack3d(*args, **full, dtype=np.longdouble)
        f64 = twin.stack3d(*args, **full, dtype=np.float64)
        rec = record(np.asarray(res.stack), np.asarray(res.weight), truth, f64)
        rec["delta_ra"], rec["delta_dec"] = res.index_map["delta_ra"], res.index_map["delta_dec"]
        rec["freq_centre"], rec["freq_width"] = res.index_map["freq"]["centre"], res.index_map["freq"]["width"]
        report(name, rec, f"empty bins {int((truth['weight'].sum(axis=(0, 1, 2)) == 0).sum())} of {truth['weight'].shape[-1]}")
        for k, v in rec.items():
            out[f"s3/{name}/{k}"] = v

    # ---- the chain: RandomSubset (3 draws of 20 out of 40) -> SourceStack -> GroupSourceStacks(ngroup=2)
    sub = ss.RandomSubset()
    sub.log, sub.comm, sub.rng = log, Comm(), np.random.default_rng(7)
    sub.number, sub.size = 3, 20
    sub.setup(beams["closed_w"])
    stk = ss.SourceStack()
    stk.log = log
    stk.freqside, stk.single_source_bin_index, stk.uniform_weight = 2, None, False
    grp = ss.GroupSourceStacks()
    grp.log, grp.ngroup = log, 2
    grp.setup()
    draws, groups = [], []
    while True:
        try:
            mock = sub.process()
        except Stop:
            break
        draws.append(np.asarray(mock.index_map["object_id"]))
        g = grp.process(stk.process(mock))
        if g is not None:
            groups.append(g)
    groups.append(grp.process_finish())
    assert len(draws) == 3 and len(groups) == 2 and grp.process_finish() is None
    # (the draws are positions in the formed beam's object axis: recover them from the object ids)
    ids = np.asarray(beams["closed_w"].index_map["object_id"])
    out["chain/indices"] = np.array([np.searchsorted(ids, d) for d in draws]).astype(np.int32)
    check = np.random.default_rng(7)
    for d in out["chain/indices"]:
        assert np.array_equal(d, np.sort(check.choice(40, 20, replace=False)))
    for i, g in enumerate(groups):
        assert type(g) is MockFrequencyStackByPol
        out[f"chain/group{i}_stack"], out[f"chain/group{i}_weight"], out[f"chain/group{i}_tag"] = np.asarray(g.stack), np.asarray(g.weight), np.array(g.attrs["tag"])
        print("chain group", i, g.attrs["tag"], np.asarray(g.stack).shape)

    path = os.path.join(GOLDEN, "stack.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def record(ref_stack, ref_weight, truth, f64):
    norm = truth["norm"]
    return {
        "ref_stack": ref_stack, "ref_weight": ref_weight, "truth_stack": truth["stack"].astype(np.float64), "truth_weight": truth["weight"].astype(np.float64), "norm": np.float64(norm),
        "e_ref": np.float64(twin.stack_error(ref_stack, truth["stack"], norm)), "e_f64": np.float64(twin.stack_error(f64["stack"], truth["stack"], norm)),
        "e_ref_w": np.float64(twin.weight_error(ref_weight, truth["weight"])), "e_f64_w": np.float64(twin.weight_error(f64["weight"], truth["weight"])),
    }


def report(name, rec, extra):
    assert np.array_equal(rec["ref_weight"] == 0, rec["truth_weight"] == 0), name
    print(f"{name:22s} e_ref {rec['e_ref']:.2e} weight {rec['e_ref_w']:.2e}   e_f64 {rec['e_f64']:.2e} weight {rec['e_f64_w']:.2e}   norm {rec['norm']:.3g}   {extra}")


if __name__ == "__main__":
    main()
