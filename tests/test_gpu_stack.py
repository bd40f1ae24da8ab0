"""Source stacking on the GPU: ``RingMapBeamForm``, ``SourceStack`` and ``RingMapStack2D`` on the cases of
``tests/golden/stack.npz`` against the long-double truth and the reference's vectors, kernel-edge shapes generated here
from a seed against the long-double twin, bit-for-bit repeatability, and the chain ``RandomSubset -> SourceStack ->
GroupSourceStacks``.

Bounds.  ``RingMapBeamForm`` is a copy: bit-equal.  Stacks and their weights: ``e_gpu <= max(32 e_f64, floor)`` against
the truth -- ``e_f64`` is the float64 twin's error, 32 the factor the other tests of this tree allow another summation
order, ``floor = 8 * 2^-53`` (there is no phase here: ``P_max = 1``) -- and ``<= 3 e_ref + floor`` against the reference's
vectors.  The stack error is measured against the size of what was summed (``tests/stack_twin.py``)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stack_twin as twin  # noqa: E402

pytestmark = pytest.mark.gpu
POL = np.array(["XX", "reXY", "imXY", "YY"])


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "stack.npz")) as z:
        return {k: z[k] for k in z.files}


def to_ring_map(rmap, wsrc, rms, frequency, ra, el, device=True):
    from draco_amd.core import containers
    from draco_amd.device import Context

    rm = containers.RingMap(beam=1, pol=POL[: rmap.shape[0]], freq=frequency, ra=ra, el=el, allocate=False)
    if rms:
        rm.add_dataset("rms")
    if device:
        ctx = Context.get()
        rm.attach("map", ctx.to_device(np.ascontiguousarray(rmap[np.newaxis])))
        rm.attach("rms" if rms else "weight", ctx.to_device(np.ascontiguousarray(wsrc)))
    else:
        rm.datasets["map"] = containers.Dataset(host=np.ascontiguousarray(rmap[np.newaxis]))
        rm.datasets["rms" if rms else "weight"] = containers.Dataset(host=np.ascontiguousarray(wsrc))
    return rm


def to_catalog(ra, dec, z, tag):
    from draco_amd.core import containers

    cat = containers.SpectroscopicCatalog(object_id=np.arange(len(ra)))
    cat["position"]["ra"][:], cat["position"]["dec"][:], cat["redshift"]["z"][:] = ra, dec, z
    cat.attrs["tag"] = tag
    return cat


def golden_map(gold, name, device=True):
    npol, frequency, ra, el, has_weight = twin.map_axes(name)
    rmap = gold["map"][:npol].astype(np.float64)
    wsrc = (gold["weight"] if has_weight else gold["rms"])[:npol].astype(np.float64)
    kind = twin.MAPS[name][2]
    cat = {k: gold[f"cat_{kind}/{k}"] for k in ("ra", "dec", "z")}
    return rmap, wsrc, not has_weight, to_ring_map(rmap, wsrc, not has_weight, frequency, ra, el, device), cat, "cat_" + kind


def beamform_golden(gold, name, device=True):
    from draco_amd.analysis.beamform import RingMapBeamForm

    rmap, wsrc, rms, rm, cat, tag = golden_map(gold, name, device)
    task = RingMapBeamForm()
    task.setup(twin.FakeTelescope(), rm)
    return task, task.process(to_catalog(cat["ra"], cat["dec"], cat["z"], tag)), (rmap, wsrc, rms, cat)


def to_formed_beam(beam, weight, frequency, z, tag="fb"):
    from draco_amd.core import containers
    from draco_amd.device import Context

    ctx = Context.get()
    fb = containers.FormedBeam(object_id=np.arange(beam.shape[0]), pol=POL[: beam.shape[1]], freq=frequency, allocate=False)
    fb.attach("beam", ctx.to_device(np.ascontiguousarray(beam, dtype=np.float64)))
    fb.attach("weight", ctx.to_device(np.ascontiguousarray(weight, dtype=np.float64)))
    fb.add_dataset("redshift")
    fb["redshift"]["z"][:] = z
    fb.attrs["tag"] = tag
    return fb


def check(label, got, got_w, truth, truth_w, norm, e_f64, e_f64_w, ref=None):
    e, ew = twin.stack_error(got, truth, norm), twin.weight_error(got_w, truth_w)
    print(f"{label}: stack e_gpu {e:.2e} (e_f64 {e_f64:.2e}) weight e_gpu {ew:.2e} (e_f64 {e_f64_w:.2e}) floor {twin.FLOOR:.2e}")
    if ref is not None:
        ref_s, ref_w, e_ref, e_ref_w = ref
        r, rw = twin.stack_error(got, ref_s, norm), twin.weight_error(got_w, ref_w)
        print(f"{label}: against the reference stack {r:.2e} (e_ref {e_ref:.2e}) weight {rw:.2e} (e_ref {e_ref_w:.2e})")
        assert np.array_equal(got_w == 0, ref_w == 0), "zero patterns of the weight differ from the reference's"
    assert np.array_equal(got_w == 0, truth_w == 0), "zero patterns of the weight differ"
    assert e <= max(32 * e_f64, twin.FLOOR)
    assert ew <= max(32 * e_f64_w, twin.FLOOR)
    if ref is not None:
        assert r <= 3 * e_ref + twin.FLOOR
        assert rw <= 3 * e_ref_w + twin.FLOOR


# ---- golden cases
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("name", list(twin.MAPS))
def test_ringmap_beamform(gold, name, device):
    """Bit-equal to the reference (whose beams the generator asserted equal to ``extract`` at its own indices)."""
    task, fb, (rmap, wsrc, rms, cat) = beamform_golden(gold, name, device)
    ri, ei, si = (gold[f"bf/{name}/{k}"] for k in ("ra_ind", "el_ind", "src_ind"))
    for ds in (fb.beam, fb.weight):
        assert ds.on_device and ds._dev.is_cuda and ds._dev.dtype == torch.float64
    beam, weight = twin.extract(rmap, wsrc, rms, ri, ei)
    assert np.array_equal(fb.beam[:], beam) and np.array_equal(fb.weight[:], weight)
    assert np.array_equal(fb.index_map["object_id"], si)
    assert np.array_equal(fb.position["ra"], cat["ra"][si]) and np.array_equal(fb.position["dec"], cat["dec"][si])
    assert np.array_equal(fb.redshift["z"], cat["z"][si]) and fb.attrs["tag"] == "cat_" + twin.MAPS[name][2]
    assert list(fb.pol) == list(POL[: rmap.shape[0]]) and np.array_equal(fb.freq, twin.map_axes(name)[1]["centre"])
    assert (weight.sum(axis=(1, 2)) == 0).sum() == 2  # the sources whose weights are all zero


def test_no_source_inside(gold):
    from draco_amd.analysis.beamform import RingMapBeamForm

    rmap, wsrc, rms, rm, cat, tag = golden_map(gold, "closed_w")
    task = RingMapBeamForm()
    task.setup(twin.FakeTelescope(), rm)
    fb = task.process(to_catalog(np.array([10.0, 200.0]), twin.LATITUDE + np.degrees(np.arcsin(np.array([0.9, -0.75]))), np.array([1.3, 1.3]), "out"))
    assert fb.beam.shape == (0, 4, twin.NFREQ) and fb.weight.shape == (0, 4, twin.NFREQ) and fb.index_map["object_id"].size == 0
    assert fb.beam.on_device and fb.position.shape == (0,)


def stack_input(gold, src):
    if src == "irregular":
        beam, weight, frequency, z = gold["irr/beam"].astype(np.float64), gold["irr/weight"].astype(np.float64), twin.irregular_axis(), gold["irr/z"]
        return to_formed_beam(beam, weight, frequency, z), (beam, weight, frequency, z)
    _, fb, (rmap, wsrc, rms, cat) = beamform_golden(gold, src)
    return fb, (fb.beam[:], fb.weight[:], fb.index_map["freq"], fb.redshift["z"])


@pytest.mark.parametrize("name", list(twin.STACK_CASES))
def test_source_stack(gold, name):
    from draco_amd.analysis.sourcestack import SourceStack
    from draco_amd.core import containers

    src, cfg = twin.STACK_CASES[name]
    fb, args = stack_input(gold, src)
    res = SourceStack(**cfg).process(fb)
    npol = args[0].shape[1]
    assert type(res) is (containers.FrequencyStackByPol if npol > 1 else containers.FrequencyStack)
    g = lambda k: gold[f"ss/{name}/{k}"]  # noqa: E731
    assert np.array_equal(res.index_map["freq"]["centre"], g("axis_centre")) and np.array_equal(res.index_map["freq"]["width"], g("axis_width"))
    got, got_w = res.stack[:].reshape(g("ref_stack").shape), res.weight[:].reshape(g("ref_stack").shape)
    check(name, got, got_w, g("truth_stack"), g("truth_weight"), float(g("norm")), float(g("e_f64")), float(g("e_f64_w")),
          (g("ref_stack"), g("ref_weight"), float(g("e_ref")), float(g("e_ref_w"))))
    if cfg.get("uniform_weight"):
        assert np.array_equal(got_w, g("ref_weight"))  # a count: exact
    assert res.attrs["tag"] == fb.attrs["tag"]
    # membership: with unit beams and weights the weight of a bin counts its (source, channel) pairs
    ones = to_formed_beam(np.ones_like(args[0]), np.ones_like(args[1]), args[2], args[3])
    count = SourceStack(**cfg).process(ones).weight[:].reshape(npol, -1)
    want = np.array([(g("index") == k).sum() for k in range(count.shape[1])], dtype=np.float64)
    assert np.array_equal(count, np.tile(want, (npol, 1)))


@pytest.mark.parametrize("name", list(twin.STACK3D_CASES))
def test_stack3d(gold, name):
    from draco_amd.analysis.beamform import RingMapStack2D
    from draco_amd.core import containers

    src, cfg = twin.STACK3D_CASES[name]
    rmap, wsrc, rms, rm, cat, tag = golden_map(gold, src)
    task = RingMapStack2D(**cfg)
    task.setup(twin.FakeTelescope(), rm)
    res = task.process(to_catalog(cat["ra"], cat["dec"], cat["z"], tag))
    assert type(res) is containers.Stack3D and res.stack.on_device and res.attrs["tag"] == tag
    g = lambda k: gold[f"s3/{name}/{k}"]  # noqa: E731
    assert res.stack.shape == g("ref_stack").shape
    assert np.array_equal(res.index_map["delta_ra"], g("delta_ra")) and np.array_equal(res.index_map["delta_dec"], g("delta_dec"))
    assert np.array_equal(res.index_map["freq"]["centre"], g("freq_centre")) and np.array_equal(res.index_map["freq"]["width"], g("freq_width"))
    check(name, res.stack[:], res.weight[:], g("truth_stack"), g("truth_weight"), float(g("norm")), float(g("e_f64")), float(g("e_f64_w")),
          (g("ref_stack"), g("ref_weight"), float(g("e_ref")), float(g("e_ref_w"))))


# ---- kernel-edge shapes
@pytest.mark.parametrize("npol", [1, 4])
@pytest.mark.parametrize("nfreq", [1, 3, 33])
@pytest.mark.parametrize("nsrc", [1, 63, 65, 1030])
def test_extract_edges(nsrc, nfreq, npol):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    rng = np.random.default_rng(100000 * nsrc + 10 * nfreq + npol)
    nra, nel = 17, 9
    ctx = Context.get()
    for rms in (False, True):
        rmap = rng.normal(size=(npol, nfreq, nra, nel))
        wsrc = rng.uniform(0.5, 2.0, size=(npol, nfreq, nra) + (() if rms else (nel,)))
        wsrc[rng.uniform(size=wsrc.shape) < 0.1] = 0.0
        ri, ei = rng.integers(0, nra, size=nsrc).astype(np.int32), rng.integers(0, nel, size=nsrc).astype(np.int32)
        ri[:4], ei[:4] = [0, 0, nra - 1, nra - 1][:nsrc], [0, nel - 1, 0, nel - 1][:nsrc]  # the corners of the map
        order = np.argsort(ri.astype(np.int64) * nel + ei, kind="stable").astype(np.int32)
        beam, weight = ctx.empty((nsrc, npol, nfreq), np.float64), ctx.empty((nsrc, npol, nfreq), np.float64)
        dev = [ctx.to_device(x) for x in (rmap, wsrc, ri, ei, order)]
        for od in (dev[4], None):  # in pixel order and in catalogue order
            beam.fill_(np.nan)
            _lib.check(_lib.lib.dmm_ringmap_extract(ctx.handle, npol, nfreq, nra, nel, ptr(dev[0]), ptr(dev[1]), int(rms), nsrc, ptr(dev[2]), ptr(dev[3]), ptr(od), ptr(beam), ptr(weight)))
            tb, tw = twin.extract(rmap, wsrc, rms, ri, ei)
            assert np.array_equal(beam.cpu().numpy(), tb) and np.array_equal(weight.cpu().numpy(), tw)


@pytest.mark.parametrize("nstack,nfreq", [(1, 1), (1, 7), (3, 7), (1, 128), (3, 128), (101, 128)])
@pytest.mark.parametrize("nsrc", [1, 63, 65, 1030, 5000])
def test_stack_edges(nsrc, nstack, nfreq):
    from draco_amd.analysis.sourcestack import SourceStack

    npol = 4 if nsrc % 2 else 1
    cfg = dict(freqside=(nstack - 1) // 2, uniform_weight=nsrc == 63)
    beam, weight, frequency, z = twin.random_formed_beam(1000 * nsrc + 10 * nstack + nfreq, nsrc, npol, nfreq, descending=nsrc != 65)
    fb = to_formed_beam(beam, weight, frequency, z)
    res = SourceStack(**cfg).process(fb)
    truth = twin.source_stack(beam, weight, frequency, z, **cfg, dtype=np.longdouble)
    f64 = twin.source_stack(beam, weight, frequency, z, **cfg, dtype=np.float64)
    norm = truth["norm"]
    check(f"stack nsrc {nsrc} nstack {nstack} nfreq {nfreq}", res.stack[:].reshape(npol, nstack), res.weight[:].reshape(npol, nstack), truth["stack"], truth["weight"], norm,
          twin.stack_error(f64["stack"], truth["stack"], norm), twin.weight_error(f64["weight"], truth["weight"]))
    # a second run, and one chunk of partial sums per pass, give the same bits
    for other in (SourceStack(**cfg).process(fb), SourceStack(**cfg, workspace_mib=0).process(fb)):
        assert np.array_equal(other.stack[:], res.stack[:]) and np.array_equal(other.weight[:], res.weight[:])


@pytest.mark.parametrize("nsrc", [1, 2, 130])
@pytest.mark.parametrize("num_freq", [0, 1, 32])
@pytest.mark.parametrize("num_ra,num_dec", [(0, 0), (1, 2), (10, 10)])
def test_stack3d_edges(num_ra, num_dec, num_freq, nsrc):
    from draco_amd.analysis.beamform import RingMapStack2D

    seed = 10000 * nsrc + 100 * num_freq + 10 * num_ra + num_dec
    mode = ("input", "dec", "patch")[seed % 3]
    rms = bool((nsrc + num_freq) % 2)
    npol, nfreq, nra, nel = 2, 2 * num_freq + 5, 24, 22
    rmap, wsrc, frequency, ra, el = twin.random_ring_map(seed, npol, nfreq, nra, nel, rms=rms)
    rng = np.random.default_rng(seed + 1)
    ri, ei = rng.integers(0, nra, size=nsrc), rng.integers(0, nel, size=nsrc)
    ri[:4], ei[:4] = [0, nra - 1, 0, nra - 1][:nsrc], [0, nel - 1, nel - 1, 0][:nsrc]  # the corners of the map
    sra = ra[ri] + rng.uniform(-0.4, 0.4, size=nsrc) * (ra[1] - ra[0])
    sdec = twin.LATITUDE + np.degrees(np.arcsin(el[ei] + rng.uniform(-0.4, 0.4, size=nsrc) * (el[1] - el[0])))
    chan = rng.integers(-1, nfreq + 1, size=nsrc)
    chan[:4] = np.clip(chan[:4], 1, nfreq - 2)  # the corner sources lie inside the band
    sf = frequency["centre"].min() + 0.5 * (chan + rng.uniform(-0.4, 0.4, size=nsrc))
    z = twin.NU21 / sf - 1.0
    cfg = dict(num_ra=num_ra, num_dec=num_dec, num_freq=num_freq, weight=mode)
    task = RingMapStack2D(**cfg)
    task.setup(twin.FakeTelescope(), to_ring_map(rmap, wsrc, rms, frequency, ra, el))
    cat = to_catalog(sra % 360.0, sdec, z, "edges")
    res = task.process(cat)
    t_ri, t_ei, t_si, _ = twin.source_ind(ra, el, sra % 360.0, sdec)
    assert np.array_equal(t_ri, ri) and np.array_equal(t_ei, ei) and t_si.size == nsrc
    args = (rmap, wsrc, rms, frequency["centre"], ra, el, ri, ei, z)
    truth = twin.stack3d(*args, **cfg, dtype=np.longdouble)
    f64 = twin.stack3d(*args, **cfg, dtype=np.float64)
    norm = truth["norm"]
    check(f"stack3d {2 * num_ra + 1}x{2 * num_dec + 1} bins {2 * num_freq + 1} nsrc {nsrc} {mode}{' rms' if rms else ''}", res.stack[:], res.weight[:], truth["stack"], truth["weight"],
          norm, twin.stack_error(f64["stack"], truth["stack"], norm), twin.weight_error(f64["weight"], truth["weight"]))
    again = task.process(cat)  # twice on one setup
    assert np.array_equal(again.stack[:], res.stack[:]) and np.array_equal(again.weight[:], res.weight[:])


def test_stack3d_bits():
    """More than one chunk of sources: two runs, two workspaces and two fresh tasks give the same bits."""
    from draco_amd.analysis.beamform import RingMapStack2D

    nsrc, npol, nfreq, nra, nel = 700, 2, 9, 24, 22
    rmap, wsrc, frequency, ra, el = twin.random_ring_map(77, npol, nfreq, nra, nel)
    rng = np.random.default_rng(78)
    sra = rng.uniform(0.0, 360.0, size=nsrc)
    sdec = twin.LATITUDE + np.degrees(np.arcsin(rng.uniform(-0.9, 0.9, size=nsrc)))
    z = twin.NU21 / rng.uniform(frequency["centre"].min(), frequency["centre"].max(), size=nsrc) - 1.0
    cat = to_catalog(sra, sdec, z, "bits")
    outs = []
    for ws in (1024, 1024, 0):
        task = RingMapStack2D(num_ra=2, num_dec=3, num_freq=2, weight="patch", workspace_mib=ws)
        task.setup(twin.FakeTelescope(), to_ring_map(rmap, wsrc, False, frequency, ra, el))
        outs.append(task.process(cat))
        outs.append(task.process(cat))
    assert outs[0].weight[:].any()
    for o in outs[1:]:
        assert np.array_equal(o.stack[:], outs[0].stack[:]) and np.array_equal(o.weight[:], outs[0].weight[:])


def test_beamform_twice(gold):
    task, fb, _ = beamform_golden(gold, "clip_rms")
    _, fresh, (rmap, wsrc, rms, cat) = beamform_golden(gold, "clip_rms")
    again = task.process(to_catalog(cat["ra"], cat["dec"], cat["z"], "cat_clip"))
    for a in (again, fresh):
        assert np.array_equal(a.beam[:], fb.beam[:]) and np.array_equal(a.weight[:], fb.weight[:])


# ---- the chain
def test_chain(gold):
    from draco_amd.analysis.sourcestack import GroupSourceStacks, RandomSubset, SourceStack
    from draco_amd.core import containers
    from draco_amd.core.task import PipelineStopIteration

    _, fb, _ = beamform_golden(gold, "closed_w")
    beam, weight, frequency, z = fb.beam[:].copy(), fb.weight[:].copy(), fb.index_map["freq"], fb.redshift["z"].copy()
    fb = to_formed_beam(beam, weight, frequency, z, tag="cat_closed")  # (device only: reading it above made host copies)
    sub = RandomSubset(number=3, size=20, seed=7)
    sub.setup(fb)
    stk, grp = SourceStack(freqside=2), GroupSourceStacks(ngroup=2)
    grp.setup()
    groups, i = [], 0
    while True:
        try:
            mock = sub.process()
        except PipelineStopIteration:
            break
        assert type(mock) is containers.FormedBeam and mock.attrs["tag"] == f"cat_closed_mock_{i:05d}"
        for ds in (mock.beam, mock.weight):
            assert ds.on_device and ds._host is None and ds._dev.is_cuda
        ind = gold["chain/indices"][i]
        assert np.array_equal(sub.last_indices, ind) and np.array_equal(mock.redshift["z"], z[ind])
        g = grp.process(stk.process(mock))
        assert (mock.beam._host is None) and (mock.weight._host is None)  # the stack did not pull them to the host
        if g is not None:
            groups.append(g)
        i += 1
    groups.append(grp.process_finish())
    assert i == 3 and len(groups) == 2 and fb.beam._host is None and fb.weight._host is None
    m = 0
    for k, g in enumerate(groups):
        assert type(g) is containers.MockFrequencyStackByPol and g.attrs["tag"] == str(gold[f"chain/group{k}_tag"])
        ref_s, ref_w = gold[f"chain/group{k}_stack"], gold[f"chain/group{k}_weight"]
        assert g.stack.shape == ref_s.shape
        for j in range(ref_s.shape[0]):
            ind = gold["chain/indices"][m]
            truth = twin.source_stack(beam[ind], weight[ind], frequency, z[ind], freqside=2, dtype=np.longdouble)
            f64 = twin.source_stack(beam[ind], weight[ind], frequency, z[ind], freqside=2, dtype=np.float64)
            norm = truth["norm"]
            check(f"chain mock {m}", g.stack[:][j], g.weight[:][j], truth["stack"], truth["weight"], norm, twin.stack_error(f64["stack"], truth["stack"], norm),
                  twin.weight_error(f64["weight"], truth["weight"]), (ref_s[j], ref_w[j], twin.stack_error(ref_s[j], truth["stack"], norm), twin.weight_error(ref_w[j], truth["weight"])))
            m += 1


def test_beamformcat_meets_sourcestack(golden_dir):
    """The ``FormedBeam`` of ``BeamFormCat``'s golden case goes through ``SourceStack``."""
    import srcbeam_twin as sb
    from draco_amd.analysis import beamform as bf
    from draco_amd.analysis.sourcestack import SourceStack
    from draco_amd.core import containers

    z = dict(np.load(os.path.join(golden_dir, "srcbeam.npz")))
    tel, data, cat, _ = sb.golden_inputs(z)
    task = bf.BeamFormCat(timetrack=sb.TIMETRACK, **sb.CASES["ss_nobeam_copol"][2])
    task.setup(tel, sb.to_container(tel, data["ss"]))
    fb = task.process(sb.to_catalog(cat, tag="cat_a"))
    assert fb.beam.on_device
    res = SourceStack(freqside=1).process(fb)
    assert type(res) is containers.FrequencyStackByPol and res.stack.shape == (2, 3) and res.weight[:].any() and np.isfinite(res.stack[:]).all()
    truth = twin.source_stack(fb.beam[:], fb.weight[:], fb.index_map["freq"], fb.redshift["z"], freqside=1, dtype=np.longdouble)
    f64 = twin.source_stack(fb.beam[:], fb.weight[:], fb.index_map["freq"], fb.redshift["z"], freqside=1, dtype=np.float64)
    check("BeamFormCat -> SourceStack", res.stack[:], res.weight[:], truth["stack"], truth["weight"], truth["norm"], twin.stack_error(f64["stack"], truth["stack"], truth["norm"]),
          twin.weight_error(f64["weight"], truth["weight"]))
