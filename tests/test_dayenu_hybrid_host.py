"""Host-side checks of the hybrid-visibility DAYENU golden vectors and of the NumPy twin
(`tests/dayenu_hybrid_twin.py`); no GPU.

* The twin's f64 form (same algorithm, same LAPACK as the reference) agrees with the reference's vectors in the golden
  file to `1e-3 e_ref + floor` (max |twin - reference| / max |reference|), `floor = 2**-22` for the float32 datasets
  and `2**-44` for the float64 ones.
* At the stored positions the reference is within the stored `e_ref` of the twin's truth.
* The file holds what `test_gpu_dayenu_hybrid.py` reads, and the cases reach what they are there for.
* The container and the tasks' configuration, which need no device.
"""

import os

import numpy as np
import pytest

import dayenu_hybrid_twin as twin
from conftest import GOLDEN

F32, F64 = 2.0**-22, 2.0**-44


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "dayenu_hybrid.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def h33(gold):
    c = twin.case(gold, "H33")
    return c, twin.filter_hybrid(c["freq"], c["vis"], c["weight"], **c["cfg"]), twin.truth_of(c)


def _close(a, ref, e_ref, floor):
    d = float(np.abs(a - ref).max() / np.abs(ref).max())
    assert d <= 1e-3 * e_ref + floor, (d, e_ref)


def _within(ref, truth, scale, e_ref):
    d = float(np.abs(ref - truth).max() / scale)
    assert d <= e_ref, (d, e_ref)


@pytest.mark.parametrize("name", twin.HYBRID_CASES)
def test_hybrid_twin(gold, name):
    g = gold
    c = twin.case(g, name)
    pos = c["pos"]
    v, w, f, cov = twin.filter_hybrid(c["freq"], c["vis"], c["weight"], **c["cfg"])
    t = twin.truth_of(c)
    assert v.dtype == np.complex64 and w.dtype == np.float32
    if name == "H6":  # nothing is applied: the reference's outputs are the inputs and are not stored
        assert np.array_equal(v, c["vis"]) and np.array_equal(w, c["weight"]) and f"{name}/ref_vis" not in g
    else:
        sampled = g[f"{name}/ref_vis"].ndim == 4
        _close(twin.at_positions("vis", v, pos) if sampled else v, g[f"{name}/ref_vis"], float(g[f"{name}/e_ref_vis"]), F32)
        _close(w, g[f"{name}/ref_weight"], float(g[f"{name}/e_ref_weight"]), F32)
        assert np.array_equal(w == 0, g[f"{name}/ref_weight"] == 0) and np.array_equal(t["weight"] == 0, g[f"{name}/ref_weight"] == 0)
        _within(g[f"{name}/ref_vis"], twin.at_positions("vis", t["vis"], pos) if sampled else t["vis"], np.abs(t["vis"]).max(), float(g[f"{name}/e_ref_vis"]))
        _within(g[f"{name}/ref_weight"], t["weight"], np.abs(t["weight"]).max(), float(g[f"{name}/e_ref_weight"]))
    for ds, got in (("filter", f), ("freq_cov", cov)):
        assert (got is not None) == (f"{name}/ref_{ds}" in g) == c["cfg"]["save_filter" if ds == "filter" else "calculate_cov"]
        if got is not None:
            _close(twin.at_positions(ds, got, pos), g[f"{name}/ref_{ds}"], float(g[f"{name}/e_ref_{ds}"]), F64)
            _within(g[f"{name}/ref_{ds}"], twin.at_positions(ds, t[ds], pos), np.abs(t[ds]).max(), float(g[f"{name}/e_ref_{ds}"]))


def test_cases_reach_their_paths(gold):
    c = twin.case(gold, "H33")
    assert c["vis"].shape == (2, 33, 3, 5, 40) and c["cfg"] == dict(tauw=0.4, epsilon=1e-3, atten_threshold=0.0, apply_filter=True, save_filter=True, calculate_cov=True)
    flag = twin.sample_mask(c["weight"])
    masks = {flag[:, x, t].tobytes() for x in range(3) for t in range(40)}
    assert len(masks) >= 4 + 2  # four filters and more, the empty mask and the single channel
    for x in (0, 1):
        assert len({flag[:, x, t].tobytes() for t in range(32)}) == 3  # one run of 32 adjacent RA holds three of them
    nvalid = flag.sum(axis=0)
    assert (nvalid == 0).any() and (nvalid == 1).any()
    one_pol = (c["weight"] > 0).any(axis=0) & ~flag
    assert one_pol.any()  # a channel zero in one polarisation only
    have = {tuple(p) for p in c["pos"]}
    assert (0, 0) in have and (2, 39) in have and {flag[:, x, t].tobytes() for x, t in have} == masks  # every distinct mask is sampled

    c = twin.case(gold, "H70")
    assert c["vis"].shape == (1, 70, 1, 1, 33) and c["cfg"]["epsilon"] == 1e-12 and c["cfg"]["atten_threshold"] > 0 and not c["cfg"]["save_filter"]
    rw, flag = gold["H70/ref_weight"], twin.sample_mask(c["weight"])
    removed = (rw == 0) & flag[np.newaxis]
    assert removed.any() and (rw != 0).any()
    # no diagonal element within 10 e_ref of the attenuation threshold: the truth and the reference remove the same channels
    e = max(float(gold["H70/e_ref_vis"]), float(gold["H70/e_ref_weight"]))
    assert len({flag[:, 0, t].tobytes() for t in range(33)}) == len({flag[:, 0, t].tobytes() for t in (0, 12, 25)})
    for t in (0, 12, 25):
        d = np.diag(twin.dt.filter_truth(c["freq"], flag[:, 0, t], 0.4, 1e-12).astype(np.float64))
        thr = c["cfg"]["atten_threshold"] * np.median(d[d > 0])
        assert np.all(np.abs(d[d > 0] - thr) > 10 * e * thr)

    c = twin.case(gold, "H6")
    assert c["vis"].shape == (2, 6, 2, 17, 65) and c["cfg"]["save_filter"] and not c["cfg"]["apply_filter"] and not c["cfg"]["calculate_cov"]
    c = twin.case(gold, "H20")
    assert c["vis"].shape[1] == 20 and np.asarray(c["cfg"]["tauw"]).size == 2 and np.asarray(c["cfg"]["epsilon"]).size == 2 and c["cfg"]["calculate_cov"]
    assert float(c["cfg"]["tauw"][0]) == 0.2 and float(c["cfg"]["epsilon"][0]) == 1e-3


@pytest.mark.parametrize("name", twin.R_CASES)
def test_ra_dependent_weights_twin(gold, h33, name):
    g = gold
    scheme, excl = twin.r_case(name)
    _, (_, w, f, cov), t33 = h33
    rw = g["R/ring_weight"].astype(np.float64)
    rpos, fpos = g["R/rpos"], g["R/fpos"]
    ow, of, oc = twin.ra_dependent_weights(w, rw, scheme, excl, f, cov)
    tw, tf, tc = (None if a is None else a.astype(np.float64) for a in twin.ra_dependent_weights(t33["weight"], rw, scheme, excl, t33["filter"], t33["freq_cov"], truth=True))
    assert (oc is None) == (scheme == "inverse_variance") == (f"{name}/ref_freq_cov" not in g)
    _close(ow[:, :, rpos, :], g[f"{name}/ref_weight"], float(g[f"{name}/e_ref_weight"]), F64)
    _within(g[f"{name}/ref_weight"], tw[:, :, rpos, :], np.abs(tw).max(), float(g[f"{name}/e_ref_weight"]))
    for ds, got, truth in (("filter", of, tf), ("freq_cov", oc, tc)):
        if got is not None:
            _close(got[..., fpos], g[f"{name}/ref_{ds}"], float(g[f"{name}/e_ref_{ds}"]), F64)
            _within(g[f"{name}/ref_{ds}"], truth[..., fpos], np.abs(truth).max(), float(g[f"{name}/e_ref_{ds}"]))


def test_container():
    from draco_amd.core import containers

    hv = containers.HybridVisStream(pol=2, freq=np.array([600.0, 601.0, 602.0]), ew=3, el=5, ra=8)
    assert "filter" not in hv and "freq_cov" not in hv and "freq_sum" not in hv.index_map
    with pytest.raises(KeyError):
        hv.filter
    hv.add_dataset("filter", allocate=True)
    assert "filter" in hv and "freq_cov" not in hv and hv.filter[:].shape == (2, 3, 3, 3, 8) and hv.filter.dtype == np.float64
    assert np.array_equal(hv.index_map["freq_sum"], hv.index_map["freq"])
    hv.add_dataset("freq_cov", allocate=True)
    assert hv.freq_cov[:].shape == (2, 3, 3, 3, 8) and hv.datasets["freq_cov"] is hv.freq_cov
    for name in ("complex_filter", "complex_freq_cov"):
        with pytest.raises(NotImplementedError):
            hv.add_dataset(name)
        with pytest.raises(NotImplementedError):
            getattr(hv, name)
    other = containers.HybridVisStream(axes_from=hv, attrs_from=hv)
    assert "filter" not in other and other.vis[:].shape == (2, 3, 3, 5, 8)


def test_task_configuration():
    from draco_amd.analysis.dayenu import DayenuDelayFilterHybridVis
    from draco_amd.analysis.ringmapmaker import RADependentWeights
    from draco_amd.core import containers

    t = DayenuDelayFilterHybridVis()
    assert (t.tauw, t.tauc, t.epsilon, t.atten_threshold, t.apply_filter, t.save_filter, t.calculate_cov, t.workspace_mib) == (0.4, 0.0, 1e-12, 0.0, True, False, False, 1024)
    t.setup()
    t = DayenuDelayFilterHybridVis(tauw=[0.2, 0.6], epsilon=[1e-3, 1e-2], save_filter=1, workspace_mib=8)
    assert np.array_equal(t.tauw, [0.2, 0.6]) and np.array_equal(t.epsilon, [1e-3, 1e-2]) and t.save_filter is True and t.workspace_mib == 8
    with pytest.raises(RuntimeError, match="At least one of `save_filter` and `apply_filter` must be True"):
        DayenuDelayFilterHybridVis(apply_filter=False).setup()
    with pytest.raises(AttributeError):
        DayenuDelayFilterHybridVis(single_mask=True)
    hv = containers.HybridVisStream(pol=1, freq=np.array([600.0, 601.0]), ew=1, el=1, ra=4)
    with pytest.raises(NotImplementedError, match="tau_centre"):
        DayenuDelayFilterHybridVis(tauc=0.1).process(hv)
    rm = containers.RingMap(beam=1, pol=1, freq=np.array([600.0, 601.0]), ra=4, el=1)
    for attrs in ({}, {"weight_ew": "natural"}, {"exclude_cyl": []}):
        rm.attrs.clear()
        rm.attrs.update(attrs)
        with pytest.raises(RuntimeError, match="must save `weight_ew` and `exclude_cyl`"):
            RADependentWeights().process(hv, rm)


def test_group_rows():
    from draco_amd.analysis.dayenu import _group_rows

    rng = np.random.default_rng(5)
    for n in (1, 6, 64, 70, 130):
        base = (rng.uniform(size=(5, n)) < 0.7).astype(np.uint8)
        flags = base[rng.integers(5, size=200)]
        flags[[3, 77]] = 0
        masks, index = _group_rows(flags)
        empty = ~flags.any(axis=1)
        assert np.all(index[empty] == -1) and np.all(index[~empty] >= 0)
        assert np.array_equal(masks[index[~empty]], flags[~empty])
        assert masks.shape[0] == np.unique(flags[~empty], axis=0).shape[0] and masks.dtype == np.uint8
    masks, index = _group_rows(np.zeros((4, 9), dtype=np.uint8))
    assert masks.shape == (0, 9) and np.all(index == -1)
