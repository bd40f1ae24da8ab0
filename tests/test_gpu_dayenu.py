"""GPU DAYENU delay filter (`csrc/dayenu.hip`, `draco_amd/analysis/dayenu.py`) against a long-double truth and
against vectors produced by executing the reference (`tests/gen_golden_dayenu.py` -> tests/golden/dayenu*.npz).

Error measure.  At `epsilon = 1e-12` the covariance has a condition number of about 1e13 and the reference's own
float64 result (`numpy.linalg.pinv`) is 1e-3 away from the truth, so nothing is compared with the reference to a
float64 tolerance.  Per case `e_gpu = max |gpu - truth| / max |truth|`, separately for data and weights, with the truth
(long-double Cholesky inverse applied in long double, `tests/dayenu_twin.py`) rounded to the container's dtype;
required: `e_gpu <= max(2 e_ref, 2**-22)`, `e_ref` the same measure of the reference's output (stored by the
generator).  The factor 2 is the margin for another rounding order; the floor is one float32 ulp of the largest value,
doubled.  Against the reference's vectors the triangle inequality gives `<= 3 e_ref + 2**-22`.

Measured `e_ref` (data, weight): A 1.1e-6, 1.7e-3; B 4.2e-5, 1.7e-5; C 2.5e-8, 1.2e-11; ring map 7.3e-7, 2.1e-3;
functions 2.0e-3 and 2.3e-3.  (The data scale of A and of the ring map is set by the skipped items' untouched 1e4.)
Each test prints its `e_gpu` before it asserts.
"""

import os
import types

import numpy as np
import pytest

import dayenu_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR = 2.0**-22


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "dayenu.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ring():
    with np.load(os.path.join(GOLDEN, "dayenu_ringmap.npz")) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(GOLDEN, "dayenu_ringmap_ref.npz")) as z:
        g.update({k: z[k] for k in z.files})
    g["map"], g["weight"] = g["map"].astype(np.float64), g["weight"].astype(np.float64)
    g["truth_map"], g["truth_weight"] = twin.filter_ringmap(g["freq"], float(g["cfg"][1]), g["map"], g["weight"], float(g["cfg"][0]), 0.0, truth=True)
    return g


def _telescope(feedpos):
    return types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None)


def _run_stream(g, name, **over):
    from draco_amd.analysis.dayenu import DayenuDelayFilter
    from draco_amd.core import containers

    eps, tauw, za, atten = (float(x) for x in g[f"{name}/cfg"])
    cfg = dict(epsilon=eps, tauw=tauw, za_cut=za, atten_threshold=atten, telescope_orientation=str(g[f"{name}/orientation"]))
    cfg.update(over)
    vis, weight = g[f"{name}/vis"], g[f"{name}/weight"]
    s = containers.SiderealStream(freq=g[f"{name}/freq"], ra=vis.shape[2], prod=g[f"{name}/prod"], input=len(g[f"{name}/feedpos"]))
    s.vis[:] = vis
    s.weight[:] = weight
    task = DayenuDelayFilter(**cfg)
    task.setup(_telescope(g[f"{name}/feedpos"]))
    out = task.process(s)
    assert out is s and s.vis.on_device and s.weight.on_device
    return task, s.vis[:], s.weight[:]


def _check(name, got, truth, ref, e_ref):
    e_gpu, e_tri = twin.rel_err(got, truth), float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"dayenu {name}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} (to the reference {e_tri:.3e})")
    assert np.isfinite(got).all()
    assert e_gpu <= max(2 * e_ref, FLOOR), (name, e_gpu, e_ref)
    assert e_tri <= 3 * e_ref + FLOOR, (name, e_tri, e_ref)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_stream(gold, name):
    g = gold
    task, vis, weight = _run_stream(g, name)
    assert np.allclose(task._get_cut(g[f"{name}/prod"]), g[f"{name}/cutoff"], rtol=1e-14, atol=0)
    assert vis.dtype == np.complex64 and weight.dtype == np.float32
    _check(f"{name} vis", vis, g[f"{name}/truth_vis"], g[f"{name}/ref_vis"], float(g[f"{name}/e_ref"][0]))
    _check(f"{name} weight", weight, g[f"{name}/truth_weight"], g[f"{name}/ref_weight"], float(g[f"{name}/e_ref"][1]))
    # flagged channels, skipped items and the channels the attenuation mask removes: exactly the reference's zeros
    assert np.array_equal(weight == 0, g[f"{name}/ref_weight"] == 0)
    flagged = ~np.all(g[f"{name}/weight"] > 0, axis=2)
    assert not weight[flagged].any() and not vis[flagged & flagged.any(axis=0) & ~flagged.all(axis=0)].any()
    if name == "A":
        assert not weight[:, 3].any() and np.array_equal(vis[:, 3].view(np.uint32), g["A/vis"][:, 3].view(np.uint32))
        assert np.array_equal(vis[:, 1].view(np.uint32), vis[:, 4].view(np.uint32)) and np.array_equal(weight[:, 1], weight[:, 4])
    if name == "B":
        low = (weight == 0).all(axis=2) & ~flagged
        assert low.any() and np.array_equal(low, (g["B/ref_weight"] == 0).all(axis=2) & ~flagged)


def test_ringmap(ring):
    from draco_amd.analysis.dayenu import DayenuDelayFilterMap
    from draco_amd.core import containers

    g = ring
    nb, npol, nfreq, nra, nel = g["map"].shape
    rm = containers.RingMap(freq=g["freq"], beam=nb, pol=np.array(["XX", "YY"]), ra=nra, el=np.linspace(-1, 1, nel))
    rm.map[:] = g["map"]
    rm.weight[:] = g["weight"]
    task = DayenuDelayFilterMap(epsilon=float(g["cfg"][0]), tauw=float(g["cfg"][1]))
    task.setup()
    assert task.process(rm) is rm and rm.map.on_device and rm.weight.on_device
    m, w = rm.map[:], rm.weight[:]
    assert twin.rel_err(g["ref_map"], g["truth_map"]) == float(g["e_ref"][0]) and twin.rel_err(g["ref_weight"], g["truth_weight"]) == float(g["e_ref"][1])
    _check("ring map", m, g["truth_map"], g["ref_map"], float(g["e_ref"][0]))
    _check("ring weight", w, g["truth_weight"], g["ref_weight"], float(g["e_ref"][1]))
    assert np.array_equal(w == 0, g["ref_weight"] == 0)
    assert not w[1, :, :, 6].any() and np.array_equal(m[0, 1, :, :, 6].view(np.uint64), g["map"][0, 1, :, :, 6].view(np.uint64))


@pytest.mark.parametrize("name", ["hp", "two"])
def test_functions(gold, name):
    from draco_amd.analysis import dayenu

    g = gold
    freq, flag = g[f"fn_{name}/freq"], g[f"fn_{name}/flag"]
    if name == "hp":
        pinv, index = dayenu.highpass_delay_filter(freq, float(g["fn_hp/tw"][0]), flag, epsilon=float(g["fn_hp/eps"][0]))
    else:
        pinv, index = dayenu.delay_filter(freq, flag, g["fn_two/tw"], 0.0, g["fn_two/eps"])
    assert pinv.is_cuda and tuple(pinv.shape) == g[f"fn_{name}/ref_pinv"].shape
    idx = np.full(flag.shape[1], -1)
    for u, ind in enumerate(index):
        idx[ind] = u
    assert np.array_equal(idx, g[f"fn_{name}/index"])
    p = pinv.cpu().numpy()
    _check(f"fn {name}", p, g[f"fn_{name}/truth_pinv"], g[f"fn_{name}/ref_pinv"], float(g[f"fn_{name}/e_ref"]))
    assert np.array_equal(p == 0, g[f"fn_{name}/ref_pinv"] == 0)
    low = np.stack([twin.atten_flag(np.diag(q), 0.1) for q in p])
    assert np.array_equal(low, g[f"fn_{name}/low"])


def test_build_block_edges():
    """`dmm_dayenu_build` at the orders around the 32-row panels of `k_dy_chol` (a last panel of 1, 2, 31, 32 and 33
    rows, behind zero to four full ones), one matrix per order, against the long-double Cholesky inverse.  Required:
    `e_gpu <= max(2 e_ref, n cond(C) 2**-52)`, `e_ref` the same measure of `numpy.linalg.pinv` of the float64
    covariance; the floor is the conditioning bound, for the two tiny orders where `pinv` is nearly exact.

    Measured (MI355X), `e_gpu` / `e_ref`: order 1 4.8e-17 / 4.8e-17, 2 3.1e-15 / 2.0e-15 (floor 2.2e-14), 31 2.2e-4 / 6.3e-4,
    32 2.5e-4 / 7.1e-4, 33 2.5e-4 / 1.5e-3, 63 5.9e-4 / 9.1e-4, 64 6.0e-4 / 2.4e-3, 65 6.1e-4 / 1.3e-3, 97 7.5e-4 / 1.9e-3,
    129 1.2e-3 / 1.7e-3: below `2 e_ref` at every order from 31 up, without the floor."""
    from draco_amd.analysis.dayenu import build_filters
    from draco_amd.device import Context

    ctx = Context.get()
    tw, eps = 0.2, 1e-12
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 97, 129):
        freq = np.linspace(400.0, 800.0, 1024)[:n].copy()
        flag = np.ones(n, dtype=bool)
        if n > 3:
            flag[[j for j in (0, 5, 32, n - 1) if j < n]] = False
        nf, status = build_filters(ctx, ctx.to_device(freq), np.array([[[tw, eps]]]), flag[np.newaxis, :])
        x = nf.cpu().numpy()[0]
        truth = twin.filter_truth(freq, flag, tw, eps)
        ref = twin.delay_filter_f64(freq, flag[:, np.newaxis], tw, eps)[0][0]
        sel = np.flatnonzero(flag)
        cond = float(np.linalg.cond(twin.covariance(freq, tw, eps)[np.ix_(sel, sel)]))
        e_gpu, e_ref = twin.rel_err(x, truth), twin.rel_err(ref, truth)
        print(f"dayenu build n {n}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} floor {n * cond * 2.0**-52:.3e}")
        assert not status.any(), (n, status)
        assert np.isfinite(x).all(), n
        assert not x[~flag, :].any() and not x[:, ~flag].any(), n
        assert e_gpu <= max(2 * e_ref, n * cond * 2.0**-52), (n, e_gpu, e_ref)


def test_failure_path(gold, caplog):
    """An indefinite covariance (negative epsilon): no exception, every weight zero, data untouched, nothing NaN."""
    task, vis, weight = _run_stream(gold, "C", epsilon=-1e-12)
    assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(weight).all()
    assert not weight.any()
    assert np.array_equal(vis.view(np.uint32), gold["C/vis"].view(np.uint32))
    assert any("Failed" in r.getMessage() for r in caplog.records)


def test_errors(gold):
    from draco_amd.analysis import dayenu

    g = gold
    with pytest.raises(NotImplementedError):
        _run_stream(g, "C", single_mask=False)
    with pytest.raises(ValueError, match="lambda_max"):
        _run_stream(g, "C", epsilon=1e-17)
    with pytest.raises(NotImplementedError):
        dayenu.delay_filter(g["fn_hp/freq"], g["fn_hp/flag"], 0.1, tau_centre=0.05)
    with pytest.raises(NotImplementedError):
        dayenu.DayenuDelayFilterMap(filename="cutoff.h5").setup()
    t = dayenu.DayenuDelayFilterMap(single_mask=False)
    t.setup()
    with pytest.raises(NotImplementedError):
        t.process(None)
