"""Host half of the Gaussian-process regridder (``draco_amd/util/kernels.py``, ``draco_amd/util/gaussian_process.py``) and
the long-double twin (``tests/gp_twin.py``) against vectors produced by executing the reference
(``tests/gen_golden_gp.py`` -> tests/golden/gp.npz).  No GPU.

* the kept output rows of ``_select_interp_samples`` (sorted searches here, a full distance table there): equal;
* the band height ``M`` found from positions alone, ``convert_band_diagonal`` in its three forms and the band edges of
  ``_get_band_inds``: equal;
* the kernels: ``rtol 1e-14``; the element-wise ``pair_kernel`` that decides ``M``: equal to the matrix entry;
* the twin against the reference's outputs: the data within the rounding of the reference's complex64 store (one
  ``2**-24`` per component) plus ``1e-10`` for its float64 sums, the weights within 2 float32 ulp, the same zeros.
"""

import os

import numpy as np
import pytest

import gp_twin as twin
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "gp.npz")) as z:
        return {k: z[k] for k in z.files}


NAMES = ["kw2_r1", "kw2_r2", "kw2_r8", "kw2_r8_jit", "kw2_r8_eps", "kw2_edge", "kw3_r4", "kw5_128r2", "kw5_128r4", "brutal", "all_masked"]
SPECS = {
    "gaussian": [{"name": "gaussian", "width": 2, "alpha": 1.3}],
    "rational": [{"name": "rational", "width": 2, "alpha": 0.7, "a": 1.5}],
    "matern15": [{"name": "matern", "width": 2, "alpha": 1.0, "nu": 1.5, "epsilon": 1e-4}],
    "matern25": [{"name": "matern", "width": 2, "alpha": 1.0, "nu": 2.5, "epsilon": 1e-3}],
    "product": [{"name": "matern", "width": 3, "alpha": 1.1, "nu": 2.5, "epsilon": 1e-3}, {"name": "gaussian", "width": 4, "alpha": 0.9, "epsilon": 2e-3}],
}


def case(gold, name):
    kw, samples, nin, eps, nstack = gold[f"case/{name}/params"]
    g = {k: gold[f"case/{name}/{k}"] for k in ("xi", "xo", "x", "w", "mt", "xout", "wout", "M", "bound")}
    g.update(kw=int(kw), samples=int(samples), eps=float(eps), spec={"name": "matern", "width": int(kw), "alpha": 1.0, "nu": 2.5, "epsilon": float(eps)})
    return g


def test_names(gold):
    assert list(gold["names"]) == NAMES


def test_task_import():
    from draco_amd.analysis.sidereal import SiderealRegridder, SiderealRegridderGP

    t = SiderealRegridderGP()
    assert issubclass(SiderealRegridderGP, SiderealRegridder)
    assert (t.mask_cutoff, t.mask_cutoff_partition, t.samples, t.kernel_width, t.epsilon, t.down_mix) == (1.7, 1, 1024, 5, 1e-3, False)


@pytest.mark.parametrize("name", NAMES)
def test_select_interp_samples(gold, name):
    from draco_amd.util import gaussian_process as gp

    g = case(gold, name)
    cutoff, partition = float(gold["cutoff"][0]), int(gold["cutoff"][1])
    mask = ~np.all(g["w"] == 0, axis=-1)
    assert np.array_equal(gp._select_interp_samples(g["xi"], g["xo"], mask, g["kw"], cutoff, partition), g["mt"])
    if name == "all_masked":
        assert not g["mt"].any()


def test_select_interp_samples_against_table():
    """Random positions with coincident points, every partition: the booleans of the full distance table."""
    from draco_amd.util import gaussian_process as gp

    rng = np.random.default_rng(5)
    xi = np.sort(rng.uniform(0, 1, 90))
    xo = np.concatenate([np.linspace(-0.1, 1.1, 61), xi[[3, 40, 41]]])
    mask = rng.uniform(size=(4, 90)) < np.array([0.9, 0.5, 0.1, 0.0])[:, None]
    mask[2, :3] = True
    med = np.median(np.abs(np.diff(xi)))
    dist = np.subtract.outer(xo, xi) / med
    for kwidth, cutoff, partition in ((3, 1.7, 1), (2.5, 1.0, 0), (6, 2.9, 2)):
        kc = kwidth - 1
        want = np.zeros((4, len(xo)), dtype=bool)
        for ii in range(3):
            d = dist[:, mask[ii]]
            p = np.min(d, axis=-1, where=d > 0, initial=kc)
            q = np.max(d, axis=-1, where=d < 0, initial=-kc)
            want[ii] = (np.maximum(p, np.abs(q)) < kc) & (np.sort(np.abs(d), axis=-1)[:, partition] < cutoff)
        assert np.array_equal(gp._select_interp_samples(xi, xo, mask, kwidth, cutoff, partition), want)


@pytest.mark.parametrize("name", list(SPECS))
def test_kernels(gold, name):
    from draco_amd.util import gaussian_process as gp
    from draco_amd.util import kernels

    xi, xo = gold["host/xi"], gold["host/xo"]
    spec = [dict(s) for s in SPECS[name]]
    Ki, Ks = gp._combine_gp_kernels_from_specs((xo, xi), spec)
    assert spec == SPECS[name], "the caller's specs are left as they are"
    np.testing.assert_allclose(Ki, gold[f"host/{name}/Ki"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(Ks, gold[f"host/{name}/Ks"], rtol=1e-14, atol=0)
    # the element-wise form is the matrix entry
    specs, eps = gp._split_specs(spec)
    _, _, pairs = gp._device_specs(specs, np.median(np.abs(np.diff(xo))))
    assert np.array_equal(gp._pair_product(pairs, xo[:, None], xi[None, :]), Ks)
    assert np.array_equal(gp._pair_product(pairs, xi[:, None], xi[None, :]) + eps * np.eye(len(xi)), Ki)
    assert gp._band_rows_from_positions(xi, pairs, eps) == kernels.band_rows(Ki)


def test_distances_and_names(gold):
    from draco_amd.util import kernels

    np.testing.assert_allclose(kernels.squared_difference_kernel((gold["host/xo"], 7), (0.5, 2.0)), gold["host/sqdiff"], rtol=1e-14)
    np.testing.assert_allclose(kernels.euclidean_difference_kernel(6, 1.5), gold["host/eudiff"], rtol=1e-14)
    assert kernels.get_kernel("Periodic", N=5, width=2.0, alpha=1.0, p=3.0).shape == (5, 5)
    assert kernels.get_kernel("moving_average", N=6, width=3, alpha=2.0).shape == (6, 6)
    with pytest.raises(ValueError, match="Invalid kernel type"):
        kernels.get_kernel("boxcar", N=4, width=1.0, alpha=1.0)
    with pytest.raises(ValueError, match="nu"):
        kernels.matern_kernel(4, 1.0, 1.0, nu=0.5)
    assert kernels.is_hermitian_positive_definite(gold["host/matern25/Ki"])
    assert not kernels.is_hermitian_positive_definite(gold["host/matern25/Ki"] - 2 * np.eye(35))
    assert not kernels.is_hermitian_positive_definite(gold["host/matern25/Ks"][:35] + np.triu(np.ones((35, 35)), 1))


def test_device_specs_refuse_host_only_kernels():
    from draco_amd.util import gaussian_process as gp

    for name in ("periodic", "moving_average"):
        with pytest.raises(NotImplementedError):
            gp._device_specs([{"name": name, "width": 2, "alpha": 1.0, "p": 3.0}], 1.0)
    with pytest.raises(ValueError):
        gp._device_specs([{"name": "boxcar", "width": 2, "alpha": 1.0}], 1.0)


@pytest.mark.parametrize("which", ["full", "upper", "lower"])
def test_convert_band_diagonal(gold, which):
    from draco_amd.util import kernels

    got = kernels.convert_band_diagonal(gold["host/matern25/Ki"], which=which)
    assert got.shape == gold[f"host/band/{which}"].shape and np.array_equal(got, gold[f"host/band/{which}"])
    with pytest.raises(ValueError):
        kernels.convert_band_diagonal(gold["host/matern25/Ki"], which="middle")


@pytest.fixture(scope="module")
def twins(gold):
    """The twin's chain of every case, computed once."""
    from draco_amd.util import gaussian_process as gp

    out = {}
    for name in NAMES:
        g = case(gold, name)
        Ki, Ks = gp._combine_gp_kernels_from_specs((g["xo"], g["xi"]), g["spec"])
        out[name] = twin.resample(g["x"], g["w"], Ki, Ks, g["mt"])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_band_rows_and_edges(gold, twins, name):
    from draco_amd.util import gaussian_process as gp
    from draco_amd.util import kernels

    g = case(gold, name)
    specs, eps = gp._split_specs(g["spec"])
    _, _, pairs = gp._device_specs(specs, np.median(np.abs(np.diff(g["xo"]))))
    for ii, p in enumerate(twins[name][2]):
        if p is None:
            assert g["M"][ii] == 0
            continue
        assert p["M"] == g["M"][ii]
        assert gp._band_rows_from_positions(g["xi"][p["mi"]], pairs, eps) == g["M"][ii]
        start, end = kernels._get_band_inds(p["A"].astype(np.float64), tol=1e-8)
        if gold[f"case/{name}/f{ii}/twin_edges_equal"]:
            assert np.array_equal(start, gold[f"case/{name}/f{ii}/start"]) and np.array_equal(end, gold[f"case/{name}/f{ii}/end"])
        assert start.dtype == end.dtype == np.int32
    if name == "brutal":
        assert g["M"][0] == int(twins[name][2][0]["mi"].sum()) // 2 + 1, "the band rule truncates entries that are not small"
    s, e = kernels._get_band_inds(np.array([[0.0, 2e-4, -3e-4, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0]]))
    assert s.tolist() == [1, 0, 0] and e.tolist() == [3, 0, 4]


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_reference(gold, twins, name):
    g = case(gold, name)
    txout, twout, _ = twins[name]
    assert np.array_equal(twout == 0, g["wout"] == 0) and np.array_equal(txout == 0, g["xout"] == 0)
    d = g["xout"].astype(np.complex128) - txout
    lim = 2.0**-24 * np.maximum(np.abs(txout.real), np.abs(txout.imag)) + 1e-10
    assert np.all(np.abs(d.real) <= lim) and np.all(np.abs(d.imag) <= lim)
    nz = twout != 0
    if nz.any():
        ulp = np.spacing(np.abs(twout[nz]))
        assert np.all(np.abs(g["wout"][nz] - twout[nz]) <= 2 * ulp)
