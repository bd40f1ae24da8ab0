"""The NumPy twin of the DAYENU m-mode filter (`tests/mfilter_twin.py`) against vectors produced by executing the
reference (`tests/gen_golden_mfilter.py` -> tests/golden/mfilter.npz), and the host-side pieces of
`draco_amd/analysis/dayenu.py`.  No GPU."""

import os

import numpy as np
import pytest

import dayenu_twin
import mfilter_twin as twin
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "mfilter.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_twin_reproduces_reference_stream(gold, name):
    g = {k.split("/")[1]: v for k, v in gold.items() if k.startswith(name + "/")}
    eps, dec, fi, fe, spacing, lat = (float(x) for x in g["cfg"])
    ov, ow = twin.filter_stream(g["freq"], g["ra"], g["feedpos"], g["prod"], spacing, lat, g["vis"], g["weight"], dec, eps, fi, fe)
    e = float(np.abs(ov - g["ref_vis"]).max() / np.abs(g["ref_vis"]).max())
    print(f"mfilter twin {name}: to the reference {e:.3e}, e_ref {float(g['e_ref']):.3e}")
    assert e <= 3 * float(g["e_ref"])
    assert np.array_equal(ow, g["ref_weight"])
    assert twin.rel_err(g["ref_vis"], g["truth_vis"]) == float(g["e_ref"])


@pytest.mark.parametrize("kind", ["bandpass", "lowpass", "highpass"])
def test_twin_reproduces_reference_functions(gold, kind):
    g = {k.split("/")[1]: v for k, v in gold.items() if k.startswith(f"fn_{kind}/")}
    mc, m0, eps = (float(x) for x in g["par"])
    p, index = twin.mmode_filter_f64(g["ra"], kind, mc, m0, g["flag"], eps)
    e = float(np.abs(p - g["ref_pinv"]).max() / np.abs(g["ref_pinv"]).max())
    print(f"mfilter twin fn {kind}: to the reference {e:.3e}, e_ref {float(g['e_ref']):.3e}")
    assert e <= 3 * float(g["e_ref"])
    idx = np.full(g["flag"].shape[:-1], -1)
    for u, ind in enumerate(index):
        idx[ind] = u
    assert np.array_equal(idx, g["index"])


def test_truth_agrees_with_the_delay_twin_on_a_high_pass():
    """The same matrix through both twins: ``I + sinc(2 tw dfreq) / eps`` is the m-mode high-pass with ``ra = freq`` and
    ``m_cut = 2 pi tw`` (taken in long double)."""
    freq = 600.0 + 0.390625 * np.arange(40)
    flag = np.ones(40, dtype=bool)
    flag[[3, 17, 18]] = False
    tw, eps = 0.15, 1e-6
    a = dayenu_twin.filter_truth(freq, flag, tw, eps)
    b = twin.filter_truth(freq, "highpass", 2 * dayenu_twin.LD(tw) * dayenu_twin.PI_LD, 0.0, flag, eps)
    assert np.array_equal(a == 0, b == 0)
    assert twin.rel_err(b, a) <= 1e-9


def test_instantaneous_m(gold):
    from draco_amd.analysis.dayenu import instantaneous_m

    got = np.array([instantaneous_m(*a) for a in gold["im/args"]])
    assert np.allclose(got, gold["im/ref"], rtol=1e-14, atol=0)
    assert np.allclose(instantaneous_m(*gold["im/args"].T), gold["im/ref"], rtol=1e-14, atol=0)
    assert np.allclose([twin.instantaneous_m(*a) for a in gold["im/args"]], gold["im/ref"], rtol=1e-14, atol=0)


def test_eigenvalue_guard_bounds_the_row_sum(gold):
    """The O(nra) bound of `check_mmode_eigenvalue_cut` is above the largest absolute row sum of the covariance."""
    from draco_amd.analysis import dayenu

    ra = gold["fn_lowpass/ra"]
    for kind, mc, m0 in (("bandpass", 3.6, 6.0), ("lowpass", 7.2, 0.0), ("highpass", 7.2, 0.0)):
        par = dayenu._mmode_params(ra, kind, mc, m0, 1e-10)
        rowsum = np.abs(twin.covariance(ra, kind, mc, m0, 1e-10)).sum(axis=1).max()
        dayenu.check_mmode_eigenvalue_cut(ra, par)
        with pytest.raises(ValueError, match="lambda_max"):
            dayenu.check_mmode_eigenvalue_cut(ra, np.asarray(par) * np.array([0.6e15 / rowsum, 0.6e15 / rowsum, 1.0, 1.0]))
