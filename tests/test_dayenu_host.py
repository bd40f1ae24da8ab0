"""Host-side checks of the DAYENU golden vectors and of the NumPy twin (`tests/dayenu_twin.py`); no GPU.

* The twin's f64 form (same algorithm, same LAPACK as the reference) agrees with the reference's outputs in the golden
  files to `1e-3 e_ref + 1e-7` (max |twin - reference| / max |reference|).
* The twin's truth agrees with the golden truth exactly, and `e_ref` recomputed from the files equals the stored value.
* The cutoff formula agrees with the reference's `_get_cut` values stored in the file.
"""

import os

import numpy as np
import pytest

import dayenu_twin as twin
from conftest import GOLDEN


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
    return g


def _close(a, ref, e_ref):
    d = float(np.abs(a - ref).max() / np.abs(ref).max())
    assert d <= 1e-3 * e_ref + 1e-7, (d, e_ref)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_stream_twin(gold, name):
    g = gold
    eps, tauw, za, atten = (float(x) for x in g[f"{name}/cfg"])
    cutoff = twin.get_cut(g[f"{name}/feedpos"], g[f"{name}/prod"], za, str(g[f"{name}/orientation"]), tauw)
    assert np.allclose(cutoff, g[f"{name}/cutoff"], rtol=1e-14, atol=0)
    args = (g[f"{name}/freq"], g[f"{name}/cutoff"], g[f"{name}/vis"], g[f"{name}/weight"], eps, atten)
    v, w = twin.filter_stream(*args)
    _close(v, g[f"{name}/ref_vis"], float(g[f"{name}/e_ref"][0]))
    _close(w, g[f"{name}/ref_weight"], float(g[f"{name}/e_ref"][1]))
    assert np.array_equal(w == 0, g[f"{name}/ref_weight"] == 0)
    tv, tw = twin.filter_stream(*args, truth=True)
    assert np.array_equal(tv, g[f"{name}/truth_vis"]) and np.array_equal(tw, g[f"{name}/truth_weight"])
    assert twin.rel_err(g[f"{name}/ref_vis"], tv) == g[f"{name}/e_ref"][0] and twin.rel_err(g[f"{name}/ref_weight"], tw) == g[f"{name}/e_ref"][1]


def test_ringmap_twin(ring):
    g = ring
    args = (g["freq"], float(g["cfg"][1]), g["map"], g["weight"], float(g["cfg"][0]), 0.0)
    m, w = twin.filter_ringmap(*args)
    _close(m, g["ref_map"], float(g["e_ref"][0]))
    _close(w, g["ref_weight"], float(g["e_ref"][1]))
    tm, tw = twin.filter_ringmap(*args, truth=True)
    assert twin.rel_err(g["ref_map"], tm) == g["e_ref"][0] and twin.rel_err(g["ref_weight"], tw) == g["e_ref"][1]


@pytest.mark.parametrize("name", ["hp", "two"])
def test_function_twin(gold, name):
    g = gold
    freq, flag, tw, eps = (g[f"fn_{name}/{k}"] for k in ("freq", "flag", "tw", "eps"))
    p, index = twin.delay_filter_f64(freq, flag, tw, eps)
    idx = np.full(flag.shape[1], -1)
    for u, ind in enumerate(index):
        idx[ind] = u
    assert np.array_equal(idx, g[f"fn_{name}/index"])
    _close(p, g[f"fn_{name}/ref_pinv"], float(g[f"fn_{name}/e_ref"]))
    tp, _ = twin.delay_filter_truth(freq, flag, tw, eps)
    assert np.array_equal(tp.astype(np.float64), g[f"fn_{name}/truth_pinv"])
    assert twin.rel_err(g[f"fn_{name}/ref_pinv"], tp) == g[f"fn_{name}/e_ref"]


def test_pseudo_inverse_keeps_every_eigenvalue(gold):
    """The fact the GPU path rests on: on the unflagged block pinv's cut, 1e-15 lambda_max, is below the smallest
    eigenvalue, so the pseudo-inverse is the inverse."""
    g = gold
    flag = np.all(g["A/weight"][:, 1] > 0, axis=-1)
    cov = twin.covariance(g["A/freq"], g["A/cutoff"][1], 1e-12)[np.ix_(flag, flag)]
    lam = np.linalg.eigvalsh(cov)
    assert lam[0] > 0.9 and 1e-15 * lam[-1] < 0.5 * lam[0]
