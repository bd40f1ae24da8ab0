"""Host side of the delay null-space filter (no GPU): the long-double twin against the vectors produced by executing
the reference (`tests/gen_golden_nullfilter.py` -> tests/golden/nullfilter*.npz), the cut / num_modes / mask bookkeeping
of `DelayFilter` and `DelayFilterBase`, and the argument errors of `null_filter`.

The twin must reproduce the reference's outputs within `2 e_ref` (`e_ref` = max |reference - truth| / max |truth| as
stored; the twin is the truth, so this pins the fixture to the twin as committed: the same value up to how the long
double sums round).  The order-1024 matrix is not recomputed here (20 s of long double): its stored rows are checked
against its stored `e_ref`.
"""

import os
import types

import numpy as np
import pytest

import nullfilter_twin as twin
from conftest import GOLDEN


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return {**_load("nullfilter.npz"), **_load("nullfilter_fnbig.npz")}


def _fn_args(g, name):
    window = str(g[f"fn_{name}/window"])
    window = {"": False, "True": True}.get(window, window)
    return g[f"fn_{name}/samples"], float(g[f"fn_{name}/cutoff"]), g[f"fn_{name}/mask"], int(g[f"fn_{name}/num_modes"]), window, str(g[f"fn_{name}/type"])


def test_twin_reproduces_reference_filters(gold):
    g = gold
    names = [str(n) for n in g["fn_names"]]
    assert {"n64_even", "n64_odd", "n64_low", "n64_ones", "n64_few", "n80_hann", "n256", "n1024"} <= set(names)
    for name in names:
        samples, cutoff, mask, K, window, type_ = _fn_args(g, name)
        rows, ref, e_ref = g[f"fn_{name}/rows"], g[f"fn_{name}/ref"], float(g[f"fn_{name}/e_ref"])
        if samples.size <= 256:
            truth, nkeep, sig = twin.null_filter_truth(samples, cutoff, mask, num_modes=K, window=window, type_=type_, full=True)
            truth = truth.astype(np.float64)[rows]
            assert nkeep == int(g[f"fn_{name}/nkeep"])
            assert np.abs(np.asarray(sig, dtype=np.float64) - g[f"fn_{name}/sig"]).max() <= 1e-15 * float(sig.max())
            assert np.abs(truth - g[f"fn_{name}/truth"]).max() <= 1e-15 * np.abs(truth).max()
        else:
            truth = g[f"fn_{name}/truth"]
        e = float(np.abs(ref - truth).max() / np.abs(truth).max())
        print(f"null_filter {name}: twin against the reference {e:.3e}, e_ref {e_ref:.3e}")
        assert e <= 2 * e_ref, (name, e, e_ref)
        rel = g[f"fn_{name}/sig"] / g[f"fn_{name}/sig"].max()
        assert not np.any((rel >= 1e-8 / 1.5) & (rel <= 1.5e-8)), name  # the fixture's input condition


def _vis(s, name, dtype):
    q = s[f"{name}/vis_q"]
    return (q[..., 0] / 64.0 + 1j * (q[..., 1] / 64.0)).astype(dtype)


def test_twin_reproduces_reference_stream(gold):
    s = _load("nullfilter_stream.npz")
    freq, cuts, weight = s["NS/freq"], s["NS/cuts"], s["NS/weight"]
    tv, tw_, infos = twin.filter_items(freq, cuts, _vis(s, "NS", np.complex64), weight, bool(s["NS/window"]))
    e, e_ref = twin.rel_err(s["NS/ref_vis_complex64"], tv), float(s["NS/e_ref_complex64"])
    print(f"stream NS: twin against the reference {e:.3e}, e_ref {e_ref:.3e}")
    assert e <= 2 * e_ref
    assert np.array_equal(tw_, s["NS/ref_weight"])
    assert [i[3] for i in infos] == list(gold["stream_NS/nkeep"]) and [i[1] for i in infos] == list(gold["stream_NS/num_modes"])


def _telescope(feedpos):
    return types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None)


@pytest.mark.parametrize("name", ["NS", "EW", "none"])
def test_stream_bookkeeping(gold, name):
    """Cuts, num_modes, masks and filter sharing of `DelayFilter` against the reference run's."""
    from draco_amd.analysis.delay import DelayFilter, null_filter_plan

    g = gold
    pre = f"stream_{name}"
    delay_cut, za_cut, extra_cut = (float(x) for x in g[f"{pre}/cfg"])
    task = DelayFilter(delay_cut=delay_cut, za_cut=za_cut, extra_cut=extra_cut, telescope_orientation=str(g[f"{pre}/orientation"]), window=bool(g[f"{pre}/window"]))
    task.setup(_telescope(g[f"{pre}/feedpos"]))
    cuts = task._cuts(g[f"{pre}/prod"])
    assert np.allclose(cuts, g[f"{pre}/cuts"], rtol=1e-14, atol=0) and len(np.unique(cuts)) == 3
    weight = g[f"{pre}/weight"]
    flags = np.stack([twin.masks(weight[:, it])[0] for it in range(weight.shape[1])]).astype(np.uint8)
    cut_u, k_u, mask_u, index = null_filter_plan(g[f"{pre}/freq"], g[f"{pre}/cuts"], flags)
    assert np.array_equal(cut_u, g[f"{pre}/cut"]) and np.array_equal(k_u, g[f"{pre}/num_modes"]) and np.array_equal(mask_u != 0, g[f"{pre}/f_mask"])
    assert index[1] == index[4] and len(cut_u) == 4  # entries 1 and 4 share a filter; the all-zero entry 3 has the full mask
    assert flags[3].all() and not flags[2][[10, 20, 33]].any()  # the maximum rule, not all(): channels 10 and 20 fall short
    expect = weight * np.stack([np.outer(*twin.masks(weight[:, it])) for it in range(weight.shape[1])], axis=1)
    assert np.array_equal(expect.astype(np.float32), g[f"{pre}/ref_weight"])


def test_ringmap_bookkeeping(gold):
    """A ring map's item is one el with the samples of both polarisations; the cut varies with el through `_delay_cut`."""
    from draco_amd.analysis.delay import DelayFilterBase, null_filter_plan

    g = gold
    r = _load("nullfilter_ringmap.npz")
    weight = r["w_q"] / 64.0  # [pol, freq, ra, el]
    cuts_el = g["ring/cuts"]

    class VaryingCut(DelayFilterBase):
        def _delay_cut(self, ss, axis, ind):
            return float(cuts_el[ind])

    task = VaryingCut(delay_cut=0.1)
    npol, nfreq, nra, nel = weight.shape
    assert [task._delay_cut(None, "el", e) for e in range(nel)] == list(cuts_el)
    joint = np.moveaxis(weight, (1, 3), (0, 1)).reshape(nfreq, nel, npol * nra)
    flags = np.stack([twin.masks(joint[:, e])[0] for e in range(nel)]).astype(np.uint8)
    cut_u, k_u, mask_u, index = null_filter_plan(g["ring/freq"], np.tile(cuts_el, npol), np.tile(flags, (npol, 1)))
    assert np.array_equal(cut_u, g["ring/cut"]) and np.array_equal(k_u, g["ring/num_modes"]) and np.array_equal(mask_u != 0, g["ring/f_mask"])
    assert np.array_equal(index[:nel], index[nel:]) and flags[6].all() and not np.delete(flags, 6, axis=0)[:, 20].any()


def test_null_filter_errors():
    from draco_amd.util.filters import null_filter

    x, m = 600.0 + 0.4 * np.arange(16), np.ones(16, dtype=bool)
    with pytest.raises(ValueError, match=r"Filter type must be one of \[high, low\]. Got band"):
        null_filter(x, 0.1, m, type_="band")
    with pytest.raises(ValueError, match="num_modes"):
        null_filter(x, 0.1, m, num_modes=0)
    with pytest.raises(NotImplementedError, match="complex"):
        null_filter(x, 0.1, m, num_modes=1)
    with pytest.raises(ValueError, match="1024"):
        null_filter(x, 0.1, m, num_modes=1025)
