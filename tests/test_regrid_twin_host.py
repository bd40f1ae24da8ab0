"""CPU tests of the banded and stacker twins in ``tests/regrid_twin.py``, which ``test_gpu_regrid_direct.py`` measures
``csrc/regrid.hip`` against: the float64 restatement of the banded algorithm against the long-double truth at every
case of the sweep (its error sets the GPU bound ``B = 8 e64`` per row), the share of outputs the rounded-once comparison
leaves out (a condition on the inputs: at most 1e-3), the float64 against the long-double mix-down, the stack twin
against the reference's executed vectors bit for bit, the truth against the dense twin, and wrong restatements that
the measures must catch.

``e64 / (2**-52 rowmax)``, worst row, measured here (in every case no output of the restatement differs from the truth
rounded once, and the excluded share is between 0 and 4.3e-4):

    width1 .. width6      121, 165, 207, 151, 277, 336
    clamp4 .. clamp6      149, 47, 63                      (maxspan 85, 106, 126)
    edge1 .. edge129      250, 35, 231, 111, 70, 238, 97
    pad0 / pad1           width 1: 226, 3.0; width 3: 59, 405; pad_task (pad 15) 247
    mix5, mix2            713, 295
    reuse_a, reuse_b      240, 604
    wide                  6.3e7  (B = 1.1e-7 of the row maximum: as large as the float32 rounding)

The angle of the mix-down and mix-up is the float64 product ``omega dphi`` in the truth as in the restatement: that is
the reference's definition (it forms the product in float64 before ``np.exp``) and the kernel's.  With the product
itself in long double the restatement is 2e3 ... 4e3 units off (the product's rounding at 1e4 rad), ``B`` grows
tenfold and the excluded share, which is proportional to ``B``, comes to 3e-3: three times the cap, and not a matter of
the seed.  The stack twin reproduces all 21600 stored values of ``tests/golden/sidereal_stack.npz`` (four keys, four
running states and the final one each) bit for bit.
"""

import os

import numpy as np
import pytest

import regrid_twin as twin
from conftest import GOLDEN

LD = twin.LD


@pytest.mark.parametrize("name", list(twin.REGRID_SWEEP))
def test_restatement_against_truth(name):
    c = twin.RegridCase.get(name)
    tr, ti, tw, B, e64 = c.truth()
    rm = c.rowmax()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(rm > 0, e64 / (LD(2.0**-52) * rm), LD(0))
    print(f"regrid twin {name}: nt {c.nt} maxspan {c.maxspan} e64 / (2**-52 rowmax) worst row {float(ratio.max()):.3g}, B / rowmax {float(8 * 2.0**-52 * ratio.max()):.3g}")
    fr, fi, fw = twin.band_wiener_f64(*c._args())
    wide = c.spec["wide"]
    m = c.check(f"{name} float64", (fr + 1j * fi).astype(np.complex64), fw.astype(np.float32), rounded=not wide)
    assert m["vis_excluded"] <= twin.EXCLUDED_CAP and m["weight_excluded"] <= twin.EXCLUDED_CAP
    # the case is what the sweep says it is
    assert np.all(np.diff(c.times) >= 0) and c.times[0] < 0 and c.times[-1] > 1
    assert not c.weight[0].any() and not tr[0].any() and not tw[0].any()
    if c.nrow > 2:
        assert np.count_nonzero(c.weight[1]) == 1 and tr[1].any()
    if not wide and c.samples >= 16:
        assert c.nrow < 10 or 0.25 <= np.mean(c.weight[2:] == 0) <= 0.35
        assert (c.end == c.start)[c.pad : c.pad + c.samples].any(), "a gap wider than the kernel"
    if not wide:
        assert float(ratio.max()) < 1e4  # (conditioning: the bound stays a bound on rounding, some 1e-12 of the row)
    if name in twin.REGRID_CLAMP_MAXSPAN:
        assert c.maxspan == twin.REGRID_CLAMP_MAXSPAN[name]
    if c.mix is not None:
        assert c.mix[1][-1] == 0 and not tr[-1].any() and not ti[-1].any() and not tw[-1].any()


def test_clamp_and_refusal_regimes():
    """Width 4 at 11 samples per cell stays under the clamp, widths 5 and 6 are clamped, the refused plan is over."""
    ms = {n: twin.RegridCase.get(n).maxspan for n in twin.REGRID_CLAMP_MAXSPAN}
    assert 2 * ms["clamp4"] <= twin.REGRID_TILE_MAX < 2 * ms["clamp5"] < 2 * ms["clamp6"] and ms["clamp6"] <= twin.REGRID_TILE_MAX
    assert twin.RegridCase(twin.REGRID_REFUSED).maxspan > twin.REGRID_TILE_MAX
    assert max(twin.RegridCase.get(f"width{a}").maxspan for a in range(1, 7)) <= 32  # (the tile of 64)


@pytest.mark.parametrize("name", ["mix5", "mix2"])
def test_mix_down_rounds_alike(name):
    """The float64 mix-down (the kernel's) and the long-double one give the same complex64 at every input element."""
    c = twin.RegridCase.get(name)
    a, b = twin._mix_down(c.vis, c.mix, np.float64), twin._mix_down(c.vis, c.mix, LD)
    diff = np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))
    span = np.abs(c.mix[0]).max()
    print(f"regrid twin {name}: {diff} of {2 * a.size} mixed-down components differ, |omega| up to {span:.0f}")
    assert diff == 0 and span > 1.5e3 and c.mix[2].max() > 6.0


@pytest.mark.parametrize("name", ["under_kw5", "over_kw3"])
def test_truth_against_the_dense_twin(name):
    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        g = lambda k: z[f"regrid/{name}/{k}"]  # noqa: E731
        samples, kw, mzw = (int(v) for v in g("cfg"))
        start, end = (float(v) for v in g("bounds"))
        vis, weight, times = g("vis"), g("weight"), g("times")
    xt, nwt = twin.band_wiener_twin(vis, weight, times, samples, start, end, kw, 1e-3, bool(mzw))
    tr, ti, tw = twin.band_wiener_truth(vis, weight, times, samples, start, end, kw, 1e-3, None, bool(mzw))
    top = np.abs(xt).max(axis=1)
    err = np.maximum(np.abs(tr - xt.real).max(axis=1), np.abs(ti - xt.imag).max(axis=1))
    print(f"regrid twin {name}: truth against the dense solve {float((err[top > 0] / top[top > 0]).max()):.3g} of the row maximum")
    assert np.all(err <= 1e-12 * top) and np.all(np.abs(tw - nwt) <= 1e-14 * nwt) and top.any()


def test_pad_argument():
    """``pad = None`` is the tasks' ``5 a``; another pad solves another (smaller) system."""
    c = twin.RegridCase.get("pad_task")
    a5 = twin.band_wiener_truth(c.vis, c.weight, c.times, c.samples, 0.0, 1.0, c.a, twin.EPS, 5 * c.a)
    assert all(np.array_equal(p, q) for p, q in zip(a5, c.truth()[:3]))
    a0 = twin.band_wiener_truth(c.vis, c.weight, c.times, c.samples, 0.0, 1.0, c.a, twin.EPS, 0)
    assert np.abs(a0[2] - a5[2]).max() <= 1e-12 * a5[2].max() and np.abs(a0[0] - a5[0]).max() > 1e-6


# ---- the measures have teeth
def test_measure_catches_a_dropped_band_entry_and_a_small_error():
    c = twin.RegridCase.get("width4")
    tr, ti, tw, B, e64 = c.truth()
    x = (tr + 1j * ti).astype(np.complex64)
    nw = tw.astype(np.float32)
    assert c.measure(x, nw)["vis"] <= 1.0
    # an error of 1e-9 of the row maximum, invisible to a float32 tolerance: the rounded-once comparison sees it
    rm = c.rowmax()[:, None]
    y = ((tr + 1e-9 * rm) + 1j * ti).astype(np.complex64)
    m = c.measure(y, nw)
    assert m["vis_mismatch"] > 0 and np.abs(y - x).max() <= 4 * 2.0**-24 * rm.max()
    # the outermost band entry left out of C: far outside everything
    bw = 2 * c.a - 1
    R = twin.forward_matrix(c.grid, c.times, c.a)
    ng = len(c.grid)
    band = np.abs(np.arange(ng)[:, None] - np.arange(ng)[None, :]) < bw
    k = 5
    C = np.where(band, (R * c.weight[k].astype(np.float64)[None, :]) @ R.T, 0.0)
    xs = np.linalg.solve(C + twin.EPS * np.eye(ng), R @ (c.weight[k] * c.vis[k].astype(np.complex128)))[c.pad : c.pad + c.samples]
    x2 = x.copy()
    x2[k] = xs.astype(np.complex64)
    m = c.measure(x2, nw)
    assert m["vis"] > 1e3 and m["vis_mismatch"] > 0
    # a weight one float32 step off, and a zero that is not one
    nw2 = nw.copy()
    i = np.unravel_index(np.argmax(nw), nw.shape)
    nw2[i] = np.nextafter(nw2[i], np.float32(np.inf))
    assert c.measure(x, nw2)["weight_mismatch"] == 1
    x3 = x.copy()
    assert not x3[0].any()
    x3[0, 3] = 1e-30
    assert c.measure(x3, nw)["vis"] == np.inf


# ---- the stack twin is the reference's arithmetic
@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "sidereal_stack.npz")) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint32}[a.dtype.itemsize]).reshape(-1)


@pytest.mark.parametrize("weight", ["uniform", "inverse_variance"])
@pytest.mark.parametrize("var", [False, True])
def test_stack_twin_reproduces_the_reference_bit_for_bit(gold, weight, var):
    key = f"{weight}_var{int(var)}"
    ndays = int(gold["ndays"])
    days = [(gold[f"day{d}/vis"].reshape(-1), gold[f"day{d}/weight"].reshape(-1), None) for d in range(ndays)]
    states = twin.stack_run(days, weight == "uniform", var, False)
    names = {"vis": "vis", "vis_weight": "weight", "nsample": "nsample", "sample_variance": "sample_variance"}
    compared = 0
    for d, st in enumerate(states):
        tag = f"after{d}" if d < ndays else "final"
        for gname, sname in names.items():
            if f"{key}/{tag}/{gname}" not in gold:
                assert gname == "sample_variance" and not var
                continue
            ref = gold[f"{key}/{tag}/{gname}"]
            got = st[sname].reshape(ref.shape)
            assert got.dtype == ref.dtype
            diff = np.count_nonzero(_bits(got) != _bits(ref))
            assert diff == 0, f"{key} {tag} {gname}: {diff} elements differ"
            compared += ref.size
    print(f"stack twin {key}: {compared} stored values of {len(states)} states reproduced bit for bit")
    assert compared > 0


def test_stack_days_hold_what_the_sweep_says():
    for n in (1, 255, 256, 257, 1000):
        days = twin.stack_days(n)
        assert len(days) == 3 and all(v.dtype == np.complex64 and w.dtype == np.float32 and ns.dtype == np.uint16 and len(v) == n for v, w, ns in days)
        tiny = np.finfo(np.float32).tiny
        for v, w, ns in days:
            for a in (v.real, v.imag, w):
                assert np.all((a == 0) | (np.abs(a) >= tiny)) and np.isfinite(a).all()
    days = twin.stack_days(1000)
    w = np.stack([d[1] for d in days])
    seen = (w > 0).sum(axis=0)
    assert (seen == 0).any() and (seen == 1).any() and (w < 0).any() and (w[0] == 0).any()
    assert ((days[1][2] == 0) & (days[1][1] > 0)).any()
    for uniform in (False, True):
        for with_ns in (False, True):
            states = twin.stack_run(days, uniform, True, with_ns)
            near = np.arange(1000) % 8 >= 6
            # the running mean nearly cancels: a part in a million of the days' values is left
            assert np.abs(states[1]["vis"][near]).max() < 1e-5 * np.abs(days[0][0][near]).max()
            for st in states:
                for k, a in st.items():
                    if a.dtype.kind in "fc":
                        a = a.view(np.float32)
                        assert np.isfinite(a).all() and np.all((a == 0) | (np.abs(a) >= np.finfo(np.float32).tiny)), k
            fin = states[-1]
            assert fin["sample_variance"].any() and not fin["sample_variance"][:, fin["nsample"] <= 1].any()


def test_stack_twin_catches_contraction():
    """The update with its products fused into the sums (what a compiler's contraction would do) is not the twin."""
    days = twin.stack_days(1000)

    def fused_add(st, vis, weight, nsample, uniform, with_var):
        before = {k: v.copy() for k, v in st.items()}
        twin.stack_add_f32(st, vis, weight, nsample, uniform, with_var)
        coeff = weight.astype(np.float64)
        db = (coeff * (vis.real.astype(np.float64) - before["vis"].real)).astype(np.float32).astype(np.float64)
        da = vis.real.astype(np.float64) - st["vis"].real
        st["sample_variance"][0] = (before["sample_variance"][0].astype(np.float64) + db * da).astype(np.float32)  # one rounding

    a = twin.stack_run(days, False, True, False)
    b = twin.stack_run(days, False, True, False, add=fused_add)
    assert np.count_nonzero(_bits(a[-1]["sample_variance"]) != _bits(b[-1]["sample_variance"])) > 50
