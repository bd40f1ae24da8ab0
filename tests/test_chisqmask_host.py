"""Host-side checks of the chi-squared mask path (no GPU): the twin's weighted median on hand cases and against the
reference-executed vectors of ``tests/golden/chisqmask.npz``, the baseline fit, what the wrappers and tasks refuse, the
bookkeeping of the reduced container, the task's defaults and the presence of the new entry points."""

import os
import types
import warnings

import numpy as np
import pytest

import chisqmask_twin as twin
from draco_amd import _lib
from draco_amd.analysis import flagging, transform
from draco_amd.core import containers
from draco_amd.util import filters, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chisqmask.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_twin_hand_cases():
    x = [1.0, 2.0, 3.0, 4.0]
    assert twin.weighted_median_1(x, [1, 1, 1, 1]) == 2.5
    assert twin.weighted_median_1(x, [3, 1, 1, 1]) == 1.5  # the split is exact at the first sample
    assert twin.weighted_median_1(x, [4, 1, 1, 1]) == 1.0
    assert twin.weighted_median_1(x, [1, 1, 1, 0]) == 2.0
    assert twin.weighted_median_1([2.0, 2.0, 5.0, 7.0], [1, 1, 1, 1]) == 3.5  # equal samples count as one step of c(v)
    assert twin.weighted_median_1([2.0, 2.0, 5.0, 7.0], [1, 1, 2, 1]) == 5.0
    assert np.isnan(twin.weighted_median_1(x, [0, 0, 0, 0]))
    assert twin.weighted_median_1([np.nan, 1.0, 2.0], [1, 1, 1]) == 2.0  # NaN sorts above everything
    out = twin.moving_weighted_median(np.array([[1.0, 2.0, 3.0, 4.0]]), np.array([[3.0, 1.0, 1.0, 1.0]]), (1, 3))
    assert np.array_equal(out, [[1.0, 1.0, 3.0, 3.5]])  # windows clipped at the edge, no padding
    assert twin.weighted_median(np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[0.0, 0.0], [1.0, 0.0]])).tolist() == [0.0, 3.0]


def test_twin_with_01_weights_is_the_masked_median():
    import rfi_twin

    rng = np.random.default_rng(3)
    x = np.round(rng.normal(size=(9, 31)) * 3) / 2
    keep = rng.uniform(size=x.shape) < 0.6
    keep[:, 10:17] = False
    a = twin.moving_weighted_median(x, keep.astype(float), (3, 5))
    assert np.array_equal(a, rfi_twin.moving_weighted_median(x, keep, (3, 5)), equal_nan=True)


def test_twin_replays_the_reference_steps(gold):
    for name in ("mad_t21", "st_t21"):
        y, w, m = gold[f"step/{name}/y"], gold[f"step/{name}/w"], gold[f"step/{name}/m"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.array_equal(twin.mask_1d(y, m), gold[f"step/{name}/mask_1d"])
        assert np.array_equal(twin.mask_2d(y, w, win=(1, 21)), gold[f"step/{name}/mask_2d"])
    assert np.array_equal(twin.mask_2d_sumthreshold(y, w, win=(1, 21)), gold["step/st_t21/mask_2d_sumthreshold"])


def test_golden_margins(gold):
    for name in gold["case/names"]:
        assert float(gold[f"case/{name}/margin"]) > 1e-9
        assert 0.0 < gold[f"case/{name}/mask"].mean() < 1.0
    for key in ("in/ts/w", "in/hyb/w"):
        w = gold[key]
        assert np.array_equal(w, np.round(w)) and w.min() >= 0 and w.max() < 2**10


def test_window_check():
    for size in ((1, 601), (3, 601), (101, 31), (1023, 3), (1, 1023)):
        assert filters.check_weighted_size(size, 2) == size
    assert filters.check_weighted_size(9, 1) == (9, 1)
    for size in ((2, 3), (3, 0), (1, -3), (1025, 1), (1, 1025), (101, 101)):
        with pytest.raises(ValueError):
            filters.check_weighted_size(size, 2)
    with pytest.raises(ValueError, match="does not match"):
        filters.check_weighted_size((3, 3, 3), 2)
    T = _lib.DMM_RFI_WMED_TILE
    assert _lib.DMM_RFI_WMED_MAX_STRIP * 16 + (T + _lib.DMM_RFI_WMED_MAX_WINDOW - 1) * 4 <= 160 * 1024  # the LDS of a CU


def test_median_refuses_before_it_touches_the_device():
    x, w = np.zeros((4, 6)), np.ones((4, 6))
    with pytest.raises(ValueError, match="odd"):
        filters.moving_weighted_median(x, w, (2, 3))
    with pytest.raises(ValueError, match="shape"):
        filters.moving_weighted_median(x, w[:, :5], (1, 3))
    with pytest.raises(ValueError, match="real"):
        filters.moving_weighted_median(x + 0j, w, (1, 3))
    for bad in (-1.0, np.nan):
        wb = w.copy()
        wb[1, 2] = bad
        with pytest.raises(ValueError, match="non-negative"):
            filters.moving_weighted_median(x, wb, (1, 3))


def test_arpls_against_the_reference(gold):
    for k in range(int(gold["arpls/n"])):
        y, m, lam = gold[f"arpls/{k}/y"], gold[f"arpls/{k}/mask"], float(gold[f"arpls/{k}/lam"])
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            z = tools.arPLS_1d(y, mask=m, lam=lam)
        np.testing.assert_allclose(z, gold[f"arpls/{k}/z"], rtol=1e-10, atol=0)
        if m.all():  # the early return
            assert not z.any() and any("Entire dataset is masked" in str(c.message) for c in caught)
    with pytest.raises(ValueError, match="1D data"):
        tools.arPLS_1d(np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="reweighting"):
        tools.penalized_least_squares_1d(np.arange(8.0), lambda d, m: d)


def test_arpls_follows_a_baseline_under_spikes():
    f = np.arange(128)
    base = 1.0 + 0.3 * np.sin(f / 20.0)
    sigma = 0.02  # (the weights are scaled by the scatter of the residuals: the data needs some)
    y = base + sigma * np.random.default_rng(5).normal(size=128)
    y[[10, 50, 51, 90]] += 5.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z = tools.arPLS_1d(y, lam=1e2)
    assert np.abs(z - base).max() < 3 * sigma  # a smoother's error stays below the scatter of one sample


def _stream(nf=4, ns=3, nt=5):
    s = containers.TimeStream(freq=np.linspace(800, 799, nf), stack=ns, time=1.6e9 + np.arange(nt))
    s.attrs["tag"] = "x"
    return s


def test_reduce_container_bookkeeping():
    s = _stream()
    task = transform.ReduceChisq(axes=["stack"], dataset="vis")
    out = task._make_output_container(s)
    assert type(out) is containers.TimeStream
    assert out.index_map["stack"].tolist() == [s.index_map["stack"][0]] and len(out.index_map["freq"]) == 4
    assert out.attrs["reduced"] is True and out.attrs["reduction_axes"].tolist() == ["stack"]
    assert out.attrs["reduced_dataset"] == "vis" and out.attrs["reduction_op"] == "chisq_per_dof" and out.attrs["tag"] == "x"
    assert transform.ReduceVar._op == "variance" and transform.ReduceBase._op is None
    assert task.weighting == "none"
    with pytest.raises(ValueError, match="weighting"):
        transform.ReduceVar(axes=["stack"], dataset="vis", weighting="other")


def test_reduce_errors():
    s = _stream()
    with pytest.raises(ValueError, match="At least one axis"):
        transform.ReduceChisq(axes=["freq", "stack", "time"], dataset="vis").process(s)
    with pytest.raises(NotImplementedError, match="adjacent"):
        transform.ReduceChisq(axes=["freq", "time"], dataset="vis").process(s)
    m = containers.Map(freq=np.linspace(800, 799, 4), nside=2)
    for weighting in ("masked", "weighted"):
        with pytest.raises(RuntimeError, match="No weights available"):
            transform.ReduceVar(axes=["pol"], dataset="map", weighting=weighting).process(m)
    with pytest.raises(NotImplementedError):
        transform.ReduceBase().reduction(None, None, (0, 0))


def test_merged_strides():
    assert transform._merged_strides((2, 3, 4), (12, 4, 1)) == [(24, 1)]
    assert transform._merged_strides((3, 4), (33, 0)) == [(3, 33), (4, 0)]
    assert transform._merged_strides((1, 5, 1), (0, 7, 0)) == [(5, 7)]
    assert transform._merged_strides((2, 2), (0, 0)) == [(4, 0)]
    assert transform._merged_strides((1,), (0,)) == []


def test_task_defaults_and_refusals():
    t = flagging.RFIMaskChisqHighDelay()
    want = dict(flag_ew=None, reg_arpls=1e5, nsigma_1d=5.0, win_t=601, win_f=1, nsigma_2d=5.0, estimate_var=False, only_positive=False, separate_pol=False, mask_type="mad",
                niter=5, rho=1.5, max_m=32)
    for k, v in want.items():
        assert getattr(t, k) == v or (v is None and getattr(t, k) is None), k
    assert t.MAD_TO_RMS == 1.48625
    from draco_amd import analysis

    assert analysis.RFIMaskChisqHighDelay is flagging.RFIMaskChisqHighDelay and analysis.ReduceChisq is transform.ReduceChisq
    with pytest.raises(ValueError, match="mask_type"):
        flagging.RFIMaskChisqHighDelay(mask_type="combine")
    st = flagging.RFIMaskChisqHighDelay(mask_type="sumthreshold", nsigma_2d=4.0, niter=3, rho=2.0)
    st.setup()
    assert st.threshold.tolist() == [16.0, 8.0, 4.0] and st.telescope is None
    assert not t._day_flag_hook(np.arange(5.0)).any() and t._source_flag_hook(np.arange(5.0), np.arange(3.0)).shape == (3, 5)

    sid = containers.SiderealStream(freq=np.linspace(800, 799, 4), stack=2, ra=8)
    t.setup()
    with pytest.raises(RuntimeError, match="must provide telescope"):
        t.process(sid)
    t.setup(types.SimpleNamespace(lmax=1, mmax=1, frequencies=None, lsd_to_unix=lambda lsd: 86164.0 * np.asarray(lsd)))
    with pytest.raises(ValueError, match="`csd` or `lsd`"):
        t.process(sid)


def test_abi_presence():
    for name in ("dmm_rfi_wmedfilt", "dmm_rfi_wdev", "dmm_axis_reduce"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    header = open(os.path.join(ROOT, "include", "draco_amd.h")).read()
    for name in ("DMM_RFI_WMED_MAX_WINDOW", "DMM_RFI_WMED_MAX_STRIP", "DMM_RFI_WMED_TILE"):
        assert f"#define {name} {getattr(_lib, name)}\n" in header
    # argument checks run before anything touches a device
    assert _lib.lib.dmm_rfi_wmedfilt(None, None, None, 1, 4, 4, 1, 3, None) == _lib.DMM_E_ARG
    assert _lib.lib.dmm_axis_reduce(None, 0, 0, None, 1, 1, 1, None, 0, 0, 1, 0, 0, 0, 1.0, None, None) == _lib.DMM_E_ARG
    assert _lib.lib.dmm_rfi_wdev(None, None, None, None, 4, None, None) == _lib.DMM_E_ARG
