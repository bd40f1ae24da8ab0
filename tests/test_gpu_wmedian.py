"""The weighted moving median on the GPU (``dmm_rfi_wmedfilt``) against the sort-based twin of
``tests/chisqmask_twin.py``: the same number at every sample, NaN at the same samples.  The weights of the first plane
of every case are small integers (every partial sum exact, many windows split exactly between two samples), those of
the second are fractions (no window splits exactly but by accident of 1 in 2^50)."""

import numpy as np
import pytest

import chisqmask_twin as twin

pytestmark = pytest.mark.gpu


def _tile():
    from draco_amd import _lib

    return _lib.DMM_RFI_WMED_TILE


def plane(seed, nf, nt, weights="int"):
    """Values on a grid of halves (many duplicates) with negatives, both zeros, both infinities and a NaN; weights by
    kind, about a third of them zero, with a zero block that empties the short windows."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.normal(size=(nf, nt)) * 4.0) / 2.0
    flat = x.reshape(-1)
    for i, v in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan, -0.0)):
        if flat.size > 6 * (i + 1):
            flat[(7 * i + 3) % flat.size] = v
    if weights == "zero":
        w = np.zeros((nf, nt))
    elif weights == "equal":
        w = np.full((nf, nt), 0.75)
    elif weights == "int":
        w = rng.integers(0, 5, size=(nf, nt)).astype(np.float64) * (rng.uniform(size=(nf, nt)) > 0.2)
    else:
        w = rng.uniform(0.1, 3.0, size=(nf, nt)) * (rng.uniform(size=(nf, nt)) > 0.3)
    if weights in ("int", "frac") and nt > 12:
        w[:, nt // 3 : nt // 3 + 9] = 0.0
    return x, w


def shapes():
    T = _tile()
    return [(1, 1), (1, T - 1), (1, T), (1, T + 1), (3, 2 * T + 1), (5, 70), (2, 1300)]


def windows():
    from draco_amd import _lib

    return [(1, 1), (1, 3), (1, 601), (3, 65), (3, 601), (5, 5), (_lib.DMM_RFI_WMED_MAX_WINDOW, 3)]


@pytest.mark.parametrize("ishape", range(7))
@pytest.mark.parametrize("iwin", range(7))
def test_equals_twin(ishape, iwin):
    from draco_amd.util import filters

    nf, nt = shapes()[ishape]
    win = windows()[iwin]
    xa, wa = plane(100 + ishape, nf, nt, "int")
    xb, wb = plane(200 + ishape, nf, nt, "frac")
    x, w = np.stack([xa, xb]), np.stack([wa, wb])  # two planes in one call
    got = filters.moving_weighted_median(x, w, win)
    detail = {}
    want = np.stack([twin.moving_weighted_median(xa, wa, win, detail), twin.moving_weighted_median(xb, wb, win)])
    assert np.array_equal(got, want, equal_nan=True), f"{int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum())} samples differ"
    if (nf, nt) == (2, 1300) and win == (1, 3):
        assert detail["exact"].sum() >= 20 and detail["empty"].sum() >= 5  # the fixtures are there


# windows the list above does not reach: a column of the full 1023 rows, more than 640 columns per output
@pytest.mark.parametrize("nf,nt,win", [(1100, 5, (1023, 3)), (2, 1300, (1, 1023)), (8, 1100, (7, 1001)), (40, 96, (101, 31))])
def test_long_windows(nf, nt, win):
    from draco_amd.util import filters

    x, w = plane(300 + nf, nf, nt, "int")
    assert np.array_equal(filters.moving_weighted_median(x, w, win), twin.moving_weighted_median(x, w, win), equal_nan=True)


@pytest.mark.parametrize("kind", ["zero", "equal"])
def test_zero_and_equal_weights(kind):
    from draco_amd.util import filters

    x, w = plane(7, 5, 70, kind)
    got = filters.moving_weighted_median(x, w, (3, 65))
    assert np.array_equal(got, twin.moving_weighted_median(x, w, (3, 65)), equal_nan=True)
    if kind == "zero":
        assert np.isnan(got).all()


@pytest.mark.parametrize("win", [(5, 21), (21, 5)])
def test_bit_equal_to_medfilt_with_01_weights(win):
    from draco_amd.util import filters

    rng = np.random.default_rng(11)
    x, _ = plane(12, 40, 96, "int")
    mask = rng.uniform(size=x.shape) < 0.3
    mask[13] = True
    mask[:, 20:50] |= rng.uniform(size=(40, 30)) < 0.6
    a = filters.moving_weighted_median(x, (~mask).astype(np.float64), win)
    b = filters.medfilt(x, mask, win)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_one_dimension_and_device_tensors():
    import torch

    from draco_amd.device import Context
    from draco_amd.util import filters

    x, w = plane(5, 70, 1, "int")
    want = twin.moving_weighted_median(x[:, 0], w[:, 0], 9)
    assert np.array_equal(filters.moving_weighted_median(x[:, 0], w[:, 0], 9), want, equal_nan=True)
    ctx = Context.get()
    out = filters.moving_weighted_median(ctx.to_device(x[:, 0]), ctx.to_device(w[:, 0]), 9)
    assert isinstance(out, torch.Tensor) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)


def test_bounds():
    from draco_amd import _lib
    from draco_amd.device import Context, ptr
    from draco_amd.util import filters

    x, w = plane(1, 5, 70, "int")
    with pytest.raises(ValueError, match="odd"):
        filters.moving_weighted_median(x, w, (2, 3))
    with pytest.raises(ValueError, match="bound"):
        filters.moving_weighted_median(x, w, (1, _lib.DMM_RFI_WMED_MAX_WINDOW + 2))
    with pytest.raises(ValueError, match="bound"):
        filters.moving_weighted_median(x, w, (101, 101))
    wn = w.copy()
    wn[2, 3] = -1.0
    with pytest.raises(ValueError, match="non-negative"):
        filters.moving_weighted_median(x, wn, (1, 3))
    for size in ((1, 601), (3, 601), (101, 31)):  # the task's defaults and the windows of the sensitivity mask
        assert filters.check_weighted_size(size, 2) == size
    ctx = Context.get()
    xd, wd = ctx.to_device(x), ctx.to_device(w)
    out = ctx.empty(x.shape, np.float64)
    assert _lib.lib.dmm_rfi_wmedfilt(ctx.handle, ptr(xd), ptr(wd), 1, 5, 70, 4, 3, ptr(out)) == _lib.DMM_E_ARG
    assert _lib.lib.dmm_rfi_wmedfilt(ctx.handle, ptr(xd), ptr(wd), 1, 5, 70, 1025, 3, ptr(out)) == _lib.DMM_E_ARG
