"""The consumer of the ring-map chain, ``csrc/ringmap.hip`` (``dmm_ringmap_deconvolve``, ``dmm_ringmap_window``), and the
analytic beam in front of it (``dmm_analytic_beam_mmodes``), each addressed directly through its entry point, against the
long-double truth of ``tests/ringmap_twin.py``.

Measures (``ringmap_twin.py`` derives them).  ``map`` and ``dirty_beam``: per row (pol, freq, el) ``max_ra |got - T| /
max_ra |T|``, the largest over the rows of a case; ``weight`` and ``dirty_beam_power``: relative error per element.
Accepted where ``e_gpu <= K e_ref + K 2**-53`` with ``e_ref`` the same figure of ``oracle.ringmap.deconvolve`` (float64) on
the same inputs, ``K = 4`` for a radix row transform and 8 through Bluestein.  Where the truth is zero the output is
zero; ``weight`` is the same bits along RA; every output buffer is NaN before the call and finite after it.  The float32
stores (window, analytic beam) are the truth rounded once wherever the truth is far enough from a rounding boundary.
Each test prints ``e_gpu``, ``e_ref`` and their ratio before it asserts.

Every shape runs in the three weight modes, each with another variety of input (``ringmap_twin.VARIETIES``): an elevation
profile of 6, 12 or 0 decades, no window / a random one / one that vanishes on a row, an excluded EW separation, ``eps``
mixed over fifteen decades or zero, a (pol, freq) without weight.

Measured on an MI355X, per row of the case tables (``ringmap_twin.THREE_KERNEL``, ``SKIP``, ``SINGLE_PASS``, ``TILE_MAP``) and
form -- ``3k``: three kernels, pair 2 without and pair 1 with the RA-space dirty beam; ``single 16`` / ``single 8``: the single
pass with 16 / 8 elevations per block.  Per output: the largest ``e_gpu``, the largest ``e_ref``, and the largest share of
the limit ``K e_ref + K 2**-53`` any case of the row reaches (at most 1 passes), over its shapes, modes and varieties:

    form          row            map                    weight                 dirty_beam_power       dirty_beam
    3k pair 2     shortest       1.4e-15 6.4e-16 0.31   6.7e-16 8.5e-16 0.62   4.2e-16 5.3e-16 0.50   -
    3k pair 1     shortest       8.4e-16 6.4e-16 0.29   6.7e-16 8.5e-16 0.62   7.2e-16 5.3e-16 0.41   9.6e-16 2.6e-16 0.45
    3k pair 2     chunks         3.9e-15 1.5e-14 0.48   1.0e-14 3.0e-14 0.22   8.3e-16 1.8e-15 0.18   -
    3k pair 1     chunks         4.9e-15 1.5e-14 0.39   1.0e-14 3.0e-14 0.22   1.9e-15 1.8e-15 0.23   2.3e-15 6.1e-16 0.49
    3k pair 2     terms          6.2e-16 7.2e-16 0.40   1.4e-15 9.3e-16 0.47   6.4e-16 6.8e-16 0.43   -
    3k pair 1     terms          6.2e-16 7.2e-16 0.40   1.4e-15 9.3e-16 0.47   6.4e-16 6.8e-16 0.43   3.7e-16 2.9e-16 0.27
    3k pair 2     bluestein      3.1e-15 7.4e-16 0.46   6.6e-16 1.6e-15 0.11   6.8e-16 2.0e-15 0.11   -
    3k pair 1     bluestein      3.4e-15 7.4e-16 0.50   6.6e-16 1.6e-15 0.11   7.2e-16 2.0e-15 0.10   1.0e-15 5.3e-16 0.30
    3k pair 2     long           4.2e-16 1.6e-15 0.19   5.3e-16 6.4e-15 0.21   2.2e-16 5.6e-15 0.01   -
    3k pair 1     long           4.0e-16 1.6e-15 0.21   5.3e-16 6.4e-15 0.21   3.5e-16 5.6e-15 0.03   2.8e-16 1.4e-15 0.31
    3k pair 2     twiddles       5.5e-16 1.9e-15 0.13   4.4e-16 8.5e-15 0.03   4.8e-16 3.2e-15 0.13   -
    3k pair 1     twiddles       5.5e-16 1.9e-15 0.13   4.4e-16 8.5e-15 0.03   6.6e-16 3.2e-15 0.09   2.3e-16 1.9e-15 0.26
    3k pair 2     bluestein8192  1.6e-15 1.7e-15 0.22   4.9e-15 2.8e-15 0.35   4.0e-16 7.6e-15 0.01   -
    3k pair 1     bluestein8192  3.8e-15 1.7e-15 0.54   4.9e-15 2.8e-15 0.35   4.8e-16 7.6e-15 0.02   5.1e-16 1.5e-15 0.32
    3k pair 2     beam           7.1e-16 5.5e-16 0.41   7.1e-16 7.1e-16 0.31   6.2e-16 1.3e-15 0.23   -
    3k pair 1     beam           7.9e-16 5.5e-16 0.35   7.1e-16 7.1e-16 0.31   5.1e-16 1.3e-15 0.18   4.1e-16 4.8e-16 0.23
    skip pair 2   shortest       9.3e-16 6.4e-16 0.28   4.9e-16 7.4e-16 0.76   4.1e-16 9.9e-16 0.50   -
    skip pair 1   shortest       1.0e-15 6.4e-16 0.41   4.9e-16 7.4e-16 0.76   4.3e-16 9.9e-16 0.50   1.1e-15 4.5e-16 0.30
    skip pair 2   chunks         3.4e-15 9.6e-16 0.64   1.2e-15 2.0e-15 0.28   1.2e-15 2.1e-15 0.17   -
    skip pair 1   chunks         2.5e-15 9.6e-16 0.53   1.2e-15 2.0e-15 0.28   2.6e-15 2.1e-15 0.30   2.6e-15 1.0e-15 0.49
    skip pair 2   terms          8.2e-16 7.3e-16 0.43   9.2e-16 1.0e-15 0.47   9.5e-16 1.1e-15 0.54   -
    skip pair 1   terms          6.4e-16 7.3e-16 0.34   9.2e-16 1.0e-15 0.47   1.0e-15 1.1e-15 0.65   5.7e-16 5.2e-16 0.48
    skip pair 2   bluestein      1.4e-15 8.7e-16 0.34   8.3e-16 1.9e-15 0.15   6.7e-16 2.4e-15 0.11   -
    skip pair 1   bluestein      1.9e-15 8.7e-16 0.36   8.3e-16 1.9e-15 0.15   1.6e-15 2.4e-15 0.25   1.3e-15 7.9e-16 0.33
    skip pair 2   long           4.3e-16 3.2e-15 0.13   3.9e-16 6.8e-15 0.12   5.0e-16 6.9e-15 0.08   -
    skip pair 1   long           4.5e-16 3.2e-15 0.15   3.9e-16 6.8e-15 0.12   8.6e-16 6.9e-15 0.08   2.8e-16 2.9e-15 0.15
    single 16     shortest       5.2e-16 6.3e-16 0.32   9.2e-16 1.1e-15 0.34   6.3e-16 5.0e-16 0.27   -
    single 8      shortest       5.2e-16 6.3e-16 0.32   9.2e-16 1.1e-15 0.34   6.3e-16 5.0e-16 0.27   -
    single 16     second_pass    1.4e-14 2.6e-14 0.39   1.5e-14 2.8e-14 0.23   9.3e-16 3.2e-15 0.16   -
    single 8      second_pass    1.4e-14 2.6e-14 0.39   1.6e-14 2.8e-14 0.21   9.0e-16 3.2e-15 0.16   -
    single 16     lds16          8.4e-16 1.9e-15 0.24   4.4e-16 3.5e-15 0.17   4.6e-16 2.9e-15 0.05   -
    single 16     parked         2.2e-15 7.4e-15 0.43   4.5e-15 1.1e-14 0.10   1.0e-15 9.1e-15 0.05   -
    single 8      parked         2.2e-15 7.4e-15 0.43   4.5e-15 1.1e-14 0.10   8.1e-16 9.1e-15 0.04   -
    single 16     tile mapping   7.5e-16 7.3e-16 0.26   1.0e-15 1.3e-15 0.23   8.2e-16 8.3e-16 0.26   -
    single 8      tile mapping   7.5e-16 7.3e-16 0.26   1.0e-15 1.3e-15 0.23   8.2e-16 8.3e-16 0.26   -

(the figures of 1e-14 and more all belong to mode 1: where a negative weight outweighs the others of its sign, that sign's
normalised weights turn negative, as the reference's do, and a mode's ``sum_w`` partly cancels between the two signs; map and
weight share the loss, and the oracle loses two to three times as much).  Window: no element outside the rule at any shape
or coefficient set; not held to equality 0 (uniform), 2.2e-4 (hann) and 8.7e-4 (nuttall) of the 4607 elements compared of
the large table.  Analytic beam (``nra``, ``mmax``, ``nel``, ``nfreq``): no component differs or is outside its tolerance in any
case; near a rounding boundary 1.0e-5 of the components of (2049, 1024, 1, 2), none in the others; the imaginary parts --
sums that cancel, held to an absolute bound only -- are 0.25 of the components of (1, 0, 1, 2), 0.40 of (8, 4, 5, 2), 0.49 of
(39, 19, 5, 2), (128, 64, 5, 2) and (128, 40, 1, 2), 0.50 of (2049, 1024, 1, 2) and 0.375 of (39, 25, 5, 2).  The stale-scratch
and repeatability runs are bit for bit.  The whole file takes 5.9 s, 1.7 s of it the first call's start-up and 1.4 s the
long-double DFT of the ``nra = 2049`` beam; no other test takes more than 0.12 s.

What this sweep found, and ``ringmap.hip`` now does: two real sequences that share one complex transform (two rows' map
modes, or a row's map and dirty-beam modes) came out with the larger one's absolute error -- ``e_gpu`` up to 2.6e-7 on a
weak row beside a strong one, and values of 1e-16 of the partner where a row without beam has to be zero under
``skip_deconvolution``; each sequence now enters its transform divided by a power of two near its norm.  And a window with
``hi < lo`` was not empty.
"""

import ctypes as C
import time

import numpy as np
import pytest

import ringmap_twin as rt

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()
_MEMO = {}


@pytest.fixture(scope="module", autouse=True)
def _file_time():
    yield
    _MEMO.clear()
    print(f"ringmap direct: the file took {time.perf_counter() - T0:.1f} s")


def _truth(case):
    """The long-double truth and the float64 oracle's outputs of a case, computed once per module run and left unchanged."""
    if case.name not in _MEMO:
        _MEMO[case.name] = (case.truth(), case.reference())
    return _MEMO[case.name]


def _nan(ctx, shape, dtype):
    import torch

    t = ctx.empty(shape, dtype)
    t.fill_(complex(np.nan, np.nan) if t.is_complex() else np.nan)
    torch.cuda.synchronize()
    return t


def _deconvolve(case, variant, dirty, hv=None, expect=None):
    """``dmm_ringmap_deconvolve`` on the inputs of ``case`` (``hv``: other visibilities of the same shape) into buffers full of
    NaN: ``(map, weight, dirty_beam_power, dirty_beam or None)`` as NumPy arrays.  ``expect``: the exception the call is to
    raise (a pair ``(type, match)``); the buffers come back as the call left them."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    c = case
    dev = [ctx.to_device(a) for a in (c.hv if hv is None else hv, c.hw, c.bv)]
    wt, eps = ctx.to_device(c.wt, np.float64), ctx.to_device(c.eps, np.float64)
    win = None if c.window is None else ctx.to_device(c.window)
    rmap = _nan(ctx, (1, c.npol, c.nfreq, c.nra, c.nel), np.float64)
    rwgt = _nan(ctx, (c.npol, c.nfreq, c.nra, c.nel), np.float64)
    rdbp = _nan(ctx, (1, c.npol, c.nfreq, c.nel), np.float64)
    rdb = _nan(ctx, (1, c.npol, c.nfreq, c.nra, c.nel), np.float64) if dirty else None

    def call():
        with ctx.options(ringmap_variant=variant):
            _lib.check(_lib.lib.dmm_ringmap_deconvolve(ctx.handle, c.nm, c.nm_beam, c.npol, c.nfreq, c.new, c.nel, c.nra, c.mode, int(c.skip), c.iref,
                                                       ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(wt), ptr(eps), ptr(win), ptr(rmap), ptr(rwgt),
                                                       ptr(rdbp), ptr(rdb)))

    if expect is None:
        call()
    else:
        with pytest.raises(expect[0], match=expect[1]):
            call()
    ctx.sync()
    return tuple(None if x is None else x.cpu().numpy() for x in (rmap, rwgt, rdbp, rdb))


def _check(case, variant, dirty, who):
    T, ref = _truth(case)
    got = _deconvolve(case, variant, dirty)
    return rt.compare(case, T, ref if dirty else ref[:3] + (None,), got, who)


def _flat(tables):
    return [pytest.param(shape, i, id=f"{k}{i}-nm{shape[0]}") for k, shapes in tables.items() for i, shape in enumerate(shapes)]


# ---- the three-kernel form
@pytest.mark.parametrize("shape,index", _flat(rt.THREE_KERNEL))
def test_three_kernel_form(shape, index):
    """``k_rm_reduce``, ``k_rm_fft<2>`` (two rows per transform, the dirty-beam power by Parseval) and ``k_rm_fft<1>`` (the
    RA-space dirty beam asked for), ``k_rm_store``; forced by ``ringmap_variant = 1`` where the single pass would take the call."""
    for case in rt.cases_of(shape, index):
        for dirty in (False, True):
            _check(case, 1, dirty, "three-kernel pair " + "21"[dirty])


@pytest.mark.parametrize("shape,index", _flat(rt.SKIP))
def test_skip_deconvolution(shape, index):
    """``C = 1`` and every row normalised by row ``iref``: the first, the middle and the last elevation."""
    nel = shape[2]
    for iref in sorted({0, nel // 2, nel - 1}):
        for case in rt.cases_of(shape, index, skip=True, iref=iref):
            for dirty in (False, True):
                _check(case, 0, dirty, "skip pair " + "21"[dirty])


@pytest.mark.parametrize("nm,oddra", rt.UNSUPPORTED)
def test_unsupported_lengths(nm, oddra):
    """Rows too long for the in-LDS transform: the call raises, names the length and writes nothing."""
    from draco_amd import _lib

    case = rt.Case(nm, oddra, 1, 1)
    for dirty in (False, True):
        got = _deconvolve(case, 0, dirty, expect=(_lib.DmmError, f"nra={case.nra}"))
        assert all(a is None or np.isnan(a).all() for a in got)


# ---- the single-pass forms
@pytest.mark.parametrize("shape,index", _flat(rt.SINGLE_PASS))
def test_single_pass_forms(shape, index):
    """``k_rm_fused<16, false>`` (``nra <= 1024``), ``<16, true>`` (2048: the second eight elevations parked) under variant 0 and
    ``<8, false>`` under variant 2, against the truth itself."""
    nm, nel, new, variants = shape
    for case in rt.cases_of((nm, False, nel, new, 1, 1, None), index):
        for variant in variants:
            _check(case, variant, False, f"single-pass variant {variant}")


@pytest.mark.parametrize("nel,npol,nfreq", rt.TILE_MAP, ids=lambda x: str(x))
def test_eight_elevation_tile_mapping(nel, npol, nfreq):
    """1, 2, 15, 16, 17 and 33 tiles under the block -> tile mapping of the 8-elevation form (pairs of tiles 8 ids apart,
    the grid rounded up to 16): every tile written exactly once."""
    index = rt.TILE_MAP.index((nel, npol, nfreq))
    case = rt.cases_of((9, False, nel, 1, npol, nfreq, None), index)[index % 3]
    _check(case, 2, False, "tile-map variant 2")
    _check(case, 0, False, "tile-map variant 0")


# ---- stale scratch, repeatability
@pytest.mark.parametrize("which", ["three-kernel", "parked"])
def test_stale_scratch_and_repeatability(which):
    """The largest three-kernel case and the largest parked case: two plain runs give the same bits, and so does a run
    right after a call of the same shape whose ``hv`` is all NaN -- the modes, ``tmp_map`` and the parked image are NaN then."""
    if which == "three-kernel":
        case, variant = rt.cases_of(rt.THREE_KERNEL["twiddles"][0], 0)[0], 1
    else:
        nm, nel, new, _ = rt.SINGLE_PASS["parked"][-1]
        case, variant = rt.cases_of((nm, False, nel, new, 1, 1, None), 0)[0], 0
    first = _deconvolve(case, variant, False)
    again = _deconvolve(case, variant, False)
    poison = _deconvolve(case, variant, False, hv=np.full(case.hv.shape, complex(np.nan, np.nan), np.complex64))
    assert np.isnan(poison[0]).any()
    after = _deconvolve(case, variant, False)
    for a, b, c in zip(first[:3], again[:3], after[:3]):
        assert np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "two plain runs differ"
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64)), "a run after NaN in the scratch differs"


# ---- the window
@pytest.mark.parametrize("shape", rt.WINDOW_CASES, ids=lambda s: "x".join(map(str, s)))
def test_window(shape):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    nfreq, nm, nel = shape
    lo, hi = rt.window_limits(*shape)
    lo_d, hi_d = ctx.to_device(lo, np.float64), ctx.to_device(hi, np.float64)
    index = rt.window_index(*shape)
    for name, coef in rt.WINDOW_COEF.items():
        out = _nan(ctx, shape, np.float32)
        _lib.check(_lib.lib.dmm_ringmap_window(ctx.handle, nfreq, nm, nel, ptr(lo_d), ptr(hi_d), (C.c_double * 4)(*[float(a) for a in coef]), ptr(out)))
        ctx.sync()
        got = out.cpu().numpy().reshape(-1)
        assert np.isfinite(got).all()
        mismatch, near = rt.window_measure(got[index], lo, hi, coef, nm, index)
        print(f"ringmap direct window {shape} {name}: mismatch {mismatch} of {len(index)}, not held to equality {near:.3g}")
        assert mismatch == 0 and near <= rt.EXCLUDED_CAP, (name, mismatch, near)
        full = got.reshape(shape)
        if nel >= 5:  # the empty windows: hi < lo, and lo == hi
            assert not full[:, :, 1].any() and not full[:, :, 4].any()


# ---- the analytic beam
@pytest.mark.parametrize("shape", rt.BEAM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_analytic_beam(shape):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    nra, mmax, nel, nfreq = shape
    inp = rt.beam_inputs(*shape)
    out = _nan(ctx, (mmax + 1, 2, len(rt.POLS), nfreq, len(inp[1]), nel), np.complex64)
    tabs = [ctx.to_device(x, np.float64) for x in inp]
    _lib.check(_lib.lib.dmm_analytic_beam_mmodes(ctx.handle, len(rt.POLS), nfreq, len(inp[1]), nel, nra, mmax, *(ptr(t) for t in tabs), ptr(out)))
    ctx.sync()
    got = out.cpu().numpy()
    assert np.isfinite(got.view(np.float32)).all()
    Tr, Ti, B = rt.analytic_beam_truth(*inp, nra, mmax)
    mismatch, loose, near, noise = rt.analytic_beam_measure(got, Tr, Ti, B, nra)
    print(f"ringmap direct beam {shape}: mismatch {mismatch} loose {loose} near {near:.3g} noise {noise:.3g} of {2 * got.size} components")
    assert mismatch == 0 and loose == 0 and near <= rt.EXCLUDED_CAP
