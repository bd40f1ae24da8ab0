"""The blocked float64 Cholesky solver of ``csrc/chol_blocked.hip`` (``dl_factor``, ``dl_solve_rows``), addressed directly
through ``dmm_mfilter_solve``, against the long-double truth of ``tests/chol_twin.py``; and ``k_mf_cov`` and the three
filter builders at the orders the task-level tests leave out.

Measures (``chol_twin.py`` derives them).  Backward, primary: ``|G x - y| <= 2 gamma_{3n+1} |U|^T |U| |x|`` elementwise,
the residual formed in long double and ``U`` the twin's factor; printed as the worst ratio of residual to bound, at most
1 passes.  Forward, secondary: ``e_gpu = max |x - x*| / max |x*| <= max(4 e_ref, n 2**-52)`` per matrix, ``e_ref`` the
same measure of the float64 reference (``numpy.linalg.cholesky`` and two triangular solves); the factor left in the
upper triangle of ``G`` likewise against ``numpy.linalg.cholesky``'s.  Every ``G`` goes to the GPU with NaN in its strict
lower triangle.  Each test prints its figures before it asserts.

Measured on an MI355X, per case of the sweep, the largest value over the three matrices (``cond`` = 1e2, 1e6, 1e10);
``e_ref`` and ``e_ref_U`` are the CPU's (``test_chol_twin_host.py`` tabulates them without a GPU; they move in the second
digit with the host's LAPACK):

    (n, nrow)    e_ref     e_gpu     e_gpu / limit   residual / bound   e_ref_U    e_U
    (1, 1)       3.1e-16   3.1e-16   0.25            2.9e-01            0.0e+00    0.0e+00
    (1, 257)     3.0e-16   2.0e-16   0.50            3.6e-01            0.0e+00    0.0e+00
    (2, 3)       2.8e-08   1.1e-08   0.25            4.5e-02            9.5e-13    3.8e-13
    (31, 64)     5.6e-08   2.7e-08   0.27            6.0e-03            1.6e-12    2.0e-12
    (32, 65)     2.2e-08   1.3e-08   0.23            7.4e-03            2.5e-12    2.7e-12
    (33, 1)      5.0e-08   1.8e-08   0.39            3.5e-03            3.6e-12    1.0e-12
    (63, 255)    3.4e-08   3.5e-08   0.51            4.8e-03            4.1e-12    5.4e-12
    (64, 256)    6.1e-08   4.9e-08   0.30            4.7e-03            4.0e-12    4.0e-12
    (65, 257)    5.6e-08   2.8e-08   0.24            4.6e-03            3.9e-12    3.6e-12
    (95, 63)     4.6e-08   5.4e-08   0.62            2.5e-03            5.2e-12    8.2e-12
    (96, 64)     9.0e-08   3.4e-08   0.23            2.5e-03            8.0e-12    4.0e-12
    (97, 65)     4.1e-08   6.4e-08   0.39            2.3e-03            4.5e-12    4.4e-12
    (128, 3)     7.5e-08   4.6e-08   0.20            1.7e-03            6.5e-12    4.1e-12
    (129, 513)   7.9e-08   7.4e-08   0.23            2.2e-03            1.1e-11    1.3e-11
    (257, 129)   1.1e-07   5.3e-08   0.12            8.6e-04            1.2e-11    5.3e-12

(``e_gpu / limit``: the worst matrix's ``e_gpu / max(4 e_ref, n 2**-52)``, at most 1 passes; it is the ``cond = 1e6`` matrix at
order 95, ``e_gpu`` 1.3e-11 against ``e_ref`` 5.1e-12.  The residual stays two orders below its bound from order 31 on; at
order 1, where the bound is 8 u, it reaches 0.36 of it, the reference 0.46.)

Status isolation (order 97, good matrices 0, 2, 5): ``e_gpu`` 2.6e-15, 6.0e-8, 3.8e-8 against ``e_ref`` 1.7e-15, 3.1e-8,
5.5e-8; residual / bound at most 2.1e-3; status ``[0, 1, 0, 1, 1, 0]``.  Row chunks (``2**21 + 257`` rows, ``cond`` 1e2 and
1e10): order 1 ``e_gpu`` 2.2e-16, 2.7e-16 (``e_ref`` 1.1e-16, 2.7e-16), residual / bound 0.42 over all rows, 0.24 at the
chunk boundary, 0.34 in the last 257 rows; order 3 ``e_gpu`` 1.2e-15, 1.3e-8 (``e_ref`` 2.1e-15, 4.3e-8), residual / bound
0.12, 0.027, 0.050.  The order-3 case takes 1.4 s, the whole file 5.5 s.

``k_mf_cov``, ``e_ref_cov = max |float64 twin - truth| / |coef|`` off the diagonal, on the CPU: between 3.1e-16 and 4.3e-16 at
orders 255, 256, 257; ``e_gpu`` between 3.1e-16 and 4.2e-16, never above ``e_ref_cov`` by more than 1 %.

Builders (``epsilon = 1e-10``), ``e_ref`` of the float64 restatement (``numpy.linalg.pinv``) / ``e_gpu``, at ``nra`` = 31, 33,
65: band-pass 5.6e-9 / 1.1e-9, 2.5e-8 / 5.7e-8, 2.1e-8 / 3.2e-8; low-pass 2.4e-6 / 2.7e-6, 6.6e-6 / 1.4e-6, 1.9e-5 / 4.8e-6;
high-pass 1.3e-5 / 9.4e-7, 5.1e-6 / 2.6e-6, 9.0e-6 / 4.4e-6; high-pass at ``nra = 1``: 0 / 1.3e-16 (the floor is 2.2e-16).
At ``nra = 1`` the low-pass and band-pass covariances have no RA spacing to take their ``a = median(dra) m_cut / pi`` from:
the truth is NaN, and the builders are required to refuse (``ValueError``) rather than return it; the high-pass one is
compared as at the other orders.
"""

import numpy as np
import pytest

import chol_twin as ct
import mfilter_twin as twin

pytestmark = pytest.mark.gpu

CHUNK = 1 << 21  # kMfRowChunk of mfilter.hip


def _solve(G, Y, status=None):
    """``dmm_mfilter_solve`` on host arrays: ``(G, Y, status)`` as the call leaves them."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    nmat, nrow, n = Y.shape
    assert G.shape == (nmat, n, n)
    G_d, Y_d = ctx.to_device(G, np.float64), ctx.to_device(Y, np.float64)
    st = ctx.zeros((nmat,), np.int32) if status is None else ctx.to_device(status, np.int32)
    _lib.check(_lib.lib.dmm_mfilter_solve(ctx.handle, n, nrow, nmat, ptr(G_d), ptr(Y_d), ptr(st)))
    return G_d.cpu().numpy(), Y_d.cpu().numpy(), st.cpu().numpy()


def _assert_solution(name, case, t, x, rows=slice(None)):
    """Section 2 on the solution ``x`` of matrix ``t`` of ``case``."""
    e_gpu, ratio = case.measure(t, x, rows)
    e_ref = case.e_ref[t]
    print(f"chol {name} matrix {t}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} residual / bound {ratio:.3e}")
    assert np.isfinite(x[rows]).all(), (name, t)
    assert ratio <= 1.0, (name, t, ratio)
    assert e_gpu <= ct.forward_limit(e_ref, case.n), (name, t, e_gpu, e_ref)
    return e_gpu, ratio


@pytest.mark.parametrize("shape", ct.SWEEP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_solve_sweep(shape):
    n, nrow = shape
    case = ct.Case(n, nrow)
    g, x, status = _solve(case.poisoned(), case.Y)
    assert not status.any(), status
    iu = np.triu(np.ones((n, n), dtype=bool))
    for t in range(case.nmat):
        _assert_solution(f"sweep {shape}", case, t, x[t])
        ut = case.U[t].astype(np.float64)
        e_u = float(np.abs(g[t][iu] - ut[iu]).max() / np.abs(ut).max())
        print(f"chol sweep {shape} matrix {t}: e_U {e_u:.3e} e_ref_U {case.e_ref_u[t]:.3e}")
        assert np.isfinite(g[t][iu]).all()
        assert e_u <= ct.forward_limit(case.e_ref_u[t], n), (shape, t, e_u, case.e_ref_u[t])


def test_status_isolation():
    """Six matrices of order 97 (a one-row last block), three of them bad in three ways; the good ones are solved as if
    alone, the bad ones keep their right-hand sides."""
    from draco_amd import _lib

    n, nrow = 97, 65
    case = ct.Case(n, nrow, conds=(1e2, 1e6, 1e10, 1e2, 1e6, 1e10), seed=[20261018, 6])
    good, bad = [0, 2, 5], [1, 3, 4]
    g = case.poisoned()
    g[1, 0, 0] = -1.0  # the first pivot of block 0
    g[3, 96, 96] = float(ct.LD(g[3, 96, 96]) - ct.schur_pivot_ld(g[3], 96) - 1)  # the only pivot of the last block: -1
    assert abs(float(ct.schur_pivot_ld(g[3], 96)) + 1.0) < 1e-6 and float(ct.schur_pivot_ld(g[3], 95)) > 0
    g[4, 40, 40] = np.nan
    _, x, status = _solve(g, case.Y)
    print(f"chol isolation: status {status.tolist()}")
    ok, fail = _lib.DMM_MFILTER_OK, _lib.DMM_MFILTER_NOT_POSDEF
    assert status.tolist() == [ok, fail, ok, fail, fail, ok]
    for t in bad:
        assert np.array_equal(x[t].view(np.uint64), case.Y[t].view(np.uint64)), t
    for t in good:
        _assert_solution("isolation", case, t, x[t])
    _, alone, status = _solve(np.ascontiguousarray(g[good]), np.ascontiguousarray(case.Y[good]))
    assert not status.any()
    assert np.array_equal(alone.view(np.uint64), x[good].view(np.uint64))


@pytest.mark.parametrize("n", [1, 3])
def test_row_chunks(n):
    """More rows than one pass of the solves takes: the second pass starts at row ``2**21`` of every matrix."""
    nrow = CHUNK + 257
    case = ct.Case(n, nrow, conds=(1e2, 1e10), small=True)
    _, x, status = _solve(case.poisoned(), case.Y)
    assert not status.any(), status
    for t in range(case.nmat):
        for name, rows in (("all rows", slice(None)), ("chunk boundary", slice(CHUNK - 2, CHUNK + 2)), ("last 257 rows", slice(nrow - 257, nrow))):
            _assert_solution(f"row chunks n = {n}, {name}", case, t, x[t], rows)


# ---- k_mf_cov element by element

COV_ORDERS = (1, 255, 256, 257)
COV_KINDS = (("lowpass", 7.2, 0.0), ("bandpass", 3.6, 6.0), ("lowpass", 11.5, 0.0))
COV_EPS = 1e-10


def _cov_inputs(n):
    """``(ra, masks [3][n], repeated pair or None)``: an irregular grid, about 10 % of each mask dropped (the only RA
    of order 1 in matrix 1), one RA value repeated at two indices every mask keeps."""
    rng = np.random.default_rng([20261018, 5, n])
    ra = np.sort(np.radians(np.linspace(0.0, 360.0, max(n, 2), endpoint=False)) + rng.uniform(0.0, 0.01, size=max(n, 2)))[:n]
    masks = rng.uniform(size=(3, n)) >= 0.10
    pair = None
    if n == 1:
        masks[:] = [[True], [False], [True]]
    else:
        pair = [n // 3, n - 2]
        ra[pair[1]] = ra[pair[0]]
        masks[:, pair] = True
        masks[:, 0] = [True, False, True]
    return ra, masks, pair


def _cov_params(ra, kind, m_cut, m_center):
    from draco_amd.analysis.dayenu import _mmode_params

    # (order 1 has no spacing of its own: the covariance's parameters are then those of a 1 degree grid)
    return _mmode_params(ra if ra.size > 1 else np.radians([0.0, 1.0]), kind, m_cut, m_center, COV_EPS)


def _cov_truth(ra, masks, pars, truth):
    """The twin's covariance of each matrix, extended by the identity on the masked rows and columns; order 1, where
    the twin has no spacing, is its one kept element ``diag + coef``."""
    out = []
    for (kind, m_cut, m_center), mask, par in zip(COV_KINDS, masks, pars):
        T = ct.LD if truth else np.float64
        c = twin.covariance(ra, kind, m_cut, m_center, COV_EPS, truth=truth) if ra.size > 1 else np.array([[T(par[0]) + T(par[1])]])
        keep = mask[:, np.newaxis] & mask[np.newaxis, :]
        out.append(np.where(keep, c, np.eye(ra.size, dtype=T)))
    return np.stack(out)


@pytest.mark.parametrize("n", COV_ORDERS)
def test_cov_elements(n):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ra, masks, pair = _cov_inputs(n)
    pars = np.array([_cov_params(ra, *k) for k in COV_KINDS])
    assert np.isfinite(pars).all() and pars[1, 3] != 0 and pars[0, 2] != pars[2, 2]
    ctx = Context.get()
    G = ctx.empty((3, n, n), np.float64)
    status = ctx.to_device(np.full(3, 7, dtype=np.int32))
    ra_d, par_d, mask_d = ctx.to_device(ra), ctx.to_device(pars), ctx.to_device(masks.astype(np.uint8))
    _lib.check(_lib.lib.dmm_mfilter_cov(ctx.handle, n, 3, ptr(ra_d), ptr(par_d), ptr(mask_d), ptr(G), ptr(status)))
    g, st = G.cpu().numpy(), status.cpu().numpy()
    assert not st.any()
    truth, ref = _cov_truth(ra, masks, pars, True), _cov_truth(ra, masks, pars, False)
    eye = np.eye(n, dtype=bool)
    for t in range(3):
        diag, coef = pars[t, 0], pars[t, 1]
        keep = masks[t][:, np.newaxis] & masks[t][np.newaxis, :]
        assert 0.05 * n <= np.count_nonzero(~masks[t]) <= 0.2 * n or n == 1
        assert np.array_equal(g[t][~keep], np.eye(n)[~keep])  # masked rows and columns: the identity, exactly
        assert np.array_equal(np.diag(g[t])[masks[t]], np.full(np.count_nonzero(masks[t]), coef + diag))
        rest = keep & ~eye
        if pair is not None:
            assert g[t][pair[0], pair[1]] == coef and g[t][pair[1], pair[0]] == coef
            rest[pair[0], pair[1]] = rest[pair[1], pair[0]] = False
        if not rest.any():
            continue
        e_gpu = float(np.abs(g[t] - truth[t])[rest].max() / abs(coef))
        e_ref = float(np.abs(ref[t] - truth[t])[rest].max() / abs(coef))
        print(f"mfilter cov n = {n} matrix {t}: e_gpu {e_gpu:.3e} e_ref_cov {e_ref:.3e}")
        assert np.isfinite(g[t]).all()
        assert e_gpu <= 4 * e_ref, (n, t, e_gpu, e_ref)


# ---- the builders at small orders

FN_PARS = {"bandpass": (3.6, 6.0), "lowpass": (7.2, 0.0), "highpass": (7.2, 0.0)}
FN_EPS = 1e-10


def _fn_flag(nra):
    """``flag (2, 3, nra)``: two different masks with flagged RAs, and one that keeps nothing."""
    m = np.ones((3, nra), dtype=bool)
    m[0, :: max(2, nra // 4)] = False
    m[1, nra // 2 :] = nra == 1
    m[1, -1] = True
    m[2] = False
    return np.stack([m[[0, 2, 1]], m[[1, 0, 0]]])


@pytest.mark.parametrize("nra", [1, 31, 33, 65])
@pytest.mark.parametrize("kind", ["bandpass", "lowpass", "highpass"])
def test_functions_small_orders(kind, nra):
    from draco_amd.analysis import dayenu

    ra = np.radians(np.linspace(0.0, 360.0, nra, endpoint=False))
    flag = _fn_flag(nra)
    mc, m0 = FN_PARS[kind]
    run = (lambda: dayenu.bandpass_mmode_filter(ra, m0, mc, flag, epsilon=FN_EPS)) if kind == "bandpass" else (lambda: getattr(dayenu, f"{kind}_mmode_filter")(ra, mc, flag, epsilon=FN_EPS))
    if nra == 1 and kind != "highpass":
        with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
            assert not np.isfinite(twin.covariance(ra, kind, mc, m0, FN_EPS, truth=True)).any()  # no spacing, no truth
            with pytest.raises(ValueError):
                run()
        return
    pinv, index = run()
    truth, tindex = twin.mmode_filter_truth(ra, kind, mc, m0, flag, FN_EPS)
    ref = twin.mmode_filter_f64(ra, kind, mc, m0, flag, FN_EPS)[0]
    nuniq = len(np.unique(flag.reshape(-1, nra), axis=0))
    assert pinv.is_cuda and tuple(pinv.shape) == (nuniq, nra, nra) == truth.shape and nuniq == (3 if nra > 1 else 2)
    assert len(index) == len(tindex) == nuniq
    for ind, tind in zip(index, tindex):
        assert isinstance(ind, tuple) and len(ind) == 2 and all(np.array_equal(a, b) for a, b in zip(ind, tind))
    p = pinv.cpu().numpy()
    t64 = truth.astype(np.float64)
    e_gpu, e_ref = twin.rel_err(p, t64), twin.rel_err(ref, t64)
    print(f"mfilter fn {kind} nra = {nra}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e}")
    assert p.dtype == np.float64 and np.isfinite(p).all()
    assert np.array_equal(p == 0, t64 == 0)
    assert not p[0].any() and not flag.reshape(-1, nra)[index[0][0][0] * 3 + index[0][1][0]].any()  # keeps nothing: all zero
    assert e_gpu <= max(2 * e_ref, 2.0**-22), (kind, nra, e_gpu, e_ref)
    assert e_gpu <= max(4 * e_ref, nra * 2.0**-52), (kind, nra, e_gpu, e_ref)
