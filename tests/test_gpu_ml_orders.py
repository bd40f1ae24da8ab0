"""The maximum-likelihood solve above order 832 against the oracle's SVD.

``dmm_ml_run`` picks its kernels by matrix order (the padded telescope size ``Np = ceil(2 npairs / 64) * 64`` and the
padded sky size of each sky-side tile): two-stage band reduction only up to the largest order whose band fits the LDS
(832, "ml_two_stage_max_order"), one-stage Householder above; the one-stage trailing update with four pending pairs up
to 768, two up to 1536, one up to 2048 and full-matrix sweeps above; the certificate's lower-triangle row sums up to
order 1024.  Every shape below sits on one side of one of those switches:

    case  ntel  Np    reaches
    A      866   896  telescope side one-stage, sky side two-stage at the orders below 832 in the same call
    B     1000  1024  last order of the certificate's lower-triangle-only Gram matrix
    C     1050  1088  first order past it (mirror + full row sums)
    D     1526  1536  the cfg-4/5 telescope: last order of the two-pending-pair trailing update
    E     1590  1600  one pending pair
    F     2100  2112  full-matrix trailing sweeps

Sampled tiles are compared with the float64 SVD solve (``pinv_svd``) on the same B, kept rank and a_lm to 1e-8
relative.  A sample is only taken where the oracle's spectrum keeps its distance from the cut (``_well_separated``):
near it the rank itself is a rounding decision of either side.
"""


import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mapmaker as omm
from oracle import synth as osyn

ACOND, RCOND = 1e-4, 1e-3


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _well_separated(sig, gap=1e-3):
    """No singular value within a relative ``gap`` of pinv_svd's threshold (exact zeros -- masked rows -- are far)."""
    t = max(RCOND * sig.max(), ACOND)
    return bool(np.all(np.abs(sig / t - 1.0) > gap))


class _Case:
    """One telescope (one frequency, ntel = 2 npairs, m = 0 .. mmax), host-made data on the device, an engine."""

    def __init__(self, npairs, lmax, mmax, seed):
        import torch

        from draco_amd import _lib
        from draco_amd.analysis._solve import SolveEngine
        from draco_amd.core.products import SyntheticProvider, TransitTelescope
        from draco_amd.device import Context

        self.ctx = Context.get()
        self.npairs, self.lmax, self.mmax, self.seed = npairs, lmax, mmax, seed
        self.ntel = 2 * npairs
        self.np_tel = (self.ntel + 63) // 64 * 64
        tel = TransitTelescope(osyn.frequencies(1), lmax=lmax, ncyl=1, nfeed_cyl=3, npairs=npairs)
        assert tel.npairs == npairs
        tel.mmax = mmax
        self.tel = tel
        self.bt = SyntheticProvider(tel, seed=seed)
        rng = np.random.default_rng(seed)
        shape = (mmax + 1, 2, 1, npairs)
        self.mv_h = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        self.mw_h = rng.uniform(5.0, 35.0, shape)
        self.mw_h[rng.uniform(size=shape) < 0.02] = 0.0
        self.mv = torch.from_numpy(self.mv_h).to(self.ctx.device)
        self.mw = torch.from_numpy(self.mw_h).to(self.ctx.device)
        self.eng = SolveEngine(self.bt, self.ctx, _lib.DMM_C128, _lib.DMM_B_PACKED)
        self._oracle = {}

    def nsky(self, m):
        return 4 * (self.lmax + 1 - m)

    def order(self, m):
        """Padded order of tile m's Gram matrix: telescope side if nsky >= ntel, sky side otherwise."""
        return self.np_tel if self.nsky(m) >= self.ntel else (self.nsky(m) + 63) // 64 * 64

    def ml(self, **opts):
        """One ML pass under the given options (restored to 0 after): a_lm [npol, mmax+1, lmax+1], the kept rank per m
        (-1: not eigen-decomposed), and the counters that say which path ran."""
        import torch

        from draco_amd import _lib
        from draco_amd.device import ptr

        lib, h = _lib.lib, self.ctx.handle
        names = (b"ml_tiles_eigen", b"ml_tiles_direct", b"ml_tiles_ql_failed", b"ml_tiles_basis")
        before = {k: self.ctx.counter(k) for k in names}
        diag = torch.full((1, self.mmax + 1, 4), -1.0, dtype=torch.float64, device=self.ctx.device)
        with self.ctx.options(**opts, profile=1):
            try:
                _lib.check(lib.dmm_ctx_set_ml_diag(h, ptr(diag)))
                out = self.eng.solve("ml", self.mv, self.mw, [0], self.mmax).cpu().numpy()[0]
                self.ctx.sync()
                cnt = {k.decode(): self.ctx.counter(k) - before[k] for k in names}
                for k in (b"band", b"chase", b"tridiag"):
                    cnt[k.decode()] = self.ctx.counter(b"prof_" + k + b"_n")
            finally:
                _lib.check(lib.dmm_ctx_set_ml_diag(h, None))
        return out, diag.cpu().numpy()[0, :, 0].round().astype(int), cnt

    def oracle(self, m):
        if m not in self._oracle:
            bm = osyn.beam_tile(self.seed, m, 0, self.npairs, 4, self.lmax)
            self._oracle[m] = omm.ml_solve_with_spectrum(bm, self.mv_h[m, :, 0], self.mw_h[m, :, 0], ACOND, RCOND)
        return self._oracle[m]

    def check_oracle(self, out, ranks, ms, tol=1e-8):
        """Sampled tiles against the SVD: spectrum clear of the cut, same kept rank (where the tile was decomposed),
        a_lm to ``tol``."""
        for m in ms:
            ref, rank_o, sig = self.oracle(m)
            assert _well_separated(sig), (m, "sample tile too close to the cut")
            if ranks is not None and ranks[m] >= 0:
                assert ranks[m] == rank_o, (m, ranks[m], rank_o)
            err = _rel(out[:, m, :], ref)
            assert err < tol, (m, self.order(m), err)

    def wiener(self, ms, tol=1e-10):
        from draco_amd.analysis.mapmaker import WienerMapMaker

        w = WienerMapMaker()
        out = self.eng.solve("wiener", self.mv, self.mw, [0], self.mmax, prior_amp=w.prior_amp, prior_tilt=w.prior_tilt)
        out = out.cpu().numpy()[0]
        assert np.all(np.isfinite(out))
        for m in ms:
            bm = osyn.beam_tile(self.seed, m, 0, self.npairs, 4, self.lmax)
            ref = omm.wiener_solve(bm, m, self.mv_h[m, :, 0], self.mw_h[m, :, 0], w.prior_amp, w.prior_tilt)
            err = _rel(out[:, m, :], ref)
            assert err < tol, (m, self.order(m), err)


def _same(a, b, ra, rb, tol=1e-9):
    assert np.array_equal(ra, rb)
    assert _rel(a, b) < tol, _rel(a, b)


# ---------------------------------------------------------------- A: Np 896, two-stage below the telescope order
def _case_a():
    c = _Case(433, 230, 230, seed=8660)
    assert c.np_tel == 896 and c.order(14) == 896 and c.order(15) == 896 and c.order(215) == 64
    return c


def test_ml_order_896_one_stage_telescope_side_two_stage_sky_side():
    """ntel 866: the telescope-side tiles (m <= 14) are above the two-stage limit, the sky-side tiles of orders 64 .. 832
    below it -- in the same call, whose dynamic-LDS attributes are set once for its telescope order.  Every tile through
    the tridiagonal path ("ml_eigen" = 4); stage 1 in its three forms ("ml_reduce" 0, 3, 2) and one-stage only (1) keep
    the same ranks and agree to 1e-9, and sampled tiles of every kind agree with the oracle."""
    c = _case_a()
    out, ranks, cnt = {}, {}, {}
    for red in (0, 3, 2, 1):
        out[red], ranks[red], cnt[red] = c.ml(ml_shortcut=2, ml_eigen=4, ml_reduce=red)
    for red in (0, 3, 2):
        k = cnt[red]
        assert k["band"] > 0 and k["chase"] > 0 and k["tridiag"] > 0, (red, k)  # two-stage AND one-stage
    assert cnt[1]["band"] == 0 and cnt[1]["tridiag"] > 0, cnt[1]
    for red in (0, 3, 2, 1):
        assert np.all(np.isfinite(out[red])), red
        assert cnt[red]["ml_tiles_ql_failed"] == 0, (red, cnt[red])
        assert cnt[red]["ml_tiles_eigen"] == c.mmax + 1, (red, cnt[red])
        assert np.all(ranks[red] >= 0), red
    for red in (3, 2, 1):
        _same(out[red], out[0], ranks[red], ranks[0])
    # telescope side (m 0, near-square 14), near-square sky side (15: order 896), two-stage orders 832, 704, 448, 128, 64
    c.check_oracle(out[0], ranks[0], (0, 14, 15, 30, 60, 120, 200, 222))
    assert c.ctx.counter(b"ml_two_stage_max_order") == 832


def test_ml_order_896_eigen_solvers_agree():
    """Case A through the default scheduler ("ml_eigen" = 0: tridiagonal chunks where a list is long enough, blocked
    Jacobi otherwise), through the blocked Jacobi alone (1), and with QL made to give up on every other matrix and those
    redone by Jacobi (3): the same ranks and a_lm to 1e-9, and against the oracle.  The Wiener solve of the same
    telescope (Cholesky at order 896) against its oracle to 1e-10."""
    c = _case_a()
    out, ranks, cnt = {}, {}, {}
    for eig in (0, 1, 3):
        out[eig], ranks[eig], cnt[eig] = c.ml(ml_shortcut=2, ml_eigen=eig)
        assert np.all(np.isfinite(out[eig])), eig
    assert cnt[0]["ml_tiles_ql_failed"] == 0, cnt[0]
    assert cnt[1]["band"] == 0 and cnt[1]["tridiag"] == 0 and cnt[1]["ml_tiles_ql_failed"] == 0, cnt[1]
    assert cnt[3]["ml_tiles_ql_failed"] > 0, cnt[3]  # (the fallback really ran)
    for eig in (1, 3):
        _same(out[eig], out[0], ranks[eig], ranks[0])
    c.check_oracle(out[0], ranks[0], (0, 15, 60))
    c.wiener((0, 14, 15, 60, 200))


def test_ml_order_896_basis_route_declines_above_the_two_stage_limit():
    """``cache_beam_basis`` builds its bases with the two-stage reduction at telescope order: at Np 896 there is none,
    and the option -- an optimisation only -- falls back to the full-order pass: no error, the plain pass's ranks and
    a_lm bit for bit, and no tile through the basis route."""
    import torch

    from draco_amd import _lib
    from draco_amd.analysis.mapmaker import MaximumLikelihoodMapMaker
    from draco_amd.core import containers
    from draco_amd.device import ptr

    c = _case_a()
    mm = containers.MModes(mmax=c.mmax, freq=c.tel.frequencies, stack=c.npairs, allocate=False)
    mm.attach("vis", c.mv)
    mm.attach("vis_weight", c.mw)
    per_f = sum(c.ntel * 4 * (c.lmax + 1 - m) for m in range(c.mmax + 1)) * 16

    def day(based):
        task = MaximumLikelihoodMapMaker(nside=64, pool_bytes=per_f + (1 << 20), cache_beam_basis=based)
        task.setup(c.bt)
        diag = torch.full((1, c.mmax + 1, 4), -1.0, dtype=torch.float64, device=c.ctx.device)
        _lib.check(_lib.lib.dmm_ctx_set_ml_diag(c.ctx.handle, ptr(diag)))
        try:
            out = task.make_alm(mm).cpu().numpy()
            c.ctx.sync()
        finally:
            _lib.check(_lib.lib.dmm_ctx_set_ml_diag(c.ctx.handle, None))
        return out, diag.cpu().numpy()[0, :, 0]

    a_ref, r_ref = day(False)
    b0 = c.ctx.counter(b"ml_tiles_basis")
    a1, r1 = day(True)
    a2, r2 = day(True)  # (a second day: where a basis would be used, not built)
    assert c.ctx.counter(b"ml_tiles_basis") == b0
    assert c.np_tel > c.ctx.counter(b"ml_two_stage_max_order")
    assert np.all(np.isfinite(a1))
    for a, r in ((a1, r1), (a2, r2)):
        assert np.array_equal(r, r_ref)
        assert np.array_equal(a, a_ref)


# ---------------------------------------------------------------- B, C: the certificate's row sums around order 1024
@pytest.mark.parametrize(
    "npairs,lmax,mmax,np_expected,samples",
    [
        (500, 270, 29, 1024, (0, 21, 29)),  # B: last order whose Gram matrix the certificate builds lower-only
        (525, 285, 23, 1088, (0, 12, 23)),  # C: first order past it (telescope side only, see below)
    ],
)
def test_ml_certificate_and_eigen_path_around_order_1024(npairs, lmax, mmax, np_expected, samples):
    """Every tile at one order above the two-stage limit: the default pass (the certificate solves what it can by
    Cholesky, the rejects go through the eigen path) and every tile through the one-stage tridiagonal path, each against
    the other and against the oracle.  C has no sky-side tile: its near-square ones (nsky 1028 .. 1048) are all
    certificate rejects, they go first, and after a batch that certifies nothing the scheduler skips the certificate
    for the telescope-side batch as well."""
    c = _Case(npairs, lmax, mmax, seed=npairs)
    assert c.np_tel == np_expected and all(c.order(m) == np_expected for m in range(mmax + 1))
    assert c.ntel <= c.nsky(0) and (c.nsky(mmax) < c.ntel) == (np_expected == 1024)
    out_d, ranks_d, cnt_d = c.ml()
    out_e, ranks_e, cnt_e = c.ml(ml_shortcut=2, ml_eigen=4)
    assert cnt_d["ml_tiles_direct"] > 0, cnt_d
    assert cnt_e["ml_tiles_direct"] == 0 and cnt_e["ml_tiles_eigen"] == mmax + 1, cnt_e
    assert cnt_e["band"] == 0 and cnt_e["tridiag"] > 0 and cnt_e["ml_tiles_ql_failed"] == 0, cnt_e
    assert cnt_d["band"] == 0, cnt_d
    assert np.all(np.isfinite(out_d)) and np.all(np.isfinite(out_e))
    assert _rel(out_d, out_e) < 1e-9, _rel(out_d, out_e)
    dec = ranks_d >= 0  # (the tiles the default pass decomposed)
    assert np.array_equal(ranks_d[dec], ranks_e[dec])
    c.check_oracle(out_e, ranks_e, samples)
    c.check_oracle(out_d, ranks_d, samples)
    if np_expected == 1088:
        c.wiener(samples)


# ---------------------------------------------------------------- D, E, F: the one-stage trailing-update variants
@pytest.mark.parametrize(
    "npairs,lmax,mmax,np_expected,samples",
    [
        (763, 384, 6, 1536, (0, 3, 6)),  # D: the cfg-4/5 telescope, two pending pairs (last order)
        (795, 399, 4, 1600, (0, 2, 4)),  # E: one pending pair
        (1050, 526, 3, 2112, (0, 2, 3)),  # F: full-matrix trailing sweeps
    ],
)
def test_ml_one_stage_trailing_update_variants(npairs, lmax, mmax, np_expected, samples):
    """Every tile above the two-stage limit (no band reduction), through the tridiagonal path, against the oracle: a
    telescope-side, the square or near-square and a sky-side tile at each order.  At 1536 (the cfg-4/5 telescope) the
    blocked Jacobi and the QL-gives-up fallback too; at 2112 the Wiener solve against its oracle."""
    c = _Case(npairs, lmax, mmax, seed=npairs)
    assert c.np_tel == np_expected and all(c.order(m) == np_expected for m in range(mmax + 1))
    assert c.nsky(mmax) < c.ntel <= c.nsky(0)
    out, ranks, cnt = c.ml(ml_shortcut=2, ml_eigen=4)
    assert cnt["band"] == 0 and cnt["chase"] == 0 and cnt["tridiag"] > 0, cnt
    assert cnt["ml_tiles_ql_failed"] == 0 and cnt["ml_tiles_eigen"] == mmax + 1, cnt
    assert np.all(np.isfinite(out)) and np.all(ranks >= 0)
    c.check_oracle(out, ranks, samples)
    if np_expected == 1536:
        for eig in (1, 3):
            o, r, k = c.ml(ml_shortcut=2, ml_eigen=eig)
            assert np.all(np.isfinite(o)), eig
            assert (k["ml_tiles_ql_failed"] > 0) == (eig == 3), (eig, k)
            _same(o, out, r, ranks)
    if np_expected == 2112:
        c.wiener(samples)
