"""Host-side checks of ``tests/dirty_twin.py`` (no GPU): the long-double reference is the contraction it claims to be,
the float64 twin stays inside the rigorous bound, the acceptance rule rejects what it is there to reject, and the
tile-table helpers speak the device layouts."""

import numpy as np
import pytest

import dirty_twin as dt


def _inputs(rng, ntel, ncol, b_dtype=dt.C128, zero_frac=0.1):
    B = dt.random_tile(rng, ntel, 1, ncol, b_dtype).reshape(ntel, ncol)
    v = rng.standard_normal(ntel) + 1j * rng.standard_normal(ntel)
    Ni = rng.uniform(0.5, 1.5, ntel)
    Ni[rng.uniform(size=ntel) < zero_frac] = 0.0
    a = rng.standard_normal(ncol) + 1j * rng.standard_normal(ncol)
    return B, v, Ni, a


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63 and np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("ntel,ncol", [(2, 1), (6, 5), (22, 21), (64, 84)])
@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64])
def test_reference_is_the_contraction(ntel, ncol, b_dtype):
    B, v, Ni, a = _inputs(np.random.default_rng(ntel * 100 + ncol), ntel, ncol, b_dtype)
    d = dt.ref_dirty(B, v, Ni)
    p = dt.ref_project(B, a)
    assert d.dtype == np.clongdouble and p.dtype == np.clongdouble
    assert dt.rel_max(np.einsum("ij,i->j", B.conj(), Ni * v), d) < 1e-13
    assert dt.rel_max(np.einsum("ij,j->i", B, a), p) < 1e-13
    # and it is better than float64: two orders of summation agree with it far below 2^-53 of each other's error
    assert dt.rel_max(dt.ref_dirty(B[::-1], v[::-1], Ni[::-1]), d) < 1e-17


def test_reference_keeps_what_float64_loses():
    """1 + 2^-60 - 1: float64 answers 0, the reference 2^-60."""
    B = np.array([[1.0], [2.0**-60], [-1.0]], dtype=np.complex128)
    one = np.ones(3)
    assert dt.ref_dirty(B, one + 0j, one)[0].real == np.longdouble(2.0) ** -60
    assert dt.twin_dirty(B, one + 0j, one)[0].real == 0.0
    assert dt.ref_project(B.T, one + 0j)[0].real == np.longdouble(2.0) ** -60
    assert dt.twin_project(B.T, one + 0j)[0].real == 0.0


@pytest.mark.parametrize("ntel", [2, 6, 16, 46, 758, 1526])
@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64])
def test_twin_inside_the_rigorous_bound(ntel, b_dtype):
    ncol = 300 if ntel < 700 else 2052
    B, v, Ni, a = _inputs(np.random.default_rng(ntel), ntel, ncol, b_dtype)
    ref, twin, bound = dt.ref_dirty(B, v, Ni), dt.twin_dirty(B, v, Ni), dt.bound_dirty(B, v, Ni)
    frac = (dt.err_inf(twin, ref) / bound).max()
    assert frac <= 1.0
    # the twin against itself through the rule (ratio 1), and what the rule reports
    st = dt.accept(twin, ref, twin, bound, "twin")
    assert st["ratio"] == 1.0 and st["frac"] == frac and st["e_twin"] < 4e-14
    if ntel >= 758:
        assert frac < 0.01  # the bound alone is loose at full size: the reason for the sharp criterion
    Bp = B.T.copy()  # [ntel' = ncol, ncol' = ntel]: a projection of the same length
    ap = Ni * v
    refp, twinp, boundp = dt.ref_project(Bp, ap), dt.twin_project(Bp, ap), dt.bound_project(Bp, ap)
    assert (dt.err_inf(twinp, refp) <= boundp).all()
    dt.accept(twinp, refp, twinp, boundp, "twin project")


@pytest.mark.parametrize("ntel,ncol", [(6, 400), (46, 400), (1526, 4100)])
def test_rule_passes_another_float64_order_and_rejects_1e13(ntel, ncol):
    """An independently rounded float64 evaluation (BLAS order) passes; the same with a relative error of 1e-13 on one
    output -- far inside the rigorous bound at full size -- does not."""
    B, v, Ni, _ = _inputs(np.random.default_rng(7 + ntel), ntel, ncol)
    ref, twin, bound = dt.ref_dirty(B, v, Ni), dt.twin_dirty(B, v, Ni), dt.bound_dirty(B, v, Ni)
    other = B.conj().T @ (Ni * v)
    st = dt.accept(other, ref, twin, bound, "blas")
    assert st["ratio"] < 4.0
    bad = other.copy()
    k = int(np.argmax(np.abs(ref)))
    bad[k] *= 1.0 + 1e-13
    if ntel == 1526:
        assert (dt.err_inf(bad, ref) <= bound).all()  # (a) alone lets it through: (b) has to catch it
    with pytest.raises(AssertionError, match="e_got" if ntel == 1526 else "e_got|rigorous bound"):
        dt.accept(bad, ref, twin, bound, "perturbed")
    with pytest.raises(AssertionError, match="rigorous bound"):
        bad[k] *= 1.0 + 1e-9
        dt.accept(bad, ref, twin, bound, "perturbed more")
    nan = other.copy()
    nan[0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        dt.accept(nan, ref, twin, bound, "nan")


def test_all_zero_input_must_come_out_exactly_zero():
    B, v, Ni, _ = _inputs(np.random.default_rng(3), 8, 5)
    Ni[:] = 0.0
    ref, twin, bound = dt.ref_dirty(B, v, Ni), dt.twin_dirty(B, v, Ni), dt.bound_dirty(B, v, Ni)
    assert not ref.any() and not twin.any() and not bound.any()
    dt.accept(np.zeros(5, complex), ref, twin, bound)
    with pytest.raises(AssertionError):
        dt.accept(np.full(5, 1e-300 + 0j), ref, twin, bound)


@pytest.mark.parametrize("b_layout", [dt.PACKED, dt.FULL])
@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64])
def test_tile_table_round_trip_against_synth_shaped_tiles(b_layout, b_dtype):
    """Tiles shaped like ``synth_beam_tile`` ([2, npairs, npol, lmax + 1], zero for l < m) go into the pool and come back;
    the expected outputs equal the dense contraction over the square arrays."""
    from draco_amd.core.products import synth_beam_tile

    npairs, npol, lmax, nfreq, n_m = 5, 3, 9, 3, 12
    ms, fs = [4, 0, 9, 4, 7], [2, 1, 0, 0, 2]
    sq = [synth_beam_tile(17, m, f, npairs, npol, lmax) for m, f in zip(ms, fs)]
    Bs = [dt.device_values(s.reshape(2 * npairs, npol, lmax + 1)[:, :, m:], b_dtype) for s, m in zip(sq, ms)]
    offs = dt.layout_tiles(ms, npairs, npol, lmax, b_layout, gaps=[3, 0, 8, 2, 1], order=[2, 0, 4, 1, 3])
    case = dt.Case(npairs, npol, lmax, nfreq, n_m, zip(ms, fs, offs), Bs, b_dtype, b_layout)
    pool = case.pool(tail=6)
    assert pool.dtype == dt.NP_DTYPE[b_dtype] and pool.size >= case.nelem + 6
    # every element of every tile is where the kernels look for it, everything else is NaN
    seen = np.zeros(pool.size, dtype=bool)
    for (m, f, o), s in zip(case.tiles, sq):
        ncolrow = npol * (lmax + 1 - (m if b_layout == dt.PACKED else 0))
        pol_stride, col0 = ncolrow // npol, (m if b_layout == dt.FULL else 0)
        flat = s.reshape(2 * npairs, npol, lmax + 1)
        for i in (0, npairs, 2 * npairs - 1):
            for pol in range(npol):
                for l in (m, lmax):
                    at = o + i * ncolrow + pol * pol_stride + col0 + (l - m)
                    assert pool[at] == flat[i, pol, l].astype(dt.NP_DTYPE[b_dtype])
        view = pool[o : o + 2 * npairs * ncolrow].reshape(2 * npairs, npol, -1)
        mark = seen[o : o + 2 * npairs * ncolrow].reshape(2 * npairs, npol, -1)
        assert not mark.any()
        mark[:, :, col0:] = True
        assert np.isnan(view[:, :, :col0]).all()
    assert np.isnan(pool[~seen]).all() and not np.isnan(pool[seen]).any()
    assert all(np.array_equal(a, b.astype(dt.NP_DTYPE[b_dtype])) for a, b in zip(case.unpool(pool), Bs))

    rng = np.random.default_rng(5)
    mvis = rng.standard_normal(case.vis_shape()) + 1j * rng.standard_normal(case.vis_shape())
    mw = rng.uniform(0.5, 1.5, case.vis_shape())
    exp = case.expected_alm(mvis, mw)
    alm_in = rng.standard_normal(case.alm_shape()) + 1j * rng.standard_normal(case.alm_shape())
    expv = case.expected_vis(alm_in)
    listed = set(zip(ms, fs))
    for f in range(nfreq):
        for m in range(n_m):
            if (m, f) not in listed:
                assert np.all(exp["ref"][f, :, m, :] == dt.SENTINEL) and not exp["owned"][f, :, m].any() and not exp["zero"][f, :, m].any()
                assert np.all(expv["ref"][m, :, f, :] == dt.SENTINEL) and not expv["owned"][m, :, f].any()
                continue
            B = dt.device_values(sq[list(zip(ms, fs)).index((m, f))], b_dtype).reshape(2 * npairs, npol, lmax + 1)
            w = (mw[m, :, f, :] * mvis[m, :, f, :]).reshape(-1)
            dense = np.einsum("ipl,i->pl", B.conj(), w)  # zero for l < m by the tile's own zeros
            assert dt.rel_max(exp["ref"][f, :, m, :], dense) < 1e-13 and dt.rel_max(exp["twin"][f, :, m, :], dense) < 1e-13
            assert exp["owned"][f, :, m, m:].all() and exp["zero"][f, :, m, :m].all() and not exp["owned"][f, :, m, :m].any()
            assert np.all(exp["ref"][f, :, m, :m] == 0)
            densev = np.einsum("ipl,pl->i", B, alm_in[f, :, m, :]).reshape(2, npairs)  # l < m of alm_in meets zeros of B
            assert dt.rel_max(expv["ref"][m, :, f, :], densev) < 1e-13 and dt.rel_max(expv["twin"][m, :, f, :], densev) < 1e-13
    # the launch check: the twin passes, a written sentinel / a non-zero structural zero / a NaN do not
    got = exp["twin"].copy()
    dt.check_launch(got, exp)
    for where, msg in ((~(exp["owned"] | exp["zero"]), "outside the tile list"), (exp["zero"], "structural zeros")):
        bad = got.copy()
        bad[tuple(np.argwhere(where)[0])] = 1e-30
        with pytest.raises(AssertionError, match=msg):
            dt.check_launch(bad, exp)
    bad = got.copy()
    bad[tuple(np.argwhere(exp["owned"])[0])] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        dt.check_launch(bad, exp)
    dt.check_launch(expv["twin"], expv)


def test_case_rejects_overlap_and_duplicates():
    B = dt.random_tile(np.random.default_rng(0), 4, 1, 3, dt.C128)
    with pytest.raises(AssertionError, match="overlap"):
        dt.Case(2, 1, 2, 2, 1, [(0, 0, 0), (0, 1, 5)], [B, B])
    with pytest.raises(AssertionError, match="twice"):
        dt.Case(2, 1, 2, 2, 1, [(0, 0, 0), (0, 0, 12)], [B, B])


def test_days_at_once_equal_day_by_day():
    rng = np.random.default_rng(11)
    Bs = [dt.random_tile(rng, 14, 2, 6 - m, dt.C64) for m in (0, 5, 2)]
    case = dt.Case(7, 2, 5, 2, 6, [(0, 1, 0), (5, 0, 200), (2, 0, 300)], Bs, dt.C64)
    days = [(rng.standard_normal(case.vis_shape()) + 1j * rng.standard_normal(case.vis_shape()), rng.uniform(0, 1, case.vis_shape())) for _ in range(3)]
    many = case.expected_alm_days([v for v, _ in days], [w for _, w in days])
    for (v, w), e in zip(days, many):
        one = case.expected_alm(v, w)
        assert all(np.array_equal(one[k], e[k]) for k in ("ref", "twin", "bound", "owned", "zero"))
