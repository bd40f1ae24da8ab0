"""``tests/sht_twin.py`` without a GPU: the float64 restatement is the oracle, the long-double truth reproduces the
definition-level and SciPy checks of ``test_oracle_sht.py``, the geometry is the library's, the backstop's accounting
is fair for every case of the sweep, and the cases reach what they were chosen for.

Measured here (``error / backstop`` of the float64 restatement, the largest over a case's elements; its relative
distance from the truth in units of ``max|T|``):

    synthesis  S0a    S0b    S1     S2a    S2b    S3     S4     S5     S6     S7      S8a    S8b
    usage      0.008  0.026  0.017  0.049  0.037  0.064  0.087  0.082  0.127  0.0004  0.111  0.052
    distance   4e-17  4e-16  7e-16  2e-15  5e-15  9e-15  1e-14  2e-13  3e-13  4e-14   2e-11  2e-15

    analysis   A0     A1 (0, 1, 3 steps)    A2 (0, 2)     A3     A4     A5     A6
    usage      0.012  0.015  0.003  0.001   0.015  0.001  0.020  0.054  0.016  0.020

The skip rule is active on 19 of S5's 36 sampled rings and 30 of S6's 42; what it drops carries 3e-48 and 2e-37 of a
ring's backstop.  On S7's rings 19, 29, 38 and 225 the m below ``2**-700`` carry 0.035 to 0.064 of ``sum_m S_m``; the
deepest start is ``2**-1585``.  The slowest truths: S6 4.4 s, S7 4.9 s (with their restatements).

S8a's 2e-11 is the spin-2 cancellation on the polar rings of nside 1024 (``1 / s^2`` is 2e6 on ring 0): large against the
map's maximum, a ninth of the backstop, which is made of the terms' magnitudes.  The magnitude sums take the larger of
``|lambda_l|`` and ``|lambda_{l-1}|``: with ``|lambda_l|`` alone the sparse map of A5 used 0.70 (a ring at ``x = 0.19`` on which
``lambda_{210,199}`` is far below its neighbours and carries the error of their size).
"""

import time

import numpy as np
import pytest

import sht_twin as st
from oracle import sht as osht

_CACHE = {}


def _synth(name):
    if name not in _CACHE:
        c = st.SynthCase(name)
        t0 = time.perf_counter()
        c.truth()
        _CACHE[name] = (c, time.perf_counter() - t0)
    return _CACHE[name]


def _anal(name):
    if name not in _CACHE:
        c = st.AnalCase(name)
        t0 = time.perf_counter()
        for niter in c.niters:
            c.truth(niter)
        _CACHE[name] = (c, time.perf_counter() - t0)
    return _CACHE[name]


def _square(a, lmax):
    """``[..., m, l]`` of the twin -> the oracle's square ``[..., l, m]``."""
    sq = np.zeros(a.shape[:-2] + (lmax + 1, lmax + 1), a.dtype)
    sq[..., : a.shape[-2]] = np.swapaxes(a, -1, -2)
    return sq


def test_long_double_is_x87():
    st.check_long_double()
    assert np.finfo(st.LD).maxexp == 16384


@pytest.mark.parametrize("nside", [1, 2, 8, 64, 256, 1024])
def test_geometry_bits(nside):
    """``ring_info`` against the expressions of ``get_geom`` (``csrc/sht.hip``) evaluated in C's order with float64
    scalars: bit for bit.  (The library keeps its tables on the device; the GPU sweep, whose sharp measure notices a
    last-bit change of ``z`` on the polar rings, is the check of the tables themselves.)"""
    z, nphi, phi0, start = osht.ring_info(nside)
    f = np.float64
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    for k in range(4 * nside - 1):
        ir = k + 1
        if ir < nside:
            want = (f(1.0) - f(ir * ir) / (f(3.0) * f(nside) * f(nside)), 4 * ir, f(np.pi) / (f(4.0) * f(ir)), 2 * ir * (ir - 1))
        elif ir <= 3 * nside:
            want = ((f(2.0) * f(nside) - f(ir)) * f(2.0) / (f(3.0) * f(nside)), 4 * nside, f((ir - nside + 1) & 1) * f(np.pi) / (f(4.0) * f(nside)),
                    ncap + (ir - nside) * 4 * nside)
        else:
            ip = 4 * nside - ir
            want = (-(f(1.0) - f(ip * ip) / (f(3.0) * f(nside) * f(nside))), 4 * ip, f(np.pi) / (f(4.0) * f(ip)), npix - 2 * ip * (ip + 1))
        got = (z[k], nphi[k], phi0[k], start[k])
        assert all(np.array(g).tobytes() == np.array(w, np.array(g).dtype).tobytes() for g, w in zip(got, want)), (k, got, want)
    # what the truth converts is exactly these floats
    assert np.array_equal(z.astype(st.LD).astype(np.float64), z)


@pytest.mark.parametrize("name", ["S0a", "S0b", "S1", "S2a", "S2b", "S3", "S4"])
def test_restatement_is_the_oracle_synthesis(name):
    c, _ = _synth(name)
    ref = c.truth()[2]
    want = np.stack([osht.alm2map(_square(c.alm[f], c.lmax), c.nside) for f in range(c.nf)])
    assert np.array_equal(ref, want[..., c.pix])  # the same operations in the same order: the same bits


@pytest.mark.parametrize("name", ["A0", "A1", "A2", "A3"])
def test_restatement_is_the_oracle_analysis(name):
    """``oracle.sht.map2alm`` sums over the rings in another order than the restatement (pairwise along another axis):
    ``2**-50`` of ``max|a|``.  With ``mmax < lmax`` the oracle's Jacobi steps synthesise other maps: the plain analysis only."""
    c, _ = _anal(name)
    full = np.zeros((c.nf, c.npol, 12 * c.nside**2))
    full[..., c.pix] = c.maps
    for niter in c.niters if c.mmax == c.lmax else (0,):
        ref = c.truth(niter)[2]
        want = np.stack([osht.map2alm(full[f], c.lmax, niter) for f in range(c.nf)])
        want = np.swapaxes(want, -1, -2)[:, :, : c.mmax + 1]
        assert np.abs(ref - want).max() <= 2.0**-50 * np.abs(want).max(), (niter, np.abs(ref - want).max())


def test_truth_against_the_definition():
    """``oracle.sht.alm2map_direct`` (O(npix lmax^2), no rings, no FFT) on nside 4 / lmax 7, all four polarisations."""
    nside, lmax = 4, 7
    alm = st.rand_alm(np.random.default_rng([st.SEED, 900]), 1, 4, lmax, lmax)
    alm[:, :, 0] = alm[:, :, 0].real
    T, _ = st.alm2map_ld(alm, nside, st.all_rings(nside))
    sq = _square(alm[0], lmax)
    Q, U = osht.alm2map_direct((sq[1], sq[2]), nside, spin_pair=True)
    want = np.stack([osht.alm2map_direct(sq[0], nside), Q, U, osht.alm2map_direct(sq[3], nside)])
    assert np.abs(T[0] - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("nside,lmax", [(1, 2), (2, 5), (4, 8), (8, 16)])
def test_truth_against_scipy_whole_map(nside, lmax):
    """The whole scalar map from SciPy's ``Y_lm`` at the pixel centres (``test_oracle_sht.py``'s check), T and V, at 1e-13
    of the map's maximum; and with a complex ``a_l0``: only its real part counts."""
    from scipy.special import sph_harm_y

    alm = st.rand_alm(np.random.default_rng([st.SEED, 901, nside]), 1, 4, lmax, lmax)
    th, ph = osht.pix_angles(nside)
    want = np.zeros((4, th.size))
    for p in (0, 3):
        for l in range(lmax + 1):
            want[p] += alm[0, p, 0, l].real * sph_harm_y(l, 0, th, ph).real
            for m in range(1, l + 1):
                want[p] += 2.0 * (alm[0, p, m, l] * sph_harm_y(l, m, th, ph)).real
    T, _ = st.alm2map_ld(alm, nside, st.all_rings(nside))
    assert np.abs(T[0, [0, 3]] - want[[0, 3]]).max() <= 1e-13 * np.abs(want).max()


def test_truth_against_scipy_spin2_derivatives():
    """Q, U from second derivatives of SciPy's ``Y_lm`` (``test_oracle_sht.py``: finite differences, 3e-5): the truth
    keeps the (E, B) -> (Q, U) signs of the HEALPix convention."""
    from scipy.special import sph_harm_y

    nside, lmax, h = 2, 4, 1e-3
    alm = st.rand_alm(np.random.default_rng([st.SEED, 902]), 1, 4, lmax, lmax)
    alm[:, :, 0] = alm[:, :, 0].real
    th, ph = osht.pix_angles(nside)
    P = np.zeros(th.size, complex)
    for l in range(2, lmax + 1):
        norm = np.sqrt(float((l - 1) * l * (l + 1) * (l + 2)))
        for m in range(-l, l + 1):
            am = abs(m)
            E = alm[0, 1, am, l] if m >= 0 else (-1) ** am * np.conj(alm[0, 1, am, l])
            B = alm[0, 2, am, l] if m >= 0 else (-1) ** am * np.conj(alm[0, 2, am, l])

            def Y(t):
                return sph_harm_y(l, m, t, 0.0)

            def spin1(t):
                return -((Y(t + h) - Y(t - h)) / (2 * h) - m / np.sin(t) * Y(t))

            def spin2(t):
                return -((spin1(t + h) - spin1(t - h)) / (2 * h) - m / np.sin(t) * spin1(t) - np.cos(t) / np.sin(t) * spin1(t))

            P += -(E + 1j * B) * spin2(th) / norm * np.exp(1j * m * ph)
    T, _ = st.alm2map_ld(alm, nside, st.all_rings(nside))
    scale = np.abs(P).max()
    assert np.abs(T[0, 1] - P.real).max() <= 3e-5 * scale and np.abs(T[0, 2] - P.imag).max() <= 3e-5 * scale


def test_analysis_truth_is_the_adjoint_of_the_synthesis_truth():
    """``<y, S a> w = sum fac Re(conj(A y) a)`` in long double: pins ``map2alm_ld`` to ``alm2map_ld`` at 1e-17."""
    nside, lmax = 4, 7
    rings = st.all_rings(nside)
    alm = st.rand_alm(np.random.default_rng([st.SEED, 903]), 1, 4, lmax, lmax)
    alm[:, :, 0] = alm[:, :, 0].real
    y = np.random.default_rng([st.SEED, 904]).standard_normal((1, 4, 12 * nside**2))
    Sa, _ = st.alm2map_ld(alm, nside, rings)
    Ay, _ = st.map2alm_ld(y, nside, lmax, lmax, rings)
    fac = np.where(np.arange(lmax + 1) == 0, 1, 2)[:, None]
    lhs = (y * Sa).sum() * 4 * st.PI / (12 * nside**2)
    rhs = (fac * (np.conj(Ay) * alm).real).sum()
    assert abs(lhs - rhs) <= 1e-17 * abs(lhs)


@pytest.mark.parametrize("name", list(st.SYNTH))
def test_synthesis_backstop_usage(name):
    c, secs = _synth(name)
    T, B, ref = c.truth()
    m = c.measure(ref)
    dist = float(np.abs(ref - T).max() / np.abs(T).max())
    print(f"sht twin {name}: {len(c.rings)} rings, truth and restatement in {secs:.1f} s; float64 restatement: error / backstop {m['usage']:.3g}, {dist:.1e} of max|T|")
    assert max(m["ratio"].values()) <= 1.0 and m["usage"] <= 0.5, m  # (the restatement against itself: ratio 1 or below)
    assert secs < 10.0


@pytest.mark.parametrize("name", list(st.ANAL))
def test_analysis_backstop_usage(name):
    c, secs = _anal(name)
    for niter in c.niters:
        T, B, ref = c.truth(niter)
        m = c.measure(ref, niter)
        print(f"sht twin {name} niter {niter}: {len(c.rings)} rings, {secs:.1f} s for all its truths; float64 restatement: error / backstop {m['usage']:.3g}")
        assert m["usage"] <= 0.5 and m["zeros"], m
        assert not np.any(T[..., np.arange(c.lmax + 1)[None, :] < np.arange(c.mmax + 1)[:, None]])
    assert secs < 10.0
    if len(c.rings) < 4 * c.nside - 1:  # a sparse map: both members of several north / south pairs
        assert sum(1 for k in c.rings if k < 2 * c.nside - 1 and 4 * c.nside - 2 - k in c.rings) >= 5


def test_sampled_rings_reach_every_class():
    for name in ("S5", "S6", "S8a"):
        c = st.SynthCase(name)
        ns, nring = c.nside, 4 * c.nside - 1
        groups = {st.ring_group(ns, k) for k in c.rings}
        want = {"belt"} | {f"cap{M}" for M in (256, 512, 1024, 2048, 4096, 8192) if M <= 8 * ns}
        assert groups == want, (name, groups)
        for k in (0, 1, nring - 1, nring - 2, ns - 1, 3 * ns - 1, 2 * ns - 1):
            assert k in c.rings
        e = 32
        while e < ns:
            assert {e - 2, e - 1, e} <= set(c.rings) and {nring - 1 - (e - 2), nring - 1 - (e - 1), nring - 1 - e} <= set(c.rings)
            e *= 2


def test_s7_reaches_the_rescaled_start():
    """On at least one ring of S7 the m whose ``log2 |lambda_mm| < -700`` carry more than 1e-3 of ``sum_m S_m``; every
    ring has ``nphi <= 256`` (801 m fold onto it) and ``sin(theta)`` in 0.25 ... 0.6."""
    c, _ = _synth("S7")
    b, S, W, lg = c.truth(detail=True)
    share = st.deep_start_share(S, lg)
    z, nphi, _, _ = osht.ring_info(c.nside)
    s = np.sqrt((1 - z[c.rings]) * (1 + z[c.rings]))
    print("sht twin S7: rings", c.rings, "share of sum_m S_m below 2**-700:", np.array2string(share, precision=3), "deepest log2 lambda_mm", lg.min())
    assert share.max() > 1e-3 and nphi[c.rings].max() <= 256 and s.min() >= 0.25 and s.max() <= 0.6
    assert lg.min() < -1500  # two steps of the block exponent


@pytest.mark.parametrize("name", ["S5", "S6"])
def test_skip_rule_drops_nothing_that_matters(name):
    """The terms that the documented skip rule drops sum to less than 1e-3 of the ring's backstop, and the rule is
    active (it drops some m) on the polar rings."""
    c, _ = _synth(name)
    b, S, W, lg = c.truth(detail=True)
    z = osht.ring_info(c.nside)[0][c.rings]
    share = st.skip_rule_share(S, W, z, c.lmax)
    s = np.sqrt((1 - z) * (1 + z))
    active = (c.mmax > c.lmax * s + max(100.0, c.lmax / 100.0) + 2.0).sum()
    print(f"sht twin {name}: the skip rule is active on {active} of {len(c.rings)} sampled rings; largest share of a ring's backstop it drops: {share.max():.3g}")
    assert active >= 4 and share.max() < 1e-3
