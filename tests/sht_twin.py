"""Long-double truths for the HEALPix transforms ``dmm_alm2map`` / ``dmm_map2alm`` (``csrc/sht*.h``, ``sht.hip``), the
float64 restatement of ``oracle/sht.py`` on a subset of rings, the acceptance measures and the case tables their tests
share.  NumPy only.

Layouts: ``alm [nf, npol, mmax+1, lmax+1]`` complex128, m-major as the library takes it (``l < m`` unused and zero);
maps on a set of ``rings`` (0-based ring indices, north to south) as one array ``[nf, npol, npix_of_those_rings]``, the
rings back to back in the order of ``rings`` (:func:`ring_pixels` gives the global pixel numbers).

* ``alm2map_ld`` / ``map2alm_ld``: the truth.  The inputs are the floats the GPU sees: ``z``, ``phi0``, ``nphi``,
  ``start`` of ``oracle.sht.ring_info`` (float64 formulas, the same bits as the library's ``get_geom``), converted
  exactly.  ``sin^2 = (1 - z)(1 + z)``, ``pi``, every recurrence and spin-2 factor are formed in long double;
  ``lambda_mm = (-1)^m sqrt((2m+1)/(4 pi) prod_k (2k-1)/(2k)) s^m`` from the closed product (x87's exponent range holds
  ``s^m`` for every case here: finiteness and a 64-bit significand are asserted); the plain three-term recurrence in
  ``l`` with no skip rule and no rescaling; F1 / F2 by the KKS expressions of ``oracle/sht.py:_spin_F``; ring phases ``m
  phi0 + 2 pi ((m j) mod nphi) / nphi`` with the product reduced in integers.  Synthesis takes ``Re``: ``Im a_l0`` drops
  out (it is removed before the magnitude sums are formed).  Vectorised over ``(m, ring)``, one Python loop over ``l``.
* ``alm2map_f64`` / ``map2alm_f64``: the oracle's algorithm (log-scaled start with the 1e100 rescaling, ``numpy.fft``
  per ring) vectorised the same way, so that it can run on a few rings of a large geometry.
  ``test_sht_twin_host.py`` shows that it reproduces ``oracle.sht.alm2map`` / ``map2alm`` on the small all-ring cases.

Measures.  Nothing of the code under test enters them; ``u = 2**-53``.

*Sharp measure.*  ``e_gpu = rms(got - T)``, ``e_ref = rms(float64 restatement - T)`` over a group's elements;
``ratio = e_gpu / max(e_ref, u rms|T|) <= 8`` (``SHARP``).  Synthesis groups: ``(pol, ring group)``, the ring groups
being the belt and each class of Bluestein length (``fft_len``: the smallest power of two ``>= 2 nphi - 1``, at least
256), both caps together.  Analysis groups: ``(pol)`` over the entries ``l >= m``.  The kernels and the restatement
evaluate the same sums in other orders (8-step MFMA chunks, radix-8 / Bluestein FFTs against pocketfft, an ``exp2``
start against ``exp(log)``): three bits are the allowance for that, a figure of the issue that set this test, not a
measured one.  A group whose truth is all zero must be all zero.

*Backstop.*  Per pixel of a ring, ``|got - T| <= 2**-52 sum_m fac_m W_m S_m`` with ``fac_0 = 1``, ``fac_m = 2``,
``S_m`` the magnitude sum of the ``(ring, m, pol)`` coefficient -- scalar: ``sum_l |a_lm| |lam_l|``; spin 2: the sum of
the *terms'* magnitudes, ``c (|(l - m^2)/s^2 + l(l-1)/2| |lam_l| + |x/s^2| d |lam_{l-1}|)`` for F1 and ``c (m/s^2) ((l-1) |x|
|lam_l| + d |lam_{l-1}|)`` for F2 (they cancel near the poles and the rounding error scales with them, not with ``|F|``).
In all of these ``|lam_l|`` stands for ``max(|lambda_lm|, |lambda_{l-1,m}|)``: the three-term recurrence carries an error
of the size of its larger neighbour into a value that is small by parity or near a zero (with ``|lambda_lm|`` itself the
float64 restatement used 0.70 of the adjoint bound on the sparse map of A5, through one ring at ``x = 0.19``) --
and ``W_m = (lmax - m + 1) + |log2 |lambda_mm(ring)|| + 3 log2 M_ring + 16`` in units of ``2 u``: the depth of the
recurrence, the rounding of the logarithmic start (``m log s`` rounded at ``u |log lambda_mm|`` moves ``lambda_mm`` by that
much relatively), three FFTs of length ``M_ring = fft_len`` (``log2 M`` butterfly levels each; the belt runs one), and 16
for the single roundings (coefficient table, ``1 / s^2``, spin-2 products, phase rotation, ``fac``).  The adjoint form
for ``a_lm``: ``|got - T| <= 2**-52 sum_ring W_m(ring) X_lm(ring) G(ring)``, ``G = (4 pi / npix) sum_j |map_j|`` of the
polarisation(s) that enter and ``X`` the same term magnitudes (``|lambda_lm|``; for E: ``T1 G_Q + T2 G_U``, for B: ``T1 G_U
+ T2 G_Q``).  A Jacobi step ``a += A(map - S a)`` keeps the inherited error (``I - A S`` is a contraction on the band
limit), analyses a residual of at most ``|map| + |S a|`` (two units) and carries the synthesis error of ``S a`` through
the analysis (one more): ``(1 + 3 niter)`` times the bound of the plain analysis.
Measured against the float64 restatement (``test_sht_twin_host.py`` tabulates every case): it uses 0.0004 to 0.13 of the
synthesis backstop and 0.001 to 0.054 of the adjoint one; the host test requires ``<= 0.5``.

*Exact zeros and finiteness.*  ``a_lm`` at ``l < m`` and E, B at ``l < 2`` are exact zeros; the GPU tests fill every
output with NaN before the call and require it finite after it.
"""

import numpy as np

from oracle import sht as osht

LD, CLD = np.longdouble, np.clongdouble
PI = 4 * np.arctan(LD(1))
U = 2.0**-53
SHARP = 8.0
SEED = 20261020


def check_long_double():
    assert np.finfo(LD).nmant == 63, "the truth needs the x87 80-bit long double"


# ------------------------------------------------------------------ geometry, ring groups, sampled rings
def fft_len(nside, k):
    """FFT length of ring ``k``: ``4 nside`` in the belt, the Bluestein length (power of two ``>= 2 nphi - 1``, at least
    256) in the caps."""
    ir = k + 1
    if nside <= ir <= 3 * nside:
        return 4 * nside
    ir = ir if ir < nside else 4 * nside - ir
    M = 256
    while M < 8 * ir - 1:
        M *= 2
    return M


def ring_group(nside, k):
    ir = k + 1
    return "belt" if nside <= ir <= 3 * nside else f"cap{fft_len(nside, k)}"


def ring_pixels(nside, rings):
    """Global pixel numbers of ``rings`` back to back, and the position in ``rings`` of every one of them."""
    _, nphi, _, start = osht.ring_info(nside)
    pix = np.concatenate([np.arange(start[k], start[k] + nphi[k]) for k in rings])
    which = np.concatenate([np.full(nphi[k], i) for i, k in enumerate(rings)])
    return pix, which


def all_rings(nside):
    return list(range(4 * nside - 1))


def sampled_rings(nside, seed, nother=10):
    """Rings 0, 1 and their mirrors; every edge of a Bluestein class (its last ring) +- 1 and the last cap ring, in both caps; the belt's
    first and last ring and the equator; ``nother`` seeded others, the mirrors of half of them included."""
    nring = 4 * nside - 1
    north = {0, 1, nside - 2, nside - 1, 2 * nside - 1}
    e = 32
    while e < nside:  # cap ring number e is the last of its class: ring indices e - 2, e - 1 | e
        north |= {e - 2, e - 1, e}
        e *= 2
    rng = np.random.default_rng([SEED, nside, seed])
    other = rng.choice(2 * nside - 1, size=min(nother, 2 * nside - 1), replace=False)
    north |= {int(k) for k in other[: (nother + 1) // 2]}
    rings = set(north) | {nring - 1 - k for k in north} | {int(k) for k in other}
    return sorted(k for k in rings if 0 <= k < nring)


def s7_rings(nside=64, n=6):
    """Cap rings with sin(theta) between 0.25 and 0.6, every other one with its mirror."""
    z, *_ = osht.ring_info(nside)
    s = np.sqrt((1 - z) * (1 + z))
    cand = [k for k in range(nside - 1) if 0.25 <= s[k] <= 0.6]
    pick = [cand[i] for i in np.linspace(0, len(cand) - 1, n * 2 // 3).round().astype(int)]
    return sorted(set(pick) | {4 * nside - 2 - k for k in pick[1::2]})


# ------------------------------------------------------------------ Legendre functions, one l at a time
# Tables are [ring, m] with m innermost: the long axis last keeps NumPy's inner loops long.
def _lam_ld(lmax, mmax, z):
    """Yield ``(l, k, lam_l[:, :k], lam_{l-1}[:, :k])`` (columns ``m < k = min(l, mmax) + 1``) in long double; first the
    ``[ring, mmax+1]`` table ``log2 |lambda_mm|``."""
    x = z.astype(LD)[:, None]
    s = np.sqrt((1 - x) * (1 + x))
    m = np.arange(mmax + 1)
    pref = np.empty(mmax + 1, LD)
    p = LD(1)
    for mm in range(mmax + 1):
        if mm:
            p = p * LD(2 * mm - 1) / LD(2 * mm)
        pref[mm] = np.sqrt(LD(2 * mm + 1) / (4 * PI) * p)
    lam_mm = (np.where(m % 2, -1, 1) * pref) * s ** m.astype(LD)
    assert np.all(np.isfinite(lam_mm)) and np.all(lam_mm != 0), "s^m left the long double's range"
    yield np.log2(np.abs(lam_mm)).astype(np.float64)
    m2 = (m * m).astype(LD)
    cur = np.zeros((z.size, mmax + 1), LD)
    prev = np.zeros_like(cur)
    for l in range(lmax + 1):
        k = min(l, mmax + 1)
        if k:
            lL, l1 = LD(l), LD(l - 1)
            A = np.sqrt((lL * lL - m2[:k]) / (4 * lL * lL - 1))
            Ap = np.sqrt((l1 * l1 - m2[:k]) / (4 * l1 * l1 - 1))
            new = (x * cur[:, :k] - Ap * prev[:, :k]) / A
            prev[:, :k] = cur[:, :k]
            cur[:, :k] = new
        if l <= mmax:
            cur[:, l] = lam_mm[:, l]
        kk = min(l, mmax) + 1
        yield l, kk, cur[:, :kk], prev[:, :kk]


def _lam_f64(lmax, mmax, z):
    """The same stream by ``oracle.sht.lambda_lm``'s algorithm, operation for operation, vectorised over m."""
    x = np.asarray(z, np.float64)
    s = np.sqrt((1.0 - x) * (1.0 + x))
    e = np.empty((x.size, mmax + 1))
    with np.errstate(divide="ignore"):
        for m in range(mmax + 1):
            k = np.arange(1, m + 1)
            log_pref = 0.5 * (np.log(2 * m + 1.0) - np.log(4 * np.pi) + np.sum(np.log((2 * k - 1.0) / (2.0 * k))))
            log_mm = log_pref + m * np.log(s)
            e[:, m] = np.where(np.isfinite(log_mm), log_mm, -1e300) if m > 0 else np.full_like(x, log_pref)
    yield e / np.log(2.0)
    x = x[:, None]
    mm = (np.arange(mmax + 1) ** 2).astype(np.float64)
    v = np.zeros((z.size, mmax + 1))
    vp = np.zeros_like(v)
    out = np.zeros_like(v)
    outp = np.zeros_like(v)
    with np.errstate(over="ignore", under="ignore"):
        for l in range(lmax + 1):
            k = min(l, mmax + 1)
            outp[:, :k] = out[:, :k]
            if k:
                A = np.sqrt((float(l * l) - mm[:k]) / (4.0 * l * l - 1.0))
                Ap = np.sqrt((float((l - 1) * (l - 1)) - mm[:k]) / (4.0 * (l - 1) * (l - 1) - 1.0))
                new = (x * v[:, :k] - Ap * vp[:, :k]) / A
                vp[:, :k] = v[:, :k]
                v[:, :k] = new
                big = np.abs(new) > 1e100
                if big.any():
                    v[:, :k][big] *= 1e-100
                    vp[:, :k][big] *= 1e-100
                    e[:, :k][big] += np.log(1e100)
                out[:, :k] = v[:, :k] * np.exp(e[:, :k])
            if l <= mmax:
                v[:, l] = (-1.0) ** l
                out[:, l] = v[:, l] * np.exp(e[:, l])
                outp[:, l] = 0.0
            kk = min(l, mmax) + 1
            yield l, kk, out[:, :kk], outp[:, :kk]


def _spin(l, kk, x, s2, lam, lam1, dt, mags):
    """F1, F2 of ``oracle.sht._spin_F`` for one l (operation for operation), and the magnitudes of their terms."""
    m = np.arange(kk).astype(dt)
    l_, one, two = dt(l), dt(1), dt(2)
    c = two / np.sqrt((l_ - one) * l_ * (l_ + one) * (l_ + two))
    d = np.sqrt((two * l_ + one) / (two * l_ - one) * (l_ * l_ - m * m))
    p = (l_ - m * m) / s2 + dt(0.5) * l_ * (l_ - one)
    q = (x / s2) * d
    F1 = c * (-p * lam + q * lam1)
    cm = c * (m / s2)
    F2 = cm * (-(l_ - one) * x * lam + d * lam1)
    if not mags:
        return F1, F2, None, None
    al1 = np.abs(lam1)
    al = np.maximum(np.abs(lam), al1)
    return F1, F2, c * (np.abs(p) * al + np.abs(q) * al1), cm * ((l_ - one) * np.abs(x) * al + d * al1)


def _legendre_synth(it, alm, z, dt, cdt, mags):
    """``b [nf, npol, ring, m] = sum_l a_lm {lambda | F1, F2}``, the magnitude sums ``S`` alike, ``log2 |lambda_mm|``.
    Real and imaginary parts are carried apart: the products are those of the complex expressions of
    ``oracle.sht.legendre_synthesis`` (a real factor times a complex one), at half the work in long double."""
    nf, npol, nm, nl = alm.shape
    x = z.astype(dt)[:, None]
    s2 = (1 - x) * (1 + x)
    at = np.ascontiguousarray(alm.transpose(0, 1, 3, 2))[:, :, :, None, :]  # [nf, npol, l, 1, m]
    ar, ai = at.real.astype(dt), at.imag.astype(dt)
    aa = np.abs(at.astype(cdt)) if mags else None
    br, bi = np.zeros((nf, npol, z.size, nm), dt), np.zeros((nf, npol, z.size, nm), dt)
    S = np.zeros((nf, npol, z.size, nm), dt) if mags else None
    lg = next(it)
    for l, kk, lam, lam1 in it:
        r, i = ar[:, :, l, :, :kk], ai[:, :, l, :, :kk]
        for p in (0, 3)[: 1 + (npol == 4)]:
            br[:, p, :, :kk] += r[:, p] * lam
            bi[:, p, :, :kk] += i[:, p] * lam
        if mags:
            al = np.maximum(np.abs(lam), np.abs(lam1))
            for p in (0, 3)[: 1 + (npol == 4)]:
                S[:, p, :, :kk] += aa[:, p, l, :, :kk] * al
        if npol == 4 and l >= 2:
            F1, F2, T1, T2 = _spin(l, kk, x, s2, lam, lam1, dt, mags)
            Er, Ei, Br, Bi = r[:, 1], i[:, 1], r[:, 2], i[:, 2]
            br[:, 1, :, :kk] -= Er * F1 - Bi * F2  # -(E F1 + i B F2)
            bi[:, 1, :, :kk] -= Ei * F1 + Br * F2
            br[:, 2, :, :kk] -= Br * F1 + Ei * F2  # -(B F1 - i E F2)
            bi[:, 2, :, :kk] -= Bi * F1 - Er * F2
            if mags:
                aE, aB = aa[:, 1, l, :, :kk], aa[:, 2, l, :, :kk]
                S[:, 1, :, :kk] += aE * T1 + aB * T2
                S[:, 2, :, :kk] += aB * T1 + aE * T2
    return br + 1j * bi, S, lg


def _legendre_anal(it, g, z, lmax, dt, cdt, G=None, W=None):
    """Adjoint: ``a [nf, npol, m, l] = sum_ring {lambda | F1, F2} g [nf, npol, ring, m]``; with ``G [nf, npol, ring]``
    and ``W [ring, m]`` also ``sum_ring W X G`` per entry."""
    nf, npol, _, nm = g.shape
    x = z.astype(dt)[:, None]
    s2 = (1 - x) * (1 + x)
    a = np.zeros((nf, npol, nm, lmax + 1), cdt)
    bound = np.zeros((nf, npol, nm, lmax + 1), dt) if G is not None else None
    next(it)
    for l, kk, lam, lam1 in it:
        for p in (0, 3)[: 1 + (npol == 4)]:
            a[:, p, :kk, l] = (lam * g[:, p, :, :kk]).sum(axis=-2)
            if G is not None:
                bound[:, p, :kk, l] = (W[:, :kk] * np.maximum(np.abs(lam), np.abs(lam1)) * G[:, p, :, None]).sum(axis=-2)
        if npol == 4 and l >= 2:
            F1, F2, T1, T2 = _spin(l, kk, x, s2, lam, lam1, dt, G is not None)
            gQ, gU = g[:, 1, :, :kk], g[:, 2, :, :kk]
            a[:, 1, :kk, l] = -(F1 * gQ + 1j * F2 * gU).sum(axis=-2)
            a[:, 2, :kk, l] = -(F1 * gU - 1j * F2 * gQ).sum(axis=-2)
            if G is not None:
                GQ, GU = G[:, 1, :, None], G[:, 2, :, None]
                bound[:, 1, :kk, l] = (W[:, :kk] * (T1 * GQ + T2 * GU)).sum(axis=-2)
                bound[:, 2, :kk, l] = (W[:, :kk] * (T1 * GU + T2 * GQ)).sum(axis=-2)
    return a, bound


def _weights(lg, lmax, nside, rings):
    """``W [ring, m]`` of the backstop."""
    m = np.arange(lg.shape[1])[None, :]
    M = np.array([fft_len(nside, k) for k in rings], np.float64)[:, None]
    return (lmax - m + 1) + np.abs(lg) + 3 * np.log2(M) + 16


# ------------------------------------------------------------------ ring stages
def _phases_ld(n, m, phi0):
    """``(cos, sin)`` of ``m phi0`` and of ``2 pi ((m j) mod n) / n`` as ``[m, j]`` tables, long double."""
    ang = 2 * PI * np.arange(n).astype(LD) / LD(n)
    idx = (m[:, None] * np.arange(n)[None, :]) % n
    a0 = LD(phi0) * m.astype(LD)
    return np.cos(a0), np.sin(a0), np.cos(ang)[idx], np.sin(ang)[idx]


def _ring_synth_ld(b, nside, rings):
    _, nphi, phi0, _ = osht.ring_info(nside)
    nf, npol, _, nm = b.shape
    m = np.arange(nm)
    fac = np.where(m == 0, 1, 2).astype(LD)
    out = []
    for i, k in enumerate(rings):
        c0, s0, Er, Ei = _phases_ld(int(nphi[k]), m, phi0[k])
        br, bi = b[:, :, i].real.reshape(nf * npol, nm), b[:, :, i].imag.reshape(nf * npol, nm)
        cr, ci = fac * (br * c0 - bi * s0), fac * (br * s0 + bi * c0)
        out.append((cr @ Er - ci @ Ei).reshape(nf, npol, -1))
    return np.concatenate(out, axis=-1)


def _ring_anal_ld(maps, nside, rings, mmax):
    """``g [nf, npol, ring, m]`` and ``G [nf, npol, ring] = w sum_j |map_j|`` from maps on ``rings`` (any real dtype)."""
    _, nphi, phi0, _ = osht.ring_info(nside)
    nf, npol, _ = maps.shape
    m = np.arange(mmax + 1)
    w = 4 * PI / LD(12 * nside * nside)
    g = np.zeros((nf, npol, len(rings), mmax + 1), CLD)
    G = np.zeros((nf, npol, len(rings)), LD)
    o = 0
    for i, k in enumerate(rings):
        n = int(nphi[k])
        v = maps[..., o : o + n].astype(LD).reshape(nf * npol, n)
        o += n
        G[..., i] = (w * np.abs(v).sum(axis=-1)).reshape(nf, npol)
        if not v.any():
            continue
        c0, s0, Er, Ei = _phases_ld(n, m, phi0[k])
        fr, fi = v @ Er.T, -(v @ Ei.T)  # sum_j map_j e^{-i 2 pi m j / n}
        g[:, :, i] = (w * ((fr * c0 + fi * s0) + 1j * (fi * c0 - fr * s0))).reshape(nf, npol, -1)
    return g, G


def _ring_synth_f64(b, nside, rings):
    """``oracle.sht.ring_synthesis`` for the chosen rings."""
    _, nphi, phi0, _ = osht.ring_info(nside)
    nf, npol, _, nm = b.shape
    m = np.arange(nm)
    fac = np.where(m == 0, 1.0, 2.0)
    out = []
    for i, k in enumerate(rings):
        n = int(nphi[k])
        c = b[:, :, i].reshape(nf * npol, nm) * (fac * np.exp(1j * m * phi0[k]))
        h = np.zeros((nf * npol, n), np.complex128)
        np.add.at(h, (slice(None), m % n), c)
        out.append((np.fft.ifft(h, axis=-1) * n).real.reshape(nf, npol, n))
    return np.concatenate(out, axis=-1)


def _ring_anal_f64(maps, nside, rings, mmax):
    """``oracle.sht.ring_analysis`` for the chosen rings."""
    _, nphi, phi0, _ = osht.ring_info(nside)
    nf, npol, _ = maps.shape
    m = np.arange(mmax + 1)
    w = 4.0 * np.pi / (12 * nside * nside)
    g = np.zeros((nf, npol, len(rings), mmax + 1), np.complex128)
    o = 0
    for i, k in enumerate(rings):
        n = int(nphi[k])
        F = np.fft.fft(maps[..., o : o + n], axis=-1)
        o += n
        g[:, :, i] = F[..., m % n] * np.exp(-1j * m * phi0[k]) * w
    return g


# ------------------------------------------------------------------ the transforms
def alm2map_ld(alm, nside, rings, detail=False):
    """Truth of the synthesis on ``rings``: ``(T [nf, npol, pix], backstop [nf, npol, pix])``, both long double;
    ``detail``: also ``(b, S, W, lg)`` -- the ring coefficients, the magnitude sums, the weights and ``log2 |lambda_mm|``,
    ``[..., ring, m]``."""
    check_long_double()
    alm = np.array(alm, np.complex128)
    alm[:, :, 0, :] = alm[:, :, 0, :].real  # Re of the m = 0 term: Im a_l0 drops out
    nm, lmax = alm.shape[2] - 1, alm.shape[3] - 1
    z = osht.ring_info(nside)[0][list(rings)]
    b, S, lg = _legendre_synth(_lam_ld(lmax, nm, z), alm, z, LD, CLD, True)
    T = _ring_synth_ld(b, nside, rings)
    assert np.all(np.isfinite(T))
    W = _weights(lg, lmax, nside, rings)
    fac = np.where(np.arange(nm + 1) == 0, 1.0, 2.0)
    Bring = 2.0**-52 * (fac * W * S).sum(axis=-1)  # [nf, npol, ring]
    which = ring_pixels(nside, rings)[1]
    return (T, Bring[..., which], (b, S, W, lg)) if detail else (T, Bring[..., which])


def alm2map_f64(alm, nside, rings):
    alm = np.asarray(alm, np.complex128)
    nm, lmax = alm.shape[2] - 1, alm.shape[3] - 1
    z = osht.ring_info(nside)[0][list(rings)]
    b, _, _ = _legendre_synth(_lam_f64(lmax, nm, z), alm, z, np.float64, np.complex128, False)
    return _ring_synth_f64(b, nside, rings)


def map2alm_ld(maps_on_rings, nside, lmax, mmax, rings, niter=0):
    """Truth of the analysis of maps that vanish off ``rings``: ``(a [nf, npol, m, l], bound)`` long double, ``bound`` the
    adjoint backstop times ``1 + 3 niter``.  ``niter > 0`` needs every ring (the Jacobi steps iterate the long-double
    stages: ``a += A(map - S a)``)."""
    check_long_double()
    z = osht.ring_info(nside)[0][list(rings)]
    maps = np.asarray(maps_on_rings)
    g, G = _ring_anal_ld(maps, nside, rings, mmax)
    lg = next(_lam_ld(0, mmax, z))
    W = _weights(lg, lmax, nside, rings)
    a, bound = _legendre_anal(_lam_ld(lmax, mmax, z), g, z, lmax, LD, CLD, G, W)
    assert niter == 0 or len(rings) == 4 * nside - 1
    for _ in range(niter):
        b, _, _ = _legendre_synth(_lam_ld(lmax, mmax, z), a, z, LD, CLD, False)
        g, _ = _ring_anal_ld(maps.astype(LD) - _ring_synth_ld(b, nside, rings), nside, rings, mmax)
        a = a + _legendre_anal(_lam_ld(lmax, mmax, z), g, z, lmax, LD, CLD)[0]
    assert np.all(np.isfinite(a.real)) and np.all(np.isfinite(a.imag))
    return a, 2.0**-52 * (1 + 3 * niter) * bound


def map2alm_f64(maps_on_rings, nside, lmax, mmax, rings, niter=0):
    z = osht.ring_info(nside)[0][list(rings)]
    maps = np.asarray(maps_on_rings, np.float64)

    def analyse(mp):
        return _legendre_anal(_lam_f64(lmax, mmax, z), _ring_anal_f64(mp, nside, rings, mmax), z, lmax, np.float64, np.complex128)[0]

    a = analyse(maps)
    for _ in range(niter):
        b, _, _ = _legendre_synth(_lam_f64(lmax, mmax, z), a, z, np.float64, np.complex128, False)
        a = a + analyse(maps - _ring_synth_f64(b, nside, rings))
    return a


# ------------------------------------------------------------------ measures
def _rms(v):
    v = np.asarray(v)
    return float(np.sqrt((np.abs(v) ** 2).mean())) if v.size else 0.0


def _sharp(got, T, ref):
    """``e_gpu / max(e_ref, u rms|T|)``; an all-zero truth wants all zeros (ratio 0, else inf)."""
    if not np.any(T):
        return 0.0 if not np.any(got) else np.inf
    return _rms(got - T) / max(_rms(ref - T), U * _rms(T))


def _usage(got, T, B):
    err = np.abs(got - T)
    ok = B > 0
    if np.any(err[~ok] != 0):
        return np.inf
    return float((err[ok] / B[ok]).max()) if ok.any() else 0.0


def synth_measure(got, T, ref, B, nside, rings):
    """``{"ratio": {(pol, group): ratio}, "usage": max |got - T| / backstop}`` of maps ``[nf, npol, pix]`` on ``rings``."""
    which = ring_pixels(nside, rings)[1]
    grp = np.array([ring_group(nside, k) for k in rings])[which]
    ratio = {}
    for p in range(T.shape[1]):
        for name in sorted(set(grp)):
            sel = grp == name
            ratio[(p, name)] = _sharp(got[:, p][:, sel], T[:, p][:, sel], ref[:, p][:, sel])
    return {"ratio": ratio, "usage": _usage(got, T, B)}


def anal_measure(got, T, ref, B):
    """The same for ``a [nf, npol, m, l]``: groups ``(pol)`` over ``l >= m``; ``zeros``: ``l < m`` and E, B at ``l < 2``
    are exact zeros."""
    nm, nl = T.shape[2:]
    live = np.arange(nl)[None, :] >= np.arange(nm)[:, None]
    ratio = {p: _sharp(got[:, p][:, live], T[:, p][:, live], ref[:, p][:, live]) for p in range(T.shape[1])}
    zeros = not np.any(got[..., ~live]) and (T.shape[1] == 1 or not np.any(got[:, 1:3, :, :2]))
    return {"ratio": ratio, "usage": _usage(got[..., live], T[..., live], B[..., live]), "zeros": bool(zeros)}


def passes(m):
    return max(m["ratio"].values()) <= SHARP and m["usage"] <= 1.0 and m.get("zeros", True)


def fmt(m):
    r = " ".join(f"{'.'.join(map(str, k)) if isinstance(k, tuple) else k}:{v:.2f}" for k, v in m["ratio"].items())
    return f"ratio [{r}] max {max(m['ratio'].values()):.2f}; error / backstop {m['usage']:.3g}" + ("" if m.get("zeros", True) else "; NON-ZERO structural zeros")


# ------------------------------------------------------------------ cases
# name -> (nside, lmax, mmax, nf, npol, rings)
SYNTH = {
    "S0a": (1, 0, 0, 1, 1, "all"),        # smallest geometry; lmax = 0
    "S0b": (1, 2, 2, 1, 4, "all"),        # the equator as an unpaired ring
    "S1": (2, 7, 7, 3, 4, "all"),         # m = 0 and m = nphi/2 folds on nphi 4 and 8; a ragged group
    "S2a": (8, 23, 11, 5, 1, "all"),      # mmax < lmax; lmax + 1 - m ragged against 8-step chunks
    "S2b": (8, 23, 11, 5, 4, "all"),      # groups 4 + 1
    "S3": (16, 40, 40, 9, 4, "all"),      # three frequency groups (8 + 1)
    "S4": (32, 95, 95, 1, 4, "all"),      # lmax = 3 nside - 1; one cap class
    "S5": (128, 300, 300, 2, 4, "sampled"),   # 256 ring pairs; classes 256 / 512 / 1024; the skip rule on the polar rings
    "S6": (256, 512, 512, 1, 4, "sampled"),   # two block rows of pairs; class 2048
    "S7": (64, 1536, 800, 1, 4, "s7"),        # lambda_mm < 2**-700 whose values grow back; nphi <= 256 against 801 m
    "S8a": (1024, 48, 48, 1, 4, "sampled"),   # class 4096; cap rings 513..1023 on the direct kernel; the belt at M = 4096
    "S8b": (1024, 48, 48, 1, 1, "sampled"),
}
S3_VARIANTS = (0, 64, 128, 8, 4)

# name -> (nside, lmax, mmax, nf, npol, niters, map): "dense" or non-zero on the sampled rings only
ANAL = {
    "A0": (1, 2, 2, 1, 4, (0,), "dense"),
    "A1": (4, 9, 9, 3, 4, (0, 1, 3), "dense"),     # Jacobi steps; ragged group
    "A2": (16, 40, 25, 5, 4, (0, 2), "dense"),     # lmax + 1 - m ragged against the 32-step chunk; mmax < lmax
    "A3": (32, 64, 64, 1, 4, (0,), "dense"),       # two chunks + 1
    "A4": (128, 300, 300, 2, 4, (0,), "sampled"),  # 256 pairs, one pass
    "A5": (256, 300, 300, 1, 4, (0,), "sampled"),  # two passes, the second adds into the first
    "A6": (1024, 48, 48, 1, 4, (0,), "sampled"),   # the largest nside the LDS ring stage takes
}
ANAL_VARIANTS = (0, 8)


def case_rings(nside, kind, idx):
    return all_rings(nside) if kind in ("all", "dense") else s7_rings(nside) if kind == "s7" else sampled_rings(nside, idx)


def rand_alm(rng, nf, npol, lmax, mmax):
    """Flat in l, complex a_l0, zeros at l < m and (E, B) at l < 2."""
    a = rng.standard_normal((nf, npol, mmax + 1, lmax + 1)) + 1j * rng.standard_normal((nf, npol, mmax + 1, lmax + 1))
    a[..., np.arange(lmax + 1)[None, :] < np.arange(mmax + 1)[:, None]] = 0
    if npol == 4:
        a[:, 1:3, :, :2] = 0
    return a


class SynthCase:
    """Inputs and (lazily, once) the truth, the backstop and the float64 restatement of one synthesis case; ``nf``
    overrides the table's frequency count (the first ``nf`` of a longer draw share their values with nobody)."""

    def __init__(self, name, nf=None):
        self.name = name
        self.nside, self.lmax, self.mmax, nf0, self.npol, kind = SYNTH[name]
        self.nf = nf0 if nf is None else nf
        idx = list(SYNTH).index(name)
        self.rings = case_rings(self.nside, kind, idx)
        self.alm = rand_alm(np.random.default_rng([SEED, idx, self.nf]), self.nf, self.npol, self.lmax, self.mmax)
        self.pix = ring_pixels(self.nside, self.rings)[0]
        self._t = None

    def truth(self, detail=False):
        """``(T, backstop, float64 restatement)``; ``detail``: ``(b, S, W, lg)`` of :func:`alm2map_ld`."""
        if self._t is None:
            T, B, d = alm2map_ld(self.alm, self.nside, self.rings, detail=True)
            self._t = (T, B, alm2map_f64(self.alm, self.nside, self.rings)), d
        return self._t[1] if detail else self._t[0]

    def measure(self, got):
        T, B, ref = self.truth()
        return synth_measure(got, T, ref, B, self.nside, self.rings)


class AnalCase:
    def __init__(self, name, nf=None):
        self.name = name
        self.nside, self.lmax, self.mmax, nf0, self.npol, self.niters, kind = ANAL[name]
        self.nf = nf0 if nf is None else nf
        idx = list(ANAL).index(name)
        self.rings = case_rings(self.nside, kind, 100 + idx)
        self.pix = ring_pixels(self.nside, self.rings)[0]
        self.maps = np.random.default_rng([SEED, 100 + idx, self.nf]).standard_normal((self.nf, self.npol, self.pix.size))
        self._t = {}

    def truth(self, niter):
        if niter not in self._t:
            a = (self.maps, self.nside, self.lmax, self.mmax, self.rings, niter)
            self._t[niter] = map2alm_ld(*a) + (map2alm_f64(*a),)
        return self._t[niter]

    def measure(self, got, niter):
        T, B, ref = self.truth(niter)
        return anal_measure(got, T, ref, B)


def skip_rule_share(S, W, z, lmax):
    """Per ring, the share of the backstop carried by the m that the documented skip rule ``m > lmax sin(theta) + max(100,
    lmax / 100) + 2`` drops: the largest over frequencies and polarisations."""
    s = np.sqrt((1 - z) * (1 + z))[:, None]
    m = np.arange(W.shape[1])[None, :]
    t = np.where(m == 0, 1.0, 2.0) * W * S
    drop = m > lmax * s + max(100.0, lmax / 100.0) + 2.0
    return ((t * drop).sum(axis=-1) / t.sum(axis=-1)).astype(np.float64).max(axis=(0, 1))


def deep_start_share(S, lg):
    """Per ring, the share of ``sum_m S_m`` carried by the m whose ``log2 |lambda_mm| < -700`` (the rescaled start): the
    largest over frequencies and polarisations."""
    return ((S * (lg < -700.0)).sum(axis=-1) / S.sum(axis=-1)).astype(np.float64).max(axis=(0, 1))
