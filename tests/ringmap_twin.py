"""Long-double truths for the consumer of the ring-map chain, ``csrc/ringmap.hip`` (``dmm_ringmap_deconvolve``,
``dmm_ringmap_window``) and the analytic beam in front of it (``dmm_analytic_beam_mmodes`` of ``csrc/mfft.hip``), with
the error measures and the case tables their tests share.  NumPy only; nothing of the code under test enters a bound.

* ``deconvolve_truth``     the formula at the head of ``ringmap.hip`` in ``numpy.longdouble``: term weights of the three
  modes the kernel receives, ``sum_w``, ``C``, ``map_m``, ``dirty_m``, ``norm``, ``weight``, ``dirty_beam_power`` and the
  two inverse real transforms, written out as direct sums (``irfft_direct``) at the RA positions asked for;
* ``window_truth``         the cosine-sum window of ``dmm_ringmap_window`` rounded once to float32;
* ``analytic_beam_truth``  the transit beam of ``k_beam_mfft``, its forward DFT written out as a direct sum, ``1 / nra``,
  the ``+m`` / ``-m`` pack, rounded once to complex64;
* ``oracle_deconvolve``    ``oracle.ringmap.deconvolve`` (float64, ``numpy.fft.irfft``) on the inputs of a case: the
  yardstick ``e_ref`` of the acceptance rule;
* ``Case`` and the tables ``THREE_KERNEL``, ``SINGLE_PASS``, ``TILE_MAP``, ``WINDOW_CASES``, ``BEAM_CASES``.

Inputs are what the GPU sees (``hv``, ``bv`` complex64, ``hw`` and the window float32, ``wt`` and ``eps`` float64),
promoted exactly.  ``|b|^2`` is the float64 formula's ``re^2 + im^2`` of the float32 values (the reference forms it in
float32; library and oracle do not).  ``2 pi`` is formed in long double, and the phase of every transform is reduced
exactly in integers, ``(k n) mod nra``, before the angle is formed.

Measures (``u = 2**-53``).

``map`` and ``dirty_beam`` are normalised to the dirty beam at transit, so a row's own maximum is its scale:
``row_measure`` is, per row (pol, freq, el), ``max_ra |got - T| / max_ra |T|`` over the positions compared, and the
figure of a case is the largest over its rows.  A measure relative to the maximum of a whole output cannot see the
weak elevations of a beam that falls by many decades.  ``weight`` and ``dirty_beam_power``: ``element_measure``, the
relative error per element, largest over the case.

Acceptance (``accept``; part (b) of ``dirty_twin.accept``): ``e_gpu <= K e_ref + K u`` with ``e_ref`` the same figure of
the float64 oracle on the same inputs.  ``K = 4`` (``K_RADIX``) where the row transform is a radix transform -- the
margin of the dirty sweep for another summation order and fused multiply-adds -- and ``K = 8`` (``K_BLUESTEIN``) where
``nra`` goes through Bluestein: three transforms of at least twice the length and two chirp products, the margin
``test_gpu_powerspec.py`` takes from the SHT sweep.

Exact zeros: where the truth is exactly zero (a row without weight or beam, a (pol, freq) without data, a window that
vanishes on the row) the output is zero, as a value: ``-0.0`` is a zero on purpose, a row's ``-Im`` of a zero
transform being one.  Both measures return whether every such element is.  ``weight`` is the same bits at every RA of
a row (``constant_along_ra``).

Float32 stores.  ``analytic_beam_measure``: with ``S = (1 / nra) sum_k |b_k|`` the magnitude sum of a row, ``a_max =
max |2 pi u|`` its largest phase and ``B = (nra + 4 + a_max) 2**-52 S`` -- the ``hv`` rule of ``ringchain_twin.py``:
``nra`` for the accumulation (a direct sum's; an FFT's ``log2`` is inside it), 4 for the single roundings on the way
(``tan``, ``exp``, ``sincos``, the product), ``a_max`` for the rounding of the ``sincos`` argument -- each component
``got == float32(T)`` wherever ``float32(T - B) == float32(T + B)``; elsewhere ``|got - float32(T)|`` is at most one
float32 ulp of ``T`` (a component below ``B`` -- a sum that cancels in exact arithmetic -- takes ``2**-24 |T| + B`` and is
counted apart: no float64 evaluation determines its float32 value).  The share of the elements elsewhere is at most ``EXCLUDED_CAP = 1e-3``, which the frequencies
and separations of ``BEAM_CASES`` are chosen for (wide spectra: a mode far below ``S`` is all rounding noise of the
float64 transform).  ``window_measure``: equal to the truth rounded once (held to equality by the same rule, with ``B`` of four
terms), except where ``x`` lies within ``4 * 2**-53`` of 0 or 1 without being there exactly: either side of the edge is
accepted; at most 1e-3 of a table may be either.
"""

import numpy as np

LD = np.longdouble
TWO_PI = 8 * np.arctan(LD(1))
U53 = 2.0**-53
K_RADIX, K_BLUESTEIN = 4, 8
EXCLUDED_CAP = 1e-3
C_LIGHT = 299792458  # m / s
BEAM_COEF = {"X": 14.87857614, "Y": 9.95746878}
WINDOW_COEF = {"uniform": [1, 0, 0, 0], "hann": [0.5, -0.5, 0, 0], "nuttall": [0.355768, -0.487396, 0.144232, -0.012604]}


def inz(x):
    """``1 / x``, and 0 where ``x`` is 0."""
    x = np.asarray(x)
    return np.where(x == 0, x.dtype.type(0), 1 / np.where(x == 0, x.dtype.type(1), x))


# ------------------------------------------------------------------------------------------------ the transforms
def _circle(n):
    ang = TWO_PI * np.arange(n).astype(LD) / LD(n)
    return np.cos(ang), np.sin(ang)


def irfft_direct(xr, xi, n, ra=None):
    """``numpy.fft.irfft(xr + i xi, n=n)`` along the last axis at the positions ``ra`` (all ``n`` by default), as a direct
    long-double sum over the Hermitian extension: ``(1 / n) sum_k c_k (xr_k cos t - xi_k sin t)``, ``t = 2 pi ((k ra) mod
    n) / n``, ``c_k = 1`` for the DC bin and (even ``n``) the Nyquist bin, whose imaginary parts are dropped, 2 otherwise;
    modes beyond ``n // 2`` are not used and modes the input does not have are zero."""
    nk = min(xr.shape[-1], n // 2 + 1)
    k = np.arange(nk, dtype=np.int64)
    edge = (k == 0) | (2 * k == n)
    c = np.where(edge, LD(1), LD(2))
    xr = np.asarray(xr, dtype=LD)[..., :nk] * c
    xi = np.where(edge, LD(0), np.asarray(xi, dtype=LD)[..., :nk]) * c
    ra = np.arange(n, dtype=np.int64) if ra is None else np.asarray(ra, dtype=np.int64)
    ct, st = _circle(n)
    idx = (k[:, np.newaxis] * ra[np.newaxis, :]) % n
    return (np.matmul(xr, ct[idx]) - np.matmul(xi, st[idx])) / LD(n)


def dft_direct(zr, zi, n, kk):
    """Bins ``kk`` of the forward DFT ``sum_j z_j exp(-2 pi i j k / n)`` of the rows ``z [..., n]``: ``(re, im) [..., len(kk)]``."""
    ct, st = _circle(n)
    idx = (np.arange(n, dtype=np.int64)[:, np.newaxis] * np.asarray(kk, dtype=np.int64)[np.newaxis, :]) % n
    c, s = ct[idx], st[idx]
    return np.matmul(zr, c) + np.matmul(zi, s), np.matmul(zi, c) - np.matmul(zr, s)


# ------------------------------------------------------------------------------------------------ the deconvolver
def term_weights(hw, wt, mode, T=LD):
    """``(w, g)`` of every (m, sign, pol, freq, EW separation) term as the kernel's three modes define them, ``g = w^2
    var``.  Mode 0: ``w = wt[ew]`` (a normalised table) where the inverse variance is positive.  Modes 1, 2: the
    inverse variance times the keep-mask ``wt``, mode 1 normalised by its sum over the separations (zero sum: zero),
    both zero where that product is not positive.  ``var`` is the inverse of the (masked) inverse variance."""
    iv = np.asarray(hw).astype(T)
    wt = np.asarray(wt).astype(T)
    if mode == 0:
        w = np.where(iv > 0, wt, T(0))
    else:
        iv = iv * wt
        w = iv * inz(iv.sum(axis=-1, keepdims=True)) if mode == 1 else iv
        w = np.where(iv > 0, w, T(0))
    return w, w * w * np.where(iv > 0, inz(iv), T(0))


def deconvolve_truth(hv, hw, bv, wt, mode, eps, nra, window=None, skip=False, iref=0, ra=None):
    """``hv [nm, 2, npol, nfreq, new, nel]``, ``hw [nm, 2, npol, nfreq, new]``, ``bv [>= nm, ...]``, ``wt [new]``, ``eps
    [nfreq, nm]``, ``window [nfreq, nm, nel]`` or None.  Returns a dict of long-double arrays: ``map`` and ``dirty_beam``
    ``[npol, nfreq, len(ra), nel]`` (the layout of the outputs, at the positions ``ra``), ``weight`` and
    ``dirty_beam_power`` ``[npol, nfreq, nel]``.

        sum_w = sum_{+/-, ew} w |b|^2         C = eps + sum_w   (1 with `skip`)
        map_m = win sum conj(b) w h / C       dirty_m = win sum_w / C
        norm  = 1 / mean_m dirty_m   (of row `iref` with `skip`)
        map = irfft(map_m, nra) norm          dirty_beam = irfft(dirty_m, nra) norm
        weight = 1 / (0.5 sum_m (sqrt(sum w^2 |b|^2 var) win norm / ((mmax + 1) C))^2)
        dirty_beam_power = sum_ra dirty_beam^2 / nra

    with ``1 / 0 = 0`` throughout.  The last is taken from the modes (Parseval: ``sum_ra d^2 = (1 / nra) sum_k X_k^2`` over
    the Hermitian extension), which is the same number in exact arithmetic; the host test holds it against the sum."""
    nm, _, npol, nfreq, _, nel = hv.shape
    bv = np.asarray(bv)[:nm]
    w, g = term_weights(hw, wt, mode)
    w, g = w[..., np.newaxis], g[..., np.newaxis]
    hr, hi, br, bi = (np.asarray(a).astype(LD) for a in (hv.real, hv.imag, bv.real, bv.imag))
    b2 = br * br + bi * bi
    sum_w = (w * b2).sum(axis=(1, 4))  # [nm, npol, nfreq, nel]
    sg = (g * b2).sum(axis=(1, 4))
    mre = (w * (br * hr + bi * hi)).sum(axis=(1, 4))  # conj(b) h
    mim = (w * (br * hi - bi * hr)).sum(axis=(1, 4))
    C = np.ones_like(sum_w) if skip else np.asarray(eps).astype(LD).T[:, np.newaxis, :, np.newaxis] + sum_w
    ic = inz(C)
    win = LD(1) if window is None else np.asarray(window).astype(LD).transpose(1, 0, 2)[:, np.newaxis]
    mr, mi, dm = win * mre * ic, win * mim * ic, win * sum_w * ic
    norm = inz(dm.sum(axis=0) / LD(nm))  # [npol, nfreq, nel]
    if skip:
        norm = np.broadcast_to(norm[..., iref : iref + 1], norm.shape)
    q = np.sqrt(sg) * win * norm * inz(LD(nm) * C)
    m = np.arange(nm)
    cm = np.where((m == 0) | (2 * m == nra), LD(1), LD(2))[:, np.newaxis, np.newaxis, np.newaxis]
    rows = lambda x: np.moveaxis(x, 0, -1)  # [npol, nfreq, nel, nm]
    tmap = irfft_direct(rows(mr), rows(mi), nra, ra) * norm[..., np.newaxis]
    tdb = irfft_direct(rows(dm), np.zeros_like(rows(dm)), nra, ra) * norm[..., np.newaxis]
    return {"map": np.swapaxes(tmap, -1, -2), "dirty_beam": np.swapaxes(tdb, -1, -2), "weight": inz(LD(0.5) * (q * q).sum(axis=0)),
            "dirty_beam_power": norm * norm * (cm * dm * dm).sum(axis=0) / LD(nra) / LD(nra)}


def row_measure(got, T):
    """``got``, ``T`` ``[npol, nfreq, J, nel]``: ``(largest over the rows of max_ra |got - T| / max_ra |T|, got is zero
    wherever T is)``.  A row whose truth is zero everywhere has no figure; a non-finite element makes it infinite."""
    got = np.asarray(got)
    assert got.shape == T.shape, (got.shape, T.shape)
    zeros_ok = bool(np.all(got[T == 0] == 0))
    if not np.isfinite(got).all():
        return np.inf, zeros_ok
    scale = np.abs(T).max(axis=2)
    err = np.abs(got.astype(LD) - T).max(axis=2)
    live = scale > 0
    return (float((err[live] / scale[live]).max()) if live.any() else 0.0), zeros_ok


def element_measure(got, T):
    """``(largest |got - T| / |T| where T != 0, got is zero wherever T is)``; ``T`` is broadcast to ``got``."""
    got = np.asarray(got)
    T = np.broadcast_to(T, got.shape)
    zero = T == 0
    zeros_ok = bool(np.all(got[zero] == 0))
    if not np.isfinite(got).all():
        return np.inf, zeros_ok
    return (float((np.abs(got.astype(LD) - T)[~zero] / np.abs(T[~zero])).max()) if not zero.all() else 0.0), zeros_ok


def constant_along_ra(weight):
    """``weight [npol, nfreq, nra, nel]`` holds the same bits at every RA of a row."""
    b = np.ascontiguousarray(weight).view(np.uint64)
    return bool(np.all(b == b[:, :, :1, :]))


def accept(e_gpu, e_ref, K):
    """``e_gpu <= K e_ref + K 2**-53``."""
    return e_gpu <= K * e_ref + K * U53


def bluestein(nra):
    """``nra`` is no power of two: the row transform goes through Bluestein."""
    return nra & (nra - 1) != 0


def fft_length(nra):
    """The length ``M`` of the transforms behind a row of ``nra`` points: ``nra`` itself, or the power of two from ``2 nra - 1``."""
    return nra if not bluestein(nra) else 1 << int(2 * nra - 2).bit_length()


def sample_positions(nra, seed):
    """Every RA where ``nra <= 512``; on longer rows 64: both ends, the three around the middle and seeded ones."""
    if nra <= 512:
        return np.arange(nra)
    fixed = [0, 1, nra // 2 - 1, nra // 2, nra // 2 + 1, nra - 1]
    rest = np.setdiff1d(np.arange(nra), fixed)
    return np.sort(np.concatenate([fixed, np.random.default_rng([20261021, 9, nra, seed]).choice(rest, 64 - len(fixed), replace=False)]))


# the three varieties of input every shape is run with, one per weight mode (which mode takes which rotates with the shape):
# (p of the elevation profile 10**(-p |el|), window, one EW separation excluded, eps all zero, a (pol, freq) without weight)
VARIETIES = ((6, "none", False, False, False), (12, "random", True, False, True), (0, "row", False, True, False))


class Case:
    """One call of ``dmm_ringmap_deconvolve``: the inputs as the GPU sees them, drawn from a fixed seed.

    ``hv``, ``bv``: Gaussian times ``10**(-p |el|)``; one elevation's ``bv`` exactly zero where ``nel >= 3``.  ``hw``:
    ``U(0.5, 1.5) 10**U(-3, 3)``, a tenth of it exactly zero, 2 % negative (but for the groups that would cancel, below), and -- where the shape has room -- one ``m``
    without any weight, one (m, sign) without, one EW separation without.  ``eps [nfreq, nm]`` cycles along ``m`` through
    ``1e-9``, 1 and ``1e6`` times the median of the positive ``sum_w`` (or is zero everywhere).  ``wt``: mode 0 the
    natural table ``new - e`` normalised, modes 1 and 2 the keep-mask; with ``excl`` the last separation's entry is zero.
    ``window``: none, random float32 in [0, 1] with 30 % exact zeros ("random"), or the same with one elevation zero at
    every ``m`` ("row")."""

    def __init__(self, nm, oddra, nel, new, npol=1, nfreq=1, mode=0, variety=0, nm_beam=None, skip=False, iref=0):
        p, window, excl, eps_zero, dead_pf = VARIETIES[variety]
        self.nm, self.oddra, self.nel, self.new, self.npol, self.nfreq, self.mode = nm, bool(oddra), nel, new, npol, nfreq, mode
        self.nra = 2 * (nm - 1) + int(oddra)
        self.nm_beam = nm_beam or nm
        self.skip, self.iref, self.p = bool(skip), iref, p
        self.name = f"nm{nm}{'o' if oddra else 'e'}-el{nel}-ew{new}-pf{npol}x{nfreq}-mode{mode}-v{variety}" + (f"-nb{nm_beam}" if nm_beam else "") + (
            f"-skip{iref}" if skip else "")
        rng = np.random.default_rng([20261021, nm, int(oddra), nel, new, npol, nfreq, mode, variety])
        self.el = np.linspace(-0.9, 0.9, nel) if nel > 1 else np.zeros(1)
        prof = 10.0 ** (-p * np.abs(self.el))

        def gauss(n0):
            s = (n0, 2, npol, nfreq, new, nel)
            return ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) * prof).astype(np.complex64)

        self.hv, self.bv = gauss(nm), gauss(self.nm_beam)
        self.zero_el = 1 if nel >= 3 else None
        if self.zero_el is not None:
            self.bv[..., self.zero_el] = 0
        s = (nm, 2, npol, nfreq, new)
        hw = (rng.uniform(0.5, 1.5, s) * 10.0 ** rng.uniform(-3, 3, s)).astype(np.float32)
        u = rng.uniform(size=s)
        hw[u < 0.1] = 0
        hw[u > 0.98] *= -1
        if nm >= 4:
            hw[nm // 2] = 0
            hw[nm // 3, 1] = 0
        if new >= 3:
            hw[..., 1] = 0
        if dead_pf and npol * nfreq > 1:
            hw[:, :, npol - 1, nfreq - 1] = 0
        self.hw = hw
        keep = np.ones(new)
        if excl and new > 1:
            keep[new - 1] = 0
        if mode == 0:
            t = (new - np.arange(new)).astype(np.float64) * keep
            self.wt = t * (1.0 / t.sum())
        else:
            self.wt = keep
        self.excl = [new - 1] if excl and new > 1 else []
        # conditioning: mode 1 divides by the signed sum of a term's weights over the separations.  Where the draw makes
        # that sum cancel to less than a tenth of its magnitude sum, the group's negative weights become zeros -- 1 / sum
        # would amplify every rounding by more than ten, in the oracle as in the kernel, and the figures would measure the draw
        iv = hw.astype(np.float64) * keep
        cancels = np.abs(iv.sum(axis=-1, keepdims=True)) < 0.1 * np.abs(iv).sum(axis=-1, keepdims=True)
        hw[cancels & (hw < 0)] = 0
        w64, _ = term_weights(hw, self.wt, mode, np.float64)
        b64 = self.bv[:nm].real.astype(np.float64) ** 2 + self.bv[:nm].imag.astype(np.float64) ** 2
        sw = (w64[..., np.newaxis] * b64).sum(axis=(1, 4))
        med = float(np.median(sw[sw > 0])) if (sw > 0).any() else 1.0
        self.eps = np.zeros((nfreq, nm)) if eps_zero else np.ascontiguousarray(
            np.broadcast_to(med * np.array([1e-9, 1.0, 1e6])[np.arange(nm) % 3], (nfreq, nm)))
        self.window = None
        if window != "none":
            win = rng.uniform(0, 1, (nfreq, nm, nel)).astype(np.float32)
            win[rng.uniform(size=win.shape) < 0.3] = 0
            if window == "row":
                win[:, :, nel // 2] = 0
            self.window = win
        self.ra = sample_positions(self.nra, nm)
        self.K = K_BLUESTEIN if bluestein(self.nra) else K_RADIX

    def truth(self):
        return deconvolve_truth(self.hv, self.hw, self.bv, self.wt, self.mode, self.eps, self.nra, self.window, self.skip, self.iref, self.ra)

    def reference(self):
        """The four outputs of ``oracle.ringmap.deconvolve`` (float64) on these inputs, in the layouts of the GPU's."""
        return oracle_deconvolve(self)

    def figures(self, T, rmap, weight, dbp, db=None):
        """``{output: (figure, zeros exact)}`` of the measures for outputs in the GPU's layouts (``db`` may be None)."""
        f = {"map": row_measure(rmap[0][:, :, self.ra, :], T["map"]),
             "weight": element_measure(weight, T["weight"][:, :, np.newaxis, :]),
             "dirty_beam_power": element_measure(dbp[0], T["dirty_beam_power"])}
        if db is not None:
            f["dirty_beam"] = row_measure(db[0][:, :, self.ra, :], T["dirty_beam"])
        return f


def maker_weights(kind, weight_ew, new, exclude=()):
    """``(mode, wt)`` as the two makers hand them to the kernel: Tikhonov with the "natural" (``new - e``) or "uniform" table,
    excluded separations zero, normalised (mode 0), or with inverse-variance weights (mode 1, keep-mask); Wiener: the raw
    inverse variance (mode 2, keep-mask)."""
    keep = np.ones(new)
    keep[list(exclude)] = 0
    if kind == "wiener":
        return 2, keep
    if weight_ew == "inverse_variance":
        return 1, keep
    t = (np.ones(new) if weight_ew == "uniform" else (new - np.arange(new)).astype(np.float64)) * keep
    return 0, t * inz(t.sum())


def oracle_deconvolve(c):
    from oracle import ringmap as orm

    kind, weight_ew = (("tikhonov", "natural"), ("tikhonov", "inverse_variance"), ("wiener", "natural"))[c.mode]
    return orm.deconvolve(kind, c.hv.astype(np.complex128), c.hw.astype(np.float64), c.bv.astype(np.complex128), np.arange(c.nfreq), c.el, None,
                          c.oddra, exclude_cyl=c.excl, skip_deconvolution=c.skip, window=c.window, weight_ew=weight_ew, iref=c.iref, eps=c.eps)


def compare(case, T, ref, got, who):
    """Print ``e_gpu``, ``e_ref`` and their ratio per output, then assert the acceptance rule, the exact zeros, the finite
    buffers and the constant weight.  ``got``, ``ref``: ``(map, weight, dirty_beam_power, dirty_beam or None)``."""
    fg, fr = case.figures(T, *got), case.figures(T, *ref)
    bad = [f"NaN or Inf in output {i}" for i, a in enumerate(got) if a is not None and not np.isfinite(a).all()]
    for k, (e_gpu, zeros) in fg.items():
        e_ref = fr[k][0]
        print(f"ringmap {who} {case.name} {k}: e_gpu {e_gpu:.3g} e_ref {e_ref:.3g} ratio {e_gpu / e_ref if e_ref else float(e_gpu > 0):.3g} K {case.K}")
        if not accept(e_gpu, e_ref, case.K):
            bad.append(f"{k}: e_gpu {e_gpu:.3g} > {case.K} e_ref + {case.K} u, e_ref {e_ref:.3g}")
        if not zeros:
            bad.append(f"{k}: not zero where the truth is")
    # exact zeros over the whole arrays, not only at the positions compared
    dead = T["weight"] == 0  # rows without weight, beam or window
    for k, a in (("map", got[0][0]), ("weight", got[1])) + ((("dirty_beam", got[3][0]),) if got[3] is not None else ()):
        if np.any(np.moveaxis(a, 2, -1)[dead] != 0):
            bad.append(f"{k}: a row without weight is not zero at every RA")
    if not constant_along_ra(got[1]):
        bad.append("weight: not the same bits along RA")
    assert not bad, f"{who} {case.name}: " + "; ".join(bad)
    return fg, fr


# ---- the shapes: (nm, oddra, nel, new, npol, nfreq, nm_beam).  Each runs in the three weight modes, mode i with variety
# (i + its index in the table) % 3.
THREE_KERNEL = {
    # M = 1, 2, 4 and Bluestein at 16
    "shortest": [(nm, odd, nel, 1, 1, 1, None) for nm, odd in ((1, True), (2, False), (3, False), (4, True)) for nel in (1, 2)],
    # MT = 16 chunks, 64-elevation tiles, the 32 x 32 store; an odd row count: the lone row of k_rm_fft<2>
    "chunks": [(nm, odd, nel, 3, 1, 3, None) for nm in (15, 16, 17) for odd in (False, True) for nel in (63, 64, 65)],
    # 2, 8, 10, 64, 66, 80 terms
    "terms": [(9, False, 5, new, 1, 1, None) for new in (1, 4, 5, 32, 33, 40)],
    "bluestein": [(20, True, 9, 2, 1, 1, None), (129, True, 9, 2, 1, 1, None)],
    "long": [(2049, False, 3, 2, 1, 1, None)],        # nra 4096: a power of two too long for the single pass
    "twiddles": [(4097, False, 2, 1, 1, 1, None)],    # nra 8192: twiddles read from memory
    "bluestein8192": [(1025, True, 3, 2, 1, 1, None), (2048, True, 3, 2, 1, 1, None)],  # nra 2049, 4095
    "beam": [(33, False, 7, 2, 1, 1, 40), (33, False, 7, 2, 1, 1, 64)],  # nm_beam > nm
}
# the rows that run with skip_deconvolution too (iref at 0, the middle and nel - 1): the shortest, the two middle rows, both
# Bluestein lengths, and nra = 4096, whose 129 chunks take more than one lane trip of the row sums
SKIP = {k: THREE_KERNEL[k] for k in ("shortest", "chunks", "terms", "bluestein", "long")}
UNSUPPORTED = [(8193, False), (2049, True)]  # nra 16384, 4097

# single pass: (nm, nel, new, variants); variant 0 the 16-elevation forms, 2 the 8-elevation form
SINGLE_PASS = {
    "shortest": [(5, nel, new, (0, 2)) for nel in (1, 7, 8, 9, 17) for new in (1, 5)],
    "second_pass": [(nm, nel, 3, (0, 2)) for nm in (65, 129) for nel in (15, 16, 17, 33)],  # a second m pass with one live m
    "lds16": [(513, 9, 2, (0,))],                                      # nra 1024: the longest LDS-resident image
    "parked": [(1025, nel, 2, (0, 2)) for nel in (8, 9, 16, 17, 24)],  # nra 2048
}
# the 8-elevation form's block -> tile mapping, nm = 9: (nel, npol, nfreq) with 1, 2, 15, 16, 17, 33 tiles
TILE_MAP = [(8, 1, 1), (9, 1, 1), (8, 3, 5), (9, 2, 4), (8, 1, 17), (8, 3, 11)]


def cases_of(shape, index, **kw):
    """The three cases (modes 0, 1, 2) of a shape ``(nm, oddra, nel, new, npol, nfreq, nm_beam)``."""
    nm, odd, nel, new, npol, nfreq, nmb = shape
    return [Case(nm, odd, nel, new, npol, nfreq, mode, (mode + index) % 3, nmb, **kw) for mode in (0, 1, 2)]


# ------------------------------------------------------------------------------------------------ the window
# (nfreq, nm, nel); the last has more than 65536 x 256 elements: a second trip of the grid-stride loop
WINDOW_CASES = [(1, 1, 1), (2, 17, 5), (1, 2049, 8200)]
assert 2049 * 8200 > 65536 * 256


def window_limits(nfreq, nm, nel):
    """``(lo, hi) [nfreq, nel]`` float64: the first columns are integer limits, an empty window (``hi < lo``), ``lo < 0``,
    ``hi > nm`` and ``lo == hi``; the rest seeded, every fourth pair integers."""
    rng = np.random.default_rng([20261021, 7, nfreq, nm, nel])
    lo = rng.uniform(-0.2 * nm, 0.5 * nm, (nfreq, nel))
    hi = lo + rng.uniform(0.1 * nm, 0.8 * nm, (nfreq, nel)) + 1
    lo[:, ::4], hi[:, ::4] = np.floor(lo[:, ::4]), np.ceil(hi[:, ::4])
    special = [(1.0 if nm > 2 else 0.0, float(max(nm - 1, 1))), (5.0, 2.0), (-3.0, nm / 2 + 0.25), (0.5, nm + 7.0), (float(nm // 2), float(nm // 2))]
    for i, (a, b) in enumerate(special[:nel]):
        lo[:, i], hi[:, i] = a, b
    return lo, hi


def window_index(nfreq, nm, nel):
    """The flat positions of a table that are compared: all of a small one; of a large one the first and last 256 and
    4096 seeded ones."""
    n = nfreq * nm * nel
    if n <= 1 << 20:
        return np.arange(n)
    rng = np.random.default_rng([20261021, 8, nfreq, nm, nel])
    return np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), rng.integers(0, n, 4096)]))


def _window_ld(lo, hi, coef, nm, index, rounded=True):
    nfreq, nel = lo.shape
    index = np.arange(nfreq * nm * nel) if index is None else np.asarray(index, dtype=np.int64)
    e, m, f = index % nel, (index // nel) % nm, index // (nel * nm)
    l, h = np.asarray(lo).astype(LD)[f, e], np.asarray(hi).astype(LD)[f, e]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (m.astype(LD) - l) / (h - l)
        t = TWO_PI * x
        c = [LD(a) for a in np.asarray(coef, dtype=np.float64)]
        inside = c[0] + c[1] * np.cos(t) + c[2] * np.cos(2 * t) + c[3] * np.cos(3 * t)
        near = ((np.abs(x) <= 4 * U53) & (x != 0)) | ((np.abs(x - 1) <= 4 * U53) & (x != 1))
        near &= h > l
        if not rounded:
            return np.where((h > l) & (x >= 0) & (x <= 1), inside, LD(0)), near
        return np.where((h > l) & (x >= 0) & (x <= 1), inside, LD(0)).astype(np.float32), near, np.where(near, inside, LD(0)).astype(np.float32)


def window_truth(lo, hi, coef, nm, index=None):
    """``window[f, m, el] = sum_i coef_i cos(2 pi i x)``, ``x = (m - lo[f, el]) / (hi[f, el] - lo[f, el])``, zero outside ``0 <= x
    <= 1``, and everywhere unless ``lo < hi`` (the reference selects ``lo <= m <= hi`` first: ``hi < lo`` is an empty window, and at
    ``lo == hi`` its ``x`` is no number and the window zero): ``(the table rounded once to float32, near)``, ``near``
    marking ``x`` within ``4 * 2**-53`` of 0 or 1 but not there exactly.  With ``index`` (flat positions) only those
    elements; both are vectors."""
    return _window_ld(lo, hi, coef, nm, index)[:2]


def window_measure(got, lo, hi, coef, nm, index=None):
    """``got``: the float32 values at ``index``.  ``(elements outside the rule, the share of the elements not held to equality)``.
    The rule: ``got == float32(T)`` wherever ``T`` is at least ``B = (4 + 6 pi) 2**-52 sum_i |coef_i|`` from a float32 rounding
    boundary -- 4 for the four terms' products and sums, ``6 pi`` for the rounding of ``x`` in the cosine arguments up to
    ``6 pi x``; nearer than that ``|got - T| <= 2**-24 |T| + B`` (the window falls to zero at its edges: there ``B`` is many
    float32 ulps of it); and where ``x`` is within ``4 * 2**-53`` of an edge without being on it,
    either side's value (the cosine sum there, or zero)."""
    T, near, inside = _window_ld(lo, hi, coef, nm, index)
    got = np.asarray(got).reshape(-1)
    assert got.dtype == np.float32 and got.shape == T.shape
    Tl = _window_ld(lo, hi, coef, nm, index, rounded=False)[0]
    B = LD((4 + 6 * np.pi) * 2.0**-52 * np.abs(np.asarray(coef, dtype=np.float64)).sum())
    sure = ((Tl - B).astype(np.float32) == (Tl + B).astype(np.float32)) | (Tl == 0)
    ok = np.where(sure, got == T, np.abs(got.astype(LD) - Tl) <= LD(2.0**-24) * np.abs(Tl) + B)
    ok |= near & ((got == 0) | (got == inside))
    noise = (Tl != 0) & (np.abs(Tl) <= B)  # a sum that cancels (a window that vanishes at its edges): counted apart
    return int(np.count_nonzero(~ok)), float(((near | ~sure) & ~noise).mean())


def window_f64(lo, hi, coef, nm, index=None):
    """The same table as ``oracle.ringmap.get_window`` forms an element (float64, stored float32)."""
    nfreq, nel = lo.shape
    index = np.arange(nfreq * nm * nel) if index is None else np.asarray(index, dtype=np.int64)
    e, m, f = index % nel, (index // nel) % nm, index // (nel * nm)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (m - lo[f, e]) / (hi[f, e] - lo[f, e])
        t = 2 * np.pi * np.arange(4)[:, np.newaxis] * x[np.newaxis, :]
        w = (np.asarray(coef, dtype=np.float64)[:, np.newaxis] * np.cos(t)).sum(axis=0)
        return np.where((m >= lo[f, e]) & (m <= hi[f, e]) & (x >= 0) & (x <= 1), w, 0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the analytic beam
POLS = ("XX", "XY", "YX", "YY")
# (nra, mmax, nel, nfreq): four polarisations and three separations throughout.  The frequencies scale with nra, so that
# the beam is neither narrower than a sample nor its spectrum narrow against mmax: no mode drowns in the transform's rounding.
BEAM_CASES = [(1, 0, 1, 2), (8, 4, 5, 2), (39, 19, 5, 2), (128, 64, 5, 2), (2049, 1024, 1, 2), (128, 40, 1, 2), (39, 25, 5, 2)]
BEAM_EW = np.array([0.17, 0.31, 0.64])  # (no zero separation: its beam is real and even, half of its components cancel)


def beam_inputs(nra, mmax, nel, nfreq):
    """``(freq [MHz], ew [m], dec [rad], coef_a, coef_b [npol])`` float64; ``dec = arcsin(el)`` of evenly spaced ``el``."""
    f0 = 400.0 * nra / 128.0  # sigma nra = 3.4 (XX) ... 1.5 (YY at 1.5 f0): resolved by the samples, and wide in m
    freq = np.linspace(f0, 1.5 * f0, nfreq)
    dec = np.arcsin(np.linspace(-0.5, 0.55, nel) if nel > 1 else np.array([0.3]))
    return freq, BEAM_EW.copy(), dec, np.array([BEAM_COEF[p[0]] for p in POLS]), np.array([BEAM_COEF[p[1]] for p in POLS])


def analytic_beam_f64(freq, ew, dec, ca, cb, nra, mmax):
    """The same beam as ``oracle.ringmap.analytic_beam_mmodes`` forms it (float64, ``numpy.fft.fft``, stored complex64), for
    any ``mmax`` against ``nra``."""
    from oracle.transform import make_marray

    phi = np.radians(np.linspace(0.0, 360.0, nra, endpoint=False))
    out = np.zeros((mmax + 1, 2, len(ca), len(freq), len(ew), len(dec)), dtype=np.complex64)
    for fi, f in enumerate(freq):
        u_dec = (ew / (C_LIGHT * 1e-6 / f))[:, np.newaxis] * np.cos(dec)[np.newaxis, :]
        sa, sb = ca[:, np.newaxis] / f / np.cos(dec), cb[:, np.newaxis] / f / np.cos(dec)
        sig = sa * sb / (sa**2 + sb**2) ** 0.5
        with np.errstate(over="ignore"):
            amp = np.exp(-((2 * np.tan(phi / 2)) ** 2) / (2 * sig[:, np.newaxis, :, np.newaxis] ** 2))
        b = np.exp(2.0j * np.pi * u_dec[np.newaxis, :, :, np.newaxis] * np.sin(phi)) * amp
        out[:, :, :, fi] = make_marray(b.conj(), mmax=mmax, dtype=np.complex64)
    return out


def pack_limits(nra, mmax):
    """``(mlim, mlim_neg)``: the ``+m`` bins kept go up to ``min(nra // 2, mmax)``; the ``-m`` bins up to ``mmax``, or, where
    ``mmax >= nra // 2``, up to ``nra // 2 - 1 + nra % 2`` (the Nyquist bin lives on the ``+m`` side)."""
    return min(nra // 2, mmax), (nra // 2 - 1 + nra % 2) if mmax >= nra // 2 else mmax


def pack_live(nra, mmax):
    """``[mmax + 1, 2]``: the slots the pack fills."""
    mlim, mneg = pack_limits(nra, mmax)
    m = np.arange(mmax + 1)
    return np.stack([m <= mlim, (m >= 1) & (m <= mneg)], axis=1)


def analytic_beam_truth(freq, ew, dec, ca, cb, nra, mmax):
    """``(Tr, Ti, B)`` ``[mmax + 1, 2, npol, nfreq, new, nel]`` long double and ``B`` broadcastable to them: the transit beam
    ``conj(exp(2 pi i u cos(dec) sin(phi)) exp(-(2 tan(phi / 2))^2 / (2 sigma^2)))``, ``phi = 2 pi k / nra``, ``u = ew freq
    / c``, ``sigma = sa sb / sqrt(sa^2 + sb^2)``, ``s = coef / freq / cos(dec)``; its forward DFT over ``k`` times ``1 / nra``;
    slot ``(m, 0)`` bin ``m``, slot ``(m, 1)`` the conjugate of bin ``nra - m``, zero outside ``pack_limits``."""
    fr = np.asarray(freq).astype(LD)[np.newaxis, :, np.newaxis, np.newaxis]
    cd = np.cos(np.asarray(dec).astype(LD))[np.newaxis, np.newaxis, np.newaxis, :]
    u = np.asarray(ew).astype(LD)[np.newaxis, np.newaxis, :, np.newaxis] * fr * LD(10**6) / LD(C_LIGHT) * cd
    sa = np.asarray(ca).astype(LD)[:, np.newaxis, np.newaxis, np.newaxis] / fr / cd
    sb = np.asarray(cb).astype(LD)[:, np.newaxis, np.newaxis, np.newaxis] / fr / cd
    is2 = (sa * sa + sb * sb) / (2 * sa * sa * sb * sb) + 0 * u  # 1 / (2 sigma^2), [npol, nfreq, new, nel]
    u = u + 0 * is2
    ct, st = _circle(nra)
    with np.errstate(divide="ignore", over="ignore"):
        half = TWO_PI * np.arange(nra).astype(LD) / LD(2 * nra)
        t = 2 * np.tan(half)
    amp = np.exp(-(t * t) * is2[..., np.newaxis])
    ang = TWO_PI * u[..., np.newaxis] * st
    zr, zi = amp * np.cos(ang), -amp * np.sin(ang)
    mlim, mneg = pack_limits(nra, mmax)
    Tr, Ti = (np.zeros((mmax + 1, 2) + u.shape, dtype=LD) for _ in range(2))
    pr, pi = dft_direct(zr, zi, nra, np.arange(mlim + 1))
    Tr[: mlim + 1, 0], Ti[: mlim + 1, 0] = np.moveaxis(pr, -1, 0) / LD(nra), np.moveaxis(pi, -1, 0) / LD(nra)
    if mneg >= 1:
        nr, ni = dft_direct(zr, zi, nra, nra - np.arange(1, mneg + 1))
        Tr[1 : mneg + 1, 1], Ti[1 : mneg + 1, 1] = np.moveaxis(nr, -1, 0) / LD(nra), -np.moveaxis(ni, -1, 0) / LD(nra)
    S = amp.sum(axis=-1) / LD(nra)
    a_max = float(np.abs(TWO_PI * u).max())
    return Tr, Ti, LD((nra + 4 + a_max) * 2.0**-52) * S[np.newaxis, np.newaxis]


def analytic_beam_measure(got, Tr, Ti, B, nra):
    """``got`` complex64 ``[mmax + 1, 2, npol, nfreq, new, nel]``.  Per real component, three classes: *sure* (``T`` at least
    ``B`` from a float32 rounding boundary, or a slot the pack leaves zero: ``got == float32(T)``), *noise* (``|T| <= B``: a sum
    that cancels in exact arithmetic -- the beam is Hermitian in ``k``, so its transform is real and every imaginary part
    is such a sum: half of all components -- whose float32 value no float64 evaluation determines: ``|got - T| <= 2**-24 |T| + B``, the ``hv`` inequality) and *near*
    (the rest: within one float32 ulp of ``float32(T)``).  Returns ``(sure components that differ, near or noise components
    outside their tolerance, the share of the near ones, the share of the noise ones)``.  Only the first share is capped:
    the cap covers the near class alone, and an imaginary part is thereby checked as an absolute bound only -- ``B``,
    about ``nra 2**-52`` of the row's magnitude sum -- never as a rounded value."""
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == Tr.shape
    B = np.broadcast_to(B, Tr.shape)
    live = np.broadcast_to(pack_live(nra, Tr.shape[0] - 1).reshape((Tr.shape[0], 2) + (1,) * (Tr.ndim - 2)), Tr.shape)
    mismatch = loose = near = nnoise = 0
    for g, T in ((got.real, Tr), (got.imag, Ti)):
        lo, hi, t32 = (T - B).astype(np.float32), (T + B).astype(np.float32), T.astype(np.float32)
        noise = live & (np.abs(T) <= B)
        sure = ~live | ((lo == hi) & ~noise)
        rest = ~sure & ~noise
        mismatch += int(np.count_nonzero(sure & ~(g == t32)))
        ulp = np.spacing(np.abs(t32)).astype(np.float64)
        loose += int(np.count_nonzero(rest & ~(np.abs(g.astype(np.float64) - t32.astype(np.float64)) <= ulp)))
        loose += int(np.count_nonzero(noise & ~(np.abs(g.astype(LD) - T) <= LD(2.0**-24) * np.abs(T) + B)))
        near += int(np.count_nonzero(rest))
        nnoise += int(np.count_nonzero(noise))
    return mismatch, loose, near / (2.0 * got.size), nnoise / (2.0 * got.size)
