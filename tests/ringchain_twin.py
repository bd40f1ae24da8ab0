"""Long-double truths for the four producers of the ring-map chain in ``csrc/beamform.hip`` (``dmm_calc_redundancy``,
``dmm_vis_grid``, ``dmm_beamform_ns``, ``dmm_beamform_ew``), with the float64 restatements, the acceptance measures and
the case tables their tests share.  NumPy only.

* ``redundancy_exact``, ``vis_grid_exact``  the integer / copy semantics of the two grid kernels as plain gathers;
* ``beamform_ns_ld``   one frequency of BeamformNS in long double: weights, their norm over ``ns``, ``T = F (gv w)``, the
  dirty beam ``Re F w``, the noise weight, and the magnitude sums the bounds are made of;
* ``beamform_ew_ld``   BeamformEW in long double: rotation, inverse real DFT over the EW baselines written out as a sum,
  variance propagation, and the magnitude sum ``A``;
* ``beamform_ns_f64``, ``beamform_ew_f64``  the float64 restatements in the style of ``oracle/ringmap.py`` (matmul,
  ``numpy.fft.irfft``): they show without a GPU that the bounds are fair;
* ``NsCase``, ``EwCase``, ``redundancy_case``, ``vis_grid_case`` and the tables ``NS_SWEEP``, ``EW_SWEEP``, ``GRID_SWEEP``:
  the inputs, drawn from fixed seeds, as the GPU sees them (``gv`` complex64, ``gw`` float32, ``gr`` int32; positions,
  elevations, inverse wavelengths, window table, rotation and EW weights float64).  The truths convert exactly these
  to long double; ``2 pi`` is formed in long double; the EW twiddle angle is ``2 pi ((x b) mod nbeam) / nbeam``.

Measures, all derived (``u = 2**-53``); nothing of the code under test enters a bound.

Grid stage: bit for bit.

NS ``hv`` (per real and imaginary component) and dirty beam (``gv -> 1``), stored as float32:
``|got - T| <= 2**-24 |T| + B``, ``B = (ny + 4 + a_max) 2**-52 S``, ``S[t] = sum_y |gv[y, t]| |w^[y, t]|`` (``sum_y |w^|`` for the
dirty beam), ``a_max = max |2 pi ns el / lambda|``.  The first term is the one rounding to float32.  ``B`` covers the
float64 work before it, in units of ``2 u`` of the magnitude sum: ``ny`` for the accumulation over ``ns``, 4 for the single
roundings on the way (``1 / norm``, ``w / norm``, ``gv w``, ``sincos``), and ``a_max`` for the rounding of the ``sincos``
argument, which moves ``F`` by about ``u`` times the angle per factor of it.  In addition the store is the truth rounded once: ``got == float32(T)`` wherever ``float32(T
- B) == float32(T + B)``; the other elements (``T`` within ``B`` of a rounding boundary) stay in the inequality, and their
share may be at most ``EXCLUDED_CAP = 1e-3`` of a case's components.  Equality is of values (``-0.0 == 0.0``).

NS ``hw`` (float32): ``|got - T| <= (2**-24 + (2 ny + 8) 2**-52) |T|``, and exactly 0 where the truth is 0.

EW ``map`` and dirty beam (float64): ``|got - T| <= (2 nx + 8) 2**-52 A``, ``A = sum_x fac_x sum_q |P_q| (|Re h_q| + |Im h_q|)``.
EW ``weight``, ``rms``: relative error at most ``(nx + 8) 2**-52``, exactly 0 where ``rv = 0``.

Every buffer must be finite everywhere (the GPU tests pre-fill them with NaN).

Inputs.  Where a case has more than one ``(pol, x, t)`` column, one of them has no positive weight at any ``ns``: its
``hv``, dirty beam and ``hw`` must be exactly zero.  Case A is a single column of a single term, which stays live (a
case with nothing but zeros is Z).  A tenth of the weights is zero and a few are negative; both count as masked.

Measured: ``test_ringchain_twin_host.py`` tabulates the float64 restatements per case, ``test_gpu_ringchain_direct.py``
the kernels.  Before the store the float64 restatement uses 0.06 … 0.25 of ``B``, at most 0.15 of ``hw``'s accumulation
term, 0.02 … 0.12 of the EW map bound and at most 0.12 of ``(nx + 8) 2**-52``.
"""

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
C_LIGHT = 299792458.0  # m / s
TWO_PI = 8 * np.arctan(LD(1))
EXCLUDED_CAP = 1e-3
INV_VAR, NATURAL, WINDOW = 0, 1, 2

# name -> (npol, nfreq, nx, ny, nra, npix, mode, include_auto, dirty): the GEMM tiles are 16 (ns) x 64 (el) x 64 (ra)
NS_SWEEP = {
    "A": (1, 1, 1, 1, 1, 1, INV_VAR, 1, True),       # one term; everything padded
    "B": (2, 2, 2, 15, 63, 63, NATURAL, 0, False),   # one under every tile; two frequencies
    "C": (1, 1, 3, 16, 64, 64, WINDOW, 0, True),     # exact multiples: the no-memset path
    "D": (1, 2, 1, 17, 65, 65, INV_VAR, 0, True),    # one past every tile; a 2nd K chunk with one live row
    "E": (1, 1, 2, 16, 65, 1, NATURAL, 1, False),    # only nra padded; one elevation
    "F": (1, 1, 1, 33, 64, 130, WINDOW, 0, False),   # only ny padded; three K chunks, three elevation tiles
    "G": (4, 1, 8, 5, 130, 7, INV_VAR, 0, True),     # 32 (pol, ew) planes
    "Z": (1, 1, 1, 1, 3, 2, INV_VAR, 0, True),       # nx = ny = 1 without the autos: everything is zero
}
# the call that fills the xw scratch with NaN before case B runs on the same context: at least B's scratch bytes, the
# same npix (so the same offset of xw), no padding of its own
NS_POISON = (2, 2, 2, 16, 128, 63, INV_VAR, 1, False)

FOUR = ("XX", "XY", "YX", "YY")
# name -> (pols, nfreq, nx, nel, nra, single, dirty, weight_ew, exclude_intracyl, flag_ew): tiles of 32 (el) x 32 (ra)
EW_SWEEP = {
    "nbeam1": (("XX",), 1, 1, 1, 1, False, False, "natural", False, None),
    "nbeam3": (FOUR, 2, 2, 31, 33, False, True, "uniform", True, None),
    "nbeam7": (FOUR, 1, 4, 32, 32, False, False, "natural", False, (1, 1, 0, 1)),  # the largest the 8-beam kernel takes
    "nbeam9": (FOUR, 1, 5, 33, 65, False, True, "natural", True, None),            # the first of the 16-beam kernel
    "nbeam15": (("XX", "YY"), 1, 8, 65, 31, False, False, "uniform", False, None),  # three elevation blocks
    "single8": (FOUR, 1, 8, 7, 40, True, False, "natural", False, None),
    "single3": (("XY", "YX"), 1, 3, 1, 97, True, True, "uniform", False, None),     # rotation rows only
}

# the grid kernels run 256 threads a block in at most 65536 blocks: one more element than that takes a second trip
GRID_TRIP = 65536 * 256
GRID_SWEEP = {
    "redundancy": [(23, nra, all_good) for nra in (1, 63, 257) for all_good in (0, 1)],  # (nprod, nra, all_good)
    "redundancy_large": (300, 56000, 0),
    "vis_grid": [(nfreq, 63, with_red) for nfreq in (1, 3) for with_red in (False, True)],  # (nfreq, nra, grid_red)
    "vis_grid_large": (3, 140000, True),
}
GRID_NINPUT, GRID_NSTACK, GRID_NPOL, GRID_NCELL_POL = 6, 7, 4, 10
assert GRID_SWEEP["redundancy_large"][0] * GRID_SWEEP["redundancy_large"][1] > GRID_TRIP
assert GRID_NPOL * GRID_NCELL_POL * GRID_SWEEP["vis_grid_large"][0] * GRID_SWEEP["vis_grid_large"][1] > GRID_TRIP


def invert_no_zero(x):
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, x.dtype.type(0), 1 / np.where(x == 0, x.dtype.type(1), x))


# ---------------------------------------------------------------------------------------------------- the grid stage
def redundancy_exact(flags, pa, pb, stack, nstack, all_good):
    """``redundancy [nstack][nra]`` float32: for every stack the sum, over the products it holds, of ``flags[a] flags[b]``
    (1 with ``all_good``).  Stack indices outside ``[0, nstack)`` are skipped, and without ``all_good`` so is a product
    with an input outside ``[0, ninput)``."""
    flags = np.asarray(flags, dtype=np.float32)
    ninput, nra = flags.shape
    pa, pb, stack = (np.asarray(a, dtype=np.int64) for a in (pa, pb, stack))
    ok = np.ones(len(stack), dtype=bool) if all_good else (pa >= 0) & (pa < ninput) & (pb >= 0) & (pb < ninput)
    red = np.zeros((nstack, nra), dtype=np.float32)
    for s in range(nstack):
        sel = np.flatnonzero(ok & (stack == s))
        if all_good:
            red[s] = len(sel)
        elif len(sel):
            red[s] = (flags[pa[sel]] * flags[pb[sel]]).sum(axis=0, dtype=np.float32)  # (0 / 1 summands: exact)
    return red


def vis_grid_exact(vis, weight, red, src, conj, npol, ncell_pol):
    """``(gv [npol][nfreq][ncell_pol][nra], gw, gr [npol][ncell_pol][nra] or None)``: cell ``c`` takes stack ``src[c]``,
    the imaginary part negated where ``conj[c]``; ``src = -1`` cells are zero; ``gr`` is the redundancy cast to int32."""
    s = np.asarray(src).reshape(npol, ncell_pol)
    cj = np.asarray(conj).reshape(npol, 1, ncell_pol, 1) != 0
    live = (s >= 0)[:, np.newaxis, :, np.newaxis]
    sc = np.where(s >= 0, s, 0)
    gv = np.asarray(vis)[:, sc, :].transpose(1, 0, 2, 3)
    gv = np.where(live, np.where(cj, gv.real - 1j * gv.imag, gv), 0).astype(np.complex64)
    gw = np.where(live, np.asarray(weight)[:, sc, :].transpose(1, 0, 2, 3), 0).astype(np.float32)
    gr = None if red is None else np.where(live[:, 0], np.asarray(red)[sc], 0).astype(np.int32)
    return gv, gw, gr


def redundancy_case(nprod, nra, all_good):
    """``(flags, pa, pb, stack)``: stack indices -1 and ``nstack`` among the products, two products with an input the
    flag table does not have; with ``all_good`` the flag table is all zero."""
    rng = np.random.default_rng([20261019, 3, nprod, nra, all_good])
    pa = rng.integers(0, GRID_NINPUT, nprod).astype(np.int32)
    pb = rng.integers(0, GRID_NINPUT, nprod).astype(np.int32)
    stack = rng.integers(0, GRID_NSTACK, nprod).astype(np.int32)
    stack[3], stack[11] = -1, GRID_NSTACK
    pa[5], pb[17] = GRID_NINPUT, -1
    stack[5] = stack[17] = 2  # (inside the table, so that only the input check can skip them)
    flags = np.zeros((GRID_NINPUT, nra), np.float32) if all_good else rng.integers(0, 2, (GRID_NINPUT, nra)).astype(np.float32)
    return flags, pa, pb, stack


def vis_grid_case(nfreq, nra):
    """``(vis, weight, red, src, conj)``: empty cells, a stack in several cells, conjugated cells."""
    rng = np.random.default_rng([20261019, 4, nfreq, nra])
    shape = (nfreq, GRID_NSTACK, nra)
    vis = (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)
    weight = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    red = rng.integers(0, 30, (GRID_NSTACK, nra)).astype(np.float32)
    ncell = GRID_NPOL * GRID_NCELL_POL
    src = rng.integers(-1, GRID_NSTACK, ncell).astype(np.int32)
    conj = rng.integers(0, 2, ncell).astype(np.uint8)
    src[0], src[1], src[2], src[ncell - 1] = -1, 3, 3, -1
    conj[0], conj[1], conj[2] = 1, 1, 0
    return vis, weight, red, src, conj


# ---------------------------------------------------------------------------------------------------- BeamformNS
def _ns_weights(gw, gr, row, mode, include_auto, T):
    """The weights over ``ns`` before their normalisation, ``[npol][nx][ny][nra]`` in type ``T``."""
    if mode == INV_VAR:
        w = gw.astype(T)
    elif mode == NATURAL:
        w = gr.astype(T)
    else:
        w = np.broadcast_to(np.asarray(row).astype(T)[np.newaxis, np.newaxis, :, np.newaxis], gw.shape)
    w = np.where(gw > 0, w, T(0))
    if not include_auto:
        w[:, 0, 0, :] = 0
    return w


def beamform_ns_ld(gv, gw, gr, row, nspos, el, iwv, mode, include_auto):
    """One frequency in long double.  ``gv`` complex64 and ``gw`` float32 ``[npol][nx][ny][nra]``, ``gr`` int32 the same,
    ``row [ny]`` the window weights of this frequency.  Returns ``(T [npol][nx][npix][nra] complex, Tb the dirty beam,
    hw [npol][nx][nra], S, Sb [npol][nx][nra], a_max)``."""
    w = _ns_weights(gw, gr, row, mode, include_auto, LD)
    wh = w * invert_no_zero(w.sum(axis=2, keepdims=True))
    ang = TWO_PI * np.asarray(nspos).astype(LD)[np.newaxis, :] * np.asarray(el).astype(LD)[:, np.newaxis] * LD(iwv)
    c, s = np.cos(ang), np.sin(ang)
    xr, xi = gv.real.astype(LD) * wh, gv.imag.astype(LD) * wh
    T = np.empty(gw.shape[:2] + (len(el), gw.shape[3]), dtype=CLD)  # F = c - i s
    T.real = np.matmul(c, xr) + np.matmul(s, xi)
    T.imag = np.matmul(c, xi) - np.matmul(s, xr)
    Tb = np.matmul(c, wh)
    gwl = gw.astype(LD)
    hw = invert_no_zero(np.where(gw != 0, wh * wh / np.where(gw != 0, gwl, LD(1)), LD(0)).sum(axis=2))
    mag = np.hypot(gv.real.astype(LD), gv.imag.astype(LD))
    return T, Tb, hw, (mag * np.abs(wh)).sum(axis=2), np.abs(wh).sum(axis=2), float(np.abs(ang).max())


def beamform_ns_f64(gv, gw, gr, row, nspos, el, iwv, mode, include_auto, store=True):
    """The same frequency as ``oracle.ringmap.beamform_ns(precision=64)`` forms it, every weight kept in float64:
    ``(hv complex64, hb float32, hw float32)``, rounded once at the end as the kernel's stores are (``store=False``:
    left in float64)."""
    w = _ns_weights(gw, gr, row, mode, include_auto, np.float64)
    w = w * invert_no_zero(w.sum(axis=2, keepdims=True))
    phase = 2.0 * np.pi * np.asarray(nspos)[np.newaxis, :] * np.asarray(el)[:, np.newaxis]
    F = np.exp(-1.0j * phase * iwv)
    hv = np.matmul(F, gv * w)
    hb = np.matmul(F, w.astype(np.complex128)).real
    hw = invert_no_zero(np.sum(invert_no_zero(gw.astype(np.float64)) * w**2, axis=2))
    if not store:
        return hv, hb, hw
    return hv.astype(np.complex64), hb.astype(np.float32), hw.astype(np.float32)


def ns_bound(ny, a_max, S):
    """``B = (ny + 4 + a_max) 2**-52 S``."""
    return LD((ny + 4 + a_max) * 2.0**-52) * S


def rounded_measure(got, T, B):
    """A float32 store ``got`` of the real long-double truth ``T`` with accumulation bound ``B``: ``(worst |got - T| /
    (2**-24 |T| + B), elements that differ from float32(T) although T is at least B from a rounding boundary, the
    share of the elements that are nearer)``.  0 / 0 counts as 0; a non-finite element makes the ratio infinite."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    B = np.broadcast_to(B, T.shape)
    lo, hi = (T - B).astype(np.float32), (T + B).astype(np.float32)
    sure = lo == hi
    mismatch = int(np.count_nonzero(sure & ~(got == lo)))
    if not np.isfinite(got).all():
        return np.inf, mismatch, float(1.0 - sure.mean())
    err, bound = np.abs(got.astype(LD) - T), LD(2.0**-24) * np.abs(T) + B
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, LD(0), err / bound)
    return float(q.max()), mismatch, float(1.0 - sure.mean())


def relative_measure(got, T):
    """``(worst |got - T| / |T| where T != 0, got is exactly 0 wherever T is)``; non-finite: infinite."""
    got = np.asarray(got)
    T = np.broadcast_to(T, got.shape)
    zero = T == 0
    zeros_ok = bool(np.all(got[zero] == 0))
    if not np.isfinite(got).all():
        return np.inf, zeros_ok
    if zero.all():
        return 0.0, zeros_ok
    return float((np.abs(got.astype(LD) - T)[~zero] / np.abs(T[~zero])).max()), zeros_ok


class NsCase:
    """One BeamformNS call: the inputs as the GPU sees them and the long-double truth of every frequency."""

    def __init__(self, shape):
        self.shape = shape
        npol, nfreq, nx, ny, nra, npix, mode, include_auto, dirty = shape
        self.npol, self.nfreq, self.nx, self.ny, self.nra, self.npix = npol, nfreq, nx, ny, nra, npix
        self.mode, self.include_auto, self.dirty = mode, include_auto, dirty
        rng = np.random.default_rng([20261019, 1, npol, nfreq, nx, ny, nra, npix, mode])
        s = (npol, nfreq, nx, ny, nra)
        self.gv = (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
        gw = rng.uniform(0.5, 1.5, s).astype(np.float32)
        gw[rng.uniform(size=s) < 0.1] = 0
        gw.reshape(-1)[rng.choice(gw.size, size=min(3, gw.size // 8), replace=False)] = -0.75  # masked like zeros
        # one (pol, x, t) column masked at every ns and frequency (where there is more than one column to begin with)
        self.masked = (npol - 1, nx - 1, nra // 2) if npol * nx * nra > 1 else None
        if self.masked:
            gw[npol - 1, :, nx - 1, :, nra // 2] = 0
        if not (gw > 0).any():
            gw.reshape(-1)[0] = 1.0
        self.gw = gw
        self.gr = rng.integers(0, 20, (npol, nx, ny, nra)).astype(np.int32)
        self.nspos = np.fft.fftfreq(ny, d=1.0 / (ny * 0.3048))
        self.el = 0.95 * np.linspace(-1.0, 1.0, npix)
        self.freq = np.linspace(450.0, 750.0, nfreq)
        self.iwv = np.ascontiguousarray(self.freq * 1e6 / C_LIGHT)
        self.table = None
        if mode == WINDOW:  # a Hamming window over the NS extent, narrower at the higher frequencies
            nsmax = np.abs(self.nspos).max()
            x = 0.5 * (self.nspos[np.newaxis, :] * self.iwv[:, np.newaxis] / (nsmax * self.iwv.max()) + 1) if nsmax > 0 else np.full((nfreq, ny), 0.5)
            self.table = np.ascontiguousarray(0.53836 - 0.46164 * np.cos(2 * np.pi * x))
        per = [beamform_ns_ld(self.gv[:, f], gw[:, f], self.gr, None if self.table is None else self.table[f], self.nspos, self.el,
                              self.iwv[f], mode, include_auto) for f in range(nfreq)]
        self.T, self.Tb, self.hw, S, Sb = (np.stack([p[i] for p in per], axis=1) for i in range(5))
        self.a_max = [p[5] for p in per]
        # B [npol][nfreq][nx][1][nra], the same for every elevation
        self.B = np.stack([ns_bound(ny, self.a_max[f], S[:, f]) for f in range(nfreq)], axis=1)[:, :, :, np.newaxis, :]
        self.Bb = np.stack([ns_bound(ny, self.a_max[f], Sb[:, f]) for f in range(nfreq)], axis=1)[:, :, :, np.newaxis, :]
        self.hw_rel = 2.0**-24 + (2 * ny + 8) * 2.0**-52

    def reference(self, store=True):
        """``(hv, hb, hw)`` of the float64 restatement, in the GPU's layouts."""
        per = [beamform_ns_f64(self.gv[:, f], self.gw[:, f], self.gr, None if self.table is None else self.table[f], self.nspos, self.el,
                               self.iwv[f], self.mode, self.include_auto, store) for f in range(self.nfreq)]
        return tuple(np.stack([p[i] for p in per], axis=1) for i in range(3))

    def measure(self, hv, hw, hb=None):
        """Every figure of the NS measures for the outputs ``hv`` complex64, ``hw`` float32, ``hb`` float32 or None."""
        hv = np.asarray(hv)
        assert hv.dtype == np.complex64 and hv.shape == self.T.shape
        parts = [rounded_measure(np.ascontiguousarray(hv.real), self.T.real, self.B), rounded_measure(np.ascontiguousarray(hv.imag), self.T.imag, self.B)]
        m = {"hv": max(p[0] for p in parts), "hv_mismatch": sum(p[1] for p in parts), "hv_excluded": 0.5 * (parts[0][2] + parts[1][2])}
        m["hw"], m["hw_zeros"] = relative_measure(hw, self.hw)
        m["hw"] /= self.hw_rel
        if hb is not None:
            m["hb"], m["hb_mismatch"], m["hb_excluded"] = rounded_measure(hb, self.Tb, self.Bb)
        return m

    def check(self, who, hv, hw, hb=None):
        """Print the figures (error / bound: at most 1 passes), then assert the measures of the module docstring."""
        m = self.measure(hv, hw, hb)
        print(f"ringchain ns {who}: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
        assert m["hv"] <= 1.0 and m["hw"] <= 1.0 and m["hw_zeros"], (who, m)
        assert m["hv_mismatch"] == 0 and m["hv_excluded"] <= EXCLUDED_CAP, (who, m)
        if hb is not None:
            assert m["hb"] <= 1.0 and m["hb_mismatch"] == 0 and m["hb_excluded"] <= EXCLUDED_CAP, (who, m)
        if self.masked:  # no weight anywhere in the column: exactly zero
            p, x, t = self.masked
            assert not np.asarray(hv)[p, :, x, :, t].any() and not np.asarray(hw)[p, :, x, t].any(), who
            assert hb is None or not np.asarray(hb)[p, :, x, :, t].any(), who
        return m


# ---------------------------------------------------------------------------------------------------- BeamformEW
def ew_weights(nx, weight_ew, exclude_intracyl, single, flag_ew):
    """The normalised EW weights, formed as ``BeamformEW.process`` forms them."""
    w = np.ones(nx) if weight_ew == "uniform" else (nx - np.arange(nx)).astype(np.float64)
    if exclude_intracyl:
        w[0] = 0.0
    if flag_ew is not None and np.size(flag_ew) == nx:
        w = w * np.asarray(flag_ew).astype(bool).astype(w.dtype)
    if single:
        w[1:] *= 2
    return w / w.sum()


def beamform_ew_ld(h, hw, P, w, single):
    """BeamformEW in long double.  ``h [npol_in][nfreq][nx][nel][nra]`` complex64 (or the real float32 dirty beam), ``hw
    [npol_in][nfreq][nx][nra]`` float32, ``P [npol_out][npol_in]`` complex128, ``w [nx]`` float64.  Returns ``(T [nbeam]
    [npol_out][nfreq][nra][nel], A [npol_out][nfreq][nra][nel], rv [npol_out][nfreq][nra])``: the map, the magnitude sum
    of its bound and the propagated variance (``weight = invert_no_zero(rv)``, ``rms = sqrt(rv)``)."""
    h, P = np.asarray(h), np.asarray(P)
    nx = h.shape[2]
    nbeam = 1 if single else 2 * nx - 1
    pr, pi = P.real.astype(LD), P.imag.astype(LD)
    hr, hi = h.real.astype(LD), h.imag.astype(LD)
    vr = np.einsum("pq,qfxet->pfxet", pr, hr) - np.einsum("pq,qfxet->pfxet", pi, hi)
    vi = np.einsum("pq,qfxet->pfxet", pr, hi) + np.einsum("pq,qfxet->pfxet", pi, hr)
    wl = np.asarray(w).astype(LD)
    fac = np.where((np.arange(nx) == 0) | bool(single), wl, 2 * wl)
    k = np.outer(np.arange(nx), np.arange(nbeam)) % nbeam
    ang = TWO_PI * k.astype(LD) / LD(nbeam)
    T = np.einsum("x,pfxet,xb->bpfte", fac, vr, np.cos(ang)) - np.einsum("x,pfxet,xb->bpfte", fac, vi, np.sin(ang))
    A = np.einsum("x,pq,qfxet->pfte", np.abs(fac), np.hypot(pr, pi), np.abs(hr) + np.abs(hi))
    rv = LD(0.5) * np.einsum("x,pq,qfxt->pft", wl * wl, pr * pr + pi * pi, invert_no_zero(np.asarray(hw).astype(LD)))
    return T, A, rv


def beamform_ew_f64(h, hw, P, w, single):
    """The same in float64 as ``oracle.ringmap.beamform_ew`` forms it (``tensordot``, ``numpy.fft.irfft``), the rotation
    kept in complex128: ``(map, weight [npol_out][nfreq][nra][nel], rms)``."""
    h, P, w = np.asarray(h), np.asarray(P, dtype=np.complex128), np.asarray(w, dtype=np.float64)
    nx, nel = h.shape[2], h.shape[3]
    nbeam = 1 if single else 2 * nx - 1
    v = np.tensordot(P, h.astype(np.complex128), axes=(1, 0)) * w[:, np.newaxis, np.newaxis]  # [pol][freq][x][el][ra]
    m = np.sum(v.real, axis=2)[:, :, np.newaxis] if single else np.fft.irfft(v, nbeam, axis=2) * nbeam
    var = np.tensordot(np.abs(P) ** 2, invert_no_zero(np.asarray(hw).astype(np.float64)), axes=(1, 0))
    rv = 0.5 * np.sum(w[:, np.newaxis] ** 2 * var, axis=2)
    weight = np.repeat(invert_no_zero(rv)[..., np.newaxis], nel, axis=-1)
    return np.ascontiguousarray(m.transpose(2, 0, 1, 4, 3)), weight, np.sqrt(rv)


def ew_measure(nx, T, A, rv, rmap=None, weight=None, rms=None):
    """``error / bound`` of whichever of the EW outputs are given (float64): ``map`` (or the dirty beam) against ``T``
    and ``(2 nx + 8) 2**-52 A``; ``weight`` and ``rms`` relative to ``(nx + 8) 2**-52``, with their zeros exact."""
    m = {}
    if rmap is not None:
        rmap = np.asarray(rmap)
        assert rmap.dtype == np.float64 and rmap.shape == T.shape
        if not np.isfinite(rmap).all():
            m["map"] = np.inf
        else:
            err, bound = np.abs(rmap.astype(LD) - T), LD((2 * nx + 8) * 2.0**-52) * np.broadcast_to(A, T.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                m["map"] = float(np.where(err == 0, LD(0), err / bound).max())
    rel = (nx + 8) * 2.0**-52
    if weight is not None:
        assert np.asarray(weight).dtype == np.float64
        m["weight"], m["weight_zeros"] = relative_measure(weight, invert_no_zero(rv)[..., np.newaxis])
        m["weight"] /= rel
    if rms is not None:
        assert np.asarray(rms).dtype == np.float64
        m["rms"], m["rms_zeros"] = relative_measure(rms, np.sqrt(rv))
        m["rms"] /= rel
    return m


class EwCase:
    """One BeamformEW call: ``hv`` complex64 standard normal, ``hw`` float32 in [0.5, 1.5] with a tenth of it zero and,
    where there is more than one, one RA column all zero; ``hb`` a float32 dirty beam where the case has one; ``P`` from
    ``BeamformEW._get_pol`` and ``w`` from ``ew_weights``."""

    def __init__(self, shape):
        from draco_amd.analysis.ringmapmaker import BeamformEW

        self.shape = shape
        pols, nfreq, nx, nel, nra, single, dirty, weight_ew, exclude_intracyl, flag_ew = shape
        self.nfreq, self.nx, self.nel, self.nra, self.single, self.dirty = nfreq, nx, nel, nra, bool(single), bool(dirty)
        self.nbeam = 1 if single else 2 * nx - 1
        self.pol_out, rot = BeamformEW._get_pol(pols)
        self.P = np.ascontiguousarray(rot, dtype=np.complex128)
        self.npol_out, self.npol_in = self.P.shape
        assert self.npol_in == len(pols)
        self.w = ew_weights(nx, weight_ew, exclude_intracyl, single, flag_ew)
        rng = np.random.default_rng([20261019, 2, len(pols), nfreq, nx, nel, nra, int(single)])
        s = (self.npol_in, nfreq, nx, nel, nra)
        self.hv = (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
        hw = rng.uniform(0.5, 1.5, (self.npol_in, nfreq, nx, nra)).astype(np.float32)
        hw[rng.uniform(size=hw.shape) < 0.1] = 0
        self.dead = nra // 2 if nra > 1 else None
        if self.dead is not None:
            hw[..., self.dead] = 0
        self.hw = hw
        self.hb = rng.standard_normal(s).astype(np.float32) if dirty else None
        self.T, self.A, self.rv = beamform_ew_ld(self.hv, hw, self.P, self.w, single)
        if dirty:
            self.Tb, self.Ab, _ = beamform_ew_ld(self.hb, hw, self.P, self.w, single)

    def reference(self):
        """``(map, weight, rms, dirty beam or None)`` of the float64 restatement."""
        m, wt, rms = beamform_ew_f64(self.hv, self.hw, self.P, self.w, self.single)
        return m, wt, rms, beamform_ew_f64(self.hb, self.hw, self.P, self.w, self.single)[0] if self.dirty else None

    def check(self, who, rmap, weight, rms, rdb=None):
        m = ew_measure(self.nx, self.T, self.A, self.rv, rmap, weight, rms)
        if self.dirty:
            m["dirty_beam"] = ew_measure(self.nx, self.Tb, self.Ab, self.rv, rdb)["map"]
        print(f"ringchain ew {who}: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
        assert m["map"] <= 1.0 and m["weight"] <= 1.0 and m["rms"] <= 1.0 and m["weight_zeros"] and m["rms_zeros"], (who, m)
        assert not self.dirty or m["dirty_beam"] <= 1.0, (who, m)
        if self.dead is not None:
            assert not np.asarray(weight)[:, :, self.dead].any() and not np.asarray(rms)[:, :, self.dead].any(), who
        return m
