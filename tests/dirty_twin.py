"""Long-double reference, float64 twin and tile-table helpers for the Dirty / projection kernels (NumPy, CPU only).

``csrc/solve_dirty.hip`` computes, per (m, freq) tile,

    dirty     a[j] = sum_i conj(B[i, j]) * (Ni[i] * v[i])        i < ntel, j < ncol = npol * (lmax + 1 - m)
    project   v[i] = sum_j B[i, j] * a[j]

in float64, whatever the storage type of B.  The tests hand every function here B as the EXACT values the device
holds (complex64 storage: rounded to float32 by the test, then promoted exactly), so storage rounding is not part of
any error figure and complex64 is tested as tightly as complex128.

* ``ref_dirty`` / ``ref_project``: ``np.longdouble`` (x87 extended, 64-bit significand), the product ``Ni * v`` too.
* ``twin_dirty`` / ``twin_project``: plain float64, accumulating over rows (dirty) or columns (project) in ascending order
  like the kernels.  They are NOT the code under test: they only measure what float64 accumulation of this length
  costs on this very input.
* ``accept``: the acceptance rule, written once (see its docstring).
* ``Case``: a hand-made tile table -- pool, expected ``alm`` and expected ``vis`` in the device layouts.
"""

import math

import numpy as np

# a longdouble that is float64 in disguise would make every figure below meaningless: fail, never degrade
assert np.finfo(np.longdouble).nmant >= 63, "dirty_twin needs an extended-precision np.longdouble (>= 64-bit significand)"

LD = np.longdouble
U53 = 2.0**-53
MARGIN = 4.0  # fused against separate roundings + extreme-value scatter of two rounding sequences over ~1e4 outputs
SENTINEL = 7.0 + 7.0j


# ---------------------------------------------------------------------------------------------------------------------
# reference and twin of ONE tile: B [n_out_or_in ...] as a 2-d complex128 array [ntel, ncol] of exact device values


def _parts(z):
    z = np.asarray(z, dtype=np.complex128)
    return z.real.astype(LD), z.imag.astype(LD)


def ref_dirty(B, v, Ni):
    """``a [ncol] = B^H (Ni o v)`` in long double (``np.clongdouble``)."""
    br, bi = _parts(B)
    vr, vi = _parts(v)
    ni = np.asarray(Ni, dtype=np.float64).astype(LD)
    wr, wi = (ni * vr)[:, None], (ni * vi)[:, None]
    out = np.empty(br.shape[1], dtype=np.clongdouble)
    out.real = (br * wr + bi * wi).sum(axis=0)
    out.imag = (br * wi - bi * wr).sum(axis=0)
    return out


def ref_project(B, a):
    """``v [ntel] = B a`` in long double (``np.clongdouble``)."""
    br, bi = _parts(B)
    ar, ai = _parts(a)
    out = np.empty(br.shape[0], dtype=np.clongdouble)
    out.real = (br * ar[None, :] - bi * ai[None, :]).sum(axis=1)
    out.imag = (br * ai[None, :] + bi * ar[None, :]).sum(axis=1)
    return out


def twin_dirty(B, v, Ni):
    """float64, rows added in ascending order (one Python step per row, vectorised over the columns).  ``v``, ``Ni`` of
    shape ``[ntel, K]`` are K right-hand sides at once: ``[K, ncol]``, each exactly what its own call gives."""
    B = np.asarray(B, dtype=np.complex128)
    br, bi = np.ascontiguousarray(B.real), np.ascontiguousarray(B.imag)
    v = np.asarray(v, dtype=np.complex128)
    ni = np.asarray(Ni, dtype=np.float64)
    wr, wi = (ni * v.real)[..., None], (ni * v.imag)[..., None]  # [ntel, (K,) 1]
    are = np.zeros(v.shape[1:] + (B.shape[1],))
    aim = np.zeros_like(are)
    for i in range(B.shape[0]):
        are = (are + bi[i] * wi[i]) + br[i] * wr[i]
        aim = (aim - bi[i] * wr[i]) + br[i] * wi[i]
    return are + 1j * aim


def twin_project(B, a):
    """float64, columns added in ascending order (one Python step per column, vectorised over the rows)."""
    B = np.asarray(B, dtype=np.complex128)
    br, bi = np.ascontiguousarray(B.real.T), np.ascontiguousarray(B.imag.T)
    a = np.asarray(a, dtype=np.complex128)
    sre, sim = np.zeros(B.shape[0]), np.zeros(B.shape[0])
    for j in range(B.shape[1]):
        sre = (sre - bi[j] * a[j].imag) + br[j] * a[j].real
        sim = (sim + bi[j] * a[j].real) + br[j] * a[j].imag
    return sre + 1j * sim


def _l1(z):
    z = np.asarray(z, dtype=np.complex128)
    return np.abs(z.real) + np.abs(z.imag)


def bound_dirty(B, v, Ni):
    """Rigorous bound on ``max(|Re err|, |Im err|)`` per column: ``2 ntel`` fused multiply-adds per real accumulator
    plus the rounding of ``w = Ni * v``: ``(2 ntel + 4) 2^-53 sum_i (|Re b| + |Im b|)(|Re w| + |Im w|)``."""
    ntel = np.shape(B)[0]
    w = np.asarray(Ni, dtype=np.float64) * np.asarray(v, dtype=np.complex128)
    return (2 * ntel + 4) * U53 * (_l1(B) * _l1(w)[:, None]).sum(axis=0)


def bound_project(B, a):
    """The same with ncol terms per row sum, plus ``ceil(log2(64)) + 3`` additions of the wave's butterfly."""
    ncol = np.shape(B)[1]
    return (2 * ncol + 4 + math.ceil(math.log2(64)) + 3) * U53 * (_l1(B) * _l1(a)[None, :]).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the acceptance rule


def err_inf(got, ref):
    """``max(|Re(got - ref)|, |Im(got - ref)|)`` per element, the difference formed in long double."""
    d = np.asarray(got).astype(np.clongdouble) - np.asarray(ref).astype(np.clongdouble)
    return np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)


def rel_max(x, ref):
    """Max-norm error relative to ``max |ref|`` (0 for an exact match, whatever the scale; inf for an error against an
    all-zero reference)."""
    d = np.asarray(x).astype(np.clongdouble) - np.asarray(ref).astype(np.clongdouble)
    e = float(np.abs(d).max()) if d.size else 0.0
    if e == 0.0:
        return 0.0
    s = float(np.abs(np.asarray(ref)).max())
    return e / s if s > 0 else float("inf")


def accept(got, ref, twin, bound, what=""):
    """The one rule of every value comparison with the long-double reference.  ``got``, ``ref``, ``twin`` and ``bound``
    hold the same outputs (any common shape): everything one launch computes, all of one scale.

    (a) rigorous, per output: ``|got - ref|_inf <= bound`` -- derived from the number of roundings, never exceeded by a
        correct float64 evaluation in any order of the fused multiply-adds the kernels use.
    (b) sharp: ``e_got = max |got - ref| / max |ref|  <=  4 e_twin + 4 * 2^-53`` with ``e_twin`` the same figure of the float64
        twin on the same input.  (a) alone lets 1e-13 pass at ntel = 1526, where a row-ordered float64 sum sits at 6e-4 of
        the bound; (b) does not.

    Returns ``dict(e_got, e_twin, ratio, frac)``: ``ratio = e_got / e_twin``, ``frac`` = the largest fraction of (a) reached.
    """
    got, twin, bound = np.asarray(got), np.asarray(twin), np.asarray(bound, dtype=np.float64)
    assert got.shape == np.shape(ref) == twin.shape == bound.shape, (what, got.shape, np.shape(ref), twin.shape, bound.shape)
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    e = err_inf(got, ref)
    over = e > bound
    if over.any():
        k = np.unravel_index(int(np.argmax(e - bound)), e.shape)
        raise AssertionError(f"{what}: rigorous bound exceeded at {int(over.sum())} of {e.size} outputs; worst at {k}: "
                             f"error {e[k]:.3e} > bound {bound[k]:.3e}")
    e_got, e_twin = rel_max(got, ref), rel_max(twin, ref)
    lim = MARGIN * e_twin + MARGIN * U53
    assert e_got <= lim, f"{what}: e_got = {e_got:.3e} > 4 e_twin + 4 * 2^-53 = {lim:.3e} (e_twin = {e_twin:.3e})"
    nz = bound > 0
    return {"e_got": e_got, "e_twin": e_twin, "ratio": e_got / e_twin if e_twin > 0 else (0.0 if e_got == 0 else float("inf")),
            "frac": float((e[nz] / bound[nz]).max()) if nz.any() else 0.0}


# ---------------------------------------------------------------------------------------------------------------------
# hand-made tile tables

C64, C128 = 0, 1  # DMM_C64, DMM_C128 of include/draco_amd.h
FULL, PACKED = 0, 1  # DMM_B_FULL, DMM_B_PACKED
NP_DTYPE = {C64: np.complex64, C128: np.complex128}


def device_values(B, b_dtype):
    """``B`` as the values a pool of ``b_dtype`` holds, in complex128 (complex64: rounded to float32, promoted exactly)."""
    return np.asarray(B).astype(NP_DTYPE[b_dtype]).astype(np.complex128)


def random_tile(rng, ntel, npol, L, b_dtype):
    """A random tile ``[ntel, npol, L]`` (variance 1 / ntel per part, like the synthetic provider) of device values."""
    s = math.sqrt(3.0 / (2.0 * ntel))
    return device_values(s * (rng.uniform(-1, 1, (ntel, npol, L)) + 1j * rng.uniform(-1, 1, (ntel, npol, L))), b_dtype)


class Case:
    """A tile table ``[(m, f, b_off)]`` with one ``[ntel, npol, lmax + 1 - m]`` array of device values per tile.

    ``b_off`` is in elements of the pool.  ``tile_elems(m)`` is what a tile occupies from its ``b_off`` on:
    ``ntel * npol * (lmax + 1 - m)`` packed, ``ntel * npol * (lmax + 1)`` in the full layout (its ``l < m`` columns belong
    to the tile's extent but are never read).
    """

    def __init__(self, npairs, npol, lmax, nfreq, n_m, tiles, Bs, b_dtype=C128, b_layout=PACKED):
        self.npairs, self.ntel, self.npol, self.lmax, self.nfreq, self.n_m = npairs, 2 * npairs, npol, lmax, nfreq, n_m
        self.tiles = [(int(m), int(f), int(o)) for m, f, o in tiles]
        self.Bs = list(Bs)
        self.b_dtype, self.b_layout = b_dtype, b_layout
        assert len(self.tiles) == len(self.Bs)
        assert len({(m, f) for m, f, _ in self.tiles}) == len(self.tiles), "an (m, f) pair twice: two tiles would own one output"
        for (m, f, o), B in zip(self.tiles, self.Bs):
            assert 0 <= m <= lmax and m < n_m and 0 <= f < nfreq and o >= 0
            assert B.shape == (self.ntel, npol, lmax + 1 - m), (B.shape, m)
        spans = sorted((o, o + self.tile_elems(m)) for m, _, o in self.tiles)
        for (a0, a1), (b0, _) in zip(spans, spans[1:]):
            assert a1 <= b0, "tiles overlap in the pool"
        self.nelem = spans[-1][1] if spans else 0

    def tile_elems(self, m):
        return self.ntel * self.npol * (self.lmax + 1 - (m if self.b_layout == PACKED else 0))

    def pool(self, tail=0):
        """The device pool as a NumPy array of the storage type: NaN wherever no tile element lives (gaps between
        tiles, ``tail`` extra elements, the ``l < m`` columns of full-layout tiles)."""
        n = max(self.nelem + tail, 1)
        n += n & 1  # whole 16-byte units for complex64
        pool = np.full(n, np.nan + 1j * np.nan, dtype=NP_DTYPE[self.b_dtype])
        for (m, _, o), B in zip(self.tiles, self.Bs):
            view = pool[o : o + self.tile_elems(m)].reshape(self.ntel, self.npol, -1)
            view[:, :, (m if self.b_layout == FULL else 0) :] = B
        return pool

    def unpool(self, pool):
        """Inverse of :meth:`pool`: the list of ``[ntel, npol, L]`` arrays read back from a pool."""
        out = []
        for m, _, o in self.tiles:
            view = pool[o : o + self.tile_elems(m)].reshape(self.ntel, self.npol, -1)
            out.append(np.array(view[:, :, (m if self.b_layout == FULL else 0) :]))
        return out

    def tile_table(self):
        """``(ms, fs, offs)`` as arrays, in table order."""
        t = np.array(self.tiles, dtype=np.int64).reshape(-1, 3)
        return t[:, 0].astype(np.int32), t[:, 1].astype(np.int32), t[:, 2].astype(np.int64)

    # ---- expected outputs in the device layouts
    def alm_shape(self):
        return (self.nfreq, self.npol, self.n_m, self.lmax + 1)

    def vis_shape(self):
        return (self.n_m, 2, self.nfreq, self.npairs)

    def _per_tile(self, fn, *args):
        return [fn(B.reshape(self.ntel, -1), *[a(m, f) for a in args]) for (m, f, _), B in zip(self.tiles, self.Bs)]

    def expected_alm(self, mvis, mweight, sentinel=SENTINEL):
        """For ``a = B^H (Ni o v)`` with ``mvis, mweight [n_m, 2, nfreq, npairs]``: ``dict(ref, twin, bound, owned, zero)``
        of shape ``alm_shape()``.  ``owned``: computed values (``l >= m`` of listed tiles); ``zero``: structural zeros
        (``l < m`` of listed tiles); everything else holds ``sentinel`` in ``ref`` and ``twin``."""
        v = lambda m, f: mvis[m, :, f, :].reshape(-1)  # noqa: E731
        w = lambda m, f: mweight[m, :, f, :].reshape(-1)  # noqa: E731
        out = self._blank(self.alm_shape(), sentinel)
        out["zero"] = np.zeros(self.alm_shape(), dtype=bool)
        for (m, f, _), r, t, b in zip(self.tiles, self._per_tile(ref_dirty, v, w), self._per_tile(twin_dirty, v, w), self._per_tile(bound_dirty, v, w)):
            for name, val in (("ref", r), ("twin", t), ("bound", b)):
                out[name][f, :, m, m:] = val.reshape(self.npol, -1)
                out[name][f, :, m, :m] = 0
            out["owned"][f, :, m, m:] = True
            out["zero"][f, :, m, :m] = True
        return out

    def expected_alm_days(self, mvis_l, mweight_l, sentinel=SENTINEL):
        """:meth:`expected_alm` of several days at once (the twin's row loop runs once for all of them)."""
        D = len(mvis_l)
        outs = [self._blank(self.alm_shape(), sentinel) for _ in range(D)]
        for o in outs:
            o["zero"] = np.zeros(self.alm_shape(), dtype=bool)
        for (m, f, _), B in zip(self.tiles, self.Bs):
            B2 = B.reshape(self.ntel, -1)
            vs = np.stack([mv[m, :, f, :].reshape(-1) for mv in mvis_l], axis=1)
            ws = np.stack([mw[m, :, f, :].reshape(-1) for mw in mweight_l], axis=1)
            twins = twin_dirty(B2, vs, ws)
            for d, o in enumerate(outs):
                for name, val in (("ref", ref_dirty(B2, vs[:, d], ws[:, d])), ("twin", twins[d]), ("bound", bound_dirty(B2, vs[:, d], ws[:, d]))):
                    o[name][f, :, m, m:] = val.reshape(self.npol, -1)
                    o[name][f, :, m, :m] = 0
                o["owned"][f, :, m, m:] = True
                o["zero"][f, :, m, :m] = True
        return outs

    def expected_vis(self, alm, sentinel=SENTINEL):
        """For ``v = B a`` with ``alm`` of shape ``alm_shape()`` (only ``l >= m`` of listed tiles is read):
        ``dict(ref, twin, bound, owned)`` of shape ``vis_shape()``."""
        a = lambda m, f: alm[f, :, m, m:].reshape(-1)  # noqa: E731
        out = self._blank(self.vis_shape(), sentinel)
        for (m, f, _), r, t, b in zip(self.tiles, self._per_tile(ref_project, a), self._per_tile(twin_project, a), self._per_tile(bound_project, a)):
            for name, val in (("ref", r), ("twin", t), ("bound", b)):
                out[name][m, :, f, :] = val.reshape(2, self.npairs)
            out["owned"][m, :, f, :] = True
        return out

    @staticmethod
    def _blank(shape, sentinel):
        return {"ref": np.full(shape, sentinel, dtype=np.clongdouble), "twin": np.full(shape, sentinel, dtype=np.complex128),
                "bound": np.zeros(shape, dtype=np.float64), "owned": np.zeros(shape, dtype=bool)}


def check_launch(got, exp, sentinel=SENTINEL, what=""):
    """Everything asserted after one launch: values (``accept``), exact structural zeros, untouched sentinels, no NaN."""
    got = np.asarray(got)
    assert got.shape == exp["owned"].shape, (what, got.shape, exp["owned"].shape)
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    zero = exp.get("zero")
    if zero is not None:
        assert np.all(got[zero] == 0), f"{what}: {int((got[zero] != 0).sum())} structural zeros (l < m) are not zero"
        rest = ~(exp["owned"] | zero)
    else:
        rest = ~exp["owned"]
    assert np.all(got[rest] == sentinel), f"{what}: {int((got[rest] != sentinel).sum())} entries outside the tile list were written"
    own = exp["owned"]
    if not own.any():
        return {"e_got": 0.0, "e_twin": 0.0, "ratio": 0.0, "frac": 0.0}
    return accept(got[own], exp["ref"][own], exp["twin"][own], exp["bound"][own], what)


def layout_tiles(ms, npairs, npol, lmax, b_layout, gaps=None, order=None):
    """Offsets for tiles of the given ``ms`` laid out one after the other (each padded to an even element count so that
    every tile starts 16-byte aligned for complex64 too), optionally with ``gaps[k]`` elements in front of tile ``k`` and
    the tiles PLACED in ``order`` (a permutation) while the table keeps the order of ``ms``."""
    n = len(ms)
    order = list(range(n)) if order is None else list(order)
    gaps = [0] * n if gaps is None else list(gaps)
    offs, pos = [0] * n, 0
    for k in order:
        pos += gaps[k]
        offs[k] = pos
        sz = 2 * npairs * npol * (lmax + 1 - (ms[k] if b_layout == PACKED else 0))
        pos += sz + (sz & 1)
    return offs
