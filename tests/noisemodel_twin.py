"""Plain NumPy restatement of ``ReconstructVisWeight`` / ``ReconstructVisFreqCov`` (``draco/analysis/ringmapmaker.py:
1318-1712``) and of the colouring of ``FreqCorrelatedNoise`` (``draco/synthesis/noise.py:377-470``), in the arithmetic of
``csrc/noisemodel.hip``, with a long-double truth.

Five things, each as an **f64 form** (what the device computes: float64 products and sums, one rounding to the dataset's
dtype) and, with ``truth=True``, a **truth form** in ``numpy.longdouble`` that does not round:

* :func:`layout` and :func:`window` -- the baseline grid, its redundancy and the normalised north-south window;
* :func:`weight_noise_factor` and :func:`cov_noise_factor`;
* :func:`masked_cholesky` -- per ``(pol, ew, ra)`` sample the lower factor of ``cov inz(noise_factor)`` on the channels
  whose weight is positive, through the identity embedding (:func:`compressed_cholesky` is the reference's literal
  form, one sample at a time; the two agree to rounding), and ``weight = 1 / diag``;
* :func:`colour` -- ``vis``, ``vis_weight`` and the Hermitian fix-up given ``L`` and ``z``;
* :func:`sidereal_weights`.

:class:`GridTel` is a regular cylinder grid with the attributes the tasks read, every stack entry oriented into the half
plane ``x >= 0`` (``x = 0``: ``y >= 0``) as ``MakeVisGrid`` expects.
"""

import numpy as np

LD = np.longdouble
U = 2.0**-53
C_LIGHT = 299792458.0

_WINDOW_COEF = {
    "uniform": (1, 0, 0, 0),
    "hann": (0.5, -0.5, 0, 0),
    "hamming": (0.53836, -0.46164, 0, 0),
    "blackman": (0.42, -0.5, 0.08, 0),
    "nuttall": (0.355768, -0.487396, 0.144232, -0.012604),
    "blackman_nuttall": (0.3635819, -0.4891775, 0.1365995, -0.0106411),
    "blackman_harris": (0.35875, -0.48829, 0.14128, -0.01168),
}


def inz(x):
    """``invert_no_zero`` in the dtype of ``x`` (float64 for integers)."""
    x = np.asarray(x)
    dt = x.dtype if x.dtype.kind == "f" else np.float64
    x = x.astype(dt)
    return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(dt)


def rel_err(a, b):
    return float(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).max() / np.abs(np.asarray(b, dtype=LD)).max())


class GridTel:
    """``ncyl`` cylinders of ``nfeed_cyl`` dual-polarisation feeds, autos included, redundancy stacked."""

    lmax = mmax = 0
    frequencies = np.zeros(1)

    def __init__(self, ncyl, nfeed_cyl, cyl_sep=22.0, feed_sep=0.3048):
        pos = [(c, y, pl) for c in range(ncyl) for y in range(nfeed_cyl) for pl in range(2)]
        n = self.nfeed = len(pos)
        self.feedpositions = np.array([(c * cyl_sep, y * feed_sep) for c, y, _ in pos])
        self.polarisation = np.array(["XY"[pl] for _, _, pl in pos])
        self.input_index = np.array([(i, i) for i in range(n)], dtype=[("chan_id", "<u2"), ("correlator_input", "<u2")])
        groups, prod = {}, []
        for i in range(n):
            for j in range(i, n):
                (ci, yi, pi), (cj, yj, pj) = pos[i], pos[j]
                sx, sy = ci - cj, yi - yj
                if sx < 0 or (sx == 0 and sy < 0):
                    key, conj = (pj, pi, -sx, -sy), 1
                else:
                    key, conj = (pi, pj, sx, sy), 0
                groups.setdefault(key, []).append((len(prod), conj))
                prod.append((i, j))
        self.prod = np.array(prod, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
        keys = sorted(groups)
        self.npairs = len(keys)
        self.stack = np.array([groups[k][0] for k in keys], dtype=[("prod", "<u4"), ("conjugate", "u1")])
        self.reverse_stack = np.zeros(len(prod), dtype=[("stack", "<u4"), ("conjugate", "u1")])
        self.feedmap = np.full((n, n), -1, dtype=np.int64)
        self.feedconj = np.zeros((n, n), dtype=bool)
        for s, k in enumerate(keys):
            for pidx, conj in groups[k]:
                self.reverse_stack[pidx] = (s, conj)
                i, j = prod[pidx]
                self.feedmap[i, j], self.feedconj[i, j] = s, bool(conj)
                self.feedmap[j, i], self.feedconj[j, i] = s, (not conj) if i != j else bool(conj)
        self.feedmask = self.feedmap >= 0
        rep = self.prod[self.stack["prod"]]
        cj = self.stack["conjugate"].astype(bool)
        a, b = np.where(cj, rep["input_b"], rep["input_a"]).astype(int), np.where(cj, rep["input_a"], rep["input_b"]).astype(int)
        self.uniquepairs = np.stack([a, b], axis=1)  # the oriented pair: what the data of a stack entry belong to
        self.prodstack = np.array(list(zip(a, b)), dtype=[("input_a", "<u2"), ("input_b", "<u2")])
        self.baselines = self.feedpositions[a] - self.feedpositions[b]
        self.redundancy = np.array([len(groups[k]) for k in keys], dtype=np.float32)


def window_generalised(x, window, ft=np.float64):
    x = np.asarray(x, dtype=ft)
    if window == "triangular":
        w = 1 - 2 * np.abs(x - ft(0.5))
    else:
        a = [ft(c) for c in _WINDOW_COEF[window]]
        pi = np.pi if ft is np.float64 else np.arccos(LD(-1))
        w = sum(a[i] * np.cos(2 * pi * i * x) for i in range(4))
    return np.where((x >= 0) & (x <= 1), w, 0)


def layout(tel, pol, ewpos, nsmax):
    """The reference's layout dictionary (``ringmapmaker.py:1375-1463``) from exact integer grid positions."""
    pairs = np.asarray(tel.uniquepairs)
    polpair = np.char.add(tel.polarisation[pairs[:, 0]], tel.polarisation[pairs[:, 1]])
    lookup = {str(p): i for i, p in enumerate(pol)}
    pol_remap = np.array([lookup.get(str(p), -1) for p in polpair])
    bl = np.asarray(tel.baselines)
    sx = np.abs(bl[:, 0])
    sy = np.abs(bl[:, 1])
    min_x, min_y = (sx[sx > 1e-4].min() if np.any(sx > 1e-4) else 1.0), sy[sy > 1e-4].min()  # (one cylinder: every x is 0)
    xind, yind = np.rint(bl[:, 0] / min_x).astype(int), np.rint(bl[:, 1] / min_y).astype(int)
    flag = (pol_remap >= 0) & (np.abs(yind * min_y) <= nsmax + 0.5 * min_y)
    ny = 2 * np.abs(yind).max() + 1
    nx = len(ewpos)
    nspos = np.fft.fftfreq(ny, d=1.0 / (ny * min_y))
    pconj = np.unique([str(p)[1] + str(p)[0] for p in pol], return_inverse=True)[1]
    nb = np.asarray(tel.redundancy, dtype=np.float32)
    grid = np.zeros((len(pol), nx, ny))
    x_, y_, p_ = xind[flag], yind[flag], pol_remap[flag]
    grid[p_, x_, y_] = nb[flag]
    intra = np.flatnonzero(x_ == 0)
    grid[pconj[p_[intra]], 0, -y_[intra]] = nb[flag][intra]
    return {"xind": x_, "yind": y_, "pind": p_, "ewpos": np.asarray(ewpos), "nspos": nspos, "nbaseline_grid": grid, "nbaseline": nb, "flag": flag, "pconjmap": pconj,
            "npol": len(pol), "nx": nx, "ny": int(ny)}


def window(freq, lay, weight, scaled, include_auto, freqmin, nsmax, truth=False):
    """Normalised window ``[npol, nfreq, nx, ny]`` (``ringmapmaker.py:1465-1506``)."""
    ft = LD if truth else np.float64
    freq = np.asarray(freq, dtype=ft)
    w = np.empty((lay["npol"], freq.size, lay["nx"], lay["ny"]), dtype=ft)
    if weight == "natural":
        w[:] = lay["nbaseline_grid"][:, np.newaxis].astype(ft)
    else:
        c = ft(C_LIGHT) * ft(1e-6) if not truth else LD(C_LIGHT) / LD(10) ** 6
        wvmin = c / ft(freqmin)
        for ff in range(freq.size):
            wv = c / freq[ff]
            vpos = lay["nspos"].astype(ft) / wv
            vmax = ft(nsmax) / wvmin if scaled else ft(nsmax) / wv
            w[:, ff] = window_generalised(ft(0.5) * (vpos / vmax + 1), weight, ft)
    if include_auto:
        w[:, :, 0, 0] = 0
    norm = np.sum(w, axis=-1, keepdims=True)
    return w * inz(norm)


def weight_noise_factor(win, lay):
    """``[pol, freq, ew]``."""
    return np.sum(win**2 * inz(lay["nbaseline_grid"].astype(win.dtype))[:, np.newaxis], axis=-1)


def cov_noise_factor(win, lay):
    """``[pol, freq, freq_sum, ew]``."""
    inv_nb = inz(lay["nbaseline_grid"].astype(win.dtype))[:, np.newaxis, np.newaxis]
    return np.sum(win[:, :, np.newaxis] * win[:, np.newaxis] * inv_nb, axis=-1)


def cholesky_batch(G):
    """Lower factors of a batch ``[B, n, n]`` in the dtype of ``G`` (column by column); ``ok [B]`` is False where a pivot
    is not positive."""
    B, n, _ = G.shape
    L = np.zeros_like(G)
    ok = np.ones(B, dtype=bool)
    for j in range(n):
        d = G[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=-1)
        ok &= d > 0
        r = np.sqrt(np.where(d > 0, d, 1))
        L[:, j, j] = r
        if j + 1 < n:
            L[:, j + 1 :, j] = (G[:, j + 1 :, j] - np.einsum("bik,bk->bi", L[:, j + 1 :, :j], L[:, j, :j])) / r[:, np.newaxis]
    return L, ok


def normalised_cov(cov_in, noise_factor, truth=False):
    """``C [pol, ew, ra, freq, freq_sum] = cov_in inz(noise_factor)``: one float64 product per entry (f64 form; the
    reciprocal is the float64 one the tasks upload) or the long-double quotient (truth)."""
    if truth:
        nf = noise_factor.astype(LD)
        c = cov_in.astype(LD) * inz(nf)[..., np.newaxis]
    else:
        c = cov_in * inz(noise_factor.astype(np.float64))[..., np.newaxis]
    return np.ascontiguousarray(c.transpose(0, 3, 4, 1, 2))


def masked_cholesky(cov_in, weight, noise_factor, truth=False):
    """``(L [pol, ew, ra, freq, freq_sum], weight_out [pol, freq, ew, ra], ok [pol, ew, ra], C)``; the lower triangle of
    the input is the one read."""
    C = normalised_cov(cov_in, noise_factor, truth)
    npol, new, nra, n, _ = C.shape
    valid = (weight > 0).transpose(0, 2, 3, 1)  # [p, x, t, f]
    both = valid[..., :, np.newaxis] & valid[..., np.newaxis, :]
    eye = np.eye(n, dtype=C.dtype)
    G = np.where(both, C, eye)
    G = np.tril(G) + np.swapaxes(np.tril(G, -1), -1, -2)
    L, ok = cholesky_batch(G.reshape(-1, n, n))
    L = np.where(both, L.reshape(C.shape), 0)
    diag = np.einsum("pxtff->pxtf", C)
    wout = np.where(valid, inz(diag), 0).transpose(0, 3, 1, 2)
    if not truth:
        wout = wout.astype(np.float32)
    return L, np.ascontiguousarray(wout), ok.reshape(npol, new, nra), np.where(both, C, 0)


def compressed_cholesky(C, valid):
    """The reference's literal form for one sample: ``chol(C[valid x valid])`` scattered into zeros (float64)."""
    out = np.zeros_like(C)
    idx = np.flatnonzero(valid)
    if idx.size:
        out[np.ix_(idx, idx)] = np.linalg.cholesky(C[np.ix_(idx, idx)])
    return out


def pconjmap(pol):
    return np.unique([str(p)[1] + str(p)[0] for p in pol], return_inverse=True)[1]


def colour(L, z, redundancy, weight, pol, truth=False):
    """``(vis [pol, freq, ew, ns, ra], vis_weight, bound)``: ``z [pol, ew, ra, freq, ns]`` complex64 (the draws of all
    slabs), ``L [pol, ew, ra, freq, freq_sum]`` float64.  f64 form: complex64 / float32; truth form: long double, with
    ``bound = nfreq u sum |L| |z|`` per real component (before the fix-up, which is exact but for the auto's sqrt 2)."""
    ft = LD if truth else np.float64
    isr = inz(np.sqrt(redundancy.astype(ft)))  # [p, x, s]
    Lf = L.astype(ft)
    re = np.einsum("pxtfk,pxtks->pfxst", Lf, z.real.astype(ft))
    im = np.einsum("pxtfk,pxtks->pfxst", Lf, z.imag.astype(ft))
    sc = isr[:, np.newaxis, :, :, np.newaxis]
    re, im = re * sc, im * sc
    vw = weight.astype(ft)[:, :, :, np.newaxis, :] * redundancy.astype(ft)[:, np.newaxis, :, :, np.newaxis]
    bound = None
    if truth:
        aL = np.abs(Lf)
        bound = (np.einsum("pxtfk,pxtks->pfxst", aL, np.abs(z.real).astype(ft)) * sc, np.einsum("pxtfk,pxtks->pfxst", aL, np.abs(z.imag).astype(ft)) * sc)
        bound = tuple((L.shape[-1] * U * b).astype(np.float64) for b in bound)
    else:
        re, im, vw = re.astype(np.float32), im.astype(np.float32), vw.astype(np.float32)
    nns = redundancy.shape[-1]
    assert nns % 2 == 1
    half = nns // 2
    re0, im0 = re.copy(), im.copy()
    for pi, po in enumerate(pconjmap(pol)):
        for k in range(1, half + 1):
            re[po, :, 0, nns - k] = re0[pi, :, 0, k]
            im[po, :, 0, nns - k] = -im0[pi, :, 0, k]
            if truth:
                for b in bound:
                    b[po, :, 0, nns - k] = b[pi, :, 0, k]
        if pi == po:
            re[po, :, 0, 0] = re0[pi, :, 0, 0] * (np.float32(2**0.5) if not truth else np.sqrt(LD(2)))
            im[po, :, 0, 0] = 0
    return (re, im) if truth else (re + 1j * im).astype(np.complex64), vw, bound


def sidereal_weights(hv_weight, nf, lay, truth=False):
    """``vis_weight [freq, stack, ra]`` of ``ReconstructVisWeight``."""
    ft = LD if truth else np.float64
    npol, nfreq, nx, nra = hv_weight.shape
    flag = lay["flag"]
    out = np.zeros((nfreq, flag.size, nra), dtype=ft)
    w0 = hv_weight.astype(ft) * nf.astype(ft)[..., np.newaxis]
    nb = lay["nbaseline"].astype(np.float32).astype(ft)
    out[:, flag] = (nb[flag][:, np.newaxis, np.newaxis] * w0[lay["pind"], :, lay["xind"], :]).transpose(1, 0, 2)
    return out if truth else out.astype(np.float32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- the cases of tests/golden/noisemodel*.npz
DF = 0.390625
CASES = {
    "N33": dict(ncyl=2, nfeed_cyl=3, pol=("XX", "YY"), nfreq=33, nra=40, weight="natural", scaled=False, include_auto=False, nsmax_y=2, seed=33050),
    "N70": dict(ncyl=1, nfeed_cyl=4, pol=("XX", "XY", "YX", "YY"), nfreq=70, nra=130, weight="hann", scaled=True, include_auto=True, nsmax_y=2, seed=70130),
    "N6": dict(ncyl=2, nfeed_cyl=2, pol=("XX",), nfreq=6, nra=17, weight="uniform", scaled=False, include_auto=False, nsmax_y=1, seed=6017),
}
# layout only: two cylinders and all four polarisations, which N70 (one cylinder) cannot put through ``_compute_layout``
LAYOUT_CASES = {"P4": dict(ncyl=2, nfeed_cyl=3, pol=("XX", "XY", "YX", "YY"), nsmax_y=1, nfreq=5)}
RPOS = {"N33": np.r_[0:12, 24, 30, 31, 39], "N70": np.array([0, 49, 50, 63, 64, 99, 100, 127, 128, 129]), "N6": np.arange(17)}


def _masks(name, wq):
    if name == "N33":
        wq[:, [3, 4, 17], :, 8:16] = 0  # mask B, every ew
        wq[:, 20:26, 1, 16:24] = 0  # mask C on ew 1: ra 0 ... 31 of ew 1 hold A, B and C
        wq[1, 7, 0, 24] = 0  # a channel missing in one polarisation only
        wq[:, :, 1, 30] = 0  # no valid channel
        wq[:, :, 1, 31] = 0
        wq[:, 12, 1, 31] = 6  # exactly one valid channel
    elif name == "N70":
        wq[:, 10:14, 0, 0:50] = 0
        wq[1, 65:, 0, 64:100] = 0
        wq[:, :, 0, 129] = 0  # no valid channel, the last RA
        wq[2, :, 0, 128] = 0
        wq[2, 69, 0, 128] = 8  # exactly one valid channel, the last one
    else:
        wq[0, 2, 0, 3:9] = 0
        wq[0, :, 1, 5] = 0
        wq[0, :, 1, 6] = 0
        wq[0, 0, 1, 6] = 4


def cov_of(A, d):
    """``[pol, freq, freq_sum, ew, ra]`` float64 (exact integers) from ``A [pol, ew, ra, freq, k]`` and ``d``."""
    a = A.astype(np.int64)
    g = np.einsum("pxtfk,pxtgk->pxtfg", a, a)
    g[..., np.arange(a.shape[3]), np.arange(a.shape[3])] += int(d)
    return np.ascontiguousarray(g.transpose(0, 3, 4, 1, 2)).astype(np.float64)


def _finish(name, c):
    spec = CASES[name]
    tel = c["tel"] = GridTel(spec["ncyl"], spec["nfeed_cyl"])
    c["pol"] = np.array(spec["pol"])
    c["nra"] = spec["nra"]
    c["ewpos"] = np.arange(spec["ncyl"]) * 22.0
    c["weight"] = (c["weight_q"].astype(np.float32) / np.float32(8)).astype(np.float32)
    c["cov"] = cov_of(c["A"], c["d"])
    c["rpos"], c["name"] = RPOS[name], name
    return c


def build_case(name):
    """The inputs of case ``name``, drawn from its seed (the generator); the tests read them back with :func:`case`."""
    spec = CASES[name]
    rng = np.random.default_rng(spec["seed"])
    npol, n, new, nra = len(spec["pol"]), spec["nfreq"], spec["ncyl"], spec["nra"]
    c = {"freq": 600.0 + DF * np.arange(n), "d": np.array(6)}
    c["A"] = rng.integers(-2, 3, size=(npol, new, nra, n, 3)).astype(np.int8)
    wq = rng.integers(4, 13, size=(npol, n, new, nra)).astype(np.uint8)
    _masks(name, wq)
    c["weight_q"] = wq
    c["freqmin"] = np.array(c["freq"].min())
    # (a little past the outermost separation kept: exactly on it, whether a uniform window counts that separation is
    # decided by the last bit of x = (v / vmax + 1) / 2, in the reference and in the truth alike)
    c["nsmax"] = np.array(spec["nsmax_y"] * 0.3048 + 0.01)
    return _finish(name, c)


def case(gold, name):
    c = {k: np.array(gold[f"{name}/{k}"]) for k in ("freq", "weight_q", "A", "d", "freqmin", "nsmax")}
    return _finish(name, c)


def attrs_of(c, **over):
    """The attributes ``BeamformNS`` leaves on its output, for case ``c`` (``over``: another window)."""
    spec = CASES[c["name"]]
    a = {"beamform_ns_freqmin": float(c["freqmin"]), "beamform_ns_nsmax": float(c["nsmax"])}
    for k in ("weight", "scaled", "include_auto"):
        a[f"beamform_ns_{k}"] = over.get(k, spec[k])
    return a


def positions(weight, limit=10):
    """``[npos, 3]`` ``(pol, ew, ra)``: the first and the last sample and one per distinct mask, at most ``limit``."""
    npol, n, new, nra = weight.shape
    flag = weight > 0
    pos, seen = [(0, 0, 0), (npol - 1, new - 1, nra - 1)], set()
    for p in range(npol):
        for x in range(new):
            for t in range(nra):
                key = flag[p, :, x, t].tobytes()
                if key not in seen:
                    seen.add(key)
                    if (p, x, t) not in pos and len(pos) < limit:
                        pos.append((p, x, t))
    return np.array(pos, dtype=np.int32)


def expand_band(Lb):
    """``L [..., n, n]`` float64 from its diagonals ``Lb [..., n, nb]``: ``L[f, f - k] = Lb[f, k]``."""
    n, nb = Lb.shape[-2:]
    L = np.zeros(Lb.shape[:-1] + (n,), dtype=np.float64)
    for k in range(nb):
        idx = np.arange(k, n)
        L[..., idx, idx - k] = Lb[..., idx, k]
    return L


def noise_case(name, c, lay):
    """A noise model with an integer banded factor (zero rows and columns on invalid channels), float32 weights that are
    no multiples of a power of two, and the layout's redundancy."""
    spec = CASES[name]
    rng = np.random.default_rng(spec["seed"] + 1)
    npol, n, new, nra = c["weight"].shape
    Lb = rng.integers(-3, 4, size=(npol, new, nra, n, 5)).astype(np.int8)
    Lb[..., 0] = rng.integers(1, 5, size=(npol, new, nra, n))
    return noise_of(Lb, c, lay, spec["seed"] + 2)


def noise_of(Lb, c, lay, seed):
    valid = (c["weight"] > 0).transpose(0, 2, 3, 1)
    L = np.where(valid[..., :, np.newaxis] & valid[..., np.newaxis, :], expand_band(Lb), 0.0)
    q = c["weight_q"].astype(np.float32)
    w = np.where(q > 0, np.float32(1) / (q + np.float32(0.3)), np.float32(0)).astype(np.float32)
    return {"L_q": Lb, "L": L, "weight": w, "redundancy": lay["nbaseline_grid"].astype(np.int32), "seed": int(seed)}


def draw(seed, shape):
    """``z [pol, ew, ra, freq, ns]`` complex64: the draws of ``FreqCorrelatedNoise`` seeded with ``seed``, slab by slab
    in its order, by the expressions of ``util.random.complex_normal``."""
    npol, new, nra, n, nns = shape
    rng = np.random.default_rng(seed)
    z = np.empty(shape, dtype=np.complex64)
    for p in range(npol):
        for x in range(new):
            s = z[p, x]
            rng.standard_normal((nra, n, 2 * nns), dtype=np.float32, out=s.view(np.float32))
            s *= 1.0 / 2**0.5
    return z


def auto_rows(pol, shape):
    """Mask ``[pol, freq, ew, ns, ra]`` of the auto-correlations the fix-up scales (``ew = 0``, ``ns = 0``, ``pconj[p] = p``)."""
    m = np.zeros(shape, dtype=bool)
    for pi, po in enumerate(pconjmap(pol)):
        if pi == po:
            m[pi, :, 0, 0, :] = True
    return m


def auto_allow(t, b):
    """Bound of the fixed-up auto against ``t = sqrt(2) x truth``: the coloured value ``v`` is within ``ulp32 / 2 + b`` of
    the truth, then ``float32(v float32(sqrt 2))``: the constant is off by at most ``2**-24`` relative and the product
    is rounded once more."""
    r2 = np.sqrt(2.0)
    return r2 * (0.5 * ulp32(t / r2) + b) * (1 + 2.0**-24) + np.abs(t) * 2.0**-24 + 0.5 * ulp32(t)


def layout_case(name):
    """Telescope, axes and attributes of a layout-only case."""
    spec = LAYOUT_CASES[name]
    freq = 600.0 + DF * np.arange(spec["nfreq"])
    return {"tel": GridTel(spec["ncyl"], spec["nfeed_cyl"]), "pol": np.array(spec["pol"]), "ewpos": np.arange(spec["ncyl"]) * 22.0, "freq": freq,
            "nsmax": spec["nsmax_y"] * 0.3048 + 0.01, "freqmin": float(freq.min())}
