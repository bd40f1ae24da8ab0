"""Float64 twins of the regridder and the stacker for the tests (dense restatements, CPU only).

``band_wiener_twin`` solves, per row, the band-masked dense system ``(band_bw(R N R^T) + eps I) x = R N y`` with
``np.linalg.solve`` in float64: the exact answer the reference (float32 right-hand side) and the GPU kernel (float64
arithmetic, one rounding to complex64) are both measured against.

``band_wiener_truth`` / ``band_wiener_f64`` state the banded algorithm of ``csrc/regrid.hip`` itself, in long double and in
float64; ``RegridCase`` holds one call of the direct sweep (``test_gpu_regrid_direct.py``) with its truth and its bound.
``stack_add_f32`` / ``stack_finish_f32`` are ``SiderealStacker``'s float32 arithmetic, operation for operation.
"""

import numpy as np

from ringchain_twin import EXCLUDED_CAP, LD, rounded_measure


def lanczos_kernel(x, a):
    return np.where(np.abs(x) < a, np.sinc(x) * np.sinc(x / a), 0.0)


def forward_matrix(grid, times, a):
    """``R [ngrid, nt]``: Lanczos interpolation from the regular ``grid`` onto ``times``, transposed."""
    dx = grid[1] - grid[0]
    return lanczos_kernel((grid[:, None] - times[None, :]) / dx, a)


def padded_grid(samples, start, end, a):
    pad = 5 * a
    g = np.arange(-pad, samples + pad, dtype=np.float64) / samples
    return g * (end - start) + start, pad


def band_wiener_twin(vis, weight, times, samples, start, end, a=5, eps=1e-3, mask_zero_weight=False):
    """``vis, weight [nrow, nt]`` -> ``(x [nrow, samples] complex128, nw [nrow, samples] float64)``."""
    grid, pad = padded_grid(samples, start, end, a)
    R = forward_matrix(grid, np.asarray(times, dtype=np.float64), a)
    ng = len(grid)
    bw = 2 * a - 1
    band = np.abs(np.arange(ng)[:, None] - np.arange(ng)[None, :]) <= bw
    vis = np.asarray(vis, dtype=np.complex128)
    weight = np.asarray(weight, dtype=np.float64)
    x = np.zeros((vis.shape[0], samples), dtype=np.complex128)
    nw = np.zeros((vis.shape[0], samples), dtype=np.float64)
    for k in range(vis.shape[0]):
        C = np.where(band, (R * weight[k][None, :]) @ R.T, 0.0)
        d = R @ (weight[k] * vis[k])
        xs = np.linalg.solve(C + eps * np.eye(ng), d)
        x[k] = xs[pad : pad + samples]
        nw[k] = np.diag(C)[pad : pad + samples]
        if mask_zero_weight and not np.any(weight[k] != 0):
            nw[k] = 0.0
    return x, nw


# ------------------------------------------------- the banded algorithm itself: long-double truth, float64 restatement
# ``band_wiener_truth`` and ``band_wiener_f64`` are one statement of ``csrc/regrid.hip``'s algorithm in two number
# types: per grid point g the band entries c[k] = sum_j R[g][j] R[g-k][j] w_j (k = 0 .. bw = 2 a - 1) and the right-hand
# side d = sum_j R[g][j] w_j y_j over the samples R[g] reaches, one row of the banded Cholesky factor of C + eps I, one
# step of the forward substitution, then the back substitution.  R is the float64 ``lanczos_kernel`` expression in both:
# the kernel values are float64 inputs of the GPU kernel.  Rows are array axes; the Python loops run over grid points.
def _mix_down(vis, mix, T):
    """``float32(y mask exp(-i omega dphi_in))`` formed in ``T``, rounded once per component (complex64).  The angle is
    the float64 product ``omega dphi`` in every type: that product of its two float64 inputs is how the reference
    (``sidereal.py:276-278``) and the kernel define the angle; its sine and cosine and all that follows are in ``T``."""
    omega, mask, dphi_in, _ = mix
    ph = (np.asarray(omega, np.float64)[:, None] * np.asarray(dphi_in, np.float64)[None, :]).astype(T)
    m = np.asarray(mask, np.float32).astype(T)[:, None]
    pr, pi = m * np.cos(ph), -m * np.sin(ph)
    yr, yi = vis.real.astype(T), vis.imag.astype(T)
    out = np.empty(vis.shape, np.complex64)
    out.real = (yr * pr - yi * pi).astype(np.float32)
    out.imag = (yr * pi + yi * pr).astype(np.float32)
    return out


def _band_wiener(vis, weight, times, samples, start, end, a, eps, pad, mask_zero_weight, mix, T, guard):
    vis = np.asarray(vis, dtype=np.complex64)
    weight = np.asarray(weight, dtype=np.float32)
    pad = 5 * a if pad is None else pad
    grid = np.arange(-pad, samples + pad, dtype=np.float64) / samples * (end - start) + start
    R = forward_matrix(grid, np.asarray(times, dtype=np.float64), a)
    ng, nrow, bw = len(grid), vis.shape[0], 2 * a - 1
    if mix is not None:
        vis = _mix_down(vis, mix, T)
    w, yr, yi = weight.astype(T), vis.real.astype(T), vis.imag.astype(T)
    # ---- the band and the right-hand side
    c = np.zeros((ng, bw + 1, nrow), dtype=T)  # c[g, k] = C[g][g - k]
    d = np.zeros((ng, 2, nrow), dtype=T)
    nz = R != 0
    for g in range(ng):
        j = np.flatnonzero(nz[g])
        if not len(j):
            continue
        s, e, lo = j[0], j[-1] + 1, max(g - bw, 0)
        t = w[:, s:e] * R[g, s:e].astype(T)
        c[g, : g - lo + 1] = np.matmul(R[lo : g + 1, s:e][::-1].astype(T), t.T)
        d[g, 0], d[g, 1] = (t * yr[:, s:e]).sum(axis=1), (t * yi[:, s:e]).sum(axis=1)
    # ---- factor L (L[g, k] = L[g][g - k], k >= 1; inv[g] = 1 / L[g][g]) and forward substitution L z = d
    L = np.zeros((ng, bw + 1, nrow), dtype=T)
    inv = np.zeros((ng, nrow), dtype=T)
    z = np.zeros((ng, 2, nrow), dtype=T)
    epsT = T(eps)
    for g in range(ng):
        m = min(bw, g)
        l = L[g]
        for k in range(m, 0, -1):
            l[k] = (c[g, k] - (l[k + 1 : m + 1] * L[g - k, 1 : m - k + 1]).sum(axis=0)) * inv[g - k]
        dd = c[g, 0] + epsT - (l[1 : m + 1] ** 2).sum(axis=0)
        if guard:
            dd = np.where(dd > 0, dd, epsT)
        inv[g] = 1 / np.sqrt(dd)
        z[g] = (d[g] - (l[1 : m + 1, None, :] * z[g - m : g][::-1]).sum(axis=0)) * inv[g]
    # ---- back substitution L^T x = z
    x = np.zeros((ng, 2, nrow), dtype=T)
    for g in range(ng - 1, pad - 1, -1):
        m = min(bw, ng - 1 - g)
        q = np.arange(1, m + 1)
        x[g] = (z[g] - (L[g + q, q][:, None, :] * x[g + 1 : g + m + 1]).sum(axis=0)) * inv[g]
    xr, xi = x[pad : pad + samples, 0].T, x[pad : pad + samples, 1].T
    nw = np.ascontiguousarray(c[pad : pad + samples, 0].T)
    if mix is not None:
        omega, mask, _, dphi_out = mix
        ph = (np.asarray(omega, np.float64)[:, None] * np.asarray(dphi_out, np.float64)[None, :]).astype(T)
        mk = np.asarray(mask, np.float32).astype(T)[:, None]
        qr, qi = mk * np.cos(ph), mk * np.sin(ph)
        xr, xi = xr * qr - xi * qi, xr * qi + xi * qr
        nw[np.asarray(mask) == 0] = 0
    if mask_zero_weight:
        nw[~np.any(weight != 0, axis=1)] = 0
    return np.ascontiguousarray(xr), np.ascontiguousarray(xi), nw


def band_wiener_truth(vis, weight, times, samples, start, end, a=5, eps=1e-3, pad=None, mask_zero_weight=False, mix=None):
    """The long-double truth: ``(x.real, x.imag, nw) [nrow, samples]`` ``np.longdouble``.  ``pad``: grid points added at
    either end (``None``: the tasks' ``5 a``).  ``mix = (omega [nrow], feed_mask [nrow], dphi_in [nt], dphi_out
    [samples])``: the mix-down ``y <- complex64(y mask exp(-i omega dphi_in))`` is formed in long double and rounded once
    (the kernel rounds there, and so does the reference's in-place product); the mix-up of ``x`` stays long double."""
    return _band_wiener(vis, weight, times, samples, start, end, a, eps, pad, mask_zero_weight, mix, np.longdouble, False)


def band_wiener_f64(vis, weight, times, samples, start, end, a=5, eps=1e-3, pad=None, mask_zero_weight=False, mix=None):
    """What the kernel does, in float64: the same band, recurrence and substitutions, ``eps`` on the diagonal and the
    ``dd <= 0 -> eps`` guard.  Not the kernel's bit pattern: its ``fma`` and the order of its sums differ from NumPy's."""
    return _band_wiener(vis, weight, times, samples, start, end, a, eps, pad, mask_zero_weight, mix, np.float64, True)


# ------------------------------------------------------------------------------------- the cases of the direct sweep
def regrid_inputs(seed, samples, nt, nrow, a, wide=False, mixing=False, times=None):
    """Jittered, sorted, slightly over-range times with one gap wider than the kernel; complex64 data; about 30 % of the
    weights zero (``wide``: weights over 1e-6 .. 1e6, 60 % zero); row 0 all zero, row 1 (if there is one) a single
    non-zero sample.  ``times``: use these time stamps in place of the seed's own.  ``mixing``: fringe rates over +-2e3 rad
    per turn, angles in [0, 2 pi), the last row's feed masked."""
    rng, other = np.random.default_rng([20261020, seed]), times
    times = np.sort(np.linspace(-0.02, 1.02, nt) + rng.uniform(-1, 1, nt) * min(0.4 * 1.04 / nt, 0.015))
    gap = (2 * a + 1.2) / samples  # at least one grid point with no sample in reach
    if gap < 0.5:
        times = times[(times < 0.37) | (times > 0.37 + gap)]
    times = times if other is None else other
    nt = len(times)
    vis = (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt))).astype(np.complex64)
    if wide:
        w = (10.0 ** rng.uniform(-6, 6, (nrow, nt))).astype(np.float32)
        w[rng.uniform(size=w.shape) < 0.6] = 0
    else:
        w = rng.uniform(0.5, 2.0, (nrow, nt)).astype(np.float32)
        w[rng.uniform(size=w.shape) < 0.3] = 0
    w[0] = 0
    if nrow > 2:
        w[1] = 0
        w[1, nt // 2] = 1.5
    mix = None
    if mixing:
        mask = np.ones(nrow, np.float32)
        mask[-1] = 0
        mix = (rng.uniform(-2e3, 2e3, nrow), mask, np.sort(rng.uniform(0, 2 * np.pi, nt)), np.linspace(0, 2 * np.pi, samples, endpoint=False))
    return times, vis, w, mix


# name -> dict(seed, samples, nt before the gap is cut, nrow, a, pad (None: 5 a), wide, mixing).  Seeds: a case whose
# share of outputs within B of a float32 rounding boundary passed 1e-3 got another one (test_regrid_twin_host.py).
def _case(seed, samples, nt, nrow, a, pad=None, wide=False, mixing=False):
    return dict(seed=seed, samples=samples, nt=nt, nrow=nrow, a=a, pad=pad, wide=wide, mixing=mixing)


REGRID_SWEEP = {}
for _a in range(1, 7):  # one full output tile and one of 6; two waves, the second with three live lanes
    REGRID_SWEEP[f"width{_a}"] = _case(23 if _a == 3 else _a, 70, 161, 67, _a)
for _a in (4, 5, 6):  # 11 samples per grid cell: spans of 85, 106 and 126 samples (the tile is clamped above 105)
    REGRID_SWEEP[f"clamp{_a}"] = _case(10 + _a, 33, 363, 5, _a)
for _s in (1, 2, 63, 64, 65, 128, 129):
    REGRID_SWEEP[f"edge{_s}"] = _case(20 + _s, _s, int(2.3 * _s) + 12, 3, 2)
for _a in (1, 3):
    for _p in (0, 1):
        REGRID_SWEEP[f"pad{_p}_width{_a}"] = _case(200 + 10 * _a + _p, 40, 92, 3, _a, pad=_p)
REGRID_SWEEP["pad_task"] = _case(260, 40, 92, 3, 3)
REGRID_SWEEP["mix5"] = _case(5, 70, 161, 67, 5, mixing=True)
REGRID_SWEEP["mix2"] = _case(2, 70, 161, 67, 2, mixing=True)
REGRID_SWEEP["wide"] = _case(300, 64, 147, 8, 5, wide=True)
REGRID_SWEEP["reuse_a"] = _case(421, 65, 150, 66, 3)
REGRID_SWEEP["reuse_b"] = _case(402, 65, 150, 66, 3)  # (the same times as reuse_a: see RegridCase)
REGRID_CLAMP_MAXSPAN = {"clamp4": 85, "clamp5": 106, "clamp6": 126}
REGRID_REFUSED = _case(500, 16, 320, 2, 6)  # spans of about 240 samples: more than the LDS tile holds
REGRID_TILE_MAX = 210
EPS = 1e-3
_CASES = {}


class RegridCase:
    """One call of the sweep: its inputs, the long-double truth and the per-row bound ``B = 8 e64``, ``e64`` the worst
    component error of ``band_wiener_f64`` against the truth in that row.  The factor 8 covers the kernel's other
    association of the same sums (each at most span + bw terms) and its ``fma``s."""

    def __init__(self, name):
        s = self.spec = REGRID_SWEEP[name] if isinstance(name, str) else name
        self.name = name if isinstance(name, str) else "unnamed"
        self.a, self.samples, self.nrow = s["a"], s["samples"], s["nrow"]
        self.pad = 5 * self.a if s["pad"] is None else s["pad"]
        times = RegridCase.get("reuse_a").times if name == "reuse_b" else None  # one plan, other rows
        self.times, self.vis, self.weight, self.mix = regrid_inputs(s["seed"], s["samples"], s["nt"], s["nrow"], s["a"], s["wide"], s["mixing"], times)
        self.nt = len(self.times)
        assert self.vis.shape == self.weight.shape == (self.nrow, self.nt)
        self.grid = np.arange(-self.pad, self.samples + self.pad, dtype=np.float64) / self.samples
        self.start, self.end, _ = compact_spans(forward_matrix(self.grid, self.times, self.a))
        self.maxspan = int((self.end - self.start).max())
        self._truth = None

    @classmethod
    def get(cls, name):
        if name not in _CASES:
            _CASES[name] = cls(name)
        return _CASES[name]

    def _args(self):
        return (self.vis, self.weight, self.times, self.samples, 0.0, 1.0, self.a, EPS, self.pad, False, self.mix)

    def truth(self):
        """``(Tr, Ti, Tw, B [nrow, 1], e64 [nrow])``, computed once."""
        if self._truth is None:
            tr, ti, tw = band_wiener_truth(*self._args())
            fr, fi, _ = band_wiener_f64(*self._args())
            e64 = np.maximum(np.abs(fr - tr).max(axis=1), np.abs(fi - ti).max(axis=1))
            self._truth = (tr, ti, tw, (8 * e64)[:, None], e64)
        return self._truth

    def rowmax(self):
        tr, ti = self.truth()[:2]
        return np.maximum(np.abs(tr).max(axis=1), np.abs(ti).max(axis=1))

    def weight_truth(self, mask_zero_weight):
        tw = self.truth()[2].copy()
        if mask_zero_weight:
            tw[~np.any(self.weight != 0, axis=1)] = 0
        return tw

    def measure(self, x, nw, mask_zero_weight=False, rounded=True):
        """The measures of ``test_gpu_regrid_direct.py`` for complex64 ``x`` and float32 ``nw [nrow, samples]``."""
        x, nw = np.asarray(x), np.asarray(nw)
        assert x.dtype == np.complex64 and nw.dtype == np.float32 and x.shape == nw.shape == (self.nrow, self.samples)
        tr, ti, _, B, _ = self.truth()
        tw = self.weight_truth(mask_zero_weight)
        m = {}
        got, T = np.stack([x.real, x.imag]), np.stack([tr, ti])
        # where the truth is an exact zero (no sample in reach, or none with weight) the solve has only zeros to add:
        # nothing is allowed there, and the element stays in the rounded-once comparison
        m["vis"], m["vis_mismatch"], m["vis_excluded"] = rounded_measure(got, T, np.where(T == 0, LD(0), np.broadcast_to(B, T.shape)))
        if not rounded:
            m["vis_mismatch"], m["vis_excluded"] = 0, 0.0
        # the weight is a sum of non-negative terms: relative error (maxspan + 2) 2**-53 before its one rounding
        Bw = LD((self.maxspan + 2) * 2.0**-53) * tw
        m["weight"], m["weight_mismatch"], m["weight_excluded"] = rounded_measure(nw, tw, Bw)
        one_ulp = np.abs(nw.astype(LD) - tw.astype(np.float32).astype(LD)) <= np.spacing(np.abs(tw).astype(np.float32)).astype(LD)
        m["weight_one_ulp"] = bool(np.isfinite(nw).all() and one_ulp.all())
        m["weight_zeros"] = bool(np.array_equal(nw == 0, tw == 0))
        return m

    def check(self, what, x, nw, mask_zero_weight=False, rounded=True):
        m = self.measure(x, nw, mask_zero_weight, rounded)
        print(f"regrid {what}: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
        assert m["vis"] <= 1.0 and m["vis_mismatch"] == 0 and m["vis_excluded"] <= EXCLUDED_CAP, (what, m)
        assert m["weight_mismatch"] == 0 and m["weight_one_ulp"] and m["weight_zeros"], (what, m)
        return m


def compact_spans(R):
    """``(start, end, values)`` as ``draco_amd.util.regrid.compact_rows`` finds them (kept here so that the twin needs
    no built library)."""
    nz = R != 0
    start = nz.argmax(axis=-1).astype(np.int32)
    end = (R.shape[-1] - nz[..., ::-1].argmax(axis=-1)).astype(np.int32)
    empty = ~nz.any(axis=-1)
    start[empty] = 0
    end[empty] = 0
    vals = np.concatenate([R[g, start[g] : end[g]] for g in range(R.shape[0])])
    return start, end, np.ascontiguousarray(vals, dtype=np.float64)


# ------------------------------------------------------------------------------- SiderealStacker's float32 arithmetic
def _invert_no_zero(x):
    """``caput.tools.invert_no_zero``: the dtype of a float input is kept, an integer input is inverted in float64."""
    x = np.asarray(x)
    out = np.zeros(x.shape, dtype=x.dtype if x.dtype.kind == "f" else np.float64)
    nz = x != 0
    out[nz] = 1.0 / x[nz]
    return out


def stack_state(n, with_var):
    """The all-zero state before the first day: flat arrays, ``sample_variance [3, n]``."""
    st = {"vis": np.zeros(n, np.complex64), "weight": np.zeros(n, np.float32), "nsample": np.zeros(n, np.uint16)}
    if with_var:
        st["sum_coeff_sq"], st["sample_variance"] = np.zeros(n, np.float32), np.zeros((3, n), np.float32)
    return st


def stack_add_f32(st, vis, weight, nsample, uniform, with_var):
    """``SiderealStacker.process`` (``sidereal.py:954-1015``) on flat arrays, in place on ``st``: every operation in the
    dtype and the order the reference executes (``nsample``: the day's own count, or ``None`` for a single day)."""
    vis, weight = np.asarray(vis, np.complex64), np.asarray(weight, np.float32)
    if nsample is not None:
        count = np.asarray(nsample, np.uint16) * (weight > 0.0)
    else:
        count = (weight > 0.0).astype(np.uint16)
    st["nsample"] += count
    if uniform:
        coeff = count.astype(np.float32)
        st["weight"] += (coeff**2) * _invert_no_zero(weight)
        sum_coeff = st["nsample"]
    else:
        coeff = weight
        st["weight"] += weight
        sum_coeff = st["weight"]
    delta_before = coeff * (vis - st["vis"])
    inv_sum_coeff = _invert_no_zero(sum_coeff)
    st["vis"] += delta_before * inv_sum_coeff
    if with_var:
        st["sum_coeff_sq"] += coeff**2
        delta_after = vis - st["vis"]
        st["sample_variance"][0] += delta_before.real * delta_after.real
        st["sample_variance"][1] += delta_before.real * delta_after.imag
        st["sample_variance"][2] += delta_before.imag * delta_after.imag


def stack_finish_f32(st, uniform, with_var):
    """``SiderealStacker.process_finish`` (``sidereal.py:1028-1060``), in place on ``st``."""
    if uniform:
        norm = st["nsample"].astype(np.float32)
        st["weight"][:] = _invert_no_zero(st["weight"]) * norm**2
    else:
        norm = st["weight"]
    if with_var:
        norm = norm - st["sum_coeff_sq"] * _invert_no_zero(norm)
        st["sample_variance"] *= np.where(st["nsample"] > 1, _invert_no_zero(norm), 0.0)[None]


def stack_days(n, seed=7):
    """Three days ``(vis, weight, nsample)`` of ``n`` elements for the bit-for-bit comparison.  By element index mod 8:
    0 ordinary; 1 never observed; 2 observed on the middle day only; 3 a zero weight on the first day; 4 a negative
    weight on the last; 5 a day count of 0 under a positive weight; 6 and 7 days that nearly cancel the running mean.
    Everything stays in float32's normal range."""
    rng = np.random.default_rng([20261020, seed, n])
    k = np.arange(n) % 8
    days = []
    base = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    for d in range(3):
        vis = (base * np.float32(1 + 0.3 * d) + 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)
        w = rng.uniform(0.5, 2.0, n).astype(np.float32)
        ns = rng.integers(1, 5, n).astype(np.uint16)
        w[k == 1] = 0
        w[(k == 2) & (d != 1)] = 0
        ns[(k == 2)] = 1
        if d == 0:
            w[k == 3] = 0
        if d == 2:
            w[k == 4] = -0.75
        if d == 1:
            ns[k == 5] = 0
        near = k >= 6
        if d > 0:  # the same weight and count as the day before, the value its negative but for a few float32 steps
            w[near], ns[near] = days[0][1][near], days[0][2][near]
            vis[near] = (-days[d - 1][0][near] * np.float32(1 + 3e-7 * d)).astype(np.complex64)
        days.append((vis, w, ns))
    return days


def stack_run(days, uniform, with_var, with_nsample, add=stack_add_f32, finish=stack_finish_f32):
    """The states after every day and after ``finish``: a list of dicts (copies)."""
    st = stack_state(len(days[0][0]), with_var)
    out = []
    for vis, w, ns in days:
        add(st, vis, w, ns if with_nsample else None, uniform, with_var)
        out.append({k: v.copy() for k, v in st.items()})
    finish(st, uniform, with_var)
    out.append({k: v.copy() for k, v in st.items()})
    return out


def fringe_phase(freq_mhz, baselines_x, feed_mask, latitude_deg, lsd):
    """``SiderealRegridder._get_phase`` in float64: ``[nfreq, nstack, len(lsd)]`` complex128."""
    c = 299792458.0
    lmbda = c / (np.asarray(freq_mhz, dtype=np.float64) * 1e6)
    u = np.asarray(baselines_x, dtype=np.float64)[None, :] / lmbda[:, None]
    omega = -2.0 * np.pi * u * np.cos(np.radians(latitude_deg))
    dphi = 2.0 * np.pi * (lsd - np.floor(lsd))
    return np.asarray(feed_mask, dtype=np.float64)[None, :, None] * np.exp(-1.0j * omega[:, :, None] * dphi[None, None, :])
