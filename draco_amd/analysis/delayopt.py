"""Delay power spectrum by maximum a posteriori optimisation (NRML) on the GPU.

Drop-in for ``draco/analysis/delayopt.py``: :func:`delay_power_spectrum_maxpost`, :class:`LogLikePS`,
:class:`GaussianProcessPrior` and :class:`AddFunctions`, same names and signatures.  The reference minimises a Gaussian
likelihood in ``x = log S`` under a Matern Gaussian-process prior with ``scipy.optimize.minimize(method="Newton-CG")``.
Here the same algorithm runs for a whole batch of baselines in lock step:

* :func:`newton_cg` is a batched port of scipy's ``_minimize_newtoncg`` with ``_line_search_wolfe12`` (scipy 1.15 is
  the specification).  It is written against a small evaluator interface, ``value_grad(x, active)``,
  ``hessian(active)``, ``direction(active)``, so that in every round each active baseline has exactly one trial point
  and all of them go to the device as one batch.
* :class:`Dcsrch` / :func:`dcstep` are the MINPACK-2 line search (More and Thuente) as a reverse-communication state
  machine, and :class:`Wolfe1` is scipy's ``scalar_search_wolfe1`` around it.  If that search fails, the public
  ``scipy.optimize.line_search`` runs for that one baseline through batch-of-one evaluations, as scipy falls back.
* :class:`DeviceEvaluator` evaluates on the GPU (``csrc/nrml.hip``): one Hermitian covariance filled from one DFT of
  ``S``, one blocked Cholesky factorisation of its real embedding, and the Hessian from f64-MFMA products.
  :class:`NumpyEvaluator` is the host form for any list of functions with ``value``, ``gradient`` and ``hessian``.

A covariance that is not positive definite at any evaluation ends that baseline with ``success = False`` and the
iterates so far (the reference's caught ``LinAlgError``); nothing is raised.  ``nchan <= 1024`` and ``ndelay <= 2048``;
``ValueError`` above, there is no CPU fallback.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import scipy.linalg as la

from ..util import kernels, tools

MAX_CHAN, MAX_DELAY = 1024, 2048

# ---- the line search (MINPACK-2 dcsrch / dcstep)


def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    """A safeguarded step of the More-Thuente search and the updated interval ``(stx, fx, dx, sty, fy, dy, stp,
    brackt)``; ``stx`` is the best step so far, ``sty`` the other endpoint, ``stp`` the current step."""
    sgnd = dp * (dx / abs(dx)) if dx != 0 else 0.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if fp > fx:  # a higher value: the minimum is bracketed
            theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
            s = max(abs(theta), abs(dx), abs(dp))
            gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
            if stp < stx:
                gamma = -gamma
            p = (gamma - dx) + theta
            q = ((gamma - dx) + gamma) + dp
            r = p / q
            stpc = stx + r * (stp - stx)
            stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
            stpf = stpc if abs(stpc - stx) <= abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
            brackt = True
        elif sgnd < 0.0:  # a lower value, derivatives of opposite sign: bracketed
            theta = 3 * (fx - fp) / (stp - stx) + dx + dp
            s = max(abs(theta), abs(dx), abs(dp))
            gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
            if stp > stx:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dx
            r = p / q
            stpc = stp + r * (stx - stp)
            stpq = stp + (dp / (dp - dx)) * (stx - stp)
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            brackt = True
        elif abs(dp) < abs(dx):  # a lower value, same sign, the derivative decreases
            theta = 3 * (fx - fp) / (stp - stx) + dx + dp
            s = max(abs(theta), abs(dx), abs(dp))
            gamma = s * np.sqrt(max(0, (theta / s) ** 2 - (dx / s) * (dp / s)))
            if stp > stx:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = (gamma + (dx - dp)) + gamma
            r = p / q
            if r < 0 and gamma != 0:
                stpc = stp + r * (stx - stp)
            elif stp > stx:
                stpc = stpmax
            else:
                stpc = stpmin
            stpq = stp + (dp / (dp - dx)) * (stx - stp)
            if brackt:
                stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
                if stp > stx:
                    stpf = min(stp + 0.66 * (sty - stp), stpf)
                else:
                    stpf = max(stp + 0.66 * (sty - stp), stpf)
            else:
                stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
                stpf = min(max(stpf, stpmin), stpmax)
        else:  # a lower value, same sign, the derivative does not decrease
            if brackt:
                theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
                s = max(abs(theta), abs(dy), abs(dp))
                gamma = s * np.sqrt((theta / s) ** 2 - (dy / s) * (dp / s))
                if stp > sty:
                    gamma = -gamma
                p = (gamma - dp) + theta
                q = ((gamma - dp) + gamma) + dy
                r = p / q
                stpf = stp + r * (sty - stp)
            elif stp > stx:
                stpf = stpmax
            else:
                stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


class Dcsrch:
    """MINPACK-2 ``dcsrch``: find a step with sufficient decrease (``ftol``) and curvature (``gtol``) by reverse
    communication.  ``iterate(stp, f, g, task)`` with ``task = "START"`` and ``f, g`` at 0 first; while it returns
    ``"FG"`` evaluate at the returned step and call again.  ``"CONVERGENCE"``, ``"WARNING: ..."`` and ``"ERROR: ..."``
    end the search."""

    def __init__(self, ftol, gtol, xtol, stpmin, stpmax):
        self.ftol, self.gtol, self.xtol, self.stpmin, self.stpmax = ftol, gtol, xtol, stpmin, stpmax

    def iterate(self, stp, f, g, task):
        p5, p66, xtrapl, xtrapu = 0.5, 0.66, 1.1, 4.0
        if task == "START":
            err = None
            if stp < self.stpmin:
                err = "ERROR: STP .LT. STPMIN"
            if stp > self.stpmax:
                err = "ERROR: STP .GT. STPMAX"
            if g >= 0:
                err = "ERROR: INITIAL G .GE. ZERO"
            if self.ftol < 0 or self.gtol < 0 or self.xtol < 0 or self.stpmin < 0 or self.stpmax < self.stpmin:
                err = "ERROR: BAD TOLERANCE OR BOUND"
            if err:
                return stp, f, g, err
            self.brackt = False
            self.stage = 1
            self.finit, self.ginit = f, g
            self.gtest = self.ftol * self.ginit
            self.width = self.stpmax - self.stpmin
            self.width1 = self.width / p5
            self.stx, self.fx, self.gx = 0.0, self.finit, self.ginit
            self.sty, self.fy, self.gy = 0.0, self.finit, self.ginit
            self.stmin = 0
            self.stmax = stp + xtrapu * stp
            return stp, f, g, "FG"
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0:
            self.stage = 2
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            task = "WARNING: ROUNDING ERRORS PREVENT PROGRESS"
        if self.brackt and self.stmax - self.stmin <= self.xtol * self.stmax:
            task = "WARNING: XTOL TEST SATISFIED"
        if stp == self.stpmax and f <= ftest and g <= self.gtest:
            task = "WARNING: STP = STPMAX"
        if stp == self.stpmin and (f > ftest or g >= self.gtest):
            task = "WARNING: STP = STPMIN"
        if f <= ftest and abs(g) <= self.gtol * -self.ginit:
            task = "CONVERGENCE"
        if task[:4] in ("WARN", "CONV"):
            return stp, f, g, task
        if self.stage == 1 and f <= self.fx and f > ftest:  # the modified function
            fm = f - stp * self.gtest
            fxm = self.fx - self.stx * self.gtest
            fym = self.fy - self.sty * self.gtest
            gm, gxm, gym = g - self.gtest, self.gx - self.gtest, self.gy - self.gtest
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt = dcstep(self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt, self.stmin, self.stmax)
            self.fx = fxm + self.stx * self.gtest
            self.fy = fym + self.sty * self.gtest
            self.gx = gxm + self.gtest
            self.gy = gym + self.gtest
        else:
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt = dcstep(self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt, self.stmin, self.stmax)
        if self.brackt:
            if abs(self.sty - self.stx) >= p66 * self.width1:
                stp = self.stx + p5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
        if self.brackt:
            self.stmin, self.stmax = min(self.stx, self.sty), max(self.stx, self.sty)
        else:
            self.stmin = stp + xtrapl * (stp - self.stx)
            self.stmax = stp + xtrapu * (stp - self.stx)
        stp = min(max(stp, self.stpmin), self.stpmax) if stp == stp else stp
        if self.brackt and (stp <= self.stmin or stp >= self.stmax) or (self.brackt and self.stmax - self.stmin <= self.xtol * self.stmax):
            stp = self.stx
        return stp, f, g, "FG"


class Wolfe1:
    """scipy's ``scalar_search_wolfe1`` by reverse communication: ``advance()`` gives the next step to evaluate, or
    ``None`` when the search is over; ``feed(phi, derphi)`` takes the evaluation.  Afterwards ``stp`` is the accepted
    step (``None``: failed), ``phi1`` the value there, ``trials`` the number of evaluations."""

    MAXITER = 100

    def __init__(self, phi0, old_phi0, derphi0, c1=1e-4, c2=0.9, amax=50, amin=1e-8, xtol=1e-14):
        if old_phi0 is not None and derphi0 != 0:
            alpha1 = min(1.0, 1.01 * 2 * (phi0 - old_phi0) / derphi0)
            if alpha1 < 0:
                alpha1 = 1.0
        else:
            alpha1 = 1.0
        self._ls = Dcsrch(c1, c2, xtol, amin, amax)
        self.phi0, self.alpha1, self.phi1, self.derphi1 = phi0, alpha1, phi0, derphi0
        self.task, self.trials, self._i, self.stp, self.done = "START", 0, 0, None, False

    def advance(self):
        if self._i >= self.MAXITER:
            self.stp, self.task, self.done = None, "WARNING: dcsrch did not converge within max iterations", True
            return None
        self._i += 1
        stp, self.phi1, self.derphi1, self.task = self._ls.iterate(self.alpha1, self.phi1, self.derphi1, self.task)
        if not np.isfinite(stp):
            self.stp, self.task, self.done = None, "WARN", True
            return None
        if self.task == "FG":
            self.alpha1 = stp
            return stp
        self.stp = None if self.task[:5] == "ERROR" or self.task[:4] == "WARN" else stp
        self.done = True
        return None

    def feed(self, phi, derphi):
        self.trials += 1
        self.phi1, self.derphi1 = phi, derphi


def scalar_search_wolfe1(phi, derphi, phi0, old_phi0, derphi0, **kw):
    """:class:`Wolfe1` driven by two callables: ``(stp, phi1, phi0, trials)``."""
    w = Wolfe1(phi0, old_phi0, derphi0, **kw)
    while True:
        a = w.advance()
        if a is None:
            return w.stp, w.phi1, w.phi0, w.trials
        w.feed(phi(a), derphi(a))


# ---- the direction (scipy's truncated conjugate gradient)


def cg_direction(H, g):
    """The inner loop of scipy's Newton-CG for ``H p = -g``: ``(p, passes, flag)``; flag 3 when the ``20 N`` passes ran
    out, 0 otherwise."""
    b = -g
    maggrad = np.abs(b).sum()
    termcond = min(0.5, math.sqrt(maggrad)) * maggrad
    x = np.zeros_like(g)
    ri = -b
    p = -ri
    i = 0
    dri0 = ri @ ri
    eps3 = 3 * np.finfo(np.float64).eps
    for _ in range(20 * len(g)):
        if np.abs(ri).sum() <= termcond:
            return x, i, 0
        Ap = H @ p
        curv = p @ Ap
        if 0 <= curv <= eps3:
            return x, i, 0
        if curv < 0:
            return (x if i > 0 else dri0 / (-curv) * b), i, 0
        if not curv > 0:  # not a number: the passes would run out
            return x, i, 3
        alphai = dri0 / curv
        x = x + alphai * p
        ri = ri + alphai * Ap
        dri1 = ri @ ri
        p = -ri + (dri1 / dri0) * p
        i += 1
        dri0 = dri1
    return x, i, 3


# ---- evaluators


def matern_prior(N):
    """``Ci [N, N]`` of the estimator's prior: the inverse Matern kernel (width 5, ``nu = 1.5``, ``reg = 1e-8``)."""
    return np.ascontiguousarray(GaussianProcessPrior(N, width=5, alpha=1.0, kernel="matern", nu=1.5).Ci)


class NumpyEvaluator:
    """The evaluator interface on the host: ``funcs[b]`` has ``value(x)``, ``gradient(x)`` and ``hessian(x)``.  A
    ``LinAlgError`` or ``ValueError`` of a function marks the evaluation as failed."""

    def __init__(self, funcs):
        self.funcs = list(funcs)
        self._x = [None] * len(self.funcs)
        self._g = [None] * len(self.funcs)
        self._H = [None] * len(self.funcs)

    def value_grad(self, x, active):
        nb, N = x.shape
        f, g, ok = np.zeros(nb), np.zeros((nb, N)), np.zeros(nb, dtype=bool)
        for b in np.flatnonzero(active):
            try:
                f[b] = self.funcs[b].value(x[b])
                g[b] = self.funcs[b].gradient(x[b])
                ok[b] = True
            except (la.LinAlgError, ValueError):
                continue
            self._x[b], self._g[b] = x[b].copy(), g[b].copy()
        return f, g, ok

    def hessian(self, active):
        for b in np.flatnonzero(active):
            self._H[b] = np.array(self.funcs[b].hessian(self._x[b]))

    def direction(self, active):
        nb, N = len(self.funcs), len(self._x[int(np.flatnonzero(active)[0])])
        p, passes, flag = np.zeros((nb, N)), np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
        for b in np.flatnonzero(active):
            p[b], passes[b], flag[b] = cg_direction(self._H[b], self._g[b])
        return p, passes, flag


def _embed(X):
    """The real embedding ``[[A, -B], [B, A]]`` of a complex matrix ``A + i B``."""
    return np.block([[X.real, -X.imag], [X.imag, X.real]])


class DeviceEvaluator:
    """The evaluator interface on the GPU for ``nb`` baselines of one shape (``csrc/nrml.hip``).  The model (window,
    noise, data covariance, sample count) lies on the device: :meth:`from_prepared` builds it from the prepare pass of
    the delay transforms, :meth:`from_arrays` from host arrays.  ``Ci [N, N]`` is the prior's inverse kernel, a host
    array or a device tensor that several evaluators share; by default the Matern prior of the estimator is built
    here (an ``N x N`` inversion on the host).  A zero ``Ci`` gives the likelihood alone."""

    def __init__(self, ctx, N, chan, nb, bounds=(1e-15, 1e10), exact=True, Ci=None):
        from .. import _lib
        from ..device import ptr

        self._lib, self._ptr = _lib, ptr
        N, n = int(N), int(len(chan))
        if not (1 <= n <= MAX_CHAN and 1 <= N <= MAX_DELAY):
            raise ValueError(f"NRML: {n} channels and {N} delays, the kernels take at most {MAX_CHAN} and {MAX_DELAY}")
        self.ctx, self.N, self.n, self.nb, self.exact = ctx, N, n, int(nb), bool(exact)
        self.lo, self.hi = sorted(math.log(v) for v in bounds)
        K = 2 * n
        e = ctx.empty
        self.chan = ctx.to_device(np.ascontiguousarray(chan, dtype=np.int32))
        self.Ci = ctx.to_device(matern_prior(N) if Ci is None else Ci)
        if tuple(self.Ci.shape) != (N, N):
            raise ValueError(f"NRML: the prior's inverse kernel is {tuple(self.Ci.shape)}, {N} delays need {(N, N)}")
        self.tw, self.wv, self.Nm, self.Xe, self.nsv = e((N, 2), np.float64), ctx.zeros((nb, n), np.float64), ctx.zeros((nb, n), np.float64), ctx.zeros((nb, K, K), np.float64), ctx.zeros((nb,), np.float64)
        self.S, self.sh, self.G, self.D = e((nb, N), np.float64), e((nb, N, 2), np.float64), e((nb, K, K), np.float64), e((nb, K, K), np.float64)
        self.U, self.Y, self.R = e((nb, N, K), np.float64), e((nb, N + n, K), np.float64), e((nb, N, K), np.float64)
        self.t, self.cix = e((nb, N), np.float64), e((nb, N), np.float64)
        self.PQ = e((nb, 4, N, N), np.float64)
        self.H = e((nb, N, N), np.float64)
        self.value, self.grad = ctx.zeros((nb,), np.float64), ctx.zeros((nb, N), np.float64)
        self.p, self.info = ctx.zeros((nb, N), np.float64), ctx.zeros((nb, 2), np.int32)
        self.base = np.zeros(nb, dtype=np.int32)  # the DMM_DELAY_* word of every baseline
        self.S0 = None
        self._ws = _lib.dmm_nrml_ws(*[C.c_void_p(t.data_ptr()) for t in
                                      (self.chan, self.tw, self.wv, self.Nm, self.Xe, self.nsv, self.Ci, self.S, self.sh, self.G, self.D, self.U, self.Y, self.R, self.t, self.cix, self.PQ)])

    @staticmethod
    def bytes_per_baseline(N, n, nsample=0):
        """Device bytes one baseline of a batch takes (the workspace formula of DESIGN 7n)."""
        K = 2 * n
        ev = 8 * (2 * K * K + K * K + 2 * N * K + (N + n) * K + 5 * N * N + 8 * N + 2 * n)
        st = 8 * ((2 * nsample + 1) * K + 3 * nsample * K + nsample * 2 * N) + 2 * nsample
        return ev + st + 64

    @classmethod
    def from_prepared(cls, ctx, N, chan, win, Xp, Xd, nzt, status, **kw):
        """From ``dmm_delay_prepare(complex_td=1, coef=1)``: ``Xp [nb, ns + 1, 2 n]``, ``nzt``, ``status`` of ``wiener=1``
        (for the averaged weights) and ``Xd [nb, ns, 2 n]`` of ``wiener=0`` (the mean-removed data), on the device.  Fills the model and ``S0 [nb, N]`` (device), the closed-form starting spectrum."""
        nb, ns = int(nzt.shape[0]), int(nzt.shape[1])
        self = cls(ctx, N, chan, nb, **kw)
        lib, ptr = self._lib, self._ptr
        n, K = self.n, 2 * self.n
        win_d = ctx.to_device(np.ascontiguousarray(win, dtype=np.float64))
        work, F2, Z = ctx.empty((nb, 3, ns, K), np.float64), ctx.empty((K, 2 * self.N), np.float64), ctx.empty((nb, ns, 2 * self.N), np.float64)
        self.S0 = ctx.zeros((nb, self.N), np.float64)
        lib.check(lib.lib.dmm_nrml_start(ctx.handle, self.N, n, ns, nb, ptr(self.chan), ptr(win_d), ptr(Xp), ptr(Xd), ptr(nzt), ptr(status), ptr(work), ptr(F2), ptr(Z), ptr(self.tw), ptr(self.wv),
                                         ptr(self.Nm), ptr(self.Xe), ptr(self.nsv), ptr(self.S0)))
        self.base = status.cpu().numpy().astype(np.int32)
        ctx.uses(win_d, work, F2, Z)
        return self

    @classmethod
    def from_arrays(cls, ctx, N, chan, wv, Nm, X, nsamp, **kw):
        """From host arrays: ``wv [nb, n]`` (zero on a cut channel), ``Nm [nb, n]``, ``X [nb, n, n]`` complex,
        ``nsamp [nb]``."""
        wv = np.atleast_2d(np.asarray(wv, dtype=np.float64))
        nb = wv.shape[0]
        self = cls(ctx, N, chan, nb, **kw)
        m = np.arange(self.N) / self.N
        self.tw.copy_(ctx.to_device(np.stack([np.cos(2 * np.pi * m), np.sin(2 * np.pi * m)], axis=1)))
        self.wv.copy_(ctx.to_device(np.ascontiguousarray(wv)))
        self.Nm.copy_(ctx.to_device(np.ascontiguousarray(np.atleast_2d(Nm), dtype=np.float64)))
        self.Xe.copy_(ctx.to_device(np.stack([_embed(x) for x in np.asarray(X).reshape(nb, self.n, self.n)])))
        self.nsv.copy_(ctx.to_device(np.asarray(nsamp, dtype=np.float64).reshape(nb)))
        return self

    def _status(self, active):
        return self.ctx.to_device(np.where(np.asarray(active, dtype=bool) & (self.base == 0), 0, 1).astype(np.int32))

    def value_grad(self, x, active):
        lib, ptr = self._lib, self._ptr
        st = self._status(active)
        x_d = self.ctx.to_device(np.ascontiguousarray(x, dtype=np.float64))
        lib.check(lib.lib.dmm_nrml_eval(self.ctx.handle, self.N, self.n, self.nb, C.byref(self._ws), ptr(x_d), self.lo, self.hi, ptr(st), ptr(self.value), ptr(self.grad)))
        st_h = st.cpu().numpy()
        self.ctx.uses(x_d, st)
        self.base[st_h == lib.DMM_DELAY_NOT_POSDEF] = lib.DMM_DELAY_NOT_POSDEF
        ok = np.asarray(active, dtype=bool) & (st_h == 0)
        f, g = self.value.cpu().numpy(), self.grad.cpu().numpy()
        return np.where(ok, f, 0.0), np.where(ok[:, None], g, 0.0), ok

    def hessian(self, active, exact=None):
        lib, ptr = self._lib, self._ptr
        st = self._status(active)
        lib.check(lib.lib.dmm_nrml_hessian(self.ctx.handle, self.N, self.n, self.nb, C.byref(self._ws), int(self.exact if exact is None else exact), ptr(st), ptr(self.H)))
        self.ctx.uses(st)

    def direction(self, active):
        lib, ptr = self._lib, self._ptr
        st = self._status(active)
        lib.check(lib.lib.dmm_nrml_direction(self.ctx.handle, self.N, self.nb, ptr(self.H), ptr(self.grad), ptr(st), ptr(self.p), ptr(self.info)))
        info = self.info.cpu().numpy()
        self.ctx.uses(st)
        return self.p.cpu().numpy(), info[:, 0].astype(np.int64), info[:, 1].astype(np.int64)


# ---- the optimiser

_MESSAGES = {0: "Optimization terminated successfully.", 1: "Maximum number of iterations has been exceeded.", 2: "Desired error not necessarily achieved due to precision loss.",
             3: "CG iterations didn't converge or a value is not a number.", 4: "The covariance is not positive definite."}


def _wolfe2(ev, b, nb, xk, pk, gfk, old_fval, old_old_fval, c1, c2):
    """scipy's fall-back, the public ``scipy.optimize.line_search`` with no cap on the step (``_line_search_wolfe12``
    forwards only ``c1`` and ``c2``), through batch-of-one evaluations:
    ``(alpha, fval, old_fval, ok)``; raises ``LinAlgError`` if an evaluation fails."""
    from scipy.optimize import line_search

    act = np.zeros(nb, dtype=bool)
    act[b] = True
    cache = {}

    def both(x):
        key = x.tobytes()
        if key not in cache:
            xs = np.zeros((nb, len(x)))
            xs[b] = x
            f, g, ok = ev.value_grad(xs, act)
            if not ok[b]:
                raise la.LinAlgError("not positive definite")
            cache.clear()
            cache[key] = (float(f[b]), g[b].copy())
        return cache[key]

    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alpha, _, _, fval, old, _ = line_search(lambda x: both(x)[0], lambda x: both(x)[1], xk, pk, gfk, old_fval, old_old_fval, c1=c1, c2=c2)
    return alpha, fval, old, alpha is not None


def newton_cg(ev, x0, maxiter=None, xtol=1e-5, c1=1e-4, c2=0.9, active=None):
    """Minimise ``nb`` functions in lock step by scipy's Newton-CG.  ``ev`` is an evaluator, ``x0 [nb, N]``.  Returns a
    list of dicts per baseline: ``x`` (all iterates, the start first), ``nit``, ``status`` (scipy's ``warnflag``; 4: an
    evaluation failed), ``success``, ``message``, ``ls_trials`` (line-search evaluations per iteration)."""
    x0 = np.array(x0, dtype=np.float64, ndmin=2)
    nb, N = x0.shape
    if maxiter is None:
        maxiter = N * 200
    tol = N * xtol
    xk = x0.copy()
    act = np.ones(nb, dtype=bool) if active is None else np.array(active, dtype=bool)
    res = [dict(x=[xk[b].copy()], nit=0, status=None, ls_trials=[]) for b in range(nb)]

    def end(b, flag):
        act[b] = False
        res[b]["status"] = flag

    for b in np.flatnonzero(~act):
        res[b]["status"] = 4
    old_fval, gfk, ok = ev.value_grad(xk, act)
    old_fval, gfk = old_fval.copy(), gfk.copy()
    old_old = [None] * nb
    for b in np.flatnonzero(act & ~ok):
        end(b, 4)
    while act.any():
        for b in np.flatnonzero(act):
            if res[b]["nit"] >= maxiter:
                end(b, 1)
        if not act.any():
            break
        ev.hessian(act)
        pk, _, flag = ev.direction(act)
        for b in np.flatnonzero(act & (flag != 0)):
            end(b, 3)
        # ---- the line searches, one trial point per baseline and round
        search = {int(b): Wolfe1(old_fval[b], old_old[b], float(gfk[b] @ pk[b]), c1=c1, c2=c2) for b in np.flatnonzero(act)}
        trial = {b: w.advance() for b, w in search.items()}
        gnew = gfk.copy()
        while any(a is not None for a in trial.values()):
            m = np.zeros(nb, dtype=bool)
            xt = xk.copy()
            for b, a in trial.items():
                if a is not None:
                    m[b] = True
                    xt[b] = xk[b] + a * pk[b]
            f, g, ok = ev.value_grad(xt, m)
            for b in np.flatnonzero(m):
                if not ok[b]:
                    end(b, 4)
                    trial[b] = None
                    continue
                gnew[b] = g[b]
                search[b].feed(float(f[b]), float(g[b] @ pk[b]))
                trial[b] = search[b].advance()
        for b, w in search.items():
            if not act[b]:
                continue
            res[b]["ls_trials"].append(w.trials)
            alpha, fval = w.stp, w.phi1
            if alpha is None:
                try:
                    alpha, fval, _, found = _wolfe2(ev, b, nb, xk[b], pk[b], gfk[b], old_fval[b], old_old[b], c1, c2)
                except la.LinAlgError:
                    end(b, 4)
                    continue
                if not found:
                    end(b, 2)
                    continue
                one = np.zeros(nb, dtype=bool)
                one[b] = True
                xt = xk.copy()
                xt[b] = xk[b] + alpha * pk[b]
                f, g, ok = ev.value_grad(xt, one)  # the workspace and the gradient at the accepted point
                if not ok[b]:
                    end(b, 4)
                    continue
                gnew[b] = g[b]
            old_old[b], old_fval[b] = old_fval[b], fval
            update = alpha * pk[b]
            xk[b] = xk[b] + update
            gfk[b] = gnew[b]
            res[b]["nit"] += 1
            res[b]["x"].append(xk[b].copy())
            l1 = np.abs(update).sum()
            if not l1 > tol:
                end(b, 3 if (np.isnan(old_fval[b]) or np.isnan(l1)) else 0)
    for r in res:
        r["success"] = r["status"] == 0
        r["message"] = _MESSAGES[r["status"]]
    return res


# ---- the reference's public interface


class GaussianProcessPrior:
    """A Gaussian-process prior on the parameters: value ``x^T Ci x / 2``.  ``Ci = inv(K + reg I) / alpha^2`` with ``K``
    the ``kernel`` of :mod:`draco_amd.util.kernels` over ``arange(N)`` at unit amplitude (``alpha K`` itself for
    ``moving_average``)."""

    def __init__(self, N, *, width=5, alpha=1, kernel="gaussian", reg=1e-8, **kernel_params):
        kernel_params.update({"N": int(N), "width": int(width), "alpha": 1.0})
        K = kernels.get_kernel(kernel, **kernel_params)
        self.Ci = alpha * K if kernel == "moving_average" else la.inv(K + np.identity(N) * reg) / alpha**2

    def value(self, x):
        return 0.5 * float(x @ (self.Ci @ x))

    def gradient(self, x):
        return self.Ci @ x

    def hessian(self, x):
        return self.Ci


class AddFunctions:
    """The sum of several functions of the same parameters."""

    def __init__(self, functions):
        if len(functions) <= 0:
            raise ValueError("At least one function must be supplied.")
        self.functions = functions

    def value(self, x):
        return sum(f.value(x) for f in self.functions)

    def gradient(self, x):
        return sum(np.asarray(f.gradient(x)) for f in self.functions)

    def hessian(self, x):
        return sum(np.asarray(f.hessian(x)) for f in self.functions)


class LogLikePS:
    """Negative log-likelihood of a delay power spectrum, its gradient and Hessian in ``x = log S``.

    ``X [n, n]`` data covariance, ``MF [n, N]`` masked Fourier matrix, ``N [n]`` noise variance, ``nsamp`` samples.
    Rows of ``MF`` that are all zero are dropped (``fsel`` overrides).

    ``device=True`` (the default) evaluates on the GPU as a batch of one, with a zero prior.  This is narrower than the
    reference, which takes any ``MF``: the kernels fill the covariance from one DFT of ``S``, so every kept row must be a
    window-scaled DFT row ``w_f exp(-2 pi i c_f a / N)`` with integer ``c_f`` and ``w_f != 0`` (what
    :func:`delay_power_spectrum_maxpost` builds).  Anything else -- a general matrix, or a zero row kept through
    ``fsel`` -- raises ``ValueError``; ``device=False`` evaluates any ``MF`` in NumPy.
    """

    def __init__(self, X, MF, N, nsamp, fsel=None, exact_hessian=True, bounds=(1e-10, 1e10), device=True):
        MF = np.asarray(MF, dtype=np.complex128)
        if fsel is None:
            fsel = (MF != 0).any(axis=1)
        self.X = np.asarray(X, dtype=np.complex128)[fsel][:, fsel]
        self.N = np.asarray(N, dtype=np.float64)[fsel]
        self.MF = MF[fsel]
        self.nsamp, self.exact_hessian = nsamp, exact_hessian
        self._bounds = bounds
        self._logbounds = tuple(sorted(np.log(b) for b in bounds))
        self._at = None
        self._dev = None
        if device:
            nd = self.MF.shape[1]
            w = self.MF[:, 0].real
            if np.any(w == 0) or np.any(self.MF[:, 0].imag != 0):
                raise ValueError("LogLikePS: a kept row of MF is zero or not a window-scaled DFT row; use device=False")
            c = np.rint(-np.angle(self.MF[:, 1 % nd] / w) * nd / (2 * np.pi)).astype(np.int64) % nd if nd > 1 else np.zeros(len(w), dtype=np.int64)
            model = w[:, None] * np.exp(-2j * np.pi * ((c[:, None] * np.arange(nd)[None, :]) % nd) / nd)
            if not np.allclose(model, self.MF, rtol=0, atol=1e-12 * np.abs(w).max()):
                raise ValueError("LogLikePS: MF is not a set of window-scaled DFT rows; use device=False")
            self._chan, self._w = c, w

    def _device(self):
        if self._dev is None:
            from ..device import Context

            self._dev = DeviceEvaluator.from_arrays(Context.get(), self.MF.shape[1], self._chan, self._w, self.N, self.X, [self.nsamp], bounds=self._bounds, exact=self.exact_hessian,
                                                     Ci=np.zeros((self.MF.shape[1],) * 2))
        return self._dev

    def _precompute(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self._at is not None and np.array_equal(x, self._at):
            return
        self._H = None
        if hasattr(self, "_chan"):
            ev = self._device()
            f, g, ok = ev.value_grad(x[None, :], np.ones(1, dtype=bool))
            if not ok[0]:
                ev.base[:] = 0
                raise la.LinAlgError("LogLikePS: the covariance is not positive definite")
            self._value, self._grad = float(f[0]), g[0].copy()
        else:
            S = np.exp(np.clip(x, *self._logbounds))
            Cm = (self.MF * S) @ self.MF.conj().T
            Cm[np.diag_indices_from(Cm)] += self.N
            ch = la.cho_factor(Cm, check_finite=False)
            self._U = self.MF * np.sqrt(S)
            self._Ut = la.cho_solve(ch, self._U, check_finite=False)
            self._R = (self.X - Cm) @ self._Ut
            lndet = 2 * np.log(np.diag(ch[0]).real).sum() + np.trace(la.cho_solve(ch, self.X, check_finite=False)).real
            self._value = self.nsamp * lndet
            self._t = -(self._Ut.conj() * self._R).real.sum(axis=0)
            self._grad = self.nsamp * self._t
        self._at = x.copy()

    def value(self, x):
        self._precompute(x)
        return self._value

    def gradient(self, x):
        self._precompute(x)
        return self._grad.copy()

    def hessian(self, x):
        self._precompute(x)
        if self._H is None:
            if hasattr(self, "_chan"):
                ev = self._device()
                ev.hessian(np.ones(1, dtype=bool))
                self._H = ev.H[0].cpu().numpy()
            else:
                P = self._U.conj().T @ self._Ut
                H = (P * P.T.conj()).real  # Re(P_ab^2), P being Hermitian: the reference's form
                if self.exact_hessian:
                    Q = self._Ut.conj().T @ self._R
                    H += 2 * (Q * P.conj()).real
                    H[np.diag_indices_from(H)] += self._t
                self._H = self.nsamp * H
        return self._H.copy()


def _model_host(data, N, Ni, window, fsel):
    """``(X, MF, Nm, nsamp, S0)`` of the reference's set-up in NumPy; ``S0`` by the closed form of the pseudo-inverse
    start (the variance of the unwindowed data of the channels with ``|w| > 1e-3 max |w|``, transformed to delay)."""
    data = np.asarray(data, dtype=np.complex128)
    nsamp = data.shape[0]
    fsel = np.asarray(fsel)
    E = np.exp(-2j * np.pi * ((fsel[:, None].astype(np.int64) * np.arange(N)[None, :]) % N) / N)
    w = np.ones(len(fsel)) if window is None else np.asarray(tools.window_generalised(fsel / N, window=window), dtype=np.float64)
    Ni = np.asarray(Ni, dtype=np.float64)
    dw = data * w
    X = dw.T @ dw.conj() / nsamp
    MF = E * w[:, None]
    MF[Ni == 0] = 0.0
    live = np.abs(w[Ni != 0])
    keep = (Ni != 0) & (np.abs(w) > 1e-3 * (live.max() if live.size else 0.0))
    S0 = ((data * keep) @ E.conj() / N).var(axis=0)
    return X, MF, tools.invert_no_zero(Ni), nsamp, S0


def delay_power_spectrum_maxpost(data, N, Ni, initial_S=None, window="nuttall", fsel=None, maxiter=100, tol=1e-3, bounds=(1e-15, 1e10), device=True):
    """Estimate the delay power spectrum of ``data [nsample, freq]`` by maximum a posteriori optimisation.

    ``N`` delays, ``Ni [freq]`` inverse noise variance, ``fsel`` the indices of the channels among the full set
    (default ``arange(freq)``), the window evaluated at ``fsel / N``.  Returns ``(samples, success)``: the list of
    spectrum iterates (host arrays, the start first) and whether the optimiser converged.  A covariance that is not
    positive definite gives ``success = False`` with the samples so far.  ``device=False`` evaluates in NumPy.
    """
    data = np.asarray(data)
    nsamp, Nf = data.shape
    fsel = np.arange(Nf) if fsel is None else np.asarray(fsel)
    if len(fsel) != Nf:
        raise ValueError(f"Length of frequency selection must match frequencies passed. {len(fsel)} != {Nf}")
    N = int(N)
    if not (1 <= Nf <= MAX_CHAN and 1 <= N <= MAX_DELAY):
        raise ValueError(f"NRML: {Nf} channels and {N} delays, the kernels take at most {MAX_CHAN} and {MAX_DELAY}")
    X, MF, Nm, nsamp, S0 = _model_host(data, N, Ni, window, fsel)
    if initial_S is None:
        initial_S = S0
    if device:
        from ..device import Context

        w = MF[:, 0].real
        ev = DeviceEvaluator.from_arrays(Context.get(), N, fsel, w, Nm, X, [nsamp], bounds=bounds)
    else:
        ev = NumpyEvaluator([AddFunctions([LogLikePS(X, MF, Nm, nsamp, bounds=bounds, device=False), GaussianProcessPrior(N, width=5, alpha=1.0, kernel="matern", nu=1.5)])])
    with np.errstate(divide="ignore"):
        r = newton_cg(ev, np.log(np.asarray(initial_S, dtype=np.float64))[None, :], maxiter=maxiter, xtol=tol)[0]
    return [np.exp(x) for x in r["x"]], r["success"]


__all__ = ["AddFunctions", "DeviceEvaluator", "GaussianProcessPrior", "LogLikePS", "NumpyEvaluator", "delay_power_spectrum_maxpost", "newton_cg"]
