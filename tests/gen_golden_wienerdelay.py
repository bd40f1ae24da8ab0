"""Generate tests/golden/wienerdelay.npz by EXECUTING the reference's own ``ConstructWienerDelayTransform`` and
``ApplyWienerDelayTransform`` (``draco/analysis/powerspec.py:118-458``: the two ``process`` methods, ``_get_prior`` and
``_get_window``) from source, unmodified, through ``oracle._refstub`` on fake containers in the style of
``gen_golden_powerspec.py`` (here with ``allgather`` and ``create_index_map``).  Only the data is committed; run where
the reference checkout exists:

    python tests/gen_golden_wienerdelay.py

Every case is run twice, with the fake operator's ``filter`` dataset complex64 (what the reference's container stores)
and complex128.  Per case the file holds

* the inputs.  They are exactly representable so that the file is small and every machine sees the same bits:
  ``K = diag(mask)(I + Q / 64)`` with ``Q`` a banded matrix of small integers, ``var``, ``w``, ``dirty_beam_power`` and
  the map multiples of 1 / 64, ``C = K diag(var) K^T`` (then exact in float64), all as int16 numerators
  (``wienerdelay_twin.case_inputs`` rebuilds them).  The physical case P20 and the ungated case U20 store a true DAYENU
  ``K`` and its ``C`` as float64;
* the per-task constants of the reference: ``window`` (its ``_get_window``), ``sdiag`` (its ``_get_prior``), ``tau``;
* ``ref64``: the reference's complex64 operator (all pixels; at order 70 the pixels of ``ref_pixels`` only);
* ``e_ref64 = rel_err(complex128 run, truth)`` and ``e_ref = rel_err(complex64 run, truth rounded to complex64)``, the
  truth being ``wienerdelay_twin.build`` in long double rounded once.  The truth of a whole case does not fit the size
  limit of a committed file (253 KB at order 33, incompressible, and no bit-pattern difference to a stored array is
  smaller): the tests recompute it with the same twin, and ``truth_check`` holds the generator's truth of the pixels
  ``check_pixels`` (all of them at orders 6 and 20, two or one at orders 33 and 70) so that a test machine whose long
  double differs is noticed;
* for the apply task, run on the reference's complex64 operator: ``spec`` and ``sweight`` of the reference, ``e_ref_spec``
  and ``e_ref_w`` against ``wienerdelay_twin.apply`` in long double, the attributes and index maps of the result.

The gated cases assert ``cond(A_valid) <= 1e5`` on every pixel.  U20 (``epsilon`` 1e-12, the default ``prior_amp``;
condition number 3e11) is informative only: its errors are printed by the tests, not bounded.  SING is a pixel made
singular by construction (a channel masked in ``K``, so ``diag C = 0`` there, but kept by the weights; ``prior_amp`` 0):
the reference's ``cho_factor`` raises ``LinAlgError``, which the generator asserts.
"""

import importlib
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wienerdelay_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = twin.DF


class Arr(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    local_array = property(lambda s: s.view(np.ndarray))
    local_shape = property(lambda s: s.shape)

    def allgather(self):
        return self.view(np.ndarray)


class DS:
    def __init__(self, arr, axis=None):
        self.arr = np.asarray(arr).view(Arr)
        self.attrs = {"axis": axis}

    def __getitem__(self, k):
        return self.arr[k]

    def __setitem__(self, k, v):
        self.arr[k] = v

    shape = property(lambda s: s.arr.shape)
    local_shape = property(lambda s: s.arr.shape)


class Fake:
    AXES = ()
    SPEC = {}
    OPTIONAL = {}

    def __init__(self, axes_from=None, attrs_from=None, **axes):
        self.index_map, self.attrs, self.comm = {}, {}, None
        if axes_from is not None:
            self.index_map.update({ax: axes_from.index_map[ax] for ax in self.AXES if ax in axes_from.index_map})
        for ax, val in axes.items():
            self.index_map[ax] = np.arange(val) if isinstance(val, (int, np.integer)) else np.asarray(val)
        if attrs_from is not None:
            self.attrs.update(attrs_from.attrs)
        self.datasets = {n: DS(np.zeros(tuple(len(self.index_map[a]) for a in ax), dtype=dt), ax) for n, (ax, dt) in self.SPEC.items()}

    def add_dataset(self, name):
        ax, dt = self.OPTIONAL[name]
        self.datasets[name] = DS(np.zeros(tuple(len(self.index_map[a]) for a in ax), dtype=dt), ax)

    def create_index_map(self, name, values):
        self.index_map[name] = np.asarray(values)

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("datasets", {}):
            return d["datasets"][name]
        raise AttributeError(name)

    def redistribute(self, axis):
        pass

    @property
    def freq(self):
        return self.index_map["freq"]


_MAT = ["pol", "freq", "freq_sum", "ra"]


class RingMap(Fake):
    AXES = ("beam", "pol", "freq", "freq_sum", "ra", "el")
    SPEC = {"map": (["beam", "pol", "freq", "ra", "el"], np.float64), "weight": (["pol", "freq", "ra", "el"], np.float64),
            "dirty_beam_power": (["beam", "pol", "freq", "el"], np.float64), "filter": (_MAT, np.float64), "freq_cov": (_MAT, np.float64)}


class DelayTransformOperator(Fake):
    AXES = ("pol", "ra", "el", "delay", "freq")
    DTYPE = np.complex64

    def __init__(self, **kw):
        self.SPEC = {"filter": (["pol", "ra", "el", "delay", "freq"], self.DTYPE)}
        super().__init__(**kw)


class DelayTransform(Fake):
    AXES = ("baseline", "sample", "delay")
    SPEC = {"spectrum": (["baseline", "sample", "delay"], np.complex128)}
    OPTIONAL = {"weight": (["baseline", "sample", "delay"], np.float32)}


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def q64(x):
    q = np.rint(np.asarray(x) * 64.0).astype(np.int16)
    assert np.array_equal(q / 64.0, x)
    return q


def coarse_inputs(rng, npol, n, nra, nel, nmask):
    """``Q`` banded (half width 2) of integers in [-6, 6], ``nmask`` channels masked per (pol, ra) in ``K`` and in the
    weights, ``var`` in [1, 2], ``w`` in [1/2, 2] with one weight in twelve zero, ``dbp`` in [1/2, 3/2]."""
    Q = rng.integers(-6, 7, size=(npol, n, n, nra)).astype(np.int16)
    band = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 2
    Q *= band[np.newaxis, :, :, np.newaxis].astype(np.int16)
    kmask = np.ones((npol, n, nra), dtype=bool)
    for p in range(npol):
        for r in range(nra):
            kmask[p, rng.choice(np.arange(1, n - 1), size=nmask, replace=False), r] = False
    var = rng.integers(64, 129, size=(npol, n, nra)) / 64.0
    w = rng.integers(32, 129, size=(npol, n, nra, nel)) / 64.0
    w[rng.random(size=w.shape) < 1.0 / 12] = 0.0
    w *= kmask[:, :, :, np.newaxis]
    dbp = rng.integers(32, 97, size=(npol, n, nel)) / 64.0
    m = rng.integers(-511, 512, size=(1, npol, n, nra, nel)) / 64.0
    return Q, kmask, var, w, dbp, m


def dayenu_k(freq, mask, tauw, epsilon):
    """The reference's ``delay_filter`` matrix for one set of flags (``dayenu.py:1179-1199``)."""
    dfreq = freq[:, np.newaxis] - freq[np.newaxis, :]
    cov = np.eye(freq.size) + np.sinc(2.0 * tauw * dfreq) / epsilon
    mm = mask[:, np.newaxis] & mask[np.newaxis, :]
    return np.linalg.pinv(mm * cov, hermitian=True) * mm


def ring_map(freq, K, C, w, dbp, m):
    npol, n, nra, nel = w.shape
    rm = RingMap(beam=1, pol=np.array(["XX", "YY"][:npol]), freq=freq, freq_sum=freq, ra=10.0 + 0.5 * np.arange(nra), el=np.linspace(-0.5, 0.5, nel))
    rm.attrs["tag"] = "wd"
    rm.map[:], rm.weight[:], rm.dirty_beam_power[:], rm.filter[:], rm.freq_cov[:] = m, w, dbp[np.newaxis], K, C
    return rm


def run_case(mod, out, name, freq, K, C, w, dbp, m, cfg, gated=True, ref_pixels=None, check_pixels=((0, 0, 0),), store_float=False, Q=None, kmask=None, var=None):
    cfgd = dict(prior_amp=2.8e-5, prior_scale=0.0, window="uniform", window_lower_freq=None, window_upper_freq=None)
    cfgd.update(cfg)
    rm = ring_map(freq, K, C, w, dbp, m)
    ops = {}
    for dt in (np.complex64, np.complex128):
        DelayTransformOperator.DTYPE = dt
        task = make_task(mod.ConstructWienerDelayTransform, **cfgd)
        ops[dt] = task.process(rm)
    op64, op128 = ops[np.complex64], ops[np.complex128]
    window = np.asarray(task._get_window(freq), dtype=np.float64)
    tau = np.asarray(op64.index_map["delay"])
    sdiag = task._get_prior(tau)
    tau_t, F, sdiag_t = twin.constants(freq, window, cfgd["prior_amp"], cfgd["prior_scale"])
    assert np.array_equal(tau, tau_t) and np.array_equal(sdiag, sdiag_t)
    cond = twin.cond_valid(K, C, w, dbp, F, sdiag, window)
    if gated:
        assert cond <= 1e5, (name, cond)
    truth = twin.build(K, C, w, dbp, F, sdiag, window, ld=True)
    t128 = truth.astype(np.complex128)
    r64, r128 = np.array(op64.filter[:]), np.array(op128.filter[:])
    e_ref64 = twin.rel_err(r128, t128)
    e_ref = twin.rel_err(r64, t128.astype(np.complex64))
    e_np = twin.rel_err(twin.build(K, C, w, dbp, F, sdiag, window, ld=False), t128)
    print(f"{name}: operator {r64.shape} ntau {int((window > 0).sum())} cond {cond:.3e} e_ref64 {e_ref64:.3e} e_ref {e_ref:.3e} float64 twin {e_np:.3e}")

    if store_float:
        out[f"{name}/K"], out[f"{name}/C"] = K, C
    else:
        assert np.array_equal(twin.kmatrix(Q, kmask), K) and np.array_equal(twin.cov_of(K, var), C)
        out[f"{name}/Q"], out[f"{name}/kmask"], out[f"{name}/var_q64"] = Q, kmask, q64(var)
    out.update({f"{name}/w_q64": q64(w), f"{name}/dbp_q64": q64(dbp), f"{name}/map_q64": q64(m), f"{name}/freq": freq, f"{name}/window": np.array(cfgd["window"]),
                f"{name}/prior_amp": np.array(cfgd["prior_amp"]), f"{name}/prior_scale": np.array(cfgd["prior_scale"]), f"{name}/win": window, f"{name}/sdiag": sdiag, f"{name}/tau": tau,
                f"{name}/e_ref64": np.array(e_ref64), f"{name}/e_ref": np.array(e_ref), f"{name}/cond": np.array(cond), f"{name}/gated": np.array(gated)})
    for k in ("window_lower_freq", "window_upper_freq"):
        out[f"{name}/{k}"] = np.array(np.nan if cfgd[k] is None else cfgd[k])
    if ref_pixels is None:
        out[f"{name}/ref64"] = r64
    else:
        out[f"{name}/ref_pixels"] = np.array(ref_pixels)
        out[f"{name}/ref64"] = np.stack([r64[p] for p in ref_pixels])
    if check_pixels == "all":
        check_pixels = [(p, r, e) for p in range(t128.shape[0]) for r in range(t128.shape[1]) for e in range(t128.shape[2])]
    out[f"{name}/check_pixels"] = np.array(check_pixels)
    out[f"{name}/truth_check"] = np.stack([t128[p] for p in check_pixels])
    for attr in ("window", "window_lower_freq", "window_upper_freq"):
        assert op64.attrs[attr] == cfgd[attr]

    # ---- the apply task on the complex64 operator
    res = make_task(mod.ApplyWienerDelayTransform).process(rm, op64)
    spec, sw = np.array(res.spectrum[:]), np.array(res.weight[:])
    assert sw.dtype == np.float32
    t_spec, t_w = twin.apply(r64, m[0], w, ld=True)
    e_spec = twin.rel_err(spec, t_spec.astype(np.complex128))
    e_w = twin.rel_err(sw, t_w.astype(np.float32))
    print(f"{name}: apply e_ref_spec {e_spec:.3e} e_ref_w {e_w:.3e} baseline_axes {list(res.attrs['baseline_axes'])}")
    out.update({f"{name}/spec": spec, f"{name}/sweight": sw, f"{name}/e_ref_spec": np.array(e_spec), f"{name}/e_ref_w": np.array(e_w), f"{name}/baseline_axes": np.array(res.attrs["baseline_axes"]),
                f"{name}/out_pol": res.index_map["pol"], f"{name}/out_el": res.index_map["el"], f"{name}/out_sample": res.index_map["sample"], f"{name}/out_delay": res.index_map["delay"],
                f"{name}/out_freq": np.asarray(res.attrs["freq"])})
    for attr in ("window_los", "window_los_lower_freq", "window_los_upper_freq"):
        v = res.attrs[attr]
        out[f"{name}/attr_{attr}"] = np.array(np.nan if v is None else v)


def main():
    _refstub.load_reference()
    mod = importlib.import_module("draco.analysis.powerspec")
    mod.tools.invert_no_zero = _refstub._invert_no_zero
    mod.containers = types.SimpleNamespace(DelayTransformOperator=DelayTransformOperator, DelayTransform=DelayTransform, RingMap=RingMap)
    out = {}

    def coarse_case(name, seed, npol, n, nra, nel, nmask, cfg, special=False, **kw):
        rng = np.random.default_rng(seed)
        freq = 600.0 + DF * np.arange(n)
        Q, kmask, var, w, dbp, m = coarse_inputs(rng, npol, n, nra, nel, nmask)
        if special:
            w[0, :, 0, 0] = 0.0  # a pixel without a valid channel
            keep = int(np.flatnonzero(kmask[0, :, 1])[n // 2])
            one = np.zeros(n)
            one[keep] = 1.5
            w[0, :, 1, 1] = one  # a pixel with one valid channel
        K = twin.kmatrix(Q, kmask)
        C = twin.cov_of(K, var)
        run_case(mod, out, name, freq, K, C, w, dbp, m, cfg, Q=Q, kmask=kmask, var=var, **kw)

    f6 = 600.0 + DF * np.arange(6)
    coarse_case("G6E", 6001, 2, 6, 3, 5, 1, dict(prior_amp=1.0), check_pixels="all")  # ntau 6
    coarse_case("G6O", 6002, 2, 6, 3, 5, 1, dict(prior_amp=0.75, prior_scale=0.25, window_lower_freq=float(f6[0] + DF / 2)), check_pixels="all")  # ntau 5
    coarse_case("G33", 3301, 2, 33, 3, 5, 3, dict(prior_amp=1.0, prior_scale=0.125, window="hann"), special=True, check_pixels=((0, 0, 1), (1, 2, 4)))
    f70 = 600.0 + DF * np.arange(70)
    coarse_case("G70", 7001, 1, 70, 2, 2, 4, dict(prior_amp=0.5, window="hann", window_lower_freq=float(f70[3] - DF / 4), window_upper_freq=float(f70[66] + DF / 4)),
                ref_pixels=((0, 0, 0), (0, 1, 1)), check_pixels=((0, 1, 0),))

    # ---- a true DAYENU filter at order 20: gated (epsilon 1e-3, a prior of the order of the noise) and ungated
    for name, eps, amp, gated in (("P20", 1e-3, 1.0, True), ("U20", 1e-12, 2.8e-5, False)):
        rng = np.random.default_rng(2001)
        n, npol, nra, nel = 20, 1, 2, 3
        freq = 600.0 + DF * np.arange(n)
        _, kmask, var, w, dbp, m = coarse_inputs(rng, npol, n, nra, nel, 2)
        K = np.stack([np.stack([dayenu_k(freq, kmask[p, :, r], 0.2, eps) for r in range(nra)], axis=-1) for p in range(npol)])
        C = twin.cov_of(K, var)
        run_case(mod, out, name, freq, K, C, w, dbp, m, dict(prior_amp=amp, window="hann"), gated=gated, store_float=True, check_pixels="all")

    # ---- a pixel singular by construction: the reference raises
    rng = np.random.default_rng(6003)
    Q, kmask, var, w, dbp, m = coarse_inputs(rng, 1, 6, 2, 2, 0)
    kmask[0, 2, 1] = False  # masked in K, kept by the weights
    w[w == 0] = 1.0
    K = twin.kmatrix(Q, kmask)
    C = twin.cov_of(K, var)
    DelayTransformOperator.DTYPE = np.complex64
    try:
        make_task(mod.ConstructWienerDelayTransform, prior_amp=0.0, prior_scale=0.0, window="uniform").process(ring_map(f6, K, C, w, dbp, m))
        raise AssertionError("the reference did not raise on the singular pixel")
    except np.linalg.LinAlgError as exc:
        print("SING: the reference raises", repr(exc))
    out.update({"SING/Q": Q, "SING/kmask": kmask, "SING/var_q64": q64(var), "SING/w_q64": q64(w), "SING/dbp_q64": q64(dbp), "SING/map_q64": q64(m), "SING/freq": f6,
                "SING/window": np.array("uniform"), "SING/prior_amp": np.array(0.0), "SING/prior_scale": np.array(0.0), "SING/window_lower_freq": np.array(np.nan),
                "SING/window_upper_freq": np.array(np.nan)})

    path = os.path.join(GOLDEN, "wienerdelay.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 520 * 1024


if __name__ == "__main__":
    main()
