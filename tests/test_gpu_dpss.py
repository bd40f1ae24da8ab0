"""GPU DPSS inpainting (`csrc/dpss.hip`, `draco_amd/util/dpss.py`, `draco_amd/analysis/interpolate.py`) against a
long-double truth and against vectors produced by executing the reference (`tests/gen_golden_dpss.py` ->
tests/golden/dpss.npz, dpss_basis_f1024.npz, dpss_basis_r1100.npz).

Measures: for the data `e = max |got - truth| / max |truth|`; for the weights the largest elementwise relative error
where the truth is non-zero, and the zero patterns must be equal.  The truth (`tests/dpss_twin.py` in long double, the
variance in the reference's direct form) is rounded to complex64 / float32.  Required, for data and weights alike:

* `e_gpu <= max(32 e_f64, floor)`, `e_f64` the same measure of the float64 twin (which forms the variance as the
  library does): the factor 32 covers another summation order and factorisation route over at most 4096 terms; the
  floors, `2**-22` for the data and `2**-21` for the weights, are float32 rounding of the output, doubled;
* `e_gpu <= e_ref`, the reference's own (float32) error;
* against the reference's own vectors: `<= 3 e_ref + floor`.

Stored by the generator (vis, weight): `e_ref` f70 1.9e-5, 9.5e-3; f161 1.5e-4, 6.4e-5; r140 8.8e-5, 4.8e-3; f1024
9.7e-5, 2.1e-4; r1100 9.7e-5, 2.9e-4; `e_f64` is zero (the rounded float64 twin equals the rounded truth) except for
the weights of f70 and r140, 5.9e-7 and 5.8e-7: their columns with one and two valid samples have a solved variance
far below `a_i^T C^-1 a_i`, where the identity `var_i = a_i^T C^-1 a_i - Si |C^-1 a_i|^2` cancels.
Each test prints its measured errors before it asserts.
"""

import os
import types

import numpy as np
import pytest

import dpss_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = 1e-3
FUNCTION_CASES = ["f70", "f161", "r140", "f1024", "r1100"]
SMALL_CASES = ["f70", "f161", "r140"]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "dpss.npz")) as z:
        g = {k: z[k] for k in z.files}
    for name in ("f1024", "r1100"):
        with np.load(os.path.join(GOLDEN, f"dpss_basis_{name}.npz")) as z:
            g[f"{name}/A"] = z["A"]
    return g


def _case(gold, name):
    return {k.split("/")[1]: v for k, v in gold.items() if k.startswith(name + "/")}


def _check(name, gv, gw, tv, tw, rv, rw, e_ref, e_f64):
    e_v, (e_w, same) = twin.rel_err(gv, tv), twin.weight_err(gw, tw)
    r_v, (r_w, same_r) = twin.rel_err(gv, rv), twin.weight_err(gw, rw)
    print(f"dpss {name}: e_gpu vis {e_v:.3e} weight {e_w:.3e}  e_f64 {e_f64[0]:.3e} {e_f64[1]:.3e}  e_ref {e_ref[0]:.3e} {e_ref[1]:.3e}  (to the reference {r_v:.3e} {r_w:.3e})")
    assert gv.dtype == np.complex64 and gw.dtype == np.float32
    assert np.isfinite(gv.view(np.float32)).all() and np.isfinite(gw).all()
    assert same and same_r, name
    assert e_v <= max(32 * e_f64[0], twin.FLOOR_VIS) and e_w <= max(32 * e_f64[1], twin.FLOOR_W), (name, e_v, e_w)
    assert e_v <= e_ref[0] and e_w <= e_ref[1], (name, e_v, e_w)
    assert r_v <= 3 * e_ref[0] + twin.FLOOR_VIS and r_w <= 3 * e_ref[1] + twin.FLOOR_W, (name, r_v, r_w)


@pytest.mark.parametrize("name", FUNCTION_CASES)
def test_filter_and_inpaint(gold, name):
    from draco_amd.util import dpss

    g = _case(gold, name)
    x, w, A = g["x"], g["w"], g["A"]
    W = w > 0
    xf, wf = dpss.filter(x, w, A, W, EPS)
    assert xf.is_cuda and wf.is_cuda and tuple(xf.shape) == x.shape
    xf, wf = xf.cpu().numpy(), wf.cpu().numpy()
    _check(name, xf, wf, g["truth_x"], g["truth_w"], g["ref_filter_x"], g["ref_filter_w"], g["e_ref"], g["e_f64"])
    xi, wi = (t.cpu().numpy() for t in dpss.inpaint(x, w, A, W, EPS))
    assert np.array_equal(xi[W].view(np.uint32), x[W].view(np.uint32)) and np.array_equal(wi[W].view(np.uint32), w[W].view(np.uint32))
    assert np.array_equal(xi[~W].view(np.uint32), xf[~W].view(np.uint32)) and np.array_equal(wi[~W].view(np.uint32), wf[~W].view(np.uint32))
    flag = dpss.flag_above_cutoff(W, float(g["fc"]))
    assert flag.is_cuda and np.array_equal(flag.cpu().numpy(), g["ref_flag"])
    assert np.array_equal(dpss.flag_above_cutoff(W, None).cpu().numpy(), W)


@pytest.mark.parametrize("name", SMALL_CASES)
def test_project_solve_accumulate(gold, name):
    """The pieces against the whole: `project` against the float64 product (`n u` per accumulated term, `n <= 161`:
    1e-13 of the largest entry), and `accumulate_variance(Ni, solve(project(x - xhat)), W)` with the mean added back
    against `filter`.  The composition rounds the solved weight to float32 once more than `filter` does and the data
    once before the mean is added: two more roundings of `2**-24`, inside the doubled floors."""
    from draco_amd.util import dpss

    g = _case(gold, name)
    x, w, A = g["x"], g["w"], g["A"]
    W = w > 0
    xp = dpss.project(x, w, A)
    assert xp.is_cuda and tuple(xp.shape) == (A.shape[1], x.shape[1])
    want = A.astype(np.float64).T @ (w.astype(np.float64) * x.astype(np.complex128))
    e_p = twin.rel_err(xp.cpu().numpy(), want)
    e_pr = twin.rel_err(xp.cpu().numpy(), g["ref_project"])
    e_ref_p = twin.rel_err(g["ref_project"], want)
    print(f"dpss {name}: project against float64 {e_p:.3e}; the reference's own {e_ref_p:.3e}, gpu to it {e_pr:.3e}")
    assert e_p <= 1e-13 and e_pr <= 3 * e_ref_p + 1e-13
    xhat = np.array([x[W[:, c], c].astype(np.complex128).mean() if W[:, c].any() else 0.0 for c in range(x.shape[1])])
    xs, ws = dpss.solve(dpss.project(x.astype(np.complex128) - xhat[np.newaxis, :], w, A), w, A, EPS)
    wa = dpss.accumulate_variance(w, ws, W)
    xf, wf = (t.cpu().numpy() for t in dpss.filter(x, w, A, W, EPS))
    e_v = twin.rel_err(xs.cpu().numpy().astype(np.complex128) + xhat[np.newaxis, :], xf)
    e_w, same = twin.weight_err(wa.cpu().numpy(), wf)
    print(f"dpss {name}: project + solve + accumulate_variance against filter: vis {e_v:.3e} weight {e_w:.3e}")
    assert same and e_v <= twin.FLOOR_VIS and e_w <= twin.FLOOR_W


def _stream(g, vis=None, weight=None):
    from draco_amd.core import containers

    nstack = g["vis"].shape[1]
    kw = dict(stack=g["stack"]) if "stack" in g else {}
    if "prodstack" in g:
        kw = dict(prod=g["prodstack"], input=int(g["feedmap"].shape[0]))
    elif "stack" not in g:
        kw = dict(stack=nstack)
    s = containers.SiderealStream(freq=g["freq"], ra=g["ra"], **kw)
    s.vis[:] = g["vis"] if vis is None else vis
    s.weight[:] = g["weight"] if weight is None else weight
    return s


def _task(g, name, **over):
    from draco_amd.analysis import interpolate as ip

    cls = {"t_plain": ip.DPSSFilter, "t_delay": ip.DPSSFilterDelayStokesI, "t_mmode": ip.DPSSFilterMMode}[name]
    cfg = {k[4:]: v.tolist() for k, v in g.items() if k.startswith("cfg_")}
    cfg.update(epsilon=EPS)
    cfg.update(over)
    task = cls(**cfg)
    if name == "t_plain":
        task.setup()
    elif name == "t_delay":
        task.setup(types.SimpleNamespace(lmax=1, mmax=1, frequencies=None))
    else:
        task.setup(types.SimpleNamespace(lmax=1, mmax=1, frequencies=None, feedmap=g["feedmap"], baselines=g["baselines"], freq_start=float(g["freq_start"]), latitude=float(g["latitude"])))
    return task


@pytest.mark.parametrize("name", ["t_plain", "t_delay", "t_mmode"])
def test_task(gold, name):
    g = _case(gold, name)
    axis = 0 if str(g["axis"]) == "freq" else 2
    task = _task(g, name)
    s = _stream(g)
    out = task.process(s)
    assert out is not s and out.vis.on_device and out.weight.on_device
    # copy=True leaves the input alone, bit for bit
    assert np.array_equal(s.vis[:].view(np.uint32), g["vis"].view(np.uint32)) and np.array_equal(s.weight[:].view(np.uint32), g["weight"].view(np.uint32))
    vis, weight = out.vis[:], out.weight[:]
    if name != "t_plain":
        assert np.allclose(task._get_baseline_cuts(), g["baseline_cuts"], rtol=1e-14, atol=0)
    # the truth from the bases the task itself cached (the same host LAPACK): long double, and the float64 twin's error
    samples = g["freq"] if axis == 0 else g["ra"]
    modes, amap, cutoff = task._get_basis(np.asarray(samples, dtype=np.float64))
    bases = [m.A.cpu().numpy() for m in modes]
    assert len(task._basis_cache) == len(bases) == len(g["cuts"]) and np.array_equal(amap, g["amap"]) and cutoff == pytest.approx(float(g["cutoff"]), rel=1e-14)
    for b, a0 in zip(bases, [g[f"A{i}"] for i in range(len(bases))]):
        assert b.shape == a0.shape
    tv, tw = twin.task_columns(g["vis"], g["weight"], axis, bases, amap, EPS, cutoff, True, ld=True)
    fv, fw = twin.task_columns(g["vis"], g["weight"], axis, bases, amap, EPS, cutoff, True, ld=False)
    e_f64 = (twin.rel_err(fv, tv), twin.weight_err(fw, tw)[0])
    _check(name, vis, weight, tv, tw, g["ref_vis"], g["ref_weight"], g["e_ref"], e_f64)
    keep = g["weight"] > 0
    assert np.array_equal(vis[keep].view(np.uint32), g["vis"][keep].view(np.uint32))
    # a second process reuses the cached bases; copy=False works in place; inpaint=False filters every sample
    again = task.process(_stream(g))
    assert len(task._basis_cache) == len(bases) and np.array_equal(again.vis[:].view(np.uint32), vis.view(np.uint32))
    s2 = _stream(g)
    same = _task(g, name, copy=False).process(s2)
    assert same is s2 and s2.vis.on_device
    assert np.array_equal(s2.vis[:].view(np.uint32), vis.view(np.uint32)) and np.array_equal(s2.weight[:].view(np.uint32), weight.view(np.uint32))
    filt = _task(g, name, inpaint=False).process(_stream(g))
    fv2, fw2 = twin.task_columns(g["vis"], g["weight"], axis, bases, amap, EPS, cutoff, False, ld=False)
    e_v, (e_w, same_z) = twin.rel_err(filt.vis[:], fv2), twin.weight_err(filt.weight[:], fw2)
    print(f"dpss {name}: inpaint=False against the float64 twin: vis {e_v:.3e} weight {e_w:.3e}")
    assert same_z and e_v <= twin.FLOOR_VIS and e_w <= twin.FLOOR_W
    assert np.array_equal(filt.vis[:][~keep].view(np.uint32), vis[~keep].view(np.uint32))


def test_time_stream(gold):
    """A `TimeStream` along frequency gives what the `SiderealStream` of the same numbers gives."""
    from draco_amd.core import containers

    g = _case(gold, "t_plain")
    ts = containers.TimeStream(freq=g["freq"], time=1.0e9 + 10.0 * np.arange(g["vis"].shape[2]), stack=g["vis"].shape[1])
    ts.vis[:] = g["vis"]
    ts.weight[:] = g["weight"]
    a = _task(g, "t_plain").process(ts)
    b = _task(g, "t_plain").process(_stream(g))
    assert isinstance(a, containers.TimeStream)
    assert np.array_equal(a.vis[:].view(np.uint32), b.vis[:].view(np.uint32)) and np.array_equal(a.weight[:].view(np.uint32), b.weight[:].view(np.uint32))


def test_batches(gold):
    """A workspace that holds one column at a time gives the same bits as one batch."""
    g = _case(gold, "t_delay")
    one = _task(g, "t_delay").process(_stream(g))
    from draco_amd.util import dpss

    task = _task(g, "t_delay", workspace_mib=0)
    assert dpss.batch_columns(161, 52, task.workspace_mib) == 1 and dpss.batch_columns(161, 52, 1024) > g["vis"].shape[1] * g["vis"].shape[2]
    many = task.process(_stream(g))
    assert np.array_equal(one.vis[:].view(np.uint32), many.vis[:].view(np.uint32)) and np.array_equal(one.weight[:].view(np.uint32), many.weight[:].view(np.uint32))


def test_order_4096():
    """The largest order along RA: `n = 4096`, `k = 301`, 3 columns, no stored vector.  The basis is the orthonormal
    real Fourier basis up to m = 150 (analytic: an eigen-decomposition of order 4096 has no place in a test); the truth
    is the float64 twin, run here.

    Bound.  Both sides solve with a Cholesky factor in float64: the computed `y = C^-1 v` carries a relative error of
    about `n u cond(C)`, `u = 2**-53` (`n` bounds the length of every accumulation, `k <= n`).  For the data that is
    `4096 x 1.1e-16 x cond(C)`, below 1e-9 at `cond(C) <= 1.5e3`: the floor `2**-22` of the float32 output decides.
    The solved variance is `s_i - Si |y_i|^2` with `s_i = a_i^T C^-1 a_i`; its absolute error is about `n u cond(C)
    s_i` on either side, so the relative error of the weight `inz(var_i + p_i)`, `p_i >= 0` the PCHIP term, is at most
    `n u cond(C) max_i s_i / (var_i + p_i)`.  Both sides' errors and the margin for another summation order go into
    the factor 32, as at function level: `e_w <= 2**-21 + 32 n u cond(C) max_i s_i / (var_i + p_i)`, every quantity
    taken from the twin's float64 matrices, none from the code under test."""
    from draco_amd.util import dpss

    n, mmax, ncol = 4096, 150, 3
    i = np.arange(n)
    cols = [np.full(n, 1.0 / np.sqrt(n))]
    for m in range(1, mmax + 1):
        cols += [np.sqrt(2.0 / n) * np.cos(2.0 * np.pi * m * i / n), np.sqrt(2.0 / n) * np.sin(2.0 * np.pi * m * i / n)]
    A = np.stack(cols, axis=1).astype(np.float32)
    k = A.shape[1]
    rng = np.random.default_rng(4096)
    x = np.zeros((n, ncol), dtype=np.complex128)
    for _ in range(4):
        m = rng.integers(-mmax + 10, mmax - 10, size=ncol)
        x += rng.uniform(0.5, 2.0, size=ncol) * np.exp(2j * np.pi * (i[:, None] * m[None, :] / n + rng.uniform(size=ncol)))
    x = (x + 0.3 - 0.2j + 0.01 * (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape))).astype(np.complex64)
    w = rng.uniform(0.5, 1.5, size=(n, ncol)).astype(np.float32)
    for c in range(ncol):
        for j0 in rng.integers(5, n - 10, size=40):
            w[j0 : j0 + int(rng.integers(1, 5)), c] = 0.0
    w[[0, 31, 32, 2047, 2048, 4095], 0] = 0.0
    w[4000:4009, 1] = 0.0
    w[1500:1900, 2] = 0.0  # about 29 modes fit this gap: their eigenvalues of C fall to Si, cond(C) rises to 1.5e3
    W = w > 0
    xf, wf = (t.cpu().numpy() for t in dpss.filter(x, w, A, W, EPS))
    tv, tw = twin.filter_columns(x, w, A, W, EPS)
    a64 = A.astype(np.float64)
    amp, cond = 0.0, 0.0
    for c in range(ncol):
        Cm = (a64.T * w[:, c]) @ a64 + EPS * np.eye(k)
        ev = np.linalg.eigvalsh(Cm)
        cond = max(cond, float(ev.max() / ev.min()))
        s = np.einsum("ik,ik->i", a64 @ np.linalg.inv(Cm), a64)
        amp = max(amp, float(np.max(s * np.abs(tw[:, c]))))  # tw = 1 / (var + p)
    limit_w = twin.FLOOR_W + 32 * n * 2.0**-53 * cond * amp
    e_v, (e_w, same) = twin.rel_err(xf, tv.astype(np.complex64)), twin.weight_err(wf, tw.astype(np.float32))
    print(f"dpss order 4096: k {k} cond(C) {cond:.3e} max s / (var + p) {amp:.3e}: e_gpu vis {e_v:.3e} (limit {twin.FLOOR_VIS:.3e}) weight {e_w:.3e} (limit {limit_w:.3e})")
    assert np.isfinite(xf.view(np.float32)).all() and np.isfinite(wf).all() and same
    assert cond <= 1.6e3
    assert e_v <= twin.FLOOR_VIS and e_w <= limit_w


def test_failure_path(gold, caplog):
    """A negative epsilon makes every `C = A^T Ni A + epsilon I` indefinite (`Ni <= 1.5`, the basis orthonormal): no
    exception, nothing NaN, the data unchanged, every weight zero, and an error in the log."""
    g = _case(gold, "t_delay")
    for copy in (True, False):
        out = _task(g, "t_delay", epsilon=-10.0, copy=copy).process(_stream(g))
        vis, weight = out.vis[:], out.weight[:]
        assert np.isfinite(vis.view(np.float32)).all() and np.isfinite(weight).all()
        assert not weight.any()
        assert np.array_equal(vis.view(np.uint32), g["vis"].view(np.uint32))
    assert any("Failed" in r.getMessage() for r in caplog.records)
    from draco_amd.util import dpss

    f = _case(gold, "f161")
    with pytest.raises(np.linalg.LinAlgError):
        dpss.filter(f["x"], f["w"], f["A"], f["w"] > 0, -10.0)


def test_errors(gold):
    from draco_amd.analysis import interpolate as ip
    from draco_amd.core import containers
    from draco_amd.util import dpss

    g = _case(gold, "f161")
    x, w, A = g["x"], g["w"], g["A"]
    Ac = dpss.get_basis(dpss.make_covariance(g["samples"], [0.1], [0.2]))
    assert np.iscomplexobj(Ac)
    for fn in (dpss.filter, dpss.inpaint):
        with pytest.raises(NotImplementedError, match="complex"):
            fn(x, w, Ac, w > 0)
    with pytest.raises(NotImplementedError, match="complex"):
        dpss.project(x, w, Ac)
    with pytest.raises(NotImplementedError, match="complex"):
        dpss.solve(np.zeros((Ac.shape[1], x.shape[1]), np.complex64), w, Ac)
    t = _case(gold, "t_plain")
    with pytest.raises(NotImplementedError, match="complex"):
        _task(t, "t_plain", centres=[0.1]).process(_stream(t))
    with pytest.raises(NotImplementedError, match="mask"):
        ip.DPSSFilter(halfwidths=[0.3], centres=[0.0]).setup(mask=types.SimpleNamespace(mask=np.zeros((70, 5), dtype=bool)))
    with pytest.raises(ValueError, match="4097"):
        dpss.filter(np.zeros((4097, 1), np.complex64), np.ones((4097, 1), np.float32), np.ones((4097, 1), np.float32), np.ones((4097, 1), dtype=bool))
    with pytest.raises(ValueError, match="4097"):
        dpss.flag_above_cutoff(np.ones((4097, 1), dtype=bool), 2.5)
    with pytest.raises(ValueError, match="Shape mismatch"):
        dpss.filter(x[:-1], w[:-1], A, w[:-1] > 0)
    big = containers.SiderealStream(freq=800.0 - 0.1 * np.arange(1025), ra=2, stack=1)
    big.weight[:] = 1.0
    task = ip.DPSSFilter(halfwidths=[0.3], centres=[0.0])
    task.setup()
    with pytest.raises(ValueError, match="1025"):
        task.process(big)
    wide = containers.SiderealStream(freq=np.array([600.0, 601.0]), ra=4097, stack=1)
    task = ip.DPSSFilter(halfwidths=[0.01], centres=[0.0], axis="ra")
    with pytest.raises(ValueError, match="4097"):
        task.process(wide)
    with pytest.raises(ValueError, match="No matching axes"):
        ip.DPSSFilter(halfwidths=[0.3], centres=[0.0], iter_axes=["el"]).process(_stream(t))
