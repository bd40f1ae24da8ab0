"""GPU Gaussian-process regridder (``csrc/gp.hip``, ``draco_amd/util/gaussian_process.py``, ``SiderealRegridderGP``)
against the long-double twin (``tests/gp_twin.py``) on the same band-truncated matrix, and against vectors produced by
executing the reference (``tests/gen_golden_gp.py`` -> tests/golden/gp.npz).

The projection ``A = Kstar K_M^-1`` is compared with the twin under

    |A_gpu - A_twin| <= C n u cond(K_M) max_row sum|A|,      u = 2**-53,

the forward error of a Cholesky solve of order ``n`` against right-hand sides whose solutions have that row sum.  The
generator records, per case, the same distance for the reference's own float64 ``A`` (SciPy's banded solve) in units of
``n u cond max_row sum|A|``:

    kw2_r1 6.3e-3   kw2_r2 3.2e-3   kw2_r8 5.1e-4   kw2_r8_jit 4.2e-4   kw2_r8_eps 2.6e-4   kw2_edge 4.7e-4
    kw3_r4 8.6e-4   kw5_128r2 9.7e-4   kw5_128r4 4.2e-4   brutal 1.4e-3

``C = 0.0504`` is 8 times the largest of them: room for another elimination order (blocked, fused multiply-adds,
matrix-core sums), not for a different matrix.  The band edges of a row may differ from the twin's only where an entry
lies within that bound of the ``1e-8`` threshold.

Outputs: the data within the bound carried through the product (``bound x sum|x|`` over the row's span), the rounding of
the complex64 store, and ``nin 1e-8 max|x|`` for entries at the band-edge threshold; the weights within 2 float32 ulp of
the twin's float32 chain; zeros exactly where the reference has zeros, in every case.
"""

import os

import numpy as np
import pytest
import scipy.linalg

import gp_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

C_BOUND = 0.0504
U = 2.0**-53
NAMES = ["kw2_r1", "kw2_r2", "kw2_r8", "kw2_r8_jit", "kw2_r8_eps", "kw2_edge", "kw3_r4", "kw5_128r2", "kw5_128r4", "brutal", "all_masked"]
LSD = 312


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "gp.npz")) as z:
        return {k: z[k] for k in z.files}


def case(gold, name):
    kw, samples, nin, eps, nstack = gold[f"case/{name}/params"]
    g = {k: gold[f"case/{name}/{k}"] for k in ("xi", "xo", "x", "w", "mt", "xout", "wout", "M", "bound")}
    g.update(kw=int(kw), samples=int(samples), eps=float(eps), spec={"name": "matern", "width": int(kw), "alpha": 1.0, "nu": 2.5, "epsilon": float(eps)})
    return g


def run(g, freqs=None, spec=None, info=None):
    """``resample_device`` on the frequencies ``freqs`` of a case: ``(xout, wout) [nfreq, nout, nstack]`` on the host."""
    from draco_amd.device import Context
    from draco_amd.util import gaussian_process as gp

    ctx = Context.get()
    sel = slice(None) if freqs is None else list(freqs)
    vis_d = ctx.to_device(np.ascontiguousarray(np.moveaxis(g["x"][sel], 1, 2)))
    w_d = ctx.to_device(np.ascontiguousarray(np.moveaxis(g["w"][sel], 1, 2)))
    xout, wout = gp.resample_device(ctx, vis_d, w_d, g["xi"], g["xo"], 1.7, 1, spec or g["spec"], info=info)
    assert xout.is_cuda and wout.is_cuda
    return np.moveaxis(xout.cpu().numpy(), 1, 2), np.moveaxis(wout.cpu().numpy(), 1, 2)


@pytest.fixture(scope="module")
def results(gold):
    """Per case, computed once: the GPU's outputs and projections, and the twin's chain."""
    from draco_amd.util import gaussian_process as gp

    out = {}
    for name in NAMES:
        g = case(gold, name)
        info = {"keep_projection": True}
        xout, wout = run(g, info=info)
        Ki, Ks = gp._combine_gp_kernels_from_specs((g["xo"], g["xi"]), g["spec"])
        out[name] = (g, xout, wout, info, twin.resample(g["x"], g["w"], Ki, Ks, g["mt"]))
    return out


def _gpu_projection(info, ii):
    """``(rows, start, end, A dense [nk, n])`` of frequency ``ii`` as the device holds it."""
    for pas in info.get("projection", []):
        for gi, members in enumerate(pas["members"]):
            if ii in members:
                nk = len(pas["rows"][gi])
                start, end = pas["start"][gi, :nk], pas["end"][gi, :nk]
                n = pas["n"][gi]
                A = np.zeros((nk, n))
                for b in range(nk):
                    A[b, start[b] : end[b]] = pas["A"][gi, : end[b] - start[b], b]
                return pas["rows"][gi], start, end, A
    return None


@pytest.mark.parametrize("name", NAMES)
def test_projection(results, name):
    g, _, _, info, (_, _, parts) = results[name]
    e_ref, cond, rowsum, amax, order = g["bound"]
    unit = order * U * cond * rowsum
    assert name == "all_masked" or 8 * e_ref <= C_BOUND * unit * (1 + 1e-3), "C is 8 times the reference's largest recorded distance"
    for ii, p in enumerate(parts):
        got = _gpu_projection(info, ii)
        if p is None:
            assert got is None
            continue
        rows, start, end, A = got
        assert np.array_equal(rows, np.flatnonzero(g["mt"][ii])), "kept rows"
        n = int(p["mi"].sum())
        ev = np.linalg.eigvalsh(twin.band_truncate(_K(g)[p["mi"]][:, p["mi"]], p["M"]))
        At = p["A"]
        bound = C_BOUND * n * U * float(ev[-1] / ev[0]) * float(np.abs(At).sum(axis=1).max())
        cols = np.arange(n)[None, :]
        inside = (cols >= start[:, None]) & (cols < end[:, None])
        err = float(np.abs(A - At)[inside].max()) if inside.any() else 0.0
        print(f"gp {name} f{ii}: n {n} M {p['M']} cond {ev[-1] / ev[0]:.3e} |A_gpu - A_twin| {err:.3e} bound {bound:.3e} (the reference's own {e_ref:.3e}); "
              f"edges equal {np.array_equal(start, p['start']) and np.array_equal(end, p['end'])}")
        assert err <= bound
        # the band edges: an entry outside the device's span is not above the threshold, the two end entries are
        assert np.all(np.abs(At)[~inside] <= 1e-8 + bound)
        live = end > start
        assert np.all(np.abs(At[live, start[live]]) > 1e-8 - bound) and np.all(np.abs(At[live, end[live] - 1]) > 1e-8 - bound)
        assert np.array_equal(live, p["end"] > p["start"])


def _K(g, _cache={}):
    from draco_amd.util import gaussian_process as gp

    key = (g["xi"].tobytes(), g["kw"], g["eps"])
    if key not in _cache:
        _cache[key] = gp._combine_gp_kernels_from_specs((g["xo"], g["xi"]), g["spec"])[0]
    return _cache[key]


@pytest.mark.parametrize("name", NAMES)
def test_outputs(results, name):
    g, xout, wout, info, (txout, twout, parts) = results[name]
    # zeros exactly where the reference has them
    assert np.array_equal(wout == 0, g["wout"] == 0) and np.array_equal(xout == 0, g["xout"] == 0)
    assert xout.dtype == np.complex64 and wout.dtype == np.float32
    if name == "all_masked":
        assert not xout.any() and not wout.any() and info["ngroup"] == 0
        return
    e_ref, cond, rowsum, amax, order = g["bound"]
    nin = g["x"].shape[1]
    worst_x = worst_w = 0.0
    for ii, p in enumerate(parts):
        if p is None:
            assert not xout[ii].any() and not wout[ii].any()
            continue
        n = int(p["mi"].sum())
        ev = np.linalg.eigvalsh(twin.band_truncate(_K(g)[p["mi"]][:, p["mi"]], p["M"]))
        bound = C_BOUND * n * U * float(ev[-1] / ev[0]) * float(np.abs(p["A"]).sum(axis=1).max())
        xs = g["x"][ii][p["mi"]]
        span = int((p["end"] - p["start"]).max())
        xmax = float(np.abs(xs).max())
        rows = g["mt"][ii]
        t = txout[ii, rows]
        _, gstart, gend, _ = _gpu_projection(info, ii)
        edge = (gstart != p["start"]) | (gend != p["end"])  # rows with an entry within rounding of the band-edge threshold
        lim = bound * span * xmax + 2.0**-24 * np.maximum(np.abs(t.real), np.abs(t.imag)) + (nin * 1e-8 * xmax) * edge[:, None]
        d = xout[ii, rows].astype(np.complex128) - t
        assert np.all(np.abs(d.real) <= lim) and np.all(np.abs(d.imag) <= lim)
        worst_x = max(worst_x, float(np.abs(d).max()))
        tw, gw = twout[ii, rows], wout[ii, rows]
        nz = tw != 0
        if nz.any():
            ulps = np.abs(gw[nz].astype(np.float64) - tw[nz]) / np.spacing(np.abs(tw[nz]))
            worst_w = max(worst_w, float(ulps.max()))
            assert np.all(ulps <= 2)
    ref_x = float(np.abs(xout - g["xout"]).max())
    print(f"gp {name}: |xout - twin| {worst_x:.3e}, weights within {worst_w:.1f} float32 ulp of the twin's chain; to the reference's complex64 output {ref_x:.3e}")
    assert ref_x <= 2.0**-22 * float(np.abs(g["xout"]).max()) + 1e-9


def test_groups_and_band_rows(results):
    for name in NAMES[:-1]:
        g, _, _, info, _ = results[name]
        nfreq = g["x"].shape[0]
        live = [m for m in g["M"] if m]
        assert info["ngroup"] == 2, "frequencies 0 and 2 share a mask and a factorisation"
        assert sorted(info["M"]) == sorted(set(live)) and len(live) == 3 and nfreq in (3, 4)


@pytest.mark.parametrize("name", ["kw2_r2", "kw5_128r2", "kw2_r8"])
def test_batch_invariance(results, name):
    g, xout, wout, _, _ = results[name]
    for ii in range(g["x"].shape[0]):
        xa, wa = run(g, freqs=[ii])
        assert xa[0].tobytes() == xout[ii].tobytes() and wa[0].tobytes() == wout[ii].tobytes()
    xb, wb = run(g, freqs=[2, 1])
    assert xb[0].tobytes() == xout[2].tobytes() and wb[1].tobytes() == wout[1].tobytes()


def test_not_positive_definite(gold, results):
    from draco_amd.util import gaussian_process as gp

    g = case(gold, "kw2_r2")
    bad = dict(g["spec"], epsilon=-0.9)
    with pytest.raises(scipy.linalg.LinAlgError, match="frequency index 0"):
        run(g, spec=bad)
    with pytest.raises(scipy.linalg.LinAlgError, match="frequency index 1"):
        run(g, freqs=[3, 1], spec=bad)  # (frequency 3 has no weight and is skipped before anything is factored)
    # the context is usable for the next call
    xout, wout = run(g)
    assert xout.tobytes() == results["kw2_r2"][1].tobytes() and wout.tobytes() == results["kw2_r2"][2].tobytes()
    with pytest.raises(NotImplementedError):
        run(g, spec={"name": "periodic", "width": 2, "alpha": 1.0, "p": 3.0})
    assert gp.BAND_TOL == 1e-8


@pytest.mark.parametrize("name", ["kw2_r2", "kw3_r4"])
def test_host_matrices(results, name):
    """``interpolate_unweighted`` and ``resample`` with ``[freq, time, stack]`` arrays: the matrices come from the host."""
    from draco_amd.util import gaussian_process as gp

    g, xout, wout, _, _ = results[name]
    xa, wa = gp.resample(g["x"], g["w"], g["xi"], g["xo"], 1.7, 1, dict(g["spec"]))
    assert xa.is_cuda and tuple(xa.shape) == g["xout"].shape
    assert xa.cpu().numpy().tobytes() == xout.tobytes() and wa.cpu().numpy().tobytes() == wout.tobytes()
    Ki, Ks = gp._combine_gp_kernels_from_specs((g["xo"], g["xi"]), g["spec"])
    xb, wb = gp.interpolate_unweighted(g["x"], g["w"], Ki, Ks, interp_samples=g["mt"])
    xb, wb = xb.cpu().numpy(), wb.cpu().numpy()
    assert np.array_equal(wb == 0, g["wout"] == 0)
    assert np.abs(xb - g["xout"]).max() <= 2.0**-22 * np.abs(g["xout"]).max() + 1e-9
    nz = wb != 0
    assert np.all(np.abs(wb[nz] - g["wout"][nz]) <= 4 * np.spacing(g["wout"][nz]))


@pytest.mark.parametrize("kind", ["rational_gaussian", "matern15"])
def test_other_kernels(gold, kind):
    """Products of the other device kernels against the twin fed with the host's matrices."""
    from draco_amd.util import gaussian_process as gp

    g = case(gold, "kw2_r2")
    spec = {
        "rational_gaussian": [{"name": "rational", "width": 2, "alpha": 1.1, "a": 1.5, "epsilon": 1e-3}, {"name": "gaussian", "width": 6, "alpha": 0.9, "epsilon": 1e-3}],
        "matern15": [{"name": "matern", "width": 2, "alpha": 1.0, "nu": 1.5, "epsilon": 1e-3}],
    }[kind]
    Ki, Ks = gp._combine_gp_kernels_from_specs((g["xo"], g["xi"]), spec)
    mt = gp._select_interp_samples(g["xi"], g["xo"], ~np.all(g["w"] == 0, axis=-1), 6 if kind == "rational_gaussian" else 2, 1.7, 1)
    try:
        txout, twout, _ = twin.resample(g["x"], g["w"], Ki, Ks, mt)
    except np.linalg.LinAlgError:
        with pytest.raises(scipy.linalg.LinAlgError):
            run(g, spec=spec)
        return
    xout, wout = run(g, spec=spec)
    assert np.array_equal(wout == 0, twout == 0)
    assert np.abs(xout - txout).max() <= 2.0**-22 * np.abs(txout).max() + 1e-7
    nz = twout != 0
    assert np.all(np.abs(wout[nz] - twout[nz]) <= 1e-5 * twout[nz])


# ------------------------------------------------------------------------------------------------------------ the task
class _Observer:
    """Linear time map and, for down_mix, the regridder fixture's feed mask, baselines and latitude."""

    lmax = mmax = 4
    frequencies = np.array([600.0, 612.5])
    t0, day = 1.6e9, 86164.0905

    def __init__(self, mixgold=None):
        if mixgold is not None:
            self.baselines, self.feedmask, self.latitude = mixgold["task/baselines"], mixgold["task/feedmask"], float(mixgold["task/obs"][2])

    def unix_to_lsd(self, t):
        return (np.asarray(t, dtype=np.float64) - self.t0) / self.day


def _stream(freq, lsd, vis, w, form, **axes):
    from draco_amd.core import containers

    if form == "time":
        data = containers.TimeStream(freq=freq, time=_Observer.t0 + lsd * _Observer.day, **(axes or {"stack": vis.shape[1]}))
    else:
        data = containers.SiderealStream(freq=freq, ra=(lsd - LSD) * 360.0, **(axes or {"stack": vis.shape[1]}))
    data.vis[:] = vis
    data.weight[:] = w
    data.attrs["lsd"] = LSD
    return data


def test_task_against_reference(gold):
    """``SiderealRegridderGP`` on a SiderealStream: the reference's ``_regrid`` (padding trimmed) of the same day."""
    from draco_amd.analysis.sidereal import SiderealRegridderGP

    g = case(gold, "kw2_r2")
    vis, w = np.moveaxis(g["x"], 1, 2), np.moveaxis(g["w"], 1, 2)
    data = _stream(600.0 + np.arange(4), LSD + g["xi"], vis, w, "ra")
    t = SiderealRegridderGP(samples=32, kernel_width=2)
    t.setup(_Observer())
    sd = t.process(data)
    assert sd.vis.on_device and sd.weight.on_device and sd.attrs["tag"] == "lsd_312" and tuple(sd.vis.shape) == (4, 3, 32)
    rv, rw = gold["task/vis"], gold["task/vis_weight"]
    assert np.array_equal(sd.weight[:] == 0, rw == 0)
    assert np.abs(sd.vis[:] - rv).max() <= 2.0**-22 * np.abs(rv).max() + 1e-7  # (the positions went through LSD + x - LSD)
    nz = rw != 0
    assert np.all(np.abs(sd.weight[:][nz] - rw[nz]) <= 1e-5 * rw[nz])
    assert np.allclose(sd.ra, np.arange(32) * 360.0 / 32)


@pytest.mark.parametrize("form", ["time", "ra"])
def test_task_down_mix(gold, form):
    """Down-mix on a TimeStream and a SiderealStream against the twin with the mixing done on the host in complex64."""
    import regrid_twin
    from draco_amd.analysis.sidereal import SiderealRegridderGP
    from draco_amd.util import gaussian_process as gp

    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        mixgold = {k: z[k] for k in z.files if k.startswith("task/")}
    g = case(gold, "kw3_r4")
    obs = _Observer(mixgold)
    prod, freq = mixgold["task/prodstack"], mixgold["task/freq"]
    rng = np.random.default_rng(7)
    nt = len(g["xi"])
    ph = regrid_twin.fringe_phase(freq, obs.baselines[:, 0], np.ones(4), obs.latitude, LSD + g["xi"])
    vis = (0.3 * (rng.normal(size=(2, 4, nt)) + 1j * rng.normal(size=(2, 4, nt))) + np.conj(ph)).astype(np.complex64)
    w = rng.uniform(0.5, 2.0, (2, 4, nt)).astype(np.float32)
    w[:, :, 60:80] = 0
    w[1, 1, 100] = 0
    data = _stream(freq, LSD + g["xi"], vis, w, form, prod=prod, input=4)
    src = obs.unix_to_lsd(data.time) if form == "time" else LSD + data.ra / 360.0
    outs = {}
    for mix in (False, True):
        t = SiderealRegridderGP(samples=64, kernel_width=3, down_mix=mix)
        t.setup(obs)
        sd = t.process(data)
        assert sd.vis.on_device and sd.vis._host is None
        outs[mix] = (np.array(sd.vis[:]), np.array(sd.weight[:]))
    fm = obs.feedmask[prod["input_a"], prod["input_b"]]
    xi = np.asarray(src, dtype=np.float64) - LSD
    Ki, Ks = gp._combine_gp_kernels_from_specs((g["xo"], xi), g["spec"])
    for mix in (False, True):
        x = vis.copy()
        if mix:
            x *= regrid_twin.fringe_phase(freq, obs.baselines[:, 0], fm, obs.latitude, src)
        xm, wm = np.moveaxis(x, 1, 2), np.moveaxis(w, 1, 2)
        mt = gp._select_interp_samples(xi, g["xo"], ~np.all(wm == 0, axis=-1), 3, 1.7, 1)
        tx, tw, _ = twin.resample(xm, wm, Ki, Ks, mt)
        tx, tw = np.moveaxis(tx, 1, 2)[..., 15:-15], np.moveaxis(tw, 1, 2)[..., 15:-15]
        if mix:
            pout = regrid_twin.fringe_phase(freq, obs.baselines[:, 0], fm, obs.latitude, np.arange(64) / 64)
            tx = tx.astype(np.complex64) * np.conj(pout)
            tw = tw * (np.abs(pout) > 0)
        gv, gw = outs[mix]
        assert np.array_equal(gw == 0, tw == 0)
        assert np.abs(gv - tx).max() <= 2.0**-21 * np.abs(tx).max()
        nz = tw != 0
        assert np.all(np.abs(gw[nz] - tw[nz]) <= 2 * np.spacing(tw[nz].astype(np.float32)))
        if mix:
            assert not gv[:, 2].any() and not gw[:, 2].any(), "the baseline with a masked feed is flagged"
    assert np.abs(outs[True][0] - outs[False][0])[:, [0, 1, 3]].max() > 1e-4, "mixing down changes what is interpolated"


def test_chain_regrid_stack_mmodes(gold):
    """TimeStream -> SiderealRegridderGP -> SiderealStacker, twice -> MModeTransform: everything stays on the device."""
    import torch

    from draco_amd.analysis.sidereal import SiderealRegridderGP, SiderealStacker
    from draco_amd.analysis.transform import MModeTransform

    g = case(gold, "kw5_128r2")
    vis, w = np.moveaxis(g["x"], 1, 2)[:2], np.moveaxis(g["w"], 1, 2)[:2]
    stacker = SiderealStacker()
    for _ in range(2):
        data = _stream(np.array([600.0, 612.5]), LSD + g["xi"], vis, w, "time")
        t = SiderealRegridderGP(samples=128)
        t.setup(_Observer())
        sd = t.process(data)
        assert sorted(sd.datasets) == ["vis", "vis_weight"] and all(ds.on_device for ds in sd.datasets.values())
        day = np.array(sd.vis[:])
        stacker.process(sd)
    stack = stacker.process_finish()
    assert all(isinstance(ds._dev_t, torch.Tensor) for ds in stack.datasets.values())
    seen = stack.weight[:] > 0
    assert seen.any() and np.abs(stack.vis[:] - day)[seen].max() <= 2.0**-22 * np.abs(day).max()
    mm = MModeTransform()
    mm.setup(None)
    m = mm.process(stack)
    assert m.vis.on_device and torch.isfinite(torch.view_as_real(m.vis._dev)).all()
