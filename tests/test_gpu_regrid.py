"""GPU regridder (`csrc/regrid.hip`, `LanczosRegridder`, `SiderealRegridder`) against the float64 twin and against
vectors produced by executing the reference (`tests/gen_golden_regrid.py` -> tests/golden/regrid.npz).

Tolerances.  The kernel works in float64 and rounds once to complex64 / float32, so against the float64 twin
(`tests/regrid_twin.py`, dense `np.linalg.solve`) the bound is `4 * 2**-24` of the row's largest output (vis) and the
same relative bound element-wise (weight): derived from the output dtype.  The reference forms its right-hand side in
float32; its own distance from the twin, `e_ref` = max |reference - twin| / max |twin|, is measured by the generator
and stored per case; against the reference vectors the bound is `2 * e_ref + 4 * 2**-24`.  Measured `e_ref`:

    over_kw5 2.7e-5, under_kw5 6.0e-5, over_kw3 1.1e-5, under_kw3 4.0e-5, inside_kw5 1.5e-5,
    task level: time_mix0 2.2e-6, time_mix1 4.9e-6, ra_mix0 7.3e-6, ra_mix1 4.0e-6

(weights: the reference is within 5e-8 relative of the twin; the bound there is `4 * 2**-24`, zero pattern identical).
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS32 = 2.0**-24


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        return {k: z[k] for k in z.files}


def _regrid(vis, weight, times, samples, start, end, kw, mzw=False, eps=1e-3):
    from draco_amd.analysis.transform import LanczosRegridder

    t = LanczosRegridder(samples=samples, kernel_width=kw, epsilon=eps, mask_zero_weight=mzw)
    t.start, t.end = start, end
    grid, v, w = t._regrid(np.ascontiguousarray(vis), np.ascontiguousarray(weight), times)
    return grid, v.cpu().numpy(), w.cpu().numpy()


def _check_twin(x, nw, xt, nwt, what):
    for k in range(x.shape[0]):
        err, top = np.abs(x[k] - xt[k]).max(), np.abs(xt[k]).max()
        print(f"{what} row {k}: vis err {err:.3e} of max {top:.3e} (bound {4 * EPS32 * top:.3e})")
        assert err <= 4 * EPS32 * top
    assert np.all(np.abs(nw - nwt) <= 4 * EPS32 * np.abs(nwt)), what
    assert np.array_equal(nw == 0, nwt == 0)


def test_fixture_cases_against_twin_and_reference(gold):
    import regrid_twin as twin

    for name in gold["regrid/names"]:
        g = lambda k: gold[f"regrid/{name}/{k}"]  # noqa: E731
        samples, kw, mzw = (int(v) for v in g("cfg"))
        start, end = (float(v) for v in g("bounds"))
        grid, x, nw = _regrid(g("vis"), g("weight"), g("times"), samples, start, end, kw, bool(mzw))
        assert x.dtype == np.complex64 and nw.dtype == np.float32 and x.shape == (6, samples)
        assert np.array_equal(grid, g("grid"))
        xt, nwt = twin.band_wiener_twin(g("vis"), g("weight"), g("times"), samples, start, end, kw, 1e-3, bool(mzw))
        _check_twin(x, nw, xt, nwt, name)
        ref, refw = g("out_vis").reshape(6, -1), g("out_weight").reshape(6, -1)
        err = np.abs(x - ref).max() / np.abs(ref).max()
        bound = 2 * float(g("e_ref")) + 4 * EPS32
        print(f"{name}: vs reference {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert np.all(np.abs(nw - refw) <= 4 * EPS32 * np.abs(refw)) and np.array_equal(nw == 0, refw == 0)
        assert not x[4].any() and not nw[4].any(), "the all-zero-weight row comes out as exact zeros"


def test_random_full_size_against_twin():
    import regrid_twin as twin

    rng = np.random.default_rng(11)
    samples, nt, nrow = 1024, 2048, 64
    times = np.sort(np.linspace(-0.01, 1.01, nt) + rng.uniform(-0.4, 0.4, nt) / nt)
    times = times[(times < 0.52) | (times > 0.535)]
    nt = len(times)
    vis = (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt))).astype(np.complex64)
    w = rng.uniform(0.5, 2, (nrow, nt)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.3] = 0
    w[17] = 0
    _, x, nw = _regrid(vis, w, times, samples, 0.0, 1.0, 5)
    xt, nwt = twin.band_wiener_twin(vis, w, times, samples, 0.0, 1.0, 5, 1e-3)
    _check_twin(x, nw, xt, nwt, "random 1024/2048")
    assert not x[17].any() and not nw[17].any()


class _Observer:
    """The fixture's observer: linear time map, feed mask, baselines, latitude (what the tasks read of a telescope)."""

    lmax = mmax = 4
    frequencies = np.array([600.0, 612.5])

    def __init__(self, gold):
        self.baselines, self.feedmask = gold["task/baselines"], gold["task/feedmask"]
        self.t0, self.day, self.latitude = (float(v) for v in gold["task/obs"])

    def unix_to_lsd(self, t):
        return (np.asarray(t, dtype=np.float64) - self.t0) / self.day


def _task_input(gold, kind):
    from draco_amd.core import containers

    cls = containers.TimeStream if kind == "time" else containers.SiderealStream
    prod = gold["task/prodstack"]
    data = cls(freq=gold["task/freq"], prod=prod, input=4, **{kind: gold[f"task/{kind}/axis"]})
    data.vis[:] = gold[f"task/{kind}/vis"]
    data.weight[:] = gold[f"task/{kind}/weight"]
    data.attrs["lsd"] = int(gold["task/lsd"])
    return data


def test_sidereal_regridder_task(gold):
    import torch

    from draco_amd.analysis.sidereal import SiderealRegridder
    from draco_amd.analysis.transform import MModeTransform
    from draco_amd.core import containers

    samples = int(gold["task/samples"])
    for name in gold["task/names"]:
        kind, mix = str(name).split("_mix")
        data = _task_input(gold, kind)
        t = SiderealRegridder(samples=samples, down_mix=bool(int(mix)))
        t.setup(_Observer(gold))
        sd = t.process(data)
        assert type(sd) is containers.SiderealStream and sd.vis.on_device and sd.weight.on_device
        assert sd.vis._host is None, "the output stays on the device"
        assert sd.vis.shape == (2, 4, samples) and sd.vis.dtype == np.complex64 and sd.weight.dtype == np.float32
        assert sd.attrs["lsd"] == int(gold["task/lsd"]) and sd.attrs["tag"] == str(gold[f"task/{name}/tag"]) == "lsd_312"
        assert np.array_equal(sd.ra, np.linspace(0.0, 360.0, samples, endpoint=False))
        assert np.array_equal(sd.freq, gold["task/freq"]) and np.array_equal(sd.index_map["prod"], gold["task/prodstack"])
        mm = MModeTransform()
        mm.setup(None)
        m = mm.process(sd)  # feeds the m-mode transform directly
        assert m.vis.on_device and torch.isfinite(torch.view_as_real(m.vis._dev)).all()
        x, nw = sd.vis[:], sd.weight[:]
        ref, refw = gold[f"task/{name}/out_vis"], gold[f"task/{name}/out_weight"]
        err = np.abs(x - ref).max() / np.abs(ref).max()
        bound = 2 * float(gold[f"task/{name}/e_ref"]) + 4 * EPS32
        print(f"task {name}: vs reference {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert np.all(np.abs(nw - refw) <= 4 * EPS32 * np.abs(refw)) and np.array_equal(nw == 0, refw == 0)
        if int(mix):
            assert not x[:, 2].any() and not nw[:, 2].any(), "the baseline with a masked feed is flagged"


def test_exceptions(gold):
    from draco_amd.analysis.sidereal import SiderealRegridder
    from draco_amd.analysis.transform import LanczosRegridder
    from draco_amd.core import containers

    data = _task_input(gold, "time")
    t = LanczosRegridder(samples=64, start=float(data.time[0]) - 1.0)
    t.setup(_Observer(gold))
    with pytest.raises(RuntimeError, match="Start or end points for regridder fall outside bounds of input data."):
        t.process(data)
    t = LanczosRegridder(samples=64)
    t.setup(_Observer(gold))
    out = t.process(data)  # bounds default to the data's
    assert type(out) is containers.TimeStream and out.vis.shape == (2, 4, 64) and out.vis.on_device
    assert out.time[0] == data.time[0] and np.isclose(out.time[1] - out.time[0], (data.time[-1] - data.time[0]) / 64)
    mm = containers.MModes(mmax=3, freq=gold["task/freq"], stack=4)
    mm.attrs["lsd"] = 312
    s = SiderealRegridder(samples=64)
    s.setup(_Observer(gold))
    with pytest.raises(TypeError, match="Invalid input data container MModes. Expected container with a `time` or an `ra` axis."):
        s.process(mm)


def test_robustness_no_nan_and_ragged_row_counts():
    rng = np.random.default_rng(3)
    samples = 128
    nt = 192  # 1.5 x samples
    times = np.sort(rng.uniform(-0.01, 1.01, nt))
    for nrow in (1, 63, 65, 379):
        vis = (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt))).astype(np.complex64)
        w = (10.0 ** rng.uniform(-6, 6, (nrow, nt))).astype(np.float32)  # weights spanning 1e-6 ... 1e6
        w[rng.uniform(size=w.shape) < 0.6] = 0  # 60 % flagged
        w[0] = 0  # an all-zero row
        if nrow > 2:
            w[1] = 0
            w[1, nt // 2] = 1.0  # a single non-zero sample
        _, x, nw = _regrid(vis, w, times, samples, 0.0, 1.0, 5)
        assert x.shape == (nrow, samples) and np.isfinite(x).all() and np.isfinite(nw).all(), nrow
        assert not x[0].any() and not nw[0].any()
        assert (nw >= 0).all()
    # rows are independent: a row's result does not depend on where in the batch it sits
    _, x1, nw1 = _regrid(vis[200:201], w[200:201], times, samples, 0.0, 1.0, 5)
    assert np.array_equal(x1[0], x[200]) and np.array_equal(nw1[0], nw[200])


def test_chain_regrid_to_dirty_map():
    """A simulated day, sampled onto jittered, gapped time stamps with the twin's forward Lanczos matrix, regridded on
    the GPU, transformed and dirty-mapped, lands as close to the map of the original day as the same chain does with
    the float64 twin in place of the GPU regridder (x 1.5: complex64 storage of the intermediate stream)."""
    import torch

    import regrid_twin as twin
    from draco_amd.analysis.mapmaker import DirtyMapMaker
    from draco_amd.analysis.sidereal import SiderealRegridder
    from draco_amd.analysis.transform import MModeTransform
    from draco_amd.core import containers
    from draco_amd.core.products import SyntheticProvider, TransitTelescope
    from draco_amd.device import Context
    from draco_amd.synthesis.stream import SimulateSidereal
    from oracle import synth as osyn

    ctx = Context.get()
    nfreq, lmax, nside, lsd, a = 2, 12, 8, 40, 5
    tel = TransitTelescope(osyn.frequencies(nfreq), lmax=lmax, ncyl=1, nfeed_cyl=3, longitude=10.0, lsd_start=1.4e9)
    bt = SyntheticProvider(tel, seed=3001)
    gen = torch.Generator(device=ctx.device).manual_seed(4)
    mp = containers.Map(nside=nside, freq=tel.frequencies, allocate=False)
    mp.attach("map", torch.randn((nfreq, 4, 12 * nside * nside), dtype=torch.float64, device=ctx.device, generator=gen))
    sim = SimulateSidereal()
    sim.setup(bt)
    day = sim.process(mp)
    vis0 = np.array(day.vis[:])
    n = vis0.shape[-1]

    rng = np.random.default_rng(8)
    nt = 4 * n
    lsds = np.sort(lsd + np.linspace(-0.05, 1.05, nt) + rng.uniform(-0.3, 0.3, nt) * 1.1 / nt)
    lsds = lsds[(lsds < lsd + 0.4) | (lsds > lsd + 0.4 + 1.5 * a / n)]  # a gap longer than the kernel
    grid, pad = twin.padded_grid(n, float(lsd), float(lsd + 1), a)
    R = twin.forward_matrix(grid, lsds, a)
    ext = vis0[..., np.arange(-pad, n + pad) % n].astype(np.complex128)  # the day is periodic
    tvis = (ext @ R).astype(np.complex64)
    tw = rng.uniform(0.5, 2.0, tvis.shape).astype(np.float32)
    tw[rng.uniform(size=tw.shape) < 0.2] = 0

    ts = containers.TimeStream(axes_from=day, time=tel.lsd_to_unix(lsds))
    ts.vis[:] = tvis
    ts.weight[:] = tw
    ts.attrs["lsd"] = lsd
    src = tel.unix_to_lsd(ts.time)

    def dirty(stream):
        t = MModeTransform()
        t.setup(bt)
        d = DirtyMapMaker(nside=nside)
        d.setup(bt)
        return np.array(d.process(t.process(stream)).map[:])

    rg = SiderealRegridder(samples=n, kernel_width=a)
    rg.setup(tel)
    sd = rg.process(ts)
    assert sd.vis.on_device
    xt, nwt = twin.band_wiener_twin(tvis.reshape(-1, len(lsds)), tw.reshape(-1, len(lsds)), src, n, float(lsd), float(lsd + 1), a, 1e-3)
    st = containers.SiderealStream(axes_from=day, attrs_from=day)
    st.vis[:] = xt.reshape(vis0.shape)
    st.weight[:] = nwt.reshape(vis0.shape)
    # the map of the original day under the regridded day's weights: the maps then differ by the interpolation error alone
    s0 = containers.SiderealStream(axes_from=day, attrs_from=day)
    s0.vis[:] = vis0
    s0.weight[:] = nwt.reshape(vis0.shape)
    m0, m_gpu, m_twin = dirty(s0), dirty(sd), dirty(st)
    e_gpu, e_twin = np.abs(m_gpu - m0).max(), np.abs(m_twin - m0).max()
    print(f"chain: |map_gpu - map_0| {e_gpu:.3e}, |map_twin - map_0| {e_twin:.3e}, map max {np.abs(m0).max():.3e}")
    assert np.isfinite(m_gpu).all() and e_twin > 0
    assert e_gpu <= 1.5 * e_twin


def test_row_chunks_give_the_same_result():
    """The factor rows go through a scratch sized by the `regrid_workspace_mib` option; with 1 MiB every wave of 64
    rows is a chunk (launch) of its own, and the result is bit for bit the one-chunk result."""
    from draco_amd.device import Context

    rng = np.random.default_rng(21)
    samples, nt, nrow = 128, 300, 379
    times = np.sort(rng.uniform(-0.01, 1.01, nt))
    vis = (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt))).astype(np.complex64)
    w = rng.uniform(0.0, 2.0, (nrow, nt)).astype(np.float32)
    _, x0, nw0 = _regrid(vis, w, times, samples, 0.0, 1.0, 5)
    ctx = Context.get()
    with ctx.options(regrid_workspace_mib=1):
        _, x1, nw1 = _regrid(vis, w, times, samples, 0.0, 1.0, 5)
    assert np.array_equal(x0, x1) and np.array_equal(nw0, nw1) and np.abs(x0[-1]).max() > 0
