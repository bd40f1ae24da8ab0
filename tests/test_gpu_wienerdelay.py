"""GPU Wiener delay transform (`csrc/wienerdelay.hip`, `ConstructWienerDelayTransform` / `ApplyWienerDelayTransform`)
against a long-double truth and against vectors produced by executing the reference
(`tests/gen_golden_wienerdelay.py` -> tests/golden/wienerdelay.npz).

Build, complex128 form: `e_gpu = max |gpu - truth| / max |truth|` with the truth (`tests/wienerdelay_twin.py`, long
double with a complex long-double Cholesky) rounded once; required `e_gpu <= max(2 e_ref64, 2**-51)`, `e_ref64` the same
measure of the reference's complex128 run (stored by the generator): the convention of `test_gpu_delay.py` on the same
solver, the factor 2 for another rounding order, the floor one float64 ulp, doubled.  Build, complex64 form: bit-equal to
the complex128 form rounded once, and `rel_err` to the reference's complex64 vectors `<= 3 e_ref + 2**-23`.  The ungated
case U20 (condition number 3e11) prints its figures only.  Exact properties: the zero operator of an empty pixel, zero
columns of masked and window-zero channels, the same bits whatever the slab, two runs the same bits, `LinAlgError` on a
pixel singular by construction (a status path, not a fault).

Apply: the spectrum against the long-double truth formed from the complex64 operator, `e_gpu <= max(2 e_ref_spec,
2**-51)`; the float32 weight against the reference to `3 e_ref_w + 2**-23`; a channel without weight contributes nothing;
attributes and index maps equal the reference's.  Chain: Construct -> Apply -> SpatialTransformDelayMap with every
dataset on the device equals the transform of a host copy of the same DelayTransform bit for bit.

Every input container is device resident.  Each test prints its figures before it asserts.
"""

import numpy as np
import pytest

import wienerdelay_twin as twin
from test_wienerdelay_host import CASES, GATED, case, gold, ref_pixels, truth_of  # noqa: F401  (gold: the fixture)

pytestmark = pytest.mark.gpu

FLOOR = 2.0**-51
POLS = np.array(["XX", "YY"])


def ring_map(c, device=True, el_values=None):
    from draco_amd.core import containers
    from draco_amd.device import Context

    npol, n, nra, nel = c["w"].shape
    el = np.linspace(-0.5, 0.5, nel) if el_values is None else el_values
    rm = containers.RingMap(beam=1, pol=POLS[:npol], freq=c["freq"], ra=10.0 + 0.5 * np.arange(nra), el=el)
    rm.attrs["tag"] = "wd"
    rm.map[:], rm.weight[:] = c["map"], c["w"]
    for name, val in (("dirty_beam_power", c["dbp"][np.newaxis]), ("filter", c["K"]), ("freq_cov", c["C"])):
        rm.add_dataset(name, allocate=True)
        rm.datasets[name][:] = val
    if device:
        ctx = Context.get()
        for ds in rm.datasets.values():
            ds.set_device(ctx.to_device(np.ascontiguousarray(ds.host())))
    return rm


def construct(c, **kw):
    from draco_amd.analysis import powerspec as ps

    return ps.ConstructWienerDelayTransform(**{**c["cfg"], **kw})


_built = {}


def built(gold, name):
    """(complex128 operator, complex64 operator) of a case as host arrays, one slab, computed once."""
    if name not in _built:
        c = case(gold, name)
        rm = ring_map(c)
        task = construct(c)
        tau, op128 = task._build(rm, np.complex128)
        tau64, op64 = task._build(rm, np.complex64)
        assert np.array_equal(tau, c["tau"]) and np.array_equal(tau64, c["tau"])
        a, b = op128.cpu().numpy(), op64.cpu().numpy()
        a.setflags(write=False)
        b.setflags(write=False)
        _built[name] = (a, b)
    return _built[name]


@pytest.mark.parametrize("name", CASES)
def test_build_complex128(gold, name):
    truth, _ = truth_of(gold, name)
    got, _ = built(gold, name)
    e_ref64 = float(gold[f"{name}/e_ref64"])
    e_gpu = twin.rel_err(got, truth.astype(np.complex128))
    print(f"wienerdelay {name}: e_gpu {e_gpu:.3e} e_ref64 {e_ref64:.3e} ratio {e_gpu / e_ref64:.2f} cond {float(gold[f'{name}/cond']):.2e}")
    assert got.dtype == np.complex128 and np.isfinite(got.view(np.float64)).all()
    if bool(gold[f"{name}/gated"]):
        assert e_gpu <= max(2 * e_ref64, FLOOR), (name, e_gpu, e_ref64)


@pytest.mark.parametrize("name", CASES)
def test_build_complex64(gold, name):
    got128, got64 = built(gold, name)
    ref = gold[f"{name}/ref64"]
    sel = np.stack([got64[p] for p in ref_pixels(gold, name, got64.shape)]).reshape(ref.shape)
    e_ref = float(gold[f"{name}/e_ref"])
    e_gpu = twin.rel_err(sel, ref)
    print(f"wienerdelay {name}: complex64 to the reference {e_gpu:.3e} e_ref {e_ref:.3e}")
    assert got64.dtype == np.complex64
    assert np.array_equal(got64.view(np.uint32), got128.astype(np.complex64).view(np.uint32))  # one computation, cast at the store
    if bool(gold[f"{name}/gated"]):
        assert e_gpu <= 3 * e_ref + 2.0**-23, (name, e_gpu, e_ref)


def test_task_output(gold):
    c = case(gold, "G6O")
    rm = ring_map(c)
    out = construct(c).process(rm)
    assert out.filter.on_device and out.filter.dtype == np.complex64
    assert np.array_equal(out.filter[:].view(np.uint32), built(gold, "G6O")[1].view(np.uint32))
    assert np.array_equal(out.index_map["delay"], c["tau"]) and np.array_equal(out.index_map["pol"], rm.index_map["pol"])
    for k in ("ra", "el"):
        assert np.array_equal(out.index_map[k], rm.index_map[k])
    assert np.array_equal(out.index_map["freq"], rm.index_map["freq"])
    assert out.attrs["window"] == "uniform" and out.attrs["window_lower_freq"] == c["cfg"]["window_lower_freq"] and out.attrs["window_upper_freq"] is None
    assert out.attrs["tag"] == "wd"


def test_exact_zeros(gold):
    c = case(gold, "G33")
    got, _ = built(gold, "G33")
    assert not got[0, 0, 0].any()  # the pixel without a valid channel
    keep = np.flatnonzero(c["w"][0, :, 1, 1])
    assert keep.size == 1 and got[0, 1, 1][:, keep[0]].any()  # the pixel with one valid channel: one column
    wm = c["win"] > 0
    assert not wm[0] and not wm[-1]  # (the edge zeros of the Hann window)
    M = wm[np.newaxis, :, np.newaxis, np.newaxis] & (c["w"] > 0)  # [pol, freq, ra, el]
    cols = np.broadcast_to(M.transpose(0, 2, 3, 1)[:, :, :, np.newaxis, :], got.shape)
    assert (~cols).any() and not got[~cols].any()


def test_slabs_and_repeats(gold):
    c = case(gold, "G33")
    rm = ring_map(c)
    one, _ = built(gold, "G33")
    n, nd = c["freq"].size, c["tau"].size
    # a pixel of order 33 takes 8 (10 n^2 + 2 n ndelay + n) bytes and a little: 1 MiB holds ten, so per polarisation the
    # five elevations of two RA make one slab and those of the third a ragged second one -- four slabs in all
    assert (1 << 20) // (8 * (10 * n * n + 2 * n * nd + n) + n + 4) == 10
    _, again = construct(c, workspace_mib=1)._build(rm, np.complex128)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), one.view(np.uint64))
    _, twice = construct(c)._build(rm, np.complex128)
    assert np.array_equal(twice.cpu().numpy().view(np.uint64), one.view(np.uint64))
    # fifteen elevations (the five, three times): slabs of ten and a ragged one of five elevations per RA
    c3 = dict(c, w=np.tile(c["w"], (1, 1, 1, 3)), dbp=np.tile(c["dbp"], (1, 1, 3)), map=np.tile(c["map"], (1, 1, 1, 1, 3)))
    _, tiled = construct(c, workspace_mib=1)._build(ring_map(c3), np.complex128)
    assert np.array_equal(tiled.cpu().numpy().view(np.uint64), np.tile(one, (1, 1, 3, 1, 1)).view(np.uint64))


def test_slabs_ragged(gold):
    # nothing couples elevations: the operator of el slices of 2, 2 and 1 (what a caller does whose operator does not fit
    # the device) is the operator of the whole map
    c = case(gold, "G6E")
    one, _ = built(gold, "G6E")
    el = np.linspace(-0.5, 0.5, 5)
    parts = []
    for sl in (slice(0, 2), slice(2, 4), slice(4, 5)):
        cs = dict(c, w=c["w"][..., sl], dbp=c["dbp"][..., sl], map=c["map"][..., sl])
        parts.append(construct(c)._build(ring_map(cs, el_values=el[sl]), np.complex128)[1].cpu().numpy())
    assert np.array_equal(np.concatenate(parts, axis=2).view(np.uint64), one.view(np.uint64))


def test_singular_pixel(gold):
    from draco_amd.device import Context

    c = case(gold, "SING")
    assert c["cfg"]["prior_amp"] == 0.0 and c["C"][0, 2, 2, 1] == 0.0 and (c["w"][0, 2, 1] > 0).all()
    with pytest.raises(np.linalg.LinAlgError, match=r"\(pol, ra, el\) = \(0, 1, 0\)"):
        construct(c).process(ring_map(c))
    Context.get().sync()
    # the context works on: the next build is the same as before
    ok = case(gold, "G6E")
    _, again = construct(ok)._build(ring_map(ok), np.complex128)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), built(gold, "G6E")[0].view(np.uint64))


def test_limits(gold):
    from draco_amd.analysis import powerspec as ps
    from draco_amd.core import containers

    c = case(gold, "G6E")
    rm = ring_map(c)
    free = ps._free_device_bytes
    try:
        ps._free_device_bytes = lambda ctx: 1000
        with pytest.raises(ValueError, match="el slice"):
            construct(c).process(rm)
    finally:
        ps._free_device_bytes = free
    big = containers.RingMap(beam=1, pol=POLS[:1], freq=600.0 + twin.DF * np.arange(1025), ra=1, el=np.array([0.0]))
    with pytest.raises(ValueError, match="1025 frequencies"):
        construct(c).process(big)
    rm.datasets["complex_filter"] = rm.datasets["filter"]
    with pytest.raises(NotImplementedError):
        construct(c).process(rm)


# ---- apply


def operator_of(gold, name, rm):
    from draco_amd.core import containers
    from draco_amd.device import Context

    op = containers.DelayTransformOperator(delay=gold[f"{name}/tau"], axes_from=rm, attrs_from=rm, allocate=False)
    op.attach("filter", Context.get().to_device(np.ascontiguousarray(gold[f"{name}/ref64"])))
    c = case(gold, name)["cfg"]
    op.attrs.update(window=c["window"], window_lower_freq=c["window_lower_freq"], window_upper_freq=c["window_upper_freq"])
    return op


@pytest.mark.parametrize("name", ["G6E", "G6O", "G33", "P20"])
def test_apply(gold, name):
    from draco_amd.analysis import powerspec as ps

    c = case(gold, name)
    rm = ring_map(c)
    out = ps.ApplyWienerDelayTransform().process(rm, operator_of(gold, name, rm))
    assert out.spectrum.on_device and out.weight.on_device
    spec, sw = out.spectrum[:], out.weight[:]
    assert spec.dtype == np.complex128 and sw.dtype == np.float32
    t_spec, t_w = twin.apply(gold[f"{name}/ref64"], c["map"][0], c["w"], ld=True)
    e_ref, e_ref_w = float(gold[f"{name}/e_ref_spec"]), float(gold[f"{name}/e_ref_w"])
    e_gpu = twin.rel_err(spec, t_spec.astype(np.complex128))
    e_tri = twin.rel_err(spec, gold[f"{name}/spec"])
    e_w = twin.rel_err(sw, gold[f"{name}/sweight"])
    e_wt = twin.rel_err(sw, t_w.astype(np.float32))
    print(f"wienerdelay apply {name}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} (to the reference {e_tri:.3e}); weight to the reference {e_w:.3e}, to the truth {e_wt:.3e}, e_ref_w {e_ref_w:.3e}")
    assert e_gpu <= max(2 * e_ref, FLOOR)
    assert e_tri <= 3 * e_ref + FLOOR
    assert e_w <= 3 * e_ref_w + 2.0**-23
    # a pixel without weights: variance 0, weight 0; attributes and index maps as the reference's
    if name == "G33":
        assert not sw[0, 0].any() and not spec[0, 0].any()  # (baseline 0 = pol 0, el 0; ra 0)
    assert list(out.attrs["baseline_axes"]) == list(gold[f"{name}/baseline_axes"]) == ["pol", "el"]
    for key, ax in (("out_pol", "pol"), ("out_el", "el"), ("out_sample", "sample"), ("out_delay", "delay")):
        assert np.array_equal(out.index_map[ax], gold[f"{name}/{key}"]), ax
    assert np.array_equal(out.attrs["freq"], gold[f"{name}/out_freq"]) and out.attrs["tag"] == "wd"
    assert len(out.index_map["baseline"]) == spec.shape[0]
    for attr in ("window_los", "window_los_lower_freq", "window_los_upper_freq"):
        want = gold[f"{name}/attr_{attr}"]
        got = out.attrs[attr]
        assert (got is None and np.isnan(want)) or got == want.item(), attr


def test_apply_entry_point_complex128(gold):
    """The entry point on a complex128 operator (the container stores complex64): against the long-double truth formed from
    that operator, within twice the error of the float64 NumPy form of the same sums."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    c = case(gold, "G33")
    op128, _ = built(gold, "G33")
    npol, n, nra, nel = c["w"].shape
    nd = op128.shape[3]
    ctx = Context.get()
    op_d, m_d, w_d = (ctx.to_device(np.array(a)) for a in (op128, c["map"][0], c["w"]))  # (copies: op128 is read-only)
    spec, sw = ctx.empty((npol * nel, nra, nd), np.complex128), ctx.empty((npol * nel, nra, nd), np.float32)
    _lib.check(_lib.lib.dmm_wienerdelay_apply(ctx.handle, npol, n, nra, nel, nd, ptr(op_d), _lib.DMM_C128, ptr(m_d), ptr(w_d), ptr(spec), ptr(sw)))
    t_spec, t_w = twin.apply(op128, c["map"][0], c["w"], ld=True)
    f_spec, f_w = twin.apply(op128, c["map"][0], c["w"], ld=False)
    e_f64 = twin.rel_err(f_spec, t_spec.astype(np.complex128))
    e_gpu = twin.rel_err(spec.cpu().numpy(), t_spec.astype(np.complex128))
    e_w = twin.rel_err(sw.cpu().numpy(), t_w.astype(np.float32))
    print(f"wienerdelay apply complex128 G33: e_gpu {e_gpu:.3e} float64 NumPy {e_f64:.3e}; weight to the truth {e_w:.3e}")
    assert e_gpu <= max(2 * e_f64, FLOOR)
    assert e_w <= 2.0**-23


def test_apply_unweighted_channels(gold):
    """A channel with weight 0 contributes nothing to the variance, whatever the operator holds there; with the map zero
    there too the spectrum does not change either."""
    from draco_amd.analysis import powerspec as ps

    c = case(gold, "G6E")
    w = c["w"].copy()
    w[:, 3] = 0.0
    m = c["map"].copy()
    m[:, :, 3] = 0.0
    rm = ring_map(dict(c, w=w, map=m))
    out = ps.ApplyWienerDelayTransform().process(rm, operator_of(gold, "G6E", rm))
    op = gold["G6E/ref64"].copy()
    op[..., 3] = 0.0
    t_spec, t_w = twin.apply(op, m[0], w, ld=True)
    assert twin.rel_err(out.spectrum[:], t_spec.astype(np.complex128)) <= FLOOR
    assert twin.rel_err(out.weight[:], t_w.astype(np.float32)) <= 2.0**-23


# ---- chain


def test_chain(gold):
    from draco_amd.analysis import powerspec as ps
    from draco_amd.core import containers
    from draco_amd.device import Context

    c = case(gold, "G33")
    npol, n, nra, nel = c["w"].shape
    el = np.sin(np.radians(0.2 * (np.arange(nel) - nel / 2)))
    rm = ring_map(c, el_values=el)
    op = construct(c).process(rm)
    dt = ps.ApplyWienerDelayTransform().process(rm, op)
    assert all(ds._host is None for ds in (op.filter, dt.spectrum, dt.weight))  # nothing was copied back between the tasks
    tel = type("Tel", (), {"latitude": 49.3, "lmax": 1, "mmax": 1, "frequencies": np.array([600.0])})()
    task = ps.SpatialTransformDelayMap(spatial_window="hamming")
    task.setup(tel)
    cube = task.process(dt)
    assert dt.spectrum._host is None and cube.vis.on_device
    host = containers.DelayTransform(baseline=npol * nel, sample=dt.index_map["sample"], delay=dt.index_map["delay"], attrs_from=dt)
    for ax in ("pol", "el"):
        host.create_index_map(ax, dt.index_map[ax])
    host.spectrum[:] = dt.spectrum.device(Context.get()).cpu().numpy()
    cube_h = task.process(host)
    a, b = cube.vis[:], cube_h.vis[:]
    assert a.shape == (npol, c["tau"].size, nra, nel) and np.isfinite(a.view(np.float64)).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert cube.attrs["window_los"] == "hann"
