"""The four producers of the ring-map chain in ``csrc/beamform.hip`` (``dmm_calc_redundancy``, ``dmm_vis_grid``,
``dmm_beamform_ns``, ``dmm_beamform_ew``), each addressed directly through its entry point, against the long-double truth
of ``tests/ringchain_twin.py``.

Measures (``ringchain_twin.py`` derives them).  Grid stage: bit for bit.  NS ``hv`` / dirty beam (float32 stores): ``|got -
T| <= 2**-24 |T| + B``, ``B = (ny + 4 + a_max) 2**-52 S``, and ``got == float32(T)`` wherever ``T`` is at least ``B`` from a
float32 rounding boundary (``mismatch``: how many such elements differ; ``excluded``: the share nearer than that, at most
1e-3); ``hw`` to ``2**-24 + (2 ny + 8) 2**-52`` relative.  EW ``map`` / dirty beam: ``|got - T| <= (2 nx + 8) 2**-52 A``;
``weight``, ``rms`` to ``(nx + 8) 2**-52`` relative.  Zeros of the truth are exact zeros; every output buffer is NaN before
the call.  Each test prints ``error / bound`` (at most 1 passes) before it asserts.

Measured on an MI355X, ``error / bound`` per case (the float64 restatements' figures: ``test_ringchain_twin_host.py``).
The ``hv`` / ``hb`` / ``hw`` ratios approach 1 wherever an element's float32 rounding happens to be nearly half a unit:
that is the bound's first term, and the rounded-once comparison is the sharper of the two.  BeamformNS (``-``: the case
has no dirty beam); in every case the kernels' stores are the truth rounded once at every element compared, so the
ratios are those of the float64 restatement to the digits shown:

    case   hv      hb      hw      mismatch   excluded
    A      0       0       0       0          0
    B      0.999   -       0.973   0          4.7e-5
    C      0.995   0.990   0.934   0          0
    D      0.992   0.988   0.956   0          0
    E      0.928   -       0.834   0          0
    F      0.988   -       0.917   0          6.0e-5
    G      0.997   0.993   0.999   0          0
    Z      0       0       0       0          0

Case B again after a call that left NaN in the whole weighted-visibility scratch: the same figures.  BeamformEW
(nbeam9 and nbeam15 run ``k_bf_ew<*, 16>``, nbeam9 and the task its dirty-beam form too):

    case      map     dirty   weight  rms
    nbeam1    0       -       0       0.006
    nbeam3    0.102   0.100   0.075   0.053
    nbeam7    0.078   -       0.086   0.072
    nbeam9    0.072   0.094   0.115   0.077
    nbeam15   0.038   -       0.064   0.054
    single8   0       -       0.081   0.063
    single3   0.022   0.028   0.118   0.069
    task      0.062   0.087   0.119   0.063     (BeamformEW on five cylinders, nine beams)

The grid stage is bit for bit at every shape, the two that take a second trip of the grid-stride loops included.  The
whole file takes 2.8 s, 1.9 s of it the first call's start-up; no other case takes more than 0.35 s.
"""

import ctypes as C
import time

import numpy as np
import pytest

import ringchain_twin as rt

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _file_time():
    yield
    print(f"ringchain direct: the file took {time.perf_counter() - T0:.1f} s")


def _nan(ctx, shape, dtype):
    import torch

    t = ctx.empty(shape, dtype)
    t.fill_(complex(np.nan, np.nan) if t.is_complex() else (np.nan if t.is_floating_point() else -(2**31) + 1))
    torch.cuda.synchronize()
    return t


# ---- the grid stage
def _redundancy(nprod, nra, all_good):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    flags, pa, pb, stack = rt.redundancy_case(nprod, nra, all_good)
    red = _nan(ctx, (rt.GRID_NSTACK, nra), np.float32)
    dev = [ctx.to_device(a) for a in (flags, pa, pb, stack)]
    _lib.check(_lib.lib.dmm_calc_redundancy(ctx.handle, ptr(dev[0]), rt.GRID_NINPUT, nra, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), nprod, rt.GRID_NSTACK,
                                            all_good, ptr(red)))
    ctx.sync()
    want = rt.redundancy_exact(flags, pa, pb, stack, rt.GRID_NSTACK, all_good)
    got = red.cpu().numpy()
    assert want.any() and np.array_equal(got, want)


@pytest.mark.parametrize("shape", rt.GRID_SWEEP["redundancy"], ids=lambda s: "x".join(map(str, s)))
def test_redundancy(shape):
    _redundancy(*shape)


def test_redundancy_second_trip():
    """More (product, ra) pairs than one pass of the grid-stride loop takes."""
    _redundancy(*rt.GRID_SWEEP["redundancy_large"])


def _vis_grid(nfreq, nra, with_red):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    npol, ncp = rt.GRID_NPOL, rt.GRID_NCELL_POL
    vis, weight, red, src, conj = rt.vis_grid_case(nfreq, nra)
    gv = _nan(ctx, (npol, nfreq, ncp, nra), np.complex64)
    gw = _nan(ctx, (npol, nfreq, ncp, nra), np.float32)
    gr = _nan(ctx, (npol, ncp, nra), np.int32) if with_red else None
    dev = [ctx.to_device(a) for a in (vis, weight, red, src, conj)]
    _lib.check(_lib.lib.dmm_vis_grid(ctx.handle, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]) if with_red else None, nfreq, rt.GRID_NSTACK, nra, npol, ncp,
                                     ptr(dev[3]), ptr(dev[4]), ptr(gv), ptr(gw), ptr(gr)))
    ctx.sync()
    tv, tw, tr = rt.vis_grid_exact(vis, weight, red if with_red else None, src, conj, npol, ncp)
    got_v, got_w = gv.cpu().numpy(), gw.cpu().numpy()
    assert np.array_equal(got_v.view(np.float32), tv.view(np.float32)) and np.array_equal(got_w, tw)
    if with_red:
        assert tr.any() and np.array_equal(gr.cpu().numpy(), tr)


@pytest.mark.parametrize("shape", rt.GRID_SWEEP["vis_grid"], ids=lambda s: "x".join(map(str, s)))
def test_vis_grid(shape):
    _vis_grid(*shape)


def test_vis_grid_second_trip():
    """More grid elements than one pass of the grid-stride loop takes."""
    _vis_grid(*rt.GRID_SWEEP["vis_grid_large"])


# ---- BeamformNS
def _beamform_ns(case, gv=None):
    """``dmm_beamform_ns`` on the inputs of ``case`` (``gv``: other visibilities of the same shape): ``(hv, hw, hb)``."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    c = case
    gv_d = ctx.to_device(c.gv if gv is None else gv)
    gw_d, gr_d = ctx.to_device(c.gw), ctx.to_device(c.gr)
    tab_d = None if c.table is None else ctx.to_device(c.table)
    ns_d, el_d = ctx.to_device(c.nspos), ctx.to_device(c.el)
    hv = _nan(ctx, (c.npol, c.nfreq, c.nx, c.npix, c.nra), np.complex64)
    hw = _nan(ctx, (c.npol, c.nfreq, c.nx, c.nra), np.float32)
    hb = _nan(ctx, (c.npol, c.nfreq, c.nx, c.npix, c.nra), np.float32) if c.dirty else None
    _lib.check(_lib.lib.dmm_beamform_ns(ctx.handle, c.npol, c.nfreq, c.nx, c.ny, c.nra, c.npix, c.mode, c.include_auto, ptr(gv_d), ptr(gw_d),
                                        ptr(gr_d) if c.mode == rt.NATURAL else None, ptr(tab_d), ptr(ns_d), ptr(el_d), C.c_void_p(c.iwv.ctypes.data),
                                        ptr(hv), ptr(hw), ptr(hb)))
    ctx.sync()
    return hv.cpu().numpy(), hw.cpu().numpy(), None if hb is None else hb.cpu().numpy()


@pytest.mark.parametrize("name", list(rt.NS_SWEEP))
def test_beamform_ns_sweep(name):
    case = rt.NsCase(rt.NS_SWEEP[name])
    hv, hw, hb = _beamform_ns(case)
    case.check(name, hv, hw, hb)
    if name == "Z":
        assert not hv.any() and not hw.any() and not hb.any()


def test_beamform_ns_stale_scratch():
    """The weighted-visibility scratch of the context is reused from call to call, and the GEMM reads its padding
    without predicates: a call that left NaN all over it (an ordinary call whose visibilities are NaN, with no padding
    of its own) must not show in the next, smaller one."""
    poison = rt.NsCase(rt.NS_POISON)
    hv, _, _ = _beamform_ns(poison, gv=np.full(poison.gv.shape, complex(np.nan, np.nan), dtype=np.complex64))
    assert np.isnan(hv).all()  # (the scratch rows of every ns held NaN)
    case = rt.NsCase(rt.NS_SWEEP["B"])
    hv, hw, hb = _beamform_ns(case)
    case.check("B after a NaN call", hv, hw, hb)


# ---- BeamformEW
def _beamform_ew(c, hv, hw, hb):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    nfreq, nx, nel, nra = c.nfreq, c.nx, c.nel, c.nra
    hv_d, hw_d = ctx.to_device(hv), ctx.to_device(hw)
    hb_d = None if hb is None else ctx.to_device(hb)
    P_d, w_d = ctx.to_device(c.P), ctx.to_device(c.w)
    rmap = _nan(ctx, (c.nbeam, c.npol_out, nfreq, nra, nel), np.float64)
    weight = _nan(ctx, (c.npol_out, nfreq, nra, nel), np.float64)
    rms = _nan(ctx, (c.npol_out, nfreq, nra), np.float64)
    rdb = None if hb is None else _nan(ctx, (c.nbeam, c.npol_out, nfreq, nra, nel), np.float64)
    _lib.check(_lib.lib.dmm_beamform_ew(ctx.handle, c.npol_in, c.npol_out, nfreq, nx, nel, nra, int(c.single), ptr(hv_d), ptr(hw_d), ptr(hb_d), ptr(P_d),
                                        ptr(w_d), ptr(rmap), ptr(weight), ptr(rms), ptr(rdb)))
    ctx.sync()
    return rmap.cpu().numpy(), weight.cpu().numpy(), rms.cpu().numpy(), None if rdb is None else rdb.cpu().numpy()


@pytest.mark.parametrize("name", list(rt.EW_SWEEP))
def test_beamform_ew_sweep(name):
    c = rt.EwCase(rt.EW_SWEEP[name])
    print(f"ringchain ew {name}: nbeam {c.nbeam}, the {8 if c.nbeam <= 8 else 16}-beam kernel{' and its dirty-beam form' if c.dirty else ''}")
    c.check(name, *_beamform_ew(c, c.hv, c.hw, c.hb))


def test_beamform_ew_task_five_cylinders():
    """``BeamformEW`` on a five-cylinder telescope grid (nine beams: the 16-beam kernel through the production path),
    its inputs the hybrid stream ``BeamformNS`` made, against ``beamform_ew_ld`` on those same inputs."""
    from draco_amd.analysis.ringmapmaker import BeamformEW, BeamformNS, MakeVisGrid
    from draco_amd.core import containers
    from draco_amd.core.products import TransitTelescope

    ncyl, nfeed_cyl, nfreq, nra, npix = 5, 3, 2, 40, 9
    rng = np.random.default_rng([20261019, 5])
    freq = np.linspace(450.0, 750.0, nfreq)
    tel = TransitTelescope(freq, lmax=4, ncyl=ncyl, nfeed_cyl=nfeed_cyl, pair_rule="halfplane")
    ss = containers.SiderealStream(freq=freq, ra=nra, input=tel.nfeed, prod=tel.index_map_prod, stack=tel.index_map_stack, reverse_map_stack=tel.reverse_map_stack)
    shape = (nfreq, tel.npairs, nra)
    ss.vis[:] = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    w = rng.uniform(0.5, 1.5, shape).astype(np.float32)
    w[rng.uniform(size=shape) < 0.1] = 0
    ss.weight[:] = w
    ss.add_dataset("input_flags")
    ss.input_flags[:] = (rng.uniform(size=(tel.nfeed, nra)) > 0.1).astype(np.float32)
    mk = MakeVisGrid()
    mk.setup(tel)
    hs = BeamformNS(npix=npix, span=0.95, weight="natural", save_dirty_beam=True).process(mk.process(ss))
    rm = BeamformEW(weight_ew="natural", exclude_intracyl=True).process(hs)
    hv, hw, hb = hs.vis[:], hs.weight[:], hs.dirty_beam[:]
    assert hv.shape == (4, nfreq, ncyl, npix, nra) and rm.map.shape == (2 * ncyl - 1, 4, nfreq, nra, npix)
    pol, rot = BeamformEW._get_pol(hs.index_map["pol"])
    assert list(rm.index_map["pol"]) == list(pol)
    wew = rt.ew_weights(ncyl, "natural", True, False, None)
    P = np.ascontiguousarray(rot, dtype=np.complex128)
    T, A, rv = rt.beamform_ew_ld(hv, hw, P, wew, False)
    Tb, Ab, _ = rt.beamform_ew_ld(hb, hw, P, wew, False)
    m = rt.ew_measure(ncyl, T, A, rv, rm.map[:], rm.weight[:], rm.rms[:])
    m["dirty_beam"] = rt.ew_measure(ncyl, Tb, Ab, rv, rm.dirty_beam[:])["map"]
    print("ringchain ew task, five cylinders: " + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
    assert T.any() and rv.any()
    assert m["map"] <= 1.0 and m["dirty_beam"] <= 1.0 and m["weight"] <= 1.0 and m["rms"] <= 1.0 and m["weight_zeros"] and m["rms_zeros"], m
