"""The a_lm of the map-making path without its structural zeros (context option ``dirty_nofill``).

``dmm_dirty_run_multi`` writes ``alm[f, pol, m, l]`` for ``l >= m`` and zeros for ``l < m`` (``mapmaker.py:76``).  In
``BaseMapMaker.process_many`` the a_lm never leaves the library: ``dmm_alm2map`` reads it and it is dropped, and every
form of the Legendre synthesis loads ``l >= m`` alone -- so that path skips the fill, half the a_lm's bytes.  Checked
here, on shapes whose ``m`` fall on and off the MFMA's K chunks (``lmax = 9, 21``), with a ragged frequency group
(5 of ``kSynF = 4``), both storage types of B and the one- and two-day kernels:

* with the a_lm buffer poisoned with NaN before the no-fill launch, the maps of ``dmm_alm2map`` (first MFMA form, as
  the map-makers run it) equal those of the zero-filled path BIT FOR BIT and hold no NaN; the ``l >= m`` entries are
  the filled path's, the ``l < m`` ones were not touched;
* ``make_alm`` (the public a_lm) still returns exact zeros at ``l < m``;
* ``process_many`` with every ``torch.empty`` block poisoned gives the maps of the whole-a_lm path.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import synth as osyn

NFREQ, NPAIRS = 5, 3
SHAPES = [(9, 4), (9, 8), (21, 4), (21, 8)]  # (lmax = mmax, nside)


def _setup(lmax, b_dtype):
    from draco_amd import _lib
    from draco_amd.analysis._solve import Slab
    from draco_amd.core.products import SyntheticProvider, TransitTelescope
    from draco_amd.device import Context

    ctx = Context.get()
    tel = TransitTelescope(osyn.frequencies(NFREQ), lmax=lmax, npairs=NPAIRS)
    assert tel.npairs == NPAIRS and tel.mmax == lmax
    bt = SyntheticProvider(tel, seed=29)
    ms = np.tile(np.arange(lmax + 1, dtype=np.int32), NFREQ)
    fs = np.repeat(np.arange(NFREQ, dtype=np.int32), lmax + 1)
    dt = {"complex128": _lib.DMM_C128, "complex64": _lib.DMM_C64}[b_dtype]
    return ctx, tel, bt, Slab(ctx, bt, ms, fs, fs, dt, _lib.DMM_B_PACKED, NFREQ, lmax + 1)


def _dirty(ctx, slab, mv, mw, alms, nofill):
    from draco_amd import _lib
    from draco_amd.device import ptr

    PA = C.c_void_p * len(alms)
    with ctx.options(dirty_nofill=int(nofill)):
        _lib.check(_lib.lib.dmm_dirty_run_multi(slab.plan, ptr(slab.pool), PA(*[ptr(x) for x in mv]), PA(*[ptr(x) for x in mw]),
                                                PA(*[ptr(x) for x in alms]), len(alms)))


def _alm2map(ctx, alm, lmax, nside):
    import torch

    from draco_amd import _lib
    from draco_amd.device import ptr

    maps = torch.empty((NFREQ, 4, 12 * nside**2), dtype=torch.float64, device=ctx.device)
    with ctx.options(sht_synth_form=1):
        _lib.check(_lib.lib.dmm_alm2map(ctx.handle, ptr(alm), NFREQ, 4, lmax, lmax, nside, ptr(maps)))
    return maps


@pytest.mark.parametrize("ND", [1, 2])
@pytest.mark.parametrize("b_dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("lmax,nside", SHAPES)
def test_nan_below_m_never_reaches_a_map(lmax, nside, b_dtype, ND):
    import torch

    ctx, tel, bt, slab = _setup(lmax, b_dtype)
    gen = torch.Generator(device=ctx.device).manual_seed(7)
    shape = (lmax + 1, 2, NFREQ, NPAIRS)
    mv = [torch.randn(shape, dtype=torch.complex128, device=ctx.device, generator=gen) for _ in range(ND)]
    mw = [torch.rand(shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(ND)]
    ashape = (NFREQ, 4, lmax + 1, lmax + 1)
    filled = [torch.full(ashape, complex(float("nan"), float("nan")), dtype=torch.complex128, device=ctx.device) for _ in range(ND)]
    bare = [x.clone() for x in filled]
    _dirty(ctx, slab, mv, mw, filled, nofill=False)
    _dirty(ctx, slab, mv, mw, bare, nofill=True)
    below = torch.tril(torch.ones((lmax + 1, lmax + 1), dtype=torch.bool, device=ctx.device), diagonal=-1)  # [m, l]: l < m
    for d in range(ND):
        assert not torch.isnan(torch.view_as_real(filled[d])).any()
        assert (filled[d][:, :, below] == 0).all()
        assert torch.isnan(torch.view_as_real(bare[d][:, :, below])).all()  # the option did skip the fill
        assert torch.equal(bare[d][:, :, ~below], filled[d][:, :, ~below])
        want = _alm2map(ctx, filled[d], lmax, nside)
        got = _alm2map(ctx, bare[d], lmax, nside)
        assert not torch.isnan(got).any()
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))  # bit for bit
    slab.close()


def _day(tel, lmax, seed):
    from draco_amd.core import containers

    shape = (lmax + 1, 2, NFREQ, NPAIRS)
    rng = np.random.default_rng(seed)
    mm = containers.MModes(mmax=lmax, freq=tel.frequencies, stack=tel.npairs)
    mm.vis[:] = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    mm.weight[:] = rng.uniform(0.5, 1.5, shape)
    return mm


def _poisoned_empty(monkeypatch):
    """Every floating-point ``torch.empty`` block comes back full of NaN (what recycled memory may hold)."""
    import torch

    real_empty = torch.empty

    def empty(*args, **kw):
        t = real_empty(*args, **kw)
        if t.is_floating_point() or t.is_complex():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", empty)


@pytest.mark.parametrize("b_dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("lmax,nside", SHAPES)
def test_public_alm_keeps_its_zeros_and_the_day_its_maps(lmax, nside, b_dtype, monkeypatch):
    from draco_amd.analysis.mapmaker import DirtyMapMaker
    from draco_amd.core.products import SyntheticProvider, TransitTelescope

    tel = TransitTelescope(osyn.frequencies(NFREQ), lmax=lmax, npairs=NPAIRS)
    bt = SyntheticProvider(tel, seed=29)
    days = [_day(tel, lmax, 40 + d) for d in range(2)]
    t = DirtyMapMaker(nside=nside, b_dtype=b_dtype)
    t.setup(bt)
    _poisoned_empty(monkeypatch)
    below = np.tril(np.ones((lmax + 1, lmax + 1), dtype=bool), k=-1)  # [m, l]: l < m
    for alm in [t.make_alm(days[0])] + t.make_alm_many(days):
        a = alm.cpu().numpy()
        assert not np.isnan(a).any()
        assert (a[:, :, below] == 0).all()
    whole = [np.asarray(t._process_whole(mm).map[:]) for mm in days]  # the public a_lm, transformed whole
    for got in (t.process_many(days), [t.process(mm) for mm in days]):
        for d in range(2):
            g = np.asarray(got[d].map[:])
            assert not np.isnan(g).any()
            np.testing.assert_array_equal(g.view(np.int64), whole[d].view(np.int64))
