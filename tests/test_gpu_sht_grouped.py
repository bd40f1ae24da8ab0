"""GPU: the frequency-grouped ring-coefficient scratch of the NPOL = 4 synthesis (groups of 4 frequencies).

Every Legendre synthesis form writes the scratch and both ring stages read it: the first MFMA form (sht_variant bit 6, the
map-makers' form), the pipelined form with one or two frequency groups per block (0 / bit 7), the vector-ALU kernel (bit 3),
each with the FFT and with the direct ring stage (bit 2).  They evaluate the same sums: 1e-12 of the map's scale apart.
Ragged groups (nf not a multiple of 4), several chunks with a ragged last one, and every Bluestein class with rings
shorter than mmax (nside 256, lmax 512) are covered; small cases are also pinned to the NumPy oracle.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import sht as osht

VARIANTS = (64, 0, 128, 8, 4 | 64, 4, 4 | 8)


def _rand_alm(rng, nfreq, lmax):
    a = np.zeros((nfreq, 4, lmax + 1, lmax + 1), dtype=np.complex128)
    for l in range(lmax + 1):
        a[:, :, l, 0] = rng.standard_normal((nfreq, 4))
        a[:, :, l, 1 : l + 1] = rng.standard_normal((nfreq, 4, l)) + 1j * rng.standard_normal((nfreq, 4, l))
    a[:, 1:3, :2] = 0
    return a


def _alm_dev(ctx, alm):
    return ctx.to_device(np.ascontiguousarray(alm.transpose(0, 1, 3, 2)), np.complex128)  # m-major


def _alm2map(ctx, a_dev, nfreq, lmax, nside, variant):
    from draco_amd import _lib
    from draco_amd.device import ptr

    out = ctx.empty((nfreq, 4, 12 * nside * nside), np.float64)
    with ctx.options(sht_variant=variant):
        _lib.check(_lib.lib.dmm_alm2map(ctx.handle, ptr(a_dev), nfreq, 4, lmax, lmax, nside, ptr(out)))
    return out.cpu().numpy()


@pytest.mark.parametrize(
    "nside,lmax,nf",
    [(8, 20, 1), (16, 40, 2), (16, 47, 3), (16, 40, 5), (64, 150, 5), (32, 100, 33), (256, 512, 2), (256, 512, 33)],
)
def test_grouped_scratch_forms_agree(nside, lmax, nf):
    from draco_amd.device import Context

    ctx = Context.get()
    rng = np.random.default_rng(1000 * nside + nf)
    alm = _rand_alm(rng, nf, lmax)
    a_dev = _alm_dev(ctx, alm)
    ref = _alm2map(ctx, a_dev, nf, lmax, nside, 64)
    scale = np.abs(ref).max()
    assert scale > 0 and np.isfinite(ref).all()
    # every frequency and polarisation carries its own field (no slot of the groups read or written twice)
    assert (np.abs(ref).max(axis=2) > 1e-3 * scale).all()
    for variant in VARIANTS[1:]:
        if variant & 8 and nside >= 256 and nf > 2:
            continue  # (the vector-ALU kernel: covered at nf = 2 of this geometry; no need to repeat it at 33)
        got = _alm2map(ctx, a_dev, nf, lmax, nside, variant)
        err = np.abs(got - ref).max() / scale
        assert err < 1e-12, (variant, err)
    if nside <= 16:
        assert np.abs(ref - osht.sphtrans_inv_sky(alm, nside)).max() < 1e-10 * scale


def test_grouped_scratch_frequencies_independent():
    """A frequency's map does not depend on the others of its group or chunk: the maps of 33 frequencies (two chunks at
    this geometry, the last one with a ragged group) equal those of the same frequencies transformed one at a time."""
    from draco_amd.device import Context

    ctx = Context.get()
    nside, lmax, nf = 256, 512, 33
    rng = np.random.default_rng(7)
    alm = _rand_alm(rng, nf, lmax)
    full = _alm2map(ctx, _alm_dev(ctx, alm), nf, lmax, nside, 64)
    for f in (0, 3, 4, 19, 20, 31, 32):
        one = _alm2map(ctx, _alm_dev(ctx, alm[f : f + 1]), 1, lmax, nside, 64)
        assert np.array_equal(one[0], full[f]), f


@pytest.mark.parametrize("nside,lmax,nf", [(16, 20, 3), (64, 64, 5)])
def test_grouped_scratch_map2alm_iterations(nside, lmax, nf):
    """map2alm with three Jacobi iterations: the residual of each iteration runs the grouped synthesis on the scratch the
    analysis uses in its own layout.  Pinned to the oracle where it is cheap, a round trip otherwise (lmax = nside: the
    iterations converge to 1e-6)."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    rng = np.random.default_rng(nside + nf)
    alm = _rand_alm(rng, nf, lmax)
    mp = _alm2map(ctx, _alm_dev(ctx, alm), nf, lmax, nside, 0)
    m_dev = ctx.to_device(mp, np.float64)
    out = ctx.empty((nf, 4, lmax + 1, lmax + 1), np.complex128)
    _lib.check(_lib.lib.dmm_map2alm(ctx.handle, ptr(m_dev), nf, 4, lmax, lmax, nside, 3, ptr(out)))
    back = out.cpu().numpy().transpose(0, 1, 3, 2)
    if nside <= 16:
        ref = osht.sphtrans_sky(mp, lmax=lmax, niter=3)
        assert np.abs(back - ref).max() < 1e-10 * np.abs(ref).max()
    else:
        assert np.abs(back - alm).max() < 1e-6 * np.abs(alm).max()
