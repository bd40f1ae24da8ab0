"""``dmm_alm2map`` / ``dmm_map2alm`` addressed directly, every form of their kernels against the long-double truth of
``tests/sht_twin.py`` (which derives the measures): per group ``ratio = rms(got - T) / max(rms(float64 restatement - T),
2**-53 rms|T|) <= 8``, per element ``|got - T| <= backstop``, exact structural zeros, every output NaN before the call
and finite after it.  Each test prints ``ratio`` and ``error / backstop`` before it asserts.

Measured on an MI355X.  ``ratio``: the largest over the polarisations, per ring group for the synthesis (``c256`` ...
``c8192``: the cap classes by FFT length; ``c8192`` runs the direct kernel), the largest over a case's groups otherwise;
``usage``: the largest ``error / backstop``.  The restatement's own usage: ``test_sht_twin_host.py``.

    synthesis    belt   c256   c512   c1024  c2048  c4096  c8192  usage
    S0a          0.40   -      -      -      -      -      -      0.008
    S0b          1.33   -      -      -      -      -      -      0.025
    S1           1.13   0.72   -      -      -      -      -      0.017
    S2a          1.10   1.32   -      -      -      -      -      0.073
    S2b          1.09   1.37   -      -      -      -      -      0.073
    S3           1.02   1.47   -      -      -      -      -      0.138
    S3 form 64   1.02   1.48   -      -      -      -      -      0.138
    S3 form 128  1.02   1.47   -      -      -      -      -      0.138
    S3 form 8    1.02   1.48   -      -      -      -      -      0.138
    S3 form 4    1.33   1.69   -      -      -      -      -      0.139
    S4           0.98   1.21   -      -      -      -      -      0.087
    S5           0.92   1.23   1.29   0.77   -      -      -      0.089
    S6           0.92   3.13   1.34   1.11   1.11   -      -      0.247
    S7           -      0.93   1.67   -      -      -      -      0.0005
    S8a          0.99   2.30   3.95   2.53   1.88   1.40   2.37   0.169
    S8b          0.96   1.60   4.26   2.18   1.45   1.32   2.17   0.114

``test_m0_imaginary_part``: S1 1.13 (FFT) and 1.52 (direct sums), S6 3.13 and 3.13 (its class 2048 at 1.11 and 1.31):
the figures of the real ``a_l0``.  ``test_stale_scratch``: the bits of a fresh context; S3 with 1, 3, 5 frequencies 2.17,
1.33, 1.48, A2 at most 1.45.

    analysis        A0     A1 (0, 1, 3 steps)   A2 (0, 2)     A3     A4     A5     A6
    ratio, MFMA     7.04   1.18   1.24   1.22   1.27   1.30   1.09   1.30   1.80   1.54
    ratio, form 8   7.05   1.16   1.25   1.22   1.26   1.30   1.09   1.30   1.80   1.54
    usage           0.034  0.019  0.004  0.002  0.013  0.002  0.019  0.070  0.029  0.020

A0 has six live entries per polarisation, for E and B three of them structural zeros: the restatement's error there is
1.4 units of ``2**-53 rms|T|``, the kernels' ten such units are 0.03 of the backstop -- three numbers, not a trend (A1
has the same kernels at 1.2).  A6 stood at
17.4 (T) and 11.6 (V) before the direct kernels restarted their phasor every 64 steps (``kDirectRun``, ``sht_rings.h``): the
cap rings 513 ... 1023 of nside 1024 take ``k_ring_anal``, whose rotation ran over all 4 ir pixels of a ring.  The same
restart took S6's class 2048 under the direct sums from 3.4 to 1.31.

The whole file takes 10 s, 2 s of it the first call's start-up and 5 s the long-double truths of S5, S6, S7, A4 and
A5 (0.7 to 1.7 s each, kernels included); no other case takes more than 0.3 s.
"""

import time

import numpy as np
import pytest

import sht_twin as st

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()
E_UNSUPPORTED = -2
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _file_time():
    yield
    _CASES.clear()
    print(f"sht direct: the file took {time.perf_counter() - T0:.1f} s")


def _case(kind, name, nf=None):
    """One truth per case for the whole file."""
    key = (name, nf)
    if key not in _CASES:
        _CASES[key] = (st.SynthCase if kind == "S" else st.AnalCase)(name, nf)
    return _CASES[key]


def _ctx(ctx=None):
    from draco_amd.device import Context

    return Context.get() if ctx is None else ctx


def _nan(ctx, shape, dtype):
    t = ctx.empty(shape, dtype)
    t.fill_(complex(np.nan, np.nan) if t.is_complex() else np.nan)
    return t


def _alm2map(c, alm=None, variant=0, ctx=None, whole=False):
    """``dmm_alm2map`` of case ``c`` (``alm``: other coefficients of its shape) into a NaN-filled map: the pixels of the
    case's rings (only those leave the device), or the whole map."""
    import torch

    from draco_amd import _lib
    from draco_amd.device import ptr

    ctx = _ctx(ctx)
    a_dev = ctx.to_device(c.alm if alm is None else alm, np.complex128)
    out = _nan(ctx, (c.nf, c.npol, 12 * c.nside * c.nside), np.float64)
    with ctx.options(sht_variant=variant):
        _lib.check(_lib.lib.dmm_alm2map(ctx.handle, ptr(a_dev), c.nf, c.npol, c.lmax, c.mmax, c.nside, ptr(out)))
    ctx.sync()
    if whole:
        return out.cpu().numpy()
    assert bool(torch.isfinite(out).all()), "the map is not finite everywhere"
    return out[:, :, torch.from_numpy(c.pix).to(out.device)].cpu().numpy()


def _map2alm(c, niter, maps=None, variant=0, ctx=None, nan_ok=False):
    """``dmm_map2alm`` of case ``c``'s map (zero off its rings) into a NaN-filled ``a_lm [nf, npol, m, l]``."""
    import torch

    from draco_amd import _lib
    from draco_amd.device import ptr

    ctx = _ctx(ctx)
    m_dev = ctx.zeros((c.nf, c.npol, 12 * c.nside * c.nside), np.float64)
    m_dev[:, :, torch.from_numpy(c.pix).to(m_dev.device)] = ctx.to_device(c.maps if maps is None else maps, np.float64)
    out = _nan(ctx, (c.nf, c.npol, c.mmax + 1, c.lmax + 1), np.complex128)
    with ctx.options(sht_variant=variant):
        _lib.check(_lib.lib.dmm_map2alm(ctx.handle, ptr(m_dev), c.nf, c.npol, c.lmax, c.mmax, c.nside, niter, ptr(out)))
    ctx.sync()
    assert nan_ok or bool(torch.isfinite(torch.view_as_real(out)).all()), "a_lm is not finite everywhere"
    return out.cpu().numpy()


def _check(label, m, t0):
    print(f"sht direct {label}: {st.fmt(m)}; {time.perf_counter() - t0:.2f} s")
    assert st.passes(m), (label, m)


# ---- synthesis
@pytest.mark.parametrize("name", list(st.SYNTH))
def test_alm2map_sweep(name):
    t0 = time.perf_counter()
    c = _case("S", name)
    _check(name, c.measure(_alm2map(c)), t0)


@pytest.mark.parametrize("variant", st.S3_VARIANTS[1:])
def test_alm2map_forms(variant):
    """Every form against the truth, not against each other: the first MFMA form (64), the pipelined kernel with one
    frequency group per block (128), the vector-ALU Legendre kernel (8), the direct ring sums (4).  Three frequency
    groups, the last ragged."""
    t0 = time.perf_counter()
    c = _case("S", "S3")
    _check(f"S3 variant {variant}", c.measure(_alm2map(c, variant=variant)), t0)


@pytest.mark.parametrize("name", ["S1", "S6"])
@pytest.mark.parametrize("variant", [0, 4])
def test_m0_imaginary_part(name, variant):
    """``Im a_l0`` at ten times the real scale (the solvers' ``B^H v`` carries one) must not reach the map: the maps are
    those of ``Re a_l0`` under the same measures.  FFT and direct ring stages; S1's rings are all shorter than the band
    limit (staged coefficients), S6's belt and outer classes are not."""
    t0 = time.perf_counter()
    c = _case("S", name)
    alm = c.alm.copy()
    alm[:, :, 0, :] = alm[:, :, 0, :].real + 10j * np.random.default_rng([st.SEED, 77]).standard_normal(alm[:, :, 0, :].shape)
    _check(f"{name} variant {variant}, Im a_l0 x 10", c.measure(_alm2map(c, alm=alm, variant=variant)), t0)


# ---- analysis
@pytest.mark.parametrize("variant", st.ANAL_VARIANTS)
@pytest.mark.parametrize("name", list(st.ANAL))
def test_map2alm_sweep(name, variant):
    """The MFMA (0) and the vector-ALU (8) Legendre analysis, each against the truth; Jacobi steps against the truth's
    own long-double iteration."""
    c = _case("A", name)
    for niter in c.niters:
        t0 = time.perf_counter()
        _check(f"{name} variant {variant} niter {niter}", c.measure(_map2alm(c, niter, variant=variant), niter), t0)


def test_map2alm_unsupported_nside_leaves_the_output_alone():
    """nside 2048 with four polarisations is more than the in-LDS ring stage takes: ``DMM_E_UNSUPPORTED``, and nothing
    is written."""
    import torch

    from draco_amd import _lib
    from draco_amd.device import ptr

    ctx = _ctx()
    nside, lmax = 2048, 8
    maps = ctx.empty((1, 4, 12 * nside * nside), np.float64)
    out = _nan(ctx, (1, 4, lmax + 1, lmax + 1), np.complex128)
    rc = _lib.lib.dmm_map2alm(ctx.handle, ptr(maps), 1, 4, lmax, lmax, nside, 0, ptr(out))
    ctx.sync()
    assert rc == E_UNSUPPORTED and bool(torch.isnan(torch.view_as_real(out)).all())


# ---- the shared scratch
def test_stale_scratch():
    """The ring-coefficient scratch of a context is shared by all its calls, and the slots of frequencies past a
    chunk's last are "never written and never read" (``sht_common.h``).  After a call with eight frequencies of NaN
    (S3's geometry; A2's, with Jacobi steps, for the analysis) has left NaN in all of them, transforms of 1, 3 and 5
    frequencies on that context give the bits of a fresh context, and pass their measures."""
    from draco_amd.device import Context

    shared = _ctx()
    fresh = Context(shared.device_index)
    big = _case("S", "S3", 8)
    nan_map = _alm2map(big, alm=np.full(big.alm.shape, complex(np.nan, np.nan)), whole=True)
    assert np.isnan(nan_map).all()
    for nf in (1, 3, 5):
        t0 = time.perf_counter()
        c = _case("S", "S3", nf)
        got = _alm2map(c)
        assert np.array_equal(got, _alm2map(c, ctx=fresh))
        _check(f"S3 nf {nf} after a NaN call", c.measure(got), t0)
    big = _case("A", "A2", 8)
    live = np.arange(big.lmax + 1)[None, :] >= np.arange(big.mmax + 1)[:, None]
    nan_alm = _map2alm(big, 2, maps=np.full(big.maps.shape, np.nan), nan_ok=True)
    assert np.isnan(nan_alm[:, (0, 3)][..., live]).all()
    for nf in (1, 3, 5):
        c = _case("A", "A2", nf)
        for niter in c.niters:
            t0 = time.perf_counter()
            got = _map2alm(c, niter)
            assert np.array_equal(got, _map2alm(c, niter, ctx=fresh))
            _check(f"A2 nf {nf} niter {niter} after a NaN call", c.measure(got, niter), t0)
