"""Frequency-correlated noise on the GPU (`csrc/noisemodel.hip`, `ReconstructVisWeight` / `ReconstructVisFreqCov` of
`draco_amd/analysis/ringmapmaker.py`, `FreqCorrelatedNoise` of `draco_amd/synthesis/noise.py`) against a long-double
truth (`tests/noisemodel_twin.py`) and against vectors produced by executing the reference
(`tests/gen_golden_noisemodel.py` -> tests/golden/noisemodel.npz, noisemodel_noise.npz).

`freq_cov`: `e_gpu = max |gpu - truth| / max |truth| <= max(2 e_ref, 2**-51)`, at the stored positions within
`3 e_ref + 2**-51` of the reference (relative to the reference's largest modulus), and per sample Higham's backward
bound of a Cholesky factorisation plus the one product that forms C, `|L L^T - C| <= gamma_{nv+1} |L| |L^T| + u |C|`
entry by entry, which does not depend on the conditioning.  float32 datasets: within one float32 ulp of the rounded
truth and `<= 3 e_ref + 2**-22` from the reference.  The colouring: per real component `|gpu - truth| <= ulp32(truth) / 2
+ nfreq u sum |L| |z|`, on the golden integer factors (whose float64 sums are exact) and on the dense factor the device
made for N33 (whose sums round).  The reference's golden `vis` from the same seed is reproduced value for value (bit for bit but for the sign of exact zeros): with integer
factors the float64 value before the one float32 rounding is the same number on both sides.  The scaled
auto-correlations carry `noisemodel_twin.auto_allow` instead (one more float32 product).  Each test prints its
figures before it asserts.

N70 has one east-west separation, which neither the reference's `find_grid_indices` nor this package's can lay out
(there is no east-west spacing to take): its layout is the twin's and the tasks are entered at `_fill_output`.
"""

import os

import numpy as np
import pytest

import noisemodel_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = tuple(twin.CASES)
U = twin.U


@pytest.fixture(scope="module")
def gold():
    out = {}
    for name in ("noisemodel.npz", "noisemodel_noise.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            out[name] = {k: z[k] for k in z.files}
    return out


_cases = {}


def case(gold, name):
    """Inputs, layout and truths of a case, computed once and frozen."""
    if name not in _cases:
        g = gold["noisemodel.npz"]
        c = twin.case(g, name)
        spec = twin.CASES[name]
        c["lay"] = lay = twin.layout(c["tel"], c["pol"], c["ewpos"], c["nsmax"])
        win = twin.window(c["freq"], lay, spec["weight"], spec["scaled"], spec["include_auto"], c["freqmin"], c["nsmax"], truth=True)
        c["tL"], c["tw"], ok, c["tC"] = twin.masked_cholesky(c["cov"], c["weight"], twin.cov_noise_factor(win, lay), truth=True)
        assert ok.all()
        c["tss"] = twin.sidereal_weights(c["weight"], twin.weight_noise_factor(win, lay), lay, truth=True)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def hybrid_of(c, device=True, cov=None, **over):
    from draco_amd.core import containers
    from draco_amd.device import Context

    hv = containers.HybridVisStream(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], el=np.zeros(1), ra=c["nra"])
    hv.attrs.update(twin.attrs_of(c, **over))
    hv.weight[:] = c["weight"]
    hv.add_dataset("freq_cov", allocate=True)
    hv.freq_cov[:] = c["cov"] if cov is None else cov
    if device:
        ctx = Context.get()
        for ds in hv.datasets.values():
            ds.set_device(ctx.to_device(np.array(ds[:])))
    return hv


def run_task(cls, c, hv, **cfg):
    """``process`` where the telescope has an east-west spacing, else the twin's layout and ``_fill_output``."""
    task = cls(**cfg)
    task.setup(c["tel"])
    if twin.CASES[c["name"]]["ncyl"] > 1:
        return task.process(hv)
    task._parse_attrs(hv.attrs)
    freq = task._redistribute_input(hv)
    return task._fill_output(hv, task._compute_window(freq, c["lay"]), c["lay"])


_models = {}


def model_of(gold, name, workspace_mib=1024):
    from draco_amd.analysis.ringmapmaker import ReconstructVisFreqCov

    key = (name, workspace_mib)
    if key not in _models:
        c = case(gold, name)
        hv = hybrid_of(c)
        m = run_task(ReconstructVisFreqCov, c, hv, workspace_mib=workspace_mib)
        assert m.freq_cov.on_device and m.weight.on_device and m.freq_cov._host is None
        assert hv.freq_cov._host is None and hv.weight._host is None  # (the inputs were read where they lay)
        _models[key] = (m, np.array(m.freq_cov[:]), np.array(m.weight[:]))
    return _models[key]


@pytest.mark.parametrize("name", NAMES)
def test_freq_cov(gold, name):
    from draco_amd.core import containers

    c, g = case(gold, name), gold["noisemodel.npz"]
    m, L, w = model_of(gold, name)
    assert isinstance(m, containers.FreqNoiseModel) and L.dtype == np.float64 and w.dtype == np.float32
    assert np.array_equal(m.redundancy[:], g[f"{name}/redundancy"]) and m.redundancy.dtype == np.int32
    assert np.array_equal(m.index_map["ns"], c["lay"]["nspos"])
    tL, e_ref = c["tL"], float(g[f"{name}/e_ref_freq_cov"])
    e_gpu = twin.rel_err(L, tL)
    pos = g[f"{name}/pos"]
    ref = g[f"{name}/ref_freq_cov"]
    d_ref = float(np.abs(L[pos[:, 0], pos[:, 1], pos[:, 2]] - ref).max() / np.abs(ref).max())
    print(f"{name}: freq_cov e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} |gpu - ref| {d_ref:.3e}")
    assert e_gpu <= max(2 * e_ref, 2.0**-51)
    assert d_ref <= 3 * e_ref + 2.0**-51
    # exact zeros: the strict upper triangle, invalid rows and columns, the empty samples
    valid = (c["weight"] > 0).transpose(0, 2, 3, 1)
    both = valid[..., :, None] & valid[..., None, :]
    assert not L[~np.broadcast_to(np.tril(np.ones(L.shape[-2:], dtype=bool)), L.shape)].any()
    assert not L[~both].any()
    assert (~valid.any(axis=-1)).any() and (valid.sum(axis=-1) == 1).any()
    # the backward bound, sample by sample
    Ll = L.astype(twin.LD)
    nv = valid.sum(axis=-1)[..., None, None]
    gam = (nv + 1) * U / (1 - (nv + 1) * U)
    res = np.abs(np.einsum("pxtik,pxtjk->pxtij", Ll, Ll) - c["tC"])
    allow = gam * np.einsum("pxtik,pxtjk->pxtij", np.abs(Ll), np.abs(Ll)) + U * np.abs(c["tC"])
    worst = float((res / np.where(allow > 0, allow, 1)).max())
    print(f"{name}: backward residual / bound, worst {worst:.3f}")
    assert np.all(res <= allow)
    # weight = 1 / diag
    tw32 = c["tw"].astype(np.float32)
    e_w = twin.rel_err(w, tw32)
    print(f"{name}: weight e_gpu {e_w:.3e} e_ref {float(g[f'{name}/e_ref_weight']):.3e}")
    assert np.all(np.abs(w.astype(np.float64) - tw32.astype(np.float64)) <= twin.ulp32(tw32))
    assert not w[~(c["weight"] > 0)].any() and np.all(w[c["weight"] > 0] > 0)
    rw = g[f"{name}/ref_weight"]
    assert np.abs(w[pos[:, 0], :, pos[:, 1], pos[:, 2]] - rw).max() <= (3 * float(g[f"{name}/e_ref_weight"]) + 2.0**-22) * np.abs(rw).max()


@pytest.mark.parametrize("name", ("N33", "N70"))
def test_chunk_splits_are_bit_identical(gold, name):
    _, L, w = model_of(gold, name)
    _, L1, w1 = model_of(gold, name, workspace_mib=1)
    n = L.shape[-1]
    assert (1 << 20) // (8 * n * n) < L.shape[0] * L.shape[1] * L.shape[2]  # (more than one chunk)
    assert np.array_equal(L.view(np.uint64), L1.view(np.uint64)) and np.array_equal(w.view(np.uint32), w1.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_sidereal_weights(gold, name):
    from draco_amd.analysis.ringmapmaker import ReconstructVisWeight
    from draco_amd.core import containers

    c, g = case(gold, name), gold["noisemodel.npz"]
    hv = hybrid_of(c)
    ss = run_task(ReconstructVisWeight, c, hv)
    assert isinstance(ss, containers.SiderealStream) and ss.weight.on_device and hv.weight._host is None
    w = np.array(ss.weight[:])
    assert w.dtype == np.float32 and not np.array(ss.vis[:]).any() and ss.vis.dtype == np.complex64
    t32 = c["tss"].astype(np.float32)
    flag = c["lay"]["flag"]
    print(f"{name}: ss weight e_gpu {twin.rel_err(w, t32):.3e}, {int(flag.sum())} of {flag.size} stack entries take part")
    assert np.all(np.abs(w.astype(np.float64) - t32.astype(np.float64)) <= twin.ulp32(t32))
    assert not w[:, ~flag].any() and (~flag).any() and w[:, flag].any()
    ref, rpos = g[f"{name}/ref_ss_weight"], g[f"{name}/rpos"]
    assert np.abs(w[:, :, rpos] - ref).max() <= (3 * float(g[f"{name}/e_ref_ss_weight"]) + 2.0**-22) * np.abs(ref).max()


def noise_model(c, n):
    from draco_amd.core import containers

    m = containers.FreqNoiseModel(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], ns=c["lay"]["nspos"], ra=c["nra"])
    m.add_dataset("freq_cov", allocate=True)
    m.freq_cov[:], m.weight[:], m.redundancy[:] = n["L"], n["weight"], n["redundancy"]
    return m


@pytest.mark.parametrize("name", NAMES)
def test_colouring_and_same_seed(gold, name):
    from draco_amd.core import containers
    from draco_amd.synthesis.noise import FreqCorrelatedNoise

    c, g = case(gold, name), gold["noisemodel_noise.npz"]
    n = twin.noise_of(g[f"{name}/L"], c, c["lay"], int(g[f"{name}/seed"]))
    out = FreqCorrelatedNoise(seed=n["seed"], save_redundancy=True).process(noise_model(c, n))
    assert isinstance(out, containers.VisGridStream) and out.vis.on_device and out.weight.on_device and out.vis._host is None
    v, vw = np.array(out.vis[:]), np.array(out.weight[:])
    assert v.dtype == np.complex64 and vw.dtype == np.float32
    nns = n["redundancy"].shape[-1]
    z = twin.draw(n["seed"], n["L"].shape[:4] + (nns,))
    (tre, tim), tvw, bound = twin.colour(n["L"], z, n["redundancy"], n["weight"], c["pol"], truth=True)
    auto = twin.auto_rows(c["pol"], v.shape)
    worst = 0.0
    allows = []
    for got, t, b in ((v.real, tre, bound[0]), (v.imag, tim, bound[1])):
        t64 = t.astype(np.float64)
        allow = np.where(auto, twin.auto_allow(t64, b), 0.5 * twin.ulp32(t64) + b)
        err = np.abs(got.astype(twin.LD) - t).astype(np.float64)
        worst = max(worst, float((err / np.where(allow > 0, allow, 1)).max()))
        allows.append(allow)
        assert np.all(err <= allow)
    print(f"{name}: colouring error / bound, worst {worst:.3f}; e_gpu {max(twin.rel_err(v.real, tre), twin.rel_err(v.imag, tim)):.3e} e_ref {float(g[f'{name}/e_ref_vis']):.3e}")
    # exact properties
    assert np.array_equal(vw.view(np.uint32), (n["weight"].astype(np.float64)[:, :, :, None, :] * n["redundancy"][:, None, :, :, None]).astype(np.float32).view(np.uint32))
    assert np.array_equal(out.redundancy[:], np.broadcast_to(n["redundancy"][..., None], out.redundancy.shape))
    half = nns // 2
    for pi, po in enumerate(twin.pconjmap(c["pol"])):
        for k in range(1, half + 1):
            assert np.array_equal(v[po, :, 0, nns - k].view(np.uint32), np.conj(v[pi, :, 0, k]).view(np.uint32))
        if pi == po:
            assert not v[pi, :, 0, 0].imag.any() and v[pi, :, 0, 0].real.any()
    # the reference's realisation from the same seed.  The golden factors are bands of small integers and z is float32,
    # so every product and partial sum is exact in float64 in any order, inv_sqrt_red is the reference's own float64
    # expression, and the value that is rounded once to float32 is the same number on both sides: bit equality.
    rpos, ref = g[f"{name}/rpos"], g[f"{name}/ref_vis"]
    got32, ref32 = np.ascontiguousarray(v[..., rpos]).view(np.float32), np.ascontiguousarray(ref).view(np.float32)
    differ = got32.view(np.uint32) != ref32.view(np.uint32)
    print(f"{name}: {int(differ.sum())} of {ref32.size} components differ in their bits from the reference's realisation, all of them zeros of the other sign: {not ref32[differ].any()}")
    for got, r, allow in ((v.real, ref.real, allows[0]), (v.imag, ref.imag, allows[1])):
        assert np.all(np.abs(got[..., rpos].astype(np.float64) - r) <= allow[..., rpos])
    # (the reference's complex matmul leaves -0 in some components whose sum is an exact zero; zeros compare equal)
    assert np.array_equal(got32, ref32) and not ref32[differ].any() and not got32[differ].any()


def test_colouring_with_sums_that_round(gold):
    """The factor ReconstructVisFreqCov made for N33 (dense, irrational entries) coloured with a seeded draw: here the
    float64 sums round, and the ``nfreq u sum |L| |z|`` term of the bound is what allows it."""
    from draco_amd.synthesis.noise import FreqCorrelatedNoise

    c = case(gold, "N33")
    m, L, w = model_of(gold, "N33")
    red = np.array(m.redundancy[:])
    out = FreqCorrelatedNoise(seed=4033).process(m)
    v, vw = np.array(out.vis[:]), np.array(out.weight[:])
    nns = red.shape[-1]
    z = twin.draw(4033, L.shape[:4] + (nns,))
    (tre, tim), tvw, bound = twin.colour(L, z, red, w, c["pol"], truth=True)
    auto = twin.auto_rows(c["pol"], v.shape)
    worst, share = 0.0, 0.0
    for got, t, b in ((v.real, tre, bound[0]), (v.imag, tim, bound[1])):
        t64 = t.astype(np.float64)
        half = 0.5 * twin.ulp32(t64)
        allow = np.where(auto, twin.auto_allow(t64, b), half + b)
        err = np.abs(got.astype(twin.LD) - t).astype(np.float64)
        worst = max(worst, float((err / np.where(allow > 0, allow, 1)).max()))
        big = np.abs(t64) >= 2.0**-6  # (away from zero, where half an ulp is not tiny itself)
        share = max(share, float((b[big] / half[big]).max()))
        assert np.all(err <= allow)
    print(f"N33 device factor: colouring error / bound, worst {worst:.3f}; the float64 term is at most {share:.2e} of half a float32 ulp where |truth| >= 1/64")
    assert np.count_nonzero(L) > L.size // 4 and not np.array_equal(L, np.rint(L))
    assert np.array_equal(vw, (w.astype(np.float64)[:, :, :, None, :] * red[:, None, :, :, None]).astype(np.float32))
    # the f64 form of the twin (another summation order) agrees but for roundings that straddle a float32 tie
    v64, _, _ = twin.colour(L, z, red, w, c["pol"])
    print(f"N33 device factor: {int((v64 != v).sum())} of {v.size} values differ from the twin's float64 form")


def test_colouring_of_integers_is_exact():
    """Dense integer L, z in multiples of 1/8: every product and sum is exact in float64, so the kernel equals NumPy's
    matmul bit for bit whatever the order; shapes cross every tile edge (16 RA, 16 rows, 8 k, 32 real columns)."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    rng = np.random.default_rng(37)
    npol, new, nra, n, nns = 2, 2, 21, 37, 19
    L = np.tril(rng.integers(-3, 4, size=(npol, new, nra, n, n))).astype(np.float64)
    red = rng.integers(0, 7, size=(npol, new, nns)).astype(np.int32)
    isr = twin.inz(np.sqrt(red))
    w = rng.uniform(0.5, 1.5, size=(npol, n, new, nra)).astype(np.float32)
    ctx = Context.get()
    dev = [ctx.to_device(a) for a in (L, w, red, isr)]
    vis = ctx.zeros((npol, n, new, nns, nra), np.complex64)
    vw = ctx.zeros((npol, n, new, nns, nra), np.float32)
    want = np.zeros((npol, n, new, nns, nra), dtype=np.complex64)
    for p in range(npol):
        for x in range(new):
            z = ((rng.integers(-16, 17, size=(nra, n, nns)) + 1j * rng.integers(-16, 17, size=(nra, n, nns))) / 8).astype(np.complex64)
            zd = ctx.to_device(z)
            _lib.check(_lib.lib.dmm_noise_colour(ctx.handle, npol, n, new, nns, nra, p, x, ptr(dev[0]), ptr(zd), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(vis), ptr(vw)))
            ctx.sync()
            want[p, :, x] = (np.matmul(L[p, x], z) * isr[p, x]).transpose(1, 2, 0)
    got = vis.cpu().numpy()
    assert np.array_equal(got, want) and np.abs(want).max() > 10
    assert np.array_equal(vw.cpu().numpy(), (w[:, :, :, None, :] * red[:, None, :, :, None]).astype(np.float32))


def test_errors(gold):
    from draco_amd.analysis.ringmapmaker import ReconstructVisFreqCov, ReconstructVisWeight
    from draco_amd.synthesis.noise import FreqCorrelatedNoise

    c = case(gold, "N6")
    cov = c["cov"].copy()
    cov[0, 3, 3, 1, 9] = -1.0  # (pol 0, ew 1, ra 9) is not positive definite
    cov[0, 1, 1, 1, 12] = -2.0  # and a later one: the first in the reference's loop order is named
    with pytest.raises(np.linalg.LinAlgError, match=r"\(pol, ew, ra\) = \(0, 1, 9\)"):
        run_task(ReconstructVisFreqCov, c, hybrid_of(c, cov=cov))
    for cls in (ReconstructVisFreqCov, ReconstructVisWeight):
        with pytest.raises(ValueError, match="inverse_variance"):
            run_task(cls, c, hybrid_of(c, weight="inverse_variance"))
        hv = hybrid_of(c)
        hv.index_map["ew"] = hv.index_map["ew"] + 1.0
        with pytest.raises(RuntimeError, match="Downselected ew axis"):
            run_task(cls, c, hv)
    hv = hybrid_of(c)
    hv.datasets["complex_freq_cov"] = hv.datasets["freq_cov"]
    with pytest.raises(NotImplementedError):
        run_task(ReconstructVisFreqCov, c, hv)
    g = gold["noisemodel_noise.npz"]
    n = twin.noise_of(g["N6/L"], c, c["lay"], 1)
    m = noise_model(c, n)
    with pytest.raises(NotImplementedError):
        m.add_dataset("complex_freq_cov")
    m.datasets["complex_freq_cov"] = m.datasets["freq_cov"]
    with pytest.raises(NotImplementedError):
        FreqCorrelatedNoise(seed=1).process(m)
    from draco_amd.core import containers

    even = containers.FreqNoiseModel(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], ns=4, ra=c["nra"])
    even.add_dataset("freq_cov", allocate=True)
    with pytest.raises(ValueError, match="odd"):
        FreqCorrelatedNoise(seed=1).process(even)


# ---- the chain on the device
def _telescope_stream(nfreq=12, nra=40, seed=11):
    from draco_amd.core import containers
    from draco_amd.core.products import TransitTelescope

    rng = np.random.default_rng(seed)
    freq = 600.0 + twin.DF * np.arange(nfreq)
    tel = TransitTelescope(freq, lmax=4, ncyl=2, nfeed_cyl=3, pair_rule="halfplane")
    ss = containers.SiderealStream(freq=freq, ra=nra, input=tel.nfeed, prod=tel.index_map_prod, stack=tel.index_map_stack, reverse_map_stack=tel.reverse_map_stack)
    ss.vis[:] = (rng.standard_normal((nfreq, tel.npairs, nra)) + 1j * rng.standard_normal((nfreq, tel.npairs, nra))).astype(np.complex64)
    w = rng.uniform(0.5, 1.5, (nfreq, tel.npairs, nra)).astype(np.float32)
    w[3, :, 5:9] = 0.0
    w[:, :, 20] = 0.0
    ss.weight[:] = w
    ss.add_dataset("input_flags")
    ss.input_flags[:] = 1.0
    return tel, ss


def test_chain_stays_on_the_device():
    """DayenuDelayFilterHybridVis (covariance kept) -> ReconstructVisFreqCov -> FreqCorrelatedNoise -> BeamformNS with
    no dataset pulled to the host in between."""
    from draco_amd.analysis.dayenu import DayenuDelayFilterHybridVis
    from draco_amd.analysis.ringmapmaker import BeamformNS, MakeVisGrid, ReconstructVisFreqCov
    from draco_amd.synthesis.noise import FreqCorrelatedNoise

    tel, ss = _telescope_stream()
    mk = MakeVisGrid()
    mk.setup(tel)
    hv = BeamformNS(npix=8, weight="natural").process(mk.process(ss))
    filt = DayenuDelayFilterHybridVis(tauw=0.2, tauc=0.0, epsilon=1e-2, calculate_cov=True)
    filt.setup()
    hv = filt.process(hv)
    assert hv.freq_cov.on_device and hv.freq_cov._host is None
    rec = ReconstructVisFreqCov()
    rec.setup(tel)
    model = rec.process(hv)
    assert hv.freq_cov._host is None and hv.weight._host is None
    assert model.freq_cov.on_device and model.freq_cov._host is None and model.weight._host is None
    assert len(model.index_map["ns"]) % 2 == 1
    grid = FreqCorrelatedNoise(seed=5, save_redundancy=True).process(model)
    assert model.freq_cov._host is None and grid.vis.on_device and grid.vis._host is None and grid.weight._host is None
    noise_hv = BeamformNS(npix=8, weight="natural").process(grid)
    assert grid.vis._host is None and noise_hv.vis.on_device and noise_hv.vis._host is None
    # the noise has the weights of the data it stands for: BeamformNS multiplies back what ReconstructVisFreqCov divided
    # out.  Both sides are float32 roundings (2**-24 each, fewer than ten of them) of one float64 quantity.  Only for
    # ew > 0: on ew = 0 the reference's window keeps the auto-correlation where BeamformNS dropped it (see below).
    a, b = np.array(noise_hv.weight[:]), np.array(hv.weight[:])
    assert np.array_equal(a == 0, b == 0) and np.isfinite(np.array(noise_hv.vis[:])).all()
    rel = np.abs(a.astype(np.float64) - b)[:, :, 1:][b[:, :, 1:] > 0] / b[:, :, 1:][b[:, :, 1:] > 0]
    print(f"chain: noise weight against data weight on ew > 0, worst relative difference {float(rel.max()):.3e}")
    assert rel.max() <= 10 * 2.0**-24


def test_weights_round_trip_through_beamform_ns():
    """BeamformNS of ReconstructVisWeight's output gives back the hybrid weights.  The tolerance is twice what the CPU
    oracle of the ring-map chain (float64 arithmetic, float32 storage) reaches on the same round trip: the device adds
    only the float32 rounding of the same sums.

    This holds for ew > 0.  On ew = 0 the reference's window (``ringmapmaker.py:1501``) zeroes the auto-correlation when
    ``include_auto`` is SET, the opposite of what ``BeamformNS`` did (``:330``), so its noise factor there counts a
    baseline the beamformer dropped (or the reverse) and the weights do not come back, in the reference, in the oracle
    and here alike; the figures of ew = 0 are printed, and the device is held to the oracle's result there."""
    from draco_amd.analysis.ringmapmaker import BeamformNS, MakeVisGrid, ReconstructVisWeight
    from draco_amd.core import containers
    from draco_amd.device import Context
    from oracle import ringmap as orm

    tel, ss = _telescope_stream(nfreq=5, nra=33, seed=12)
    mk = MakeVisGrid()
    mk.setup(tel)
    results = {}
    for weight in ("natural", "uniform"):
        hv = BeamformNS(npix=8, weight=weight).process(mk.process(ss))
        rec = ReconstructVisWeight()
        rec.setup(tel)
        ss2 = rec.process(hv)
        assert ss2.weight.on_device and hv.weight._host is None
        # (onto the telescope's own stack axis, whose entries carry the conjugation flags MakeVisGrid compares; the
        # weights go over as the device tensor they are)
        ss3 = containers.SiderealStream(axes_from=ss, attrs_from=ss2, allocate=False)
        ss3.attach("vis", ss2.vis.device(Context.get()))
        ss3.attach("vis_weight", ss2.weight.device(Context.get()))
        ss3.add_dataset("input_flags")
        ss3.input_flags[:] = 1.0
        hv2 = BeamformNS(npix=8, weight=weight).process(mk.process(ss3))
        want = np.array(hv.weight[:])
        got = np.array(hv2.weight[:])
        pos = want > 0
        assert np.array_equal(got > 0, pos) and (~pos).any()
        outer = pos.copy()
        outer[:, :, 0] = False
        e_gpu = float((np.abs(got.astype(np.float64) - want)[outer] / want[outer]).max())
        # the same round trip with the oracle, from the twin's float32 sidereal weights
        lay = rec._compute_layout(hv)
        rec._parse_attrs(hv.attrs)
        nf = twin.weight_noise_factor(rec._compute_window(np.asarray(hv.freq), lay), lay)
        w2 = twin.sidereal_weights(want, nf, lay)
        pairs = np.stack([tel.prodstack["input_a"].astype(int), tel.prodstack["input_b"].astype(int)], axis=1)
        prod = [(int(a), int(b)) for a, b in tel.index_map_prod]
        flags = np.ones((tel.nfeed, w2.shape[-1]), dtype=np.float32)
        gv, gw, gr, _, _, ns = orm.make_vis_grid(np.zeros(w2.shape, np.complex64), w2, pairs, tel.polarisation, tel.baselines, flags, prod, tel.reverse_map_stack["stack"])
        _, ohw, _, _, _ = orm.beamform_ns(gv, gw, gr, ns, np.asarray(hv.freq), npix=8, weight=weight)
        assert np.array_equal(ohw > 0, pos)
        e_cpu = float((np.abs(ohw.astype(np.float64) - want)[outer] / want[outer]).max())
        inner = pos & ~outer
        e0_ref = float((np.abs(ohw.astype(np.float64) - want)[inner] / want[inner]).max())
        e0_dev = float((np.abs(got.astype(np.float64) - ohw)[inner] / ohw[inner]).max())
        results[weight] = (e_gpu, e_cpu, e0_dev)
        print(f"round trip {weight}: ew > 0 e_gpu {e_gpu:.3e} e_cpu {e_cpu:.3e}; ew = 0 oracle against input {e0_ref:.3e}, device against oracle {e0_dev:.3e}")
    for weight, (e_gpu, e_cpu, e0_dev) in results.items():
        assert e_gpu <= 2 * e_cpu, weight
        assert e0_dev <= 2 * e_cpu, weight
