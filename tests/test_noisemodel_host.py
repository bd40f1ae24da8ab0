"""Host side of the noise model, on the CPU: the ``FreqNoiseModel`` container, the layout, window and noise factors of
``ReconstructVisNoiseBase`` against the vectors the reference produced (tests/golden/noisemodel.npz; the same NumPy
expressions, so within 4 float64 ulps), the twin's float64 forms against its own long-double truth, the multiple-
realisation mixin, and ``GaussianNoiseDataset`` against the reference's dataset from the same seed."""

import os

import numpy as np
import pytest

import noisemodel_twin as twin
from conftest import GOLDEN

NAMES = tuple(twin.CASES)
WINDOWS = [(w, s, a) for w in ("natural", "uniform", "hann") for s in (False, True) for a in (False, True)]


@pytest.fixture(scope="module")
def gold():
    out = {}
    for name in ("noisemodel.npz", "noisemodel_noise.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            out[name] = {k: z[k] for k in z.files}
    return out


def within_ulps(a, b, n):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= n * np.spacing(np.abs(b))))


def test_container():
    from draco_amd.core import containers

    m = containers.FreqNoiseModel(pol=["XX", "YY"], freq=[600.0, 601.0, 602.0], ew=2, ns=5, ra=4)
    assert m._axes == ("pol", "freq", "freq_sum", "ew", "ns", "ra")
    assert m.redundancy.shape == (2, 2, 5) and m.redundancy.dtype == np.int32
    assert m.weight.shape == (2, 3, 2, 4) and m.weight.dtype == np.float32
    assert "freq_cov" not in m
    with pytest.raises(KeyError):
        m.freq_cov
    m.add_dataset("freq_cov", allocate=True)
    assert m.freq_cov.shape == (2, 2, 4, 3, 3) and m.freq_cov.dtype == np.float64
    assert np.array_equal(m.index_map["freq_sum"], m.index_map["freq"]) and np.array_equal(m.freq, [600.0, 601.0, 602.0])
    with pytest.raises(NotImplementedError):
        m.add_dataset("complex_freq_cov")
    with pytest.raises(NotImplementedError):
        m.complex_freq_cov
    g = containers.VisGridStream(axes_from=m, attrs_from=m)
    assert g.vis.shape == (2, 3, 2, 5, 4)
    assert containers.FreqNoiseModel in containers._all_containers()


def hybrid_of(c, **over):
    from draco_amd.core import containers

    hv = containers.HybridVisStream(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], el=np.zeros(1), ra=c["nra"], allocate=False)
    hv.attrs.update(twin.attrs_of(c, **over))
    return hv


def task_of(c, cls=None, **over):
    from draco_amd.analysis import ringmapmaker as rm

    t = (cls or rm.ReconstructVisFreqCov)()
    t.setup(c["tel"])
    t._parse_attrs(twin.attrs_of(c, **over))
    return t


@pytest.mark.parametrize("name", NAMES)
def test_layout_window_and_factors(gold, name):
    from draco_amd.analysis import ringmapmaker as rm

    g = gold["noisemodel.npz"]
    c = twin.case(g, name)
    task = task_of(c)
    assert np.array_equal(task.bt_stack, c["tel"].stack) and np.array_equal(task.bt_rev["stack"], c["tel"].reverse_stack["stack"])
    if twin.CASES[name]["ncyl"] > 1:
        lay = task._compute_layout(hybrid_of(c))
        for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid"):
            assert np.array_equal(lay[k], g[f"{name}/layout_{k}"]), k
        assert within_ulps(lay["nspos"], g[f"{name}/layout_nspos"], 4) and (lay["npol"], lay["nx"], lay["ny"]) == g[f"{name}/layout_nbaseline_grid"].shape
    else:  # one east-west separation: no spacing to take, here as in the reference
        with pytest.raises(ValueError):
            task._compute_layout(hybrid_of(c))
        lay = twin.layout(c["tel"], c["pol"], c["ewpos"], c["nsmax"])
        for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid"):
            assert np.array_equal(lay[k], g[f"{name}/layout_{k}"]), k
    for wname, scaled, auto in WINDOWS:
        t2 = task_of(c, weight=wname, scaled=scaled, include_auto=auto)
        w = t2._compute_window(c["freq"], lay)
        ref = g[f"{name}/window_{wname}_{int(scaled)}_{int(auto)}"]
        assert w.shape == ref.shape and within_ulps(w, ref, 4), (wname, scaled, auto)
        assert (not w[:, :, 0, 0].any()) == auto
    window = task._compute_window(c["freq"], lay)
    assert within_ulps(rm.cov_noise_factor(window, lay), g[f"{name}/cov_noise_factor"], 4)
    assert within_ulps(rm.weight_noise_factor(window, lay), g[f"{name}/weight_noise_factor"], 4)
    # the twin's float64 forms agree with them too
    spec = twin.CASES[name]
    tw = twin.window(c["freq"], lay, spec["weight"], spec["scaled"], spec["include_auto"], c["freqmin"], c["nsmax"])
    assert within_ulps(tw, window, 4) and within_ulps(twin.cov_noise_factor(tw, lay), g[f"{name}/cov_noise_factor"], 8)


@pytest.mark.parametrize("name", tuple(twin.LAYOUT_CASES))
def test_layout_of_four_polarisations(gold, name):
    """Two cylinders and XX, XY, YX, YY: the cross-polarisation conjugate map of the intra-cylinder cells and the pair
    each stack entry is read from (the telescope's ``prodstack``), against the reference's ``_compute_layout``."""
    from draco_amd.analysis import ringmapmaker as rm

    g = gold["noisemodel.npz"]
    c = twin.layout_case(name)
    task = rm.ReconstructVisFreqCov()
    task.setup(c["tel"])
    task._parse_attrs({"beamform_ns_weight": "hann", "beamform_ns_scaled": False, "beamform_ns_include_auto": False, "beamform_ns_freqmin": c["freqmin"],
                       "beamform_ns_nsmax": c["nsmax"]})
    hv = containers_hybrid(c)
    lay = task._compute_layout(hv)
    for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid"):
        assert np.array_equal(lay[k], g[f"{name}/layout_{k}"]), k
    assert list(lay["pconjmap"]) == [0, 2, 1, 3] and lay["npol"] == 4 and (lay["nbaseline_grid"][:, 0] > 0).any()
    assert within_ulps(lay["nspos"], g[f"{name}/layout_nspos"], 4)
    assert within_ulps(task._compute_window(c["freq"], lay), g[f"{name}/window"], 4)
    # a telescope without `prodstack` is read through `uniquepairs` (the same pairs here)
    bare = type("Tel", (), {k: v for k, v in vars(c["tel"]).items() if k != "prodstack"})()
    bare.lmax = bare.mmax = 0
    bare.frequencies = np.zeros(1)
    task.setup(bare)
    lay2 = task._compute_layout(hv)
    assert all(np.array_equal(lay2[k], lay[k]) for k in ("pind", "nbaseline_grid", "flag"))


def containers_hybrid(c):
    from draco_amd.core import containers

    return containers.HybridVisStream(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], el=np.zeros(1), ra=2, allocate=False)


def test_parse_attrs_and_ew_axis(gold):
    from draco_amd.analysis import ringmapmaker as rm

    c = twin.case(gold["noisemodel.npz"], "N6")
    for cls in (rm.ReconstructVisWeight, rm.ReconstructVisFreqCov):
        assert issubclass(cls, rm.ReconstructVisNoiseBase)
        with pytest.raises(ValueError, match="inverse_variance"):
            task_of(c, cls, weight="inverse_variance")
        task = task_of(c, cls)
        assert task.wvmin == twin.C_LIGHT * 1e-6 / float(c["freqmin"])
        hv = hybrid_of(c)
        hv.index_map["ew"] = hv.index_map["ew"][:1]
        with pytest.raises(RuntimeError, match="Downselected ew axis"):
            task._compute_layout(hv)
    with pytest.raises(NotImplementedError):
        rm.ReconstructVisNoiseBase()._fill_output(None, None, None)
    assert rm.ReconstructVisFreqCov(workspace_mib=7).workspace_mib == 7


@pytest.mark.parametrize("name", NAMES)
def test_twin_forms(gold, name):
    """The float64 forms against the long-double truth: the identity embedding gives the reference's compressed factor."""
    g = gold["noisemodel.npz"]
    c = twin.case(g, name)
    lay = twin.layout(c["tel"], c["pol"], c["ewpos"], c["nsmax"])
    nf = g[f"{name}/cov_noise_factor"]
    L, w, ok, C = twin.masked_cholesky(c["cov"], c["weight"], nf)
    tL, tw, tok, _ = twin.masked_cholesky(c["cov"], c["weight"], nf.astype(twin.LD), truth=True)
    assert ok.all() and tok.all() and twin.rel_err(L, tL) <= 1e-14 and np.array_equal(w == 0, ~(c["weight"] > 0))
    pos = g[f"{name}/pos"]
    ref = g[f"{name}/ref_freq_cov"]
    Cn = twin.normalised_cov(c["cov"], nf)
    for i, (p, x, t) in enumerate(pos):
        lit = twin.compressed_cholesky(Cn[p, x, t], c["weight"][p, :, x, t] > 0)
        assert np.array_equal(lit, ref[i])  # (the reference's own loop body on its own inputs)
        assert np.abs(L[p, x, t] - lit).max() <= 1e-14 * np.abs(lit).max() if lit.any() else not L[p, x, t].any()
    assert np.array_equal(w[pos[:, 0], :, pos[:, 1], pos[:, 2]], g[f"{name}/ref_weight"])
    tss = twin.sidereal_weights(c["weight"], g[f"{name}/weight_noise_factor"], lay)
    assert np.abs(tss[:, :, g[f"{name}/rpos"]].astype(np.float64) - g[f"{name}/ref_ss_weight"]).max() <= 2.0**-23 * np.abs(tss).max()
    # the colouring: the float64 form is within the bound of the truth
    gn = gold["noisemodel_noise.npz"]
    n = twin.noise_of(gn[f"{name}/L"], c, lay, int(gn[f"{name}/seed"]))
    z = twin.draw(n["seed"], n["L"].shape[:4] + (n["redundancy"].shape[-1],))
    v, vw, _ = twin.colour(n["L"], z, n["redundancy"], n["weight"], c["pol"])
    (tre, tim), tvw, bound = twin.colour(n["L"], z, n["redundancy"], n["weight"], c["pol"], truth=True)
    auto = twin.auto_rows(c["pol"], v.shape)
    for got, t, b in ((v.real, tre, bound[0]), (v.imag, tim, bound[1])):
        t64 = t.astype(np.float64)
        allow = np.where(auto, twin.auto_allow(t64, b), 0.5 * twin.ulp32(t64) + b)
        assert np.all(np.abs(got.astype(twin.LD) - t) <= allow)
    assert np.array_equal(vw, tvw.astype(np.float32))
    rpos = gn[f"{name}/rpos"]
    assert np.abs(v[..., rpos] - gn[f"{name}/ref_vis"]).max() <= 2.0**-22 * np.abs(v).max()


def _stream(gold):
    from draco_amd.core import containers

    g = gold["noisemodel_noise.npz"]
    c = twin.case(gold["noisemodel.npz"], "N6")
    tel = c["tel"]
    ss = containers.SiderealStream(freq=c["freq"], ra=c["nra"], input=tel.nfeed, prod=tel.prod, stack=tel.stack, reverse_map_stack=tel.reverse_stack)
    ss.weight[:] = g["N6/gaussian_weight"]
    return ss, g


def test_gaussian_noise_dataset(gold):
    from draco_amd.synthesis.noise import GaussianNoiseDataset

    ss, g = _stream(gold)
    task = GaussianNoiseDataset(seed=int(g["N6/gaussian_seed"]))
    assert task.dataset is None and task.in_place is True
    out = task.process(ss)
    assert out is ss
    v, ref = np.array(ss.vis[:]), g["N6/gaussian_vis"]
    assert v.dtype == np.complex64
    for a, b in ((v.real, ref.real), (v.imag, ref.imag)):
        assert np.all(np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b)))
    autos = ss.prodstack["input_a"] == ss.prodstack["input_b"]
    assert autos.sum() == 2 and not v[:, autos].imag.any() and v[:, ~autos].imag.any()
    assert not v[ss.weight[:] == 0].any()
    # a copy on request, another dataset by name, and the errors
    ss2, _ = _stream(gold)
    out2 = GaussianNoiseDataset(seed=int(g["N6/gaussian_seed"]), in_place=False, dataset="vis").process(ss2)
    assert out2 is not ss2 and not ss2.vis[:].any() and np.array_equal(out2.vis[:], v)
    from draco_amd.core.task import CaputConfigError

    with pytest.raises(CaputConfigError, match="does not exist"):
        GaussianNoiseDataset(dataset="nope").process(ss2)
    with pytest.raises(ValueError, match="No default dataset"):
        GaussianNoiseDataset().process(type("Bare", (), {"datasets": {}})())


def test_gaussian_noise_default_datasets():
    """Without ``dataset`` every container with a data / weight pair has its data dataset filled; a real one gets real
    noise of variance ``1 / weight`` from ``standard_normal``, zero where the weight is zero."""
    from draco_amd.core import containers
    from draco_amd.synthesis import noise

    rm = containers.RingMap(beam=1, pol=["XX"], freq=[600.0, 601.0], ra=6, el=np.linspace(-0.5, 0.5, 3))
    w = np.full(rm.weight.shape, 4.0)
    w[0, 1, 2] = 0.0
    rm.weight[:] = w
    out = noise.GaussianNoiseDataset(seed=3).process(rm)
    want = np.random.default_rng(3).standard_normal(rm.map.shape) * np.where(w > 0, 0.5, 0.0)
    assert out is rm and np.array_equal(rm.map[:], want) and rm.map[:].any()
    for cls, name in noise._DATA_DSET:
        assert name in ("vis", "map", "beam", "stack") and hasattr(cls, "weight")
    assert noise._default_dataset(rm) == "map"
    assert noise._default_dataset(containers.SiderealStream(freq=[600.0], ra=2, stack=1)) == "vis"
    for cls, name in ((containers.FormedBeam, "beam"), (containers.GridBeam, "beam"), (containers.FrequencyStack, "stack"), (containers.Stack3D, "stack")):
        assert noise._default_dataset(cls.__new__(cls)) == name


def test_multiple_realisations(gold):
    from draco_amd.core.task import PipelineStopIteration
    from draco_amd.synthesis import noise

    a, g = _stream(gold)
    b, _ = _stream(gold)
    b.weight[:] = 4.0 * b.weight[:]
    task = noise.MultipleGaussianNoiseDatasets(niter=3, seed=9)
    assert isinstance(task, noise.MultipleNoiseRealizationsMixin) and task.in_place is False
    task.setup(a, b)
    outs = [task.process() for _ in range(3)]
    with pytest.raises(PipelineStopIteration):
        task.process()
    assert not a.vis[:].any() and not b.vis[:].any()  # (copies: the inputs are kept for the next realisation)
    for out, src in zip(outs, (a, b, a)):
        assert np.array_equal(out.weight[:], src.weight[:]) and out.vis[:].any()
    assert not np.array_equal(outs[0].vis[:], outs[2].vis[:])
    # one input: every realisation comes from it; a second setup starts the count again
    task.setup(a)
    assert np.array_equal(task.process().weight[:], a.weight[:]) and task._count == 1
    assert issubclass(noise.MultipleFreqCorrelatedNoise, noise.MultipleNoiseRealizationsMixin) and issubclass(noise.MultipleFreqCorrelatedNoise, noise.FreqCorrelatedNoise)
    assert noise.MultipleFreqCorrelatedNoise(niter=2, save_redundancy=True, seed=1).niter == 2
    assert noise.FreqCorrelatedNoise().save_redundancy is False
