"""GPU delay null-space filter (`csrc/nullfilter.hip`, `draco_amd/util/filters.py`, `DelayFilter` / `DelayFilterBase` in
`draco_amd/analysis/delay.py`) against a long-double truth and against vectors produced by executing the reference
(`tests/gen_golden_nullfilter.py` -> tests/golden/nullfilter*.npz).

Error measure.  Singular vectors at `sig ~ 1e-8 sig.max()` are determined to `eps sig.max() / sig` only, so the
reference's own float64 filter is about 1e-8 away from the truth and nothing is compared with it to a float64
tolerance.  Per case `e_gpu = max |gpu - truth| / max |truth|`, for filter matrices and for filtered data, with the truth
(`tests/nullfilter_twin.py`) rounded to the output's dtype; required: `e_gpu <= 4 e_ref`, `e_ref` the same measure of
the reference's output, read from the fixture.  Both are backward-stable float64 algorithms with an error proportional
to `eps sig.max() / sig_cut`, but they rotate in different orders: hence the factor.  `nkeep` must equal the fixture's
for every matrix (the fixture keeps `sig / sig.max()` out of `[1e-8 / 1.5, 1.5e-8]`), `sig` must agree with the twin's to
`1e-12 sig.max()`, the weights are bit-equal to the reference's, and no matrix may reach the sweep cap.

Each test prints its `e_gpu`, the ratio to `e_ref` and the sweeps before it asserts.  Measured (MI355X) `e_gpu / e_ref`: functions
0.67, 0.015, 0.96, 1.21, 0.74, 1.14, 1.03, 1.61 (in the order of `FN_NAMES`), streams 0.92, 1.17, 0.85, 0.96, ring map 1.13 and 1.42;
10 - 21 sweeps.  The table is in DESIGN.md section 7r.
"""

import os
import types

import numpy as np
import pytest

import nullfilter_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FN_NAMES = ["n64_even", "n64_odd", "n64_low", "n64_ones", "n64_few", "n80_hann", "n256", "n1024"]


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def gold():
    return {**_load("nullfilter.npz"), **_load("nullfilter_fnbig.npz")}


@pytest.fixture(scope="module")
def streams():
    return {**_load("nullfilter_stream.npz"), **_load("nullfilter_stream2.npz")}


@pytest.fixture(scope="module")
def ring(gold):
    """The ring map's inputs, reference outputs and (computed once, shared) truth in both dtypes."""
    g = {**_load("nullfilter_ringmap.npz"), "ref_map64": _load("nullfilter_ringmap64.npz")["ref_map"]}
    g["ref_map32"] = g.pop("ref_map")
    freq, cuts = gold["ring/freq"], gold["ring/cuts"]
    nbeam, npol, nfreq, nra, nel = g["map_q"].shape
    cache = {}
    for tag, dt in (("32", np.float32), ("64", np.float64)):
        rmap, weight = (g["map_q"] / 64.0).astype(dt), (g["w_q"] / 64.0).astype(dt)
        data = np.moveaxis(rmap, (2, 4), (0, 1)).reshape(nfreq, nel, nbeam * npol * nra)
        wgt = np.moveaxis(weight, (1, 3), (0, 1)).reshape(nfreq, nel, npol * nra)
        fd, fw, _ = twin.filter_items(freq, cuts, data, wgt, False, cache=cache)
        g[f"truth_map{tag}"] = np.ascontiguousarray(np.moveaxis(fd.reshape(nfreq, nel, nbeam, npol, nra), (0, 1), (2, 4)))
        g[f"truth_weight{tag}"] = np.ascontiguousarray(np.moveaxis(fw.reshape(nfreq, nel, npol, nra), (0, 1), (1, 3)))
    return g


def _check(name, got, truth, e_ref):
    e_gpu = twin.rel_err(got, truth)
    print(f"nullfilter {name}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {e_gpu / e_ref:.3f}")
    assert np.isfinite(np.abs(got)).all()
    assert e_gpu <= 4 * e_ref, (name, e_gpu, e_ref)


def _check_matrices(name, g, pre, status, nkeep, sig, sweeps):
    """`nkeep`, `sig` and the sweep cap of the distinct matrices of a task run, in the fixture's order of first use."""
    print(f"nullfilter {name}: nkeep {list(nkeep)} sweeps {list(sweeps)}")
    assert not np.any(status), (name, status)
    assert np.array_equal(nkeep, g[f"{pre}/nkeep"]), (name, nkeep, g[f"{pre}/nkeep"])
    ref = g[f"{pre}/sig"]
    assert sig.shape == ref.shape
    assert np.all(np.abs(sig - ref).max(axis=1) <= 1e-12 * ref.max(axis=1)), (name, np.abs(sig - ref).max(axis=1) / ref.max(axis=1))


@pytest.mark.parametrize("name", FN_NAMES)
def test_null_filter(gold, name):
    from draco_amd.device import Context
    from draco_amd.util import filters

    g = gold
    window = str(g[f"fn_{name}/window"])
    window = {"": False, "True": True}.get(window, window)
    samples, cutoff, mask, K, type_ = g[f"fn_{name}/samples"], float(g[f"fn_{name}/cutoff"]), g[f"fn_{name}/mask"], int(g[f"fn_{name}/num_modes"]), str(g[f"fn_{name}/type"])
    rows = g[f"fn_{name}/rows"]
    ctx = Context.get()
    info = {}
    nf, status, nkeep, sig = filters.build_null_filters(ctx, ctx.to_device(samples), [cutoff], K, mask[np.newaxis, :], filters.null_filter_window(samples, window), type_=type_, info=info)
    print(f"nullfilter fn {name}: n {samples.size} K {K} nkeep {nkeep[0]} sweeps {info['sweeps'][0]}")
    assert status[0] == 0 and nkeep[0] == int(g[f"fn_{name}/nkeep"])
    tsig = g[f"fn_{name}/sig"]
    assert np.abs(sig[0] - tsig).max() <= 1e-12 * tsig.max(), np.abs(sig[0] - tsig).max() / tsig.max()
    x = nf[0].cpu().numpy()
    _check(f"fn {name}", x[rows], g[f"fn_{name}/truth"], float(g[f"fn_{name}/e_ref"]))
    assert not x[:, ~mask].any()  # mask (and window) scale the columns ...
    assert not x[~mask][:, mask].any()  # ... and the rows of masked samples come out zero because the basis is zero there
    # the public function: the same matrix, on the device or as an array
    y = filters.null_filter(samples, cutoff, mask, num_modes=K, window=window, type_=type_, lapack_driver="gesdd")
    assert y.is_cuda and np.array_equal(y.cpu().numpy(), x)
    if samples.size <= 80:
        z = filters.null_filter(samples, cutoff, mask.astype(np.float64), num_modes=K, window=window, type_=type_, device=False)
        assert isinstance(z, np.ndarray) and z.dtype == np.float64 and np.array_equal(z, x)


def _telescope(feedpos):
    return types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None)


def _spy(monkeypatch):
    """Record what every `build_null_filters` call of a task returns."""
    from draco_amd.util import filters

    seen = []
    orig = filters.build_null_filters

    def wrapped(*a, **k):
        info = {}
        out = orig(*a, info=info, **k)
        seen.append((out[1], out[2], out[3], info["sweeps"]))
        return out

    monkeypatch.setattr(filters, "build_null_filters", wrapped)
    return seen


@pytest.mark.parametrize("name,dtype", [("NS", np.complex64), ("NS", np.complex128), ("EW", np.complex64), ("none", np.complex64)])
def test_stream(gold, streams, monkeypatch, name, dtype):
    from draco_amd.analysis.delay import DelayFilter
    from draco_amd.core import containers

    g, s = gold, streams
    tag = np.dtype(dtype).name
    q = s[f"{name}/vis_q"]
    vis = (q[..., 0] / 64.0 + 1j * (q[..., 1] / 64.0)).astype(dtype)
    weight = s[f"{name}/weight"]
    ss = containers.SiderealStream(freq=s[f"{name}/freq"], ra=vis.shape[2], prod=s[f"{name}/prod"], input=len(s[f"{name}/feedpos"]))
    ss.datasets["vis"] = containers.Dataset(host=vis.copy(), attrs={"axis": ["freq", "stack", "ra"]})
    ss.weight[:] = weight
    delay_cut, za_cut, extra_cut = (float(x) for x in s[f"{name}/cfg"])
    task = DelayFilter(delay_cut=delay_cut, za_cut=za_cut, extra_cut=extra_cut, telescope_orientation=str(s[f"{name}/orientation"]), window=bool(s[f"{name}/window"]))
    task.setup(_telescope(s[f"{name}/feedpos"]))
    seen = _spy(monkeypatch)
    assert task.process(ss) is ss and ss.vis.on_device and ss.weight.on_device
    out, w = ss.vis[:], ss.weight[:]
    assert out.dtype == dtype and w.dtype == np.float32
    assert len(seen) == 1
    _check_matrices(f"stream {name} {tag}", g, f"stream_{name}", *seen[0])
    _check(f"stream {name} {tag}", out, s[f"{name}/truth_vis_{tag}"], float(s[f"{name}/e_ref_{tag}"]))
    assert np.array_equal(w.view(np.uint32), s[f"{name}/ref_weight"].view(np.uint32))  # w * 0 or w * 1: exact
    real = np.float32 if dtype == np.complex64 else np.float64
    assert np.array_equal(out[:, 1].view(real), out[:, 4].view(real))  # entries 1 and 4 share a filter and their input rows
    # the entry without any weight is filtered with the full mask and keeps its zero weight
    assert not w[:, 3].any() and g[f"stream_{name}/f_mask"][3].all()
    assert not np.array_equal(out[:, 3], vis[:, 3])


@pytest.mark.parametrize("tag,dtype", [("32", np.float32), ("64", np.float64)])
def test_ringmap(gold, ring, monkeypatch, tag, dtype):
    from draco_amd.analysis.delay import DelayFilterBase
    from draco_amd.core import containers

    g, r = gold, ring
    cuts_el = g["ring/cuts"]

    class VaryingCut(DelayFilterBase):
        def _delay_cut(self, ss, axis, ind):
            assert axis == "el"
            return float(cuts_el[ind])

    rmap, weight = (r["map_q"] / 64.0).astype(dtype), (r["w_q"] / 64.0).astype(dtype)
    nb, npol, nfreq, nra, nel = rmap.shape
    assert nel % 16 != 0
    rm = containers.RingMap(freq=g["ring/freq"], beam=nb, pol=np.array(["XX", "YY"]), ra=nra, el=np.linspace(-1, 1, nel))
    rm.datasets["map"] = containers.Dataset(host=rmap.copy(), attrs={"axis": ["beam", "pol", "freq", "ra", "el"]})
    rm.datasets["weight"] = containers.Dataset(host=weight.copy(), attrs={"axis": ["pol", "freq", "ra", "el"]})
    task = VaryingCut(delay_cut=0.1)
    task.setup()
    seen = _spy(monkeypatch)
    assert task.process(rm) is rm and rm.map.on_device and rm.weight.on_device
    m, w = rm.map[:], rm.weight[:]
    assert m.dtype == dtype and w.dtype == dtype
    assert len(seen) == 1
    _check_matrices(f"ring map f{tag}", g, "ring", *seen[0])
    name = "float32" if tag == "32" else "float64"
    assert twin.rel_err(r[f"ref_map{tag}"], r[f"truth_map{tag}"]) <= 1.0001 * float(g[f"ring/e_ref_{name}"])  # the truth as stored by the generator
    _check(f"ring map f{tag}", m, r[f"truth_map{tag}"], float(g[f"ring/e_ref_{name}"]))
    assert np.array_equal(w, g["ring/ref_weight"].astype(dtype)) and np.array_equal(w, r[f"truth_weight{tag}"])
    assert not w[:, :, :, 6].any()  # the el without weight: full mask, zero weight


def test_errors():
    from draco_amd.analysis.delay import DelayFilterBase
    from draco_amd.core import containers

    task = DelayFilterBase()
    task.setup()
    with pytest.raises(TypeError, match="FreqContainer"):
        task.process(containers.SVDSpectrum(m=3, singularvalue=2))
    freq = 600.0 + 0.4 * np.arange(4)
    with pytest.raises(NotImplementedError, match="HybridVisMModes"):
        task.process(containers.HybridVisMModes(mmax=2, pol=2, freq=freq, ew=1, el=3))
    with pytest.raises(NotImplementedError, match="GridBeam"):
        task.process(containers.GridBeam(freq=freq, pol=2, input=1, theta=3, phi=2))
    ss = containers.SiderealStream(freq=freq, ra=4, stack=2)
    for cfg in (dict(axis="ra"), dict(dataset="vis_weight")):
        t = DelayFilterBase(**cfg)
        t.setup()
        with pytest.raises(NotImplementedError, match="apply path"):
            t.process(ss)
