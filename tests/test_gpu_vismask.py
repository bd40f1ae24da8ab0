"""The transient RFI mask from visibilities on the GPU (``csrc/vismask.hip``): the weighted FIR
filter and the transform across baselines against the long-double twin (``tests/vismask_twin.py``) under the bound of
section 7l, ``max(32 e_f64, 8 * 2^-53 * scale)`` with ``e_f64`` the error of a float64 NumPy computation of the same
thing; the hysteresis threshold and the Stokes-I sum exactly; ``RFITransientVisMask`` against the reference-executed
masks of ``tests/golden/vismask.npz`` (equal exactly, whatever the batch sizes), and the chain mask -> weights.

Recorded on the MI355X: see DESIGN.md section 7t for the burst-free fraction of ``test_chain_clean_stream``.
"""

import os
import types

import numpy as np
import pytest
import scipy.fft
from scipy import signal

import vismask_twin as twin
from test_vismask_host import case_config, telescope

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vismask.npz")
CASES = ["defaults", "all_pol", "small_windows", "frac30", "sidereal"]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _bound(e_f64, truth):
    return max(32.0 * e_f64, 8.0 * 2.0**-53 * float(np.abs(truth).max()))


# ---- the filter


def _filter_input(rng, n, ntap, dtype):
    nrow = 6
    if np.dtype(dtype).kind == "c":
        d = (rng.normal(size=(nrow, n)) + 1j * rng.normal(size=(nrow, n)) + (2.0 - 1.0j)).astype(dtype)
    else:
        d = (rng.normal(size=(nrow, n)) + 2.0).astype(dtype)
    w = rng.uniform(0.5, 2.0, size=(nrow, n))
    w[1] = 0.0  # a row without weight
    w[2, n // 4 : n // 4 + ntap + 3] = 0.0  # a gap longer than the taps (the whole tail, where the row is short)
    w[3][rng.uniform(size=n) < 0.3] = 0.0
    w[4] = 1.0
    w[5, : min(n, ntap + 1)] = 0.0  # ... and one at the start of the row
    return d, w.astype(np.float32 if dtype == np.complex64 else np.float64)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128, np.float64])
@pytest.mark.parametrize("n,ntap", [(n, k) for n in (1, 63, 64, 65, 160, 257) for k in (1, 3, 11, 101)] + [(20, 33), (1500, 31)])
def test_filter(n, ntap, dtype):
    from draco_amd.device import Context
    from draco_amd.util import filters

    rng = np.random.default_rng(1000 * n + ntap)
    d, w = _filter_input(rng, n, ntap, dtype)
    taps = signal.firwin(ntap, 1.0 / (ntap + 1), window="flattop", fs=2.0)
    ctx = Context.get()
    c = (ntap - 1) // 2
    support = np.stack([np.convolve((w[r] != 0).astype(float), np.ones(ntap), mode="full")[c : c + n] for r in range(len(w))])  # samples with weight under the taps
    assert (support == 0).any()
    for highpass in (False, True):
        got = filters.wconv_filter_device(ctx, ctx.to_device(d), ctx.to_device(w), taps, highpass=highpass).cpu().numpy()
        assert got.dtype == (np.float64 if dtype == np.float64 else np.complex128) and got.shape == d.shape
        truth = twin.wconv(d, w, taps, highpass=highpass)
        e_f64 = float(np.abs(twin.wconv(d, w, taps, highpass=highpass, real=np.float64) - truth).max())
        err = float(np.abs(got - truth).max())
        print(f"n {n} ntap {ntap} {np.dtype(dtype).name} highpass {highpass}: err {err:.3e} e_f64 {e_f64:.3e} bound {_bound(e_f64, truth):.3e}")
        assert err <= _bound(e_f64, truth)
        # no weight under the taps: the low-pass is exactly zero, the high-pass exactly the input
        want = d.astype(got.dtype) if highpass else np.zeros_like(got)
        assert np.array_equal(got[support == 0], want[support == 0])


def test_filter_public(gold):
    """NumPy in, NumPy out; tensors in, a tensor out; another axis; the taps are the reference's design."""
    from draco_amd.device import Context
    from draco_amd.util import filters

    tel = telescope(gold)
    ra = np.unwrap(tel.unix_to_lsa(gold["in/time"]), period=360.0) * np.pi / 180.0
    cut = gold["in/freq"].min() * 1e6 / twin.SPEED_OF_LIGHT * gold["stokes/ubase"][:, 0].max() / np.cos(np.deg2rad(tel.latitude))
    v, w = gold["stokes/vis"], gold["stokes/weight"]
    got = filters.highpass_weighted_convolution_filter(v, w, ra, cut)
    truth = twin.wconv(v, w, twin.design(ra, cut), highpass=True)
    e_ref = float(gold["hp/e_ref"])
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128
    assert float(np.abs(got - truth).max()) <= 2.0 * e_ref and float(np.abs(got - gold["hp/ref"]).max()) <= 2.0 * e_ref
    ctx = Context.get()
    low = filters.lowpass_weighted_convolution_filter(ctx.to_device(np.ascontiguousarray(v.transpose(0, 2, 1))), ctx.to_device(np.ascontiguousarray(w.transpose(0, 2, 1))), ra, cut, axis=1)
    assert hasattr(low, "device") and np.array_equal(v - low.cpu().numpy().transpose(0, 2, 1), got)
    with pytest.raises(ValueError):
        filters.highpass_weighted_convolution_filter(v, w, ra, 1e9)  # firwin: a cutoff beyond fs / 2


# ---- the transform across baselines


@pytest.mark.parametrize("nt", [1, 65, 160])
@pytest.mark.parametrize("nstack", [1, 2, 3, 8, 11, 12, 17, 64, 100, 129])
def test_beam_transform(nstack, nt):
    import torch

    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    rng = np.random.default_rng(100 * nstack + nt)
    x = rng.normal(size=(3, nstack, nt)) + 1j * rng.normal(size=(3, nstack, nt))
    x[1, nstack // 2] = 0.0
    ctx = Context.get()
    xd = ctx.to_device(x)
    out = torch.full((3, nstack, nt), float("nan"), dtype=torch.float64, device=xd.device)
    _lib.check(_lib.lib.dmm_beam_abs_fft(ctx.handle, ptr(xd), 3, nstack, nt, ptr(out)))
    got = out.cpu().numpy()
    truth = twin.beam_dft(x)
    e_f64 = float(np.abs(np.abs(scipy.fft.fft(x, axis=1)) - truth).max())
    err = float(np.abs(got - truth).max())
    print(f"nstack {nstack} nt {nt}: err {err:.3e} e_f64 {e_f64:.3e} bound {_bound(e_f64, truth):.3e}")
    assert err <= _bound(e_f64, truth)


# ---- the hysteresis threshold


def _hyst(x, low, high, out=None, info=None):
    from draco_amd.device import Context
    from draco_amd.util import rfi

    ctx = Context.get()
    return rfi.hysteresis_device(ctx, ctx.to_device(np.ascontiguousarray(x, dtype=np.float64)), low, high, out=out, info=info).cpu().numpy().astype(bool)


@pytest.mark.parametrize("shape", [(1, 1), (1, 97), (97, 1), (5, 7), (64, 64), (65, 129), (3, 65, 129)])
def test_hysteresis(shape):
    from draco_amd.util import rfi

    rng = np.random.default_rng(shape[-1] + 7 * shape[-2])
    x = rng.normal(size=shape) * 2.0
    x[rng.uniform(size=shape) < 0.05] = np.nan
    x[rng.uniform(size=shape) < 0.05] = 1.0  # equal to the low threshold: not above it
    x[rng.uniform(size=shape) < 0.02] = 3.0  # equal to the high threshold: a low sample, no seed
    for low, high in ((1.0, 3.0), (0.0, 3.0), (-1.0, 5.0), (3.5, 3.0), (1.0, 50.0)):
        want = twin.hysteresis(x, low, high)
        assert np.array_equal(_hyst(x, low, high), want)
        assert np.array_equal(rfi.apply_hysteresis_threshold(x if len(shape) > 2 or min(shape) > 1 else x.reshape(-1), low, high).reshape(shape), want)
    assert not want.any()  # (1, 50): no seed anywhere
    if x.size > 1000:
        first = twin.hysteresis(x, 1.0, 3.0)
        assert (x > 3.0).sum() < first.sum() < (x > 1.0).sum()  # the middle ground: some low samples join, not all


def test_hysteresis_serpentine_and_accumulate():
    import torch

    from draco_amd import _lib

    nf, nt = 33, 65
    x = np.zeros((nf, nt))
    x[0::2] = 3.0
    for r in range(1, nf, 2):  # the turns, at alternating ends
        x[r, nt - 1 if (r // 2) % 2 == 0 else 0] = 3.0
    x[0, 0] = 9.0  # the only seed, at one end of the path
    info = {}
    got = _hyst(x, 2.0, 8.0, info=info)
    assert np.array_equal(got, twin.hysteresis(x, 2.0, 8.0)) and np.array_equal(got, x > 2.0)
    print(f"serpentine {nf} x {nt}: {info['sweeps']} sweeps")
    assert 2 <= info["sweeps"] <= nf < _lib.DMM_RFI_HYST_MAX_SWEEPS
    x[16, 30] = 0.0  # cut the path: the far half is no longer reached
    cut = _hyst(x, 2.0, 8.0)
    assert np.array_equal(cut, twin.hysteresis(x, 2.0, 8.0)) and cut.sum() < got.sum() - 100
    from draco_amd.device import Context

    prior = np.zeros((nf, nt), dtype=np.uint8)
    prior[5, 5] = prior[1, 3] = 1
    out = Context.get().to_device(prior)
    assert np.array_equal(_hyst(x, 2.0, 8.0, out=out), cut | (prior != 0)) and out.dtype == torch.uint8


# ---- Stokes I


def _stream(gold, sidereal=False, device=False):
    from draco_amd.core import containers
    from draco_amd.device import Context

    ns = gold["in/vis"].shape[1]
    if sidereal:
        s = containers.SiderealStream(freq=gold["in/freq"], stack=ns, ra=gold["in/ra"])
        s.attrs["lsd"] = int(gold["in/lsd"])
    else:
        s = containers.TimeStream(freq=gold["in/freq"], stack=ns, time=gold["in/time"])
    s.vis[:] = gold["in/vis"]
    s.weight[:] = gold["in/weight"]
    if device:
        ctx = Context.get()
        s.vis.set_device(s.vis.device(ctx))
        s.weight.set_device(s.weight.device(ctx))
    return s


def test_stokes_i_bits(gold):
    import torch

    from draco_amd.analysis.transform import stokes_I

    for device in (False, True):
        vi, wi, ubase = stokes_I(_stream(gold, device=device), telescope(gold))
        assert vi.dtype == torch.complex64 and wi.dtype == torch.float32 and np.array_equal(ubase, gold["stokes/ubase"])
        assert np.array_equal(vi.cpu().numpy().view(np.uint32), gold["stokes/vis"].view(np.uint32))
        assert np.array_equal(wi.cpu().numpy(), gold["stokes/weight"])
    assert not vi.cpu().numpy()[:, ~np.any(ubase, axis=1)].any()  # the zero separation: a zero row


# ---- the task


def _task(gold, name, **over):
    from draco_amd.analysis import flagging

    cfg, sidereal = case_config(gold, name)
    static = gold["in/static"]

    class Hooked(flagging.RFITransientVisMask):
        def _static_rfi_mask_hook(self, freq, timestamp=None):
            assert len(freq) == len(static) and timestamp is not None
            return static

    task = Hooked(**dict(cfg, **over))
    task.setup(telescope(gold))
    return task, sidereal


@pytest.fixture(scope="module")
def masks(gold):
    """Every case once, from a host-resident stream: shared by the tests below."""
    from draco_amd.core import containers

    out = {}
    for name in CASES:
        task, sidereal = _task(gold, name)
        res = task.process(_stream(gold, sidereal))
        assert type(res) is (containers.SiderealRFIMask if sidereal else containers.RFIMask)
        out[name] = np.array(res.mask[:])
    return out


@pytest.mark.parametrize("name", CASES)
def test_task_golden(gold, masks, name):
    assert masks[name].dtype == np.bool_
    assert np.array_equal(masks[name], gold[f"case/{name}/mask"])


@pytest.mark.parametrize("name", CASES)
def test_task_device_stream_and_batches(gold, masks, name):
    """Device-resident input, a second run of one task, a fresh task, and a workspace that forces one frequency per
    batch, one beam per slab and the flag cube through the host: the same bits."""
    task, sidereal = _task(gold, name)
    s = _stream(gold, sidereal, device=True)
    a = np.array(task.process(s).mask[:])
    b = np.array(task.process(s).mask[:])
    small, _ = _task(gold, name, workspace_mib=0.01)
    c = np.array(small.process(_stream(gold, sidereal)).mask[:])
    for m in (a, b, c):
        assert np.array_equal(m, masks[name])


def test_batch_sizes_are_what_the_test_means(gold):
    from draco_amd.analysis.transform import stokes_I
    from draco_amd.device import Context

    ctx = Context.get()
    tel = telescope(gold)
    vi, wi, ubase = stokes_I(_stream(gold), tel)
    mask0 = ctx.to_device(((gold["stokes/weight"] == 0).all(axis=1) | gold["in/static"][:, None]).view(np.uint8))
    got = {}
    for mib in (0.01, 1024):
        task, _ = _task(gold, "defaults", workspace_mib=mib)
        info = {}
        got[mib] = (task.generate_mask(vi, wi, mask0, gold["in/freq"], ubase, gold["in/time"], info=info), info)
    assert np.array_equal(got[0.01][0], got[1024][0]) and np.array_equal(got[1024][0], gold["case/defaults/mask"])
    assert (got[0.01][1]["freq_per_batch"], got[0.01][1]["beams_per_slab"], got[0.01][1]["cube_on_device"]) == (1, 1, False)
    assert got[1024][1]["freq_per_batch"] >= 6 and got[1024][1]["beams_per_slab"] == 11 and got[1024][1]["cube_on_device"]
    assert 1 <= got[1024][1]["sweeps"] < 64


def test_task_errors(gold):
    from draco_amd.analysis import flagging

    task, _ = _task(gold, "sidereal")
    s = _stream(gold, sidereal=True)
    del s.attrs["lsd"]
    with pytest.raises(ValueError, match="csd"):
        task.process(s)
    other = types.SimpleNamespace(index_map={"freq": gold["in/freq"]}, redistribute=lambda axis: None)
    with pytest.raises(TypeError, match="time"):
        task.process(other)
    base = flagging.RFIVisMask()
    base.setup(telescope(gold))
    with pytest.raises(NotImplementedError):
        base.process(_stream(gold))
    assert not base._static_rfi_mask_hook(gold["in/freq"], 0.0).any()
    assert flagging.apply_hysteresis_threshold is not None
    t = flagging.RFITransientVisMask()
    assert (tuple(t.mad_base_size), tuple(t.mad_dev_size), t.sigma_high, t.sigma_low, t.frac_samples, t.stokes_i) == ((1, 101), (1, 51), 8.0, 2.0, 0.01, True)


# ---- the chain


def _noise_stream(gold, seed):
    from draco_amd.core import containers

    rng = np.random.default_rng(seed)
    ns = gold["in/vis"].shape[1]
    nf, nt = 4, len(gold["in/time"])
    s = containers.TimeStream(freq=gold["in/freq"][:nf], stack=ns, time=gold["in/time"])
    vis = (1.0 + 0.5j) + 0.5 * (rng.normal(size=(nf, ns, nt)) + 1j * rng.normal(size=(nf, ns, nt)))
    s.vis[:] = vis.astype(np.complex64)
    s.weight[:] = 3.0
    return s


def test_chain_burst_is_zeroed(gold):
    from draco_amd.analysis import flagging

    s = _noise_stream(gold, 5)
    vis = np.array(s.vis[:])
    vis[2, :, 90:93] += 30.0
    s.vis[:] = vis
    task = flagging.RFITransientVisMask()
    task.setup(telescope(gold))
    mask = task.process(s)
    assert np.array(mask.mask[:])[2, 90:93].all()
    out = flagging.ApplyTimeFreqMask().process(s, mask)
    w = np.array(out.weight[:])
    assert not w[2, :, 90:93].any() and np.array_equal(w == 0, np.broadcast_to(np.array(mask.mask[:])[:, None, :], w.shape))


def test_chain_clean_stream(gold):
    """A burst-free stream under the default windows: the fraction of clean samples the task flags is recorded (DESIGN.md
    section 7t), not prescribed; it must stay a minority."""
    from draco_amd.analysis import flagging

    task = flagging.RFITransientVisMask()
    task.setup(telescope(gold))
    frac = float(np.array(task.process(_noise_stream(gold, 6)).mask[:]).mean())
    print(f"burst-free stream: {100 * frac:.2f} % of samples flagged")
    assert frac < 0.5
