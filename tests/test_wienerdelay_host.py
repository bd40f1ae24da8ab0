"""Host side of the Wiener delay transform: the float64 twin against vectors produced by executing the reference
(`tests/gen_golden_wienerdelay.py` -> tests/golden/wienerdelay.npz), the long-double twin against the generator's own
truth, the containers, the tasks' configuration and their host-side constants.  No GPU is touched."""

import os

import numpy as np
import pytest

import wienerdelay_twin as twin
from conftest import GOLDEN

GATED = ["G6E", "G6O", "G33", "G70", "P20"]
CASES = GATED + ["U20"]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "wienerdelay.npz")) as z:
        return {k: z[k] for k in z.files}


class _Z:
    """The dict of the golden file with the ``files`` attribute ``case_inputs`` reads."""

    def __init__(self, d):
        self.d, self.files = d, list(d)

    def __getitem__(self, k):
        return self.d[k]


def case(gold, name):
    c = twin.case_inputs(_Z(gold), name)
    c["win"], c["sdiag"], c["tau"] = (gold[f"{name}/{k}"] for k in ("win", "sdiag", "tau")) if f"{name}/win" in gold else (None, None, None)
    return c


def ref_pixels(gold, name, shape):
    if f"{name}/ref_pixels" in gold:
        return [tuple(int(i) for i in p) for p in gold[f"{name}/ref_pixels"]]
    return [(p, r, e) for p in range(shape[0]) for r in range(shape[1]) for e in range(shape[2])]


_truth_cache = {}


def truth_of(gold, name):
    """The long-double truth of a case (complex long double), computed once per session and checked against the pixels
    the generator stored."""
    if name not in _truth_cache:
        c = case(gold, name)
        _, F, sdiag = twin.constants(c["freq"], c["win"], c["cfg"]["prior_amp"], c["cfg"]["prior_scale"])
        assert np.array_equal(sdiag, c["sdiag"])
        t = twin.build(c["K"], c["C"], c["w"], c["dbp"], F, sdiag, c["win"], ld=True)
        for p, want in zip(gold[f"{name}/check_pixels"], gold[f"{name}/truth_check"]):
            got = t[tuple(int(i) for i in p)].astype(np.complex128)
            assert twin.rel_err(got, want) <= 2.0**-52, (name, p)  # (the same long double: the same bits, give or take the last)
        t.setflags(write=False)
        _truth_cache[name] = (t, F)
    return _truth_cache[name]


@pytest.mark.parametrize("name", CASES)
def test_float64_twin_against_reference(gold, name):
    c = case(gold, name)
    truth, F = truth_of(gold, name)
    got = twin.build(c["K"], c["C"], c["w"], c["dbp"], F, c["sdiag"], c["win"], ld=False)
    ref = gold[f"{name}/ref64"]
    pix = ref_pixels(gold, name, got.shape)
    sel = np.stack([got[p] for p in pix]).reshape(ref.shape)
    e_twin = twin.rel_err(got, truth.astype(np.complex128))
    e_ref, e_ref64 = float(gold[f"{name}/e_ref"]), float(gold[f"{name}/e_ref64"])
    e_tri = twin.rel_err(sel.astype(np.complex64), ref)
    print(f"wienerdelay host {name}: float64 twin {e_twin:.3e} e_ref64 {e_ref64:.3e} to the reference's complex64 {e_tri:.3e} e_ref {e_ref:.3e}")
    if bool(gold[f"{name}/gated"]):
        assert e_twin <= max(4 * e_ref64, 2.0**-50)
        assert e_tri <= 3 * e_ref + 2.0**-23


def test_twin_cholesky():
    rng = np.random.default_rng(5)
    B = rng.standard_normal((9, 9)) + 1j * rng.standard_normal((9, 9))
    A = (B @ B.conj().T + 9 * np.eye(9)).astype(twin.CLD)
    A = (A + A.conj().T) / 2  # (exactly Hermitian: the factorisation reads the lower triangle)
    L = twin.cholesky_ld(A)
    assert np.abs(L @ L.conj().T - A).max() < 1e-17 and np.abs(np.triu(L, 1)).max() == 0
    assert np.abs(twin.inverse_ld(A) @ A - np.eye(9)).max() < 1e-17
    with pytest.raises(np.linalg.LinAlgError):
        twin.cholesky_ld(np.diag([1.0, 0.0, 1.0]).astype(twin.CLD))


def test_apply_twin_against_reference(gold):
    for name in GATED:
        if f"{name}/ref_pixels" in gold:
            continue
        c = case(gold, name)
        spec, sw = twin.apply(gold[f"{name}/ref64"], c["map"][0], c["w"], ld=False)
        assert twin.rel_err(spec, gold[f"{name}/spec"]) <= 2.0**-50
        assert twin.rel_err(sw.astype(np.float32), gold[f"{name}/sweight"]) <= 3 * float(gold[f"{name}/e_ref_w"]) + 2.0**-23


# ---- containers


def test_containers():
    from draco_amd.core import containers

    freq = 600.0 + twin.DF * np.arange(4)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "YY"]), freq=freq, ra=3, el=np.linspace(-0.1, 0.1, 5))
    assert "filter" not in rm and "freq_cov" not in rm
    with pytest.raises(KeyError):
        rm.filter
    for name in ("filter", "freq_cov"):
        rm.add_dataset(name, allocate=True)
        ds = getattr(rm, name)
        assert ds.shape == (2, 4, 4, 3) and ds.dtype == np.float64 and rm.dataset_shape(name) == (2, 4, 4, 3)
    assert np.array_equal(rm.index_map["freq_sum"], rm.index_map["freq"])
    rm.add_dataset("dirty_beam_power", allocate=True)
    assert rm.dirty_beam_power.shape == (1, 2, 4, 5)
    for name in ("complex_filter", "complex_freq_cov"):
        with pytest.raises(NotImplementedError):
            rm.add_dataset(name)
        with pytest.raises(NotImplementedError):
            getattr(rm, name)

    tau = np.array([0.0, 0.64, 1.28])
    op = containers.DelayTransformOperator(delay=tau, axes_from=rm, attrs_from=rm)
    assert op.filter.shape == (2, 3, 5, 3, 4) and op.filter.dtype == np.complex64
    assert np.array_equal(op.delay, tau) and np.array_equal(op.index_map["freq"]["centre"], freq)
    assert containers.DelayTransformOperator in containers._all_containers()


# ---- configuration and the host-side constants


def test_config():
    from draco_amd.analysis import powerspec as ps

    t = ps.ConstructWienerDelayTransform()
    assert (t.prior_amp, t.prior_scale, t.window, t.window_lower_freq, t.window_upper_freq, t.workspace_mib) == (2.8e-5, 0.0, "uniform", None, None, 1024)
    t = ps.ConstructWienerDelayTransform(prior_amp=1, prior_scale="0.5", window="hann", window_lower_freq=601, workspace_mib=8)
    assert isinstance(t.prior_amp, float) and t.prior_scale == 0.5 and t.window_lower_freq == 601.0 and t.workspace_mib == 8
    with pytest.raises(ValueError, match="window"):
        ps.ConstructWienerDelayTransform(window="boxcar")
    with pytest.raises(ValueError, match="workspace_mib"):
        ps.ConstructWienerDelayTransform(workspace_mib=0)
    with pytest.raises(AttributeError):
        ps.ConstructWienerDelayTransform(epsilon=1.0)
    with pytest.raises(AttributeError):
        ps.ApplyWienerDelayTransform(window="hann")
    for name in ("ConstructWienerDelayTransform", "ApplyWienerDelayTransform"):
        assert name in ps.__all__


@pytest.mark.parametrize("name", CASES)
def test_prior_and_window(gold, name):
    from draco_amd.analysis import powerspec as ps

    c = case(gold, name)
    t = ps.ConstructWienerDelayTransform(**c["cfg"])
    assert np.array_equal(t._get_window(c["freq"]), c["win"])
    assert np.array_equal(t._get_prior(c["tau"]), c["sdiag"])
    tau, F, sdiag, FSFT, window = t._constants(c["freq"])
    tau_t, F_t, sdiag_t = twin.constants(c["freq"], c["win"], c["cfg"]["prior_amp"], c["cfg"]["prior_scale"])
    assert np.array_equal(tau, c["tau"]) and np.array_equal(F, F_t) and np.array_equal(sdiag, sdiag_t) and np.array_equal(window, c["win"])
    assert FSFT.shape == (c["freq"].size,) * 2 and tau.size == F.shape[1]
