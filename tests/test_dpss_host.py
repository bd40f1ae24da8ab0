"""Host-side checks of the DPSS inpainting (no GPU): the NumPy twin (`tests/dpss_twin.py`) against vectors produced by
executing the reference (`tests/gen_golden_dpss.py` -> tests/golden/dpss.npz), the host basis functions against the
stored bases, and the quirks of the gap flag.

Measures as in the generator: `max |got - truth| / max |truth|` for the data; for the weights the largest elementwise
relative error where the other side is non-zero, with equal zero patterns.  The float64 twin has to agree with the
reference within `3 e_ref`, `e_ref` the reference's own (float32) error against the long-double truth.
"""

import os

import numpy as np
import pytest

import dpss_twin as twin
from conftest import GOLDEN

FUNCTION_CASES = ["f70", "f161", "r140", "f1024", "r1100"]
TASK_CASES = {"t_plain": 0, "t_delay": 0, "t_mmode": 2}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "dpss.npz")) as z:
        g = {k: z[k] for k in z.files}
    for name in ("f1024", "r1100"):
        with np.load(os.path.join(GOLDEN, f"dpss_basis_{name}.npz")) as z:
            g[f"{name}/A"] = z["A"]
    return g


@pytest.mark.parametrize("name", FUNCTION_CASES)
def test_twin_against_reference_functions(gold, name):
    g = {k.split("/")[1]: v for k, v in gold.items() if k.startswith(name + "/")}
    W = g["w"] > 0
    xf, wf = twin.filter_columns(g["x"], g["w"], g["A"], W, 1e-3)
    e_v = twin.rel_err(xf.astype(np.complex64), g["ref_filter_x"])
    e_w, same = twin.weight_err(wf.astype(np.float32), g["ref_filter_w"])
    print(f"dpss twin {name}: to the reference vis {e_v:.3e} weight {e_w:.3e}; e_ref {g['e_ref']}")
    assert same
    assert e_v <= 3 * g["e_ref"][0] and e_w <= 3 * g["e_ref"][1]
    # and against the stored truth: the float64 twin reproduces its own stored error
    e_t, same = twin.weight_err(wf.astype(np.float32), g["truth_w"])
    assert same and twin.rel_err(xf.astype(np.complex64), g["truth_x"]) <= max(2 * g["e_f64"][0], twin.FLOOR_VIS) and e_t <= max(2 * g["e_f64"][1], twin.FLOOR_W)


@pytest.mark.parametrize("name", list(TASK_CASES))
def test_twin_against_reference_tasks(gold, name):
    g = {k.split("/")[1]: v for k, v in gold.items() if k.startswith(name + "/")}
    bases = [g[f"A{i}"] for i in range(len(g["cuts"]))]
    vo, wo = twin.task_columns(g["vis"], g["weight"], TASK_CASES[name], bases, g["amap"], 1e-3, float(g["cutoff"]), True)
    e_v = twin.rel_err(vo, g["ref_vis"])
    e_w, same = twin.weight_err(wo, g["ref_weight"])
    print(f"dpss twin {name}: to the reference vis {e_v:.3e} weight {e_w:.3e}; e_ref {g['e_ref']}")
    assert same
    assert e_v <= 3 * g["e_ref"][0] and e_w <= 3 * g["e_ref"][1]
    keep = g["weight"] > 0
    assert np.array_equal(vo[keep].view(np.uint32), g["vis"][keep].view(np.uint32))  # the put-back


@pytest.mark.parametrize("name", FUNCTION_CASES)
def test_host_basis(gold, name):
    """`make_covariance` + `get_basis` against the basis the reference built: equal shape and dtype, and the projector
    `A A^T` equal to the float32 rounding of the basis (an entry is a sum of products of two entries rounded to 2**-24
    relative, over rows of norm at most one: 2 x 2**-24, doubled for the two sides)."""
    from draco_amd.util import dpss

    g = {k.split("/")[1]: v for k, v in gold.items() if k.startswith(name + "/")}
    cov = dpss.make_covariance(g["samples"], float(g["cut"]), 0.0)
    assert cov.dtype == np.float64 and cov.shape == (g["samples"].size,) * 2
    A = dpss.get_basis(cov)
    assert A.shape == g["A"].shape and A.dtype == g["A"].dtype == np.float32
    a, b = A.astype(np.float64), g["A"].astype(np.float64)
    d = float(np.abs(a @ a.T - b @ b.T).max())
    print(f"dpss basis {name}: shape {A.shape}, max |A A^T - A0 A0^T| {d:.3e}")
    assert d <= 2.0**-22


def test_host_basis_complex_and_arguments():
    from draco_amd.util import dpss

    s = 800.0 - 0.390625 * np.arange(24)
    cov = dpss.make_covariance(s, [0.2, 0.1], [0.0, 0.5])
    assert np.iscomplexobj(cov)
    assert dpss.get_basis(cov).dtype == np.complex64 and dpss.get_basis(cov, dtype=np.float64).dtype == np.complex128
    assert dpss.get_basis(dpss.make_covariance(s, 0.2, 0.0), dtype=np.float64).dtype == np.float64
    with pytest.raises(ValueError, match="same length"):
        dpss.make_covariance(s, [0.2, 0.1], [0.0])


@pytest.mark.parametrize("name", FUNCTION_CASES)
def test_gap_flag_against_reference(gold, name):
    W = gold[f"{name}/w"] > 0
    assert np.array_equal(twin.flag_above_cutoff(W, float(gold[f"{name}/fc"])), gold[f"{name}/ref_flag"])


def test_gap_flag_quirks():
    """`fc = 2.5` on 12 samples: a gap from `ri` to `fi` has `dist = fi - ri`, so the 3-wide gap (dist 2) is kept and the
    4-wide gap (dist 3) is not; everything before the first valid sample is flagged; the last valid sample is flagged
    with everything after it; a column without a valid sample loses only its last sample."""
    W = np.ones((12, 4), dtype=bool)
    W[2:5, 0] = False  # 3 wide
    W[4:8, 1] = False  # 4 wide
    W[:2, 2] = False  # a gap at the start
    W[10:, 2] = False  # and one at the end
    W[:, 3] = False
    k = twin.flag_above_cutoff(W, 2.5)
    assert k[:11, 0].all() and not k[11, 0]
    assert k[:4, 1].all() and not k[4:8, 1].any() and k[8:11, 1].all() and not k[11, 1]
    assert not k[:2, 2].any() and k[2:9, 2].all() and not k[9:, 2].any()
    assert k[:11, 3].all() and not k[11, 3]
    assert twin.flag_above_cutoff(W, None) is not None and np.array_equal(twin.flag_above_cutoff(W, None), W)


def test_task_surface():
    """Names, config attributes and defaults of the reference (`interpolate.py:56-66, 212, 293-295, 325`)."""
    from draco_amd.analysis import interpolate as ip

    t = ip.DPSSFilter()
    assert (t.inpaint, t.axis, t.iter_axes, t.centres, t.halfwidths, t.epsilon, t.cutoff_frac, t.copy) == (True, "freq", ["stack", "el"], None, None, 1.0e-3, 1.0, True)
    d = ip.DPSSFilterDelayStokesI(halfwidths=[0.2], centres=[0.0], za_cut=0.5, extra_cut=0.1, telescope_orientation="EW")
    assert (d.axis, d.za_cut, d.extra_cut, d.telescope_orientation) == ("freq", 0.5, 0.1, "EW")
    assert ip.DPSSFilterMMode().axis == "ra" and ip.DPSSFilterMModeStokesI().telescope_orientation == "NS"
    assert issubclass(ip.DPSSFilterDelayStokesI, ip.StokesIMixin) and issubclass(ip.DPSSFilterMMode, ip.DPSSFilterBaseline)
    with pytest.raises(ValueError, match="axis"):
        ip.DPSSFilterDelay(axis="ra")
    with pytest.raises(ValueError, match="telescope_orientation"):
        ip.DPSSFilterMMode(telescope_orientation="up")
    with pytest.raises(NotImplementedError, match="mask"):
        ip.DPSSFilter().setup(mask=object())
    with pytest.raises(NotImplementedError):
        ip.DPSSFilterBaseline()._get_baseline_cuts()


def test_telescope_freq_start():
    from draco_amd.core.products import TransitTelescope

    tel = TransitTelescope(np.array([600.0, 640.0, 620.0]), lmax=4, ncyl=1, nfeed_cyl=2)
    assert tel.freq_start == 640.0
