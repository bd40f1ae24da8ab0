"""The twin of the transient RFI mask (``tests/vismask_twin.py``) against the reference-executed vectors of
``tests/golden/vismask.npz``, on the CPU: the masks of every case and the bits of ``stokes_I`` exactly, the high-pass
within twice the reference's own error, and the host-side pieces of the library (the Stokes-I table, the taps,
``unix_to_lsa``)."""

import os

import numpy as np
import pytest

import vismask_twin as twin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vismask.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def telescope(gold):
    from draco_amd.core.products import TransitTelescope

    kw = {k: gold[f"tel/{k}"].item() for k in ("ncyl", "nfeed_cyl", "npol_feed", "pair_rule", "latitude", "longitude", "lsd_start")}
    return TransitTelescope(gold["in/freq"], lmax=1, **kw)


def case_config(gold, name):
    cfg = {k: gold[f"case/{name}/{k}"].item() for k in ("stokes_i", "sigma_high", "sigma_low", "frac_samples")}
    cfg.update({k: [int(s) for s in gold[f"case/{name}/{k}"]] for k in ("mad_base_size", "mad_dev_size")})
    return cfg, bool(gold[f"case/{name}/sidereal"])


def test_telescope_and_table(gold):
    from draco_amd.analysis.transform import stokes_i_table

    tel = telescope(gold)
    ubase, ptr, rows = stokes_i_table(tel)
    assert len(tel.uniquepairs) == gold["in/vis"].shape[1] == 43
    assert np.array_equal(ubase, gold["stokes/ubase"]) and len(ubase) == 11
    counts = np.diff(ptr)
    assert sorted(set(counts.tolist())) == [0, 2] and (counts == 0).sum() == 1  # XX and YY per baseline; the zero separation keeps nothing
    assert not ubase[counts == 0].any()
    assert all(np.all(np.diff(rows[ptr[b] : ptr[b + 1]]) > 0) for b in range(len(ubase)))
    t = gold["in/time"]
    assert np.array_equal(tel.unix_to_lsa(t), 360.0 * (tel.unix_to_lsd(t) % 1.0))
    assert np.allclose(tel.unix_to_lsa(t), gold["in/ra"], rtol=0, atol=1e-9)
    # under the default pair rule no baseline has all four polarisation pairs
    from draco_amd.core.products import TransitTelescope

    _, ptr_c, rows_c = stokes_i_table(TransitTelescope(gold["in/freq"], lmax=1, ncyl=2, nfeed_cyl=4, npol_feed=2))
    assert len(rows_c) == 0 and not ptr_c.any()


def test_stokes_bits(gold):
    from draco_amd.analysis.transform import stokes_i_table

    _, ptr, rows = stokes_i_table(telescope(gold))
    vi, wi = twin.stokes_i(gold["in/vis"], gold["in/weight"], ptr, rows)
    assert vi.dtype == np.complex64 and wi.dtype == np.float32
    assert np.array_equal(vi.view(np.uint32), gold["stokes/vis"].view(np.uint32)) and np.array_equal(wi, gold["stokes/weight"])


def test_highpass_against_the_reference(gold):
    from draco_amd.util.filters import convolution_taps

    tel = telescope(gold)
    ra = np.unwrap(tel.unix_to_lsa(gold["in/time"]), period=360.0) * np.pi / 180.0
    cut = gold["in/freq"].min() * 1e6 / twin.SPEED_OF_LIGHT * gold["stokes/ubase"][:, 0].max() / np.cos(np.deg2rad(tel.latitude))
    taps = twin.design(ra, cut)
    assert len(taps) == 31 and np.array_equal(taps, convolution_taps(ra, cut))
    hp = twin.wconv(gold["stokes/vis"], gold["stokes/weight"], taps, highpass=True)
    e_ref = float(gold["hp/e_ref"])
    err = float(np.abs(hp - gold["hp/ref"]).max())
    print(f"twin against the reference: {err:.3e}, e_ref {e_ref:.3e}, scale {float(gold['hp/scale']):.3f}, conditioning {float(gold['hp/cond']):.3f}")
    assert 0.0 < e_ref < 1e-5 * float(gold["hp/scale"]) and err <= 2.0 * e_ref
    assert float(gold["hp/cond"]) >= 0.05


@pytest.mark.parametrize("name", ["defaults", "all_pol", "small_windows", "frac30", "sidereal"])
def test_twin_reproduces_the_reference(gold, name):
    assert name in gold["case/names"]
    tel = telescope(gold)
    cfg, sidereal = case_config(gold, name)
    if cfg.pop("stokes_i"):
        v, w, bl = gold["stokes/vis"], gold["stokes/weight"], gold["stokes/ubase"]
    else:
        v, w, bl = gold["in/vis"], gold["in/weight"], tel.baselines
    mask0 = (w == 0).all(axis=1) | gold["in/static"][:, None]
    times = tel.lsd_to_unix(int(gold["in/lsd"]) + gold["in/ra"] / 360.0) if sidereal else gold["in/time"]
    got = twin.transient_mask(v, w, mask0, gold["in/freq"], bl, times, tel.unix_to_lsa, tel.latitude, **cfg)
    assert np.array_equal(got, gold[f"case/{name}/mask"])
    assert 0.0 < got.mean() < 1.0 and float(gold[f"case/{name}/margin"]) > 1e-9


def test_twin_hysteresis():
    x = np.array([[0.0, 3.0, 3.0, 0.0, 3.0], [9.0, 0.0, 3.0, 0.0, 3.0], [3.0, 0.0, np.nan, 3.0, 2.0]])
    want = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0]], dtype=bool)
    assert np.array_equal(twin.hysteresis(x, 2.0, 8.0), want)
    assert np.array_equal(twin.hysteresis(x, 9.5, 8.0), x > 8.0)  # low > high: low <- high
    assert not twin.hysteresis(x, 2.0, 9.0).any()  # strict comparisons
