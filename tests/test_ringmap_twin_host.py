"""The long-double twin of the ring-map deconvolver (``tests/ringmap_twin.py``) proved on the host, before the GPU sweep
(``test_gpu_ringmap_direct.py``) trusts it: against the float64 oracle on every case table of the sweep, against the
reference-executed golden vectors, its direct transforms against ``numpy.fft``, and the exclusion caps of the float32
measures reached by the float64 restatements alone.

``e_ref`` -- the oracle's figure under the sweep's own measures -- is printed per case and held under the sanity ceiling
``64 * 2**-53 * log2(M)`` (``M`` the transform length behind a row, at least 2).  Measured here: 1e-16 ... 1.1e-14, but for a few
mode-1 cases up to 3.0e-14 (``nm = 17``, odd, 65 elevations: a negative weight turns one sign's normalised weights negative
and a mode's ``sum_w`` partly cancels); the ceiling there is 5.0e-14.  The whole file takes about 10 s.
"""

import math
import os

import numpy as np
import pytest

import ringmap_twin as rt
from oracle import ringmap as orm


def _ceiling(nra):
    return 64 * rt.U53 * math.log2(max(rt.fft_length(nra), 2))


def _against_oracle(case):
    T, ref = case.truth(), case.reference()
    f = case.figures(T, *ref)
    print(f"ringmap twin host {case.name}: " + " ".join(f"{k} e_ref {v[0]:.3g}" for k, v in f.items()))
    for k, (e_ref, zeros) in f.items():
        assert zeros, (case.name, k)
        assert e_ref <= _ceiling(case.nra), (case.name, k, e_ref)
    assert rt.constant_along_ra(ref[1])


@pytest.mark.parametrize("table", list(rt.THREE_KERNEL))
def test_truth_against_oracle_three_kernel_shapes(table):
    for i, shape in enumerate(rt.THREE_KERNEL[table]):
        for case in rt.cases_of(shape, i):
            _against_oracle(case)


@pytest.mark.parametrize("table", list(rt.SKIP))
def test_truth_against_oracle_skip_deconvolution(table):
    for i, shape in enumerate(rt.SKIP[table]):
        nel = shape[2]
        for iref in sorted({0, nel // 2, nel - 1}):
            for case in rt.cases_of(shape, i, skip=True, iref=iref):
                _against_oracle(case)


@pytest.mark.parametrize("table", list(rt.SINGLE_PASS))
def test_truth_against_oracle_single_pass_shapes(table):
    for i, (nm, nel, new, _) in enumerate(rt.SINGLE_PASS[table]):
        for case in rt.cases_of((nm, False, nel, new, 1, 1, None), i):
            _against_oracle(case)


def test_truth_against_oracle_tile_map_shapes():
    for i, (nel, npol, nfreq) in enumerate(rt.TILE_MAP):
        _against_oracle(rt.cases_of((9, False, nel, 1, npol, nfreq, None), i)[i % 3])


def test_case_tables_hold_what_they_promise():
    """Exact zeros, negative weights, dead rows and a dead (pol, freq) are really in the inputs."""
    c = rt.Case(17, False, 63, 3, 1, 3, mode=1, variety=1)
    T = c.truth()
    assert (c.hw < 0).any() and (c.hw == 0).mean() > 0.1 and not c.hw[c.nm // 2].any() and not c.hw[c.nm // 3, 1].any() and not c.hw[..., 1].any()
    assert not T["map"][0, 2].any() and not T["weight"][0, 2].any()  # the (pol, freq) without weight
    assert not T["map"][..., c.zero_el].any() and T["map"][0, 0, :, 0].any()
    w = T["weight"][T["weight"] > 0]
    assert w.max() / w.min() > 1e15  # p = 12: the weights of one call span many decades
    c = rt.Case(17, False, 63, 3, 1, 3, mode=2, variety=2)
    assert not c.eps.any() and not c.window[:, :, c.nel // 2].any() and not c.truth()["map"][..., c.nel // 2].any()
    assert rt.Case(9, False, 5, 4, mode=0, variety=1).wt[-1] == 0 and rt.Case(9, False, 5, 4, mode=2, variety=1).wt[-1] == 0


def test_dirty_beam_power_by_parseval_is_the_sum_over_ra():
    for shape in ((9, False, 5, 4, 1, 1, None), (20, True, 9, 2, 1, 1, None), (4, True, 2, 1, 1, 1, None)):
        for case in rt.cases_of(shape, 0):
            T = case.truth()
            direct = (T["dirty_beam"] ** 2).sum(axis=2) / rt.LD(case.nra)
            e, zeros = rt.element_measure(direct.astype(np.float64), T["dirty_beam_power"])
            assert zeros and e < 4 * rt.U53, (case.name, e)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 39, 64])
def test_direct_dft_against_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n // 2 + 1)) + 1j * rng.standard_normal((3, n // 2 + 1))
    got = rt.irfft_direct(x.real, x.imag, n)
    ref = np.fft.irfft(x, n=n, axis=-1)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 8 * rt.U53 * math.log2(max(n, 2)) * np.abs(ref).max()
    sub = np.array([0, n - 1, n // 2])
    assert np.array_equal(rt.irfft_direct(x.real, x.imag, n, sub), got[:, sub])
    # fewer modes than n // 2 + 1: the missing ones are zero; more: not used
    if n >= 7:
        assert np.abs(rt.irfft_direct(x.real[:, :3], x.imag[:, :3], n) - np.fft.irfft(x[:, :3], n=n, axis=-1)).max() < 1e-14
    z = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    fr, fi = rt.dft_direct(z.real.astype(rt.LD), z.imag.astype(rt.LD), n, np.arange(n))
    assert np.abs((fr + 1j * fi).astype(np.complex128) - np.fft.fft(z, axis=-1)).max() <= 8 * rt.U53 * n * np.abs(z).max()


def test_truth_against_reference_golden(golden_dir):
    """The twin with the makers' conventions on top, against the reference classes' own outputs (which form ``|b|^2`` and,
    with inverse-variance weights, the whole product in float32: 5e-6 of the largest element, as ``test_gpu_ringmap.py``)."""
    g = np.load(os.path.join(golden_dir, "ringmap_deconvolve.npz"))
    freq, ew, el = g["freq"], g["ew"], g["el"]
    for i in range(int(g["ncase"])):
        kind, weight_ew = str(g[f"c{i}_kind"]), str(g[f"c{i}_weight_ew"])
        skip, oddra = (bool(x) for x in g[f"c{i}_opts"])
        excl = [int(x) for x in g[f"c{i}_exclude"]]
        inv_SN, gal_amp, psrc_amp = (float(x) for x in g[f"c{i}_params"])
        hv, hw, bv = g[f"c{i}_hv"], g[f"c{i}_hw"], g[f"c{i}_bv"]
        nm, new = hv.shape[0], hv.shape[4]
        nra = 2 * (nm - 1) + int(oddra)
        m = np.arange(nm)
        reg = dict(inv_SN=inv_SN) if kind == "tikhonov" else dict(gal_amp=gal_amp, psrc_amp=psrc_amp)
        eps = np.stack([np.broadcast_to(np.asarray(orm.regularisation(kind, f, m, **reg), dtype=np.float64).reshape(-1), (nm,)) for f in freq])
        wtype = str(g[f"c{i}_window"])
        window = None if wtype == "none" else orm.get_window(freq, m, el, ew, float(g["latitude"]), wtype, exclude_cyl=excl)
        mode, wt = rt.maker_weights(kind, weight_ew, new, excl)
        T = rt.deconvolve_truth(hv, hw, bv, wt, mode, eps, nra, window, skip, int(np.argmin(np.abs(el))))
        for name, t in (("map", T["map"][np.newaxis]), ("wgt", np.repeat(T["weight"][:, :, np.newaxis, :], nra, axis=2)),
                        ("dbp", T["dirty_beam_power"][np.newaxis]), ("db", T["dirty_beam"][np.newaxis])):
            ref = g[f"c{i}_{name}"]
            assert t.shape == ref.shape, (i, name)
            if np.abs(ref).max() == 0:
                assert not t.any(), (i, name)
                continue
            assert np.abs(t - ref).max() / np.abs(ref).max() < 5e-6, (i, name)


def test_analytic_truth_against_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "ringmap_analytic.npz"))
    pol = [str(p) for p in g["pol"]]
    ca, cb = np.array([rt.BEAM_COEF[p[0]] for p in pol]), np.array([rt.BEAM_COEF[p[1]] for p in pol])
    for i in range(int(g["ncase"])):
        ref = g[f"c{i}_beam_m"]
        mmax = ref.shape[0] - 1
        nra = 2 * mmax + int(g[f"c{i}_oddra"])
        dec = np.arcsin(g[f"c{i}_el"]) + np.radians(float(g["latitude"]))
        Tr, Ti, _ = rt.analytic_beam_truth(g["freq"], g["ew"], dec, ca, cb, nra, mmax)
        assert Tr.shape == ref.shape
        assert np.abs((Tr + 1j * Ti).astype(np.complex128) - ref).max() < 2e-7 * np.abs(ref).max(), i


@pytest.mark.parametrize("shape", rt.BEAM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_analytic_beam_caps_hold_for_the_float64_restatement(shape):
    nra, mmax, nel, nfreq = shape
    inp = rt.beam_inputs(*shape)
    f64 = rt.analytic_beam_f64(*inp, nra, mmax)
    Tr, Ti, B = rt.analytic_beam_truth(*inp, nra, mmax)
    mismatch, loose, near, noise = rt.analytic_beam_measure(f64, Tr, Ti, B, nra)
    print(f"ringmap twin host beam {shape}: mismatch {mismatch} loose {loose} near {near:.3g} noise {noise:.3g}")
    assert mismatch == 0 and loose == 0 and near <= rt.EXCLUDED_CAP
    if mmax == nra // 2:  # the shapes the oracle's signature takes: its own output under the same measure
        own = orm.analytic_beam_mmodes(inp[0], inp[1], np.sin(inp[2]), rt.POLS, 0.0, mmax, nra % 2)
        mismatch, loose, near, noise = rt.analytic_beam_measure(own, Tr, Ti, B, nra)
        print(f"ringmap twin host beam {shape}, oracle.ringmap.analytic_beam_mmodes: mismatch {mismatch} loose {loose} near {near:.3g} noise {noise:.3g}")
        assert own.dtype == np.complex64 and mismatch == 0 and loose == 0 and near <= rt.EXCLUDED_CAP
    # the slots the pack leaves zero
    mlim, mneg = rt.pack_limits(nra, mmax)
    assert not Tr[mlim + 1 :, 0].any() and not Tr[0, 1].any() and not Tr[mneg + 1 :, 1].any() and Tr[:mlim + 1, 0].all()


@pytest.mark.parametrize("shape", rt.WINDOW_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(rt.WINDOW_COEF))
def test_window_caps_hold_for_the_float64_restatement(shape, name):
    nfreq, nm, nel = shape
    lo, hi = rt.window_limits(*shape)
    index = rt.window_index(*shape)
    coef = rt.WINDOW_COEF[name]
    mismatch, near = rt.window_measure(rt.window_f64(lo, hi, coef, nm, index), lo, hi, coef, nm, index)
    print(f"ringmap twin host window {shape} {name}: mismatch {mismatch} near {near:.3g}")
    assert mismatch == 0 and near <= rt.EXCLUDED_CAP
    T, _ = rt.window_truth(lo, hi, coef, nm, index)
    assert T.any() or nm == 1
    if nm == 17:  # integer limits: m == lo and m == hi are inside; hi < lo: empty
        full, _ = rt.window_truth(lo, hi, coef, nm)
        full = full.reshape(nfreq, nm, nel)
        assert not full[:, :, 1].any()
        if name == "uniform":
            assert full[0, 1, 0] == 1 and full[0, nm - 1, 0] == 1 and full[0, 0, 0] == 0  # lo = 1, hi = nm - 1
