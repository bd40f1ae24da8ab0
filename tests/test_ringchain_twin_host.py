"""CPU tests of ``tests/ringchain_twin.py``, the long-double truth of the ring-map chain producers' GPU tests
(``test_gpu_ringchain_direct.py``): the float64 restatements inside every acceptance bound at every shape of the sweeps,
the share of elements the rounded-once comparison leaves out, the twin against the oracle restatements of the
reference (``oracle/ringmap.py``), and two deliberately wrong restatements outside the bounds.

Measured here, ``error / bound`` of the float64 restatements on the committed inputs (at most 1 passes; ``-``: the case
has no dirty beam).  BeamformNS, as stored (float32) and before the store (float64, against the accumulation term
alone: ``B`` for ``hv`` and ``hb``, ``(2 ny + 8) 2**-52`` for ``hw``).  As stored the ratios approach 1 because the bound's
first term is the half unit of the float32 rounding itself; no element of any case differs from the truth rounded
once, and the share of components within ``B`` of a float32 rounding boundary is 4.7e-5 in case B, 6.0e-5 in case F and 0
in the others (the cap is 1e-3):

           as stored               before the store
    case   hv      hb      hw      hv / B   hb / B   hw
    A      0       0       0       0        0        0
    B      0.999   -       0.973   0.251    0.206    0.047
    C      0.995   0.990   0.934   0.119    0.051    0.083
    D      0.992   0.988   0.956   0.172    0.113    0.038
    E      0.928   -       0.834   0.165    0.069    0.049
    F      0.988   -       0.917   0.061    0.058    0.047
    G      0.997   0.993   0.999   0.252    0.211    0.146
    Z      0       0       0       0        0        0

(A is one term with weight 1, Z has no weight at all: both are exact.)  BeamformEW:

    case      map     dirty   weight  rms
    nbeam1    0       -       0       0.006
    nbeam3    0.123   0.119   0.075   0.053
    nbeam7    0.096   -       0.086   0.072
    nbeam9    0.089   0.104   0.109   0.071
    nbeam15   0.043   -       0.064   0.054
    single8   0       -       0.101   0.066
    single3   0.020   0.049   0.118   0.080

(single8: the natural weights of eight baselines, doubled beyond the first, sum to 64, so every product and partial sum
of the float32 inputs is exact in float64.)  The restatement that drops the last ``ns`` term is at 2e11 … 7e11 times the
bound with 85 … 90 % of its components not the truth rounded once.
"""

import numpy as np
import pytest

import ringchain_twin as rt
from oracle import ringmap as orm


@pytest.fixture(scope="module")
def ns_cases():
    return {k: rt.NsCase(s) for k, s in rt.NS_SWEEP.items()}


@pytest.fixture(scope="module")
def ew_cases():
    return {k: rt.EwCase(s) for k, s in rt.EW_SWEEP.items()}


def _share(got, T, B):
    """Worst ``|got - T| / B`` (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got).astype(rt.LD) - T)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, rt.LD(0), err / np.broadcast_to(B, T.shape)).max())


def test_vis_grid_exact_semantics():
    vis = np.array([[[1 + 2j, 3 - 4j], [5 + 6j, 7 + 8j]]], dtype=np.complex64)  # [1 freq][2 stacks][2 ra]
    w = np.array([[[1, 2], [3, 4]]], dtype=np.float32)
    red = np.array([[9, 8], [7, 6]], dtype=np.float32)
    gv, gw, gr = rt.vis_grid_exact(vis, w, red, [-1, 1, 1, 0], [1, 1, 0, 0], 2, 2)
    assert gv.shape == (2, 1, 2, 2) and gv.dtype == np.complex64 and gw.dtype == np.float32 and gr.dtype == np.int32
    assert np.array_equal(gv[:, 0], [[[0, 0], [5 - 6j, 7 - 8j]], [[5 + 6j, 7 + 8j], [1 + 2j, 3 - 4j]]])
    assert np.array_equal(gw[:, 0], [[[0, 0], [3, 4]], [[3, 4], [1, 2]]]) and np.array_equal(gr, [[[0, 0], [7, 6]], [[7, 6], [9, 8]]])


def test_long_double_is_wider():
    """The truths need a type with more than float64's 53 bits (x87 extended: 64)."""
    assert np.finfo(rt.LD).nmant >= 63


# ---- the float64 restatements inside the bounds
@pytest.mark.parametrize("name", list(rt.NS_SWEEP))
def test_ns_reference_inside_bounds(ns_cases, name):
    c = ns_cases[name]
    hv, hb, hw = c.reference()
    m = c.check(f"{name} float64", hv, hw, hb if c.dirty else None)
    # before the store: the share of B, the accumulation term alone, that the float64 restatement uses
    hv64, hb64, hw64 = c.reference(store=False)
    acc = max(_share(hv64.real, c.T.real, c.B), _share(hv64.imag, c.T.imag, c.B))
    acc_b = _share(hb64, c.Tb, c.Bb)
    acc_w = rt.relative_measure(hw64, c.hw)[0] / ((2 * c.ny + 8) * 2.0**-52)
    print(f"ringchain ns {name} float64 before the store: hv / B {acc:.3g} hb / B {acc_b:.3g} hw / ((2 ny + 8) 2**-52) {acc_w:.3g}")
    assert acc <= 1.0 and acc_b <= 1.0 and acc_w <= 1.0
    # the truth's own share of elements near a rounding boundary is a condition on the inputs, not on the code
    assert m["hv_excluded"] <= rt.EXCLUDED_CAP and m.get("hb_excluded", 0.0) <= rt.EXCLUDED_CAP
    if name == "Z":
        assert not hv.any() and not hb.any() and not hw.any() and not c.T.any() and not c.hw.any()
    else:
        assert c.T.any() and c.hw.any()


def test_ns_case_properties(ns_cases):
    """The inputs are what the sweep says: a tenth of the weights masked, negative weights among them, one dead column."""
    for name, c in ns_cases.items():
        assert c.gv.dtype == np.complex64 and c.gw.dtype == np.float32 and c.gr.dtype == np.int32
        assert c.nspos.dtype == c.el.dtype == c.iwv.dtype == np.float64 and c.nspos[0] == 0.0
        assert 0 <= c.gr.min() and c.gr.max() <= 19
        if c.gw.size >= 64:
            assert 0.05 <= np.mean(c.gw <= 0) <= 0.2 and (c.gw < 0).any(), name
        if c.masked:
            p, x, t = c.masked
            assert not (c.gw[p, :, x, :, t] > 0).any() and not c.T[p, :, x, :, t].any() and not c.hw[p, :, x, t].any()
        assert (c.table is not None) == (c.mode == rt.WINDOW)
    b, p = ns_cases["B"], rt.NsCase(rt.NS_POISON)
    pad = lambda c: c.npol * c.nx * (-(-c.ny // 16) * 16) * (-(-c.nra // 64) * 64)  # elements of the xw scratch
    assert pad(p) >= pad(b) and -(-p.npix // 64) == -(-b.npix // 64) and -(-p.ny // 16) == -(-b.ny // 16)
    assert p.ny % 16 == 0 and p.nra % 64 == 0


@pytest.mark.parametrize("name", list(rt.EW_SWEEP))
def test_ew_reference_inside_bounds(ew_cases, name):
    c = ew_cases[name]
    rmap, weight, rms, rdb = c.reference()
    assert rmap.shape == (c.nbeam, c.npol_out, c.nfreq, c.nra, c.nel) and c.T.any()
    c.check(f"{name} float64", rmap, weight, rms, rdb)


def test_ew_case_properties(ew_cases):
    kinds = {c.shape[7] for c in ew_cases.values()}
    assert kinds == {"natural", "uniform"}
    assert sum(bool(c.shape[8]) for c in ew_cases.values()) >= 2 and all(c.w[0] == 0 for c in ew_cases.values() if c.shape[8])
    flagged = [c for c in ew_cases.values() if c.shape[9] is not None]
    assert len(flagged) == 1 and flagged[0].w[2] == 0 and flagged[0].w[1] > 0 and flagged[0].w[3] > 0
    assert sorted(c.nbeam for c in ew_cases.values()) == [1, 1, 1, 3, 7, 9, 15]
    for c in ew_cases.values():
        assert abs(c.w.sum() - 1.0) < 1e-15 and np.count_nonzero(c.P, axis=1).max() <= 2
        if c.dead is not None:
            assert not c.rv[:, :, c.dead].any() and c.rv.any()
        if c.hw.size >= 64:
            assert 0.05 <= np.mean(c.hw == 0) <= 0.25


# ---- the twin against the oracle's restatements of the reference
@pytest.mark.parametrize("name", ["B", "D"])
def test_ns_twin_against_the_oracle(ns_cases, name):
    c = ns_cases[name]
    weight = {rt.INV_VAR: "inverse_variance", rt.NATURAL: "natural"}[c.mode]
    hv, hw, hb, el, _ = orm.beamform_ns(c.gv, c.gw, c.gr, c.nspos, c.freq, npix=c.npix, span=0.95, weight=weight, include_auto=bool(c.include_auto), precision=64)
    assert np.array_equal(el, c.el)
    t = c.T.astype(np.complex128)
    # (the oracle, like the reference, forms the weights in float32 before its float64 product)
    assert np.abs(hv - t).max() < 3e-6 * np.abs(t).max()
    assert np.abs(hb - c.Tb.astype(np.float64)).max() < 3e-6 * float(np.abs(c.Tb).max())
    assert np.allclose(hw, c.hw.astype(np.float64), rtol=3e-6, atol=0)


@pytest.mark.parametrize("name", ["nbeam3", "nbeam7", "single8"])
def test_ew_twin_against_the_oracle(ew_cases, name):
    c = ew_cases[name]
    pols, _, _, _, _, single, dirty, weight_ew, excl, flag = c.shape
    rmm, rmw, rmr, pol, rmb = orm.beamform_ew(c.hv, c.hw, pols, exclude_intracyl=excl, single_beam=single, weight_ew=weight_ew, flag_ew=flag, dirty_beam=c.hb)
    assert list(pol) == list(c.pol_out)
    t = c.T.astype(np.float64)
    # (the oracle, like the reference, rotates the polarisations in complex64)
    assert np.abs(rmm - t).max() < 1e-6 * np.abs(t).max()
    assert np.allclose(rmw, rt.invert_no_zero(c.rv).astype(np.float64)[..., np.newaxis], rtol=1e-6, atol=0)
    assert np.allclose(rmr, np.sqrt(c.rv).astype(np.float64), rtol=1e-6, atol=0)
    if dirty:
        assert np.abs(rmb - c.Tb.astype(np.float64)).max() < 1e-6 * float(np.abs(c.Tb).max())


@pytest.mark.parametrize("all_good", [0, 1])
def test_redundancy_twin_against_the_oracle(all_good):
    flags, pa, pb, stack = rt.redundancy_case(23, 63, all_good)
    pa[5], pb[17] = 1, 4  # (the oracle's loop has no rule for an input outside the flag table)
    got = rt.redundancy_exact(flags, pa, pb, stack, rt.GRID_NSTACK, all_good)
    assert np.array_equal(got, orm.calculate_redundancy(flags, list(zip(pa, pb)), stack, rt.GRID_NSTACK)) and got.any()


def test_redundancy_skips():
    """What the oracle has no rule for: a product with an input outside the table counts with ``all_good`` only."""
    flags, pa, pb, stack = rt.redundancy_case(23, 5, 0)
    flags[:] = 1
    ok = (stack >= 0) & (stack < rt.GRID_NSTACK)
    want = np.bincount(stack[ok], minlength=rt.GRID_NSTACK)
    assert np.array_equal(rt.redundancy_exact(flags, pa, pb, stack, rt.GRID_NSTACK, 1)[:, 0], want)
    want[2] -= 2
    assert np.array_equal(rt.redundancy_exact(flags, pa, pb, stack, rt.GRID_NSTACK, 0)[:, 0], want)


@pytest.mark.parametrize("ncyl,nfeed_cyl,nfreq,nra", [(2, 3, 2, 5), (3, 4, 1, 9)])
def test_vis_grid_twin_against_the_oracle(ncyl, nfeed_cyl, nfreq, nra):
    """The gather, driven by the cell tables ``MakeVisGrid.process`` builds, is the oracle's scatter."""
    from draco_amd.analysis.ringmapmaker import find_grid_indices
    from draco_amd.core.products import TransitTelescope

    rng = np.random.default_rng([ncyl, nfeed_cyl])
    tel = TransitTelescope(np.linspace(450.0, 750.0, nfreq), lmax=4, ncyl=ncyl, nfeed_cyl=nfeed_cyl, pair_rule="halfplane")
    nstack = tel.npairs
    vis = (rng.standard_normal((nfreq, nstack, nra)) + 1j * rng.standard_normal((nfreq, nstack, nra))).astype(np.complex64)
    w = rng.uniform(0.5, 1.5, (nfreq, nstack, nra)).astype(np.float32)
    flags = (rng.uniform(size=(tel.nfeed, nra)) > 0.2).astype(np.float32)
    pa, pb = tel.index_map_prod["input_a"].astype(np.int32), tel.index_map_prod["input_b"].astype(np.int32)
    stack = np.asarray(tel.reverse_map_stack["stack"], dtype=np.int32)
    pairs = np.stack([tel.prodstack["input_a"].astype(int), tel.prodstack["input_b"].astype(int)], axis=1)
    gv, gw, gr, pol, _, _ = orm.make_vis_grid(vis, w, pairs, tel.polarisation, tel.baselines, flags, list(zip(pa, pb)), stack)
    red = rt.redundancy_exact(flags, pa, pb, stack, nstack, 0)
    assert np.array_equal(red, orm.calculate_redundancy(flags, list(zip(pa, pb)), stack, nstack))
    # the cell tables, as MakeVisGrid.process inverts the reference's scatter loop (FFT order along ns)
    polprod = np.asarray(tel.polarisation)[pairs]
    _, pind = np.unique(np.char.add(polprod[:, 0], polprod[:, 1]), return_inverse=True)
    pconjmap = np.unique([b + a for a, b in pol], return_inverse=True)[1]
    xind, yind, _, _ = find_grid_indices(tel.baselines)
    nx, ny = gv.shape[2], gv.shape[3]
    src, conj = np.full(4 * nx * ny, -1, dtype=np.int32), np.zeros(4 * nx * ny, dtype=np.uint8)
    for vi, (p_, x_, y_) in enumerate(zip(pind, xind, yind)):
        cell = (p_ * nx + x_ % nx) * ny + y_ % ny
        src[cell], conj[cell] = vi, 0
        if x_ == 0:
            cellc = (pconjmap[p_] * nx + x_) * ny + (-y_) % ny
            src[cellc], conj[cellc] = vi, 1
    tv, tw, tr = rt.vis_grid_exact(vis, w, red, src, conj, 4, nx * ny)
    assert conj.any() and len(np.unique(src)) < len(src)  # (a full grid: every cell has a stack, the intra-cylinder ones two)
    assert np.array_equal(tv.reshape(gv.shape), gv) and np.array_equal(tw.reshape(gw.shape), gw) and np.array_equal(tr.reshape(gr.shape), gr)
    assert rt.vis_grid_exact(vis, w, None, src, conj, 4, nx * ny)[2] is None


# ---- the measures have teeth
def test_ns_bound_catches_a_dropped_term(ns_cases):
    """A restatement that leaves the last ``ns`` term out of the product (the weights as they should be) is far outside
    the inequality, and most of its elements are not the truth rounded once."""
    for name in ("B", "D", "F"):
        c = ns_cases[name]
        gv = c.gv.copy()
        gv[:, :, :, -1, :] = 0
        per = [rt.beamform_ns_f64(gv[:, f], c.gw[:, f], c.gr, None if c.table is None else c.table[f], c.nspos, c.el, c.iwv[f], c.mode, c.include_auto)
               for f in range(c.nfreq)]
        hv, hw = np.stack([p[0] for p in per], axis=1), np.stack([p[2] for p in per], axis=1)
        m = c.measure(hv, hw)
        assert m["hv"] > 1e3 and m["hv_mismatch"] > 0.5 * hv.size, (name, m)
        with pytest.raises(AssertionError):
            c.check(f"{name} dropped term", hv, hw)


def test_ns_bound_catches_float_twiddles(ns_cases):
    """``F`` rounded to float32 is an error of 6e-8 of each term, the size of the one rounding the inequality allows the
    store: it is the rounded-once comparison that catches it."""
    c = ns_cases["F"]
    w = rt._ns_weights(c.gw[:, 0], c.gr, c.table[0], c.mode, c.include_auto, np.float64)
    w = w * rt.invert_no_zero(w.sum(axis=2, keepdims=True))
    F = np.exp(-2.0j * np.pi * c.nspos[np.newaxis, :] * c.el[:, np.newaxis] * c.iwv[0]).astype(np.complex64).astype(np.complex128)
    hv = np.matmul(F, c.gv[:, 0] * w).astype(np.complex64)[:, np.newaxis]
    m = c.measure(hv, c.reference()[2])
    assert m["hv_mismatch"] > 0.25 * hv.size and m["hw"] <= 1.0, m


def test_ew_bound_catches_a_wrong_factor(ew_cases):
    """``fac = w_x`` on every EW baseline instead of ``2 w_x`` beyond the first; and the right sum passes."""
    for name in ("nbeam3", "nbeam9", "nbeam15"):
        c = ew_cases[name]
        v = np.tensordot(c.P, c.hv.astype(np.complex128), axes=(1, 0))  # [pol][freq][x][el][ra]
        ang = 2.0 * np.pi * (np.outer(np.arange(c.nx), np.arange(c.nbeam)) % c.nbeam) / c.nbeam
        tw = np.exp(1j * ang)
        for wrong in (False, True):
            fac = np.where((np.arange(c.nx) == 0) | wrong, c.w, 2.0 * c.w)
            rmap = np.einsum("x,pfxet,xb->bpfte", fac, v, tw).real
            ratio = rt.ew_measure(c.nx, c.T, c.A, c.rv, rmap)["map"]
            assert ratio > 1e6 if wrong else ratio <= 1.0, (name, wrong, ratio)


def test_ew_variance_bound_catches_a_float_weight(ew_cases):
    """The variance formed in float32: outside ``(nx + 8) 2**-52`` by many orders."""
    c = ew_cases["nbeam9"]
    _, weight, rms, _ = c.reference()
    m = rt.ew_measure(c.nx, c.T, c.A, c.rv, None, weight.astype(np.float32).astype(np.float64), rms)
    assert m["weight"] > 1e5 and m["rms"] <= 1.0 and m["weight_zeros"]


def test_rounded_measure_edges():
    """``rounded_measure`` itself: an element one float32 step off is a mismatch; a truth that sits on a rounding
    boundary is left out of the bit comparison and kept in the inequality; NaN never passes."""
    T = np.array([1.0, 1.0 + 2.0**-24, 0.0, -3.0], dtype=rt.LD)  # T[1]: halfway between 1 and 1 + 2**-23
    B = np.array([2.0**-50, 2.0**-50, 0.0, 2.0**-50], dtype=rt.LD)
    good = np.array([1.0, 1.0 + 2.0**-23, 0.0, -3.0], dtype=np.float32)
    ratio, mism, excl = rt.rounded_measure(good, T, B)
    assert ratio <= 1.0 and mism == 0 and excl == 0.25
    off = good.copy()
    off[0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    ratio, mism, _ = rt.rounded_measure(off, T, B)
    assert ratio > 1.0 and mism == 1
    off = good.copy()
    off[2] = 1e-30
    assert rt.rounded_measure(off, T, B)[0] == np.inf
    off[2] = np.nan
    assert rt.rounded_measure(off, T, B)[0] == np.inf
