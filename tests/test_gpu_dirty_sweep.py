"""Shape sweep of ``csrc/solve_dirty.hip`` at the C ABI against the long-double reference of ``tests/dirty_twin.py``.

Tile tables and random pools are made by hand (no provider, no telescope), so every shape-dependent path of ``k_dirty``
(one day and 8 / 4 / 2 days per launch) and ``k_project`` / ``k_project_rg`` is placed on purpose: rows below / on / above multiples of the
pipelined loop's ``kUnroll``, one or two columns per lane, both layouts, the 8/4/2/1-day groups, row groups of 8 inside
64-row tasks, ticket and static task hand-out, every tuning variant the timing tools switch on.

Every output buffer starts as the sentinel 7+7j; every pool byte that is not a tile element (gaps, tails, the l < m columns
of full-layout tiles) is NaN, and so is every ``alm`` input the projection must not read.  After each launch
``dirty_twin.check_launch`` asserts: values by the acceptance rule (``dirty_twin.accept``), exact structural zeros,
untouched sentinels outside the tile list, no NaN.

The acceptance figure is taken over everything one launch computes: every tile of a plan has the same ``ntel`` and
entries of the same distribution, so all outputs of a launch are of one scale.

Largest ``e_gpu / e_twin`` and largest fraction of the rigorous bound seen on an MI355X over this module (limits: 4 and 1):
dirty complex128 1.46 / 0.22, dirty complex64 1.61 / 0.13, multi-day 1.40 / 0.017, project complex128 1.61 / 0.080, project
complex64 1.36 / 0.096.  The module prints them when it ends (``-s``) and writes them to the file ``DIRTY_SWEEP_STATS`` names.
"""

import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import dirty_twin as dt

pytestmark = pytest.mark.gpu

KINDS = ("c128", "c64p", "c64u")  # complex128; complex64 on the paired 16-byte path; complex64 dropped to one column per lane
STATS = {}  # family -> [largest e_gpu / e_twin, largest fraction of the rigorous bound, launches]


def _note(family, st):
    s = STATS.setdefault(family, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], st["ratio"]), max(s[1], st["frac"]), s[2] + 1


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for plan in _PLANS:
        plan.close()
    _PLANS.clear()
    _multi_setup.cache_clear()
    _many_tiles.cache_clear()
    print("\ndirty sweep: family: max e_gpu/e_twin, max fraction of the rigorous bound, launches")
    for fam in sorted(STATS):
        print(f"  {fam}: {STATS[fam][0]:.3f} {STATS[fam][1]:.3e} {STATS[fam][2]}")
    path = os.environ.get("DIRTY_SWEEP_STATS")
    if path:
        with open(path, "w") as fh:
            json.dump(STATS, fh, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI by hand


def _ctx():
    from draco_amd.device import Context

    return Context.get()


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).to(_ctx().device)


def _filled(shape, value=dt.SENTINEL):
    import torch

    return torch.full(tuple(shape), value, dtype=torch.complex128, device=_ctx().device)


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


_PLANS = []


class Plan:
    """``dmm_solve_plan_create`` for a :class:`dirty_twin.Case` + its pool on the device."""

    def __init__(self, case, tail=0, keep=False):
        from draco_amd import _lib
        from draco_amd.device import ptr

        self.case, self.lib, self.ptr, self.check = case, _lib.lib, ptr, _lib.check
        ms, fs, offs = case.tile_table()
        h = C.c_void_p()
        _lib.check(_lib.lib.dmm_solve_plan_create(_ctx().handle, _lib.tile_array(ms, fs, offs), len(ms), case.npairs, case.npol, case.lmax,
                                                  case.nfreq, case.n_m, case.b_dtype, case.b_layout, C.byref(h)))
        self.h = h
        self.pool_h = case.pool(tail)
        self.pool = _dev(self.pool_h)
        if keep:
            _PLANS.append(self)

    def close(self):
        if self.h:
            self.lib.dmm_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def dirty(self, mvis_d, mw_d):
        alm = _filled(self.case.alm_shape())
        self.check(self.lib.dmm_dirty_run(self.h, self.ptr(self.pool), self.ptr(mvis_d), self.ptr(mw_d), self.ptr(alm)))
        return _host(alm)

    def dirty_multi(self, mvis_l, mw_l):
        D = len(mvis_l)
        alms = [_filled(self.case.alm_shape()) for _ in range(D)]
        PA = C.c_void_p * D
        pv, pw, pa = PA(*[self.ptr(x) for x in mvis_l]), PA(*[self.ptr(x) for x in mw_l]), PA(*[self.ptr(x) for x in alms])
        self.check(self.lib.dmm_dirty_run_multi(self.h, self.ptr(self.pool), pv, pw, pa, D))
        return [_host(a) for a in alms]

    def project(self, alm_d):
        vis = _filled(self.case.vis_shape())
        self.check(self.lib.dmm_project_run(self.h, self.ptr(self.pool), self.ptr(alm_d), self.ptr(vis)))
        return _host(vis)

    def pool_unchanged(self):
        return np.array_equal(_host(self.pool).view(np.uint8), self.pool_h.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# cases


def _kind(kind):
    """``(b_dtype, wants an odd b_off)`` of a storage kind."""
    return (dt.C128 if kind == "c128" else dt.C64), kind == "c64u"


def make_case(rng, npairs, npol, lmax, nfreq, n_m, mf, kind="c128", b_layout=dt.PACKED, shuffle=True, gaps=None):
    """A case over the (m, f) list ``mf``: random tiles, placed in a shuffled order with gaps.  ``kind`` "c64u" puts one
    tile on an odd ``b_off`` (which drops the whole plan to one column per lane), every other kind keeps all of them even."""
    b_dtype, odd = _kind(kind)
    ms = [m for m, _ in mf]
    n = len(ms)
    if gaps is None:
        gaps = [2 * int(g) for g in rng.integers(0, 4, n)]
    if odd and n:
        gaps = list(gaps)
        gaps[n // 2] += 1
    order = rng.permutation(n) if shuffle else None
    offs = dt.layout_tiles(ms, npairs, npol, lmax, b_layout, gaps=gaps, order=order)
    if odd and n:  # (tiles placed behind the odd one are odd too unless the padding evens them out: at least one is)
        assert any(o & 1 for o in offs)
    else:
        assert not any(o & 1 for o in offs)
    Bs = [dt.random_tile(rng, 2 * npairs, npol, lmax + 1 - m, b_dtype) for m in ms]
    return dt.Case(npairs, npol, lmax, nfreq, n_m, [(m, f, o) for (m, f), o in zip(mf, offs)], Bs, b_dtype, b_layout)


def paired(case):
    """What ``dmm_solve_plan_create`` decides (``pair_ok``): two columns per lane."""
    return case.b_dtype == dt.C64 and case.b_layout == dt.PACKED and case.npol % 2 == 0 and all(o % 2 == 0 for _, _, o in case.tiles)


def make_data(rng, case, zero_frac=0.1, zero_baseline=None, zero_mf=None):
    """``mvis, mweight [n_m, 2, nfreq, npairs]``: ``zero_frac`` of the weights zero, optionally one baseline and one whole
    (m, f) on top."""
    shape = case.vis_shape()
    mvis = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    mw = rng.uniform(0.5, 1.5, shape)
    mw[rng.uniform(size=shape) < zero_frac] = 0.0
    if zero_baseline is not None:
        mw[..., zero_baseline] = 0.0
    if zero_mf is not None:
        mw[zero_mf[0], :, zero_mf[1], :] = 0.0
    return mvis, mw


def make_alm_in(rng, case):
    """Input of the projection: random where a listed tile reads it, NaN everywhere else (l < m, other (m, f))."""
    alm = np.full(case.alm_shape(), np.nan + 1j * np.nan, dtype=np.complex128)
    for m, f, _ in case.tiles:
        shape = (case.npol, case.lmax + 1 - m)
        alm[f, :, m, m:] = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return alm


def dirty_family(case):
    return "dirty c128" if case.b_dtype == dt.C128 else "dirty c64"


def project_family(case):
    return "project c128" if case.b_dtype == dt.C128 else "project c64"


def check_dirty(plan, rng, what, **data_kw):
    case = plan.case
    mvis, mw = make_data(rng, case, **data_kw)
    got = plan.dirty(_dev(mvis), _dev(mw))
    st = dt.check_launch(got, case.expected_alm(mvis, mw), what=what)
    _note(dirty_family(case), st)
    return got, (mvis, mw)


def check_project(plan, rng, what):
    case = plan.case
    alm = make_alm_in(rng, case)
    got = plan.project(_dev(alm))
    st = dt.check_launch(got, case.expected_vis(alm), what=what)
    _note(project_family(case), st)
    return got, alm


# ---------------------------------------------------------------------------------------------------------------------
# k_dirty: rows

ROW_NPAIRS = (1, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 28, 31, 32, 33, 40, 41)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("npairs", ROW_NPAIRS)
def test_dirty_row_regimes(npairs, kind):
    """ntel = 2 npairs below, on and above 1x .. 5x kUnroll for kUnroll 8 (complex128, unpaired complex64) and 16 (paired
    complex64): every exit of the pipelined loop and the tail behind each."""
    rng = np.random.default_rng(1000 + npairs)
    mf = [(0, 0), (7, 1), (20, 0), (13, 1), (7, 0), (19, 1)]
    case = make_case(rng, npairs, 2, 20, 2, 21, mf, kind)
    assert paired(case) == (kind == "c64p")
    with Plan(case, tail=5) as plan:
        check_dirty(plan, rng, f"dirty npairs={npairs} {kind}", zero_mf=(13, 1))
        assert plan.pool_unchanged()


# ---------------------------------------------------------------------------------------------------------------------
# k_dirty: columns

COL_EDGES = (64, 128, 256, 512)


def _edge_Ls(edge, npol):
    """L = lmax + 1 - m with ncol = npol * L just below, on (or just above) and above ``edge``."""
    return sorted({max((edge - 1) // npol, 1), -(-edge // npol), -(-(edge + 1) // npol), edge // npol + 1})


@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64], ids=["c128", "c64"])
@pytest.mark.parametrize("b_layout", [dt.PACKED, dt.FULL], ids=["packed", "full"])
@pytest.mark.parametrize("npol", [1, 2, 3, 4])
@pytest.mark.parametrize("edge", COL_EDGES)
def test_dirty_column_regimes(edge, npol, b_layout, b_dtype):
    """ncol = npol L on each side of one lane / one wave (1, 63-65), one paired wave (127-129), one block (255-257), one paired
    block (511-513), and the last tile m = lmax (L = 1).  Edge 64 carries L = 1 and an ``alm`` with more m rows than any
    tile uses; the others have n_m < lmax + 1."""
    rng = np.random.default_rng(2000 + edge * 10 + npol)
    Ls = _edge_Ls(edge, npol) + ([1] if edge == 64 else [])
    lmax = max(Ls) + 2
    Ls = sorted(set(Ls))
    mf = [(lmax + 1 - L, k % 2) for k, L in enumerate(Ls)]
    n_m = lmax + 4 if edge == 64 else max(m for m, _ in mf) + 1
    assert edge == 64 or n_m < lmax + 1
    ncols = {npol * L for L in Ls}
    assert min(ncols) < edge <= max(ncols) and any(c > edge for c in ncols) and any(edge <= c <= edge + npol - 1 for c in ncols)
    case = make_case(rng, 9, npol, lmax, 2, n_m, mf, "c128" if b_dtype == dt.C128 else "c64p", b_layout)
    assert paired(case) == (b_dtype == dt.C64 and b_layout == dt.PACKED and npol % 2 == 0)
    with Plan(case, tail=3) as plan:
        what = f"edge={edge} npol={npol} layout={b_layout} dtype={b_dtype} L={Ls}"
        check_dirty(plan, rng, "dirty " + what)
        check_project(plan, rng, "project " + what)
        assert plan.pool_unchanged()


@pytest.mark.parametrize("npol", [1, 2, 3, 4])
def test_dirty_one_column_per_polarisation(npol):
    """lmax = 0: every tile is m = 0 with ONE column per polarisation (ncol = npol <= 4, one lane or two)."""
    rng = np.random.default_rng(2100 + npol)
    for kind in KINDS:
        case = make_case(rng, 5, npol, 0, 3, 1, [(0, 0), (0, 2), (0, 1)], kind)
        with Plan(case) as plan:
            check_dirty(plan, rng, f"lmax=0 npol={npol} {kind}")
            check_project(plan, rng, f"lmax=0 npol={npol} {kind}")


# ---------------------------------------------------------------------------------------------------------------------
# pairing


@pytest.mark.parametrize("npairs", [5, 20, 33])
def test_pairing_even_offsets_pair_one_odd_offset_does_not(npairs):
    """The same complex64 tiles at all-even ``b_off`` (16-byte loads, two columns per lane), with one odd ``b_off``, and with
    odd npol: all pass the same rule.  Every column's rows are added in ascending order by the same chain of fused
    multiply-adds whichever lane owns it, so paired and unpaired results are bit-identical."""
    rng = np.random.default_rng(3000 + npairs)
    mf = [(0, 0), (5, 1), (30, 1), (17, 0)]
    even = make_case(rng, npairs, 2, 30, 2, 31, mf, "c64p", shuffle=False, gaps=[0, 2, 4, 0])
    offs = [o + (1 if k >= 2 else 0) for k, (_, _, o) in enumerate(even.tiles)]
    odd = dt.Case(npairs, 2, 30, 2, 31, [(m, f, o) for (m, f), o in zip(mf, offs)], even.Bs, dt.C64, dt.PACKED)
    assert paired(even) and not paired(odd)
    mvis, mw = make_data(rng, even)
    outs = []
    for case in (even, odd):
        with Plan(case, tail=4) as plan:
            got = plan.dirty(_dev(mvis), _dev(mw))
            _note("dirty c64", dt.check_launch(got, case.expected_alm(mvis, mw), what=f"pairing npairs={npairs} paired={paired(case)}"))
            outs.append(got)
    assert np.array_equal(outs[0], outs[1])
    case3 = make_case(rng, npairs, 3, 30, 2, 31, mf, "c64p")
    assert not paired(case3)
    with Plan(case3) as plan:
        check_dirty(plan, rng, f"pairing npairs={npairs} npol=3")


# ---------------------------------------------------------------------------------------------------------------------
# tile tables


@pytest.mark.parametrize("b_layout", [dt.PACKED, dt.FULL], ids=["packed", "full"])
@pytest.mark.parametrize("kind", KINDS)
def test_tile_table_shuffled_repeated_m_gaps(kind, b_layout):
    """Table order unrelated to pool order, the same m under several f, non-monotonic ``b_off`` with gaps; (m, f) pairs that
    are not listed keep the sentinel."""
    rng = np.random.default_rng(4000)
    mf = [(9, 2), (0, 1), (44, 0), (9, 0), (31, 2), (0, 2), (44, 1), (9, 1), (2, 0)]
    case = make_case(rng, 13, 4, 44, 3, 47, mf, kind, b_layout)
    offs = [o for _, _, o in case.tiles]
    assert offs != sorted(offs)
    with Plan(case, tail=7) as plan:
        check_dirty(plan, rng, f"table {kind} layout={b_layout}", zero_baseline=4)
        check_project(plan, rng, f"table {kind} layout={b_layout}")
        assert plan.pool_unchanged()


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_tasks_than_cus(kind):
    rng = np.random.default_rng(4100)
    case = make_case(rng, 30, 2, 11, 1, 12, [(3, 0)], kind)
    with Plan(case) as plan:
        check_dirty(plan, rng, f"one task {kind}")
        check_project(plan, rng, f"one task {kind}")


@functools.lru_cache(maxsize=None)
def _many_tiles(kind):
    """61 m x 64 frequencies = 3904 small tiles: each block draws many tickets, ``find_tile`` searches 12 levels deep."""
    rng = np.random.default_rng(4200)
    mf = [(m, f) for f in range(64) for m in range(61)]
    mf = [mf[k] for k in rng.permutation(len(mf))]
    case = make_case(rng, 3, 2, 60, 64, 61, mf, kind)
    mvis, mw = make_data(rng, case)
    return case, mvis, mw, case.expected_alm(mvis, mw)


@pytest.mark.parametrize("kind", ["c128", "c64p"])
def test_several_thousand_small_tiles(kind):
    case, mvis, mw, exp = _many_tiles(kind)
    assert len(case.tiles) == 3904
    with Plan(case) as plan:
        got = plan.dirty(_dev(mvis), _dev(mw))
        _note(dirty_family(case), dt.check_launch(got, exp, what=f"3904 tiles {kind}"))
        with _ctx().options(dirty_static=1):  # static striding over the same table: same sums, same bits
            assert np.array_equal(plan.dirty(_dev(mvis), _dev(mw)), got)
        with _ctx().options(grid_mult=8):
            assert np.array_equal(plan.dirty(_dev(mvis), _dev(mw)), got)
        check_project(plan, np.random.default_rng(4201), f"3904 tiles {kind}")


def test_empty_plan_writes_nothing():
    rng = np.random.default_rng(4300)
    case = dt.Case(4, 2, 6, 2, 7, [], [], dt.C128, dt.PACKED)
    with Plan(case, tail=16) as plan:
        mvis, mw = make_data(rng, case)
        assert np.all(plan.dirty(_dev(mvis), _dev(mw)) == dt.SENTINEL)
        assert all(np.all(a == dt.SENTINEL) for a in plan.dirty_multi([_dev(mvis)] * 3, [_dev(mw)] * 3))
        assert np.all(plan.project(_dev(make_alm_in(rng, case))) == dt.SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------
# weights


@pytest.mark.parametrize("kind", KINDS)
def test_weight_patterns(kind):
    """10 % zeros, one baseline zero throughout, one (m, f) all zero: that tile's ``alm`` is exactly zero (checked by the
    rule: reference and bound are zero there), nothing turns NaN."""
    rng = np.random.default_rng(5000)
    mf = [(0, 0), (3, 1), (12, 0), (25, 1), (12, 1)]
    case = make_case(rng, 21, 4, 25, 2, 26, mf, kind)
    with Plan(case) as plan:
        got, _ = check_dirty(plan, rng, f"weights {kind}", zero_frac=0.1, zero_baseline=7, zero_mf=(12, 0))
        assert np.all(got[0, :, 12, :] == 0)
        got, (_, mw) = check_dirty(plan, rng, f"weights all zero {kind}", zero_frac=1.0)  # (the bound is zero: exact zeros or failure)
        assert not mw.any() and not got[got != dt.SENTINEL].any()


# ---------------------------------------------------------------------------------------------------------------------
# full size


@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64], ids=["c128", "c64"])
@pytest.mark.parametrize("npairs,lmax,m", [(379, 512, 0), (379, 512, 511), (763, 1024, 0)], ids=["cfg3-m0", "cfg3-m511", "cfg4-m0"])
def test_full_size_single_tile(npairs, lmax, m, b_dtype):
    """One tile at the size the benchmark runs (cfg 3: 758 x 2052, cfg 4: 1526 x 4100), Dirty and projection."""
    rng = np.random.default_rng(6000 + npairs + m)
    case = make_case(rng, npairs, 4, lmax, 1, m + 1, [(m, 0)], "c128" if b_dtype == dt.C128 else "c64p")
    with Plan(case) as plan:
        check_dirty(plan, rng, f"full size npairs={npairs} lmax={lmax} m={m} dtype={b_dtype}")
        check_project(plan, rng, f"full size project npairs={npairs} lmax={lmax} m={m} dtype={b_dtype}")


@pytest.mark.parametrize("kind", KINDS)
def test_lds_limit_npairs_3072(kind):
    """w = Ni o v of 6144 rows fills the 96 KiB the plan allows; one more baseline is refused."""
    rng = np.random.default_rng(6100)
    case = make_case(rng, 3072, 2, 8, 1, 9, [(0, 0), (8, 0), (5, 0)], kind)
    with Plan(case) as plan:
        check_dirty(plan, rng, f"npairs=3072 {kind}")
    over = dt.Case(3073, 2, 8, 1, 9, [], [], case.b_dtype, dt.PACKED)
    with pytest.raises(ValueError, match="too large for the LDS stage"):
        Plan(over)


# ---------------------------------------------------------------------------------------------------------------------
# k_dirty, several days per launch (dmm_dirty_run_multi)

MULTI_D = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16)
MULTI_NPAIRS = (23, 512, 513, 763, 1024, 1025, 2048, 2049)


@functools.lru_cache(maxsize=None)
def _multi_setup(npairs, kind):
    """Per (npairs, kind): the plan, 16 days of data (each its own values and zero pattern; one baseline zero on every day; one
    (m, f) all zero on one day only), every day's own ``dmm_dirty_run`` and its expected values."""
    rng = np.random.default_rng(7000 + npairs)
    if npairs <= 512:
        case = make_case(rng, npairs, 4, 70, 2, 71, [(0, 0), (33, 1), (70, 0), (2, 1)], kind) if npairs < 100 else \
            make_case(rng, npairs, 2, 20, 2, 21, [(0, 0), (20, 1), (9, 1)], kind)
    else:  # narrow tiles
        case = make_case(rng, npairs, 2, 8, 2, 9, [(0, 1), (8, 0), (3, 0)], kind)
    plan = Plan(case, tail=2, keep=True)
    days = []
    for d in range(max(MULTI_D)):
        m0, f0, _ = case.tiles[d % len(case.tiles)]
        days.append(make_data(rng, case, zero_frac=0.04 + 0.02 * d, zero_baseline=npairs // 2, zero_mf=(m0, f0) if d in (1, 6, 12) else None))
    dev = [(_dev(v), _dev(w)) for v, w in days]
    single = [plan.dirty(v, w) for v, w in dev]
    exp = case.expected_alm_days([v for v, _ in days], [w for _, w in days])
    return plan, dev, single, exp


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("npairs", MULTI_NPAIRS)
@pytest.mark.parametrize("D", MULTI_D)
def test_dirty_multi_days(D, npairs, kind):
    """Groups of 8 / 4 / 2 / 1 days by the LDS the days' weights take (8 up to 512 baselines, 4 up to 1024, 2 up to 2048, 1
    above): every day bit-identical to its own single-day launch (the kernel's documented claim), day 0 and the last day
    by the value rule."""
    plan, dev, single, exp = _multi_setup(npairs, kind)
    got = plan.dirty_multi([v for v, _ in dev[:D]], [w for _, w in dev[:D]])
    for d in range(D):
        assert np.array_equal(got[d], single[d]), f"day {d} of {D} differs from its own dmm_dirty_run (npairs={npairs}, {kind})"
    for d in {0, D - 1}:
        _note("multi", dt.check_launch(got[d], exp[d], what=f"multi D={D} day={d} npairs={npairs} {kind}"))
    assert plan.pool_unchanged()


def test_dirty_multi_single_day_results_pass_the_rule():
    """(the single-day launches the multi-day test compares with are themselves right, every day of them)"""
    for npairs in (23, 763, 2049):
        for kind in KINDS:
            _, _, single, exp = _multi_setup(npairs, kind)
            for d, (g, e) in enumerate(zip(single, exp)):
                dt.check_launch(g, e, what=f"single day {d} npairs={npairs} {kind}")


# ---------------------------------------------------------------------------------------------------------------------
# k_project_rg

PROJECT_NPAIRS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 36, 63, 64, 65, 379, 763)


@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64], ids=["c128", "c64"])
@pytest.mark.parametrize("b_layout", [dt.PACKED, dt.FULL], ids=["packed", "full"])
@pytest.mark.parametrize("npairs", PROJECT_NPAIRS)
def test_project_row_regimes(npairs, b_layout, b_dtype):
    """ntel = 2 npairs around the row group of 8, a wave's share of 16 rows and the 64-row task; ncol = 2 L in {62, 64, 66, 2}
    on each side of one wave-load of a row."""
    rng = np.random.default_rng(8000 + npairs)
    mf = [(0, 0), (1, 1), (2, 0), (32, 1), (1, 0)]
    case = make_case(rng, npairs, 2, 32, 2, 35, mf, "c128" if b_dtype == dt.C128 else "c64p", b_layout)
    assert sorted({2 * (33 - m) for m, _ in mf}) == [2, 62, 64, 66]
    with Plan(case, tail=3) as plan:
        check_project(plan, rng, f"project npairs={npairs} layout={b_layout} dtype={b_dtype}")
        assert plan.pool_unchanged()


@pytest.mark.parametrize("b_dtype", [dt.C128, dt.C64], ids=["c128", "c64"])
@pytest.mark.parametrize("b_layout", [dt.PACKED, dt.FULL], ids=["packed", "full"])
def test_project_at_the_lds_limit(b_layout, b_dtype):
    """npol (lmax + 1) = 10240 complex doubles = the 160 KiB stage, filled by the m = 0 tile."""
    rng = np.random.default_rng(8100)
    case = make_case(rng, 4, 4, 2559, 1, 3, [(0, 0), (2, 0)], "c128" if b_dtype == dt.C128 else "c64p", b_layout)
    assert case.npol * (case.lmax + 1) == 10240
    with Plan(case) as plan:
        check_project(plan, rng, f"project nsky=10240 layout={b_layout} dtype={b_dtype}")


def test_project_one_over_the_lds_limit_is_refused():
    from draco_amd import _lib

    rng = np.random.default_rng(8200)
    case = make_case(rng, 2, 1, 10240, 1, 1, [(0, 0)], "c128")
    assert case.npol * (case.lmax + 1) == 10241
    with Plan(case) as plan:
        with pytest.raises(_lib.DmmError, match="too large for the LDS stage") as ei:
            vis = _filled(case.vis_shape())
            _lib.check(_lib.lib.dmm_project_run(plan.h, plan.ptr(plan.pool), plan.ptr(_dev(make_alm_in(rng, case))), plan.ptr(vis)))
        assert ei.value.code == _lib.DMM_E_UNSUPPORTED
        assert np.all(_host(vis) == dt.SENTINEL)
        check_dirty(plan, rng, "dirty nsky=10241")  # (the Dirty kernel has no such stage)


# ---------------------------------------------------------------------------------------------------------------------
# tuning options (tools/tune_dirty.py, multi_tune.py, step_ab.py, project_timing.py and DMM_OPTS of the benchmark set them)


@functools.lru_cache(maxsize=None)
def _option_case(which, kind):
    rng = np.random.default_rng(9000)
    if which == "mid":  # ntel = 92; ncol up to 564: three column blocks (two paired)
        return make_case(rng, 46, 4, 140, 3, 141, [(77, 1), (0, 0), (140, 2), (13, 2), (139, 0), (0, 1), (77, 2)], kind)
    # ntel = 48 = 12 x 4 = 6 x 8 = 4 x 12 = 3 x 16 = 2 x 24; ntel = 96 = 12 x 8 = 8 x 12 = 6 x 16 = 4 x 24 = 3 x 32: on a multiple of
    # every kUnroll the variants instantiate (no tail behind the pipelined groups); ntel = 94: two rows short of them
    npairs = {"on48": 24, "on96": 48, "below96": 47}[which]
    return make_case(rng, npairs, 2, 70, 2, 71, [(0, 0), (70, 1), (33, 1), (5, 0)], kind)


OPTION_PLANS = ("mid", "on48", "on96", "below96")
DIRTY_OPTIONS = [{"dirty_variant": v} for v in range(1, 8)] + [{"dirty_static": 1}, {"grid_mult": 2}, {"grid_mult": 8}, {"dirty_prio": 1},
                                                                {"dirty_variant": 3, "dirty_static": 1, "grid_mult": 2}]


def _opt_id(o):
    return "-".join(f"{k}{v}" for k, v in o.items())


@pytest.mark.parametrize("kind", ["c128", "c64p"])
@pytest.mark.parametrize("which", OPTION_PLANS)
def test_dirty_options_bit_identical_to_default(which, kind):
    """Every form of ``k_dirty`` -- any kUnroll, pipelined or not, temporal or non-temporal loads, raised priority -- adds the
    rows of a column in ascending order through the same chain of fused multiply-adds in one lane's registers, and the
    task hand-out (ticket / static, any grid) only decides WHICH block computes a column: the results must be bit-identical to
    the default's, which passes the value rule."""
    case = _option_case(which, kind)
    rng = np.random.default_rng(9100)
    with Plan(case) as plan:
        base, (mvis, mw) = check_dirty(plan, rng, f"options default {which} {kind}")
        v, w = _dev(mvis), _dev(mw)
        for opts in DIRTY_OPTIONS:
            with _ctx().options(**opts):
                got = plan.dirty(v, w)
            assert np.array_equal(got, base), f"{_opt_id(opts)} on {which} {kind} differs from the default"
        assert np.array_equal(plan.dirty(v, w), base)  # options are back at 0


@pytest.mark.parametrize("kind", ["c128", "c64p"])
@pytest.mark.parametrize("which", OPTION_PLANS)
def test_dirty_multi_options_bit_identical_to_default(which, kind):
    """The multi-day kernel's variants (kUnroll 16 / 4 / 12, temporal loads) and hand-out options: same argument, same bits --
    against the single-day default of every day.  D = 11 runs a group of 8, a group of 2 and a single day."""
    case = _option_case(which, kind)
    rng = np.random.default_rng(9200)
    days = [make_data(rng, case, zero_frac=0.05 + 0.03 * d) for d in range(11)]
    with Plan(case) as plan:
        dev = [(_dev(v), _dev(w)) for v, w in days]
        single = [plan.dirty(v, w) for v, w in dev]
        _note(dirty_family(case), dt.check_launch(single[10], case.expected_alm(*days[10]), what=f"multi options day 10 {which} {kind}"))
        for opts in [{}] + DIRTY_OPTIONS:
            with _ctx().options(**opts):
                got = plan.dirty_multi([v for v, _ in dev], [w for _, w in dev])
            for d in range(11):
                assert np.array_equal(got[d], single[d]), f"{_opt_id(opts) or 'default'} on {which} {kind}: day {d} differs"


@pytest.mark.parametrize("which", OPTION_PLANS)
def test_project_options(which):
    """``project_variant`` 5 / 6 and ``project_grid_mult`` keep the default's per-lane column order and its butterfly over the
    lane bits 0..5 in that order (row groups of 4 scatter two levels later, the additions are the same pairs): bit-identical.
    Variants 1-4 (one row per wave, a loop per polarisation, shuffle-down tree) add in another order: the value rule."""
    case = _option_case(which, "c128")
    rng = np.random.default_rng(9300)
    with Plan(case) as plan:
        base, alm = check_project(plan, rng, f"project options default {which}")
        a = _dev(alm)
        exp = case.expected_vis(alm)
        for opts in ({"project_variant": 5}, {"project_variant": 6}, {"project_grid_mult": 2}, {"project_variant": 6, "project_grid_mult": 2}):
            with _ctx().options(**opts):
                got = plan.project(a)
            assert np.array_equal(got, base), f"{_opt_id(opts)} on {which} differs from the default"
        for v in (1, 2, 3, 4):
            for gm in (0, 2):
                with _ctx().options(project_variant=v, project_grid_mult=gm):
                    got = plan.project(a)
                _note("project c128", dt.check_launch(got, exp, what=f"project_variant={v} project_grid_mult={gm} on {which}"))
        assert np.array_equal(plan.project(a), base)


def test_project_options_complex64_and_full_layout():
    """complex64 has one projection kernel: the options must not change its result; the full-layout loop per polarisation under
    every complex128 variant."""
    rng = np.random.default_rng(9400)
    case = _option_case("mid", "c64p")
    with Plan(case) as plan:
        base, alm = check_project(plan, rng, "project options c64")
        for opts in [{"project_variant": v} for v in range(1, 7)] + [{"project_grid_mult": 2}]:
            with _ctx().options(**opts):
                assert np.array_equal(plan.project(_dev(alm)), base), _opt_id(opts)
    full = make_case(rng, 20, 3, 70, 2, 71, [(0, 0), (69, 1), (33, 1), (6, 0)], "c128", dt.FULL)
    with Plan(full) as plan:
        base, alm = check_project(plan, rng, "project options full layout")
        exp = full.expected_vis(alm)
        for v in range(1, 7):
            with _ctx().options(project_variant=v):
                got = plan.project(_dev(alm))
            _note("project c128", dt.check_launch(got, exp, what=f"project_variant={v} full layout"))
            if v >= 5:
                assert np.array_equal(got, base)
