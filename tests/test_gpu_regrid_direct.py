"""``csrc/regrid.hip`` addressed directly through its entry points (``dmm_regrid_plan_create``, ``dmm_regrid_band_wiener``,
``dmm_sidereal_stack_add``, ``dmm_sidereal_stack_finish``) against the long-double truth and the float32 stack twin of
``tests/regrid_twin.py``.

Measures.  ``out_vis``, per row and component: ``|got - T| <= 2**-24 |T| + B`` with ``B = 8 e64``, ``e64`` the worst error
in that row of the twin's float64 restatement of the banded algorithm (``test_regrid_twin_host.py`` tabulates it; ``B``
is some 1e-13 ... 1e-12 of the row maximum), and ``got == float32(T)`` wherever ``T`` is at least ``B`` from a float32
rounding boundary (``mismatch``: how many such elements differ, must be 0; ``excluded``: the share nearer than that, at
most 1e-3).  Where the truth is an exact zero (no sample in reach, or none with weight) the output is an exact zero.
``out_weight``: ``got == float32(T)`` wherever ``T`` is ``(maxspan + 2) 2**-53 T`` from a boundary, one float32 step
elsewhere, the zero pattern the truth's.  The wide-weight case (weights over 1e-6 ... 1e6, ``B`` about 1e-7 of the row
maximum, as large as the float32 rounding itself) is held to the inequality alone: the rounded-once equality is dropped
there.  With mixing the angle ``omega dphi`` is the float64 product in the truth as in the kernel and the reference.  The
stacker kernels: every dataset after every day and after the finish, compared as integers with the twin that
reproduces the reference's executed vectors bit for bit.  Every output buffer is NaN before the call; each test prints
``error / bound`` (at most 1 passes) before it asserts.

Measured on an MI355X, ``error / bound`` (the ``vis`` and ``weight`` ratios approach 1 wherever an element's float32
rounding is nearly half a unit: that is the bound's first term, and the rounded-once comparison is the sharper of the
two; ``e64``: the float64 restatement's worst error, in units of 2**-52 of the row maximum, from
``test_regrid_twin_host.py``).  No element of any case differs from the truth rounded once; with ``mask_zero_weight`` the
figures are the same:

    case          maxspan   e64    vis     weight   mismatch   excluded
    width1        5         121    0.992   0.974    0          0
    width2        10        165    0.997   0.980    0          0
    width3        14        207    0.994   0.997    0          2.1e-4
    width4        18        151    0.994   0.997    0          3.2e-4
    width5        23        277    0.987   0.998    0          2.1e-4
    width6        27        336    0.988   0.985    0          4.3e-4
    clamp4        85        149    0.919   0.964    0          0          (tile 170)
    clamp5        106       47     0.916   0.955    0          0          (tile clamped to 210)
    clamp6        126       63     0.924   0.923    0          0          (tile clamped to 210)
    edge1         14        250    0.562   0.626    0          0
    edge2         16        35     0.795   0.322    0          0
    edge63        10        231    0.858   0.925    0          0
    edge64        10        111    0.901   0.845    0          0
    edge65        10        70     0.893   0.960    0          0
    edge128       10        238    0.967   0.936    0          0
    edge129       10        97     0.917   0.854    0          0
    pad0_width1   5         226    0.893   0.923    0          0
    pad1_width1   5         3.0    0.873   0.907    0          0
    pad0_width3   14        59     0.946   0.785    0          0
    pad1_width3   14        405    0.911   0.835    0          0
    pad_task      14        247    0.741   0.889    0          0
    mix5          23        713    0.989   0.998    0          3.2e-4
    mix2          10        295    0.971   0.980    0          2.1e-4
    wide          23        6.3e7  0.822   0.989    -          -          (B / rowmax 6e-13 ... 1.1e-7 over its rows)
    reuse_a       14        240    0.991   0.983    0          3.5e-4
    reuse_b       14        604    0.993   0.976    0          1.2e-4

Reuse of one plan, and a call after NaN in the scratch: the bits of a fresh call.  The stacker: 0 elements differ in all
40 cases.  The whole file takes 2.2 ... 3.1 s, 1.8 ... 2.6 s of it the first call's start-up; no other case takes more
than 0.1 s.
"""

import ctypes as C
import time

import numpy as np
import pytest

import regrid_twin as twin

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _file_time():
    yield
    print(f"regrid direct: the file took {time.perf_counter() - T0:.1f} s")


def _nan(ctx, shape, dtype):
    import torch

    t = ctx.empty(shape, dtype)
    t.fill_(complex(np.nan, np.nan) if t.is_complex() else np.nan)
    torch.cuda.synchronize()
    return t


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


class _Plan:
    """``dmm_regrid_plan_create`` on the spans ``compact_rows`` finds, as ``RegridPlan`` builds it."""

    def __init__(self, case):
        from draco_amd import _lib
        from draco_amd.device import Context
        from draco_amd.util import regrid

        self.ctx = Context.get()
        R = regrid.lanczos_forward_matrix(case.grid, case.times, case.a).T.copy()
        start, end, vals = regrid.compact_rows(R)
        assert np.array_equal(start, case.start) and np.array_equal(end, case.end)
        self.handle = C.c_void_p()
        self.rc = _lib.lib.dmm_regrid_plan_create(self.ctx.handle, case.nt, len(case.grid), case.a, _np_ptr(start), _np_ptr(end), _np_ptr(vals), C.byref(self.handle))

    def close(self):
        from draco_amd import _lib

        if self.handle:
            self.ctx.sync()
            _lib.lib.dmm_regrid_plan_destroy(self.handle)
            self.handle = C.c_void_p()


def _band_wiener(plan, case, mask_zero_weight=False, vis=None, weight=None):
    """One ``dmm_regrid_band_wiener`` call on the inputs of ``case`` (or other rows of the same shape)."""
    from draco_amd import _lib
    from draco_amd.device import ptr

    ctx = plan.ctx
    vis_d = ctx.to_device(case.vis if vis is None else vis)
    w_d = ctx.to_device(case.weight if weight is None else weight)
    assert tuple(vis_d.shape) == tuple(w_d.shape) == (case.nrow, case.nt)
    mix_d = [None] * 4 if case.mix is None else [ctx.to_device(a) for a in case.mix]
    assert case.mix is None or [str(t.dtype) for t in mix_d] == ["torch.float64", "torch.float32", "torch.float64", "torch.float64"]
    # the outputs end in a guard of NaN that no store may touch (an output tile is 64 grid points wide)
    nout = case.nrow * case.samples
    out_v = _nan(ctx, (nout + GUARD,), np.complex64)
    out_w = _nan(ctx, (nout + GUARD,), np.float32)
    _lib.check(_lib.lib.dmm_regrid_band_wiener(ctx.handle, plan.handle, ptr(vis_d), ptr(w_d), case.nrow, twin.EPS, case.pad, case.samples, int(mask_zero_weight),
                                               ptr(mix_d[0]), ptr(mix_d[1]), ptr(mix_d[2]), ptr(mix_d[3]), ptr(out_v), ptr(out_w)))
    ctx.sync()
    x, nw = out_v.cpu().numpy(), out_w.cpu().numpy()
    assert np.isnan(x[nout:]).all() and np.isnan(nw[nout:]).all(), "a store past the end of the output"
    return x[:nout].reshape(case.nrow, case.samples), nw[:nout].reshape(case.nrow, case.samples)


def _run(name, mask_zero_weight=False):
    case = twin.RegridCase.get(name)
    plan = _Plan(case)
    try:
        assert plan.rc == 0
        x, nw = _band_wiener(plan, case, mask_zero_weight)
    finally:
        plan.close()
    case.check(f"{name}{' mask_zero_weight' if mask_zero_weight else ''} (maxspan {case.maxspan})", x, nw, mask_zero_weight, rounded=not case.spec["wide"])
    assert not x[0].any() and not nw[0].any(), "a row of all-zero weights gives exact zeros"
    if case.mix is not None:
        assert not x[-1].any() and not nw[-1].any(), "a row with feed_mask == 0 has zero weights and visibilities"
    return case, x, nw


@pytest.mark.parametrize("mask_zero_weight", [False, True], ids=["keep", "mask_zero_weight"])
@pytest.mark.parametrize("a", range(1, 7))
def test_width_sweep(a, mask_zero_weight):
    """``k_regrid<1>`` ... ``k_regrid<6>``: 67 rows (two waves, the second with three live lanes), 70 outputs (one
    full output tile and one of 6)."""
    case, x, nw = _run(f"width{a}", mask_zero_weight)
    assert case.a == a and case.nrow == 67 and case.samples == 70 and x[1].any()


@pytest.mark.parametrize("a", [4, 5, 6])
def test_tile_clamp(a):
    """Eleven samples per grid cell: at widths 5 and 6 twice the longest span is more than the 210 samples the LDS tile
    holds, so the tile is clamped and a group is one or a few grid points; width 4 (tile 170) sits just under."""
    case = twin.RegridCase.get(f"clamp{a}")
    assert case.maxspan == twin.REGRID_CLAMP_MAXSPAN[f"clamp{a}"] == {4: 85, 5: 106, 6: 126}[a]
    assert (2 * case.maxspan > twin.REGRID_TILE_MAX) == (a >= 5) and case.maxspan <= twin.REGRID_TILE_MAX
    _run(f"clamp{a}")


def test_refusal():
    """A grid point that reads more samples than the LDS tile holds: ``DMM_E_UNSUPPORTED`` from the plan, a Python
    exception from ``LanczosRegridder._regrid``, nothing launched."""
    from draco_amd import _lib
    from draco_amd.analysis.transform import LanczosRegridder

    case = twin.RegridCase(twin.REGRID_REFUSED)
    assert case.maxspan > twin.REGRID_TILE_MAX
    plan = _Plan(case)
    assert plan.rc == _lib.DMM_E_UNSUPPORTED and not plan.handle
    with pytest.raises(_lib.DmmError, match=rf"a grid point reads {case.maxspan} samples, the LDS tile holds {twin.REGRID_TILE_MAX}"):
        _lib.check(plan.rc)
    with pytest.raises(ValueError, match="plan is NULL"):  # no plan came back, so there is nothing a launch could use
        _band_wiener(plan, case)
    t = LanczosRegridder(samples=case.samples, kernel_width=case.a, epsilon=twin.EPS)
    t.start, t.end = 0.0, 1.0
    with pytest.raises(_lib.DmmError, match="LDS tile holds"):
        t._regrid(case.vis, case.weight, case.times)
    # the context is as usable as before
    _run("edge2")


@pytest.mark.parametrize("samples", [1, 2, 63, 64, 65, 128, 129])
def test_output_tile_edges(samples):
    case, x, nw = _run(f"edge{samples}")
    assert case.samples == samples and case.a == 2 and case.nrow == 3 and x[2].any()


@pytest.mark.parametrize("name", ["pad0_width1", "pad1_width1", "pad0_width3", "pad1_width3", "pad_task"])
def test_padding(name):
    """``pad`` 0 and 1 through the entry point (the Python side always passes ``5 kernel_width``: ``pad_task``)."""
    case, x, nw = _run(name)
    assert case.pad == {"pad0": 0, "pad1": 1, "pad": 15}[name.split("_")[0]] and len(case.grid) == 40 + 2 * case.pad


def test_padding_through_the_task():
    """``LanczosRegridder._regrid`` (``RegridPlan``, ``pad = 5 kernel_width``) gives the direct call's bits."""
    from draco_amd.analysis.transform import LanczosRegridder

    case, x, nw = _run("pad_task")
    t = LanczosRegridder(samples=case.samples, kernel_width=case.a, epsilon=twin.EPS)
    t.start, t.end = 0.0, 1.0
    _, v, w = t._regrid(case.vis, case.weight, case.times)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), x.view(np.uint32)) and np.array_equal(w.cpu().numpy().view(np.uint32), nw.view(np.uint32))


@pytest.mark.parametrize("name", ["mix5", "mix2"])
def test_mixing(name):
    """The fused mix-down and mix-up: fringe rates over +-2e3 rad per turn, one row with its feed masked."""
    case, x, nw = _run(name)
    assert x[2:-1].any(axis=1).all() and nw[2:-1].any(axis=1).all()


def test_wide_weights():
    """Weights over 1e-6 ... 1e6, 60 % flagged: the inequality alone (``B`` is as large as the float32 rounding)."""
    case = twin.RegridCase.get("wide")
    _, _, _, B, _ = case.truth()
    rm = case.rowmax()
    print(f"regrid wide: B / rowmax {', '.join(f'{float(b / r):.2g}' for b, r in zip(B[1:, 0], rm[1:]))}")
    _run("wide")


def test_reuse():
    """One plan, two calls with different rows; and a call after one that left NaN in the whole factor scratch (NaN
    weights and data): the same bits as a fresh call each."""
    a, b = twin.RegridCase.get("reuse_a"), twin.RegridCase.get("reuse_b")
    assert np.array_equal(a.times, b.times) and not np.array_equal(a.vis, b.vis) and a.a == b.a
    _, xa, wa = _run("reuse_a")
    _, xb, wb = _run("reuse_b")
    plan = _Plan(a)
    try:
        assert plan.rc == 0
        xa1, wa1 = _band_wiener(plan, a)
        xb1, wb1 = _band_wiener(plan, b)
        xn, wn = _band_wiener(plan, a, vis=np.full(a.vis.shape, complex(np.nan, np.nan), np.complex64), weight=np.full(a.weight.shape, np.nan, np.float32))
        reach = (a.end > a.start)[a.pad : a.pad + a.samples]
        assert np.isnan(xn).all() and np.isnan(wn[:, reach]).all()  # (the factor, z and every weight with a sample in reach held NaN)
        xa2, wa2 = _band_wiener(plan, a)
    finally:
        plan.close()
    same = lambda p, q: np.array_equal(p.view(np.uint32), q.view(np.uint32))  # noqa: E731
    assert same(xa1, xa) and same(wa1, wa) and same(xb1, xb) and same(wb1, wb) and same(xa2, xa) and same(wa2, wa)
    assert not same(xa, xb)


# ---- the stacker
def _stack_gpu(days, uniform, with_var, with_nsample):
    import torch

    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    n = len(days[0][0])
    mode = _lib.DMM_STACK_UNIFORM if uniform else _lib.DMM_STACK_INVERSE_VARIANCE
    st = {"vis": ctx.zeros((n,), np.complex64), "weight": ctx.zeros((n,), np.float32), "nsample": ctx.zeros((n,), np.int16).view(torch.uint16)}
    if with_var:
        st["sum_coeff_sq"], st["sample_variance"] = ctx.zeros((n,), np.float32), ctx.zeros((3, n), np.float32)
    var = (ptr(st["sum_coeff_sq"]), ptr(st["sample_variance"])) if with_var else (None, None)
    out = []

    def snap():
        ctx.sync()
        out.append({k: (v.view(torch.int16).cpu().numpy().view(np.uint16) if v.dtype == torch.uint16 else v.cpu().numpy()) for k, v in st.items()})

    for vis, w, ns in days:
        dev = [ctx.to_device(vis), ctx.to_device(w), ctx.to_device(ns.view(np.int16)) if with_nsample else None]
        _lib.check(_lib.lib.dmm_sidereal_stack_add(ctx.handle, mode, int(with_var), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(st["vis"]), ptr(st["weight"]),
                                                   ptr(st["nsample"]), var[0], var[1], n))
        snap()
    _lib.check(_lib.lib.dmm_sidereal_stack_finish(ctx.handle, mode, int(with_var), ptr(st["weight"]), ptr(st["nsample"]), var[0], var[1], n))
    snap()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32).reshape(-1)


@pytest.mark.parametrize("with_nsample", [False, True], ids=["single_days", "day_nsample"])
@pytest.mark.parametrize("with_var", [False, True], ids=["novar", "var"])
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "inverse_variance"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_stacker_bit_for_bit(n, uniform, with_var, with_nsample):
    days = twin.stack_days(n)
    want = twin.stack_run(days, uniform, with_var, with_nsample)
    got = _stack_gpu(days, uniform, with_var, with_nsample)
    total = 0
    report = []
    for d, (g, t) in enumerate(zip(got, want)):
        assert set(g) == set(t)
        for k in t:
            assert g[k].dtype == t[k].dtype and g[k].shape == t[k].shape
            diff = int(np.count_nonzero(_bits(g[k]) != _bits(t[k])))
            total += diff
            if diff:
                report.append(f"{'after day ' + str(d) if d < 3 else 'finish'} {k}: {diff}")
    print(f"stack direct n {n} {'uniform' if uniform else 'inverse_variance'} var {int(with_var)} day_nsample {int(with_nsample)}: {total} elements differ {report}")
    assert total == 0, report
    assert n < 8 or (want[-1]["vis"].any() and want[-1]["weight"].any())
