"""m-mode transform tasks on the GPU.

Drop-in for ``draco/analysis/transform.py``:

* :class:`MModeTransform`         ``transform.py:535-641``
* :class:`MModeInverseTransform`  ``transform.py:708-792``
* :func:`_make_marray`            ``transform.py:644-705``
* :func:`_make_ssarray`           ``transform.py:814-817`` (+ ``_unpack_marray`` :820-851)

Same class names, config attributes (``remove_integration_window``, ``use_fftw``,
``nra``, ``apply_integration_window``), ``setup``/``process`` signatures and exceptions.
The arithmetic runs in ``libdraco_amd.so`` (``csrc/mfft.hip``): a batched in-LDS FFT fused
with the +/-m pack and the transposed store.  ``use_fftw`` is accepted and ignored
(there is one FFT, the HIP one).
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import tools


def _dev_dataset(ds, ctx, dtype):
    """Device tensor for a dataset-like (our Dataset, ndarray, or foreign ``ds[:]``)."""
    if isinstance(ds, containers.Dataset):
        t = ds.device(ctx)
        want = {np.complex64: torch.complex64, np.complex128: torch.complex128, np.float32: torch.float32, np.float64: torch.float64}[dtype]
        return t if t.dtype == want else t.to(want)
    if isinstance(ds, torch.Tensor):
        return ctx.to_device(ds, dtype)
    return ctx.to_device(np.asarray(ds[:]), dtype)


def mmode_forward(ctx, vis_d, weight_d, mmax, remove_integration_window=False, vis_dtype=np.complex128):
    """Device-level transform: ``vis [..., nra]`` c64 (+ weight f32) -> ``(mvis, mweight)``.

    ``mvis [mmax+1, 2, ...]`` complex128 (complex64 on request) and ``mweight`` float64, as
    ``transform.py:594-639``.  ``weight`` may have fewer leading axes than ``vis`` (hybrid streams).
    """
    lead = tuple(vis_d.shape[:-1])
    nra = int(vis_d.shape[-1])
    nrow = int(np.prod(lead)) if lead else 1
    mscale = wscale = None
    if remove_integration_window:
        m = np.arange(mmax + 1)
        w = np.sinc(m / nra)  # transform.py:631-633
        mscale = ctx.to_device(tools.invert_no_zero(w), np.float64)
        wscale = ctx.to_device(w**2, np.float64)
    mvis = ctx.empty((mmax + 1, 2, *lead), vis_dtype)
    out_dt = _lib.DMM_C128 if np.dtype(vis_dtype) == np.complex128 else _lib.DMM_C64
    _lib.check(_lib.lib.dmm_mfft_pack(ctx.handle, ptr(vis_d), nrow, nra, ptr(mvis), mmax, out_dt, ptr(mscale)))
    mweight = None
    if weight_d is not None:
        wlead = tuple(weight_d.shape[:-1])
        wrow = int(np.prod(wlead)) if wlead else 1
        mweight = ctx.empty((mmax + 1, 2, *wlead), np.float64)
        _lib.check(_lib.lib.dmm_mmode_weight(ctx.handle, ptr(weight_d), wrow, nra, ptr(mweight), mmax, ptr(wscale)))
    return mvis, mweight


class MModeTransform(ContainerTask):
    """Transform a sidereal stream to m-modes (``transform.py:535-641``).

    The maximum m is ``telescope.mmax`` if a manager was given to :meth:`setup`, else
    ``nra // 2``.

    Attributes
    ----------
    remove_integration_window : bool
        Deconvolve the rectangular RA integration window (vis and weights).
    use_fftw : bool
        Accepted for compatibility; the transform always runs the HIP FFT.
    """

    remove_integration_window = False
    use_fftw = True
    _config_names = ("remove_integration_window", "use_fftw")

    telescope = None

    def setup(self, manager=None):
        """Set the telescope instance if a manager object is given (``transform.py:557-571``)."""
        if manager is not None:
            self.telescope = io.get_telescope(manager)
        else:
            self.telescope = None

    def process(self, sstream):
        """Perform the m-mode transform: ``SiderealStream -> MModes`` (``transform.py:573-641``)."""
        contmap = {
            containers.SiderealStream: containers.MModes,
            containers.HybridVisStream: containers.HybridVisMModes,
        }
        out_cont = contmap[sstream.__class__]  # KeyError for unsupported containers, like :590

        sstream.redistribute("freq")
        ctx = Context.get()
        svis = _dev_dataset(sstream.vis, ctx, np.complex64)
        sweight = _dev_dataset(sstream.weight, ctx, np.float32)
        nra = int(svis.shape[-1])

        if self.telescope is not None:
            mmax = int(self.telescope.mmax)
        else:
            mmax = nra // 2

        ma = out_cont(mmax=mmax, oddra=bool(nra % 2), axes_from=sstream, attrs_from=sstream, comm=sstream.comm, allocate=False)
        ma.redistribute("freq")
        hybrid = out_cont is containers.HybridVisMModes  # keeps complex64 / float32 (containers.py:1559-1574)
        mvis, mweight = mmode_forward(ctx, svis, sweight, mmax, self.remove_integration_window, np.complex64 if hybrid else np.complex128)
        ma.attach("vis", mvis)
        ma.attach("vis_weight", mweight.to(torch.float32) if hybrid else mweight)
        return ma


def _make_marray(ts, mmodes=None, mmax=None, dtype=None, use_fftw=True):
    """GPU version of the reference helper (``transform.py:644-705``), same contract.

    ``ts [..., N]`` complex -> ``mmodes [mmax+1, 2, ...]``; writes into ``mmodes`` if given
    (every slot of it is defined: filled modes, zeros elsewhere).
    """
    ts = np.asarray(ts)
    if dtype is None:
        dtype = np.complex64
    if mmodes is None and mmax is None:
        raise ValueError("One of `mmodes` or `mmax` must be set.")
    if mmodes is not None and mmax is not None:
        raise ValueError("If mmodes is set, mmax must be None.")
    if mmodes is not None and mmodes.shape[2:] != ts.shape[:-1]:
        raise ValueError(f"ts and mmodes have incompatible shapes: {mmodes.shape[2:]} != {ts.shape[:-1]}")
    if mmax is None:
        mmax = mmodes.shape[0] - 1
    ctx = Context.get()
    ts_d = ctx.to_device(ts, np.complex64)
    mvis, _ = mmode_forward(ctx, ts_d, None, int(mmax))
    out = mvis.cpu().numpy()
    if mmodes is None:
        return out.astype(dtype, copy=False)
    mmodes[...] = out
    return mmodes


def _unpack_limits(ctx, mvis_d, n=None):
    """``mmax_plus`` / ``mmax_minus`` / ``ntimes`` of ``_unpack_marray`` (``transform.py:824-836``)."""
    import ctypes as C

    n_m = int(mvis_d.shape[0])
    nrow = int(np.prod(mvis_d.shape[2:])) if mvis_d.dim() > 2 else 1
    mmax_plus = n_m - 1
    z = C.c_int(0)
    _lib.check(_lib.lib.dmm_mrow_is_zero(ctx.handle, ptr(mvis_d), n_m, nrow, mmax_plus, 1, C.byref(z)))
    mmax_minus = mmax_plus - 1 if z.value else mmax_plus
    if n is None:
        ntimes = mmax_plus + mmax_minus + 1
    else:
        ntimes = int(n)
        mmax_plus = min(ntimes // 2, mmax_plus)
        mmax_minus = min((ntimes - 1) // 2, mmax_minus)
    return mmax_plus, max(mmax_minus, 0), ntimes


def mmode_inverse(ctx, mvis_d, n=None, mscale=None, limits=None):
    """Device-level inverse: ``mvis [n_m, 2, ...]`` c128 -> ``vis [..., ntimes]`` complex64."""
    lead = tuple(mvis_d.shape[2:])
    nrow = int(np.prod(lead)) if lead else 1
    mp, mm, ntimes = limits if limits is not None else _unpack_limits(ctx, mvis_d, n)
    out = ctx.empty((*lead, ntimes), np.complex64)
    _lib.check(_lib.lib.dmm_mifft_unpack(ctx.handle, ptr(mvis_d), int(mvis_d.shape[0]), nrow, ntimes, mp, mm, ptr(mscale), ptr(out)))
    return out


def _make_ssarray(mmodes, n=None):
    """GPU version of ``transform.py:814-817``; returns complex64 (the SiderealStream dtype).

    The reference returns complex128 and casts on assignment into ``SiderealStream.vis``
    (``transform.py:787``); the kernel computes in float64 and rounds once at the store.
    """
    ctx = Context.get()
    mv = ctx.to_device(np.asarray(mmodes), np.complex128)
    return mmode_inverse(ctx, mv, n).cpu().numpy()


class MModeInverseTransform(ContainerTask):
    """Transform m-modes back to a sidereal stream (``transform.py:708-792``).

    Attributes
    ----------
    nra : int
        Number of RA bins in the output (default: natural ``2*mmax + oddra``).
    apply_integration_window : bool
        Apply the rectangular integration window to visibilities and weights.  Unlike the
        reference (warning at ``transform.py:713-714``) the input container is NOT modified.
    """

    nra = None
    apply_integration_window = False
    _config_names = ("nra", "apply_integration_window")

    def process(self, mmodes):
        """``MModes -> SiderealStream`` (``transform.py:733-792``)."""
        mmodes.redistribute("freq")
        ctx = Context.get()
        nra_cont = 2 * mmodes.mmax + (1 if mmodes.oddra else 0)
        nra = self.nra if self.nra is not None else nra_cont

        mvis = _dev_dataset(mmodes.vis, ctx, np.complex128)
        mweight = _dev_dataset(mmodes.weight, ctx, np.float64)
        mscale = None
        wfac = 1.0
        if self.apply_integration_window:
            m = np.arange(mmodes.mmax + 1)
            w = np.sinc(m / nra)
            mscale = ctx.to_device(w, np.float64)
            wfac = float(tools.invert_no_zero(w)[0] ** 2)  # weight[0, 0] *= inv_w[0]**2 (:769)

        vis = mmode_inverse(ctx, mvis, int(nra), mscale)
        nra = int(vis.shape[-1])
        sstream = containers.SiderealStream(ra=nra, axes_from=mmodes, attrs_from=mmodes, comm=mmodes.comm, allocate=False)
        sstream.redistribute("freq")
        sstream.attach("vis", vis)
        # no time information survives for the weights: the time average per (freq, baseline), :790
        w0 = (mweight[0, 0] * (wfac / nra)).to(torch.float32)
        sstream.attach("vis_weight", w0.unsqueeze(-1).expand(*w0.shape, nra).contiguous())
        return sstream


class SiderealMModeResample(ContainerTask):
    """Resample a sidereal stream by FFT: a forward then an inverse m-mode transform
    (``transform.py:795-811``, the reference's ``group_tasks(MModeTransform, MModeInverseTransform)``).

    Attributes
    ----------
    nra : int
        The number of RA bins for the output stream.
    remove_integration_window, apply_integration_window : bool
        Remove the integration window from the incoming data, and/or apply it to the output stream.
    use_fftw : bool
        Accepted and ignored, as in :class:`MModeTransform`.
    """

    nra = None
    remove_integration_window = False
    apply_integration_window = False
    use_fftw = True
    _config_names = ("nra", "remove_integration_window", "apply_integration_window", "use_fftw")

    _manager = None

    def setup(self, manager=None):
        self._manager = manager

    def process(self, sstream):
        fwd = MModeTransform(remove_integration_window=self.remove_integration_window, use_fftw=self.use_fftw)
        fwd.setup(self._manager)
        inv = MModeInverseTransform(nra=self.nra, apply_integration_window=self.apply_integration_window)
        return inv.process(fwd.process(sstream))  # the m-modes never leave the device


def _cmap(i, j, n):
    if i > j:
        i, j = j, i
    return (n * (n + 1) // 2) - ((n - i) * (n - i + 1) // 2) + (j - i)


_find_inputs = tools.find_inputs  # the name this module has always used for it


class TelescopeStreamMixIn:
    """Pre-computes the telescope's prod / stack / reverse-stack index maps (``transform.py:91-139``)."""

    def setup(self, tel):
        self.telescope = tel = io.get_telescope(tel)
        n = tel.nfeed
        self.bt_stack = np.array(
            [(_cmap(a, b, n), 0) if a <= b else (_cmap(b, a, n), 1) for a, b in tel.uniquepairs],
            dtype=[("prod", "<u4"), ("conjugate", "u1")],
        )
        triu = np.triu_indices(n)
        self.bt_prod = np.zeros(len(triu[0]), dtype=[("input_a", "<u2"), ("input_b", "<u2")])
        self.bt_prod["input_a"], self.bt_prod["input_b"] = triu
        fm = np.asarray(tel.feedmask)[triu]
        self.bt_rev = np.empty(fm.size, dtype=[("stack", "<u4"), ("conjugate", "u1")])
        self.bt_rev["stack"] = np.where(fm, np.asarray(tel.feedmap)[triu], tel.npairs)
        self.bt_rev["conjugate"] = np.where(fm, np.asarray(tel.feedconj)[triu], 0)


_redefine_stack_index_map = tools.redefine_stack_from_index


class CollateProducts(TelescopeStreamMixIn, ContainerTask):
    """Extract, order and stack the correlation products for map-making (``transform.py:142-330``).

    The input may hold more inputs and frequencies than the telescope; the converse raises
    ``ValueError`` like the reference.  For inputs that are ALREADY redundancy-stacked the
    representative product of every stack entry is re-derived so that it only involves inputs the
    telescope has and does not mask (``transform.py:206-221``, ``util/tools.py:359-414``).

    Attributes
    ----------
    weight : {"natural", "uniform", "inverse_variance"}
        How to weight the redundant baselines when stacking.
    """

    weight = "natural"
    _config_names = ("weight",)

    def process(self, ss):
        tel = self.telescope
        ss_input = np.asarray(ss.index_map["input"])
        input_ind = _find_inputs(tel.input_index, ss_input, require_match=False)
        rev_input_ind = _find_inputs(ss_input, tel.input_index, require_match=True)
        freq_ind = tools.find_keys(list(ss.index_map["freq"]["centre"]), list(tel.frequencies), require_match=True)
        bt_freq = ss.index_map["freq"][freq_ind]
        file_prod = np.asarray(ss.index_map["prod"])
        stacked = bool(getattr(ss, "is_stacked", False))
        if stacked:
            stack_new, stack_flag = _redefine_stack_index_map(tel, input_ind, file_prod, np.asarray(ss.index_map["stack"]), np.asarray(ss.reverse_map["stack"]))
            if not np.all(stack_flag):
                self.log.warning(f"There are {np.sum(~stack_flag):0.0f} stacked baselines that are masked in the telescope instance.")
            ss_prod = file_prod[stack_new["prod"]]
            ss_conj = stack_new["conjugate"].astype(bool)
        else:
            ss_prod = file_prod
            ss_conj = np.zeros(len(ss_prod), dtype=bool)
        if self.weight not in ("natural", "uniform", "inverse_variance"):
            raise ValueError(f"unknown weight {self.weight!r}")

        sp = type(ss)(freq=bt_freq, ra=np.asarray(ss.index_map["ra"]), input=tel.input_index, prod=self.bt_prod, stack=self.bt_stack,
                      reverse_map_stack=self.bt_rev, attrs_from=ss, comm=ss.comm, allocate=False)
        ctx = Context.get()
        ssv = _dev_dataset(ss.vis, ctx, np.complex64)
        ssw = _dev_dataset(ss.weight, ctx, np.float32)
        nf_in, nprod_in, nt = ssv.shape

        # invert the reference's product loop (transform.py:277-320) into output-major lists
        lists = [[] for _ in range(tel.npairs)]
        for ss_pi, (ii, ij) in enumerate(zip(ss_prod["input_a"], ss_prod["input_b"])):
            bi, bj = input_ind[ii], input_ind[ij]
            if bi is None or bj is None:
                continue
            sp_pi = int(tel.feedmap[bi, bj])
            if sp_pi < 0:
                continue
            lists[sp_pi].append((ss_pi, bool(tel.feedconj[bi, bj]) != bool(ss_conj[ss_pi])))  # conjugate unless feedconj == conj (:303)
        ptr_ = np.zeros(tel.npairs + 1, dtype=np.int32)
        ptr_[1:] = np.cumsum([len(x) for x in lists])
        src = np.array([p for x in lists for p, _ in x], dtype=np.int32)
        cj = np.array([c for x in lists for _, c in x], dtype=np.uint8)

        flags = None
        if "input_flags" in ss.datasets:
            flags = np.asarray(ss.input_flags[:], dtype=np.float32)
        red_d = None
        if self.weight != "inverse_variance":
            fl = flags if flags is not None and np.any(flags) else np.ones((len(ss_input), nt), np.float32)
            if stacked:  # products that went into each stack entry with both inputs good (util/tools.py:313-356)
                red = np.zeros((nprod_in, nt), np.float32)
                np.add.at(red, np.asarray(ss.reverse_map["stack"]["stack"]).astype(np.int64),
                          fl[file_prod["input_a"].astype(int)] * fl[file_prod["input_b"].astype(int)])
            else:
                red = fl[ss_prod["input_a"].astype(int)] * fl[ss_prod["input_b"].astype(int)]  # one product per "stack" entry
            if self.weight == "uniform":
                red = (red > 0).astype(np.float32)
            red_d = ctx.to_device(np.ascontiguousarray(red, dtype=np.float32))
        out_v = ctx.empty((len(freq_ind), tel.npairs, nt), np.complex64)
        out_w = ctx.empty((len(freq_ind), tel.npairs, nt), np.float32)
        d = lambda a: ctx.to_device(a) if a.size else ctx.to_device(np.zeros(1, a.dtype))  # noqa: E731
        # keep the index tensors referenced until the launch is enqueued (a temporary would be recycled at once)
        find_d, ptr_d, src_d, cj_d = d(np.asarray(freq_ind, dtype=np.int32)), d(ptr_), d(src), d(cj)
        _lib.check(
            _lib.lib.dmm_collate_products(
                ctx.handle, ptr(ssv), ptr(ssw), int(nf_in), int(nprod_in), int(nt), len(freq_ind), ptr(find_d),
                int(tel.npairs), ptr(ptr_d), ptr(src_d), ptr(cj_d), ptr(red_d), ptr(out_v), ptr(out_w),
            )
        )
        ctx.sync()  # the small index tensors go out of scope below
        sp.attach("vis", out_v)
        sp.attach("vis_weight", out_w)
        if flags is not None:
            sp.add_dataset("input_flags", allocate=True)
            sp.input_flags[:] = flags[rev_input_ind, :]
        return sp


class LanczosRegridder(ContainerTask):
    """Interpolate the time-like axis of a dataset onto a regular grid (``transform.py:854-986``).

    A maximum-likelihood inverse of a Lanczos interpolation: per (frequency, stack) row a banded Wiener solve, which
    runs in ``libdraco_amd.so`` (``csrc/regrid.hip``); the Lanczos matrix is evaluated on the host
    (``draco_amd/util/regrid.py``).  Config attributes, ``setup`` / ``process`` signatures and the out-of-bounds
    ``RuntimeError`` are the reference's.  The output datasets stay on the device.
    """

    _config_names = ("samples", "start", "end", "kernel_width", "epsilon", "mask_zero_weight")
    samples = 1024
    start = None
    end = None
    kernel_width = 5
    epsilon = 1e-3
    mask_zero_weight = False

    def setup(self, observer):
        self.observer = io.get_telescope(observer)

    def process(self, data):
        data.redistribute("freq")
        timelike_axis = data.vis.attrs["axis"][-1]
        times = data.index_map[timelike_axis][:]
        if self.start is None:
            self.start = times[0]
        if self.end is None:
            self.end = times[-1]
        if self.start < times[0] or self.end > times[-1]:
            msg = "Start or end points for regridder fall outside bounds of input data."
            self.log.error(msg)
            raise RuntimeError(msg)
        new_grid, new_vis, ni = self._regrid(data.vis, data.weight, times)
        cont_type = data.__class__
        new_data = cont_type(axes_from=data, allocate=False, **{timelike_axis: new_grid})
        new_data.redistribute("freq")
        new_data.attach("vis", new_vis)
        new_data.attach("vis_weight", ni)
        return new_data

    def _regrid(self, vis_data, weight, times, mix=None):
        """``(grid, vis, weight)`` on the regular grid; ``vis`` / ``weight`` device tensors shaped like the input with
        the last axis replaced (``transform.py:951-986``).  ``mix``: see :func:`draco_amd.util.regrid.band_wiener`."""
        from ..util import regrid

        ctx = Context.get()
        vis_d = _dev_dataset(vis_data, ctx, np.complex64)
        w_d = _dev_dataset(weight, ctx, np.float32)
        times = np.asarray(times, dtype=np.float64)
        # a regular grid, padded at either end to suppress interpolation issues
        pad = 5 * self.kernel_width
        interp_grid = np.arange(-pad, self.samples + pad, dtype=np.float64) / self.samples
        interp_grid = interp_grid * (self.end - self.start) + self.start
        plan = regrid.RegridPlan(ctx, interp_grid, times, self.kernel_width)
        try:
            lead = tuple(vis_d.shape[:-1])
            nt = int(vis_d.shape[-1])
            sts, ni = regrid.band_wiener(ctx, plan, vis_d.reshape(-1, nt), w_d.reshape(-1, nt), self.epsilon, pad, self.samples, self.mask_zero_weight, mix)
        finally:
            ctx.sync()  # the plan's tables are freed with it
            plan.close()
        return interp_grid[pad:-pad].copy(), sts.reshape(*lead, self.samples), ni.reshape(*lead, self.samples)


# Alias for compatibility
Regridder = LanczosRegridder


# ---------------------------------------------------------------------------------------------------------------
# Weighted reductions over axes (``transform.py:1904-2117``), ``csrc/reduce.hip``

_REDUCE_DTYPE = {torch.float32: _lib.DMM_REDUCE_F32, torch.float64: _lib.DMM_REDUCE_F64, torch.complex64: _lib.DMM_REDUCE_C64, torch.complex128: _lib.DMM_REDUCE_C128}


def _merged_strides(shape, strides):
    """The ``(length, stride)`` runs that address the same elements as the axes given, in the same order: axes of
    length one are dropped and an axis is merged into the one before it where ``stride_before == length * stride``."""
    runs = []
    for n, s in zip(shape, strides):
        n, s = int(n), int(s)
        if n == 1:
            continue
        if runs and runs[-1][1] == n * s:
            runs[-1] = (runs[-1][0] * n, s)
        else:
            runs.append((n, s))
    return runs


def axis_reduce_device(ctx, op, x, w, first, last, factor=1.0):
    """Reduce the adjacent axes ``first ... last`` of the contiguous device tensor ``x`` (float32, float64, complex64 or
    complex128) with ``dmm_axis_reduce``.

    ``w``: ``None`` or a float32 / float64 device tensor that broadcasts against ``x`` (same number of axes, length one
    where it lacks an axis); it is read in place through its strides when the axes ahead of the reduced ones, and those
    behind them, merge into one stride each and the reduced ones into at most two, and is expanded otherwise.  Returns
    ``(out, out_w)`` shaped like ``x`` with every reduced axis of length one; their types are the header's.
    """
    if x.dtype not in _REDUCE_DTYPE:
        raise TypeError(f"axis_reduce: data of type {x.dtype} is not supported")
    x = x.contiguous()
    shape = [int(s) for s in x.shape]
    nouter, nred, ninner = (int(np.prod(shape[a:b], dtype=np.int64)) for a, b in ((0, first), (first, last + 1), (last + 1, len(shape))))
    wdtype, strides = _lib.DMM_REDUCE_F32, (0, 1, 0, 0, 0)  # (outer, nred2, red1, red2, inner)
    if w is not None:
        if w.dtype not in (torch.float32, torch.float64):
            w = w.to(torch.float32)
        wdtype = _lib.DMM_REDUCE_F64 if w.dtype == torch.float64 else _lib.DMM_REDUCE_F32
        wv = w.expand(*shape)
        for attempt in range(2):
            groups = [_merged_strides(shape[a:b], wv.stride()[a:b]) for a, b in ((0, first), (first, last + 1), (last + 1, len(shape)))]
            if len(groups[0]) <= 1 and len(groups[1]) <= 2 and len(groups[2]) <= 1:
                break
            wv = w = wv.contiguous()  # (the second attempt always merges)
        red = groups[1] + [(1, 0)] * (2 - len(groups[1]))
        strides = (groups[0][0][1] if groups[0] else 0, red[1][0], red[0][1], red[1][1], groups[2][0][1] if groups[2] else 0)
        if len(groups[1]) == 1:  # one run: it is the inner of the two reduced axes
            strides = (strides[0], nred if nred else 1, 0, red[0][1], strides[4])
    keep = [1 if first <= d <= last else s for d, s in enumerate(shape)]
    if op == _lib.DMM_REDUCE_WMEAN:
        out, out_w = ctx.empty(keep, np.float64), ctx.empty(keep, np.float64)
    else:
        out = torch.empty(keep, dtype=x.dtype, device=x.device)
        out_w = ctx.empty(keep, np.float64 if wdtype == _lib.DMM_REDUCE_F64 else np.float32)
    _lib.check(
        _lib.lib.dmm_axis_reduce(
            ctx.handle, int(op), _REDUCE_DTYPE[x.dtype], ptr(x), nouter, nred, ninner, ptr(w), wdtype, int(strides[0]), int(max(strides[1], 1)), int(strides[2]),
            int(strides[3]), int(strides[4]), float(factor), ptr(out), ptr(out_w),
        )
    )
    return out, out_w


class ReduceBase(ContainerTask):
    """Apply a weighted reduction across adjacent axes of one dataset (``transform.py:1904-2062``).

    Config: ``axes``, the names of the axes to reduce; ``dataset``, the dataset to reduce; ``weighting``, "none",
    "masked" or "weighted" where the operation has a choice.  At least one axis must be left.  The output is a
    container of the input's class in which every reduced axis has length one and carries the first entry of its index
    map, with the attributes ``reduced``, ``reduction_axes``, ``reduced_dataset`` and ``reduction_op``; only the
    reduced dataset and the weight are set, and both stay on the device.  The weight is the reduced weight at index 0
    of the axes the input's weight lacks.  Reduced axes that are not adjacent in the dataset: ``NotImplementedError``.
    """

    axes = None
    dataset = None
    weighting = "none"
    _config_names = ("axes", "dataset", "weighting")
    _op = None

    def read_config(self, params):
        super().read_config(params)
        if self.weighting not in ("none", "masked", "weighted"):
            raise ValueError(f"weighting must be 'none', 'masked' or 'weighted', not {self.weighting!r}")

    def process(self, data):
        axes = list(self.axes or ())
        ds = data.datasets[self.dataset]
        ds_axes = list(ds.attrs["axis"])
        if not [ax for ax in ds_axes if ax not in axes]:
            raise ValueError("Could not find a valid axis to redistribute. At least one axis must be omitted from filtering.")
        weight, w_axes = self._get_weights(data)
        apply_over = sorted(ds_axes.index(ax) for ax in axes if ax in ds_axes)
        if not apply_over or apply_over != list(range(apply_over[0], apply_over[-1] + 1)):
            raise NotImplementedError(f"the reduced axes {axes} must be adjacent axes of the dataset, which has {ds_axes}")
        out = self._make_output_container(data)

        ctx = Context.get()
        x = ds.device(ctx)
        wt = None
        if weight is not None:
            wt = weight.device(ctx) if isinstance(weight, containers.Dataset) else ctx.to_device(np.asarray(weight[:]))
            wt = wt.reshape([wt.shape[w_axes.index(ax)] if ax in w_axes else 1 for ax in ds_axes])
        reduced, reduced_weight = self.reduction(x, wt, (apply_over[0], apply_over[-1]))

        if self.dataset not in out._dataset_spec:
            out.add_dataset(self.dataset, allocate=False)
        out.attach(self.dataset, reduced)
        wname = self._weight_name(data)
        if wname is not None:
            pick = tuple(slice(None) if ax in w_axes else 0 for ax in ds_axes)
            out.attach(wname, reduced_weight[pick].contiguous())
        return out

    @staticmethod
    def _weight_name(data):
        return next((name for name in ("weight", "vis_weight") if name in data.datasets), None)

    def _get_weights(self, data):
        """The weight dataset and its axis names, ``(None, None)`` for a container without weights."""
        name = self._weight_name(data)
        if name is None:
            if self.weighting != "none":
                raise RuntimeError("No weights available. Cannot use weighted or masked weighting.")
            return None, None
        return data.datasets[name], list(data.datasets[name].attrs["axis"])

    def _make_output_container(self, data):
        # the first entry of a reduced axis' index map stands for the whole axis, whatever the operation
        output_axes = {ax: np.array([data.index_map[ax][0]]) for ax in self.axes}
        out = data.__class__(axes_from=data, attrs_from=data, allocate=False, **output_axes)
        out.attrs["reduced"] = True
        out.attrs["reduction_axes"] = np.array(self.axes)
        out.attrs["reduced_dataset"] = self.dataset
        out.attrs["reduction_op"] = self._op
        return out

    def reduction(self, arr, weight, axis):
        """``(reduced, reduced_weight)`` of the device tensor ``arr`` over its adjacent axes ``axis = (first, last)``,
        both with those axes of length one; ``weight`` broadcasts against ``arr`` or is ``None``."""
        raise NotImplementedError


class ReduceVar(ReduceBase):
    """The weighted variance over the axes (``transform.py:2065-2089``): with "none" ``mean |x - mean x|^2`` and unit
    weights; with "masked" (weights set to ``w > 0``) and "weighted", ``sum w (x - mu)^2 / sum w`` about the weighted
    mean ``mu`` and the weight ``sum w``."""

    _op = "variance"

    def reduction(self, arr, weight, axis):
        op = {"none": _lib.DMM_REDUCE_VAR_NONE, "masked": _lib.DMM_REDUCE_VAR_MASKED, "weighted": _lib.DMM_REDUCE_VAR_WEIGHTED}[self.weighting]
        if op != _lib.DMM_REDUCE_VAR_NONE and weight is None:
            raise RuntimeError("No weights available. Cannot use weighted or masked weighting.")
        return axis_reduce_device(Context.get(), op, arr, weight, axis[0], axis[1])


class ReduceChisq(ReduceBase):
    """The chi-squared per degree of freedom over the axes (``transform.py:2092-2117``), for data that is uncorrelated
    noise of inverse variance ``weight``: ``sum w |x - mu|^2 / num`` about the weighted mean, with ``num`` one less than
    the number of samples of positive weight, which is also the weight that comes out."""

    _op = "chisq_per_dof"

    def reduction(self, arr, weight, axis):
        return axis_reduce_device(Context.get(), _lib.DMM_REDUCE_CHISQ, arr, weight, axis[0], axis[1])


def stokes_i_table(tel):
    """The products that make up instrumental Stokes I, per unique baseline (``transform.py:1403-1442``).

    The telescope's ``baselines`` are rounded to 0.1 mm and grouped; a product enters its baseline's sum if it is
    co-polar, if its baseline occurs with all four polarisation pairs, and if its ``feedmap`` entry is not -1.  Returns
    ``(ubase [nbase, 2], ptr [nbase + 1], rows)``, the products of baseline ``b`` being ``rows[ptr[b]:ptr[b + 1]]`` in
    ascending order, the order in which the reference accumulates them.
    """
    bl_round = np.around(tel.baselines[:, 0] + 1.0j * tel.baselines[:, 1], 4)
    ubase, uinv, ucount = np.unique(bl_round, return_inverse=True, return_counts=True)
    ubase = ubase.astype(np.complex128, copy=False).view(np.float64).reshape(-1, 2)
    pairs = np.asarray(tel.uniquepairs)
    pols = np.asarray(tel.polarisation)[pairs]
    keep = (pols[:, 0] == pols[:, 1]) & (ucount[uinv] >= 4) & (np.asarray(tel.feedmap)[pairs[:, 0], pairs[:, 1]] != -1)
    prods = np.flatnonzero(keep)
    order = np.argsort(uinv[prods], kind="stable")  # by baseline, ascending product within one
    rows = prods[order].astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(uinv[prods], minlength=len(ubase)))]).astype(np.int32)
    return ubase, ptr, rows


def stokes_i_device(ctx, vis, weight, base_ptr, rows):
    """``vis [nf, nprod, nt]`` complex64 and ``weight`` float32 device tensors -> ``(vis_I, weight_I)`` ``[nf, nbase,
    nt]`` (``dmm_stokes_i_sum``); ``base_ptr`` / ``rows``: int32 device tensors of :func:`stokes_i_table`."""
    nf, nprod, nt = (int(s) for s in vis.shape)
    nbase = int(base_ptr.numel()) - 1
    vis_i = torch.empty((nf, nbase, nt), dtype=torch.complex64, device=vis.device)
    weight_i = torch.empty((nf, nbase, nt), dtype=torch.float32, device=vis.device)
    if vis_i.numel():
        _lib.check(_lib.lib.dmm_stokes_i_sum(ctx.handle, ptr(vis), ptr(weight), nf, nprod, nt, ptr(base_ptr), ptr(rows), nbase, int(rows.numel()), ptr(vis_i), ptr(weight_i)))
    return vis_i, weight_i


def stokes_I(sstream, tel):
    """Extract instrumental Stokes I from a time / sidereal stream (``transform.py:1382-1448``).

    Returns ``(vis_I, weight_I, ubase)``: ``[nfreq, nbase, ntime]`` complex64 and float32 device tensors and the
    ``[nbase, 2]`` baseline vectors.  The sums are the reference's (:func:`stokes_i_table`), accumulated in the
    stream's own precision in product order.  A telescope whose redundancy classes do not hold all four polarisation
    pairs per baseline (``pair_rule="canonical"``) keeps nothing: every row comes back zero.
    """
    sstream.redistribute("freq")
    ctx = Context.get()
    ubase, ptr_h, rows_h = stokes_i_table(tel)
    vis = _dev_dataset(sstream.vis, ctx, np.complex64).contiguous()
    weight = _dev_dataset(sstream.weight, ctx, np.float32).contiguous()
    if int(vis.shape[1]) != len(tel.uniquepairs):
        raise ValueError(f"stokes_I: the stream has {int(vis.shape[1])} stack entries, the telescope {len(tel.uniquepairs)} unique pairs")
    ptr_d, rows_d = ctx.to_device(ptr_h), ctx.to_device(rows_h if len(rows_h) else np.zeros(1, dtype=np.int32))
    vis_i, weight_i = stokes_i_device(ctx, vis, weight, ptr_d, rows_d[: len(rows_h)])
    ctx.uses(ptr_d, rows_d)
    return vis_i, weight_i, ubase
