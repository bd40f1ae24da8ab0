"""Sensitivity of the beamformed visibilities of a time stream on the GPU (drop-in for ``draco/analysis/sensitivity.py``).

``ComputeSystemSensitivity`` turns a ``TimeStream`` into the ``SystemSensitivity`` container that ``RFISensitivityMask``
reads: per frequency, polarisation product and time the noise *measured* by the weights of the stacked visibilities, the
*radiometer* expectation from the autocorrelations, and the number of baselines behind them.  Everything with
``freq x stack x time`` cost is ``csrc/sensitivity.hip``, which reads the weight cube and the autocorrelation rows of the
visibility cube once each; the host does the index work (:meth:`ComputeSystemSensitivity.tables`), once per call.  The
four datasets of the result are written on the device and stay there.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import tools
from .transform import _dev_dataset


def _i32(a):
    """An int32 table and its host pointer (an empty table still gets an address)."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.size == 0:
        a = np.zeros(1, dtype=np.int32)[:0]
    return a, C.c_void_p(a.ctypes.data)


def stack_maps(data):
    """``(prod, stack, reverse_stack)`` of a stream; one that was never stacked has one entry per product."""
    prod = np.asarray(data.index_map["prod"])
    stack = data.index_map.get("stack")
    if stack is not None and stack.dtype.names is not None and "prod" in stack.dtype.names and "stack" in data.reverse_map:
        return prod, np.asarray(stack), np.asarray(data.reverse_map["stack"])
    stack = np.zeros(len(prod), dtype=[("prod", "<u4"), ("conjugate", "u1")])
    stack["prod"] = np.arange(len(prod))
    reverse = np.zeros(len(prod), dtype=[("stack", "<u4"), ("conjugate", "u1")])
    reverse["stack"] = np.arange(len(prod))
    return prod, stack, reverse


class ComputeSystemSensitivity(ContainerTask):
    """Compute the sensitivity of beamformed visibilities (``sensitivity.py:11-261``).

    Attributes
    ----------
    exclude_intracyl : bool
        Exclude the intracylinder baselines from the estimate (default False: all baselines).  A ``ValueError`` is
        raised if it is set and the visibilities were already stacked over cylinders.
    """

    exclude_intracyl = False
    _config_names = ("exclude_intracyl",)

    def setup(self, telescope):
        self.telescope = io.get_telescope(telescope)

    def tables(self, data):
        """The index work of one call, as plain arrays (a dict):

        ``cnt [nstack, ncol]`` float32, the redundancy of every stack entry under every distinct column of input flags,
        and ``col [niff, ntime]``, the column of every sample (``niff`` is ``nfreq`` with a ``gain`` dataset, else 1);
        ``pol``, ``pol_ptr [npol + 1]`` and ``rows [n, 2]``: per polarisation product its stack entries, each with the
        factor 2 (1 for an autocorrelation); ``grp_ptr``, ``auto_rows``: the autocorrelation entries grouped by (input
        polarisation, east-west position); ``pair_ptr [npol + 1]``, ``pairs [m, 2]``: per polarisation product the
        ordered group pairs whose autocorrelations multiply; ``dnu_tint``: samples per integration at no packet loss."""
        tel = self.telescope
        nfreq, nstack, ntime = data.vis.shape
        flags = np.asarray(data.input_flags[:]).astype(bool)
        niff = 1
        if "gain" in data.datasets:  # the default gain marks an input that was masked at that frequency and time
            gainflg = np.asarray(data.datasets["gain"][:]) != (1.0 + 0.0j)
            flags = np.swapaxes(flags[np.newaxis, :, :] & gainflg, 0, 1).reshape(flags.shape[0], -1)
            niff = nfreq
        uniq, index_cnt = tools.unique_columns(flags)
        prod, stack, reverse = stack_maps(data)
        cnt = tools.calculate_redundancy(uniq.astype(np.float32), prod, reverse["stack"], nstack)

        inputs = np.asarray(data.index_map["input"])
        stack_new, stack_flag = tools.redefine_stack_index_map(tel, inputs, prod, stack, reverse)
        if not np.all(stack_flag):
            self.log.warning(f"There are {np.sum(~stack_flag):0.0f} stacked baselines that are masked in the telescope instance.")
        ps = prod[stack_new["prod"]]
        conj = stack_new["conjugate"].astype(bool)
        in_a = np.where(conj, ps["input_b"], ps["input_a"]).astype(np.int64)
        in_b = np.where(conj, ps["input_a"], ps["input_b"]).astype(np.int64)

        tel_index = tools.find_inputs(tel.input_index, inputs, require_match=False)
        present = np.array([ti is not None for ti in tel_index], dtype=bool)
        slot = np.array([ti if ti is not None else 0 for ti in tel_index], dtype=np.int64)
        input_pol = np.where(present, np.asarray(tel.polarisation)[slot], "N")
        ew_position = np.where(present, np.asarray(tel.feedpositions)[slot, 0], 0.0)

        # XY and YX are one polarisation product, named in alphabetical order
        pa, pb = input_pol[in_a], input_pol[in_b]
        baseline_pol = np.char.add(np.where(pa <= pb, pa, pb), np.where(pa <= pb, pb, pa))
        ew_intra = 0.5 * tel.cylinder_width
        if self.exclude_intracyl:
            baseline_flag = np.abs(ew_position[in_a] - ew_position[in_b]) > ew_intra
        else:
            baseline_flag = np.ones(nstack, dtype=bool)
        pol_uniq = [str(bp) for bp in np.unique(baseline_pol) if "N" not in bp]
        npol = len(pol_uniq)
        is_auto = in_a == in_b
        if self.exclude_intracyl and is_auto.sum() == npol:
            raise ValueError(
                "You have requested the exclusion of intracylinder baselines,  however it appears that the visibilities "
                "have already been stacked over cylinder, preventing calculation of the radiometric estimate."
            )
        pol_index = [np.flatnonzero((baseline_pol == up) & baseline_flag) for up in pol_uniq]
        pol_ptr = np.concatenate([[0], np.cumsum([len(ix) for ix in pol_index])])
        rows = np.zeros((int(pol_ptr[-1]), 2), dtype=np.int32)
        if len(rows):
            rows[:, 0] = np.concatenate(pol_index)
            rows[:, 1] = 2 - is_auto[rows[:, 0]]

        # autocorrelations by (polarisation of the input, east-west position): which pairs of them the reference's double
        # loop multiplies depends on nothing else (an input the telescope lacks belongs to no polarisation product)
        auto_id = np.flatnonzero(is_auto & (input_pol[in_a] != "N"))
        key = np.zeros(len(auto_id), dtype=[("pol", "<U1"), ("ew", np.float64)])
        key["pol"], key["ew"] = input_pol[in_a[auto_id]], ew_position[in_a[auto_id]]
        groups, member = np.unique(key, return_inverse=True)
        member = np.asarray(member).reshape(-1)
        order = np.argsort(member, kind="stable")
        grp_ptr = np.concatenate([[0], np.cumsum(np.bincount(member, minlength=len(groups)))])
        pair_lists = [[] for _ in pol_uniq]
        for g, (pg, eg) in enumerate(groups):
            for h, (ph, eh) in enumerate(groups):
                if self.exclude_intracyl and abs(eg - eh) < ew_intra:
                    continue
                name = pg + ph if pg <= ph else ph + pg
                if name in pol_uniq:
                    pair_lists[pol_uniq.index(name)].append((g, h))
        pair_ptr = np.concatenate([[0], np.cumsum([len(pl) for pl in pair_lists])])
        pairs = np.array([gh for pl in pair_lists for gh in pl], dtype=np.int32).reshape(-1, 2)

        tint = np.median(np.abs(np.diff(data.time))) if ntime > 1 else np.nan  # one sample has no integration time: NaN, as the reference
        dnu = np.median(data.index_map["freq"]["width"]) * 1e6
        return {
            "cnt": np.ascontiguousarray(cnt, dtype=np.float32), "col": index_cnt.reshape(niff, ntime).astype(np.int32), "niff": niff,
            "pol": np.array(pol_uniq, dtype="<U2"), "pol_ptr": pol_ptr.astype(np.int32), "rows": rows,
            "grp_ptr": grp_ptr.astype(np.int32), "auto_rows": auto_id[order].astype(np.int32),
            "pair_ptr": pair_ptr.astype(np.int32), "pairs": pairs, "dnu_tint": float(dnu * tint),
        }  # fmt: skip

    def process(self, data):
        """``containers.TimeStream`` -> ``containers.SystemSensitivity`` (device resident)."""
        if "time" not in data.index_map:
            raise TypeError(f"ComputeSystemSensitivity needs a time stream (a container with a `time` axis), got {type(data).__name__}.")
        data.redistribute("freq")
        return self.run(data, self.tables(data))

    def run(self, data, tb):
        """The device side of :meth:`process`: the two kernels over ``data`` with the index tables ``tb`` of
        :meth:`tables`."""
        nfreq, nstack, ntime = (int(s) for s in data.vis.shape)
        npol, niff, ncol = len(tb["pol"]), tb["niff"], tb["cnt"].shape[1]
        if len(tb["grp_ptr"]) - 1 > _lib.DMM_SENS_MAX_GROUP:
            raise ValueError(f"the autocorrelations fall into {len(tb['grp_ptr']) - 1} (polarisation, east-west position) groups, more than the {_lib.DMM_SENS_MAX_GROUP} supported")
        metrics = containers.SystemSensitivity(pol=tb["pol"], axes_from=data, attrs_from=data, comm=data.comm, allocate=False)
        if npol == 0:
            raise ValueError("no stack entry lies between two inputs of the telescope: there is no polarisation product to estimate")

        ctx = Context.get()
        vis = _dev_dataset(data.vis, ctx, np.complex64)
        weight = _dev_dataset(data.weight, ctx, np.float32)
        frac_lost = None
        if "flags" in data and "frac_lost" in data["flags"]:
            frac_lost = _dev_dataset(data["flags"]["frac_lost"], ctx, np.float32)
        cnt = ctx.to_device(tb["cnt"])
        measured, radiometer, count = (ctx.empty((nfreq, npol, ntime), np.float32) for _ in range(3))
        frac_out = ctx.empty((nfreq, ntime), np.float32)

        col, col_p = _i32(tb["col"])
        pol_ptr, pol_ptr_p = _i32(tb["pol_ptr"])
        rows, rows_p = _i32(tb["rows"])
        grp_ptr, grp_ptr_p = _i32(tb["grp_ptr"])
        arows, arows_p = _i32(tb["auto_rows"])
        pair_ptr, pair_ptr_p = _i32(tb["pair_ptr"])
        pairs, pairs_p = _i32(tb["pairs"])
        # one scratch per launch: the second call's tables may not overwrite what the first kernel still reads
        t_meas = ctx.empty((col.size + pol_ptr.size + rows.size + 1,), np.int32)
        t_rad = ctx.empty((col.size + grp_ptr.size + arows.size + pair_ptr.size + pairs.size + 1,), np.int32)
        _lib.check(
            _lib.lib.dmm_sens_measured(ctx.handle, ptr(weight), nfreq, nstack, ntime, ptr(cnt), ncol, niff, col_p, npol, pol_ptr_p, rows_p, ptr(t_meas), ptr(measured), ptr(count))
        )
        _lib.check(
            _lib.lib.dmm_sens_radiometer(ctx.handle, ptr(vis), ptr(weight), nfreq, nstack, ntime, ptr(cnt), ncol, niff, col_p, len(grp_ptr) - 1, grp_ptr_p, arows_p, npol, pair_ptr_p,
                                         pairs_p, ptr(frac_lost), tb["dnu_tint"], ptr(t_rad), ptr(radiometer), ptr(frac_out))
        )
        metrics.attach("measured", measured)
        metrics.attach("radiometer", radiometer)
        metrics.attach("weight", count)
        metrics.attach("frac_lost", frac_out)
        return metrics
