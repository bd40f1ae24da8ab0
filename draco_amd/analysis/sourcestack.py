"""Source stack analysis tasks, on the GPU.

Drop-in for ``draco/analysis/sourcestack.py``: :class:`SourceStack`, :class:`RandomSubset` and
:class:`GroupSourceStacks` with the reference's config attributes, defaults and ``setup`` / ``process`` /
``process_finish`` signatures.  A :class:`FormedBeam` whose ``beam`` and ``weight`` are on the device stays there through
``RandomSubset -> SourceStack -> GroupSourceStacks``: a draw is an ``index_select``, the stack is ``dmm_source_stack``
(``csrc/sourcestack.hip``), and only the ``nstack``-sized results come back to the host.

Which channels of a source fall into which bin of the stack is ``np.digitize(freq - source_freq, stackbins) - 1`` in the
reference; the kernel does the same float64 subtraction and comparison against the same edges, so membership is equal,
on a descending axis and on an irregular one.  The host builds the stack axis and the edges exactly as the reference
and uploads one float64 (the line frequency) and, with ``single_source_bin_index``, one byte per source.

Deliberate differences from the reference:

* ``int(nfreq / 2) - freqside < 0``, or a window that runs past the end of the band (``int(nfreq / 2) + freqside + 1 >
  nfreq``), raises ``ValueError``: the reference slices a wrong (or short) stack axis there.
* The frequency axis and the stack's bin edges must be strictly monotonic (``np.digitize`` demands it of the edges; the
  reference's ``f_indices[0] : f_indices[-1] + 1`` slice is the mask itself on such an axis, and fails on any other).
* One process: no distribution over ``object_id``, no collectives.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..core import containers
from ..core.task import ContainerTask, PipelineStopIteration
from ..device import Context, ptr
from ..synthesis.noise import _RandomTask
from .transform import _dev_dataset

NU21 = 1420.40575177  # MHz


def _monotonic(x):
    """+1 strictly ascending, -1 strictly descending, 0 neither (one element: +1)."""
    d = np.diff(np.asarray(x, dtype=np.float64))
    if d.size == 0 or np.all(d > 0):
        return 1
    return -1 if np.all(d < 0) else 0


def stack_partials(ctx, n, nsrc, workspace_mib):
    """``(partial, chunks, running)``: room for the partial sums of ``chunks`` source chunks of ``n`` output elements
    within ``workspace_mib``, and the running sums.  The result does not depend on ``chunks``."""
    nchunk = max(1, -(-int(nsrc) // _lib.DMM_STACK_SRC_CHUNK))
    chunks = int(min(nchunk, max(1, (int(workspace_mib) << 20) // (16 * n))))
    return ctx.empty((chunks, 2, n), np.float64), chunks, ctx.empty((2, n), np.float64)


class SourceStack(ContainerTask):
    """Stack the product of ``BeamForm`` (with ``collapse_ha``) or ``RingMapBeamForm`` across sources
    (``sourcestack.py:17-211``).

    Attributes
    ----------
    freqside : int
        Number of frequency bins to keep on each side of the source bin.  Default 50.
    single_source_bin_index : int, optional
        Only stack on sources in the frequency channel with this index.  Default None.
    uniform_weight : bool
        Uniform instead of inverse variance weights; zero weights stay zero.  Default False.
    workspace_mib : int
        Device memory the partial sums of a pass may take.  The result does not depend on it.  Default 256.
    """

    _config_names = ("freqside", "single_source_bin_index", "uniform_weight", "workspace_mib")
    freqside = 50
    single_source_bin_index = None
    uniform_weight = False
    workspace_mib = 256

    def _axis(self, formed_beam):
        """The stack axis and its bin edges, as the reference builds them (``sourcestack.py:80-109``)."""
        frequency = formed_beam.index_map["freq"]
        nfreq = len(frequency)
        self.nstack = 2 * self.freqside + 1
        lo = int(nfreq / 2) - self.freqside
        if self.freqside < 0 or lo < 0 or lo + self.nstack > nfreq:
            raise ValueError(f"freqside = {self.freqside} does not fit a band of {nfreq} channels around channel {int(nfreq / 2)}")
        self.stack_axis = np.copy(frequency[lo : lo + self.nstack])
        self.stack_axis["centre"] = self.stack_axis["centre"] - self.stack_axis["centre"][self.freqside]
        if self.stack_axis["centre"][0] > self.stack_axis["centre"][-1]:
            stackbins = self.stack_axis["centre"] + 0.5 * self.stack_axis["width"]
            stackbins = np.append(stackbins, self.stack_axis["centre"][-1] - 0.5 * self.stack_axis["width"][-1])
        else:
            stackbins = self.stack_axis["centre"] - 0.5 * self.stack_axis["width"]
            stackbins = np.append(stackbins, self.stack_axis["centre"][-1] + 0.5 * self.stack_axis["width"][-1])
        return np.asarray(stackbins, dtype=np.float64)

    def process(self, formed_beam):
        """``formed_beam``: a ``FormedBeam`` with a ``redshift`` table.  Returns a ``FrequencyStack`` (one
        polarisation) or a ``FrequencyStackByPol``."""
        if int(self.freqside) != self.freqside:
            raise ValueError(f"freqside = {self.freqside!r} is not an integer")
        self.freqside = int(self.freqside)
        freq = np.asarray(formed_beam.freq, dtype=np.float64)
        nfreq = freq.size
        pol = formed_beam.pol
        npol = len(pol)
        stackbins = self._axis(formed_beam)
        fdir, bdir = _monotonic(freq), _monotonic(stackbins)
        if fdir == 0:
            raise ValueError("the frequency axis is not strictly monotonic")
        if bdir == 0:
            raise ValueError("bins must be monotonically increasing or decreasing")
        if nfreq > _lib.DMM_STACK_MAX_FREQ:
            raise ValueError(f"{nfreq} channels: at most {_lib.DMM_STACK_MAX_FREQ}")
        if "redshift" not in formed_beam:
            raise ValueError("Input is missing a required redshift table.")
        source_freq = NU21 / (np.asarray(formed_beam["redshift"]["z"], dtype=np.float64) + 1.0)
        nsrc = source_freq.size
        smask = None
        if self.single_source_bin_index is not None:
            fs = formed_beam.index_map["freq"][int(self.single_source_bin_index)]
            smask = (np.abs(source_freq - fs["centre"]) < (0.5 * fs["width"])).astype(np.uint8)

        ctx = Context.get()
        beam = _dev_dataset(formed_beam.beam, ctx, np.float64).contiguous()
        weight = _dev_dataset(formed_beam.weight, ctx, np.float64).contiguous()
        if tuple(beam.shape) != (nsrc, npol, nfreq) or tuple(weight.shape) != (nsrc, npol, nfreq):
            raise ValueError(f"beam of shape {tuple(beam.shape)} and weight of shape {tuple(weight.shape)}, expected {(nsrc, npol, nfreq)}")
        n = npol * self.nstack
        partial, chunks, running = stack_partials(ctx, n, nsrc, self.workspace_mib)
        out_s, out_w = ctx.empty((npol, self.nstack), np.float64), ctx.empty((npol, self.nstack), np.float64)
        freq_d, bins_d, sf_d = ctx.to_device(freq), ctx.to_device(stackbins), ctx.to_device(source_freq) if nsrc else None
        sm_d = None if smask is None or not nsrc else ctx.to_device(smask)
        _lib.check(_lib.lib.dmm_source_stack(ctx.handle, nsrc, npol, nfreq, self.nstack, ptr(beam), ptr(weight), ptr(freq_d), int(fdir < 0), ptr(sf_d), ptr(sm_d),
                                             ptr(bins_d), int(bdir > 0), int(bool(self.uniform_weight)), ptr(partial), chunks, ptr(running), ptr(out_s), ptr(out_w)))
        if npol > 1:
            stack = containers.FrequencyStackByPol(freq=self.stack_axis, pol=pol, attrs_from=formed_beam)
            stack.stack[:], stack.weight[:] = out_s.cpu().numpy(), out_w.cpu().numpy()
        else:
            stack = containers.FrequencyStack(freq=self.stack_axis, attrs_from=formed_beam)
            stack.stack[:], stack.weight[:] = out_s[0].cpu().numpy(), out_w[0].cpu().numpy()
        return stack


class RandomSubset(_RandomTask):
    """Take a large mock catalogue and draw ``number`` catalogues of ``size`` objects (``sourcestack.py:214-329``).

    ``rng.choice(num_cat, size, replace=False)`` on ``np.random.default_rng(seed)``, sorted, as the reference through
    caput's ``RandomTask`` -- whose generator is seeded per MPI rank; with a given ``seed`` and one process the golden
    test compares the indices themselves.  Datasets on the device are drawn there (``index_select``).

    Attributes
    ----------
    number : int
        Number of catalogues to construct.
    size : int
        Number of objects in each catalogue.
    seed : int, optional
        Seed of the generator.
    """

    _config_names = ("number", "size")
    number = None
    size = None

    def __init__(self, **params):
        super().__init__(**params)
        self.catalog_ind = 0

    def setup(self, catalog):
        """``catalog``: the ``SourceCatalog`` or ``FormedBeam`` to draw from."""
        self.base_tag = f"{catalog.attrs['tag']}_mock_{{:05d}}" if "tag" in catalog.attrs else "mock_{:05d}"
        self.catalog = catalog

    def process(self):
        """A catalogue of the same type as the input with a random set of its objects."""
        if self.number is None or self.size is None:
            raise ValueError("RandomSubset needs number and size")
        if self.catalog_ind >= int(self.number):
            raise PipelineStopIteration
        objects = self.catalog.index_map["object_id"]
        ind = np.sort(self.rng.choice(len(objects), int(self.size), replace=False))
        self.last_indices = ind

        cat = self.catalog
        new_catalog = cat.__class__(object_id=objects[ind], attrs_from=cat, axes_from=cat, allocate=False)
        new_catalog._dataset_spec = dict(cat._dataset_spec)
        new_catalog.attrs["tag"] = self.base_tag.format(self.catalog_ind)
        ind_d = None
        for name, dset in cat.datasets.items():
            by_object = dset.attrs["axis"][0] == "object_id"
            attrs = dict(dset.attrs)
            if dset.on_device:
                t = dset._dev
                if by_object:
                    if ind_d is None:
                        ind_d = torch.from_numpy(ind.astype(np.int64)).to(t.device)
                    t = t.index_select(0, ind_d)
                new_catalog.datasets[name] = containers.Dataset(dev=t, attrs=attrs)
            else:
                h = dset.host()
                new_catalog.datasets[name] = containers.Dataset(host=h[ind] if by_object else np.array(h, copy=True), attrs=attrs)
        self.catalog_ind += 1
        return new_catalog


class GroupSourceStacks(ContainerTask):
    """Accumulate many frequency stacks into a single container (``sourcestack.py:332-467``).

    Attributes
    ----------
    ngroup : int
        The number of frequency stacks to accumulate into a single container.  Default 100.
    """

    _config_names = ("ngroup",)
    ngroup = 100

    def __init__(self, **params):
        super().__init__(**params)
        self.setup()

    def setup(self):
        """An empty list for ``process`` to fill."""
        self.stack = []
        self.nmock = 0
        self.counter = 0
        self._container_lookup = {
            containers.FrequencyStack: containers.MockFrequencyStack,
            containers.FrequencyStackByPol: containers.MockFrequencyStackByPol,
            containers.MockFrequencyStack: containers.MockFrequencyStack,
            containers.MockFrequencyStackByPol: containers.MockFrequencyStackByPol,
        }

    def process(self, stack):
        """Add a stack to the list; once the list holds ``ngroup`` of them they are returned in one container."""
        self.stack.append(stack)
        self.nmock += stack.index_map["mock"].size if "mock" in stack.index_map else 1
        self.log.info(f"Collected frequency stack.  Current size is {len(self.stack):d}.")
        if (len(self.stack) % self.ngroup) == 0:
            return self._reset()
        return None

    def process_finish(self):
        """Whatever stacks are in the list, in one container (None: the list is empty)."""
        if len(self.stack) > 0:
            return self._reset()
        return None

    def _reset(self):
        """Combine the stacks of the list into a new container, empty the list and count the group."""
        self.log.info(f"We have accumulated {self.nmock:d} mock realizations.  Saving to file. [group {self.counter:03d}]")
        mock = np.arange(self.nmock, dtype=np.int64)
        OutputContainer = self._container_lookup[self.stack[0].__class__]
        out = OutputContainer(mock=mock, axes_from=self.stack[0], attrs_from=self.stack[0])
        counter_str = f"{self.counter:03d}"

        # a group holds several mocks, a supergroup several groups
        if "tag" in out.attrs:
            tag = out.attrs["tag"].split("_")
            if "group" in tag:
                ig = max(ii for ii, tt in enumerate(tag) if tt == "group")
                tag[ig] = "supergroup"
                tag[ig + 1] = counter_str
            elif "mock" in tag:
                im = max(ii for ii, tt in enumerate(tag) if tt == "mock")
                tag[im] = "group"
                tag[im + 1] = counter_str
            else:
                tag.append(f"group_{counter_str}")
            out.attrs["tag"] = "_".join(tag)
        else:
            out.attrs["tag"] = f"group_{counter_str}"

        for name, odset in out.datasets.items():
            rows = []
            for stack in self.stack:
                dset = stack.datasets[name]
                data = dset[:]
                rows.append(data if dset.attrs["axis"][0] == "mock" else data[np.newaxis, ...])
            odset[:] = np.concatenate(rows, axis=0)

        self.stack = []
        self.nmock = 0
        self.counter += 1
        return out
