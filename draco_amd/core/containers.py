"""Minimal container duck-types for the m-mode path.

These mirror the parts of the reference containers the path touches
(``draco/core/containers.py``): dataset names, axis order and dtypes, ``index_map``,
``attrs`` and the ``axes_from`` / ``attrs_from`` constructor protocol.  They are not a
re-implementation of caput's memh5 containers [3P]; HDF5 I/O, MPI distribution and
selections are out of scope.

* :class:`SiderealStream`  ``containers.py:489-593``  vis c64 ``[freq, stack, ra]``, weight f32
* :class:`MModes`          ``containers.py:1167-1193`` vis c128 ``[m, msign, freq, stack]``, weight f64
* :class:`Map`             ``containers.py:470-486`` (+ cora ``Map`` [3P]) map f64 ``[freq, pol, pixel]``

A dataset may live on the host (ndarray), on the GPU (torch tensor) or both; tasks of
this package hand device-resident containers to each other so that a
``MModeTransform -> DirtyMapMaker`` chain never crosses PCIe.  ``ds[:]`` always gives
NumPy (copying back once if needed).
"""

from __future__ import annotations

import numpy as np


class Dataset:
    """An array that is valid on the host, on a device, or both."""

    def __init__(self, host=None, dev=None, attrs=None, pending=None):
        assert host is not None or dev is not None
        self._host = host
        self._dev_t = dev
        self._pending = pending
        self.attrs = dict(attrs or {})

    # The device copy may still be in the making on another stream: `pending` is then what orders a reader behind
    # that work -- an object with `done()` (has the producer finished? never blocks) and `order()` (make the CALLER's
    # current stream wait for it: a stream wait, not a host wait).  EVERY access to the data orders the stream that is
    # current at that moment, until the producer has finished -- readers on different streams (the caller's, a side
    # context, the fill stream, the RCCL stream) are each ordered, whichever comes first.  A producer that returns
    # early (the map-maker's side-stream SHT) does not hold up work that never looks at its output (the next sidereal
    # day's transform and solves).
    @property
    def _dev(self):
        p = self._pending
        if p is not None:
            if p.done():
                self._pending = None
            else:
                p.order()
        return self._dev_t

    @_dev.setter
    def _dev(self, t):
        self._dev_t = t

    # -- shape/dtype without forcing a copy
    @property
    def shape(self):
        return tuple(self._host.shape) if self._host is not None else tuple(self._dev_t.shape)

    @property
    def dtype(self):
        if self._host is not None:
            return self._host.dtype
        import torch

        return np.dtype(
            {
                torch.complex64: np.complex64,
                torch.complex128: np.complex128,
                torch.float32: np.float32,
                torch.float64: np.float64,
                torch.int32: np.int32,
                torch.uint8: np.uint8,
                torch.uint16: np.uint16,
                torch.bool: np.bool_,
            }[self._dev_t.dtype]
        )

    @property
    def on_device(self):
        return self._dev_t is not None

    def host(self) -> np.ndarray:
        if self._host is None:
            self._host = self._dev.detach().cpu().numpy()
        return self._host

    def device(self, ctx):
        """Device tensor on ``ctx`` (uploading the host copy the first time)."""
        if self._dev is None or self._dev.device != ctx.device:
            self._dev = ctx.to_device(self.host())
        return self._dev

    def set_device(self, t):
        """Make a device tensor the (only) valid copy."""
        self._dev = t
        self._host = None

    def __getitem__(self, key):
        return self.host()[key]

    def __setitem__(self, key, value):
        h = self.host()
        h[key] = value
        self._dev = None  # host copy is now the authority

    def __array__(self, dtype=None, copy=None):
        a = self.host()
        return a if dtype is None else a.astype(dtype)

    @property
    def local_array(self):  # MPIArray compatibility (single process)
        return self.host()


def _freq_map(freq):
    """Build the structured ``index_map['freq']`` (fields ``centre``, ``width``)."""
    if freq is None:
        return None
    f = np.asarray(freq)
    if f.dtype.names and "centre" in f.dtype.names:
        return f
    out = np.zeros(f.shape[0], dtype=[("centre", np.float64), ("width", np.float64)])
    out["centre"] = f
    out["width"] = np.abs(np.diff(f)).mean() if f.shape[0] > 1 else 1.0
    return out


class ContainerBase:
    """Axes + datasets + attrs; ``axes_from`` / ``attrs_from`` copy like caput does."""

    _axes: tuple = ()
    _dataset_spec: dict = {}

    def __init__(self, axes_from=None, attrs_from=None, comm=None, distributed=True, allocate=True, **axes):
        self.index_map = {}
        self.index_attrs = {}
        self.attrs = {}
        self.comm = comm
        self.reverse_map = {}
        axes = {k: v for k, v in axes.items() if v is not None}
        if axes_from is not None:
            for ax in self._axes:
                if ax in axes_from.index_map and ax not in axes:
                    self.index_map[ax] = axes_from.index_map[ax]
            if "stack" in getattr(axes_from, "reverse_map", {}):
                self.reverse_map["stack"] = axes_from.reverse_map["stack"]
        for ax, val in axes.items():
            if val is None:
                continue
            if ax == "freq":
                val = _freq_map(val)
            elif isinstance(val, (int, np.integer)):
                val = np.arange(int(val))
            self.index_map[ax] = np.asarray(val)
        for ax in self.index_map:
            self.index_attrs[ax] = {}
        if attrs_from is not None:
            self.attrs.update(attrs_from.attrs)
            for ax, a in getattr(attrs_from, "index_attrs", {}).items():  # (caput: axis attributes travel too)
                if ax in self.index_attrs:
                    self.index_attrs[ax].update(a)
        self.datasets = {}
        for name, spec in self._dataset_spec.items():
            missing = [a for a in spec["axes"] if a not in self.index_map]
            if missing:
                raise ValueError(f"{type(self).__name__}: axes {missing} are not defined")
            shape = tuple(len(self.index_map[a]) for a in spec["axes"])
            if allocate:  # allocate=False: the producing task attaches device tensors instead
                self.datasets[name] = Dataset(host=np.zeros(shape, dtype=spec["dtype"]), attrs={"axis": spec["axes"]})
                src = getattr(attrs_from, "datasets", {}).get(name) if attrs_from is not None else None
                if src is not None:  # dataset attributes too, but never the receiving dataset's own axis tuple
                    self.datasets[name].attrs.update({k: v for k, v in src.attrs.items() if k != "axis"})

    def copy(self, shared=()):
        """A copy with its own datasets, except those named in ``shared``, which are the SAME objects (data and
        attributes) as the original's -- caput's ``copy(shared=...)``.  Container and axis attributes are copied."""
        import copy as _copy

        out = type(self).__new__(type(self))
        out.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("datasets", "attrs", "index_attrs", "index_map", "reverse_map")})
        out.index_map = dict(self.index_map)
        out.reverse_map = dict(self.reverse_map)
        out.attrs = _copy.deepcopy(self.attrs)
        out.index_attrs = _copy.deepcopy(self.index_attrs)
        out.datasets = {}
        for name, ds in self.datasets.items():
            if name in shared:
                out.datasets[name] = ds
            else:
                out.datasets[name] = Dataset(host=np.array(ds.host(), copy=True), attrs=_copy.deepcopy(ds.attrs))
        return out

    def redistribute(self, axis):  # single process: nothing to move
        return None

    # ---- stage outputs on disk (the reference's `save` / `output_root` task parameters write every task's output
    # container to HDF5, and a pipeline resumes by loading it, doc/pipeline_params.yaml:12-13, examples/test.yaml:10-13
    # [caput, 3P]).  h5py is not in this image: the same round trip through one .npz per container.
    def save(self, path):
        """Write axes, attributes, reverse maps and datasets (copied back from the device if need be) to ``path``."""
        blob = {"__class__": np.array(type(self).__name__)}
        for k, v in self.index_map.items():
            blob["index_map/" + k] = np.asarray(v)
        for k, v in self.reverse_map.items():
            blob["reverse_map/" + k] = np.asarray(v)
        for k, v in self.attrs.items():
            blob["attrs/" + k] = np.asarray(v)
        for k, ds in self.datasets.items():
            blob["dataset/" + k] = np.asarray(ds.host())
            for ak, av in ds.attrs.items():
                if ak != "axis":
                    blob[f"dataset_attrs/{k}/{ak}"] = np.asarray(av)
        for ax, a in getattr(self, "index_attrs", {}).items():
            for ak, av in a.items():
                blob[f"index_attrs/{ax}/{ak}"] = np.asarray(av)
        with open(path, "wb") as fh:  # (np.savez would append ".npz" to a bare name)
            np.savez(fh, **blob)

    @classmethod
    def load(cls, path):
        """Rebuild a container written by :meth:`save` (host resident)."""
        with np.load(path, allow_pickle=False) as z:
            name = str(z["__class__"])
            if name != cls.__name__ and cls is not ContainerBase:
                raise TypeError(f"{path} holds a {name}, not a {cls.__name__}")
            klass = cls if cls is not ContainerBase else next(c for c in _all_containers() if c.__name__ == name)
            out = klass.__new__(klass)
            out.index_map, out.reverse_map, out.attrs, out.datasets, out.comm = {}, {}, {}, {}, None
            out.index_attrs = {}
            if hasattr(klass, "_optional_spec"):
                out._dataset_spec = dict(klass._dataset_spec)
            for key in z.files:
                kind, _, k = key.partition("/")
                if kind == "index_map":
                    out.index_map[k] = z[key]
                elif kind == "reverse_map":
                    out.reverse_map[k] = z[key]
                elif kind == "attrs":
                    v = z[key]
                    out.attrs[k] = v.item() if v.ndim == 0 else v
                elif kind == "dataset":
                    if k not in out._dataset_spec and k in getattr(klass, "_optional_spec", {}):
                        out._dataset_spec[k] = klass._optional_spec[k]
                    out.datasets[k] = Dataset(host=z[key])
            # second pass: attributes of the datasets and of the axes (the `axis` tuple of a dataset comes from its spec)
            item = lambda v: v.item() if v.ndim == 0 else v  # noqa: E731
            for k, ds in out.datasets.items():
                if k in out._dataset_spec:
                    ds.attrs["axis"] = out._dataset_spec[k]["axes"]
            for ax in out.index_map:
                out.index_attrs.setdefault(ax, {})
            for key in z.files:
                parts = key.split("/")
                if parts[0] == "dataset_attrs" and parts[1] in out.datasets:
                    out.datasets[parts[1]].attrs["/".join(parts[2:])] = item(z[key])
                elif parts[0] == "index_attrs":
                    out.index_attrs.setdefault(parts[1], {})["/".join(parts[2:])] = item(z[key])
        return out

    def dataset_shape(self, name):
        return tuple(len(self.index_map[a]) for a in self._dataset_spec[name]["axes"])

    def attach(self, name, dev_tensor, pending=None):
        """Attach a device tensor as dataset ``name`` (shape/dtype checked against the spec).  ``pending``: see
        :class:`Dataset` -- orders every reader behind the producer until the producer has finished."""
        spec = self._dataset_spec[name]
        if tuple(dev_tensor.shape) != self.dataset_shape(name):
            raise ValueError(f"{name}: shape {tuple(dev_tensor.shape)} != {self.dataset_shape(name)}")
        ds = Dataset(dev=dev_tensor, attrs={"axis": spec["axes"]}, pending=pending)
        if ds.dtype != np.dtype(spec["dtype"]):
            raise ValueError(f"{name}: dtype {ds.dtype} != {np.dtype(spec['dtype'])}")
        self.datasets[name] = ds
        return ds

    def __getitem__(self, name):
        return self.datasets[name]

    def __contains__(self, name):
        return name in self.datasets

    def __delitem__(self, name):
        """Drop dataset ``name`` (``del container["effective_ra"]``)."""
        del self.datasets[name]

    def _optional(self, name):
        if name in self.datasets:
            return self.datasets[name]
        raise KeyError(f"Dataset '{name}' not initialised.")


class _FreqMixin:
    @property
    def freq(self):
        return self.index_map["freq"]["centre"]


class _VisMixin:
    @property
    def vis(self):
        return self.datasets["vis"]

    @property
    def weight(self):
        return self.datasets["vis_weight"]


class SiderealStream(ContainerBase, _FreqMixin, _VisMixin):
    """``vis [freq, stack, ra]`` complex64 + ``vis_weight`` float32 (``containers.py:489-593``)."""

    _axes = ("freq", "stack", "ra", "prod", "input", "component")
    _dataset_spec = {
        "vis": {"axes": ["freq", "stack", "ra"], "dtype": np.complex64},
        "vis_weight": {"axes": ["freq", "stack", "ra"], "dtype": np.float32},
    }
    _optional_spec = {
        "input_flags": {"axes": ["input", "ra"], "dtype": np.float32},  # containers.py:525-530
        # what SiderealStacker adds to its stack (containers.py:536-552): days per sample, variance over days (rr, ri, ii)
        "sample_variance": {"axes": ["component", "freq", "stack", "ra"], "dtype": np.float32},
        "nsample": {"axes": ["freq", "stack", "ra"], "dtype": np.uint16},
        # what SiderealRebinner adds (containers.py:517-523): the weighted centre of the samples of every bin, degrees
        "effective_ra": {"axes": ["freq", "stack", "ra"], "dtype": np.float32},
    }

    @property
    def effective_ra(self):
        return self._optional("effective_ra")

    def add_dataset(self, name, allocate=True):
        self._dataset_spec = dict(self._dataset_spec)
        self._dataset_spec[name] = self._optional_spec[name]
        if "component" in self._optional_spec[name]["axes"] and "component" not in self.index_map:
            self.index_map["component"] = np.array(["rr", "ri", "ii"])
            self.index_attrs["component"] = {}
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=self._optional_spec[name]["dtype"]))

    @property
    def input_flags(self):
        return self.datasets["input_flags"]

    @property
    def nsample(self):
        return self._optional("nsample")

    @property
    def sample_variance(self):
        return self.datasets["sample_variance"]

    @property
    def is_stacked(self):
        st = self.index_map.get("stack")
        return st is not None and st.dtype.names is not None and "prod" in st.dtype.names and len(st) != len(self.index_map.get("prod", st))

    def __init__(self, ra=None, stack=None, prod=None, input=None, reverse_map_stack=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)  # containers.py:407-410
        if stack is None and prod is not None and kwargs.get("axes_from") is None:
            stack = len(prod)  # VisContainer default: one stack entry per product
        super().__init__(ra=ra, stack=stack, prod=prod, input=input, **kwargs)
        if reverse_map_stack is not None:
            self.reverse_map["stack"] = reverse_map_stack

    @property
    def ra(self):
        return self.index_map["ra"]

    @property
    def prodstack(self):
        """The representative input pair of every stack entry, conjugation applied (``containers.py:211-229``)."""
        prod = self.index_map["prod"]
        stack = self.index_map.get("stack")
        if stack is None or stack.dtype.names is None or "prod" not in stack.dtype.names:
            return prod
        t = prod[stack["prod"]].copy()
        conj = stack["conjugate"].astype(bool)
        t["input_a"] = np.where(conj, prod[stack["prod"]]["input_b"], prod[stack["prod"]]["input_a"])
        t["input_b"] = np.where(conj, prod[stack["prod"]]["input_a"], prod[stack["prod"]]["input_b"])
        return t


class _DatasetGroup:
    """The datasets ``<group>/<name>`` of a container under their short names: ``data["flags"]["frac_lost"]``."""

    def __init__(self, cont, group):
        self._cont, self._prefix = cont, group + "/"

    def __getitem__(self, name):
        return self._cont.datasets[self._prefix + name]

    def __contains__(self, name):
        return self._prefix + name in self._cont.datasets


class TimeStream(ContainerBase, _FreqMixin, _VisMixin):
    """Time-ordered visibilities: ``vis [freq, stack, time]`` complex64 + ``vis_weight`` float32, ``time`` the samples'
    UNIX time stamps (``containers.py:821-880``).  Optional, through :meth:`add_dataset`: ``input_flags [input, time]``
    float32, ``gain [freq, input, time]`` complex64, and ``flags/frac_lost [freq, time]`` float32, the fraction of
    correlator packets lost, which is read as ``data["flags"]["frac_lost"]``."""

    _axes = ("freq", "stack", "time", "prod", "input")
    _dataset_spec = {
        "vis": {"axes": ["freq", "stack", "time"], "dtype": np.complex64},
        "vis_weight": {"axes": ["freq", "stack", "time"], "dtype": np.float32},
    }
    _optional_spec = {
        "input_flags": {"axes": ["input", "time"], "dtype": np.float32},  # containers.py:854-859
        "gain": {"axes": ["freq", "input", "time"], "dtype": np.complex64},  # containers.py:860-868
        "flags/frac_lost": {"axes": ["freq", "time"], "dtype": np.float32},
    }

    def __init__(self, time=None, stack=None, prod=None, input=None, reverse_map_stack=None, **kwargs):
        if time is not None and not isinstance(time, (int, np.integer)):
            time = np.asarray(time, dtype=np.float64)
        if stack is None and prod is not None and kwargs.get("axes_from") is None:
            stack = len(prod)
        super().__init__(time=time, stack=stack, prod=prod, input=input, **kwargs)
        if reverse_map_stack is not None:
            self.reverse_map["stack"] = reverse_map_stack

    def add_dataset(self, name, allocate=True):
        self._dataset_spec = dict(self._dataset_spec)
        self._dataset_spec[name] = spec = self._optional_spec[name]
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=spec["dtype"]), attrs={"axis": spec["axes"]})

    def _groups(self):
        return {k.split("/")[0] for k in self.datasets if "/" in k}

    def __getitem__(self, name):
        if name not in self.datasets and name in self._groups():
            return _DatasetGroup(self, name)
        return self.datasets[name]

    def __contains__(self, name):
        return name in self.datasets or name in self._groups()

    @property
    def time(self):
        return self.index_map["time"]

    @property
    def input_flags(self):
        return self._optional("input_flags")

    @property
    def gain(self):
        return self._optional("gain")

    prodstack = SiderealStream.prodstack


class MContainer(ContainerBase):
    """m-mode containers: axes ``m``, ``msign`` and the ``oddra`` attribute (``containers.py:422-467``)."""

    def __init__(self, mmax=None, oddra=None, **kwargs):
        if mmax is not None:
            kwargs["m"] = int(mmax) + 1
        kwargs["msign"] = np.array(["+", "-"])
        super().__init__(**kwargs)
        if oddra is not None:
            self.attrs["oddra"] = bool(oddra)
        elif "oddra" not in self.attrs:
            self.attrs["oddra"] = False

    @property
    def mmax(self) -> int:
        return int(self.index_map["m"][-1])

    @property
    def oddra(self) -> bool:
        return bool(self.attrs["oddra"])


class MModes(MContainer, _FreqMixin, _VisMixin):
    """``vis [m, msign, freq, stack]`` complex128 + ``vis_weight`` float64 (``containers.py:1167-1193``)."""

    _axes = ("m", "msign", "freq", "stack", "prod", "input")
    _dataset_spec = {
        "vis": {"axes": ["m", "msign", "freq", "stack"], "dtype": np.complex128},
        "vis_weight": {"axes": ["m", "msign", "freq", "stack"], "dtype": np.float64},
    }


class HybridVisStream(ContainerBase, _FreqMixin, _VisMixin):
    """NS-beamformed visibilities: ``vis [pol, freq, ew, el, ra]`` c64, ``vis_weight [pol, freq, ew, ra]`` f32
    (``containers.py:1389-1428``); optional ``dirty_beam``, ``effective_ra``, ``nsample`` and, from a delay filter that
    kept them, ``filter`` and ``freq_cov`` ``[pol, freq, freq_sum, ew, ra]`` float64 (``containers.py:1459-1488``) via
    :meth:`add_dataset`; the ``freq_sum`` axis is a copy of ``freq``.  The complex forms of the last two are not
    provided."""

    _axes = ("pol", "freq", "freq_sum", "ew", "el", "ra")
    _dataset_spec = {
        "vis": {"axes": ["pol", "freq", "ew", "el", "ra"], "dtype": np.complex64},
        "vis_weight": {"axes": ["pol", "freq", "ew", "ra"], "dtype": np.float32},
    }

    _optional_spec = {
        "dirty_beam": {"axes": ["pol", "freq", "ew", "el", "ra"], "dtype": np.float32},  # containers.py:1409-1417
        # what SiderealRebinner adds (containers.py:1439-1458)
        "effective_ra": {"axes": ["pol", "freq", "ew", "ra"], "dtype": np.float32},
        "nsample": {"axes": ["pol", "freq", "ew", "ra"], "dtype": np.float32},
        # what DayenuDelayFilterHybridVis keeps (containers.py:1459-1488)
        "filter": {"axes": ["pol", "freq", "freq_sum", "ew", "ra"], "dtype": np.float64},
        "freq_cov": {"axes": ["pol", "freq", "freq_sum", "ew", "ra"], "dtype": np.float64},
    }
    _complex_datasets = ("complex_filter", "complex_freq_cov")

    @property
    def ra(self):
        return self.index_map["ra"]

    @property
    def filter(self):
        return self._optional("filter")

    @property
    def freq_cov(self):
        return self._optional("freq_cov")

    @property
    def complex_filter(self):
        raise NotImplementedError("HybridVisStream: complex filters are not supported")

    @property
    def complex_freq_cov(self):
        raise NotImplementedError("HybridVisStream: complex noise covariances are not supported")

    @property
    def effective_ra(self):
        return self._optional("effective_ra")

    @property
    def nsample(self):
        return self._optional("nsample")

    def __init__(self, ra=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(ra=ra, **kwargs)

    def add_dataset(self, name, allocate=False):
        if name in self._complex_datasets:
            raise NotImplementedError(f"HybridVisStream: the dataset {name!r} is not provided (complex filters are not supported)")
        self._dataset_spec[name] = self._optional_spec[name]
        if "freq_sum" in self._optional_spec[name]["axes"] and "freq_sum" not in self.index_map:
            self.index_map["freq_sum"] = self.index_map["freq"]  # (a copy of the frequency axis: the second index of a matrix)
            self.index_attrs.setdefault("freq_sum", {})
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=self._optional_spec[name]["dtype"]))

    @property
    def dirty_beam(self):
        return self.datasets["dirty_beam"]


class VisGridStream(ContainerBase, _FreqMixin, _VisMixin):
    """Visibilities on the (pol, ew, ns) baseline grid: ``vis [pol, freq, ew, ns, ra]`` c64, ``vis_weight`` f32, optional
    ``redundancy [pol, ew, ns, ra]`` int32 (``containers.py:1245-1299``)."""

    _axes = ("pol", "freq", "ew", "ns", "ra")
    _dataset_spec = {
        "vis": {"axes": ["pol", "freq", "ew", "ns", "ra"], "dtype": np.complex64},
        "vis_weight": {"axes": ["pol", "freq", "ew", "ns", "ra"], "dtype": np.float32},
    }
    _optional_spec = {"redundancy": {"axes": ["pol", "ew", "ns", "ra"], "dtype": np.int32}}

    def __init__(self, ra=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(ra=ra, **kwargs)

    def add_dataset(self, name, allocate=False):
        self._dataset_spec[name] = self._optional_spec[name]
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=np.int32))

    @property
    def redundancy(self):
        if "redundancy" in self.datasets:
            return self.datasets["redundancy"]
        raise KeyError("Dataset 'redundancy' not initialised.")


class FreqNoiseModel(ContainerBase, _FreqMixin):
    """Cholesky factors of the frequency-frequency noise covariance, for noise realisations on the baseline grid
    (``containers.py:1777-1837``): ``redundancy [pol, ew, ns]`` int32, ``weight [pol, freq, ew, ra]`` float32 and,
    through :meth:`add_dataset`, ``freq_cov [pol, ew, ra, freq, freq_sum]`` float64, the lower factor of every
    ``(pol, ew, ra)`` sample as one contiguous matrix; the ``freq_sum`` axis is a copy of ``freq``.  The complex form is
    not provided."""

    _axes = ("pol", "freq", "freq_sum", "ew", "ns", "ra")
    _dataset_spec = {
        "redundancy": {"axes": ["pol", "ew", "ns"], "dtype": np.int32},
        "weight": {"axes": ["pol", "freq", "ew", "ra"], "dtype": np.float32},
    }
    _optional_spec = {"freq_cov": {"axes": ["pol", "ew", "ra", "freq", "freq_sum"], "dtype": np.float64}}
    _complex_datasets = ("complex_freq_cov",)

    def __init__(self, ra=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(ra=ra, **kwargs)

    def add_dataset(self, name, allocate=False):
        if name in self._complex_datasets:
            raise NotImplementedError(f"FreqNoiseModel: the dataset {name!r} is not provided (complex covariances are not supported)")
        self._dataset_spec[name] = self._optional_spec[name]
        if "freq_sum" not in self.index_map:
            self.index_map["freq_sum"] = self.index_map["freq"]  # (a copy of the frequency axis: the second index of a matrix)
            self.index_attrs.setdefault("freq_sum", {})
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=self._optional_spec[name]["dtype"]))

    @property
    def ra(self):
        return self.index_map["ra"]

    @property
    def redundancy(self):
        return self.datasets["redundancy"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def freq_cov(self):
        return self._optional("freq_cov")

    @property
    def complex_freq_cov(self):
        raise NotImplementedError("FreqNoiseModel: complex noise covariances are not supported")


class HybridVisMModes(MContainer, _FreqMixin, _VisMixin):
    """m-mode transformed hybrid visibilities: ``vis [m, msign, pol, freq, ew, el]`` **complex64**,
    ``vis_weight [m, msign, pol, freq, ew]`` **float32** (``containers.py:1550-1574``)."""

    _axes = ("m", "msign", "pol", "freq", "ew", "el")
    _dataset_spec = {
        "vis": {"axes": ["m", "msign", "pol", "freq", "ew", "el"], "dtype": np.complex64},
        "vis_weight": {"axes": ["m", "msign", "pol", "freq", "ew"], "dtype": np.float32},
    }


class RingMap(ContainerBase, _FreqMixin):
    """Multi-frequency ring maps: ``map [beam, pol, freq, ra, el]``, ``weight [pol, freq, ra, el]`` float64
    (``containers.py:1577-1693``); optional ``dirty_beam``, ``dirty_beam_power``, ``rms`` and, from a foreground filter
    that kept them, ``filter`` and ``freq_cov`` ``[pol, freq, freq_sum, ra]`` float64 via :meth:`add_dataset`; the
    ``freq_sum`` axis is a copy of ``freq``.  The complex forms of the last two are not provided."""

    _axes = ("beam", "pol", "freq", "freq_sum", "ra", "el", "ew")
    _dataset_spec = {
        "map": {"axes": ["beam", "pol", "freq", "ra", "el"], "dtype": np.float64},
        "weight": {"axes": ["pol", "freq", "ra", "el"], "dtype": np.float64},
    }
    _optional_spec = {
        "dirty_beam": {"axes": ["beam", "pol", "freq", "ra", "el"], "dtype": np.float64},
        "dirty_beam_power": {"axes": ["beam", "pol", "freq", "el"], "dtype": np.float64},
        "rms": {"axes": ["pol", "freq", "ra"], "dtype": np.float64},  # containers.py:1643-1650
        "filter": {"axes": ["pol", "freq", "freq_sum", "ra"], "dtype": np.float64},  # containers.py:1654-1693
        "freq_cov": {"axes": ["pol", "freq", "freq_sum", "ra"], "dtype": np.float64},
    }
    _complex_datasets = ("complex_filter", "complex_freq_cov")

    def __init__(self, ra=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(ra=ra, **kwargs)

    def add_dataset(self, name, allocate=False):
        if name in self._complex_datasets:
            raise NotImplementedError(f"RingMap: the dataset {name!r} is not provided (complex filters are not supported)")
        self._dataset_spec[name] = self._optional_spec[name]
        if "freq_sum" in self._optional_spec[name]["axes"] and "freq_sum" not in self.index_map:
            self.index_map["freq_sum"] = self.index_map["freq"]  # (a copy of the frequency axis: the second index of a matrix)
            self.index_attrs.setdefault("freq_sum", {})
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=np.float64))

    @property
    def map(self):
        return self.datasets["map"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def dirty_beam(self):
        return self.datasets["dirty_beam"]

    @property
    def dirty_beam_power(self):
        return self.datasets["dirty_beam_power"]

    @property
    def rms(self):
        return self.datasets["rms"]

    @property
    def filter(self):
        return self.datasets["filter"]

    @property
    def freq_cov(self):
        return self.datasets["freq_cov"]

    @property
    def complex_filter(self):
        raise NotImplementedError("RingMap: complex filters are not supported")

    @property
    def complex_freq_cov(self):
        raise NotImplementedError("RingMap: complex noise covariances are not supported")


class SVDSpectrum(ContainerBase):
    """``spectrum [m, singularvalue]`` float64: the per-m SVD spectrum of MModes (``containers.py:2589-2607``)."""

    _axes = ("m", "singularvalue")
    _dataset_spec = {"spectrum": {"axes": ["m", "singularvalue"], "dtype": np.float64}}

    @property
    def spectrum(self):
        return self.datasets["spectrum"]


class SVDModes(MContainer, _VisMixin):
    """SVD-projected m-modes: ``vis [m, mode]`` complex128, ``vis_weight [m, mode]`` float64, ``nmode [m]`` int32
    (``containers.py:1196-1234``): per m the modes of every frequency packed back to back, ``nmode[m]`` of them."""

    _axes = ("m", "msign", "mode")
    _dataset_spec = {
        "vis": {"axes": ["m", "mode"], "dtype": np.complex128},
        "vis_weight": {"axes": ["m", "mode"], "dtype": np.float64},
        "nmode": {"axes": ["m"], "dtype": np.int32},
    }

    def __init__(self, mode=None, **kwargs):
        super().__init__(mode=mode, **kwargs)

    @property
    def nmode(self):
        return self.datasets["nmode"]


class KLModes(SVDModes):
    """KL-projected m-modes, same layout (``containers.py:1237-1246``)."""


class Map(ContainerBase, _FreqMixin):
    """``map [freq, pol, pixel]`` float64, HEALPix RING (``containers.py:470-486``, cora ``Map`` [3P])."""

    _axes = ("freq", "pol", "pixel")
    _dataset_spec = {"map": {"axes": ["freq", "pol", "pixel"], "dtype": np.float64}}

    def __init__(self, nside=None, polarisation=True, **kwargs):
        if nside is not None:
            kwargs["pixel"] = 12 * int(nside) ** 2
        if "pol" not in kwargs:
            kwargs["pol"] = np.array(["I", "Q", "U", "V"] if polarisation else ["I"])
        super().__init__(**kwargs)

    @property
    def map(self):
        return self.datasets["map"]

    @property
    def nside(self):
        return int(round((len(self.index_map["pixel"]) // 12) ** 0.5))


class DelayContainer(ContainerBase):
    """A container with a ``delay`` axis, in micro-seconds (``containers.py:2038-2046``)."""

    _axes = ("delay",)

    def __init__(self, weight_boost=1.0, **kwargs):
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(**kwargs)
        self.attrs["weight_boost"] = weight_boost

    def add_dataset(self, name, allocate=True):
        self._dataset_spec[name] = self._optional_spec[name]
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=self._optional_spec[name]["dtype"]), attrs={"axis": self._optional_spec[name]["axes"]})

    def create_index_map(self, name, values):
        """Carry the index map of an axis that was folded into ``baseline``."""
        self.index_map[name] = np.asarray(values)
        self.index_attrs.setdefault(name, {})

    @property
    def delay(self):
        return self.index_map["delay"]

    @property
    def spectrum(self):
        return self.datasets["spectrum"]

    @property
    def weight_boost(self):
        """The factor the weights were multiplied by when the spectrum was computed."""
        return self.attrs["weight_boost"]

    @property
    def freq(self):
        """The frequency axis of the input data (kept as an attribute)."""
        return self.attrs["freq"]


class DelaySpectrum(DelayContainer):
    """A delay POWER spectrum: ``spectrum [baseline, delay]`` float64; optional ``spectrum_samples [sample, baseline,
    delay]`` float64 and ``spectrum_mask [baseline]`` bool (``containers.py:2049-2110``)."""

    _axes = ("baseline", "sample", "delay")
    _dataset_spec = {"spectrum": {"axes": ["baseline", "delay"], "dtype": np.float64}}
    _optional_spec = {
        "spectrum_samples": {"axes": ["sample", "baseline", "delay"], "dtype": np.float64},
        "spectrum_mask": {"axes": ["baseline"], "dtype": np.bool_},
    }

    def __init__(self, weight_boost=1.0, sample=1, **kwargs):
        super().__init__(weight_boost=weight_boost, sample=sample, **kwargs)


class DelayTransform(DelayContainer):
    """A delay spectrum: ``spectrum [baseline, sample, delay]`` complex128; optional ``weight`` float32 of the same
    shape and ``spectrum_mask [baseline, sample]`` bool (``containers.py:2113-2182``)."""

    _axes = ("baseline", "sample", "delay")
    _dataset_spec = {"spectrum": {"axes": ["baseline", "sample", "delay"], "dtype": np.complex128}}
    _optional_spec = {
        "weight": {"axes": ["baseline", "sample", "delay"], "dtype": np.float32},
        "spectrum_mask": {"axes": ["baseline", "sample"], "dtype": np.bool_},
    }

    @property
    def weight(self):
        return self.datasets["weight"]


class DelayTransformOperator(DelayContainer):
    """The operator of a Wiener delay transform: ``filter [pol, ra, el, delay, freq]`` complex64, per pixel the matrix
    that takes the filtered map from frequency to delay (``containers.py:2185-2203``)."""

    _axes = ("pol", "ra", "el", "delay", "freq")
    _dataset_spec = {"filter": {"axes": ["pol", "ra", "el", "delay", "freq"], "dtype": np.complex64}}

    @property
    def filter(self):
        return self.datasets["filter"]


class CosmologyContainer(ContainerBase):
    """A container that carries the background cosmology its axes were computed with (``cosmology=``; by default
    that of ``attrs_from``): a :class:`draco_amd.util.cosmology.Cosmology` duck type, read back as ``.cosmology``."""

    def __init__(self, cosmology=None, **kwargs):
        super().__init__(**kwargs)
        if cosmology is None:
            cosmology = getattr(kwargs.get("attrs_from"), "cosmology", None)
        self._cosmology = cosmology

    @property
    def cosmology(self):
        return getattr(self, "_cosmology", None)  # (not written by `save`: a loaded container has none)

    def set_host(self, name, values):
        """Make ``values`` the (host) dataset ``name``; shape and dtype as the spec says."""
        spec = self._dataset_spec[name]
        arr = np.ascontiguousarray(values, dtype=spec["dtype"])
        if arr.shape != self.dataset_shape(name):
            raise ValueError(f"{name}: shape {arr.shape} != {self.dataset_shape(name)}")
        self.datasets[name] = Dataset(host=arr, attrs={"axis": spec["axes"]})
        return self.datasets[name]


_FOURIER_AXES_SPEC = {
    "kx": {"axes": ["u"], "dtype": np.float64},
    "ky": {"axes": ["v"], "dtype": np.float64},
    "kpara": {"axes": ["delay"], "dtype": np.float64},
    "uv_mask": {"axes": ["u", "v"], "dtype": np.bool_},
}


class Fourier3DContainer(CosmologyContainer, DelayContainer):
    """Base of the containers with Fourier axes ``(pol, delay, u, v)``: ``kx [u]``, ``ky [v]``, ``kpara [delay]``
    float64 in h / Mpc and ``uv_mask [u, v]`` bool (``containers.py:2206-2266``)."""

    _axes = ("pol", "delay", "u", "v")
    _dataset_spec = dict(_FOURIER_AXES_SPEC)

    kx = property(lambda self: self.datasets["kx"])
    ky = property(lambda self: self.datasets["ky"])
    kpara = property(lambda self: self.datasets["kpara"])
    uv_mask = property(lambda self: self.datasets["uv_mask"])
    redshift = property(lambda self: self.attrs["redshift"])
    freq_center = property(lambda self: self.attrs["freq_center"])


class SpatialDelayCube(Fourier3DContainer):
    """A delay cube in the ``(u, v)`` domain: ``vis [pol, delay, u, v]`` complex128 (``containers.py:2269-2285``)."""

    _dataset_spec = {**_FOURIER_AXES_SPEC, "vis": {"axes": ["pol", "delay", "u", "v"], "dtype": np.complex128}}

    vis = property(lambda self: self.datasets["vis"])


class PowerSpectrum3D(Fourier3DContainer):
    """A 3-D power spectrum: ``spectrum [pol, delay, u, v]`` complex128 (``containers.py:2288-2309``)."""

    _dataset_spec = {**_FOURIER_AXES_SPEC, "spectrum": {"axes": ["pol", "delay", "u", "v"], "dtype": np.complex128}}

    ps_norm = property(lambda self: self.attrs["ps_norm"])


class PowerSpectrum2D(CosmologyContainer):
    """A cylindrically averaged power spectrum over ``[pol, delay, uv_dist]``: ``spectrum`` complex128, ``weight``
    and ``neff`` float64, ``mask`` bool, with ``kpara [delay]`` and ``kperp [uv_dist]`` float64
    (``containers.py:2312-2391``)."""

    _axes = ("pol", "delay", "uv_dist")
    _dataset_spec = {
        "spectrum": {"axes": ["pol", "delay", "uv_dist"], "dtype": np.complex128},
        "weight": {"axes": ["pol", "delay", "uv_dist"], "dtype": np.float64},
        "neff": {"axes": ["pol", "delay", "uv_dist"], "dtype": np.float64},
        "mask": {"axes": ["pol", "delay", "uv_dist"], "dtype": np.bool_},
        "kpara": {"axes": ["delay"], "dtype": np.float64},
        "kperp": {"axes": ["uv_dist"], "dtype": np.float64},
    }

    spectrum = property(lambda self: self.datasets["spectrum"])
    weight = property(lambda self: self.datasets["weight"])
    neff = property(lambda self: self.datasets["neff"])
    mask = property(lambda self: self.datasets["mask"])
    kpara = property(lambda self: self.datasets["kpara"])
    kperp = property(lambda self: self.datasets["kperp"])
    delay_cut = property(lambda self: self.attrs["delay_cut"])


class PowerSpectrum1D(CosmologyContainer):
    """A spherically averaged power spectrum over ``[pol, k]``: ``spectrum`` complex128, ``samp_var``, ``var``,
    ``neff`` and ``k1D`` float64 (``containers.py:2394-2455``)."""

    _axes = ("pol", "k")
    _dataset_spec = {
        "spectrum": {"axes": ["pol", "k"], "dtype": np.complex128},
        "samp_var": {"axes": ["pol", "k"], "dtype": np.float64},
        "var": {"axes": ["pol", "k"], "dtype": np.float64},
        "neff": {"axes": ["pol", "k"], "dtype": np.float64},
        "k1D": {"axes": ["pol", "k"], "dtype": np.float64},
    }

    spectrum = property(lambda self: self.datasets["spectrum"])
    samp_var = property(lambda self: self.datasets["samp_var"])
    var = property(lambda self: self.datasets["var"])
    neff = property(lambda self: self.datasets["neff"])
    k1D = property(lambda self: self.datasets["k1D"])


_POSITION_DTYPE = np.dtype([("ra", np.float64), ("dec", np.float64)])
_REDSHIFT_DTYPE = np.dtype([("z", np.float64), ("z_error", np.float64)])


class SourceCatalog(ContainerBase):
    """A catalogue of sources: the table ``position [object_id]`` with columns ``ra``, ``dec`` in degrees
    (``containers.py:2745-2758``)."""

    _axes = ("object_id",)
    _dataset_spec = {"position": {"axes": ["object_id"], "dtype": _POSITION_DTYPE}}

    @property
    def position(self):
        return self.datasets["position"]


class SpectroscopicCatalog(SourceCatalog):
    """A catalogue with the table ``redshift [object_id]``, columns ``z``, ``z_error``, beside ``position``
    (``containers.py:2761-2769``)."""

    _dataset_spec = {
        "position": {"axes": ["object_id"], "dtype": _POSITION_DTYPE},
        "redshift": {"axes": ["object_id"], "dtype": _REDSHIFT_DTYPE},
    }

    @property
    def redshift(self):
        return self.datasets["redshift"]


class FormedBeam(ContainerBase, _FreqMixin):
    """Formed beams: ``beam`` and ``weight [object_id, pol, freq]`` float64, ``position [object_id]`` and the optional
    ``redshift [object_id]`` (``containers.py:2772-2840``)."""

    _axes = ("object_id", "pol", "freq")
    _dataset_spec = {
        "beam": {"axes": ["object_id", "pol", "freq"], "dtype": np.float64},
        "weight": {"axes": ["object_id", "pol", "freq"], "dtype": np.float64},
        "position": {"axes": ["object_id"], "dtype": _POSITION_DTYPE},
    }
    _optional_spec = {"redshift": {"axes": ["object_id"], "dtype": _REDSHIFT_DTYPE}}

    def __init__(self, **kwargs):
        self._dataset_spec = dict(type(self)._dataset_spec)
        super().__init__(**kwargs)

    def add_dataset(self, name, allocate=True):
        self._dataset_spec[name] = self._optional_spec[name]
        if allocate:
            self.datasets[name] = Dataset(host=np.zeros(self.dataset_shape(name), dtype=self._optional_spec[name]["dtype"]), attrs={"axis": self._optional_spec[name]["axes"]})

    @property
    def beam(self):
        return self.datasets["beam"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def position(self):
        return self.datasets["position"]

    @property
    def redshift(self):
        if "redshift" in self.datasets:
            return self.datasets["redshift"]
        raise KeyError("Dataset 'redshift' not initialised.")

    @property
    def frequency(self):
        return self.index_map["freq"]

    @property
    def id(self):
        return self.index_map["object_id"]

    @property
    def pol(self):
        return self.index_map["pol"]


class FormedBeamHA(FormedBeam):
    """Formed beams that keep the hour-angle axis: ``beam`` and ``weight [object_id, pol, freq, ha]`` float64 and
    ``object_ha [object_id, ha]``, which ``.ha`` returns (``containers.py:2843-2883``)."""

    _axes = ("object_id", "pol", "freq", "ha")
    _dataset_spec = {
        "beam": {"axes": ["object_id", "pol", "freq", "ha"], "dtype": np.float64},
        "weight": {"axes": ["object_id", "pol", "freq", "ha"], "dtype": np.float64},
        "position": {"axes": ["object_id"], "dtype": _POSITION_DTYPE},
        "object_ha": {"axes": ["object_id", "ha"], "dtype": np.float64},
    }

    @property
    def ha(self):
        return self.datasets["object_ha"]


class FrequencyStack(ContainerBase, _FreqMixin):
    """The stack of formed beams over the sources of a catalogue: ``stack`` and ``weight [freq]`` float64, ``freq`` the
    offset from the sources' line frequency (``containers.py:2610-2639``)."""

    _axes = ("freq",)
    _dataset_spec = {"stack": {"axes": ["freq"], "dtype": np.float64}, "weight": {"axes": ["freq"], "dtype": np.float64}}

    @property
    def stack(self):
        return self.datasets["stack"]

    @property
    def weight(self):
        return self.datasets["weight"]


class FrequencyStackByPol(FrequencyStack):
    """A frequency stack split by polarisation: ``[pol, freq]`` (``containers.py:2642-2665``)."""

    _axes = ("pol", "freq")
    _dataset_spec = {"stack": {"axes": ["pol", "freq"], "dtype": np.float64}, "weight": {"axes": ["pol", "freq"], "dtype": np.float64}}

    @property
    def pol(self):
        return self.index_map["pol"]


class MockFrequencyStack(FrequencyStack):
    """Frequency stacks of many mock catalogues: ``[mock, freq]`` (``containers.py:2668-2689``)."""

    _axes = ("mock", "freq")
    _dataset_spec = {"stack": {"axes": ["mock", "freq"], "dtype": np.float64}, "weight": {"axes": ["mock", "freq"], "dtype": np.float64}}


class MockFrequencyStackByPol(FrequencyStackByPol):
    """Frequency stacks by polarisation of many mock catalogues: ``[mock, pol, freq]`` (``containers.py:2692-2713``)."""

    _axes = ("mock", "pol", "freq")
    _dataset_spec = {"stack": {"axes": ["mock", "pol", "freq"], "dtype": np.float64}, "weight": {"axes": ["mock", "pol", "freq"], "dtype": np.float64}}


class Stack3D(ContainerBase, _FreqMixin):
    """A 3-D stack of ring-map patches: ``stack`` and ``weight [pol, delta_ra, delta_dec, freq]`` float64
    (``containers.py:2716-2742``)."""

    _axes = ("pol", "delta_ra", "delta_dec", "freq")
    _dataset_spec = {
        "stack": {"axes": ["pol", "delta_ra", "delta_dec", "freq"], "dtype": np.float64},
        "weight": {"axes": ["pol", "delta_ra", "delta_dec", "freq"], "dtype": np.float64},
    }

    @property
    def stack(self):
        return self.datasets["stack"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def pol(self):
        return self.index_map["pol"]


class GridBeam(ContainerBase, _FreqMixin):
    """A beam on a rectangular grid: ``beam [freq, pol, input, theta, phi]`` complex64, ``weight`` float32 of the same
    shape, ``attrs["coords"]`` (``containers.py:883-954``; ``quality`` and ``gain`` are not carried)."""

    _axes = ("freq", "pol", "input", "theta", "phi")
    _dataset_spec = {
        "beam": {"axes": ["freq", "pol", "input", "theta", "phi"], "dtype": np.complex64},
        "weight": {"axes": ["freq", "pol", "input", "theta", "phi"], "dtype": np.float32},
    }

    def __init__(self, coords="celestial", **kwargs):
        super().__init__(**kwargs)
        self.attrs["coords"] = coords

    @property
    def beam(self):
        return self.datasets["beam"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def coords(self):
        return self.attrs["coords"]

    @property
    def pol(self):
        return self.index_map["pol"]

    @property
    def input(self):
        return self.index_map["input"]

    @property
    def theta(self):
        return self.index_map["theta"]

    @property
    def phi(self):
        return self.index_map["phi"]


class _TimeAxisMixin:
    def __init__(self, time=None, **kwargs):
        if time is not None and not isinstance(time, (int, np.integer)):
            time = np.asarray(time, dtype=np.float64)
        super().__init__(time=time, **kwargs)

    @property
    def time(self):
        return self.index_map["time"]


class _RaAxisMixin:
    def __init__(self, ra=None, **kwargs):
        if isinstance(ra, (int, np.integer)):
            ra = np.linspace(0.0, 360.0, int(ra), endpoint=False)
        super().__init__(ra=ra, **kwargs)

    @property
    def ra(self):
        return self.index_map["ra"]


class _MaskMixin:
    @property
    def mask(self):
        return self.datasets["mask"]

    @property
    def pol(self):
        return self.index_map["pol"]


class SystemSensitivity(_TimeAxisMixin, ContainerBase, _FreqMixin):
    """The total system sensitivity: ``measured``, ``radiometer`` and ``weight [freq, pol, time]`` float32 and
    ``frac_lost [freq, time]`` float32 (``containers.py:596-658``)."""

    _axes = ("freq", "pol", "time")
    _dataset_spec = {
        "measured": {"axes": ["freq", "pol", "time"], "dtype": np.float32},
        "radiometer": {"axes": ["freq", "pol", "time"], "dtype": np.float32},
        "weight": {"axes": ["freq", "pol", "time"], "dtype": np.float32},
        "frac_lost": {"axes": ["freq", "time"], "dtype": np.float32},
    }

    @property
    def measured(self):
        return self.datasets["measured"]

    @property
    def radiometer(self):
        return self.datasets["radiometer"]

    @property
    def weight(self):
        return self.datasets["weight"]

    @property
    def frac_lost(self):
        return self.datasets["frac_lost"]

    @property
    def pol(self):
        return self.index_map["pol"]


class RFIMask(_TimeAxisMixin, ContainerBase, _FreqMixin, _MaskMixin):
    """An RFI mask for a timestream: ``mask [freq, time]`` bool, True for contaminated samples (``containers.py:661-681``)."""

    _axes = ("freq", "time")
    _dataset_spec = {"mask": {"axes": ["freq", "time"], "dtype": np.bool_}}


class RFIMaskByPol(RFIMask):
    """A polarisation-dependent RFI mask: ``mask [pol, freq, time]`` bool (``containers.py:684-706``)."""

    _axes = ("pol", "freq", "time")
    _dataset_spec = {"mask": {"axes": ["pol", "freq", "time"], "dtype": np.bool_}}


class SiderealRFIMask(_RaAxisMixin, ContainerBase, _FreqMixin, _MaskMixin):
    """An RFI mask for a sidereal stream: ``mask [freq, ra]`` bool (``containers.py:709-729``)."""

    _axes = ("freq", "ra")
    _dataset_spec = {"mask": {"axes": ["freq", "ra"], "dtype": np.bool_}}


class SiderealRFIMaskByPol(SiderealRFIMask):
    """A polarisation-dependent RFI mask as a function of RA: ``mask [pol, freq, ra]`` bool (``containers.py:732-754``)."""

    _axes = ("pol", "freq", "ra")
    _dataset_spec = {"mask": {"axes": ["pol", "freq", "ra"], "dtype": np.bool_}}


class RingMapMask(_RaAxisMixin, ContainerBase, _FreqMixin, _MaskMixin):
    """Mask of bad ring-map pixels: ``mask [pol, freq, ra, el]`` bool (``containers.py:1730-1748``)."""

    _axes = ("pol", "freq", "ra", "el")
    _dataset_spec = {"mask": {"axes": ["pol", "freq", "ra", "el"], "dtype": np.bool_}}


class _BandpassMixin:
    @property
    def pol(self):
        return self.index_map["pol"]

    @property
    def bandpass(self):
        return self.datasets["bandpass"]

    @property
    def window(self):
        return self.datasets["window"]

    @property
    def comp_bandpass(self):
        return self.datasets["comp_bandpass"]

    @property
    def sval(self):
        return self.datasets["sval"]


class VisBandpassWindow(ContainerBase, _FreqMixin, _BandpassMixin):
    """Bandpass gains estimated by HyFoReS and their window: ``bandpass [pol, freq]``, ``window [pol, freq, freq]``
    complex128 (``containers.py:3172-3201``).  Kilobytes: host resident."""

    _axes = ("pol", "freq")
    _dataset_spec = {
        "bandpass": {"axes": ["pol", "freq"], "dtype": np.complex128},
        "window": {"axes": ["pol", "freq", "freq"], "dtype": np.complex128},
    }


class VisBandpassCompensate(ContainerBase, _FreqMixin, _BandpassMixin):
    """Window-compensated bandpass gains: ``comp_bandpass`` and ``sval [pol, freq]`` complex128
    (``containers.py:3204-3233``)."""

    _axes = ("pol", "freq")
    _dataset_spec = {
        "comp_bandpass": {"axes": ["pol", "freq"], "dtype": np.complex128},
        "sval": {"axes": ["pol", "freq"], "dtype": np.complex128},
    }


class VisBandpassWindowBaseline(VisBandpassWindow):
    """:class:`VisBandpassWindow` per east-west baseline: ``bandpass [pol, ew, freq]``, ``window [pol, ew, freq, freq]``
    complex128 (``containers.py:3236-3264``)."""

    _axes = ("pol", "ew", "freq")
    _dataset_spec = {
        "bandpass": {"axes": ["pol", "ew", "freq"], "dtype": np.complex128},
        "window": {"axes": ["pol", "ew", "freq", "freq"], "dtype": np.complex128},
    }


class VisBandpassCompensateBaseline(VisBandpassCompensate):
    """:class:`VisBandpassCompensate` per east-west baseline: ``comp_bandpass`` and ``sval [pol, ew, freq]`` complex128
    (``containers.py:3267-3295``); the clean task sets the attributes ``rank [pol, ew]`` and ``cutoff``."""

    _axes = ("pol", "ew", "freq")
    _dataset_spec = {
        "comp_bandpass": {"axes": ["pol", "ew", "freq"], "dtype": np.complex128},
        "sval": {"axes": ["pol", "ew", "freq"], "dtype": np.complex128},
    }


def _all_containers():
    found, todo = [], [ContainerBase]
    while todo:
        c = todo.pop()
        for sub in c.__subclasses__():
            found.append(sub)
            todo.append(sub)
    return found
