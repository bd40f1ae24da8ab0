"""Generate tests/golden/regrid.npz and tests/golden/sidereal_stack.npz by EXECUTING the reference's own
``LanczosRegridder._regrid``, ``SiderealRegridder.process`` and ``SiderealStacker.process / process_finish`` from
source (through ``oracle._refstub``).  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_regrid.py

The one compiled helper on this path, ``_fast_tools._linear_covariance_banded`` (``_fast_tools.pyx:59-88``), gets a
plain NumPy stand-in of its loop.  Per regrid case the file also records ``e_ref`` = max |reference - float64 twin| /
max |twin| (``tests/regrid_twin.py``): the reference forms its right-hand side in float32, the tests' tolerance
against the reference vectors is built from that measured distance.
"""

import logging
import os
import sys
import types

import numpy as np
import scipy.constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import regrid_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _linear_covariance_banded(Rn, Ni, start_ind, end_ind, bw):
    n = Rn.shape[0]
    Ci = np.zeros((bw + 1, n), dtype=np.float64)
    for beta in range(n):
        si, ei = start_ind[beta], end_ind[beta]
        for alpha in range(max(0, bw - beta), bw + 1):
            betap = alpha + beta - bw
            t = 0.0
            for j in range(si, ei):
                t = t + Rn[betap, j] * Rn[beta, j] * Ni[j]
            Ci[alpha, beta] = t
    return Ci


class LA(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    @property
    def local_array(self):
        return self.view(np.ndarray)

    @property
    def local_shape(self):
        return self.shape

    local_bounds = slice(None)


class DS:
    def __init__(self, arr, axis):
        self.arr = np.asarray(arr).view(LA)
        self.attrs = {"axis": list(axis)}

    def __getitem__(self, k):
        return self.arr[k]

    def __setitem__(self, k, v):
        self.arr[k] = v

    @property
    def dtype(self):
        return self.arr.dtype


_SPEC = {
    "vis": (("freq", "stack", "ra"), np.complex64),
    "vis_weight": (("freq", "stack", "ra"), np.float32),
    "nsample": (("freq", "stack", "ra"), np.uint16),
    "sample_variance": (("component", "freq", "stack", "ra"), np.float32),
}


class FakeStream:
    """Stand-in for SiderealStream / TimeStream (last axis ``ra`` or ``time``)."""

    def __init__(self, freq, prodstack, last, last_name="ra", attrs=None, names=("vis", "vis_weight")):
        self.freq = np.asarray(freq, dtype=np.float64)
        self.prodstack = prodstack
        self.index_map = {"freq": self.freq, last_name: np.asarray(last, dtype=np.float64), "component": np.arange(3)}
        self.last_name = last_name
        self.attrs = dict(attrs or {})
        self.comm = None
        self.datasets = {}
        for n in names:
            self.add_dataset(n)

    def add_dataset(self, name):
        axes, dt = _SPEC[name]
        axes = tuple(self.last_name if a == "ra" else a for a in axes)
        n = {"freq": len(self.freq), "stack": len(self.prodstack), self.last_name: len(self.index_map[self.last_name]), "component": 3}
        self.datasets[name] = DS(np.zeros([n[a] for a in axes], dtype=dt), axes)

    vis = property(lambda s: s.datasets["vis"])
    weight = property(lambda s: s.datasets["vis_weight"])
    nsample = property(lambda s: s.datasets["nsample"])
    sample_variance = property(lambda s: s.datasets["sample_variance"])
    ra = property(lambda s: s.index_map["ra"])
    time = property(lambda s: s.index_map["time"])

    def redistribute(self, axis):
        pass


class FakeSidereal(FakeStream):
    def __init__(self, attrs_from=None, axes_from=None, ra=None):
        super().__init__(axes_from.freq, axes_from.prodstack, np.linspace(0.0, 360.0, ra, endpoint=False), "ra", attrs_from.attrs)


class Observer:
    """Linear time map, feed mask, baselines, latitude: all stored in the fixture."""

    def __init__(self, nfeed, baselines, feedmask, latitude, t0, day):
        self.baselines, self.feedmask, self.latitude, self.t0, self.day = baselines, feedmask, latitude, t0, day

    def unix_to_lsd(self, t):
        return (np.asarray(t, dtype=np.float64) - self.t0) / self.day


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    t.comm = types.SimpleNamespace(Barrier=lambda: None)
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def sample_times(rng, nt, lo, hi, jitter, gap=None):
    t = np.linspace(lo, hi, nt) + jitter * (hi - lo) / nt * rng.uniform(-0.5, 0.5, nt)
    t = np.sort(t)
    if gap is not None:
        t = t[(t < gap[0]) | (t > gap[1])]
    return t


def make_rows(rng, times, nrow, flag=0.3, zero_row=None):
    nt = len(times)
    ph = rng.uniform(0, 2 * np.pi, (nrow, 3, 1))
    fr = rng.uniform(2.0, 25.0, (nrow, 3, 1))
    vis = (np.exp(1j * (2 * np.pi * fr * (times - times[0])[None, None, :] + ph)) * rng.uniform(0.5, 2, (nrow, 3, 1))).sum(axis=1)
    vis = (vis + 0.05 * (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt)))).astype(np.complex64)
    w = rng.uniform(0.5, 2.0, (nrow, nt)).astype(np.float32)
    w[rng.uniform(size=(nrow, nt)) < flag] = 0.0
    if zero_row is not None:
        w[zero_row] = 0.0
    return vis, w


def gen_regrid(transform, sidereal):
    out = {}
    rng = np.random.default_rng(20240611)
    # ---- LanczosRegridder._regrid: name -> (samples, nt, kernel_width, jitter, gap, start, end, mask_zero_weight)
    cases = {
        "over_kw5": (128, 300, 5, 0.8, (0.40, 0.47), 0.0, 1.0, False),
        "under_kw5": (128, 100, 5, 0.8, None, 0.0, 1.0, False),
        "over_kw3": (64, 160, 3, 0.6, (0.2, 0.32), 0.0, 1.0, True),
        "under_kw3": (96, 80, 3, 0.5, None, 0.0, 1.0, True),
        "inside_kw5": (64, 400, 5, 0.8, (0.55, 0.6), 0.25, 0.8, False),
    }
    names = []
    for name, (samples, nt, kw, jit, gap, start, end, mzw) in cases.items():
        times = sample_times(rng, nt, -0.02, 1.02, jit, gap)
        vis, w = make_rows(rng, times, 6, zero_row=4)
        task = make_task(transform.LanczosRegridder, samples=samples, start=start, end=end, kernel_width=kw, epsilon=1e-3, mask_zero_weight=mzw)
        grid, sts, ni = task._regrid(vis.copy().reshape(2, 3, -1), w.copy().reshape(2, 3, -1), times)
        assert sts.dtype == np.complex64 and ni.dtype == np.float32 and not sts[1, 1].any() and not ni[1, 1].any()
        xt, nwt = twin.band_wiener_twin(vis, w, times, samples, start, end, kw, 1e-3, mzw)
        e_ref = np.abs(sts.reshape(6, -1) - xt).max() / np.abs(xt).max()
        e_w = np.abs(ni.reshape(6, -1) - nwt).max() / np.abs(nwt).max()
        print(f"regrid {name}: nt={len(times)} e_ref={e_ref:.3e} weight rel={e_w:.3e}")
        for k, v in dict(times=times, vis=vis, weight=w, grid=grid, out_vis=sts, out_weight=ni, e_ref=e_ref, cfg=np.array([samples, kw, int(mzw)]), bounds=np.array([start, end])).items():
            out[f"regrid/{name}/{k}"] = v
        names.append(name)
    out["regrid/names"] = np.array(names)

    # ---- SiderealRegridder.process: both container kinds, down_mix on and off
    nfreq, nstack, nfeed, samples, lsd = 2, 4, 4, 96, 312
    freq = np.array([600.0, 612.5])
    prodstack = np.array([(0, 1), (0, 2), (1, 3), (0, 3)], dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    baselines = np.array([[0.0, 0.3], [22.0, 0.0], [22.0, 0.6], [44.0, -0.3]])
    feedmask = np.ones((nfeed, nfeed), dtype=bool)
    feedmask[1, 3] = feedmask[3, 1] = False
    t0, day, latitude = 1.6e9, 86164.0905, 49.3
    obs = Observer(nfeed, baselines, feedmask, latitude, t0, day)
    for k, v in dict(freq=freq, prodstack=prodstack, baselines=baselines, feedmask=feedmask, obs=np.array([t0, day, latitude]), lsd=np.array(lsd), samples=np.array(samples)).items():
        out[f"task/{k}"] = v
    tnames = []
    for kind in ("time", "ra"):
        lsds = sample_times(rng, 230, lsd - 0.03, lsd + 1.03, 0.7, (lsd + 0.61, lsd + 0.66))
        if kind == "ra":
            lsds = lsds[(lsds >= lsd - 1e-9)]
            last = (lsds - lsd) * 360.0  # an RA axis running past 360: the day and the start of the next
        else:
            last = t0 + lsds * day
        vis, w = make_rows(rng, lsds, nfreq * nstack, zero_row=5)
        # fringes of a source at zenith, so that mixing down matters
        ph = twin.fringe_phase(freq, baselines[:, 0], np.ones(nstack), latitude, lsds)
        vis = (vis.reshape(nfreq, nstack, -1) * 0.3 + np.conj(ph)).astype(np.complex64)
        w = w.reshape(nfreq, nstack, -1)
        out[f"task/{kind}/axis"], out[f"task/{kind}/vis"], out[f"task/{kind}/weight"] = last, vis, w
        for mix in (False, True):
            data = FakeStream(freq, prodstack, last, kind, {"lsd": lsd})
            data.vis[:] = vis
            data.weight[:] = w
            task = make_task(sidereal.SiderealRegridder, samples=samples, kernel_width=5, epsilon=1e-3, mask_zero_weight=False, down_mix=mix, observer=obs)
            sd = task.process(data)
            src = obs.unix_to_lsd(last) if kind == "time" else lsd + last / 360.0
            y = vis.astype(np.complex128)
            if mix:
                y = y * twin.fringe_phase(freq, baselines[:, 0], feedmask[prodstack["input_a"], prodstack["input_b"]], latitude, src)
            xt, nwt = twin.band_wiener_twin(y.reshape(nfreq * nstack, -1), w.reshape(nfreq * nstack, -1), src, samples, lsd, lsd + 1, 5, 1e-3)
            if mix:
                grid = lsd + np.arange(samples) / samples
                xt = xt * np.conj(twin.fringe_phase(freq, baselines[:, 0], feedmask[prodstack["input_a"], prodstack["input_b"]], latitude, grid)).reshape(nfreq * nstack, -1)
            e_ref = np.abs(np.asarray(sd.vis[:]).reshape(nfreq * nstack, -1) - xt).max() / np.abs(xt).max()
            nm = f"{kind}_mix{int(mix)}"
            print(f"task {nm}: e_ref={e_ref:.3e} tag={sd.attrs['tag']}")
            out[f"task/{nm}/out_vis"], out[f"task/{nm}/out_weight"], out[f"task/{nm}/e_ref"] = np.asarray(sd.vis[:]), np.asarray(sd.weight[:]), e_ref
            out[f"task/{nm}/tag"] = np.array(sd.attrs["tag"])
            tnames.append(nm)
    out["task/names"] = np.array(tnames)
    path = os.path.join(GOLDEN, "regrid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def gen_stack(sidereal):
    out = {}
    rng = np.random.default_rng(77001)
    nfreq, nstack, nra, ndays = 2, 3, 40, 4
    freq = np.array([600.0, 601.0])
    prodstack = np.zeros(nstack, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    sky = rng.normal(size=(nfreq, nstack, nra)) + 1j * rng.normal(size=(nfreq, nstack, nra))
    days = []
    for d in range(ndays):
        vis = (sky + 0.2 * (rng.normal(size=sky.shape) + 1j * rng.normal(size=sky.shape))).astype(np.complex64)
        w = rng.uniform(0.5, 30.0, sky.shape).astype(np.float32)
        w[rng.uniform(size=sky.shape) < 0.1] = 0.0
        if d == 1:
            w[:, :, 10:22] = 0.0  # a day with a zero-weight region
        w[0, 1, 5] = 0.0  # never observed
        if d != 2:
            w[1, 2, 7] = 0.0  # observed once
        days.append((vis, w))
        out[f"day{d}/vis"], out[f"day{d}/weight"] = vis, w
    out["lsd"] = np.arange(100, 100 + ndays)
    for weight in ("uniform", "inverse_variance"):
        for var in (False, True):
            task = make_task(sidereal.SiderealStacker, tag="stack", weight=weight, with_sample_variance=var)
            task.stack = None
            key = f"{weight}_var{int(var)}"
            for d, (vis, w) in enumerate(days):
                s = FakeStream(freq, prodstack, np.linspace(0, 360, nra, endpoint=False), "ra", {"lsd": 100 + d})
                s.vis[:] = vis
                s.weight[:] = w
                task.process(s)
                for n, ds in task.stack.datasets.items():
                    out[f"{key}/after{d}/{n}"] = np.array(ds[:])
            st = task.process_finish()
            for n, ds in st.datasets.items():
                out[f"{key}/final/{n}"] = np.array(ds[:])
            assert list(st.attrs["lsd"]) == list(range(100, 100 + ndays)) and st.attrs["tag"] == "stack"
            print(f"stack {key}: datasets {sorted(st.datasets)} max nsample {st.nsample[:].max()}")
    out["ndays"] = np.array(ndays)
    path = os.path.join(GOLDEN, "sidereal_stack.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def main():
    transform, _ = _refstub.load_reference()
    import importlib

    ft = importlib.import_module("draco.util._fast_tools")
    ft._linear_covariance_banded = _linear_covariance_banded
    sidereal = importlib.import_module("draco.analysis.sidereal")
    sidereal.constants = types.SimpleNamespace(c=scipy.constants.c)
    sidereal.containers = types.SimpleNamespace(SiderealStream=FakeSidereal)
    sidereal.tools.invert_no_zero = _refstub._invert_no_zero
    sidereal.mpiarray = types.SimpleNamespace(zeros=lambda shape, axis=0, comm=None, dtype=None: np.zeros(shape, dtype=dtype))

    def empty_like(s):
        return FakeStream(s.freq, s.prodstack, s.index_map[s.last_name], s.last_name, s.attrs)

    sidereal.empty_like = empty_like
    gen_regrid(transform, sidereal)
    gen_stack(sidereal)


if __name__ == "__main__":
    main()
