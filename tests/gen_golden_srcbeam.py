"""Generate tests/golden/srcbeam.npz by EXECUTING the reference's own ``tools.polarization_map``, ``baseline_vector``,
``calculate_redundancy``, ``BeamForm.process``, ``BeamFormCat.process``, the ``GridBeam`` mixin
(``BeamFormExternalCat``) and ``_fast_tools.beamform`` from source (through ``oracle._refstub``, unmodified).  The
reference's ``_fast_tools.pyx`` is compiled with the installed Cython and gcc into a temporary directory outside the
repository and imported in place of the stub; nothing compiled or copied from the reference is kept, only the data.
On the imported modules ``containers`` and ``io`` are small stand-ins (NumPy arrays with the attributes the tasks
touch), the ``config.enum`` attributes are set on the instances (the stub returns ``None`` for them) and the constants
(``nu21``, ``c``, ``SIDEREAL_S``) carry their public values.  Run where the reference checkout exists:

    python tests/gen_golden_srcbeam.py

Per case the file holds the reference's outputs, the truth (``tests/srcbeam_twin.py`` in long double, rounded to
float64), ``e_ref`` (the reference against the truth), ``e_f64`` (the float64 twin against the truth), for beam and
weight in the measures of the twin, ``norm`` (the size of what was summed) and ``P_max``; the inputs (one sidereal
stream, one time stream, one catalogue, one grid beam) are stored once.

Asserted here, so that the reference is well determined on the inputs: ``ha_side`` and every ``ha_side / cos(dec)``
lie 1e-6 or more from an integer; no source frequency lies within 1 % of a channel width of the midpoint between two
channels; no time-stream source lies within 1 % of the ``1.5 cadence`` cut; the interpolated grid-beam flags lie 1e-3
or more from 0.99 and 1.01; no non-zero ``sum pb^2 SW`` is below 1e-6 of the largest.
"""

import importlib.util
import logging
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import srcbeam_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FREQ, TIMETRACK = twin.FREQ, twin.TIMETRACK
NRA, NTIME, CADENCE = 64, 40, 1300.0

CASES = twin.CASES


def compile_fast_tools():
    """The reference's Cython module, built in a temporary directory and imported from there."""
    tmp = tempfile.mkdtemp(prefix="srcbeam_ref_")
    c_file, so = os.path.join(tmp, "_fast_tools.c"), os.path.join(tmp, "_fast_tools.so")
    subprocess.run([sys.executable, "-m", "cython", "-3", os.path.join(_refstub.REFERENCE_ROOT, "draco", "util", "_fast_tools.pyx"), "-o", c_file], check=True)
    subprocess.run(["gcc", "-shared", "-fPIC", "-O2", "-w", "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(), c_file, "-o", so, "-lm"], check=True)
    spec = importlib.util.spec_from_file_location("draco.util._fast_tools", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, tmp


class LA(np.ndarray):
    local_offset = property(lambda s: (0,) * s.ndim)
    local_shape = property(lambda s: s.shape)
    local_array = property(lambda s: np.asarray(s))


class RefData:
    """What ``_process_data`` touches of a stream."""

    def __init__(self, tel, d):
        inputs, prod, stack, rev = twin.make_index_maps(tel)
        fm = np.zeros(len(d["freq"]), dtype=[("centre", np.float64), ("width", np.float64)])
        fm["centre"], fm["width"] = d["freq"], 2.0
        self.index_map = {"freq": fm, "input": inputs, "prod": prod, "stack": stack}
        self.reverse_map = {"stack": rev}
        self.attrs = {"tag": d["tag"]}
        if d["is_sstream"]:
            self.index_map["ra"] = np.asarray(d["ra"])
            self.attrs["lsd"] = d["lsd"]
        else:
            self.index_map["time"] = np.asarray(d["time"])
            self.time = self.index_map["time"]
        self.vis = np.asarray(d["vis"]).view(LA)
        self.weight = np.asarray(d["weight"]).view(LA)
        self.input_flags = np.asarray(d["input_flags"], dtype=np.float32)
        self.comm = types.SimpleNamespace(allgather=lambda x: [x])

    def redistribute(self, axis):
        pass


class RefCatalog:
    def __init__(self, cat, tag):
        n = len(cat["ra"])
        self.index_map = {"object_id": np.arange(n)}
        pos = np.zeros(n, dtype=[("ra", np.float64), ("dec", np.float64)])
        pos["ra"], pos["dec"] = cat["ra"], cat["dec"]
        red = np.zeros(n, dtype=[("z", np.float64), ("z_error", np.float64)])
        red["z"] = cat["z"]
        self.datasets = {"position": pos, "redshift": red}
        self.attrs = {"tag": tag, "coordinates": "CIRS"}

    def __contains__(self, k):
        return k in self.datasets

    def __getitem__(self, k):
        return self.datasets[k]


class RefFormedBeam:
    _ha = False

    def __init__(self, freq=None, object_id=None, pol=None, ha=None, distributed=True):
        shape = (len(object_id), len(pol), len(freq)) + ((len(ha),) if self._ha else ())
        self.beam, self.weight = np.zeros(shape), np.zeros(shape)
        if self._ha:
            self.ha = np.zeros((len(object_id), len(ha)))
        self.attrs = {}
        self.datasets = {"position": np.zeros(len(object_id), dtype=[("ra", np.float64), ("dec", np.float64)])}
        self._n = len(object_id)

    def add_dataset(self, name):
        self.datasets[name] = np.zeros(self._n, dtype=[("z", np.float64), ("z_error", np.float64)])

    def __getitem__(self, k):
        return self.datasets[k]

    def redistribute(self, axis):
        pass


class RefFormedBeamHA(RefFormedBeam):
    _ha = True


class RefGridBeam:
    def __init__(self, g):
        self.coords = "celestial"
        self.input = np.arange(1)
        self.freq, self.pol, self.theta, self.phi = g["freq"], g["pol"], g["theta"], g["phi"]
        self.beam, self.weight = g["beam"].view(LA), g["weight"].view(LA)

    def redistribute(self, axis):
        pass


def make_inputs():
    rng = np.random.default_rng(20260)
    tel = twin.FakeTelescope(FREQ)
    inputs, prod, stack, rev = twin.make_index_maps(tel)
    nstack = len(stack)
    ra = np.linspace(0.0, 360.0, NRA, endpoint=False) + 1.0
    # catalogue: below the first sample, above the last, on a sample, two in one bin, declination 60, a source whose
    # whole window has no weight (200 deg), the ends and the outside of the time stream (22 ... 240 deg of LSA)
    cra = np.array([0.4, 359.0, ra[10], 100.1, 101.7, 150.3, 200.2, 24.9, 236.4, 300.7, 75.5, 180.9])
    cdec = np.array([35.0, 52.0, 49.3, 20.5, 41.0, 60.0, 48.0, 55.5, 30.2, 44.4, 49.0, 67.3])
    sfreq = np.array([608.3, 601.9, 606.2, 604.4, 603.7, 605.6, 607.5, 602.3, 604.9, 606.7, 608.9, 601.2])
    cat = {"ra": cra, "dec": cdec, "z": twin.NU21 / sfreq - 1.0}

    def stream(n):
        vis = (rng.normal(size=(FREQ.size, nstack, n)) + 1j * rng.normal(size=(FREQ.size, nstack, n))).astype(np.complex64)
        w = rng.uniform(0.5, 2.0, size=(FREQ.size, nstack, n)).astype(np.float32)
        w[rng.uniform(size=w.shape) < 0.05] = 0.0  # scattered zero weights
        flags = np.ones((tel.nfeed, n), dtype=np.float32)
        flags[3, n // 3 : 2 * n // 3] = 0.0  # an input flagged bad over part of the day
        return vis, w, flags

    vis, w, flags = stream(NRA)
    w[2, :, 17] = 0.0  # one (f, ra) with every weight zero
    i200 = int(np.searchsorted(ra, 200.2))
    w[:, :, i200 - 5 : i200 + 6] = 0.0  # the whole window of the source at 200.2 deg, variable time track included
    ss = {"is_sstream": True, "freq": FREQ, "ra": ra, "lsd": 4021, "vis": vis, "weight": w, "input_flags": flags, "tag": "lsd_4021",
          "dt": 240.0 * twin.SIDEREAL_S * np.median(np.abs(np.diff(ra)))}
    # the time stream starts where the local stellar angle is about 22 degrees
    t_first = tel.t0 + ((22.0 - tel.longitude) % 360.0) / 360.0 * 86400.0 * twin.SIDEREAL_S
    time = t_first + CADENCE * np.arange(NTIME)
    vis, w, flags = stream(NTIME)
    ts = {"is_sstream": False, "freq": FREQ, "time": time, "ra": tel.unix_to_lsa(time), "vis": vis, "weight": w, "input_flags": flags, "tag": "ts_a",
          "dt": np.median(np.abs(np.diff(time)))}
    assert np.all(np.diff(ts["ra"]) > 0), "the time stream must not wrap"
    # a 9 x 16 grid beam in power with a masked patch
    theta, phi = np.linspace(15.0, 75.0, 9), np.linspace(-45.0, 45.0, 16)
    gb = np.zeros((FREQ.size, 2, 1, 9, 16), dtype=np.complex64)
    for ff in range(FREQ.size):
        for pp in range(2):
            sig = (9.0 + pp) * 600.0 / FREQ[ff]
            gb[ff, pp, 0] = (np.sin(np.radians(90.0 - 0.3 * (theta[:, None] - 49.3))) ** 2 * np.exp(-0.5 * (phi[None, :] / sig) ** 2)).astype(np.float32)
    # the masked patch: the first position (searched) whose interpolated flag clears 0.99 and 1.01 by 1e-3 at every
    # point the sources' windows evaluate, and that masks the beam of at least one of them
    import scipy.interpolate

    hs = int(TIMETRACK / ss["dt"])
    pts = [(np.radians(dc), twin.ha_array(ra, int(np.searchsorted(ra, sr)), sr, hs, True, np.float64)[0]) for sr, dc in zip(cra, cdec)]

    def patch():
        for t0 in range(1, 6):
            for p0 in range(5, 11):
                flag = np.ones((9, 16), dtype=np.float32)
                flag[t0 : t0 + 2, p0 : p0 + 3] = 0.0
                spl = scipy.interpolate.RectBivariateSpline(np.radians(theta), np.radians(phi), flag)
                fl = np.concatenate([spl(dc, h)[0] for dc, h in pts])
                if min(np.abs(fl - 0.99).min(), np.abs(fl - 1.01).min()) >= 1e-3 and (np.abs(fl - 1.0) >= 0.01).sum() >= 3:
                    return t0, p0
        raise AssertionError("no patch found")

    t0, p0 = patch()
    gw = np.ones(gb.shape, dtype=np.float32)
    gw[:, :, 0, t0 : t0 + 2, p0 : p0 + 3] = 0.0
    grid = {"freq": FREQ, "pol": np.array(["XX", "YY"]), "theta": theta, "phi": phi, "beam": gb, "weight": gw}
    return tel, ss, ts, cat, grid


def check_inputs(tel, ss, ts, cat):
    for d in (ss, ts):
        hs = TIMETRACK / d["dt"]
        for x in [hs] + [hs / np.cos(np.radians(dc)) for dc in cat["dec"]]:
            assert abs(x - round(x)) >= 1e-6, x
        assert 2 * int(max(hs / np.cos(np.radians(cat["dec"])))) + 1 <= len(d["ra"])
    sfreq = twin.NU21 / (cat["z"] + 1.0)
    mid = 0.5 * (FREQ[1:] + FREQ[:-1])
    assert np.abs(sfreq[:, None] - mid[None, :]).min() > 0.01 * 2.0
    near = np.abs(ts["ra"][None, :] - cat["ra"][:, None]).min(axis=1)
    cut = 1.5 * (ts["ra"][1] - ts["ra"][0])
    assert np.abs(near / cut - 1.0).min() > 0.01, near / cut
    return near > cut  # the sources that never transit in the time stream


def main():
    _refstub.load_reference()
    fast, tmp = compile_fast_tools()
    try:
        from draco.analysis import beamform as bf
        from draco.util import tools as rtools

        rtools._calc_redundancy = fast._calc_redundancy
        rtools.invert_no_zero = _refstub._invert_no_zero
        bf.beamform = fast.beamform
        bf.invert_no_zero = _refstub._invert_no_zero
        bf.NU21, bf.C = twin.NU21, twin.C
        bf.constants = types.SimpleNamespace(SIDEREAL_S=twin.SIDEREAL_S, c=twin.C, nu21=twin.NU21)
        bf.containers = types.SimpleNamespace(FormedBeam=RefFormedBeam, FormedBeamHA=RefFormedBeamHA, GridBeam=RefGridBeam)
        bf.io = types.SimpleNamespace(get_telescope=lambda m: m)

        tel, ss, ts, cat, grid = make_inputs()
        never = check_inputs(tel, ss, ts, cat)
        out = {"freq": FREQ, "cat_ra": cat["ra"], "cat_dec": cat["dec"], "cat_z": cat["z"], "ts_never": never, "timetrack": np.float64(TIMETRACK)}
        for k in ("ra", "vis", "weight", "input_flags"):
            out["ss_" + k] = ss[k]
        for k in ("time", "vis", "weight", "input_flags"):
            out["ts_" + k] = ts[k]
        for k, v in grid.items():
            out["grid_" + k] = v

        # ---- host helpers
        rd = {"ss": RefData(tel, ss), "ts": RefData(tel, ts)}
        polmap = rtools.polarization_map(rd["ss"].index_map, tel)
        bvec_m = rtools.baseline_vector(rd["ss"].index_map, tel)
        out["polmap"], out["bvec_m"] = polmap, bvec_m
        print("stacks per polarisation:", [int((polmap == p).sum()) for p in range(4)], "autos", int((polmap == -1).sum()))
        red = {}
        for name, d in (("ss", ss), ("ts", ts)):
            red[name] = rtools.calculate_redundancy(d["input_flags"], rd[name].index_map["prod"], rd[name].reverse_map["stack"]["stack"], len(polmap))
            out[name + "_redundancy"] = red[name]
        out["redundancy_zero_flags"] = rtools.calculate_redundancy(np.zeros_like(ss["input_flags"]), rd["ss"].index_map["prod"], rd["ss"].reverse_map["stack"]["stack"], len(polmap))

        # ---- the tasks
        for name, (dname, cls, cfg) in CASES.items():
            d = ss if dname == "ss" else ts
            task = getattr(bf, cls)()
            task.log = logging.getLogger("gen")
            full = twin.full_config(cfg)
            for k, v in full.items():
                setattr(task, k, v)
            rcat = RefCatalog(cat, "cat_a")
            args = ([RefGridBeam(grid)] if "External" in cls else []) + [tel]
            if "Cat" in cls:
                task.setup(*args, rd[dname])
                res = task.process(rcat)
            else:
                task.setup(*args, rcat)
                res = task.process(rd[dname])
            assert res.attrs["tag"] == d["tag"] + "_cat_a"
            beamfunc = None
            if "External" in cls:
                beamfunc = lambda pol, dec, ha, t=task: t._grid_beam(pol, dec, ha)  # noqa: E731
                for pol in ("XX", "YY"):
                    for sr, dc in zip(cat["ra"], np.radians(cat["dec"])):
                        pp = task._beam_pol.index(pol)
                        h = twin.ha_array(d["ra"], int(np.searchsorted(d["ra"], sr)), sr, int(TIMETRACK / d["dt"]), True, np.float64)[0]
                        fl = np.array([task._beam_flag[ff][pp](dc, h)[0] for ff in range(FREQ.size)])
                        assert min(np.abs(fl - 0.99).min(), np.abs(fl - 1.01).min()) >= 1e-3, (pol, sr, fl)
            truth = twin.process(tel, d, cat, full, polmap, bvec_m, red[dname], np.longdouble, beamfunc)
            f64 = twin.process(tel, d, cat, full, polmap, bvec_m, red[dname], np.float64, beamfunc)
            assert np.array_equal(truth["skipped"], f64["skipped"])
            if dname == "ts":
                assert np.array_equal(truth["skipped"], never)
            check_determined(tel, d, cat, full, polmap, red[dname], task, truth["skipped"])
            norm = truth["norm"]
            rec = {
                "ref_beam": np.asarray(res.beam), "ref_weight": np.asarray(res.weight),
                "truth_beam": truth["beam"].astype(np.float64), "truth_weight": truth["weight"].astype(np.float64),
                "norm": np.float64(norm), "pmax": np.float64(truth["pmax"]), "skipped": truth["skipped"],
                "e_ref_beam": np.float64(twin.beam_error(res.beam, truth["beam"], norm)), "e_ref_weight": np.float64(twin.weight_error(res.weight, truth["weight"])),
                "e_f64_beam": np.float64(twin.beam_error(f64["beam"], truth["beam"], norm)), "e_f64_weight": np.float64(twin.weight_error(f64["weight"], truth["weight"])),
            }
            if not full["collapse_ha"]:
                rec["ref_ha"] = np.asarray(res.ha)
                assert np.abs(rec["ref_ha"] - truth["ha"].astype(np.float64)).max() < 1e-14
            assert np.array_equal(np.asarray(res["position"]["ra"]), cat["ra"]) and np.array_equal(np.asarray(res["redshift"]["z"]), cat["z"])
            print(f"{name:22s} e_ref beam {rec['e_ref_beam']:.2e} weight {rec['e_ref_weight']:.2e}   e_f64 beam {rec['e_f64_beam']:.2e} weight {rec['e_f64_weight']:.2e}   "
                  f"P_max {truth['pmax']:.1f} norm {norm:.3g} skipped {int(truth['skipped'].sum())}")
            for k, v in rec.items():
                out[f"{name}/{k}"] = v

        # ---- the function: one source of the sidereal stream, a strict subset of the frequencies
        P = twin.prepare(ss, polmap, bvec_m, red["ss"], ["XX"], "natural", np.float64)
        src = 3
        dec = np.radians(cat["dec"][src])
        ha, idx, _ = twin.ha_array(ss["ra"], int(np.searchsorted(ss["ra"], cat["ra"][src])), cat["ra"][src], 2, True, np.float64)
        f_index = np.array([0, 2], dtype=np.int32)
        fargs = dict(vis=np.ascontiguousarray(P["vis"][0]), weight=np.ascontiguousarray(P["sumweight"][0]), dec=dec, lat=np.deg2rad(tel.latitude), cosha=np.cos(ha), sinha=np.sin(ha),
                     u=np.ascontiguousarray(P["bvec"][0][0]), v=np.ascontiguousarray(P["bvec"][0][1]), f_index=f_index, ra_index=idx.astype(np.int32))
        ref = np.asarray(fast.beamform(*fargs.values()))
        truth, pmax = twin.beamform(*fargs.values(), dtype=np.longdouble, want_pmax=True)
        f64 = twin.beamform(*fargs.values(), dtype=np.float64)
        norm = float(np.max(np.sum(fargs["weight"] * np.abs(fargs["vis"]), axis=-1)[:, idx]))
        for k, v in fargs.items():
            out["func/" + k] = np.asarray(v)
        out["func/ref"], out["func/truth"], out["func/norm"], out["func/pmax"] = ref, truth.astype(np.float64), np.float64(norm), np.float64(pmax)
        out["func/e_ref"], out["func/e_f64"] = np.float64(twin.beam_error(ref, truth, norm)), np.float64(twin.beam_error(f64, truth, norm))
        print(f"function               e_ref {out['func/e_ref']:.2e}   e_f64 {out['func/e_f64']:.2e}   P_max {pmax:.1f}")

        path = os.path.join(GOLDEN, "srcbeam.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def check_determined(tel, d, cat, cfg, polmap, red, task, skipped):
    """No non-zero ``sum pb^2 SW`` below 1e-6 of the largest (collapsed cases)."""
    if not cfg["collapse_ha"]:
        return
    vals = []
    process_pol = ["XX", "YY"] if cfg["polarization"] in ("I", "copol") else twin.FULLPOL
    P = twin.prepare(d, polmap, np.zeros((2, len(polmap))), red, process_pol, cfg["weight"], np.float64)
    for src in np.flatnonzero(~skipped):
        dec = np.radians(cat["dec"][src])
        if d["is_sstream"]:
            si = np.searchsorted(d["ra"], cat["ra"][src])
        else:
            si = np.argmin(abs(d["ra"] - cat["ra"][src]))
        hs = TIMETRACK / d["dt"]
        hs = int(hs / np.cos(dec)) if cfg["variable_timetrack"] else int(hs)
        ha, idx, _ = twin.ha_array(d["ra"], si, cat["ra"][src], hs, d["is_sstream"], np.float64)
        for p, pol in enumerate(process_pol):
            pb = np.ones((FREQ.size, ha.size)) if cfg["no_beam_model"] else task._beamfunc(pol, dec, ha)
            vals.append(np.sum(np.sum(P["sumweight"][p][:, idx, :], axis=-1) * pb**2, axis=1))
    vals = np.concatenate(vals)
    nz = vals[vals != 0]
    assert nz.min() >= 1e-6 * nz.max(), (nz.min(), nz.max())


if __name__ == "__main__":
    main()
