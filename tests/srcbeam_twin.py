"""NumPy twin of source beamforming (``draco_amd/util/_fast_tools.py``, ``draco_amd/analysis/beamform.py``; the
reference's ``_fast_tools.pyx:211-290`` and ``beamform.py:139-385``), runnable in float64 and in ``np.longdouble``: the
long-double run is the truth of the tests.  Index decisions (``searchsorted``, ``argmin``, ``int(ha_side)``, the
transit cut) are taken in float64 as the reference takes them (the generator asserts that its inputs leave them well
determined); everything that follows -- hour angles, baselines in wavelengths, phases, sums -- runs in the chosen type.
The primary beam is an input table: evaluated in float64 (telescope model or spline), then cast.

Also here: the fake telescope and the dataset / catalogue builders that the generator and the tests share, and the
error measures.
"""

import numpy as np

NU21 = 1420.40575177
C = 299792458.0
SIDEREAL_S = 1.0 / (1.0 + 1.0 / 365.259636)
FULLPOL = ["XX", "XY", "YX", "YY"]


def inz(x):
    x = np.asarray(x)
    out = np.zeros_like(x)
    nz = x != 0
    out[nz] = 1 / x[nz]
    return out


# ------------------------------------------------------------------------------------------------ the fake telescope
class FakeTelescope:
    """16 inputs on a 4 x 3 grid of positions (22 m east-west, 0.9 m north-south): every position has a Y feed, four
    (the first cylinder and one feed of the second) have an X feed too, so the four polarisation pairs get very
    different numbers of stacks.  Products are stacked over redundant baselines with east >= 0 (conjugated otherwise),
    as driftscan does: ``feedmap``, ``feedconj``, ``baselines``."""

    stack_type = "redundant"
    lmax = mmax = 0  # (what marks a telescope for ``io.get_telescope``)

    def __init__(self, frequencies, latitude=49.3, longitude=-119.6, t0=1.6e9):
        self.frequencies = np.asarray(frequencies, dtype=np.float64)
        self.latitude, self.longitude, self.t0 = float(latitude), float(longitude), float(t0)
        grid = [(22.0 * c, 0.9 * r) for c in range(4) for r in range(3)]
        pos = grid[:4] + grid
        pol = ["X"] * 4 + ["Y"] * 12
        self.feedpositions = np.array(pos)
        self.polarisation = np.array(pol)
        self.beamclass = np.array([0 if p == "X" else 1 for p in pol])
        n = len(pol)
        self.nfeed = n
        self.feedmap = np.full((n, n), -1, dtype=np.int64)
        self.feedconj = np.zeros((n, n), dtype=bool)
        keys, base = {}, []
        for i in range(n):
            for j in range(i, n):
                d = self.feedpositions[i] - self.feedpositions[j]
                conj = bool(d[0] < 0 or (d[0] == 0 and d[1] < 0))
                pp = (pol[i] + pol[j])[::-1] if conj else pol[i] + pol[j]
                d = -d if conj else d
                key = (pp, round(float(d[0]), 6), round(float(d[1]), 6))
                if key not in keys:
                    keys[key] = len(base)
                    base.append(d)
                self.feedmap[i, j], self.feedconj[i, j] = keys[key], conj
                self.feedmap[j, i], self.feedconj[j, i] = keys[key], (not conj) if i != j else conj
        self.baselines = np.array(base)

    def unix_to_lsa(self, t):
        return (360.0 * ((np.asarray(t, dtype=np.float64) - self.t0) / (86400.0 * SIDEREAL_S)) + self.longitude) % 360.0

    def lsd_to_unix(self, lsd):
        return self.t0 + (lsd - self.longitude / 360.0) * 86400.0 * SIDEREAL_S

    def beam(self, feed, freq, angpos):
        """An analytic complex beam ``(n, 2)``: Gaussian in hour angle, narrower at higher frequency, a leakage term
        linear in hour angle; X and Y differ in width, leakage and phase."""
        theta, phi = angpos[:, 0], angpos[:, 1]
        nu = self.frequencies[freq] / 600.0
        y = self.polarisation[feed] == "Y"
        sig = (0.17 if y else 0.15) / nu
        g = np.exp(-0.5 * (phi / sig) ** 2) * np.sin(theta) ** (1.5 if y else 1.0)
        co = g * np.exp(1j * (0.3 if y else -0.2) * phi / sig)
        cross = (0.3 if y else 0.2) * g * phi / sig * np.exp(0.4j)
        return np.stack([cross, co] if y else [co, cross], axis=1)


def make_index_maps(tel):
    """``input``, ``prod`` (all pairs, autos included), ``stack`` (first product of every unique baseline, with its
    conjugation) and the reverse map, with the dtypes the containers use."""
    n = tel.nfeed
    prod = np.array([(i, j) for i in range(n) for j in range(i, n)], dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    nstack = int(tel.feedmap.max()) + 1
    stack = np.zeros(nstack, dtype=[("prod", "<u4"), ("conjugate", "u1")])
    rev = np.zeros(len(prod), dtype=[("stack", "<u4"), ("conjugate", "u1")])
    seen = set()
    for pi, (i, j) in enumerate(prod):
        s = int(tel.feedmap[i, j])
        rev[pi] = (s, tel.feedconj[i, j])
        if s not in seen:
            seen.add(s)
            stack[s] = (pi, tel.feedconj[i, j])
    return np.arange(n), prod, stack, rev


# ------------------------------------------------------------------------------------------------------- the function
def beamform(vis, weight, dec, lat, cosha, sinha, u, v, f_index, ra_index, dtype=np.float64, want_pmax=False):
    """``_fast_tools.pyx:211-290`` in ``dtype``: ``[vis.shape[0], len(ra_index)]``."""
    T = dtype
    pi = 4 * np.arctan(T(1))
    dec, lat = T(dec), T(lat)
    cosha, sinha = np.asarray(cosha).astype(T), np.asarray(sinha).astype(T)
    u, v = np.asarray(u).astype(T), np.asarray(v).astype(T)
    ut = 2 * pi * np.cos(dec) * sinha
    vt = -2 * pi * (np.cos(lat) * np.sin(dec) - np.sin(lat) * np.cos(dec) * cosha)
    ra_index = np.asarray(ra_index, dtype=np.int64)
    out = np.zeros((vis.shape[0], ra_index.size), dtype=T)
    pmax = 0.0
    for fi in np.asarray(f_index, dtype=np.int64):
        phase = u[fi][np.newaxis, :] * ut[:, np.newaxis] + v[fi][np.newaxis, :] * vt[:, np.newaxis]
        x = vis[fi][ra_index]
        w = np.asarray(weight[fi][ra_index]).astype(T)
        out[fi] = np.sum(w * (x.real.astype(T) * np.cos(phase) - x.imag.astype(T) * np.sin(phase)), axis=-1)
        if phase.size:
            pmax = max(pmax, float(np.abs(phase).max()))
    return (out, pmax) if want_pmax else out


# ----------------------------------------------------------------------------------------------------------- the task
def prepare(d, polmap, bvec_m, redundancy, process_pol, weight_mode, dtype):
    """``_process_data`` (:573-630): per processed polarisation ``vis``, ``visweight``, ``sumweight [f, ra, k]`` and
    ``bvec [2, f, k]``.  ``redundancy [nstack, nra]`` is ``calculate_redundancy``'s output."""
    T = dtype
    out = {"vis": [], "visweight": [], "sumweight": [], "bvec": []}
    freq = np.asarray(d["freq"]).astype(T)
    for pol in process_pol:
        m = polmap == FULLPOL.index(pol)
        out["vis"].append(np.moveaxis(d["vis"][:, m, :], 1, 2))
        vw = np.moveaxis(d["weight"][:, m, :], 1, 2).astype(T)
        out["visweight"].append(vw)
        out["bvec"].append(np.asarray(bvec_m).astype(T)[:, np.newaxis, m] * freq[np.newaxis, :, np.newaxis] * T(1e6) / T(C))
        if weight_mode == "inverse_variance":
            out["sumweight"].append(vw)
        else:
            sw = (vw > 0).astype(T) * np.moveaxis(redundancy[m].astype(T), 0, 1)[np.newaxis]
            if weight_mode == "uniform":
                sw = (sw > 0).astype(T)
            out["sumweight"].append(sw)
    return out


def ha_array(ra, sra_index, sra, ha_side, is_sstream, dtype):
    """``_ha_array`` (:399-454): hour angles in ``dtype``, sample indices, mask of the slots that exist."""
    T = dtype
    pi = 4 * np.arctan(T(1))
    idx = np.arange(sra_index - ha_side, sra_index + ha_side + 1, dtype=np.int64)
    nra = len(ra)
    if is_sstream:
        idx[idx < 0] += nra
        idx[idx >= nra] -= nra
        mask = np.ones(idx.size, dtype=bool)
    else:
        mask = (idx >= 0) & (idx < nra)
        idx = idx[mask]
    ha = (np.asarray(ra)[idx].astype(T) - T(sra)) * (pi / 180)
    ha = (ha + pi) % (2 * pi) - pi
    return ha, idx, mask


def process(tel, d, cat, cfg, polmap, bvec_m, redundancy, dtype=np.float64, beamfunc=None):
    """``BeamFormBase.process`` (:139-385) in ``dtype``.

    ``d``: ``freq`` (MHz), ``ra`` (degrees; for a time stream the LSA of every sample), ``dt`` (seconds per sample),
    ``is_sstream``, ``vis`` / ``weight [freq, stack, ra]``.  ``cat``: ``ra``, ``dec`` (degrees), ``z`` (or None).
    ``cfg``: the task's config.  ``beamfunc(pol, dec, ha) -> [freq, ha]`` float64 (None: the telescope's model, or ones
    with ``no_beam_model``).  Returns ``beam``, ``weight``, ``ha`` (``collapse_ha`` off), ``skipped``, ``norm`` -- the
    largest ``sum_j |pb| sum_k ws |vis| inz(sum_j pb^2 SW)`` (float64), the size of what was summed -- and ``pmax``."""
    T = dtype
    collapse_ha = cfg.get("collapse_ha", True)
    polarization = cfg.get("polarization", "full")
    weight_mode = cfg.get("weight", "natural")
    no_beam = cfg.get("no_beam_model", False)
    freqside = cfg.get("freqside", None)
    variable = cfg.get("variable_timetrack", False)
    process_pol = ["XX", "YY"] if polarization in ("I", "copol") else list(FULLPOL)
    return_pol = ["I"] if polarization == "I" else process_pol
    npol = len(process_pol)
    lat = T(np.deg2rad(tel.latitude)) if T is np.float64 else T(tel.latitude) * (4 * np.arctan(T(1)) / 180)
    freq = np.asarray(d["freq"], dtype=np.float64)
    nfreq = freq.size
    ra = np.asarray(d["ra"], dtype=np.float64)
    ha_side_f = cfg.get("timetrack", 900.0) / d["dt"]
    nha = 2 * int(ha_side_f) + 1
    P = prepare(d, polmap, bvec_m, redundancy, process_pol, weight_mode, T)
    if beamfunc is None and not no_beam:
        tindex = np.array([np.argmin(np.abs(nu - tel.frequencies)) for nu in freq])
        feed = {p: list(tel.polarisation).index(p) for p in "XY"}

        def beamfunc(pol, dec, ha):
            angpos = np.array([(0.5 * np.pi - dec) * np.ones_like(ha), ha]).T
            pb = np.zeros((nfreq, ha.size), dtype=np.float64)
            for ff, fi in enumerate(tindex):
                bii = tel.beam(feed[pol[0]], fi, angpos)
                bjj = tel.beam(feed[pol[1]], fi, angpos) if pol[0] != pol[1] else bii
                pb[ff] = np.real(np.sum(bii * bjj.conjugate(), axis=1))
            return pb

    nsrc = len(cat["ra"])
    shape = (nsrc, len(return_pol), nfreq) + (() if collapse_ha else (nha,))
    fbb, fbw = np.zeros(shape, dtype=T), np.zeros(shape, dtype=T)
    oha = np.zeros((nsrc, nha), dtype=T)
    skipped = np.zeros(nsrc, dtype=bool)
    norm, pmax = 0.0, 0.0
    f_local = np.arange(nfreq, dtype=np.int32)
    f_mask = np.zeros(nfreq, dtype=bool)
    for src in range(nsrc):
        dec64 = np.radians(cat["dec"][src])
        dec = T(dec64) if T is np.float64 else T(cat["dec"][src]) * (4 * np.arctan(T(1)) / 180)
        if freqside is not None:
            sfreq = NU21 / (cat["z"][src] + 1.0)
            si = np.argmin(abs(freq - sfreq))
            f_mask = np.ones(nfreq, dtype=bool)
            f_mask[max(0, si - freqside) : min(nfreq, si + freqside + 1)] = False
            f_local = np.arange(nfreq, dtype=np.int32)[~f_mask]
        if d["is_sstream"]:
            sra_index = np.searchsorted(ra, cat["ra"][src])
        else:
            diff = abs(ra - cat["ra"][src])
            sra_index = np.argmin(diff)
            if diff[sra_index] > 1.5 * (ra[1] - ra[0]):
                skipped[src] = True
                continue
        ha_side = int(ha_side_f / np.cos(dec64)) if variable else int(ha_side_f)
        ha, idx, mask = ha_array(ra, sra_index, cat["ra"][src], ha_side, d["is_sstream"], T)
        ha64 = ha.astype(np.float64)
        full = np.zeros((npol,) + shape[2:], dtype=T)
        wfull = np.zeros((npol,) + shape[2:], dtype=T)
        for p, pol in enumerate(process_pol):
            pb = (np.ones((nfreq, ha.size)) if no_beam else beamfunc(pol, dec64, ha64)).astype(T)
            fb, pm = beamform(P["vis"][p], P["sumweight"][p], dec, lat, np.cos(ha), np.sin(ha), P["bvec"][p][0], P["bvec"][p][1], f_local, idx, T, want_pmax=True)
            pmax = max(pmax, pm)
            sw_in = P["sumweight"][p][:, idx, :]
            vw_in = P["visweight"][p][:, idx, :]
            size = np.sum(sw_in.astype(np.float64) * np.abs(P["vis"][p][:, idx, :]), axis=-1)  # [f, j]
            if collapse_ha:
                this_sw = np.sum(np.sum(sw_in, axis=-1) * pb**2, axis=1)
                full[p] = np.sum(fb * pb, axis=1) * inz(this_sw)
                if weight_mode != "inverse_variance":
                    w2 = np.sum(np.sum(sw_in**2 * inz(vw_in), axis=-1) * pb**2, axis=1)
                    wfull[p] = this_sw**2 * inz(w2)
                else:
                    wfull[p] = this_sw
                norm = max(norm, float(np.max(np.sum(np.abs(pb.astype(np.float64)) * size, axis=1) * inz(this_sw.astype(np.float64)))))
            else:
                this_sw = np.sum(sw_in, axis=-1)
                full[p][:, mask] = fb * inz(this_sw)
                if weight_mode != "inverse_variance":
                    w2 = np.sum(sw_in**2 * inz(vw_in), axis=-1)
                    wfull[p][:, mask] = this_sw**2 * inz(w2)
                else:
                    wfull[p][:, mask] = this_sw
                if size.size:
                    norm = max(norm, float(np.max(size * inz(this_sw.astype(np.float64)))))
            wfull[p][f_mask] = 0
        if polarization == "I":
            full = (np.sum(full * wfull, axis=0) * inz(np.sum(wfull, axis=0)))[np.newaxis]
            wfull = np.sum(wfull, axis=0)[np.newaxis]
        fbb[src] = full
        fbw[src] = 2 * wfull
        if not collapse_ha:
            oha[src, mask] = ha
    return {"beam": fbb, "weight": fbw, "ha": oha, "skipped": skipped, "norm": norm, "pmax": pmax}


# ------------------------------------------------------------------------------------------------ the error measures
def beam_error(got, truth, norm):
    """``max |got - truth| / norm``: the error against the size of what was summed."""
    got, truth = np.asarray(got, dtype=np.longdouble), np.asarray(truth, dtype=np.longdouble)
    if got.size == 0:
        return 0.0
    return float(np.abs(got - truth).max() / norm) if norm > 0 else float(np.abs(got - truth).max())


def weight_error(got, truth):
    """Largest elementwise relative error where the truth is non-zero; the zero patterns must be identical."""
    got, truth = np.asarray(got, dtype=np.longdouble), np.asarray(truth, dtype=np.longdouble)
    assert np.array_equal(got == 0, truth == 0), "zero patterns differ"
    nz = truth != 0
    return float(np.max(np.abs(got[nz] - truth[nz]) / np.abs(truth[nz]))) if nz.any() else 0.0


def floor(pmax):
    """The float64 rounding of a phase of size ``pmax``."""
    return 8.0 * 2.0**-53 * pmax


# ---------------------------------------------------------------------------------- draco_amd containers from arrays
def to_container(tel, d):
    """The ``SiderealStream`` / ``TimeStream`` of ``draco_amd`` for a dataset dict (host resident)."""
    from draco_amd.core import containers

    inputs, prod, stack, rev = make_index_maps(tel)
    if d["is_sstream"]:
        c = containers.SiderealStream(freq=d["freq"], ra=np.asarray(d["ra"]), stack=stack, prod=prod, input=inputs, reverse_map_stack=rev)
        c.attrs["lsd"] = d["lsd"]
        c.add_dataset("input_flags")
        c.input_flags[:] = d["input_flags"]
    else:
        c = containers.TimeStream(freq=d["freq"], time=d["time"], stack=stack, prod=prod, input=inputs, reverse_map_stack=rev)
        c.datasets["input_flags"] = containers.Dataset(host=np.array(d["input_flags"], dtype=np.float32))
    c.vis[:] = d["vis"]
    c.weight[:] = d["weight"]
    if d.get("tag") is not None:
        c.attrs["tag"] = d["tag"]
    return c


def to_catalog(cat, tag=None, coordinates="CIRS"):
    from draco_amd.core import containers

    n = len(cat["ra"])
    if cat.get("z") is not None:
        c = containers.SpectroscopicCatalog(object_id=np.arange(n))
        c["redshift"]["z"][:] = cat["z"]
    else:
        c = containers.SourceCatalog(object_id=np.arange(n))
    c["position"]["ra"][:] = cat["ra"]
    c["position"]["dec"][:] = cat["dec"]
    if coordinates is not None:
        c.attrs["coordinates"] = coordinates
    if tag is not None:
        c.attrs["tag"] = tag
    return c


# ------------------------------------------------------------------------------------------- the golden file's cases
FREQ = np.array([608.0, 606.0, 604.0, 602.0])
TIMETRACK = 3500.0

# name -> (dataset, task, config)
CASES = {
    "ss_natural_full": ("ss", "BeamForm", {"weight": "natural", "polarization": "full"}),
    "ss_uniform_copol": ("ss", "BeamFormCat", {"weight": "uniform", "polarization": "copol"}),
    "ss_ivar_I": ("ss", "BeamForm", {"weight": "inverse_variance", "polarization": "I"}),
    "ss_natural_full_ha": ("ss", "BeamFormCat", {"weight": "natural", "polarization": "full", "collapse_ha": False}),
    "ss_nobeam_I_ha": ("ss", "BeamForm", {"weight": "uniform", "polarization": "I", "collapse_ha": False, "no_beam_model": True}),
    "ss_nobeam_copol": ("ss", "BeamFormCat", {"weight": "natural", "polarization": "copol", "no_beam_model": True}),
    "ss_freqside1": ("ss", "BeamFormCat", {"weight": "natural", "polarization": "copol", "freqside": 1}),
    "ss_variable_I": ("ss", "BeamForm", {"weight": "natural", "polarization": "I", "variable_timetrack": True}),
    "ts_natural_full": ("ts", "BeamFormCat", {"weight": "natural", "polarization": "full"}),
    "ts_ivar_copol_ha": ("ts", "BeamForm", {"weight": "inverse_variance", "polarization": "copol", "collapse_ha": False}),
    "ss_external_cat": ("ss", "BeamFormExternalCat", {"weight": "natural", "polarization": "copol"}),
}


def full_config(cfg):
    full = {"collapse_ha": True, "polarization": "full", "weight": "natural", "no_beam_model": False, "timetrack": TIMETRACK, "variable_timetrack": False, "freqside": None}
    full.update(cfg)
    return full


def golden_inputs(z):
    """``(tel, {"ss": ..., "ts": ...}, cat, grid)`` from the golden file: the dicts :func:`process` and
    :func:`to_container` take."""
    tel = FakeTelescope(z["freq"])
    ss = {"is_sstream": True, "freq": z["freq"], "ra": z["ss_ra"], "lsd": 4021, "vis": z["ss_vis"], "weight": z["ss_weight"], "input_flags": z["ss_input_flags"], "tag": "lsd_4021",
          "dt": 240.0 * SIDEREAL_S * np.median(np.abs(np.diff(z["ss_ra"])))}
    ts = {"is_sstream": False, "freq": z["freq"], "time": z["ts_time"], "ra": tel.unix_to_lsa(z["ts_time"]), "vis": z["ts_vis"], "weight": z["ts_weight"],
          "input_flags": z["ts_input_flags"], "tag": "ts_a", "dt": np.median(np.abs(np.diff(z["ts_time"])))}
    cat = {"ra": z["cat_ra"], "dec": z["cat_dec"], "z": z["cat_z"]}
    grid = {k: z["grid_" + k] for k in ("freq", "pol", "theta", "phi", "beam", "weight")}
    return tel, {"ss": ss, "ts": ts}, cat, grid
