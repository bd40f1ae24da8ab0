"""NumPy twins of the three source-stacking computations (``draco_amd/csrc/sourcestack.hip``): the pencil beams out of
a ring map, the frequency stack of formed beams and the 3-D stack of ring-map patches -- in long double (the truth)
and in float64 -- with the case table and the input builders the golden generator (``gen_golden_stack.py``) and the
tests share.

What decides an index or a bin is float64 in every precision, as in the reference and in the kernels: the nearest
pixel, ``np.digitize(freq - source_freq, edges)``.  Only the sums (and the variances of the patch weights) are carried
in ``dtype``.  The twins are written from the definition (a table of bins per source and channel); the kernels ask which
run of channels falls into a bin, so the two are independent.

Errors: ``stack_error = max |x - truth| / norm`` with ``norm = max_b sum |w b| inz(sum w)``, the size of what was summed;
``weight_error = max |w - truth| / max |truth|``.
"""

import numpy as np

NU21 = 1420.40575177
LATITUDE = 49.3
FLOOR = 8.0 * 2.0**-53

# ---- the golden cases.  Ring maps: name -> (npol, frequency axis, ra axis, weight dataset or rms only)
NRA, NEL, NFREQ = 32, 24, 13
MAPS = {
    "closed_w": (4, "desc", "closed", "weight"),
    "clip_rms": (4, "asc", "clip", "rms"),
    "closed_1pol": (1, "desc", "closed", "weight"),
    "clip_w": (4, "desc", "clip", "weight"),
}
# SourceStack: name -> (formed beam: a ring map's, or "irregular"), config
STACK_CASES = {
    "ss_side2": ("closed_w", dict(freqside=2)),
    "ss_side0": ("closed_w", dict(freqside=0)),
    "ss_side1_asc": ("clip_rms", dict(freqside=1)),
    "ss_side6": ("closed_w", dict(freqside=6)),
    "ss_side6_asc_uniform": ("clip_rms", dict(freqside=6, uniform_weight=True)),
    "ss_single_bin": ("closed_w", dict(freqside=3, single_source_bin_index=5)),
    "ss_uniform": ("closed_w", dict(freqside=2, uniform_weight=True)),
    "ss_1pol": ("closed_1pol", dict(freqside=4)),
    "ss_irregular": ("irregular", dict(freqside=3)),
    "ss_irregular_uniform": ("irregular", dict(freqside=5, uniform_weight=True)),
}
# RingMapStack2D: name -> (ring map, config)
STACK3D_CASES = {
    "s3_0x0": ("closed_w", dict(num_ra=0, num_dec=0, num_freq=2)),
    "s3_1x2": ("closed_w", dict(num_ra=1, num_dec=2, num_freq=3)),
    "s3_1x2_clip_rms": ("clip_rms", dict(num_ra=1, num_dec=2, num_freq=2)),
    "s3_10x10": ("closed_1pol", dict(num_ra=10, num_dec=10, num_freq=1)),
    "s3_10x10_clip": ("clip_w", dict(num_ra=10, num_dec=10, num_freq=0)),
    "s3_wide": ("closed_w", dict(num_ra=1, num_dec=1, num_freq=1, freq_width=9.0)),  # 3 channels of 2 MHz in a bin
    "s3_narrow": ("closed_w", dict(num_ra=1, num_dec=1, num_freq=4, freq_width=3.0)),  # bins of 2 / 3 MHz: some are empty
    "s3_tie": ("closed_w", dict(num_ra=0, num_dec=1, num_freq=1, freq_width=6.0)),  # edges on multiples of the channel width
    "s3_dec": ("closed_w", dict(num_ra=1, num_dec=2, num_freq=2, weight="dec")),
    "s3_patch": ("closed_w", dict(num_ra=2, num_dec=2, num_freq=2, weight="patch")),
    "s3_patch_clip_rms": ("clip_rms", dict(num_ra=2, num_dec=1, num_freq=1, weight="patch")),
    "s3_dec_1pol": ("closed_1pol", dict(num_ra=2, num_dec=1, num_freq=1, weight="dec")),
}
STACK_DEFAULTS = dict(freqside=50, single_source_bin_index=None, uniform_weight=False)
STACK3D_DEFAULTS = dict(num_ra=10, num_dec=10, num_freq=256, freq_width=0.0, weight="input")


class FakeTelescope:
    """What ``io.get_telescope`` and the tasks need of a telescope."""

    latitude = LATITUDE
    lmax = mmax = 1
    frequencies = np.zeros(1)

    def lsd_to_unix(self, lsd):
        return 1.0e9 + 86164.0905 * float(lsd)


def inz(x):
    x = np.asarray(x)
    return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(x.dtype)


def freq_map(centre, width):
    out = np.zeros(len(centre), dtype=[("centre", np.float64), ("width", np.float64)])
    out["centre"], out["width"] = centre, width
    return out


def map_axes(name):
    """``(npol, freq map, ra, el, has_weight)`` of a golden ring map."""
    npol, fdir, radir, wkind = MAPS[name]
    centre = 600.0 + 2.0 * np.arange(NFREQ)
    if fdir == "desc":
        centre = centre[::-1].copy()
    ra = np.linspace(0.0, 360.0 if radir == "closed" else 300.0, NRA, endpoint=False)
    el = np.linspace(-0.6, 0.8, NEL)
    return npol, freq_map(centre, 2.0), ra, el, wkind == "weight"


def irregular_axis():
    """A descending axis of 15 channels with unequal widths that do not overlap."""
    width = np.array([2.0, 2.0, 3.0, 1.0, 2.0, 2.5, 1.5, 2.0, 2.0, 1.0, 3.0, 2.0, 2.0, 1.5, 2.5])
    edges = 640.0 - np.concatenate([[0.0], np.cumsum(width)])
    return freq_map(0.5 * (edges[1:] + edges[:-1]), width)


def search_nearest(x, xeval):
    nxt = np.searchsorted(x, xeval, side="left")
    prev = np.maximum(0, nxt - 1)
    nxt = np.minimum(x.size - 1, nxt)
    return np.where(np.abs(xeval - x[prev]) < np.abs(xeval - x[nxt]), prev, nxt)


def source_ind(ra, el, src_ra, src_dec, latitude=LATITUDE):
    """``(ra_ind, el_ind, src_ind, margin)``: the nearest pixels of the sources inside the map, and how far (in pixels)
    the nearest source is from the half-pixel cut."""
    src_el = np.sin(np.radians(src_dec - latitude))
    dra, dell = np.median(np.abs(np.diff(ra))), np.median(np.abs(np.diff(el)))
    ri = search_nearest(np.append(ra, 360.0 + ra[0]), src_ra) % ra.size
    rsep = (src_ra - ra[ri] + 180.0) % 360.0 - 180.0
    ei = search_nearest(el, src_el)
    esep = src_el - el[ei]
    flag = (np.abs(rsep) > 0.5 * dra) | (np.abs(esep) > 0.5 * dell)
    margin = min(np.abs(np.abs(rsep) / dra - 0.5).min(), np.abs(np.abs(esep) / dell - 0.5).min())
    keep = np.flatnonzero(~flag)
    return ri[keep], ei[keep], keep, margin


def extract(rmap, wsrc, rms, ra_ind, el_ind):
    """``beam, weight [nsrc, npol, nfreq]`` out of ``rmap [npol, nfreq, nra, nel]``: a copy."""
    beam = np.ascontiguousarray(np.moveaxis(rmap[:, :, ra_ind, el_ind], 2, 0))
    if rms:
        weight = np.ascontiguousarray(np.moveaxis(inz(wsrc)[:, :, ra_ind] ** 2, 2, 0))
    else:
        weight = np.ascontiguousarray(np.moveaxis(wsrc[:, :, ra_ind, el_ind], 2, 0))
    return beam, weight


def stack_bins(frequency, freqside):
    """The stack axis and its edges (``sourcestack.py:80-109``)."""
    nfreq = len(frequency)
    axis = np.copy(frequency[int(nfreq / 2) - freqside : int(nfreq / 2) + freqside + 1])
    axis["centre"] = axis["centre"] - axis["centre"][freqside]
    if axis["centre"][0] > axis["centre"][-1]:
        bins = np.append(axis["centre"] + 0.5 * axis["width"], axis["centre"][-1] - 0.5 * axis["width"][-1])
    else:
        bins = np.append(axis["centre"] - 0.5 * axis["width"], axis["centre"][-1] + 0.5 * axis["width"][-1])
    return axis, bins


def stack_membership(frequency, z, freqside, single=None):
    """``index [nsrc, nfreq]``: the bin of every channel of every source, -1 where it takes no part."""
    axis, bins = stack_bins(frequency, freqside)
    sfreq = NU21 / (np.asarray(z, dtype=np.float64) + 1.0)
    idx = np.digitize(frequency["centre"][np.newaxis, :] - sfreq[:, np.newaxis], bins) - 1
    idx = np.where((idx >= 0) & (idx < 2 * freqside + 1), idx, -1)
    if single is not None:
        fs = frequency[single]
        idx[~(np.abs(sfreq - fs["centre"]) < 0.5 * fs["width"])] = -1
    return idx, axis, bins, sfreq


def source_stack(beam, weight, frequency, z, freqside=50, single_source_bin_index=None, uniform_weight=False, dtype=np.float64):
    """``{"stack", "weight" [npol, nstack], "norm", "index"}`` of ``beam / weight [nsrc, npol, nfreq]``."""
    idx, axis, bins, _ = stack_membership(frequency, z, freqside, single_source_bin_index)
    nsrc, npol, nfreq = beam.shape
    nstack = 2 * freqside + 1
    b = np.asarray(beam, dtype=dtype)
    w = np.asarray(weight, dtype=dtype)
    if uniform_weight:
        w = (w > 0).astype(dtype)
    S, W, A = (np.zeros((npol, nstack), dtype=dtype) for _ in range(3))
    for s in range(nsrc):  # sources in catalogue order, channels in ascending order, as the reference
        sel = np.flatnonzero(idx[s] >= 0)
        if sel.size:
            at = (slice(None), idx[s, sel])
            np.add.at(S, at, w[s][:, sel] * b[s][:, sel])
            np.add.at(A, at, np.abs(w[s][:, sel] * b[s][:, sel]))
            np.add.at(W, at, w[s][:, sel])
    return {"stack": S * inz(W), "weight": W, "norm": float(np.max(A * inz(W))), "index": idx, "axis": axis}


def stack3d_edges(freq, num_freq, freq_width):
    nbins = 2 * num_freq + 1
    if freq_width > 0:
        return np.linspace(-freq_width, freq_width, nbins + 1, endpoint=True)
    return (np.arange(-num_freq, num_freq + 2) - 0.5) * np.median(np.abs(np.diff(freq)))


def ra_wraps(ra):
    dra = np.median(np.abs(np.diff(ra)))
    return bool(np.isclose(ra[-1] + dra, 360.0, atol=dra / 100.0) and np.isclose(ra[0], 0.0, atol=dra / 100.0))


def stack3d(rmap, wsrc, rms, freq, ra, el, ra_ind, el_ind, z, num_ra=10, num_dec=10, num_freq=256, freq_width=0.0, weight="input", dtype=np.float64):
    """``{"stack", "weight" [npol, 2 num_ra + 1, 2 num_dec + 1, nbins], "norm"}`` of ``rmap [npol, nfreq, nra, nel]`` around
    the pixels ``(ra_ind, el_ind)`` of sources at redshift ``z`` (all inside the map)."""
    npol, nfreq, nra, nel = rmap.shape
    edges = stack3d_edges(freq, num_freq, freq_width)
    nbins = 2 * num_freq + 1
    wraps = ra_wraps(ra)
    m = np.asarray(rmap, dtype=dtype)
    if rms:
        wfull = (inz(np.asarray(wsrc, dtype=np.float64)) ** 2)[..., np.newaxis] * np.ones(nel)
    else:
        wfull = np.asarray(wsrc, dtype=np.float64)
    wfull = wfull.astype(dtype)
    if weight == "dec":
        var = m.var(axis=2)
        wdec = inz(np.where(var < 3e-7, 0, var).astype(dtype))
    nrp, ndp = 2 * num_ra + 1, 2 * num_dec + 1
    S, W, A = (np.zeros((npol, nrp, ndp, nbins), dtype=dtype) for _ in range(3))
    sfreq = NU21 / (1 + np.asarray(z, dtype=np.float64))
    for ri, ei, sf in zip(ra_ind, el_ind, sfreq):
        if sf > freq.max() or sf < freq.min():
            continue
        bin_ind = np.digitize(freq - sf, edges)
        rr = ri - num_ra + np.arange(nrp)
        ee = ei - num_dec + np.arange(ndp)
        if wraps:
            rok = np.ones(nrp, dtype=bool)
            rr = rr % nra
        else:
            rok = (rr >= 0) & (rr < nra)
        eok = (ee >= 0) & (ee < nel)
        ro, eo = np.flatnonzero(rok), np.flatnonzero(eok)
        for f in np.flatnonzero((bin_ind >= 1) & (bin_ind <= nbins)):
            k = bin_ind[f] - 1
            b = m[:, f][:, rr[ro]][:, :, ee[eo]]
            w = wfull[:, f][:, rr[ro]][:, :, ee[eo]]
            if weight == "patch":
                w = (w != 0) * inz(b.var(axis=(1, 2)))[:, np.newaxis, np.newaxis]
            elif weight == "dec":
                w = (w != 0) * wdec[:, f][:, np.newaxis, ee[eo]]
            sl = np.ix_(np.arange(npol), ro, eo, [k])
            S[sl] += (b * w)[..., np.newaxis]
            A[sl] += np.abs(b * w)[..., np.newaxis]
            W[sl] += w[..., np.newaxis]
    return {"stack": S * inz(W), "weight": W, "norm": float(np.max(A * inz(W))) if A.size else 0.0}


def stack_error(x, truth, norm):
    d = np.abs(np.asarray(x, dtype=np.longdouble) - np.asarray(truth, dtype=np.longdouble))
    return float(d.max() / norm) if d.size and norm > 0 else float(d.max()) if d.size else 0.0


def weight_error(x, truth):
    t = np.asarray(truth, dtype=np.longdouble)
    d = np.abs(np.asarray(x, dtype=np.longdouble) - t)
    scale = np.abs(t).max() if t.size else 0
    return float(d.max() / scale) if scale > 0 else (float(d.max()) if d.size else 0.0)


# ---- seeded inputs for the kernel-edge shapes
def random_formed_beam(seed, nsrc, npol, nfreq, descending=True):
    """``(beam, weight [nsrc, npol, nfreq], frequency map, z)``: sources spread over the band and a little beyond, never
    within 1 % of a channel width of a bin edge; some zero weights."""
    rng = np.random.default_rng(seed)
    centre = 400.0 + 0.5 * np.arange(nfreq)
    if descending:
        centre = centre[::-1].copy()
    frequency = freq_map(centre, 0.5)
    sf = centre.min() + 0.5 * (rng.integers(-2, nfreq + 2, size=nsrc) + rng.uniform(-0.4, 0.4, size=nsrc))
    beam = rng.normal(size=(nsrc, npol, nfreq))
    weight = rng.uniform(0.5, 2.0, size=(nsrc, npol, nfreq))
    weight[rng.uniform(size=weight.shape) < 0.1] = 0.0
    return beam, weight, frequency, NU21 / sf - 1.0


def random_ring_map(seed, npol, nfreq, nra, nel, rms=False):
    """``(map [npol, nfreq, nra, nel], weight or rms, frequency map, ra, el)``: a closed ra axis, a descending band."""
    rng = np.random.default_rng(seed)
    rmap = rng.normal(size=(npol, nfreq, nra, nel))
    if rms:
        w = rng.uniform(0.5, 2.0, size=(npol, nfreq, nra))
    else:
        w = rng.uniform(0.5, 2.0, size=(npol, nfreq, nra, nel))
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    centre = (400.0 + 0.5 * np.arange(nfreq))[::-1].copy()
    return rmap, w, freq_map(centre, 0.5), np.linspace(0.0, 360.0, nra, endpoint=False), np.linspace(-0.9, 0.9, nel)
