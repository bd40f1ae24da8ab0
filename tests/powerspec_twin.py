"""Long-double restatements of the cube-sized stages of the power-spectrum chain (``draco_amd/analysis/powerspec.py``,
``csrc/powerspec.hip``): the (RA, el) -> (u, v) transform of ``image_to_uv``, the cross product of
``CrossPowerSpectrum3D`` and the binned sums of ``get_2d_ps``.  Inputs are the float64 / complex128 numbers the task
holds (the data, the two window vectors, ``ps_norm``, the weights); every operation on them is carried out in long
double and the result rounded once.

The DFT is a direct sum with the phase ``k j mod n`` reduced in integers.  Axes of up to 256 points are transformed in
full; for a longer axis the transform is evaluated only at a sample of output cells (:func:`sample_cells`).
"""

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI_LD = LD("3.14159265358979323846264338327950288419716939937510")
FULL_MAX = 256
NSAMPLE = 64


def rel_err(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a.astype(CLD) - b.astype(CLD)).max() / np.abs(b.astype(CLD)).max())


def from_q64(q):
    """A coarse complex input of the golden file, stored as int16 numerators over 64 with (re, im) as the last axis."""
    q = np.asarray(q)
    return q[..., 0] / 64.0 + 1j * (q[..., 1] / 64.0)


def from_bits(ref, bits):
    """The truth stored beside the complex128 array ``ref`` as the difference of the two bit patterns (exact)."""
    ref = np.ascontiguousarray(ref)
    t = (ref.view(np.int64).reshape(ref.shape + (2,)) + np.asarray(bits)).view(np.float64)
    return np.ascontiguousarray(t).view(np.complex128).reshape(ref.shape)


LATITUDE = 49.3  # of the telescope of the golden cases


def delay_transform(spectrum, ra, el, delay, freq, pol, axes, window_los, nbeam=0, **attrs):
    """A ``DelayTransform`` as ``DelaySpectrumFFT(sample_axis="ra")`` leaves it for a ring map: ``spectrum [baseline, ra,
    delay]`` with ``baseline`` the folded ``axes``."""
    from draco_amd.core import containers

    ds = containers.DelayTransform(baseline=spectrum.shape[0], sample=ra, delay=delay)
    ds.create_index_map("pol", np.asarray(pol))
    ds.create_index_map("el", np.asarray(el))
    if nbeam:
        ds.create_index_map("beam", np.arange(nbeam))
    ds.attrs.update(baseline_axes=[str(a) for a in axes], freq=np.asarray(freq), window_los=str(window_los), **attrs)
    ds.spectrum[:] = spectrum
    return ds


def golden_delay_transform(g, name, **attrs):
    axes = [str(a) for a in g[f"{name}/axes"]]
    spectrum = from_q64(g[f"{name}/spectrum_q64"])
    nbeam = spectrum.shape[0] // (len(g[f"{name}/pol"]) * len(g[f"{name}/el"])) if "beam" in axes else 0
    return delay_transform(spectrum, g[f"{name}/ra"], g[f"{name}/el"], g[f"{name}/delay"], g[f"{name}/freq"], g[f"{name}/pol"], axes, g[f"{name}/window_los"], nbeam, **attrs)


def power_spectrum_3d(spectrum, pol, delay, u, v, kx, ky, kpara, uv_mask, redshift, freq_center, cosmology):
    from draco_amd.core import containers

    ps = containers.PowerSpectrum3D(pol=np.asarray(pol), delay=delay, u=u, v=v, cosmology=cosmology)
    for name, val in (("kx", kx), ("ky", ky), ("kpara", kpara), ("uv_mask", uv_mask)):
        ps.datasets[name][:] = val
    ps.attrs.update(redshift=float(redshift), freq_center=float(freq_center))
    ps.spectrum[:] = spectrum
    return ps


def _phases(n, ks):
    """``exp(-2 pi i k j / n)`` for the bins ``ks`` [nk] and ``j = 0 ... n - 1``: ``[nk, n]`` complex long double."""
    kj = (np.asarray(ks, dtype=np.int64)[:, np.newaxis] * np.arange(n, dtype=np.int64)[np.newaxis, :]) % n
    ang = -2 * PI_LD * kj.astype(LD) / LD(n)
    return np.cos(ang) + 1j * np.sin(ang)


def shifted_bin(pos, n):
    """The DFT bin that ``numpy.fft.fftshift`` puts at position ``pos`` of an axis of length ``n``."""
    return (np.asarray(pos) - n // 2) % n


def tapered(data, w_ra=None, w_el=None):
    """``data [..., ra, el] * (w_ra (x) w_el)`` in complex long double (the data alone without windows)."""
    x = np.asarray(data).astype(CLD)
    if w_ra is not None:
        x = x * (np.asarray(w_ra).astype(LD)[:, np.newaxis] * np.asarray(w_el).astype(LD)[np.newaxis, :])
    return x


def sampled(nra, nel):
    return nra > FULL_MAX or nel > FULL_MAX


def sample_cells(nra, nel, seed):
    """At most ``NSAMPLE`` output cells ``(iu [n], iv [n])`` of a shifted ``[nra, nel]`` plane: the zero mode, its
    neighbours next to the Nyquist position on either axis (positions 1 and n - 1 beside position 0, where the shift
    puts the most negative frequency), the four corners, and seeded cells."""
    cu, cv = nra // 2, nel // 2
    cells = {(cu, cv), (1 % nra, cv), (nra - 1, cv), (cu, 1 % nel), (cu, nel - 1), (0, 0), (0, nel - 1), (nra - 1, 0), (nra - 1, nel - 1)}
    rng = np.random.default_rng(seed)
    want = min(NSAMPLE, nra * nel)
    while len(cells) < want:
        cells.add((int(rng.integers(nra)), int(rng.integers(nel))))
    cells = sorted(cells)
    return np.array([c[0] for c in cells]), np.array([c[1] for c in cells])


def uv_full(data, w_ra=None, w_el=None):
    """``fftshift(fft2(tapered)) / (nra nel)`` over the last two axes of ``data [..., ra, el]``, complex long double."""
    x = tapered(data, w_ra, w_el)
    nra, nel = x.shape[-2:]
    fu = _phases(nra, shifted_bin(np.arange(nra), nra))  # [u, ra]
    fv = _phases(nel, shifted_bin(np.arange(nel), nel))  # [v, el]
    y = np.matmul(np.matmul(fu, x), fv.T)
    return y / LD(nra * nel)


def uv_at(data, iu, iv, w_ra=None, w_el=None):
    """The same at the output cells ``(iu, iv)`` only: ``[..., n]`` complex long double."""
    x = tapered(data, w_ra, w_el)
    nra, nel = x.shape[-2:]
    fu = _phases(nra, shifted_bin(iu, nra))  # [n, ra]
    fv = _phases(nel, shifted_bin(iv, nel))  # [n, el]
    out = np.zeros(x.shape[:-2] + (len(iu),), dtype=CLD)
    for s in range(len(iu)):
        out[..., s] = np.matmul(np.matmul(x, fv[s]), fu[s])
    return out / LD(nra * nel)


def spectrum_to_cube(spectrum, shape, axes):
    """The ``[pol, delay, ra, el]`` view ``SpatialTransformDelayMap`` takes of ``spectrum [baseline, ra, delay]``:
    ``shape`` the lengths of the ``axes`` folded into ``baseline``, beam 0 if there is a beam axis."""
    nra, ndelay = spectrum.shape[1:]
    cube = np.asarray(spectrum).reshape(*shape, nra, ndelay)
    if "beam" in axes:
        cube = np.take(cube, 0, axis=list(axes).index("beam"))
    return np.swapaxes(cube, 1, 3)


def cross(vis_1, vis_2, ps_norm):
    """``ps_norm vis_1[p1] conj(vis_2[p2])`` for every pair, ``p = p1 npol2 + p2``, complex long double."""
    a, b = np.asarray(vis_1).astype(CLD), np.asarray(vis_2).astype(CLD)
    out = np.zeros((a.shape[0] * b.shape[0],) + a.shape[1:], dtype=CLD)
    for p1 in range(a.shape[0]):
        for p2 in range(b.shape[0]):
            out[p1 * b.shape[0] + p2] = LD(ps_norm) * (a[p1] * np.conj(b[p2]))
    return out


def inverse_variance(sigma):
    """The weights the reference forms of a cube of sigma, ``invert_no_zero(|sigma|^2)``, in float64."""
    a = np.abs(np.asarray(sigma)) ** 2
    with np.errstate(divide="ignore"):
        return np.where(a == 0, 0.0, 1.0 / np.where(a == 0, 1.0, a))


def cyl_bin(spec, weight, binmap, nbins):
    """The binned sums over the last two axes of ``spec [..., u, v]`` with the float64 weights ``weight`` (same shape;
    None: 1 everywhere) and ``binmap [u, v]`` (-1: in no bin).  Returns float64 / complex128 arrays ``[..., nbins]``:
    ``spectrum = sum w p / sum w``, ``weight = sum w``, ``neff = (sum w)^2 / sum w^2`` (NaN, 0, NaN in a bin that is
    empty or holds no weight), the population ``n`` of every bin ``[nbins]``, and ``sum |w p|``."""
    spec = np.asarray(spec)
    lead = spec.shape[:-2]
    p = spec.reshape(lead + (-1,)).astype(CLD)
    w = np.ones(p.shape, dtype=LD) if weight is None else np.asarray(weight).reshape(p.shape).astype(LD)
    flat = np.asarray(binmap).reshape(-1)
    o_s = np.full(lead + (nbins,), np.nan + 1j * np.nan, dtype=np.complex128)
    o_w = np.zeros(lead + (nbins,), dtype=np.float64)
    o_n = np.full(lead + (nbins,), np.nan, dtype=np.float64)
    o_a = np.zeros(lead + (nbins,), dtype=np.float64)
    count = np.zeros(nbins, dtype=np.int64)
    for b in range(nbins):
        sel = np.flatnonzero(flat == b)
        count[b] = sel.size
        if sel.size == 0:
            continue
        wb, pb = w[..., sel], p[..., sel]
        sw, sw2, swp = wb.sum(axis=-1), (wb * wb).sum(axis=-1), (wb * pb).sum(axis=-1)
        o_w[..., b] = sw.astype(np.float64)
        o_a[..., b] = np.abs(wb * pb).sum(axis=-1).astype(np.float64)
        ok = sw != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            o_s[..., b] = np.where(ok, (swp / np.where(ok, sw, 1)).astype(np.complex128), np.nan + 1j * np.nan)
            o_n[..., b] = np.where(ok, (sw * sw / np.where(ok, sw2, 1)).astype(np.float64), np.nan)
    return o_s, o_w, o_n, count, o_a
