"""Float64 twins of the regridder and the stacker for the tests (dense restatements, CPU only).

``band_wiener_twin`` solves, per row, the band-masked dense system ``(band_bw(R N R^T) + eps I) x = R N y`` with
``np.linalg.solve`` in float64: the exact answer the reference (float32 right-hand side) and the GPU kernel (float64
arithmetic, one rounding to complex64) are both measured against.
"""

import numpy as np


def lanczos_kernel(x, a):
    return np.where(np.abs(x) < a, np.sinc(x) * np.sinc(x / a), 0.0)


def forward_matrix(grid, times, a):
    """``R [ngrid, nt]``: Lanczos interpolation from the regular ``grid`` onto ``times``, transposed."""
    dx = grid[1] - grid[0]
    return lanczos_kernel((grid[:, None] - times[None, :]) / dx, a)


def padded_grid(samples, start, end, a):
    pad = 5 * a
    g = np.arange(-pad, samples + pad, dtype=np.float64) / samples
    return g * (end - start) + start, pad


def band_wiener_twin(vis, weight, times, samples, start, end, a=5, eps=1e-3, mask_zero_weight=False):
    """``vis, weight [nrow, nt]`` -> ``(x [nrow, samples] complex128, nw [nrow, samples] float64)``."""
    grid, pad = padded_grid(samples, start, end, a)
    R = forward_matrix(grid, np.asarray(times, dtype=np.float64), a)
    ng = len(grid)
    bw = 2 * a - 1
    band = np.abs(np.arange(ng)[:, None] - np.arange(ng)[None, :]) <= bw
    vis = np.asarray(vis, dtype=np.complex128)
    weight = np.asarray(weight, dtype=np.float64)
    x = np.zeros((vis.shape[0], samples), dtype=np.complex128)
    nw = np.zeros((vis.shape[0], samples), dtype=np.float64)
    for k in range(vis.shape[0]):
        C = np.where(band, (R * weight[k][None, :]) @ R.T, 0.0)
        d = R @ (weight[k] * vis[k])
        xs = np.linalg.solve(C + eps * np.eye(ng), d)
        x[k] = xs[pad : pad + samples]
        nw[k] = np.diag(C)[pad : pad + samples]
        if mask_zero_weight and not np.any(weight[k] != 0):
            nw[k] = 0.0
    return x, nw


def fringe_phase(freq_mhz, baselines_x, feed_mask, latitude_deg, lsd):
    """``SiderealRegridder._get_phase`` in float64: ``[nfreq, nstack, len(lsd)]`` complex128."""
    c = 299792458.0
    lmbda = c / (np.asarray(freq_mhz, dtype=np.float64) * 1e6)
    u = np.asarray(baselines_x, dtype=np.float64)[None, :] / lmbda[:, None]
    omega = -2.0 * np.pi * u * np.cos(np.radians(latitude_deg))
    dphi = 2.0 * np.pi * (lsd - np.floor(lsd))
    return np.asarray(feed_mask, dtype=np.float64)[None, :, None] * np.exp(-1.0j * omega[:, :, None] * dphi[None, None, :])
