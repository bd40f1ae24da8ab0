"""Helpers of ``draco/util/tools.py`` that the path uses."""

from __future__ import annotations

import numpy as np


def invert_no_zero(x):
    """``1/x`` where ``x != 0`` else 0 (caput.algorithms.invert_no_zero [3P], ``tools.py:12``)."""
    x = np.asarray(x)
    if x.ndim == 0:
        return np.float64(0.0 if x == 0 else 1.0 / float(x))
    dt = x.dtype if x.dtype.kind in "fc" else np.float64
    out = np.zeros(x.shape, dtype=dt)
    nz = x != 0
    out[nz] = 1.0 / x[nz]
    return out


def _as_key(k):
    """A hashable form of one key: scalars as they are, sequences (rows of a 2-D key list) as tuples."""
    try:
        hash(k)
        return k
    except TypeError:
        return tuple(k)


def find_keys(key_list, keys, require_match=False):
    """Position of every entry of ``keys`` inside ``key_list`` (exact equality; ``tools.py:95-127``).

    Entries that do not occur give ``None``, or -- with ``require_match`` -- the reference's
    ``ValueError("Could not find all of the keys.")``, which ``BaseMapMaker.process`` relies on for data frequencies
    the beam transfers lack (``mapmaker.py:59``).  When a key occurs twice the last occurrence wins, as in a dict.
    """
    position = {}
    for i, k in enumerate(key_list):
        position[_as_key(k)] = i
    found = [position.get(_as_key(k)) for k in keys]
    if require_match and None in found:
        raise ValueError("Could not find all of the keys.")
    return found


_WINDOW_COEFFS = {
    "uniform": (1.0, 0.0, 0.0, 0.0),
    "hann": (0.5, -0.5, 0.0, 0.0),
    "hanning": (0.5, -0.5, 0.0, 0.0),
    "hamming": (0.53836, -0.46164, 0.0, 0.0),
    "blackman": (0.42, -0.5, 0.08, 0.0),
    "nuttall": (0.355768, -0.487396, 0.144232, -0.012604),
    "blackman_nuttall": (0.3635819, -0.4891775, 0.1365995, -0.0106411),
    "blackman_harris": (0.35875, -0.48829, 0.14128, -0.01168),
}


def window_generalised(x, window="nuttall"):
    """A window function evaluated at arbitrary locations ``x``; zero outside ``[0, 1]``.

    ``window``: 'uniform', 'hann', 'hanning', 'hamming', 'blackman', 'nuttall', 'blackman_nuttall', 'blackman_harris'
    (cosine sums ``sum_k a_k cos(2 pi k x)`` of up to four terms), 'triangular', or 'tukey-0.X' with 0.X the tapered
    fraction of the window (half of it at either end, a raised cosine).
    """
    x = np.asarray(x, dtype=np.float64)
    if window == "triangular":
        w = 1.0 - np.abs(2.0 * x - 1.0)
    elif window.startswith("tukey"):
        half = 0.5 * float(window.split("-")[1])
        # depth into the nearer taper, in units of its width: 0 on the flat top, 1 at the edge of the window
        depth = np.maximum(np.maximum(half - x, x - (1.0 - half)), 0.0) / half
        w = 0.5 + 0.5 * np.cos(np.pi * depth)
    else:
        # cos(k theta) is the Chebyshev polynomial T_k of cos(theta)
        w = np.polynomial.chebyshev.chebval(np.cos(2.0 * np.pi * x), _WINDOW_COEFFS[window])
    inside = (x >= 0) & (x <= 1)
    return np.where(inside, w, 0.0)
