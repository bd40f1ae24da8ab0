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


def find_inputs(input_index, inputs, require_match=False):
    """Position of every entry of ``inputs`` inside ``input_index`` (``tools.py:130-170``): :func:`find_keys` on the
    ``correlator_input`` field, or on ``chan_id`` where ``input_index`` has no ``correlator_input``.  An index without
    either field, or ``inputs`` without the chosen one, raises ``ValueError``."""
    names = input_index.dtype.names or ()
    field = "correlator_input" if "correlator_input" in names else ("chan_id" if "chan_id" in names else None)
    if field is None:
        raise ValueError("`input_index` must have either a `chan_id` or `correlator_input` field.")
    if field not in (inputs.dtype.names or ()):
        raise ValueError(f"`inputs` array does not have a `{field!s}` field.")
    return find_keys(input_index[field], inputs[field], require_match=require_match)


def redefine_stack_index_map(telescope, inputs, prod, stack, reverse_stack):
    """Give every stack entry a representative product between unmasked inputs (``tools.py:359-414``).

    A product is *usable* when both of its inputs exist in the telescope and ``telescope.feedmask`` has the pair.
    Entries whose representative is usable keep it (one vectorised test over the stack axis); only the products of the
    others are searched, and each of those entries takes the first usable product that was stacked into it, in product
    order, with that product's conjugation flag from ``reverse_stack``.  Returns ``(stack_new, stack_flag)``: the new map and, per entry, whether a usable representative
    exists at all (an entry without one keeps its old representative)."""
    return redefine_stack_from_index(telescope, find_inputs(telescope.input_index, inputs, require_match=False), prod, stack, reverse_stack)


def redefine_stack_from_index(telescope, tel_index, prod, stack, reverse_stack):
    """:func:`redefine_stack_index_map` for a caller that already holds ``tel_index``, the telescope's number of every
    input of the data (``None``: not in the telescope)."""
    present = np.array([t is not None for t in tel_index], dtype=bool)
    slot = np.array([t if t is not None else 0 for t in tel_index], dtype=np.int64)
    pa, pb = _fields(prod, 2)
    usable = present[pa] & present[pb] & np.asarray(telescope.feedmask)[slot[pa], slot[pb]]  # per product of the data
    nstack = stack.size
    member_of = np.asarray(reverse_stack["stack"]).astype(np.int64)
    keep = usable[np.asarray(stack["prod"]).astype(np.int64)]
    # only the entries that need another representative are searched: the lowest usable product stacked into each
    stacked = (member_of >= 0) & (member_of < nstack)
    cand = np.flatnonzero(usable & stacked & ~keep[np.where(stacked, member_of, 0)])
    first = np.full(nstack, len(pa), dtype=np.int64)
    np.minimum.at(first, member_of[cand], cand)
    swap = first < len(pa)
    out = stack.copy()
    out["prod"][swap] = first[swap]
    out["conjugate"][swap] = reverse_stack["conjugate"][first[swap]]
    return out, keep | swap


def unique_columns(flags):
    """The distinct columns of a Boolean ``[n, m]`` array: ``(columns [n, k] bool, inverse [m])`` with ``columns[:,
    inverse]`` the input.  The rows are packed to bits first, so that ``np.unique`` sorts ``ceil(n / 8)`` bytes per
    column as one key instead of ``n`` values; the order of the distinct columns is that of the packed keys."""
    flags = np.ascontiguousarray(np.asarray(flags, dtype=bool))
    packed = np.ascontiguousarray(np.packbits(flags, axis=0).T)  # [m, nbyte]
    if packed.shape[1] == 0:
        return flags[:, :1] if flags.shape[1] else flags, np.zeros(flags.shape[1], dtype=np.int64)
    keys = packed.view(np.dtype((np.void, packed.shape[1]))).ravel()
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return flags[:, first], np.asarray(inverse).reshape(-1).astype(np.int64)


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


def _fields(table, count):
    """The first ``count`` columns of a structured or two-dimensional table, as integer arrays."""
    table = np.asarray(table)
    if table.dtype.names:
        return [table[name].astype(np.int64) for name in table.dtype.names[:count]]
    return [table[..., c].astype(np.int64) for c in range(count)]


def calculate_redundancy(input_flags, prod_map, stack_index, nstack):
    """How many products with two good inputs went into every stack entry at every time: float32 ``[nstack, ntime]``
    (``tools.calculate_redundancy`` of the reference, computed here on the host in one scatter-add).

    ``input_flags [ninput, ntime]`` is non-zero where an input is good; flags that are zero everywhere count as all
    good.  ``prod_map [nprod]`` holds the input pairs and ``stack_index [nprod]`` the stack entry of every product; a
    product whose entry lies outside ``0 ... nstack - 1`` was not stacked.  A product index outside the inputs raises
    ``RuntimeError``, tables of different lengths ``ValueError``."""
    good = np.asarray(input_flags, dtype=np.float32)
    if not good.any():
        good = np.ones_like(good)
    first, second = _fields(prod_map, 2)
    entry = np.asarray(stack_index).astype(np.int64)
    if entry.shape[0] != first.shape[0]:
        raise ValueError(f"Number of prod_map rows ({first.shape[0]}) must match stack_index length ({entry.shape[0]}).")
    if first.size and (min(first.min(), second.min()) < 0 or max(first.max(), second.max()) >= good.shape[0]):
        raise RuntimeError("Input index in prod_map out of bounds.")
    stacked = np.flatnonzero((entry >= 0) & (entry < nstack))
    count = np.zeros((int(nstack), good.shape[1]), dtype=np.float32)
    # (np.add.at takes repeated entries one after the other, in product order)
    np.add.at(count, entry[stacked], good[first[stacked]] * good[second[stacked]])
    return count


def _stack_feeds(index_map):
    """The two inputs (as the telescope numbers them) of the representative product of every stack entry."""
    inputs = np.asarray(index_map["input"][:])
    if inputs.dtype.names and "chan_id" in inputs.dtype.names:
        inputs = inputs["chan_id"]
    (rep,) = _fields(index_map["stack"][:], 1)
    first, second = _fields(index_map["prod"][:], 2)
    return inputs[first[rep]].astype(np.int64), inputs[second[rep]].astype(np.int64)


def polarization_map(index_map, telescope, exclude_autos=True):
    """For every entry of ``index_map['stack']`` its place in ``['XX', 'XY', 'YX', 'YY']``, or -1 (``tools.
    polarization_map`` of the reference, vectorised over the stack axis).

    The two letters come from ``telescope.beamclass`` of the representative product's inputs (0: X, 1: Y, anything
    else: -1) and swap where ``telescope.feedconj`` marks the pair as conjugated.  Auto-correlations give -1 unless
    ``exclude_autos`` is off.  A telescope whose ``stack_type`` is set and is not ``"redundant"`` raises
    ``RuntimeError``."""
    kind = getattr(telescope, "stack_type", None)
    if kind is not None and kind != "redundant":
        raise RuntimeError(f"Telescope stack type needs to be 'redundant'. Is {kind}")
    a, b = _stack_feeds(index_map)
    beamclass = np.asarray(telescope.beamclass)
    ca, cb = beamclass[a], beamclass[b]
    swap = np.asarray(telescope.feedconj[a, b], dtype=bool)
    lead, trail = np.where(swap, cb, ca), np.where(swap, ca, cb)
    polmap = (2 * lead + trail).astype(int)  # XX, XY, YX, YY in this order
    polmap[~(np.isin(ca, (0, 1)) & np.isin(cb, (0, 1)))] = -1
    if exclude_autos:
        polmap[a == b] = -1
    return polmap


def baseline_vector(index_map, telescope):
    """Baseline in metres of every entry of ``index_map['stack']``, shape ``(2, nstack)`` float64 (``tools.
    baseline_vector`` of the reference, vectorised): the telescope's unique baseline of the representative product,
    ``telescope.baselines[telescope.feedmap[a, b]]``, which already carries the conjugation."""
    a, b = _stack_feeds(index_map)
    unique = np.asarray(telescope.feedmap[a, b], dtype=np.int64)
    return np.ascontiguousarray(np.asarray(telescope.baselines, dtype=np.float64)[unique].T)


def penalized_least_squares_1d(y, reweight_func, mask=None, lam=1e2, epsilon=1e-2, max_iter=100):
    """A smooth baseline of the 1-D signal ``y`` by iteratively reweighted penalised least squares (``tools.py:604-714``).

    Every iteration solves ``(W + lam D^T D) z = W y`` with ``D`` the second-difference operator and ``W`` the diagonal
    weights, through ``scipy.linalg.solveh_banded`` (the matrix has two sub-diagonals), then asks ``reweight_func(y - z,
    mask, iteration)`` for the next weights; masked samples always weigh nothing.  It stops when ``norm(w - w_next) /
    norm(w) < epsilon``, and warns after ``max_iter`` iterations without that.  An input that is masked everywhere gives
    zeros and a warning.  Host only: the arrays are one frequency axis long.
    """
    import warnings

    import scipy.linalg as la

    y = np.squeeze(y)
    if y.ndim != 1:
        raise ValueError(f"Expected 1D data array - got array with shape {y.shape}")
    n = y.shape[0]
    if mask is None:
        mask = np.zeros(n, dtype=bool)
    elif np.all(mask):
        warnings.warn("Entire dataset is masked.")
        return np.zeros_like(y)
    mask = np.squeeze(mask)
    if mask.ndim != 1:
        raise ValueError(f"Expected 1D mask array - got array with shape {mask.shape}")

    # lam D D^T in lower band form: the rows hold the main diagonal and the two below it
    band = np.ones((3, n), dtype=np.float64)
    pattern = np.array([1.0, -2.0, 1.0])
    for k in range(3):
        diag = np.zeros(n - k if n > k else 0)
        for j in range(max(n - 2, 0)):  # column j of D holds the pattern in rows j ... j + 2
            for a in range(3 - k):
                diag[j + a] += (lam * pattern[a + k]) * pattern[a]
        band[k, : n - k] = diag
    weights = np.zeros_like(band)
    weights[0] = 1.0

    z = None
    for it in range(max_iter):
        weights[:, mask] = 0.0
        w = weights[0]
        z = la.solveh_banded(band + weights, w * y, lower=True, check_finite=False)
        try:
            w_next = reweight_func(y - z, mask, it)
        except Exception as exc:
            raise RuntimeError("Invalid reweighting function") from exc
        if la.norm(w - w_next) / la.norm(w) < epsilon:
            break
        weights[0] = w_next
    else:
        warnings.warn(f"PLS did not converge after {max_iter} iterations.")
    return z


def arPLS_1d(y, mask=None, lam=1e2, epsilon=1e-2, max_iter=100):
    """Baseline of ``y`` by asymmetrically reweighted penalised least squares (``tools.py:717-780``; Baek et al. 2015).

    The weights are ``1 / (1 + exp(2 (r - (2 sigma - mu)) / sigma))`` with ``r = y - z`` and ``mu``, ``sigma`` the mean
    and the standard deviation of the negative, unmasked residuals: samples far above the baseline stop pulling on it.
    The rest is :func:`penalized_least_squares_1d`.
    """
    y = np.asarray(y)
    largest = np.log(np.finfo(y.dtype).max)  # exp() of anything beyond would overflow

    def reweight(resid, masked, it):
        below = (resid < 0) & ~masked
        mu = np.mean(resid, where=below)
        sigma = np.std(resid, where=below)
        arg = 2 * (resid - (2 * sigma - mu)) * invert_no_zero(sigma)
        arg = np.clip(arg, -largest, largest)
        return invert_no_zero(np.exp(arg) + 1.0)

    return penalized_least_squares_1d(y, reweight, mask, lam, epsilon, max_iter)
