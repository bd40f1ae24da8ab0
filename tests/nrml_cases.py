"""The cases of tests/golden/nrml.npz (written by gen_golden_nrml.py) as the tests read them: the task settings per
case, the ``[baseline, sample, freq]`` views of the stored containers, and per baseline the inputs of
``delay_power_spectrum_maxpost`` after the task's cuts (``delay_twin.cut_data``)."""

import os

import numpy as np

import delay_twin

DF = 0.390625
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nrml.npz")
BASE = dict(window="nuttall", apply_window=True, complex_timedomain=False, weight_boost=1.0, freq_frac=0.0, time_frac=0.0, remove_mean=True, skip_nyquist=True)
CFG = {
    "N16": {},
    "N32": {},
    "C23": dict(complex_timedomain=True, apply_window=False),
    "N70": dict(freq_zero=600.0, freq_spacing=DF, freq_frac=0.3),
    "N80hann": dict(window="hann"),
    "RM32": dict(skip_nyquist=False, dataset="map"),
    "N160": {},
    "NEG": dict(weight_boost=-1.0),
}
TASK_CASES = tuple(CFG)
POINTS = ("first", "last")


def load():
    return np.load(GOLDEN)


def cfg(name):
    return {**BASE, **CFG[name]}


def views(z, name):
    """The data and the weights as the task folds them: ``[baseline, sample, freq]``."""
    if f"{name}/map" in z.files:
        rmap, rw = z[f"{name}/map"], z[f"{name}/weight"]
        nb = rmap.shape[0] * rmap.shape[1] * rmap.shape[4]
        dv = rmap.transpose(0, 1, 4, 3, 2).reshape(nb, rmap.shape[3], rmap.shape[2])
        wv = np.broadcast_to(rw[np.newaxis], rmap.shape).transpose(0, 1, 4, 3, 2).reshape(dv.shape)
        return dv, wv
    return z[f"{name}/vis"].transpose(1, 2, 0), z[f"{name}/weight"].transpose(1, 2, 0)


def baselines(z, name, truth=False):
    """``(b, data, Ni, fsel, N, window)`` of every baseline the task does not skip (``data`` in long double if ``truth``)."""
    if f"{name}/b0/data" in z.files:  # a function case: stored as it is
        yield 0, z[f"{name}/b0/data"], z[f"{name}/b0/Ni"], z[f"{name}/b0/fsel"], int(z[f"{name}/b0/N"]), _win(z, name, 0)
        return
    c = cfg(name)
    dv, wv = views(z, name)
    for b in range(dv.shape[0]):
        t = delay_twin.cut_data(np.array(dv[b]), np.array(wv[b]), c, truth=truth)
        if t is None:
            assert b in z[f"{name}/skipped"]
            continue
        data, Ni, nzf, _ = t
        assert np.array_equal(nzf, z[f"{name}/b{b}/nzf"])
        yield b, data, np.asarray(Ni, dtype=np.float64), z[f"{name}/channel_ind"][nzf], int(z[f"{name}/b{b}/N"]), _win(z, name, b)


def _win(z, name, b):
    w = str(z[f"{name}/b{b}/window"])
    return None if w == "None" else w
