"""Generate tests/golden/gp.npz by EXECUTING the reference's own ``draco/util/kernels.py``, ``draco/util/gaussian_process.py``
and ``SiderealRegridderGP._regrid`` from source (through ``oracle._refstub``).  Only the data is committed; run where
the reference checkout exists:

    python tests/gen_golden_gp.py

The reference's two compiled loops (the banded matrix-vector product and the banded covariance diagonal) are stated
here in Python with the sums in the same order.  Per case and distinct mask the file records what the tests' bound on
the projection ``A`` is built from: ``e_ref``, the largest distance of the reference's float64 ``A`` (SciPy's banded
solve) from the long-double twin (``tests/gp_twin.py``) over the kept rows, ``cond`` of the band-truncated kernel
matrix, and the largest row sum of ``|A|``.  A case whose truncated matrix is not positive definite stops the
generator.
"""

import importlib
import os
import sys

import numpy as np
import scipy.linalg as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gp_twin as twin  # noqa: E402
from gen_golden_regrid import make_task  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CUTOFF, PARTITION = 1.7, 1

# name -> (kernel_width, samples, nin, jitter, gaps, epsilon, nstack, with an all-zero frequency)
CASES = {
    "kw2_r1": (2, 32, 35, 0.0, [], 1e-3, 17, False),
    "kw2_r2": (2, 32, 66, 0.0, [(20, 25)], 1e-3, 3, True),
    "kw2_r8": (2, 64, 526, 0.0, [(100, 140)], 1e-3, 1, False),
    "kw2_r8_jit": (2, 64, 526, 0.2, [(100, 140)], 1e-3, 1, False),
    "kw2_r8_eps": (2, 64, 526, 0.0, [(100, 140)], 1e-6, 1, False),
    "kw2_edge": (2, 64, 526, 0.0, [(0, 30), (500, 526)], 1e-3, 3, False),
    "kw3_r4": (3, 64, 256, 0.0, [(60, 80)], 1e-3, 3, False),
    "kw5_128r2": (5, 128, 256, 0.0, [(60, 80)], 1e-3, 3, False),
    "kw5_128r4": (5, 128, 512, 0.1, [(60, 80), (300, 301)], 1e-3, 1, False),
    "brutal": (5, 64, 128, 0.0, [(30, 41)], 1e-3, 3, False),
    "all_masked": (1, 32, 263, 0.0, [], 1e-3, 3, False),
}


def matmul_banded(A, x, start_ind, end_ind):
    out = np.zeros(A.shape[0])
    for beta in range(A.shape[0]):
        t = 0.0
        for j in range(start_ind[beta], end_ind[beta]):
            t = t + A[beta, j] * x[j]
        out[beta] = t
    return out


def linear_covariance_banded(Rn, Ni, start_ind, end_ind, bw):
    Ci = np.zeros((bw + 1, Rn.shape[0]))
    for beta in range(Rn.shape[0]):
        for alpha in range(max(0, bw - beta), bw + 1):
            betap = alpha + beta - bw
            t = 0.0
            for j in range(start_ind[beta], end_ind[beta]):
                t = t + Rn[betap, j] * Rn[beta, j] * Ni[j]
            Ci[alpha, beta] = t
    return Ci


def spec_of(kw, eps):
    return {"name": "matern", "width": kw, "alpha": 1.0, "nu": 2.5, "epsilon": eps}


def make_case(rng, kw, samples, nin, jit, gaps, nstack, zero_freq):
    """Positions, data ``[nfreq, nin, nstack]`` and weights: frequencies 0 and 2 share the gaps, frequency 1 has one more;
    with three or more stacks, stack 1 of frequency 0 has no weight at all; one sample of stack 0 has none."""
    xi = (np.arange(nin) + 0.3 + jit * rng.uniform(-1, 1, nin)) / nin
    pad = 5 * kw
    xo = np.arange(-pad, samples + pad, dtype=np.float64) / samples
    nfreq = 4 if zero_freq else 3
    t = xi[None, :, None]
    fr, ph = rng.uniform(1.0, 6.0, (nfreq, 1, nstack)), rng.uniform(0, 2 * np.pi, (nfreq, 1, nstack))
    x = np.exp(1j * (2 * np.pi * fr * t + ph)) + 0.05 * (rng.normal(size=(nfreq, nin, nstack)) + 1j * rng.normal(size=(nfreq, nin, nstack)))
    w = rng.uniform(0.5, 2.0, (nfreq, nin, nstack)).astype(np.float32)
    for a, b in gaps:
        w[:, a:b] = 0
    extra = nin // 2 + 3
    w[1, extra : extra + 3] = 0
    if nstack >= 3:
        w[0, :, 1] = 0
    free = [j for j in range(nin) if not any(a <= j < b for a, b in gaps)]
    if nstack >= 2:
        w[0, free[7], 0] = 0
    if zero_freq:
        w[3] = 0
    return xi, xo, x.astype(np.complex64), w


def main():
    _refstub.load_reference()
    ft = importlib.import_module("draco.util._fast_tools")
    ft._matmul_banded = matmul_banded
    ft._linear_covariance_banded = linear_covariance_banded
    ref_k = importlib.import_module("draco.util.kernels")
    ref_gp = importlib.import_module("draco.util.gaussian_process")
    ref_gp._fast_tools = ft
    ref_gp.invert_no_zero = _refstub._invert_no_zero

    out = {"names": np.array(list(CASES)), "cutoff": np.array([CUTOFF, PARTITION])}
    rng = np.random.default_rng(20261019)

    # ---- host functions
    xi, xo = (np.arange(35) + 0.3) / 35, np.arange(-10, 42, dtype=np.float64) / 32
    specs = {
        "gaussian": [{"name": "gaussian", "width": 2, "alpha": 1.3}],
        "rational": [{"name": "rational", "width": 2, "alpha": 0.7, "a": 1.5}],
        "matern15": [{"name": "matern", "width": 2, "alpha": 1.0, "nu": 1.5, "epsilon": 1e-4}],
        "matern25": [{"name": "matern", "width": 2, "alpha": 1.0, "nu": 2.5, "epsilon": 1e-3}],
        "product": [{"name": "matern", "width": 3, "alpha": 1.1, "nu": 2.5, "epsilon": 1e-3}, {"name": "gaussian", "width": 4, "alpha": 0.9, "epsilon": 2e-3}],
    }
    out["host/xi"], out["host/xo"], out["host/names"] = xi, xo, np.array(list(specs))
    for name, sp in specs.items():
        Ki, Ks = ref_gp._combine_gp_kernels_from_specs((xo, xi), [dict(s) for s in sp])
        out[f"host/{name}/Ki"], out[f"host/{name}/Ks"] = Ki, Ks
    Ki = out["host/matern25/Ki"]
    for which in ("full", "upper", "lower"):
        out[f"host/band/{which}"] = ref_k.convert_band_diagonal(Ki, which=which)
    out["host/sqdiff"] = ref_k.squared_difference_kernel((xo, 7), (0.5, 2.0))
    out["host/eudiff"] = ref_k.euclidean_difference_kernel(6, 1.5)

    for cname, (kw, samples, nin, jit, gaps, eps, nstack, zero_freq) in CASES.items():
        xi, xo, x, w = make_case(rng, kw, samples, nin, jit, gaps, nstack, zero_freq)
        spec = spec_of(kw, eps)
        Ki, Ks = ref_gp._combine_gp_kernels_from_specs((xo, xi), [dict(spec)])
        inp_mask = ~np.all(w == 0, axis=-1)
        mt = ref_gp._select_interp_samples(xi, xo, inp_mask, kw, CUTOFF, PARTITION)
        xout, wout = ref_gp.resample(x.copy(), w.copy(), xi=xi.copy(), xo=xo.copy(), cutoff_dist=CUTOFF, cutoff_partition=PARTITION, kernel_spec=dict(spec))
        key = f"case/{cname}"
        out[f"{key}/params"] = np.array([kw, samples, nin, eps, nstack], dtype=np.float64)
        out[f"{key}/xi"], out[f"{key}/xo"], out[f"{key}/x"], out[f"{key}/w"] = xi, xo, x, w
        out[f"{key}/mt"], out[f"{key}/xout"], out[f"{key}/wout"] = mt, xout, wout
        # ---- per distinct mask: M, band edges, and the reference's float64 A against the twin
        txout, twout, parts = twin.resample(x, w, Ki, Ks, mt)
        M, e_ref, cond, rowsum, amax, norder = [], [], [], [], [], []
        for ii, p in enumerate(parts):
            if p is None:
                M.append(0)
                continue
            mi = p["mi"]
            kd = ref_k.convert_band_diagonal(Ki[mi][:, mi], which="lower")
            A = la.solveh_banded(kd, Ks[mt[ii]][:, mi].T, lower=True, check_finite=False).T
            start, end = ref_k._get_band_inds(A, tol=1.0e-8)
            assert kd.shape[0] == p["M"]
            M.append(kd.shape[0])
            out[f"{key}/f{ii}/start"], out[f"{key}/f{ii}/end"] = start, end
            out[f"{key}/f{ii}/twin_edges_equal"] = np.array(np.array_equal(start, p["start"]) and np.array_equal(end, p["end"]))
            ev = np.linalg.eigvalsh(twin.band_truncate(Ki[mi][:, mi], kd.shape[0]))
            e_ref.append(float(np.abs(A - p["A"]).max()))
            cond.append(float(ev[-1] / ev[0]))
            rowsum.append(float(np.abs(p["A"]).sum(axis=1).max()))
            amax.append(float(np.abs(p["A"]).max()))
            norder.append(int(mi.sum()))
        out[f"{key}/M"] = np.array(M)
        out[f"{key}/bound"] = np.array([max(e_ref, default=0.0), max(cond, default=0.0), max(rowsum, default=0.0), max(amax, default=0.0), max(norder, default=0)])
        nz = twout != 0
        e_x = np.abs(xout - txout).max() / max(np.abs(txout).max(), 1e-300)
        e_w = (np.abs(wout - twout)[nz] / twout[nz]).max() if nz.any() else 0.0
        assert np.array_equal(wout == 0, twout == 0), cname
        out[f"{key}/e_ref_out"] = np.array([e_x, e_w])
        print(f"{cname}: M {M} n {norder} kept {mt.sum(axis=1)} e_ref(A) {max(e_ref, default=0):.2e} cond {max(cond, default=0):.3g} rowsum {max(rowsum, default=0):.3f} "
              f"ref-twin xout {e_x:.2e} wout {e_w:.2e} zero outputs {int((wout == 0).sum())}/{wout.size}")

    # ---- SiderealRegridderGP._regrid: the padded grid, the offset of the times, the trimming
    sidereal = importlib.import_module("draco.analysis.sidereal")
    sidereal.gaussian_process = ref_gp
    kw, samples, nin, jit, gaps, eps, nstack, _ = CASES["kw2_r2"]
    x, w = out["case/kw2_r2/x"], out["case/kw2_r2/w"]  # (four frequencies, three stacks: the reference's reshape needs them to differ)
    task = make_task(sidereal.SiderealRegridderGP, samples=samples, kernel_width=kw, epsilon=eps, mask_cutoff=CUTOFF, mask_cutoff_partition=PARTITION, start=312, end=313)
    vis = np.ascontiguousarray(np.moveaxis(x, 1, 2))
    wgt = np.ascontiguousarray(np.moveaxis(w, 1, 2))
    grid, vout, wout = task._regrid(vis, wgt, 312 + out["case/kw2_r2/xi"])
    out["task/lsd"], out["task/grid"], out["task/vis"], out["task/vis_weight"] = np.array(312), grid, vout, wout

    path = os.path.join(GOLDEN, "gp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
