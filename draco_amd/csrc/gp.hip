// Gaussian-process regridding (draco/util/gaussian_process.py:71-226 interpolate_unweighted, draco/util/kernels.py,
// draco/analysis/sidereal.py:281-346 SiderealRegridderGP).
//
// A "group" is one distinct pair (input mask, kept output rows); frequencies with the same pair share everything up to
// the apply.  Per group g, with n compressed input samples, M band rows (decided on the host), nk kept output rows:
//   Kb [n][Mmax]   lower band by row: Kb[i][d] = K[i][i - d], d < M (everything beyond the band is dropped)
//   Y  [n][nkpad]  right-hand sides by column: Y[j][b] = Kstar[b][j]; replaced by A^T = K^-1 Kstar^T
//   Ac [W][nkpad]  A on each row's span [start_b, end_b): Ac[w][b] = A[b][start_b + w]
// dmm_gp_fill      evaluates Kb and Y from positions (products of gaussian / rational / matern kernels);
// dmm_gp_project   K = L L^T in place on the band (left-looking, 64 x 64 blocks, the products of a block row against
//                  the M-wide window on the f64 matrix cores), L Z = Y, L^T X = Z per tile of 64 right-hand sides, and
//                  the band edges of every column of X by the |x| > tol rule;
// dmm_gp_compact   Ac from X;
// dmm_gp_apply     per (frequency, 64 stacks, 64 kept rows): three tile products over the union of the rows' spans
//                  (real part, imaginary part, variance) through the compressed-sample index, the float32 chain of the
//                  weights, the optional mix-down on load and mix-up on store.
// Every k loop starts at a multiple of 16 of the group's own index range and every block works on one group alone, so a
// frequency's result does not depend on what else is in the batch; no atomics anywhere.
#include "chol_blocked.h"

#include <algorithm>

namespace {

constexpr int kT = 64;         // block height / tile edge
constexpr int kTP = kT + 1;    // LDS pitch of a 64 x 64 block
constexpr int kMaxSpec = 4;
constexpr int kMaxOrder = 1 << 20;

struct GpSpecs {
  int n;
  int type[kMaxSpec];
  double width[kMaxSpec], alpha2[kMaxSpec], p[kMaxSpec];
  double eps;
};

struct GpDims {
  int32_t n, M, nk, pad_;
};

// ---------------------------------------------------------------------------------------------------- kernel functions
__device__ __forceinline__ double gp_kernel(const GpSpecs& sp, double xa, double xb) {
#pragma clang fp contract(off)
  double prod = 1.0;
  for (int s = 0; s < sp.n; ++s) {
    const double w = sp.width[s];
    const double diff = xa / w - xb / w;
    double c;
    switch (sp.type[s]) {
      case DMM_GP_GAUSSIAN: c = sp.alpha2[s] * exp(-0.5 * (diff * diff)); break;
      case DMM_GP_RATIONAL: c = sp.alpha2[s] * pow(1.0 + (diff * diff) / (2.0 * sp.p[s]), -sp.p[s]); break;
      case DMM_GP_MATERN15: {
        const double d = fabs(diff) * sqrt(3.0);
        c = (1.0 + d) * exp(-d) * sp.alpha2[s];
        break;
      }
      default: {
        const double d = fabs(diff) * sqrt(5.0);
        c = (1.0 + d + (d * d) / 3.0) * exp(-d) * sp.alpha2[s];
        break;
      }
    }
    prod = s == 0 ? c : prod * c;
  }
  return prod;
}

__global__ void k_gp_fill_band(GpSpecs sp, const GpDims* __restrict__ dims, int nmax, int Mmax, const double* __restrict__ pos, double* __restrict__ Kb) {
  const int g = blockIdx.y;
  const GpDims D = dims[g];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)D.n * Mmax) return;
  const int i = (int)(e / Mmax), d = (int)(e % Mmax);
  const double* x = pos + (size_t)g * nmax;
  double v = 0.0;
  if (d < D.M && i - d >= 0) {
    v = gp_kernel(sp, x[i], x[i - d]);
    if (d == 0) v += sp.eps;
  }
  Kb[((size_t)g * nmax + i) * Mmax + d] = v;
}

__global__ void k_gp_fill_rhs(GpSpecs sp, const GpDims* __restrict__ dims, int nmax, int nkpad, const double* __restrict__ pos, const double* __restrict__ xok,
                              double* __restrict__ Y) {
  const int g = blockIdx.y;
  const GpDims D = dims[g];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)D.n * nkpad) return;
  const int j = (int)(e / nkpad), b = (int)(e % nkpad);
  double v = 0.0;
  if (b < D.nk) v = gp_kernel(sp, xok[(size_t)g * nkpad + b], pos[(size_t)g * nmax + j]);
  Y[((size_t)g * nmax + j) * nkpad + b] = v;
}

// ------------------------------------------------------------------------------------------------------------ masks
// mi[f][t] = any over stacks of w > 0, nz[f][t] = any of w != 0
__global__ void k_gp_sample_masks(const float* __restrict__ w, int nstack, int nt, uint8_t* __restrict__ mi, uint8_t* __restrict__ nz) {
  const int f = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const float* p = w + (size_t)f * nstack * nt + t;
  int a = 0, b = 0;
  for (int s = 0; s < nstack; ++s) {
    const float v = p[(size_t)s * nt];
    a |= v > 0.f;
    b |= v != 0.f;
  }
  mi[(size_t)f * nt + t] = (uint8_t)a;
  nz[(size_t)f * nt + t] = (uint8_t)b;
}

// rowflag[row] = any over time of w > 0
__global__ void k_gp_row_flags(const float* __restrict__ w, int nt, uint8_t* __restrict__ rowflag) {
  const int64_t row = blockIdx.x;
  int a = 0;
  for (int t = threadIdx.x; t < nt; t += blockDim.x) a |= w[row * nt + t] > 0.f;
  a = __syncthreads_or(a);
  if (threadIdx.x == 0) rowflag[row] = (uint8_t)(a != 0);
}

// ------------------------------------------------------------------------------------------------- band and tile code
struct Band {
  double* p;  // rows of pitch Mmax
  int n, M, Mmax;
  __device__ __forceinline__ double get(int i, int j) const {  // L[i][j], zero outside the band and the matrix
    const int d = i - j;
    return (j >= 0 && d >= 0 && d < M && i < n) ? p[(size_t)i * Mmax + d] : 0.0;
  }
};

// acc += sum_{k in [k0, k1)} a(r, k) b(c, k) over chunks of 16 (k0 a multiple of 16); 256 threads, slices as / bs in LDS.
// The next chunk's operands are fetched into registers before the current chunk's products are issued.
template <typename FA, typename FB>
__device__ __forceinline__ void gp_tile_product(v4d (&acc)[2][2], double* as, double* bs, int k0, int k1, FA fa, FB fb) {
  if (k0 >= k1) return;
  constexpr int NP = kT * kTileK / 256;
  double ra[NP], rb[NP];
  auto fetch = [&](int k) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int e = threadIdx.x + 256 * p;
      ra[p] = fa(e >> 4, k + (e & (kTileK - 1)));
      rb[p] = fb(e & (kT - 1), k + (e >> 6));
    }
  };
  fetch(k0);
  for (int k = k0; k < k1; k += kTileK) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int e = threadIdx.x + 256 * p;
      as[(e >> 4) * kTileLP + (e & (kTileK - 1))] = ra[p];
      bs[(e & (kT - 1)) * kTileLP + (e >> 6)] = rb[p];
    }
    __syncthreads();
    if (k + kTileK < k1) fetch(k + kTileK);
    dl_tile_mma(as, bs, acc);
  }
}

__device__ __forceinline__ void gp_zero(v4d (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
}

// K = L L^T on the band, one block of 256 threads per group.  LDS: as, bs, T [64][65], D [64][65].
__global__ __launch_bounds__(256) void k_gp_chol(const GpDims* __restrict__ dims, int nmax, int Mmax, double* __restrict__ Kb, int32_t* __restrict__ status) {
  extern __shared__ double sm[];
  double* as = sm;
  double* bs = as + kT * kTileLP;
  double(*T)[kTP] = (double(*)[kTP])(bs + kT * kTileLP);
  double(*D)[kTP] = (double(*)[kTP])(&T[kT][0]);
  const int g = blockIdx.x;
  const GpDims dm = dims[g];
  if (dm.n <= 0) return;
  Band L{Kb + (size_t)g * nmax * Mmax, dm.n, dm.M, Mmax};
  const int nblk = (dm.n + kT - 1) / kT;
  for (int bi = 0; bi < nblk; ++bi) {
    const int i0 = bi * kT, nb = min(kT, dm.n - i0);
    const int klo = max(0, i0 - dm.M + 1) & ~(kTileK - 1);
    for (int bj = max(0, i0 - dm.M + 1) / kT; bj <= bi; ++bj) {
      const int j0 = bj * kT;
      v4d acc[2][2];
      gp_zero(acc);
      gp_tile_product(acc, as, bs, klo, j0, [&](int r, int k) { return L.get(i0 + r, k); }, [&](int c, int k) { return L.get(j0 + c, k); });
      __syncthreads();
      // T[c][r] = K[i0 + r][j0 + c] - acc inside the band, zero elsewhere
      dl_tile_each(acc, [&](int r, int c, double v) {
        const int i = i0 + r, j = j0 + c, d = i - j;
        T[c][r] = (i < dm.n && d >= 0 && d < dm.M) ? L.p[(size_t)i * Mmax + d] - v : 0.0;
      });
      if (bj < bi) {
        for (int e = threadIdx.x; e < kT * kT; e += 256) {
          const int a = e >> 6, b = e & 63;
          D[a][b] = L.get(j0 + a, j0 + b);
        }
        __syncthreads();
        if (threadIdx.x < kT) {  // row r of the block: z D^T = t, columns ascending
          const int r = threadIdx.x;
          for (int c = 0; c < kT; ++c) {
            double s = T[c][r];
            for (int q = 0; q < c; ++q) s = fma(-D[c][q], T[q][r], s);
            T[c][r] = s / D[c][c];
          }
        }
        __syncthreads();
      } else {
        __syncthreads();
        for (int c = 0; c < nb; ++c) {  // U = L^T of the diagonal block in T[c][r], c <= r
          const double d = T[c][c];
          if (!(d > 0.0)) {  // (the same value in every thread)
            if (threadIdx.x == 0) status[g] = DMM_GP_NOT_POSDEF;
            return;
          }
          const double rt = sqrt(d);
          __syncthreads();
          if ((int)threadIdx.x == c) T[c][c] = rt;
          if ((int)threadIdx.x > c && (int)threadIdx.x < nb) T[c][threadIdx.x] = T[c][threadIdx.x] / rt;
          __syncthreads();
          for (int e = threadIdx.x; e < nb * nb; e += 256) {
            const int a = e / nb, b = e % nb;
            if (a > c && b >= a) T[a][b] = fma(-T[c][a], T[c][b], T[a][b]);
          }
          __syncthreads();
        }
      }
      for (int e = threadIdx.x; e < kT * kT; e += 256) {
        const int c = e >> 6, r = e & 63;
        const int i = i0 + r, j = j0 + c, d = i - j;
        if (i < dm.n && d >= 0 && d < dm.M) L.p[(size_t)i * Mmax + d] = T[c][r];
      }
      __syncthreads();
    }
  }
}

// L Z = Y, then L^T X = Z, for one tile of 64 right-hand sides of one group
__global__ __launch_bounds__(256) void k_gp_solve(const GpDims* __restrict__ dims, int nmax, int Mmax, int nkpad, double* __restrict__ Kb, double* __restrict__ Yall,
                                                  const int32_t* __restrict__ status) {
  // LDS: T and D [64][65]; the slices of the window products share D's space (D is loaded after the last product of a
  // block row and is done with before the next one starts): 67 KB, two blocks per CU
  extern __shared__ double sm[];
  double(*T)[kTP] = (double(*)[kTP])sm;
  double(*D)[kTP] = (double(*)[kTP])(&T[kT][0]);
  double* as = &D[0][0];
  double* bs = as + kT * kTileLP;
  const int g = blockIdx.y;
  const GpDims dm = dims[g];
  const int c0 = blockIdx.x * kT;
  if (dm.n <= 0 || c0 >= dm.nk || status[g] != DMM_GP_OK) return;
  Band L{Kb + (size_t)g * nmax * Mmax, dm.n, dm.M, Mmax};
  double* Y = Yall + (size_t)g * nmax * nkpad + c0;  // (c0 + 63 < nkpad: nkpad is a multiple of 64)
  const int n = dm.n, nblk = (n + kT - 1) / kT;
  auto ycol = [&](int c, int k) { return k < n ? Y[(size_t)k * nkpad + c] : 0.0; };
  auto load_block = [&](int i0, int nb, const v4d(&acc)[2][2]) {
    __syncthreads();
    dl_tile_each(acc, [&](int r, int c, double v) { T[r][c] = r < nb ? Y[(size_t)(i0 + r) * nkpad + c] - v : 0.0; });
    for (int e = threadIdx.x; e < kT * kT; e += 256) {
      const int a = e >> 6, b = e & 63;
      D[a][b] = a < nb ? L.get(i0 + a, i0 + b) : (a == b ? 1.0 : 0.0);
    }
    __syncthreads();
  };
  auto store_block = [&](int i0, int nb) {
    __syncthreads();
    for (int e = threadIdx.x; e < kT * kT; e += 256) {
      const int r = e >> 6, c = e & 63;
      if (r < nb) Y[(size_t)(i0 + r) * nkpad + c] = T[r][c];
    }
    __syncthreads();
  };
  for (int bi = 0; bi < nblk; ++bi) {
    const int i0 = bi * kT, nb = min(kT, n - i0);
    v4d acc[2][2];
    gp_zero(acc);
    gp_tile_product(acc, as, bs, max(0, i0 - dm.M + 1) & ~(kTileK - 1), i0, [&](int r, int k) { return L.get(i0 + r, k); }, ycol);
    load_block(i0, nb, acc);
    if (threadIdx.x < kT) {
      const int c = threadIdx.x;
      for (int r = 0; r < nb; ++r) {
        double s = T[r][c];
        for (int q = 0; q < r; ++q) s = fma(-D[r][q], T[q][c], s);
        T[r][c] = s / D[r][r];
      }
    }
    store_block(i0, nb);
  }
  for (int bi = nblk - 1; bi >= 0; --bi) {
    const int i0 = bi * kT, nb = min(kT, n - i0);
    v4d acc[2][2];
    gp_zero(acc);
    gp_tile_product(acc, as, bs, i0 + kT, min(n, i0 + kT + dm.M - 1), [&](int r, int k) { return L.get(k, i0 + r); }, ycol);
    load_block(i0, nb, acc);
    if (threadIdx.x < kT) {
      const int c = threadIdx.x;
      for (int r = nb - 1; r >= 0; --r) {
        double s = T[r][c];
        for (int q = r + 1; q < nb; ++q) s = fma(-D[q][r], T[q][c], s);
        T[r][c] = s / D[r][r];
      }
    }
    store_block(i0, nb);
  }
}

// start / end of every kept row of A: the first and one past the last j with |A[b][j]| > tol, (0, 0) if none
__global__ void k_gp_edges(const GpDims* __restrict__ dims, int nmax, int nkpad, const double* __restrict__ Yall, double tol, const int32_t* __restrict__ status,
                           int32_t* __restrict__ start, int32_t* __restrict__ end) {
  const int g = blockIdx.y;
  const GpDims dm = dims[g];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nkpad) return;
  int s = 0, e = 0;
  if (b < dm.nk && status[g] == DMM_GP_OK) {
    const double* Y = Yall + (size_t)g * nmax * nkpad + b;
    int first = -1, last = -1;
    for (int j = 0; j < dm.n; ++j)
      if (fabs(Y[(size_t)j * nkpad]) > tol) {
        if (first < 0) first = j;
        last = j;
      }
    if (first >= 0) {
      s = first;
      e = last + 1;
    }
  }
  start[(size_t)g * nkpad + b] = s;
  end[(size_t)g * nkpad + b] = e;
}

__global__ void k_gp_compact(const GpDims* __restrict__ dims, int nmax, int nkpad, int W, const double* __restrict__ Yall, const int32_t* __restrict__ start,
                             const int32_t* __restrict__ end, double* __restrict__ Ac) {
  const int g = blockIdx.y;
  const GpDims dm = dims[g];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)W * nkpad) return;
  const int w = (int)(e / nkpad), b = (int)(e % nkpad);
  double v = 0.0;
  if (b < dm.nk) {
    const int s = start[(size_t)g * nkpad + b], en = end[(size_t)g * nkpad + b];
    const int j = s + w;
    if (j < en && j < dm.n) v = Yall[((size_t)g * nmax + j) * nkpad + b];
  }
  Ac[((size_t)g * W + w) * nkpad + b] = v;
}

// ------------------------------------------------------------------------------------------------------------ apply
struct GpApply {
  const GpDims* dims;
  const int32_t* fgroup;   // [nfreq] group of each frequency, -1: nothing to do
  const int32_t* idx;      // [G][nmax] time sample of each compressed sample
  const int32_t* kout;     // [G][nkpad] padded-grid index of each kept row
  const int32_t* start;    // [G][nkpad]
  const int32_t* end;
  const double* Ac;        // [G][W][nkpad]
  const uint8_t* rowflag;  // [nfreq nstack]
  const float2* vis;
  const float* weight;
  const double* omega;
  const float* fmask;
  const double* dphi_in;
  const double* dphi_out;
  float2* out_vis;
  float* out_w;
  int G, nfreq, nstack, nt, samples, pad, nmax, nkpad, W;
};

__global__ __launch_bounds__(256) void k_gp_apply(GpApply a) {
#pragma clang fp contract(off)
  __shared__ double s_re[kT * kTileLP], s_im[kT * kTileLP], s_v[kT * kTileLP], s_a[kT * kTileLP], s_a2[kT * kTileLP];
  __shared__ int s_start[kT], s_end[kT], s_rng[2];
  const int f = blockIdx.z;
  const int g = a.fgroup[f];
  if (g < 0 || g >= a.G) return;
  const GpDims dm = a.dims[g];
  const int b0 = blockIdx.x * kT, s0 = blockIdx.y * kT;
  if (b0 >= dm.nk) return;
  if (threadIdx.x < kT) {
    const int b = b0 + threadIdx.x;
    int s = 0, e = 0;
    if (b < dm.nk) {
      s = a.start[(size_t)g * a.nkpad + b];
      e = a.end[(size_t)g * a.nkpad + b];
      if (s < 0 || e > dm.n || e - s > a.W) s = e = 0;
    }
    s_start[threadIdx.x] = s;
    s_end[threadIdx.x] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int lo = 0x7fffffff, hi = 0;
    for (int b = 0; b < kT; ++b)
      if (s_end[b] > s_start[b]) {
        lo = min(lo, s_start[b]);
        hi = max(hi, s_end[b]);
      }
    if (hi == 0) lo = 0;
    s_rng[0] = lo & ~(kTileK - 1);
    s_rng[1] = hi;
  }
  __syncthreads();
  const int jlo = s_rng[0], jhi = s_rng[1];
  const int32_t* idx = a.idx + (size_t)g * a.nmax;
  const double* Ac = a.Ac + (size_t)g * a.W * a.nkpad;
  v4d acc_re[2][2], acc_im[2][2], acc_v[2][2];
  gp_zero(acc_re);
  gp_zero(acc_im);
  gp_zero(acc_v);
  for (int k = jlo; k < jhi; k += kTileK) {
    __syncthreads();
    for (int e = threadIdx.x; e < kT * kTileK; e += 256) {
      const int kk = e & (kTileK - 1), s = e >> 4;
      const int j = k + kk, st = s0 + s;
      double xr = 0.0, xi = 0.0, v = 0.0;
      if (j < dm.n && st < a.nstack) {
        const int tt = idx[j];
        if ((unsigned)tt < (unsigned)a.nt) {
          const int64_t row = (int64_t)f * a.nstack + st;
          const float w = a.weight[row * a.nt + tt];
          float2 y = a.vis[row * a.nt + tt];
          if (a.omega) {  // mix down: y *= mask exp(-i omega dphi), rounded to complex64
            double sn, cs;
            sincos(a.omega[row] * a.dphi_in[tt], &sn, &cs);
            const double mk = (double)a.fmask[row];
            const double pr = mk * cs, pi = -mk * sn;
            const double yr = (double)y.x * pr - (double)y.y * pi, yi = (double)y.x * pi + (double)y.y * pr;
            y = make_float2((float)yr, (float)yi);
          }
          const float vf = w != 0.f ? 1.f / w : 0.f;
          xr = (double)y.x;
          xi = (double)y.y;
          v = (double)vf;
        }
      }
      s_re[s * kTileLP + kk] = xr;
      s_im[s * kTileLP + kk] = xi;
      s_v[s * kTileLP + kk] = v;
    }
    for (int e = threadIdx.x; e < kT * kTileK; e += 256) {
      const int b = e & (kT - 1), kk = e >> 6;
      const int j = k + kk;
      double v = 0.0;
      if (j >= s_start[b] && j < s_end[b]) v = Ac[(size_t)(j - s_start[b]) * a.nkpad + b0 + b];
      s_a[b * kTileLP + kk] = v;
      s_a2[b * kTileLP + kk] = v * v;
    }
    __syncthreads();
    dl_tile_mma(s_re, s_a, acc_re);
    dl_tile_mma(s_im, s_a, acc_im);
    dl_tile_mma(s_v, s_a2, acc_v);
  }
  // the accumulators' (row, column) map of dl_tile_each
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int st = s0 + 32 * wr + 16 * ti + lk + 4 * reg, b = b0 + 32 * wc + 16 * tj + lr;
        if (st >= a.nstack || b >= dm.nk) continue;
        const int64_t row = (int64_t)f * a.nstack + st;
        if (!a.rowflag[row]) continue;  // a stack without a positive weight is skipped
        const int go = a.kout[(size_t)g * a.nkpad + b] - a.pad;
        if (go < 0 || go >= a.samples) continue;
        const float var = (float)acc_v[ti][tj][reg];
        float w = var != 0.f ? 1.f / var : 0.f;
        float2 x = make_float2((float)acc_re[ti][tj][reg], (float)acc_im[ti][tj][reg]);
        if (w < 0.f) {
          w = 0.f;
          x = make_float2(0.f, 0.f);
        }
        if (a.omega) {  // mix up: x *= conj(mask exp(-i omega dphi)), weight kept where the mask is set
          double sn, cs;
          sincos(a.omega[row] * a.dphi_out[go], &sn, &cs);
          const double mk = (double)a.fmask[row];
          const double qr = mk * cs, qi = mk * sn;
          const double vr = (double)x.x * qr - (double)x.y * qi, vi = (double)x.x * qi + (double)x.y * qr;
          x = make_float2((float)vr, (float)vi);
          if (mk == 0.0) w = 0.f;
        }
        a.out_vis[row * a.samples + go] = x;
        a.out_w[row * a.samples + go] = w;
      }
}

constexpr size_t kBlockLds = sizeof(double) * (2 * kT * kTileLP + 2 * kT * kTP);  // k_gp_chol
constexpr size_t kSolveLds = sizeof(double) * (2 * kT * kTP);                      // k_gp_solve
static_assert(2 * kT * kTileLP <= kT * kTP, "the slices fit D");

// the shared checks of the group tables; copies them to dims_d
int gp_dims(dmm_ctx* ctx, const char* who, int G, const int32_t* dims_h, int32_t* dims_d, int nmax, int Mmax, int nkpad) {
  DMM_REQUIRE(dims_h && dims_d, "%s: NULL argument", who);
  DMM_REQUIRE(nmax >= 1 && nmax <= kMaxOrder, "%s: order %d outside 1 ... %d", who, nmax, kMaxOrder);
  DMM_REQUIRE(Mmax >= 1 && Mmax <= nmax, "%s: band rows %d outside 1 ... %d", who, Mmax, nmax);
  DMM_REQUIRE(nkpad >= kT && nkpad % kT == 0 && nkpad <= kMaxOrder, "%s: bad row pitch %d (a multiple of %d)", who, nkpad, kT);
  for (int g = 0; g < G; ++g) {
    const int32_t* d = dims_h + 4 * g;
    DMM_REQUIRE(d[0] >= 1 && d[0] <= nmax && d[1] >= 1 && d[1] <= Mmax && d[1] <= d[0] && d[2] >= 0 && d[2] <= nkpad,
                "%s: bad sizes of group %d: n %d M %d nk %d", who, g, d[0], d[1], d[2]);
  }
  DMM_HIP(hipSetDevice(ctx->device));
  DMM_HIP(hipMemcpyAsync(dims_d, dims_h, sizeof(int32_t) * 4 * (size_t)G, hipMemcpyHostToDevice, ctx->stream));
  return DMM_OK;
}

}  // namespace

#define GP_GROUPS(who)                                                    \
  DMM_REQUIRE(ctx != nullptr, who ": ctx is NULL");                       \
  DMM_REQUIRE(ngroup >= 0 && ngroup <= 65535, who ": bad group count %d", ngroup); \
  if (ngroup == 0) return DMM_OK;

extern "C" {

int dmm_gp_masks(dmm_ctx* ctx, const float* weight, int nfreq, int nstack, int nt, uint8_t* mask_pos, uint8_t* mask_nonzero, uint8_t* rowflag) {
  DMM_REQUIRE(ctx != nullptr, "dmm_gp_masks: ctx is NULL");
  DMM_REQUIRE(nfreq >= 0 && nfreq <= 65535 && nstack >= 0 && nt >= 0, "dmm_gp_masks: bad sizes nfreq=%d nstack=%d nt=%d", nfreq, nstack, nt);
  if (nfreq == 0 || nstack == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(weight && mask_pos && mask_nonzero && rowflag, "dmm_gp_masks: NULL argument");
  DMM_REQUIRE((int64_t)nfreq * nstack <= 0x7fffffff, "dmm_gp_masks: too many rows");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_gp_sample_masks, dim3((nt + 255) / 256, nfreq), dim3(256), 0, ctx->stream, weight, nstack, nt, mask_pos, mask_nonzero);
  hipLaunchKernelGGL(k_gp_row_flags, dim3((unsigned)((int64_t)nfreq * nstack)), dim3(256), 0, ctx->stream, weight, nt, rowflag);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_gp_fill(dmm_ctx* ctx, int nspec, const int32_t* types, const double* params, double epsilon, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax,
                int Mmax, int nkpad, const double* pos, const double* xout, double* Kb, double* Y) {
  GP_GROUPS("dmm_gp_fill")
  DMM_REQUIRE(types && params && pos && xout && Kb && Y, "dmm_gp_fill: NULL argument");
  DMM_REQUIRE(nspec >= 1 && nspec <= kMaxSpec, "dmm_gp_fill: kernel count %d outside 1 ... %d", nspec, kMaxSpec);
  DMM_REQUIRE(epsilon == epsilon, "dmm_gp_fill: epsilon is NaN");
  GpSpecs sp{};
  sp.n = nspec;
  sp.eps = epsilon;
  for (int s = 0; s < nspec; ++s) {
    DMM_REQUIRE(types[s] >= DMM_GP_GAUSSIAN && types[s] <= DMM_GP_MATERN25, "dmm_gp_fill: bad kernel type %d", types[s]);
    DMM_REQUIRE(params[3 * s] > 0.0, "dmm_gp_fill: kernel width %g must be positive", params[3 * s]);
    DMM_REQUIRE(types[s] != DMM_GP_RATIONAL || params[3 * s + 2] > 0.0, "dmm_gp_fill: rational scale %g must be positive", params[3 * s + 2]);
    sp.type[s] = types[s];
    sp.width[s] = params[3 * s];
    sp.alpha2[s] = params[3 * s + 1] * params[3 * s + 1];
    sp.p[s] = params[3 * s + 2];
  }
  int rc = gp_dims(ctx, "dmm_gp_fill", ngroup, dims, dims_dev, nmax, Mmax, nkpad);
  if (rc) return rc;
  const GpDims* dd = (const GpDims*)dims_dev;
  hipLaunchKernelGGL(k_gp_fill_band, dim3((unsigned)(((int64_t)nmax * Mmax + 255) / 256), ngroup), dim3(256), 0, ctx->stream, sp, dd, nmax, Mmax, pos, Kb);
  hipLaunchKernelGGL(k_gp_fill_rhs, dim3((unsigned)(((int64_t)nmax * nkpad + 255) / 256), ngroup), dim3(256), 0, ctx->stream, sp, dd, nmax, nkpad, pos, xout, Y);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_gp_project(dmm_ctx* ctx, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int Mmax, int nkpad, double* Kb, double* Y, double tol, int32_t* status,
                   int32_t* start, int32_t* end) {
  GP_GROUPS("dmm_gp_project")
  DMM_REQUIRE(Kb && Y && status && start && end, "dmm_gp_project: NULL argument");
  DMM_REQUIRE(tol >= 0.0, "dmm_gp_project: bad tolerance %g", tol);
  int rc = gp_dims(ctx, "dmm_gp_project", ngroup, dims, dims_dev, nmax, Mmax, nkpad);
  if (rc) return rc;
  const GpDims* dd = (const GpDims*)dims_dev;
  DMM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)ngroup, ctx->stream));
  DMM_HIP(hipFuncSetAttribute((const void*)k_gp_chol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBlockLds));
  DMM_HIP(hipFuncSetAttribute((const void*)k_gp_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSolveLds));
  hipLaunchKernelGGL(k_gp_chol, dim3(ngroup), dim3(256), kBlockLds, ctx->stream, dd, nmax, Mmax, Kb, status);
  hipLaunchKernelGGL(k_gp_solve, dim3(nkpad / kT, ngroup), dim3(256), kSolveLds, ctx->stream, dd, nmax, Mmax, nkpad, Kb, Y, (const int32_t*)status);
  hipLaunchKernelGGL(k_gp_edges, dim3((nkpad + 63) / 64, ngroup), dim3(64), 0, ctx->stream, dd, nmax, nkpad, (const double*)Y, tol, (const int32_t*)status, start, end);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_gp_compact(dmm_ctx* ctx, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int nkpad, int width, const double* Y, const int32_t* start,
                   const int32_t* end, double* Ac) {
  GP_GROUPS("dmm_gp_compact")
  DMM_REQUIRE(Y && start && end && Ac, "dmm_gp_compact: NULL argument");
  DMM_REQUIRE(width >= 1 && width <= nmax, "dmm_gp_compact: span width %d outside 1 ... %d", width, nmax);
  int rc = gp_dims(ctx, "dmm_gp_compact", ngroup, dims, dims_dev, nmax, nmax, nkpad);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gp_compact, dim3((unsigned)(((int64_t)width * nkpad + 255) / 256), ngroup), dim3(256), 0, ctx->stream, (const GpDims*)dims_dev, nmax, nkpad, width, Y,
                     start, end, Ac);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_gp_apply(dmm_ctx* ctx, int nfreq, int nstack, int nt, int samples, int pad, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int nkpad, int width,
                 const int32_t* freq_group, const int32_t* sample_index, const int32_t* out_index, const int32_t* start, const int32_t* end, const double* Ac,
                 const uint8_t* rowflag, const void* vis, const float* weight, const double* omega, const float* feed_mask, const double* dphi_in,
                 const double* dphi_out, void* out_vis, float* out_weight) {
  GP_GROUPS("dmm_gp_apply")
  DMM_REQUIRE(nfreq >= 0 && nfreq <= 65535 && nstack >= 0 && nt >= 1 && samples >= 1 && pad >= 0, "dmm_gp_apply: bad sizes nfreq=%d nstack=%d nt=%d samples=%d pad=%d",
              nfreq, nstack, nt, samples, pad);
  if (nfreq == 0 || nstack == 0) return DMM_OK;
  DMM_REQUIRE(freq_group && sample_index && out_index && start && end && Ac && rowflag && vis && weight && out_vis && out_weight, "dmm_gp_apply: NULL argument");
  DMM_REQUIRE(width >= 1 && width <= nmax, "dmm_gp_apply: span width %d outside 1 ... %d", width, nmax);
  DMM_REQUIRE((nstack + kT - 1) / kT <= 65535, "dmm_gp_apply: too many stacks");
  const bool mix = omega || feed_mask || dphi_in || dphi_out;
  DMM_REQUIRE(!mix || (omega && feed_mask && dphi_in && dphi_out), "dmm_gp_apply: the mixing arrays come all four or not at all");
  int rc = gp_dims(ctx, "dmm_gp_apply", ngroup, dims, dims_dev, nmax, nmax, nkpad);
  if (rc) return rc;
  GpApply a{};
  a.dims = (const GpDims*)dims_dev;
  a.fgroup = freq_group;
  a.idx = sample_index;
  a.kout = out_index;
  a.start = start;
  a.end = end;
  a.Ac = Ac;
  a.rowflag = rowflag;
  a.vis = (const float2*)vis;
  a.weight = weight;
  a.omega = omega;
  a.fmask = feed_mask;
  a.dphi_in = dphi_in;
  a.dphi_out = dphi_out;
  a.out_vis = (float2*)out_vis;
  a.out_w = out_weight;
  a.G = ngroup;
  a.nfreq = nfreq;
  a.nstack = nstack;
  a.nt = nt;
  a.samples = samples;
  a.pad = pad;
  a.nmax = nmax;
  a.nkpad = nkpad;
  a.W = width;
  hipLaunchKernelGGL(k_gp_apply, dim3(nkpad / kT, (nstack + kT - 1) / kT, nfreq), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
