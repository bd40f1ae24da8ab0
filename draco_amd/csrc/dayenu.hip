// DAYENU delay filter along the frequency axis (draco/analysis/dayenu.py:20-193, 776-975, 1125-1232).
//
// Per item (a stack entry of a stream, a (pol, el) column of a ring map), with flag[f] = all_t(weight[f, t] > 0):
//   C  = I + sum_k sinc(2 tw_k (nu_f - nu_f')) / eps_k   on the unflagged channels, 1 on the diagonal of the flagged ones,
//   NF = C^-1 o (flag x flag),   vis <- NF vis,   weight <- inz((NF o NF) inz(weight)).
// The reference takes a pseudo-inverse; its eigenvalue cut (1e-15 lambda_max) keeps every eigenvalue of these matrices
// (the smallest is about 1), so NF is the plain inverse of the unflagged block: a Cholesky factorisation, no eigensolver.
//
// Build, batched over distinct matrices (order n <= 1024, all in float64, global memory):
//   k_dy_cov    the masked covariance, full and symmetric;
//   k_dy_chol   C = U^T U in place, one block per matrix, left-looking in panels of 32 rows: a thread owns one column
//               of the panel in registers, the rows above arrive through LDS; a non-positive pivot sets status[mat];
//   k_dy_inv    V = U^-1 by back substitution, one lane per column;
//   k_dy_prod   NF = (V V^T) o (flag x flag) on v_mfma_f64_16x16x4_f64, 64 x 64 tiles (zero where status is set).
// The factorisation of a diagonal block, the forward substitution of a panel column and the tile product are the
// inline pieces of chol_blocked.h, the same code the blocked solver of chol_blocked.hip runs.
// Apply (the hot path), k_dy_apply: a block stages a stripe of columns of its item(s), every frequency, in LDS (so the
// product can be written back in place), then walks the rows of NF: the A operand streams from global memory one
// K-chunk ahead, the B operand comes from the stripe, f64 MFMA accumulates, the store rounds once to the container's
// dtype.  The weight side is the same kernel with A squared on load, inz on the stripe and on the store, and the
// attenuation byte applied.  Two layouts: columns contiguous (stream: vis [freq, stack, ra], a stripe = 32 reals of one
// item) and items contiguous (ring map: map [.., freq, ra, el], a stripe = 16 adjacent el of one RA sample, whole lines;
// the columns of a stripe may belong to different matrices: one MFMA pass per distinct matrix with the other columns
// zeroed).
#include "chol_blocked.h"

#include <algorithm>

namespace {

constexpr int kDyMaxOrder = 1024;

__device__ __forceinline__ double dy_sinc(double x) { return x == 0.0 ? 1.0 : sinpi(x) / (M_PI * x); }

__global__ void k_dy_cov(int n, int nband, const double* __restrict__ freq, const double* __restrict__ bands, const uint8_t* __restrict__ mask, double* __restrict__ A) {
  const int mat = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * n) return;
  const int i = (int)(idx / n), j = (int)(idx % n);
  const uint8_t* mk = mask + (size_t)mat * n;
  const double* bd = bands + (size_t)mat * nband * 2;
  double v = i == j ? 1.0 : 0.0;
  if (mk[i] && mk[j]) {
    const double df = freq[i] - freq[j];
    for (int k = 0; k < nband; ++k) v += dy_sinc(2.0 * bd[2 * k] * df) / bd[2 * k + 1];
  }
  A[(size_t)mat * n * n + idx] = v;
}

// blockDim.x = n rounded up to 64: thread i owns column i.
__global__ __launch_bounds__(1024) void k_dy_chol(int n, double* __restrict__ Aall, int32_t* __restrict__ status) {
  __shared__ double sU[kDB][kDB];
  __shared__ double sD[kDB][kDB + 1];
  double* A = Aall + (size_t)blockIdx.x * n * n;
  const int i = threadIdx.x;
  for (int J0 = 0; J0 < n; J0 += kDB) {
    const int nb = min(kDB, n - J0);
    const bool active = i >= J0 && i < n;
    double acc[kDB];
#pragma unroll
    for (int c = 0; c < kDB; ++c) acc[c] = (active && c < nb) ? A[(size_t)(J0 + c) * n + i] : 0.0;
    // ---- acc[c] = A[J0 + c][i] - sum_{k < J0} U[k][J0 + c] U[k][i]
    for (int k0 = 0; k0 < J0; k0 += kDB) {
      __syncthreads();
      for (int e = threadIdx.x; e < kDB * kDB; e += blockDim.x) {
        const int kk = e / kDB, c = e % kDB;
        sU[kk][c] = c < nb ? A[(size_t)(k0 + kk) * n + J0 + c] : 0.0;
      }
      __syncthreads();
      if (active) {
        for (int kk = 0; kk < kDB; ++kk) {
          const double a = A[(size_t)(k0 + kk) * n + i];
#pragma unroll
          for (int c = 0; c < kDB; ++c) acc[c] = fma(-a, sU[kk][c], acc[c]);
        }
      }
    }
    // ---- the diagonal block: D = Ud^T Ud in LDS
    __syncthreads();
    if (active && i < J0 + nb) {
#pragma unroll
      for (int c = 0; c < kDB; ++c) sD[c][i - J0] = acc[c];
    }
    __syncthreads();
    if (dl_potrf_lds(sD, nb, blockDim.x)) {  // (the whole block leaves)
      if (threadIdx.x == 0) status[blockIdx.x] = 1;
      return;
    }
    // ---- the panel's rows: Ud^T x = acc, column by column
    if (active) {
      if (i < J0 + nb) {
        for (int c = 0; c <= i - J0; ++c) A[(size_t)(J0 + c) * n + i] = sD[c][i - J0];
      } else {
        dl_fwd_col(sD, nb, acc, [&](int c, double x) { A[(size_t)(J0 + c) * n + i] = x; });
      }
    }
    __syncthreads();
  }
}

// V = U^-1 (upper triangle): lane j solves U v = e_j from row j upwards.
__global__ __launch_bounds__(64) void k_dy_inv(int n, const double* __restrict__ Uall, double* __restrict__ Vall, const int32_t* __restrict__ status) {
  const int mat = blockIdx.y;
  if (status[mat]) return;
  const double* __restrict__ U = Uall + (size_t)mat * n * n;
  double* V = Vall + (size_t)mat * n * n;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int jmax = min(n - 1, blockIdx.x * 64 + 63);
  const int jc = min(j, n - 1);
  for (int i = jmax; i >= 0; --i) {
    double s = i == j ? 1.0 : 0.0;
    const double* __restrict__ ui = U + (size_t)i * n;
    for (int k = i + 1; k <= jmax; ++k) {
      const double vk = k <= j ? V[(size_t)k * n + jc] : 0.0;
      s = fma(-ui[k], vk, s);
    }
    if (i <= j && j < n) V[(size_t)i * n + j] = s / ui[i];
  }
}

// NF(I, J) = sum_{k >= max(i, j)} V[i][k] V[j][k], masked: one 64 x 64 tile per block, 4 waves of 2 x 2 MFMA tiles.
__global__ __launch_bounds__(256) void k_dy_prod(int n, const double* __restrict__ Vall, const uint8_t* __restrict__ mask, const int32_t* __restrict__ status, double* __restrict__ NFall) {
  constexpr int KC = kTileK, LP = kTileLP;
  __shared__ double xs[64 * LP];
  __shared__ double ys[64 * LP];
  const int mat = blockIdx.y;
  const int nt = (n + 63) / 64;
  const int I0 = (blockIdx.x / nt) * 64, J0 = (blockIdx.x % nt) * 64;
  const double* __restrict__ V = Vall + (size_t)mat * n * n;
  double* NF = NFall + (size_t)mat * n * n;
  const uint8_t* mk = mask + (size_t)mat * n;
  const bool ok = status[mat] == 0;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d acc[2][2] = {{vz, vz}, {vz, vz}};
  const int r = threadIdx.x >> 2, c0 = (threadIdx.x & 3) * 4;
  if (ok) {
    for (int k0 = max(I0, J0); k0 < n; k0 += KC) {
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = k0 + c0 + c, ri = I0 + r, rj = J0 + r;
        xs[r * LP + c0 + c] = (ri < n && k < n && k >= ri) ? V[(size_t)ri * n + k] : 0.0;
        ys[r * LP + c0 + c] = (rj < n && k < n && k >= rj) ? V[(size_t)rj * n + k] : 0.0;
      }
      __syncthreads();
      dl_tile_mma(xs, ys, acc);
    }
  }
  dl_tile_each(acc, [&](int tr, int tc, double v) {
    const int row = I0 + tr, col = J0 + tc;
    if (row < n && col < n) NF[(size_t)row * n + col] = (ok && mk[row] && mk[col]) ? v : 0.0;
  });
}

struct DySide {
  void* p;
  int64_t ncol, sf, sc, si, so;
};

// ---- flag[item, f] = all_t(w > 0), weight *= flag
template <typename T>
__global__ __launch_bounds__(256) void k_dy_mask_cols(DySide w, int n, int ninner, uint8_t* __restrict__ flag) {
  const int in = blockIdx.x, f = blockIdx.y, o = blockIdx.z;
  T* p = (T*)w.p + o * w.so + in * w.si + f * w.sf;
  int all = 1;
  for (int64_t c = threadIdx.x; c < w.ncol; c += blockDim.x) all &= p[c * w.sc] > (T)0 ? 1 : 0;
  all = __syncthreads_and(all);
  if (threadIdx.x == 0) flag[((size_t)o * ninner + in) * n + f] = (uint8_t)all;
  if (!all)
    for (int64_t c = threadIdx.x; c < w.ncol; c += blockDim.x) p[c * w.sc] = (T)0;
}

template <typename T>
__global__ __launch_bounds__(64) void k_dy_mask_items(DySide w, int n, int ninner, uint8_t* __restrict__ flag) {
  const int in = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y, o = blockIdx.z;
  if (in >= ninner) return;
  T* p = (T*)w.p + o * w.so + in * w.si + f * w.sf;
  bool all = true;
  for (int64_t c = 0; c < w.ncol; ++c) all = all && p[c * w.sc] > (T)0;
  flag[((size_t)o * ninner + in) * n + f] = all ? 1 : 0;
  if (!all)
    for (int64_t c = 0; c < w.ncol; ++c) p[c * w.sc] = (T)0;
}

struct DyApplyArgs {
  const double* nf;
  const int32_t* imat;   // [nouter * ninner] matrix of each item; -1: not in this launch; -2: failed (weights zeroed)
  const uint8_t* atten;  // [nmat][n] or NULL
  const int32_t* units;  // the units (items, or groups of adjacent items) this launch covers, or NULL: all
  DySide d, w;
  int n, n16, nmat, layout, ninner, nouter, ngroup, d_cb;
};

template <typename T>
__device__ __forceinline__ T dy_inz(T x) {
  return x != (T)0 ? (T)1 / x : (T)0;
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void k_dy_apply(DyApplyArgs a) {
  constexpr int W = 16 * NT;
  constexpr int P = sizeof(T) == 4 ? W + 4 : W;  // stripe pitch: the four k rows of a 4-byte read fall on different banks
  extern __shared__ __align__(16) unsigned char dy_smem[];
  T* xs = reinterpret_cast<T*>(dy_smem);
  __shared__ int s_cm[W];
  __shared__ int64_t s_off[W];
  __shared__ int s_mats[W];
  __shared__ int s_nm, s_fail;

  const int unit = a.units ? a.units[blockIdx.x] : (int)blockIdx.x;
  const bool wside = (int)blockIdx.y >= a.d_cb;
  const int cb = wside ? (int)blockIdx.y - a.d_cb : (int)blockIdx.y;
  const DySide S = wside ? a.w : a.d;
  if (!S.p) return;
  T* base = (T*)S.p;
  const int n = a.n;
  const int nunit = a.layout == 0 ? a.nouter * a.ninner : a.nouter * a.ngroup;
  if (unit < 0 || unit >= nunit) return;

  if (threadIdx.x < W) {
    const int c = threadIdx.x;
    int o, inner;
    int64_t col;
    if (a.layout == 0) {
      o = unit / a.ninner;
      inner = unit % a.ninner;
      col = (int64_t)cb * W + c;
    } else {
      o = unit / a.ngroup;
      inner = (unit % a.ngroup) * W + c;
      col = cb;
    }
    int m = -1;
    if (col < S.ncol && inner < a.ninner) {
      m = a.imat[(size_t)o * a.ninner + inner];
      if (m >= a.nmat || m < -2) m = -1;
    }
    s_cm[c] = m;
    s_off[c] = o * S.so + inner * S.si + col * S.sc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int nm = 0, fail = 0;
    for (int c = 0; c < W; ++c) {
      const int m = s_cm[c];
      if (m == -2) fail = 1;
      if (m < 0) continue;
      bool seen = false;
      for (int q = 0; q < nm; ++q) seen = seen || s_mats[q] == m;
      if (!seen) s_mats[nm++] = m;
    }
    s_nm = nm;
    s_fail = fail;
  }
  __syncthreads();
  const int nm = s_nm;
  if (nm == 0 && !(wside && s_fail)) return;

  // ---- stage the stripe, every frequency (zero rows up to the next multiple of 16)
  for (int e = threadIdx.x; e < a.n16 * W; e += 256) {
    const int f = e / W, c = e % W;
    T v = (T)0;
    if (f < n && s_cm[c] >= 0) {
      v = base[s_off[c] + f * S.sf];
      if (wside) v = dy_inz(v);
    }
    xs[f * P + c] = v;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < nm; ++q) {
    const int m = s_mats[q];
    const double* __restrict__ NF = a.nf + (size_t)m * n * n;
    bool mine[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) mine[t] = s_cm[16 * t + lr] == m;
    for (int r0 = 32 * wave; r0 < n; r0 += 128) {
      v4d acc[2][NT];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = vz;
      const int row0 = r0 + lr, row1 = r0 + 16 + lr;
      const double* __restrict__ p0 = NF + (size_t)min(row0, n - 1) * n;
      const double* __restrict__ p1 = NF + (size_t)min(row1, n - 1) * n;
      const double z0 = row0 < n ? 1.0 : 0.0, z1 = row1 < n ? 1.0 : 0.0;
      double an[2][4];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = k0 + 4 * lk + s;
          const int kc = min(k, n - 1);
          const double zk = k < n ? 1.0 : 0.0;
          an[0][s] = p0[kc] * (z0 * zk);
          an[1][s] = p1[kc] * (z1 * zk);
        }
      };
      fetch(0);
      for (int k0 = 0; k0 < a.n16; k0 += 16) {
        double ac[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int s = 0; s < 4; ++s) ac[t][s] = wside ? an[t][s] * an[t][s] : an[t][s];
        if (k0 + 16 < a.n16) fetch(k0 + 16);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            const double b = mine[u] ? (double)xs[(k0 + 4 * lk + s) * P + 16 * u + lr] : 0.0;
            acc[0][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[0][s], b, acc[0][u], 0, 0, 0);
            acc[1][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[1][s], b, acc[1][u], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int row = r0 + 16 * t + lk + 4 * reg;
            if (row < n && mine[u]) {
              double v = acc[t][u][reg];
              if (wside) {
                v = v != 0.0 ? 1.0 / v : 0.0;
                if (a.atten && !a.atten[(size_t)m * n + row]) v = 0.0;
              }
              base[s_off[16 * u + lr] + row * S.sf] = (T)v;
            }
          }
    }
  }
  if (wside && s_fail) {
    for (int e = threadIdx.x; e < n * W; e += 256) {
      const int f = e / W, c = e % W;
      if (s_cm[c] == -2) base[s_off[c] + f * S.sf] = (T)0;
    }
  }
}

DySide dy_side(const dmm_dayenu_side* s) {
  DySide r{};
  if (s) {
    r.p = s->ptr;
    r.ncol = s->ncol;
    r.sf = s->stride_freq;
    r.sc = s->stride_col;
    r.si = s->stride_inner;
    r.so = s->stride_outer;
  }
  return r;
}

template <typename T, int NT>
int launch_apply(dmm_ctx* ctx, DyApplyArgs& a, int64_t nunit) {
  constexpr int W = 16 * NT;
  constexpr int P = sizeof(T) == 4 ? W + 4 : W;
  const int64_t dcb = !a.d.p ? 0 : (a.layout == 0 ? (a.d.ncol + W - 1) / W : a.d.ncol);
  const int64_t wcb = !a.w.p ? 0 : (a.layout == 0 ? (a.w.ncol + W - 1) / W : a.w.ncol);
  if (dcb + wcb > 65535) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_dayenu_apply: %lld column blocks do not fit the grid", (long long)(dcb + wcb));
  if (dcb + wcb == 0) return DMM_OK;
  a.d_cb = (int)dcb;
  a.ngroup = (a.ninner + W - 1) / W;
  const size_t lds = (size_t)a.n16 * P * sizeof(T);
  auto k = k_dy_apply<T, NT>;
  DMM_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, dim3((unsigned)nunit, (unsigned)(dcb + wcb)), dim3(256), lds, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

bool dy_side_ok(const dmm_dayenu_side* s) { return s->ncol >= 0 && s->stride_freq >= 0 && s->stride_col >= 0 && s->stride_inner >= 0 && s->stride_outer >= 0; }

}  // namespace

extern "C" {

int dmm_dayenu_build(dmm_ctx* ctx, int nfreq, int nmat, int nband, const double* freq, const double* bands, const uint8_t* mask, double* nf, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_build: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyMaxOrder, "dmm_dayenu_build: order %d outside 1 ... %d", nfreq, kDyMaxOrder);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535, "dmm_dayenu_build: bad matrix count %d", nmat);
  DMM_REQUIRE(nband >= 1, "dmm_dayenu_build: bad stop band count %d", nband);
  if (nmat == 0) return DMM_OK;
  DMM_REQUIRE(freq && bands && mask && nf && status, "dmm_dayenu_build: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int n = nfreq;
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)nmat * n * n * sizeof(double), &scratch);
  if (rc) return rc;
  DMM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * nmat, ctx->stream));
  hipLaunchKernelGGL(k_dy_cov, dim3((unsigned)(((int64_t)n * n + 255) / 256), (unsigned)nmat), dim3(256), 0, ctx->stream, n, nband, freq, bands, mask, nf);
  hipLaunchKernelGGL(k_dy_chol, dim3((unsigned)nmat), dim3((unsigned)((n + 63) / 64 * 64)), 0, ctx->stream, n, nf, status);
  hipLaunchKernelGGL(k_dy_inv, dim3((unsigned)((n + 63) / 64), (unsigned)nmat), dim3(64), 0, ctx->stream, n, (const double*)nf, (double*)scratch, (const int32_t*)status);
  const int nt = (n + 63) / 64;
  hipLaunchKernelGGL(k_dy_prod, dim3((unsigned)(nt * nt), (unsigned)nmat), dim3(256), 0, ctx->stream, n, (const double*)scratch, mask, (const int32_t*)status, nf);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dayenu_mask(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, const dmm_dayenu_side* weight, uint8_t* flag) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_mask: ctx is NULL");
  DMM_REQUIRE(dtype == DMM_DAYENU_F32 || dtype == DMM_DAYENU_F64, "dmm_dayenu_mask: bad dtype %d", dtype);
  DMM_REQUIRE(layout == DMM_DAYENU_COLS || layout == DMM_DAYENU_ITEMS, "dmm_dayenu_mask: bad layout %d", layout);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyMaxOrder, "dmm_dayenu_mask: order %d outside 1 ... %d", nfreq, kDyMaxOrder);
  DMM_REQUIRE(ninner >= 0 && nouter >= 0 && nouter <= 65535, "dmm_dayenu_mask: bad item counts %d x %d", nouter, ninner);
  DMM_REQUIRE(weight && weight->ptr && flag, "dmm_dayenu_mask: NULL argument");
  DMM_REQUIRE(dy_side_ok(weight), "dmm_dayenu_mask: negative count or stride");
  if (ninner == 0 || nouter == 0) return DMM_OK;
  DMM_HIP(hipSetDevice(ctx->device));
  const DySide w = dy_side(weight);
  if (layout == DMM_DAYENU_COLS) {
    const dim3 g((unsigned)ninner, (unsigned)nfreq, (unsigned)nouter);
    if (dtype == DMM_DAYENU_F32) hipLaunchKernelGGL(k_dy_mask_cols<float>, g, dim3(256), 0, ctx->stream, w, nfreq, ninner, flag);
    else hipLaunchKernelGGL(k_dy_mask_cols<double>, g, dim3(256), 0, ctx->stream, w, nfreq, ninner, flag);
  } else {
    const dim3 g((unsigned)((ninner + 63) / 64), (unsigned)nfreq, (unsigned)nouter);
    if (dtype == DMM_DAYENU_F32) hipLaunchKernelGGL(k_dy_mask_items<float>, g, dim3(64), 0, ctx->stream, w, nfreq, ninner, flag);
    else hipLaunchKernelGGL(k_dy_mask_items<double>, g, dim3(64), 0, ctx->stream, w, nfreq, ninner, flag);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dayenu_apply(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, const double* nf, int nmat, const int32_t* item_matrix, const uint8_t* atten,
                     const int32_t* units, int64_t nunit, const dmm_dayenu_side* data, const dmm_dayenu_side* weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_apply: ctx is NULL");
  DMM_REQUIRE(dtype == DMM_DAYENU_F32 || dtype == DMM_DAYENU_F64, "dmm_dayenu_apply: bad dtype %d", dtype);
  DMM_REQUIRE(layout == DMM_DAYENU_COLS || layout == DMM_DAYENU_ITEMS, "dmm_dayenu_apply: bad layout %d", layout);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyMaxOrder, "dmm_dayenu_apply: order %d outside 1 ... %d", nfreq, kDyMaxOrder);
  DMM_REQUIRE(ninner >= 0 && nouter >= 0 && nmat >= 0 && nunit >= 0, "dmm_dayenu_apply: negative count");
  DMM_REQUIRE(nunit <= 0x7fffffff, "dmm_dayenu_apply: %lld units do not fit the grid", (long long)nunit);
  if (ninner == 0 || nouter == 0 || nunit == 0) return DMM_OK;
  DMM_REQUIRE(nf && item_matrix, "dmm_dayenu_apply: NULL argument");
  DMM_REQUIRE((data && data->ptr) || (weight && weight->ptr), "dmm_dayenu_apply: neither data nor weight given");
  DMM_REQUIRE((!data || dy_side_ok(data)) && (!weight || dy_side_ok(weight)), "dmm_dayenu_apply: negative count or stride");
  DMM_HIP(hipSetDevice(ctx->device));
  DyApplyArgs a{};
  a.nf = nf;
  a.imat = item_matrix;
  a.atten = atten;
  a.units = units;
  a.d = dy_side(data);
  a.w = dy_side(weight);
  a.n = nfreq;
  a.n16 = (nfreq + 15) / 16 * 16;
  a.nmat = nmat;
  a.layout = layout;
  a.ninner = ninner;
  a.nouter = nouter;
  if (dtype == DMM_DAYENU_F32) return launch_apply<float, 2>(ctx, a, nunit);
  return launch_apply<double, 1>(ctx, a, nunit);
}

}  // extern "C"
