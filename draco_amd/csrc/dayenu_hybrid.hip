// DAYENU filter of hybrid beam-formed visibilities (draco/analysis/dayenu.py:407-572) and the east-west averages of
// RADependentWeights (draco/analysis/ringmapmaker.py:1202-1315).
//
// vis [pol, freq, ew, el, ra] c64, weight [pol, freq, ew, ra] f32, filter / freq_cov [pol, freq, freq_sum, ew, ra] f64:
// ra is the innermost axis of all of them, so lanes run along ra in every kernel here and a wave instruction touches
// whole contiguous lines.  One filter per (ew, ra) sample: imat [new][nra] int32 names it (< 0: none).  The filters are
// built by dmm_dayenu_build and applied by dmm_dayenu_apply in its items-contiguous form (csrc/dayenu.hip).
//
//   k_dyh_mask   flag[f, x, t] = all_pol(weight > 0); nothing is written back.
//   k_dyh_save   out[p, f, f', x, t] = NF[imat[x, t]][f, f']: a pure store stream.  A wave owns 64 adjacent RA of one
//                ew; where they share a filter (tested per wave) the value is one wave-uniform read, otherwise a gather.
//                Read once, stored for every polarisation from the same register.
//   k_dyh_cov    C[p, f, f', x, t] = sum_k NF[f, k] NF[f', k] var[p, k, x, t], var = inz(weight) taken in float32.
//                Over RA this is a GEMM with rows (f, f'), columns t and depth k: a block stages the variances of 32
//                adjacent RA of one (pol, ew), every channel, in LDS (the B operand); a wave takes a row f and walks the
//                16-row tiles f' <= f: A = NF[f, k] NF[f', k], one multiply per v_mfma_f64_16x16x4_f64, formed from NF
//                rows that stream through the cache (NF of order 1024 does not fit LDS).  C is symmetric: tiles strictly
//                below the diagonal tile are stored to both triangles, the diagonal tile is computed whole (a product
//                commutes and the k order is the same, so the two halves agree bit for bit).  Columns of a stripe that
//                hold different filters: one MFMA pass per distinct filter with the other columns zeroed, as
//                k_dy_apply does.  The k order of a sample's sum is fixed, so the result does not depend on which
//                other samples share the launch.
//   k_ew_coef    per (pol, freq): the RA mean of var per ew, the ew weights of the scheme, and from them the
//                coefficients of the two averages and of the RA dependence.
//   k_ew_scale   ringmap weight [pol, freq, ra, el] *= num[p, f] inz(sum_ew w^2 var[p, f, ew, ra]).
//   k_ew_average out[a, t] = sum_ew coef[a / rows_per_coef, ew] in[a, ew, t], float64, in ew order.
#include "chol_blocked.h"

#include <algorithm>

namespace {

constexpr int kDyhMaxOrder = 1024;
constexpr int kCovW = 32;        // RA samples of a covariance stripe
constexpr int kCovP = kCovW + 4;  // its pitch in LDS: the four k rows of a read fall on different banks
typedef double dyh_run __attribute__((ext_vector_type(4), aligned(8)));  // four adjacent float64 of a row of NF (rows are 8-byte aligned)

__device__ __forceinline__ float dyh_inz(float x) { return x != 0.0f ? 1.0f / x : 0.0f; }
__device__ __forceinline__ double dyh_inz(double x) { return x != 0.0 ? 1.0 / x : 0.0; }

__global__ __launch_bounds__(256) void k_dyh_mask(int npol, int n, int64_t nxt, const float* __restrict__ w, uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= nxt) return;
  bool all = true;
  for (int p = 0; p < npol; ++p) all = all && w[((size_t)p * n + f) * nxt + i] > 0.0f;
  flag[(size_t)f * nxt + i] = all ? 1 : 0;
}

// grid (ceil(nra / 64), new, z): wave q of block z takes the matrix elements e = 4 z + q, stride 4 gridDim.z.
__global__ __launch_bounds__(256) void k_dyh_save(int npol, int n, int new_, int nra, const double* __restrict__ nf, int nmat, const int32_t* __restrict__ imat, int skip_negative,
                                                   double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane, x = blockIdx.y;
  const bool in = t < nra;
  int m = in ? imat[(size_t)x * nra + t] : -1;
  if (m >= nmat) m = -1;
  if (!in || (m < 0 && skip_negative)) m = -3;  // no store
  const int m0 = __builtin_amdgcn_readfirstlane(m);
  const bool uniform = __all(m == m0);
  if (uniform && m0 == -3) return;
  const int64_t nn = (int64_t)n * n;
  const size_t plane = (size_t)new_ * nra;
  const size_t pstride = (size_t)nn * plane;
  double* o = out + (size_t)x * nra + t;
  const double* __restrict__ mine = nf + (size_t)max(m, 0) * nn;
  const double* __restrict__ shared = nf + (size_t)max(m0, 0) * nn;
  for (int64_t e = (int64_t)blockIdx.z * 4 + wave; e < nn; e += 4 * (int64_t)gridDim.z) {
    double v;
    if (uniform) v = m0 >= 0 ? shared[e] : 0.0;
    else v = m >= 0 ? mine[e] : 0.0;
    if (m != -3)
      for (int p = 0; p < npol; ++p) o[(size_t)p * pstride + (size_t)e * plane] = v;
  }
}

// grid (ceil(nra / 32), npol * new, z); dynamic LDS n16 * kCovP floats.  Wave q of block z takes the rows
// f = 4 z + q, stride 4 gridDim.z.
__global__ __launch_bounds__(256) void k_dyh_cov(int npol, int n, int n16, int new_, int nra, const double* __restrict__ nf, int nmat, const int32_t* __restrict__ imat,
                                                  const float* __restrict__ weight, int skip_negative, double* __restrict__ out) {
  constexpr int W = kCovW, P = kCovP;
  extern __shared__ __align__(16) unsigned char dyh_smem[];
  float* xs = reinterpret_cast<float*>(dyh_smem);
  __shared__ int s_cm[W];
  __shared__ int s_mats[W];
  __shared__ int s_nm;

  const int t0 = blockIdx.x * W;
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra;

  if (threadIdx.x < W) {
    const int t = t0 + threadIdx.x;
    int m = -3;  // outside the axis: never stored
    if (t < nra) {
      m = imat[(size_t)x * nra + t];
      if (m >= nmat || m < 0) m = skip_negative ? -3 : -1;  // -1: stored as zero
    }
    s_cm[threadIdx.x] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int nm = 0;
    for (int c = 0; c < W; ++c) {
      const int m = s_cm[c];
      if (m < 0) continue;
      bool seen = false;
      for (int q = 0; q < nm; ++q) seen = seen || s_mats[q] == m;
      if (!seen) s_mats[nm++] = m;
    }
    s_nm = nm;
  }
  // ---- the variances of the stripe, every channel (zero rows up to the next multiple of 16, zero columns where
  // there is no filter)
  const float* __restrict__ wp = weight + (size_t)p * n * plane + (size_t)x * nra;
  for (int e = threadIdx.x; e < n16 * W; e += 256) {
    const int k = e / W, c = e % W;
    float v = 0.0f;
    if (k < n && s_cm[c] >= 0) v = dyh_inz(wp[(size_t)k * plane + t0 + c]);
    xs[k * P + c] = v;
  }
  __syncthreads();
  const int nm = s_nm;
  bool any = false;
  for (int c = 0; c < W; ++c) any = any || s_cm[c] != -3;
  if (!any) return;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  int cm[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) cm[u] = s_cm[16 * u + lr];
  double* __restrict__ obase = out + (size_t)p * n * n * plane + (size_t)x * nra + t0;

  for (int f = (int)blockIdx.z * 4 + wave; f < n; f += 4 * (int)gridDim.z) {
    const int jd = f / 16 * 16;  // the diagonal tile
    for (int j0 = 0; j0 <= jd; j0 += 16) {
      v4d acc[2] = {vz, vz};
      const int rowj = j0 + lr;
      for (int q = 0; q < nm; ++q) {
        const int m = s_mats[q];
        const double* __restrict__ pf = nf + ((size_t)m * n + f) * n;
        const double* __restrict__ pj = nf + ((size_t)m * n + min(rowj, n - 1)) * n;
        // (one filter in the stripe: its columns are all the non-zero ones)
        const bool mine0 = nm == 1 || cm[0] == m, mine1 = nm == 1 || cm[1] == m;
        double af[4], aj[4];  // the two rows of NF, one K-chunk ahead
        auto fetch = [&](int k0) {
          const int kb = k0 + 4 * lk;
          if (kb + 3 < n) {  // a lane's four k are adjacent: one 32-byte run per row
            const dyh_run vf = *reinterpret_cast<const dyh_run*>(pf + kb), vj = *reinterpret_cast<const dyh_run*>(pj + kb);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              af[s] = vf[s];
              aj[s] = rowj < n ? vj[s] : 0.0;
            }
          } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const int k = kb + s;
              const int kc = min(k, n - 1);
              af[s] = pf[kc];
              aj[s] = (k < n && rowj < n) ? pj[kc] : 0.0;
            }
          }
        };
        fetch(0);
        for (int k0 = 0; k0 < n16; k0 += 16) {
          double a[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) a[s] = af[s] * aj[s];
          if (k0 + 16 < n16) fetch(k0 + 16);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float* xr = xs + (k0 + 4 * lk + s) * P + lr;
            const double b0 = mine0 ? (double)xr[0] : 0.0;
            const double b1 = mine1 ? (double)xr[16] : 0.0;
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b1, acc[1], 0, 0, 0);
          }
        }
      }
      // ---- acc[u][reg] = C[f, j0 + lk + 4 reg] of sample 16 u + lr: both triangles, lines along ra
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (cm[u] == -3) continue;
        const int c = 16 * u + lr;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int j = j0 + lk + 4 * reg;
          if (j >= n) continue;
          const double v = cm[u] >= 0 ? acc[u][reg] : 0.0;
          obase[((size_t)f * n + j) * plane + c] = v;
          if (j0 < jd) obase[((size_t)j * n + f) * plane + c] = v;
        }
      }
    }
  }
}

// One block per (pol, freq).  scheme 0: w = table (natural or uniform, the excluded ew already zero); 1: inverse
// variance, w = inz(mean_ra var) table (table = 1 or 0).
__global__ __launch_bounds__(256) void k_ew_coef(int new_, int nra, int scheme, const double* __restrict__ table, const float* __restrict__ weight, double* __restrict__ coef_f,
                                                  double* __restrict__ coef_c, double* __restrict__ w2, double* __restrict__ num) {
  __shared__ double red[256];
  __shared__ double s_mean[64];
  const size_t pf = blockIdx.x;
  for (int x = 0; x < new_; ++x) {
    const float* __restrict__ wr = weight + (pf * new_ + x) * nra;
    double s = 0.0;
    for (int t = threadIdx.x; t < nra; t += 256) s += (double)dyh_inz(wr[t]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) s_mean[x] = red[0] / (double)nra;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double sw = 0.0, sn = 0.0;
    for (int x = 0; x < new_; ++x) {
      const double w = scheme == 1 ? dyh_inz(s_mean[x]) * table[x] : table[x];
      sw += w;
      sn += (w * w) * s_mean[x];
    }
    const double isw = dyh_inz(sw), isw2 = dyh_inz(sw * sw);
    for (int x = 0; x < new_; ++x) {
      const double w = scheme == 1 ? dyh_inz(s_mean[x]) * table[x] : table[x];
      coef_f[pf * new_ + x] = w * isw;
      coef_c[pf * new_ + x] = (w * w) * isw2;
      w2[pf * new_ + x] = w * w;
    }
    num[pf] = sn;
  }
}

// grid (ceil(nra * nel / 256), npol * nfreq): lanes along (ra, el), the ring map's innermost axes.
__global__ __launch_bounds__(256) void k_ew_scale(int new_, int nra, int nel, const float* __restrict__ weight, const double* __restrict__ w2, const double* __restrict__ num,
                                                   double* __restrict__ rweight) {
  const size_t pf = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nra * nel) return;
  const int t = (int)(i / nel);
  double s = 0.0;
  for (int x = 0; x < new_; ++x) s = s + w2[pf * new_ + x] * (double)dyh_inz(weight[(pf * new_ + x) * nra + t]);
  rweight[pf * nra * nel + i] *= num[pf] * dyh_inz(s);
}

// grid (ceil(nra / 256), rows).
__global__ __launch_bounds__(256) void k_ew_average(size_t row0, int64_t rows_per_coef, int new_, int nra, const double* __restrict__ coef, const double* __restrict__ in, double* __restrict__ out) {
  const size_t a = row0 + (size_t)blockIdx.y + (size_t)blockIdx.z * 65535;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nra) return;
  const double* __restrict__ c = coef + (a / (size_t)rows_per_coef) * new_;
  const double* __restrict__ r = in + a * new_ * nra + t;
  double s = 0.0;
  for (int x = 0; x < new_; ++x) s = __dadd_rn(s, __dmul_rn(c[x], r[(size_t)x * nra]));
  out[a * nra + t] = s;
}

bool dyh_shape_ok(int npol, int nfreq, int new_, int nra) { return npol >= 1 && npol <= 65535 && nfreq >= 1 && nfreq <= kDyhMaxOrder && new_ >= 1 && new_ <= 65535 && nra >= 1; }

}  // namespace

extern "C" {

int dmm_dayenu_hybrid_mask(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const float* weight, uint8_t* flag) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_hybrid_mask: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyhMaxOrder, "dmm_dayenu_hybrid_mask: order %d outside 1 ... %d", nfreq, kDyhMaxOrder);
  DMM_REQUIRE(dyh_shape_ok(npol, nfreq, new_, nra), "dmm_dayenu_hybrid_mask: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(weight && flag, "dmm_dayenu_hybrid_mask: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t nxt = (int64_t)new_ * nra;
  hipLaunchKernelGGL(k_dyh_mask, dim3((unsigned)((nxt + 255) / 256), (unsigned)nfreq), dim3(256), 0, ctx->stream, npol, nfreq, nxt, weight, flag);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dayenu_hybrid_save(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const double* nf, int nmat, const int32_t* item_matrix, int skip_negative, double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_hybrid_save: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyhMaxOrder, "dmm_dayenu_hybrid_save: order %d outside 1 ... %d", nfreq, kDyhMaxOrder);
  DMM_REQUIRE(dyh_shape_ok(npol, nfreq, new_, nra), "dmm_dayenu_hybrid_save: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(nmat >= 0, "dmm_dayenu_hybrid_save: bad matrix count %d", nmat);
  DMM_REQUIRE(item_matrix && out && (nf || nmat == 0), "dmm_dayenu_hybrid_save: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t nn = (int64_t)nfreq * nfreq;
  const unsigned gz = (unsigned)std::min<int64_t>((nn + 3) / 4, 256);
  hipLaunchKernelGGL(k_dyh_save, dim3((unsigned)((nra + 63) / 64), (unsigned)new_, gz), dim3(256), 0, ctx->stream, npol, nfreq, new_, nra, nf, nmat, item_matrix, skip_negative, out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dayenu_hybrid_cov(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const double* nf, int nmat, const int32_t* item_matrix, const float* weight, int skip_negative,
                          double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dayenu_hybrid_cov: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kDyhMaxOrder, "dmm_dayenu_hybrid_cov: order %d outside 1 ... %d", nfreq, kDyhMaxOrder);
  DMM_REQUIRE(dyh_shape_ok(npol, nfreq, new_, nra), "dmm_dayenu_hybrid_cov: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE((int64_t)npol * new_ <= 65535, "dmm_dayenu_hybrid_cov: %d x %d (pol, ew) pairs do not fit the grid", npol, new_);
  DMM_REQUIRE(nmat >= 0, "dmm_dayenu_hybrid_cov: bad matrix count %d", nmat);
  DMM_REQUIRE(item_matrix && weight && out && (nf || nmat == 0), "dmm_dayenu_hybrid_cov: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int n16 = (nfreq + 15) / 16 * 16;
  const size_t lds = (size_t)n16 * kCovP * sizeof(float);
  const int64_t stripes = (int64_t)((nra + kCovW - 1) / kCovW) * npol * new_;
  // enough blocks to fill the device, each wave with at least one row
  const unsigned gz = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nfreq + 3) / 4, (2048 + stripes - 1) / stripes));
  DMM_HIP(hipFuncSetAttribute((const void*)k_dyh_cov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_dyh_cov, dim3((unsigned)((nra + kCovW - 1) / kCovW), (unsigned)(npol * new_), gz), dim3(256), lds, ctx->stream, npol, nfreq, n16, new_, nra, nf, nmat, item_matrix,
                     weight, skip_negative, out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_ew_coef(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int scheme, const double* table, const float* weight, double* coef_filter, double* coef_cov, double* w2,
                double* num) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ew_coef: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && nfreq >= 1 && nra >= 1 && (int64_t)npol * nfreq <= 0x7fffffff, "dmm_ew_coef: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(new_ >= 1 && new_ <= 64, "dmm_ew_coef: %d east-west baselines outside 1 ... 64", new_);
  DMM_REQUIRE(scheme == DMM_EW_TABLE || scheme == DMM_EW_INVERSE_VARIANCE, "dmm_ew_coef: bad scheme %d", scheme);
  DMM_REQUIRE(table && weight && coef_filter && coef_cov && w2 && num, "dmm_ew_coef: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_ew_coef, dim3((unsigned)(npol * nfreq)), dim3(256), 0, ctx->stream, new_, nra, scheme, table, weight, coef_filter, coef_cov, w2, num);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_ew_scale(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int nel, const float* weight, const double* w2, const double* num, double* ringmap_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ew_scale: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && nfreq >= 1 && new_ >= 1 && nra >= 1 && nel >= 1 && (int64_t)npol * nfreq <= 65535, "dmm_ew_scale: bad shape %d x %d x %d x %d x %d", npol, nfreq, new_,
              nra, nel);
  DMM_REQUIRE(weight && w2 && num && ringmap_weight, "dmm_ew_scale: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_ew_scale, dim3((unsigned)(((int64_t)nra * nel + 255) / 256), (unsigned)(npol * nfreq)), dim3(256), 0, ctx->stream, new_, nra, nel, weight, w2, num,
                     ringmap_weight);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_ew_average(dmm_ctx* ctx, int64_t nrow, int64_t rows_per_coef, int new_, int nra, const double* coef, const double* in, double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ew_average: ctx is NULL");
  DMM_REQUIRE(nrow >= 0 && rows_per_coef >= 1 && new_ >= 1 && nra >= 1, "dmm_ew_average: bad shape %lld x %d x %d (%lld rows per coefficient)", (long long)nrow, new_, nra,
              (long long)rows_per_coef);
  DMM_REQUIRE(nrow / 65535 <= 65535, "dmm_ew_average: %lld rows do not fit the grid", (long long)nrow);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(coef && in && out, "dmm_ew_average: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  // rows as (y, z) of the grid: z full slabs of 65535 rows, then the remainder
  const int64_t full = nrow / 65535, rest = nrow % 65535;
  const unsigned gx = (unsigned)((nra + 255) / 256);
  if (full) hipLaunchKernelGGL(k_ew_average, dim3(gx, 65535u, (unsigned)full), dim3(256), 0, ctx->stream, (size_t)0, rows_per_coef, new_, nra, coef, in, out);
  if (rest) hipLaunchKernelGGL(k_ew_average, dim3(gx, (unsigned)rest, 1u), dim3(256), 0, ctx->stream, (size_t)full * 65535, rows_per_coef, new_, nra, coef, in, out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
