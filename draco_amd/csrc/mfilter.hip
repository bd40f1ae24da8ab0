// DAYENU m-mode filter along right ascension (draco/analysis/dayenu.py:977-1122, 1235-1427).
//
// Per frequency of vis [freq, stack, ra] complex64 / weight float32: one RA mask for all baselines (an RA is kept where
// more than 90 % of the baselines that have any weight have weight there), and per filter kind (band-pass for the
// intra-cylinder baselines, low-pass on the fringe-stopped inter-cylinder ones) the covariance
//   C[i][j] = diag d_ij + coef sinc(m_cut (ra_i - ra_j) / pi) cos(m_center (ra_i - ra_j))
// on the kept RAs.  The filter is C^-1 on the kept block and zero elsewhere; it is never formed: C = U^T U and the
// 2 nentry real right-hand sides of the frequency are solved (n^3 / 3 + 4 n^2 nentry flop instead of an n^3 inverse and
// an n x n matrix per kind).  Only the builder functions need the matrix itself: the same solve on a masked identity.
//
// Stages, all float64 inside, batched over matrices = (frequency, kind):
//   k_mf_gb / k_mf_count / k_mf_wmul   the mask: gb[f][s] = any_ra(weight > 0); flag[f][ra] = (count over gb of
//                 weight > 0) > 0.90 * len(gb) in float64; the state word of the frequency; weight *= flag;
//   k_mf_cov      G [nmat][n][n] from ra, (diag, coef, m_cut, m_center) and the mask, masked rows and columns identity;
//   k_mf_pack     Y [nmat][2 nentry][n]: rows 2 e, 2 e + 1 the real and imaginary part of entry e times its mixer
//                 exp(-i m ra), zero at masked RAs; k_mf_unpack undoes the mixer, rounds to complex64, exact zeros at
//                 masked RAs.  RA is the contiguous axis on both sides: a wave moves 512 contiguous bytes of vis and
//                 two runs of 512 bytes of Y;
//   chol_blocked.hip   G = U^T U and the two triangular solves on the rows of Y (dl_factor and dl_solve_rows of
//                 chol_blocked.h: the one compiled copy that delay.hip and dpss.hip call too);
//   k_mf_eye      the masked identity as right-hand sides, and the (mask x mask) zeroing of the solution.
// A non-positive pivot sets the matrix's status word; every later kernel leaves that matrix alone.
//
// Index ranges at n = 4096: i * n + j < 2^24 inside a matrix; every offset that carries a batch, frequency or entry
// index is formed in size_t; grid dimensions are checked against 65535 (y, z) and 2^31 - 1 (x) on the host.
#include "chol_blocked.h"

#include <algorithm>

namespace {

constexpr int kMfMaxOrder = 4096;
constexpr int kMfRowChunk = 1 << 21;  // right-hand-side rows per pass of the solves (k_dl_gemm's grid.y holds 65535 x 64)

__global__ __launch_bounds__(256) void k_mf_gb(int nstack, int nra, const float* __restrict__ w, uint8_t* __restrict__ gb) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= nstack) return;  // (whole waves)
  const float* __restrict__ row = w + ((size_t)f * nstack + s) * nra;
  int any = 0;
  for (int r = lane; r < nra; r += 64) any |= row[r] > 0.0f ? 1 : 0;
  const int all = __any(any);
  if (lane == 0) gb[(size_t)f * nstack + s] = (uint8_t)(all ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_mf_count(int nstack, int nra, const float* __restrict__ w, const uint8_t* __restrict__ gb, uint8_t* __restrict__ flag, int32_t* __restrict__ state) {
  const int f = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  const uint8_t* __restrict__ g = gb + (size_t)f * nstack;
  const float* __restrict__ wf = w + (size_t)f * nstack * nra;
  int cnt = 0, ngb = 0;
  for (int s = 0; s < nstack; ++s) {
    if (!g[s]) continue;  // (the same in every thread)
    ++ngb;
    if (r < nra) cnt += wf[(size_t)s * nra + r] > 0.0f ? 1 : 0;
  }
  const int keep = (r < nra && ngb > 0 && (double)cnt > 0.90 * (double)ngb) ? 1 : 0;
  if (r < nra) flag[(size_t)f * nra + r] = (uint8_t)keep;
  const int any = __syncthreads_or(keep);
  if (threadIdx.x == 0 && ngb > 0) atomicMax(&state[f], any ? DMM_MFILTER_FILTER : DMM_MFILTER_WEIGHT_ONLY);
}

__global__ __launch_bounds__(256) void k_mf_wmul(int64_t per_freq, int nra, float* __restrict__ w, const uint8_t* __restrict__ flag, const int32_t* __restrict__ state) {
  const int f = blockIdx.y;
  if (state[f] == DMM_MFILTER_UNTOUCHED) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per_freq) return;
  const int r = (int)(e % nra);
  float* p = w + (size_t)f * per_freq + e;
  *p = *p * (flag[(size_t)f * nra + r] ? 1.0f : 0.0f);
}

__global__ __launch_bounds__(256) void k_mf_cov(int n, const double* __restrict__ ra, const double* __restrict__ par, const uint8_t* __restrict__ mask, double* __restrict__ Gall) {
  const int mat = blockIdx.z, i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint8_t* __restrict__ mk = mask + (size_t)mat * n;
  double v;
  if (mk[i] && mk[j]) {
    const double diag = par[4 * mat], coef = par[4 * mat + 1], mcut = par[4 * mat + 2], mcen = par[4 * mat + 3];
    const double dra = ra[i] - ra[j];
    const double x = mcut * dra / M_PI, y = M_PI * x;
    const double sc = x == 0.0 ? 1.0 : sin(y) / y;
    v = coef * sc * cos(mcen * dra);
    if (i == j) v += diag;
  } else {
    v = i == j ? 1.0 : 0.0;
  }
  Gall[((size_t)mat * n + i) * n + j] = v;
}

struct MfRows {
  int n, nstack, nent, nbr;
  const int32_t* mat_freq;
  const int32_t* entry;
  const double* mix;  // [nmat][nent] or nullptr (unit mixer)
  const double* ra;
  const uint8_t* mask;
  const int32_t* status;
  float2* vis;
  double* Y;
};

template <bool kUnpack>
__global__ __launch_bounds__(256) void k_mf_rows(MfRows a) {
  const int mat = blockIdx.y;
  if (a.status[mat]) return;
  const int ent = blockIdx.x / a.nbr, r = (blockIdx.x % a.nbr) * 256 + threadIdx.x;
  if (r >= a.n) return;
  const int n = a.n;
  float2* v = a.vis + ((size_t)a.mat_freq[mat] * a.nstack + a.entry[ent]) * n + r;
  double* y0 = a.Y + ((size_t)mat * 2 * a.nent + 2 * ent) * n + r;
  double* y1 = y0 + n;
  const bool keep = a.mask[(size_t)mat * n + r] != 0;
  double sn = 0.0, cs = 1.0;
  if (keep && a.mix) sincos(a.mix[(size_t)mat * a.nent + ent] * a.ra[r], &sn, &cs);
  if (!kUnpack) {
    double yr = 0.0, yi = 0.0;
    if (keep) {
      const float2 z = *v;
      const double vr = (double)z.x, vi = (double)z.y;
      yr = a.mix ? vr * cs + vi * sn : vr;  // (vr + i vi) (cs - i sn)
      yi = a.mix ? vi * cs - vr * sn : vi;
    }
    *y0 = yr;
    *y1 = yi;
  } else {
    float2 o = make_float2(0.0f, 0.0f);
    if (keep) {
      const double xr = *y0, xi = *y1;
      o.x = (float)(a.mix ? xr * cs - xi * sn : xr);  // (xr + i xi) (cs + i sn)
      o.y = (float)(a.mix ? xr * sn + xi * cs : xi);
    }
    *v = o;
  }
}

__global__ __launch_bounds__(256) void k_mf_eye(int n, int stage, const uint8_t* __restrict__ mask, double* __restrict__ Yall, const int32_t* __restrict__ status) {
  const int mat = blockIdx.z, i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint8_t* __restrict__ mk = mask + (size_t)mat * n;
  double* p = Yall + ((size_t)mat * n + i) * n + j;
  if (stage == 0) *p = (i == j && mk[i]) ? 1.0 : 0.0;
  else if (status[mat] || !(mk[i] && mk[j])) *p = 0.0;
}

int mf_rows(dmm_ctx* ctx, const char* who, bool unpack, int nra, int nstack, int nmat, int nent, const int32_t* mat_freq, const int32_t* entry, const double* mix, const double* ra,
            const uint8_t* mask, const int32_t* status, void* vis, double* Y) {
  DMM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
  DMM_REQUIRE(nra >= 1 && nra <= kMfMaxOrder, "%s: order %d outside 1 ... %d", who, nra, kMfMaxOrder);
  DMM_REQUIRE(nstack >= 1, "%s: bad stack size %d", who, nstack);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535 && nent >= 0, "%s: bad matrix or entry count %d, %d", who, nmat, nent);
  if (nmat == 0 || nent == 0) return DMM_OK;
  DMM_REQUIRE(mat_freq && entry && ra && mask && status && vis && Y, "%s: NULL argument", who);
  const int nbr = (nra + 255) / 256;
  DMM_REQUIRE((int64_t)nent * nbr <= 0x7fffffff, "%s: too many entries %d", who, nent);
  DMM_HIP(hipSetDevice(ctx->device));
  MfRows a{nra, nstack, nent, nbr, mat_freq, entry, mix, ra, mask, status, (float2*)vis, Y};
  const dim3 grid((unsigned)((int64_t)nent * nbr), (unsigned)nmat);
  if (unpack) hipLaunchKernelGGL(k_mf_rows<true>, grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_mf_rows<false>, grid, dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // namespace

extern "C" {

int dmm_mfilter_mask(dmm_ctx* ctx, int nfreq, int nstack, int nra, float* weight, uint8_t* flag, int32_t* state) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mfilter_mask: ctx is NULL");
  DMM_REQUIRE(nra >= 1 && nra <= kMfMaxOrder, "dmm_mfilter_mask: order %d outside 1 ... %d", nra, kMfMaxOrder);
  DMM_REQUIRE(nfreq >= 0 && nfreq <= 65535 && nstack >= 1, "dmm_mfilter_mask: bad frequency or stack count %d, %d", nfreq, nstack);
  if (nfreq == 0) return DMM_OK;
  DMM_REQUIRE(weight && flag && state, "dmm_mfilter_mask: NULL argument");
  const int64_t per_freq = (int64_t)nstack * nra;
  DMM_REQUIRE((per_freq + 255) / 256 <= 0x7fffffff, "dmm_mfilter_mask: too many stack entries %d", nstack);
  DMM_HIP(hipSetDevice(ctx->device));
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)nfreq * nstack, &scratch);
  if (rc) return rc;
  uint8_t* gb = (uint8_t*)scratch;
  DMM_HIP(hipMemsetAsync(state, 0, sizeof(int32_t) * nfreq, ctx->stream));
  hipLaunchKernelGGL(k_mf_gb, dim3((unsigned)((nstack + 3) / 4), (unsigned)nfreq), dim3(256), 0, ctx->stream, nstack, nra, (const float*)weight, gb);
  hipLaunchKernelGGL(k_mf_count, dim3((unsigned)((nra + 255) / 256), (unsigned)nfreq), dim3(256), 0, ctx->stream, nstack, nra, (const float*)weight, (const uint8_t*)gb, flag, state);
  hipLaunchKernelGGL(k_mf_wmul, dim3((unsigned)((per_freq + 255) / 256), (unsigned)nfreq), dim3(256), 0, ctx->stream, per_freq, nra, weight, (const uint8_t*)flag, (const int32_t*)state);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_mfilter_cov(dmm_ctx* ctx, int nra, int nmat, const double* ra, const double* params, const uint8_t* mask, double* G, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mfilter_cov: ctx is NULL");
  DMM_REQUIRE(nra >= 1 && nra <= kMfMaxOrder, "dmm_mfilter_cov: order %d outside 1 ... %d", nra, kMfMaxOrder);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535, "dmm_mfilter_cov: bad matrix count %d", nmat);
  if (nmat == 0) return DMM_OK;
  DMM_REQUIRE(ra && params && mask && G && status, "dmm_mfilter_cov: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  DMM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * nmat, ctx->stream));
  hipLaunchKernelGGL(k_mf_cov, dim3((unsigned)((nra + 255) / 256), (unsigned)nra, (unsigned)nmat), dim3(256), 0, ctx->stream, nra, ra, params, mask, G);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_mfilter_pack(dmm_ctx* ctx, int nra, int nstack, int nmat, int nent, const int32_t* mat_freq, const int32_t* entry, const double* mix, const double* ra, const uint8_t* mask,
                     const int32_t* status, const void* vis, double* Y) {
  return mf_rows(ctx, "dmm_mfilter_pack", false, nra, nstack, nmat, nent, mat_freq, entry, mix, ra, mask, status, (void*)vis, Y);
}

int dmm_mfilter_unpack(dmm_ctx* ctx, int nra, int nstack, int nmat, int nent, const int32_t* mat_freq, const int32_t* entry, const double* mix, const double* ra, const uint8_t* mask,
                       const int32_t* status, const double* Y, void* vis) {
  return mf_rows(ctx, "dmm_mfilter_unpack", true, nra, nstack, nmat, nent, mat_freq, entry, mix, ra, mask, status, vis, (double*)Y);
}

int dmm_mfilter_solve(dmm_ctx* ctx, int nra, int nrow, int nmat, double* G, double* Y, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mfilter_solve: ctx is NULL");
  DMM_REQUIRE(nra >= 1 && nra <= kMfMaxOrder, "dmm_mfilter_solve: order %d outside 1 ... %d", nra, kMfMaxOrder);
  DMM_REQUIRE(nrow >= 0, "dmm_mfilter_solve: bad row count %d", nrow);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535, "dmm_mfilter_solve: bad matrix count %d", nmat);
  if (nmat == 0) return DMM_OK;
  DMM_REQUIRE(G && status && (Y || nrow == 0), "dmm_mfilter_solve: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  dl_factor(ctx, nra, nmat, G, status, DMM_MFILTER_NOT_POSDEF);
  for (int r0 = 0; r0 < nrow; r0 += kMfRowChunk)
    dl_solve_rows(ctx, nra, nrow, std::min(kMfRowChunk, nrow - r0), nmat, G, Y + (size_t)r0 * nra, status);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_mfilter_eye(dmm_ctx* ctx, int nra, int nmat, int stage, const uint8_t* mask, double* Y, const int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mfilter_eye: ctx is NULL");
  DMM_REQUIRE(nra >= 1 && nra <= kMfMaxOrder, "dmm_mfilter_eye: order %d outside 1 ... %d", nra, kMfMaxOrder);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535, "dmm_mfilter_eye: bad matrix count %d", nmat);
  DMM_REQUIRE(stage == 0 || stage == 1, "dmm_mfilter_eye: bad stage %d", stage);
  if (nmat == 0) return DMM_OK;
  DMM_REQUIRE(mask && Y && status, "dmm_mfilter_eye: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_mf_eye, dim3((unsigned)((nra + 255) / 256), (unsigned)nra, (unsigned)nmat), dim3(256), 0, ctx->stream, nra, stage, mask, Y, status);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
