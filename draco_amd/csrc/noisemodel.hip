// Frequency-correlated noise from the per-sample noise covariance of hybrid beam-formed visibilities: the Cholesky
// factors of ReconstructVisFreqCov and the sidereal weights of ReconstructVisWeight (draco/analysis/ringmapmaker.py:
// 1318-1712) and the colouring of FreqCorrelatedNoise (draco/synthesis/noise.py:377-470).
//
// freq_cov [pol, freq, freq_sum, ew, ra] f64 and weight [pol, freq, ew, ra] f32 of the hybrid stream have RA innermost;
// the factors go out as [pol, ew, ra, freq, freq_sum], one contiguous matrix per sample, sample s = (p new + x) nra + t
// in the reference's loop order; the coloured noise vis / vis_weight [pol, freq, ew, ns, ra] has RA innermost again.  So
// three of the kernels are transposes through LDS, with both their loads and their stores in contiguous runs:
//
//   k_nm_pack     G[s][i][j] (j >= i) = cov[p, j, i, x, t] scale[p, j, i, x] where both channels are valid (weight > 0),
//                 the identity's entry where one is not (an invalid channel is a unit row and column, so every matrix has
//                 order nfreq and the factor of the embedding is the factor of the valid block); the lower triangle of
//                 the input is the one read, as LAPACK's lower Cholesky does.  A block moves 32 samples x 32 entries of
//                 one row: loads with lanes along RA, stores with lanes along j.  weight_out = inz(G[s][i][i]), rounded
//                 once to float32, exactly 0 on invalid channels;
//   (dl_factor)   G = U^T U on the upper triangle, chol_blocked.hip; a non-positive pivot sets status[s];
//   k_nm_store    out[s][r][c] = U[c][r] for c <= r where both are valid, 0 elsewhere: 32 x 32 tiles turned in LDS;
//   k_nm_weight   vis_weight[f, stack, ra] = float(nb[stack] (double(hvw[cell[stack], f, ra]) nf[cell[stack], f])), 0
//                 where cell[stack] < 0, lanes along RA;
//   k_nc_colour   per RA a lower-triangular product out[f][c] = sum_{k <= f} L[f][k] z[k][c] over the 2 nns real columns
//                 of z (complex64, interleaved), float64 FMAs with k ascending, times inv_sqrt_red[ns], rounded once to
//                 float32: a block takes 16 RA x 16 rows x 32 columns, stages L and z in LDS in slices of 8 k, and turns
//                 the result in LDS so that a store is a run of 16 RA of one (f, ns);
//   k_nc_vw       vis_weight[f, ns, ra] = float(double(weight[f, ra]) red[ns]), lanes along RA;
//   k_nc_herm     on ew = 0: vis[po, f, 0, nns - k, ra] = conj(vis[pi, f, 0, k, ra]) for k = 1 ... nns / 2 (nns odd: the
//                 two halves do not overlap), and for pi == po the auto k = 0 becomes (sqrt(2) Re, 0) in float32.
// No floating-point atomics; every sum has an order fixed by the shapes, and no result depends on how the samples are
// chunked.
#include "chol_blocked.h"

namespace {

constexpr int kNmMaxOrder = 1024;
constexpr int kNmT = 32;  // tile edge of the transposes

struct NmSample {
  size_t p, x, t;
};
__device__ __forceinline__ NmSample nm_sample(int64_t s, int new_, int nra) {
  const size_t px = (size_t)s / (size_t)nra;
  return {px / (size_t)new_, px % (size_t)new_, (size_t)s % (size_t)nra};
}

// grid (ceil(ns / 32), n, ceil(n / 32)): row i = blockIdx.y, columns j = 32 blockIdx.z ...
__global__ __launch_bounds__(256) void k_nm_pack(int n, int new_, int nra, int64_t s0, int ns, const double* __restrict__ cov, const double* __restrict__ scale,
                                                  const float* __restrict__ weight, double* __restrict__ G, float* __restrict__ wout) {
  __shared__ double tile[kNmT][kNmT + 1];
  const int i = blockIdx.y, c0 = (int)blockIdx.z * kNmT;
  if (c0 + kNmT - 1 < i) return;  // (the whole block: wholly below the diagonal)
  const int lj = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t sl = (int64_t)blockIdx.x * kNmT + lj;
  const bool in = sl < ns;
  const NmSample q = nm_sample(s0 + (in ? sl : 0), new_, nra);
  const size_t plane = (size_t)new_ * nra, at = q.x * nra + q.t;
  const bool wi = weight[(q.p * n + i) * plane + at] > 0.0f;
#pragma unroll
  for (int it = 0; it < kNmT / 8; ++it) {
    const int e = g + 8 * it, j = c0 + e;
    double v = 0.0;
    if (in && j < n && j >= i) {
      const bool wj = weight[(q.p * n + j) * plane + at] > 0.0f;
      const size_t ent = (q.p * n + j) * n + i;
      if (wi && wj) v = cov[ent * plane + at] * scale[ent * new_ + q.x];
      else v = i == j ? 1.0 : 0.0;
      if (j == i) wout[(q.p * n + i) * plane + at] = wi ? (float)(v != 0.0 ? 1.0 / v : 0.0) : 0.0f;
    }
    tile[e][lj] = v;
  }
  __syncthreads();
  const int j = c0 + lj;
#pragma unroll
  for (int it = 0; it < kNmT / 8; ++it) {
    const int r = g + 8 * it;
    const int64_t s2 = (int64_t)blockIdx.x * kNmT + r;
    if (s2 < ns && j < n && j >= i) G[((size_t)s2 * n + i) * n + j] = tile[lj][r];
  }
}

// grid (ceil(n / 32)^2, ns): tile (rb, cb) of the output matrix of sample blockIdx.y
__global__ __launch_bounds__(256) void k_nm_store(int n, int new_, int nra, int64_t s0, const double* __restrict__ G, const float* __restrict__ weight,
                                                   const int32_t* __restrict__ status, double* __restrict__ out) {
  __shared__ double tile[kNmT][kNmT + 1];
  __shared__ uint8_t vr[kNmT], vc[kNmT];
  const int ntile = (n + kNmT - 1) / kNmT;
  const int rb = (int)blockIdx.x / ntile, cb = (int)blockIdx.x % ntile;
  const size_t sl = blockIdx.y;
  const NmSample q = nm_sample(s0 + (int64_t)sl, new_, nra);
  const size_t plane = (size_t)new_ * nra, at = q.x * nra + q.t;
  const bool ok = status[sl] == 0;
  const int lj = threadIdx.x & 31, g = threadIdx.x >> 5;
  if (threadIdx.x < 2 * kNmT) {
    const int f = (g == 0 ? rb : cb) * kNmT + lj;
    const uint8_t v = f < n && weight[(q.p * n + f) * plane + at] > 0.0f;
    if (g == 0) vr[lj] = v;
    else vc[lj] = v;
  }
  if (ok && cb <= rb) {  // U[c][r]: row c of G, column r
#pragma unroll
    for (int it = 0; it < kNmT / 8; ++it) {
      const int e = g + 8 * it, row = cb * kNmT + e, col = rb * kNmT + lj;
      tile[e][lj] = (row < n && col < n) ? G[(sl * n + row) * n + col] : 0.0;
    }
  }
  __syncthreads();
  double* __restrict__ o = out + (size_t)(s0 + (int64_t)sl) * n * n;
#pragma unroll
  for (int it = 0; it < kNmT / 8; ++it) {
    const int e = g + 8 * it, r = rb * kNmT + e, c = cb * kNmT + lj;
    if (r < n && c < n) o[(size_t)r * n + c] = (ok && c <= r && vr[e] && vc[lj]) ? tile[lj][e] : 0.0;
  }
}

// grid (ceil(nra / 256), nstack, nfreq)
__global__ __launch_bounds__(256) void k_nm_weight(int n, int nstack, int ncell, int nra, const float* __restrict__ hvw, const double* __restrict__ nf,
                                                    const int32_t* __restrict__ cell, const double* __restrict__ nb, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nra) return;
  const int st = blockIdx.y, f = blockIdx.z;
  const int c = cell[st];  // p new + x
  float v = 0.0f;
  if (c >= 0) {
    const int p = c / ncell, x = c % ncell;
    const size_t row = ((size_t)p * n + f) * ncell + x;
    v = (float)(nb[st] * ((double)hvw[row * nra + t] * nf[row]));
  }
  out[((size_t)f * nstack + st) * nra + t] = v;
}

constexpr int kNcR = 16, kNcF = 16, kNcC = 32, kNcK = 8;
constexpr int kNcLP = kNcF * kNcK + 2;    // doubles of one RA's slice of L (the pad spreads the RAs over the banks)
constexpr int kNcZP = kNcK * kNcC + 16;   // floats of one RA's slice of z
constexpr int kNcOP = kNcR + 1;           // pitch of one (f, column) run of the staged output
constexpr size_t kNcStage = kNcR * kNcLP * sizeof(double) + kNcR * kNcZP * sizeof(float);
constexpr size_t kNcOut = (size_t)kNcF * kNcC * kNcOP * sizeof(float);
constexpr size_t kNcLds = kNcStage > kNcOut ? kNcStage : kNcOut;
static_assert(kNcLds <= 65536, "static LDS");

// grid (ceil(nra / 16), ceil(n / 16), ceil(2 nns / 32)); thread (r = tid / 16, c = tid % 16) holds the 16 rows of the
// columns c and c + 16 of RA r.
__global__ __launch_bounds__(256) void k_nc_colour(int n, int new_, int nns, int nra, int p, int x, const double* __restrict__ L, const float* __restrict__ z,
                                                    const double* __restrict__ isr, float2* __restrict__ vis) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kNcLds];
  double* Ls = (double*)smem;
  float* zs = (float*)(smem + kNcR * kNcLP * sizeof(double));
  float* os = (float*)smem;
  const int ra0 = (int)blockIdx.x * kNcR, f0 = (int)blockIdx.y * kNcF, c0 = (int)blockIdx.z * kNcC;
  const int ncol = 2 * nns;
  const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
  const double* __restrict__ Lp = L + ((size_t)p * new_ + x) * nra * n * n;
  double acc0[kNcF], acc1[kNcF];
#pragma unroll
  for (int i = 0; i < kNcF; ++i) acc0[i] = acc1[i] = 0.0;
  const int kend = min(n, f0 + kNcF);  // k <= f: the last k any row of the tile takes
  for (int k0 = 0; k0 < kend; k0 += kNcK) {
#pragma unroll
    for (int it = 0; it < kNcR * kNcF * kNcK / 256; ++it) {
      const int idx = threadIdx.x + 256 * it;
      const int kk = idx % kNcK, fi = (idx / kNcK) % kNcF, rr = idx / (kNcK * kNcF);
      const int ra = ra0 + rr, f = f0 + fi, k = k0 + kk;
      Ls[rr * kNcLP + fi * kNcK + kk] = (ra < nra && f < n && k <= f) ? Lp[((size_t)ra * n + f) * n + k] : 0.0;  // (the strict upper triangle is not read)
    }
#pragma unroll
    for (int it = 0; it < kNcR * kNcK * kNcC / 256; ++it) {
      const int idx = threadIdx.x + 256 * it;
      const int cc = idx % kNcC, kk = (idx / kNcC) % kNcK, rr = idx / (kNcC * kNcK);
      const int ra = ra0 + rr, k = k0 + kk, col = c0 + cc;
      zs[rr * kNcZP + kk * kNcC + cc] = (ra < nra && k < kend && col < ncol) ? z[((size_t)ra * n + k) * ncol + col] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kNcK; ++kk) {
      const double z0 = (double)zs[r * kNcZP + kk * kNcC + c], z1 = (double)zs[r * kNcZP + kk * kNcC + c + 16];
#pragma unroll
      for (int fi = 0; fi < kNcF; ++fi) {
        const double l = Ls[r * kNcLP + fi * kNcK + kk];
        acc0[fi] = fma(l, z0, acc0[fi]);
        acc1[fi] = fma(l, z1, acc1[fi]);
      }
    }
    __syncthreads();
  }
  const int n0 = min((c0 + c) >> 1, nns - 1), n1 = min((c0 + c + 16) >> 1, nns - 1);
  const double s0 = isr[((size_t)p * new_ + x) * nns + n0], s1 = isr[((size_t)p * new_ + x) * nns + n1];
#pragma unroll
  for (int fi = 0; fi < kNcF; ++fi) {
    os[(fi * kNcC + c) * kNcOP + r] = (float)(acc0[fi] * s0);
    os[(fi * kNcC + c + 16) * kNcOP + r] = (float)(acc1[fi] * s1);
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kNcF * (kNcC / 2) * kNcR / 256; ++it) {
    const int idx = threadIdx.x + 256 * it;
    const int rr = idx % kNcR, nl = (idx / kNcR) % (kNcC / 2), fi = idx / (kNcR * (kNcC / 2));
    const int ra = ra0 + rr, f = f0 + fi, s = c0 / 2 + nl;
    if (ra < nra && f < n && s < nns)
      vis[((((size_t)p * n + f) * new_ + x) * nns + s) * nra + ra] = make_float2(os[(fi * kNcC + 2 * nl) * kNcOP + rr], os[(fi * kNcC + 2 * nl + 1) * kNcOP + rr]);
  }
}

// grid (ceil(nra / 256), nns, n)
__global__ __launch_bounds__(256) void k_nc_vw(int n, int new_, int nns, int nra, int p, int x, const float* __restrict__ weight, const int32_t* __restrict__ red,
                                                float* __restrict__ vw) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nra) return;
  const int s = blockIdx.y, f = blockIdx.z;
  const size_t row = ((size_t)p * n + f) * new_ + x;
  vw[(row * nns + s) * nra + t] = (float)((double)weight[row * nra + t] * (double)red[((size_t)p * new_ + x) * nns + s]);
}

// grid (ceil(nra / 256), nns / 2 + 1, npol * n): k = blockIdx.y
__global__ __launch_bounds__(256) void k_nc_herm(int n, int new_, int nns, int nra, const int32_t* __restrict__ pconj, float2* __restrict__ vis) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nra) return;
  const int k = blockIdx.y, pi = (int)blockIdx.z / n, f = (int)blockIdx.z % n;
  const int po = pconj[pi];
  const size_t src = ((((size_t)pi * n + f) * new_) * nns + k) * nra + t;
  const float2 v = vis[src];
  if (k == 0) {
    if (pi == po) vis[src] = make_float2(v.x * 1.41421356237309504880f, 0.0f);
    return;
  }
  vis[((((size_t)po * n + f) * new_) * nns + (nns - k)) * nra + t] = make_float2(v.x, -v.y);
}

bool nm_shape_ok(int npol, int nfreq, int new_, int nra) { return npol >= 1 && new_ >= 1 && (int64_t)npol * new_ <= 65535 && nfreq >= 1 && nfreq <= kNmMaxOrder && nra >= 1; }

}  // namespace

#define NM_ORDER(who, n) DMM_REQUIRE((n) >= 1 && (n) <= kNmMaxOrder, who ": order %d outside 1 ... %d", (n), kNmMaxOrder)
#define NM_CHUNK(who) \
  DMM_REQUIRE(nsample >= 1 && nsample <= 65535 && first >= 0 && first + nsample <= (int64_t)npol * new_ * nra, who ": bad sample range %lld + %d", (long long)first, nsample)

extern "C" {

int dmm_noisemodel_pack(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int64_t first, int nsample, const double* cov, const double* scale, const float* weight, double* G,
                        float* weight_out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noisemodel_pack: ctx is NULL");
  NM_ORDER("dmm_noisemodel_pack", nfreq);
  DMM_REQUIRE(nm_shape_ok(npol, nfreq, new_, nra), "dmm_noisemodel_pack: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  NM_CHUNK("dmm_noisemodel_pack");
  DMM_REQUIRE(cov && scale && weight && G && weight_out, "dmm_noisemodel_pack: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((nsample + kNmT - 1) / kNmT), (unsigned)nfreq, (unsigned)((nfreq + kNmT - 1) / kNmT));
  hipLaunchKernelGGL(k_nm_pack, grid, dim3(256), 0, ctx->stream, nfreq, new_, nra, first, nsample, cov, scale, weight, G, weight_out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_noisemodel_factor(dmm_ctx* ctx, int nfreq, int nsample, double* G, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noisemodel_factor: ctx is NULL");
  NM_ORDER("dmm_noisemodel_factor", nfreq);
  DMM_REQUIRE(nsample >= 1 && nsample <= 65535, "dmm_noisemodel_factor: bad matrix count %d", nsample);
  DMM_REQUIRE(G && status, "dmm_noisemodel_factor: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  DMM_HIP(hipMemsetAsync(status, 0, (size_t)nsample * sizeof(int32_t), ctx->stream));
  dl_factor(ctx, nfreq, nsample, G, status, DMM_NOISE_NOT_POSDEF);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_noisemodel_store(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int64_t first, int nsample, const double* G, const float* weight, const int32_t* status,
                         double* freq_cov) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noisemodel_store: ctx is NULL");
  NM_ORDER("dmm_noisemodel_store", nfreq);
  DMM_REQUIRE(nm_shape_ok(npol, nfreq, new_, nra), "dmm_noisemodel_store: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  NM_CHUNK("dmm_noisemodel_store");
  DMM_REQUIRE(G && weight && status && freq_cov, "dmm_noisemodel_store: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int ntile = (nfreq + kNmT - 1) / kNmT;
  hipLaunchKernelGGL(k_nm_store, dim3((unsigned)(ntile * ntile), (unsigned)nsample), dim3(256), 0, ctx->stream, nfreq, new_, nra, first, G, weight, status, freq_cov);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_noisemodel_weight(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int nstack, const float* weight, const double* noise_factor, const int32_t* cell, const double* nbaseline,
                          float* vis_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noisemodel_weight: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && new_ >= 1 && nra >= 1 && nfreq >= 1 && nfreq <= 65535, "dmm_noisemodel_weight: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(nstack >= 1 && nstack <= 65535, "dmm_noisemodel_weight: bad stack count %d", nstack);
  DMM_REQUIRE(weight && noise_factor && cell && nbaseline && vis_weight, "dmm_noisemodel_weight: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_nm_weight, dim3((unsigned)((nra + 255) / 256), (unsigned)nstack, (unsigned)nfreq), dim3(256), 0, ctx->stream, nfreq, nstack, new_, nra, weight, noise_factor, cell,
                     nbaseline, vis_weight);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_noise_colour(dmm_ctx* ctx, int npol, int nfreq, int new_, int nns, int nra, int pol, int ew, const double* chol, const void* z, const float* weight, const int32_t* redundancy,
                     const double* inv_sqrt_red, void* vis, float* vis_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noise_colour: ctx is NULL");
  NM_ORDER("dmm_noise_colour", nfreq);
  DMM_REQUIRE(nm_shape_ok(npol, nfreq, new_, nra), "dmm_noise_colour: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(nns >= 1 && nns <= 32767, "dmm_noise_colour: bad ns count %d", nns);
  DMM_REQUIRE(pol >= 0 && pol < npol && ew >= 0 && ew < new_, "dmm_noise_colour: slab (%d, %d) outside %d x %d", pol, ew, npol, new_);
  DMM_REQUIRE(chol && z && weight && redundancy && inv_sqrt_red && vis && vis_weight, "dmm_noise_colour: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((nra + kNcR - 1) / kNcR), (unsigned)((nfreq + kNcF - 1) / kNcF), (unsigned)((2 * nns + kNcC - 1) / kNcC));
  hipLaunchKernelGGL(k_nc_colour, grid, dim3(256), 0, ctx->stream, nfreq, new_, nns, nra, pol, ew, chol, (const float*)z, inv_sqrt_red, (float2*)vis);
  DMM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_nc_vw, dim3((unsigned)((nra + 255) / 256), (unsigned)nns, (unsigned)nfreq), dim3(256), 0, ctx->stream, nfreq, new_, nns, nra, pol, ew, weight, redundancy, vis_weight);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_noise_hermitian(dmm_ctx* ctx, int npol, int nfreq, int new_, int nns, int nra, const int32_t* pconj, void* vis) {
  DMM_REQUIRE(ctx != nullptr, "dmm_noise_hermitian: ctx is NULL");
  NM_ORDER("dmm_noise_hermitian", nfreq);
  DMM_REQUIRE(nm_shape_ok(npol, nfreq, new_, nra) && (int64_t)npol * nfreq <= 65535, "dmm_noise_hermitian: bad shape %d x %d x %d x %d", npol, nfreq, new_, nra);
  DMM_REQUIRE(nns >= 1 && nns <= 32767 && (nns & 1), "dmm_noise_hermitian: the ns axis must have an odd length, got %d", nns);
  DMM_REQUIRE(pconj && vis, "dmm_noise_hermitian: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_nc_herm, dim3((unsigned)((nra + 255) / 256), (unsigned)(nns / 2 + 1), (unsigned)(npol * nfreq)), dim3(256), 0, ctx->stream, nfreq, new_, nns, nra, pconj,
                     (float2*)vis);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
