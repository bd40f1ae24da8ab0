// Sidereal rebinning, its gradient correction, and the direct (nearest / linear / cubic) interpolators.
//
// Reference: draco/analysis/sidereal.py:550-731 (SiderealRebinner), :734-831 (RebinGradientCorrection), :349-547
// (SiderealRegridderNearest / Linear / Cubic), draco/util/regrid.py:161-270 (rebin_matrix, grad_1d).
//
// k_rebin: the rebinning matrix R [nra, nt] comes in CSR form by output bin; a sample touches at most two adjacent
// bins, so for ordered time stamps the samples of a tile of 64 bins are one contiguous span of the row.  A block is
// four waves = four rows on one tile of bins: each wave stages its row's part of the span in LDS with 16-byte loads
// (lanes along time), then lane g sums bin g's entries in ascending sample order in float64 -- no atomics, nothing
// crosses lanes, every output is rounded once.  A span longer than the LDS tile is walked in chunks, the sums stay in
// the lane's registers.  k_rebin_gradient: one block per row, the reference row staged in LDS (with its two wrapped
// samples) before anything is written, so a stream may be its own reference.  k_regrid_interp: a gather of 1, 2 or 4
// taps per output sample, the tap indices and coefficients evaluated on the host.
#include "dmm_internal.h"

#include <algorithm>

namespace {

constexpr int kBins = 64;       // bins per tile = lanes of a wave
constexpr int kWaves = 4;       // rows per block
constexpr int kCap = 640;       // samples per row and LDS chunk
constexpr int kSlack = 8;       // the chunk starts at the 16-byte boundary below its first sample
constexpr int kMaxGradNra = DMM_MAX_NRA;

struct RebinArgs {
  const float2* vis;
  const float* weight;
  const int32_t* rowptr;
  const int32_t* idx;
  const double* val;
  const int32_t* tspan;  // [ntile, 2] first and one-past-last sample of each tile of bins
  const double* lsd;
  const double* ra;
  float2* out_vis;
  float* out_weight;
  void* out_nsample;
  float* out_era;
  double start;
  int64_t nrow;
  int mode, nsample_f32, fold, nt, nra, nnz;
};

__global__ __launch_bounds__(kBins* kWaves) void k_rebin(RebinArgs a) {
  __shared__ __attribute__((aligned(16))) float lw[kWaves][kCap + kSlack];
  __shared__ __attribute__((aligned(16))) float2 lv[kWaves][kCap + kSlack];
  const int wave = threadIdx.x / kBins, lane = threadIdx.x % kBins;
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
  const bool live = row < a.nrow;
  const int64_t wrow = live ? row / a.fold : 0;
  const int tile = blockIdx.y;
  const int g = tile * kBins + lane;
  const bool valid = g < a.nra;
  const int j0 = max(0, min(a.tspan[2 * tile], a.nt)), j1 = max(j0, min(a.tspan[2 * tile + 1], a.nt));
  int p = 0, pend = 0;
  if (valid) {
    p = max(0, min(a.rowptr[g], a.nnz));
    pend = max(p, min(a.rowptr[g + 1], a.nnz));
  }
  const int64_t totv = a.nrow * a.nt, totw = (a.nrow / a.fold) * a.nt;
  double sw = 0.0, svr = 0.0, svi = 0.0, sm = 0.0, sl = 0.0, sv2 = 0.0;

  for (int jc0 = j0; jc0 < j1; jc0 += kCap) {
    const int jc1 = min(jc0 + kCap, j1);
    // element offsets of the chunk in the flat arrays, rounded down to a 16-byte boundary
    const int64_t ow = wrow * a.nt + jc0, ov = row * a.nt + jc0;
    const int64_t aw = ow & ~(int64_t)3, av = ov & ~(int64_t)1;
    const int sh_w = (int)(ow - aw), sh_v = (int)(ov - av);
    __syncthreads();
    if (live) {
      const int nqw = (sh_w + (jc1 - jc0) + 3) / 4;
      for (int q = lane; q < nqw; q += kBins) {
        const int64_t e = aw + 4 * (int64_t)q;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e + 4 <= totw) {
          t = *(const float4*)(a.weight + e);
        } else {
          if (e < totw) t.x = a.weight[e];
          if (e + 1 < totw) t.y = a.weight[e + 1];
          if (e + 2 < totw) t.z = a.weight[e + 2];
        }
        *(float4*)&lw[wave][4 * q] = t;
      }
      const int nqv = (sh_v + (jc1 - jc0) + 1) / 2;
      for (int q = lane; q < nqv; q += kBins) {
        const int64_t e = av + 2 * (int64_t)q;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e + 2 <= totv) {
          t = *(const float4*)(a.vis + e);
        } else if (e < totv) {
          const float2 y = a.vis[e];
          t.x = y.x;
          t.y = y.y;
        }
        *(float4*)&lv[wave][2 * q] = t;
      }
    }
    __syncthreads();
    if (live) {
      while (p < pend) {
        const int j = a.idx[p];
        if (j >= jc1) break;
        if (j >= jc0) {
          const double r = a.val[p];
          const float wf = lw[wave][sh_w + (j - jc0)];
          const float2 y = lv[wave][sh_v + (j - jc0)];
          const double m = wf > 0.f ? 1.0 : 0.0;
          double w, v;
          if (a.mode == DMM_REBIN_UNIFORM) {
            w = m;
            v = wf != 0.f ? (double)(float)(1.0 / (double)wf) : 0.0;  // the reference's variance is a float32
          } else {
            w = v = (double)wf;
          }
          const double rw = r * w;
          sw += rw;
          svr += rw * (double)y.x;
          svi += rw * (double)y.y;
          sm += r * m;
          sl += rw * a.lsd[j];
          sv2 += r * r * v;
        }
        ++p;
      }
    }
  }
  if (!live || !valid) return;
  const double norm = sw != 0.0 ? 1.0 / sw : 0.0;
  a.out_vis[row * a.nra + g] = make_float2((float)(norm * svr), (float)(norm * svi));
  if (row % a.fold) return;  // the weight, the count and the effective RA are per weight row
  const double d = norm * norm * sv2;
  const float wout = (float)(d != 0.0 ? 1.0 / d : 0.0);
  const int64_t o = wrow * a.nra + g;
  a.out_weight[o] = wout;
  if (a.nsample_f32)
    ((float*)a.out_nsample)[o] = (float)sm;
  else
    ((uint16_t*)a.out_nsample)[o] = (uint16_t)(long long)sm;  // truncation toward zero, as an array assignment does
  const double era = 360.0 * (norm * sl - a.start);
  a.out_era[o] = wout == 0.f ? (float)a.ra[g] : (float)era;
}

struct GradArgs {
  float2* vis;
  float* weight;
  const float* era;
  const double* ra;
  const float2* ref_vis;
  const float* ref_weight;
  const float* ref_era;  // [nrow, nra] positions of the reference row, or NULL:
  const double* ref_ra;  // [nra] shared positions
  int nra;
};

__global__ __launch_bounds__(256) void k_rebin_gradient(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gl[];
  const int n = a.nra;
  double* S = (double*)gl;             // [n + 2] positions, wrapped
  float2* X = (float2*)(S + (n + 2));  // [n + 2] reference values, wrapped
  unsigned char* M = (unsigned char*)(X + (n + 2));  // [n + 2] reference sample is flagged
  const int64_t base = (int64_t)blockIdx.x * n;
  int any = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) any |= a.weight[base + i] != 0.f;
  if (!__syncthreads_or(any)) return;  // an entirely masked row is left alone
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    S[i + 1] = a.ref_era ? (double)a.ref_era[base + i] : a.ref_ra[i];
    X[i + 1] = a.ref_vis[base + i];
    M[i + 1] = a.ref_weight[base + i] == 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double shift = ceil(S[n] / 360.0) * 360.0;
    S[0] = S[n] - shift;
    S[n + 1] = S[1] + shift;
    X[0] = X[n];
    X[n + 1] = X[1];
    M[0] = M[n];
    M[n + 1] = M[1];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int k = i + 1;
    const double hd = S[k] - S[k - 1], hs = S[k + 1] - S[k];
    const double ca = -hs / (hd * (hd + hs)), cb = (hs - hd) / (hd * hs), cc = hd / (hs * (hd + hs));
    double gr = ca * (double)X[k - 1].x + cb * (double)X[k].x + cc * (double)X[k + 1].x;
    double gi = ca * (double)X[k - 1].y + cb * (double)X[k].y + cc * (double)X[k + 1].y;
    bool mask = M[k - 1] || M[k] || M[k + 1];
    mask = mask || hd == 0.0 || hs == 0.0 || !isfinite(gr) || !isfinite(gi);
    if (mask) gr = gi = 0.0;
    const float w = a.weight[base + i];
    if (w > 0.f && !mask) {
      const double dx = (double)a.era[base + i] - a.ra[i];
      float2 y = a.vis[base + i];
      y.x = (float)((double)y.x - gr * dx);
      y.y = (float)((double)y.y - gi * dx);
      a.vis[base + i] = y;
    }
    a.weight[base + i] = w * (mask ? 0.f : 1.f);
  }
}

struct InterpArgs {
  const float2* vis;
  const float* weight;
  const int32_t* tap;
  const double* coef;
  const unsigned char* bad;
  const double* omega;
  const float* mask;
  const double* dphi_in;
  const double* dphi_out;
  float2* out_vis;
  float* out_weight;
  int nt, nout;
};

template <int NTAP>
__global__ __launch_bounds__(256) void k_regrid_interp(InterpArgs a) {
  const int64_t row = blockIdx.x;
  const int o = blockIdx.y * 256 + threadIdx.x;
  if (o >= a.nout) return;
  double om = 0.0;
  float mk = 1.f;
  if (a.omega) {
    om = a.omega[row];
    mk = a.mask[row];
  }
  double xr = 0.0, xi = 0.0, var = 0.0;
  bool all = true;
  float w0 = 0.f;
#pragma unroll
  for (int k = 0; k < NTAP; ++k) {
    const int j = max(0, min(a.tap[(size_t)k * a.nout + o], a.nt - 1));
    const double c = a.coef[(size_t)k * a.nout + o];
    float2 y = a.vis[row * a.nt + j];
    const float w = a.weight[row * a.nt + j];
    if (a.omega) {  // mix down, rounded to complex64 like the reference's in-place product
      double s, cs;
      sincos(om * a.dphi_in[j], &s, &cs);
      const double pr = (double)mk * cs, pi = -(double)mk * s;
      y = make_float2((float)((double)y.x * pr - (double)y.y * pi), (float)((double)y.x * pi + (double)y.y * pr));
    }
    xr += c * (double)y.x;
    xi += c * (double)y.y;
    var += c * c * (w != 0.f ? (double)(float)(1.0 / (double)w) : 0.0);  // the reference's variance is a float32
    all = all && w > 0.f;
    w0 = w;
  }
  float wout;
  if (NTAP == 1)  // nearest: the sample itself (its coefficient is 1), weight untouched
    wout = w0;
  else
    wout = all && var != 0.0 ? (float)(1.0 / var) : 0.f;
  if (a.omega) {  // mix up: x *= conj(mask exp(-i omega dphi))
    double s, cs;
    sincos(om * a.dphi_out[o], &s, &cs);
    const double qr = (double)mk * cs, qi = (double)mk * s;
    const double vr = xr * qr - xi * qi, vi = xr * qi + xi * qr;
    xr = vr;
    xi = vi;
    if (mk == 0.f) wout = 0.f;
  }
  if (a.bad[o]) wout = 0.f;
  a.out_vis[row * a.nout + o] = make_float2((float)xr, (float)xi);
  a.out_weight[row * a.nout + o] = wout;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int dmm_rebin(dmm_ctx* ctx, int mode, int nsample_f32, const void* vis, const float* weight, int64_t nrow, int fold, int nt, int nra, const int32_t* row_ptr,
              const int32_t* sample_index, const double* value, int nnz, const int32_t* tile_span, const double* lsd, double start, const double* ra, void* out_vis,
              float* out_weight, void* out_nsample, float* out_effective_ra) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rebin: ctx is NULL");
  DMM_REQUIRE(mode == DMM_REBIN_UNIFORM || mode == DMM_REBIN_INVERSE_VARIANCE, "dmm_rebin: bad mode %d", mode);
  DMM_REQUIRE(nrow >= 0, "dmm_rebin: bad nrow %lld", (long long)nrow);
  DMM_REQUIRE(nt >= 1 && nra >= 1 && nnz >= 0, "dmm_rebin: bad sizes nt=%d nra=%d nnz=%d", nt, nra, nnz);
  DMM_REQUIRE(fold >= 1 && nrow % fold == 0, "dmm_rebin: fold %d does not divide nrow %lld", fold, (long long)nrow);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(vis && weight && row_ptr && sample_index && value && tile_span && lsd && ra && out_vis && out_weight && out_nsample && out_effective_ra, "dmm_rebin: NULL argument");
  DMM_REQUIRE(aligned16(vis) && aligned16(weight), "dmm_rebin: vis and weight must be 16-byte aligned");
  DMM_REQUIRE((nrow + kWaves - 1) / kWaves <= 0x7fffffff, "dmm_rebin: nrow %lld does not fit the grid", (long long)nrow);
  const int ntile = (nra + kBins - 1) / kBins;
  if (ntile > 65535) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_rebin: nra %d needs %d tiles of bins, the grid holds 65535", nra, ntile);
  DMM_HIP(hipSetDevice(ctx->device));
  RebinArgs a{};
  a.vis = (const float2*)vis;
  a.weight = weight;
  a.rowptr = row_ptr;
  a.idx = sample_index;
  a.val = value;
  a.tspan = tile_span;
  a.lsd = lsd;
  a.ra = ra;
  a.out_vis = (float2*)out_vis;
  a.out_weight = out_weight;
  a.out_nsample = out_nsample;
  a.out_era = out_effective_ra;
  a.start = start;
  a.nrow = nrow;
  a.mode = mode;
  a.nsample_f32 = nsample_f32 ? 1 : 0;
  a.fold = fold;
  a.nt = nt;
  a.nra = nra;
  a.nnz = nnz;
  hipLaunchKernelGGL(k_rebin, dim3((unsigned)((nrow + kWaves - 1) / kWaves), (unsigned)ntile), dim3(kBins * kWaves), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rebin_gradient(dmm_ctx* ctx, void* vis, float* weight, const float* effective_ra, const double* ra, const void* ref_vis, const float* ref_weight,
                       const float* ref_effective_ra, const double* ref_ra, int64_t nrow, int nra) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rebin_gradient: ctx is NULL");
  DMM_REQUIRE(nrow >= 0 && nrow <= 0x7fffffff, "dmm_rebin_gradient: bad nrow %lld", (long long)nrow);
  DMM_REQUIRE(nra >= 1, "dmm_rebin_gradient: bad nra %d", nra);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(vis && weight && effective_ra && ra && ref_vis && ref_weight, "dmm_rebin_gradient: NULL argument");
  DMM_REQUIRE((ref_effective_ra != nullptr) != (ref_ra != nullptr), "dmm_rebin_gradient: the reference positions are ref_effective_ra or ref_ra, one of the two");
  if (nra > kMaxGradNra) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_rebin_gradient: nra %d, a row of at most %d fits the LDS", nra, kMaxGradNra);
  DMM_HIP(hipSetDevice(ctx->device));
  GradArgs a{(float2*)vis, weight, effective_ra, ra, (const float2*)ref_vis, ref_weight, ref_effective_ra, ref_ra, nra};
  const size_t lds = (size_t)(nra + 2) * (sizeof(double) + sizeof(float2) + 1);
  DMM_HIP(hipFuncSetAttribute((const void*)k_rebin_gradient, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_rebin_gradient, dim3((unsigned)nrow), dim3(256), lds, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_regrid_interp(dmm_ctx* ctx, int ntap, const void* vis, const float* weight, int64_t nrow, int nt, int nout, const int32_t* tap, const double* coeff,
                      const uint8_t* bad, const double* omega, const float* feed_mask, const double* dphi_in, const double* dphi_out, void* out_vis, float* out_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_regrid_interp: ctx is NULL");
  DMM_REQUIRE(ntap == 1 || ntap == 2 || ntap == 4, "dmm_regrid_interp: bad mode: %d taps (1 nearest, 2 linear, 4 cubic)", ntap);
  DMM_REQUIRE(nrow >= 0 && nrow <= 0x7fffffff, "dmm_regrid_interp: bad nrow %lld", (long long)nrow);
  DMM_REQUIRE(nt >= 1 && nout >= 1, "dmm_regrid_interp: bad sizes nt=%d nout=%d", nt, nout);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(vis && weight && tap && coeff && bad && out_vis && out_weight, "dmm_regrid_interp: NULL argument");
  const bool mix = omega || feed_mask || dphi_in || dphi_out;
  DMM_REQUIRE(!mix || (omega && feed_mask && dphi_in && dphi_out), "dmm_regrid_interp: the mixing arrays come all four or not at all");
  const int ntile = (nout + 255) / 256;
  if (ntile > 65535) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_regrid_interp: nout %d does not fit the grid", nout);
  DMM_HIP(hipSetDevice(ctx->device));
  InterpArgs a{(const float2*)vis, weight, tap, coeff, bad, omega, feed_mask, dphi_in, dphi_out, (float2*)out_vis, out_weight, nt, nout};
  const dim3 grid((unsigned)nrow, (unsigned)ntile);
  if (ntap == 1)
    hipLaunchKernelGGL(k_regrid_interp<1>, grid, dim3(256), 0, ctx->stream, a);
  else if (ntap == 2)
    hipLaunchKernelGGL(k_regrid_interp<2>, grid, dim3(256), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL(k_regrid_interp<4>, grid, dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
