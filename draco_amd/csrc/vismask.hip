// The stages of the transient RFI mask from visibilities (draco/analysis/flagging.py:1042-1277, RFIVisMask and
// RFITransientVisMask) that csrc/rfi.hip does not already hold: the Stokes-I sum over products
// (draco/analysis/transform.py:1382-1448), the weighted FIR filter along time (draco/util/filters.py:22-96), the
// transform across the baseline axis with the modulus, the hysteresis threshold and the count over beams.  DESIGN.md
// section 7t.
//
// k_stokes_sum: one thread per (freq, baseline, time); the products of a baseline (a CSR table) are added in ascending
// row order in the stream's own precision, from a zero: the reference's `+=` on a zeroed array, bit for bit.
// k_wconv: a block takes one row and a tile of kConvTile outputs.  The taps and the tile with its halo of ntap - 1
// samples (d w and w, float64, one array per component) are staged in LDS; every output then sums its ntap products in
// ascending tap order in float64 and is rounded once, at the store.  ww == 0 gives a low-pass of exactly 0.
// k_beam_abs: a transform down the columns of x [plane][stack][time].  A block takes a run of RB adjacent times (RB
// from the row-FFT planner: what fits the LDS), so that every global access is a run of RB contiguous samples, and runs
// one RowFft<double> per column in LDS -- radix passes for powers of two, Bluestein otherwise, the passes of fft_lds.h
// as the second pass of dmm_uv_fft2 uses them.  The modulus is taken at the store.
// k_hyst_*: the hysteresis threshold as a fixed point.  A state byte per sample (0: not above low, 1: above low, 2:
// set), seeded with x > high; a sweep carries "set" along every row in both directions (a wave per row, 64 samples at
// a time as two ballot masks and a bit fill) and then along every column in both directions (a thread per column).
// The fixed point is unique, so the order of the sweeps does not show in the result.  The host repeats the sweep until
// one changes nothing.
// k_beam_count: count[f][t] += #{b : flag[f][b][t] != 0}, a thread per (f, t).
// Nothing here uses a floating-point atomic: two runs give the same bits.
#include "dmm_internal.h"
#include "fft_lds.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

using dmm_fft::C;
using dmm_fft::cmul;
using dmm_fft::RowFft;

constexpr int kWave = 64;

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// ---------------------------------------------------------------- Stokes-I sum

struct StokesArgs {
  const float2* vis;    // [nf][nprod][nt]
  const float* weight;  // [nf][nprod][nt]
  const int32_t* ptr;   // [nbase + 1]
  const int32_t* rows;  // [nrows]
  float2* vis_i;        // [nf][nbase][nt]
  float* weight_i;
  int nprod, nbase, nt, nrows;
};

__global__ __launch_bounds__(256) void k_stokes_sum(StokesArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.nt) return;
  const int b = blockIdx.y, f = blockIdx.z;
  const int p0 = max(0, min(a.ptr[b], a.nrows)), p1 = max(p0, min(a.ptr[b + 1], a.nrows));
  float vr = 0.f, vi = 0.f, w = 0.f;
  for (int p = p0; p < p1; ++p) {
    const int r = max(0, min(a.rows[p], a.nprod - 1));
    const int64_t o = ((int64_t)f * a.nprod + r) * a.nt + t;
    const float2 v = a.vis[o];
    vr = vr + v.x;
    vi = vi + v.y;
    w = w + a.weight[o];
  }
  const int64_t o = ((int64_t)f * a.nbase + b) * a.nt + t;
  a.vis_i[o] = make_float2(vr, vi);
  a.weight_i[o] = w;
}

// ---------------------------------------------------------------- weighted FIR filter along the last axis

constexpr int kConvThreads = 256;
constexpr int kConvTile = 1024;  // outputs of one block

struct ConvArgs {
  const void* data;
  const void* weight;
  const double* taps;
  void* out;
  int64_t nrow;
  int n, ntap, highpass, ntile;
};

// T: the scalar type of data and weight; CPLX: the data are complex
template <typename T, bool CPLX>
__global__ __launch_bounds__(kConvThreads) void k_wconv(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char conv_lds[];
  const int c = (a.ntap - 1) / 2, L = kConvTile + a.ntap - 1;
  double* taps = (double*)conv_lds;  // [ntap]
  double* ws = taps + a.ntap;        // [L] w
  double* dr = ws + L;               // [L] Re d w
  double* di = dr + L;               // [L] Im d w (complex data only)
  const int64_t row = blockIdx.x / a.ntile;
  const int t0 = (int)(blockIdx.x - row * a.ntile) * kConvTile;
  const T* d = (const T*)a.data + row * a.n * (CPLX ? 2 : 1);
  const T* w = (const T*)a.weight + row * a.n;
  for (int j = threadIdx.x; j < a.ntap; j += kConvThreads) taps[j] = a.taps[j];
  for (int i = threadIdx.x; i < L; i += kConvThreads) {
    const int g = t0 - c + i;  // the sample slot i holds; outside the row: zero
    double wv = 0.0, xr = 0.0, xi = 0.0;
    if (g >= 0 && g < a.n) {
      wv = (double)w[g];
      if (CPLX) {
        xr = (double)d[2 * g] * wv;
        xi = (double)d[2 * g + 1] * wv;
      } else {
        xr = (double)d[g] * wv;
      }
    }
    ws[i] = wv;
    dr[i] = xr;
    if (CPLX) di[i] = xi;
  }
  __syncthreads();
  double* out = (double*)a.out + row * a.n * (CPLX ? 2 : 1);
  for (int k = threadIdx.x; k < kConvTile; k += kConvThreads) {
    const int t = t0 + k;
    if (t >= a.n) break;
    // output t, tap j reads sample t + c - j: slot k + 2 c - j
    double vr = 0.0, vi = 0.0, ww = 0.0;
    for (int j = 0; j < a.ntap; ++j) {
      const double h = taps[j];
      const int i = k + 2 * c - j;
      vr = vr + h * dr[i];
      if (CPLX) vi = vi + h * di[i];
      ww = ww + h * ws[i];
    }
    const double inv = ww == 0.0 ? 0.0 : 1.0 / ww;  // invert_no_zero, then a product
    double lr = vr * inv, li = vi * inv;
    if (a.highpass) {
      lr = (double)d[CPLX ? 2 * t : t] - lr;
      if (CPLX) li = (double)d[2 * t + 1] - li;
    }
    if (CPLX) {
      out[2 * t] = lr;
      out[2 * t + 1] = li;
    } else {
      out[t] = lr;
    }
  }
}

// ---------------------------------------------------------------- transform across the baseline axis, modulus

constexpr int kFftThreads = 1024;
// the sizing of dmm_uv_fft2: up to 16 columns per block in 150 KB of LDS, one column of 8192 points reads its twiddles
// from memory
constexpr dmm_fft_sizing kSizeBeam = {16, 150 * 1024, 160 * 1024, true, true};

struct BeamArgs {
  RowFft<double> fft;
  const double2* x;  // [nplane][nstack][nt]
  double* out;       // [nplane][nstack][nt]
  int nt, nrun;      // runs of RB columns per plane
};

template <bool BLUE>
__global__ __launch_bounds__(kFftThreads) void k_beam_abs(BeamArgs a) {
  extern __shared__ __align__(16) unsigned char beam_lds[];
  C<double>* buf = reinterpret_cast<C<double>*>(beam_lds);
  const RowFft<double>& q = a.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int plane = blockIdx.x / a.nrun, t0 = (blockIdx.x - plane * a.nrun) * RB;
  const C<double>* tw = dmm_fft::stage_twiddles<double, kFftThreads, true>(q, buf + (size_t)RB * P);
  const int64_t base = (int64_t)plane * N * a.nt + t0;
  for (int idx = threadIdx.x; idx < RB * M; idx += kFftThreads) {
    const int r = idx % RB, k = idx / RB;  // consecutive threads on consecutive times
    C<double> v = {0.0, 0.0};
    if (k < N && t0 + r < a.nt) {
      const double2 s = a.x[base + (int64_t)k * a.nt + r];
      v = {s.x, s.y};
      if (BLUE) {
        const double2 ch = q.chirp[k];
        v = cmul<double>(v, {ch.x, ch.y});
      }
    }
    buf[r * P + k] = v;
  }
  __syncthreads();
  if (BLUE) dmm_fft::bluestein_convolve<double, kFftThreads>(buf, tw, q.bfilt, RB, M, q.logM, P, true);
  else dmm_fft::fft_dif8<double, kFftThreads>(buf, tw, RB, M, q.logM, P);
  for (int idx = threadIdx.x; idx < RB * N; idx += kFftThreads) {
    const int r = idx % RB, k = idx / RB;
    if (t0 + r >= a.nt) continue;
    const C<double> v = dmm_fft::spectrum_at<double>(buf + r * P, q.chirp, BLUE, k, q.logM);
    a.out[base + (int64_t)k * a.nt + r] = hypot(v.x, v.y);
  }
}

// ---------------------------------------------------------------- hysteresis threshold

enum : uint8_t { kOff = 0, kLow = 1, kSet = 2 };

__global__ __launch_bounds__(256) void k_hyst_init(const double* x, double low, double high, int64_t n, uint8_t* state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];  // a NaN fails both comparisons
  state[i] = v > high ? kSet : (v > low ? kLow : kOff);
}

// "set" carried through the runs of `low` bits that hold a `set` bit, in both directions within the 64-bit word (the
// occluded fill of bitboards: six doubling steps each way).  set is a subset of low.
__device__ inline uint64_t fill_runs(uint64_t set, uint64_t low) {
  uint64_t g = set, p = low;
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    g |= p & (g << sh);
    p &= p << sh;
  }
  p = low;
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    g |= p & (g >> sh);
    p &= p >> sh;
  }
  return g;
}

// One 64-sample word of a line: the wave's lanes hold its state bytes, two ballots make the masks, fill_runs carries "set"
// within the word, `carry` brings it in from the word before (at bit `edge`).  Returns the filled mask.
__device__ inline uint64_t hyst_word(uint8_t* line, int i0, int nt, int lane, bool carry, int edge, int& any) {
  const int i = i0 + lane;
  const uint8_t s = i < nt ? line[i] : (uint8_t)kOff;
  const uint64_t low = __ballot(s != kOff);
  uint64_t set = __ballot(s == kSet);
  if (carry) set |= low & (1ull << edge);
  const uint64_t f = fill_runs(set, low);
  if (s == kLow && ((f >> lane) & 1)) {
    line[i] = kSet;
    any = 1;
  }
  return f;
}

// Along the rows (nline = nplane nf lines of nt bytes): a wave per line walks it in words of 64 samples, forward and
// then backward (the fill inside a word runs both ways, so the backward pass only carries across words).
constexpr int kHystRowWaves = 4;
__global__ __launch_bounds__(kHystRowWaves * kWave) void k_hyst_rows(uint8_t* state, int64_t nline, int nt, int32_t* changed) {
  const int lane = threadIdx.x % kWave;
  const int64_t l = (int64_t)blockIdx.x * kHystRowWaves + threadIdx.x / kWave;
  if (l >= nline) return;  // uniform per wave
  uint8_t* line = state + l * nt;
  int any = 0;
  bool carry = false;
  for (int i0 = 0; i0 < nt; i0 += kWave) carry = (hyst_word(line, i0, nt, lane, carry, 0, any) >> 63) & 1;
  carry = false;
  for (int i0 = ((nt - 1) / kWave) * kWave; i0 >= 0; i0 -= kWave) carry = hyst_word(line, i0, nt, lane, carry, 63, any) & 1;
  if (any) *changed = 1;  // every writer stores the same value
}

// Along the columns of every plane, down then up: a thread per (plane, time), adjacent lanes on adjacent bytes.  The
// bytes of kHystColRun rows are loaded before the first of them is looked at, so that the loads are in flight together.
constexpr int kHystColRun = 16;
__global__ __launch_bounds__(256) void k_hyst_cols(uint8_t* state, int nf, int nt, int32_t* changed) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  uint8_t* col = state + (int64_t)blockIdx.y * nf * nt + t;
  int any = 0;
  bool carry = false;
  for (int f0 = 0; f0 < nf; f0 += kHystColRun) {
    uint8_t s[kHystColRun];
#pragma unroll
    for (int k = 0; k < kHystColRun; ++k) s[k] = f0 + k < nf ? col[(int64_t)(f0 + k) * nt] : (uint8_t)kOff;
#pragma unroll
    for (int k = 0; k < kHystColRun; ++k) {
      if (s[k] == kLow && carry) {
        s[k] = kSet;
        col[(int64_t)(f0 + k) * nt] = kSet;  // (s[k] is kOff beyond the plane: never reached there)
        any = 1;
      }
      carry = s[k] == kSet;
    }
  }
  carry = false;
  for (int f1 = nf - 1; f1 >= 0; f1 -= kHystColRun) {
    uint8_t s[kHystColRun];
#pragma unroll
    for (int k = 0; k < kHystColRun; ++k) s[k] = f1 - k >= 0 ? col[(int64_t)(f1 - k) * nt] : (uint8_t)kOff;
#pragma unroll
    for (int k = 0; k < kHystColRun; ++k) {
      if (s[k] == kLow && carry) {
        s[k] = kSet;
        col[(int64_t)(f1 - k) * nt] = kSet;
        any = 1;
      }
      carry = s[k] == kSet;
    }
  }
  if (any) *changed = 1;
}

__global__ __launch_bounds__(256) void k_hyst_store(const uint8_t* state, int64_t n, int accumulate, uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t r = state[i] == kSet;
  out[i] = accumulate ? (uint8_t)((out[i] != 0) || r) : r;
}

// ---------------------------------------------------------------- count over beams

__global__ __launch_bounds__(256) void k_beam_count(const uint8_t* flag, int nb, int nt, int32_t* count) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (t >= nt) return;
  const uint8_t* p = flag + (int64_t)f * nb * nt + t;
  int c = 0;
  for (int b = 0; b < nb; ++b) c += p[(int64_t)b * nt] != 0;
  count[(int64_t)f * nt + t] += c;
}

template <typename T, bool CPLX>
int launch_wconv(dmm_ctx* ctx, const ConvArgs& a, size_t lds) {
  return dmm_launch_blocks("dmm_wconv_filter", k_wconv<T, CPLX>, a.nrow * a.ntile, kConvThreads, lds, ctx->stream, a);
}

}  // namespace

extern "C" {

int dmm_stokes_i_sum(dmm_ctx* ctx, const void* vis, const float* weight, int nf, int nprod, int nt, const int32_t* ptr, const int32_t* rows, int nbase, int nrows,
                     void* vis_i, float* weight_i) {
  DMM_REQUIRE(ctx != nullptr, "dmm_stokes_i_sum: ctx is NULL");
  DMM_REQUIRE(nf >= 1 && nprod >= 1 && nt >= 1 && nbase >= 1 && nrows >= 0, "dmm_stokes_i_sum: bad sizes nf=%d nprod=%d nt=%d nbase=%d nrows=%d", nf, nprod, nt, nbase,
              nrows);
  DMM_REQUIRE(nf <= 65535 && nbase <= 65535, "dmm_stokes_i_sum: nf %d or nbase %d does not fit the grid (65535)", nf, nbase);
  DMM_REQUIRE(vis && weight && ptr && vis_i && weight_i && (nrows == 0 || rows), "dmm_stokes_i_sum: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  StokesArgs a{(const float2*)vis, weight, ptr, rows, (float2*)vis_i, weight_i, nprod, nbase, nt, nrows};
  hipLaunchKernelGGL(k_stokes_sum, dim3(blocks256(nt), (unsigned)nbase, (unsigned)nf), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_wconv_filter(dmm_ctx* ctx, int dtype, const void* data, const void* weight, int64_t nrow, int n, const double* taps, int ntap, int highpass, void* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_wconv_filter: ctx is NULL");
  DMM_REQUIRE(dtype == DMM_REDUCE_C64 || dtype == DMM_REDUCE_C128 || dtype == DMM_REDUCE_F64, "dmm_wconv_filter: bad data type %d", dtype);
  DMM_REQUIRE(nrow >= 1 && n >= 1, "dmm_wconv_filter: bad sizes nrow=%lld n=%d", (long long)nrow, n);
  DMM_REQUIRE(ntap >= 1 && (ntap & 1), "dmm_wconv_filter: the number of taps must be odd and positive, got %d", ntap);
  DMM_REQUIRE(ntap <= DMM_WCONV_MAX_TAPS, "dmm_wconv_filter: %d taps beyond the supported bound of %d", ntap, DMM_WCONV_MAX_TAPS);
  DMM_REQUIRE(data && weight && taps && out, "dmm_wconv_filter: NULL argument");
  DMM_REQUIRE(data != out, "dmm_wconv_filter: the output may not be the input");
  DMM_HIP(hipSetDevice(ctx->device));
  ConvArgs a{data, weight, taps, out, nrow, n, ntap, highpass ? 1 : 0, (n + kConvTile - 1) / kConvTile};
  const bool cplx = dtype != DMM_REDUCE_F64;
  const size_t lds = ((size_t)ntap + (size_t)(kConvTile + ntap - 1) * (cplx ? 3 : 2)) * sizeof(double);
  if (dtype == DMM_REDUCE_C64) return launch_wconv<float, true>(ctx, a, lds);
  if (dtype == DMM_REDUCE_C128) return launch_wconv<double, true>(ctx, a, lds);
  return launch_wconv<double, false>(ctx, a, lds);
}

int dmm_beam_abs_fft_supported(int n) { return dmm_uv_fft2_supported(n); }

int dmm_beam_abs_fft(dmm_ctx* ctx, const void* x, int nplane, int nstack, int nt, double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_beam_abs_fft: ctx is NULL");
  DMM_REQUIRE(nplane >= 1 && nstack >= 1 && nt >= 1, "dmm_beam_abs_fft: bad sizes nplane=%d nstack=%d nt=%d", nplane, nstack, nt);
  DMM_REQUIRE(x && out, "dmm_beam_abs_fft: NULL argument");
  DMM_REQUIRE(x != (const void*)out, "dmm_beam_abs_fft: the output may not be the input");
  if (!dmm_beam_abs_fft_supported(nstack))
    return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_beam_abs_fft: the stack axis of length %d does not fit the in-LDS transform", nstack);
  DMM_HIP(hipSetDevice(ctx->device));
  BeamArgs a{};
  size_t lds = 0;
  bool fits = false;
  const int rc = dmm_row_fft_plan<double>(ctx, nstack, (int64_t)nplane * nt, kSizeBeam, &a.fft, &lds, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_beam_abs_fft: nstack=%d needs %zu B of LDS", nstack, lds);
  a.x = (const double2*)x;
  a.out = out;
  a.nt = nt;
  a.nrun = (nt + a.fft.RB - 1) / a.fft.RB;
  return dmm_launch_blocks("dmm_beam_abs_fft", a.fft.chirp ? k_beam_abs<true> : k_beam_abs<false>, (int64_t)nplane * a.nrun, kFftThreads, lds, ctx->stream, a);
}

int dmm_rfi_hysteresis(dmm_ctx* ctx, const double* x, int nplane, int nf, int nt, double low, double high, int accumulate, uint8_t* state, int32_t* changed, uint8_t* out,
                       int32_t* sweeps) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_hysteresis: ctx is NULL");
  DMM_REQUIRE(nplane >= 1 && nf >= 1 && nt >= 1 && nplane <= 65535, "dmm_rfi_hysteresis: bad sizes nplane=%d nf=%d nt=%d", nplane, nf, nt);
  DMM_REQUIRE(low == low && high == high, "dmm_rfi_hysteresis: a threshold is NaN");
  DMM_REQUIRE(x && state && changed && out, "dmm_rfi_hysteresis: NULL argument");
  DMM_REQUIRE(state != out, "dmm_rfi_hysteresis: the scratch may not be the output");
  const int64_t nline = (int64_t)nplane * nf, n = nline * nt;
  DMM_REQUIRE((nline + kHystRowWaves - 1) / kHystRowWaves <= 0x7fffffff && (n + 255) / 256 <= 0x7fffffff, "dmm_rfi_hysteresis: too many samples");
  if (low > high) low = high;
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_hyst_init, dim3(blocks256(n)), dim3(256), 0, ctx->stream, x, low, high, n, state);
  DMM_HIP(hipGetLastError());
  int done = 0, pass = 0;
  while (!done && pass < DMM_RFI_HYST_MAX_SWEEPS) {
    ++pass;
    int32_t any = 0;
    DMM_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_hyst_rows, dim3((unsigned)((nline + kHystRowWaves - 1) / kHystRowWaves)), dim3(kHystRowWaves * kWave), 0, ctx->stream, state, nline, nt, changed);
    hipLaunchKernelGGL(k_hyst_cols, dim3(blocks256(nt), (unsigned)nplane), dim3(256), 0, ctx->stream, state, nf, nt, changed);
    DMM_HIP(hipGetLastError());
    DMM_HIP(hipMemcpyAsync(&any, changed, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    DMM_HIP(hipStreamSynchronize(ctx->stream));
    done = any == 0;
  }
  if (sweeps) *sweeps = pass;
  if (!done) return dmm_set_error(DMM_E_STATE, "dmm_rfi_hysteresis: no fixed point after %d sweeps: the mask is not finished", DMM_RFI_HYST_MAX_SWEEPS);
  hipLaunchKernelGGL(k_hyst_store, dim3(blocks256(n)), dim3(256), 0, ctx->stream, state, n, accumulate ? 1 : 0, out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_beam_count(dmm_ctx* ctx, const uint8_t* flag, int nf, int nb, int nt, int32_t* count) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_beam_count: ctx is NULL");
  DMM_REQUIRE(nf >= 1 && nb >= 1 && nt >= 1 && nf <= 65535, "dmm_rfi_beam_count: bad sizes nf=%d nb=%d nt=%d", nf, nb, nt);
  DMM_REQUIRE(flag && count, "dmm_rfi_beam_count: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_beam_count, dim3(blocks256(nt), (unsigned)nf), dim3(256), 0, ctx->stream, flag, nb, nt, count);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
