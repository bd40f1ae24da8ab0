// DPSS gap inpainting (draco/util/dpss.py, draco/analysis/interpolate.py): a Wiener filter of every column of a stream
// onto a real basis A [n][k] (the leading eigenvectors of a sinc covariance, built on the host), in float64.
//
// Per column, with Ni its weights, W its mask and Si the regulariser (dpss.py:359-404):
//   xhat = sum(W x) / sum(W);  xp = A^T (Ni o (x - xhat));  C = A^T diag(Ni) A + Si I = U^T U;  b = C^-1 xp;
//   xfilt = A b + xhat;  var_i = a_i^T (C^-1 - Si C^-2) a_i = a_i . y_i - Si |y_i|^2 with y_i = C^-1 a_i (a_i the rows
//   of A: the diagonal of F N F^H, F = A C^-1 A^T Ni, because Ni inz(Ni) Ni = Ni);  weight = inz(var + pchip(inz(Ni))).
// A column whose Ni is all zero skips the solve (b = 0, solved weight 0); a column whose C is not positive definite keeps
// its data and loses its weight.
//
// Columns are addressed through a layout (DpLayout): column c starts at (c / ninner) stride_outer + (c % ninner)
// stride_inner and its samples are stride_samp apart.  Along frequency the samples of a column are nstack nra elements
// apart and adjacent columns are adjacent in memory; along RA a column is contiguous.  A batch is a list of columns
// (`cols`) that share one basis; everything between pack and store works on packed float64 rows [slot][n].
//
// Stages (all batched over the slots of a batch):
//   k_dp_pack     stream -> X [nb][2][n] (real and imaginary rows, unchanged values), Ni, W, xhat, status (skipped);
//                 lanes run along the axis that is contiguous in the stream (columns or samples);
//   k_dp_gram     C = A^T diag(Ni) A + Si I on v_mfma_f64_16x16x4_f64, 64 x 64 upper tiles, four columns per block: a
//                 16-sample slice of A is staged in LDS once and scaled by each column's Ni on the way to the registers
//                 (the tile product and its epilogue map are dl_tile_mma / dl_tile_each of chol_blocked.h);
//   k_dp_apply    out[j] = sum_s M[s][j] v[s] for eight vectors (four columns, real and imaginary) per block: the
//                 projection (M = A, v = Ni o (x - xhat) formed on load) and the synthesis A b (M = A^T);
//   chol_blocked.hip   C = U^T U, the solve of the two rows of xp, and the solve of the n rows of A for the variance
//                 (dl_factor and dl_solve_rows: the one compiled copy that delay.hip and mfilter.hip call too);
//   k_dp_var      var_i = a_i . y_i - Si |y_i|^2, one wave per row;
//   k_dp_gap      the gap-width pass of flag_above_cutoff (dpss.py:307-356), one wave per column;
//   k_dp_pchip    SciPy's PchipInterpolator of inz(Ni) through the valid samples, evaluated at every sample, one wave
//                 per column over the compacted knot indices in LDS; weight = inz(var + max(pchip, 0));
//   k_dp_store    packed rows -> stream, rounded once to complex64 / float32, with the put-back and the gap flag.
//
// Index ranges (n <= 4096, k <= n, nb <= 65535): offsets inside one packed matrix stay below 2^24; every offset that
// carries a slot or a column is formed in size_t / int64_t; knot indices fit 16 bits.
#include "chol_blocked.h"

namespace {

constexpr int kDpMaxOrder = 4096;
constexpr int kDpGramCols = 4;  // columns that share one staged slice of A in k_dp_gram and k_dp_apply

struct DpLayout {
  int64_t ninner, stride_outer, stride_inner, stride_samp;
};

__device__ __forceinline__ int64_t dp_col_off(const DpLayout& L, int64_t c) { return (c / L.ninner) * L.stride_outer + (c % L.ninner) * L.stride_inner; }

// thread -> (slot, first sample, sample step): lanes along the columns (kColFast: 64 slots x 8 phases per block) or
// along the samples (8 slots x 64 phases)
template <bool kColFast>
__device__ __forceinline__ void dp_map(int* slot_local, int* phase, int* nphase) {
  if (kColFast) *slot_local = threadIdx.x & 63, *phase = threadIdx.x >> 6, *nphase = 8;
  else *slot_local = threadIdx.x >> 6, *phase = threadIdx.x & 63, *nphase = 64;
}

struct DpPack {
  int n, nb;
  DpLayout lay;
  const int64_t* cols;
  const float2* vis;
  const float* weight;
  const uint8_t* wext;  // the mask in the weights' layout, or nullptr: W = weight > 0
  double* X;
  double* Ni;
  uint8_t* W;
  double* xhat;
  int32_t* status;
};

template <bool kColFast>
__global__ __launch_bounds__(512) void k_dp_pack(DpPack a) {
  __shared__ double sr[512], si[512];
  __shared__ int sc[512], sa[512];
  int sl, phase, nphase;
  dp_map<kColFast>(&sl, &phase, &nphase);
  const int per = kColFast ? 64 : 8;
  const int64_t b = (int64_t)blockIdx.x * per + sl;
  double accr = 0.0, acci = 0.0;
  int cnt = 0, any = 0;
  if (b < a.nb) {
    const int64_t off = dp_col_off(a.lay, a.cols[b]);
    double* xr = a.X + (size_t)b * 2 * a.n;
    double* xi = xr + a.n;
    double* ni = a.Ni + (size_t)b * a.n;
    uint8_t* wo = a.W + (size_t)b * a.n;
    for (int i = phase; i < a.n; i += nphase) {
      const int64_t p = off + (int64_t)i * a.lay.stride_samp;
      const float2 z = a.vis[p];
      const float w = a.weight[p];
      const int keep = a.wext ? (a.wext[p] != 0) : (w > 0.0f);
      xr[i] = (double)z.x;
      xi[i] = (double)z.y;
      ni[i] = (double)w;
      wo[i] = (uint8_t)keep;
      if (keep) accr += (double)z.x, acci += (double)z.y, ++cnt;
      any |= w != 0.0f;
    }
  }
  sr[threadIdx.x] = accr, si[threadIdx.x] = acci, sc[threadIdx.x] = cnt, sa[threadIdx.x] = any;
  __syncthreads();
  if (phase == 0 && b < a.nb) {
    const int step = kColFast ? 64 : 1, base = kColFast ? sl : sl * 64;
    double tr = 0.0, ti = 0.0;
    int tc = 0, ta = 0;
    for (int q = 0; q < nphase; ++q) tr += sr[base + q * step], ti += si[base + q * step], tc += sc[base + q * step], ta |= sa[base + q * step];
    const double inv = tc > 0 ? 1.0 / (double)tc : 0.0;
    a.xhat[2 * b] = tr * inv;
    a.xhat[2 * b + 1] = ti * inv;
    a.status[b] = ta ? DMM_DPSS_OK : DMM_DPSS_SKIPPED;
  }
}

// C[b] = A^T diag(Ni[b]) A + eps I, upper 64 x 64 tiles; kDpGramCols columns per block share the staged slice of A.
__global__ __launch_bounds__(256) void k_dp_gram(int n, int k, int nb, const double* __restrict__ A, const double* __restrict__ Ni, double eps, double* __restrict__ C,
                                                 const int32_t* __restrict__ status) {
  constexpr int KC = kTileK, LP = kTileLP;
  __shared__ double as[64 * LP];
  __shared__ double bs[64 * LP];
  __shared__ double ns[kDpGramCols][KC];
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (m0 > n0) return;
  const int64_t b0 = (int64_t)blockIdx.z * kDpGramCols;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d acc[kDpGramCols][2][2];
#pragma unroll
  for (int c = 0; c < kDpGramCols; ++c) acc[c][0][0] = acc[c][0][1] = acc[c][1][0] = acc[c][1][1] = vz;
  for (int s0 = 0; s0 < n; s0 += KC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + 256 * i;
      const int r = e & 63, kk = e >> 6;
      const int s = s0 + kk;
      as[r * LP + kk] = (s < n && m0 + r < k) ? A[(size_t)s * k + m0 + r] : 0.0;
      bs[r * LP + kk] = (s < n && n0 + r < k) ? A[(size_t)s * k + n0 + r] : 0.0;
    }
    if (threadIdx.x < kDpGramCols * KC) {
      const int c = threadIdx.x / KC, kk = threadIdx.x % KC;
      ns[c][kk] = (b0 + c < nb && s0 + kk < n) ? Ni[(size_t)(b0 + c) * n + s0 + kk] : 0.0;
    }
    __syncthreads();
    dl_tile_mma<kDpGramCols>(as, bs, acc, [&](int c, double a, int kk) { return a * ns[c][kk]; });
  }
#pragma unroll
  for (int c = 0; c < kDpGramCols; ++c) {
    if (b0 + c >= nb || status[b0 + c]) continue;
    double* Cb = C + (size_t)(b0 + c) * k * k;
    dl_tile_each(acc[c], [&](int r, int cc, double v) {
      const int row = m0 + r, col = n0 + cc;
      if (row < k && col < k) Cb[(size_t)row * k + col] = v + (row == col ? eps : 0.0);
    });
  }
}

// out[b][part][j] = sum_s M[s][j] v[b][part][s], M [S][J] shared by the batch.  kProject: v = Ni o (x - xhat) formed
// from the packed rows on load (the mean never makes a pass of its own); otherwise v is read as it is.
template <bool kProject>
__global__ __launch_bounds__(256) void k_dp_apply(int S, int J, int nb, const double* __restrict__ M, const double* __restrict__ in, const double* __restrict__ Ni,
                                                  const double* __restrict__ xhat, double* __restrict__ out) {
  constexpr int NV = 2 * kDpGramCols, SC = 64;
  __shared__ double v[NV][SC];
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.y * kDpGramCols;
  double acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.0;
  for (int s0 = 0; s0 < S; s0 += SC) {
    __syncthreads();
    for (int e = threadIdx.x; e < NV * SC; e += 256) {
      const int q = e / SC, ss = e % SC, s = s0 + ss;
      const int64_t b = b0 + (q >> 1);
      double val = 0.0;
      if (b < nb && s < S) {
        val = in[((size_t)b * 2 + (q & 1)) * S + s];
        if (kProject) val = Ni[(size_t)b * S + s] * (val - xhat[2 * b + (q & 1)]);
      }
      v[q][ss] = val;
    }
    __syncthreads();
    if (j < J) {
      const int top = min(SC, S - s0);
      for (int ss = 0; ss < top; ++ss) {
        const double m = M[(size_t)(s0 + ss) * J + j];
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] = fma(m, v[q][ss], acc[q]);
      }
    }
  }
  if (j >= J) return;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int64_t b = b0 + (q >> 1);
    if (b < nb) out[((size_t)b * 2 + (q & 1)) * J + j] = acc[q];
  }
}

// Z[b] = A for every slot whose matrix was factored: the right-hand sides of the variance solve
__global__ __launch_bounds__(256) void k_dp_bcast(int64_t nk, const double* __restrict__ A, double* __restrict__ Z, const int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < nk) Z[(size_t)b * nk + e] = A[e];
}

// var[b][i] = a_i . y_i - eps |y_i|^2, one wave per row
__global__ __launch_bounds__(256) void k_dp_var(int n, int k, const double* __restrict__ A, const double* __restrict__ Y, double eps, double* __restrict__ var,
                                                const int32_t* __restrict__ status) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  if (status[b]) return;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (whole waves)
  const double* __restrict__ a = A + (size_t)i * k;
  const double* __restrict__ y = Y + ((size_t)b * n + i) * k;
  double s1 = 0.0, s2 = 0.0;
  for (int m = lane; m < k; m += 64) {
    const double yv = y[m];
    s1 = fma(a[m], yv, s1);
    s2 = fma(yv, yv, s2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  if (lane == 0) var[(size_t)b * n + i] = s1 - eps * s2;
}

// The indices of the non-zero bytes of valid[0 ... n) in increasing order, into knots (LDS, one wave); returns their number.
__device__ __forceinline__ int dp_compact(const uint8_t* __restrict__ valid, int n, uint16_t* knots) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int K = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int f = (i < n && valid[i]) ? 1 : 0;
    const unsigned long long mask = __ballot(f);
    if (f) knots[K + __popcll(mask & below)] = (uint16_t)i;
    K += __popcll(mask);
  }
  return K;
}

// keep[b][i] of flag_above_cutoff (dpss.py:333-356) for valid [nb][n]: a gap from ri to fi has dist = fi - ri and is
// kept where dist < fc; a gap that reaches the end has no falling edge and keeps dist = 0; everything before the first
// valid sample and from the last valid sample on has dist = 2 fc (no valid sample at all: only the last sample).
__global__ __launch_bounds__(256) void k_dp_gap(int n, int nb, const uint8_t* __restrict__ valid, double fc, uint8_t* __restrict__ keep) {
  extern __shared__ uint16_t dp_knots[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= nb) return;  // (whole waves; no block-wide barrier below)
  uint16_t* knots = dp_knots + (size_t)wave * n;
  const uint8_t* __restrict__ v = valid + (size_t)b * n;
  const int K = dp_compact(v, n, knots);
  __builtin_amdgcn_wave_barrier();
  const int lbound = K > 0 ? knots[0] : 0, rbound = K > 0 ? knots[K - 1] : n - 1;
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  int seen = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int f = (i < n && v[i]) ? 1 : 0;
    const unsigned long long mask = __ballot(f);
    const int cnt = seen + __popcll(mask & upto);  // valid samples at or before i
    seen += __popcll(mask);
    if (i >= n) continue;
    double dist = 0.0;
    if (!f && cnt < K) {
      const int ri = cnt > 0 ? knots[cnt - 1] + 1 : 0, fi = knots[cnt] - 1;
      dist = (double)(fi - ri);
    }
    if (i < lbound || i >= rbound) dist = 2.0 * fc;
    keep[(size_t)b * n + i] = dist < fc ? 1 : 0;
  }
}

struct DpKnots {
  const uint16_t* x;
  const double* ni;
  int K;
  __device__ __forceinline__ double pos(int j) const { return (double)x[j]; }
  __device__ __forceinline__ double val(int j) const {
    const double w = ni[x[j]];
    return w == 0.0 ? 0.0 : 1.0 / w;
  }
  __device__ __forceinline__ double slope(int j) const { return (val(j + 1) - val(j)) / (pos(j + 1) - pos(j)); }
};

__device__ __forceinline__ double dp_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// SciPy's PchipInterpolator._edge_case: the one-sided three-point estimate, shape preserving
__device__ __forceinline__ double dp_edge(double h0, double h1, double m0, double m1) {
  const double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
  if (dp_sign(d) != dp_sign(m0)) return 0.0;
  if (dp_sign(m0) != dp_sign(m1) && fabs(d) > 3.0 * fabs(m0)) return 3.0 * m0;
  return d;
}

// the derivative PchipInterpolator._find_derivatives assigns to knot j (K >= 2)
__device__ __forceinline__ double dp_deriv(const DpKnots& q, int j) {
  if (q.K == 2) return q.slope(0);
  if (j == 0) return dp_edge(q.pos(1) - q.pos(0), q.pos(2) - q.pos(1), q.slope(0), q.slope(1));
  if (j == q.K - 1) return dp_edge(q.pos(j) - q.pos(j - 1), q.pos(j - 1) - q.pos(j - 2), q.slope(j - 1), q.slope(j - 2));
  const double hm = q.pos(j) - q.pos(j - 1), h = q.pos(j + 1) - q.pos(j);
  const double mm = q.slope(j - 1), m = q.slope(j);
  if (dp_sign(mm) != dp_sign(m) || mm == 0.0 || m == 0.0) return 0.0;
  const double w1 = 2.0 * h + hm, w2 = h + 2.0 * hm;
  return 1.0 / ((w1 / mm + w2 / m) / (w1 + w2));
}

// wout[b][i] = inz(var + max(pchip_i, 0)): the interpolant of inz(Ni) through the samples where W is set, evaluated at
// every sample index (the end pieces extrapolate); fewer than two knots: no interpolant.  A skipped column has var = 0.
__global__ __launch_bounds__(256) void k_dp_pchip(int n, int nb, const double* __restrict__ Ni, const uint8_t* __restrict__ W, const double* __restrict__ var,
                                                  const int32_t* __restrict__ status, double* __restrict__ wout) {
  extern __shared__ uint16_t dp_knots[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= nb) return;  // (whole waves; no block-wide barrier below)
  const int st = status[b];
  double* __restrict__ wo = wout + (size_t)b * n;
  if (st == DMM_DPSS_NOT_POSDEF) {
    for (int i = lane; i < n; i += 64) wo[i] = 0.0;
    return;
  }
  uint16_t* knots = dp_knots + (size_t)wave * n;
  const uint8_t* __restrict__ w = W + (size_t)b * n;
  DpKnots q{knots, Ni + (size_t)b * n, 0};
  q.K = dp_compact(w, n, knots);
  __builtin_amdgcn_wave_barrier();
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  int seen = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int f = (i < n && w[i]) ? 1 : 0;
    const unsigned long long mask = __ballot(f);
    const int cnt = seen + __popcll(mask & upto);
    seen += __popcll(mask);
    if (i >= n) continue;
    double v = st == DMM_DPSS_OK ? var[(size_t)b * n + i] : 0.0;
    if (q.K >= 2) {
      const int j = min(max(cnt - 1, 0), q.K - 2);
      const double h = q.pos(j + 1) - q.pos(j), t = (double)i - q.pos(j);
      const double sl = q.slope(j), d0 = dp_deriv(q, j), d1 = dp_deriv(q, j + 1);
      const double tt = (d0 + d1 - 2.0 * sl) / h;
      const double c0 = tt / h, c1 = (sl - d0) / h - tt;
      double p = q.val(j) + d0 * t + c1 * (t * t) + c0 * (t * t * t);
      if (p < 0.0) p = 0.0;
      v += p;
    }
    wo[i] = v == 0.0 ? 0.0 : 1.0 / v;
  }
}

struct DpStore {
  int n, nb, inpaint;
  DpLayout lay;
  const int64_t* cols;
  const double* F;
  const double* xhat;
  const double* X;
  const double* Ni;
  const uint8_t* W;
  const double* wout;
  const uint8_t* keep;  // the gap flag, or nullptr
  const int32_t* status;
  float2* vis;
  float* weight;
};

template <bool kColFast>
__global__ __launch_bounds__(512) void k_dp_store(DpStore a) {
  int sl, phase, nphase;
  dp_map<kColFast>(&sl, &phase, &nphase);
  const int64_t b = (int64_t)blockIdx.x * (kColFast ? 64 : 8) + sl;
  if (b >= a.nb) return;
  const int64_t off = dp_col_off(a.lay, a.cols[b]);
  const bool failed = a.status[b] == DMM_DPSS_NOT_POSDEF;
  const double hr = a.xhat[2 * b], hi = a.xhat[2 * b + 1];
  const double* xr = a.X + (size_t)b * 2 * a.n;
  const double* fr = a.F + (size_t)b * 2 * a.n;
  for (int i = phase; i < a.n; i += nphase) {
    const size_t e = (size_t)b * a.n + i;
    float2 z;
    float w;
    if (failed) {
      z = make_float2((float)xr[i], (float)xr[a.n + i]);
      w = 0.0f;
    } else if (a.inpaint && a.W[e]) {
      z = make_float2((float)xr[i], (float)xr[a.n + i]);
      w = (float)a.Ni[e];
    } else {
      z = make_float2((float)(fr[i] + hr), (float)(fr[a.n + i] + hi));
      w = (float)a.wout[e];
    }
    if (a.keep && !a.keep[e]) w = 0.0f;
    const int64_t p = off + (int64_t)i * a.lay.stride_samp;
    a.vis[p] = z;
    a.weight[p] = w;
  }
}

bool dp_layout(const int64_t* layout, DpLayout* L) {
  if (!layout) return false;
  *L = DpLayout{layout[0], layout[1], layout[2], layout[3]};
  return L->ninner >= 1 && L->stride_outer >= 0 && L->stride_inner >= 0 && L->stride_samp >= 1;
}

}  // namespace

#define DP_ORDER(who, n) DMM_REQUIRE((n) >= 1 && (n) <= kDpMaxOrder, who ": order %d outside 1 ... %d", (n), kDpMaxOrder)
#define DP_MODES(who, k, n) DMM_REQUIRE((k) >= 1 && (k) <= (n), who ": mode count %d outside 1 ... %d", (k), (n))
#define DP_BATCH(who, nb) DMM_REQUIRE((nb) >= 0 && (nb) <= 65535, who ": bad column count %d", (nb))

extern "C" {

int dmm_dpss_pack(dmm_ctx* ctx, int n, int nb, const int64_t* layout, const int64_t* cols, const void* vis, const float* weight, const uint8_t* wext, double* X, double* Ni,
                  uint8_t* W, double* xhat, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_pack: ctx is NULL");
  DP_ORDER("dmm_dpss_pack", n);
  DP_BATCH("dmm_dpss_pack", nb);
  if (nb == 0) return DMM_OK;
  DpLayout L;
  DMM_REQUIRE(layout && cols && vis && weight && X && Ni && W && xhat && status, "dmm_dpss_pack: NULL argument");
  DMM_REQUIRE(dp_layout(layout, &L), "dmm_dpss_pack: bad layout");
  DMM_HIP(hipSetDevice(ctx->device));
  DpPack a{n, nb, L, cols, (const float2*)vis, weight, wext, X, Ni, W, xhat, status};
  if (L.stride_samp != 1) hipLaunchKernelGGL(k_dp_pack<true>, dim3((unsigned)((nb + 63) / 64)), dim3(512), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_dp_pack<false>, dim3((unsigned)((nb + 7) / 8)), dim3(512), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_gram(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* Ni, double eps, double* C, const int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_gram: ctx is NULL");
  DP_ORDER("dmm_dpss_gram", n);
  DP_MODES("dmm_dpss_gram", k, n);
  DP_BATCH("dmm_dpss_gram", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(A && Ni && C && status, "dmm_dpss_gram: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const unsigned nt = (unsigned)((k + 63) / 64);
  hipLaunchKernelGGL(k_dp_gram, dim3(nt, nt, (unsigned)((nb + kDpGramCols - 1) / kDpGramCols)), dim3(256), 0, ctx->stream, n, k, nb, A, Ni, eps, C, status);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_project(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* X, const double* Ni, const double* xhat, double* B) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_project: ctx is NULL");
  DP_ORDER("dmm_dpss_project", n);
  DP_MODES("dmm_dpss_project", k, n);
  DP_BATCH("dmm_dpss_project", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(A && X && Ni && xhat && B, "dmm_dpss_project: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dp_apply<true>, dim3((unsigned)((k + 255) / 256), (unsigned)((nb + kDpGramCols - 1) / kDpGramCols)), dim3(256), 0, ctx->stream, n, k, nb, A, X, Ni, xhat, B);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_solve(dmm_ctx* ctx, int k, int nb, double* C, double* B, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_solve: ctx is NULL");
  DP_ORDER("dmm_dpss_solve", k);
  DP_BATCH("dmm_dpss_solve", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(C && B && status, "dmm_dpss_solve: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  dl_factor(ctx, k, nb, C, status, DMM_DPSS_NOT_POSDEF);
  dl_solve_rows(ctx, k, 2, 2, nb, C, B, status);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_variance(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* C, double eps, double* Z, double* var, const int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_variance: ctx is NULL");
  DP_ORDER("dmm_dpss_variance", n);
  DP_MODES("dmm_dpss_variance", k, n);
  DP_BATCH("dmm_dpss_variance", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(A && C && Z && var && status, "dmm_dpss_variance: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t nk = (int64_t)n * k;
  hipLaunchKernelGGL(k_dp_bcast, dim3((unsigned)((nk + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, nk, A, Z, status);
  dl_solve_rows(ctx, k, n, n, nb, C, Z, status);
  hipLaunchKernelGGL(k_dp_var, dim3((unsigned)((n + 3) / 4), (unsigned)nb), dim3(256), 0, ctx->stream, n, k, A, (const double*)Z, eps, var, status);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_synth(dmm_ctx* ctx, int n, int k, int nb, const double* At, const double* B, double* F) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_synth: ctx is NULL");
  DP_ORDER("dmm_dpss_synth", n);
  DP_MODES("dmm_dpss_synth", k, n);
  DP_BATCH("dmm_dpss_synth", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(At && B && F, "dmm_dpss_synth: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dp_apply<false>, dim3((unsigned)((n + 255) / 256), (unsigned)((nb + kDpGramCols - 1) / kDpGramCols)), dim3(256), 0, ctx->stream, k, n, nb, At, B, (const double*)nullptr,
                     (const double*)nullptr, F);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_gapflag(dmm_ctx* ctx, int n, int nb, const uint8_t* valid, double fc, uint8_t* keep) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_gapflag: ctx is NULL");
  DP_ORDER("dmm_dpss_gapflag", n);
  DMM_REQUIRE(nb >= 0, "dmm_dpss_gapflag: bad column count %d", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(valid && keep, "dmm_dpss_gapflag: NULL argument");
  DMM_REQUIRE(fc == fc, "dmm_dpss_gapflag: the cutoff is NaN");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dp_gap, dim3((unsigned)((nb + 3) / 4)), dim3(256), sizeof(uint16_t) * 4 * n, ctx->stream, n, nb, valid, fc, keep);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_pchip(dmm_ctx* ctx, int n, int nb, const double* Ni, const uint8_t* W, const double* var, const int32_t* status, double* wout) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_pchip: ctx is NULL");
  DP_ORDER("dmm_dpss_pchip", n);
  DMM_REQUIRE(nb >= 0, "dmm_dpss_pchip: bad column count %d", nb);
  if (nb == 0) return DMM_OK;
  DMM_REQUIRE(Ni && W && var && status && wout, "dmm_dpss_pchip: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dp_pchip, dim3((unsigned)((nb + 3) / 4)), dim3(256), sizeof(uint16_t) * 4 * n, ctx->stream, n, nb, Ni, W, var, status, wout);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_dpss_store(dmm_ctx* ctx, int n, int nb, const int64_t* layout, const int64_t* cols, const double* F, const double* xhat, const double* X, const double* Ni,
                   const uint8_t* W, const double* wout, const uint8_t* keep, const int32_t* status, int inpaint, void* vis, float* weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_dpss_store: ctx is NULL");
  DP_ORDER("dmm_dpss_store", n);
  DP_BATCH("dmm_dpss_store", nb);
  if (nb == 0) return DMM_OK;
  DpLayout L;
  DMM_REQUIRE(layout && cols && F && xhat && X && Ni && W && wout && status && vis && weight, "dmm_dpss_store: NULL argument");
  DMM_REQUIRE(dp_layout(layout, &L), "dmm_dpss_store: bad layout");
  DMM_HIP(hipSetDevice(ctx->device));
  DpStore a{n, nb, inpaint ? 1 : 0, L, cols, F, xhat, X, Ni, W, wout, keep, status, (float2*)vis, weight};
  if (L.stride_samp != 1) hipLaunchKernelGGL(k_dp_store<true>, dim3((unsigned)((nb + 63) / 64)), dim3(512), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_dp_store<false>, dim3((unsigned)((nb + 7) / 8)), dim3(512), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
