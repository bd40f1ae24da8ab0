// Stored per-sample delay filters applied to hybrid beam-formed visibilities (draco/analysis/dayenu.py:575-773) and the
// HyFoReS bandpass estimate (draco/analysis/hyforesbandpass.py).
//
// filter / freq_cov [pol, freq, freq_sum, ew, ra] f64, vis / post [pol, freq, ew, el, ra] c64, weight [pol, freq, ew, ra]
// f32, pix [pol, freq, el, ra] bytes: ra is innermost, so lanes run along ra as in dayenu_hybrid.hip and every wave load
// is one contiguous line.  Every sum is float64 in an order that depends on the shapes alone; there are no
// floating-point atomics.
//
//   k_hf_scan     one pass over F per (pol, ew, ra) sample: is any entry non-zero, is a column non-zero where the data's
//                 weight is not positive (two bits, OR-ed per sample with an integer atomic), and the tentative
//                 weight' [f] = inz(sum_k F[f, k]^2 var[k]).  A wave keeps four rows f per pass, so a variance is
//                 fetched once for four entries of F.
//   k_hf_finish   status per sample from the bits and the weights; weight' of a sample that is not filtered is put
//                 back (skipped) or zeroed; the attenuation flag is applied.
//   k_hf_apply    out[f, l] = sum_k F[f, k] d[k] vis[k, l] per lane: a register tile of 4 rows f x 4 columns el in
//                 float64; a block's four waves take adjacent row tiles and so share the lines of vis.
//   k_hf_cov      C[f, f'] = sum_k (F[f, k] F[f', k]) var[k]: 4 x 4 tiles of the lower triangle, stored to both
//                 triangles; the product of the two entries commutes, so the diagonal tiles are symmetric bit for bit.
//   k_hf_gain     yN[f] = sum_{l, t} conj(g) s, D[f] = sum_{l, t} |g|^2, g = (vis - post) m, s = post m: one block
//                 per (pol, freq, ew), a fixed tree over its threads.
//   k_hf_window   per (pol, ew), a 4 x 4 tile of (f, f') on or below the diagonal and 64 adjacent RA: the Gram entries
//                 over el per lane, formed once per pair (they are Hermitian), times F[f, f', t] and F[f', f, t], a
//                 butterfly over the lanes; k_hf_window_sum adds the runs of 64 RA in order.
#include "dmm_internal.h"

#include <algorithm>

namespace {

constexpr int kHfMaxOrder = 1024;
constexpr int kHfR = 4;  // rows (and columns) of a register tile
constexpr int kHfE = 4;  // el columns of an apply tile
constexpr int kHfRun = DMM_HYFORES_RUN;
static_assert(kHfRun == 64, "a run of the window sum is one wave of RA");

__device__ __forceinline__ float hf_inz(float x) { return x != 0.0f ? 1.0f / x : 0.0f; }
__device__ __forceinline__ double hf_inz(double x) { return x != 0.0 ? 1.0 / x : 0.0; }

// var[k] = inz(weight[k]) |1 - g[k]|^2, inz in float32
__device__ __forceinline__ double hf_var(float w, const double* __restrict__ gp, int k) {
  double var = (double)hf_inz(w);
  if (gp) {
    const double dr = 1.0 - gp[2 * k], di = -gp[2 * k + 1];
    var *= dr * dr + di * di;
  }
  return var;
}

// grid (ceil(nra / 64), npol * new, z): wave q of block z takes the row tiles r = 4 z + q, stride 4 gridDim.z.
__global__ __launch_bounds__(256) void k_hf_scan(int n, int new_, int nra, const double* __restrict__ F, const float* __restrict__ weight, const double* __restrict__ gain,
                                                  float* __restrict__ wout, unsigned* __restrict__ bits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  if (t >= nra) return;
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra, at = (size_t)x * nra + t;
  const double* __restrict__ Fp = F + (size_t)p * n * n * plane + at;
  const float* __restrict__ wp = weight + (size_t)p * n * plane + at;
  const double* __restrict__ gp = gain ? gain + ((size_t)p * new_ + x) * n * 2 : nullptr;
  const int ntile = (n + kHfR - 1) / kHfR;
  unsigned nz = 0, miss = 0;
  for (int r = (int)blockIdx.z * 4 + wave; r < ntile; r += 4 * (int)gridDim.z) {
    const int f0 = r * kHfR;
    const double* row[kHfR];
    double s[kHfR];
#pragma unroll
    for (int i = 0; i < kHfR; ++i) {
      row[i] = Fp + (size_t)min(f0 + i, n - 1) * n * plane;
      s[i] = 0.0;
    }
    for (int k = 0; k < n; ++k) {
      const float w = wp[(size_t)k * plane];
      const bool pos = w > 0.0f;
      const double var = hf_var(w, gp, k);
#pragma unroll
      for (int i = 0; i < kHfR; ++i) {
        const double v = row[i][(size_t)k * plane];
        const bool on = v != 0.0 && f0 + i < n;
        nz |= on ? 1u : 0u;
        miss |= (on && !pos) ? 1u : 0u;
        s[i] = fma(v * v, var, s[i]);
      }
    }
    if (wout) {
#pragma unroll
      for (int i = 0; i < kHfR; ++i)
        if (f0 + i < n) wout[((size_t)p * n + f0 + i) * plane + at] = (float)hf_inz(s[i]);
    }
  }
  if (nz | miss) atomicOr(&bits[(size_t)blockIdx.y * nra + t], nz | (miss << 1));
}

// grid (ceil(nra / 256), npol * new)
__global__ __launch_bounds__(256) void k_hf_finish(int n, int new_, int nra, const float* __restrict__ weight, const unsigned* __restrict__ bits, const uint8_t* __restrict__ atten,
                                                    float* __restrict__ wout, uint8_t* __restrict__ status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nra) return;
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra, at = (size_t)x * nra + t;
  const size_t base = (size_t)p * n * plane + at;
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || weight[base + (size_t)k * plane] > 0.0f;
  const unsigned b = bits[(size_t)blockIdx.y * nra + t];
  const int st = !any ? DMM_HFA_SKIPPED : !(b & 1u) ? DMM_HFA_ZERO_FILTER : (b & 2u) ? DMM_HFA_MISSING_FREQ : DMM_HFA_OK;
  status[(size_t)blockIdx.y * nra + t] = (uint8_t)st;
  if (!wout) return;
  for (int f = 0; f < n; ++f) {
    const size_t i = base + (size_t)f * plane;
    float v;
    if (st == DMM_HFA_OK) v = atten ? wout[i] * (float)atten[i] : wout[i];
    else v = st == DMM_HFA_SKIPPED ? weight[i] : 0.0f;
    wout[i] = v;
  }
}

// grid (ceil(nra / 64), npol * new, ntile16 * nelt): wave q takes the rows f0 = 16 (z % ntile16) + 4 q and the el columns
// l0 = 4 (z / ntile16).
__global__ __launch_bounds__(256) void k_hf_apply(int n, int new_, int nel, int nra, int ntile16, const double* __restrict__ F, const float2* __restrict__ vis,
                                                   const double* __restrict__ gain, const uint8_t* __restrict__ atten, int atten_vis, int keep_input,
                                                   const uint8_t* __restrict__ status, float2* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const int f0 = ((int)blockIdx.z % ntile16) * 16 + wave * kHfR, l0 = ((int)blockIdx.z / ntile16) * kHfE;
  if (t >= nra || f0 >= n) return;
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra, at = (size_t)x * nra + t;
  const bool ok = status[(size_t)blockIdx.y * nra + t] == DMM_HFA_OK;
  double ar[kHfR][kHfE], ai[kHfR][kHfE];
#pragma unroll
  for (int i = 0; i < kHfR; ++i)
#pragma unroll
    for (int j = 0; j < kHfE; ++j) ar[i][j] = ai[i][j] = 0.0;
  const size_t vstep = (size_t)new_ * nel * nra;  // one channel of vis
  const size_t vat = ((size_t)p * n * new_ + x) * nel * nra + t;
  if (__any(ok)) {
    const double* __restrict__ gp = gain ? gain + ((size_t)p * new_ + x) * n * 2 : nullptr;
    const double* row[kHfR];
#pragma unroll
    for (int i = 0; i < kHfR; ++i) row[i] = F + ((size_t)p * n + min(f0 + i, n - 1)) * n * plane + at;
    for (int k = 0; k < n; ++k) {
      double vr[kHfE], vi[kHfE];
#pragma unroll
      for (int j = 0; j < kHfE; ++j) {
        const float2 v = l0 + j < nel ? vis[vat + (size_t)k * vstep + (size_t)(l0 + j) * nra] : make_float2(0.0f, 0.0f);
        vr[j] = (double)v.x;
        vi[j] = (double)v.y;
      }
      if (gp) {
        const double dr = 1.0 - gp[2 * k], di = -gp[2 * k + 1];
#pragma unroll
        for (int j = 0; j < kHfE; ++j) {
          const double re = vr[j] * dr - vi[j] * di, im = vr[j] * di + vi[j] * dr;
          vr[j] = re;
          vi[j] = im;
        }
      }
#pragma unroll
      for (int i = 0; i < kHfR; ++i) {
        const double fv = row[i][(size_t)k * plane];
#pragma unroll
        for (int j = 0; j < kHfE; ++j) {
          ar[i][j] = fma(fv, vr[j], ar[i][j]);
          ai[i][j] = fma(fv, vi[j], ai[i][j]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kHfR; ++i) {
    const int f = f0 + i;
    if (f >= n) continue;
    double a = 1.0;
    if (atten && atten_vis) a = (double)atten[((size_t)p * n + f) * plane + at];
#pragma unroll
    for (int j = 0; j < kHfE; ++j) {
      const int l = l0 + j;
      if (l >= nel) continue;
      const size_t o = vat + (size_t)f * vstep + (size_t)l * nra;
      float2 v;
      if (ok) v = make_float2((float)(ar[i][j] * a), (float)(ai[i][j] * a));
      else v = keep_input ? vis[o] : make_float2(0.0f, 0.0f);
      out[o] = v;
    }
  }
}

// grid (ceil(nra / 64), npol * new, ceil(npair / 4)): wave q of block z takes pair 4 z + q of the 4 x 4 tiles (a >= b).
__global__ __launch_bounds__(256) void k_hf_cov(int n, int new_, int nra, int npair, const double* __restrict__ F, const float* __restrict__ weight, const double* __restrict__ gain,
                                                 const uint8_t* __restrict__ status, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const int q = (int)blockIdx.z * 4 + wave;
  if (t >= nra || q >= npair) return;
  int a = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
  while (a * (a + 1) / 2 > q) --a;
  while ((a + 1) * (a + 2) / 2 <= q) ++a;
  const int b = q - a * (a + 1) / 2;
  const int fa = a * kHfR, fb = b * kHfR;
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra, at = (size_t)x * nra + t;
  const bool ok = status[(size_t)blockIdx.y * nra + t] == DMM_HFA_OK;
  double acc[kHfR][kHfR];
#pragma unroll
  for (int i = 0; i < kHfR; ++i)
#pragma unroll
    for (int j = 0; j < kHfR; ++j) acc[i][j] = 0.0;
  const double* __restrict__ Fp = F + (size_t)p * n * n * plane + at;
  if (__any(ok)) {
    const float* __restrict__ wp = weight + (size_t)p * n * plane + at;
    const double* __restrict__ gp = gain ? gain + ((size_t)p * new_ + x) * n * 2 : nullptr;
    const double *ra_[kHfR], *rb_[kHfR];
#pragma unroll
    for (int i = 0; i < kHfR; ++i) {
      ra_[i] = Fp + (size_t)min(fa + i, n - 1) * n * plane;
      rb_[i] = Fp + (size_t)min(fb + i, n - 1) * n * plane;
    }
    for (int k = 0; k < n; ++k) {
      const double var = hf_var(wp[(size_t)k * plane], gp, k);
      double va[kHfR], vb[kHfR];
#pragma unroll
      for (int i = 0; i < kHfR; ++i) {
        va[i] = ra_[i][(size_t)k * plane];
        vb[i] = rb_[i][(size_t)k * plane];
      }
#pragma unroll
      for (int i = 0; i < kHfR; ++i)
#pragma unroll
        for (int j = 0; j < kHfR; ++j) {
          const double ab = va[i] * vb[j];
          acc[i][j] = fma(ab, var, acc[i][j]);
        }
    }
  }
  double* __restrict__ op = out + (size_t)p * n * n * plane + at;
#pragma unroll
  for (int i = 0; i < kHfR; ++i)
#pragma unroll
    for (int j = 0; j < kHfR; ++j) {
      const int f = fa + i, g = fb + j;
      if (f >= n || g >= n) continue;
      const double v = ok ? acc[i][j] : 0.0;
      op[((size_t)f * n + g) * plane] = v;
      if (a != b) op[((size_t)g * n + f) * plane] = v;
    }
}

// m = (weight > 0) elm[l] !pix: whether a pixel enters the sums
__device__ __forceinline__ void hf_diff(const float2* __restrict__ vis, const float2* __restrict__ post, size_t i, bool on, double& gr, double& gi) {
  const float2 v = vis[i], s = post[i];  // (loaded whether or not the pixel counts: no branch around the loads)
  gr = on ? (double)v.x - (double)s.x : 0.0;
  gi = on ? (double)v.y - (double)s.y : 0.0;
}

// grid (npol * nfreq * new): block b = (p n + f) new + x
__global__ __launch_bounds__(256) void k_hf_gain(int n, int new_, int nel, int nra, const float2* __restrict__ vis, const float2* __restrict__ post, const float* __restrict__ weight,
                                                  const uint8_t* __restrict__ elm, const uint8_t* __restrict__ pix, double* __restrict__ yn, double* __restrict__ dd) {
  __shared__ double red[3][256];
  const size_t b = blockIdx.x;
  const int x = (int)(b % new_);
  const size_t pf = b / new_;
  const int f = (int)(pf % n);
  const size_t p = pf / n;
  double yr = 0.0, yi = 0.0, d = 0.0;
  for (int l = 0; l < nel; ++l) {
    if (!elm[l]) continue;
    for (int t = threadIdx.x; t < nra; t += 256) {
      if (!(weight[b * nra + t] > 0.0f)) continue;
      if (pix && pix[(pf * nel + l) * nra + t]) continue;
      const size_t i = (b * nel + l) * nra + t;
      const float2 v = vis[i], s = post[i];
      const double sr = (double)s.x, si = (double)s.y;
      const double gr = (double)v.x - sr, gi = (double)v.y - si;
      yr = fma(gr, sr, fma(gi, si, yr));
      yi = fma(gr, si, fma(-gi, sr, yi));
      d = fma(gr, gr, fma(gi, gi, d));
    }
  }
  red[0][threadIdx.x] = yr;
  red[1][threadIdx.x] = yi;
  red[2][threadIdx.x] = d;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
      for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const size_t o = (p * new_ + x) * n + f;
    yn[2 * o] = red[0][0];
    yn[2 * o + 1] = red[1][0];
    dd[o] = red[2][0];
  }
}

// grid (ceil(nra / 64), npol * new, ceil(npair / 4)): wave q of block z takes pair 4 z + q of the 4 x 4 tiles (a >= b),
// rows f = 4 a ..., columns f' = 4 b ...: the Gram tile is formed once and gives N[f][f'] = F[f][f'] G and, below the
// diagonal tiles, N[f'][f] = F[f'][f] conj(G); part [run][npol * new][n][n] complex.
__global__ __launch_bounds__(256) void k_hf_window(int n, int new_, int nel, int nra, int npair, const double* __restrict__ F, const float2* __restrict__ vis,
                                                    const float2* __restrict__ post, const float* __restrict__ weight, const uint8_t* __restrict__ elm, const uint8_t* __restrict__ pix,
                                                    double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = (int)blockIdx.z * 4 + wave;
  if (q >= npair) return;  // (the whole wave; there is no block barrier below)
  int a = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
  while (a * (a + 1) / 2 > q) --a;
  while ((a + 1) * (a + 2) / 2 <= q) ++a;
  const int b = q - a * (a + 1) / 2;
  const int fa = a * kHfR, fb = b * kHfR;
  const int t = blockIdx.x * kHfRun + lane;
  const bool in = t < nra;
  const int tc = min(t, nra - 1);
  const int p = blockIdx.y / new_, x = blockIdx.y % new_;
  const size_t plane = (size_t)new_ * nra, at = (size_t)x * nra + tc;
  int ia[kHfR], ib[kHfR];
  bool wa[kHfR], wb[kHfR];
#pragma unroll
  for (int i = 0; i < kHfR; ++i) {
    ia[i] = min(fa + i, n - 1);
    ib[i] = min(fb + i, n - 1);
    wa[i] = in && fa + i < n && weight[((size_t)p * n + ia[i]) * plane + at] > 0.0f;
    wb[i] = in && fb + i < n && weight[((size_t)p * n + ib[i]) * plane + at] > 0.0f;
  }
  double gr[kHfR][kHfR], gi[kHfR][kHfR];
#pragma unroll
  for (int i = 0; i < kHfR; ++i)
#pragma unroll
    for (int j = 0; j < kHfR; ++j) gr[i][j] = gi[i][j] = 0.0;
  // (an aliased el is carried as zeros, not skipped, and the loads of a row do not sit behind a branch: the sixteen
  // rows of an el are in flight together)
#pragma unroll 1
  for (int l = 0; l < nel; ++l) {
    const bool el_on = elm[l] != 0;
    double ar[kHfR], ai[kHfR], br[kHfR], bi[kHfR];
#pragma unroll
    for (int i = 0; i < kHfR; ++i) {
      const size_t ca = (size_t)p * n + ia[i], cb = (size_t)p * n + ib[i];
      const bool ona = el_on && wa[i] && !(pix && pix[(ca * nel + l) * nra + tc]);
      const bool onb = el_on && wb[i] && !(pix && pix[(cb * nel + l) * nra + tc]);
      hf_diff(vis, post, ((ca * new_ + x) * nel + l) * nra + tc, ona, ar[i], ai[i]);
      hf_diff(vis, post, ((cb * new_ + x) * nel + l) * nra + tc, onb, br[i], bi[i]);
    }
#pragma unroll
    for (int i = 0; i < kHfR; ++i)
#pragma unroll
      for (int j = 0; j < kHfR; ++j) {  // conj(a) b
        gr[i][j] = fma(ar[i], br[j], fma(ai[i], bi[j], gr[i][j]));
        gi[i][j] = fma(ar[i], bi[j], fma(-ai[i], br[j], gi[i][j]));
      }
  }
  double* __restrict__ o = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * n * n * 2;
#pragma unroll
  for (int i = 0; i < kHfR; ++i)
#pragma unroll
    for (int j = 0; j < kHfR; ++j) {
      const double fv = F[(((size_t)p * n + ia[i]) * n + ib[j]) * plane + at];
      double re = fv * gr[i][j], im = fv * gi[i][j];
      for (int h = 32; h > 0; h >>= 1) {
        re += __shfl_xor(re, h, 64);
        im += __shfl_xor(im, h, 64);
      }
      const bool store = lane == 0 && fa + i < n && fb + j < n;
      if (store) {
        const size_t e = (size_t)(fa + i) * n + fb + j;
        o[2 * e] = re;
        o[2 * e + 1] = im;
      }
      if (a == b) continue;  // (wave-uniform)
      const double ft = F[(((size_t)p * n + ib[j]) * n + ia[i]) * plane + at];
      re = ft * gr[i][j];
      im = -(ft * gi[i][j]);
      for (int h = 32; h > 0; h >>= 1) {
        re += __shfl_xor(re, h, 64);
        im += __shfl_xor(im, h, 64);
      }
      if (store) {
        const size_t e = (size_t)(fb + j) * n + fa + i;
        o[2 * e] = re;
        o[2 * e + 1] = im;
      }
    }
}

// out[e] = sum over the runs, in order; e over npol * new * n * n complex entries
__global__ __launch_bounds__(256) void k_hf_window_sum(size_t count, int nrun, const double* __restrict__ part, double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double re = 0.0, im = 0.0;
  for (int r = 0; r < nrun; ++r) {
    re += part[2 * ((size_t)r * count + e)];
    im += part[2 * ((size_t)r * count + e) + 1];
  }
  out[2 * e] = re;
  out[2 * e + 1] = im;
}

bool hf_shape_ok(int npol, int nfreq, int new_, int nel, int nra) {
  return npol >= 1 && new_ >= 1 && (int64_t)npol * new_ <= 65535 && nfreq >= 1 && nfreq <= kHfMaxOrder && nel >= 1 && nel <= 65535 && nra >= 1;
}

}  // namespace

extern "C" {

int dmm_hybrid_filter_apply(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const double* filter, const void* vis, const float* weight, const double* gain,
                            const uint8_t* atten, int atten_vis, int keep_input, void* vis_out, float* weight_out, double* freq_cov, uint32_t* bits, uint8_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_hybrid_filter_apply: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kHfMaxOrder, "dmm_hybrid_filter_apply: order %d outside 1 ... %d", nfreq, kHfMaxOrder);
  DMM_REQUIRE(hf_shape_ok(npol, nfreq, new_, nel, nra), "dmm_hybrid_filter_apply: bad shape %d x %d x %d x %d x %d", npol, nfreq, new_, nel, nra);
  const int ntile16 = (nfreq + 15) / 16, nelt = (nel + kHfE - 1) / kHfE;
  DMM_REQUIRE((int64_t)ntile16 * nelt <= 65535, "dmm_hybrid_filter_apply: %d x %d (freq, el) tiles do not fit the grid", ntile16, nelt);
  DMM_REQUIRE(filter && vis && weight && vis_out && bits && status, "dmm_hybrid_filter_apply: NULL argument");
  DMM_REQUIRE(vis_out != vis && (const float*)weight_out != weight, "dmm_hybrid_filter_apply: works out of place");
  DMM_HIP(hipSetDevice(ctx->device));
  const unsigned px = (unsigned)(npol * new_), g64 = (unsigned)((nra + 63) / 64);
  DMM_HIP(hipMemsetAsync(bits, 0, (size_t)px * nra * sizeof(uint32_t), ctx->stream));
  const int ntile = (nfreq + kHfR - 1) / kHfR;
  // enough blocks to fill the device, each wave with at least one row tile
  const int64_t stripes = (int64_t)g64 * px;
  const unsigned gz = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ntile + 3) / 4, (2048 + stripes - 1) / stripes));
  hipLaunchKernelGGL(k_hf_scan, dim3(g64, px, gz), dim3(256), 0, ctx->stream, nfreq, new_, nra, filter, weight, gain, weight_out, bits);
  DMM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_hf_finish, dim3((unsigned)((nra + 255) / 256), px), dim3(256), 0, ctx->stream, nfreq, new_, nra, weight, bits, atten, weight_out, status);
  DMM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_hf_apply, dim3(g64, px, (unsigned)(ntile16 * nelt)), dim3(256), 0, ctx->stream, nfreq, new_, nel, nra, ntile16, filter, (const float2*)vis, gain, atten, atten_vis,
                     keep_input, status, (float2*)vis_out);
  DMM_HIP(hipGetLastError());
  if (freq_cov) {
    const int npair = ntile * (ntile + 1) / 2;
    hipLaunchKernelGGL(k_hf_cov, dim3(g64, px, (unsigned)((npair + 3) / 4)), dim3(256), 0, ctx->stream, nfreq, new_, nra, npair, filter, weight, gain, status, freq_cov);
    DMM_HIP(hipGetLastError());
  }
  return DMM_OK;
}

int dmm_hyfores_gain(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const void* vis, const void* post, const float* weight, const uint8_t* elm, const uint8_t* pix,
                     double* yn, double* d) {
  DMM_REQUIRE(ctx != nullptr, "dmm_hyfores_gain: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kHfMaxOrder, "dmm_hyfores_gain: order %d outside 1 ... %d", nfreq, kHfMaxOrder);
  DMM_REQUIRE(hf_shape_ok(npol, nfreq, new_, nel, nra), "dmm_hyfores_gain: bad shape %d x %d x %d x %d x %d", npol, nfreq, new_, nel, nra);
  DMM_REQUIRE(vis && post && weight && elm && yn && d, "dmm_hyfores_gain: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_hf_gain, dim3((unsigned)(npol * new_ * nfreq)), dim3(256), 0, ctx->stream, nfreq, new_, nel, nra, (const float2*)vis, (const float2*)post, weight, elm, pix, yn, d);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_hyfores_window(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const double* filter, const void* vis, const void* post, const float* weight,
                       const uint8_t* elm, const uint8_t* pix, double* partial, double* window) {
  DMM_REQUIRE(ctx != nullptr, "dmm_hyfores_window: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kHfMaxOrder, "dmm_hyfores_window: order %d outside 1 ... %d", nfreq, kHfMaxOrder);
  DMM_REQUIRE(hf_shape_ok(npol, nfreq, new_, nel, nra), "dmm_hyfores_window: bad shape %d x %d x %d x %d x %d", npol, nfreq, new_, nel, nra);
  DMM_REQUIRE(filter && vis && post && weight && elm && partial && window, "dmm_hyfores_window: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int ntile = (nfreq + kHfR - 1) / kHfR;  // <= 256: at most 8224 blocks in z
  const int npair = ntile * (ntile + 1) / 2;
  const int nrun = (nra + kHfRun - 1) / kHfRun;
  const unsigned px = (unsigned)(npol * new_);
  hipLaunchKernelGGL(k_hf_window, dim3((unsigned)nrun, px, (unsigned)((npair + 3) / 4)), dim3(256), 0, ctx->stream, nfreq, new_, nel, nra, npair, filter, (const float2*)vis,
                     (const float2*)post, weight, elm, pix, partial);
  DMM_HIP(hipGetLastError());
  const size_t count = (size_t)px * nfreq * nfreq;
  hipLaunchKernelGGL(k_hf_window_sum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, count, nrun, partial, window);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
