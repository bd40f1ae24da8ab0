// Delay null-space filter along the frequency axis (draco/util/filters.py:133-212, draco/analysis/delay.py:29-339).
//
// Per distinct (cutoff, num_modes K, mask) the reference takes the SVD of the masked, windowed Fourier matrix
// F [n, K] = exp(2 pi i f_k s), f = linspace(-cutoff, cutoff, K), keeps the left singular vectors U with sig > tol sig_max
// and returns NF = (I - U U^H) o (1 x mask) o (1 x w) ("high") or (U U^H) o ... ("low").  The modes are symmetric about
// zero, so F F^H is real: the real matrix Fr with the columns sqrt2 cos(2 pi f_k s), sqrt2 sin(2 pi f_k s) for f_k > 0
// (and a column of ones for an odd K) has Fr Fr^T = F F^H, hence the same singular values, the same kept subspace and a
// real filter.  The cut sits at 1e-16 in the eigenvalues of the Gram matrix, the float64 rounding floor: the
// factorisation has to be an SVD of Fr itself, here a one-sided (Hestenes) Jacobi.
//
// Build, batched over matrices (order n <= 1024; every matrix has its own 2 <= K <= 1024 and the pitch of the largest;
// all float64):
//   k_nf_basis   Fr [mat][K][n]: a column of Fr is contiguous.  The phase f s is reduced exactly before sincospi;
//   k_nf_jacobi  one block per matrix, in place.  A sweep is K - 1 (K even) or K steps of a round-robin tournament;
//                a step rotates floor(K / 2) disjoint column pairs, one wave per pair at a time, and ends in the one
//                block barrier.  A wave holds both columns in registers (n / 64 elements per lane each), reduces the
//                three dot products across its lanes, forms the rotation in every lane and stores the pair.  The
//                matrix lives in global memory (L2); LDS holds the squared column norms.  A pair is left alone when
//                |a_i . a_j| <= n eps |a_i| |a_j| (sqrt(n) eps is what the float64 dot product itself is good for: the
//                sweeps would never end), or when either norm is below 1e-13 of the largest one, five decades under
//                the cut.  Such a column is rounding noise that lies in the span of the others (all of it, when
//                there are more modes than unmasked channels): every rotation against a large column would shrink
//                it by another factor eps and keep the sweeps going, while leaving it as it is moves a kept singular
//                vector by (1e-13 / 1e-8)^2 at the most.  Exchanging a pair so that the larger column stays in the
//                lower index (de Rijk's pivoting, which needs the serial row-cyclic order to pay) costs sweeps in
//                the tournament order, 30 instead of 19 at n = 256, K = 40, and is left out.  The columns of Fr have
//                equal norms and a spectrum that falls from a plateau to 1e-16: the sweeps peel it off slowly (13
//                sweeps at n = 64, K = 20; 18 ... 22 and 24 ... 28 at n = 1024, K = 160 and 400), so the cap is 60; a matrix that
//                reaches it sets status[mat].  The sweeps end with the first one that rotates nothing.  Then sig = the column norms
//                (recomputed), nkeep = #(sig > tol sig_max), and the columns are scaled by 1 / sig where kept and by
//                0 elsewhere, so the order the columns end in does not matter;
//   k_nf_proj    NF = (I - U U^T) o (1 x mask) o (1 x w) or (U U^T) o ..., 64 x 64 tiles on v_mfma_f64_16x16x4_f64 (the
//                tile product of chol_blocked.h).  Mask and window scale the columns only, as in the reference.
// Mask pass (k_nf_count*, k_nf_masks, k_nf_weight): per item f_samp[f] = #t(w > 0), f_mask = (f_samp == max f_samp),
// t_mask likewise along the other axis, weight *= f_mask x t_mask.  An item without any weight keeps both masks full.
// The reference's item of a ring map is one el with the (pol, ra) samples of both polarisations: the (pol, el) columns
// of one el are then joined (their counts per frequency add up, the maxima are taken over all of them).
// The data side, vis <- NF vis, is dmm_dayenu_apply of dayenu.hip.
#include "chol_blocked.h"

#include <cfloat>

namespace {

constexpr int kNfMaxOrder = 1024, kNfMaxModes = 1024, kNfSweepCap = 60;
constexpr int kNfRows = kNfMaxOrder / 64;  // elements of a column per lane
constexpr double kNfFloor = 1e-13;         // columns below this fraction of the largest norm are noise

// K of one matrix: its own entry of kmodes, or the pitch Kp where there is no table; 0 (nothing to do) if out of range
__device__ __forceinline__ int nf_modes_of(const int32_t* kmodes, int mat, int Kp) {
  const int K = kmodes ? kmodes[mat] : Kp;
  return (K >= 2 && K <= Kp) ? K : 0;
}

__global__ void k_nf_basis(int n, int Kp, const int32_t* __restrict__ kmodes, const double* __restrict__ samples, const double* __restrict__ modes, const uint8_t* __restrict__ mask, const double* __restrict__ window,
                           double* __restrict__ Fall) {
  const int mat = blockIdx.y;
  const int K = nf_modes_of(kmodes, mat, Kp);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)K * n) return;
  const int k = (int)(idx / n), r = (int)(idx % n);
  const int P = K / 2;
  double v;
  if (k >= 2 * P) {
    v = 1.0;  // the zero mode of an odd K
  } else {
    const double f = modes[(size_t)mat * Kp + (K - P) + (k >> 1)];
    // the phase f s in turns: the product exactly (head and fma tail), less its nearest integer (exact), so that the
    // argument carries one rounding; 2 pi f s in float64 would be off by 1e-13 at 10^3 radians, and eps sig_max / sig_cut
    // turns that into 1e-8 in the filter (the reference's own error)
    const double sr = samples[r];
    const double ph = f * sr, tail = fma(f, sr, -ph);
    double sn, cs;
    sincospi(2.0 * ((ph - rint(ph)) + tail), &sn, &cs);
    v = M_SQRT2 * ((k & 1) ? sn : cs);
  }
  if (!mask[(size_t)mat * n + r]) v = 0.0;
  if (window) v *= window[r];
  Fall[(size_t)mat * Kp * n + idx] = v;
}

__device__ __forceinline__ double nf_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;  // (the same bits in every lane)
}

// squared norm of one column by one wave
__device__ __forceinline__ double nf_col_norm2(const double* col, int n, int lane) {
  double s = 0.0;
  for (int r = lane; r < n; r += 64) s = fma(col[r], col[r], s);
  return nf_wave_sum(s);
}

__global__ __launch_bounds__(1024) void k_nf_jacobi(int n, int Kp, const int32_t* __restrict__ kmodes, double tol, double* Fall, double* __restrict__ sig, int32_t* __restrict__ nkeep, int32_t* __restrict__ status,
                                                    int32_t* __restrict__ sweeps) {
  __shared__ double s_nrm[kNfMaxModes];  // squared column norms
  __shared__ double s_red[16];
  __shared__ double s_cut;
  __shared__ int s_any;
  const int mat = blockIdx.x;
  const int K = nf_modes_of(kmodes, mat, Kp);
  double* F = Fall + (size_t)mat * Kp * n;
  for (int k = K + (int)threadIdx.x; k < Kp; k += blockDim.x) sig[(size_t)mat * Kp + k] = 0.0;
  if (K == 0) {  // (the whole block leaves)
    if (threadIdx.x == 0) {
      nkeep[mat] = 0;
      status[mat] = 2;
      if (sweeps) sweeps[mat] = 0;
    }
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  for (int k = wave; k < K; k += nwave) {
    const double s = nf_col_norm2(F + (size_t)k * n, n, lane);
    if (lane == 0) s_nrm[k] = s;
  }
  __syncthreads();

  const int M = (K + 1) & ~1;  // players of the tournament: an odd K gets a bye
  const double otol = (double)n * DBL_EPSILON;
  int sweep = 0;
  bool clean = false;
  while (sweep < kNfSweepCap && !clean) {
    double m = 0.0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) m = fmax(m, s_nrm[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if (lane == 0) s_red[wave] = m;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    m = 0.0;
    for (int w = 0; w < nwave; ++w) m = fmax(m, s_red[w]);
    const double floor2 = kNfFloor * kNfFloor * m;
    for (int step = 0; step < M - 1; ++step) {
      int moved = 0;
      for (int q = wave; q < M / 2; q += nwave) {
        const int a = q == 0 ? M - 1 : (step + q) % (M - 1);
        const int b = q == 0 ? step : (step + (M - 1) - q) % (M - 1);
        if (a >= K || b >= K) continue;  // the bye
        const int i = min(a, b), j = max(a, b);
        if (s_nrm[i] < floor2 || s_nrm[j] < floor2) continue;  // (a stale norm only errs towards taking the pair)
        double* ci = F + (size_t)i * n;
        double* cj = F + (size_t)j * n;
        double x[kNfRows], y[kNfRows];
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int t = 0; t < kNfRows; ++t) {
          const int r = lane + 64 * t;
          x[t] = r < n ? ci[r] : 0.0;
          y[t] = r < n ? cj[r] : 0.0;
          alpha = fma(x[t], x[t], alpha);
          beta = fma(y[t], y[t], beta);
          gamma = fma(x[t], y[t], gamma);
        }
        alpha = nf_wave_sum(alpha);
        beta = nf_wave_sum(beta);
        gamma = nf_wave_sum(gamma);
        double na = alpha, nb = beta;
        if (fabs(gamma) > otol * sqrt(alpha * beta) && alpha >= floor2 && beta >= floor2) {
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
          // the new norms from the rotated columns themselves: alpha - t gamma cancels to rounding noise for a column
          // that falls by more than eight decades, and a norm that reads zero would leave it frozen under the floor
          double pa = 0.0, pb = 0.0;
#pragma unroll
          for (int t2 = 0; t2 < kNfRows; ++t2) {
            const int r = lane + 64 * t2;
            const double xn = c * x[t2] - s * y[t2], yn = s * x[t2] + c * y[t2];
            pa = fma(xn, xn, pa);
            pb = fma(yn, yn, pb);
            if (r < n) {
              ci[r] = xn;
              cj[r] = yn;
            }
          }
          na = nf_wave_sum(pa);
          nb = nf_wave_sum(pb);
          moved = 1;
        }
        if (lane == 0) {
          s_nrm[i] = na;
          s_nrm[j] = nb;
        }
      }
      if (moved && lane == 0) s_any = 1;
      __syncthreads();  // (also makes the rotated columns visible to the waves that take them next)
    }
    ++sweep;
    clean = s_any == 0;
    __syncthreads();
  }

  // ---- singular values from the columns as they stand, the cut, the scaling
  for (int k = wave; k < K; k += nwave) {
    const double s = nf_col_norm2(F + (size_t)k * n, n, lane);
    if (lane == 0) s_nrm[k] = sqrt(s);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double smax = 0.0;
    for (int k = 0; k < K; ++k) smax = fmax(smax, s_nrm[k]);
    int cnt = 0;
    for (int k = 0; k < K; ++k) cnt += s_nrm[k] > tol * smax ? 1 : 0;
    s_cut = tol * smax;
    nkeep[mat] = cnt;
    status[mat] = clean ? 0 : 1;
    if (sweeps) sweeps[mat] = sweep;
  }
  __syncthreads();
  const double cut = s_cut;
  for (int k = threadIdx.x; k < K; k += blockDim.x) sig[(size_t)mat * Kp + k] = s_nrm[k];
  for (int k = wave; k < K; k += nwave) {
    const double sk = s_nrm[k];
    const double inv = sk > cut ? 1.0 / sk : 0.0;
    double* col = F + (size_t)k * n;
    for (int r = lane; r < n; r += 64) col[r] = inv != 0.0 ? col[r] * inv : 0.0;
  }
}

// One 64 x 64 tile of NF per block: P(I, J) = sum_k U[k][I] U[k][J] over the scaled columns (the dropped ones are zero).
__global__ __launch_bounds__(256) void k_nf_proj(int n, int Kp, const int32_t* __restrict__ kmodes, int low, const double* __restrict__ Uall, const uint8_t* __restrict__ mask, const double* __restrict__ window,
                                                 double* __restrict__ NFall) {
  constexpr int KC = kTileK, LP = kTileLP;
  __shared__ double xs[64 * LP];
  __shared__ double ys[64 * LP];
  const int mat = blockIdx.y;
  const int nt = (n + 63) / 64;
  const int I0 = (blockIdx.x / nt) * 64, J0 = (blockIdx.x % nt) * 64;
  const int K = nf_modes_of(kmodes, mat, Kp);
  const double* __restrict__ U = Uall + (size_t)mat * Kp * n;
  double* NF = NFall + (size_t)mat * n * n;
  const uint8_t* mk = mask + (size_t)mat * n;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d acc[2][2] = {{vz, vz}, {vz, vz}};
  const int r = threadIdx.x & 63, kq = threadIdx.x >> 6;
  for (int k0 = 0; k0 < K; k0 += KC) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < KC / 4; ++c) {
      const int kk = kq + 4 * c, k = k0 + kk;
      xs[r * LP + kk] = (I0 + r < n && k < K) ? U[(size_t)k * n + I0 + r] : 0.0;
      ys[r * LP + kk] = (J0 + r < n && k < K) ? U[(size_t)k * n + J0 + r] : 0.0;
    }
    __syncthreads();
    dl_tile_mma(xs, ys, acc);
  }
  dl_tile_each(acc, [&](int tr, int tc, double p) {
    const int row = I0 + tr, col = J0 + tc;
    if (row < n && col < n) {
      double v = low ? p : (row == col ? 1.0 : 0.0) - p;
      if (!mk[col]) v = 0.0;
      if (window) v *= window[col];
      NF[(size_t)row * n + col] = v;
    }
  });
}

// ---- the mask pass
struct NfSide {
  void* p;
  int64_t ncol, sf, sc, si, so;
};

// out[(o ninner + in) nx + x] = #r(w[o so + in si + x sx + r sr] > 0), one thread per count; the inner items or x run
// along the threads, whichever is contiguous in memory.
template <typename T>
__global__ __launch_bounds__(256) void k_nf_count(const T* __restrict__ p, int64_t so, int64_t si, int64_t sx, int64_t sr, int ninner, int64_t nx, int64_t nr, int inner_fast,
                                                  int64_t total, int32_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  int64_t o, in, x;
  if (inner_fast) {
    in = e % ninner;
    x = (e / ninner) % nx;
    o = e / (ninner * nx);
  } else {
    x = e % nx;
    in = (e / nx) % ninner;
    o = e / (ninner * nx);
  }
  const T* q = p + o * so + in * si + x * sx;
  int cnt = 0;
  for (int64_t r = 0; r < nr; ++r) cnt += q[r * sr] > (T)0 ? 1 : 0;
  out[(o * ninner + in) * nx + x] = cnt;
}

// the same count by one block per (item, frequency) where the columns are contiguous
template <typename T>
__global__ __launch_bounds__(256) void k_nf_count_row(NfSide w, int n, int ninner, int32_t* __restrict__ out) {
  const int in = blockIdx.x, f = blockIdx.y, o = blockIdx.z;
  const T* q = (const T*)w.p + o * w.so + in * w.si + f * w.sf;
  int cnt = 0;
  for (int64_t c = threadIdx.x; c < w.ncol; c += blockDim.x) cnt += q[c * w.sc] > (T)0 ? 1 : 0;
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  if (cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (threadIdx.x == 0) out[((size_t)o * ninner + in) * n + f] = s_cnt;
}

// per item: flag[f] = (fs[f] == max fs), ts[c] <- (ts[c] == max ts).  With nj > 1 the nj items (o, in), o < nj, are one
// item whose samples are the columns of all of them: the counts per frequency add up, the maxima are joint.
__global__ __launch_bounds__(256) void k_nf_masks(int n, int64_t ncol, int ninner, int nj, const int32_t* __restrict__ fs, int32_t* __restrict__ ts, uint8_t* __restrict__ flag) {
  __shared__ int s_max[2];
  const size_t first = blockIdx.x;  // the item, or item (0, in) of a joint item
  if (threadIdx.x < 2) s_max[threadIdx.x] = 0;
  __syncthreads();
  int mf = 0, mt = 0;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    int tot = 0;
    for (int o = 0; o < nj; ++o) tot += fs[(first + (size_t)o * ninner) * n + k];
    mf = max(mf, tot);
  }
  for (int o = 0; o < nj; ++o) {
    const int32_t* t = ts + (first + (size_t)o * ninner) * ncol;
    for (int64_t c = threadIdx.x; c < ncol; c += blockDim.x) mt = max(mt, t[c]);
  }
  atomicMax(&s_max[0], mf);
  atomicMax(&s_max[1], mt);
  __syncthreads();
  mf = s_max[0];
  mt = s_max[1];
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    int tot = 0;
    for (int o = 0; o < nj; ++o) tot += fs[(first + (size_t)o * ninner) * n + k];
    for (int o = 0; o < nj; ++o) flag[(first + (size_t)o * ninner) * n + k] = tot == mf ? 1 : 0;
  }
  for (int o = 0; o < nj; ++o) {
    int32_t* t = ts + (first + (size_t)o * ninner) * ncol;
    for (int64_t c = threadIdx.x; c < ncol; c += blockDim.x) t[c] = t[c] == mt ? 1 : 0;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_nf_weight(NfSide w, int n, int ninner, int inner_fast, int64_t total, const uint8_t* __restrict__ flag, const int32_t* __restrict__ tflag) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  int64_t in, c, rest;
  if (inner_fast) {
    in = e % ninner;
    c = (e / ninner) % w.ncol;
  } else {
    c = e % w.ncol;
    in = (e / w.ncol) % ninner;
  }
  rest = e / (ninner * w.ncol);
  const int64_t f = rest % n, o = rest / n;
  const int64_t item = o * ninner + in;
  if (flag[item * n + f] && tflag[item * w.ncol + c]) return;  // (w * 1 is w)
  T* q = (T*)w.p + o * w.so + in * w.si + f * w.sf + c * w.sc;
  *q = *q * (T)0;
}

template <typename T>
void nf_mask_launch(dmm_ctx* ctx, int layout, int n, int ninner, int nouter, int join, const NfSide& w, int32_t* fs, int32_t* ts, uint8_t* flag) {
  const int64_t nitem = (int64_t)ninner * nouter;
  const int items = layout == DMM_DAYENU_ITEMS;
  const int64_t tot_f = nitem * n, tot_t = nitem * w.ncol, tot_w = nitem * n * w.ncol;
  if (items) {
    hipLaunchKernelGGL(k_nf_count<T>, dim3((unsigned)((tot_f + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)w.p, w.so, w.si, w.sf, w.sc, ninner, (int64_t)n, w.ncol, 1, tot_f, fs);
  } else {
    hipLaunchKernelGGL(k_nf_count_row<T>, dim3((unsigned)ninner, (unsigned)n, (unsigned)nouter), dim3(256), 0, ctx->stream, w, n, ninner, fs);
  }
  hipLaunchKernelGGL(k_nf_count<T>, dim3((unsigned)((tot_t + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)w.p, w.so, w.si, w.sc, w.sf, ninner, w.ncol, (int64_t)n, items, tot_t, ts);
  hipLaunchKernelGGL(k_nf_masks, dim3((unsigned)(join ? ninner : nitem)), dim3(256), 0, ctx->stream, n, w.ncol, ninner, join ? nouter : 1, (const int32_t*)fs, ts, flag);
  hipLaunchKernelGGL(k_nf_weight<T>, dim3((unsigned)((tot_w + 255) / 256)), dim3(256), 0, ctx->stream, w, n, ninner, items, tot_w, (const uint8_t*)flag, (const int32_t*)ts);
}

}  // namespace

extern "C" {

int dmm_nullfilter_build(dmm_ctx* ctx, int nfreq, int nmat, int num_modes, const int32_t* nmodes, int low, double tol, const double* samples, const double* modes, const uint8_t* mask, const double* window,
                         double* nf, double* sig, int32_t* nkeep, int32_t* status, int32_t* sweeps) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nullfilter_build: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kNfMaxOrder, "dmm_nullfilter_build: order %d outside 1 ... %d", nfreq, kNfMaxOrder);
  DMM_REQUIRE(num_modes >= 2 && num_modes <= kNfMaxModes, "dmm_nullfilter_build: num_modes %d outside 2 ... %d", num_modes, kNfMaxModes);
  DMM_REQUIRE(nmat >= 0 && nmat <= 65535, "dmm_nullfilter_build: bad matrix count %d", nmat);
  DMM_REQUIRE(low == 0 || low == 1, "dmm_nullfilter_build: bad filter type %d", low);
  DMM_REQUIRE(tol >= 0.0 && tol < 1.0, "dmm_nullfilter_build: tol %g outside [0, 1)", tol);
  if (nmat == 0) return DMM_OK;
  DMM_REQUIRE(samples && modes && mask && nf && sig && nkeep && status, "dmm_nullfilter_build: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int n = nfreq, K = num_modes;
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)nmat * K * n * sizeof(double), &scratch);
  if (rc) return rc;
  double* basis = (double*)scratch;
  hipLaunchKernelGGL(k_nf_basis, dim3((unsigned)(((int64_t)K * n + 255) / 256), (unsigned)nmat), dim3(256), 0, ctx->stream, n, K, nmodes, samples, modes, mask, window, basis);
  hipLaunchKernelGGL(k_nf_jacobi, dim3((unsigned)nmat), dim3(1024), 0, ctx->stream, n, K, nmodes, tol, basis, sig, nkeep, status, sweeps);
  const int nt = (n + 63) / 64;
  hipLaunchKernelGGL(k_nf_proj, dim3((unsigned)(nt * nt), (unsigned)nmat), dim3(256), 0, ctx->stream, n, K, nmodes, low, (const double*)basis, mask, window, nf);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_nullfilter_mask(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, int join_outer, const dmm_dayenu_side* weight, uint8_t* flag) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nullfilter_mask: ctx is NULL");
  DMM_REQUIRE(dtype == DMM_DAYENU_F32 || dtype == DMM_DAYENU_F64, "dmm_nullfilter_mask: bad dtype %d", dtype);
  DMM_REQUIRE(layout == DMM_DAYENU_COLS || layout == DMM_DAYENU_ITEMS, "dmm_nullfilter_mask: bad layout %d", layout);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kNfMaxOrder, "dmm_nullfilter_mask: order %d outside 1 ... %d", nfreq, kNfMaxOrder);
  DMM_REQUIRE(ninner >= 0 && nouter >= 0 && nouter <= 65535, "dmm_nullfilter_mask: bad item counts %d x %d", nouter, ninner);
  DMM_REQUIRE(join_outer == 0 || join_outer == 1, "dmm_nullfilter_mask: bad join_outer %d", join_outer);
  DMM_REQUIRE(weight && weight->ptr && flag, "dmm_nullfilter_mask: NULL argument");
  DMM_REQUIRE(weight->ncol >= 0 && weight->stride_freq >= 0 && weight->stride_col >= 0 && weight->stride_inner >= 0 && weight->stride_outer >= 0,
              "dmm_nullfilter_mask: negative count or stride");
  if (ninner == 0 || nouter == 0) return DMM_OK;
  const int64_t nitem = (int64_t)ninner * nouter;
  const int64_t ncol = weight->ncol;
  DMM_REQUIRE(nitem <= 0x7fffffff && (double)nitem * nfreq * (double)(ncol > 0 ? ncol : 1) < 256.0 * 2147483647.0, "dmm_nullfilter_mask: %lld items of %lld columns do not fit the grid",
              (long long)nitem, (long long)ncol);
  DMM_HIP(hipSetDevice(ctx->device));
  if (ncol == 0) {  // no sample at all: every count is zero, which is the maximum
    DMM_HIP(hipMemsetAsync(flag, 1, (size_t)nitem * nfreq, ctx->stream));
    return DMM_OK;
  }
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)nitem * ((size_t)nfreq + (size_t)ncol) * sizeof(int32_t), &scratch);
  if (rc) return rc;
  int32_t* fs = (int32_t*)scratch;
  int32_t* ts = fs + (size_t)nitem * nfreq;
  const NfSide w{weight->ptr, ncol, weight->stride_freq, weight->stride_col, weight->stride_inner, weight->stride_outer};
  if (dtype == DMM_DAYENU_F32) nf_mask_launch<float>(ctx, layout, nfreq, ninner, nouter, join_outer, w, fs, ts, flag);
  else nf_mask_launch<double>(ctx, layout, nfreq, ninner, nouter, join_outer, w, fs, ts, flag);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
