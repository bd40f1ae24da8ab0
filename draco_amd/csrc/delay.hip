// Delay spectrum estimators along the frequency axis (draco/analysis/delay.py:347-1106, 1480-1710, 2102-2201).
//
// Per baseline (a stack entry of a stream, a (beam, pol, el) column of a ring map), with d [sample, freq] and the
// weights averaged over the retained samples:
//   y = F^T diag(c) d,   G = F^T diag(c) F + diag(Si),   G x = y          (the Wiener filter),
//   x = F^T diag(w / N) d                                                   (the inverse-FFT estimator),
// c_f = w_f^2 Ni_r,f the window, the inverse noise and the real / imaginary factors of the reference's Ni_r in one
// coefficient per real row, zero on a channel that is cut.  F^T diag(c) F is circulant (2 x 2 block circulant in the
// complex time domain): it is fixed by g[d] = sum_f c_f cos(2 pi f d / N) (and the sine sum), which is the projection
// of c itself -- one more right-hand side of the product that gives y.  So no Gram product is formed and every
// baseline shares one unmasked Fourier matrix over the channels of the container.
//
// Stages, all float64, batched over baselines:
//   k_dl_fourier  the shared Fourier matrix F0 [2 nchan][order], twiddle arguments reduced in integers;
//   k_dl_prep     one block per baseline walks its [sample, freq] block through strides: sample and channel masks, the
//                 skip status, the channel means, c, and X [sample (+ 1)][2 nchan] = c o (d - mean) with c as last row;
//   k_dl_gemm     C = beta C + alpha A B on v_mfma_f64_16x16x4_f64, 64 x 64 tiles, either operand through any strides:
//                 the projection Y = X F0, the trailing updates of the factorisation, the updates of the solves;
//   k_dl_fill     G = circ(g) + diag(Si) from the last row of Y;
//   k_dl_potrf / k_dl_panel   G = U^T U, right-looking in blocks of 32 rows: the diagonal block in LDS, the row panel
//                 one column per thread, the rest is k_dl_gemm on the upper tiles; a non-positive pivot sets status;
//   k_dl_trsm     the 32 x 32 diagonal step of Z U = Y and X U^T = Z, one right-hand side per thread (the sample rows);
//   k_dl_store    spectrum[b, s, :] = fftshift(x) as complex128, zeros outside the retained samples, the mask bytes.
// Every kernel after k_dl_prep leaves a baseline alone once its status word is set.  k_dl_gemm, k_dl_potrf, k_dl_panel,
// k_dl_trsm and their host loops (dl_gemm, dl_factor, dl_solve_rows) are compiled once, in chol_blocked.hip, and
// reached through chol_blocked.h; mfilter.hip and dpss.hip call the same copy.
#include "chol_blocked.h"

namespace {

constexpr int kDlMaxOrder = 2048;
constexpr int kDlFold = 4;

struct DlView {
  const void* p;
  int dtype;
  int64_t ss, sf, sb[kDlFold];
};

__device__ __forceinline__ double dl_weight(const DlView& v, int64_t i) {
  return v.dtype == DMM_DELAY_F32 ? (double)((const float*)v.p)[i] : ((const double*)v.p)[i];
}

__device__ __forceinline__ double2 dl_data(const DlView& v, int64_t i) {
  switch (v.dtype) {
    case DMM_DELAY_F32: return make_double2((double)((const float*)v.p)[i], 0.0);
    case DMM_DELAY_F64: return make_double2(((const double*)v.p)[i], 0.0);
    case DMM_DELAY_C64: {
      const float2 z = ((const float2*)v.p)[i];
      return make_double2((double)z.x, (double)z.y);
    }
    default: return ((const double2*)v.p)[i];
  }
}

// F0[2 f][.] / F0[2 f + 1][.]: the real and imaginary rows of channel chan[f]; (chan t) mod N in integers, then sincospi.
__global__ void k_dl_fourier(int N, int nchan, int complex_td, const int32_t* __restrict__ chan, double* __restrict__ F) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)nchan * N) return;
  const int f = (int)(e / N), t = (int)(e % N);
  const int64_t m = ((int64_t)chan[f] * t) % N;
  double s, c;
  sincospi(2.0 * (double)m / (double)N, &s, &c);
  if (complex_td) {
    double* r0 = F + (size_t)(2 * f) * 2 * N;
    double* r1 = r0 + 2 * N;
    r0[2 * t] = c;
    r0[2 * t + 1] = s;
    r1[2 * t] = -s;
    r1[2 * t + 1] = c;
  } else {
    F[(size_t)(2 * f) * N + t] = c;
    F[(size_t)(2 * f + 1) * N + t] = -s;
  }
}

struct DlPrep {
  DlView d, w;
  int nfold;
  int64_t fold_n[kDlFold];
  int64_t base0;
  int ns, nchan, N, nrow;
  int complex_td, wiener, remove_mean;
  double time_frac, freq_frac, weight_boost;
  const double* coef;
  const int32_t* chan;
  double* X;
  uint8_t* nzt;
  int32_t* status;
  double* cc;      // scratch [nbase][2 nchan]
  double2* mean;   // scratch [nbase][nchan]
  uint8_t* nzf;    // scratch [nbase][nchan]
};

__global__ __launch_bounds__(256) void k_dl_prep(DlPrep a) {
  __shared__ int s_ntr, s_any, s_nzf, s_nz;
  const int b = blockIdx.x;
  int64_t gb = a.base0 + b, od = 0, ow = 0;
  for (int q = a.nfold - 1; q >= 0; --q) {
    const int64_t i = gb % a.fold_n[q];
    gb /= a.fold_n[q];
    od += i * a.d.sb[q];
    ow += i * a.w.sb[q];
  }
  if (threadIdx.x == 0) {
    s_ntr = 0;
    s_any = 0;
    s_nzf = 0;
    s_nz = 0;
  }
  __syncthreads();
  const int ns = a.ns, nchan = a.nchan, K = 2 * nchan;
  uint8_t* nzt = a.nzt + (size_t)b * ns;
  uint8_t* nzf = a.nzf + (size_t)b * nchan;
  double* cc = a.cc + (size_t)b * K;
  double2* mean = a.mean + (size_t)b * nchan;
  double* X = a.X + (size_t)b * a.nrow * K;

  // ---- samples: nzt[s] = (share of channels with weight > 0) > time_frac
  {
    int ntr = 0, any = 0;
    for (int s = threadIdx.x; s < ns; s += 256) {
      int cnt = 0;
      for (int f = 0; f < nchan; ++f) cnt += dl_weight(a.w, ow + s * a.w.ss + f * a.w.sf) > 0.0 ? 1 : 0;
      const int keep = (double)cnt / (double)nchan > a.time_frac ? 1 : 0;
      nzt[s] = (uint8_t)keep;
      ntr += keep;
      any |= cnt > 0 ? 1 : 0;
    }
    if (ntr) atomicAdd(&s_ntr, ntr);
    if (any) atomicOr(&s_any, 1);
  }
  __syncthreads();
  const int ntr = s_ntr;
  if (!s_any || ntr == 0) {  // (the same in every thread)
    if (threadIdx.x == 0) a.status[b] = DMM_DELAY_SKIPPED;
    return;
  }

  // ---- channels, over the retained samples: nzf, the mean, the average weight and the coefficients
  {
    int kept = 0;
    for (int f = threadIdx.x; f < nchan; f += 256) {
      int cnt = 0;
      double wsum = 0.0, mr = 0.0, mi = 0.0;
      for (int s = 0; s < ns; ++s) {
        if (!nzt[s]) continue;
        const double w = dl_weight(a.w, ow + s * a.w.ss + f * a.w.sf);
        cnt += w > 0.0 ? 1 : 0;
        wsum += w;
        const double2 z = dl_data(a.d, od + s * a.d.ss + f * a.d.sf);
        mr += z.x;
        mi += z.y;
      }
      const int keep = (double)cnt / (double)ntr > a.freq_frac ? 1 : 0;
      nzf[f] = (uint8_t)keep;
      kept += keep;
      mean[f] = a.remove_mean ? make_double2(mr / ntr, mi / ntr) : make_double2(0.0, 0.0);
      double cre = 0.0, cim = 0.0;
      if (keep) {
        if (a.wiener) {
          const double ni = wsum / ntr * a.weight_boost;
          const int ci = a.chan[f];
          const bool real_chan = !a.complex_td && (ci == 0 || ci == a.N / 2);
          cre = a.coef[f] * (real_chan ? ni : 2.0 * ni);
          cim = real_chan ? 0.0 : a.coef[f] * 2.0 * ni;
        } else {
          cre = cim = a.coef[f];
        }
      }
      cc[2 * f] = cre;
      cc[2 * f + 1] = cim;
    }
    if (kept) atomicAdd(&s_nzf, kept);
  }
  __syncthreads();
  if (s_nzf == 0) {
    if (threadIdx.x == 0) a.status[b] = DMM_DELAY_SKIPPED;
    return;
  }

  // ---- X = c o (d - mean) on the retained samples, zero rows elsewhere; c itself as the last row (Wiener)
  int nz = 0;
  for (int64_t e = threadIdx.x; e < (int64_t)ns * nchan; e += 256) {
    const int s = (int)(e / nchan), f = (int)(e % nchan);
    double xr = 0.0, xi = 0.0;
    if (nzt[s] && nzf[f]) {
      const double2 z = dl_data(a.d, od + s * a.d.ss + f * a.d.sf);
      const double2 m = mean[f];
      const double dr = z.x - m.x, di = z.y - m.y;
      nz |= (dr != 0.0 || di != 0.0) ? 1 : 0;
      const double cre = cc[2 * f], cim = cc[2 * f + 1];
      xr = cre != 0.0 ? cre * dr : 0.0;
      xi = cim != 0.0 ? cim * di : 0.0;
    }
    X[(size_t)s * K + 2 * f] = xr;
    X[(size_t)s * K + 2 * f + 1] = xi;
  }
  if (a.wiener) {
    for (int f = threadIdx.x; f < nchan; f += 256) {
      X[(size_t)ns * K + 2 * f] = cc[2 * f];
      X[(size_t)ns * K + 2 * f + 1] = 0.0;
    }
  }
  if (nz) atomicOr(&s_nz, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!s_nz) a.status[b] = DMM_DELAY_SKIPPED;
    else if (!a.wiener && s_nzf != nchan) a.status[b] = DMM_DELAY_CUT;
  }
}

// G = circ(g) + diag(Si); g (and the sine sequence, interleaved, in the complex time domain) is row `crow` of Y.
__global__ void k_dl_fill(int n, int complex_td, int nrow, const double* __restrict__ Yall, const double* __restrict__ Si, double* __restrict__ Gall, const int32_t* __restrict__ status) {
  const int bat = blockIdx.y;
  if (status[bat]) return;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)n * n) return;
  const int i = (int)(idx / n), j = (int)(idx % n);
  const double* __restrict__ g = Yall + ((size_t)bat * nrow + (nrow - 1)) * n;
  double v;
  if (complex_td) {
    const int N = n / 2, t = i >> 1, p = i & 1, u = j >> 1, q = j & 1;
    const int d = (t - u + N) % N;
    v = p == q ? g[2 * d] : (p ? g[2 * d + 1] : -g[2 * d + 1]);
  } else {
    v = g[(i - j + n) % n];
  }
  if (i == j) v += Si[(size_t)bat * n + i];
  Gall[(size_t)bat * n * n + idx] = v;
}

// spectrum[b][s][j] = x[s][(j - N / 2) mod N] (numpy's fftshift), complex128; zero where the sample or the baseline
// was dropped.  mask[b][s] = 1 there.
__global__ void k_dl_store(int N, int complex_td, int ns, int nrow, const double* __restrict__ Yall, const uint8_t* __restrict__ nzt, const int32_t* __restrict__ status, double2* __restrict__ spec,
                           uint8_t* __restrict__ mask) {
  const int bat = blockIdx.z, s = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = status[bat] == 0 && nzt[(size_t)bat * ns + s] != 0;
  if (mask && j == 0) mask[(size_t)bat * ns + s] = ok ? 0 : 1;
  if (j >= N) return;
  double2 v = make_double2(0.0, 0.0);
  if (ok) {
    const int t = (j + N - N / 2) % N;
    const int n = complex_td ? 2 * N : N;
    const double* __restrict__ x = Yall + ((size_t)bat * nrow + s) * n;
    v = complex_td ? make_double2(x[2 * t], x[2 * t + 1]) : make_double2(x[t], 0.0);
  }
  spec[((size_t)bat * ns + s) * N + j] = v;
}

DlView dl_view(const dmm_delay_view* v) {
  DlView r{};
  r.p = v->ptr;
  r.dtype = v->dtype;
  r.ss = v->stride_sample;
  r.sf = v->stride_freq;
  for (int q = 0; q < kDlFold; ++q) r.sb[q] = v->stride_fold[q];
  return r;
}

bool dl_view_ok(const dmm_delay_view* v) {
  bool ok = v->stride_sample >= 0 && v->stride_freq >= 0;
  for (int q = 0; q < kDlFold; ++q) ok = ok && v->stride_fold[q] >= 0;
  return ok;
}

}  // namespace

extern "C" {

int dmm_delay_fourier(dmm_ctx* ctx, int ndelay, int nchan, int complex_td, const int32_t* chan, double* F) {
  DMM_REQUIRE(ctx != nullptr, "dmm_delay_fourier: ctx is NULL");
  DMM_REQUIRE(ndelay >= 1 && nchan >= 1, "dmm_delay_fourier: bad sizes %d delays, %d channels", ndelay, nchan);
  DMM_REQUIRE(chan && F, "dmm_delay_fourier: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t ne = (int64_t)nchan * ndelay;
  hipLaunchKernelGGL(k_dl_fourier, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, ndelay, nchan, complex_td ? 1 : 0, chan, F);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_delay_prepare(dmm_ctx* ctx, int ndelay, int nchan, int nsample, int nbase, int64_t base0, int nfold, const int64_t* fold_n, const dmm_delay_view* data, const dmm_delay_view* weight,
                      int complex_td, int wiener, int remove_mean, double time_frac, double freq_frac, double weight_boost, const double* coef, const int32_t* chan, double* X, uint8_t* nzt,
                      int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_delay_prepare: ctx is NULL");
  DMM_REQUIRE(ndelay >= 1 && nchan >= 1 && nsample >= 1, "dmm_delay_prepare: bad sizes %d delays, %d channels, %d samples", ndelay, nchan, nsample);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535 && base0 >= 0, "dmm_delay_prepare: bad baseline count %d", nbase);
  DMM_REQUIRE(nfold >= 0 && nfold <= kDlFold, "dmm_delay_prepare: %d folded axes, at most %d", nfold, kDlFold);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(data && weight && data->ptr && weight->ptr && coef && chan && X && nzt && status && (nfold == 0 || fold_n), "dmm_delay_prepare: NULL argument");
  DMM_REQUIRE(dl_view_ok(data) && dl_view_ok(weight), "dmm_delay_prepare: negative stride");
  DMM_REQUIRE(data->dtype >= DMM_DELAY_F32 && data->dtype <= DMM_DELAY_C128, "dmm_delay_prepare: bad data dtype %d", data->dtype);
  DMM_REQUIRE(weight->dtype == DMM_DELAY_F32 || weight->dtype == DMM_DELAY_F64, "dmm_delay_prepare: bad weight dtype %d", weight->dtype);
  for (int q = 0; q < nfold; ++q) DMM_REQUIRE(fold_n[q] >= 1, "dmm_delay_prepare: bad length of folded axis %d", q);
  DMM_HIP(hipSetDevice(ctx->device));
  DlPrep a{};
  a.d = dl_view(data);
  a.w = dl_view(weight);
  a.nfold = nfold;
  for (int q = 0; q < nfold; ++q) a.fold_n[q] = fold_n[q];
  a.base0 = base0;
  a.ns = nsample;
  a.nchan = nchan;
  a.N = ndelay;
  a.nrow = nsample + (wiener ? 1 : 0);
  a.complex_td = complex_td ? 1 : 0;
  a.wiener = wiener ? 1 : 0;
  a.remove_mean = remove_mean ? 1 : 0;
  a.time_frac = time_frac;
  a.freq_frac = freq_frac;
  a.weight_boost = weight_boost;
  a.coef = coef;
  a.chan = chan;
  a.X = X;
  a.nzt = nzt;
  a.status = status;
  const size_t per = (size_t)nchan * (2 * sizeof(double) + sizeof(double2));
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)nbase * (per + nchan), &scratch);
  if (rc) return rc;
  a.cc = (double*)scratch;
  a.mean = (double2*)((char*)scratch + (size_t)nbase * nchan * 2 * sizeof(double));
  a.nzf = (uint8_t*)scratch + (size_t)nbase * per;
  DMM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * nbase, ctx->stream));
  hipLaunchKernelGGL(k_dl_prep, dim3((unsigned)nbase), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_delay_project(dmm_ctx* ctx, int order, int nchan, int nrow, int nbase, const double* X, const double* F, double* Y, const int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_delay_project: ctx is NULL");
  DMM_REQUIRE(order >= 1 && nchan >= 1 && nrow >= 1, "dmm_delay_project: bad sizes order %d, %d channels, %d rows", order, nchan, nrow);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_delay_project: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(X && F && Y && status, "dmm_delay_project: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int K = 2 * nchan;
  DlGemm g{};
  g.A = X, g.a_rs = K, g.a_cs = 1, g.a_bs = (int64_t)nrow * K;
  g.B = F, g.b_rs = order, g.b_cs = 1, g.b_bs = 0;
  g.C = Y, g.c_rs = order, g.c_bs = (int64_t)nrow * order;
  g.M = nrow, g.N = order, g.K = K;
  g.alpha = 1.0, g.beta = 0, g.upper = 0;
  g.status = status;
  dl_gemm(ctx, g, nbase);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_delay_solve(dmm_ctx* ctx, int order, int complex_td, int nsample, int nbase, double* Y, const double* Si, double* G, int32_t* status) {
  DMM_REQUIRE(ctx != nullptr, "dmm_delay_solve: ctx is NULL");
  DMM_REQUIRE(order >= 1 && order <= kDlMaxOrder, "dmm_delay_solve: order %d outside 1 ... %d", order, kDlMaxOrder);
  DMM_REQUIRE(!complex_td || order % 2 == 0, "dmm_delay_solve: odd order %d in the complex time domain", order);
  DMM_REQUIRE(nsample >= 1, "dmm_delay_solve: bad sample count %d", nsample);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_delay_solve: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(Y && Si && G && status, "dmm_delay_solve: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int n = order, nrow = nsample + 1;
  const int64_t nn = (int64_t)n * n;
  hipLaunchKernelGGL(k_dl_fill, dim3((unsigned)((nn + 255) / 256), (unsigned)nbase), dim3(256), 0, ctx->stream, n, complex_td ? 1 : 0, nrow, (const double*)Y, Si, G, (const int32_t*)status);
  dl_factor(ctx, n, nbase, G, status, DMM_DELAY_NOT_POSDEF);
  dl_solve_rows(ctx, n, nrow, nsample, nbase, G, Y, status);  // (the last row of Y, the circulant sequence, is not solved)
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_delay_store(dmm_ctx* ctx, int ndelay, int complex_td, int nsample, int nrow, int nbase, const double* Y, const uint8_t* nzt, const int32_t* status, void* spectrum, uint8_t* mask) {
  DMM_REQUIRE(ctx != nullptr, "dmm_delay_store: ctx is NULL");
  DMM_REQUIRE(ndelay >= 1 && nsample >= 1 && nsample <= 65535 && nrow >= nsample, "dmm_delay_store: bad sizes %d delays, %d samples, %d rows", ndelay, nsample, nrow);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_delay_store: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(Y && nzt && status && spectrum, "dmm_delay_store: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_dl_store, dim3((unsigned)((ndelay + 255) / 256), (unsigned)nsample, (unsigned)nbase), dim3(256), 0, ctx->stream, ndelay, complex_td ? 1 : 0, nsample, nrow, Y, nzt, status,
                     (double2*)spectrum, mask);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
