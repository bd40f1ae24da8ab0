// m-mode transform kernels: batched sidereal-time <-> m FFT fused with the +/-m pack / unpack (k_mfft_pack,
// k_mifft_unpack), the analytic transit beam generated into the same forward transform (k_beam_mfft), the noise-weight
// reduction (k_mmode_weight) -- and the host side of every in-LDS row FFT of the library: the twiddle / chirp / filter
// tables and the planner dmm_row_fft_plan (ringmap.hip plans its transforms through it too; the passes are in fft_lds.h).
//
// Replaces (reference radiocosmology/draco):
//   _make_marray            draco/analysis/transform.py:644-705  -> k_mfft_pack
//   weight reduction        draco/analysis/transform.py:599-602,627,638-639 -> k_mmode_weight
//   _unpack_marray/_make_ssarray  transform.py:814-851           -> k_mifft_unpack
//
// Design (gfx950): one workgroup transforms RB rows that are adjacent in the
// (freq, baseline) order entirely inside LDS, so that the transposed store into
// the m-major MModes layout [m, +/-, row] writes RB*16-byte contiguous segments
// and the spectrum never makes a round trip through HBM.  Power-of-two lengths run
// an in-place radix-2 decimation-in-frequency pass (natural in, bit-reversed out;
// the pack stage reads through the bit reversal for free).  Every other length --
// SimulateSidereal always produces the odd length 2*mmax+1 (stream.py:76) -- runs
// Bluestein's chirp-z inside the same LDS image: DIF forward, pointwise filter stored
// in bit-reversed order, DIT inverse, so no reordering pass exists anywhere.
// The forward transform is single precision like the reference's complex64 FFT
// (transform.py:689); the inverse is double precision like the reference's complex128
// ifft (transform.py:817).
#include <math.h>

#include <vector>

#include "dmm_internal.h"
#include "fft_lds.h"

namespace {

using dmm_fft::C;
using dmm_fft::cmul;
using dmm_fft::RowFft;

constexpr int kThreads = 1024;

// The +/-m pack of a forward transform (transform.py:678-703): out[m, s, row], s = 0 the +m side, s = 1 the conjugated -m side
struct PmPack {
  int mmax, mlim, mlim_neg;  // slots m <= mmax; bins kept: +m up to mlim, -m up to mlim_neg (pm_pack_limits)
};
// Slot (m, s) of a row: bin k = m or N - m of its spectrum times inv_n (and mscale[m]), the -m side conjugated; zero in every slot the
// reference leaves at its :623 zero fill.
template <typename T>
__device__ __forceinline__ void pm_pack_value(const RowFft<T>& q, bool blue, const dmm_fft::C<T>* row, const PmPack& pk, int m, int s,
                                              double inv_n, const double* mscale, double& re, double& im) {
  re = im = 0.0;
  int k = -1;
  if (s == 0 && m <= pk.mlim) k = m;
  if (s == 1 && m >= 1 && m <= pk.mlim_neg) k = q.N - m;
  if (k >= 0) {
    const C<T> v = dmm_fft::spectrum_at<T>(row, q.chirp, blue, k, q.logM);
    double sc = inv_n;
    if (mscale) sc *= mscale[m];
    re = (double)v.x * sc;
    im = (s ? -(double)v.y : (double)v.y) * sc;
  }
}

struct MfftParams {
  const float2* ts;
  int64_t nrow;
  RowFft<float> fft;
  void* out;
  int out_c128;
  PmPack pk;
  const double* mscale;
};

// Forward: FFT RB rows in LDS, then pack +/-m straight into out[m, s, row].
template <bool BLUESTEIN>
__global__ __launch_bounds__(kThreads) void k_mfft_pack(MfftParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  C<float>* buf = reinterpret_cast<C<float>*>(smem);
  const RowFft<float>& q = p.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int64_t r0 = (int64_t)blockIdx.x * RB;

  const C<float>* tw = dmm_fft::stage_twiddles<float, kThreads, false>(q, buf + (size_t)RB * P);
  // coalesced row loads; rows past the end of the batch are zero
  if (!BLUESTEIN && (N & 1) == 0) {  // power of two: 16 bytes per lane
    const int n2 = N >> 1;
    for (int idx = threadIdx.x; idx < RB * n2; idx += kThreads) {
      const int r = idx / n2, k2 = idx - r * n2;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < p.nrow) x = reinterpret_cast<const float4*>(p.ts + (r0 + r) * (int64_t)N)[k2];
      buf[r * P + 2 * k2] = {x.x, x.y};
      buf[r * P + 2 * k2 + 1] = {x.z, x.w};
    }
  } else {
    for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
      const int r = idx / M, k = idx - r * M;
      C<float> v = {0.f, 0.f};
      if (k < N && r0 + r < p.nrow) {
        const float2 x = p.ts[(r0 + r) * (int64_t)N + k];
        v = {x.x, x.y};
        if (BLUESTEIN) {
          const float2 c = q.chirp[k];
          v = cmul<float>(v, {c.x, c.y});
        }
      }
      buf[r * P + k] = v;
    }
  }
  __syncthreads();
  dmm_fft::row_fft_forward<float, kThreads>(q, BLUESTEIN, buf, tw);

  // pack: consecutive threads -> consecutive rows, so each (m, s) slot is one
  // RB*elem-byte contiguous store segment
  const double inv_n = 1.0 / (double)N;
  const int nslot = (p.pk.mmax + 1) * 2;
  for (int idx = threadIdx.x; idx < nslot * RB; idx += kThreads) {
    const int r = idx % RB, ms = idx / RB;
    if (r0 + r >= p.nrow) continue;
    double re, im;
    pm_pack_value<float>(q, BLUESTEIN, buf + r * P, p.pk, ms >> 1, ms & 1, inv_n, p.mscale, re, im);
    const int64_t o = (int64_t)ms * p.nrow + r0 + r;
    if (p.out_c128) {  // written once, read by a later kernel
      __builtin_nontemporal_store(re, reinterpret_cast<double*>(p.out) + 2 * o);
      __builtin_nontemporal_store(im, reinterpret_cast<double*>(p.out) + 2 * o + 1);
    } else {
      reinterpret_cast<float2*>(p.out)[o] = make_float2((float)re, (float)im);
    }
  }
}

struct BeamParams {
  int npol, nfreq, n_ew, nel;
  int64_t nrow;
  RowFft<double> fft;
  const double* freq;    // [nfreq] MHz
  const double* ew;      // [n_ew] m
  const double* dec;     // [nel] rad
  const double* coef_a;  // [npol] beam-width coefficient of the first / second feed of the pol pair
  const double* coef_b;
  float2* out;  // [mmax+1, 2, nrow]
  PmPack pk;
};

// Analytic transit beam (ringmapmaker.py:1019-1025,1046-1064), conjugated (:1066), generated straight into the LDS
// image of a double-precision forward transform and packed like k_mfft_pack; rows are (pol, freq, ew, el).
template <bool BLUESTEIN>
__global__ __launch_bounds__(kThreads) void k_beam_mfft(BeamParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  __shared__ double s_u[16], s_is2[16];
  const RowFft<double>& q = p.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int64_t r0 = (int64_t)blockIdx.x * RB;

  const C<double>* tw = dmm_fft::stage_twiddles<double, kThreads, true>(q, buf + (size_t)RB * P);
  if (threadIdx.x < RB && r0 + threadIdx.x < p.nrow) {
    int64_t r = r0 + threadIdx.x;
    const int el = (int)(r % p.nel);
    r /= p.nel;
    const int e = (int)(r % p.n_ew);
    r /= p.n_ew;
    const int f = (int)(r % p.nfreq);
    const int pol = (int)(r / p.nfreq);
    const double fr = p.freq[f], cd = cos(p.dec[el]);
    const double wv = 299792458.0 * 1e-6 / fr;  // scipy.constants.c * 1e-6 / freq (:1047)
    s_u[threadIdx.x] = p.ew[e] / wv * cd;
    const double sa = p.coef_a[pol] / fr / cd, sb = p.coef_b[pol] / fr / cd;
    const double sig = sa * sb / sqrt(sa * sa + sb * sb);
    s_is2[threadIdx.x] = 1.0 / (2.0 * sig * sig);
  }
  __syncthreads();
  const double step = 360.0 / (double)N;  // np.linspace(0, 360, nra, endpoint=False) then np.radians
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx / M, k = idx - r * M;
    C<double> v = {0.0, 0.0};
    if (k < N && r0 + r < p.nrow) {
      const double phi = ((double)k * step) * (M_PI / 180.0);
      const double t = 2.0 * tan(0.5 * phi);
      const double amp = exp(-(t * t) * s_is2[r]);
      double sn, cs;
      sincos(2.0 * M_PI * s_u[r] * sin(phi), &sn, &cs);
      v = {amp * cs, -amp * sn};
      if (BLUESTEIN) {
        const double2 c = q.chirp[k];
        v = cmul<double>(v, {c.x, c.y});
      }
    }
    buf[r * P + k] = v;
  }
  __syncthreads();
  dmm_fft::row_fft_forward<double, kThreads>(q, BLUESTEIN, buf, tw);
  const double inv_n = 1.0 / (double)N;
  const int nslot = (p.pk.mmax + 1) * 2;
  for (int idx = threadIdx.x; idx < nslot * RB; idx += kThreads) {
    const int r = idx % RB, ms = idx / RB;
    if (r0 + r >= p.nrow) continue;
    double re, im;
    pm_pack_value<double>(q, BLUESTEIN, buf + r * P, p.pk, ms >> 1, ms & 1, inv_n, nullptr, re, im);
    p.out[(int64_t)ms * p.nrow + r0 + r] = make_float2((float)re, (float)im);
  }
}

struct MifftParams {
  const double2* mvis;  // [n_m, 2, nrow]
  int64_t nrow;
  RowFft<double> fft;
  int mmax_plus, mmax_minus;
  const double* mscale;
  float2* out;  // [nrow, N]
};

// Inverse: gather the +/-m slots into FFT order (transform.py:838-849), run
// y[n] = sum_k X[k] exp(+2 pi i k n / N)  (= ifft(X * N), transform.py:817) and store
// complex64 rows.  Computed as conj(DFT(conj X)) so the forward machinery is shared.
template <bool BLUESTEIN>
__global__ __launch_bounds__(kThreads) void k_mifft_unpack(MifftParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  const RowFft<double>& q = p.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int64_t r0 = (int64_t)blockIdx.x * RB;

  const C<double>* tw = dmm_fft::stage_twiddles<double, kThreads, true>(q, buf + (size_t)RB * P);
  // transposed gather: consecutive threads -> consecutive rows of one (m, s) slot
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx % RB, k = idx / RB;
    C<double> v = {0.0, 0.0};
    if (k < N && r0 + r < p.nrow) {
      int m = -1, s = 0;
      if (k <= p.mmax_plus) {  // k == 0, the +m side and (even lengths) the Nyquist bin
        m = k;
        s = 0;
        // the -m side wins where both map to the same bin only if k > mmax_plus: never here
      }
      if (k >= 1 && N - k >= 1 && N - k <= p.mmax_minus && k > p.mmax_plus) {
        m = N - k;
        s = 1;
      }
      if (m >= 0) {
        const double2 x = p.mvis[((int64_t)m * 2 + s) * p.nrow + r0 + r];
        const double sc = p.mscale ? p.mscale[m] : 1.0;
        // X[k] = +m value, or conj(-m value); we load conj(X[k])
        v = {x.x * sc, (s ? x.y : -x.y) * sc};
        if (BLUESTEIN) {
          const double2 c = q.chirp[k];
          v = cmul<double>(v, {c.x, c.y});
        }
      }
    }
    buf[r * P + dmm_fft::inverse_slot(BLUESTEIN, k, q.logM)] = v;
  }
  __syncthreads();
  dmm_fft::row_fft_inverse<double, kThreads>(q, BLUESTEIN, buf, tw);
  for (int idx = threadIdx.x; idx < RB * N; idx += kThreads) {
    const int r = idx / N, n = idx - r * N;
    if (r0 + r >= p.nrow) continue;
    C<double> v = buf[r * P + n];
    if (BLUESTEIN) {
      const double2 c = q.chirp[n];
      v = cmul<double>(v, {c.x, c.y});
    }
    p.out[(r0 + r) * (int64_t)N + n] = make_float2((float)v.x, (float)(-v.y));
  }
}

// weight: ws[r] = nra^2 * inz(sum_ra inz(w[r, ra])); out[m, s, r] = ws[r] * wscale[m].
// One wave per row; the broadcast over (m, s) is written by the same block with
// consecutive threads on consecutive rows.
constexpr int kWRows = 64;  // rows per block (16 waves x 4 rows each): every (m, +/-) slot is one 512-byte store segment
                            // (16 rows = 128-byte segments ran at 4.2 TB/s: tools/stage_timings.py)
__global__ __launch_bounds__(kThreads) void k_mmode_weight(const float* __restrict__ w, int64_t nrow,
                                                           int nra, double* __restrict__ out, int mmax,
                                                           const double* __restrict__ wscale) {
  __shared__ double ws[kWRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kWRows;
  const bool vec = (nra & 3) == 0;  // rows 16-byte aligned: four weights per load
  for (int rr = wave; rr < kWRows; rr += kThreads / 64) {
    const int64_t r = r0 + rr;
    double acc = 0.0;
    if (r < nrow) {
      const float* row = w + r * (int64_t)nra;
      if (vec) {
        for (int k = lane; k < (nra >> 2); k += 64) {
          const float4 x = reinterpret_cast<const float4*>(row)[k];
          acc += ((x.x != 0.f) ? 1.0 / (double)x.x : 0.0) + ((x.y != 0.f) ? 1.0 / (double)x.y : 0.0);
          acc += ((x.z != 0.f) ? 1.0 / (double)x.z : 0.0) + ((x.w != 0.f) ? 1.0 / (double)x.w : 0.0);
        }
      } else {
        for (int k = lane; k < nra; k += 64) {
          const float x = row[k];
          acc += (x != 0.f) ? 1.0 / (double)x : 0.0;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) ws[rr] = (acc != 0.0) ? (double)nra * (double)nra / acc : 0.0;
  }
  __syncthreads();
  const int nslot = (mmax + 1) * 2;
  if ((nrow & 1) == 0) {  // slots 16-byte aligned: two rows per store
    for (int idx = threadIdx.x; idx < nslot * (kWRows / 2); idx += kThreads) {
      const int rr = 2 * (idx % (kWRows / 2)), ms = idx / (kWRows / 2);
      if (r0 + rr >= nrow) continue;
      const double sc = wscale ? wscale[ms >> 1] : 1.0;
      double* dst = &out[(int64_t)ms * nrow + r0 + rr];
      __builtin_nontemporal_store(ws[rr] * sc, dst);  // written once, read by a later kernel
      __builtin_nontemporal_store(ws[rr + 1] * sc, dst + 1);
    }
    return;
  }
  for (int idx = threadIdx.x; idx < nslot * kWRows; idx += kThreads) {
    const int rr = idx % kWRows, ms = idx / kWRows;
    if (r0 + rr >= nrow) continue;
    double v = ws[rr];
    if (wscale) v *= wscale[ms >> 1];
    __builtin_nontemporal_store(v, &out[(int64_t)ms * nrow + r0 + rr]);  // written once, read by a later kernel
  }
}

__global__ void k_row_is_zero(const double2* __restrict__ x, int64_t n, int* flag) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int nz = 0;
  for (; i < n; i += stride) nz |= (x[i].x != 0.0 || x[i].y != 0.0);
  if (nz) atomicOr(flag, 1);
}

// ---- host side: tables
template <typename T2>
int upload(const std::vector<T2>& h, T2** d) {
  DMM_HIP(hipMalloc((void**)d, h.size() * sizeof(T2)));
  DMM_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T2), hipMemcpyHostToDevice));
  return DMM_OK;
}

int host_bitrev(int i, int logM) {
  int j = 0;
  for (int b = 0; b < logM; ++b) j |= ((i >> b) & 1) << (logM - 1 - b);
  return j;
}

void host_fft(std::vector<double>& re, std::vector<double>& im) {  // in-place radix-2, forward
  const int M = (int)re.size(), logM = ilog2(M);
  for (int i = 0; i < M; ++i) {
    const int j = host_bitrev(i, logM);
    if (j > i) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (int half = 1; half < M; half <<= 1)
    for (int g = 0; g < M; g += 2 * half)
      for (int t = 0; t < half; ++t) {
        const double ang = -M_PI * (double)t / (double)half;
        const double wr = cos(ang), wi = sin(ang);
        const int a = g + t, b = a + half;
        const double xr = re[b] * wr - im[b] * wi, xi = re[b] * wi + im[b] * wr;
        re[b] = re[a] - xr;
        im[b] = im[a] - xi;
        re[a] += xr;
        im[a] += xi;
      }
}

std::map<int, dmm_fft_tables<float2>>& table_cache(dmm_ctx* ctx, float) { return ctx->fft_f32; }
std::map<int, dmm_fft_tables<double2>>& table_cache(dmm_ctx* ctx, double) { return ctx->fft_f64; }

// Build (or fetch) the tables for length n in precision T.
template <typename T, typename T2 = typename dmm_fft::Vec2<T>::type>
int get_tables(dmm_ctx* ctx, int n, const dmm_fft_tables<T2>** out) {
  auto& cache = table_cache(ctx, T());
  auto it = cache.find(n);
  if (it != cache.end()) {
    *out = &it->second;
    return DMM_OK;
  }
  dmm_fft_tables<T2> t;
  t.n = n;
  const bool pow2 = dmm_is_pow2(n);
  t.M = pow2 ? n : (1 << ilog2(2 * n - 1));
  const int M = t.M, logM = ilog2(M);
  std::vector<T2> tw(M / 2 > 0 ? M / 2 : 1);
  for (int k = 0; k < M / 2; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)M;
    tw[k].x = (T)cos(a);
    tw[k].y = (T)sin(a);
  }
  int rc = upload<T2>(tw, &t.tw);
  if (rc) return rc;
  if (!pow2) {
    std::vector<T2> chirp(n);
    std::vector<double> br(M, 0.0), bi(M, 0.0);
    for (int k = 0; k < n; ++k) {
      const int64_t k2 = ((int64_t)k * k) % (2 * (int64_t)n);  // exact phase reduction
      const double a = -M_PI * (double)k2 / (double)n;
      chirp[k].x = (T)cos(a);
      chirp[k].y = (T)sin(a);
      br[k] = cos(a);  // b[j] = conj(chirp[|j|]) wrapped to length M
      bi[k] = -sin(a);
      if (k > 0) {
        br[M - k] = cos(a);
        bi[M - k] = -sin(a);
      }
    }
    host_fft(br, bi);
    std::vector<T2> bf(M);
    for (int pidx = 0; pidx < M; ++pidx) {
      const int j = host_bitrev(pidx, logM);
      bf[pidx].x = (T)(br[j] / (double)M);
      bf[pidx].y = (T)(bi[j] / (double)M);
    }
    rc = upload<T2>(chirp, &t.chirp);
    if (rc) return rc;
    rc = upload<T2>(bf, &t.bfilt);
    if (rc) return rc;
  }
  auto ins = cache.emplace(n, t);
  *out = &ins.first->second;
  return DMM_OK;
}

// Sizing of the m-mode transforms: up to 16 rows per block in about half the LDS, fewer for a batch that small
constexpr size_t kLdsTarget = 80 * 1024, kLdsLimit = 160 * 1024;
constexpr dmm_fft_sizing kSizeF32 = {16, kLdsTarget, kLdsLimit, false, true};
// (the twiddles are read from memory by the double-precision Bluestein transforms of 2049 ... 4096 points: M = 8192)
constexpr dmm_fft_sizing kSizeF64 = {16, kLdsTarget, kLdsLimit, true, true};

PmPack pm_pack_limits(int nra, int mmax) {
  PmPack pk;
  pk.mmax = mmax;
  pk.mlim = nra / 2 < mmax ? nra / 2 : mmax;                       // transform.py:678
  pk.mlim_neg = (mmax >= nra / 2) ? nra / 2 - 1 + nra % 2 : mmax;  // transform.py:679
  return pk;
}

}  // namespace

void dmm_row_fft_sizes(int M, size_t elem, int64_t ntrans, const dmm_fft_sizing& sz, int* RB, int* P, int* tw_lds, size_t* lds, bool* fits) {
  *P = M + 1;
  const size_t row = (size_t)(*P) * elem, tw = (size_t)(M / 2) * elem;
  int rb = sz.rb_max;
  while (rb > 1 && (size_t)rb * row + tw > sz.lds_target) rb >>= 1;
  if (sz.shrink_rb)
    while (rb > 1 && rb / 2 >= ntrans) rb >>= 1;
  *RB = rb;
  *tw_lds = row + tw <= sz.lds_limit;  // (if not, rb is 1: the target is below the limit)
  *fits = *tw_lds || (sz.tw_fallback && row <= sz.lds_limit);
  *lds = (size_t)rb * row + (*tw_lds || !*fits ? tw : 0);
}

template <typename T>
int dmm_row_fft_plan(dmm_ctx* ctx, int nra, int64_t ntrans, const dmm_fft_sizing& sz, RowFft<T>* q, size_t* lds, bool* fits) {
  const dmm_fft_tables<typename RowFft<T>::T2>* t = nullptr;
  const int rc = get_tables<T>(ctx, nra, &t);
  if (rc) return rc;
  q->N = nra;
  q->M = t->M;
  q->logM = ilog2(t->M);
  q->tw = t->tw;
  q->chirp = t->chirp;
  q->bfilt = t->bfilt;
  dmm_row_fft_sizes(q->M, sizeof(typename RowFft<T>::T2), ntrans, sz, &q->RB, &q->P, &q->tw_lds, lds, fits);
  return DMM_OK;
}
template int dmm_row_fft_plan<float>(dmm_ctx*, int, int64_t, const dmm_fft_sizing&, RowFft<float>*, size_t*, bool*);
template int dmm_row_fft_plan<double>(dmm_ctx*, int, int64_t, const dmm_fft_sizing&, RowFft<double>*, size_t*, bool*);

extern "C" {

int dmm_mfft_pack(dmm_ctx* ctx, const void* ts, int64_t nrow, int nra, void* out, int mmax,
                  int out_dtype, const double* mscale) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mfft_pack: ctx is NULL");
  if (nrow == 0) return DMM_OK;  // an empty batch is legal (and has no buffers)
  DMM_REQUIRE(ts && out, "dmm_mfft_pack: NULL argument");
  DMM_REQUIRE(nrow >= 0 && nra >= 1 && mmax >= 0, "dmm_mfft_pack: bad sizes nrow=%lld nra=%d mmax=%d",
              (long long)nrow, nra, mmax);
  DMM_REQUIRE(out_dtype == DMM_C64 || out_dtype == DMM_C128, "dmm_mfft_pack: bad out_dtype %d", out_dtype);
  if (nra > DMM_MAX_NRA) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_mfft_pack: nra=%d > %d", nra, DMM_MAX_NRA);
  DMM_HIP(hipSetDevice(ctx->device));
  MfftParams p;
  size_t lds = 0;
  bool fits = false;
  const int rc = dmm_row_fft_plan<float>(ctx, nra, nrow, kSizeF32, &p.fft, &lds, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_mfft_pack: nra=%d needs %zu B of LDS", nra, lds);
  p.ts = (const float2*)ts;
  p.nrow = nrow;
  p.out = out;
  p.out_c128 = out_dtype == DMM_C128;
  p.pk = pm_pack_limits(nra, mmax);
  p.mscale = mscale;
  return dmm_launch_blocks("dmm_mfft_pack", p.fft.chirp ? k_mfft_pack<true> : k_mfft_pack<false>, (nrow + p.fft.RB - 1) / p.fft.RB,
                           kThreads, lds, ctx->stream, p);
}

int dmm_analytic_beam_mmodes(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, int mmax, const double* freq,
                             const double* ew, const double* dec, const double* coef_a, const double* coef_b, void* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_analytic_beam_mmodes: ctx is NULL");
  DMM_REQUIRE(npol >= 0 && nfreq >= 0 && new_ >= 0 && nel >= 0 && nra >= 1 && mmax >= 0,
              "dmm_analytic_beam_mmodes: bad sizes npol=%d nfreq=%d new=%d nel=%d nra=%d mmax=%d", npol, nfreq, new_, nel, nra, mmax);
  const int64_t nrow = (int64_t)npol * nfreq * new_ * nel;
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(freq && ew && dec && coef_a && coef_b && out, "dmm_analytic_beam_mmodes: NULL argument");
  if (nra > DMM_MAX_NRA) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_analytic_beam_mmodes: nra=%d > %d", nra, DMM_MAX_NRA);
  DMM_HIP(hipSetDevice(ctx->device));
  BeamParams p;
  size_t lds = 0;
  bool fits = false;
  const int rc = dmm_row_fft_plan<double>(ctx, nra, nrow, kSizeF64, &p.fft, &lds, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_analytic_beam_mmodes: nra=%d needs %zu B of LDS", nra, lds);
  p.npol = npol, p.nfreq = nfreq, p.n_ew = new_, p.nel = nel;
  p.nrow = nrow;
  p.freq = freq, p.ew = ew, p.dec = dec, p.coef_a = coef_a, p.coef_b = coef_b;
  p.out = (float2*)out;
  p.pk = pm_pack_limits(nra, mmax);
  return dmm_launch_blocks("dmm_analytic_beam_mmodes", p.fft.chirp ? k_beam_mfft<true> : k_beam_mfft<false>,
                           (nrow + p.fft.RB - 1) / p.fft.RB, kThreads, lds, ctx->stream, p);
}

int dmm_mmode_weight(dmm_ctx* ctx, const float* weight, int64_t nrow, int nra, double* out, int mmax,
                     const double* wscale) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mmode_weight: ctx is NULL");
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(weight && out, "dmm_mmode_weight: NULL argument");
  DMM_REQUIRE(nrow >= 0 && nra >= 1 && mmax >= 0, "dmm_mmode_weight: bad sizes");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t nblk = (nrow + kWRows - 1) / kWRows;
  DMM_REQUIRE(nblk <= 0x7fffffff, "dmm_mmode_weight: too many rows");
  hipLaunchKernelGGL(k_mmode_weight, dim3((unsigned)nblk), dim3(kThreads), 0, ctx->stream, weight, nrow, nra,
                     out, mmax, wscale);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_mifft_unpack(dmm_ctx* ctx, const void* mvis, int n_m, int64_t nrow, int nra, int mmax_plus,
                     int mmax_minus, const double* mscale, void* vis_out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mifft_unpack: ctx is NULL");
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(mvis && vis_out, "dmm_mifft_unpack: NULL argument");
  DMM_REQUIRE(nrow >= 0 && nra >= 1 && n_m >= 1, "dmm_mifft_unpack: bad sizes");
  DMM_REQUIRE(mmax_plus >= 0 && mmax_plus < n_m && mmax_minus >= 0 && mmax_minus <= mmax_plus,
              "dmm_mifft_unpack: bad limits +%d -%d (n_m=%d)", mmax_plus, mmax_minus, n_m);
  DMM_REQUIRE(mmax_plus <= nra / 2 && mmax_minus <= (nra - 1) / 2,
              "dmm_mifft_unpack: limits +%d -%d exceed nra=%d", mmax_plus, mmax_minus, nra);
  if (nra > DMM_MAX_NRA / 2 && !dmm_is_pow2(nra))
    return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_mifft_unpack: non power-of-two nra=%d > %d", nra, DMM_MAX_NRA / 2);
  if (nra > DMM_MAX_NRA) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_mifft_unpack: nra=%d > %d", nra, DMM_MAX_NRA);
  DMM_HIP(hipSetDevice(ctx->device));
  MifftParams p;
  size_t lds = 0;
  bool fits = false;
  const int rc = dmm_row_fft_plan<double>(ctx, nra, nrow, kSizeF64, &p.fft, &lds, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_mifft_unpack: nra=%d needs %zu B of LDS", nra, lds);
  p.mvis = (const double2*)mvis;
  p.nrow = nrow;
  p.mmax_plus = mmax_plus;
  p.mmax_minus = mmax_minus;
  p.mscale = mscale;
  p.out = (float2*)vis_out;
  return dmm_launch_blocks("dmm_mifft_unpack", p.fft.chirp ? k_mifft_unpack<true> : k_mifft_unpack<false>,
                           (nrow + p.fft.RB - 1) / p.fft.RB, kThreads, lds, ctx->stream, p);
}

int dmm_mrow_is_zero(dmm_ctx* ctx, const void* mvis, int n_m, int64_t nrow, int m, int sign, int* is_zero) {
  DMM_REQUIRE(ctx && mvis && is_zero, "dmm_mrow_is_zero: NULL argument");
  DMM_REQUIRE(m >= 0 && m < n_m && (sign == 0 || sign == 1) && nrow >= 0, "dmm_mrow_is_zero: bad index");
  DMM_HIP(hipSetDevice(ctx->device));
  int* flag = nullptr;
  DMM_HIP(hipMalloc((void**)&flag, sizeof(int)));
  DMM_HIP(hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
  if (nrow > 0) {
    const double2* x = (const double2*)mvis + ((int64_t)m * 2 + sign) * nrow;
    int64_t nb = (nrow + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_row_is_zero, dim3((unsigned)nb), dim3(256), 0, ctx->stream, x, nrow, flag);
  }
  int h = 0;
  hipError_t e = hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(flag);
  if (e != hipSuccess) return dmm_set_error((int)e, "dmm_mrow_is_zero: %s", hipGetErrorString(e));
  *is_zero = h ? 0 : 1;
  return DMM_OK;
}

}  // extern "C"
