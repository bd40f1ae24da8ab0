// Deconvolving ring-map makers on hybrid beam-formed m-modes.
//
//   dmm_ringmap_deconvolve  replaces the per-frequency loop of
//   DeconvolveHybridMBase.process (reference draco/analysis/ringmapmaker.py:744-823) with the
//   EW weights / regularisation of TikhonovRingMapMaker (:1096-1121) and WienerRingMapMaker
//   (:1161-1183):
//     sum_w  = sum_{+/-, ew} w |b|^2            C = eps + sum_w  (1 if skip_deconvolution)
//     map_m  = win * sum conj(b) w h / C        dirty_m = win * sum_w / C
//     norm   = 1 / mean_m(dirty_m)              map(ra) = irfft(map_m, nra) * norm  (same for dirty)
//     weight = 1 / (0.5 sum_m (sqrt(sum (w|b|)^2 var) win norm / ((mmax+1) C))^2)
// All HBM-bound elementwise / small-reduction work plus one length-nra inverse FFT per
// (pol, freq, el):
//   k_rm_reduce  lanes across el (coalesced 512-byte row pieces of hv / bv), the (+/-, ew) sums in registers, the modes transposed through LDS to rows contiguous in m, and the
//                block's share of the four per-row sums over m the next stage needs (normalisation, noise weight,
//                dirty-beam power by Parseval, the norm of the map modes), so that every mode is read ONCE downstream;
//   k_rm_fft     one inverse FFT per TWO rows: the Hermitian spectra of two rows' map modes are packed into one
//                complex sequence z = X_map(row0) + i X_map(row1) (when the RA-space dirty beam is asked for:
//                z = X_map + i X_dirty of one row), each of the two scaled by a power of two to the other's size
//                (rm_seq_scale); powers of two run the in-LDS radix passes, other lengths Bluestein (shared machinery,
//                fft_lds.h);
//   k_rm_store   tiled transpose [el][ra] -> the reference's [ra][el] layout.
// Where nra is a power of two, the RA-space dirty beam is not asked for and every row is normalised by itself:
//   k_rm_fused<EL, PARK>  the three stages in one pass: a block owns 8 or 16 elevations of one (pol, freq) for all m, so
//                neither the modes nor the [el][ra] rows reach HBM (16 elevations: 128-byte pieces of the input rows;
//                PARK: the second eight's image waits in a scratch image while the first eight's is transformed).
// The term-weight rule (rm_term_weight), the per-(m, el) mode (rm_mode), the row finish (rm_row_finish) and the scaling of the
// two sequences that share a transform (rm_seq_scale) are shared.
// float64 arithmetic throughout (the reference mixes float32 and float64 by weight scheme).
#include <math.h>

#include "dmm_internal.h"
#include "fft_lds.h"

namespace {

using dmm_fft::C;
constexpr int kThreads = 256;

// What a row needs from all its m before its transform, four sums: dirty (point-source normalisation), q^2 (noise weight),
// c_m dirty^2 (dirty-beam power by Parseval; the scale of the dirty-beam modes) and c_m |map_m|^2 (the scale of the map modes).
struct RmSums {
  double d, q2, p2, x2;
};

struct RmParams {
  int nm, nm_beam, npol, nfreq, new_, nel, nra, mmax;
  int mode;   // 0: w = wt[ew] (normalised table); 1: inverse variance normalised over ew; 2: inverse variance raw
  int skip, iref;
  int nchunk;         // number of m chunks of k_rm_reduce (ceil(nm / MT))
  const float2* hv;   // [nm, 2, npol, nfreq, new, nel]
  const float* hw;    // [nm, 2, npol, nfreq, new]
  const float2* bv;   // [nm_beam, 2, npol, nfreq, new, nel]
  const double* wt;   // [new] weight table (mode 0) or keep-mask (modes 1, 2)
  const double* eps;  // [nfreq, nm]
  const float* window;  // [nfreq, nm, nel] or null
  double2* s_map;     // [npol*nfreq][nel][nm] map modes (re, im)
  double* s_dirty;    // [npol*nfreq][nel][nm] dirty-beam modes (real)
  RmSums* psum;       // [npol*nfreq][nchunk][nel] the chunk's share of the per-row sums over m
  double* tmp_map;    // [npol*nfreq][nel][nra]
  double* tmp_db;     // same or null
  double* dbp;        // [npol*nfreq][nel]   -> dirty_beam_power [1, npol, nfreq, nel]
  double* wv;         // [npol*nfreq][nel]
  double* map;        // [1, npol, nfreq, nra, nel]
  double* weight;     // [npol, nfreq, nra, nel]
  double* db;         // [1, npol, nfreq, nra, nel] or null
};

constexpr int MT = 16;  // m per block in k_rm_reduce
constexpr int kTermBatch = 8;  // (sign, EW) terms whose hv / bv loads are in flight together

// Weight w of the (sign, EW separation) term t of mode m and g = w^2 var: `mode` 0 / 1 / 2 of RmParams.  The term's
// weights do not depend on the elevation: one lane works them out -- two float64 divisions -- and the others pick them up.
__device__ __forceinline__ void rm_term_weight(const RmParams& p, int m, int pol, int f, int t, double& w, double& g) {
  const int s = t / p.new_, e = t - s * p.new_;
  const int64_t wbase = ((((int64_t)m * 2 + s) * p.npol + pol) * p.nfreq + f) * p.new_;
  double iv = (double)p.hw[wbase + e];
  if (p.mode == 0) {
    w = iv > 0.0 ? p.wt[e] : 0.0;
  } else {
    iv *= p.wt[e];  // the reference zeroes the excluded cylinders inside inv_var itself
    if (p.mode == 1) {
      double wsumv = 0.0;
      for (int e2 = 0; e2 < p.new_; ++e2) wsumv += (double)p.hw[wbase + e2] * p.wt[e2];
      w = iv * (wsumv != 0.0 ? 1.0 / wsumv : 0.0);
    } else {
      w = iv;
    }
    if (!(iv > 0.0)) w = 0.0;
  }
  g = w * w * (iv > 0.0 ? 1.0 / iv : 0.0);
}

// One (m, el) from its (+/-, ew) sums: the map mode (ar, ai), the dirty-beam mode rd, and the mode's share of the four
// per-row sums over m (RmSums).
__device__ __forceinline__ void rm_mode(const RmParams& p, double sw, double mre, double mim, double sg, int m, int f, int el,
                                        double& ar, double& ai, double& rd, double& acc_d, double& acc_q, double& acc_p, double& acc_x) {
  const double cinv = p.skip ? 1.0 : p.eps[(int64_t)f * p.nm + m] + sw;
  const double ic = cinv != 0.0 ? 1.0 / cinv : 0.0;
  const double win = p.window ? (double)p.window[((int64_t)f * p.nm + m) * p.nel + el] : 1.0;
  ar = win * mre * ic;
  ai = win * mim * ic;
  rd = win * sw * ic;
  const double qv = sqrt(sg) * win * ic / (double)(p.mmax + 1);  // 1 / ((mmax + 1) C): one division serves all
  acc_d += rd;
  acc_q += qv * qv;
  // weight of mode m in sum_k X_ext(k)^2 of the Hermitian extension to N bins: DC and (even N) Nyquist once
  const bool edge = m == 0 || 2 * m == p.nra;
  acc_p += (edge ? 1.0 : 2.0) * rd * rd;
  acc_x += edge ? ar * ar : 2.0 * (ar * ar + ai * ai);  // (the transform drops the imaginary part of the DC and Nyquist modes)
}

// Two real sequences share one complex transform, z = X_A + i X_B, whose rounding error is relative to the norm of z: a
// weak row -- an elevation far down the beam, a row whose regularisation dwarfs its weights -- beside a strong one would
// come out with the strong one's absolute error.  So each sequence goes in divided by a power of two near the norm of
// its spectrum (exact; `x2` = sum_k |X_ext(k)|^2) and comes out multiplied by it: `scl` on the way in, `isc` on the way
// out.  A sequence without any mode comes out as zeros whatever its partner leaves behind (isc = 0).
__device__ __forceinline__ void rm_seq_scale(double x2, double& scl, double& isc) {
  scl = 1.0;
  isc = x2 == 0.0 ? 0.0 : 1.0;
  if (x2 > 0.0 && x2 < INFINITY) {
    int e = ilogb(x2) >> 1;
    e = e < -480 ? -480 : (e > 480 ? 480 : e);
    scl = ldexp(1.0, -e);
    isc = ldexp(1.0, e);
  }
}

// A row from its three sums over m: normalisation, noise weight, and the dirty-beam power by Parseval --
// sum_n d(n)^2 = (1/N) sum_k X_ext(k)^2 for d = irfft(X), the beam scaled by nrm.
__device__ __forceinline__ void rm_row_finish(double d, double q2, double p2, int nm, int N, double& nrm, double& wv, double& dbp) {
  const double mean = d / (double)nm;
  nrm = mean != 0.0 ? 1.0 / mean : 0.0;
  const double sv = 0.5 * nrm * nrm * q2;
  wv = sv != 0.0 ? 1.0 / sv : 0.0;
  dbp = nrm * nrm * p2 / (double)N / (double)N;
}

// One (el tile, 16 m, pol x freq) per block; EPL elevations per lane (1 is what ships).
// Per (m, el): the (+/-, ew) sums, the map / dirty-beam modes (to s_map / s_dirty, transposed through LDS so that
// rows are contiguous in m) and the block's share of the four sums over m that the FFT stage needs per row (RmSums), so
// that the FFT stage reads every mode once.
template <int EPL>
__global__ __launch_bounds__(kThreads) void k_rm_reduce(RmParams p) {
  constexpr int ET = 64 * EPL;
  __shared__ double2 tmap[MT][ET + 1];
  __shared__ double tdirty[MT][ET + 1];
  __shared__ double wsum[4][kThreads / 64][ET];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int el0 = blockIdx.x * ET, m0 = blockIdx.y * MT, pf = blockIdx.z;
  const int pol = pf / p.nfreq, f = pf - pol * p.nfreq;
  double acc_d[EPL], acc_q[EPL], acc_p[EPL], acc_x[EPL];
#pragma unroll
  for (int u = 0; u < EPL; ++u) acc_d[u] = acc_q[u] = acc_p[u] = acc_x[u] = 0.0;
  for (int mi = wave; mi < MT; mi += kThreads / 64) {
    const int m = m0 + mi;
    double sw[EPL], mre[EPL], mim[EPL], sg[EPL];
#pragma unroll
    for (int u = 0; u < EPL; ++u) sw[u] = mre[u] = mim[u] = sg[u] = 0.0;
    const int el = el0 + EPL * lane;
    if (m < p.nm) {  // (uniform over the wave)
      // The weights of the 2 x new (sign, EW separation) terms do not depend on the elevation: lane s * new + e works
      // out w and w^2 var once -- two float64 divisions -- and the row loop picks them up by shuffles, instead of every
      // lane repeating the divisions for every term (they were 40 % of the kernel's vector instructions).
      const int nterm = 2 * p.new_;
      double w_l = 0.0, g_l = 0.0;
      for (int t0 = 0; t0 < nterm; t0 += 64) {  // (one round unless there are more than 32 EW separations)
        const int t = t0 + lane;
        double w = 0.0, g = 0.0;
        if (t < nterm) rm_term_weight(p, m, pol, f, t, w, g);
        w_l = w;
        g_l = g;
        const int tend = nterm - t0 < 64 ? nterm - t0 : 64;
        const int elc = el < p.nel ? el : p.nel - EPL;  // lanes past the last elevation load a valid address
        for (int tt = 0; tt < tend; tt += kTermBatch) {  // a batch of terms: loads issued together, then consumed
          float2 h[kTermBatch][EPL], b[kTermBatch][EPL];
          double w2[kTermBatch], g2[kTermBatch];
#pragma unroll
          for (int k = 0; k < kTermBatch; ++k) {
            const bool live = tt + k < tend;
            const int tg = t0 + (live ? tt + k : tend - 1), s = tg / p.new_, e = tg - s * p.new_;
            const double wk = __shfl(w_l, live ? tt + k : 0, 64), gk = __shfl(g_l, live ? tt + k : 0, 64);
            w2[k] = live ? wk : 0.0;
            g2[k] = live ? gk : 0.0;
            const int64_t rbase = (((((int64_t)m * 2 + s) * p.npol + pol) * p.nfreq + f) * p.new_ + e) * p.nel + (elc < 0 ? 0 : elc);
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
              h[k][u] = p.hv[rbase + u];
              b[k][u] = p.bv[rbase + u];
            }
          }
#pragma unroll
          for (int k = 0; k < kTermBatch; ++k)
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
              const double br = b[k][u].x, bi = b[k][u].y, hr = h[k][u].x, hi = h[k][u].y;
              const double b2 = br * br + bi * bi;
              sw[u] = fma(w2[k], b2, sw[u]);
              mre[u] = fma(w2[k], br * hr + bi * hi, mre[u]);  // conj(b) * h
              mim[u] = fma(w2[k], br * hi - bi * hr, mim[u]);
              sg[u] = fma(g2[k], b2, sg[u]);
            }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < EPL; ++u) {
      double2 rm = make_double2(0.0, 0.0);
      double rd = 0.0;
      if (m < p.nm && el + u < p.nel) rm_mode(p, sw[u], mre[u], mim[u], sg[u], m, f, el + u, rm.x, rm.y, rd, acc_d[u], acc_q[u], acc_p[u], acc_x[u]);
      tmap[mi][EPL * lane + u] = rm;
      tdirty[mi][EPL * lane + u] = rd;
    }
  }
#pragma unroll
  for (int u = 0; u < EPL; ++u) {
    wsum[0][wave][EPL * lane + u] = acc_d[u];
    wsum[1][wave][EPL * lane + u] = acc_q[u];
    wsum[2][wave][EPL * lane + u] = acc_p[u];
    wsum[3][wave][EPL * lane + u] = acc_x[u];
  }
  __syncthreads();
  // this block's share of the per-row sums, waves added in a fixed order
  for (int e = threadIdx.x; e < ET; e += kThreads) {
    if (el0 + e < p.nel) {
      RmSums t = {wsum[0][0][e], wsum[1][0][e], wsum[2][0][e], wsum[3][0][e]};
#pragma unroll
      for (int w2 = 1; w2 < kThreads / 64; ++w2) {
        t.d += wsum[0][w2][e];
        t.q2 += wsum[1][w2][e];
        t.p2 += wsum[2][w2][e];
        t.x2 += wsum[3][w2][e];
      }
      p.psum[((int64_t)pf * p.nchunk + blockIdx.y) * p.nel + el0 + e] = t;
    }
  }
  // transposed store: rows (el) contiguous in m
  for (int idx = threadIdx.x; idx < ET * MT; idx += kThreads) {
    const int e = idx / MT, mi = idx - e * MT;
    if (el0 + e < p.nel && m0 + mi < p.nm) {
      const int64_t o = ((int64_t)pf * p.nel + el0 + e) * p.nm + m0 + mi;
      p.s_map[o] = tmap[mi][e];
      p.s_dirty[o] = tdirty[mi][e];
    }
  }
}

using RmFft = dmm_fft::RowFft<double>;  // the inverse transform of length nra (dmm_row_fft_plan)

// Hermitian extension to N bins of a row's map modes (complex) or dirty-beam modes (real, `d` only): what
// np.fft.irfft(x, n=N) transforms.  Bins 1..half are plain, N/2 (even N) is the real Nyquist bin.
__device__ __forceinline__ void rm_spec(const RmParams& p, int64_t row, int k, int N, int half, bool dirty, double& xr, double& xi) {
  xr = xi = 0.0;
  const int kk = k <= half || 2 * k == N ? k : N - k;
  if (kk >= p.nm) return;
  if (dirty) {
    xr = p.s_dirty[row * p.nm + kk];
    return;
  }
  const double2 v = p.s_map[row * p.nm + kk];
  xr = v.x;
  if (k != 0 && 2 * k != N) xi = k <= half ? v.y : -v.y;
}

// PAIR = 2: two rows per complex transform (z = X_map(row0) + i X_map(row1)); the dirty beam is not transformed at
// all -- its power comes from the modes by Parseval.  PAIR = 1 (the dirty beam is wanted in RA space): z = X_map + i
// X_dirty of one row, as before.  Either way a single inverse FFT yields two real outputs.
template <int PAIR>
__global__ __launch_bounds__(kThreads) void k_rm_fft(RmParams p, RmFft q) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int kRbMax = 8;  // (the plan's rb_max)
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  const bool blue = q.chirp != nullptr;
  const int N = p.nra, M = q.M, RB = q.RB, P = q.P;
  const int64_t nrow = (int64_t)p.npol * p.nfreq * p.nel;
  const int64_t t0 = (int64_t)blockIdx.x * RB;  // first transform of the block; transform t holds rows PAIR t (, +1)
  const C<double>* tw = dmm_fft::stage_twiddles<double, kThreads, true>(q, buf + (size_t)RB * P);
  const int half = (N - 1) / 2;
  // per transform and sequence: the row's normalisation, noise weight and dirty-beam power (PAIR = 2: sequence w is row
  // row0 + w; PAIR = 1: both are row0's), and the sequence's scale in and out of the transform (rm_seq_scale)
  __shared__ double s_nrm[kRbMax][2], s_wv[kRbMax][2], s_dbp[kRbMax][2], s_scl[kRbMax][2], s_isc[kRbMax][2];
  // per-row sums over m from the reduce stage's chunk partials: a wave per row, lanes over the chunks, then a butterfly
  // -- the same order every time
  for (int job = threadIdx.x >> 6; job < RB * PAIR; job += kThreads / 64) {
    const int r = job / PAIR, w2 = job - r * PAIR, ln = threadIdx.x & 63;
    const int64_t row = (t0 + r) * PAIR + w2;
    double d = 0.0, q2 = 0.0, p2 = 0.0, x2 = 0.0, d1 = 0.0;
    if (row < nrow) {
      const int64_t pf = row / p.nel;
      const int el = (int)(row - pf * p.nel);
      const int eln = p.skip ? p.iref : el;  // skip_deconvolution: normalised at the reference declination
      for (int c = ln; c < p.nchunk; c += 64) {
        d += p.psum[(pf * p.nchunk + c) * p.nel + eln].d;
        const RmSums t = p.psum[(pf * p.nchunk + c) * p.nel + el];
        q2 += t.q2;
        p2 += t.p2;
        x2 += t.x2;
        d1 += t.d;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      d += __shfl_xor(d, o, 64);
      q2 += __shfl_xor(q2, o, 64);
      p2 += __shfl_xor(p2, o, 64);
      x2 += __shfl_xor(x2, o, 64);
      d1 += __shfl_xor(d1, o, 64);
    }
    if (ln == 0) {  // (a row past the end: all zero)
      rm_row_finish(d, q2, p2, p.nm, N, s_nrm[r][w2], s_wv[r][w2], s_dbp[r][w2]);
      rm_seq_scale(x2, s_scl[r][w2], s_isc[r][w2]);
      // (the dirty-beam modes add up in phase at RA 0.  Beside the map it is that peak, the sum of the modes, that has to
      // be of the map's size: Bluestein's last product mixes the two, and the peak's rounding would be the map's error
      // there.  The beam's sidelobes in turn take the map's rounding, so the peak is left four times the map's norm.)
      if (PAIR == 1) rm_seq_scale(fmax(p2, 0.0625 * d1 * d1), s_scl[r][1], s_isc[r][1]);
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx / M, k = idx - r * M;
    C<double> v = {0.0, 0.0};
    const int64_t row0 = (t0 + r) * PAIR;
    if (k < N && row0 < nrow) {
      double ar, ai, br = 0.0, bi = 0.0;
      rm_spec(p, row0, k, N, half, false, ar, ai);
      if (PAIR == 2) {
        if (row0 + 1 < nrow) rm_spec(p, row0 + 1, k, N, half, false, br, bi);
      } else {
        rm_spec(p, row0, k, N, half, true, br, bi);
      }
      ar *= s_scl[r][0], ai *= s_scl[r][0], br *= s_scl[r][1], bi *= s_scl[r][1];
      // z = A + i B = (ar - bi) + i (ai + br); we load conj(z)
      v = {ar - bi, -(ai + br)};
      if (blue) v = dmm_fft::cmul<double>(v, {q.chirp[k].x, q.chirp[k].y});
    }
    buf[r * P + dmm_fft::inverse_slot(blue, k, q.logM)] = v;
  }
  __syncthreads();
  if (blue) {
    // (not dmm_fft::bluestein_convolve: spelt this way the compiler fuses the OTHER product of the filter multiply's
    // imaginary part -- fma(a.y, f.x, a.x f.y), the helper's call sites fma(f.y, a.x, f.x a.y) -- and moving over would
    // change the last bit of every Bluestein ring map)
    dmm_fft::fft_dif<double, kThreads>(buf, tw, RB, M, q.logM, P);
    for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
      const int r = idx / M, k = idx - r * M;
      buf[r * P + k] = dmm_fft::cmul<double>(buf[r * P + k], {q.bfilt[k].x, q.bfilt[k].y});
    }
    __syncthreads();
    dmm_fft::fft_dit<double, true, kThreads>(buf, tw, RB, M, q.logM, P);
  } else {
    dmm_fft::row_fft_inverse<double, kThreads>(q, false, buf, tw);
  }
  // finish: y = conj(result) / N; first output = Re y, second = Im y, each times its row's normalisation and its
  // sequence's scale
  __shared__ double red[kThreads];
  for (int r = 0; r < RB; ++r) {
    const int64_t row0 = (t0 + r) * PAIR;
    if (row0 >= nrow) break;  // uniform
    const double sc0 = s_nrm[r][0] / (double)N * s_isc[r][0], sc1 = s_nrm[r][PAIR - 1] / (double)N * s_isc[r][1];
    double pw = 0.0;
    for (int n = threadIdx.x; n < N; n += kThreads) {
      C<double> v = buf[r * P + n];
      if (blue) v = dmm_fft::cmul<double>(v, {q.chirp[n].x, q.chirp[n].y});
      p.tmp_map[row0 * N + n] = v.x * sc0;
      if (PAIR == 2) {
        if (row0 + 1 < nrow) p.tmp_map[(row0 + 1) * N + n] = -v.y * sc1;
      } else {
        const double dbv = -v.y * sc1;
        if (p.tmp_db) p.tmp_db[row0 * N + n] = dbv;
        pw += dbv * dbv;
      }
    }
    if (PAIR == 1) {  // dirty-beam power from the RA-space beam
      red[threadIdx.x] = pw;
      __syncthreads();
      for (int s2 = kThreads / 2; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < s2) red[threadIdx.x] += red[threadIdx.x + s2];
        __syncthreads();
      }
    }
    if (threadIdx.x < PAIR && row0 + threadIdx.x < nrow) {
      const int w2 = threadIdx.x;
      p.dbp[row0 + w2] = PAIR == 1 ? red[0] / (double)N : s_dbp[r][w2];
      p.wv[row0 + w2] = s_wv[r][w2];
    }
    __syncthreads();
  }
}

// ---- the three stages in ONE pass over the m-modes (power-of-two nra, RA-space dirty beam not asked for, own-row
// normalisation): a block owns EL elevations of one (pol, freq) for ALL m.  Its 16 waves read the (sign, EW) terms of
// 16 x 64 / EL m at a time -- lane = (m, el): pieces of 8 EL bytes of the hv / bv rows, each lane 2 x nterm loads in flight --,
// keep the sums in registers and put the map modes straight into the LDS image of the inverse FFT (two rows per complex
// sequence, bit-reversed positions: the even row's modes at the places of the bins m, the odd row's at those of the mirror
// bins N - m, combined into one sequence once both rows' norms are known); the per-row sums over m never leave the block.  After the in-LDS FFT the RA rows go out as pieces of map[ra][el] and weight[ra][el]:
// the [pol, el, m] modes and the [pol, el, ra] rows of the three-kernel form (1.34 GB of scratch traffic beside 2.69 GB
// of input and output at the CHIME-like shape) never reach HBM.
//   EL = 8 (round 3): 64-byte pieces.  Two blocks of neighbouring elevations share every 128-byte line of the input:
// block ids are mapped so that such a pair sits on the same XCD (same L2), 8 ids apart.
//   EL = 16 (round 4): HBM serves 128-byte lines: read in 64-byte pieces at a 4 KB stride -- what 8 elevations of
// complex64 are -- it delivers 3.0 TB/s, in 128-byte pieces 6.2 (tools/probe/piece_bw.hip), and 3.0 TB/s is exactly
// what the load phase of the 8-elevation form ran at.  So the block reads 128-byte pieces (lane = (m, 16 elevations)).
//   PARK = false: the image of all sixteen elevations fits the LDS (nra <= 1024): one transform of eight sequences,
// 128-byte pieces on the way out too.
//   PARK = true: the LDS holds the inverse-FFT image of 8 elevations, no more; the block puts the modes of elevations
// 0-7 into the LDS image and PARKS those of elevations 8-15 in a global scratch image (131 KB per block, 64-byte pieces
// in natural order; it lives in L2 / the Infinity Cache until it is read back), transforms and stores the first eight,
// reads the parked image in (bit reversal on the LDS side), transforms and stores the second eight.
constexpr int kFuThreads = 1024;
template <int EL, bool PARK>
__global__ __launch_bounds__(kFuThreads) void k_rm_fused(RmParams p, RmFft q, int ntile_el, double2* __restrict__ park) {
  static_assert(EL == 16 || (EL == 8 && !PARK), "8 or 16 elevations per block; only sixteen are ever parked");
  constexpr int kMW = 64 / EL;              // m per wave
  constexpr int kSeq = PARK ? 4 : EL / 2;   // sequences in the LDS image
  constexpr int kPass = PARK ? 2 : 1;       // passes over the tail
  constexpr int kElOut = PARK ? 8 : EL;     // elevations per output pass
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double s_acc[3][kFuThreads / 64][EL];
  __shared__ double s_nrm[EL], s_wv[EL], s_scl[EL], s_isc[EL];
  __shared__ double s_x2[kFuThreads / 64][2];  // the waves' shares of the norms of the sequences' two rows
  C<double>* buf = reinterpret_cast<C<double>*>(smem);  // [kSeq][P]
  C<double>* twl = buf + (size_t)kSeq * q.P;
  const int N = p.nra, M = q.M, P = q.P;
  int64_t tile_lin;
  if constexpr (EL == 8) {
    // block -> (pf, elevation tile): ids L and L + 8 (same XCD under round-robin dispatch) take neighbouring tiles
    const int L = blockIdx.x, grp = L >> 4, r16 = L & 15;
    tile_lin = (int64_t)2 * (grp * 8 + (r16 & 7)) + (r16 >> 3);
    if (tile_lin >= (int64_t)ntile_el * p.npol * p.nfreq) return;  // (grid rounded up to 16)
  } else {
    tile_lin = blockIdx.x;  // (grid = tiles exactly)
  }
  C<double>* const pk = reinterpret_cast<C<double>*>(park) + (size_t)blockIdx.x * 4 * N;
  const int pf = (int)(tile_lin / ntile_el), tile = (int)(tile_lin - (int64_t)pf * ntile_el);
  const int pol = pf / p.nfreq, f = pf - pol * p.nfreq;
  const int el0 = tile * EL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int eli = lane & (EL - 1), ms = lane / EL;  // EL elevations x 64 / EL m per wave
  const int el = el0 + eli;
  const bool el_ok = el < p.nel;
  const int elc = el_ok ? el : p.nel - 1;
  // (not dmm_fft::stage_twiddles: with it the allocator takes <16, true> from 117 registers to 128 and 12 bytes of scratch)
  for (int k = threadIdx.x; k < (M >> 1); k += kFuThreads) twl[k] = {q.tw[k].x, q.tw[k].y};
  const int nterm = 2 * p.new_;
  double acc_d = 0.0, acc_q = 0.0, acc_p = 0.0;
  // (measured, CHIME-like shape, EL = 8, 0.89 ms as it stands: the load phase alone takes 0.72 ms = 3.0 TB/s -- 64-byte
  // pieces are what the LDS allows, 8 elevations x 2048 RA x 16 bytes --; two m per lane and pass, i.e. 32 loads in flight
  // per lane: 0.93; the term weights from a table made by a pre-pass instead of in the loop: 0.95; blocks staggered over m
  // so that they do not read the same rows at the same time: 1.07 -- lock step is what keeps the DRAM pages open.)
  for (int mb = 0; mb < p.nm; mb += kMW * (kFuThreads / 64)) {
    const int m = mb + wave * kMW + ms;
    const bool m_ok = m < p.nm;
    const int mc = m_ok ? m : p.nm - 1;
    double sw = 0.0, mre = 0.0, mim = 0.0, sg = 0.0;
    for (int t0 = 0; t0 < nterm; t0 += kTermBatch) {
      // lane `eli & 7` of each 8-lane group works out the weights of term t0 + (eli & 7) of its m; the group's lanes pick
      // them up below (with EL = 16 both halves of an m work them out: each picks them up from its own)
      double w = 0.0, g = 0.0;
      if (t0 + (eli & 7) < nterm) rm_term_weight(p, mc, pol, f, t0 + (eli & 7), w, g);
      float2 h[kTermBatch], b[kTermBatch];
      double w2[kTermBatch], g2[kTermBatch];
#pragma unroll
      for (int k = 0; k < kTermBatch; ++k) {
        const bool live = t0 + k < nterm;
        const int tg = live ? t0 + k : nterm - 1, s = tg / p.new_, e = tg - s * p.new_;
        const double wk = __shfl(w, (lane & ~7) + k, 64), gk = __shfl(g, (lane & ~7) + k, 64);
        w2[k] = live ? wk : 0.0;
        g2[k] = live ? gk : 0.0;
        const int64_t rbase = (((((int64_t)mc * 2 + s) * p.npol + pol) * p.nfreq + f) * p.new_ + e) * p.nel + elc;
        h[k] = p.hv[rbase];
        b[k] = p.bv[rbase];
      }
#pragma unroll
      for (int k = 0; k < kTermBatch; ++k) {
        const double br = b[k].x, bi = b[k].y, hr = h[k].x, hi = h[k].y;
        const double b2 = br * br + bi * bi;
        sw = fma(w2[k], b2, sw);
        mre = fma(w2[k], br * hr + bi * hi, mre);  // conj(b) * h
        mim = fma(w2[k], br * hi - bi * hr, mim);
        sg = fma(g2[k], b2, sg);
      }
    }
    double ar = 0.0, ai = 0.0, rd;
    if (m_ok && el_ok) {  // (never launched with `skip`)
      double x2 = 0.0;  // (the norms of the rows are taken from the image below: an accumulator more in this loop spills)
      rm_mode(p, sw, mre, mim, sg, m, f, el, ar, ai, rd, acc_d, acc_q, acc_p, x2);
    }
    const bool edge = m == 0 || 2 * m == N;  // DC and Nyquist bins are real, and their own mirror
    // rows 2j (A) and 2j + 1 (B) share a transform, z = X_A + i X_B.  Their modes are put down side by side first -- A's at
    // the place of bin m, B's at the place of bin N - m; the real DC / Nyquist pair at the bin's own place -- and made
    // into z once the rows' scales are known (below)
    const double orr = __shfl_xor(ar, 1, 64);
    const bool odd = eli & 1;
    if (m_ok && !(edge && odd)) {
      const int mm = odd ? N - m : m;
      const C<double> v = {ar, edge ? orr : ai};
      if (!PARK || eli < 8) buf[(size_t)(eli >> 1) * P + dmm_fft::bitrev(mm, q.logM)] = v;  // the LDS image: bit-reversed positions
      else pk[(size_t)((eli - 8) >> 1) * N + mm] = v;  // elevations 8-15: parked in natural order, transformed second
    }
  }
  // the block's per-row sums over m: the m of a wave by a butterfly, the waves in a fixed order
#pragma unroll
  for (int o = EL; o < 64; o <<= 1) {
    acc_d += __shfl_xor(acc_d, o, 64);
    acc_q += __shfl_xor(acc_q, o, 64);
    acc_p += __shfl_xor(acc_p, o, 64);
  }
  if (ms == 0) {
    s_acc[0][wave][eli] = acc_d;
    s_acc[1][wave][eli] = acc_q;
    s_acc[2][wave][eli] = acc_p;
  }
  __syncthreads();
  if (threadIdx.x < EL) {
    double d = 0.0, q2 = 0.0, p2 = 0.0;
    for (int w2 = 0; w2 < kFuThreads / 64; ++w2) {
      d += s_acc[0][w2][threadIdx.x];
      q2 += s_acc[1][w2][threadIdx.x];
      p2 += s_acc[2][w2][threadIdx.x];
    }
    double dbp;
    rm_row_finish(d, q2, p2, p.nm, N, s_nrm[threadIdx.x], s_wv[threadIdx.x], dbp);
    if (el0 + (int)threadIdx.x < p.nel) p.dbp[(int64_t)pf * p.nel + el0 + threadIdx.x] = dbp;
  }
  __syncthreads();
  for (int pass = 0; pass < kPass; ++pass) {
    // the norms of the two rows of every sequence: kFuThreads / kSeq threads per sequence (whole waves), a butterfly per
    // wave, the waves in a fixed order.  (Measured, CHIME-like shape: this pass and the one after it cost 0.07 ms of 0.85 at
    // nra = 2048 -- parked form; 0.87 -> 0.95 with 8 elevations -- and 0.04 of 0.39 at nra = 1024.)
    if (pass == 1) __syncthreads();
    const int nh = N / 2 + 1;
    {
      constexpr int kTs = kFuThreads / kSeq;
      const int j = threadIdx.x / kTs;
      const C<double>* src = pass == 1 ? pk + (size_t)j * N : buf + (size_t)j * P;
      double xa = 0.0, xb = 0.0;
      for (int m = threadIdx.x - j * kTs; m < nh; m += kTs) {
        if (m == 0 || 2 * m == N) {
          const C<double> v = src[pass == 1 ? m : dmm_fft::bitrev(m, q.logM)];
          xa += v.x * v.x;
          xb += v.y * v.y;
        } else {
          const C<double> a = src[pass == 1 ? m : dmm_fft::bitrev(m, q.logM)], b = src[pass == 1 ? N - m : dmm_fft::bitrev(N - m, q.logM)];
          xa += 2.0 * (a.x * a.x + a.y * a.y);
          xb += 2.0 * (b.x * b.x + b.y * b.y);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        xa += __shfl_xor(xa, o, 64);
        xb += __shfl_xor(xb, o, 64);
      }
      if (lane == 0) s_x2[wave][0] = xa, s_x2[wave][1] = xb;
      __syncthreads();
      if (threadIdx.x < 2 * kSeq) {
        const int js = threadIdx.x >> 1, ab = threadIdx.x & 1;
        double x2 = 0.0;
        for (int w2 = js * (kTs / 64); w2 < (js + 1) * (kTs / 64); ++w2) x2 += s_x2[w2][ab];
        rm_seq_scale(x2, s_scl[kElOut * pass + threadIdx.x], s_isc[kElOut * pass + threadIdx.x]);
      }
      __syncthreads();
    }
    // the side-by-side modes of each pair of rows become the conjugated z of its transform, every row times its scale:
    // in place in the LDS image; from the parked image (coalesced reads, bit reversal on the LDS side) in the second pass
    for (int idx = threadIdx.x; idx < kSeq * nh; idx += kFuThreads) {
      const int j = idx / nh, m = idx - j * nh;
      const double sa = s_scl[kElOut * pass + 2 * j], sb = s_scl[kElOut * pass + 2 * j + 1];
      C<double>* row = buf + (size_t)j * P;
      const C<double>* src = pass == 1 ? pk + (size_t)j * N : nullptr;
      const int slot_a = dmm_fft::bitrev(m, q.logM), slot_b = dmm_fft::bitrev(N - m, q.logM);
      if (m == 0 || 2 * m == N) {  // (A_r, B_r) -> conj(A_r + i B_r)
        const C<double> v = pass == 1 ? src[m] : row[slot_a];
        row[slot_a] = {v.x * sa, -(v.y * sb)};
      } else {
        C<double> a = pass == 1 ? src[m] : row[slot_a], b = pass == 1 ? src[N - m] : row[slot_b];
        a = {a.x * sa, a.y * sa};
        b = {b.x * sb, b.y * sb};
        row[slot_a] = {a.x - b.y, -(a.y + b.x)};  // bin m: conj(X_A + i X_B)
        row[slot_b] = {a.x + b.y, a.y - b.x};     // bin N - m: conj(conj(X_A) + i conj(X_B))
      }
    }
    __syncthreads();
    dmm_fft::fft_dit<double, false, kFuThreads>(buf, twl, kSeq, M, q.logM, P);
    // y = conj(result) / N: even row = Re, odd row = -Im, each times its row's normalisation; pieces of 8 kElOut bytes of [ra][el]
    const int eo = threadIdx.x & (kElOut - 1);
    const int ele = el0 + kElOut * pass + eo;
    const double sc = s_nrm[kElOut * pass + eo] / (double)N * s_isc[kElOut * pass + eo], wv = s_wv[kElOut * pass + eo];
    if (ele < p.nel)
      for (int ra = threadIdx.x / kElOut; ra < N; ra += kFuThreads / kElOut) {
        const C<double> v = buf[(size_t)(eo >> 1) * P + ra];
        const int64_t o = ((int64_t)pf * p.nra + ra) * p.nel + ele;
        p.map[o] = (eo & 1) ? -v.y * sc : v.x * sc;
        p.weight[o] = wv;
      }
  }
}

// [pf][el][ra] -> map[pf][ra][el] (+ dirty beam), weight[pf][ra][el] = wv[pf][el]; 32x32 tiles
__global__ __launch_bounds__(kThreads) void k_rm_store(RmParams p) {
  __shared__ double ta[32][33], tb[32][33];
  const int pf = blockIdx.z;
  const int ra0 = blockIdx.x * 32, el0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int el = el0 + j, ra = ra0 + tx;
    if (el < p.nel && ra < p.nra) {
      const int64_t o = ((int64_t)pf * p.nel + el) * p.nra + ra;
      ta[j][tx] = p.tmp_map[o];
      if (p.db) tb[j][tx] = p.tmp_db[o];
    }
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int ra = ra0 + j, el = el0 + tx;
    if (el < p.nel && ra < p.nra) {
      const int64_t o = ((int64_t)pf * p.nra + ra) * p.nel + el;
      p.map[o] = ta[tx][j];
      if (p.db) p.db[o] = tb[tx][j];
      p.weight[o] = p.wv[(int64_t)pf * p.nel + el];
    }
  }
}

// Which kernels take a call: the three-kernel form, or a single pass with 8 / 16 / 16 (second eight parked) elevations
// per block.
enum RmForm { kRmThreeKernel, kRmSingle8, kRmSingle16, kRmSingle16Parked };

// The form of a call the single pass can take.  "ringmap_variant" = 1: the three-kernel form, 2: the 8-elevation form.
// The parked half of the image is 131 KB per block at nra = 2048 and is indexed by TILE: it grows with nfreq npol nel, and
// the form only pays while it stays in the Infinity Cache (256 MiB) -- beyond that the 8-elevation form takes the call
// (0.5 GB of scratch at 4096 tiles, kept by the context)
RmForm rm_single_pass_form(bool lds16_fits, size_t park_bytes, int variant) {
  if (variant == 1) return kRmThreeKernel;
  if (variant == 2) return kRmSingle8;
  if (lds16_fits) return kRmSingle16;
  return park_bytes <= ((size_t)192 << 20) ? kRmSingle16Parked : kRmSingle8;
}

// window[f, m, el] = sum_i coef_i cos(2 pi i x), x = (m - min_m[f, el]) / (max_m[f, el] - min_m[f, el]), zero outside
// [0, 1] and wherever max_m <= min_m (window_generalised, reference draco/util/tools.py:547-601, as used at ringmapmaker.py:917-925); float64
// arithmetic, stored float32 like the reference's `.astype(np.float32)`
__global__ void k_rm_window(int nfreq, int nm, int nel, const double* __restrict__ min_m, const double* __restrict__ max_m,
                            double c0, double c1, double c2, double c3, float* __restrict__ out) {
  const int64_t n = (int64_t)nfreq * nm * nel;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int el = (int)(idx % nel);
    const int64_t fm = idx / nel;
    const int m = (int)(fm % nm), f = (int)(fm / nm);
    const double lo = min_m[(int64_t)f * nel + el], hi = max_m[(int64_t)f * nel + el];
    const double x = ((double)m - lo) / (hi - lo);
    double w = 0.0;
    if (hi > lo && x >= 0.0 && x <= 1.0) {  // (hi < lo: the reference selects lo <= m <= hi first, an empty window)
      const double t = 2.0 * M_PI * x;
      w = c0 + c1 * cos(t) + c2 * cos(2.0 * t) + c3 * cos(3.0 * t);
    }
    out[idx] = (float)w;
  }
}

}  // namespace

extern "C" int dmm_ringmap_deconvolve(dmm_ctx* ctx, int nm, int nm_beam, int npol, int nfreq, int new_, int nel,
                                      int nra, int weight_mode, int skip_deconvolution, int iref, const void* hv,
                                      const float* hw, const void* bv, const double* ew_table, const double* eps,
                                      const float* window, double* map, double* weight, double* dirty_beam_power,
                                      double* dirty_beam) {
  DMM_REQUIRE(ctx && hv && hw && bv && ew_table && eps && map && weight && dirty_beam_power,
              "dmm_ringmap_deconvolve: NULL argument");
  DMM_REQUIRE(nm >= 1 && nm_beam >= nm && npol >= 1 && nfreq >= 1 && new_ >= 1 && nel >= 1,
              "dmm_ringmap_deconvolve: bad sizes (beam must have at least as many m as the visibilities)");
  DMM_REQUIRE(nra == 2 * (nm - 1) || nra == 2 * (nm - 1) + 1, "dmm_ringmap_deconvolve: nra=%d is not 2*mmax (+1)", nra);
  DMM_REQUIRE(nra >= 1, "dmm_ringmap_deconvolve: nra must be positive (mmax = 0 needs oddra)");
  DMM_REQUIRE(weight_mode >= 0 && weight_mode <= 2, "dmm_ringmap_deconvolve: bad weight_mode %d", weight_mode);
  DMM_REQUIRE(!skip_deconvolution || (iref >= 0 && iref < nel), "dmm_ringmap_deconvolve: iref out of range");
  DMM_HIP(hipSetDevice(ctx->device));
  // the three-kernel form's transforms: up to 8 per block in 72 KB of LDS, twiddles from memory where a row leaves no room
  constexpr size_t kLdsLimit = 150 * 1024;
  const int64_t nrow = (int64_t)npol * nfreq * nel, ntrans = dirty_beam ? nrow : (nrow + 1) / 2;  // (two rows per transform)
  RmFft q;
  size_t lds = 0;
  bool fits = false;
  int rc = dmm_row_fft_plan<double>(ctx, nra, ntrans, {8, 72 * 1024, kLdsLimit, true, false}, &q, &lds, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_ringmap_deconvolve: nra=%d too long for the in-LDS FFT", nra);
  const size_t tw_b = (size_t)(q.M / 2) * sizeof(double2);

  RmParams p;
  p.nm = nm;
  p.nm_beam = nm_beam;
  p.npol = npol;
  p.nfreq = nfreq;
  p.new_ = new_;
  p.nel = nel;
  p.nra = nra;
  p.mmax = nm - 1;
  p.mode = weight_mode;
  p.skip = skip_deconvolution;
  p.iref = iref;
  p.hv = (const float2*)hv;
  p.hw = hw;
  p.bv = (const float2*)bv;
  p.wt = ew_table;
  p.eps = eps;
  p.window = window;
  p.dbp = dirty_beam_power;
  p.map = map;
  p.weight = weight;
  p.db = dirty_beam;
  // one pass over the m-modes where the whole inverse FFT of 8 elevations fits the LDS (power-of-two nra up to 2048)
  const size_t fused_lds = (size_t)4 * q.P * sizeof(double2) + tw_b;
  const size_t lds16 = (size_t)8 * q.P * sizeof(double2) + tw_b;  // all sixteen elevations' image in the LDS?
  const int64_t ntile16 = (int64_t)((nel + 15) / 16) * npol * nfreq;
  const size_t park_bytes = (size_t)ntile16 * 4 * nra * sizeof(double2);
  const bool single_ok = !dirty_beam && !skip_deconvolution && !q.chirp && nra >= 8 && fused_lds <= kLdsLimit;
  const RmForm form = single_ok ? rm_single_pass_form(lds16 <= kLdsLimit, park_bytes, ctx->opt_ringmap_variant) : kRmThreeKernel;
  if (form != kRmThreeKernel) {
    const int el_blk = form == kRmSingle8 ? 8 : 16;
    const int ntile_el = (nel + el_blk - 1) / el_blk;
    const int64_t ntile = (int64_t)ntile_el * npol * nfreq;
    void* park = nullptr;
    switch (form) {
      case kRmSingle8:  // (the grid in whole groups of 16 ids: the XCD pairing of the tiles)
        return dmm_launch_blocks("dmm_ringmap_deconvolve", k_rm_fused<8, false>, (ntile + 15) / 16 * 16, kFuThreads, fused_lds, ctx->stream, p, q,
                                 ntile_el, (double2*)nullptr);
      case kRmSingle16:
        return dmm_launch_blocks("dmm_ringmap_deconvolve", k_rm_fused<16, false>, ntile, kFuThreads, lds16, ctx->stream, p, q, ntile_el,
                                 (double2*)nullptr);
      default:  // kRmSingle16Parked
        rc = dmm_get_scratch(ctx, park_bytes + 256, &park);
        if (rc) return rc;
        return dmm_launch_blocks("dmm_ringmap_deconvolve", k_rm_fused<16, true>, ntile, kFuThreads, fused_lds, ctx->stream, p, q, ntile_el,
                                 (double2*)park);
    }
  }
  const int nchunk = (nm + MT - 1) / MT;
  const size_t b_map = (size_t)nrow * nm * sizeof(double2);
  const size_t b_dirty = ((size_t)nrow * nm * sizeof(double) + 255) / 256 * 256;
  const size_t b_psum = ((size_t)npol * nfreq * nchunk * nel * sizeof(RmSums) + 255) / 256 * 256;
  const size_t b_vec = ((size_t)nrow * sizeof(double) + 255) / 256 * 256;
  const size_t b_tmp = (size_t)nrow * nra * sizeof(double);
  void* scratch = nullptr;
  rc = dmm_get_scratch(ctx, b_map + b_dirty + b_psum + b_vec + (dirty_beam ? 2 : 1) * b_tmp + 1024, &scratch);
  if (rc) return rc;
  unsigned char* sp = (unsigned char*)scratch;
  p.nchunk = nchunk;
  p.s_map = (double2*)sp;
  sp += b_map;
  p.s_dirty = (double*)sp;
  sp += b_dirty;
  p.psum = (RmSums*)sp;
  sp += b_psum;
  p.wv = (double*)sp;
  sp += b_vec;
  p.tmp_map = (double*)sp;
  sp += b_tmp;
  p.tmp_db = dirty_beam ? (double*)sp : nullptr;

  // (two elevations per lane with 16-byte loads were tried: 715 instead of 630 us for this kernel at the CHIME-like
  // shape -- half as many resident waves; the kernel is latency bound on its 16 loads per m)
  hipLaunchKernelGGL(k_rm_reduce<1>, dim3((nel + 63) / 64, nchunk, npol * nfreq), dim3(kThreads), 0, ctx->stream, p);
  rc = dmm_launch_blocks("dmm_ringmap_deconvolve", dirty_beam ? k_rm_fft<1> : k_rm_fft<2>, (ntrans + q.RB - 1) / q.RB, kThreads, lds,
                         ctx->stream, p, q);
  if (rc) return rc;
  hipLaunchKernelGGL(k_rm_store, dim3((nra + 31) / 32, (nel + 31) / 32, npol * nfreq), dim3(kThreads), 0, ctx->stream, p);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

extern "C" int dmm_ringmap_window(dmm_ctx* ctx, int nfreq, int nm, int nel, const double* min_m, const double* max_m,
                                  const double* coef /*[host] 4*/, float* window) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ringmap_window: ctx is NULL");
  DMM_REQUIRE(nfreq >= 0 && nm >= 0 && nel >= 0, "dmm_ringmap_window: bad sizes nfreq=%d nm=%d nel=%d", nfreq, nm, nel);
  const int64_t n = (int64_t)nfreq * nm * nel;
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(min_m && max_m && coef && window, "dmm_ringmap_window: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 65536);
  hipLaunchKernelGGL(k_rm_window, dim3(blocks), dim3(256), 0, ctx->stream, nfreq, nm, nel, min_m, max_m, coef[0], coef[1], coef[2],
                     coef[3], window);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}
