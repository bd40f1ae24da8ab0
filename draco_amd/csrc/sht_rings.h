// SHT stage 2 / 1': the per-ring Fourier transforms (in-LDS FFT for the belt, Bluestein for the polar
// caps, direct sums as fallback and cross-check).  Included by sht.hip only.
#pragma once
#include "sht_common.h"

namespace {

// ---------------------------------------------------------------- ring stages (2 and 1')
struct RingParams {
  ShtGeom g;
  int nf, npol;
  double2* b;     // [nf, npol, nring, mmax+1]; the NPOL = 4 synthesis: frequency-grouped (syn4_at)
  double* map;    // [nf, npol, npix]
  int64_t npix;
  const double* map_ref;  // analysis only, or nullptr: the field analysed is map_ref - map (the residual of a Jacobi iteration of
                          // map2alm, formed on the way in instead of by a pass of its own over the maps)
  int stage_all;          // synthesis: 1 = every ring stages the rotated coefficients of a pass in LDS (k_ring_synth_fft), 0 = the aliased ones
};

// A launch covers one CLASS of rings that share an FFT length:
//   belt:  rings nside .. 3 nside (nphi = 4 nside, a power of two): plain FFT, M = nphi
//   cap:   ring numbers ir in [r_lo, r_hi] of BOTH caps (nphi = 4 ir): Bluestein with M = the
//          class's power of two >= 2 nphi - 1 (at least kMinBlue, so the tiny rings share a class)
struct RingClass {
  int belt;        // 1: equatorial belt
  int r_lo, r_hi;  // cap ring numbers (1-based), inclusive
  int M, logM;
};
constexpr int kMinBlue = 256, kMaxBlue = 4096;

__host__ __device__ __forceinline__ int blue_len(int ir) {  // Bluestein FFT length of cap ring number ir
  int M = kMinBlue;
  while (M < 8 * ir - 1) M <<= 1;
  return M;
}

__device__ __forceinline__ int class_ring(const RingClass& rc, const ShtGeom& g, int i) {
  if (rc.belt) return g.nside - 1 + i;
  const int ir = rc.r_lo + (i >> 1);
  return (i & 1) ? g.nring - ir : ir - 1;  // south : north
}

// direct evaluation, block = (ring of the class, f): map(j) = Re sum_m fac_m b_m e^{i m phi_j}.
// Fallback for rings whose FFT does not fit the LDS (nside > 512) and the check of the FFT path.
// The phasor of the direct sums is rotated step by step; the rotation's rounding error grows with the number of steps
// (over the 4092 pixels of a cap ring of nside 1024 the analysis was 17 times as far from a long-double evaluation as
// float64 NumPy), so it restarts from sincospi of the exactly reduced angle every kDirectRun steps.  Sums of at most
// kDirectRun terms keep the values they had.
constexpr int kDirectRun = 64;
template <int NPOL>
__global__ __launch_bounds__(kThreads) void k_ring_synth(RingParams p, RingClass rc) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* c = reinterpret_cast<double2*>(smem);  // [NPOL][mmax+1]
  const int ring = class_ring(rc, p.g, blockIdx.x);
  const int f = blockIdx.y;
  const int nm = p.g.mmax + 1;
  const double phi0 = p.g.phi0[ring];
  const int nphi = p.g.nphi[ring];
  for (int idx = threadIdx.x; idx < NPOL * nm; idx += kThreads) {
    const int pol = idx / nm, m = idx - pol * nm;
    double2 v;
    if (NPOL == 1) {
      v = p.b[((int64_t)f * p.g.nring + ring) * nm + m];
    } else {  // the frequency-grouped scratch (syn4_at)
      const double* q = reinterpret_cast<const double*>(p.b) + syn4_at(f, m, ring, pol >> 1, p.g.nring, nm) + syn4_slot(pol);
      v = make_double2(q[0], q[2]);
    }
    double sn, cs;
    sincos((double)m * phi0, &sn, &cs);
    const double fac = m == 0 ? 1.0 : 2.0;
    c[idx] = make_double2(fac * (v.x * cs - v.y * sn), fac * (v.x * sn + v.y * cs));
  }
  __syncthreads();
  const int64_t base = p.g.start[ring];
  for (int j = threadIdx.x; j < nphi; j += kThreads) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)nphi, &sn, &cs);
    double acc[NPOL];
#pragma unroll
    for (int q = 0; q < NPOL; ++q) acc[q] = 0.0;
    for (int m0 = 0; m0 < nm; m0 += kDirectRun) {
      double pr, pi_;  // e^{2 pi i m0 j / nphi}, then rotated by one pixel step per m
      sincospi(2.0 * (double)(((int64_t)m0 * j) % nphi) / (double)nphi, &pi_, &pr);
      const int m1 = min(m0 + kDirectRun, nm);
      for (int m = m0; m < m1; ++m) {
#pragma unroll
        for (int q = 0; q < NPOL; ++q) {
          const double2 cm = c[q * nm + m];
          acc[q] = fma(cm.x, pr, fma(-cm.y, pi_, acc[q]));
        }
        const double nr = pr * cs - pi_ * sn;
        pi_ = fma(pr, sn, pi_ * cs);
        pr = nr;
      }
    }
#pragma unroll
    for (int q = 0; q < NPOL; ++q) p.map[((int64_t)f * NPOL + q) * p.npix + base + j] = acc[q];
  }
}

// ---- FFT ring stages.  A ring of N = nphi pixels is a length-N DFT: a plain in-LDS FFT when N
// is a power of two (the belt), Bluestein's chirp-z otherwise (the caps):
//   X_j = c_j * sum_k (x_k c_k) conj(c)_{j-k},  c_k = exp(-i pi k^2 / N)
// i.e. multiply by the chirp, FFT_M, multiply by the precomputed spectrum of the wrapped conjugate
// chirp (ShtGeom::bfilt, stored in the DIF kernel's bit-reversed order and scaled by 1/M),
// inverse FFT_M, multiply by the chirp.  TWO real fields ride one complex transform.
constexpr int kFftThreads = 256;

struct RingLds {
  dmm_fft::C<double>* buf;    // [NROW][M + 1]
  dmm_fft::C<double>* tw;     // [M / 2]   exp(-2 pi i k / M)
  dmm_fft::C<double>* chirp;  // [N]       (Bluestein only)
};

// (twiddles and chirp are copied from the geometry's tables: same values as computing them here, none of the cost)
template <int NROW, bool BLUE>
__device__ __forceinline__ RingLds ring_lds(unsigned char* smem, const ShtGeom& g, int N, int M) {
  RingLds l;
  l.buf = reinterpret_cast<dmm_fft::C<double>*>(smem);
  l.tw = l.buf + NROW * (M + 1);
  l.chirp = l.tw + (M >> 1);
  const int stride = g.tw_len / M;
  for (int k = threadIdx.x; k < (M >> 1); k += kFftThreads) {
    const double2 t = g.tw[k * stride];
    l.tw[k] = {t.x, t.y};
  }
  if (BLUE) {
    const int ir = N >> 2;
    const double2* src = g.chirp + (int64_t)2 * ir * (ir - 1);
    for (int k = threadIdx.x; k < N; k += kFftThreads) {
      const double2 t = src[k];
      l.chirp[k] = {t.x, t.y};
    }
  }
  return l;
}

// geometry build: block b < nring fills the phase row of ring b, block nring the twiddles, block nring + ir the chirp
// of cap ring number ir.  The expressions are the ones the ring kernels evaluated in place before.
__global__ void k_fill_ring_tables(const double* phi0, int nring, int mmax, double2* phase, double2* tw, int tw_len,
                                   double2* chirp) {
  const int b = blockIdx.x;
  if (b < nring) {
    const double p0 = phi0[b];
    for (int m = threadIdx.x; m <= mmax; m += blockDim.x) {
      double sn, cs;
      sincos((double)m * p0, &sn, &cs);
      phase[(int64_t)b * (mmax + 1) + m] = make_double2(cs, sn);
    }
  } else if (b == nring) {
    for (int k = threadIdx.x; k < tw_len / 2; k += blockDim.x) {
      double sn, cs;
      sincospi(-2.0 * (double)k / (double)tw_len, &sn, &cs);
      tw[k] = make_double2(cs, sn);
    }
  } else {
    const int ir = b - nring, N = 4 * ir;
    double2* dst = chirp + (int64_t)2 * ir * (ir - 1);
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
      const int k2 = (int)(((int64_t)k * k) % (2 * (int64_t)N));  // exact phase reduction
      double sn, cs;
      sincospi(-(double)k2 / (double)N, &sn, &cs);
      dst[k] = make_double2(cs, sn);
    }
  }
}

// forward DFT_N of the NROW rows in l.buf (natural order, already multiplied by the chirp and
// zero-padded to M when BLUE).  Afterwards X_k is ring_dft_at(l, r, k).  (The transforms with three stages per pass.)
template <int NROW, bool BLUE>
__device__ __forceinline__ void ring_dft(const RingLds& l, const double2* bfilt, int M, int logM) {
  const int P = M + 1;
  if (BLUE) dmm_fft::bluestein_convolve<double, kFftThreads>(l.buf, l.tw, bfilt, NROW, M, logM, P, true);
  else dmm_fft::fft_dif8<double, kFftThreads>(l.buf, l.tw, NROW, M, logM, P);
}

template <bool BLUE>
__device__ __forceinline__ dmm_fft::C<double> ring_dft_at(const RingLds& l, int r, int k, int M, int logM) {
  if (BLUE) return dmm_fft::cmul<double>(l.buf[r * (M + 1) + k], l.chirp[k]);
  return l.buf[r * (M + 1) + dmm_fft::bitrev(k, logM)];
}

// Synthesis: the Hermitian spectrum H_k = b_k e^{i k phi0} (k <= mmax), H_{N-k} = conj(H_k),
// folded modulo N, makes the map real, so two polarisations ride one transform:
// z = H_a + i H_b  ->  IDFT(z) = map_a + i map_b, and IDFT(z) = conj(DFT(conj z)).
// NPOL = 4: block = (ring of the class, frequency group, transform r = blockIdx.z), r = 0 carrying (T, Q) and r = 1 (U, V);
// the group's kSynF frequencies are NB complex transforms at a time, and the block reads one contiguous run of the
// frequency-grouped scratch (128 bytes per m).  NPOL = 1: block = (ring, frequency), one transform (NB = 1).
// Rings shorter than the band limit (n < nm) alias many m onto one k: there (and on every ring of a launch with
// p.stage_all, whose loads are then coalesced) the phase rotation of a pass's frequencies runs in parallel over m first, into
// LDS, and the fold below only adds (a fixed order, so still reproducible); the other rings rotate each row where the fold
// reads it.  Same operations in the same order per transform either way.
template <int NPOL, int NB, bool BLUE>
__global__ __launch_bounds__(kFftThreads) void k_ring_synth_fft(RingParams p, RingClass rc) {
  using dmm_fft::C;
  constexpr int KF = NPOL == 4 ? kSynF : 1;  // frequencies of a block
  static_assert(KF % NB == 0, "passes of NB transforms");
  extern __shared__ __align__(16) unsigned char smem[];
  const int ring = class_ring(rc, p.g, blockIdx.x), r = NPOL == 4 ? (int)blockIdx.z : 0;
  const int f0 = KF * blockIdx.y, nfb = min(KF, p.nf - f0);  // the block's frequencies f0 .. f0 + nfb - 1 of the chunk
  const int n = p.g.nphi[ring], M = rc.M, P = M + 1;
  const RingLds l = ring_lds<NB, BLUE>(smem, p.g, n, M);
  if (BLUE) __syncthreads();  // the chirp is used by the load below
  const int nm = p.g.mmax + 1;
  const double2* phase = p.g.phase + (int64_t)ring * nm;  // e^{i m phi0} of this ring
  // (b_m of the transform's two polarisations a, b) of frequency f0 + fi.  NPOL = 4: slots (T, Q) of r = 0, (V, U) of r = 1
  auto load = [&](int fi, int m, double2& va, double2& vb) {
    if (NPOL == 1) {
      va = p.b[((int64_t)(f0 + fi) * p.g.nring + ring) * nm + m];
    } else {
      const double* q = reinterpret_cast<const double*>(p.b) + syn4_at(f0 + fi, m, ring, r, p.g.nring, nm);
      const double2 re = *reinterpret_cast<const double2*>(q), im = *reinterpret_cast<const double2*>(q + 2);
      va = r == 0 ? make_double2(re.x, im.x) : make_double2(re.y, im.y);
      vb = r == 0 ? make_double2(re.y, im.y) : make_double2(re.x, im.x);
    }
  };
  const bool staged = p.stage_all || n < nm;
  C<double>* rot = l.chirp + (BLUE ? 4 * rc.r_hi : 0);  // [NB][2][nm], present when the class has staged rings
  const double2* bfilt = BLUE ? p.g.bfilt + p.g.bf_off[rc.belt ? 0 : rc.r_lo + ((int)blockIdx.x >> 1)] : nullptr;
  const int64_t base = p.g.start[ring];
  // passes of NB transforms: the block's later passes read their slots of the lines its first pass brought in (L2)
  for (int fb = 0; fb < nfb; fb += NB) {
    if (fb > 0) __syncthreads();  // the previous pass reads rot and l.buf until here
    if (staged) {
      // thread <-> (m, frequency of the pass): the block's run of the scratch is read front to back
      for (int q = threadIdx.x; q < NB * nm; q += kFftThreads) {
        const int m = q / NB, j = q - m * NB;
        C<double> a = {0.0, 0.0}, b = {0.0, 0.0};
        if (fb + j < nfb) {  // (slots beyond the chunk's last frequency are neither read nor stored)
          const double2 ph = phase[m];
          const double cs = ph.x, sn = ph.y;
          double2 va, vb;
          load(fb + j, m, va, vb);
          a = {va.x * cs - va.y * sn, va.x * sn + va.y * cs};
          if (NPOL == 4) b = {vb.x * cs - vb.y * sn, vb.x * sn + vb.y * cs};
          if (m == 0) a.y = b.y = 0.0;  // the m = 0 term of a real field is real
        }
        rot[(j * 2 + 0) * nm + m] = a;
        rot[(j * 2 + 1) * nm + m] = b;
      }
      __syncthreads();
    }
    for (int k = threadIdx.x; k < M; k += kFftThreads) {
      double zr[NB], zi[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) zr[j] = zi[j] = 0.0;
      if (k < n && staged) {
        for (int m = k; m < nm; m += n) {  // direct terms: z += H_a + i H_b
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const C<double> a = rot[(j * 2 + 0) * nm + m], b = rot[(j * 2 + 1) * nm + m];
            zr[j] += a.x - b.y;
            zi[j] += a.y + b.x;
          }
        }
        for (int m = (k == 0 ? n : n - k); m < nm; m += n) {  // mirrored terms: z += conj(H_a) + i conj(H_b)
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const C<double> a = rot[(j * 2 + 0) * nm + m], b = rot[(j * 2 + 1) * nm + m];
            zr[j] += a.x + b.y;
            zi[j] += b.x - a.y;
          }
        }
      } else if (k < n) {
        // direct terms m == k (mod n)
        for (int m = k; m < nm; m += n) {
          const double2 ph = phase[m];
          const double cs = ph.x, sn = ph.y;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            if (fb + j >= nfb) continue;
            double2 va, vb;
            load(fb + j, m, va, vb);
            double ar = va.x * cs - va.y * sn, ai = va.x * sn + va.y * cs;
            double br = 0.0, bi = 0.0;
            if (NPOL == 4) {
              br = vb.x * cs - vb.y * sn;
              bi = vb.x * sn + vb.y * cs;
            }
            if (m == 0) ai = bi = 0.0;  // the m = 0 term of a real field is real
            zr[j] += ar - bi;           // z = H_a + i H_b
            zi[j] += ai + br;
          }
        }
        // mirrored terms m == -k (mod n), m >= 1: conj(H_a) + i conj(H_b)
        for (int m = (k == 0 ? n : n - k); m < nm; m += n) {
          const double2 ph = phase[m];
          const double cs = ph.x, sn = ph.y;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            if (fb + j >= nfb) continue;
            double2 va, vb;
            load(fb + j, m, va, vb);
            const double ar = va.x * cs - va.y * sn, ai = va.x * sn + va.y * cs;
            double br = 0.0, bi = 0.0;
            if (NPOL == 4) {
              br = vb.x * cs - vb.y * sn;
              bi = vb.x * sn + vb.y * cs;
            }
            zr[j] += ar + bi;  // conj(a) + i conj(b) = (ar + bi) + i(br - ai)
            zi[j] += br - ai;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        C<double> v = {zr[j], -zi[j]};  // conj(z)
        if (BLUE && k < n) v = dmm_fft::cmul<double>(v, l.chirp[k]);
        l.buf[j * P + k] = v;
      }
    }
    __syncthreads();
    ring_dft<NB, BLUE>(l, bfilt, M, rc.logM);
    for (int j = threadIdx.x; j < n; j += kFftThreads) {
#pragma unroll
      for (int jj = 0; jj < NB; ++jj) {
        if (fb + jj >= nfb) continue;
        const int64_t f = f0 + fb + jj;
        const C<double> y = ring_dft_at<BLUE>(l, jj, j, M, rc.logM);  // IDFT(z)_j = conj(y)
        p.map[(f * NPOL + 2 * r) * p.npix + base + j] = y.x;
        if (NPOL == 4) p.map[(f * NPOL + 2 * r + 1) * p.npix + base + j] = -y.y;
      }
    }
  }
}

// ---------------------------------------------------------------- analysis, stage 1'
// direct evaluation, block = (ring of the class, f): g_m = w * sum_j map_j e^{-i m phi_j};
// thread <-> m, pixels broadcast from LDS.  Fallback / check, as k_ring_synth.
template <int NPOL>
__global__ __launch_bounds__(kThreads) void k_ring_anal(RingParams p, RingClass rc) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* px = reinterpret_cast<double*>(smem);  // [NPOL][nphi]
  const int ring = class_ring(rc, p.g, blockIdx.x), f = blockIdx.y;
  const int nm = p.g.mmax + 1;
  const double phi0 = p.g.phi0[ring];
  const int nphi = p.g.nphi[ring];
  const int64_t base = p.g.start[ring];
  for (int idx = threadIdx.x; idx < NPOL * nphi; idx += kThreads) {
    const int pol = idx / nphi, j = idx - pol * nphi;
    const int64_t pi = ((int64_t)f * NPOL + pol) * p.npix + base + j;
    px[idx] = p.map_ref ? p.map_ref[pi] - p.map[pi] : p.map[pi];
  }
  __syncthreads();
  const double w = 4.0 * M_PI / (double)p.npix;
  for (int m = threadIdx.x; m < nm; m += kThreads) {
    // e^{-i m phi_j} = e^{-i m phi0} * step^j, step = e^{-2 pi i m / nphi} (m reduced mod nphi exactly)
    const int mr = m % nphi;
    double sn, cs;
    sincospi(-2.0 * (double)mr / (double)nphi, &sn, &cs);
    double are[NPOL], aim[NPOL];
#pragma unroll
    for (int q = 0; q < NPOL; ++q) are[q] = aim[q] = 0.0;
    for (int j0 = 0; j0 < nphi; j0 += kDirectRun) {
      double pr, pi_;  // step^j0, then rotated by one step per pixel
      sincospi(-2.0 * (double)(((int64_t)mr * j0) % nphi) / (double)nphi, &pi_, &pr);
      const int j1 = min(j0 + kDirectRun, nphi);
      for (int j = j0; j < j1; ++j) {
#pragma unroll
        for (int q = 0; q < NPOL; ++q) {
          const double v = px[q * nphi + j];
          are[q] = fma(v, pr, are[q]);
          aim[q] = fma(v, pi_, aim[q]);
        }
        const double nr = pr * cs - pi_ * sn;
        pi_ = fma(pr, sn, pi_ * cs);
        pr = nr;
      }
    }
    double s0, c0;
    sincos(-(double)m * phi0, &s0, &c0);
#pragma unroll
    for (int q = 0; q < NPOL; ++q)
      p.b[(((int64_t)f * NPOL + q) * p.g.nring + ring) * nm + m] =
          make_double2(w * (are[q] * c0 - aim[q] * s0), w * (are[q] * s0 + aim[q] * c0));
  }
}

// FFT version: x = map_a + i map_b, X = DFT_N(x); the two real fields separate through
// A_k = (X_k + conj X_{N-k}) / 2, B_k = (X_k - conj X_{N-k}) / (2i); g_m = w e^{-i m phi0} A_{m mod N}.
template <int NPOL, int NROW, bool BLUE>
__global__ __launch_bounds__(kFftThreads) void k_ring_anal_fft(RingParams p, RingClass rc) {
  using dmm_fft::C;
  extern __shared__ __align__(16) unsigned char smem[];
  const int rb = blockIdx.z * NROW;
  const int ring = class_ring(rc, p.g, blockIdx.x), f = blockIdx.y;
  const int n = p.g.nphi[ring], M = rc.M, P = M + 1;
  const RingLds l = ring_lds<NROW, BLUE>(smem, p.g, n, M);
  if (BLUE) __syncthreads();
  const int64_t base = p.g.start[ring];
  for (int k = threadIdx.x; k < M; k += kFftThreads) {
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
      C<double> v = {0.0, 0.0};
      if (k < n) {
        const int64_t p0 = ((int64_t)f * NPOL + (NPOL == 4 ? 2 * (r + rb) : 0)) * p.npix + base + k, p1 = p0 + p.npix;
        v.x = p.map_ref ? p.map_ref[p0] - p.map[p0] : p.map[p0];
        if (NPOL == 4) v.y = p.map_ref ? p.map_ref[p1] - p.map[p1] : p.map[p1];
        if (BLUE) v = dmm_fft::cmul<double>(v, l.chirp[k]);
      }
      l.buf[r * P + k] = v;
    }
  }
  __syncthreads();
  const double2* bfilt = BLUE ? p.g.bfilt + p.g.bf_off[rc.belt ? 0 : rc.r_lo + ((int)blockIdx.x >> 1)] : nullptr;
  ring_dft<NROW, BLUE>(l, bfilt, M, rc.logM);
  const int nm = p.g.mmax + 1;
  const double2* phase = p.g.phase + (int64_t)ring * nm;
  const double w = 4.0 * M_PI / (double)p.npix;
  for (int m = threadIdx.x; m < nm; m += kFftThreads) {
    const int k = m % n, k2 = (n - k) % n;
    const double2 ph = phase[m];
    const double c0 = ph.x, s0 = -ph.y;  // e^{-i m phi0}
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
      const C<double> X = ring_dft_at<BLUE>(l, r, k, M, rc.logM), Y = ring_dft_at<BLUE>(l, r, k2, M, rc.logM);
      const double ar = 0.5 * (X.x + Y.x), ai = 0.5 * (X.y - Y.y);
      p.b[(((int64_t)f * NPOL + (NPOL == 4 ? 2 * (r + rb) : 0)) * p.g.nring + ring) * nm + m] =
          make_double2(w * (ar * c0 - ai * s0), w * (ar * s0 + ai * c0));
      if (NPOL == 4) {
        const double br = 0.5 * (X.y + Y.y), bi = -0.5 * (X.x - Y.x);
        p.b[(((int64_t)f * NPOL + 2 * (r + rb) + 1) * p.g.nring + ring) * nm + m] =
            make_double2(w * (br * c0 - bi * s0), w * (br * s0 + bi * c0));
      }
    }
  }
}

// geometry build: spectrum of the wrapped conjugate chirp of cap ring number ir = blockIdx.x + 1
__global__ __launch_bounds__(kFftThreads) void k_build_bfilt(double2* table, const int64_t* bf_off) {
  using dmm_fft::C;
  extern __shared__ __align__(16) unsigned char smem[];
  const int ir = blockIdx.x + 1, N = 4 * ir, M = blue_len(ir), P = M + 1;
  int logM = 0;
  while ((1 << logM) < M) ++logM;
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  C<double>* tw = buf + P;
  for (int k = threadIdx.x; k < (M >> 1); k += kFftThreads) {
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)M, &sn, &cs);
    tw[k] = {cs, sn};
  }
  for (int j = threadIdx.x; j < M; j += kFftThreads) {
    const int nn = j < N ? j : (j > M - N ? M - j : -1);
    C<double> v = {0.0, 0.0};
    if (nn >= 0) {
      const int k2 = (int)(((int64_t)nn * nn) % (2 * (int64_t)N));
      double sn, cs;
      sincospi((double)k2 / (double)N, &sn, &cs);  // conj(c_n) = exp(+i pi n^2 / N)
      v = {cs, sn};
    }
    buf[j] = v;
  }
  __syncthreads();
  dmm_fft::fft_dif<double, kFftThreads>(buf, tw, 1, M, logM, P);
  const double inv = 1.0 / (double)M;
  double2* out = table + bf_off[ir];
  for (int k = threadIdx.x; k < M; k += kFftThreads) out[k] = make_double2(buf[k].x * inv, buf[k].y * inv);
}

}  // namespace
