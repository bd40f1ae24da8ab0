// Block-cooperative in-LDS row FFTs shared by the m-mode transform (mfft.hip), the ring-map maker (ringmap.hip) and the
// SHT ring stage (sht.hip).  What this file holds:
//   RowFft<T>        the description of one batched row transform, filled on the host by dmm_row_fft_plan (mfft.hip);
//   fft_dif / fft_dit, fft_dif8 / fft_dit8, bluestein_convolve   the passes over RB rows in LDS;
//   stage_twiddles, row_fft_forward / row_fft_inverse, spectrum_at, inverse_slot   what a kernel does with a RowFft:
//                    bring the twiddles in, run the transform, read bin k of a forward transform in natural order,
//                    place input bin k of an inverse transform.
// kThreads = threads of the calling block.
#pragma once
#include <hip/hip_runtime.h>

namespace dmm_fft {

template <typename T>
struct Vec2;
template <>
struct Vec2<float> {
  using type = float2;
};
template <>
struct Vec2<double> {
  using type = double2;
};

// One batched row transform of length N in precision T: a block holds RB rows of pitch P in LDS (and, when `tw_lds`,
// the M / 2 twiddles behind them) and runs an M-point FFT on each -- M = N for powers of two, else Bluestein's
// chirp-z with M the power of two >= 2 N - 1 (`chirp` != nullptr says which).
template <typename T>
struct RowFft {
  using T2 = typename Vec2<T>::type;
  int N, M, logM, RB, P;
  int tw_lds;       // twiddles staged in LDS (0: the passes read them from the table in memory)
  const T2* tw;     // [M/2] exp(-2 pi i k / M)
  const T2* chirp;  // [N]   exp(-i pi k^2 / N)                                  (Bluestein) or null
  const T2* bfilt;  // [M]   FFT_M(conj chirp, wrapped) / M, bit-reversed order  (Bluestein) or null
};

template <typename T>
struct C {
  T x, y;
};
template <typename T>
__device__ __forceinline__ C<T> cmul(C<T> a, C<T> b) {
  return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
template <typename T>
__device__ __forceinline__ C<T> cmulc(C<T> a, C<T> b) {  // a * conj(b)
  return {a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y};
}

// ---- block-cooperative in-LDS transforms over RB rows of length M (pitch P)
// The span-1 stage (twiddle = 1): the last of a DIF, the first of a DIT with an odd number of stages left over.
template <typename T, int kThreads>
__device__ __forceinline__ void pass_span1(C<T>* buf, int RB, int M, int P) {
  const int halfM = M >> 1;
  for (int b = threadIdx.x; b < RB * halfM; b += kThreads) {
    const int r = b / halfM, k = b - r * halfM;
    C<T>* p = buf + r * P + 2 * k;
    const C<T> a = p[0], c = p[1];
    p[0] = {a.x + c.x, a.y + c.y};
    p[1] = {a.x - c.x, a.y - c.y};
  }
  __syncthreads();
}
// The spans 2 and 1 as one radix-4 pass over groups of four: the last two stages of a DIF, or (DIT) the first two of a DIT --
// the same butterfly with elements 1 and 2 of the group changing places on the way in and out (the 4-point bit reversal).
template <typename T, bool DIT, bool CONJ, int kThreads>
__device__ __forceinline__ void pass_span21(C<T>* buf, const C<T>* tw, int RB, int M, int logM, int P) {
  constexpr int i1 = DIT ? 2 : 1, i2 = DIT ? 1 : 2;
  const int nq = M >> 2;
  for (int b = threadIdx.x; b < RB * nq; b += kThreads) {
    const int r = b / nq, q = b - r * nq;
    C<T>* p = buf + r * P + 4 * q;
    const C<T> e0 = p[0], e1 = p[i1], e2 = p[i2], e3 = p[3];
    const C<T> wa1 = tw[1 << (logM - 2)];  // exp(-2 pi i / 4): the one non-trivial twiddle of the span-2 stage
    const C<T> d = {e1.x - e3.x, e1.y - e3.y};
    const C<T> a0 = {e0.x + e2.x, e0.y + e2.y}, a1 = {e1.x + e3.x, e1.y + e3.y};
    const C<T> a2 = {e0.x - e2.x, e0.y - e2.y}, a3 = CONJ ? cmulc<T>(d, wa1) : cmul<T>(d, wa1);
    p[0] = {a0.x + a1.x, a0.y + a1.y};
    p[i1] = {a0.x - a1.x, a0.y - a1.y};
    p[i2] = {a2.x + a3.x, a2.y + a3.y};
    p[3] = {a2.x - a3.x, a2.y - a3.y};
  }
  __syncthreads();
}
// DIF: natural order in, bit-reversed order out, forward sign (tw = exp(-2 pi i k/M)).
// Two radix-2 stages are fused per pass (4 elements in registers): half the LDS traffic and
// half the barriers of a plain radix-2 loop, same data flow, so the output stays bit-reversed.
template <typename T, int kThreads>
__device__ void fft_dif(C<T>* buf, const C<T>* tw, int RB, int M, int logM, int P) {
  int s = logM - 1;
  for (; s >= 1; s -= 2) {  // stages s (span half) and s-1 (span quarter)
    const int half = 1 << s, quarter = half >> 1, nq = M >> 2;
    for (int b = threadIdx.x; b < RB * nq; b += kThreads) {
      const int r = b / nq, q = b - r * nq;
      const int t = q & (quarter - 1);
      const int j = ((q >> (s - 1)) << (s + 1)) | t;
      C<T>* p = buf + r * P + j;
      const C<T> e0 = p[0], e1 = p[quarter], e2 = p[half], e3 = p[half + quarter];
      const C<T> wa0 = tw[t << (logM - 1 - s)], wa1 = tw[(t + quarter) << (logM - 1 - s)];
      const C<T> wb = tw[t << (logM - s)];
      const C<T> a0 = {e0.x + e2.x, e0.y + e2.y}, a1 = {e1.x + e3.x, e1.y + e3.y};
      const C<T> a2 = cmul<T>({e0.x - e2.x, e0.y - e2.y}, wa0), a3 = cmul<T>({e1.x - e3.x, e1.y - e3.y}, wa1);
      p[0] = {a0.x + a1.x, a0.y + a1.y};
      p[quarter] = cmul<T>({a0.x - a1.x, a0.y - a1.y}, wb);
      p[half] = {a2.x + a3.x, a2.y + a3.y};
      p[half + quarter] = cmul<T>({a2.x - a3.x, a2.y - a3.y}, wb);
    }
    __syncthreads();
  }
  if (s == 0) {  // odd number of stages: last span-1 stage (twiddle = 1)
    pass_span1<T, kThreads>(buf, RB, M, P);
  }
}
// DIT: bit-reversed order in, natural order out; CONJ selects exp(+2 pi i k/M).  Same pairing.
template <typename T, bool CONJ, int kThreads>
__device__ void fft_dit(C<T>* buf, const C<T>* tw, int RB, int M, int logM, int P) {
  int s = 0;
  if (logM & 1) {  // odd number of stages: first span-1 stage alone (twiddle = 1)
    pass_span1<T, kThreads>(buf, RB, M, P);
    s = 1;
  }
  for (; s + 1 < logM; s += 2) {  // stages s (span quarter) then s+1 (span half)
    const int quarter = 1 << s, half = quarter << 1, nq = M >> 2;
    for (int b = threadIdx.x; b < RB * nq; b += kThreads) {
      const int r = b / nq, q = b - r * nq;
      const int t = q & (quarter - 1);
      const int j = ((q >> s) << (s + 2)) | t;
      C<T>* p = buf + r * P + j;
      const C<T> e0 = p[0], e1 = p[quarter], e2 = p[half], e3 = p[half + quarter];
      const C<T> wb = tw[t << (logM - 1 - s)];
      const C<T> wa0 = tw[t << (logM - 2 - s)], wa1 = tw[(t + quarter) << (logM - 2 - s)];
      const C<T> c1 = CONJ ? cmulc<T>(e1, wb) : cmul<T>(e1, wb);
      const C<T> c3 = CONJ ? cmulc<T>(e3, wb) : cmul<T>(e3, wb);
      const C<T> a0 = {e0.x + c1.x, e0.y + c1.y}, a1 = {e0.x - c1.x, e0.y - c1.y};
      const C<T> a2 = {e2.x + c3.x, e2.y + c3.y}, a3 = {e2.x - c3.x, e2.y - c3.y};
      const C<T> d2 = CONJ ? cmulc<T>(a2, wa0) : cmul<T>(a2, wa0);
      const C<T> d3 = CONJ ? cmulc<T>(a3, wa1) : cmul<T>(a3, wa1);
      p[0] = {a0.x + d2.x, a0.y + d2.y};
      p[half] = {a0.x - d2.x, a0.y - d2.y};
      p[quarter] = {a1.x + d3.x, a1.y + d3.y};
      p[half + quarter] = {a1.x - d3.x, a1.y - d3.y};
    }
    __syncthreads();
  }
}

// ---- the same transforms with THREE radix-2 stages fused per pass (8 elements in registers): a pass costs one LDS read and
// one write per element whatever its radix, so 11 stages take 4 passes instead of 6 (and 4 barriers instead of 6); the leftover
// one or two stages go through a radix-2 / radix-4 pass of the forms above.  Same butterflies, same twiddle table, same data
// flow (DIF: natural in, bit-reversed out; DIT: the reverse) -- the products are associated as in the radix-4 passes, stage by stage.
template <typename T, int kThreads>
__device__ void fft_dif8(C<T>* buf, const C<T>* tw, int RB, int M, int logM, int P) {
  int s = logM - 1;
  for (; s >= 2; s -= 3) {  // stages s (span half), s-1 (quarter), s-2 (eighth)
    const int eighth = 1 << (s - 2), no = M >> 3;
    for (int b = threadIdx.x; b < RB * no; b += kThreads) {
      const int r = b / no, o = b - r * no;
      const int t = o & (eighth - 1);
      const int j = ((o >> (s - 2)) << (s + 1)) | t;
      C<T>* p = buf + r * P + j;
      C<T> e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = p[k * eighth];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // stage s: (k, k + 4)
        const C<T> w = tw[(t + k * eighth) << (logM - 1 - s)];
        const C<T> u = e[k], v = e[k + 4];
        e[k] = {u.x + v.x, u.y + v.y};
        e[k + 4] = cmul<T>({u.x - v.x, u.y - v.y}, w);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {  // stage s-1: (g + k, g + k + 2), g = 0, 4
        const C<T> w = tw[(t + k * eighth) << (logM - s)];
#pragma unroll
        for (int g = 0; g < 8; g += 4) {
          const C<T> u = e[g + k], v = e[g + k + 2];
          e[g + k] = {u.x + v.x, u.y + v.y};
          e[g + k + 2] = cmul<T>({u.x - v.x, u.y - v.y}, w);
        }
      }
      {  // stage s-2: (g, g + 1), g = 0, 2, 4, 6
        const C<T> w = tw[t << (logM - s + 1)];
#pragma unroll
        for (int g = 0; g < 8; g += 2) {
          const C<T> u = e[g], v = e[g + 1];
          e[g] = {u.x + v.x, u.y + v.y};
          e[g + 1] = cmul<T>({u.x - v.x, u.y - v.y}, w);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k * eighth] = e[k];
    }
    __syncthreads();
  }
  if (s == 1) {  // two stages left (spans 2 and 1): one radix-4 pass
    pass_span21<T, false, false, kThreads>(buf, tw, RB, M, logM, P);
  } else if (s == 0) {  // one stage left (span 1, twiddle 1)
    pass_span1<T, kThreads>(buf, RB, M, P);
  }
}

template <typename T, bool CONJ, int kThreads>
__device__ void fft_dit8(C<T>* buf, const C<T>* tw, int RB, int M, int logM, int P) {
  auto mul = [](C<T> a, C<T> w) { return CONJ ? cmulc<T>(a, w) : cmul<T>(a, w); };
  int s = 0;
  const int rem = logM % 3;
  if (rem == 1) {  // first the span-1 stage alone (twiddle 1)
    pass_span1<T, kThreads>(buf, RB, M, P);
    s = 1;
  } else if (rem == 2) {  // first the spans 1 and 2 as one radix-4 pass
    pass_span21<T, true, CONJ, kThreads>(buf, tw, RB, M, logM, P);
    s = 2;
  }
  for (; s + 2 < logM; s += 3) {  // stages s (span e), s+1 (2 e), s+2 (4 e)
    const int e1 = 1 << s, no = M >> 3;
    for (int b = threadIdx.x; b < RB * no; b += kThreads) {
      const int r = b / no, o = b - r * no;
      const int t = o & (e1 - 1);
      const int j = ((o >> s) << (s + 3)) | t;
      C<T>* p = buf + r * P + j;
      C<T> e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = p[k * e1];
      {  // stage s: (g, g + 1)
        const C<T> w = tw[t << (logM - 1 - s)];
#pragma unroll
        for (int g = 0; g < 8; g += 2) {
          const C<T> u = e[g], v = mul(e[g + 1], w);
          e[g] = {u.x + v.x, u.y + v.y};
          e[g + 1] = {u.x - v.x, u.y - v.y};
        }
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {  // stage s+1: (g + k, g + k + 2), g = 0, 4
        const C<T> w = tw[(t + k * e1) << (logM - 2 - s)];
#pragma unroll
        for (int g = 0; g < 8; g += 4) {
          const C<T> u = e[g + k], v = mul(e[g + k + 2], w);
          e[g + k] = {u.x + v.x, u.y + v.y};
          e[g + k + 2] = {u.x - v.x, u.y - v.y};
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // stage s+2: (k, k + 4)
        const C<T> w = tw[(t + k * e1) << (logM - 3 - s)];
        const C<T> u = e[k], v = mul(e[k + 4], w);
        e[k] = {u.x + v.x, u.y + v.y};
        e[k + 4] = {u.x - v.x, u.y - v.y};
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k * e1] = e[k];
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int bitrev(int k, int logM) {
  return logM == 0 ? 0 : (int)(__brev((unsigned)k) >> (32 - logM));
}

// ---- Bluestein's convolution on RB rows already multiplied by the chirp and zero-padded to M: DIF forward, pointwise
// product with the filter spectrum (`bfilt`: float2 / double2, bit-reversed order, scaled by 1/M), DIT inverse -- natural
// order in and out, no reordering pass.  `radix8`: the passes with three stages each.
template <typename T, int kThreads, typename T2>
__device__ __forceinline__ void bluestein_convolve(C<T>* buf, const C<T>* tw, const T2* bfilt, int RB, int M, int logM, int P,
                                                   bool radix8 = false) {
  if (radix8) fft_dif8<T, kThreads>(buf, tw, RB, M, logM, P);
  else fft_dif<T, kThreads>(buf, tw, RB, M, logM, P);
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx / M, k = idx - r * M;
    const T2 f = bfilt[k];
    buf[r * P + k] = cmul<T>(buf[r * P + k], {f.x, f.y});
  }
  __syncthreads();
  if (radix8) fft_dit8<T, true, kThreads>(buf, tw, RB, M, logM, P);
  else fft_dit<T, true, kThreads>(buf, tw, RB, M, logM, P);
}

// ---- a kernel's use of a RowFft.  The LDS image is q.RB rows of pitch q.P at `buf`, the staged twiddles at `tw_s` behind them.
// `blue` is q.chirp != nullptr, handed in so that a kernel instantiated per kind passes its template constant.
// Twiddles: staged in LDS (barrier left to the caller: every kernel fills its rows next), or the table in memory where the
// plan says they do not fit.  FALLBACK = false for a kernel whose plan never reads them from memory: its passes then
// address the LDS directly instead of through a pointer that may be either.
template <typename T, int kThreads, bool FALLBACK>
__device__ __forceinline__ const C<T>* stage_twiddles(const RowFft<T>& q, C<T>* tw_s) {
  if (FALLBACK && !q.tw_lds) return reinterpret_cast<const C<T>*>(q.tw);
  for (int k = threadIdx.x; k < (q.M >> 1); k += kThreads) {
    const typename RowFft<T>::T2 w = q.tw[k];
    tw_s[k] = {w.x, w.y};
  }
  return tw_s;
}
// Forward DFT_N of rows in natural order (Bluestein: already times the chirp, zero-padded to M); read with spectrum_at.
template <typename T, int kThreads>
__device__ __forceinline__ void row_fft_forward(const RowFft<T>& q, bool blue, C<T>* buf, const C<T>* tw) {
  if (blue) bluestein_convolve<T, kThreads>(buf, tw, q.bfilt, q.RB, q.M, q.logM, q.P);
  else fft_dif<T, kThreads>(buf, tw, q.RB, q.M, q.logM, q.P);
}
// The same sum over rows whose bin k was stored at inverse_slot(k) (Bluestein: times the chirp); natural order out, the
// Bluestein result still to be multiplied by the chirp.  An inverse transform is conj(this(conj X)).
template <typename T, int kThreads>
__device__ __forceinline__ void row_fft_inverse(const RowFft<T>& q, bool blue, C<T>* buf, const C<T>* tw) {
  if (blue) bluestein_convolve<T, kThreads>(buf, tw, q.bfilt, q.RB, q.M, q.logM, q.P);
  else fft_dit<T, false, kThreads>(buf, tw, q.RB, q.M, q.logM, q.P);
}
__device__ __forceinline__ int inverse_slot(bool blue, int k, int logM) { return blue ? k : bitrev(k, logM); }
// Bin k of a forward transform's row, natural order (`chirp`: the table in memory or a copy in LDS)
template <typename T, typename TC>
__device__ __forceinline__ C<T> spectrum_at(const C<T>* row, const TC* chirp, bool blue, int k, int logM) {
  if (blue) {
    const TC c = chirp[k];
    return cmul<T>(row[k], {c.x, c.y});
  }
  return row[bitrev(k, logM)];
}

}  // namespace dmm_fft
