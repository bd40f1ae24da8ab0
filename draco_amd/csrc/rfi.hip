// RFI flagging: masked moving median, row quantile, SumThreshold, the scale-invariant rank operator and the elementwise
// stages of the mask tasks.
//
// Reference: draco/util/filters.py:99-130 (medfilt), draco/util/rfi.py:8-257 (sumthreshold_py, _sir_lastaxis,
// scale_invariant_rank), draco/analysis/flagging.py:1808-2117 (RFISensitivityMask), :2120-2219 (RFIMask), :2222-2377
// (ApplyTimeFreqMask), :3231-3381 (mad, tv_channels_flag).  The median conventions (caput's routines are not pinned by
// the reference itself) are DESIGN.md section 7i.
//
// k_medfilt: one block per frequency row and tile of T output times.  The block stages the sf x (T + st - 1) strip as
// order-preserving 64-bit keys, column by column, sorts every time column once (rank sort, flagged samples dropped),
// then each wave selects the median of one output's window: a bisection over the key, lanes own columns, the count a
// wave reduction.  Each column keeps the bracket of places its probes can still fall into, so a step searches only
// inside it and a settled column is not read again.  The bisection starts below the common leading bits of the
// window's smallest and largest key.  The result is a sample (or the mean of two), never an accumulated value: it does
// not depend on the block shape or the launch order.
// k_wmedfilt: the weighted moving median of RFIMaskChisqHighDelay (draco/analysis/flagging.py:1670-1773; the convention is
// DESIGN.md section 7s).  k_medfilt's strip, sort and bisection, with each key's weight as payload: every sorted column
// carries the inclusive prefix sums of its weights, a probe reads the prefix weight at the place it finds, and the wave
// reduces the weight instead of the count and compares it with half the window's total.  The strip holds 16 bytes per
// sample, up to 8192 samples, and the windows reach 1023 columns: the kernel is compiled for 4, 10 and 16 columns per lane.
// k_quantile: one wave per row, the same bisection over the unsorted row in LDS.
// k_st_hit / k_st_spread: one SumThreshold step (one window length along one axis) as two launches, so that the flag
// update of an axis completes before the next one reads it.  Window sums run in ascending sample order in float64.
// k_sir / k_sir_rows: one lane per line, strictly sequential float64 running sum (np.cumsum's order), forward pass for
// the running minimum, backward pass for the running maximum; along time the flags pass through an LDS transpose tile.
// Everything here is compiled with floating-point contraction off: the Boolean outcomes follow NumPy's expressions.
#include "dmm_internal.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMedThreads = 512;
constexpr int kMedWaves = kMedThreads / kWave;
constexpr int kMedTile = 32;                                  // output times per block, at most
constexpr int kMedPer = DMM_RFI_MAX_STRIP / kMedThreads;      // strip samples per thread in the sort
constexpr int kMedColsPerLane = (DMM_RFI_MAX_WINDOW + kWave) / kWave;  // 4
constexpr uint64_t kDropped = ~0ull;                          // key of a flagged sample (no kept sample maps to it)

// order-preserving key of a double; every NaN maps to one key above +inf
__device__ inline uint64_t key_of(double v) {
  if (v != v) return 0xFFF8000000000000ull;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double val_of(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ inline int wave_sum(int v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline uint64_t wave_min(uint64_t v) {
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint64_t u = (uint64_t)__shfl_xor((unsigned long long)v, o);
    v = u < v ? u : v;
  }
  return v;
}
__device__ inline uint64_t wave_max(uint64_t v) {
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint64_t u = (uint64_t)__shfl_xor((unsigned long long)v, o);
    v = u > v ? u : v;
  }
  return v;
}

// 0.5 (v[k1] + v[k2]) of the n >= 1 keys a wave holds, k2 = k1 or k1 + 1; kmin / kmax their smallest and largest.
// The bisection keeps the answer in [x, U): x starts at the keys' common leading bits, U one step of the first free bit
// above it.  S::probe(t): this lane's count of keys < t for a t inside (x, U); S::accept(up): the wave took t as the
// new x (up) or the new U.  After the last bit U = x + 1, and S::count_le(x) / S::min_gt(x) give this lane's count of
// keys <= x and its smallest key > x (kDropped if none).
// S::bracket_min(x): this lane's smallest key in [x, U).  Once one key is left in [x, U) it is v[k1]: the rest of the
// bits are not walked.
template <class S>
__device__ inline double wave_select(S& s, int n, int k1, int k2, uint64_t kmin, uint64_t kmax) {
  uint64_t x = kmin;
  if (kmin != kmax) {
    const int b = 63 - __clzll((long long)(kmin ^ kmax));
    x = b == 63 ? 0ull : ((kmin >> (b + 1)) << (b + 1));
    int clo = 0, chi = n;  // count(keys < x) <= k1 < count(keys < U)
    for (int bit = b; bit >= 0; --bit) {  // the largest x with count(keys < x) <= k1 is v[k1]
      const uint64_t t = x | (1ull << bit);
      const int c = wave_sum(s.probe(t));
      const bool up = c <= k1;
      if (up) {
        x = t;
        clo = c;
      } else {
        chi = c;
      }
      s.accept(up);
      if (chi - clo == 1) {
        x = wave_min(s.bracket_min(x));
        break;
      }
    }
  }
  uint64_t x2 = x;
  if (k2 != k1 && wave_sum(s.count_le(x)) <= k2) x2 = wave_min(s.min_gt(x));
  return 0.5 * (val_of(x) + val_of(x2));
}

// ---------------------------------------------------------------- masked moving median

struct MedArgs {
  const double* x;
  const uint8_t* flag;
  double* out;
  int nf, nt, hf, ht, T;
};

// The sorted columns one lane owns.  Per column lo = count(keys < x) and hi = count(keys < U) bracket the place of
// every later probe, so each binary search runs inside [lo, hi) only: once a column's bracket is empty it costs no
// LDS read any more, and a column is read about log2(sf) + a few times per output, not log2(sf) times per step.
struct ColumnSet {
  const uint64_t* col[kMedColsPerLane];
  int cnt[kMedColsPerLane], lo[kMedColsPerLane], hi[kMedColsPerLane], mid[kMedColsPerLane];
  __device__ inline int probe(uint64_t t) {
    int tot = 0;
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) {
      int l = lo[j], len = hi[j] - l;
      while (len > 0) {
        const int half = len >> 1;
        if (col[j][l + half] < t) {
          l += half + 1;
          len -= half + 1;
        } else {
          len = half;
        }
      }
      mid[j] = l;
      tot += l;
    }
    return tot;
  }
  __device__ inline void accept(bool up) {
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) {
      if (up)
        lo[j] = mid[j];
      else
        hi[j] = mid[j];
    }
  }
  __device__ inline uint64_t bracket_min(uint64_t) const {
    uint64_t best = kDropped;
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) {
      if (lo[j] < hi[j]) {
        const uint64_t k = col[j][lo[j]];
        best = k < best ? k : best;
      }
    }
    return best;
  }
  __device__ inline int count_le(uint64_t) const {  // no key lies in (x, U) when this is asked
    int tot = 0;
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) tot += hi[j];
    return tot;
  }
  __device__ inline uint64_t min_gt(uint64_t) const {
    uint64_t best = kDropped;
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) {
      if (hi[j] < cnt[j]) {
        const uint64_t k = col[j][hi[j]];
        best = k < best ? k : best;
      }
    }
    return best;
  }
};

__global__ __launch_bounds__(kMedThreads) void k_medfilt(MedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char med_lds[];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int f = blockIdx.y;
  const int t0 = blockIdx.x * a.T;
  const int t1 = min(t0 + a.T, a.nt);  // one past the block's last output
  const int r0 = max(f - a.hf, 0), r1 = min(f + a.hf, a.nf - 1);
  const int c0 = max(t0 - a.ht, 0), c1 = min(t1 - 1 + a.ht, a.nt - 1);
  const int R = r1 - r0 + 1, C = c1 - c0 + 1, total = R * C;  // total <= DMM_RFI_MAX_STRIP (checked by the host)
  uint64_t* keys = (uint64_t*)med_lds;  // [C][R], column c at keys + c R
  int* cnt = (int*)(keys + total);      // [C] kept samples of every column
  const size_t plane = (size_t)blockIdx.z * a.nf * a.nt;
  const double* x = a.x + plane;
  const uint8_t* fl = a.flag + plane;

  for (int e = tid; e < total; e += kMedThreads) {  // time fastest: coalesced reads
    const int r = e / C, c = e - r * C;
    const size_t o = (size_t)(r0 + r) * a.nt + (c0 + c);
    keys[c * R + r] = fl[o] ? kDropped : key_of(x[o]);
  }
  __syncthreads();
  for (int c = tid; c < C; c += kMedThreads) {
    int n = 0;
    for (int r = 0; r < R; ++r) n += keys[c * R + r] != kDropped;
    cnt[c] = n;
  }
  // rank sort of every column: each thread ranks its samples among the kept ones of their column, all threads hold
  // their keys in registers across the barrier, then write them to their places
  uint64_t kk[kMedPer];
  int rk[kMedPer];
#pragma unroll
  for (int i = 0; i < kMedPer; ++i) {
    const int e = tid + i * kMedThreads;
    rk[i] = -1;
    kk[i] = kDropped;
    if (e < total) {
      const int c = e / R, r = e - c * R;
      const uint64_t k = keys[e];
      if (k != kDropped) {
        const uint64_t* col = keys + c * R;
        int rank = 0;
        for (int q = 0; q < R; ++q) {
          const uint64_t u = col[q];
          rank += (u < k) || (u == k && q < r);
        }
        kk[i] = k;
        rk[i] = c * R + rank;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kMedPer; ++i)
    if (rk[i] >= 0) keys[rk[i]] = kk[i];
  __syncthreads();

  for (int t = t0 + wave; t < t1; t += kMedWaves) {  // uniform per wave
    const int ca = max(t - a.ht, 0) - c0, cb = min(t + a.ht, a.nt - 1) - c0;
    ColumnSet s;
    int n = 0;
    uint64_t kmin = kDropped, kmax = 0;
#pragma unroll
    for (int j = 0; j < kMedColsPerLane; ++j) {
      const int c = ca + lane + j * kWave;
      s.col[j] = keys;
      s.cnt[j] = 0;
      s.lo[j] = s.mid[j] = 0;
      if (c <= cb) {
        s.col[j] = keys + c * R;
        s.cnt[j] = cnt[c];
        if (s.cnt[j] > 0) {
          const uint64_t lo = s.col[j][0], hi = s.col[j][s.cnt[j] - 1];
          kmin = lo < kmin ? lo : kmin;
          kmax = hi > kmax ? hi : kmax;
        }
      }
      s.hi[j] = s.cnt[j];
      n += s.cnt[j];
    }
    n = wave_sum(n);
    double res = __longlong_as_double(0x7FF8000000000000ll);  // empty window
    if (n > 0) {
      kmin = wave_min(kmin);
      kmax = wave_max(kmax);
      res = wave_select(s, n, (n - 1) / 2, n / 2, kmin, kmax);
    }
    if (lane == 0) a.out[plane + (size_t)f * a.nt + t] = res;
  }
}

// ---------------------------------------------------------------- weighted moving median

constexpr int kWmedPer = DMM_RFI_WMED_MAX_STRIP / kMedThreads;  // strip samples per thread in the sort

__device__ inline double wave_sum_d(double v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

struct WMedArgs {
  const double* x;
  const double* w;
  double* out;
  int nf, nt, hf, ht, T;
};

// The sorted columns one lane owns, as in ColumnSet, with the inclusive prefix sums of the weights beside the keys:
// pw[c R + i] is the weight of the i + 1 smallest kept samples of column c.  wl[j] is the prefix weight below lo[j]; a
// column whose bracket is empty answers a probe from it without an LDS read.
template <int CPL>
struct WColumnSet {
  const uint64_t* keys;
  const double* pw;
  const int* cnt;
  int R, c0, cb;  // this lane's columns are c0 + 64 j, those beyond cb do not exist
  int lo[CPL], hi[CPL], mid[CPL];
  double wl[CPL];
  __device__ inline double below(int j, int l) const { return l > 0 ? pw[(c0 + j * kWave) * R + l - 1] : 0.0; }
  // this lane's count and weight of keys < t
  __device__ inline int probe(uint64_t t, double& wsum) {
    int tot = 0;
    double ws = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      int l = lo[j], len = hi[j] - l;
      double wj = wl[j];
      if (len > 0) {
        const uint64_t* col = keys + (c0 + j * kWave) * R;
        while (len > 0) {
          const int half = len >> 1;
          if (col[l + half] < t) {
            l += half + 1;
            len -= half + 1;
          } else {
            len = half;
          }
        }
        if (l != lo[j]) wj = below(j, l);
      }
      mid[j] = l;
      tot += l;
      ws = ws + wj;
    }
    wsum = ws;
    return tot;
  }
  __device__ inline void accept(bool up) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      if (up) {
        if (mid[j] != lo[j]) {
          lo[j] = mid[j];
          wl[j] = below(j, lo[j]);
        }
      } else {
        hi[j] = mid[j];
      }
    }
  }
  __device__ inline uint64_t bracket_min() const {
    uint64_t best = kDropped;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      if (lo[j] < hi[j]) {
        const uint64_t k = keys[(c0 + j * kWave) * R + lo[j]];
        best = k < best ? k : best;
      }
    }
    return best;
  }
  __device__ inline double weight_le() const {  // no key lies in (x, U) when this is asked
    double ws = 0.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) ws = ws + below(j, hi[j]);
    return ws;
  }
  __device__ inline uint64_t min_gt() const {
    uint64_t best = kDropped;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = c0 + j * kWave;
      if (c <= cb && hi[j] < cnt[c]) {
        const uint64_t k = keys[c * R + hi[j]];
        best = k < best ? k : best;
      }
    }
    return best;
  }
};

// 0.5 (lo + hi) of the n >= 1 weighted keys a wave holds, W > 0 their total weight and c(v) the weight of the keys <= v:
// lo the smallest key with c(lo) >= W / 2, hi the smallest with c(hi) > W / 2.  With g(t) the weight of the keys < t, lo
// is the largest t with g(t) < W / 2: the bisection of wave_select with the weight in the place of the count.  The
// count is carried along for the early exit only: one key left in [x, U) is lo.  hi is lo unless c(lo) == W / 2
// exactly, then the next key.  Every weight is a sum of per-column prefix sums in one fixed order (a lane's columns in
// ascending order, then the butterfly): it depends on the output's window alone, not on the tile or the block.
template <int CPL>
__device__ inline double wave_wselect(WColumnSet<CPL>& s, int n, double W, uint64_t kmin, uint64_t kmax) {
  const double half = 0.5 * W;
  uint64_t x = kmin;
  if (kmin != kmax) {
    const int b = 63 - __clzll((long long)(kmin ^ kmax));
    x = b == 63 ? 0ull : ((kmin >> (b + 1)) << (b + 1));
    int clo = 0, chi = n;
    for (int bit = b; bit >= 0; --bit) {
      const uint64_t t = x | (1ull << bit);
      double g;
      const int c = wave_sum(s.probe(t, g));
      g = wave_sum_d(g);
      const bool up = g < half;
      if (up) {
        x = t;
        clo = c;
      } else {
        chi = c;
      }
      s.accept(up);
      if (chi - clo == 1) {
        x = wave_min(s.bracket_min());
        break;
      }
    }
  }
  uint64_t x2 = x;
  if (wave_sum_d(s.weight_le()) == half) x2 = wave_min(s.min_gt());
  return 0.5 * (val_of(x) + val_of(x2));
}

// One block per frequency row and tile of T output times, as k_medfilt.  LDS: the keys [C][R], the weights and then
// their prefix sums [C][R], the kept count of every column.  Samples whose weight is not > 0 carry the largest key and
// are dropped by the sort.
template <int CPL>
__global__ __launch_bounds__(kMedThreads) void k_wmedfilt(WMedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wmed_lds[];
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int f = blockIdx.y;
  const int t0 = blockIdx.x * a.T;
  const int t1 = min(t0 + a.T, a.nt);
  const int r0 = max(f - a.hf, 0), r1 = min(f + a.hf, a.nf - 1);
  const int c0 = max(t0 - a.ht, 0), c1 = min(t1 - 1 + a.ht, a.nt - 1);
  const int R = r1 - r0 + 1, C = c1 - c0 + 1, total = R * C;  // total <= DMM_RFI_WMED_MAX_STRIP (checked by the host)
  uint64_t* keys = (uint64_t*)wmed_lds;   // [C][R]
  double* pw = (double*)(keys + total);   // [C][R]
  int* cnt = (int*)(pw + total);          // [C]
  const size_t plane = (size_t)blockIdx.z * a.nf * a.nt;
  const double* x = a.x + plane;
  const double* w = a.w + plane;

  for (int e = tid; e < total; e += kMedThreads) {  // time fastest: coalesced reads
    const int r = e / C, c = e - r * C;
    const size_t o = (size_t)(r0 + r) * a.nt + (c0 + c);
    const double wv = w[o];
    const bool kept = wv > 0.0;
    keys[c * R + r] = kept ? key_of(x[o]) : kDropped;
    pw[c * R + r] = kept ? wv : 0.0;
  }
  __syncthreads();
  for (int c = tid; c < C; c += kMedThreads) {
    int n = 0;
    for (int r = 0; r < R; ++r) n += keys[c * R + r] != kDropped;
    cnt[c] = n;
  }
  // rank sort of every column, the weight travelling with its key; equal keys keep their row order
  uint64_t kk[kWmedPer];
  double ww[kWmedPer];
  int rk[kWmedPer];
#pragma unroll
  for (int i = 0; i < kWmedPer; ++i) {
    const int e = tid + i * kMedThreads;
    rk[i] = -1;
    kk[i] = kDropped;
    ww[i] = 0.0;
    if (e < total) {
      const int c = e / R, r = e - c * R;
      const uint64_t k = keys[e];
      if (k != kDropped) {
        const uint64_t* col = keys + c * R;
        int rank = 0;
        for (int q = 0; q < R; ++q) {
          const uint64_t u = col[q];
          rank += (u < k) || (u == k && q < r);
        }
        kk[i] = k;
        ww[i] = pw[e];
        rk[i] = c * R + rank;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kWmedPer; ++i) {
    if (rk[i] >= 0) {
      keys[rk[i]] = kk[i];
      pw[rk[i]] = ww[i];
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += kMedThreads) {  // inclusive prefix sums in sorted order, strictly sequential
    double s = 0.0;
    const int n = cnt[c];
    for (int r = 0; r < n; ++r) {
      s = s + pw[c * R + r];
      pw[c * R + r] = s;
    }
  }
  __syncthreads();

  for (int t = t0 + wave; t < t1; t += kMedWaves) {  // uniform per wave
    const int ca = max(t - a.ht, 0) - c0, cb = min(t + a.ht, a.nt - 1) - c0;  // cb - ca < 64 CPL (chosen by the host)
    WColumnSet<CPL> s;
    s.keys = keys;
    s.pw = pw;
    s.cnt = cnt;
    s.R = R;
    s.c0 = ca + lane;
    s.cb = cb;
    int n = 0;
    double W = 0.0;
    uint64_t kmin = kDropped, kmax = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = ca + lane + j * kWave;
      s.lo[j] = s.mid[j] = s.hi[j] = 0;
      s.wl[j] = 0.0;
      if (c <= cb) {
        const int m = cnt[c];
        s.hi[j] = m;
        if (m > 0) {
          const uint64_t lo = keys[c * R], hi = keys[c * R + m - 1];
          kmin = lo < kmin ? lo : kmin;
          kmax = hi > kmax ? hi : kmax;
          W = W + pw[c * R + m - 1];
        }
        n += m;
      }
    }
    n = wave_sum(n);
    double res = __longlong_as_double(0x7FF8000000000000ll);  // empty window
    if (n > 0) {
      W = wave_sum_d(W);
      kmin = wave_min(kmin);
      kmax = wave_max(kmax);
      res = wave_wselect(s, n, W, kmin, kmax);
    }
    if (lane == 0) a.out[plane + (size_t)f * a.nt + t] = res;
  }
}

// ---------------------------------------------------------------- row quantile ("split" method)

struct RowSet {
  const uint64_t* keys;
  int n, lane;
  __device__ inline int probe(uint64_t t) const {
    int tot = 0;
    for (int i = lane; i < n; i += kWave) tot += keys[i] < t;
    return tot;
  }
  __device__ inline void accept(bool) const {}
  __device__ inline uint64_t bracket_min(uint64_t x) const {
    uint64_t best = kDropped;
    for (int i = lane; i < n; i += kWave) {
      const uint64_t k = keys[i];
      if (k >= x && k < best) best = k;
    }
    return best;
  }
  __device__ inline int count_le(uint64_t x) const {  // (dropped samples carry the largest key: never <= a kept one)
    int tot = 0;
    for (int i = lane; i < n; i += kWave) tot += keys[i] <= x;
    return tot;
  }
  __device__ inline uint64_t min_gt(uint64_t x) const {
    uint64_t best = kDropped;
    for (int i = lane; i < n; i += kWave) {
      const uint64_t k = keys[i];
      if (k > x && k < best) best = k;
    }
    return best;
  }
};

__global__ __launch_bounds__(kWave) void k_quantile(const double* y, const uint8_t* flag, int n, double q, double* out, int32_t* count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char q_lds[];
  uint64_t* keys = (uint64_t*)q_lds;
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * n;
  int nv = 0;
  uint64_t kmin = kDropped, kmax = 0;
  for (int i = lane; i < n; i += kWave) {
    const uint64_t k = flag[base + i] ? kDropped : key_of(y[base + i]);
    keys[i] = k;
    if (k != kDropped) {
      ++nv;
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    }
  }
  __syncthreads();
  nv = wave_sum(nv);
  double res = __longlong_as_double(0x7FF8000000000000ll);
  if (nv > 0) {
    kmin = wave_min(kmin);
    kmax = wave_max(kmax);
    const double t = q * (double)nv;
    int lo = (int)ceil(t) - 1, hi = (int)floor(t);
    lo = max(0, min(lo, nv - 1));
    hi = max(0, min(hi, nv - 1));
    RowSet s{keys, n, lane};
    res = wave_select(s, nv, lo, hi, kmin, kmax);
  }
  if (lane == 0) {
    out[blockIdx.x] = res;
    if (count) count[blockIdx.x] = nv;
  }
}

// ---------------------------------------------------------------- SumThreshold

struct StArgs {
  const double* data;
  const double* var;
  uint8_t* flag;
  uint8_t* hit;
  double thr;
  int nf, nt, m, axis, correct, positive;
};

__global__ __launch_bounds__(256) void k_st_init(const double* data, uint8_t* flag, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flag[i] = (flag[i] != 0) || !isfinite(data[i]);
}

__global__ __launch_bounds__(256) void k_st_hit(StArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (t >= a.nt) return;
  const int j = a.axis == 0 ? f : t;
  const int64_t stride = a.axis == 0 ? a.nt : 1;
  const int64_t base = a.axis == 0 ? (int64_t)t : (int64_t)f * a.nt;
  double ds = 0.0, cs = 0.0;
  for (int i = j - a.m + 1; i <= j; ++i) {  // samples below 0 repeat sample 0
    const int64_t o = base + (int64_t)max(i, 0) * stride;
    const bool fl = a.flag[o] != 0;
    const double d = fl ? 0.0 : a.data[o];
    double c = fl ? 0.0 : 1.0;
    if (a.var) c = c * a.var[o];  // 0 * NaN stays NaN: a NaN variance under a flag makes the comparison false
    ds = ds + d;
    cs = cs + c;
  }
  if (a.correct) cs = __dsqrt_rn(cs);
  const double lhs = a.positive ? ds : fabs(ds);
  a.hit[(int64_t)f * a.nt + t] = lhs > cs * a.thr;
}

__global__ __launch_bounds__(256) void k_st_spread(StArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (t >= a.nt) return;
  const int i = a.axis == 0 ? f : t, n = a.axis == 0 ? a.nf : a.nt;
  const int64_t stride = a.axis == 0 ? a.nt : 1;
  const int64_t base = a.axis == 0 ? (int64_t)t : (int64_t)f * a.nt;
  bool any = false;
  for (int j = i; j <= min(i + a.m - 1, n - 1); ++j) any = any || a.hit[base + (int64_t)j * stride] != 0;  // a hit at j flags j - m + 1 ... j
  if (any) a.flag[(int64_t)f * a.nt + t] = 1;
}

// ---------------------------------------------------------------- scale-invariant rank

struct SirArgs {
  const uint8_t* flag;
  uint8_t* out;
  double* S;   // [n][nline] running sums S_1 ... S_n
  double* MP;  // [n][nline] minimum of S_0 ... S_i
  double em1;  // eta - 1
  int64_t stride_line, stride_elem;
  int nline, n, accumulate;
};

__global__ __launch_bounds__(kWave) void k_sir(SirArgs a) {
  const int l = blockIdx.x * kWave + threadIdx.x;
  if (l >= a.nline) return;
  const uint8_t* fl = a.flag + (int64_t)l * a.stride_line;
  uint8_t* out = a.out + (int64_t)l * a.stride_line;
  double s = 0.0, mn = 0.0;
  for (int i = 0; i < a.n; ++i) {
    a.MP[(int64_t)i * a.nline + l] = mn;
    const double v = (fl[(int64_t)i * a.stride_elem] ? 1.0 : 0.0) + a.em1;
    s = s + v;
    a.S[(int64_t)i * a.nline + l] = s;
    mn = s < mn ? s : mn;
  }
  // the reference's running maximum from the right leaves the last sum out for every sample but the last
  double rm = 0.0;
  for (int i = a.n - 1; i >= 0; --i) {
    double mx;
    if (i == a.n - 1) {
      mx = a.S[(int64_t)i * a.nline + l];
    } else {
      const double si = a.S[(int64_t)i * a.nline + l];
      rm = (i == a.n - 2) ? si : (si > rm ? si : rm);
      mx = rm;
    }
    const uint8_t res = (fl[(int64_t)i * a.stride_elem] != 0) || (mx >= a.MP[(int64_t)i * a.nline + l]);
    uint8_t* o = out + (int64_t)i * a.stride_elem;
    *o = a.accumulate ? (uint8_t)((*o != 0) || res) : res;
  }
}

// The same for lines that lie along memory (SIR along time: stride_elem = 1, adjacent lanes nt bytes apart).  A block
// is one wave on 64 lines; flags and results pass through a 64 x 64 byte tile in LDS, so every global access is a run
// of 64 contiguous bytes of one line and lane l walks row l of the tile (rows 68 bytes apart: no bank conflict).
__global__ __launch_bounds__(kWave) void k_sir_rows(SirArgs a) {
  __shared__ uint8_t tile[kWave][kWave + 4];
  const int lane = threadIdx.x, l0 = blockIdx.x * kWave, l = l0 + lane;
  const bool live = l < a.nline;
  const int rows = min(kWave, a.nline - l0);
  double s = 0.0, mn = 0.0;
  for (int i0 = 0; i0 < a.n; i0 += kWave) {
    const int len = min(kWave, a.n - i0);
    for (int r = 0; r < rows; ++r)
      if (lane < len) tile[r][lane] = a.flag[(int64_t)(l0 + r) * a.stride_line + i0 + lane];
    __syncthreads();
    if (live) {
      for (int k = 0; k < len; ++k) {
        const int64_t o = (int64_t)(i0 + k) * a.nline + l;
        a.MP[o] = mn;
        const double v = (tile[lane][k] ? 1.0 : 0.0) + a.em1;
        s = s + v;
        a.S[o] = s;
        mn = s < mn ? s : mn;
      }
    }
    __syncthreads();
  }
  double rm = 0.0;
  for (int i0 = ((a.n - 1) / kWave) * kWave; i0 >= 0; i0 -= kWave) {
    const int len = min(kWave, a.n - i0);
    for (int r = 0; r < rows; ++r)
      if (lane < len) tile[r][lane] = a.flag[(int64_t)(l0 + r) * a.stride_line + i0 + lane];
    __syncthreads();
    if (live) {
      for (int k = len - 1; k >= 0; --k) {
        const int i = i0 + k;
        const int64_t o = (int64_t)i * a.nline + l;
        const double si = a.S[o];
        double mx = si;
        if (i != a.n - 1) {
          rm = (i == a.n - 2) ? si : (si > rm ? si : rm);
          mx = rm;
        }
        tile[lane][k] = (tile[lane][k] != 0) || (mx >= a.MP[o]);
      }
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      if (lane < len) {
        uint8_t* o = a.out + (int64_t)(l0 + r) * a.stride_line + i0 + lane;
        *o = a.accumulate ? (uint8_t)((*o != 0) || tile[r][lane]) : tile[r][lane];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- elementwise stages

__global__ __launch_bounds__(256) void k_absdev(const double* yr, const double* mr, const double* yi, const double* mi, int64_t n, double* dy, double* ady) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double dr = yr[i] - mr[i];
  if (dy) dy[i] = dr;
  ady[i] = yi ? hypot(dr, yi[i] - mi[i]) : fabs(dr);
}

// the deviation from the weighted median in expected standard deviations: w is the inverse variance
__global__ __launch_bounds__(256) void k_wdev(const double* y, const double* med, const double* w, int64_t n, double* dy, double* ady) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double d = (y[i] - med[i]) * __dsqrt_rn(w[i]);
  dy[i] = d;
  if (ady) ady[i] = fabs(d);
}

__global__ __launch_bounds__(256) void k_nsigma(const double* ady, const double* mad, double scale, double nsigma, double nan_fill, int divide, int64_t n, double* ratio,
                                                double* var, uint8_t* mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s = scale * mad[i];
  double r;
  if (divide) {
    r = ady[i] / s;
  } else {
    const double inv = s == 0.0 ? 0.0 : 1.0 / s;  // invert_no_zero: a reciprocal, then a product
    r = ady[i] * inv;
  }
  if (r != r && nan_fill == nan_fill) r = nan_fill;
  ratio[i] = r;
  if (var) var[i] = s * s;
  if (mask) mask[i] = r > nsigma;
}

struct TvArgs {
  const double* x;
  const int32_t* row_chan;   // [nf] the channel whose fraction a row keeps, -1: none
  const int32_t* chan_ptr;   // [nchan + 1]
  const int32_t* chan_rows;  // rows of every channel
  const double* chan_thr;    // [nchan]
  float* frac;
  uint8_t* mask;
  float f;
  int nf, nt, nchan, nrows;
};

__global__ __launch_bounds__(256) void k_tv_flag(TvArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (t >= a.nt) return;
  const int c = a.row_chan[f];
  float fr = 1.0f;
  if (c >= 0 && c < a.nchan) {
    const int p0 = max(0, min(a.chan_ptr[c], a.nrows)), p1 = max(p0, min(a.chan_ptr[c + 1], a.nrows));
    const double thr = a.chan_thr[c];
    int cnt = 0;
    for (int p = p0; p < p1; ++p) {
      const int r = max(0, min(a.chan_rows[p], a.nf - 1));
      cnt += a.x[(int64_t)r * a.nt + t] > thr;
    }
    fr = (float)((double)cnt / (double)(p1 - p0));
  }
  const int64_t o = (int64_t)f * a.nt + t;
  if (a.frac) a.frac[o] = fr;
  a.mask[o] = fr > a.f;
}

__global__ __launch_bounds__(256) void k_mask_op(int op, const uint8_t* x, const uint8_t* y, const uint8_t* z, int64_t n, uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool xb = x[i] != 0, yb = y[i] != 0;
  bool r;
  if (op == DMM_RFI_OR)
    r = xb || yb;
  else
    r = z[i] ? xb : yb;
  out[i] = r;
}

__global__ __launch_bounds__(256) void k_rows(double* y, uint8_t* flag, const double* sub, const uint8_t* rflag, int nt) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (t >= nt) return;
  const int64_t o = (int64_t)f * nt + t;
  if (sub) y[o] = y[o] - sub[f];
  if (rflag && rflag[f]) flag[o] = 1;
}

__global__ __launch_bounds__(256) void k_radiometer(const float* meas, const float* rad, const float* w, int nf, int npol, int nt, double* y, uint8_t* flag) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const int f = blockIdx.y / npol, p = blockIdx.y % npol;
  const int64_t i = ((int64_t)f * npol + p) * nt + t, o = ((int64_t)p * nf + f) * nt + t;
  const float r = rad[i];
  const float inv = r == 0.f ? 0.f : 1.0f / r;  // the ratio is a float32
  y[o] = (double)(meas[i] * inv);
  flag[o] = w[i] == 0.f;
}

struct ApplyArgs {
  float* weight;
  const uint8_t* mask;
  const int32_t* data_idx;  // [nsel] samples of the weight's last axis
  const int32_t* mask_idx;  // [nsel] the mask sample each of them reads
  int64_t dims[4];          // leading axes of the weight
  int64_t mstride[4];       // the mask's element stride along each of them (0: broadcast)
  int64_t mstride_t, nrow;
  int nt, nsel, nmask;
};

__global__ __launch_bounds__(256) void k_apply_mask(ApplyArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.nsel) return;
  for (int64_t row = blockIdx.y; row < a.nrow; row += gridDim.y) {
    int64_t rem = row, mo = 0;
    for (int d = 3; d >= 0; --d) {
      mo += (rem % a.dims[d]) * a.mstride[d];
      rem /= a.dims[d];
    }
    const int td = max(0, min(a.data_idx[k], a.nt - 1)), tm = max(0, min(a.mask_idx[k], a.nmask - 1));
    float* w = a.weight + row * a.nt + td;
    *w = *w * (a.mask[mo + (int64_t)tm * a.mstride_t] ? 0.f : 1.f);
  }
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int dmm_rfi_medfilt(dmm_ctx* ctx, const double* x, const uint8_t* flag, int nplane, int nf, int nt, int size_f, int size_t_, double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_medfilt: ctx is NULL");
  DMM_REQUIRE(nplane >= 0 && nf >= 0 && nt >= 0, "dmm_rfi_medfilt: bad sizes nplane=%d nf=%d nt=%d", nplane, nf, nt);
  DMM_REQUIRE(size_f >= 1 && size_t_ >= 1 && (size_f & 1) && (size_t_ & 1), "dmm_rfi_medfilt: window sizes must be odd and positive, got (%d, %d)", size_f, size_t_);
  DMM_REQUIRE(size_f <= DMM_RFI_MAX_WINDOW && size_t_ <= DMM_RFI_MAX_WINDOW && (int64_t)size_f * size_t_ <= DMM_RFI_MAX_STRIP,
              "dmm_rfi_medfilt: window (%d, %d) beyond the supported bound: each size at most %d, their product at most %d", size_f, size_t_, DMM_RFI_MAX_WINDOW,
              DMM_RFI_MAX_STRIP);
  if (nplane == 0 || nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(x && flag && out, "dmm_rfi_medfilt: NULL argument");
  DMM_REQUIRE(nplane <= 65535 && nf <= 65535, "dmm_rfi_medfilt: nplane %d or nf %d does not fit the grid (65535)", nplane, nf);
  const int rows = std::min(size_f, nf);
  const int T = std::max(1, std::min(kMedTile, DMM_RFI_MAX_STRIP / rows - (size_t_ - 1)));
  const int cols = std::min(T + size_t_ - 1, nt);
  DMM_REQUIRE((int64_t)rows * cols <= DMM_RFI_MAX_STRIP, "dmm_rfi_medfilt: strip of %d x %d does not fit", rows, cols);
  DMM_HIP(hipSetDevice(ctx->device));
  MedArgs a{x, flag, out, nf, nt, size_f / 2, size_t_ / 2, T};
  const size_t lds = (size_t)rows * cols * sizeof(uint64_t) + (size_t)cols * sizeof(int);
  DMM_HIP(hipFuncSetAttribute((const void*)k_medfilt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_medfilt, dim3((unsigned)((nt + T - 1) / T), (unsigned)nf, (unsigned)nplane), dim3(kMedThreads), lds, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_wmedfilt(dmm_ctx* ctx, const double* x, const double* w, int nplane, int nf, int nt, int size_f, int size_t_, double* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_wmedfilt: ctx is NULL");
  DMM_REQUIRE(nplane >= 0 && nf >= 0 && nt >= 0, "dmm_rfi_wmedfilt: bad sizes nplane=%d nf=%d nt=%d", nplane, nf, nt);
  DMM_REQUIRE(size_f >= 1 && size_t_ >= 1 && (size_f & 1) && (size_t_ & 1), "dmm_rfi_wmedfilt: window sizes must be odd and positive, got (%d, %d)", size_f, size_t_);
  DMM_REQUIRE(size_f <= DMM_RFI_WMED_MAX_WINDOW && size_t_ <= DMM_RFI_WMED_MAX_WINDOW && (int64_t)size_f * size_t_ <= DMM_RFI_WMED_MAX_STRIP,
              "dmm_rfi_wmedfilt: window (%d, %d) beyond the supported bound: each size at most %d, their product at most %d", size_f, size_t_,
              DMM_RFI_WMED_MAX_WINDOW, DMM_RFI_WMED_MAX_STRIP);
  if (nplane == 0 || nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(x && w && out, "dmm_rfi_wmedfilt: NULL argument");
  DMM_REQUIRE(nplane <= 65535 && nf <= 65535, "dmm_rfi_wmedfilt: nplane %d or nf %d does not fit the grid (65535)", nplane, nf);
  const int rows = std::min(size_f, nf);
  const int T = std::max(1, std::min(DMM_RFI_WMED_TILE, DMM_RFI_WMED_MAX_STRIP / rows - (size_t_ - 1)));
  const int cols = std::min(T + size_t_ - 1, nt);
  DMM_REQUIRE((int64_t)rows * cols <= DMM_RFI_WMED_MAX_STRIP, "dmm_rfi_wmedfilt: strip of %d x %d does not fit", rows, cols);
  DMM_HIP(hipSetDevice(ctx->device));
  WMedArgs a{x, w, out, nf, nt, size_f / 2, size_t_ / 2, T};
  const size_t lds = (size_t)rows * cols * (sizeof(uint64_t) + sizeof(double)) + (size_t)cols * sizeof(int);
  const dim3 grid((unsigned)((nt + T - 1) / T), (unsigned)nf, (unsigned)nplane);
  const int wcols = std::min(size_t_, nt);  // columns of one output's window, 64 per lane and pass
  if (wcols <= 4 * kWave) {
    DMM_HIP(hipFuncSetAttribute((const void*)k_wmedfilt<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_wmedfilt<4>, grid, dim3(kMedThreads), lds, ctx->stream, a);
  } else if (wcols <= 10 * kWave) {
    DMM_HIP(hipFuncSetAttribute((const void*)k_wmedfilt<10>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_wmedfilt<10>, grid, dim3(kMedThreads), lds, ctx->stream, a);
  } else {
    static_assert(DMM_RFI_WMED_MAX_WINDOW <= 16 * kWave, "columns per lane");
    DMM_HIP(hipFuncSetAttribute((const void*)k_wmedfilt<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_wmedfilt<16>, grid, dim3(kMedThreads), lds, ctx->stream, a);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_quantile(dmm_ctx* ctx, const double* y, const uint8_t* flag, int64_t nrow, int n, double q, double* out, int32_t* count) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_quantile: ctx is NULL");
  DMM_REQUIRE(nrow >= 0 && nrow <= 0x7fffffff, "dmm_rfi_quantile: bad nrow %lld", (long long)nrow);
  DMM_REQUIRE(n >= 0 && n <= DMM_RFI_MAX_ROW, "dmm_rfi_quantile: row length %d outside 0 ... %d", n, DMM_RFI_MAX_ROW);
  DMM_REQUIRE(q >= 0.0 && q <= 1.0, "dmm_rfi_quantile: quantile %g outside [0, 1]", q);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(out && (n == 0 || (y && flag)), "dmm_rfi_quantile: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const size_t lds = (size_t)std::max(n, 1) * sizeof(uint64_t);
  DMM_HIP(hipFuncSetAttribute((const void*)k_quantile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_quantile, dim3((unsigned)nrow), dim3(kWave), lds, ctx->stream, y, flag, n, q, out, count);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_sumthreshold(dmm_ctx* ctx, const double* data, const double* variance, uint8_t* flag, uint8_t* hit, int nf, int nt, int nstep, const int32_t* window,
                         const int32_t* axis, const double* threshold, int correct_for_missing, int only_positive) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_sumthreshold: ctx is NULL");
  DMM_REQUIRE(nf >= 0 && nt >= 0 && nf <= 65535, "dmm_rfi_sumthreshold: bad sizes nf=%d nt=%d", nf, nt);
  DMM_REQUIRE(nstep >= 0 && nstep <= 4096, "dmm_rfi_sumthreshold: bad step count %d", nstep);
  if (nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(data && flag && hit && (nstep == 0 || (window && axis && threshold)), "dmm_rfi_sumthreshold: NULL argument");
  for (int s = 0; s < nstep; ++s) {
    DMM_REQUIRE(window[s] >= 1 && window[s] <= DMM_RFI_MAX_ST_WINDOW, "dmm_rfi_sumthreshold: window %d of step %d outside 1 ... %d", window[s], s, DMM_RFI_MAX_ST_WINDOW);
    DMM_REQUIRE(axis[s] == 0 || axis[s] == 1, "dmm_rfi_sumthreshold: bad axis %d of step %d", axis[s], s);
  }
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t n = (int64_t)nf * nt;
  hipLaunchKernelGGL(k_st_init, dim3(blocks256(n)), dim3(256), 0, ctx->stream, data, flag, n);
  const dim3 grid(blocks256(nt), (unsigned)nf);
  for (int s = 0; s < nstep; ++s) {
    StArgs a{data, variance, flag, hit, threshold[s], nf, nt, window[s], axis[s], correct_for_missing ? 1 : 0, only_positive ? 1 : 0};
    hipLaunchKernelGGL(k_st_hit, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_st_spread, grid, dim3(256), 0, ctx->stream, a);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_sir(dmm_ctx* ctx, const uint8_t* flag, int nf, int nt, int axis, double eta, int accumulate, double* work, uint8_t* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_sir: ctx is NULL");
  DMM_REQUIRE(nf >= 0 && nt >= 0, "dmm_rfi_sir: bad sizes nf=%d nt=%d", nf, nt);
  DMM_REQUIRE(axis == 0 || axis == 1, "dmm_rfi_sir: bad axis %d", axis);
  DMM_REQUIRE(eta == eta, "dmm_rfi_sir: eta is NaN");
  if (nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(flag && work && out, "dmm_rfi_sir: NULL argument");
  DMM_REQUIRE(flag != out, "dmm_rfi_sir: the output may not be the input");
  DMM_HIP(hipSetDevice(ctx->device));
  SirArgs a{};
  a.flag = flag;
  a.out = out;
  a.nline = axis == 0 ? nt : nf;
  a.n = axis == 0 ? nf : nt;
  a.S = work;
  a.MP = work + (int64_t)a.n * a.nline;
  a.em1 = eta - 1.0;
  a.stride_line = axis == 0 ? 1 : nt;
  a.stride_elem = axis == 0 ? nt : 1;
  a.accumulate = accumulate ? 1 : 0;
  const dim3 grid((unsigned)((a.nline + kWave - 1) / kWave));
  if (axis == 1)  // lines along memory: through the LDS tile
    hipLaunchKernelGGL(k_sir_rows, grid, dim3(kWave), 0, ctx->stream, a);
  else  // adjacent lanes on adjacent lines: coalesced as it stands
    hipLaunchKernelGGL(k_sir, grid, dim3(kWave), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_absdev(dmm_ctx* ctx, const double* y, const double* med, const double* y_imag, const double* med_imag, int64_t n, double* dy, double* ady) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_absdev: ctx is NULL");
  DMM_REQUIRE(n >= 0 && n <= ((int64_t)1 << 39), "dmm_rfi_absdev: bad count %lld", (long long)n);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(y && med && ady, "dmm_rfi_absdev: NULL argument");
  DMM_REQUIRE((y_imag != nullptr) == (med_imag != nullptr), "dmm_rfi_absdev: the imaginary parts come both or not at all");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_absdev, dim3(blocks256(n)), dim3(256), 0, ctx->stream, y, med, y_imag, med_imag, n, dy, ady);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_wdev(dmm_ctx* ctx, const double* y, const double* med, const double* w, int64_t n, double* dy, double* ady) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_wdev: ctx is NULL");
  DMM_REQUIRE(n >= 0 && n <= ((int64_t)1 << 39), "dmm_rfi_wdev: bad count %lld", (long long)n);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(y && med && w && dy, "dmm_rfi_wdev: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_wdev, dim3(blocks256(n)), dim3(256), 0, ctx->stream, y, med, w, n, dy, ady);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_nsigma(dmm_ctx* ctx, const double* ady, const double* mad, double scale, double nsigma, double nan_fill, int divide, int64_t n, double* ratio,
                   double* variance, uint8_t* mask) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_nsigma: ctx is NULL");
  DMM_REQUIRE(n >= 0 && n <= ((int64_t)1 << 39), "dmm_rfi_nsigma: bad count %lld", (long long)n);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(ady && mad && ratio, "dmm_rfi_nsigma: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_nsigma, dim3(blocks256(n)), dim3(256), 0, ctx->stream, ady, mad, scale, nsigma, nan_fill, divide ? 1 : 0, n, ratio, variance, mask);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_tv_flag(dmm_ctx* ctx, const double* x, int nf, int nt, const int32_t* row_chan, int nchan, const int32_t* chan_ptr, const int32_t* chan_rows, int nrows,
                    const double* chan_thr, double f, float* frac, uint8_t* mask) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_tv_flag: ctx is NULL");
  DMM_REQUIRE(nf >= 0 && nt >= 0 && nf <= 65535, "dmm_rfi_tv_flag: bad sizes nf=%d nt=%d", nf, nt);
  DMM_REQUIRE(nchan >= 0 && nrows >= 0, "dmm_rfi_tv_flag: bad channel table sizes nchan=%d nrows=%d", nchan, nrows);
  if (nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(x && row_chan && chan_ptr && mask && (nrows == 0 || chan_rows) && (nchan == 0 || chan_thr), "dmm_rfi_tv_flag: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  TvArgs a{x, row_chan, chan_ptr, chan_rows, chan_thr, frac, mask, (float)f, nf, nt, nchan, nrows};
  hipLaunchKernelGGL(k_tv_flag, dim3(blocks256(nt), (unsigned)nf), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_mask_op(dmm_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, const uint8_t* c, int64_t n, uint8_t* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_mask_op: ctx is NULL");
  DMM_REQUIRE(op == DMM_RFI_OR || op == DMM_RFI_SELECT, "dmm_rfi_mask_op: bad operation %d", op);
  DMM_REQUIRE(n >= 0 && n <= ((int64_t)1 << 39), "dmm_rfi_mask_op: bad count %lld", (long long)n);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(a && b && out && (op != DMM_RFI_SELECT || c), "dmm_rfi_mask_op: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_mask_op, dim3(blocks256(n)), dim3(256), 0, ctx->stream, op, a, b, c, n, out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_rows(dmm_ctx* ctx, double* y, uint8_t* flag, const double* row_sub, const uint8_t* row_flag, int nf, int nt) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_rows: ctx is NULL");
  DMM_REQUIRE(nf >= 0 && nt >= 0 && nf <= 65535, "dmm_rfi_rows: bad sizes nf=%d nt=%d", nf, nt);
  if (nf == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE((!row_sub || y) && (!row_flag || flag), "dmm_rfi_rows: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_rows, dim3(blocks256(nt), (unsigned)nf), dim3(256), 0, ctx->stream, y, flag, row_sub, row_flag, nt);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_radiometer(dmm_ctx* ctx, const float* measured, const float* radiometer, const float* weight, int nf, int npol, int nt, double* y, uint8_t* flag) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_radiometer: ctx is NULL");
  DMM_REQUIRE(nf >= 0 && npol >= 0 && nt >= 0 && (int64_t)nf * npol <= 65535, "dmm_rfi_radiometer: bad sizes nf=%d npol=%d nt=%d", nf, npol, nt);
  if (nf == 0 || npol == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(measured && radiometer && weight && y && flag, "dmm_rfi_radiometer: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_radiometer, dim3(blocks256(nt), (unsigned)(nf * npol)), dim3(256), 0, ctx->stream, measured, radiometer, weight, nf, npol, nt, y, flag);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_rfi_apply_mask(dmm_ctx* ctx, float* weight, int ndim, const int64_t* dims, int nt, const uint8_t* mask, const int64_t* mask_stride, int64_t mask_stride_t,
                       int nmask, int nsel, const int32_t* data_index, const int32_t* mask_index) {
  DMM_REQUIRE(ctx != nullptr, "dmm_rfi_apply_mask: ctx is NULL");
  DMM_REQUIRE(ndim >= 0 && ndim <= 4, "dmm_rfi_apply_mask: %d leading axes, at most 4", ndim);
  DMM_REQUIRE(nt >= 0 && nmask >= 0 && nsel >= 0, "dmm_rfi_apply_mask: bad sizes nt=%d nmask=%d nsel=%d", nt, nmask, nsel);
  DMM_REQUIRE(ndim == 0 || (dims && mask_stride), "dmm_rfi_apply_mask: NULL argument");
  ApplyArgs a{};
  a.nrow = 1;
  for (int d = 0; d < 4; ++d) {
    a.dims[d] = 1;
    a.mstride[d] = 0;
  }
  for (int d = 0; d < ndim; ++d) {
    DMM_REQUIRE(dims[d] >= 0 && dims[d] <= 0x7fffffff && mask_stride[d] >= 0, "dmm_rfi_apply_mask: bad axis %d", d);
    a.dims[4 - ndim + d] = dims[d];
    a.mstride[4 - ndim + d] = mask_stride[d];
    a.nrow *= dims[d];
  }
  DMM_REQUIRE(mask_stride_t >= 0, "dmm_rfi_apply_mask: bad mask stride");
  if (a.nrow == 0 || nsel == 0 || nt == 0) return DMM_OK;
  DMM_REQUIRE(nmask >= 1, "dmm_rfi_apply_mask: the mask has no samples");
  DMM_REQUIRE(weight && mask && data_index && mask_index, "dmm_rfi_apply_mask: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  a.weight = weight;
  a.mask = mask;
  a.data_idx = data_index;
  a.mask_idx = mask_index;
  a.mstride_t = mask_stride_t;
  a.nt = nt;
  a.nsel = nsel;
  a.nmask = nmask;
  hipLaunchKernelGGL(k_apply_mask, dim3(blocks256(nsel), (unsigned)std::min<int64_t>(a.nrow, 65535)), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
