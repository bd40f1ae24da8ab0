// Batched beam-transfer contractions over (m, freq) tiles.
//
//   k_dirty    a = B^H (Ni o v)     DirtyMapMaker._solve_m     reference mapmaker.py:156-168
//   k_project  v = B a              bt.project_vector_sky_to_telescope as called at
//                                   reference stream.py:109-112 [driftscan, 3P]
//
// This is THE bandwidth kernel of the path: B_m[f] (ntel x npol*(lmax+1-m) complex) is
// read exactly once per solve and is ~99 % of the bytes, so the
// design goal is nothing but streaming B at the HBM rate:
//   * a block = one tile x 256*CPL adjacent output columns; each of its 4 waves owns 64*CPL
//     columns and walks down ALL ntel rows, so every wave-load is one contiguous
//     1 KiB piece of a B row (16 B per lane) and there is NO cross-lane or cross-wave
//     reduction -- each lane keeps its own complex accumulator in registers;
//   * w = Ni o v (ntel complex doubles, <= 24 KB) is formed once per block in LDS and
//     read back as a wave-uniform broadcast, the l<m columns are never touched;
//   * rows are issued UNROLL deep so 8 x 1 KiB per wave are in flight: with the default of one
//     4-wave block per CU that is the ~32 KB per CU the HBM latency-bandwidth product needs;
//   * the grid is ONE block per CU (`grid_mult` more) whose blocks draw their tasks from a
//     prefix-summed task list through a device counter (`dirty_static`: they stride over it), each
//     task found by a scalar binary search, so uneven tiles (the triangle in m) stay balanced.
// Accumulation is always float64, whatever the storage type of B.
#include "dmm_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct SolveParams {
  const dmm_tile* tiles;
  const int32_t* work_start;  // [ntile+1]
  int64_t ntile;
  int64_t nwork;
  int npairs, ntel, npol, lmax, nfreq, n_m;
  int full_layout;  // 1: tile [ntel, npol, lmax+1]; 0: [ntel, npol, lmax+1-m]
  // "w mode" (Wiener / ML back-projection): w comes from wbuf[t * ntel + i] instead of Ni o v, the output is scaled by
  // Sl[l] if given
  const double2* wbuf;
  const double* Sl;
  // dynamic task hand-out: a device counter (zeroed before the launch) from which blocks draw their next task, so a
  // CU slowed down by a neighbour on another stream simply takes fewer tasks; nullptr = static striding
  unsigned long long* ticket;
  int prio;  // 1: the kernel's waves raise their issue priority (s_setprio 3) over whatever shares their SIMDs
  // 1: the structural zeros l < m are NOT written -- for an a_lm that never leaves the library (the map-makers' slab loop:
  // the Legendre synthesis reads l >= m alone); half of the square a_lm's bytes, written beside the stream of B
  int nofill;
};

__device__ __forceinline__ int64_t find_tile(const int32_t* __restrict__ ws, int64_t ntile, int64_t w) {
  int64_t lo = 0, hi = ntile;  // largest t with ws[t] <= w
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ws[mid] <= w) lo = mid; else hi = mid;
  }
  return lo;
}

// The block's next task (none left: >= p.nwork): drawn from the ticket, or `strided` = blockIdx.x + k * gridDim.x.
// Every thread of the block calls it, once per task, and meets a barrier between two calls.
__device__ __forceinline__ int64_t take_task(const SolveParams& p, int64_t strided) {
  __shared__ unsigned long long s_next;
  if (!p.ticket) return strided;
  // (the previous task's reads of s_next all happened before its second barrier: thread 0 may overwrite it)
  if (threadIdx.x == 0) s_next = atomicAdd(p.ticket, 1ull);
  __syncthreads();
  return (int64_t)s_next;
}

// Where a tile's columns and rows lie, in B and in the two arrays around it
struct TileGeom {
  const SolveParams& p;
  int m, f;
  int L, ncol;         // l = m .. lmax per polarisation; npol * L columns
  int pol_stride;      // elements between two polarisations of a row of B
  int col0;            // first stored column of l = m
  int64_t row_stride;  // elements between two rows of B
  int64_t b_off;
  __device__ __forceinline__ TileGeom(const SolveParams& p_, const dmm_tile& tile)
      : p(p_), m(tile.m), f(tile.f), L(p_.lmax + 1 - tile.m), ncol(p_.npol * L), pol_stride(p_.full_layout ? p_.lmax + 1 : L),
        col0(p_.full_layout ? tile.m : 0), row_stride((int64_t)p_.npol * pol_stride), b_off(tile.b_off) {}
  // alm[nfreq, npol, n_m, lmax+1]
  __device__ __forceinline__ int64_t alm_at(int pol, int l) const { return (((int64_t)f * p.npol + pol) * p.n_m + m) * (p.lmax + 1) + l; }
  // mvis / mweight [n_m, 2, nfreq, npairs]: row i of the tile is baseline i (+m half), then baseline i - npairs (-m half)
  __device__ __forceinline__ int64_t vis_at(int i) const {
    const int s = i >= p.npairs, pp = i - s * p.npairs;
    return (((int64_t)m * 2 + s) * p.nfreq + f) * p.npairs + pp;
  }
};

typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// NT: non-temporal (streaming) load -- B is read exactly once, keep it out of the caches' way
template <typename BT, bool NT = false>
__device__ __forceinline__ void load_b(const BT* p, double& re, double& im) {
  if constexpr (sizeof(BT) == 16) {
    const v2d v = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p)) : *reinterpret_cast<const v2d*>(p);
    re = v.x;
    im = v.y;
  } else {
    const v2f v = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2f*>(p)) : *reinterpret_cast<const v2f*>(p);
    re = (double)v.x;
    im = (double)v.y;
  }
}

// CPL adjacent columns per lane.  CPL == 2 exists only for packed complex64 tiles whose
// rows are 16-byte aligned (plan->pair_ok): one 16-byte load brings both columns.
// Loads return the RAW register image (no conversion): what is prefetched stays untouched until it is consumed.
template <typename BT, int CPL> struct RawOf;
template <> struct RawOf<double2, 1> { typedef v2d type; };
template <> struct RawOf<float2, 1> { typedef v2f type; };
template <> struct RawOf<float2, 2> { typedef v4f type; };

template <typename BT, int CPL, bool NT>
__device__ __forceinline__ typename RawOf<BT, CPL>::type load_raw(const BT* p, const int64_t (&off)[CPL], int64_t roff) {
  typedef typename RawOf<BT, CPL>::type R;
  const R* q = reinterpret_cast<const R*>(p + off[0] + roff);
  return NT ? __builtin_nontemporal_load(q) : *q;
}

// acc += conj(b) * w for the CPL columns of one raw row piece
template <typename BT, int CPL>
__device__ __forceinline__ void accumulate(const typename RawOf<BT, CPL>::type& r, const double2 wv, double (&are)[CPL], double (&aim)[CPL]) {
  double br[CPL], bi[CPL];
  if constexpr (CPL == 2) {
    br[0] = (double)r.x; bi[0] = (double)r.y; br[1] = (double)r.z; bi[1] = (double)r.w;
  } else {
    br[0] = (double)r.x; bi[0] = (double)r.y;
  }
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    are[c] = fma(br[c], wv.x, fma(bi[c], wv.y, are[c]));
    aim[c] = fma(br[c], wv.y, fma(-bi[c], wv.x, aim[c]));
  }
}

// The CPL adjacent output columns of a lane (columns past the tile's last are clamped onto it and not stored)
template <int CPL>
struct ColSet {
  int64_t off[CPL];  // element of row 0 in B
  bool ok[CPL];
  int opol[CPL], ol[CPL];
  __device__ __forceinline__ ColSet(const TileGeom& g, int jbase) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int j = jbase + c;
      ok[c] = j < g.ncol;
      const int jj = ok[c] ? j : g.ncol - 1;
      opol[c] = jj / g.L;
      const int lrel = jj - opol[c] * g.L;
      ol[c] = g.m + lrel;
      off[c] = g.b_off + (int64_t)opol[c] * g.pol_stride + g.col0 + lrel;
    }
  }
};

// All ntel rows of a lane's columns, in row order: `group(r, i)` takes the raw pieces of the kUnroll rows from i on,
// `row(r, i)` the piece of row i alone.
// PIPE: software-pipelined -- the loads of the NEXT kUnroll rows are issued before the current ones are
// consumed.  With one wave per SIMD nothing else hides the arithmetic (4 f64 FMAs per 16 bytes at complex128, 8 + 4
// conversions at complex64): unpipelined, every group of rows cost a memory latency PLUS its arithmetic.
template <typename BT, int CPL, bool NT, int kUnroll, bool PIPE, typename RowFn, typename GroupFn>
__device__ __forceinline__ void row_loop(const BT* __restrict__ B, const int64_t (&off)[CPL], int64_t row_stride, int ntel,
                                         const RowFn& row, const GroupFn& group) {
  typedef typename RawOf<BT, CPL>::type Raw;
  int i = 0;
  if constexpr (!PIPE) {  // the first version's loop (complex128's default, and kept for A/B: `dirty_variant` 7)
    for (; i + kUnroll <= ntel; i += kUnroll) {
      Raw r[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) r[u] = load_raw<BT, CPL, NT>(B, off, (int64_t)(i + u) * row_stride);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row(r[u], i + u);
    }
  } else if (ntel >= kUnroll) {
    Raw ra[kUnroll], rb[kUnroll];  // ping-pong register sets: no copies between iterations
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) ra[u] = load_raw<BT, CPL, NT>(B, off, (int64_t)u * row_stride);
    // invariant at the top: ra holds rows i .. i+kUnroll-1 (in flight or arrived)
    // The scheduling barriers keep every group's loads in ONE burst ahead of the arithmetic.  Left to itself the
    // compiler threads the loads between the FMAs; beside the SHT kernels of the side stream (which keep the f64
    // pipe busy) the FMAs stall and hold the loads behind them back: 37.9 instead of 31.4 ms per launch in the step.
    for (; i + 3 * kUnroll <= ntel; i += 2 * kUnroll) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) rb[u] = load_raw<BT, CPL, NT>(B, off, (int64_t)(i + kUnroll + u) * row_stride);
      __builtin_amdgcn_sched_barrier(0);
      group(ra, i);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) ra[u] = load_raw<BT, CPL, NT>(B, off, (int64_t)(i + 2 * kUnroll + u) * row_stride);
      __builtin_amdgcn_sched_barrier(0);
      group(rb, i + kUnroll);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (i + 2 * kUnroll <= ntel) {  // one more full group behind the one in ra
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) rb[u] = load_raw<BT, CPL, NT>(B, off, (int64_t)(i + kUnroll + u) * row_stride);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row(ra[u], i + u);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row(rb[u], i + kUnroll + u);
      i += 2 * kUnroll;
    } else {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) row(ra[u], i + u);
      i += kUnroll;
    }
  }
  for (; i < ntel; ++i) row(load_raw<BT, CPL, NT>(B, off, (int64_t)i * row_stride), i);
}

template <int ND>
struct MultiPtrs {  // the ND days of one launch (w mode: alm[0] alone is used)
  const double2* mvis[ND];
  const double* mweight[ND];
  double2* alm[ND];
};

// a_d[pol, l] = sum_i conj(B[i, pol, l]) * Ni_d[i] * v_d[i] for ND sidereal days d against ONE read of B
// (BaseMapMaker.process_many; the reference calls mapmaker.py:79-94 once per pipeline item against the same beam
// transfers); ND = 1 is the single day.  ND complex accumulators per column, and w = Ni o v of the ND days side by
// side in LDS ([ntel][ND], wave-uniform broadcasts).  Per 16 bytes of B: 4 ND f64 FMAs, so the kernel leaves the HBM
// roofline for the FP64 one near ND = 16.  Every day's column is accumulated over the rows in the same order by the
// same FMA chain whatever ND: the results of one launch are bit-identical to those of ND single-day launches.
template <typename BT, int CPL, int ND, bool WMODE, bool NT, int kUnroll, bool PIPE>
__global__ __launch_bounds__(kThreads) void k_dirty(SolveParams p, const BT* __restrict__ B, MultiPtrs<ND> q) {
  static_assert(!WMODE || ND == 1, "w mode has one right-hand side per tile");
  extern __shared__ __align__(16) unsigned char smem[];
  double2* w = reinterpret_cast<double2*>(smem);  // [ntel][ND]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntel = p.ntel;
  if (p.prio) __builtin_amdgcn_s_setprio(3);

  // (the ticket's task replaces the loop variable itself: with a second variable beside the strided one the compiler
  // runs the task loop under an exec mask and parks seven more scalars in VGPR lanes at ND = 8)
  for (int64_t work = blockIdx.x;; work += gridDim.x) {
    work = take_task(p, work);
    if (work >= p.nwork) break;
    const int64_t t = find_tile(p.work_start, p.ntile, work);
    const TileGeom g(p, p.tiles[t]);
    const int cb = (int)(work - p.work_start[t]);

    __syncthreads();  // previous task's readers of w are done
    // (all ND days of a baseline by one thread, their 2 ND loads in flight together: ntel / 256 rounds of memory
    // latency per task whatever ND -- one day after the other it was ND times that, a third of the task's time at ND = 8)
    for (int i = threadIdx.x; i < ntel; i += kThreads) {
      if constexpr (WMODE) {
        w[i] = p.wbuf[t * ntel + i];
      } else {
        const int64_t o = g.vis_at(i);
        double2 v[ND];
        double ni[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          v[d] = q.mvis[d][o];
          ni[d] = q.mweight[d][o];
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) w[i * ND + d] = make_double2(ni[d] * v[d].x, ni[d] * v[d].y);
      }
    }
    __syncthreads();

    // structural zeros l < m (mapmaker.py:76 zero fill): written by the first column block
    if (cb == 0 && !p.nofill)
      for (int idx = threadIdx.x; idx < p.npol * g.m; idx += kThreads) {
        const int pol = idx / g.m, l = idx - pol * g.m;
        const int64_t o = g.alm_at(pol, l);
#pragma unroll
        for (int d = 0; d < ND; ++d) q.alm[d][o] = make_double2(0.0, 0.0);
      }

    const int jbase = (cb * kWaves + wave) * 64 * CPL + lane * CPL;
    if (jbase >= g.ncol) continue;  // tail lanes/waves idle; they still meet the barriers above
    const ColSet<CPL> cs(g, jbase);
    double are[ND][CPL], aim[ND][CPL];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
      for (int c = 0; c < CPL; ++c) are[d][c] = aim[d][c] = 0.0;

    typedef typename RawOf<BT, CPL>::type Raw;
    auto row = [&](const Raw& r, int i) __attribute__((always_inline)) {
      const double2* wr = w + i * ND;
#pragma unroll
      for (int d = 0; d < ND; ++d) accumulate<BT, CPL>(r, wr[d], are[d], aim[d]);
    };
    auto group = [&](const Raw (&r)[kUnroll], int i0) __attribute__((always_inline)) {
      if constexpr (ND == 1) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) row(r[u], i0 + u);
      } else {
        // the ND broadcast reads of row u + 1 are issued before the 4 ND FMAs of row u, so that with one wave per SIMD
        // the LDS latency hides under arithmetic instead of being paid once per row
        double2 wa[ND], wb[ND];
        const double2* wr = w + i0 * ND;
#pragma unroll
        for (int d = 0; d < ND; ++d) wa[d] = wr[d];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (u + 1 < kUnroll) {
#pragma unroll
            for (int d = 0; d < ND; ++d) (u & 1 ? wa : wb)[d] = wr[(u + 1) * ND + d];
          }
#pragma unroll
          for (int d = 0; d < ND; ++d) accumulate<BT, CPL>(r[u], (u & 1 ? wb : wa)[d], are[d], aim[d]);
        }
      }
    };
    row_loop<BT, CPL, NT, kUnroll, PIPE>(B, cs.off, g.row_stride, ntel, row, group);

#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (cs.ok[c]) {
        const int64_t o = g.alm_at(cs.opol[c], cs.ol[c]);
        const double sc = (WMODE && p.Sl) ? p.Sl[cs.ol[c]] : 1.0;
#pragma unroll
        for (int d = 0; d < ND; ++d) q.alm[d][o] = make_double2(sc * are[d][c], sc * aim[d][c]);
      }
  }
}

// The a_lm of a tile into LDS for the project kernels: a[npol * L] in packed (pol, l-m) order
__device__ __forceinline__ void stage_alm(const TileGeom& g, const double2* __restrict__ alm, double2* a) {
  __syncthreads();  // previous task's readers of a are done
  for (int j = threadIdx.x; j < g.ncol; j += kThreads) {
    const int pol = j / g.L, lrel = j - pol * g.L;
    a[j] = alm[g.alm_at(pol, g.m + lrel)];
  }
  __syncthreads();
}

// v[i] = sum_{pol,l} B[i, pol, l] * a[pol, l]: one wave per row, lanes across the
// contiguous row (coalesced), shuffle reduction; a (<= 64 KB) staged in LDS per block.
template <typename BT, bool NT = false, int UNR = 4>
__global__ __launch_bounds__(kThreads) void k_project(SolveParams p, const BT* __restrict__ B,
                                                      const double2* __restrict__ alm,
                                                      double2* __restrict__ vis) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* a = reinterpret_cast<double2*>(smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // (static striding: with 64-row tasks the dynamic hand-out of k_dirty costs more than it balances, 5.9 vs 6.1 TB/s)
  for (int64_t work = blockIdx.x; work < p.nwork; work += gridDim.x) {
    const int64_t t = find_tile(p.work_start, p.ntile, work);
    const TileGeom g(p, p.tiles[t]);
    const int rb = (int)(work - p.work_start[t]);  // block of 64 rows
    stage_alm(g, alm, a);
    for (int rr = wave; rr < 64; rr += kWaves) {
      const int i = rb * 64 + rr;
      if (i >= p.ntel) break;
      const BT* row = B + g.b_off + (int64_t)i * g.row_stride + g.col0;
      double sre = 0.0, sim = 0.0;
      for (int pol = 0; pol < p.npol; ++pol) {
        const BT* seg = row + (int64_t)pol * g.pol_stride;
        const double2* as = a + pol * g.L;
#pragma unroll UNR
        for (int lrel = lane; lrel < g.L; lrel += 64) {
          double br, bi;
          load_b<BT, NT>(seg + lrel, br, bi);
          const double2 av = as[lrel];
          sre = fma(br, av.x, fma(-bi, av.y, sre));
          sim = fma(br, av.y, fma(bi, av.x, sim));
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        sre += __shfl_down(sre, off, 64);
        sim += __shfl_down(sim, off, 64);
      }
      if (lane == 0) vis[g.vis_at(i)] = make_double2(sre, sim);
    }
  }
}

// Row-group form of k_project: a wave works on RG rows of its task at once -- RG independent row pieces in flight per
// lane, ONE LDS read of a_lm per RG loads, and the 2 RG row sums leave the wave through one reduce-scatter butterfly
// (2 RG + 3 shuffles instead of 12 per row).
template <int NV>
__device__ __forceinline__ void proj_wave_sums(double (&x)[NV], int lane) {  // as wave_sums of herm_tridiag.h
  int bit = 0;
#pragma unroll
  for (int h = NV / 2; h >= 1; h >>= 1, ++bit) {
    const bool up = (lane >> bit) & 1;
#pragma unroll
    for (int k = 0; k < h; ++k) {
      double lo = x[k], hi = x[h + k];
      asm volatile("" : "+v"(lo), "+v"(hi));  // (keeps the selects from becoming one dynamically indexed register read)
      const double keep = up ? hi : lo, send = up ? lo : hi;
      x[k] = keep + __shfl_xor(send, 1 << bit);
    }
  }
#pragma unroll
  for (int o = NV; o < 64; o <<= 1) x[0] += __shfl_xor(x[0], o);
}

template <typename BT, bool NT, int RG>
__global__ __launch_bounds__(kThreads) void k_project_rg(SolveParams p, const BT* __restrict__ B,
                                                         const double2* __restrict__ alm,
                                                         double2* __restrict__ vis) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* a = reinterpret_cast<double2*>(smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kRowsPerWave = 64 / kWaves;
  static_assert(kRowsPerWave % RG == 0, "row groups must tile a wave's rows");
  for (int64_t work = blockIdx.x; work < p.nwork; work += gridDim.x) {
    const int64_t t = find_tile(p.work_start, p.ntile, work);
    const TileGeom g(p, p.tiles[t]);
    const int rb = (int)(work - p.work_start[t]);  // block of 64 rows
    stage_alm(g, alm, a);
    for (int gr = 0; gr < kRowsPerWave; gr += RG) {
      const int i0 = rb * 64 + wave * kRowsPerWave + gr;
      if (i0 >= p.ntel) break;
      const BT* row[RG];
      double acc[2 * RG];
#pragma unroll
      for (int k = 0; k < RG; ++k) {
        const int i = i0 + k < p.ntel ? i0 + k : p.ntel - 1;  // (clamped duplicates are not stored)
        row[k] = B + g.b_off + (int64_t)i * g.row_stride + g.col0;
        acc[2 * k] = acc[2 * k + 1] = 0.0;
      }
      // packed tiles: a row is npol * L contiguous elements in the order of `a` -- ONE loop over them (at m = 0, L = 513:
      // 33 wave-loads per row instead of 4 x 9 with a one-lane runt at the end of every polarisation); full-layout tiles
      // (gaps of m elements between the polarisations) keep the loop per polarisation
      const int npass = p.full_layout ? p.npol : 1;
      const int plen = p.full_layout ? g.L : g.ncol;
      for (int pol = 0; pol < npass; ++pol) {
        const int64_t so = (int64_t)pol * g.pol_stride;
        const double2* as = a + pol * g.L;
        for (int lrel = lane; lrel < plen; lrel += 64) {
          const double2 av = as[lrel];
          double br[RG], bi[RG];
#pragma unroll
          for (int k = 0; k < RG; ++k) load_b<BT, NT>(row[k] + so + lrel, br[k], bi[k]);
#pragma unroll
          for (int k = 0; k < RG; ++k) {
            acc[2 * k] = fma(br[k], av.x, fma(-bi[k], av.y, acc[2 * k]));
            acc[2 * k + 1] = fma(br[k], av.y, fma(bi[k], av.x, acc[2 * k + 1]));
          }
        }
      }
      proj_wave_sums<2 * RG>(acc, lane);
      if (lane < 2 * RG) {  // lane holds value number bitrev(lane) = 2 k + (0: re, 1: im)
        int idx = 0, nb = 0;
        for (int q = 2 * RG; q > 1; q >>= 1) ++nb;
        for (int bq = 0; bq < nb; ++bq) idx |= ((lane >> bq) & 1) << (nb - 1 - bq);
        const int i = i0 + (idx >> 1);
        if (i < p.ntel) reinterpret_cast<double*>(&vis[g.vis_at(i)])[idx & 1] = acc[0];
      }
    }
  }
}

// column-block tasks of a tile with mode m: the Dirty kernel's decomposition
int col_blocks(const dmm_plan* pl, int m) { return (pl->npol * (pl->lmax + 1 - m) + pl->cols_per_block - 1) / pl->cols_per_block; }

// tasks per tile: by column blocks (`by_cols`) or by blocks of 64 rows
int make_work(const dmm_plan* pl, bool by_cols, std::vector<int32_t>& ws, int64_t* nwork) {
  ws.resize(pl->ntile + 1);
  int64_t acc = 0;
  for (int64_t t = 0; t < pl->ntile; ++t) {
    ws[t] = (int32_t)acc;
    acc += by_cols ? col_blocks(pl, pl->tiles_h[t].m) : (2 * pl->npairs + 63) / 64;
    if (acc > 0x7fffffff) return dmm_set_error(DMM_E_UNSUPPORTED, "plan too large: split the batch");
  }
  ws[pl->ntile] = (int32_t)acc;
  *nwork = acc;
  return DMM_OK;
}

SolveParams base_params(const dmm_plan* pl) {
  SolveParams p;
  p.tiles = pl->tiles_d;
  p.work_start = pl->work_start_d;
  p.ntile = pl->ntile;
  p.nwork = pl->nwork;
  p.npairs = pl->npairs;
  p.ntel = 2 * pl->npairs;
  p.npol = pl->npol;
  p.lmax = pl->lmax;
  p.nfreq = pl->nfreq;
  p.n_m = pl->n_m;
  p.full_layout = pl->b_layout == DMM_B_FULL;
  p.wbuf = nullptr;
  p.Sl = nullptr;
  p.ticket = nullptr;
  p.prio = pl->ctx->opt_dirty_prio;
  p.nofill = 0;
  return p;
}

// One launch of a task-list kernel `kern(p, args...)` on the context's stream: grid_mult blocks per CU but no more than
// tasks, `lds` bytes of dynamic LDS, and with `ticketed` a fresh task counter for the dynamic hand-out.
template <typename Kern, typename... Args>
int launch_tasks(dmm_ctx* ctx, Kern kern, int grid_mult, size_t lds, SolveParams p, bool ticketed, Args... args) {
  int64_t grid = (int64_t)ctx->num_cu * grid_mult;
  if (grid > p.nwork) grid = p.nwork;
  if (grid <= 0) return DMM_OK;
  if (ticketed) {
    DMM_HIP(dmm_ticket(ctx, &p.ticket));
    DMM_HIP(hipMemsetAsync(p.ticket, 0, sizeof(unsigned long long), ctx->stream));
  }
  DMM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kThreads), lds, ctx->stream, p, args...);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

template <typename BT, int CPL, int ND, bool WMODE, bool NT, int kUnroll, bool PIPE = true>
int dirty_form(dmm_plan* pl, const SolveParams& p, const void* B, const MultiPtrs<ND>& q) {
  dmm_ctx* ctx = pl->ctx;
  // defaults from tools/tune_dirty.py on MI355X (profiles/r01_tune_dirty.txt): non-temporal loads, 8 row
  // loads in flight per wave and ONE 4-wave block per CU (one wave per SIMD, 32 KB in flight per CU) --
  // more resident waves only add contention at the memory side (6.7 vs 6.0 TB/s at 8 blocks per CU)
  const int gm_default = 1;
  return launch_tasks(ctx, k_dirty<BT, CPL, ND, WMODE, NT, kUnroll, PIPE>, ctx->opt_grid_mult > 0 ? ctx->opt_grid_mult : gm_default,
                      (size_t)p.ntel * ND * sizeof(double2), p, ctx->opt_dirty_static == 0, (const BT*)B, q);
}

// the forms behind `dirty_variant` (0 = shipped default); w mode has the default of each storage type alone
template <int ND, bool WMODE>
int launch_dirty(dmm_plan* pl, const SolveParams& p, const void* B, const MultiPtrs<ND>& q) {
  const int variant = WMODE ? 0 : pl->ctx->opt_dirty_variant;
  if (pl->b_dtype == DMM_C128) {
    if constexpr (ND > 1) {
      switch (variant) {  // (tools/multi_tune.py)
        case 1: return dirty_form<double2, 1, ND, false, true, 16>(pl, p, B, q);
        case 2: return dirty_form<double2, 1, ND, false, true, 4>(pl, p, B, q);
        case 3: return dirty_form<double2, 1, ND, false, false, 8>(pl, p, B, q);
        case 4: return dirty_form<double2, 1, ND, false, true, 12>(pl, p, B, q);
        default: return dirty_form<double2, 1, ND, false, true, 8>(pl, p, B, q);
      }
    } else {
      if constexpr (!WMODE) switch (variant) {  // tuning variants (tools/tune_dirty.py)
        case 1: return dirty_form<double2, 1, 1, false, false, 8>(pl, p, B, q);
        case 2: return dirty_form<double2, 1, 1, false, true, 16>(pl, p, B, q);
        case 3: return dirty_form<double2, 1, 1, false, true, 4>(pl, p, B, q);
        case 4: return dirty_form<double2, 1, 1, false, true, 12>(pl, p, B, q);
        case 7: return dirty_form<double2, 1, 1, false, true, 8>(pl, p, B, q);
        default: break;  // the shipped form below
      }
      // complex128 keeps the plain loop: prefetching a second group buys nothing with the GPU to itself (29.9 vs
      // 29.7 ms per launch, tools/step_ab.py) and its 116 registers no longer fit beside two waves of the side stream's
      // Legendre kernels on a SIMD (96 + 2 x 208 = 512): 37.4 instead of 31.6 ms per launch inside the step
      return dirty_form<double2, 1, 1, WMODE, true, 8, false>(pl, p, B, q);
    }
  } else if (pl->pair_ok) {
    if constexpr (ND > 1) {
      return dirty_form<float2, 2, ND, false, true, 8>(pl, p, B, q);
    } else {
      if constexpr (!WMODE) switch (variant) {
        case 1: return dirty_form<float2, 2, 1, false, false, 8>(pl, p, B, q);
        case 2: case 4: return dirty_form<float2, 2, 1, false, true, 8>(pl, p, B, q);
        case 3: return dirty_form<float2, 2, 1, false, true, 24>(pl, p, B, q);
        case 5: return dirty_form<float2, 2, 1, false, true, 12>(pl, p, B, q);
        case 6: return dirty_form<float2, 2, 1, false, true, 32>(pl, p, B, q);
        case 7: return dirty_form<float2, 2, 1, false, true, 8, false>(pl, p, B, q);
        default: break;  // the shipped form below
      }
      // complex64: two pipelined groups of 16 rows -- 32 KB of B in flight per wave while the 12 f64 operations per
      // 16 bytes of the group before run (tools/step_ab.py, cfg 3: 18.2 vs 21.4 ms per launch inside the step, 15.6 vs
      // 15.7 alone, against the plain groups of 8)
      return dirty_form<float2, 2, 1, WMODE, true, 16>(pl, p, B, q);
    }
  } else {
    if constexpr (ND > 1) return dirty_form<float2, 1, ND, false, true, 8>(pl, p, B, q);
    else return dirty_form<float2, 1, 1, WMODE, false, 8>(pl, p, B, q);
  }
}

template <int ND>
MultiPtrs<ND> day_ptrs(const void* const* mvis, const double* const* mweight, void* const* alm) {
  MultiPtrs<ND> q;
  for (int d = 0; d < ND; ++d) {
    q.mvis[d] = (const double2*)mvis[d];
    q.mweight[d] = mweight[d];
    q.alm[d] = (double2*)alm[d];
  }
  return q;
}

// the launch of the two compact-list entries below: the plan's parameters with the list in place of its tiles
template <bool WMODE>
int launch_dirty_list(dmm_plan* pl, const void* B, const dmm_tile* tiles_d, const int32_t* work_d, int nmat, int64_t nwork,
                      const double2* wbuf, const double* Sl, const void* mvis, const double* mweight, void* alm) {
  DMM_HIP(hipSetDevice(pl->ctx->device));
  SolveParams p = base_params(pl);
  p.tiles = tiles_d;
  p.work_start = work_d;
  p.ntile = nmat;
  p.nwork = nwork;
  p.wbuf = wbuf;
  p.Sl = Sl;
  return launch_dirty<1, WMODE>(pl, p, B, day_ptrs<1>(&mvis, &mweight, &alm));
}

template <typename BT, bool NT, int N, bool RG = true>
int project_form(dmm_plan* pl, const SolveParams& p, size_t lds, const void* B, const void* alm_in, void* vis_out) {
  dmm_ctx* ctx = pl->ctx;
  // (tools/project_timing.py: the row-group kernel is fastest with ONE block per CU, like the Dirty kernel: 6.26 TB/s)
  const int grid_mult = ctx->opt_project_grid_mult > 0 ? ctx->opt_project_grid_mult : 1;
  if constexpr (RG) return launch_tasks(ctx, k_project_rg<BT, NT, N>, grid_mult, lds, p, false, (const BT*)B, (const double2*)alm_in, (double2*)vis_out);
  else return launch_tasks(ctx, k_project<BT, NT, N>, grid_mult, lds, p, false, (const BT*)B, (const double2*)alm_in, (double2*)vis_out);
}

}  // namespace

extern "C" {

int dmm_solve_plan_create(dmm_ctx* ctx, const dmm_tile* tiles, int64_t ntile, int npairs, int npol,
                          int lmax, int nfreq, int n_m, int b_dtype, int b_layout, dmm_plan** out) {
  DMM_REQUIRE(ctx && out && (tiles || ntile == 0), "dmm_solve_plan_create: NULL argument");
  *out = nullptr;
  DMM_REQUIRE(ntile >= 0 && npairs >= 1 && npol >= 1 && lmax >= 0 && nfreq >= 1 && n_m >= 1,
              "dmm_solve_plan_create: bad sizes");
  DMM_REQUIRE(b_dtype == DMM_C64 || b_dtype == DMM_C128, "dmm_solve_plan_create: bad b_dtype %d", b_dtype);
  DMM_REQUIRE(b_layout == DMM_B_FULL || b_layout == DMM_B_PACKED, "dmm_solve_plan_create: bad b_layout %d", b_layout);
  DMM_REQUIRE((size_t)2 * npairs * sizeof(double2) <= 96 * 1024, "dmm_solve_plan_create: npairs=%d too large for the LDS stage", npairs);
  bool even_off = true;
  for (int64_t t = 0; t < ntile; ++t) {
    DMM_REQUIRE(tiles[t].m >= 0 && tiles[t].m < n_m && tiles[t].m <= lmax, "tile %lld: m=%d out of range (n_m=%d, lmax=%d)",
                (long long)t, tiles[t].m, n_m, lmax);
    DMM_REQUIRE(tiles[t].f >= 0 && tiles[t].f < nfreq, "tile %lld: f=%d out of range (nfreq=%d)", (long long)t, tiles[t].f, nfreq);
    DMM_REQUIRE(tiles[t].b_off >= 0, "tile %lld: negative b_off", (long long)t);
    even_off = even_off && (tiles[t].b_off % 2 == 0);
  }
  DMM_HIP(hipSetDevice(ctx->device));
  dmm_plan* pl = new (std::nothrow) dmm_plan();
  if (!pl) return dmm_set_error(DMM_E_NOMEM, "dmm_solve_plan_create: out of host memory");
  pl->ctx = ctx;
  pl->ntile = ntile;
  pl->npairs = npairs;
  pl->npol = npol;
  pl->lmax = lmax;
  pl->nfreq = nfreq;
  pl->n_m = n_m;
  pl->b_dtype = b_dtype;
  pl->b_layout = b_layout;
  pl->tiles_h.assign(tiles, tiles + ntile);
  const size_t es = b_dtype == DMM_C128 ? 16 : 8;
  for (int64_t t = 0; t < ntile; ++t)
    pl->b_bytes += (int64_t)2 * npairs * npol * (lmax + 1 - tiles[t].m) * (int64_t)es;
  // two columns per lane (one 16-byte load) when every packed complex64 row is 16-byte aligned
  pl->pair_ok = b_dtype == DMM_C64 && b_layout == DMM_B_PACKED && npol % 2 == 0 && even_off;
  pl->cols_per_block = kThreads * (pl->pair_ok ? 2 : 1);
  std::vector<int32_t> ws, wr;
  int rc = make_work(pl, true, ws, &pl->nwork);
  if (!rc) rc = make_work(pl, false, wr, &pl->nwork_rows);
  if (rc) {
    delete pl;
    return rc;
  }
  if (ntile > 0) {
    const size_t wb = (ntile + 1) * sizeof(int32_t);
    hipError_t e = hipMalloc((void**)&pl->tiles_d, ntile * sizeof(dmm_tile));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->work_start_d, wb);
    if (e == hipSuccess) e = hipMalloc((void**)&pl->work_rows_d, wb);
    if (e == hipSuccess) e = hipMemcpy(pl->tiles_d, tiles, ntile * sizeof(dmm_tile), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->work_start_d, ws.data(), wb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->work_rows_d, wr.data(), wb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      dmm_plan_destroy(pl);
      return dmm_set_error((int)e, "dmm_solve_plan_create: %s", hipGetErrorString(e));
    }
  }
  *out = pl;
  return DMM_OK;
}

int dmm_plan_destroy(dmm_plan* pl) {
  if (!pl) return DMM_OK;
  (void)hipSetDevice(pl->ctx->device);
  if (pl->tiles_d) (void)hipFree(pl->tiles_d);
  if (pl->work_start_d) (void)hipFree(pl->work_start_d);
  if (pl->work_rows_d) (void)hipFree(pl->work_rows_d);
  delete pl;
  return DMM_OK;
}

int64_t dmm_plan_b_bytes(const dmm_plan* pl) { return pl ? pl->b_bytes : 0; }

int dmm_dirty_run(dmm_plan* pl, const void* B, const void* mvis, const double* mweight, void* alm) {
  DMM_REQUIRE(pl && B && mvis && mweight && alm, "dmm_dirty_run: NULL argument");
  DMM_REQUIRE(((uintptr_t)B & 15) == 0 && ((uintptr_t)mvis & 15) == 0 && ((uintptr_t)alm & 15) == 0,
              "dmm_dirty_run: B, mvis and alm must be 16-byte aligned");
  if (pl->ntile == 0) return DMM_OK;
  DMM_HIP(hipSetDevice(pl->ctx->device));
  return launch_dirty<1, false>(pl, base_params(pl), B, day_ptrs<1>(&mvis, &mweight, &alm));
}

int dmm_dirty_run_multi(dmm_plan* pl, const void* B, const void* const* mvis, const double* const* mweight, void* const* alm, int nday) {
  DMM_REQUIRE(pl && B && mvis && mweight && alm, "dmm_dirty_run_multi: NULL argument");
  DMM_REQUIRE(nday >= 1, "dmm_dirty_run_multi: nday = %d", nday);
  DMM_REQUIRE(((uintptr_t)B & 15) == 0, "dmm_dirty_run_multi: B must be 16-byte aligned");
  for (int d = 0; d < nday; ++d) {
    DMM_REQUIRE(mvis[d] && mweight[d] && alm[d], "dmm_dirty_run_multi: NULL array of day %d", d);
    DMM_REQUIRE(((uintptr_t)mvis[d] & 15) == 0 && ((uintptr_t)alm[d] & 15) == 0, "dmm_dirty_run_multi: mvis and alm of day %d must be 16-byte aligned", d);
    for (int e = 0; e < d; ++e) DMM_REQUIRE(alm[e] != alm[d], "dmm_dirty_run_multi: days %d and %d share their alm", e, d);
  }
  if (pl->ntile == 0) return DMM_OK;
  DMM_HIP(hipSetDevice(pl->ctx->device));
  SolveParams p = base_params(pl);
  p.nofill = pl->ctx->opt_dirty_nofill != 0;  // (this entry alone: dmm_dirty_run and the back-projections always fill)
  // groups of 8, 4, 2 days per read of B (8 days' w = Ni o v take 8 x 12 KB of LDS at cfg 3), then a last single day
  const size_t w_day = (size_t)2 * pl->npairs * sizeof(double2);  // LDS of one day's w = Ni o v
  const int nd_max = 8 * w_day <= 128 * 1024 ? 8 : (4 * w_day <= 128 * 1024 ? 4 : (2 * w_day <= 128 * 1024 ? 2 : 1));
  int d = 0;
  while (d < nday) {
    const int left = nday - d;
    int rc;
    if (left >= 8 && nd_max >= 8) { rc = launch_dirty<8, false>(pl, p, B, day_ptrs<8>(mvis + d, mweight + d, alm + d)); d += 8; }
    else if (left >= 4 && nd_max >= 4) { rc = launch_dirty<4, false>(pl, p, B, day_ptrs<4>(mvis + d, mweight + d, alm + d)); d += 4; }
    else if (left >= 2 && nd_max >= 2) { rc = launch_dirty<2, false>(pl, p, B, day_ptrs<2>(mvis + d, mweight + d, alm + d)); d += 2; }
    else { rc = launch_dirty<1, false>(pl, p, B, day_ptrs<1>(mvis + d, mweight + d, alm + d)); d += 1; }
    if (rc) return rc;
  }
  return DMM_OK;
}

int dmm_project_run(dmm_plan* pl, const void* B, const void* alm_in, void* vis_out) {
  DMM_REQUIRE(pl && B && alm_in && vis_out, "dmm_project_run: NULL argument");
  DMM_REQUIRE(((uintptr_t)B & 15) == 0 && ((uintptr_t)alm_in & 15) == 0 && ((uintptr_t)vis_out & 15) == 0,
              "dmm_project_run: B, alm and vis must be 16-byte aligned");
  if (pl->ntile == 0) return DMM_OK;
  DMM_HIP(hipSetDevice(pl->ctx->device));
  SolveParams p = base_params(pl);
  p.work_start = pl->work_rows_d;
  p.nwork = pl->nwork_rows;
  const size_t lds = (size_t)p.npol * (p.lmax + 1) * sizeof(double2);
  if (lds > 160 * 1024)
    return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_project_run: nsky=%d too large for the LDS stage", p.npol * (p.lmax + 1));
  if (pl->b_dtype != DMM_C128) return project_form<float2, true, 8>(pl, p, lds, B, alm_in, vis_out);
  switch (pl->ctx->opt_project_variant) {  // tools/project_timing.py: row groups of 8 with NT loads: 6.26 TB/s; one row per wave (4): 5.97
    case 1: return project_form<double2, false, 4, false>(pl, p, lds, B, alm_in, vis_out);
    case 2: return project_form<double2, false, 8, false>(pl, p, lds, B, alm_in, vis_out);
    case 3: return project_form<double2, true, 8, false>(pl, p, lds, B, alm_in, vis_out);
    case 4: return project_form<double2, true, 4, false>(pl, p, lds, B, alm_in, vis_out);
    case 5: return project_form<double2, true, 4>(pl, p, lds, B, alm_in, vis_out);
    case 6: return project_form<double2, false, 8>(pl, p, lds, B, alm_in, vis_out);
    default: return project_form<double2, true, 8>(pl, p, lds, B, alm_in, vis_out);
  }
}

}  // extern "C"

void dmm_dirty_tile_list(const dmm_plan* pl, const int64_t* ids, int n, std::vector<dmm_tile>& tiles, std::vector<int32_t>& work) {
  tiles.resize(n);
  work.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    tiles[i] = pl->tiles_h[ids[i]];
    work[i + 1] = work[i] + col_blocks(pl, tiles[i].m);
  }
}

int dmm_dirty_launch_list(dmm_plan* pl, const void* B, const void* mvis, const double* mweight, const dmm_tile* tiles_d,
                          const int32_t* work_d, int nmat, int64_t nwork, void* alm) {
  return launch_dirty_list<false>(pl, B, tiles_d, work_d, nmat, nwork, nullptr, nullptr, mvis, mweight, alm);
}

int dmm_dirty_w_launch_list(dmm_plan* pl, const void* B, const double2* wbuf, const double* Sl, const dmm_tile* tiles_d,
                            const int32_t* work_d, int nmat, int64_t nwork, void* alm) {
  return launch_dirty_list<true>(pl, B, tiles_d, work_d, nmat, nwork, wbuf, Sl, nullptr, nullptr, alm);
}
