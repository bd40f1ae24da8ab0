// Source stacking (draco/analysis/sourcestack.py:17-211, draco/analysis/beamform.py:915-1302): pencil beams out of a ring
// map at the pixels of a catalogue, the frequency stack of formed beams, and the 3-D stack of ring-map patches.
//
//   dmm_ringmap_extract   beam[s][p][f] = map[p][f][ra_s][el_s], weight likewise or inz(rms[p][f][ra_s])^2: a pure copy
//   dmm_source_stack      S[p][b] = sum_s sum_{f in bin b of s} w_eff beam, W = sum w_eff, stack = S inz(W)
//   dmm_ringmap_stack3d   the same over the (2 num_ra + 1) x (2 num_dec + 1) pixels around every source
//
// Traffic model of the extract kernel.  A source reads npol nfreq isolated 8-byte elements, one per (p, f) plane of
// nra nel elements: no two of them share a cache line, and at catalogue densities (one source in tens of pixels)
// neighbouring sources do not either, so the read side costs one 64-byte sector per element whatever the kernel does.
// What the kernel can choose is where the reads of one wave fall: with lanes along (p, f) they are a plane (tens of MB)
// apart, 64 translations and 64 DRAM pages per wave; with lanes along sources visited in pixel order (`order`, sorted
// by ra nel + el on the host) they fall within a few KB of one plane.  So the READ side has lanes along sources, and the
// WRITE side goes through LDS to become whole lines: a block reads a tile of 64 sources x 32 (p, f), turns it in LDS and
// stores 256 contiguous bytes of each source's row where the catalogue has the source.  Model bytes: nsrc npol nfreq
// (64 read + 8 written) per dataset.
//
// Bin membership.  The bin of a frequency for a source is np.digitize(freq[f] - source_freq, edges): the kernels do
// the same float64 subtraction and the same comparison against the same edges (IEEE makes them identical), but ask the
// question the other way round -- which run of channels falls into bin b -- by bisection over the monotonic frequency
// axis.  (freq[f] - s is monotonic in f because rounding is; so is "edge <= x" in x.)
//
// Sums have a fixed order and no floating-point atomics: one owner per output element sums the sources of a chunk of
// kSrcChunk (a compile-time constant) in catalogue order, and k_stack_combine adds the chunks' partial sums one after the
// other onto a running sum.  How many chunks one pass holds (the workspace) does not change a bit of the result.
#include <math.h>

#include "dmm_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSrcChunk = DMM_STACK_SRC_CHUNK;

__device__ __forceinline__ double inz(double x) { return x != 0.0 ? 1.0 / x : 0.0; }

// Block (tile of kTS visited sources, tile of kTP (p, f)): lanes along sources to read, along (p, f) to write.
constexpr int kTS = 64, kTP = 32;
__global__ __launch_bounds__(kThreads) void k_rm_extract(int npf, int nfreq, int nra, int nel, const double* __restrict__ map, const double* __restrict__ wsrc, int rms,
                                                         int64_t nsrc, const int32_t* __restrict__ ra_ind, const int32_t* __restrict__ el_ind,
                                                         const int32_t* __restrict__ order, double* __restrict__ beam, double* __restrict__ weight) {
  __shared__ double t_b[kTS][kTP + 1], t_w[kTS][kTP + 1];
  __shared__ int64_t t_row[kTS];  // where the catalogue has the tile's sources (-1: no such source)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kTS + lane;
  const int pf0 = blockIdx.y * kTP;
  int64_t s = -1, pix = -1;
  int ri = 0;
  if (i < nsrc) {
    s = order ? (int64_t)order[i] : i;
    if (s < 0 || s >= nsrc) s = -1;
  }
  if (s >= 0) {
    ri = ra_ind[s];
    const int ei = el_ind[s];
    if ((unsigned)ri < (unsigned)nra && (unsigned)ei < (unsigned)nel) pix = (int64_t)ri * nel + ei;  // (else: zeros)
  }
  if (wave == 0) t_row[lane] = s;
  const int64_t plane = (int64_t)nra * nel;
#pragma unroll
  for (int q = wave; q < kTP; q += kThreads / 64) {
    const int pf = pf0 + q;
    double b = 0.0, w = 0.0;
    if (pf < npf && pix >= 0) {
      b = map[pf * plane + pix];
      if (rms) {
        const double r = inz(wsrc[(int64_t)pf * nra + ri]);
        w = r * r;
      } else {
        w = wsrc[pf * plane + pix];
      }
    }
    t_b[lane][q] = b;
    t_w[lane][q] = w;
  }
  __syncthreads();
  const int q = threadIdx.x & (kTP - 1), pf = pf0 + q;
  if (pf >= npf) return;
  for (int r = threadIdx.x / kTP; r < kTS; r += kThreads / kTP) {
    const int64_t row = t_row[r];
    if (row < 0) continue;
    beam[row * npf + pf] = t_b[r][q];
    weight[row * npf + pf] = t_w[r][q];
  }
}

// The frequency axis as the bisection walks it: position j of the walk is channel j, or nfreq - 1 - j when `rev`.
struct FreqWalk {
  const double* freq;  // (LDS)
  int nfreq, rev, asc;  // asc: the edges ascend (a channel is at or past an edge when edge <= x), else edge > x
  __device__ __forceinline__ bool past(int j, double sf, double edge) const {
    const double x = freq[rev ? nfreq - 1 - j : j] - sf;
    return asc ? edge <= x : edge > x;
  }
  // first position whose channel is at or past `edge` (nfreq: none)
  __device__ __forceinline__ int first(double sf, double edge) const {
    int lo = 0, hi = nfreq;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (past(mid, sf, edge))
        hi = mid;
      else
        lo = mid + 1;
    }
    return lo;
  }
};

struct StackArgs {
  int npol, nfreq, nstack, freq_desc, bins_asc, uniform;
  const double *beam, *weight, *freq, *sfreq, *bins;
  const uint8_t* smask;
  int64_t nsrc;
};

// Block (chunk of sources, tile of 256 (p, b)): thread (p, b) sums bin b of polarisation p over the chunk's sources in
// catalogue order, per source first (as np.bincount does), then onto the chunk's sum.
__global__ __launch_bounds__(kThreads) void k_stack_partial(StackArgs a, int64_t chunk0, double* __restrict__ partial) {
  extern __shared__ double s_tab[];
  double* s_freq = s_tab;
  double* s_bins = s_tab + a.nfreq;
  for (int k = threadIdx.x; k < a.nfreq; k += kThreads) s_freq[k] = a.freq[k];
  for (int k = threadIdx.x; k <= a.nstack; k += kThreads) s_bins[k] = a.bins[k];
  __syncthreads();
  const int n = a.npol * a.nstack;
  const int t = blockIdx.y * kThreads + threadIdx.x;
  if (t >= n) return;
  const int p = t / a.nstack, b = t - p * a.nstack;
  const double e0 = s_bins[b], e1 = s_bins[b + 1];
  const FreqWalk walk{s_freq, a.nfreq, (a.freq_desc != 0) == (a.bins_asc != 0), a.bins_asc};
  const int64_t c = chunk0 + blockIdx.x;
  const int64_t s0 = c * kSrcChunk, s1 = s0 + kSrcChunk < a.nsrc ? s0 + kSrcChunk : a.nsrc;
  double S = 0.0, W = 0.0;
  for (int64_t s = s0; s < s1; ++s) {
    if (a.smask && !a.smask[s]) continue;
    const double sf = a.sfreq[s];
    const int j0 = walk.first(sf, e0), j1 = walk.first(sf, e1);
    if (j1 <= j0) continue;
    const int f0 = walk.rev ? a.nfreq - j1 : j0, f1 = walk.rev ? a.nfreq - j0 : j1;
    const int64_t row = (s * a.npol + p) * a.nfreq;
    double ss = 0.0, sw = 0.0;
    for (int f = f0; f < f1; ++f) {
      const double w = a.weight[row + f];
      const double we = a.uniform ? (w > 0.0 ? 1.0 : 0.0) : w;
      ss += we * a.beam[row + f];
      sw += we;
    }
    S += ss;
    W += sw;
  }
  const int64_t o = (int64_t)blockIdx.x * 2 * n;
  partial[o + t] = S;
  partial[o + n + t] = W;
}

// running[q][t] (+)= partial[c][q][t] for c = 0 ... nchunk - 1 in that order; with `final` element t = (b, rest) of
// nb x nrest goes to stack / weight [rest][b].
__global__ __launch_bounds__(kThreads) void k_stack_combine(const double* __restrict__ partial, int64_t nchunk, int64_t n, int first, int final, int nb,
                                                            double* __restrict__ running, double* __restrict__ stack, double* __restrict__ weight) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= n) return;
  double S = first ? 0.0 : running[t], W = first ? 0.0 : running[n + t];
  for (int64_t c = 0; c < nchunk; ++c) {
    S += partial[c * 2 * n + t];
    W += partial[c * 2 * n + n + t];
  }
  running[t] = S;
  running[n + t] = W;
  if (final) {
    const int64_t nrest = n / nb, b = t / nrest, o = (t - b * nrest) * nb + b;
    stack[o] = S * inz(W);
    weight[o] = W;
  }
}

// fixed-order sum over the block: lanes by butterfly, then the four waves in order; every thread gets the sum
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // (the previous sum's readers are done)
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

struct Stack3dArgs {
  int npol, nfreq, nra, nel, nbins, num_ra, num_dec, ra_wraps, freq_desc, rms, mode;
  const double *map, *wsrc, *wdec, *freq, *edges, *sfreq;
  const int32_t *ra_ind, *el_ind;
  int64_t nsrc;
};

// Block (tile of 256 patch pixels, (bin, pol), chunk of sources): thread = one output element, summed over the chunk's
// sources in catalogue order.  The patch variance (mode "patch") is a two-pass block reduction over the whole clipped
// patch, which every tile of the patch repeats.
__global__ __launch_bounds__(kThreads) void k_stack3d_partial(Stack3dArgs a, int64_t chunk0, double* __restrict__ partial) {
  extern __shared__ double s_tab[];
  __shared__ double s_red[4];
  double* s_freq = s_tab;
  for (int k = threadIdx.x; k < a.nfreq; k += kThreads) s_freq[k] = a.freq[k];
  __syncthreads();
  const int nrp = 2 * a.num_ra + 1, ndp = 2 * a.num_dec + 1, npatch = nrp * ndp;
  const int b = blockIdx.y / a.npol, p = blockIdx.y - b * a.npol;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const int dr = e / ndp, de = e - dr * ndp;
  const double e0 = a.edges[b], e1 = a.edges[b + 1];
  const FreqWalk walk{s_freq, a.nfreq, a.freq_desc, 1};
  const int64_t c = chunk0 + blockIdx.z;
  const int64_t s0 = c * kSrcChunk, s1 = s0 + kSrcChunk < a.nsrc ? s0 + kSrcChunk : a.nsrc;
  double S = 0.0, W = 0.0;
  for (int64_t s = s0; s < s1; ++s) {  // (everything that decides the trip counts is the same in every thread)
    const int ri = a.ra_ind[s], ei = a.el_ind[s];
    if ((unsigned)ri >= (unsigned)a.nra || (unsigned)ei >= (unsigned)a.nel) continue;
    const double sf = a.sfreq[s];
    const int j0 = walk.first(sf, e0), j1 = walk.first(sf, e1);
    if (j1 <= j0) continue;
    const int f0 = walk.rev ? a.nfreq - j1 : j0, f1 = walk.rev ? a.nfreq - j0 : j1;
    // this thread's pixel
    const int el = ei - a.num_dec + de;
    int ra = ri - a.num_ra + dr;
    if (a.ra_wraps) ra = ra < 0 ? ra + a.nra : (ra >= a.nra ? ra - a.nra : ra);
    const bool ok = e < npatch && (unsigned)el < (unsigned)a.nel && (unsigned)ra < (unsigned)a.nra;
    for (int f = f0; f < f1; ++f) {
      const int64_t plane = (int64_t)p * a.nfreq + f;
      double wvar = 0.0;
      if (a.mode == DMM_STACK3D_PATCH) {
        const int r_lo = a.ra_wraps ? 0 : (a.num_ra - ri > 0 ? a.num_ra - ri : 0), r_hi = a.ra_wraps ? nrp : (a.nra - ri + a.num_ra < nrp ? a.nra - ri + a.num_ra : nrp);
        const int d_lo = a.num_dec - ei > 0 ? a.num_dec - ei : 0, d_hi = a.nel - ei + a.num_dec < ndp ? a.nel - ei + a.num_dec : ndp;
        const double cnt = (double)(r_hi - r_lo) * (double)(d_hi - d_lo);
        double mean = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
          double acc = 0.0;
          for (int q = threadIdx.x; q < npatch; q += kThreads) {
            const int qr = q / ndp, qd = q - qr * ndp;
            if (qr < r_lo || qr >= r_hi || qd < d_lo || qd >= d_hi) continue;
            int qra = ri - a.num_ra + qr;
            if (a.ra_wraps) qra = qra < 0 ? qra + a.nra : (qra >= a.nra ? qra - a.nra : qra);
            const double x = a.map[(plane * a.nra + qra) * a.nel + (ei - a.num_dec + qd)];
            acc += pass ? (x - mean) * (x - mean) : x;
          }
          const double tot = block_sum(acc, s_red);
          if (pass)
            wvar = inz(tot / cnt);
          else
            mean = tot / cnt;
        }
      }
      if (!ok) continue;
      const int64_t row = plane * a.nra + ra;
      const double x = a.map[row * a.nel + el];
      double w;
      if (a.rms) {
        const double r = inz(a.wsrc[row]);
        w = r * r;
      } else {
        w = a.wsrc[row * a.nel + el];
      }
      if (a.mode == DMM_STACK3D_PATCH)
        w = w != 0.0 ? wvar : 0.0;
      else if (a.mode == DMM_STACK3D_DEC)
        w = w != 0.0 ? a.wdec[plane * a.nel + el] : 0.0;
      S += x * w;
      W += w;
    }
  }
  if (e >= npatch) return;
  const int64_t n = (int64_t)a.nbins * a.npol * npatch;
  const int64_t t = ((int64_t)b * a.npol + p) * npatch + e;
  const int64_t o = (int64_t)blockIdx.z * 2 * n;
  partial[o + t] = S;
  partial[o + n + t] = W;
}

}  // namespace

extern "C" {

int dmm_ringmap_extract(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, const double* map, const double* wsrc, int rms, int64_t nsrc, const int32_t* ra_ind,
                        const int32_t* el_ind, const int32_t* order, double* beam, double* weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ringmap_extract: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && npol <= 4, "dmm_ringmap_extract: polarisation count %d outside 1 ... 4", npol);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= 65535, "dmm_ringmap_extract: frequency count %d outside 1 ... 65535", nfreq);
  DMM_REQUIRE(nra >= 1, "dmm_ringmap_extract: bad ra count %d", nra);
  DMM_REQUIRE(nel >= 1, "dmm_ringmap_extract: bad el count %d", nel);
  DMM_REQUIRE(rms == 0 || rms == 1, "dmm_ringmap_extract: unknown weight source %d", rms);
  DMM_REQUIRE(nsrc >= 0, "dmm_ringmap_extract: bad source count %lld", (long long)nsrc);
  DMM_REQUIRE(nsrc <= 0x7fffffff, "dmm_ringmap_extract: too many sources: %lld", (long long)nsrc);
  if (nsrc == 0) return DMM_OK;  // nothing to do
  DMM_REQUIRE(map && wsrc && ra_ind && el_ind && beam && weight, "dmm_ringmap_extract: NULL argument");
  const int npf = npol * nfreq;
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_rm_extract, dim3((unsigned)((nsrc + kTS - 1) / kTS), (unsigned)((npf + kTP - 1) / kTP)), dim3(kThreads), 0, ctx->stream, npf, nfreq, nra, nel, map, wsrc, rms, nsrc, ra_ind, el_ind, order, beam, weight);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_source_stack(dmm_ctx* ctx, int64_t nsrc, int npol, int nfreq, int nstack, const double* beam, const double* weight, const double* freq, int freq_descending,
                     const double* sfreq, const uint8_t* smask, const double* bins, int bins_ascending, int uniform, double* partial, int64_t partial_chunks,
                     double* running, double* stack, double* out_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_source_stack: ctx is NULL");
  DMM_REQUIRE(nsrc >= 0, "dmm_source_stack: bad source count %lld", (long long)nsrc);
  DMM_REQUIRE(npol >= 1 && npol <= 4, "dmm_source_stack: polarisation count %d outside 1 ... 4", npol);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= DMM_STACK_MAX_FREQ, "dmm_source_stack: frequency count %d outside 1 ... %d", nfreq, DMM_STACK_MAX_FREQ);
  DMM_REQUIRE(nstack >= 1 && nstack <= nfreq, "dmm_source_stack: stack length %d outside 1 ... %d", nstack, nfreq);
  DMM_REQUIRE(partial_chunks >= 1, "dmm_source_stack: room for %lld chunks of partial sums", (long long)partial_chunks);
  DMM_REQUIRE(freq && bins && partial && running && stack && out_weight, "dmm_source_stack: NULL argument");
  DMM_REQUIRE(nsrc == 0 || (beam && weight && sfreq), "dmm_source_stack: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t n = (int64_t)npol * nstack;
  const unsigned ntile = (unsigned)((n + kThreads - 1) / kThreads), nblk = (unsigned)((n + kThreads - 1) / kThreads);
  const size_t lds = sizeof(double) * ((size_t)nfreq + nstack + 1);
  const StackArgs a{npol, nfreq, nstack, freq_descending != 0, bins_ascending != 0, uniform != 0, beam, weight, freq, sfreq, bins, smask, nsrc};
  const int64_t nchunk = (nsrc + kSrcChunk - 1) / kSrcChunk;
  int64_t c0 = 0;
  do {  // (no sources: one pass over no chunks writes the zeros)
    int64_t nc = nchunk - c0 < partial_chunks ? nchunk - c0 : partial_chunks;
    if (nc > 65535) nc = 65535;
    if (nc > 0) {
      hipLaunchKernelGGL(k_stack_partial, dim3((unsigned)nc, ntile), dim3(kThreads), lds, ctx->stream, a, c0, partial);
      DMM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_stack_combine, dim3(nblk), dim3(kThreads), 0, ctx->stream, (const double*)partial, nc, n, c0 == 0, c0 + nc >= nchunk, 1, running, stack, out_weight);
    DMM_HIP(hipGetLastError());
    c0 += nc;
  } while (c0 < nchunk);
  return DMM_OK;
}

int dmm_ringmap_stack3d(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, const double* map, const double* wsrc, int rms, int mode, const double* wdec, int64_t nsrc,
                        const int32_t* ra_ind, const int32_t* el_ind, const double* sfreq, const double* freq, int freq_descending, int nbins, const double* edges,
                        int num_ra, int num_dec, int ra_wraps, double* partial, int64_t partial_chunks, double* running, double* stack, double* out_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ringmap_stack3d: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && npol <= 4, "dmm_ringmap_stack3d: polarisation count %d outside 1 ... 4", npol);
  DMM_REQUIRE(nfreq >= 1 && nfreq <= DMM_STACK_MAX_FREQ, "dmm_ringmap_stack3d: frequency count %d outside 1 ... %d", nfreq, DMM_STACK_MAX_FREQ);
  DMM_REQUIRE(nra >= 1, "dmm_ringmap_stack3d: bad ra count %d", nra);
  DMM_REQUIRE(nel >= 1, "dmm_ringmap_stack3d: bad el count %d", nel);
  DMM_REQUIRE(rms == 0 || rms == 1, "dmm_ringmap_stack3d: unknown weight source %d", rms);
  DMM_REQUIRE(mode >= DMM_STACK3D_INPUT && mode <= DMM_STACK3D_PATCH, "dmm_ringmap_stack3d: unknown weight mode %d", mode);
  DMM_REQUIRE(nsrc >= 0, "dmm_ringmap_stack3d: bad source count %lld", (long long)nsrc);
  DMM_REQUIRE(nbins >= 1 && (int64_t)nbins * npol <= 65535, "dmm_ringmap_stack3d: bin count %d outside 1 ... %d", nbins, 65535 / npol);
  DMM_REQUIRE(num_ra >= 0 && num_ra <= (nra - 1) / 2, "dmm_ringmap_stack3d: a patch of %lld pixels is longer than the ra axis (%d)", 2 * (long long)num_ra + 1, nra);
  DMM_REQUIRE(num_dec >= 0 && num_dec <= (nel - 1) / 2, "dmm_ringmap_stack3d: a patch of %lld pixels is longer than the el axis (%d)", 2 * (long long)num_dec + 1, nel);
  DMM_REQUIRE(partial_chunks >= 1, "dmm_ringmap_stack3d: room for %lld chunks of partial sums", (long long)partial_chunks);
  DMM_REQUIRE(freq && edges && partial && running && stack && out_weight, "dmm_ringmap_stack3d: NULL argument");
  DMM_REQUIRE(mode != DMM_STACK3D_DEC || wdec, "dmm_ringmap_stack3d: NULL argument");
  DMM_REQUIRE(nsrc == 0 || (map && wsrc && ra_ind && el_ind && sfreq), "dmm_ringmap_stack3d: NULL argument");
  const int64_t npatch = (2 * (int64_t)num_ra + 1) * (2 * (int64_t)num_dec + 1);
  DMM_REQUIRE(npatch <= (int64_t)kThreads * 65535 && npatch * nbins * npol <= 0x7fffffff, "dmm_ringmap_stack3d: the stack of %lld x %d x %d elements is too large",
              (long long)npatch, nbins, npol);
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t n = npatch * nbins * npol;
  const unsigned ntile = (unsigned)((npatch + kThreads - 1) / kThreads), nblk = (unsigned)((n + kThreads - 1) / kThreads);
  const size_t lds = sizeof(double) * (size_t)nfreq;
  const Stack3dArgs a{npol, nfreq, nra, nel, nbins, num_ra, num_dec, ra_wraps != 0, freq_descending != 0, rms, mode, map, wsrc, wdec, freq, edges, sfreq, ra_ind, el_ind, nsrc};
  const int64_t nchunk = (nsrc + kSrcChunk - 1) / kSrcChunk;
  int64_t c0 = 0;
  do {  // (no sources: one pass over no chunks writes the zeros)
    int64_t nc = nchunk - c0 < partial_chunks ? nchunk - c0 : partial_chunks;
    if (nc > 65535) nc = 65535;
    if (nc > 0) {
      hipLaunchKernelGGL(k_stack3d_partial, dim3(ntile, (unsigned)(nbins * npol), (unsigned)nc), dim3(kThreads), lds, ctx->stream, a, c0, partial);
      DMM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_stack_combine, dim3(nblk), dim3(kThreads), 0, ctx->stream, (const double*)partial, nc, n, c0 == 0, c0 + nc >= nchunk, nbins, running, stack, out_weight);
    DMM_HIP(hipGetLastError());
    c0 += nc;
  } while (c0 < nchunk);
  return DMM_OK;
}

}  // extern "C"
