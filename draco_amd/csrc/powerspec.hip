// 3-D power spectrum of a ring-map delay cube (draco/analysis/powerspec.py:539-1017): the (RA, Dec) -> (u, v) transform
// of the delay cube, the cross / auto power spectrum and its cylindrical average.  float64 throughout.
//
//   k_uv_el / k_uv_ra   fftshift(fft2(x * (w_ra (x) w_el))) / (nra nel) per (pol, delay) plane (image_to_uv, :1585-1625)
//                       as two in-LDS row transforms planned through dmm_row_fft_plan<double> (mfft.hip, fft_lds.h).
//                       k_uv_el: a block takes one (pol, ra) and a run of RB consecutive delays of spectrum [pol][el][ra]
//                       [delay] -- reads are RB x 16 bytes contiguous per el -- tapers, transforms along el and writes
//                       whole v rows of vis [pol][delay][ra][v], fftshift applied.  k_uv_ra: a block takes one (pol,
//                       delay) and a run of RB consecutive v, transforms along ra in place in vis (every load of a block
//                       comes before its first store, blocks own disjoint columns) and stores with the fftshift of the
//                       ra axis and the 1 / (nra nel) scale.  64 bytes of traffic per cell against 32 algorithmic; the
//                       host loop goes slab by slab of delays so that the second pass finds the first one's output in
//                       the last-level cache.
//   k_ps_cross          out[p1 npol2 + p2] = ps_norm (v1[p1] conj(v2[p2]))  (:804-813), one pass.
//   k_ps_bin            the cylindrical average (:959-1000, get_2d_ps :1836-1896).  The bin of a (u, v) cell is the same
//                       for every plane: the host turns the int16 bin map into one cell list per bin, and a block sums
//                       one (plane, bin): each thread a strided share of the list, then a tree over the block.  The
//                       order is fixed by the sizes alone; every sum is carried as a pair hi + lo, so a bin's mean is
//                       good to the last bit whatever its population.
// The products and sums of k_ps_cross and k_ps_bin are not contracted into fused multiply-adds (the pragma below): the
// imaginary part of v conj(v) is then exactly zero, and the error terms of the pairs are what they are meant to be.
#include <math.h>

#include <vector>

#include "dmm_internal.h"
#include "fft_lds.h"

#pragma clang fp contract(off)

namespace {

using dmm_fft::C;
using dmm_fft::cmul;
using dmm_fft::RowFft;

constexpr int kThreads = 1024;
// up to 16 rows per block in 150 KB of LDS (four rows of 2048 points with their twiddles); one row of 8192 points reads
// its twiddles from memory
constexpr dmm_fft_sizing kSizeUv = {16, 150 * 1024, 160 * 1024, true, true};

struct UvPass {
  RowFft<double> fft;
  const double2* in;  // spectrum [npol][nel][nra][nd]
  double2* vis;       // [npol][nd][nra][nel]
  const double* w_ra;
  const double* w_el;  // both or neither
  int nel, nra, nd;
  int pol, d0, nds;  // the slab: delays d0 ... d0 + nds of this pol
  int nrun;          // runs of RB rows per ra (k_uv_el) / per delay (k_uv_ra)
  double scale;
};

// The forward transform of the rows in LDS with three radix-2 stages per pass (fft_lds.h): 4 passes over 2048 points
// where the two-stage passes take 6.  Measured on the 2 x 128 x 2048 x 512 cube, interleaved in one process: 6.81 ms
// against 7.38 ms for the whole transform, 5.77 against 6.41 ms on 2 x 32 x 1500 x 500 (Bluestein).
template <bool BLUE>
__device__ __forceinline__ void uv_forward(const RowFft<double>& q, C<double>* buf, const C<double>* tw) {
  if (BLUE) dmm_fft::bluestein_convolve<double, kThreads>(buf, tw, q.bfilt, q.RB, q.M, q.logM, q.P, true);
  else dmm_fft::fft_dif8<double, kThreads>(buf, tw, q.RB, q.M, q.logM, q.P);
}

// Along el.  Block = (ra, run of RB delays), the runs of one ra next to each other.
template <bool BLUE>
__global__ __launch_bounds__(kThreads) void k_uv_el(UvPass a) {
  extern __shared__ __align__(16) unsigned char smem[];
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  const RowFft<double>& q = a.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int ra = blockIdx.x / a.nrun, dl0 = (blockIdx.x - ra * a.nrun) * RB;
  const C<double>* tw = dmm_fft::stage_twiddles<double, kThreads, true>(q, buf + (size_t)RB * P);
  const double wr = a.w_ra ? a.w_ra[ra] : 1.0;
  const int64_t el_stride = (int64_t)a.nra * a.nd;
  const double2* src = a.in + ((int64_t)a.pol * a.nel * a.nra + ra) * a.nd + a.d0 + dl0;
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx % RB, k = idx / RB;  // consecutive threads on consecutive delays
    C<double> v = {0.0, 0.0};
    if (k < N && dl0 + r < a.nds) {
      const double2 x = src[k * el_stride + r];
      v = {x.x, x.y};
      if (a.w_ra) {
        const double t = wr * a.w_el[k];  // the outer product first, then the data (powerspec.py:1617-1618)
        v = {v.x * t, v.y * t};
      }
      if (BLUE) {
        const double2 c = q.chirp[k];
        v = cmul<double>(v, {c.x, c.y});
      }
    }
    buf[r * P + k] = v;
  }
  __syncthreads();
  uv_forward<BLUE>(q, buf, tw);
  const int h = N / 2;  // fftshift: bin k lands at (k + N / 2) mod N
  for (int idx = threadIdx.x; idx < RB * N; idx += kThreads) {
    const int r = idx / N, pos = idx - r * N;
    if (dl0 + r >= a.nds) continue;
    const int k = pos >= h ? pos - h : pos - h + N;
    const C<double> v = dmm_fft::spectrum_at<double>(buf + r * P, q.chirp, BLUE, k, q.logM);
    a.vis[(((int64_t)a.pol * a.nd + a.d0 + dl0 + r) * a.nra + ra) * a.nel + pos] = make_double2(v.x, v.y);
  }
}

// Along ra, in place.  Block = (delay, run of RB columns v), the runs of one delay next to each other.
template <bool BLUE>
__global__ __launch_bounds__(kThreads) void k_uv_ra(UvPass a) {
  extern __shared__ __align__(16) unsigned char smem[];
  C<double>* buf = reinterpret_cast<C<double>*>(smem);
  const RowFft<double>& q = a.fft;
  const int N = q.N, M = q.M, RB = q.RB, P = q.P;
  const int dl = blockIdx.x / a.nrun, v0 = (blockIdx.x - dl * a.nrun) * RB;
  const C<double>* tw = dmm_fft::stage_twiddles<double, kThreads, true>(q, buf + (size_t)RB * P);
  double2* base = a.vis + (((int64_t)a.pol * a.nd + a.d0 + dl) * a.nra) * a.nel + v0;
  for (int idx = threadIdx.x; idx < RB * M; idx += kThreads) {
    const int r = idx % RB, k = idx / RB;  // consecutive threads on consecutive columns
    C<double> v = {0.0, 0.0};
    if (k < N && v0 + r < a.nel) {
      const double2 x = base[(int64_t)k * a.nel + r];
      v = {x.x, x.y};
      if (BLUE) {
        const double2 c = q.chirp[k];
        v = cmul<double>(v, {c.x, c.y});
      }
    }
    buf[r * P + k] = v;
  }
  __syncthreads();  // (every load of the block is done: the stores below overwrite what it read, and nothing else)
  uv_forward<BLUE>(q, buf, tw);
  const int h = N / 2;
  for (int idx = threadIdx.x; idx < RB * N; idx += kThreads) {
    const int r = idx % RB, pos = idx / RB;
    if (v0 + r >= a.nel) continue;
    const int k = pos >= h ? pos - h : pos - h + N;
    const C<double> v = dmm_fft::spectrum_at<double>(buf + r * P, q.chirp, BLUE, k, q.logM);
    base[(int64_t)pos * a.nel + r] = make_double2(v.x * a.scale, v.y * a.scale);  // the one scaling, at the last store
  }
}

__global__ __launch_bounds__(256) void k_ps_cross(const double2* __restrict__ v1, const double2* __restrict__ v2, int npol2, int64_t ncell, double ps_norm,
                                                  double2* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncell) return;
  const int p = blockIdx.y, p1 = p / npol2, p2 = p - p1 * npol2;
  const double2 a = v1[p1 * ncell + c], b = v2[p2 * ncell + c];
  const double tr = a.x * b.x + a.y * b.y, ti = a.y * b.x - a.x * b.y;  // a conj(b)
  out[p * ncell + c] = make_double2(ps_norm * tr, ps_norm * ti);
}

// A sum carried as an unevaluated pair hi + lo (the rounding error of every addition goes into lo): the binned sums are
// then good to the last bit whatever the population of a bin, and the mean of a single cell is that cell.
struct Dd {
  double hi, lo;
};
__device__ __forceinline__ void dd_add(Dd& a, double x) {
  const double s = a.hi + x, bb = s - a.hi;
  a.lo += (a.hi - (s - bb)) + (x - bb);
  a.hi = s;
}
__device__ __forceinline__ void dd_add_prod(Dd& a, double w, double x) {
  const double p = w * x;
  dd_add(a, p);
  a.lo += fma(w, x, -p);
}
__device__ __forceinline__ Dd dd_merge(Dd a, Dd b) {
  Dd r = a;
  dd_add(r, b.hi);
  r.lo += b.lo;
  return r;
}
__device__ __forceinline__ Dd dd_norm(Dd a) {
  const double s = a.hi + a.lo;
  return {s, a.lo - (s - a.hi)};
}
__device__ __forceinline__ double dd_div(Dd n, Dd d) {  // (n.hi + n.lo) / (d.hi + d.lo), 0 / 0 = NaN
  const double q = n.hi / d.hi;
  const double r = fma(-q, d.hi, n.hi) + (n.lo - q * d.lo);
  return q + r / d.hi;
}

// One (plane, bin): sum w p, sum w, sum w^2 over the bin's cell list.
__global__ __launch_bounds__(256) void k_ps_bin(const double2* __restrict__ spec, const double2* __restrict__ sigma, const int32_t* __restrict__ start,
                                                const int32_t* __restrict__ cells, int64_t ncell, int nbins, double2* __restrict__ out, double* __restrict__ ow,
                                                double* __restrict__ on) {
  __shared__ Dd s[4][256];
  const int64_t plane = blockIdx.x / nbins;
  const int bin = (int)(blockIdx.x - plane * nbins);
  const int s0 = start[bin], s1 = start[bin + 1];
  const double2* __restrict__ p = spec + plane * ncell;
  const double2* __restrict__ g = sigma ? sigma + plane * ncell : nullptr;
  Dd sr = {0.0, 0.0}, si = sr, sw = sr, sw2 = sr;
  for (int j = s0 + threadIdx.x; j < s1; j += 256) {
    const int c = cells[j];
    const double2 x = p[c];
    if (g) {
      const double2 sg = g[c];
      const double m = hypot(sg.x, sg.y), m2 = m * m;  // invert_no_zero(np.abs(sigma) ** 2)
      const double w = m2 != 0.0 ? 1.0 / m2 : 0.0;
      dd_add_prod(sr, w, x.x);
      dd_add_prod(si, w, x.y);
      dd_add(sw, w);
      dd_add_prod(sw2, w, w);
    } else {
      dd_add(sr, x.x);
      dd_add(si, x.y);
      dd_add(sw, 1.0);
      dd_add(sw2, 1.0);
    }
  }
  s[0][threadIdx.x] = sr, s[1][threadIdx.x] = si, s[2][threadIdx.x] = sw, s[3][threadIdx.x] = sw2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int q = 0; q < 4; ++q) s[q][threadIdx.x] = dd_merge(s[q][threadIdx.x], s[q][threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const Dd w = dd_norm(s[2][0]), w2 = dd_norm(s[3][0]);
    const int64_t o = plane * nbins + bin;
    out[o] = make_double2(dd_div(dd_norm(s[0][0]), w), dd_div(dd_norm(s[1][0]), w));  // 0 / 0 = NaN in an empty bin, as the reference's
    ow[o] = w.hi;
    on[o] = w.hi * w.hi / w2.hi;
  }
}

bool uv_fits(int n) {
  int RB = 0, P = 0, tw_lds = 0;
  size_t lds = 0;
  bool fits = false;
  const int M = dmm_is_pow2(n) ? n : (1 << ilog2(2 * n - 1));
  dmm_row_fft_sizes(M, sizeof(double2), 1, kSizeUv, &RB, &P, &tw_lds, &lds, &fits);
  return fits;
}

}  // namespace

extern "C" {

int dmm_uv_fft2_supported(int n) { return n >= 1 && n <= DMM_MAX_NRA && uv_fits(n) ? 1 : 0; }

int dmm_uv_fft2(dmm_ctx* ctx, const void* spectrum, int npol, int nel, int nra, int ndelay, const double* w_ra, const double* w_el, void* vis, int64_t slab_mib) {
  DMM_REQUIRE(ctx != nullptr, "dmm_uv_fft2: ctx is NULL");
  DMM_REQUIRE(npol >= 1 && nel >= 1 && nra >= 1 && ndelay >= 1, "dmm_uv_fft2: bad sizes npol=%d nel=%d nra=%d ndelay=%d", npol, nel, nra, ndelay);
  DMM_REQUIRE(spectrum && vis, "dmm_uv_fft2: NULL argument");
  DMM_REQUIRE((w_ra == nullptr) == (w_el == nullptr), "dmm_uv_fft2: one taper without the other");
  DMM_REQUIRE(slab_mib >= 0, "dmm_uv_fft2: bad slab size %lld MiB", (long long)slab_mib);
  if (!dmm_uv_fft2_supported(nra)) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_uv_fft2: the ra axis of length %d does not fit the in-LDS transform", nra);
  if (!dmm_uv_fft2_supported(nel)) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_uv_fft2: the el axis of length %d does not fit the in-LDS transform", nel);
  DMM_HIP(hipSetDevice(ctx->device));
  const int64_t plane_bytes = (int64_t)nra * nel * (int64_t)sizeof(double2);
  int64_t nds = ((slab_mib ? slab_mib : 128) << 20) / plane_bytes;
  nds = nds < 1 ? 1 : (nds > ndelay ? ndelay : nds);
  UvPass e{}, r{};
  size_t lds_e = 0, lds_r = 0;
  bool fits = false;
  int rc = dmm_row_fft_plan<double>(ctx, nel, nds, kSizeUv, &e.fft, &lds_e, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_uv_fft2: nel=%d needs %zu B of LDS", nel, lds_e);
  rc = dmm_row_fft_plan<double>(ctx, nra, nel, kSizeUv, &r.fft, &lds_r, &fits);
  if (rc) return rc;
  if (!fits) return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_uv_fft2: nra=%d needs %zu B of LDS", nra, lds_r);
  e.in = (const double2*)spectrum, e.vis = (double2*)vis, e.w_ra = w_ra, e.w_el = w_el;
  e.nel = nel, e.nra = nra, e.nd = ndelay;
  e.scale = 1.0 / ((double)nra * (double)nel);
  const RowFft<double> fr = r.fft;
  r = e;
  r.fft = fr;
  for (int p = 0; p < npol; ++p)
    for (int64_t d0 = 0; d0 < ndelay; d0 += nds) {
      const int n = (int)(ndelay - d0 < nds ? ndelay - d0 : nds);
      e.pol = r.pol = p, e.d0 = r.d0 = (int)d0, e.nds = r.nds = n;
      e.nrun = (n + e.fft.RB - 1) / e.fft.RB;
      r.nrun = (nel + r.fft.RB - 1) / r.fft.RB;
      rc = dmm_launch_blocks("dmm_uv_fft2", e.fft.chirp ? k_uv_el<true> : k_uv_el<false>, (int64_t)nra * e.nrun, kThreads, lds_e, ctx->stream, e);
      if (rc) return rc;
      rc = dmm_launch_blocks("dmm_uv_fft2", r.fft.chirp ? k_uv_ra<true> : k_uv_ra<false>, (int64_t)n * r.nrun, kThreads, lds_r, ctx->stream, r);
      if (rc) return rc;
    }
  return DMM_OK;
}

int dmm_ps3d_cross(dmm_ctx* ctx, const void* vis1, const void* vis2, int npol1, int npol2, int64_t ncell, double ps_norm, void* out) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ps3d_cross: ctx is NULL");
  DMM_REQUIRE(npol1 >= 1 && npol2 >= 1 && ncell >= 1 && (int64_t)npol1 * npol2 <= 65535, "dmm_ps3d_cross: bad sizes npol1=%d npol2=%d ncell=%lld", npol1, npol2, (long long)ncell);
  DMM_REQUIRE(vis1 && vis2 && out, "dmm_ps3d_cross: NULL argument");
  const int64_t nblk = (ncell + 255) / 256;
  DMM_REQUIRE(nblk <= 0x7fffffff, "dmm_ps3d_cross: too many cells");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_ps_cross, dim3((unsigned)nblk, (unsigned)(npol1 * npol2)), dim3(256), 0, ctx->stream, (const double2*)vis1, (const double2*)vis2, npol2, ncell, ps_norm,
                     (double2*)out);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_ps_cyl_bin(dmm_ctx* ctx, const void* spec, const void* sigma, const int16_t* binmap, int nplane, int nu, int nv, int nbins, void* out_spec, double* out_weight,
                   double* out_neff) {
  DMM_REQUIRE(ctx != nullptr, "dmm_ps_cyl_bin: ctx is NULL");
  DMM_REQUIRE(nplane >= 1 && nu >= 1 && nv >= 1 && (int64_t)nu * nv <= 0x7fffffff, "dmm_ps_cyl_bin: bad sizes nplane=%d nu=%d nv=%d", nplane, nu, nv);
  DMM_REQUIRE(nbins >= 1, "dmm_ps_cyl_bin: bad bin count %d", nbins);
  DMM_REQUIRE(nbins <= DMM_PS_MAX_BINS, "dmm_ps_cyl_bin: too many bins: %d > %d", nbins, DMM_PS_MAX_BINS);
  DMM_REQUIRE((int64_t)nplane * nbins <= 0x7fffffff, "dmm_ps_cyl_bin: too many (plane, bin) pairs");
  DMM_REQUIRE(spec && binmap && out_spec && out_weight && out_neff, "dmm_ps_cyl_bin: NULL argument");
  const int64_t ncell = (int64_t)nu * nv;
  std::vector<int32_t> tab(nbins + 1, 0);
  int64_t nsel = 0;
  for (int64_t c = 0; c < ncell; ++c) {
    const int b = binmap[c];
    DMM_REQUIRE(b >= -1 && b < nbins, "dmm_ps_cyl_bin: bin index %d of cell %lld outside -1 ... %d", b, (long long)c, nbins - 1);
    if (b >= 0) {
      ++tab[b + 1];
      ++nsel;
    }
  }
  for (int b = 0; b < nbins; ++b) tab[b + 1] += tab[b];
  const size_t nstart = (size_t)nbins + 1;
  tab.resize(nstart + (size_t)(nsel > 0 ? nsel : 1));
  {
    std::vector<int32_t> fill(tab.begin(), tab.begin() + nbins);
    for (int64_t c = 0; c < ncell; ++c) {  // ascending cell order within a bin
      const int b = binmap[c];
      if (b >= 0) tab[nstart + fill[b]++] = (int32_t)c;
    }
  }
  DMM_HIP(hipSetDevice(ctx->device));
  int32_t* tab_d = nullptr;
  DMM_HIP(hipMalloc((void**)&tab_d, tab.size() * sizeof(int32_t)));
  hipError_t err = hipMemcpy(tab_d, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_ps_bin, dim3((unsigned)((int64_t)nplane * nbins)), dim3(256), 0, ctx->stream, (const double2*)spec, (const double2*)sigma, (const int32_t*)tab_d,
                       (const int32_t*)(tab_d + nstart), ncell, nbins, (double2*)out_spec, out_weight, out_neff);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);  // the tables are freed below
  (void)hipFree(tab_d);
  if (err != hipSuccess) return dmm_set_error((int)err, "dmm_ps_cyl_bin: %s", hipGetErrorString(err));
  return DMM_OK;
}

}  // extern "C"
