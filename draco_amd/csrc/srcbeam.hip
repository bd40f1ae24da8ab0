// Source beamforming (draco/analysis/beamform.py:139-385, draco/util/_fast_tools.pyx:211-290): fringestop a sidereal
// stream or time stream to every source of a catalogue, sum over baselines and hour angle.
//
//   dmm_srcbeam_prepare   once per dataset and processed polarisation: gather the polarisation's stacks into
//                         visT / ws [freq][ra][k] (k contiguous), ws the weight of the sum (BeamFormBase._process_data,
//                         :573-630), and the two source-independent sums over stacks SW, SW2 [freq][ra] in float64
//   dmm_srcbeam_form      the hot kernel: F[src][f][j] = sum_k ws[f][ra_j][k] Re(vis[f][ra_j][k] e^{i phi}),
//                         phi = 2 pi (u_k[f] ut[src][j] + v_k[f] vt[src][j])
//   dmm_srcbeam_collapse  primary beam, sums over hour angle, the two weight forms, the factor 2, zero weight at
//                         frequencies a source does not process, the Stokes I combination (:290-376)
//
// Decomposition of the form kernel.  A block owns one (f, ra) row of the data: ns stacks of vis (8 bytes), ws (4) and the
// baseline of the frequency in wavelengths u, v (8 + 8, L2 resident: one row per frequency).  The host inverts the
// sources' windows into a list, sorted by ra, of the (source, hour-angle slot) pairs that read each ra; the block stages
// its row in LDS in passes of kKT stacks and every wave takes every fourth pair of the row's list: lanes stride over the
// stacks, one sincospi per term with the phase in turns (exact argument reduction), a wave reduction, one store.  No two
// waves ever write the same F element, so the result of a pair does not depend on where the catalogue put its source.
// Each row is read from memory once per chunk of sources instead of once per source; the kernel is bound by the
// float64 sin / cos evaluation.
#include <math.h>

#include "dmm_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kKT = 1024;  // stacks per LDS pass: 32 KB

__device__ __forceinline__ double inz(double x) { return x != 0.0 ? 1.0 / x : 0.0; }

// the weight of the sum of one sample: mode 0 inverse_variance, 1 natural, 2 uniform
__device__ __forceinline__ float sum_weight(int mode, float w, const float* red, int64_t ridx) {
  if (mode == 0) return w;
  if (!(w > 0.0f)) return 0.0f;
  const float r = red[ridx];
  return mode == 1 ? r : (r > 0.0f ? 1.0f : 0.0f);
}

// visT / ws [f][ra][k] <- vis / weight [f][sel[k]][ra]: a 32 x 32 tile through LDS, both sides coalesced
__global__ __launch_bounds__(256) void k_sb_gather(int nstack, int nra, int ns, const int32_t* __restrict__ sel, int mode, const float2* __restrict__ vis,
                                                   const float* __restrict__ weight, const float* __restrict__ red, float2* __restrict__ visT, float* __restrict__ ws) {
  __shared__ float2 tv[32][33];
  __shared__ float tw[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int ra0 = blockIdx.x * 32, k0 = blockIdx.y * 32, f = blockIdx.z;
  for (int i = 0; i < 4; ++i) {
    const int kk = ty + 8 * i, k = k0 + kk, ra = ra0 + tx;
    float2 x = make_float2(0.0f, 0.0f);
    float w = 0.0f;
    if (k < ns && ra < nra) {
      const int st = sel[k];
      if ((unsigned)st < (unsigned)nstack) {
        const int64_t idx = ((int64_t)f * nstack + st) * nra + ra;
        x = vis[idx];
        w = sum_weight(mode, weight[idx], red, (int64_t)st * nra + ra);
      }
    }
    tv[kk][tx] = x;
    tw[kk][tx] = w;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int rr = ty + 8 * i, ra = ra0 + rr, k = k0 + tx;
    if (ra < nra && k < ns) {
      const int64_t o = ((int64_t)f * nra + ra) * ns + k;
      visT[o] = tv[tx][rr];
      ws[o] = tw[tx][rr];
    }
  }
}

// SW = sum_k ws, SW2 = sum_k ws^2 inz(wv): a thread per (f, ra), lanes along ra
__global__ __launch_bounds__(256) void k_sb_sums(int nfreq, int nstack, int nra, int ns, const int32_t* __restrict__ sel, int mode, const float* __restrict__ weight,
                                                 const float* __restrict__ red, double* __restrict__ SW, double* __restrict__ SW2) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nfreq * nra) return;
  const int f = (int)(t / nra), ra = (int)(t - (int64_t)f * nra);
  double sw = 0.0, sw2 = 0.0;
  for (int k = 0; k < ns; ++k) {
    const int st = sel[k];
    if ((unsigned)st >= (unsigned)nstack) continue;
    const float w = weight[((int64_t)f * nstack + st) * nra + ra];
    const double s = (double)sum_weight(mode, w, red, (int64_t)st * nra + ra);
    sw += s;
    sw2 += s * s * inz((double)w);
  }
  SW[t] = sw;
  SW2[t] = sw2;
}

template <typename W>
__global__ __launch_bounds__(kThreads) void k_sb_form(int nfreq, int nra, int ns, const float2* __restrict__ vis, const W* __restrict__ ws, const double* __restrict__ u,
                                                      const double* __restrict__ v, int nsrc, int nha, const double* __restrict__ ut, const double* __restrict__ vt,
                                                      const uint8_t* __restrict__ fmask, int64_t npair, const int32_t* __restrict__ pair_start,
                                                      const int32_t* __restrict__ pair_id, double* __restrict__ F) {
  __shared__ float2 s_vis[kKT];
  __shared__ double s_w[kKT], s_u[kKT], s_v[kKT];
  const int ra = blockIdx.x, f = blockIdx.y;
  int64_t p0 = pair_start[ra], p1 = pair_start[ra + 1];
  p0 = p0 < 0 ? 0 : p0;
  p1 = p1 > npair ? npair : p1;
  if (p1 <= p0) return;  // (the whole block: nobody looks at this sample)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = ((int64_t)f * nra + ra) * ns, brow = (int64_t)f * ns;
  const int nid = nsrc * nha;
  for (int k0 = 0; k0 < ns; k0 += kKT) {
    const int kn = ns - k0 < kKT ? ns - k0 : kKT;
    if (k0) __syncthreads();
    for (int k = threadIdx.x; k < kn; k += kThreads) {
      s_vis[k] = vis[row + k0 + k];
      s_w[k] = (double)ws[row + k0 + k];
      s_u[k] = u[brow + k0 + k];
      s_v[k] = v[brow + k0 + k];
    }
    __syncthreads();
    for (int64_t p = p0 + wave; p < p1; p += kWaves) {
      const int id = pair_id[p];
      if ((unsigned)id >= (unsigned)nid) continue;
      const int s = id / nha;
      if (fmask && !fmask[(int64_t)s * nfreq + f]) continue;
      const double a = ut[id], b = vt[id];
      double acc = 0.0;
      for (int k = lane; k < kn; k += 64) {
        const double turns = fma(s_u[k], a, s_v[k] * b);
        double sn, cs;
        sincospi(2.0 * turns, &sn, &cs);
        const float2 x = s_vis[k];
        acc += s_w[k] * ((double)x.x * cs - (double)x.y * sn);
      }
      for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) {
        const int64_t o = ((int64_t)s * nfreq + f) * nha + (id - s * nha);
        F[o] = k0 ? F[o] + acc : acc;
      }
    }
  }
}

struct CollapseArgs {
  int nfreq, nra, npol, nsrc, nha, collapse_ha, inverse_variance, stokes_i;
  const double *F, *pb, *SW, *SW2;
  const int32_t* ra_index;
  const uint8_t* fmask;
  const int64_t* rows;
  int64_t nobj;
  double *beam, *weight;
};

// a thread per (source, frequency); the sums over hour angle run in the order of the window
__global__ __launch_bounds__(256) void k_sb_collapse(CollapseArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)a.nsrc * a.nfreq) return;
  const int s = (int)(t / a.nfreq), f = (int)(t - (int64_t)s * a.nfreq);
  const int64_t row = a.rows[s];
  if (row < 0 || row >= a.nobj) return;
  const bool fm = a.fmask ? a.fmask[t] != 0 : true;
  const int npo = a.stokes_i ? 1 : a.npol;
  const int32_t* ri = a.ra_index + (int64_t)s * a.nha;
  if (a.collapse_ha) {
    double bsum = 0.0, wsum = 0.0;
    for (int p = 0; p < a.npol; ++p) {
      const int64_t fo = (((int64_t)p * a.nsrc + s) * a.nfreq + f) * a.nha, so = ((int64_t)p * a.nfreq + f) * a.nra;
      double sw = 0.0, w2 = 0.0, fb = 0.0;
      for (int j = 0; j < a.nha; ++j) {
        const int ra = ri[j];
        if ((unsigned)ra >= (unsigned)a.nra) continue;
        const double pbv = a.pb ? a.pb[fo + j] : 1.0, pb2 = pbv * pbv;
        sw += a.SW[so + ra] * pb2;
        w2 += a.SW2[so + ra] * pb2;
        fb += a.F[fo + j] * pbv;
      }
      const double b = fb * inz(sw);
      double w = a.inverse_variance ? sw : sw * sw * inz(w2);
      if (!fm) w = 0.0;
      if (a.stokes_i) {
        bsum += b * w;
        wsum += w;
      } else {
        const int64_t o = (row * npo + p) * a.nfreq + f;
        a.beam[o] = b;
        a.weight[o] = 2.0 * w;
      }
    }
    if (a.stokes_i) {
      const int64_t o = row * a.nfreq + f;
      a.beam[o] = bsum * inz(wsum);
      a.weight[o] = 2.0 * wsum;
    }
    return;
  }
  for (int j = 0; j < a.nha; ++j) {
    const int ra = ri[j];
    const bool ok = (unsigned)ra < (unsigned)a.nra;
    double bsum = 0.0, wsum = 0.0;
    for (int p = 0; p < a.npol; ++p) {
      double b = 0.0, w = 0.0;
      if (ok) {
        const int64_t so = ((int64_t)p * a.nfreq + f) * a.nra + ra;
        const double sw = a.SW[so];
        b = a.F[(((int64_t)p * a.nsrc + s) * a.nfreq + f) * a.nha + j] * inz(sw);
        w = a.inverse_variance ? sw : sw * sw * inz(a.SW2[so]);
        if (!fm) w = 0.0;
      }
      if (a.stokes_i) {
        bsum += b * w;
        wsum += w;
      } else {
        const int64_t o = ((row * npo + p) * a.nfreq + f) * a.nha + j;
        a.beam[o] = b;
        a.weight[o] = 2.0 * w;
      }
    }
    if (a.stokes_i) {
      const int64_t o = (row * a.nfreq + f) * a.nha + j;
      a.beam[o] = bsum * inz(wsum);
      a.weight[o] = 2.0 * wsum;
    }
  }
}

}  // namespace

extern "C" {

int dmm_srcbeam_prepare(dmm_ctx* ctx, int nfreq, int nstack, int nra, int nsel, const int32_t* sel, int mode, const void* vis, const float* weight,
                        const float* redundancy, void* visT, float* ws, double* SW, double* SW2) {
  DMM_REQUIRE(ctx != nullptr, "dmm_srcbeam_prepare: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= 65535, "dmm_srcbeam_prepare: frequency count %d outside 1 ... 65535", nfreq);
  DMM_REQUIRE(nstack >= 1, "dmm_srcbeam_prepare: bad stack count %d", nstack);
  DMM_REQUIRE(nra >= 1, "dmm_srcbeam_prepare: bad sample count %d", nra);
  DMM_REQUIRE(nsel >= 0 && nsel <= nstack, "dmm_srcbeam_prepare: bad selection count %d", nsel);
  DMM_REQUIRE(mode >= DMM_SRCBEAM_INVERSE_VARIANCE && mode <= DMM_SRCBEAM_UNIFORM, "dmm_srcbeam_prepare: unknown weight mode %d", mode);
  DMM_REQUIRE(vis && weight && SW && SW2 && (redundancy || mode == DMM_SRCBEAM_INVERSE_VARIANCE), "dmm_srcbeam_prepare: NULL argument");
  DMM_REQUIRE(nsel == 0 || (sel && visT && ws), "dmm_srcbeam_prepare: NULL argument");
  DMM_REQUIRE((int64_t)(nsel + 31) / 32 <= 65535, "dmm_srcbeam_prepare: too many stacks");
  DMM_HIP(hipSetDevice(ctx->device));
  if (nsel > 0) {
    hipLaunchKernelGGL(k_sb_gather, dim3((unsigned)((nra + 31) / 32), (unsigned)((nsel + 31) / 32), (unsigned)nfreq), dim3(256), 0, ctx->stream, nstack, nra, nsel, sel, mode,
                       (const float2*)vis, weight, redundancy, (float2*)visT, ws);
    DMM_HIP(hipGetLastError());
  }
  const int64_t n = (int64_t)nfreq * nra;
  DMM_REQUIRE((n + 255) / 256 <= 0x7fffffff, "dmm_srcbeam_prepare: too many samples");
  hipLaunchKernelGGL(k_sb_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, nfreq, nstack, nra, nsel, sel, mode, weight, redundancy, SW, SW2);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_srcbeam_form(dmm_ctx* ctx, int nfreq, int nra, int nsel, int wtype, const void* visT, const void* ws, const double* u, const double* v, int nsrc, int nha,
                     const double* ut, const double* vt, const uint8_t* fmask, int64_t npair, const int32_t* pair_start, const int32_t* pair_id, double* F) {
  DMM_REQUIRE(ctx != nullptr, "dmm_srcbeam_form: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= 65535, "dmm_srcbeam_form: frequency count %d outside 1 ... 65535", nfreq);
  DMM_REQUIRE(nra >= 1, "dmm_srcbeam_form: bad sample count %d", nra);
  DMM_REQUIRE(nsel >= 0, "dmm_srcbeam_form: bad stack count %d", nsel);
  DMM_REQUIRE(nsrc >= 0, "dmm_srcbeam_form: bad source count %d", nsrc);
  DMM_REQUIRE(nha >= 1, "dmm_srcbeam_form: bad window length %d", nha);
  DMM_REQUIRE(nha <= nra, "dmm_srcbeam_form: window of %d samples is longer than the axis (%d)", nha, nra);
  DMM_REQUIRE((int64_t)nsrc * nha <= 0x7fffffff, "dmm_srcbeam_form: too many sources in one chunk");
  DMM_REQUIRE(npair >= 0 && npair <= (int64_t)nsrc * nha, "dmm_srcbeam_form: bad pair count %lld", (long long)npair);
  DMM_REQUIRE(wtype == DMM_SRCBEAM_W_F32 || wtype == DMM_SRCBEAM_W_F64, "dmm_srcbeam_form: unknown weight type %d", wtype);
  DMM_REQUIRE(F != nullptr, "dmm_srcbeam_form: NULL argument");
  if (nsrc == 0) return DMM_OK;  // nothing to do
  DMM_REQUIRE(visT && ws && u && v && ut && vt && pair_start && pair_id, "dmm_srcbeam_form: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  DMM_HIP(hipMemsetAsync(F, 0, sizeof(double) * (size_t)nsrc * nfreq * nha, ctx->stream));
  if (npair == 0 || nsel == 0) return DMM_OK;
  const dim3 grid((unsigned)nra, (unsigned)nfreq);
  if (wtype == DMM_SRCBEAM_W_F32)
    hipLaunchKernelGGL(k_sb_form<float>, grid, dim3(kThreads), 0, ctx->stream, nfreq, nra, nsel, (const float2*)visT, (const float*)ws, u, v, nsrc, nha, ut, vt, fmask, npair,
                       pair_start, pair_id, F);
  else
    hipLaunchKernelGGL(k_sb_form<double>, grid, dim3(kThreads), 0, ctx->stream, nfreq, nra, nsel, (const float2*)visT, (const double*)ws, u, v, nsrc, nha, ut, vt, fmask, npair,
                       pair_start, pair_id, F);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_srcbeam_collapse(dmm_ctx* ctx, int nfreq, int nra, int npol, int nsrc, int nha, int collapse_ha, int inverse_variance, int stokes_i, const double* F,
                         const double* pb, const double* SW, const double* SW2, const int32_t* ra_index, const uint8_t* fmask, const int64_t* rows, int64_t nobj,
                         double* beam, double* weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_srcbeam_collapse: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= 65535, "dmm_srcbeam_collapse: frequency count %d outside 1 ... 65535", nfreq);
  DMM_REQUIRE(nra >= 1, "dmm_srcbeam_collapse: bad sample count %d", nra);
  DMM_REQUIRE(npol >= 1 && npol <= 4, "dmm_srcbeam_collapse: polarisation count %d outside 1 ... 4", npol);
  DMM_REQUIRE(nsrc >= 0, "dmm_srcbeam_collapse: bad source count %d", nsrc);
  DMM_REQUIRE(nha >= 1, "dmm_srcbeam_collapse: bad window length %d", nha);
  DMM_REQUIRE(nha <= nra, "dmm_srcbeam_collapse: window of %d samples is longer than the axis (%d)", nha, nra);
  DMM_REQUIRE(nobj >= nsrc, "dmm_srcbeam_collapse: %lld output rows for %d sources", (long long)nobj, nsrc);
  DMM_REQUIRE(beam && weight, "dmm_srcbeam_collapse: NULL argument");
  if (nsrc == 0) return DMM_OK;  // nothing to do
  DMM_REQUIRE(F && SW && SW2 && ra_index && rows, "dmm_srcbeam_collapse: NULL argument");
  const int64_t n = (int64_t)nsrc * nfreq;
  DMM_REQUIRE((n + 255) / 256 <= 0x7fffffff, "dmm_srcbeam_collapse: too many sources in one chunk");
  DMM_HIP(hipSetDevice(ctx->device));
  CollapseArgs a{nfreq, nra, npol, nsrc, nha, collapse_ha != 0, inverse_variance != 0, stokes_i != 0, F, pb, SW, SW2, ra_index, fmask, rows, nobj, beam, weight};
  hipLaunchKernelGGL(k_sb_collapse, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
