// Weighted reductions over adjacent axes of a dataset: the chi-squared per degree of freedom, the variance, and the
// weighted mean of the real part.
//
// Reference: draco/analysis/transform.py:1904-2117 (ReduceBase, ReduceVar, ReduceChisq) and the collapse at the head of
// RFIMaskChisqHighDelay.process (draco/analysis/flagging.py:1548-1579).  DESIGN.md section 7s.
//
// k_axis_reduce: the data is [nouter][nred][ninner]; one thread per (outer, inner) column, lanes along inner, so every
// load of a wave is one contiguous run.  The weight is addressed by element strides (0: an axis it lacks).  Sums run in
// float64 in ascending order of the reduced index: no atomics, and the result does not depend on the launch shape.  The
// ops that need the mean walk the column twice.  One rounding, at the store.
#include "dmm_internal.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int kRedThreads = 256;

struct RedArgs {
  const void* x;
  const void* w;
  void* out;
  void* out_w;
  int64_t nouter, nred, ninner, nred2, ws_outer, ws_red1, ws_red2, ws_inner;
  double factor;
  int op, wdtype;
};

template <int DT>
__device__ inline void red_load(const void* p, int64_t i, double& re, double& im) {
  im = 0.0;
  if constexpr (DT == DMM_REDUCE_F32) {
    re = (double)((const float*)p)[i];
  } else if constexpr (DT == DMM_REDUCE_F64) {
    re = ((const double*)p)[i];
  } else if constexpr (DT == DMM_REDUCE_C64) {
    const float2 v = ((const float2*)p)[i];
    re = (double)v.x;
    im = (double)v.y;
  } else {
    const double2 v = ((const double2*)p)[i];
    re = v.x;
    im = v.y;
  }
}

template <int DT>
__device__ inline void red_store(void* p, int64_t i, double re, double im) {
  if constexpr (DT == DMM_REDUCE_F32) {
    ((float*)p)[i] = (float)re;
  } else if constexpr (DT == DMM_REDUCE_F64) {
    ((double*)p)[i] = re;
  } else if constexpr (DT == DMM_REDUCE_C64) {
    ((float2*)p)[i] = make_float2((float)re, (float)im);
  } else {
    ((double2*)p)[i] = make_double2(re, im);
  }
}

__device__ inline double inz(double v) { return v == 0.0 ? 0.0 : 1.0 / v; }

template <int DT>
__global__ __launch_bounds__(kRedThreads) void k_axis_reduce(RedArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= a.ninner) return;
  const bool unit = a.w == nullptr || a.op == DMM_REDUCE_VAR_NONE;
  const bool masked = a.op == DMM_REDUCE_VAR_MASKED;
  for (int64_t o = blockIdx.y; o < a.nouter; o += gridDim.y) {
    const int64_t xbase = o * a.nred * a.ninner + i;
    const int64_t wbase = o * a.ws_outer + i * a.ws_inner;
    auto weight = [&](int64_t r) -> double {
      if (unit) return 1.0;
      const int64_t off = wbase + (r / a.nred2) * a.ws_red1 + (r % a.nred2) * a.ws_red2;
      const double wv = a.wdtype == DMM_REDUCE_F64 ? ((const double*)a.w)[off] : (double)((const float*)a.w)[off];
      return masked ? (wv > 0.0 ? 1.0 : 0.0) : wv;
    };
    double sw = 0.0, sr = 0.0, si = 0.0;
    int64_t cnt = 0;
    for (int64_t r = 0; r < a.nred; ++r) {
      const double wv = weight(r);
      double xr, xi;
      red_load<DT>(a.x, xbase + r * a.ninner, xr, xi);
      sw = sw + wv;
      cnt += wv > 0.0;
      sr = sr + wv * xr;
      si = si + wv * xi;
    }
    const int64_t oi = o * a.ninner + i;
    if (a.op == DMM_REDUCE_WMEAN) {
      const double s = a.factor * sw;
      ((double*)a.out)[oi] = sr * inz(s);
      ((double*)a.out_w)[oi] = s;
      continue;
    }
    const double iws = inz(sw);
    const double mr = sr * iws, mi = si * iws;
    double vr = 0.0, vi = 0.0;
    for (int64_t r = 0; r < a.nred; ++r) {
      const double wv = weight(r);
      double xr, xi;
      red_load<DT>(a.x, xbase + r * a.ninner, xr, xi);
      const double dr = xr - mr, di = xi - mi;
      if (a.op == DMM_REDUCE_VAR_MASKED || a.op == DMM_REDUCE_VAR_WEIGHTED) {  // (x - mu)^2, complex for complex data
        vr = vr + wv * (dr * dr - di * di);
        vi = vi + wv * (2.0 * (dr * di));
      } else {  // |x - mu|^2
        vr = vr + wv * (dr * dr + di * di);
      }
    }
    double ow;
    if (a.op == DMM_REDUCE_CHISQ) {
      const double num = (double)(cnt > 1 ? cnt - 1 : 0);
      vr = vr * inz(num);
      ow = num;
    } else {
      vr = vr * iws;
      vi = vi * iws;
      ow = a.op == DMM_REDUCE_VAR_NONE ? 1.0 : sw;
    }
    red_store<DT>(a.out, oi, vr, vi);
    if (a.wdtype == DMM_REDUCE_F64)
      ((double*)a.out_w)[oi] = ow;
    else
      ((float*)a.out_w)[oi] = (float)ow;
  }
}

}  // namespace

extern "C" int dmm_axis_reduce(dmm_ctx* ctx, int op, int dtype, const void* x, int64_t nouter, int64_t nred, int64_t ninner, const void* w, int wdtype,
                               int64_t ws_outer, int64_t nred2, int64_t ws_red1, int64_t ws_red2, int64_t ws_inner, double factor, void* out, void* out_w) {
  DMM_REQUIRE(ctx != nullptr, "dmm_axis_reduce: ctx is NULL");
  DMM_REQUIRE(op >= DMM_REDUCE_CHISQ && op <= DMM_REDUCE_WMEAN, "dmm_axis_reduce: bad operation %d", op);
  DMM_REQUIRE(dtype >= DMM_REDUCE_F32 && dtype <= DMM_REDUCE_C128, "dmm_axis_reduce: bad data type %d", dtype);
  DMM_REQUIRE(wdtype == DMM_REDUCE_F32 || wdtype == DMM_REDUCE_F64, "dmm_axis_reduce: the weight is float32 or float64, got type %d", wdtype);
  DMM_REQUIRE(nouter >= 0 && nred >= 0 && ninner >= 0, "dmm_axis_reduce: bad sizes nouter=%lld nred=%lld ninner=%lld", (long long)nouter, (long long)nred, (long long)ninner);
  DMM_REQUIRE(nred2 >= 1 && nred % nred2 == 0, "dmm_axis_reduce: the inner reduced axis of %lld does not divide the %lld reduced samples", (long long)nred2, (long long)nred);
  DMM_REQUIRE(ws_outer >= 0 && ws_red1 >= 0 && ws_red2 >= 0 && ws_inner >= 0, "dmm_axis_reduce: negative weight stride");
  DMM_REQUIRE(ninner <= ((int64_t)1 << 31) * kRedThreads - 1, "dmm_axis_reduce: ninner %lld does not fit the grid", (long long)ninner);
  if (nouter == 0 || ninner == 0) return DMM_OK;
  DMM_REQUIRE(x || nred == 0, "dmm_axis_reduce: NULL data");
  DMM_REQUIRE(out && out_w, "dmm_axis_reduce: NULL output");
  DMM_REQUIRE(w || op == DMM_REDUCE_VAR_NONE || op == DMM_REDUCE_CHISQ || op == DMM_REDUCE_WMEAN, "dmm_axis_reduce: the masked and weighted variances need weights");
  DMM_HIP(hipSetDevice(ctx->device));
  RedArgs a{x, w, out, out_w, nouter, nred, ninner, nred2, ws_outer, ws_red1, ws_red2, ws_inner, factor, op, wdtype};
  const dim3 grid((unsigned)((ninner + kRedThreads - 1) / kRedThreads), (unsigned)std::min<int64_t>(nouter, 65535));
  switch (dtype) {
    case DMM_REDUCE_F32: hipLaunchKernelGGL(k_axis_reduce<DMM_REDUCE_F32>, grid, dim3(kRedThreads), 0, ctx->stream, a); break;
    case DMM_REDUCE_F64: hipLaunchKernelGGL(k_axis_reduce<DMM_REDUCE_F64>, grid, dim3(kRedThreads), 0, ctx->stream, a); break;
    case DMM_REDUCE_C64: hipLaunchKernelGGL(k_axis_reduce<DMM_REDUCE_C64>, grid, dim3(kRedThreads), 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL(k_axis_reduce<DMM_REDUCE_C128>, grid, dim3(kRedThreads), 0, ctx->stream, a); break;
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}
