// Elementwise kernels on m-mode weights and correlation products that are not transforms: MaskMModeData,
// CollateProducts and ExpandProducts.
#include "dmm_internal.h"

// ------------------------------------------------------------------ MaskMModeData
// Zero m-mode noise weights ahead of map-making (reference draco/analysis/flagging.py:113-173):
// auto-correlations, m = 0, one sign of m, m below a threshold.  weight [n_m, 2, nfreq, nstack].
namespace {
__global__ void k_mask_mmode(double* __restrict__ w, int n_m, int64_t nfreq, int nstack,
                             const unsigned char* __restrict__ is_auto, int m_zero, int positive_m, int negative_m,
                             int mask_low_m) {
  const int64_t per_ms = nfreq * nstack, total = (int64_t)n_m * 2 * per_ms;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ms = i / per_ms;
    const int m = (int)(ms >> 1), s = (int)(ms & 1);
    const int p = (int)(i % nstack);
    bool kill = false;
    if (is_auto && is_auto[p]) kill = true;
    if (!m_zero && m == 0) kill = true;
    if (!positive_m && m >= 1 && s == 0) kill = true;
    if (!negative_m && m >= 1 && s == 1) kill = true;
    if (m < mask_low_m) kill = true;
    if (kill) w[i] = 0.0;
  }
}
}  // namespace

extern "C" int dmm_mask_mmode_weight(dmm_ctx* ctx, double* mweight, int n_m, int64_t nfreq, int nstack,
                                     const unsigned char* is_auto, int m_zero, int positive_m, int negative_m,
                                     int mask_low_m) {
  DMM_REQUIRE(ctx != nullptr, "dmm_mask_mmode_weight: ctx is NULL");
  DMM_REQUIRE(n_m >= 0 && nfreq >= 0 && nstack >= 0 && mask_low_m >= 0, "dmm_mask_mmode_weight: bad sizes");
  const int64_t total = (int64_t)n_m * 2 * nfreq * nstack;
  if (total == 0) return DMM_OK;
  DMM_REQUIRE(mweight != nullptr, "dmm_mask_mmode_weight: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  int64_t nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(k_mask_mmode, dim3((unsigned)nb), dim3(256), 0, ctx->stream, mweight, n_m, nfreq, nstack, is_auto,
                     m_zero, positive_m, negative_m, mask_low_m);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

// ------------------------------------------------------------------ CollateProducts
// Weighted stacking of correlation products into the telescope's unique baselines
// (reference draco/analysis/transform.py:277-320).  The reference scatters product by product
// into the output; here the host inverts the map once (CSR: output baseline -> contributing
// input products) so every output sample is one thread's deterministic gather, no atomics.
namespace {
__global__ void k_collate(const float2* __restrict__ ssv, const float* __restrict__ ssw, int nprod_in, int nt,
                          int nf_out, const int* __restrict__ freq_ind, int nstack_out,
                          const int* __restrict__ csr_ptr, const int* __restrict__ csr_src,
                          const unsigned char* __restrict__ csr_conj, const float* __restrict__ red,
                          float2* __restrict__ out_vis, float* __restrict__ out_w) {
  const int64_t total = (int64_t)nf_out * nstack_out * nt;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % nt);
    const int sp = (int)((i / nt) % nstack_out);
    const int fo = (int)(i / ((int64_t)nt * nstack_out));
    const int64_t fbase = (int64_t)freq_ind[fo] * nprod_in;
    double vr = 0.0, vi = 0.0, var = 0.0, cnt = 0.0;
    for (int e = csr_ptr[sp]; e < csr_ptr[sp + 1]; ++e) {
      const int pi = csr_src[e];
      const int64_t o = (fbase + pi) * nt + t;
      const double w = (double)ssw[o];
      const double wss = red ? (w > 0.0 ? (double)red[(int64_t)pi * nt + t] : 0.0) : w;  // transform.py:297-301
      const float2 v = ssv[o];
      vr += wss * (double)v.x;
      vi += wss * (csr_conj[e] ? -(double)v.y : (double)v.y);
      var += w != 0.0 ? wss * wss / w : 0.0;
      cnt += wss;
    }
    const double ic = cnt != 0.0 ? 1.0 / cnt : 0.0;
    out_vis[i] = make_float2((float)(vr * ic), (float)(vi * ic));
    out_w[i] = (float)(var != 0.0 ? cnt * cnt / var : 0.0);
  }
}

// ExpandProducts (reference synthesis/stream.py:228-244): out[f, p, t] = (conj?) in[f, src[p], t], weight 1; products
// of a masked pair (src < 0) stay zero with zero weight.  One thread per output sample, t fastest.
__global__ void k_expand(const float2* __restrict__ in, int nstack, int nt, int nprod, const int* __restrict__ src,
                         const unsigned char* __restrict__ cj, float2* __restrict__ out, float* __restrict__ out_w,
                         int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int t = (int)(i % nt);
    const int64_t fp = i / nt;
    const int p = (int)(fp % nprod);
    const int64_t f = fp / nprod;
    const int sp = src[p];
    float2 v = make_float2(0.f, 0.f);
    if (sp >= 0) {
      v = in[(f * nstack + sp) * nt + t];
      if (cj[p]) v.y = -v.y;
    }
    out[i] = v;
    out_w[i] = sp >= 0 ? 1.f : 0.f;
  }
}
}  // namespace

extern "C" int dmm_collate_products(dmm_ctx* ctx, const void* ssv, const float* ssw, int nf_in, int nprod_in, int nt,
                                    int nf_out, const int* freq_ind, int nstack_out, const int* csr_ptr,
                                    const int* csr_src, const unsigned char* csr_conj, const float* red,
                                    void* out_vis, float* out_w) {
  DMM_REQUIRE(ctx != nullptr, "dmm_collate_products: ctx is NULL");
  DMM_REQUIRE(nf_in >= 0 && nprod_in >= 0 && nt >= 0 && nf_out >= 0 && nstack_out >= 0, "dmm_collate_products: bad sizes");
  const int64_t total = (int64_t)nf_out * nstack_out * nt;
  if (total == 0) return DMM_OK;
  DMM_REQUIRE(ssv && ssw && freq_ind && csr_ptr && out_vis && out_w, "dmm_collate_products: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  int64_t nb = (total + 255) / 256;
  if (nb > 16384) nb = 16384;
  hipLaunchKernelGGL(k_collate, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const float2*)ssv, ssw, nprod_in, nt, nf_out,
                     freq_ind, nstack_out, csr_ptr, csr_src, csr_conj, red, (float2*)out_vis, out_w);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

extern "C" int dmm_expand_products(dmm_ctx* ctx, const void* vis_in, int nfreq, int nstack, int nt, int nprod,
                                   const int* src, const unsigned char* conj, void* out_vis, float* out_w) {
  DMM_REQUIRE(ctx != nullptr, "dmm_expand_products: ctx is NULL");
  DMM_REQUIRE(nfreq >= 0 && nstack >= 0 && nt >= 0 && nprod >= 0, "dmm_expand_products: bad sizes");
  const int64_t total = (int64_t)nfreq * nprod * nt;
  if (total == 0) return DMM_OK;
  DMM_REQUIRE(vis_in && src && conj && out_vis && out_w, "dmm_expand_products: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  int64_t nb = (total + 255) / 256;
  if (nb > 16384) nb = 16384;
  hipLaunchKernelGGL(k_expand, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const float2*)vis_in, nstack, nt, nprod, src, conj,
                     (float2*)out_vis, out_w, total);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}
