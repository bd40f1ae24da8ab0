// Wiener delay transform of a filtered ring map (draco/analysis/powerspec.py:118-458).
//
// Build.  Per pixel (pol, ra, el), with K = filter[pol, :, :, ra], C = freq_cov[pol, :, :, ra], w = weight[pol, :, ra, el],
// b = sqrt(dirty_beam_power[0, pol, :, el]), the window and win_mask = window > 0:
//   M = win_mask and (w > 0),   H = diag(M) K,   r = sqrt(inv0(w diag C)) win_mask,
//   A = H (F S F^H o b b^T) H^T + C o r r^T,   D = diag(S) F^H H^T A^-1_valid window      [delay, freq],
// A^-1_valid the inverse of the block of the valid channels, zero elsewhere.  A is complex Hermitian, K, C and w are
// real: the system is solved in its real symmetric embedding E = [[Re A, -Im A], [Im A, Re A]] of order 2 nfreq with the
// batched float64 solver of chol_blocked.h.  A masked channel has a zero row and column and 1 on the diagonal, so its
// part of the solution is exactly zero; like LAPACK's zpotrf only the upper triangle of A is used.  Row d of
// F^H H^T A^-1 is the conjugate of the solution z of A z = (H F)[:, d], so the right-hand sides are the columns of H F.
//
// Stages, all float64, batched over the pixels of one slab (a run of RA times a run of elevations of one polarisation):
//   k_wd_transpose  filter and freq_cov of the slab's RA, [freq freq][ra] -> [ra][freq freq], once per run of RA;
//   k_wd_assemble   one block per pixel: M, r, the status of an empty pixel, H and Hb = H diag(b);
//   dl_gemm         T = Hb [Re P | Im P] (P = F S F^H, shared), Re A = T_r Hb^T into E's upper left block, -Im A =
//                   -T_i Hb^T into its upper right block, Y = [Re (H F)^T | Im (H F)^T];
//   k_wd_embed      in place on E: the noise term, the masks, the unit diagonal, the antisymmetric upper right block
//                   from its upper triangle and the copy of Re A into the lower right block;
//   dl_factor / dl_solve_rows    E = U^T U and the ndelay solves; a pivot that is not positive sets the status word;
//   k_wd_store      D[pol, ra, el, d, f] = (S_d (z_r - i z_i)) window_f, zero on masked channels and empty pixels, cast to
//                   the output type, every pixel one contiguous run of ndelay nfreq elements.
// No atomics on floating-point data and no dependence of any sum on the slab: the output is the same bits whatever the
// workspace.  After each slab the status words are read back; the first pixel that is not positive definite ends the call.
//
// Apply.  k_wd_apply: one block per (pol, ra, group of kWdGroup elevations); the strided map and weight columns of the
// group go to LDS once, then every pixel's operator is read once, sixteen [freq] rows per pass of the block (sixteen
// lanes to a row, so one butterfly of a wave reduces four rows), in a fixed order: spec[d] = sum_f op[d, f] m[f]
// (complex128), sweight[d] = inv0(sum_f |op[d, f]|^2 inv0(w[f])) (float32).
#include "chol_blocked.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int kWdMaxFreq = 1024;
constexpr int kWdGroup = 4;
constexpr int32_t kWdEmpty = 1, kWdNotPosdef = 2;

// T[c][r] = S[r][c0 + c] for c < nc: columns c0 ... c0 + nc of S [rows][cols] as the rows of T [nc][rows].
__global__ __launch_bounds__(256) void k_wd_transpose(int64_t rows, int64_t cols, int64_t c0, int64_t nc, const double* __restrict__ S, double* __restrict__ T) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t rb = (int64_t)blockIdx.y * 32, cb = (int64_t)blockIdx.x * 32;
  for (int i = ty; i < 32; i += 8) {
    const int64_t r = rb + i, c = cb + tx;
    tile[i][tx] = (r < rows && c < nc) ? S[r * cols + c0 + c] : 0.0;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int64_t c = cb + i, r = rb + tx;
    if (c < nc && r < rows) T[c * rows + r] = tile[tx][i];
  }
}

struct WdSlab {
  int n, nd, nra, nel, pol, r0, e0, ne;  // pixel b of the slab: ra = r0 + b / ne, el = e0 + b % ne
  const double* KT;                      // [nr][n][n] of the slab's run of RA
  const double* CT;
  const double* weight;  // [npol][n][nra][nel]
  const double* beam;    // [npol][n][nel]
  const double* window;  // [n]
  double* H;             // [nb][n][n]
  double* Hb;
  double* rr;            // [nb][n]
  uint8_t* mk;           // [nb][n]
  int32_t* status;       // [nb]
};

__global__ __launch_bounds__(256) void k_wd_assemble(WdSlab a) {
  __shared__ double sb[kWdMaxFreq];
  __shared__ uint8_t sm[kWdMaxFreq];
  __shared__ int s_valid;
  const int b = blockIdx.x, n = a.n;
  const int ral = b / a.ne, ra = a.r0 + ral, el = a.e0 + b % a.ne;
  const double* __restrict__ K = a.KT + (size_t)ral * n * n;
  const double* __restrict__ C = a.CT + (size_t)ral * n * n;
  if (threadIdx.x == 0) s_valid = 0;
  __syncthreads();
  int valid = 0;
  for (int g = threadIdx.x; g < n; g += 256) {
    const double w = a.weight[(((int64_t)a.pol * n + g) * a.nra + ra) * a.nel + el];
    const bool wm = a.window[g] > 0.0;
    const bool m = wm && w > 0.0;
    const double x = w * C[(size_t)g * n + g];
    const double r = wm ? sqrt(x == 0.0 ? 0.0 : 1.0 / x) : 0.0;
    a.rr[(size_t)b * n + g] = r;
    a.mk[(size_t)b * n + g] = sm[g] = m ? 1 : 0;
    sb[g] = sqrt(a.beam[((int64_t)a.pol * n + g) * a.nel + el]);
    valid += m ? 1 : 0;
  }
  if (valid) atomicAdd(&s_valid, valid);
  __syncthreads();
  if (s_valid == 0) {  // (the same in every thread)
    if (threadIdx.x == 0) a.status[b] = kWdEmpty;
    return;
  }
  double* H = a.H + (size_t)b * n * n;
  double* Hb = a.Hb + (size_t)b * n * n;
  for (int e = threadIdx.x; e < n * n; e += 256) {
    const int g = e / n, f = e % n;
    const double k = sm[g] ? K[e] : 0.0;
    H[e] = k;
    Hb[e] = k * sb[f];
  }
}

// E [2 n][2 n] holds Re (H P H^T) in its upper left block and -Im (H P H^T) in its upper right block (upper triangles).
__global__ __launch_bounds__(256) void k_wd_embed(int n, int ne, const double* __restrict__ CT, const double* __restrict__ rr, const uint8_t* __restrict__ mk, double* __restrict__ Eall,
                                                  const int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * n) return;
  const int g = idx / n, h = idx % n;
  if (g > h) return;
  const size_t N2 = 2 * (size_t)n;
  double* E = Eall + (size_t)b * N2 * N2;
  const double* __restrict__ C = CT + (size_t)(b / ne) * n * n;
  const double* __restrict__ r = rr + (size_t)b * n;
  const bool valid = mk[(size_t)b * n + g] && mk[(size_t)b * n + h];
  const double a = valid ? E[g * N2 + h] + C[idx] * (r[g] * r[h]) : (g == h ? 1.0 : 0.0);
  E[g * N2 + h] = a;
  E[(n + g) * N2 + n + h] = a;
  if (g == h) {
    E[g * N2 + n + g] = 0.0;
  } else {
    const double v = valid ? E[g * N2 + n + h] : 0.0;
    E[g * N2 + n + h] = v;
    E[h * N2 + n + g] = -v;
  }
}

template <typename T2>
__global__ __launch_bounds__(256) void k_wd_store(WdSlab a, const double* __restrict__ Yall, const double* __restrict__ sdiag, T2* __restrict__ out) {
  const int b = blockIdx.y, n = a.n, nd = a.nd;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nd * n) return;
  const int d = idx / n, g = idx % n;
  const int ra = a.r0 + b / a.ne, el = a.e0 + b % a.ne;
  double re = 0.0, im = 0.0;
  if (a.status[b] == 0 && a.mk[(size_t)b * n + g]) {
    const double* __restrict__ y = Yall + ((size_t)b * nd + d) * 2 * n;
    const double s = sdiag[d], w = a.window[g];
    re = (s * y[g]) * w;
    im = (s * -y[n + g]) * w;
  }
  T2 v;
  v.x = re;
  v.y = im;
  out[(((int64_t)a.pol * a.nra + ra) * a.nel + el) * nd * n + idx] = v;
}

// Sum over each group of kWdRowLanes consecutive lanes (a butterfly: the same order in every run), in every lane.
constexpr int kWdRowLanes = 16;
__device__ __forceinline__ double wd_group_sum(double v) {
#pragma unroll
  for (int o = kWdRowLanes / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T2>
__global__ __launch_bounds__(256) void k_wd_apply(int n, int nd, int nra, int nel, const T2* __restrict__ op, const double* __restrict__ map, const double* __restrict__ weight,
                                                  double2* __restrict__ spec, float* __restrict__ sweight) {
  extern __shared__ double s_lds[];  // m [kWdGroup][n], v [kWdGroup][n]
  double* sm = s_lds;
  double* sv = s_lds + kWdGroup * n;
  const int pol = blockIdx.z, ra = blockIdx.y, e0 = blockIdx.x * kWdGroup;
  const int ng = min(kWdGroup, nel - e0);
  for (int i = threadIdx.x; i < n * kWdGroup; i += 256) {
    const int f = i / kWdGroup, e = i % kWdGroup;
    if (e < ng) {
      const int64_t at = (((int64_t)pol * n + f) * nra + ra) * nel + e0 + e;
      const double w = weight[at];
      sm[e * n + f] = map[at];
      sv[e * n + f] = w == 0.0 ? 0.0 : 1.0 / w;
    }
  }
  __syncthreads();
  // sixteen lanes share a row, so a wave reduces four rows with one butterfly and the block takes sixteen rows a pass
  const int sub = threadIdx.x % kWdRowLanes, row = threadIdx.x / kWdRowLanes, nrow = 256 / kWdRowLanes;
  for (int e = 0; e < ng; ++e) {
    const int el = e0 + e;
    const T2* __restrict__ o = op + (((int64_t)pol * nra + ra) * nel + el) * nd * n;
    const double* m = sm + e * n;
    const double* v = sv + e * n;
    for (int d0 = 0; d0 < nd; d0 += nrow) {  // (every lane of a wave stays in the loop: the butterfly needs them all)
      const int d = d0 + row;
      double sr = 0.0, si = 0.0, sw = 0.0;
      if (d < nd) {
#pragma unroll 4
        for (int f = sub; f < n; f += kWdRowLanes) {
          const T2 z = o[(size_t)d * n + f];
          const double zr = (double)z.x, zi = (double)z.y;
          sr = fma(zr, m[f], sr);
          si = fma(zi, m[f], si);
          sw = fma(fma(zr, zr, zi * zi), v[f], sw);
        }
      }
      sr = wd_group_sum(sr);
      si = wd_group_sum(si);
      sw = wd_group_sum(sw);
      if (sub == 0 && d < nd) {
        const int64_t at = (((int64_t)pol * nel + el) * nra + ra) * nd + d;
        spec[at] = make_double2(sr, si);
        sweight[at] = (float)(sw == 0.0 ? 0.0 : 1.0 / sw);
      }
    }
  }
}

size_t wd_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int dmm_wienerdelay_build(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, int ndelay, const double* filter, const double* freq_cov, const double* weight, const double* beam_power,
                          const double* prior, const double* fourier, const double* sdiag, const double* window, void* out, int out_dtype, int64_t workspace_mib, int64_t* first_bad) {
  DMM_REQUIRE(ctx != nullptr, "dmm_wienerdelay_build: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kWdMaxFreq, "dmm_wienerdelay_build: nfreq %d outside 1 ... %d", nfreq, kWdMaxFreq);
  DMM_REQUIRE(ndelay >= 1 && ndelay <= nfreq, "dmm_wienerdelay_build: ndelay %d outside 1 ... nfreq = %d", ndelay, nfreq);
  DMM_REQUIRE(npol >= 0 && nra >= 0 && nel >= 0, "dmm_wienerdelay_build: negative count (%d pol, %d ra, %d el)", npol, nra, nel);
  DMM_REQUIRE(out_dtype == DMM_C64 || out_dtype == DMM_C128, "dmm_wienerdelay_build: bad output dtype %d", out_dtype);
  DMM_REQUIRE(workspace_mib >= 0, "dmm_wienerdelay_build: negative workspace %lld MiB", (long long)workspace_mib);
  DMM_REQUIRE(first_bad != nullptr, "dmm_wienerdelay_build: first_bad is NULL");
  *first_bad = -1;
  if (npol == 0 || nra == 0 || nel == 0) return DMM_OK;
  DMM_REQUIRE(filter && freq_cov && weight && beam_power && prior && fourier && sdiag && window && out, "dmm_wienerdelay_build: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));

  const int n = nfreq, nd = ndelay, N2 = 2 * n;
  const size_t nn = (size_t)n * n;
  // per pixel: H, Hb, T [n][2 n], E [2 n][2 n], Y [nd][2 n], r, the mask; and, per RA, the two transposed matrices
  const size_t per_pixel = sizeof(double) * (2 * nn + 2 * nn + 4 * nn + (size_t)nd * N2 + n) + n + sizeof(int32_t) + 2 * sizeof(double) * nn;
  const size_t ws = (size_t)(workspace_mib > 0 ? workspace_mib : 1024) << 20;
  const int64_t nbmax = std::max<int64_t>(1, std::min<int64_t>(65535, (int64_t)(ws / per_pixel)));
  const int ne_max = (int)std::min<int64_t>(nel, nbmax);
  const int nr_max = (int)std::min<int64_t>(nra, std::max<int64_t>(1, nbmax / ne_max));
  const size_t nbm = (size_t)ne_max * nr_max;

  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += wd_up(bytes);
    return at;
  };
  const size_t o_kt = take(sizeof(double) * nr_max * nn), o_ct = take(sizeof(double) * nr_max * nn);
  const size_t o_h = take(sizeof(double) * nbm * nn), o_hb = take(sizeof(double) * nbm * nn), o_t = take(sizeof(double) * nbm * 2 * nn);
  const size_t o_e = take(sizeof(double) * nbm * 4 * nn), o_y = take(sizeof(double) * nbm * nd * N2), o_r = take(sizeof(double) * nbm * n);
  const size_t o_m = take(nbm * n), o_s = take(sizeof(int32_t) * nbm);
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, off, &scratch);
  if (rc) return rc;
  char* base = (char*)scratch;
  double* KT = (double*)(base + o_kt);
  double* CT = (double*)(base + o_ct);
  double* T = (double*)(base + o_t);
  double* E = (double*)(base + o_e);
  double* Y = (double*)(base + o_y);
  int32_t* status = (int32_t*)(base + o_s);
  std::vector<int32_t> status_h(nbm);

  for (int pol = 0; pol < npol; ++pol) {
    for (int r0 = 0; r0 < nra; r0 += nr_max) {
      const int nr = std::min(nr_max, nra - r0);
      const dim3 tg((unsigned)((nr + 31) / 32), (unsigned)((nn + 31) / 32));
      hipLaunchKernelGGL(k_wd_transpose, tg, dim3(256), 0, ctx->stream, (int64_t)nn, (int64_t)nra, (int64_t)r0, (int64_t)nr, filter + (size_t)pol * nn * nra, KT);
      hipLaunchKernelGGL(k_wd_transpose, tg, dim3(256), 0, ctx->stream, (int64_t)nn, (int64_t)nra, (int64_t)r0, (int64_t)nr, freq_cov + (size_t)pol * nn * nra, CT);
      for (int e0 = 0; e0 < nel; e0 += ne_max) {
        const int ne = std::min(ne_max, nel - e0);
        const int nb = nr * ne;
        WdSlab a{};
        a.n = n, a.nd = nd, a.nra = nra, a.nel = nel, a.pol = pol, a.r0 = r0, a.e0 = e0, a.ne = ne;
        a.KT = KT, a.CT = CT, a.weight = weight, a.beam = beam_power, a.window = window;
        a.H = (double*)(base + o_h), a.Hb = (double*)(base + o_hb), a.rr = (double*)(base + o_r), a.mk = (uint8_t*)(base + o_m), a.status = status;
        DMM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * nb, ctx->stream));
        hipLaunchKernelGGL(k_wd_assemble, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
        DlGemm g{};  // T = Hb [Re P | Im P]
        g.A = a.Hb, g.a_rs = n, g.a_cs = 1, g.a_bs = (int64_t)nn;
        g.B = prior, g.b_rs = N2, g.b_cs = 1, g.b_bs = 0;
        g.C = T, g.c_rs = N2, g.c_bs = (int64_t)(2 * nn);
        g.M = n, g.N = N2, g.K = n, g.alpha = 1.0, g.beta = 0, g.upper = 0, g.status = status;
        dl_gemm(ctx, g, nb);
        for (int part = 0; part < 2; ++part) {  // Re A = T_r Hb^T and -Im A = -T_i Hb^T, upper tiles
          DlGemm q{};
          q.A = T + part * n, q.a_rs = N2, q.a_cs = 1, q.a_bs = (int64_t)(2 * nn);
          q.B = a.Hb, q.b_rs = 1, q.b_cs = n, q.b_bs = (int64_t)nn;
          q.C = E + part * n, q.c_rs = N2, q.c_bs = (int64_t)(4 * nn);
          q.M = n, q.N = n, q.K = n, q.alpha = part ? -1.0 : 1.0, q.beta = 0, q.upper = 1, q.status = status;
          dl_gemm(ctx, q, nb);
        }
        for (int part = 0; part < 2; ++part) {  // Y[d] = [Re (H F)[:, d] | Im (H F)[:, d]]
          DlGemm q{};
          q.A = fourier + (size_t)part * n * nd, q.a_rs = 1, q.a_cs = nd, q.a_bs = 0;
          q.B = a.H, q.b_rs = 1, q.b_cs = n, q.b_bs = (int64_t)nn;
          q.C = Y + part * n, q.c_rs = N2, q.c_bs = (int64_t)nd * N2;
          q.M = nd, q.N = n, q.K = n, q.alpha = 1.0, q.beta = 0, q.upper = 0, q.status = status;
          dl_gemm(ctx, q, nb);
        }
        hipLaunchKernelGGL(k_wd_embed, dim3((unsigned)((nn + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, n, ne, (const double*)CT, (const double*)a.rr, (const uint8_t*)a.mk, E,
                           (const int32_t*)status);
        dl_factor(ctx, N2, nb, E, status, kWdNotPosdef);
        dl_solve_rows(ctx, N2, nd, nd, nb, E, Y, status);
        const dim3 sg((unsigned)(((size_t)nd * n + 255) / 256), (unsigned)nb);
        if (out_dtype == DMM_C64)
          hipLaunchKernelGGL(k_wd_store<float2>, sg, dim3(256), 0, ctx->stream, a, (const double*)Y, sdiag, (float2*)out);
        else
          hipLaunchKernelGGL(k_wd_store<double2>, sg, dim3(256), 0, ctx->stream, a, (const double*)Y, sdiag, (double2*)out);
        DMM_HIP(hipGetLastError());
        DMM_HIP(hipMemcpyAsync(status_h.data(), status, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, ctx->stream));
        DMM_HIP(hipStreamSynchronize(ctx->stream));
        int64_t bad = -1;
        for (int b = 0; b < nb; ++b) {
          if (status_h[b] != kWdNotPosdef) continue;
          const int64_t at = ((int64_t)pol * nra + r0 + b / ne) * nel + e0 + b % ne;
          if (bad < 0 || at < bad) bad = at;
        }
        if (bad >= 0) {
          *first_bad = bad;
          return DMM_OK;
        }
      }
    }
  }
  return DMM_OK;
}

int dmm_wienerdelay_apply(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, int ndelay, const void* op, int op_dtype, const double* map, const double* weight, void* spectrum,
                          float* sweight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_wienerdelay_apply: ctx is NULL");
  DMM_REQUIRE(nfreq >= 1 && nfreq <= kWdMaxFreq, "dmm_wienerdelay_apply: nfreq %d outside 1 ... %d", nfreq, kWdMaxFreq);
  DMM_REQUIRE(ndelay >= 1, "dmm_wienerdelay_apply: bad delay count %d", ndelay);
  DMM_REQUIRE(npol >= 0 && npol <= 65535 && nra >= 0 && nra <= 65535 && nel >= 0, "dmm_wienerdelay_apply: bad count (%d pol, %d ra, %d el)", npol, nra, nel);
  DMM_REQUIRE(op_dtype == DMM_C64 || op_dtype == DMM_C128, "dmm_wienerdelay_apply: bad operator dtype %d", op_dtype);
  if (npol == 0 || nra == 0 || nel == 0) return DMM_OK;
  DMM_REQUIRE(op && map && weight && spectrum && sweight, "dmm_wienerdelay_apply: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((nel + kWdGroup - 1) / kWdGroup), (unsigned)nra, (unsigned)npol);
  const size_t lds = sizeof(double) * 2 * kWdGroup * nfreq;
  if (op_dtype == DMM_C64) {
    DMM_HIP(hipFuncSetAttribute((const void*)k_wd_apply<float2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_wd_apply<float2>, grid, dim3(256), lds, ctx->stream, nfreq, ndelay, nra, nel, (const float2*)op, map, weight, (double2*)spectrum, sweight);
  } else {
    DMM_HIP(hipFuncSetAttribute((const void*)k_wd_apply<double2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_wd_apply<double2>, grid, dim3(256), lds, ctx->stream, nfreq, ndelay, nra, nel, (const double2*)op, map, weight, (double2*)spectrum, sweight);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
