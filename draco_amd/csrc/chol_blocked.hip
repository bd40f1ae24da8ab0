// Batched float64 Cholesky factorisation and triangular solves of dense symmetric positive definite systems, behind
// chol_blocked.h: delay.hip (the Wiener filter, order up to 2048), mfilter.hip (the DAYENU m-mode filter, order up to
// 4096) and dpss.hip (the DPSS Wiener filter) call the one copy compiled here.
//
//   k_dl_gemm     C = beta C + alpha A B on v_mfma_f64_16x16x4_f64, 64 x 64 tiles, either operand through any strides:
//                 the trailing updates of the factorisation, the updates of the solves (and delay.hip's projection);
//   k_dl_potrf / k_dl_panel   G = U^T U, right-looking in blocks of 32 rows: the diagonal block in LDS, the row panel
//                 one column per thread, the rest is k_dl_gemm on the upper tiles; a non-positive pivot sets status;
//   k_dl_trsm     the 32 x 32 diagonal step of Z U = Y and X U^T = Z, one right-hand side per thread (the rows of Y).
// dl_factor and dl_solve_rows are the host loops.  The tile product, the factorisation of a diagonal block and the
// forward substitution of a column are the inline pieces of chol_blocked.h, which dayenu.hip and dpss.hip use too.
//
// Index ranges (n <= 4096, nbase <= 65535): element offsets inside one matrix stay below 2^24 and are formed in
// size_t / int64_t together with the batch offset; k_dl_gemm forms m * a_rs + k * a_cs in int64_t; the grids are
// (ceil(N / 64), ceil(M / 64), nbase) and (ceil(rows / 256), nbase), so M and nsolve may reach 65535 x 64 rows per call.
#include "chol_blocked.h"

#include <algorithm>

namespace {

__global__ __launch_bounds__(256) void k_dl_gemm(DlGemm g) {
  __shared__ double as[64 * kTileLP];
  __shared__ double bs[64 * kTileLP];
  const int bat = blockIdx.z;
  if (g.status[bat]) return;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (g.upper && m0 > n0) return;
  const double* __restrict__ A = g.A + (size_t)bat * g.a_bs;
  const double* __restrict__ B = g.B + (size_t)bat * g.b_bs;
  double* C = g.C + (size_t)bat * g.c_bs;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d acc[2][2] = {{vz, vz}, {vz, vz}};
  const bool a_kfast = g.a_cs == 1, b_nfast = g.b_cs == 1;
  for (int k0 = 0; k0 < g.K; k0 += kTileK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + 256 * i;
      {
        const int r = a_kfast ? e >> 4 : e & 63, kk = a_kfast ? e & 15 : e >> 6;
        const int m = m0 + r, k = k0 + kk;
        as[r * kTileLP + kk] = (m < g.M && k < g.K) ? A[m * g.a_rs + k * g.a_cs] : 0.0;
      }
      {
        const int c = b_nfast ? e & 63 : e >> 4, kk = b_nfast ? e >> 6 : e & 15;
        const int n = n0 + c, k = k0 + kk;
        bs[c * kTileLP + kk] = (n < g.N && k < g.K) ? B[k * g.b_rs + n * g.b_cs] : 0.0;
      }
    }
    __syncthreads();
    dl_tile_mma(as, bs, acc);
  }
  dl_tile_each(acc, [&](int r, int c, double a) {
    const int row = m0 + r, col = n0 + c;
    if (row < g.M && col < g.N) {
      double* p = C + (size_t)row * g.c_rs + col;
      const double v = g.alpha * a;
      *p = g.beta ? *p + v : v;
    }
  });
}

// The diagonal block J0 ... J0 + nb of the upper triangle: D = Ud^T Ud in LDS, one block per matrix.  A pivot that
// is not positive stores `fail` in the matrix's status word.
__global__ __launch_bounds__(256) void k_dl_potrf(int n, int J0, int nb, double* __restrict__ Gall, int32_t* __restrict__ status, int32_t fail) {
  __shared__ double sD[kDB][kDB + 1];
  const int bat = blockIdx.x;
  if (status[bat]) return;
  double* G = Gall + (size_t)bat * n * n;
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    sD[r][c] = c >= r ? G[(size_t)(J0 + r) * n + J0 + c] : 0.0;
  }
  __syncthreads();
  if (dl_potrf_lds(sD, nb, 256)) {  // (the whole block leaves)
    if (threadIdx.x == 0) status[bat] = fail;
    return;
  }
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int r = e / nb, c = e % nb;
    if (c >= r) G[(size_t)(J0 + r) * n + J0 + c] = sD[r][c];
  }
}

__device__ __forceinline__ void dl_load_diag(double (*sD)[kDB + 1], const double* G, int n, int J0, int nb) {
  for (int e = threadIdx.x; e < kDB * kDB; e += blockDim.x) {
    const int r = e / kDB, c = e % kDB;
    sD[r][c] = (r < nb && c < nb && c >= r) ? G[(size_t)(J0 + r) * n + J0 + c] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
}

// The row panel right of the diagonal block: Ud^T x = a, one column per thread.
__global__ __launch_bounds__(256) void k_dl_panel(int n, int J0, int nb, double* __restrict__ Gall, const int32_t* __restrict__ status) {
  __shared__ double sD[kDB][kDB + 1];
  const int bat = blockIdx.y;
  if (status[bat]) return;
  double* G = Gall + (size_t)bat * n * n;
  dl_load_diag(sD, G, n, J0, nb);
  const int i = J0 + nb + blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[kDB];
#pragma unroll
  for (int c = 0; c < kDB; ++c) acc[c] = c < nb ? G[(size_t)(J0 + c) * n + i] : 0.0;
  dl_fwd_col(sD, nb, acc, [&](int c, double x) { G[(size_t)(J0 + c) * n + i] = x; });
}

// The diagonal step of the solves on the rows of Y, one right-hand side per thread:
// forward  z_c = (y_c - sum_{q < c} z_q U[q][c]) / U[c][c],   backward  x_c = (z_c - sum_{q > c} x_q U[c][q]) / U[c][c].
__global__ __launch_bounds__(256) void k_dl_trsm(int n, int J0, int nb, int nrow, int nsolve, int backward, const double* __restrict__ Gall, double* __restrict__ Yall, const int32_t* __restrict__ status) {
  __shared__ double sD[kDB][kDB + 1];
  const int bat = blockIdx.y;
  if (status[bat]) return;
  dl_load_diag(sD, Gall + (size_t)bat * n * n, n, J0, nb);
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nsolve) return;
  double* y = Yall + ((size_t)bat * nrow + r) * n + J0;
  double acc[kDB];
#pragma unroll
  for (int c = 0; c < kDB; ++c) acc[c] = c < nb ? y[c] : 0.0;
  // (the block is padded with the identity: both directions run over all kDB rows, and those from nb on stay zero)
  if (!backward) {
    dl_fwd_col(sD, kDB, acc, [](int, double) {});
  } else {
#pragma unroll
    for (int c = kDB - 1; c >= 0; --c) {
      double s = acc[c];
#pragma unroll
      for (int q = c + 1; q < kDB; ++q) s = fma(-sD[c][q], acc[q], s);
      acc[c] = s / sD[c][c];
    }
  }
#pragma unroll
  for (int c = 0; c < kDB; ++c)
    if (c < nb) y[c] = acc[c];
}

}  // namespace

int dl_gemm(dmm_ctx* ctx, const DlGemm& g, int nbase) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return DMM_OK;
  const dim3 grid((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 63) / 64), (unsigned)nbase);
  hipLaunchKernelGGL(k_dl_gemm, grid, dim3(256), 0, ctx->stream, g);
  return DMM_OK;
}

void dl_factor(dmm_ctx* ctx, int n, int nbase, double* G, int32_t* status, int32_t fail) {
  const int64_t nn = (int64_t)n * n;
  for (int J0 = 0; J0 < n; J0 += kDB) {
    const int nb = std::min(kDB, n - J0), rem = n - J0 - nb;
    hipLaunchKernelGGL(k_dl_potrf, dim3((unsigned)nbase), dim3(256), 0, ctx->stream, n, J0, nb, G, status, fail);
    if (rem == 0) break;
    hipLaunchKernelGGL(k_dl_panel, dim3((unsigned)((rem + 255) / 256), (unsigned)nbase), dim3(256), 0, ctx->stream, n, J0, nb, G, (const int32_t*)status);
    DlGemm g{};  // G[J1 + i][J1 + j] -= sum_k U[J0 + k][J1 + i] U[J0 + k][J1 + j]
    const double* P = G + (size_t)J0 * n + J0 + nb;
    g.A = P, g.a_rs = 1, g.a_cs = n, g.a_bs = nn;
    g.B = P, g.b_rs = n, g.b_cs = 1, g.b_bs = nn;
    g.C = G + (size_t)(J0 + nb) * n + J0 + nb, g.c_rs = n, g.c_bs = nn;
    g.M = rem, g.N = rem, g.K = nb;
    g.alpha = -1.0, g.beta = 1, g.upper = 1;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
}

void dl_solve_rows(dmm_ctx* ctx, int n, int nrow, int nsolve, int nbase, const double* G, double* Y, const int32_t* status) {
  const int64_t nn = (int64_t)n * n;
  // ---- Z U = Y, block column by block column
  const unsigned rb = (unsigned)((nsolve + 255) / 256);
  for (int J0 = 0; J0 < n; J0 += kDB) {
    const int nb = std::min(kDB, n - J0), rem = n - J0 - nb;
    hipLaunchKernelGGL(k_dl_trsm, dim3(rb, (unsigned)nbase), dim3(256), 0, ctx->stream, n, J0, nb, nrow, nsolve, 0, G, Y, status);
    DlGemm g{};  // Y[:, J1 ...] -= Z[:, J0 ... J1] U[J0 ... J1][J1 ...]
    g.A = Y + J0, g.a_rs = n, g.a_cs = 1, g.a_bs = (int64_t)nrow * n;
    g.B = G + (size_t)J0 * n + J0 + nb, g.b_rs = n, g.b_cs = 1, g.b_bs = nn;
    g.C = Y + J0 + nb, g.c_rs = n, g.c_bs = (int64_t)nrow * n;
    g.M = nsolve, g.N = rem, g.K = nb;
    g.alpha = -1.0, g.beta = 1, g.upper = 0;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
  // ---- X U^T = Z, from the last block column down
  for (int J0 = (n - 1) / kDB * kDB; J0 >= 0; J0 -= kDB) {
    const int nb = std::min(kDB, n - J0);
    hipLaunchKernelGGL(k_dl_trsm, dim3(rb, (unsigned)nbase), dim3(256), 0, ctx->stream, n, J0, nb, nrow, nsolve, 1, G, Y, status);
    DlGemm g{};  // Z[:, j] -= sum_k X[:, J0 + k] U[j][J0 + k], j < J0
    g.A = Y + J0, g.a_rs = n, g.a_cs = 1, g.a_bs = (int64_t)nrow * n;
    g.B = G + J0, g.b_rs = 1, g.b_cs = n, g.b_bs = nn;
    g.C = Y, g.c_rs = n, g.c_bs = (int64_t)nrow * n;
    g.M = nsolve, g.N = J0, g.K = nb;
    g.alpha = -1.0, g.beta = 1, g.upper = 0;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
}
