// Batched float64 Cholesky factorisation and triangular solves of dense symmetric positive definite systems, shared by
// delay.hip (the Wiener filter, order up to 2048) and mfilter.hip (the DAYENU m-mode filter, order up to 4096).
//
//   k_dl_gemm     C = beta C + alpha A B on v_mfma_f64_16x16x4_f64, 64 x 64 tiles, either operand through any strides:
//                 the trailing updates of the factorisation, the updates of the solves (and delay.hip's projection);
//   k_dl_potrf / k_dl_panel   G = U^T U, right-looking in blocks of 32 rows: the diagonal block in LDS, the row panel
//                 one column per thread, the rest is k_dl_gemm on the upper tiles; a non-positive pivot sets status;
//   k_dl_trsm     the 32 x 32 diagonal step of Z U = Y and X U^T = Z, one right-hand side per thread (the rows of Y).
// dl_factor and dl_solve_rows are the host loops.  G [nbase][n][n] row-major (only the upper triangle is read and
// written), Y [nbase][nrow][n]: each of the first nsolve rows is a right-hand side and is replaced by its solution.
// Every kernel leaves a matrix alone once its status word is set.
//
// Index ranges (n <= 4096, nbase <= 65535): element offsets inside one matrix stay below 2^24 and are formed in
// size_t / int64_t together with the batch offset; k_dl_gemm forms m * a_rs + k * a_cs in int64_t; the grids are
// (ceil(N / 64), ceil(M / 64), nbase) and (ceil(rows / 256), nbase), so M and nsolve may reach 65535 x 64 rows per call.
#pragma once
#include "dmm_internal.h"

#include <algorithm>

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kDB = 32;  // block height of the factorisation and of the triangular solves

// C[m][n] = beta C[m][n] + alpha sum_k A[m][k] B[k][n]; A and B through (row, column) strides, C rows of stride c_rs.
struct DlGemm {
  const double* A;
  const double* B;
  double* C;
  int64_t a_rs, a_cs, a_bs, b_rs, b_cs, b_bs, c_rs, c_bs;
  int M, N, K;
  double alpha;
  int beta, upper;  // upper: tiles wholly below the diagonal are left alone
  const int32_t* status;
};

__global__ __launch_bounds__(256) void k_dl_gemm(DlGemm g) {
  constexpr int KC = 16, LP = KC + 1;
  __shared__ double as[64 * LP];
  __shared__ double bs[64 * LP];
  const int bat = blockIdx.z;
  if (g.status[bat]) return;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  if (g.upper && m0 > n0) return;
  const double* __restrict__ A = g.A + (size_t)bat * g.a_bs;
  const double* __restrict__ B = g.B + (size_t)bat * g.b_bs;
  double* C = g.C + (size_t)bat * g.c_bs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
  const v4d vz = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d acc[2][2] = {{vz, vz}, {vz, vz}};
  const bool a_kfast = g.a_cs == 1, b_nfast = g.b_cs == 1;
  for (int k0 = 0; k0 < g.K; k0 += KC) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + 256 * i;
      {
        const int r = a_kfast ? e >> 4 : e & 63, kk = a_kfast ? e & 15 : e >> 6;
        const int m = m0 + r, k = k0 + kk;
        as[r * LP + kk] = (m < g.M && k < g.K) ? A[m * g.a_rs + k * g.a_cs] : 0.0;
      }
      {
        const int c = b_nfast ? e & 63 : e >> 4, kk = b_nfast ? e >> 6 : e & 15;
        const int n = n0 + c, k = k0 + kk;
        bs[c * LP + kk] = (n < g.N && k < g.K) ? B[k * g.b_rs + n * g.b_cs] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = as[(32 * wr + 16 * t + lr) * LP + kk + lk];
        b[t] = bs[(32 * wc + 16 * t + lr) * LP + kk + lk];
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
    }
  }
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = m0 + 32 * wr + 16 * ti + lk + 4 * reg, col = n0 + 32 * wc + 16 * tj + lr;
        if (row < g.M && col < g.N) {
          double* p = C + (size_t)row * g.c_rs + col;
          const double v = g.alpha * acc[ti][tj][reg];
          *p = g.beta ? *p + v : v;
        }
      }
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
  const int i = threadIdx.x;
  for (int c = 0; c < nb; ++c) {
    const double d = sD[c][c];
    if (!(d > 0.0)) {  // (the same value in every thread: the whole block leaves)
      if (threadIdx.x == 0) status[bat] = fail;
      return;
    }
    const double r = sqrt(d);
    __syncthreads();
    if (i == c) sD[c][c] = r;
    if (i > c && i < nb) sD[c][i] = sD[c][i] / r;
    __syncthreads();
    for (int e = threadIdx.x; e < nb * nb; e += 256) {
      const int rr = e / nb, cc = e % nb;
      if (rr > c && cc >= rr) sD[rr][cc] = fma(-sD[c][rr], sD[c][cc], sD[rr][cc]);
    }
    __syncthreads();
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
#pragma unroll
  for (int c = 0; c < kDB; ++c) {
    if (c < nb) {
      double s = acc[c];
#pragma unroll
      for (int q = 0; q < c; ++q) s = fma(-sD[q][c], acc[q], s);
      acc[c] = s / sD[c][c];
      G[(size_t)(J0 + c) * n + i] = acc[c];
    }
  }
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
  if (!backward) {
#pragma unroll
    for (int c = 0; c < kDB; ++c) {
      double s = acc[c];
#pragma unroll
      for (int q = 0; q < c; ++q) s = fma(-sD[q][c], acc[q], s);
      acc[c] = s / sD[c][c];
    }
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

int dl_gemm(dmm_ctx* ctx, const DlGemm& g, int nbase) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return DMM_OK;
  const dim3 grid((unsigned)((g.N + 63) / 64), (unsigned)((g.M + 63) / 64), (unsigned)nbase);
  hipLaunchKernelGGL(k_dl_gemm, grid, dim3(256), 0, ctx->stream, g);
  return DMM_OK;
}

// G = U^T U, upper triangle, right-looking; `fail` is what a non-positive pivot stores in status.
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

// U^T U x = y for the first nsolve rows of every Y [nrow][n] (the rows behind them are not touched).
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

}  // namespace
