// Batched float64 Cholesky factorisation and triangular solves of dense symmetric positive definite systems: the
// interface of chol_blocked.hip (the solver that delay.hip, mfilter.hip and dpss.hip call) and the device pieces it
// shares with the kernels of dayenu.hip and dpss.hip that have the same bodies.
//
// Host side (chol_blocked.hip): dl_gemm, dl_factor and dl_solve_rows.  G [nbase][n][n] row-major (only the upper
// triangle is read and written), Y [nbase][nrow][n]: each of the first nsolve rows is a right-hand side and is replaced
// by its solution.  Every kernel leaves a matrix alone once its status word is set.
//
// Device side (inline, compiled into the kernel that calls them):
//   dl_tile_mma / dl_tile_each   the 64 x 64 tile product on v_mfma_f64_16x16x4_f64 of 256 threads, 2 x 2 waves of
//                 2 x 2 accumulators each, from two staged LDS slices, and the accumulators' (row, column) map;
//   dl_potrf_lds  D = Ud^T Ud of one diagonal block (at most 32 x 32) in LDS;
//   dl_fwd_col    Ud^T x = a for one column held in registers.
#pragma once
#include "dmm_internal.h"

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

// chol_blocked.hip: the launches go to ctx->stream; nbase <= 65535 matrices per call.
int dl_gemm(dmm_ctx* ctx, const DlGemm& g, int nbase);
// G = U^T U, upper triangle, right-looking; `fail` is what a non-positive pivot stores in status.
void dl_factor(dmm_ctx* ctx, int n, int nbase, double* G, int32_t* status, int32_t fail);
// U^T U x = y for the first nsolve rows of every Y [nrow][n] (the rows behind them are not touched).
void dl_solve_rows(dmm_ctx* ctx, int n, int nrow, int nsolve, int nbase, const double* G, double* Y, const int32_t* status);

// ---- the 64 x 64 tile product
constexpr int kTileK = 16, kTileLP = kTileK + 1;  // K-chunk of one staged slice, and the pitch of its 64 rows in LDS

// acc[c] += a_c(as) bs^T over one staged pair of slices as, bs [64][kTileLP], for NC accumulator sets that share the
// slices: aop(c, a, k) is the A operand set c multiplies at column k of the slice (a itself, or a scaled).
template <int NC, typename AOp>
__device__ __forceinline__ void dl_tile_mma(const double* as, const double* bs, v4d (*acc)[2][2], AOp aop) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < kTileK; kk += 4) {
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = as[(32 * wr + 16 * t + lr) * kTileLP + kk + lk];
      b[t] = bs[(32 * wc + 16 * t + lr) * kTileLP + kk + lk];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        const double ac = aop(c, a[ti], kk + lk);
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[c][ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac, b[tj], acc[c][ti][tj], 0, 0, 0);
      }
  }
}

__device__ __forceinline__ void dl_tile_mma(const double* as, const double* bs, v4d (&acc)[2][2]) {
  dl_tile_mma<1>(as, bs, &acc, [](int, double a, int) { return a; });
}

// f(row, column, value) for the 16 elements of the tile this thread's accumulators hold (row, column in 0 ... 63)
template <typename F>
__device__ __forceinline__ void dl_tile_each(const v4d (&acc)[2][2], F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) f(32 * wr + 16 * ti + lk + 4 * reg, 32 * wc + 16 * tj + lr, acc[ti][tj][reg]);
}

// ---- the diagonal block
// D = Ud^T Ud in place on the upper triangle of sD (order nb <= kDB), by the nthreads >= kDB threads of the block; sD is
// complete behind a barrier on entry and on return.  Returns true, in every thread, at the first pivot that is not
// positive.
__device__ __forceinline__ bool dl_potrf_lds(double (*sD)[kDB + 1], int nb, int nthreads) {
  const int i = threadIdx.x;
  for (int c = 0; c < nb; ++c) {
    const double d = sD[c][c];
    if (!(d > 0.0)) return true;  // (the same value in every thread)
    const double r = sqrt(d);
    __syncthreads();
    if (i == c) sD[c][c] = r;
    if (i > c && i < nb) sD[c][i] = sD[c][i] / r;
    __syncthreads();
    for (int e = threadIdx.x; e < nb * nb; e += nthreads) {
      const int rr = e / nb, cc = e % nb;
      if (rr > c && cc >= rr) sD[rr][cc] = fma(-sD[c][rr], sD[c][cc], sD[rr][cc]);
    }
    __syncthreads();
  }
  return false;
}

// Ud^T x = a for one column in registers: x_c = (a_c - sum_{q < c} x_q Ud[q][c]) / Ud[c][c] for c < nb, in place, and
// put(c, x_c) as each one is known.  (nb = kDB on a block padded with the identity: no test per element.)
template <typename Put>
__device__ __forceinline__ void dl_fwd_col(const double (*sD)[kDB + 1], int nb, double (&acc)[kDB], Put put) {
#pragma unroll
  for (int c = 0; c < kDB; ++c) {
    if (c < nb) {
      double s = acc[c];
#pragma unroll
      for (int q = 0; q < c; ++q) s = fma(-sD[q][c], acc[q], s);
      acc[c] = s / sD[c][c];
      put(c, acc[c]);
    }
  }
}
