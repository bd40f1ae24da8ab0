// Dense per-(m, freq) solves: Wiener filter (Gram + Cholesky) and maximum likelihood (Gram + certificate and Cholesky, or
// a Hermitian eigen-decomposition with the reference's singular-value cut: two-stage reduction to tridiagonal form
// (herm_band.h) + QL in factored form (herm_tridiag.h) by default, blocked Jacobi for a handful of matrices and as fallback).
//
//   dmm_wiener_run  WienerMapMaker._solve_m             reference mapmaker.py:235-284
//   dmm_ml_run      MaximumLikelihoodMapMaker._solve_m  reference mapmaker.py:184-201
//                   + pinv_svd                          reference mapmaker.py:287-300
//
// Both are formed on the TELESCOPE side (ntel x ntel), which is the reference's own
// branch whenever ntel <= nsky (mapmaker.py:267,275-278: every BASELINE config) and is
// algebraically the same estimator otherwise:
//   Wiener:  G = I + D B S B^H D,  a = S o B^H D G^-1 D v            (D = diag sqrt(Ni))
//   ML:      G =     D B   B^H D = U L U^H,  a = B^H D U_r L_r^-1 U_r^H D v
//            with the columns kept where sqrt(L) > rcond*sqrt(L_max) and sqrt(L) > acond.
// Rows with Ni = 0 decouple (unit diagonal / zero eigenvalue): no NaN, like the reference.
//
// ML, full-rank shortcut.  pinv_svd keeps sigma > rcond*sigma_max and sigma > acond; when NO
// singular value of D B is cut the pseudo-inverse is an ordinary inverse:
//   ntel <= nsky_m (telescope side):  a = B^H D (D B B^H D)^-1 D v
//   nsky_m < ntel  (sky side):        a = (B^H Ni B)^-1 B^H Ni v     (the smaller Gram matrix)
// and "nothing is cut" is CERTIFIED without an eigen-decomposition: with theta >= lambda_max
// (theta = max row sum of |G|) and tau = max(rcond^2 theta, acond^2), the Cholesky factorisation
// of G - tau I succeeds  <=>  lambda_min(G) > tau >= the reference's cut.  Tiles that pass are
// solved by a second Cholesky (of G itself); tiles that fail -- some mode really is, or may be,
// cut -- take the Jacobi eigen-decomposition of the same (smaller-side) Gram matrix.  Exactly
// zero rows (masked baselines, structurally empty sky columns) are zero modes the reference
// drops: they are pinned to a unit-scale diagonal and contribute nothing either way.
//
// Kernel structure (all batched over the matrices of a sub-batch):
//   k_nt<GRAM>    G(I,J)  = [delta] + d_i d_j sum_k B[i,k] S_k conj(B[j,k])   64x64 tiles, f64 MFMA
//   k_nt<UPDATE>  A(I,J) -= sum_{k<64J} L[i,k] conj(L[j,k])                   (left-looking Cholesky)
//   k_chol_diag   A(J,J) = L L^H in LDS, Linv_J = L^-1
//   k_nt<PANEL>   L(I,J)  = A(I,J) Linv_J^H
//   k_chol_solve  y = L^-H L^-1 (D v);  w = D y
//   k_dirty (w mode, solve_dirty.hip)  a = S o B^H w
// The complex products run on v_mfma_f64_16x16x4_f64 through the real embedding
//   Re = [Xr Xi].[Yr Yi]^T,  Im = [Xr Xi].[-Yi Yr]^T   (4 real k per 2 complex k).
//
// Host structure.  dense_layout.h: sizes, batch capacity, the carving of the workspace, the work ranges (no HIP).  Shared by
// both makers: carve_ws, partition_tiles, gslot_table, batch_params, upload_lists / upload_slots, form_gram, chol_factor.
// dmm_ml_run is the schedule of an ML pass over one MlPass, whose member functions are the steps: null_certificate;
// certify -> cert_batch; early; eigen_list -> launch_chunk / retire (pipelined) or eigen_batch -> reduce, jacobi; drain.
#include "dense_kernels.h"
#include "dense_layout.h"
#include "herm_tridiag.h"
#include "herm_band.h"
#ifdef DMM_AB  // forms measured slower than the shipped ones, kept buildable (make EXTRA=-DDMM_AB): "ml_reduce" = 5
#include "herm_band_fused.h"
#endif

#define DMM_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)  // (as DMM_HIP, for the library's own status codes)

namespace {

// One sweep over the trailing matrix of column tp.j.  np_pend = rank-2 updates pending at this point; the sweep
// applies them all once their number reaches what the kernel variant keeps in registers (4 pairs at three column
// chunks per wave, 2 at six, 1 at eight or with full-matrix storage), otherwise it only reads.  Returns through
// np_pend the number still pending afterwards.
template <int KK, int NB>
void td_launch_tri(TdParams& tp, int& np_pend, dim3 grid, hipStream_t st) {
  tp.np = np_pend;
  if (np_pend < NB) {
    hipLaunchKernelGGL((k_td_trail_tri<KK, 0>), grid, dim3(kThreads), 0, st, tp);
  } else {
    hipLaunchKernelGGL((k_td_trail_tri<KK, NB>), grid, dim3(kThreads), 0, st, tp);
    np_pend = 0;
  }
}

void td_launch_trail(TdParams& tp, int& np_pend, int nmat, hipStream_t st) {
  const int n = tp.d.Np, j = tp.j;
  const dim3 grid((n - j - 1 + kTdRows - 1) / kTdRows, nmat);
  if (!tp.tri) {
    tp.np = np_pend;  // 0 (first column) or 1
    hipLaunchKernelGGL(k_td_trail, grid, dim3(kThreads), (size_t)3 * (n - j - 1) * sizeof(double2), st, tp);
    np_pend = 0;
  } else if (n <= 768) {
    td_launch_tri<3, 4>(tp, np_pend, grid, st);
  } else if (n <= 1536) {
    td_launch_tri<6, 2>(tp, np_pend, grid, st);
  } else {
    td_launch_tri<8, 1>(tp, np_pend, grid, st);
  }
}

// Householder reduction of the launch's matrices to tridiagonal form: n column steps (k_td_col) and n-1 sweeps.
void td_reduce(TdParams& tp, int nmat, hipStream_t st) {
  const int n = tp.d.Np;
  const size_t col_lds = (size_t)2 * n * sizeof(double2);
  int np_pend = 0;
  for (int j = 0; j < n; ++j) {
    tp.j = j;
    tp.np = np_pend;
    hipLaunchKernelGGL(k_td_col, dim3(nmat), dim3(kThreads), col_lds, st, tp);
    if (j >= 1) ++np_pend;  // k_td_col has completed the pair of column j-1
    if (j < n - 1) td_launch_trail(tp, np_pend, nmat, st);
  }
}

// ---- two-stage reduction (herm_band.h): dense -> band of half-width 8 on the MFMA units, band -> tridiagonal in LDS
constexpr size_t kSbLdsMax = 160 * 1024;
bool sb_fits(int n) {
  return n >= 64 && n % 64 == 0 && n <= kSbRows * kThreads && sb_chase_lds(n) + 4608 <= kSbLdsMax;  // (+ the chase kernel's static scratch)
}
bool sb_usable(const dmm_ctx* ctx, int n) { return ctx->opt_ml_reduce != 1 && sb_fits(n); }
// the largest order <= n the two-stage reduction takes (0: none).  A call whose telescope order is above the limit still
// reduces its smaller sky-side matrices in two stages: the dynamic-LDS attributes are set for this order, not for n
int sb_top(const dmm_ctx* ctx, int n) {
  for (int k = n / 64 * 64; k >= 64; k -= 64)
    if (sb_usable(ctx, k)) return k;
  return 0;
}
// QL's rotation log shares the matrix's log region with the T factors and the chase's reflector log at its tail
// "ml_rank_stop": the tolerance of the band reduction's rank stop (herm_band.h), relative to the lower bound of lambda_max
double sb_stop_tol(const dmm_ctx* ctx) {
  const int v = ctx->opt_ml_rank_stop;
  if (v == 1) return 0.0;
  double t = 1e-13;
  if (v >= 2) {  // (clamped: never looser than 1e-11 of lambda_max -- the bound ||C|| <= trace T_k of herm_band.h holds for
    t = 1.0;     //  positive semi-definite input only, which is what every caller of sb_reduce with a stop passes)
    for (int i = 0; i < (v < 11 ? 11 : v) && i < 30; ++i) t *= 0.1;
  }
  return t;
}
int64_t sb_log_cap(int64_t log_stride, int n, int runs) {
  return log_stride - sb_tail(n) - ((int64_t)3 * runs * (int64_t)sizeof(int) + 15) / 16;
}
// "ml_reduce" = 0: up to kSbNB two-sided updates pending (herm_band.h: the trailing matrix is written by every kSbNB-th
// sweep only); 2: none deferred (rounds 3-5).  Small orders, whose log region has no room for the rings, defer nothing.
int sb_pending(const dmm_ctx* ctx, int n, int64_t log_stride) {
  int nb = ctx->opt_ml_reduce == 2 ? 1 : kSbNB;
  while (nb > 1 && sb_head(n, nb) + sb_tail(n) > log_stride) nb >>= 1;
  return nb;
}
void sb_reduce(TdParams& tp, int nmat, hipStream_t st) {
  const int n = tp.d.Np, K = sb_npanel(n);
#ifdef DMM_AB
  if (tp.fused && n <= 3 * kThreads && sb_fused_lds(n) <= kSbFusedLdsMax) {  // the whole of stage 1 as one launch, a block per matrix (herm_band_fused.h)
    const size_t lds = sb_fused_lds(n);
    if (n <= kThreads) hipLaunchKernelGGL(k_sb_fused<1>, dim3(nmat), dim3(kThreads), lds, st, tp);
    else if (n <= 2 * kThreads) hipLaunchKernelGGL(k_sb_fused<2>, dim3(nmat), dim3(kThreads), lds, st, tp);
    else hipLaunchKernelGGL(k_sb_fused<3>, dim3(nmat), dim3(kThreads), lds, st, tp);
    return;
  }
#endif
  hipLaunchKernelGGL(k_sb_zero, dim3(12, nmat), dim3(kThreads), 0, st, tp);
  auto panel = [&]() {  // rows per thread by what is left of the matrix: the later panels take fewer registers (more blocks per CU)
    const int rows = (n - kSbB * tp.j + kThreads - 1) / kThreads;
    if (rows <= 1) hipLaunchKernelGGL(k_sb_panel<1>, dim3(nmat), dim3(kThreads), 0, st, tp);
    else if (rows == 2) hipLaunchKernelGGL(k_sb_panel<2>, dim3(nmat), dim3(kThreads), 0, st, tp);
    else if (rows == 3) hipLaunchKernelGGL(k_sb_panel<3>, dim3(nmat), dim3(kThreads), 0, st, tp);
    else hipLaunchKernelGGL(k_sb_panel<4>, dim3(nmat), dim3(kThreads), 0, st, tp);
  };
  tp.p0 = 0;
  int zfull_next = 0, zw_next = 64;
  for (int k = 0; k < K; ++k) {
    tp.j = k;
    tp.zfull = zfull_next;
    tp.zw = zw_next;
    zfull_next = 0;
    zw_next = 64;
    if (tp.p0 < k - 1) hipLaunchKernelGGL(k_sb_pend, dim3(nmat), dim3(kThreads), 0, st, tp);  // (update k-2 still pending: its corrections)
    panel();
    const int org = (kSbB * (k + 1)) & ~15;
    const dim3 grid(nmat, (n - org + 63) / 64);
    if (k - tp.p0 < tp.nb) {  // fewer than nb updates pending: the sweep only reads
      if (tp.one_block) {
        hipLaunchKernelGGL(k_sb_sweep_one, dim3(nmat), dim3(64 * kSbOneWaves), sb_one_lds(n - org), st, tp);
        zfull_next = 1;
      } else {
        constexpr int BW0 = 16 * sb_ncb(0);
        hipLaunchKernelGGL(k_sb_sweep_lo<0>, dim3(nmat, (n - org + BW0 - 1) / BW0), dim3(kThreads), 0, st, tp);
        zw_next = BW0;
      }
    } else {  // the flush: updates p0 .. k-1 go into the stored matrix
      if (tp.nb == 1) hipLaunchKernelGGL(k_sb_sweep_lo<1>, grid, dim3(kThreads), 0, st, tp);
      else hipLaunchKernelGGL(k_sb_sweep_lo<kSbNB>, grid, dim3(kThreads), 0, st, tp);
      tp.p0 = k;
    }
  }
  tp.j = K;
  tp.zfull = zfull_next;
  tp.zw = zw_next;
  if (tp.p0 < K - 1) hipLaunchKernelGGL(k_sb_pend, dim3(nmat), dim3(kThreads), 0, st, tp);
  panel();
}
void sb_chase(const dmm_ctx* ctx, const TdParams& tp, int nmat, hipStream_t st, int cap_hint = 0) {
  const int grid = nmat;
  const int n = tp.d.Np;
  auto lds_of = [&](int order) { return sb_chase_lds(order); };
  // The rank stop leaves the matrices of a telescope at a fraction of their order, and which fraction is known from the
  // chunks before (ctx->ml_order_hist).  A launch sized for the largest order seen so far plus 64 columns (the orders
  // drift with frequency and m, a few columns from one chunk to the next) takes (and keeps) half a CU's LDS or less --
  // its blocks start beside the next chunk's sweep / Gram blocks instead of waiting for a CU whose LDS is empty --; a
  // matrix above that goes through a second, small persistent launch with the full image.
  int cap = n;
  if (tp.stop_tol > 0.0 && ctx->opt_ml_chase_split != 1 && cap_hint > 0) {
    cap = std::max(cap_hint, 128);  // the chunk's own tiles were decomposed before (dmm_plan::ml_ne): their largest order + 64
  } else if (tp.stop_tol > 0.0 && ctx->opt_ml_chase_split != 1) {
    int64_t total = 0;
    int top = 0;
    for (int b = 0; b < 17; ++b) {
      total += ctx->ml_order_hist[b];
      if (ctx->ml_order_hist[b]) top = b;
    }
    if (total >= 64) cap = std::max(64 * (top + 1), 128);
  }
  if (cap + 64 >= n) {
    hipLaunchKernelGGL(k_sb_chase, dim3(grid), dim3(64 * kSbCW), lds_of(n), st, tp, nmat, 0, n);
    return;
  }
  hipLaunchKernelGGL(k_sb_chase, dim3(grid), dim3(64 * kSbCW), lds_of(cap), st, tp, nmat, 0, cap);
  hipLaunchKernelGGL(k_sb_chase, dim3(std::min(nmat, 64)), dim3(64 * kSbCW), lds_of(n), st, tp, nmat, cap, n);
}

// QL, the cut and the back-transformation of the reduced matrices: x into wbuf (telescope side) or alm (sky side)
void td_solve(const TdParams& tp, int nmat, hipStream_t st) {
  const size_t n = tp.d.Np;
  // three launches: the long serial QL phase runs as ONE 64-thread wave per matrix (see k_td_solve)
  hipLaunchKernelGGL(k_td_solve<1>, dim3(nmat), dim3(kThreads), (n + (size_t)tp.d.lr_n) * sizeof(double2), st, tp);  // (basis route: + D v)
  hipLaunchKernelGGL(k_td_solve<2>, dim3(nmat), dim3(64), n * 2 * sizeof(double), st, tp);
  hipLaunchKernelGGL(k_td_solve<3>, dim3(nmat), dim3(kThreads), n * (sizeof(double2) + 2 * sizeof(double)), st, tp);
}

}  // namespace

namespace {

// ---------------------------------------------------------------- ML: basis route (resident beam bases)
// X = Sigma U^H D of every matrix of a chunk from its resident basis: row j = sigma_j conj(U[:, j]) (the slot's row j)
// times the day's d_row; rows from the tile's rank up to the chunk's order nr are zero.  Also the rank per matrix.
__global__ __launch_bounds__(kThreads) void k_basis_x(DenseParams p, const double2* U, const double* sigma, const int32_t* rank, const int* slots,
                                                     int rmax, double2* X, int64_t xstride, int nr, int* rank_out) {
  __shared__ double s_d[kSbRows * kThreads];
  const int mat = blockIdx.x, slot = slots[mat], n = p.N, r = rank[slot];
  const dmm_tile tile = p.tiles[p.tile0 + mat];
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int s = i >= p.npairs, pp = i - s * p.npairs;
    s_d[i] = sqrt(p.mweight[(((int64_t)tile.m * 2 + s) * p.nfreq + tile.f) * p.npairs + pp]);
  }
  if (threadIdx.x == 0) rank_out[mat] = r;
  __syncthreads();
  const double2* Us = U + (int64_t)slot * rmax * n;
  const double* sg = sigma + (int64_t)slot * rmax;
  double2* Xm = X + (int64_t)mat * xstride;
  for (int64_t e = threadIdx.x; e < (int64_t)nr * n; e += kThreads) {
    const int j = (int)(e / n), row = (int)(e - (int64_t)j * n);
    double2 v = make_double2(0.0, 0.0);
    if (j < r) {
      const double2 u = Us[(int64_t)j * n + row];
      const double f = sg[j] * s_d[row];
      v = make_double2(f * u.x, f * u.y);
    }
    Xm[e] = v;
  }
}

// ---------------------------------------------------------------- ML: certificate of "nothing cut"
// X[mat][k][i] = d_i conj(B[i][k]): the rows of (D B)^H, so that the NT tile product gives B^H Ni B
__global__ __launch_bounds__(kThreads) void k_xpose(DenseParams p, double2* X) {
  __shared__ double2 t[32][33];
  const int mat = blockIdx.z;
  const dmm_tile tile = p.tiles[p.tile0 + mat];
  const int L = p.lmax + 1 - tile.m, K = p.npol * L, ntel = 2 * p.npairs;
  const int k0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int pol_stride = p.full_layout ? p.lmax + 1 : L;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, k = k0 + tx;
    double2 v = make_double2(0.0, 0.0);
    if (i < ntel && k < K) {
      const int pol = k / L, lrel = k - pol * L;
      const int64_t off = tile.b_off + ((int64_t)i * p.npol + pol) * pol_stride + (p.full_layout ? tile.m : 0) + lrel;
      const int s = i >= p.npairs, pp = i - s * p.npairs;
      const double d = sqrt(p.mweight[(((int64_t)tile.m * 2 + s) * p.nfreq + tile.f) * p.npairs + pp]);
      const double2 b = load_bc(p.B, p.b_c128, off);
      v = make_double2(d * b.x, -d * b.y);
    }
    t[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, i = i0 + tx;
    if (k < K && i < ntel) X[((int64_t)mat * p.Np + k) * p.ldx + i] = t[tx][r];
  }
}

// theta[mat] = max_i sum_j |A_ij| >= lambda_max (A Hermitian, full storage); one block per matrix
__global__ __launch_bounds__(kThreads) void k_rowsum(DenseParams p) {
  __shared__ double red[kThreads / 64];
  const int mat = blockIdx.x, n = p.Np;
  const int N = order_of(p, p.tiles[p.tile0 + mat]);
  const double2* A = p.A + (int64_t)mat * n * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double best = 0.0;
  for (int i = wave; i < N; i += kThreads / 64) {
    double sum = 0.0;
    for (int j = lane; j < N; j += 64) {
      const double2 v = A[(int64_t)i * n + j];
      sum += sqrt(v.x * v.x + v.y * v.y);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    best = fmax(best, sum);
  }
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) m = fmax(m, red[w]);
    p.theta[mat] = m;
  }
}

// The same bound from the LOWER triangle alone (the Gram kernels write only that): sum_j |A_ij| = the row's own part
// plus the column part sum_{k>i} |A_ki|.  Wave w walks the rows w, w+4, ...; a lane only ever adds to the columns
// j = lane (mod 64) of its wave's private LDS array, so there are no atomics and the sums are formed in a fixed order.
// Dynamic LDS: 5 Np doubles (orders up to 1024 in 40 KB; larger ones mirror first and use k_rowsum).
__global__ __launch_bounds__(kThreads) void k_rowsum_lower(DenseParams p) {
  extern __shared__ __align__(16) unsigned char smem_rs[];
  double* col = reinterpret_cast<double*>(smem_rs);  // [4][n]
  const int mat = blockIdx.x, n = p.Np;
  double* rowpart = col + 4 * n;                      // [n]
  const int N = order_of(p, p.tiles[p.tile0 + mat]);
  const double2* A = p.A + (int64_t)mat * n * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < 5 * n; j += kThreads) col[j] = 0.0;
  __syncthreads();
  double* mine = col + wave * n;
  for (int i = wave; i < N; i += kThreads / 64) {
    double sum = 0.0;
    for (int j = lane; j <= i; j += 64) {
      const double2 v = A[(int64_t)i * n + j];
      const double a = sqrt(v.x * v.x + v.y * v.y);
      sum += a;
      if (j < i) mine[j] += a;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) rowpart[i] = sum;
  }
  __syncthreads();
  double best = 0.0;
  for (int i = threadIdx.x; i < N; i += kThreads) best = fmax(best, rowpart[i] + ((col[i] + col[n + i]) + (col[2 * n + i] + col[3 * n + i])));
  for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
  __syncthreads();
  if (lane == 0) col[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) p.theta[mat] = fmax(fmax(col[0], col[1]), fmax(col[2], col[3]));
}

// the diagonal of A itself prepared for a factorisation in place: zero modes and padding pinned as k_shift_copy does
__global__ void k_pin_diag(DenseParams p) {
  const int mat = blockIdx.y, n = p.Np;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int N = order_of(p, p.tiles[p.tile0 + mat]);
  double2* d = p.A + (int64_t)mat * n * n + (int64_t)i * n + i;
  const double th = p.theta[mat];
  if (i >= N || d->x == 0.0) *d = make_double2(th > 0.0 ? th : 1.0, 0.0);
  else d->y = 0.0;
}

// C = A - shift*I with the zero modes pinned: rows that are exactly zero (and the padding) get the
// diagonal theta.  shift = max(rcond2 * theta, acond2) when `shifted`, else 0.
// `lower`: only the lower triangle is copied (all a Cholesky factorisation reads).
__global__ __launch_bounds__(kThreads) void k_shift_copy(DenseParams p, double2* C, int shifted, double rcond2, double acond2, int lower = 0) {
  const int mat = blockIdx.y, n = p.Np;
  const int N = order_of(p, p.tiles[p.tile0 + mat]);
  const double2* A = p.A + (int64_t)mat * n * n;
  double2* dst = C + (int64_t)mat * n * n;
  const double th = p.theta[mat];
  const double pin = th > 0.0 ? th : 1.0;
  const double shift = shifted ? fmax(rcond2 * th, acond2) : 0.0;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (int64_t)n * n;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / n), j = (int)(idx % n);
    if (lower && j > i) continue;
    double2 v = A[idx];
    if (i == j) v = (i >= N || v.x == 0.0) ? make_double2(pin, 0.0) : make_double2(v.x - shift, 0.0);
    dst[idx] = v;
  }
}

// w = D U_r L_r^-1 U_r^H D v with the reference's cut on sigma = sqrt(lambda)
__global__ __launch_bounds__(kThreads) void k_ml_filter(JacobiParams jp) {
  extern __shared__ __align__(16) unsigned char smem[];
  const DenseParams& p = jp.d;
  const int n = p.Np;
  double2* b = reinterpret_cast<double2*>(smem);  // [n]  D v
  double2* c = b + n;                             // [n]  coefficients
  __shared__ double lam_max;
  const int mat = p.msel ? p.msel[blockIdx.x] : blockIdx.x;
  const dmm_tile tile = p.tiles[p.tile0 + mat];
  const double2* A = p.A + (int64_t)mat * n * n;
  const double2* V = jp.V + (int64_t)mat * n * n;
  const int Lsky = p.lmax + 1 - tile.m, N = order_of(p, tile);
  for (int i = threadIdx.x; i < n; i += kThreads) {
    double2 v = make_double2(0.0, 0.0);
    if (i < N) {
      if (p.sky) {
        const int pol = i / Lsky, lrel = i - pol * Lsky;
        v = p.alm[(((int64_t)tile.f * p.npol + pol) * p.n_m + tile.m) * (p.lmax + 1) + tile.m + lrel];
      } else {
        const int s = i >= p.npairs, pp = i - s * p.npairs;
        const int64_t o = (((int64_t)tile.m * 2 + s) * p.nfreq + tile.f) * p.npairs + pp;
        const double d = sqrt(p.mweight[o]);
        const double2 x = p.mvis[o];
        v = make_double2(d * x.x, d * x.y);
      }
    }
    b[i] = v;
  }
  if (threadIdx.x == 0) {
    double mx = 0.0;
    for (int i = 0; i < n; ++i) mx = fmax(mx, A[(int64_t)i * n + i].x);
    lam_max = mx;
  }
  __syncthreads();
  const double smax = sqrt(fmax(lam_max, 0.0));
  // c_k = (u_k^H b) / lambda_k for kept k.  Eigenvector k = column k of V.  Padded
  // coordinates (i >= N) never mix with the rest (their rows/cols are those of the identity).
  double cnt = 0.0, mnk = 1e300, mxc = 0.0;
  for (int k = threadIdx.x; k < n; k += kThreads) {
    const double lam = A[(int64_t)k * n + k].x;
    const double sig = sqrt(fmax(lam, 0.0));
    double2 acc = make_double2(0.0, 0.0);
    const bool keep = sig > jp.rcond * smax && sig > jp.acond;
    cnt += keep ? 1.0 : 0.0;
    mnk = keep ? fmin(mnk, sig) : mnk;
    mxc = keep ? mxc : fmax(mxc, sig);
    if (keep) {  // pinv_svd's rank rule, mapmaker.py:296
      for (int i = 0; i < n; ++i) {
        const double2 u = V[(int64_t)i * n + k], x = b[i];
        acc.x += u.x * x.x + u.y * x.y;
        acc.y += u.x * x.y - u.y * x.x;
      }
      acc.x /= lam;
      acc.y /= lam;
    }
    c[k] = acc;
  }
  if (p.diag) ml_diag_write(p, tile, cnt, mnk, mxc, smax);
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += kThreads) {
    double2 acc = make_double2(0.0, 0.0);
    for (int k = 0; k < n; ++k) {
      const double2 u = V[(int64_t)i * n + k], x = c[k];
      acc.x += u.x * x.x - u.y * x.y;
      acc.y += u.x * x.y + u.y * x.x;
    }
    if (p.sky) {
      const int pol = i / Lsky, lrel = i - pol * Lsky;
      p.alm[(((int64_t)tile.f * p.npol + pol) * p.n_m + tile.m) * (p.lmax + 1) + tile.m + lrel] = acc;
    } else {
      const int s = i >= p.npairs, pp = i - s * p.npairs;
      const double d = sqrt(p.mweight[(((int64_t)tile.m * 2 + s) * p.nfreq + tile.f) * p.npairs + pp]);
      p.wbuf[(int64_t)mat * p.N + i] = make_double2(d * acc.x, d * acc.y);
    }
  }
}

// ---- ML, null certificate.  pinv_svd keeps sigma > acond (mapmaker.py:296): a tile whose LARGEST singular value is at
// most acond keeps nothing and its solution is exactly zero.  sigma_max^2 <= trace(G) = sum_i Ni_i sum_j |B_ij|^2 (the
// squared Frobenius norm of D B), and that costs one pass over the tile -- no Gram matrix, no decomposition.  Beam
// transfers beyond the m a telescope's east-west extent can see are numerically empty; on the structured tiles of
// bench.py --maker ml that is every tile above m ~ 300, two fifths of the day's tiles.
// grid (ntile, kTraceSplit): a block sums the rows of its split, lanes along the contiguous packed row.
constexpr int kTraceSplit = 4;
__global__ __launch_bounds__(kThreads) void k_ml_trace(const dmm_tile* __restrict__ tiles, DenseParams p, double* __restrict__ trace,
                                                       const int32_t* __restrict__ list) {
  const dmm_tile tile = tiles[list[blockIdx.x]];  // (trace[blockIdx.x] belongs to tile list[blockIdx.x])
  const int L = p.lmax + 1 - tile.m;
  const int pol_stride = p.full_layout ? p.lmax + 1 : L;
  const int col0 = p.full_layout ? tile.m : 0;
  const int64_t row_stride = (int64_t)p.npol * pol_stride;
  const int ntel = 2 * p.npairs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = (int)((int64_t)ntel * blockIdx.y / kTraceSplit), r1 = (int)((int64_t)ntel * (blockIdx.y + 1) / kTraceSplit);
  double acc = 0.0;
  for (int i = r0 + wave; i < r1; i += kThreads / 64) {
    const int s = i >= p.npairs, pp = i - s * p.npairs;
    const double ni = p.mweight[(((int64_t)tile.m * 2 + s) * p.nfreq + tile.f) * p.npairs + pp];
    if (ni == 0.0) continue;  // (wave-uniform)
    double rs = 0.0;
    for (int pol = 0; pol < p.npol; ++pol) {
      const int64_t base = tile.b_off + (int64_t)i * row_stride + (int64_t)pol * pol_stride + col0;
#pragma unroll 4
      for (int l = lane; l < L; l += 64) {
        const double2 b = load_bc(p.B, p.b_c128, base + l);
        rs = fma(b.x, b.x, fma(b.y, b.y, rs));
      }
    }
    acc = fma(ni, rs, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ double part[kThreads / 64];
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(trace + blockIdx.x, (part[0] + part[1]) + (part[2] + part[3]));
}

// a_lm of the tiles in `list` := 0 (l >= m columns; the caller's array may hold anything)
__global__ __launch_bounds__(kThreads) void k_zero_alm_tiles(const dmm_tile* __restrict__ tiles, const int32_t* __restrict__ list, DenseParams p, double2* __restrict__ alm) {
  const dmm_tile tile = tiles[list[blockIdx.x]];
  const int nl = p.lmax + 1;
  for (int idx = threadIdx.x; idx < p.npol * nl; idx += kThreads) {
    const int pol = idx / nl, l = idx - pol * nl;
    alm[(((int64_t)tile.f * p.npol + pol) * p.n_m + tile.m) * nl + l] = make_double2(0.0, 0.0);
  }
}

__global__ void k_prior(double* Sl, int lmax, double amp, double tilt) {
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l <= lmax; l += gridDim.x * blockDim.x) {
    const double dl = l == 0 ? 1.0 : (double)l;  // mapmaker.py:261: l[0] = 1
    Sl[l] = amp * amp * pow(dl, -tilt);
  }
}

// Wiener, sky side: C^-1 = diag(1 / S_l) + B^H Ni B (mapmaker.py:267-270); padded rows get a unit diagonal
// the prior per packed column of every m: Sk[m][k] = S_l(m + k mod L), L = lmax+1-m, zero beyond npol*L
__global__ void k_prior_expand(const double* Sl, double* Sk, int lmax, int npol, int pitch) {
  const int m = blockIdx.x, L = lmax + 1 - m, K = npol * L;
  for (int k = threadIdx.x; k < pitch; k += blockDim.x) Sk[(int64_t)m * pitch + k] = k < K ? Sl[m + k % L] : 0.0;
}

__global__ void k_add_prior_diag(DenseParams p, const double* Sl) {
  const int mat = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.Np) return;
  const dmm_tile tile = p.tiles[p.tile0 + mat];
  const int L = p.lmax + 1 - tile.m, N = p.npol * L;
  double2* d = p.A + ((int64_t)mat * p.Np + i) * p.Np + i;
  if (i < N) d->x += 1.0 / Sl[tile.m + i % L];
  else *d = make_double2(1.0, 0.0);
}

// ---------------------------------------------------------------- host: workspace and the pieces both makers share
namespace dl = dense_layout;  // sizes, batch capacity, carving, work ranges: dense_layout.h (plain integers, no HIP)
using dl::Layout;
static_assert(dl::kTB == TB && dl::kKC == KC && dl::kC128 == sizeof(double2) && dl::kTileRec == sizeof(dmm_tile), "dense_layout.h and dense_kernels.h disagree");

int64_t workspace_bytes(const dmm_plan* pl, int aux_slots) {
  if (!pl) return 0;
  const Layout L = dl::layout_of(pl->npairs, pl->npol, pl->lmax, aux_slots);
  const int64_t opt = aux_slots >= 2 ? pl->ctx->opt_ml_ws_mib : pl->ctx->opt_wiener_ws_mib;
  return dl::workspace_bytes(L, dl::batch_cap(L, aux_slots, pl->ntile, opt));
}

// The caller's workspace carved for either maker (aux_slots: 1 Wiener, 2 ML), as typed pointers, and the DenseParams
// every batch starts from.  L is the layout of the telescope-side order: the largest any batch uses.
struct DenseWs {
  Layout L;
  int cap;           // matrices in flight
  DenseParams base;  // A, Linv (= aux) and wbuf at matrix slot 0
  double2* aux;      // Wiener: X, the rows of (D B)^H (sky side).  ML, two matrices per slot: X, Cholesky copies, eigenvectors / logs
  double2* blocks;   // inverted diagonal blocks of the factorisations / pair rotations (Jacobi) / Householder vectors
  double *scale, *theta;
  dmm_tile* tiles;
  int32_t* work;  // dl::work_first
  int *flag, *slots, *fail, *msel, *any_rot;
};
DenseWs carve_ws(const dmm_plan* pl, int aux_slots, const void* B, const void* mvis, const double* mweight, void* workspace) {
  DenseWs w;
  w.L = dl::layout_of(pl->npairs, pl->npol, pl->lmax, aux_slots);
  w.cap = dl::batch_cap(w.L, aux_slots, pl->ntile, aux_slots >= 2 ? pl->ctx->opt_ml_ws_mib : pl->ctx->opt_wiener_ws_mib);
  const dl::Carve c = dl::carve(w.L, w.cap, aux_slots);
  unsigned char* ws = (unsigned char*)workspace;
  w.aux = (double2*)(ws + c.aux);
  w.blocks = (double2*)(ws + c.blocks);
  w.flag = (int*)(ws + c.flag);
  w.scale = (double*)(ws + c.scale);
  w.theta = (double*)(ws + c.theta);
  w.tiles = (dmm_tile*)(ws + c.tiles);
  w.work = (int32_t*)(ws + c.work);
  w.slots = (int*)(ws + c.slots);
  w.fail = (int*)(ws + c.fail);
  w.msel = (int*)(ws + c.msel);
  w.any_rot = (int*)(ws + c.any_rot);
  DenseParams& p = w.base = DenseParams{};  // (everything not named here: 0 / nullptr)
  p.tiles = pl->tiles_d;
  p.N = w.L.N;
  p.Np = w.L.Np;
  p.T = w.L.T;
  p.B = B;
  p.b_c128 = pl->b_dtype == DMM_C128;
  p.full_layout = pl->b_layout == DMM_B_FULL;
  p.gram_dma = pl->ctx->opt_gram_stage == 1;
  p.npairs = pl->npairs;
  p.npol = pl->npol;
  p.lmax = pl->lmax;
  p.nfreq = pl->nfreq;
  p.mvis = (const double2*)mvis;
  p.mweight = mweight;
  p.A = (double2*)(ws + c.A);
  p.Linv = w.aux;  // (the ML path reuses this region as V: sized accordingly)
  p.wbuf = (double2*)(ws + c.wbuf);
  p.n_m = pl->n_m;
  p.diag = pl->ctx->ml_diag;
  return w;
}

struct StreamRestore {  // a run that moves ctx->stream to the library's second stream leaves the caller's pointer behind
  dmm_ctx* c;
  hipStream_t s;
  ~StreamRestore() { c->stream = s; }
};

// The smaller Gram matrix of each tile that is not null (`is_null` empty: none is): telescope side (any m; "ml_shortcut"
// = 3: every tile) or sky side, by padded order -- the tiles of one padded order share batches
void partition_tiles(const dmm_plan* pl, const std::vector<char>& is_null, std::vector<int64_t>& tel_list, std::map<int, std::vector<int64_t>>& sky_lists) {
  const int ntel = 2 * pl->npairs;
  for (int64_t t = 0; t < pl->ntile; ++t) {
    if (!is_null.empty() && is_null[t]) continue;
    const int nsky = pl->npol * (pl->lmax + 1 - pl->tiles_h[t].m);
    if (nsky >= ntel || pl->ctx->opt_ml_shortcut == 3) tel_list.push_back(t);
    else sky_lists[(nsky + TB - 1) / TB * TB].push_back(t);
  }
}

std::vector<int64_t> concat(const std::map<int, std::vector<int64_t>>& lists) {
  std::vector<int64_t> all;
  for (auto& kv : lists) all.insert(all.end(), kv.second.begin(), kv.second.end());
  return all;
}

// resident beam Gram products and bases: slot of a telescope-side tile = its rank among them in plan order (-1: sky side)
std::vector<int32_t> gslot_table(const dmm_plan* pl) {
  std::vector<int32_t> gslot_of((size_t)pl->ntile, -1);
  int32_t s = 0;
  for (int64_t t = 0; t < pl->ntile; ++t)
    if (pl->npol * (pl->lmax + 1 - pl->tiles_h[t].m) >= 2 * pl->npairs) gslot_of[(size_t)t] = s++;
  return gslot_of;
}

// DenseParams of a batch of nmat matrices in the matrix slots from `off` on, its tiles at tiles_d + off.  Sky side: the
// matrices share the padded order of np_sky, the order of each one comes from its tile (order_of)
DenseParams batch_params(const DenseWs& W, size_t off, int nmat, bool sky, int np_sky, void* alm) {
  DenseParams p = W.base;
  p.A = W.base.A + off * W.L.Np * W.L.Np;
  p.wbuf = W.base.wbuf + off * W.L.N;
  p.tiles = W.tiles + off;
  p.tile0 = 0;
  p.nmat = nmat;
  p.sky = sky ? 1 : 0;
  p.N = sky ? np_sky : W.L.N;
  p.Np = (p.N + TB - 1) / TB * TB;
  p.T = p.Np / TB;
  p.alm = (double2*)alm;
  return p;
}

// the batch's tiles and the column-block prefix of its back-projection -> device, on S (the host vectors must outlive the copies)
int upload_lists(dmm_plan* pl, const int64_t* ids, int nmat, std::vector<dmm_tile>& tiles_c, std::vector<int32_t>& work_c, dmm_tile* tiles_d,
                 int32_t* work_d, hipStream_t S) {
  dmm_dirty_tile_list(pl, ids, nmat, tiles_c, work_c);
  DMM_HIP(hipMemcpyAsync(tiles_d, tiles_c.data(), nmat * sizeof(dmm_tile), hipMemcpyHostToDevice, S));
  DMM_HIP(hipMemcpyAsync(work_d, work_c.data(), (nmat + 1) * sizeof(int32_t), hipMemcpyHostToDevice, S));
  return DMM_OK;
}
// ... and the slots of its resident products / bases
int upload_slots(const std::vector<int32_t>& gslot_of, const int64_t* ids, int nmat, std::vector<int>& slots_c, int* slots_d, hipStream_t S) {
  slots_c.resize(nmat);
  for (int i = 0; i < nmat; ++i) slots_c[i] = gslot_of[(size_t)ids[i]];
  DMM_HIP(hipMemcpyAsync(slots_d, slots_c.data(), nmat * sizeof(int), hipMemcpyHostToDevice, S));
  return DMM_OK;
}

// Gram matrices of a batch on S: lower triangle and the diagonal tiles in full.
//   sky side (p.sky):  X = the rows of (D B)^H (k_xpose), G = X X^H
//   telescope side:    G = [I +] D B [S] B^H D; with `slots` (resident beam Gram products, dmm_ctx_set_ml_gram_cache) the Gram
//                      kernel skips the matrices whose product is resident, k_gram_scale forms those from the slot.  Both
//                      kernels always: which matrices each of them takes is decided by the DEVICE flags -- the host's mirror
//                      of them only feeds the counters, and may lag when a caller alternates between caches.
// count_tiles (ML; nullptr: Wiener): the batch's tiles, for bench.py's roofline -- useful flops of the products computed,
// a Gram matrix formed from a resident product counts none.
void form_gram(dmm_ctx* ctx, DenseParams& p, int nmat, hipStream_t S, double2* X, const std::vector<int>* slots, const int* slots_d,
               const dmm_tile* count_tiles) {
  const int ntel = 2 * p.npairs, T = p.T;
  auto flops = [&](const dmm_tile& t) {
    const double nsky = (double)p.npol * (p.lmax + 1 - t.m);
    const double k = std::min<double>(ntel, nsky), K = std::max<double>(ntel, nsky);
    return (int64_t)(4.0 * k * k * K);
  };
  for (int i = 0; count_tiles && i < nmat; ++i) ctx->ml_gram_flops += flops(count_tiles[i]);
  if (p.sky) {
    p.ldx = ntel;
    p.X = X;
    hipLaunchKernelGGL(k_xpose, dim3((p.N + 31) / 32, (ntel + 31) / 32, nmat), dim3(kThreads), 0, S, p, X);
    hipLaunchKernelGGL(k_nt<MODE_GRAMX>, dim3(T * (T + 1) / 2, nmat), dim3(kThreads), 0, S, p);
  } else if (slots) {
    for (int i = 0; i < nmat; ++i)
      if ((*slots)[i] >= 0 && ctx->ml_gvalid_h[(size_t)(*slots)[i]]) {
        ++ctx->ml_gram_cached;
        if (count_tiles) ctx->ml_gram_flops -= flops(count_tiles[i]);
      }
    p.gcache = ctx->ml_gcache;
    p.gslot = slots_d;
    p.gvalid = ctx->ml_gvalid;
    hipLaunchKernelGGL(k_nt<MODE_GRAM>, dim3(T * (T + 1) / 2, nmat), dim3(kThreads), 0, S, p);
    hipLaunchKernelGGL(k_gram_scale, dim3(T * (T + 1) / 2, nmat), dim3(kThreads), 0, S, p);
    hipLaunchKernelGGL(k_gram_mark, dim3((nmat + 255) / 256), dim3(256), 0, S, slots_d, ctx->ml_gvalid, nmat);
    for (int i = 0; i < nmat; ++i)
      if ((*slots)[i] >= 0) ctx->ml_gvalid_h[(size_t)(*slots)[i]] = 1;
    p.gcache = nullptr;  // (nothing downstream looks at the cache)
  } else {
    launch_gram(p, nmat, S);
  }
}

// left-looking tile Cholesky of p.A in place, the inverted diagonal blocks into p.Linv; solve_lds > 0: and the solve, in the same span
constexpr size_t kDiagLds = (size_t)TB * (TB + 1) * sizeof(double2);
size_t solve_lds(const Layout& L) { return ((size_t)L.Np + TB + 4 * TB) * sizeof(double2); }
void chol_factor(dmm_ctx* ctx, DenseParams& p, int nmat, hipStream_t S, size_t solve_lds = 0) {
  dmm_prof_scope prof(ctx, DMM_PROF_CHOL, S);
  const int T = p.T;
  for (int J = 0; J < T; ++J) {
    p.J = J;
    if (J > 0) hipLaunchKernelGGL(k_nt<MODE_UPDATE>, dim3(T - J, nmat), dim3(kThreads), 0, S, p);
    hipLaunchKernelGGL(k_chol_diag, dim3(nmat), dim3(kThreads), kDiagLds, S, p);
    if (J < T - 1) hipLaunchKernelGGL(k_nt<MODE_PANEL>, dim3(T - J - 1, nmat), dim3(kThreads), 0, S, p);
  }
  if (solve_lds) hipLaunchKernelGGL(k_chol_solve, dim3(nmat), dim3(kThreads), solve_lds, S, p);  // sky: a_lm in place
}
int chol_attributes(const Layout& L) {
  DMM_HIP(hipFuncSetAttribute((const void*)k_chol_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds(L)));
  DMM_HIP(hipFuncSetAttribute((const void*)k_chol_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDiagLds));
  return DMM_OK;
}

// B^H Ni v of the sky-side tiles only -- the right-hand sides of their systems (the telescope-side tiles, most of the
// bytes of B, get their a_lm from the back-projection): lists of at most W.cap tiles through the device arrays of a
// batch at slot 0
int sky_rhs(dmm_plan* pl, const void* B, const void* mvis, const double* mweight, void* alm,
            const std::map<int, std::vector<int64_t>>& sky_lists, const DenseWs& W) {
  const std::vector<int64_t> all = concat(sky_lists);
  std::vector<dmm_tile> tiles_c;
  std::vector<int32_t> work_c;
  hipStream_t st = pl->ctx->stream;
  for (size_t i0 = 0; i0 < all.size(); i0 += W.cap) {
    const int nmat = (int)std::min<size_t>(W.cap, all.size() - i0);
    DMM_TRY(upload_lists(pl, all.data() + i0, nmat, tiles_c, work_c, W.tiles, W.work, st));
    DMM_HIP(hipStreamSynchronize(st));  // the host vectors are reused
    DMM_TRY(dmm_dirty_launch_list(pl, B, mvis, mweight, W.tiles, W.work, nmat, work_c[nmat], alm));
    DMM_HIP(hipStreamSynchronize(st));  // the device lists are rewritten by the next list and by the batches
  }
  return DMM_OK;
}

// ---------------------------------------------------------------- host: the ML pass
// The eigen path's launch parameters for the matrices of p (order p.Np) with their vectors in `vec` and their log regions
// (two matrices of the telescope order each) in `log`.  The last four arguments are where the synchronous batch and the
// pipelined chunk differ: the selection list (the chunk decomposes all its matrices), upper-triangle trailing updates and
// the two-stage reduction ("ml_eigen" = 2 switches both off, in the synchronous batch only), and the rank stop's tolerance
// (a basis build, always pipelined, has its own).
TdParams td_params(const dmm_ctx* ctx, const DenseParams& p, const Layout& L, double2* vec, double2* log, int* fail, double acond, double rcond,
                   const int* msel, int tri, int two_stage, double stop_tol) {
  const int n = p.Np;
  TdParams tp;
  tp.d = p;
  tp.d.msel = msel;
  tp.vec = vec;
  tp.log_cs = log;
  tp.log_stride = (int64_t)2 * L.Np * L.Np;
  const int runs = 16 * n;  // a chase per QL iteration: ~1.7 n in practice
  tp.run_cap = ctx->opt_ml_eigen == 3 ? -runs : runs;  // negative: every other matrix is made to give up (tests)
  tp.log_cap = (int)std::min<int64_t>(tp.log_stride - ((int64_t)3 * runs * sizeof(int) + 15) / 16, 0x7fffffff);
  tp.acond = acond;
  tp.rcond = rcond;
  tp.fail = fail;
  tp.tri = tri;
  tp.two_stage = two_stage;
  tp.nb = sb_pending(ctx, n, tp.log_stride);
  tp.one_block = ctx->opt_ml_reduce == 3 ? 1 : 0;  // ("ml_reduce" = 3: every reading sweep as one block per matrix: herm_band.h)
  tp.fused = ctx->opt_ml_reduce == 5 ? 1 : 0;
  tp.stop_tol = stop_tol;
  tp.bs_U = nullptr;
  if (tp.two_stage) tp.log_cap = (int)std::min<int64_t>(sb_log_cap(tp.log_stride, n, runs), 0x7fffffff);
  return tp;
}

// Sky-side lists go through the eigen pass one padded order at a time, and every order pays a latency-bound launch
// chain (~0.08 ms per Householder column whatever the batch) that a few hundred matrices do not fill: short lists
// of NEIGHBOURING orders are decomposed together at the larger one (order_of() keeps each tile's own size, the
// padding is zeros).  At cfg 3 / 16 frequencies: eleven chains of 4224 columns become six of 2304.
void pair_orders(std::map<int, std::vector<int64_t>>& lists) {
  std::map<int, std::vector<int64_t>> out;
  for (auto it = lists.rbegin(); it != lists.rend(); ++it) {
    auto nx = std::next(it);
    if (nx != lists.rend() && it->second.size() < 600 && nx->second.size() < 600 && it->first - nx->first <= TB) {
      std::vector<int64_t>& d = out[it->first];
      d = it->second;
      d.insert(d.end(), nx->second.begin(), nx->second.end());
      it = nx;
    } else {
      out[it->first] = it->second;
    }
  }
  lists.swap(out);
}

constexpr size_t kSubLds = (size_t)2 * TB * (TB + 1) * sizeof(double2);

// One call of dmm_ml_run: its arguments, the carved workspace and everything the steps of the pass (file head) hand to each other
struct MlPass {
  dmm_plan* pl;
  dmm_ctx* ctx;
  const void* B;
  void* alm;
  double acond, rcond;
  DenseWs W;
  int ntel, cap, capE, E, cap_direct;  // telescope order; matrices in flight: all, per half, per early slot, in the direct batches
  // resident beam bases (dmm_ctx_set_ml_basis): build = this call decomposes B B^H of the telescope-side tiles and leaves the
  // bases; resident Gram products; the certificate ("ml_shortcut" = 2: always take the eigen path (tests, timing))
  bool bs_build, bs_use, gcache_on, shortcut;
  std::vector<int32_t> gslot_of;  // gslot_table, if anything resident is in use
  // host sides of the synchronous batches' lists (one batch at a time: reused)
  std::vector<dmm_tile> tiles_c;
  std::vector<int32_t> work_c;
  std::vector<int> fail_h, msel_h, td_fail_h;
  // tiles whose certificate failed, collected over all batches so that the (launch-latency bound) eigen path runs on well
  // filled batches at the end
  std::vector<int64_t> tel_deferred;
  std::map<int, std::vector<int64_t>> sky_deferred;

  // ---- pipelined eigen pass (tridiagonal path).  The workspace is used as two chunk slots: while the serial QL chases of
  // one chunk run on the library's second stream (one wave per matrix, a latency floor that leaves the GPU empty), the
  // Gram matrices and the HBM-bound reduction of the next chunk run on the caller's stream.
  // Where chunk slot h starts and how many matrices it holds: normally the two halves of the workspace; while direct
  // (certificate) batches are still running, the chunks of early-known rejects use two small slots of E matrices at the
  // END of the workspace instead and the batches keep the front, [0, cap_direct) (dmm_ml_run sets and resets it).
  enum SlotLayout { kHalves, kEarlySlots } slot_layout = kHalves;
  int slot_off(int h) const { return slot_layout == kEarlySlots ? cap_direct + h * E : h * capE; }
  int slot_cap(int h) const { return slot_layout == kEarlySlots ? E : capE; }
  struct Half {
    std::vector<dmm_tile> tiles;
    std::vector<int32_t> work;
    std::vector<int64_t> ids;
    std::vector<int> slots;
    int nmat = 0, off = 0, np = 0, np_sky = 0;
    bool sky = false, busy = false;
  } half[2];
  int chunk_no = 0;
  bool early_used[2] = {false, false};
  // matrices whose QL gave up (counted: "ml_tiles_ql_failed"), for drain
  std::vector<int64_t> redo_tel;
  std::map<int, std::vector<int64_t>> redo_sky;
  int batch_no = 0;  // certificate batches so far (certify)

  MlPass(dmm_plan* pl_, const void* B_, const void* mvis, const double* mweight, double acond_, double rcond_, void* workspace, void* alm_)
      : pl(pl_), ctx(pl_->ctx), B(B_), alm(alm_), acond(acond_), rcond(rcond_), W(carve_ws(pl_, 2, B_, mvis, mweight, workspace)) {
    ntel = W.L.N;
    cap = W.cap;
    const bool bs_have = ctx->ml_bs_U != nullptr && ctx->opt_ml_shortcut != 3 && ctx->opt_ml_reduce == 0 && sb_stop_tol(ctx) > 0.0 &&
                         sb_usable(ctx, W.L.Np) && dmm_ml_gram_cache_slots(pl) <= ctx->ml_bs_slots;
    bs_build = bs_have && ctx->ml_bs_build;
    bs_use = bs_have && !ctx->ml_bs_build && (int64_t)ctx->ml_bs_rank_h.size() >= dmm_ml_gram_cache_slots(pl);
    gcache_on = !bs_build && ctx->ml_gcache && ctx->opt_gram_stage != 1 && ctx->opt_ml_shortcut != 3 && dmm_ml_gram_cache_slots(pl) <= ctx->ml_gslots;
    shortcut = ctx->opt_ml_shortcut != 2 && !bs_build;
    capE = cap / 2;
    E = std::min(128, cap / 8);
    cap_direct = E >= 8 ? cap - 2 * E : cap;  // (a workspace too small for early slots: every batch may use all of it)
  }

  // ---- bookkeeping for bench.py's rooflines: algorithmic bytes of a stage-1 reduction (the Gram flops: form_gram)
  // algorithmic bytes of stage 1's sweeps (herm_band.h): 4.5 KB per tile of a reading sweep, 8.5 KB of a flush
  double sweep_bytes(int n, int k) const {
    const int nb = sb_pending(ctx, n, (int64_t)2 * W.L.Np * W.L.Np);
    const double t = (n - ((8 * (k + 1)) & ~15)) / 16;
    return t * (t + 1) / 2 * (k > 0 && k % nb == 0 ? 8.5 : 4.5) * 1024;
  }
  void count_band(int n, int nmat) {
    double by = 0.0;
    for (int k = 0; k < n / 8 - 1; ++k) by += sweep_bytes(n, k);
    ctx->ml_band_bytes += (int64_t)(by * nmat);
  }
  // a matrix the rank stop cut off at order ne: the sweeps from panel ne / 8 - 1 on did not run; counted as stopped
  void count_stop(int n, int ne) {
    ++ctx->ml_order_hist[std::min(((ne ? ne : n) + 63) / 64, 16)];
    if (!ne) return;
    double by = 0.0;
    for (int k = ne / 8 - 1; k < n / 8 - 1; ++k) by += sweep_bytes(n, k);
    ctx->ml_band_bytes -= (int64_t)by;
    ++ctx->ml_tiles_stopped;
    ctx->ml_stop_cols += ne;
  }

  // reduction to tridiagonal form on S: stage 1 of two (the bulge chase is the caller's), or the one-stage Householder form
  void reduce(TdParams& tp, int nmat, hipStream_t S) {
    dmm_prof_scope prof(ctx, tp.two_stage ? DMM_PROF_BAND : DMM_PROF_TRIDIAG, S);
    if (tp.two_stage) count_band(tp.d.Np, nmat), sb_reduce(tp, nmat, S);
    else td_reduce(tp, nmat, S);
  }

  // Null certificate (k_ml_trace): tiles whose Frobenius norm says that EVERY singular value is at or below acond keep
  // nothing under pinv_svd's rule -- their a_lm is zero and they never see a Gram matrix.  Which tiles are worth the pass
  // is found on a SAMPLE first: a telescope sees the sky up to some m, so per frequency every 16th m is tried from the top
  // down (6 % of the bytes of B), and only the tiles above the highest sampled m that is NOT null are then checked one by
  // one (a tile is never called null unseen; a null tile below that m is simply decomposed like any other).  The scratch
  // is the workspace header (the prior tables of the Wiener solve: unused here).  "ml_null" = 1 switches it off.
  int null_certificate(void* workspace, std::vector<char>& is_null) {
    if (ctx->opt_ml_null == 1 || bs_build || !(acond > 0.0) || (size_t)pl->ntile * (sizeof(double) + sizeof(int32_t)) > W.L.header) return DMM_OK;
    double* const trace_d = (double*)workspace;
    int32_t* const list_d = (int32_t*)(trace_d + pl->ntile);
    // (the sum is exact to a few ulp; the margin keeps a tile AT the threshold on the decomposing side, where the cut
    // is decided on the eigenvalues themselves)
    const double lim = acond * acond * (1.0 - 1e-9);
    std::vector<double> trace_h;
    auto traces = [&](const std::vector<int32_t>& list) -> int {  // trace_h[i] = trace of tile list[i]
      if (list.empty()) return DMM_OK;
      DMM_HIP(hipMemcpyAsync(list_d, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
      DMM_HIP(hipMemsetAsync(trace_d, 0, list.size() * sizeof(double), ctx->stream));
      {
        dmm_prof_scope prof(ctx, DMM_PROF_NULL, ctx->stream);
        hipLaunchKernelGGL(k_ml_trace, dim3((unsigned)list.size(), kTraceSplit), dim3(kThreads), 0, ctx->stream, pl->tiles_d, W.base, trace_d,
                           (const int32_t*)list_d);
      }
      DMM_HIP(hipGetLastError());
      trace_h.resize(list.size());
      DMM_HIP(hipMemcpyAsync(trace_h.data(), trace_d, list.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      DMM_HIP(hipStreamSynchronize(ctx->stream));  // (also: `list` may die now)
      return DMM_OK;
    };
    const int step = ctx->opt_ml_null == 2 ? 1 : 16;  // ("ml_null" = 2: every tile, the A/B)
    // per frequency: the tiles sorted by m
    std::map<int, std::vector<std::pair<int, int32_t>>> by_f;
    for (int64_t t = 0; t < pl->ntile; ++t) by_f[pl->tiles_h[t].f].push_back({pl->tiles_h[t].m, (int32_t)t});
    std::vector<int32_t> sample;
    for (auto& kv : by_f) {
      std::sort(kv.second.begin(), kv.second.end());
      for (int64_t i = (int64_t)kv.second.size() - 1; i >= 0; i -= step) sample.push_back(kv.second[i].second);
    }
    DMM_TRY(traces(sample));
    std::map<int32_t, double> seen;
    for (size_t i = 0; i < sample.size(); ++i) seen[sample[i]] = trace_h[i];
    std::vector<int32_t> rest;
    for (auto& kv : by_f) {
      // from the top: the sampled tiles are null down to (excluding) position `stop`; everything above it is a candidate
      int64_t stop = -1;
      for (int64_t i = (int64_t)kv.second.size() - 1; i >= 0; i -= step)
        if (!(seen[kv.second[i].second] <= lim)) {
          stop = i;
          break;
        }
      for (int64_t i = stop + 1; i < (int64_t)kv.second.size(); ++i)
        if (!seen.count(kv.second[i].second)) rest.push_back(kv.second[i].second);
    }
    DMM_TRY(traces(rest));
    for (size_t i = 0; i < rest.size(); ++i) seen[rest[i]] = trace_h[i];
    std::vector<int32_t> null_h;
    for (auto& sv : seen)
      if (sv.second <= lim) {
        is_null[sv.first] = 1;
        null_h.push_back(sv.first);
      }
    if (!null_h.empty()) {
      DMM_HIP(hipMemcpyAsync(list_d, null_h.data(), null_h.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(k_zero_alm_tiles, dim3((unsigned)null_h.size()), dim3(kThreads), 0, ctx->stream, pl->tiles_d, list_d, W.base, (double2*)alm);
      DMM_HIP(hipGetLastError());
      DMM_HIP(hipStreamSynchronize(ctx->stream));  // null_h dies with this block
      ctx->ml_tiles_null += (int64_t)null_h.size();
    }
    return DMM_OK;
  }

  // ---- synchronous batches: nothing of the pipeline is in flight, the matrix slots from 0 on, the caller's stream
  // the batch's parameters, its lists on the device
  int begin_batch(const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky, DenseParams& p) {
    p = batch_params(W, 0, nmat, sky, np_sky, alm);
    p.theta = W.theta;
    DMM_TRY(upload_lists(pl, list.data() + i0, nmat, tiles_c, work_c, W.tiles, W.work + dl::work_first(0, dl::kBatch), ctx->stream));
    DMM_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors are reused by the next batch
    return DMM_OK;
  }
  // telescope side: a = B^H w of the batch's tiles
  int end_batch(const DenseParams& p) {
    if (p.sky) return DMM_OK;
    dmm_prof_scope prof(ctx, DMM_PROF_BACKPROJ, ctx->stream);
    DMM_TRY(dmm_dirty_w_launch_list(pl, B, p.wbuf, nullptr, W.tiles, W.work + dl::work_first(0, dl::kBatch), p.nmat, work_c[p.nmat], alm));
    DMM_HIP(hipStreamSynchronize(ctx->stream));  // the device lists are rewritten by the next batch
    return DMM_OK;
  }

  // Certificate batch: G - tau I positive definite  <=>  no mode is cut (file head).  Certified tiles are solved with G
  // itself; the rejects are deferred (they get their Gram matrix again in the deferred pass), so nothing after the
  // factorisations reads A: the upper triangle is never built here, the row sums come from the lower one and the second
  // factorisation runs in place (k_mirror + 1.5 matrix copies per batch less: 8 % of the pass).
  int cert_batch(const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky) {
    hipStream_t S = ctx->stream;
    DenseParams p;
    DMM_TRY(begin_batch(list, i0, nmat, sky, np_sky, p));
    const size_t rs_lds = (size_t)5 * p.Np * sizeof(double);
    const bool lower_only = rs_lds <= 40 * 1024;
    {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S);
      form_gram(ctx, p, nmat, S, W.aux, nullptr, nullptr, tiles_c.data());
      if (!lower_only) hipLaunchKernelGGL(k_mirror, dim3(64, nmat), dim3(kThreads), 0, S, p);
    }
    DMM_HIP(hipGetLastError());
    if (lower_only) hipLaunchKernelGGL(k_rowsum_lower, dim3(nmat), dim3(kThreads), rs_lds, S, p);
    else hipLaunchKernelGGL(k_rowsum, dim3(nmat), dim3(kThreads), 0, S, p);
    DMM_HIP(hipMemsetAsync(W.fail, 0, nmat * sizeof(int), S));
    DenseParams pc = p;  // the certificate's factorisation runs on a copy, the solve's in A itself
    pc.A = W.aux;
    pc.Linv = W.blocks;
    pc.fail = W.fail;
    hipLaunchKernelGGL(k_shift_copy, dim3(64, nmat), dim3(kThreads), 0, S, p, W.aux, 1, rcond * rcond, acond * acond, 1);
    chol_factor(ctx, pc, nmat, S);
    // solve with G itself (certified tiles only write their result)
    hipLaunchKernelGGL(k_pin_diag, dim3((p.Np + 255) / 256, nmat), dim3(256), 0, S, p);
    pc.A = p.A;
    chol_factor(ctx, pc, nmat, S);
    {
      dmm_prof_scope prof(ctx, DMM_PROF_CHOL, S);
      hipLaunchKernelGGL(k_chol_solve, dim3(nmat), dim3(kThreads), solve_lds(W.L), S, pc);
    }
    DMM_HIP(hipGetLastError());
    fail_h.assign(nmat, 1);
    DMM_HIP(hipMemcpyAsync(fail_h.data(), W.fail, nmat * sizeof(int), hipMemcpyDeviceToHost, S));
    DMM_HIP(hipStreamSynchronize(S));
    int nrej = 0;
    for (int i = 0; i < nmat; ++i)
      if (fail_h[i]) (sky ? sky_deferred[np_sky] : tel_deferred).push_back(list[i0 + i]), ++nrej;  // (their wbuf / alm entries are rewritten by the deferred pass)
    ctx->ml_tiles_direct += nmat - nrej;
    return end_batch(p);
  }

  // Blocked Jacobi eigen-decomposition of the nsel matrices of p that W.msel selects, then the reference's cut (k_ml_filter)
  int jacobi(const DenseParams& p, int nsel) {
    hipStream_t S = ctx->stream;
    const int max_sweeps = ctx->opt_ml_outer_sweeps > 0 ? ctx->opt_ml_outer_sweeps : 60;
    const int inner_sweeps = ctx->opt_ml_inner_sweeps > 0 ? ctx->opt_ml_inner_sweeps : 1;  // tools/ml_tune.py
    JacobiParams jp;
    jp.d = p;
    jp.d.msel = W.msel;
    jp.V = W.aux;
    jp.acond = acond;
    jp.rcond = rcond;
    jp.max_sweeps = max_sweeps;
    BjParams bp = {};  // (round, target: 0)
    bp.d = jp.d;
    bp.V = W.aux;
    bp.Wh = W.blocks;
    bp.flag = W.flag;
    bp.scale = W.scale;
    bp.any_rot = W.any_rot;
    bp.inner_sweeps = inner_sweeps;
    bp.nb = p.Np / JB;
    const int npr = bp.nb / 2, T = p.T;
    hipLaunchKernelGGL(k_bj_init, dim3(64, nsel), dim3(kThreads), 0, S, bp);
    for (int sweep = 0; sweep < max_sweeps && bp.nb > 1; ++sweep) {
      DMM_HIP(hipMemsetAsync(W.any_rot, 0, sizeof(int), S));
      for (int round = 0; round < bp.nb - 1; ++round) {
        bp.round = round;
        hipLaunchKernelGGL(k_bj_sub, dim3(npr, nsel), dim3(kSubThreads), kSubLds, S, bp);
        bp.target = 0;
        hipLaunchKernelGGL(k_bj_apply, dim3(T, npr, nsel), dim3(kThreads), 0, S, bp);
        bp.target = 2;
        hipLaunchKernelGGL(k_bj_apply, dim3(T, npr, nsel), dim3(kThreads), 0, S, bp);
        bp.target = 1;
        hipLaunchKernelGGL(k_bj_apply, dim3(T, npr, nsel), dim3(kThreads), 0, S, bp);
      }
      // converged when a whole sweep found every pair diagonal to working precision
      int any = 1;
      DMM_HIP(hipMemcpyAsync(&any, W.any_rot, sizeof(int), hipMemcpyDeviceToHost, S));
      DMM_HIP(hipStreamSynchronize(S));
      if (!any) break;
      if (sweep == max_sweeps - 1) return dmm_set_error(DMM_E_STATE, "dmm_ml_run: Jacobi did not converge in %d sweeps", max_sweeps);
    }
    hipLaunchKernelGGL(k_ml_filter, dim3(nsel), dim3(kThreads), (size_t)2 * W.L.Np * sizeof(double2), S, jp);
    DMM_HIP(hipGetLastError());
    return DMM_OK;
  }

  // Synchronous eigen batch: every matrix of the batch decomposed, the reference's cut applied.  jacobi_only: the blocked
  // Jacobi whatever "ml_eigen" says (drain: these matrices' QL has given up once already).
  int eigen_batch(const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky, bool jacobi_only) {
    hipStream_t S = ctx->stream;
    DenseParams p;
    DMM_TRY(begin_batch(list, i0, nmat, sky, np_sky, p));
    auto gram = [&]() {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S);
      form_gram(ctx, p, nmat, S, W.aux, nullptr, nullptr, tiles_c.data());
      hipLaunchKernelGGL(k_mirror, dim3(64, nmat), dim3(kThreads), 0, S, p);
    };
    gram();
    DMM_HIP(hipGetLastError());
    ctx->ml_tiles_eigen += nmat;
    msel_h.resize(nmat);
    for (int i = 0; i < nmat; ++i) msel_h[i] = i;
    int nsel = nmat;
    DMM_HIP(hipMemcpyAsync(W.msel, msel_h.data(), nsel * sizeof(int), hipMemcpyHostToDevice, S));
    DMM_HIP(hipStreamSynchronize(S));
    // tridiagonalisation + QL in factored form (herm_tridiag.h) has a latency floor per launch (the serial QL
    // chases, ~0.12 s at order 768, ~ n^2); a handful of matrices is through the blocked Jacobi sooner
    const int eig = ctx->opt_ml_eigen;
    const bool use_td = !jacobi_only && (eig == 0 ? (double)nsel * p.Np >= 12000.0 : eig != 1);
    if (use_td) {
      const int n = p.Np;
      // ("ml_eigen" = 2: full-matrix trailing updates, one stage)
      TdParams tp = td_params(ctx, p, W.L, W.blocks, W.aux, W.fail, acond, rcond, W.msel, (n <= 2048 && eig != 2) ? 1 : 0,
                              (eig != 2 && sb_usable(ctx, n)) ? 1 : 0, sb_stop_tol(ctx));
      DMM_HIP(hipMemsetAsync(W.fail, 0, nsel * sizeof(int), S));
      reduce(tp, nsel, S);
      if (tp.two_stage) {
        dmm_prof_scope prof(ctx, DMM_PROF_CHASE, S);
        sb_chase(ctx, tp, nsel, S);
      }
      {
        dmm_prof_scope prof(ctx, DMM_PROF_QL, S);
        td_solve(tp, nsel, S);
      }
      DMM_HIP(hipGetLastError());
      td_fail_h.assign(nsel, 0);
      DMM_HIP(hipMemcpyAsync(td_fail_h.data(), W.fail, nsel * sizeof(int), hipMemcpyDeviceToHost, S));
      DMM_HIP(hipStreamSynchronize(S));
      // QL stalled or its log overflowed (counted: "ml_tiles_ql_failed"): those matrices -- and only those, the others have
      // already replaced their right-hand side by the solution -- go through Jacobi on re-formed Gram matrices
      std::vector<int> redo;
      for (int k = 0; k < nsel; ++k)
        if (td_fail_h[k] & 1) redo.push_back(msel_h[k]);
        else count_stop(n, td_fail_h[k] >> 8);  // (the rank stop's effective order, 0: none)
      ctx->ml_tiles_ql_failed += (int64_t)redo.size();
      msel_h = redo;
      nsel = (int)msel_h.size();
      if (nsel) {
        DMM_HIP(hipMemcpyAsync(W.msel, msel_h.data(), nsel * sizeof(int), hipMemcpyHostToDevice, S));
        DMM_HIP(hipStreamSynchronize(S));
        gram();
      }
    }
    if (nsel) {
      DMM_TRY(jacobi(p, nsel));
    }
    return end_batch(p);
  }

  // ---- pipelined chunks
  int pipe_ready() {
    if (!ctx->aux_stream) DMM_HIP(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
    if (!ctx->aux_stream_b) DMM_HIP(hipStreamCreateWithFlags(&ctx->aux_stream_b, hipStreamNonBlocking));
    for (hipEvent_t& e : ctx->aux_ev)
      if (!e) DMM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (ctx->aux_pinned_n < (size_t)cap + 1) {
      if (ctx->aux_pinned) DMM_HIP(hipHostFree(ctx->aux_pinned));
      ctx->aux_pinned = nullptr;
      DMM_HIP(hipHostMalloc((void**)&ctx->aux_pinned, ((size_t)cap + 1) * sizeof(int), hipHostMallocDefault));
      ctx->aux_pinned_n = (size_t)cap + 1;
    }
    return DMM_OK;
  }
  // wait for the solve of the chunk in slot h and collect the matrices whose QL gave up
  int retire(int h) {
    Half& H = half[h];
    if (!H.busy) return DMM_OK;
    DMM_HIP(hipEventSynchronize(ctx->aux_ev[2 + h]));
    const int* fl = ctx->aux_pinned + (size_t)H.off;
    for (int k = 0; k < H.nmat; ++k)
      if (fl[k] & 1) {
        (H.sky ? redo_sky[H.np_sky] : redo_tel).push_back(H.ids[k]);
        ++ctx->ml_tiles_ql_failed;
      } else if (!bs_build) {  // the rank stop's effective order (0: none)
        count_stop(H.np, fl[k] >> 8);
        if (!H.sky && !pl->ml_ne.empty()) pl->ml_ne[(size_t)H.ids[k]] = (int16_t)((fl[k] >> 8) ? (fl[k] >> 8) : H.np);
      }
    H.busy = false;
    return DMM_OK;
  }
  int retire_both() {
    const int rc = retire(0);
    return rc ? rc : retire(1);
  }
  // Chunk slot h: Gram matrices and reduction of list[i0, i0 + nmat) on the caller's stream, then chase, QL and the
  // back-projection on the slot's own stream (one stream per slot: the two QL launches overlap)
  int launch_chunk(int h, const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky) {
    DMM_TRY(retire(h));
    Half& H = half[h];
    const size_t off = (size_t)slot_off(h);
    const Layout& L = W.L;
    hipStream_t S1 = ctx->stream, S2 = h ? ctx->aux_stream_b : ctx->aux_stream;
    DenseParams p = batch_params(W, off, nmat, sky, np_sky, alm);
    dmm_tile* const tiles_h = W.tiles + off;
    int32_t* const work_h = W.work + dl::work_first(off, h ? dl::kChunk1 : dl::kChunk0);
    int* const fail_hd = W.fail + off;
    double2* const Vb = W.aux + off * 2 * L.Np * L.Np;
    H.off = (int)off;
    H.nmat = nmat;
    H.np = p.Np;
    H.sky = sky;
    H.np_sky = np_sky;
    H.ids.assign(list.begin() + i0, list.begin() + i0 + nmat);
    DMM_TRY(upload_lists(pl, H.ids.data(), nmat, H.tiles, H.work, tiles_h, work_h, S1));
    int n = p.Np;
    // slots of the chunk's telescope-side matrices (resident Gram products / bases) -> device (the int array of the Jacobi
    // flags is free on this path)
    int* const slots_d = W.flag + off;
    if (!sky && (gcache_on || bs_build || bs_use)) {
      DMM_TRY(upload_slots(gslot_of, H.ids.data(), nmat, H.slots, slots_d, S1));
    }
    // Basis route (dmm_ctx_set_ml_basis): every tile of the chunk has its singular basis resident -- the day's problem is
    // M = X X^H with X = Sigma U^H D, of the order of the chunk's largest rank; no Gram product of B
    int nr = 0;
    if (!sky && bs_use) {
      int rmx = 0;
      bool all = true;
      for (int i = 0; i < nmat; ++i) {
        const int r = H.slots[i] >= 0 ? ctx->ml_bs_rank_h[(size_t)H.slots[i]] : -1;
        all = all && r >= 0;
        rmx = std::max(rmx, r);
      }
      nr = std::max((rmx + TB - 1) / TB * TB, 2 * TB);
      if (!all || nr + 128 > n || !sb_usable(ctx, nr)) nr = 0;
      // X (nr x ntel) sits in the second half of the matrix's log region, the T factors and the chase's reflector log
      // of the order-nr reduction at the region's tail: the route is taken only where the two do not meet (otherwise the
      // full-order path; ADVICE r4: Np 576 at nr 448, Np 768 at nr >= 576, Np 1024 at nr >= 768 would overlap)
      if (nr > 0 && (int64_t)L.Np * L.Np + (int64_t)nr * ntel + sb_tail(nr) > (int64_t)2 * L.Np * L.Np) nr = 0;
    }
    if (nr > 0) {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S1);
      double2* const Xb = Vb + (int64_t)L.Np * L.Np;  // second half of every matrix's log region (the QL log is capped below it)
      const int64_t xs = (int64_t)2 * L.Np * L.Np;
      int* const rank_d = W.msel + off;                // (the selection list of the synchronous batches: free here)
      hipLaunchKernelGGL(k_basis_x, dim3(nmat), dim3(kThreads), 0, S1, p, (const double2*)ctx->ml_bs_U, (const double*)ctx->ml_bs_sigma,
                         (const int32_t*)ctx->ml_bs_rank, (const int*)slots_d, ctx->ml_bs_rmax, Xb, xs, nr, rank_d);
      p.X = Xb;
      p.xstride = xs;
      p.ldx = ntel;
      p.lr_n = ntel;
      p.lr_rank = rank_d;
      p.N = p.Np = nr;
      p.T = nr / TB;
      hipLaunchKernelGGL(k_nt<MODE_GRAMX>, dim3(p.T * (p.T + 1) / 2, nmat), dim3(kThreads), 0, S1, p);  // M = X X^H
      ctx->ml_gram_flops += (int64_t)(4.0 * nr * (double)nr * ntel) * nmat;
      n = nr;
      H.np = nr;
      ctx->ml_tiles_basis += nmat;
    } else {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S1);
      form_gram(ctx, p, nmat, S1, Vb, gcache_on ? &H.slots : nullptr, slots_d, H.tiles.data());
      // (the lower-triangle band reduction reads the upper triangle only inside the diagonal tiles, which the Gram
      // kernel writes in full)
      if (!sb_usable(ctx, n)) hipLaunchKernelGGL(k_mirror, dim3(64, nmat), dim3(kThreads), 0, S1, p);
    }
    // (a basis must hold B B^H to 1e-15: its truncation enters the day's Gram matrix in first order)
    TdParams tp = td_params(ctx, p, L, W.blocks + off * (L.Np / 64) * TB * TB, Vb, fail_hd, acond, rcond, nullptr, n <= 2048 ? 1 : 0,
                            sb_usable(ctx, n) ? 1 : 0, bs_build ? 1e-16 : sb_stop_tol(ctx));
    if (nr > 0) tp.log_cap = (int)std::min<int64_t>(tp.log_cap, (int64_t)L.Np * L.Np - ((int64_t)3 * 16 * n * sizeof(int) + 15) / 16);  // (QL's log and its chase headers end where X begins)
    if (bs_build && !sky) {
      DMM_REQUIRE(tp.two_stage, "dmm_ml_run: the basis build needs the two-stage reduction (order %d)", n);
      tp.bs_U = ctx->ml_bs_U;
      tp.bs_sigma = ctx->ml_bs_sigma;
      tp.bs_rank = ctx->ml_bs_rank;
      tp.bs_slot = slots_d;
      tp.bs_rmax = ctx->ml_bs_rmax;
      tp.bs_ld = ntel;
      tp.bs_tol = 1e-15;
    }
    DMM_HIP(hipMemsetAsync(fail_hd, 0, nmat * sizeof(int), S1));
    reduce(tp, nmat, S1);
    DMM_HIP(hipGetLastError());
    DMM_HIP(hipEventRecord(ctx->aux_ev[h], S1));
    DMM_HIP(hipStreamWaitEvent(S2, ctx->aux_ev[h], 0));
    if (tp.two_stage) {  // the chase is one wave per matrix, as latency bound as QL: it runs beside the next chunk's sweeps too
      dmm_prof_scope prof(ctx, DMM_PROF_CHASE, S2);
      int hint = 0;  // the chunk's largest known effective order + 64 columns, if every tile of it has one (full-order chunks)
      if (!sky && nr == 0 && !pl->ml_ne.empty()) {
        int mx = 0;
        bool all = true;
        for (int i = 0; i < nmat; ++i) {
          const int v = pl->ml_ne[(size_t)list[i0 + i]];
          all = all && v > 0;
          mx = std::max(mx, v);
        }
        if (all) hint = (mx + TB - 1) / TB * TB + TB;
      }
      sb_chase(ctx, tp, nmat, S2, hint);
    }
    {
      dmm_prof_scope prof(ctx, DMM_PROF_QL, S2);
      td_solve(tp, nmat, S2);
    }
    DMM_HIP(hipGetLastError());
    if (!sky && !bs_build) {  // back-projection a = B^H w of the chunk's tiles, behind its solve on the second stream
      dmm_prof_scope prof(ctx, DMM_PROF_BACKPROJ, S2);
      ctx->stream = S2;
      const int rc = dmm_dirty_w_launch_list(pl, B, p.wbuf, nullptr, tiles_h, work_h, nmat, H.work[nmat], alm);
      ctx->stream = S1;
      if (rc) return rc;
    }
    DMM_HIP(hipMemcpyAsync(ctx->aux_pinned + off, fail_hd, nmat * sizeof(int), hipMemcpyDeviceToHost, S2));
    DMM_HIP(hipEventRecord(ctx->aux_ev[2 + h], S2));
    H.busy = true;
    ctx->ml_tiles_eigen += nmat;
    return DMM_OK;
  }

  // One list of same-order matrices through the eigen path: pipelined tridiagonal chunks, or (few matrices, or the
  // Jacobi / full-matrix variants asked for) synchronous batches
  int eigen_list(const std::vector<int64_t>& list_in, bool sky, int np_sky) {
    if (list_in.empty()) return DMM_OK;
    // basis route: the chunks' small problems have the order of their LARGEST rank -- tiles of like rank share chunks
    std::vector<int64_t> by_rank;
    if (!sky && bs_use) {
      by_rank = list_in;
      auto rk = [&](int64_t t) { const int32_t sl = gslot_of[(size_t)t]; return sl >= 0 ? ctx->ml_bs_rank_h[(size_t)sl] : -1; };
      std::stable_sort(by_rank.begin(), by_rank.end(), [&](int64_t a, int64_t b) { return rk(a) > rk(b); });
    }
    // full-order path: by the effective order of the tiles' last decomposition, where the plan knows it (dmm_plan::ml_ne) --
    // chunks of like rank end their stage 1 together, and their bulge chase gets an LDS image sized for the chunk
    if (!sky && !bs_use && !bs_build && ctx->opt_ml_chase_split != 1) {
      if (pl->ml_ne.empty()) pl->ml_ne.assign((size_t)pl->ntile, 0);
      size_t known = 0;
      for (int64_t t : list_in) known += pl->ml_ne[(size_t)t] > 0;
      if (known * 10 >= list_in.size() * 9) {
        by_rank = list_in;
        auto rk = [&](int64_t t) { const int v = pl->ml_ne[(size_t)t]; return v > 0 ? v : 32767; };
        std::stable_sort(by_rank.begin(), by_rank.end(), [&](int64_t a, int64_t b) { return rk(a) > rk(b); });
      }
    }
    const std::vector<int64_t>& list = by_rank.empty() ? list_in : by_rank;
    const int np = ((sky ? np_sky : ntel) + TB - 1) / TB * TB;
    const int eig = ctx->opt_ml_eigen;
    const bool pipelined = capE >= 1 && (eig == 4 || eig == 3 || bs_build || (eig == 0 && (double)std::min<size_t>(capE, list.size()) * np >= 12000.0));
    if (!pipelined) {
      // the synchronous batches use the whole workspace: nothing of the pipeline may still be in flight in it
      int rc = retire_both();
      for (size_t i0 = 0; i0 < list.size() && !rc; i0 += cap) rc = eigen_batch(list, i0, (int)std::min<size_t>(cap, list.size() - i0), sky, np_sky, false);
      return rc;
    }
    int rc = pipe_ready();
    for (size_t i0 = 0; i0 < list.size() && !rc; ++chunk_no) {
      const int h = chunk_no & 1;
      const int nm = (int)std::min<size_t>(slot_cap(h), list.size() - i0);
      rc = launch_chunk(h, list, i0, nm, sky, np_sky);
      i0 += nm;
    }
    return rc;
  }

  // the end of the pipeline: both slots retired, then the matrices whose QL gave up as synchronous Jacobi batches
  int drain() {
    DMM_TRY(retire_both());
    int rc = DMM_OK;
    auto redo = [&](const std::vector<int64_t>& list, bool sky, int np_sky) {
      for (size_t i0 = 0; i0 < list.size() && !rc; i0 += cap) {
        const int nmat = (int)std::min<size_t>(cap, list.size() - i0);
        ctx->ml_tiles_eigen -= nmat;  // (counted once already)
        rc = eigen_batch(list, i0, nmat, sky, np_sky, true);
      }
    };
    redo(redo_tel, false, 0);
    for (auto& kv : redo_sky) redo(kv.second, true, kv.first);
    redo_tel.clear();
    redo_sky.clear();
    return rc;
  }

  // Certificate first; rejected tiles are deferred.  Trying the certificate costs a Gram matrix and two
  // factorisations per tile (about a fifth of a decomposition): where almost nothing passes -- ill-conditioned beam
  // transfers -- the batches go to the eigen pass directly, and every eighth batch probes again.
  // (break-even: a certificate attempt costs ~0.10 ms per tile, a decomposition ~0.44: worth trying above ~0.25)
  // The pass rate is a property of the telescope's beam transfers, not of the day: it is remembered across calls (per
  // context).  A call whose predecessor found (almost) nothing to certify starts with a 128-tile probe instead of a
  // full batch, and while the probes keep failing they thin out: every 8th batch, then every 16th, ... (a full batch of
  // rejects costs a Gram matrix and two factorisations per tile: 6 % of the structured-tile day went there).
  int certify(const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky) {
    double& pass_rate = ctx->ml_pass_rate;
    int& probe_every = ctx->ml_probe_every;
    auto defer = [&](size_t a, size_t b) {  // untried, to the deferred pass
      std::vector<int64_t>& d = sky ? sky_deferred[np_sky] : tel_deferred;
      d.insert(d.end(), list.begin() + a, list.begin() + b);
      return DMM_OK;
    };
    if (pass_rate < 0.3 && batch_no > 0 && (++batch_no % probe_every) != 0) return defer(i0, i0 + nmat);
    if (batch_no == 0) batch_no = 1;
    // a probe (the rate was low last time) is a sample of the batch, not the batch: 128 tiles cost a hundredth of a
    // pass, a full batch of rejects a twentieth
    constexpr int kProbe = 128;
    const bool probe = pass_rate < 0.3 && nmat > 2 * kProbe;
    const int first = probe ? kProbe : nmat;
    const int64_t before = ctx->ml_tiles_direct;
    int rc = cert_batch(list, i0, first, sky, np_sky);
    pass_rate = (double)(ctx->ml_tiles_direct - before) / (double)first;
    if (probe) probe_every = pass_rate < 0.3 ? std::min(probe_every * 2, 64) : 8;
    if (rc || first == nmat) return rc;
    if (pass_rate >= 0.3) return cert_batch(list, i0 + first, nmat - first, sky, np_sky);
    return defer(i0 + first, i0 + nmat);
  }

  // Rejects that are known while direct batches remain are decomposed EARLY, on two small chunk slots at the end of the
  // workspace: Gram matrices and reduction on this stream, then the serial QL (a ~0.1 s latency floor whatever the
  // count) on the slot's own stream, under the direct batches that follow in the front of the workspace.  Left to the
  // end, as before, that floor had nothing to hide behind: a fifth of the whole ML pass for the forty-odd near-square
  // tiles of a well-conditioned cfg-3 slab.  To know the rejects early the near-square tiles go FIRST: the sky-side orders
  // from the largest down (their rejects to slot 1), then the telescope-side tiles by descending m (slot 0).
  // This step launches a reject list in `slot` if that slot is free right now (never waits), and empties the list if it did.
  int early(std::vector<int64_t>& list, bool sky, int np_sky, int slot) {
    const int np = ((sky ? np_sky : ntel) + TB - 1) / TB * TB;
    // (a list that does not fit one slot is the ill-conditioned regime: it belongs to the full-size pipeline at the end)
    // and ONE early chunk per slot: a trickle of small chunks would each pay the per-column launch chain and the QL floor
    if (slot_layout != kEarlySlots || early_used[slot] || list.empty() || (int)list.size() > E || ctx->opt_ml_eigen != 0 || (double)list.size() * np < 12000.0) return DMM_OK;
    early_used[slot] = true;
    if (half[slot].busy) {
      if (hipEventQuery(ctx->aux_ev[2 + slot]) != hipSuccess) return DMM_OK;  // its QL is still running: next time
      DMM_TRY(retire(slot));
    }
    if ((chunk_no & 1) != slot) ++chunk_no;
    int rc = eigen_list(list, sky, np_sky);  // one chunk, in slot `slot`
    ++ctx->ml_early_chunks;
    list.clear();
    return rc;
  }
};

}  // namespace

// largest matrix order the two-stage reduction takes (dmm_ctx_get_counter "ml_two_stage_max_order"): the basis route of
// a telescope above it is declined by the caller
int dmm_ml_two_stage_max_order() {
  for (int n = kSbRows * kThreads; n >= 64; n -= 64)
    if (sb_fits(n)) return n;
  return 0;
}

extern "C" {

// (the Wiener solve stages the sky-side operand like ML does: same workspace layout)
int64_t dmm_wiener_workspace_bytes(const dmm_plan* pl) { return workspace_bytes(pl, 1); }
int64_t dmm_ml_workspace_bytes(const dmm_plan* pl) { return workspace_bytes(pl, 2); }
// resident beam Gram products (dmm_ctx_set_ml_gram_cache): one slot per telescope-side tile of the plan, in plan order
int64_t dmm_ml_gram_cache_slots(const dmm_plan* pl) {
  if (!pl) return 0;
  int64_t n = 0;
  for (const dmm_tile& t : pl->tiles_h) n += pl->npol * (pl->lmax + 1 - t.m) >= 2 * pl->npairs;
  return n;
}
int64_t dmm_ml_gram_cache_bytes(const dmm_plan* pl) {
  if (!pl) return 0;
  const int64_t T = (2 * pl->npairs + TB - 1) / TB;
  return dmm_ml_gram_cache_slots(pl) * (T * (T + 1) / 2) * TB * TB * (int64_t)sizeof(double2);
}

int dmm_wiener_run(dmm_plan* pl, const void* B, const void* mvis, const double* mweight, double prior_amp,
                   double prior_tilt, void* workspace, void* alm) {
  DMM_REQUIRE(pl && B && mvis && mweight && workspace && alm, "dmm_wiener_run: NULL argument");
  DMM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dmm_wiener_run: workspace must be 256-byte aligned");
  if (pl->ntile == 0) return DMM_OK;
  dmm_ctx* ctx = pl->ctx;
  DMM_HIP(hipSetDevice(ctx->device));
  const DenseWs W = carve_ws(pl, 1, B, mvis, mweight, workspace);
  const Layout& L = W.L;
  const int cap = W.cap;
  double* Sl = (double*)workspace;
  double* Sk = (double*)((unsigned char*)workspace + L.sl_bytes);
  hipLaunchKernelGGL(k_prior, dim3(4), dim3(256), 0, ctx->stream, Sl, pl->lmax, prior_amp, prior_tilt);
  hipLaunchKernelGGL(k_prior_expand, dim3(pl->lmax + 1), dim3(256), 0, ctx->stream, (const double*)Sl, Sk, pl->lmax, pl->npol, L.sk_pitch);

  // Both of the reference's branches (mapmaker.py:267-278) are the same estimator; the smaller system is
  // solved: telescope side G = I + D B S B^H D while nsky_m >= ntel, sky side C^-1 = S^-1 + B^H Ni B at high m
  std::vector<int64_t> tel_list;
  std::map<int, std::vector<int64_t>> sky_lists;  // by padded order
  partition_tiles(pl, {}, tel_list, sky_lists);
  if (!sky_lists.empty()) {
    DMM_TRY(sky_rhs(pl, B, mvis, mweight, alm, sky_lists, W));
  }
  // resident beam Gram products (dmm_ctx_set_ml_gram_cache; here B S B^H: the cache belongs to this maker and this prior)
  const bool gcache_on = ctx->ml_gcache && ctx->opt_gram_stage != 1 && ctx->opt_ml_shortcut != 3 && dmm_ml_gram_cache_slots(pl) <= ctx->ml_gslots;
  std::vector<int32_t> gslot_of;
  if (gcache_on) gslot_of = gslot_table(pl);
  std::vector<int> slots_c[2];
  DMM_TRY(chol_attributes(L));

  // The batches go down TWO streams in turn, half the workspace each: the factorisation of one batch -- its diagonal
  // blocks and the triangular solves are latency bound, one block per matrix -- runs beside the Gram products of the
  // next.  ("wiener_overlap" = 0: one stream, whole workspace, the A/B.)
  const size_t ntiles = tel_list.size() + concat(sky_lists).size();
  const bool two = ctx->opt_wiener_overlap && cap >= 2 && ntiles > (size_t)cap / 2;
  const int caph = two ? cap / 2 : cap;
  // host-side sources of the batches' asynchronous list uploads: declared FIRST so that they outlive every guard
  // below (destructors run in reverse order) -- on an early error return both streams are drained before they die
  std::vector<dmm_tile> tiles_c[2];
  std::vector<int32_t> work_c[2];
  dmm_aux_scope aux_guard(ctx);  // the second stream is drained on every return path
  StreamRestore stream_guard{ctx, ctx->stream};
  hipStream_t st[2] = {ctx->stream, ctx->stream};
  struct DrainCaller {  // the caller's stream too: copies out of tiles_c / work_c may still be queued on it
    hipStream_t s;
    ~DrainCaller() { (void)hipStreamSynchronize(s); }
  } drain_guard{st[0]};
  dmm_prof_scope prof_all(ctx, DMM_PROF_SOLVE, st[0]);  // the whole pass on the caller's stream (both halves are joined before it ends)
  if (two) {
    if (!ctx->aux_stream) DMM_HIP(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
    if (!ctx->aux_ev[0]) DMM_HIP(hipEventCreateWithFlags(&ctx->aux_ev[0], hipEventDisableTiming));
    st[1] = ctx->aux_stream;
    DMM_HIP(hipEventRecord(ctx->aux_ev[0], st[0]));  // the prior tables and the sky-side right-hand sides are ready
    DMM_HIP(hipStreamWaitEvent(st[1], ctx->aux_ev[0], 0));
  }
  int batch_no = 0;
  auto run_batch = [&](const std::vector<int64_t>& list, size_t i0, int nmat, bool sky, int np_sky) -> int {
    const int h = two ? (batch_no++ & 1) : 0;
    hipStream_t S = st[h];
    const size_t off = (size_t)h * caph;
    // the half's previous batch is done: its host vectors and device lists are free again
    DMM_HIP(hipStreamSynchronize(S));
    dmm_tile* const tiles_h = W.tiles + off;
    int32_t* const work_h = W.work + dl::work_first(off, dl::kBatch);
    DenseParams p = batch_params(W, off, nmat, sky, np_sky, alm);
    p.Linv = W.blocks + off * (L.Np / 64) * TB * TB;
    DMM_TRY(upload_lists(pl, list.data() + i0, nmat, tiles_c[h], work_c[h], tiles_h, work_h, S));
    if (sky) {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S);
      form_gram(ctx, p, nmat, S, W.aux + off * L.Np * L.Np, nullptr, nullptr, nullptr);
      hipLaunchKernelGGL(k_add_prior_diag, dim3((p.Np + 255) / 256, nmat), dim3(256), 0, S, p, (const double*)Sl);
    } else {
      dmm_prof_scope prof(ctx, DMM_PROF_GRAM, S);
      p.Sl = Sl;
      p.Sk = Sk;
      p.sk_pitch = L.sk_pitch;
      p.add_identity = 1;
      if (gcache_on) {
        DMM_TRY(upload_slots(gslot_of, list.data() + i0, nmat, slots_c[h], W.slots + off, S));
      }
      form_gram(ctx, p, nmat, S, nullptr, gcache_on ? &slots_c[h] : nullptr, W.slots + off, nullptr);
    }
    chol_factor(ctx, p, nmat, S, solve_lds(L));
    DMM_HIP(hipGetLastError());
    if (!sky) {
      dmm_prof_scope prof(ctx, DMM_PROF_BACKPROJ, S);
      ctx->stream = S;
      const int rc = dmm_dirty_w_launch_list(pl, B, p.wbuf, Sl, tiles_h, work_h, nmat, work_c[h][nmat], alm);
      ctx->stream = st[0];
      if (rc) return rc;
    }
    return DMM_OK;
  };
  for (size_t i0 = 0; i0 < tel_list.size(); i0 += caph) {
    DMM_TRY(run_batch(tel_list, i0, (int)std::min<size_t>(caph, tel_list.size() - i0), false, 0));
  }
  for (auto& kv : sky_lists)
    for (size_t i0 = 0; i0 < kv.second.size(); i0 += caph) {
      DMM_TRY(run_batch(kv.second, i0, (int)std::min<size_t>(caph, kv.second.size() - i0), true, kv.first));
    }
  // the caller's stream continues behind both halves (the host vectors die with this frame: wait for their copies)
  if (two) DMM_HIP(hipStreamSynchronize(st[1]));
  DMM_HIP(hipStreamSynchronize(st[0]));
  return DMM_OK;
}

// The ML pass.  Its steps are MlPass's member functions; this function checks the arguments, holds the guards, sets the
// kernels' attributes and gives the schedule.
int dmm_ml_run(dmm_plan* pl, const void* B, const void* mvis, const double* mweight, double acond, double rcond,
               void* workspace, void* alm) {
  DMM_REQUIRE(pl && B && mvis && mweight && workspace && alm, "dmm_ml_run: NULL argument");
  DMM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dmm_ml_run: workspace must be 256-byte aligned");
  if (pl->ntile == 0) return DMM_OK;
  dmm_ctx* ctx = pl->ctx;
  DMM_HIP(hipSetDevice(ctx->device));
  // the eigen pass runs chunks on the library's second stream inside B, workspace and alm: drained on every
  // return path (dmm_internal.h, "Buffer rule"); the caller's stream pointer is restored with it
  dmm_aux_scope aux_guard(ctx);
  StreamRestore stream_guard{ctx, ctx->stream};
  MlPass P(pl, B, mvis, mweight, acond, rcond, workspace, alm);
  const Layout& L = P.W.L;
  DMM_REQUIRE(!ctx->ml_bs_build || P.bs_build, "dmm_ml_run: the basis build needs the two-stage reduction with its rank stop and enough slots");

  std::vector<char> is_null(pl->ntile, 0);
  DMM_TRY(P.null_certificate(workspace, is_null));
  std::vector<int64_t> tel_list;
  std::map<int, std::vector<int64_t>> sky_lists;
  partition_tiles(pl, is_null, tel_list, sky_lists);
  if (P.bs_build) sky_lists.clear();  // (a basis belongs to a telescope-side tile)
  if (P.gcache_on || P.bs_build || P.bs_use) P.gslot_of = gslot_table(pl);
  if (!sky_lists.empty()) {
    DMM_TRY(sky_rhs(pl, B, mvis, mweight, alm, sky_lists, P.W));
  }
  DMM_TRY(chol_attributes(L));
  DMM_HIP(hipFuncSetAttribute((const void*)k_bj_sub, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSubLds));
  DMM_HIP(hipFuncSetAttribute((const void*)k_ml_filter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)2 * L.Np * sizeof(double2))));
  {
    const size_t td_vec = (size_t)3 * L.Np * sizeof(double2);
    const size_t td_sol = (size_t)L.Np * (sizeof(double2) + 2 * sizeof(double));
    DMM_REQUIRE(td_vec <= 160 * 1024 && td_sol <= 160 * 1024, "dmm_ml_run: matrix order %d too large for the LDS", L.Np);
    DMM_HIP(hipFuncSetAttribute((const void*)k_td_col, hipFuncAttributeMaxDynamicSharedMemorySize, (int)td_vec));
    DMM_HIP(hipFuncSetAttribute((const void*)k_td_trail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)td_vec));
    DMM_HIP(hipFuncSetAttribute((const void*)k_td_solve<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)td_sol));
    DMM_HIP(hipFuncSetAttribute((const void*)k_td_solve<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)td_sol));
    DMM_HIP(hipFuncSetAttribute((const void*)k_td_solve<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)td_sol));
    const int sb_n = sb_top(ctx, L.Np);  // (sky-side matrices are smaller than L.Np: they may take two stages where it does not)
    if (sb_n) DMM_HIP(hipFuncSetAttribute((const void*)k_sb_chase, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb_chase_lds(sb_n)));
    if (sb_n) DMM_HIP(hipFuncSetAttribute((const void*)k_sb_sweep_one, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb_one_lds(sb_n)));
#ifdef DMM_AB
    if (sb_n && ctx->opt_ml_reduce == 5) {
      const int fl = (int)std::min(sb_fused_lds(std::min(sb_n, 3 * kThreads)), kSbFusedLdsMax);
      DMM_HIP(hipFuncSetAttribute((const void*)k_sb_fused<1>, hipFuncAttributeMaxDynamicSharedMemorySize, fl));
      DMM_HIP(hipFuncSetAttribute((const void*)k_sb_fused<2>, hipFuncAttributeMaxDynamicSharedMemorySize, fl));
      DMM_HIP(hipFuncSetAttribute((const void*)k_sb_fused<3>, hipFuncAttributeMaxDynamicSharedMemorySize, fl));
    }
#endif
  }

  if (!P.shortcut) {  // every tile through the eigen path
    pair_orders(sky_lists);
    // largest systems first: the pass ends on the serial QL of its LAST chunk, which nothing is left to hide
    int rc = P.eigen_list(tel_list, false, 0);
    for (auto it = sky_lists.rbegin(); it != sky_lists.rend(); ++it)
      if (!rc) rc = P.eigen_list(it->second, true, it->first);
    const int rc2 = P.drain();
    return rc ? rc : rc2;
  }
  // Certificate passes (MlPass::certify) in the front of the workspace, [0, cap_direct), with the early chunks of their
  // rejects (MlPass::early) in the two slots behind -- if the workspace has room for them
  const int cap_direct = P.cap_direct;
  if (cap_direct < P.cap) P.slot_layout = MlPass::kEarlySlots;
  for (auto it = sky_lists.rbegin(); it != sky_lists.rend(); ++it) {
    const std::vector<int64_t>& list = it->second;
    for (size_t i0 = 0; i0 < list.size(); i0 += cap_direct) {
      DMM_TRY(P.certify(list, i0, (int)std::min<size_t>(cap_direct, list.size() - i0), true, it->first));
    }
    if (!P.sky_deferred.empty() && (std::next(it) != sky_lists.rend() || !tel_list.empty())) {  // rejects of the orders so far (while direct work remains), decomposed together at the largest of their orders
      std::vector<int64_t> all = concat(P.sky_deferred);
      DMM_TRY(P.early(all, true, P.sky_deferred.rbegin()->first, 1));
      if (all.empty()) P.sky_deferred.clear();  // launched (all of it: a list goes whole or not at all); otherwise the
                                                // tiles stay filed under their own orders
    }
  }
  // telescope side: the near-square tiles (high m) first, so that the rejects are known after the first batch and their
  // chunk runs under the remaining batches
  std::stable_sort(tel_list.begin(), tel_list.end(), [&](int64_t a, int64_t b) { return pl->tiles_h[a].m > pl->tiles_h[b].m; });
  for (size_t i0 = 0; i0 < tel_list.size(); i0 += cap_direct) {
    DMM_TRY(P.certify(tel_list, i0, (int)std::min<size_t>(cap_direct, tel_list.size() - i0), false, 0));
    if (i0 + cap_direct < tel_list.size()) DMM_TRY(P.early(P.tel_deferred, false, 0, 0));  // (only while batches remain)
  }
  if (P.slot_layout == MlPass::kEarlySlots) {  // back to the two halves for whatever is left: nothing of the early chunks may still be in them
    DMM_TRY(P.retire_both());
    P.slot_layout = MlPass::kHalves;
  }
  // A handful of rejected sky-side tiles spread over many padded orders would pay one launch chain (and its latency
  // floor) per order: they are decomposed together at the largest of their orders instead (order_of() keeps every
  // tile's own size; the padding is zeros).
  const size_t nsky_def = concat(P.sky_deferred).size();
  if (P.sky_deferred.size() > 1 && nsky_def <= 128) {
    const int np_max = P.sky_deferred.rbegin()->first;
    P.sky_deferred = {{np_max, concat(P.sky_deferred)}};
  }
  if (nsky_def > 128) pair_orders(P.sky_deferred);
  int rc = P.eigen_list(P.tel_deferred, false, 0);
  for (auto it = P.sky_deferred.rbegin(); it != P.sky_deferred.rend(); ++it)  // (largest first, as in the eigen-only pass)
    if (!rc) rc = P.eigen_list(it->second, true, it->first);
  const int rc2 = P.drain();
  return rc ? rc : rc2;
}

}  // extern "C"
