// Delay power spectrum by NRML: value, gradient, Hessian and Newton-CG direction of the maximum a posteriori problem of
// draco/analysis/delayopt.py (LogLikePS + GaussianProcessPrior), batched over baselines.
//
// Per baseline, n = nchan channels with indices chan[f] in the full set and N = ndelay delays; x = log S:
//   S = exp(clip(x)),  C = MF diag(S) MF^H + diag(Nm),  MF_fa = w_f exp(-2 pi i chan_f a / N),
//   U = MF diag(S^1/2),  Ut = C^-1 U,  R = (X - C) Ut,
//   value = ns (log det C + Re tr C^-1 X) + x^T Ci x / 2,
//   grad_a = ns t_a + (Ci x)_a,  t_a = -sum_f Re(conj(Ut_fa) R_fa),
//   H_ab = ns (Re(P_ab^2) + 2 Re(Q_ab conj(P_ab)) + delta_ab t_a) + Ci_ab,  P = U^H Ut,  Q = Ut^H R
//   (the reference forms P o (P^H)^T, which for the Hermitian P is P_ab^2 and not |P_ab|^2; this follows it).
// A channel that is cut (zero weight, cut by freq_frac, or a window coefficient that is exactly zero) has w_f = 0 and
// stays in place as an identity row and column of C and a zero row and column of X: value, gradient and Hessian are
// those of the smaller problem and every baseline of a batch keeps one shape.
//
// Complex n-vectors are held as real 2n-vectors [Re ; Im] and C as its real embedding [[A, -B], [B, A]] of order 2n, so
// the factorisation, the solves and the products are those of chol_blocked.h.  Rows of U, Y (= Ut after the solve) and
// R are the COLUMNS of the matrices above: U [N][2n] row a = [Re U_:a ; Im U_:a].
//
//   k_nrml_tw       tw[m] = (cos, sin)(2 pi m / N);
//   k_nrml_split    from two prepare passes of delay.hip (the mean-removed data with a unit coefficient, and the form
//                   that carries twice the averaged weight as last row): the averaged weight, Nm, w, the retained-sample count, the windowed data in the two layouts
//                   whose Gram products add up to the embedding of X, and the unwindowed data of the channels above
//                   the pseudo-inverse cut for the starting point;
//   k_nrml_scale / k_nrml_var   X / ns, and the variance over the retained samples of the projected data;
//   k_nrml_exp / k_nrml_spec    S, and s^[m] = sum_a S_a exp(-2 pi i a m / N): C_ff' = w_f w_f' s^[(chan_f - chan_f') mod N];
//   k_nrml_fill     G = emb(C), D = emb(X) - G;   k_nrml_rows  U, and Y = [U ; columns of X];
//   (dl_factor, dl_solve_rows, dl_gemm: G = U^T U, Y <- C^-1 Y, R = Y D)
//   k_nrml_grad / k_nrml_value   t, Ci x, the gradient; log det, the trace, the prior, the value;
//   (dl_gemm: the planes Re P, Im P, Re Q, Im Q; the imaginary parts pair component k with its partner in the other
//   half, Im(conj(u) v) = u_re v_im - u_im v_re, so each is two products over K = n)
//   k_nrml_hess_ew  the Hadamard combination of the four planes, the prior and the diagonal, the lower triangle mirrored;
//   k_nrml_cg       scipy's truncated conjugate gradient for H p = -g, one block per baseline, the whole inner loop in
//                   one launch, sums in a fixed order.
// Every kernel leaves a baseline alone once its status word is set.
#include "chol_blocked.h"

#include <cfloat>

namespace {

constexpr int kNrMaxChan = 1024, kNrMaxDelay = 2048;
constexpr int kCgThreads = 512, kCgPer = kNrMaxDelay / kCgThreads;

// (hi, lo) += a b in double-double: the product exactly (fma), the sum by Knuth's two-sum.  C and the prior's gradient
// are sums with heavy cancellation (S spans many decades, Ci is the inverse of a smooth kernel) and their rounding is
// what the gradient at the optimum, itself a small difference, shows first.
__device__ __forceinline__ void nr_dd_add(double p, double e, double& hi, double& lo) {
  const double s = hi + p, bb = s - hi;
  lo += ((hi - (s - bb)) + (p - bb)) + e;
  hi = s;
}
__device__ __forceinline__ void nr_dd_fma(double a, double b, double& hi, double& lo) {
  const double p = a * b;
  nr_dd_add(p, fma(a, b, -p), hi, lo);
}

__global__ void k_nrml_tw(int N, double2* __restrict__ tw) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= N) return;
  double s, c;
  sincospi(2.0 * (double)m / (double)N, &s, &c);
  tw[m] = make_double2(c, s);
}

// One block per baseline.  Xd [ns][2 n] interleaved (Re, Im) per channel: d - mean, zero where cut; the last row of Xp
// [ns + 1][2 n] is c = 2 ni on the real entries.
__global__ __launch_bounds__(256) void k_nrml_split(int n, int ns, const double* __restrict__ win, const double* __restrict__ Xp_all, const double* __restrict__ Xd_all, const uint8_t* __restrict__ nzt_all,
                                                    const int32_t* __restrict__ status, double* __restrict__ work, double* __restrict__ wv_all, double* __restrict__ Nm_all,
                                                    double* __restrict__ nsv) {
  __shared__ double s_max[256];
  __shared__ int s_cnt[256];
  const int b = blockIdx.x;
  if (status[b]) return;
  const int K = 2 * n;
  const double* last = Xp_all + ((size_t)b * (ns + 1) + ns) * K;
  const double* Xd = Xd_all + (size_t)b * ns * K;
  const uint8_t* nzt = nzt_all + (size_t)b * ns;
  double* W = work + (size_t)b * 3 * ns * K;
  double* W2 = W + (size_t)ns * K;
  double* Xu = W2 + (size_t)ns * K;
  double* wv = wv_all + (size_t)b * n;
  double* Nm = Nm_all + (size_t)b * n;
  double mx = 0.0;
  int cnt = 0;
  for (int f = threadIdx.x; f < n; f += 256) {
    const double ni = 0.5 * last[2 * f];
    const double w = ni != 0.0 ? win[f] : 0.0;
    wv[f] = w;
    Nm[f] = ni != 0.0 ? 1.0 / ni : 0.0;
    mx = fmax(mx, fabs(w));
  }
  for (int s = threadIdx.x; s < ns; s += 256) cnt += nzt[s] ? 1 : 0;
  s_max[threadIdx.x] = mx;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + h]);
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
    }
    __syncthreads();
  }
  const double thr = 1e-3 * s_max[0];
  if (threadIdx.x == 0) nsv[b] = (double)s_cnt[0];
  for (int64_t e = threadIdx.x; e < (int64_t)ns * n; e += 256) {
    const int s = (int)(e / n), f = (int)(e % n);
    const double dr = Xd[(size_t)s * K + 2 * f], di = Xd[(size_t)s * K + 2 * f + 1];
    const double w = wv[f];
    const bool keep = fabs(w) > thr;
    W[(size_t)s * K + f] = w * dr;
    W[(size_t)s * K + n + f] = w * di;
    W2[(size_t)s * K + f] = -(w * di);
    W2[(size_t)s * K + n + f] = w * dr;
    Xu[(size_t)s * K + 2 * f] = keep ? dr : 0.0;
    Xu[(size_t)s * K + 2 * f + 1] = keep ? di : 0.0;
  }
}

__global__ void k_nrml_scale(int64_t count, const double* __restrict__ nsv, const int32_t* __restrict__ status, double* __restrict__ Xe) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  Xe[(size_t)b * count + e] /= nsv[b];
}

// S0[b][a] = variance over the retained samples of Z[b][s][a] / N (Z complex, interleaved)
__global__ void k_nrml_var(int N, int ns, const double* __restrict__ Z, const uint8_t* __restrict__ nzt_all, const double* __restrict__ nsv, const int32_t* __restrict__ status,
                           double* __restrict__ S0) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const uint8_t* nzt = nzt_all + (size_t)b * ns;
  const double* z = Z + (size_t)b * ns * 2 * N + 2 * a;
  const double cnt = nsv[b], inv = 1.0 / (double)N;
  double mr = 0.0, mi = 0.0;
  for (int s = 0; s < ns; ++s)
    if (nzt[s]) {
      mr += z[(size_t)s * 2 * N] * inv;
      mi += z[(size_t)s * 2 * N + 1] * inv;
    }
  mr /= cnt;
  mi /= cnt;
  double v = 0.0;
  for (int s = 0; s < ns; ++s)
    if (nzt[s]) {
      const double dr = z[(size_t)s * 2 * N] * inv - mr, di = z[(size_t)s * 2 * N + 1] * inv - mi;
      v += dr * dr + di * di;
    }
  S0[(size_t)b * N + a] = v / cnt;
}

__global__ void k_nrml_exp(int N, const double* __restrict__ x, double lo, double hi, const int32_t* __restrict__ status, double* __restrict__ S) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const double v = x[(size_t)b * N + a];
  S[(size_t)b * N + a] = exp(fmin(fmax(v, lo), hi));
}

__global__ void k_nrml_spec(int N, const double2* __restrict__ tw, const double* __restrict__ S_all, const int32_t* __restrict__ status, double2* __restrict__ sh) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= N) return;
  const double* __restrict__ S = S_all + (size_t)b * N;
  double re = 0.0, rl = 0.0, im = 0.0, il = 0.0;
  int idx = 0;
  for (int a = 0; a < N; ++a) {
    const double2 t = tw[idx];
    const double s = S[a];
    nr_dd_fma(s, t.x, re, rl);
    nr_dd_fma(-s, t.y, im, il);
    idx += m;
    if (idx >= N) idx -= N;
  }
  sh[(size_t)b * N + m] = make_double2(re + rl, im + il);
}

// G = emb(C), D = emb(X) - emb(C); both [2n][2n]
__global__ void k_nrml_fill(int N, int n, const int32_t* __restrict__ chan, const double* __restrict__ wv_all, const double* __restrict__ Nm_all, const double* __restrict__ Xe_all,
                            const double2* __restrict__ sh_all, const int32_t* __restrict__ status, double* __restrict__ G_all, double* __restrict__ D_all) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int K = 2 * n;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)K * K) return;
  const int i = (int)(idx / K), j = (int)(idx % K);
  const int f = i % n, pi = i / n, g = j % n, pj = j / n;
  const double wf = wv_all[(size_t)b * n + f], wg = wv_all[(size_t)b * n + g];
  double cr, ci;
  if (wf == 0.0 || wg == 0.0) {
    cr = f == g ? 1.0 : 0.0;
    ci = 0.0;
  } else {
    int d = (chan[f] - chan[g]) % N;
    if (d < 0) d += N;
    const double2 s = sh_all[(size_t)b * N + d];
    const double ww = wf * wg;
    cr = ww * s.x + (f == g ? Nm_all[(size_t)b * n + f] : 0.0);
    ci = f == g ? 0.0 : ww * s.y;
  }
  const double v = pi == pj ? cr : (pi ? ci : -ci);
  G_all[(size_t)b * K * K + idx] = v;
  D_all[(size_t)b * K * K + idx] = Xe_all[(size_t)b * K * K + idx] - v;
}

// U [N][2n] and Y [N + n][2n] = [U ; columns of X]
__global__ void k_nrml_rows(int N, int n, const int32_t* __restrict__ chan, const double2* __restrict__ tw, const double* __restrict__ wv_all, const double* __restrict__ S_all,
                            const double* __restrict__ Xe_all, const int32_t* __restrict__ status, double* __restrict__ U_all, double* __restrict__ Y_all) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int K = 2 * n;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)(N + n) * K) return;
  const int a = (int)(idx / K), k = (int)(idx % K);
  double* Y = Y_all + (size_t)b * (N + n) * K;
  if (a >= N) {
    Y[idx] = Xe_all[(size_t)b * K * K + (size_t)k * K + (a - N)];
    return;
  }
  const int f = k % n;
  const int64_t m = ((int64_t)chan[f] * a) % N;
  const double2 t = tw[m];
  const double v = wv_all[(size_t)b * n + f] * sqrt(S_all[(size_t)b * N + a]) * (k < n ? t.x : -t.y);
  U_all[(size_t)b * N * K + idx] = v;
  Y[idx] = v;
}

// one wave per (baseline, delay): t_a, (Ci x)_a, grad_a
__global__ __launch_bounds__(256) void k_nrml_grad(int N, int n, const double* __restrict__ Y_all, const double* __restrict__ R_all, const double* __restrict__ Ci, const double* __restrict__ x_all,
                                                   const double* __restrict__ nsv, const int32_t* __restrict__ status, double* __restrict__ t_all, double* __restrict__ cix_all,
                                                   double* __restrict__ grad) {
  const int b = blockIdx.y;
  if (status[b]) return;
  const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= N) return;
  const int K = 2 * n;
  const double* y = Y_all + ((size_t)b * (N + n) + a) * K;
  const double* r = R_all + ((size_t)b * N + a) * K;
  const double* c = Ci + (size_t)a * N;
  const double* x = x_all + (size_t)b * N;
  double t = 0.0, p = 0.0, pl = 0.0;
  for (int k = lane; k < K; k += 64) t = fma(y[k], r[k], t);
  for (int j = lane; j < N; j += 64) nr_dd_fma(c[j], x[j], p, pl);
  for (int o = 32; o > 0; o >>= 1) {
    t += __shfl_down(t, o);
    const double ph = __shfl_down(p, o), pe = __shfl_down(pl, o);
    nr_dd_add(ph, pe, p, pl);
  }
  p += pl;
  if (lane == 0) {
    t_all[(size_t)b * N + a] = -t;
    cix_all[(size_t)b * N + a] = p;
    grad[(size_t)b * N + a] = nsv[b] * -t + p;
  }
}

__device__ __forceinline__ double nr_block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

// one block per baseline: ns (sum log diag U + sum_j Re (C^-1 X)_jj) + x . Ci x / 2
__global__ __launch_bounds__(256) void k_nrml_value(int N, int n, const double* __restrict__ G_all, const double* __restrict__ Y_all, const double* __restrict__ x_all,
                                                    const double* __restrict__ cix_all, const double* __restrict__ nsv, const int32_t* __restrict__ status, double* __restrict__ value) {
  __shared__ double red[256];
  const int b = blockIdx.x;
  if (status[b]) return;
  const int K = 2 * n;
  const double* G = G_all + (size_t)b * K * K;
  const double* Y = Y_all + ((size_t)b * (N + n) + N) * K;
  double ld = 0.0, tr = 0.0, pr = 0.0;
  for (int i = threadIdx.x; i < K; i += 256) ld += log(G[(size_t)i * K + i]);
  for (int j = threadIdx.x; j < n; j += 256) tr += Y[(size_t)j * K + j];
  for (int a = threadIdx.x; a < N; a += 256) pr = fma(x_all[(size_t)b * N + a], cix_all[(size_t)b * N + a], pr);
  ld = nr_block_sum(ld, red);
  tr = nr_block_sum(tr, red);
  pr = nr_block_sum(pr, red);
  if (threadIdx.x == 0) value[b] = nsv[b] * (ld + tr) + 0.5 * pr;
}

struct NrHess {
  const double* t;   // [nb][N]
  const double* Ci;  // [N][N]
  const double* nsv;
  const int32_t* status;
  double* H;  // [nb][N][N]
  int N, exact;
};

__device__ __forceinline__ double nr_hess_entry(double pr, double pi, double qr, double qi, double ns, double t, double ci, bool diag, int exact) {
  double h = pr * pr - pi * pi;
  if (exact) {
    h += 2.0 * (qr * pr + qi * pi);
    if (diag) h += t;
  }
  return ns * h + ci;
}

// H from planes PQ [nb][4][N][N] = Re P, Im P, Re Q, Im Q (formed by dl_gemm), the lower triangle mirrored
__global__ void k_nrml_hess_ew(NrHess h, const double* __restrict__ PQ) {
  const int bat = blockIdx.y;
  if (h.status[bat]) return;
  const int N = h.N;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nn = (int64_t)N * N;
  if (idx >= nn) return;
  const int a = (int)(idx / N), b = (int)(idx % N);
  if (a < b) return;
  const double* p = PQ + (size_t)bat * 4 * nn + idx;
  const double v = nr_hess_entry(p[0], p[nn], p[2 * nn], p[3 * nn], h.nsv[bat], h.t[(size_t)bat * N + a], h.Ci[idx], a == b, h.exact);
  h.H[(size_t)bat * nn + idx] = v;
  h.H[(size_t)bat * nn + (size_t)b * N + a] = v;
}

// scipy's inner loop of Newton-CG (scipy/optimize/_optimize.py, _minimize_newtoncg) for H p = -g.  Thread i owns the
// elements i, i + 512, ...; H is symmetric and is read column-wise, so a wave reads consecutive addresses.
// info[b] = (passes, flag): flag 0 a direction, 3 the passes ran out ("CG iterations didn't converge").
__global__ __launch_bounds__(kCgThreads) void k_nrml_cg(int N, const double* __restrict__ H_all, const double* __restrict__ g_all, const int32_t* __restrict__ status, double* __restrict__ p_out,
                                                        int32_t* __restrict__ info) {
  __shared__ double red[kCgThreads];
  __shared__ double ps[kNrMaxDelay];
  const int bat = blockIdx.x;
  if (status[bat]) return;
  const double* __restrict__ H = H_all + (size_t)bat * N * N;
  const double* __restrict__ g = g_all + (size_t)bat * N;
  double bb[kCgPer], xs[kCgPer], ri[kCgPer], pp[kCgPer], ap[kCgPer];
  double v = 0.0, d = 0.0;
#pragma unroll
  for (int q = 0; q < kCgPer; ++q) {
    const int i = threadIdx.x + kCgThreads * q;
    const double gi = i < N ? g[i] : 0.0;
    bb[q] = -gi;
    xs[q] = 0.0;
    ri[q] = gi;
    pp[q] = -gi;
    v += fabs(gi);
    d = fma(gi, gi, d);
  }
  const double maggrad = nr_block_sum(v, red);
  double dri0 = nr_block_sum(d, red);
  const double termcond = fmin(0.5, sqrt(maggrad)) * maggrad;
  const int cg_maxiter = 20 * N;
  int it = 0, flag = 3;
  for (int k2 = 0; k2 < cg_maxiter; ++k2) {
    v = 0.0;
#pragma unroll
    for (int q = 0; q < kCgPer; ++q) v += fabs(ri[q]);
    if (nr_block_sum(v, red) <= termcond) {
      flag = 0;
      break;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kCgPer; ++q) {
      const int i = threadIdx.x + kCgThreads * q;
      if (i < N) ps[i] = pp[q];
      ap[q] = 0.0;
    }
    __syncthreads();
    for (int j = 0; j < N; ++j) {
      const double pj = ps[j];
      const double* row = H + (size_t)j * N;
#pragma unroll
      for (int q = 0; q < kCgPer; ++q) {
        const int i = threadIdx.x + kCgThreads * q;
        if (i < N) ap[q] = fma(row[i], pj, ap[q]);
      }
    }
    v = 0.0;
#pragma unroll
    for (int q = 0; q < kCgPer; ++q) v = fma(pp[q], ap[q], v);
    const double curv = nr_block_sum(v, red);
    if (curv >= 0.0 && curv <= 3.0 * DBL_EPSILON) {
      flag = 0;
      break;
    }
    if (curv < 0.0) {
      if (it == 0) {
        const double s = dri0 / (-curv);
#pragma unroll
        for (int q = 0; q < kCgPer; ++q) xs[q] = s * bb[q];
      }
      flag = 0;
      break;
    }
    if (!(curv > 0.0)) break;  // not a number: the passes would run out
    const double alphai = dri0 / curv;
    d = 0.0;
#pragma unroll
    for (int q = 0; q < kCgPer; ++q) {
      xs[q] += alphai * pp[q];
      ri[q] += alphai * ap[q];
      d = fma(ri[q], ri[q], d);
    }
    const double dri1 = nr_block_sum(d, red);
    const double betai = dri1 / dri0;
#pragma unroll
    for (int q = 0; q < kCgPer; ++q) pp[q] = -ri[q] + betai * pp[q];
    ++it;
    dri0 = dri1;
  }
#pragma unroll
  for (int q = 0; q < kCgPer; ++q) {
    const int i = threadIdx.x + kCgThreads * q;
    if (i < N) p_out[(size_t)bat * N + i] = xs[q];
  }
  if (threadIdx.x == 0) {
    info[2 * bat] = it;
    info[2 * bat + 1] = flag;
  }
}

bool nr_sizes_ok(int ndelay, int nchan) { return ndelay >= 1 && ndelay <= kNrMaxDelay && nchan >= 1 && nchan <= kNrMaxChan; }

bool nr_ws_ok(const dmm_nrml_ws* w) {
  return w && w->chan && w->tw && w->wv && w->Nm && w->Xe && w->nsv && w->Ci && w->S && w->sh && w->G && w->D && w->U && w->Y && w->R && w->t && w->cix;
}

}  // namespace

extern "C" {

int dmm_nrml_start(dmm_ctx* ctx, int ndelay, int nchan, int nsample, int nbase, const int32_t* chan, const double* win, const double* Xp, const double* Xd, const uint8_t* nzt, const int32_t* status, double* work,
                   double* F2, double* Z, double* tw, double* wv, double* Nm, double* Xe, double* nsv, double* S0) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nrml_start: ctx is NULL");
  DMM_REQUIRE(nr_sizes_ok(ndelay, nchan), "dmm_nrml_start: %d delays, %d channels outside 1 ... %d, 1 ... %d", ndelay, nchan, kNrMaxDelay, kNrMaxChan);
  DMM_REQUIRE(nsample >= 1 && nsample <= 65535, "dmm_nrml_start: bad sample count %d", nsample);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_nrml_start: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(chan && win && Xp && Xd && nzt && status && work && F2 && Z && tw && wv && Nm && Xe && nsv && S0, "dmm_nrml_start: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int N = ndelay, n = nchan, K = 2 * n;
  hipLaunchKernelGGL(k_nrml_tw, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, N, (double2*)tw);
  hipLaunchKernelGGL(k_nrml_split, dim3((unsigned)nbase), dim3(256), 0, ctx->stream, n, nsample, win, Xp, Xd, nzt, status, work, wv, Nm, nsv);
  for (int part = 0; part < 2; ++part) {  // emb(X) ns = W^T W + W2^T W2
    DlGemm g{};
    const double* W = work + (size_t)part * nsample * K;
    g.A = W, g.a_rs = 1, g.a_cs = K, g.a_bs = (int64_t)3 * nsample * K;
    g.B = W, g.b_rs = K, g.b_cs = 1, g.b_bs = g.a_bs;
    g.C = Xe, g.c_rs = K, g.c_bs = (int64_t)K * K;
    g.M = K, g.N = K, g.K = nsample;
    g.alpha = 1.0, g.beta = part, g.upper = 0;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
  const int64_t kk = (int64_t)K * K;
  hipLaunchKernelGGL(k_nrml_scale, dim3((unsigned)((kk + 255) / 256), (unsigned)nbase), dim3(256), 0, ctx->stream, kk, (const double*)nsv, status, Xe);
  // the starting point: the unwindowed data of the channels above the pseudo-inverse cut, projected on exp(+i theta)
  int rc = dmm_delay_fourier(ctx, N, n, 1, chan, F2);
  if (rc) return rc;
  {
    DlGemm g{};
    g.A = work + (size_t)2 * nsample * K, g.a_rs = K, g.a_cs = 1, g.a_bs = (int64_t)3 * nsample * K;
    g.B = F2, g.b_rs = 2 * N, g.b_cs = 1, g.b_bs = 0;
    g.C = Z, g.c_rs = 2 * N, g.c_bs = (int64_t)nsample * 2 * N;
    g.M = nsample, g.N = 2 * N, g.K = K;
    g.alpha = 1.0, g.beta = 0, g.upper = 0;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
  hipLaunchKernelGGL(k_nrml_var, dim3((unsigned)((N + 255) / 256), (unsigned)nbase), dim3(256), 0, ctx->stream, N, nsample, (const double*)Z, nzt, (const double*)nsv, status, S0);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_nrml_eval(dmm_ctx* ctx, int ndelay, int nchan, int nbase, const dmm_nrml_ws* ws, const double* x, double lo, double hi, int32_t* status, double* value, double* grad) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nrml_eval: ctx is NULL");
  DMM_REQUIRE(nr_sizes_ok(ndelay, nchan), "dmm_nrml_eval: %d delays, %d channels outside 1 ... %d, 1 ... %d", ndelay, nchan, kNrMaxDelay, kNrMaxChan);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_nrml_eval: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(nr_ws_ok(ws) && x && status && value && grad, "dmm_nrml_eval: NULL argument");
  DMM_REQUIRE(lo <= hi, "dmm_nrml_eval: bad bounds");
  DMM_HIP(hipSetDevice(ctx->device));
  const int N = ndelay, n = nchan, K = 2 * n;
  const unsigned nb = (unsigned)nbase;
  const int64_t kk = (int64_t)K * K, rows = (int64_t)(N + n) * K;
  hipLaunchKernelGGL(k_nrml_exp, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, ctx->stream, N, x, lo, hi, (const int32_t*)status, ws->S);
  hipLaunchKernelGGL(k_nrml_spec, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, ctx->stream, N, (const double2*)ws->tw, (const double*)ws->S, (const int32_t*)status, (double2*)ws->sh);
  hipLaunchKernelGGL(k_nrml_fill, dim3((unsigned)((kk + 255) / 256), nb), dim3(256), 0, ctx->stream, N, n, ws->chan, ws->wv, ws->Nm, ws->Xe, (const double2*)ws->sh, (const int32_t*)status, ws->G,
                     ws->D);
  hipLaunchKernelGGL(k_nrml_rows, dim3((unsigned)((rows + 255) / 256), nb), dim3(256), 0, ctx->stream, N, n, ws->chan, (const double2*)ws->tw, ws->wv, (const double*)ws->S, ws->Xe,
                     (const int32_t*)status, ws->U, ws->Y);
  dl_factor(ctx, K, nbase, ws->G, status, DMM_DELAY_NOT_POSDEF);
  dl_solve_rows(ctx, K, N + n, N + n, nbase, ws->G, ws->Y, status);
  {
    DlGemm g{};  // R rows = Ut rows times emb(X - C) (symmetric)
    g.A = ws->Y, g.a_rs = K, g.a_cs = 1, g.a_bs = (int64_t)(N + n) * K;
    g.B = ws->D, g.b_rs = K, g.b_cs = 1, g.b_bs = kk;
    g.C = ws->R, g.c_rs = K, g.c_bs = (int64_t)N * K;
    g.M = N, g.N = K, g.K = K;
    g.alpha = 1.0, g.beta = 0, g.upper = 0;
    g.status = status;
    dl_gemm(ctx, g, nbase);
  }
  hipLaunchKernelGGL(k_nrml_grad, dim3((unsigned)((N + 3) / 4), nb), dim3(256), 0, ctx->stream, N, n, (const double*)ws->Y, (const double*)ws->R, ws->Ci, x, ws->nsv, (const int32_t*)status, ws->t,
                     ws->cix, grad);
  hipLaunchKernelGGL(k_nrml_value, dim3(nb), dim3(256), 0, ctx->stream, N, n, (const double*)ws->G, (const double*)ws->Y, x, (const double*)ws->cix, ws->nsv, (const int32_t*)status, value);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_nrml_hessian(dmm_ctx* ctx, int ndelay, int nchan, int nbase, const dmm_nrml_ws* ws, int exact, const int32_t* status, double* H) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nrml_hessian: ctx is NULL");
  DMM_REQUIRE(nr_sizes_ok(ndelay, nchan), "dmm_nrml_hessian: %d delays, %d channels outside 1 ... %d, 1 ... %d", ndelay, nchan, kNrMaxDelay, kNrMaxChan);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_nrml_hessian: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(nr_ws_ok(ws) && ws->PQ && status && H, "dmm_nrml_hessian: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  const int N = ndelay, n = nchan, K = 2 * n;
  NrHess h{};
  h.t = ws->t, h.Ci = ws->Ci, h.nsv = ws->nsv, h.status = status, h.H = H;
  h.N = N, h.exact = exact ? 1 : 0;
  {
    const int64_t nn = (int64_t)N * N;
    for (int plane = 0; plane < 4; ++plane) {  // Re P = U Y^T, Im P = U J(Y)^T, Re Q = Y R^T, Im Q = Y J(R)^T
      const double* A = plane < 2 ? ws->U : ws->Y;
      const double* B = plane < 2 ? ws->Y : ws->R;
      const int64_t a_bs = (int64_t)(plane < 2 ? N : N + n) * K, b_bs = (int64_t)(plane < 2 ? N + n : N) * K;
      for (int half = 0; half < (plane & 1 ? 2 : 1); ++half) {
        DlGemm g{};
        g.a_rs = K, g.a_cs = 1, g.a_bs = a_bs;
        g.b_rs = 1, g.b_cs = K, g.b_bs = b_bs;
        g.C = ws->PQ + (size_t)plane * nn, g.c_rs = N, g.c_bs = 4 * nn;
        g.M = N, g.N = N;
        g.upper = 0, g.status = status;
        if (plane & 1) {  // sum_{k < n} A[k] B[k + n] - sum_{k < n} A[k + n] B[k]
          g.A = A + (half ? n : 0), g.B = B + (half ? 0 : n), g.K = n;
          g.alpha = half ? -1.0 : 1.0, g.beta = half;
        } else {
          g.A = A, g.B = B, g.K = K;
          g.alpha = 1.0, g.beta = 0;
        }
        dl_gemm(ctx, g, nbase);
      }
    }
    hipLaunchKernelGGL(k_nrml_hess_ew, dim3((unsigned)((nn + 255) / 256), (unsigned)nbase), dim3(256), 0, ctx->stream, h, (const double*)ws->PQ);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_nrml_direction(dmm_ctx* ctx, int ndelay, int nbase, const double* H, const double* g, const int32_t* status, double* p, int32_t* info) {
  DMM_REQUIRE(ctx != nullptr, "dmm_nrml_direction: ctx is NULL");
  DMM_REQUIRE(ndelay >= 1 && ndelay <= kNrMaxDelay, "dmm_nrml_direction: %d delays outside 1 ... %d", ndelay, kNrMaxDelay);
  DMM_REQUIRE(nbase >= 0 && nbase <= 65535, "dmm_nrml_direction: bad baseline count %d", nbase);
  if (nbase == 0) return DMM_OK;
  DMM_REQUIRE(H && g && status && p && info, "dmm_nrml_direction: NULL argument");
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_nrml_cg, dim3((unsigned)nbase), dim3(kCgThreads), 0, ctx->stream, ndelay, H, g, status, p, info);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
