// Sidereal regridding (banded Wiener solve of the inverse Lanczos problem) and day stacking.
//
// Reference: draco/util/regrid.py:14-89 (band_wiener), draco/analysis/transform.py:951-986 (LanczosRegridder._regrid),
// draco/analysis/sidereal.py:221-234, 256-278 (mix-down / mix-up), :933-1030 (SiderealStacker).
//
// Per row k (one (frequency, stack) pair), with R [ngrid, nt] the Lanczos matrix of the padded grid:
//   d = R (Ni_k o y_k),  C = band_bw(R diag(Ni_k) R^T),  nw = diag(C),  x = (C + eps I)^-1 d.
// R depends on the times only and is shared by every row, so the control flow of a row's solve is the same for all
// rows: one LANE per row, 64 rows per wave (k_regrid).  The kernel walks the grid points in groups whose time samples
// fit an LDS tile [sample][row] (loaded row by row, so the global reads are contiguous); per grid point it gathers the
// bw + 1 band entries and the right-hand side in float64, takes one step of the banded Cholesky factorisation and of
// the forward substitution with the bw x bw window of the factor in registers, and writes the factor row, z and the
// weight to a scratch laid out [grid point][entry][row] (every store and load of it is one contiguous 512-byte line
// per entry).  The back substitution reads the scratch in descending order and leaves through an LDS tile, so the
// output stores are contiguous as well.  Nothing crosses lanes.
#include "dmm_internal.h"

#include <string.h>

#include <algorithm>

namespace {

constexpr int kRows = 64;           // rows per wave (= per block)
constexpr int kRowPad = kRows + 1;  // LDS row pitch: the transposing accesses hit distinct banks
constexpr int kOutTile = 64;        // grid points per output tile
constexpr int kMaxLds = 160 * 1024;
constexpr int kMaxKernelWidth = 6;

struct RegridGroup {
  int g0, g1;  // grid points [g0, g1)
  int j0, j1;  // time samples [j0, j1) they read
};

}  // namespace

struct dmm_regrid_plan {
  dmm_ctx* ctx = nullptr;
  int nt = 0, ngrid = 0, bw = 0, tile = 0, ngroup = 0;
  int32_t* start_d = nullptr;  // [ngrid] first sample of each grid point's span
  int32_t* end_d = nullptr;    // [ngrid] one past its last
  int64_t* off_d = nullptr;    // [ngrid] offset of its kernel values in tab_d
  double* tab_d = nullptr;     // per grid point g, per sample j of its span: R[g - k][j], k = 0 .. bw
  RegridGroup* group_d = nullptr;
};

namespace {

struct RegridArgs {
  const float2* vis;
  const float* weight;
  float2* out_vis;
  float* out_weight;
  const int32_t* start;
  const int32_t* end;
  const int64_t* off;
  const double* tab;
  const RegridGroup* group;
  double* scratch;
  const double* omega;     // [nrow] fringe rate of each row (NULL: no mixing)
  const float* mask;       // [nrow] feed mask of each row
  const double* dphi_in;   // [nt] sidereal angle of the input samples
  const double* dphi_out;  // [samples] ... of the output grid
  double eps;
  int64_t row0, nrow;
  int nt, ngrid, ngroup, pad, samples, tile, mask_zero_weight;
};

// One wave = 64 rows.  LDS: the input tile (3 floats per sample and row) and, in the second half of the kernel, the
// output tile (complex64 + float per grid point and row) share the dynamic allocation.
template <int KW>
__global__ __launch_bounds__(kRows) void k_regrid(RegridArgs a) {
  constexpr int BW = 2 * KW - 1;
  constexpr int NE = BW + 4;  // scratch entries per grid point: l[1..BW], 1 / l[0], z.re, z.im, nw
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int64_t rbase = a.row0 + (int64_t)blockIdx.x * kRows;
  const int64_t row = rbase + lane;
  const int nvalid = (int)min((int64_t)kRows, a.nrow - rbase);
  double* __restrict__ sc = a.scratch + (size_t)blockIdx.x * a.ngrid * NE * kRows + lane;
  float* tw = lds;
  float* tr = lds + (size_t)a.tile * kRowPad;
  float* ti = lds + (size_t)2 * a.tile * kRowPad;

  double win[BW][BW];  // win[i][t] = L[g-1-i][g-1-i-(t+1)]: the rows of the factor the next step still reads
  double invd[BW];     // invd[i] = 1 / L[g-1-i][g-1-i]
  double zr[BW], zi[BW];
#pragma unroll
  for (int i = 0; i < BW; ++i) {
    invd[i] = 0.0;
    zr[i] = zi[i] = 0.0;
#pragma unroll
    for (int t = 0; t < BW; ++t) win[i][t] = 0.0;
  }
  bool any = false;

  for (int gi = 0; gi < a.ngroup; ++gi) {
    const RegridGroup G = a.group[gi];
    const int nj = G.j1 - G.j0;
    __syncthreads();
    // ---- stage the group's samples: row by row, lanes along time
    for (int r = 0; r < kRows; ++r) {
      const bool live = r < nvalid;
      const int64_t base = (rbase + r) * a.nt + G.j0;
      double om = 0.0;
      float mk = 1.f;
      if (a.omega && live) {
        om = a.omega[rbase + r];
        mk = a.mask[rbase + r];
      }
      for (int jj = lane; jj < nj; jj += kRows) {
        float w = 0.f;
        float2 y = make_float2(0.f, 0.f);
        if (live) {
          w = a.weight[base + jj];
          y = a.vis[base + jj];
          if (a.omega) {  // mix down: y *= mask exp(-i omega dphi), rounded to complex64 like the reference's in-place product
            double s, c;
            sincos(om * a.dphi_in[G.j0 + jj], &s, &c);
            const double pr = (double)mk * c, pi = -(double)mk * s;
            const double yr = (double)y.x * pr - (double)y.y * pi, yi = (double)y.x * pi + (double)y.y * pr;
            y = make_float2((float)yr, (float)yi);
          }
        }
        tw[jj * kRowPad + r] = w;
        tr[jj * kRowPad + r] = y.x;
        ti[jj * kRowPad + r] = y.y;
      }
    }
    __syncthreads();

    for (int g = G.g0; g < G.g1; ++g) {
      // ---- gather: c[k] = sum_j R[g][j] R[g-k][j] w_j,  d = sum_j R[g][j] w_j y_j
      double c[BW + 1];
#pragma unroll
      for (int k = 0; k <= BW; ++k) c[k] = 0.0;
      double dr = 0.0, di = 0.0;
      const int s = a.start[g], e = a.end[g];
      const double* __restrict__ tp = a.tab + a.off[g];
      for (int j = s; j < e; ++j, tp += BW + 1) {
        const int q = (j - G.j0) * kRowPad + lane;
        const float wf = tw[q];
        any = any || (wf != 0.f);
        const double t = tp[0] * (double)wf;
        dr = fma(t, (double)tr[q], dr);
        di = fma(t, (double)ti[q], di);
#pragma unroll
        for (int k = 0; k <= BW; ++k) c[k] = fma(tp[k], t, c[k]);
      }
      // ---- one row of the banded Cholesky factor of C + eps I, and of the forward substitution
      double l[BW + 1];
#pragma unroll
      for (int k = BW; k >= 1; --k) {
        double acc = c[k];
#pragma unroll
        for (int q = k + 1; q <= BW; ++q) acc = fma(-l[q], win[k - 1][q - k - 1], acc);
        l[k] = acc * invd[k - 1];
      }
      double dd = c[0] + a.eps;
#pragma unroll
      for (int q = 1; q <= BW; ++q) dd = fma(-l[q], l[q], dd);
      if (!(dd > 0.0)) dd = a.eps;  // C + eps I is positive definite: only rounding can bring a pivot here
      const double id0 = 1.0 / sqrt(dd);
      double ar = dr, ai = di;
#pragma unroll
      for (int q = 1; q <= BW; ++q) {
        ar = fma(-l[q], zr[q - 1], ar);
        ai = fma(-l[q], zi[q - 1], ai);
      }
      ar *= id0;
      ai *= id0;
      double* __restrict__ o = sc + (size_t)g * NE * kRows;
#pragma unroll
      for (int q = 1; q <= BW; ++q) o[(q - 1) * kRows] = l[q];
      o[BW * kRows] = id0;
      o[(BW + 1) * kRows] = ar;
      o[(BW + 2) * kRows] = ai;
      o[(BW + 3) * kRows] = c[0];
      // ---- slide the window: row g becomes the newest
#pragma unroll
      for (int i = BW - 1; i >= 1; --i) {
        invd[i] = invd[i - 1];
        zr[i] = zr[i - 1];
        zi[i] = zi[i - 1];
#pragma unroll
        for (int t = 0; t < BW - 1 - i; ++t) win[i][t] = win[i - 1][t];
      }
      invd[0] = id0;
      zr[0] = ar;
      zi[0] = ai;
#pragma unroll
      for (int t = 0; t < BW - 1; ++t) win[0][t] = l[t + 1];
    }
  }

  // ---- back substitution L^T x = z, grid points descending; the kept ones leave through an LDS tile
  __syncthreads();
  float2* ov = (float2*)lds;
  float* ow = lds + 2 * kOutTile * kRowPad;
  double pr[BW + 1], pi[BW + 1];  // pr[k]: what the rows solved so far contribute to grid point g - k
#pragma unroll
  for (int k = 0; k <= BW; ++k) pr[k] = pi[k] = 0.0;
  double om = 0.0;
  float mk = 1.f;
  if (a.omega && lane < nvalid) {
    om = a.omega[row];
    mk = a.mask[row];
  }
  const bool keep_w = mk != 0.f && (!a.mask_zero_weight || any);
  for (int g = a.ngrid - 1; g >= a.pad; --g) {
    const double* __restrict__ o = sc + (size_t)g * NE * kRows;
    const double id0 = o[BW * kRows];
    const double xr = (o[(BW + 1) * kRows] - pr[0]) * id0;
    const double xi = (o[(BW + 2) * kRows] - pi[0]) * id0;
#pragma unroll
    for (int k = 1; k <= BW; ++k) {
      const double lk = o[(k - 1) * kRows];
      pr[k - 1] = fma(lk, xr, pr[k]);
      pi[k - 1] = fma(lk, xi, pi[k]);
    }
    pr[BW] = pi[BW] = 0.0;
    const int go = g - a.pad;
    if (go < a.samples) {
      double vr = xr, vi = xi;
      if (a.omega) {  // mix up: x *= conj(mask exp(-i omega dphi))
        double s, c;
        sincos(om * a.dphi_out[go], &s, &c);
        const double qr = (double)mk * c, qi = (double)mk * s;
        vr = xr * qr - xi * qi;
        vi = xr * qi + xi * qr;
      }
      const int slot = go % kOutTile;
      ov[slot * kRowPad + lane] = make_float2((float)vr, (float)vi);
      ow[slot * kRowPad + lane] = keep_w ? (float)o[(BW + 3) * kRows] : 0.f;
      if (slot == 0) {  // the tile [go, go + n) is complete
        const int n = min(kOutTile, a.samples - go);
        __syncthreads();
        for (int r = 0; r < nvalid; ++r) {
          if (lane < n) {
            a.out_vis[(rbase + r) * a.samples + go + lane] = ov[lane * kRowPad + r];
            a.out_weight[(rbase + r) * a.samples + go + lane] = ow[lane * kRowPad + r];
          }
        }
        __syncthreads();
      }
    }
  }
}

// West's update of the running mean and of the sum of squared differences, one element per thread
// (sidereal.py:960-1030); float32 state and float32 operations in the reference's order (no contraction).
#pragma clang fp contract(off)
__device__ __forceinline__ float inv_no_zero(float x) { return x != 0.f ? 1.f / x : 0.f; }

__global__ void k_stack_add(int mode, int with_var, const float2* __restrict__ dvis, const float* __restrict__ dw, const uint16_t* __restrict__ dns, float2* svis, float* sw,
                            uint16_t* sns, float* scsq, float* svar, int64_t n) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = dw[i];
  const uint16_t count = dns ? (uint16_t)(dns[i] * (w > 0.f ? 1 : 0)) : (uint16_t)(w > 0.f ? 1 : 0);
  const uint16_t ns = (uint16_t)(sns[i] + count);
  sns[i] = ns;
  float coeff, sum_coeff;
  if (mode == 0) {  // uniform
    coeff = (float)count;
    sw[i] = sw[i] + (coeff * coeff) * inv_no_zero(w);
    sum_coeff = (float)ns;
  } else {
    coeff = w;
    sum_coeff = sw[i] + w;
    sw[i] = sum_coeff;
  }
  const float2 v = dvis[i];
  float2 m = svis[i];
  const float dbr = coeff * (v.x - m.x), dbi = coeff * (v.y - m.y);
  if (mode == 0) {  // the reference inverts the integer count in float64 and rounds the updated mean once
    const double isc = ns != 0 ? 1.0 / (double)ns : 0.0;
    m.x = (float)((double)m.x + (double)dbr * isc);
    m.y = (float)((double)m.y + (double)dbi * isc);
  } else {
    const float isc = inv_no_zero(sum_coeff);
    m.x = m.x + dbr * isc;
    m.y = m.y + dbi * isc;
  }
  svis[i] = m;
  if (with_var) {
    scsq[i] = scsq[i] + coeff * coeff;
    const float dar = v.x - m.x, dai = v.y - m.y;
    svar[i] = svar[i] + dbr * dar;
    svar[n + i] = svar[n + i] + dbr * dai;
    svar[2 * n + i] = svar[2 * n + i] + dbi * dai;
  }
}

__global__ void k_stack_finish(int mode, int with_var, float* sw, const uint16_t* __restrict__ sns, const float* __restrict__ scsq, float* svar, int64_t n) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint16_t ns = sns[i];
  float norm;
  if (mode == 0) {
    norm = (float)ns;
    sw[i] = inv_no_zero(sw[i]) * (norm * norm);
  } else {
    norm = sw[i];
  }
  if (with_var) {
    norm = norm - scsq[i] * inv_no_zero(norm);  // Bessel's correction
    const float f = ns > 1 ? inv_no_zero(norm) : 0.f;
    svar[i] = svar[i] * f;
    svar[n + i] = svar[n + i] * f;
    svar[2 * n + i] = svar[2 * n + i] * f;
  }
}

template <int KW>
int launch_regrid(dmm_ctx* ctx, const RegridArgs& a0, int64_t nrow, size_t lds) {
  constexpr int NE = 2 * KW - 1 + 4;
  const size_t per_wave = (size_t)a0.ngrid * NE * kRows * sizeof(double);
  const int64_t nwave = (nrow + kRows - 1) / kRows;
  const size_t budget = (size_t)(ctx->opt_regrid_ws_mib > 0 ? ctx->opt_regrid_ws_mib : 12288) << 20;
  int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / per_wave));
  chunk = std::min(chunk, nwave);
  void* scratch = nullptr;
  int rc = dmm_get_scratch(ctx, (size_t)chunk * per_wave, &scratch);
  if (rc) return rc;
  auto k = k_regrid<KW>;
  DMM_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t w0 = 0; w0 < nwave; w0 += chunk) {
    RegridArgs a = a0;
    a.scratch = (double*)scratch;
    a.row0 = w0 * kRows;
    a.nrow = nrow;
    const int64_t nb = std::min(chunk, nwave - w0);
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(kRows), lds, ctx->stream, a);
  }
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // namespace

extern "C" {

int dmm_regrid_plan_create(dmm_ctx* ctx, int nt, int ngrid, int kernel_width, const int32_t* span_start, const int32_t* span_end, const double* kernel_values,
                           dmm_regrid_plan** plan) {
  DMM_REQUIRE(ctx != nullptr, "dmm_regrid_plan_create: ctx is NULL");
  DMM_REQUIRE(span_start && span_end && kernel_values && plan, "dmm_regrid_plan_create: NULL argument");
  DMM_REQUIRE(nt >= 1 && ngrid >= 1, "dmm_regrid_plan_create: bad sizes nt=%d ngrid=%d", nt, ngrid);
  DMM_REQUIRE(kernel_width >= 1 && kernel_width <= kMaxKernelWidth, "dmm_regrid_plan_create: kernel_width %d outside 1 ... %d", kernel_width, kMaxKernelWidth);
  const int bw = 2 * kernel_width - 1;
  std::vector<int64_t> voff(ngrid + 1, 0);
  int maxspan = 0;
  for (int g = 0; g < ngrid; ++g) {
    DMM_REQUIRE(span_start[g] >= 0 && span_start[g] <= span_end[g] && span_end[g] <= nt, "dmm_regrid_plan_create: span of grid point %d is not inside [0, nt]", g);
    voff[g + 1] = voff[g] + (span_end[g] - span_start[g]);
    maxspan = std::max(maxspan, span_end[g] - span_start[g]);
  }
  // LDS tile: room for the longest span twice over, at least 64 samples, at most what the CU has
  const int tile_max = kMaxLds / (3 * kRowPad * (int)sizeof(float));
  if (maxspan > tile_max)
    return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_regrid_plan_create: a grid point reads %d samples, the LDS tile holds %d", maxspan, tile_max);
  const int tile = std::min(tile_max, std::max(2 * maxspan, 64));
  // expanded table: for grid point g and sample j of its span, R[g - k][j] for k = 0 .. bw (0 outside that row's span)
  std::vector<int64_t> off(ngrid);
  std::vector<double> tab((size_t)voff[ngrid] * (bw + 1));
  for (int g = 0; g < ngrid; ++g) {
    off[g] = voff[g] * (bw + 1);
    for (int j = span_start[g]; j < span_end[g]; ++j)
      for (int k = 0; k <= bw; ++k) {
        const int gp = g - k;
        double v = 0.0;
        if (gp >= 0 && j >= span_start[gp] && j < span_end[gp]) v = kernel_values[voff[gp] + (j - span_start[gp])];
        tab[off[g] + (size_t)(j - span_start[g]) * (bw + 1) + k] = v;
      }
  }
  // groups of consecutive grid points whose samples fit the tile
  std::vector<RegridGroup> groups;
  for (int g = 0; g < ngrid;) {
    RegridGroup G{g, g, 0, 0};
    bool have = false;
    while (G.g1 < ngrid) {
      const int s = span_start[G.g1], e = span_end[G.g1];
      if (e > s) {
        const int j0 = have ? std::min(G.j0, s) : s, j1 = have ? std::max(G.j1, e) : e;
        if (j1 - j0 > tile) break;
        G.j0 = j0;
        G.j1 = j1;
        have = true;
      }
      ++G.g1;
    }
    groups.push_back(G);
    g = G.g1;
  }
  DMM_HIP(hipSetDevice(ctx->device));
  dmm_regrid_plan* p = new dmm_regrid_plan;
  p->ctx = ctx;
  p->nt = nt;
  p->ngrid = ngrid;
  p->bw = bw;
  p->tile = tile;
  p->ngroup = (int)groups.size();
  hipError_t e = hipMalloc((void**)&p->start_d, sizeof(int32_t) * ngrid);
  if (e == hipSuccess) e = hipMalloc((void**)&p->end_d, sizeof(int32_t) * ngrid);
  if (e == hipSuccess) e = hipMalloc((void**)&p->off_d, sizeof(int64_t) * ngrid);
  if (e == hipSuccess) e = hipMalloc((void**)&p->tab_d, sizeof(double) * std::max<size_t>(tab.size(), 1));
  if (e == hipSuccess) e = hipMalloc((void**)&p->group_d, sizeof(RegridGroup) * groups.size());
  if (e == hipSuccess) e = hipMemcpy(p->start_d, span_start, sizeof(int32_t) * ngrid, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->end_d, span_end, sizeof(int32_t) * ngrid, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->off_d, off.data(), sizeof(int64_t) * ngrid, hipMemcpyHostToDevice);
  if (e == hipSuccess && !tab.empty()) e = hipMemcpy(p->tab_d, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->group_d, groups.data(), sizeof(RegridGroup) * groups.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dmm_regrid_plan_destroy(p);
    return dmm_set_error((int)e, "dmm_regrid_plan_create: %s", hipGetErrorString(e));
  }
  *plan = p;
  return DMM_OK;
}

int dmm_regrid_plan_destroy(dmm_regrid_plan* plan) {
  if (!plan) return DMM_OK;
  (void)hipFree(plan->start_d);
  (void)hipFree(plan->end_d);
  (void)hipFree(plan->off_d);
  (void)hipFree(plan->tab_d);
  (void)hipFree(plan->group_d);
  delete plan;
  return DMM_OK;
}

int dmm_regrid_band_wiener(dmm_ctx* ctx, const dmm_regrid_plan* plan, const void* vis, const float* weight, int64_t nrow, double eps, int pad, int samples,
                           int mask_zero_weight, const double* omega, const float* feed_mask, const double* dphi_in, const double* dphi_out, void* out_vis,
                           float* out_weight) {
  DMM_REQUIRE(ctx != nullptr, "dmm_regrid_band_wiener: ctx is NULL");
  DMM_REQUIRE(plan != nullptr, "dmm_regrid_band_wiener: plan is NULL");
  DMM_REQUIRE(nrow >= 0, "dmm_regrid_band_wiener: bad nrow %lld", (long long)nrow);
  if (nrow == 0) return DMM_OK;
  DMM_REQUIRE(vis && weight && out_vis && out_weight, "dmm_regrid_band_wiener: NULL argument");
  DMM_REQUIRE(plan->ctx == ctx, "dmm_regrid_band_wiener: the plan belongs to another context");
  DMM_REQUIRE(eps > 0.0, "dmm_regrid_band_wiener: eps %g must be positive", eps);
  DMM_REQUIRE(pad >= 0 && samples >= 1 && (int64_t)samples + 2 * (int64_t)pad == plan->ngrid, "dmm_regrid_band_wiener: samples %d + 2 pad %d != ngrid %d of the plan", samples,
              pad, plan->ngrid);
  DMM_REQUIRE(nrow <= ((int64_t)1 << 31) * kRows / 2, "dmm_regrid_band_wiener: nrow %lld does not fit the grid", (long long)nrow);
  const bool mix = omega || feed_mask || dphi_in || dphi_out;
  DMM_REQUIRE(!mix || (omega && feed_mask && dphi_in && dphi_out), "dmm_regrid_band_wiener: the mixing arrays come all four or not at all");
  DMM_HIP(hipSetDevice(ctx->device));
  RegridArgs a{};
  a.vis = (const float2*)vis;
  a.weight = weight;
  a.out_vis = (float2*)out_vis;
  a.out_weight = out_weight;
  a.start = plan->start_d;
  a.end = plan->end_d;
  a.off = plan->off_d;
  a.tab = plan->tab_d;
  a.group = plan->group_d;
  a.omega = omega;
  a.mask = feed_mask;
  a.dphi_in = dphi_in;
  a.dphi_out = dphi_out;
  a.eps = eps;
  a.nt = plan->nt;
  a.ngrid = plan->ngrid;
  a.ngroup = plan->ngroup;
  a.pad = pad;
  a.samples = samples;
  a.tile = plan->tile;
  a.mask_zero_weight = mask_zero_weight ? 1 : 0;
  const size_t lds = sizeof(float) * kRowPad * (size_t)std::max(3 * plan->tile, 3 * kOutTile);
  switch ((plan->bw + 1) / 2) {
    case 1: return launch_regrid<1>(ctx, a, nrow, lds);
    case 2: return launch_regrid<2>(ctx, a, nrow, lds);
    case 3: return launch_regrid<3>(ctx, a, nrow, lds);
    case 4: return launch_regrid<4>(ctx, a, nrow, lds);
    case 5: return launch_regrid<5>(ctx, a, nrow, lds);
    case 6: return launch_regrid<6>(ctx, a, nrow, lds);
  }
  return dmm_set_error(DMM_E_UNSUPPORTED, "dmm_regrid_band_wiener: kernel width %d", (plan->bw + 1) / 2);
}

int dmm_sidereal_stack_add(dmm_ctx* ctx, int mode, int with_variance, const void* day_vis, const float* day_weight, const uint16_t* day_nsample, void* stack_vis,
                           float* stack_weight, uint16_t* stack_nsample, float* sum_coeff_sq, float* sample_variance, int64_t n) {
  DMM_REQUIRE(ctx != nullptr, "dmm_sidereal_stack_add: ctx is NULL");
  DMM_REQUIRE(n >= 0, "dmm_sidereal_stack_add: bad n %lld", (long long)n);
  DMM_REQUIRE(mode == DMM_STACK_UNIFORM || mode == DMM_STACK_INVERSE_VARIANCE, "dmm_sidereal_stack_add: bad mode %d", mode);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(day_vis && day_weight && stack_vis && stack_weight && stack_nsample, "dmm_sidereal_stack_add: NULL argument");
  DMM_REQUIRE(!with_variance || (sum_coeff_sq && sample_variance), "dmm_sidereal_stack_add: NULL argument (with_variance needs sum_coeff_sq and sample_variance)");
  DMM_REQUIRE(n <= (int64_t)0x7fffffff * 256, "dmm_sidereal_stack_add: n %lld does not fit the grid", (long long)n);
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_stack_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mode, with_variance ? 1 : 0, (const float2*)day_vis, day_weight, day_nsample,
                     (float2*)stack_vis, stack_weight, stack_nsample, sum_coeff_sq, sample_variance, n);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_sidereal_stack_finish(dmm_ctx* ctx, int mode, int with_variance, float* stack_weight, const uint16_t* stack_nsample, const float* sum_coeff_sq,
                              float* sample_variance, int64_t n) {
  DMM_REQUIRE(ctx != nullptr, "dmm_sidereal_stack_finish: ctx is NULL");
  DMM_REQUIRE(n >= 0, "dmm_sidereal_stack_finish: bad n %lld", (long long)n);
  DMM_REQUIRE(mode == DMM_STACK_UNIFORM || mode == DMM_STACK_INVERSE_VARIANCE, "dmm_sidereal_stack_finish: bad mode %d", mode);
  if (n == 0) return DMM_OK;
  DMM_REQUIRE(stack_weight && stack_nsample, "dmm_sidereal_stack_finish: NULL argument");
  DMM_REQUIRE(!with_variance || (sum_coeff_sq && sample_variance), "dmm_sidereal_stack_finish: NULL argument (with_variance needs sum_coeff_sq and sample_variance)");
  DMM_REQUIRE(n <= (int64_t)0x7fffffff * 256, "dmm_sidereal_stack_finish: n %lld does not fit the grid", (long long)n);
  DMM_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_stack_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mode, with_variance ? 1 : 0, stack_weight, stack_nsample, sum_coeff_sq,
                     sample_variance, n);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
