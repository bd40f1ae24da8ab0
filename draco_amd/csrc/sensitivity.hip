// System sensitivity of a time stream: the measured and the radiometer estimate of the noise of the beamformed
// visibilities, and the mask of negative autocorrelations.
//
// Reference: draco/analysis/sensitivity.py:11-261 (ComputeSystemSensitivity), draco/analysis/flagging.py:666-699
// (NegativeAutosMask).  DESIGN.md section 7j.
//
// All three kernels stream [freq][stack][time] cubes once and reduce over rows of the stack axis that an index list
// names.  A block is kSplit waves over one tile of 64 times: consecutive lanes run along time, so every load of a wave
// is one contiguous run (256 bytes of weight, 512 of vis), and wave v takes the rows v, v + kSplit, ... of the list,
// eight of them in flight at a time.  Every lane adds its terms in list order in float64; the kSplit partial sums meet
// in LDS and wave 0 adds them in wave order, so a result depends on nothing but the list: no atomics, and two runs
// give the same bits.  The float32 result is rounded once, at the store.
// k_sens_measured: per (time tile, polarisation, frequency) V = sum c^2 k [w > 0] / w and C = sum c k [w > 0] over the
// rows of the polarisation, c the redundancy of the row under the sample's input-flag column.
// k_sens_radiometer: per (time tile, frequency) the sums S_g = sum n a and N_g = sum n over the autocorrelation rows of
// every (polarisation, east-west position) group g, n = c [w > 0], a = Re vis; then per output polarisation the sums of
// S_g S_h and N_g N_h over its list of ordered group pairs.  This is the reference's double loop over autocorrelations
// term by term, at a cost of nauto + ngroup^2 per sample.
// k_sens_negative_autos: per (time tile, frequency) whether any autocorrelation row has Re vis < 0.
#include "dmm_internal.h"

#include <algorithm>

namespace {

constexpr int kWave = 64;
constexpr int kSplit = 4;  // waves of a block = parts the row list is dealt into
constexpr int kThreads = kWave * kSplit;
constexpr int kFlight = 8;  // rows a wave has in flight (4: 8 % slower on the CHIME-like block of tools/sens_timing.py)

__device__ inline double inv0(double x) { return x == 0.0 ? 0.0 : 1.0 / x; }

struct MeasArgs {
  const float* weight;     // [nf][nstack][nt]
  const float* cnt;        // [nstack][ncol]
  const int32_t* col;      // [niff][nt]
  const int32_t* pol_ptr;  // [npol + 1]
  const int32_t* rows;     // [nrows][2]: stack entry, factor k
  float* measured;         // [nf][npol][nt]
  float* out_weight;
  int nf, nstack, nt, ncol, niff, npol;
};

__global__ __launch_bounds__(kThreads) void k_sens_measured(MeasArgs a) {
  __shared__ double part[2][kSplit][kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int t = blockIdx.x * kWave + lane, p = blockIdx.y, f = blockIdx.z;
  const bool live = t < a.nt;
  const int tt = live ? t : a.nt - 1;  // lanes past the end repeat the last sample: their reads stay inside
  const int c = a.col[(int64_t)(f % a.niff) * a.nt + tt];
  const float* w = a.weight + (int64_t)f * a.nstack * a.nt + tt;
  const float* cnt = a.cnt + c;
  const int hi = a.pol_ptr[p + 1];
  int i = a.pol_ptr[p] + wave;
  double V = 0.0, C = 0.0;
  for (; i + (kFlight - 1) * kSplit < hi; i += kFlight * kSplit) {
    float wv[kFlight], cv[kFlight];
    int k[kFlight];
#pragma unroll
    for (int u = 0; u < kFlight; ++u) {
      const int s = a.rows[2 * (i + u * kSplit)];
      k[u] = a.rows[2 * (i + u * kSplit) + 1];
      wv[u] = w[(int64_t)s * a.nt];
      cv[u] = cnt[(int64_t)s * a.ncol];
    }
#pragma unroll
    for (int u = 0; u < kFlight; ++u)
      if (wv[u] > 0.f) {
        const double ck = (double)cv[u] * (double)k[u];
        V += (double)cv[u] * ck / (double)wv[u];
        C += ck;
      }
  }
  for (; i < hi; i += kSplit) {
    const int s = a.rows[2 * i], k = a.rows[2 * i + 1];
    const float wv = w[(int64_t)s * a.nt], cv = cnt[(int64_t)s * a.ncol];
    if (wv > 0.f) {
      const double ck = (double)cv * (double)k;
      V += (double)cv * ck / (double)wv;
      C += ck;
    }
  }
  part[0][wave][lane] = V;
  part[1][wave][lane] = C;
  __syncthreads();
  if (wave == 0 && live) {
    V = part[0][0][lane];
    C = part[1][0][lane];
    for (int v = 1; v < kSplit; ++v) {
      V += part[0][v][lane];
      C += part[1][v][lane];
    }
    const int64_t o = ((int64_t)f * a.npol + p) * a.nt + t;
    a.measured[o] = (float)sqrt(2.0 * V * inv0(C * C));
    a.out_weight[o] = (float)C;
  }
}

struct RadArgs {
  const float2* vis;        // [nf][nstack][nt]
  const float* weight;
  const float* cnt;         // [nstack][ncol]
  const int32_t* col;       // [niff][nt]
  const int32_t* grp_ptr;   // [ngroup + 1]
  const int32_t* arows;     // [nauto] stack entries, group by group
  const int32_t* pair_ptr;  // [npol + 1]
  const int32_t* pairs;     // [npair][2]: groups g, h
  const float* frac_lost;   // [nf][nt] or NULL
  float* radiometer;        // [nf][npol][nt]
  float* frac_out;          // [nf][nt]
  double dnu_tint;
  int nf, nstack, nt, ncol, niff, npol, ngroup;
};

// dynamic LDS: part [2][kSplit][kWave], then the group sums [2][ngroup][kWave]
__global__ __launch_bounds__(kThreads) void k_sens_radiometer(RadArgs a) {
  extern __shared__ double lds[];
  double* part = lds;
  double* gsum = lds + 2 * kSplit * kWave;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int t = blockIdx.x * kWave + lane, f = blockIdx.y;
  const bool live = t < a.nt;
  const int tt = live ? t : a.nt - 1;
  const int c = a.col[(int64_t)(f % a.niff) * a.nt + tt];
  const int64_t base = (int64_t)f * a.nstack * a.nt + tt;
  const float* w = a.weight + base;
  const float2* vis = a.vis + base;
  const float* cnt = a.cnt + c;
  for (int g = 0; g < a.ngroup; ++g) {
    const int hi = a.grp_ptr[g + 1];
    int i = a.grp_ptr[g] + wave;
    double S = 0.0, N = 0.0;
    for (; i + (kFlight - 1) * kSplit < hi; i += kFlight * kSplit) {
      float wv[kFlight], cv[kFlight], re[kFlight];
#pragma unroll
      for (int u = 0; u < kFlight; ++u) {
        const int s = a.arows[i + u * kSplit];
        wv[u] = w[(int64_t)s * a.nt];
        re[u] = vis[(int64_t)s * a.nt].x;
        cv[u] = cnt[(int64_t)s * a.ncol];
      }
#pragma unroll
      for (int u = 0; u < kFlight; ++u) {
        const double n = wv[u] > 0.f ? (double)cv[u] : 0.0;
        S += n * (double)re[u];
        N += n;
      }
    }
    for (; i < hi; i += kSplit) {
      const int s = a.arows[i];
      const double n = w[(int64_t)s * a.nt] > 0.f ? (double)cnt[(int64_t)s * a.ncol] : 0.0;
      S += n * (double)vis[(int64_t)s * a.nt].x;
      N += n;
    }
    part[wave * kWave + lane] = S;
    part[(kSplit + wave) * kWave + lane] = N;
    __syncthreads();
    if (wave == 0) {
      S = part[lane];
      N = part[kSplit * kWave + lane];
      for (int v = 1; v < kSplit; ++v) {
        S += part[v * kWave + lane];
        N += part[(kSplit + v) * kWave + lane];
      }
      gsum[g * kWave + lane] = S;
      gsum[(a.ngroup + g) * kWave + lane] = N;
    }
    __syncthreads();  // the partial sums are read before the next group overwrites them
  }
  if (wave != 0 || !live) return;
  const int64_t ft = (int64_t)f * a.nt + t;
  const float lost = a.frac_lost ? a.frac_lost[ft] : 0.f;
  a.frac_out[ft] = lost;
  const double nint = a.dnu_tint * (1.0 - (double)lost);
  for (int p = 0; p < a.npol; ++p) {
    double R = 0.0, K = 0.0;
    for (int q = a.pair_ptr[p]; q < a.pair_ptr[p + 1]; ++q) {
      const int g = a.pairs[2 * q], h = a.pairs[2 * q + 1];
      R += gsum[g * kWave + lane] * gsum[h * kWave + lane];
      K += gsum[(a.ngroup + g) * kWave + lane] * gsum[(a.ngroup + h) * kWave + lane];
    }
    a.radiometer[((int64_t)f * a.npol + p) * a.nt + t] = (float)sqrt(2.0 * R * inv0(nint * K * K));  // R < 0: NaN
  }
}

__global__ __launch_bounds__(kThreads) void k_sens_negative_autos(const float2* vis, const int32_t* arows, int nauto, int nstack, int nt, uint8_t* mask) {
  __shared__ int part[kSplit][kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int t = blockIdx.x * kWave + lane, f = blockIdx.y;
  const bool live = t < nt;
  const float2* v = vis + (int64_t)f * nstack * nt + (live ? t : nt - 1);
  int neg = 0;
  for (int i = wave; i < nauto; i += kSplit) neg |= v[(int64_t)arows[i] * nt].x < 0.f;
  part[wave][lane] = neg;
  __syncthreads();
  if (wave == 0 && live) {
    for (int u = 1; u < kSplit; ++u) neg |= part[u][lane];
    mask[(int64_t)f * nt + t] = neg ? 1 : 0;
  }
}

inline unsigned tiles(int nt) { return (unsigned)((nt + kWave - 1) / kWave); }

// the checks the three entry points share: sizes, and the input-flag column of every (frequency block, time)
int check_cube(const char* who, int nf, int nstack, int nt) {
  DMM_REQUIRE(nf >= 1 && nstack >= 1 && nt >= 1, "%s: sizes must be positive, got nf=%d nstack=%d nt=%d", who, nf, nstack, nt);
  DMM_REQUIRE(nf <= 65535, "%s: nf %d does not fit the grid (65535)", who, nf);
  return DMM_OK;
}
int check_cols(const char* who, int nf, int nt, int ncol, int niff, const int32_t* col) {
  DMM_REQUIRE(ncol >= 1, "%s: ncol must be positive, got %d", who, ncol);
  DMM_REQUIRE(niff == 1 || niff == nf, "%s: niff %d is neither 1 nor nf = %d", who, niff, nf);
  for (int64_t i = 0; i < (int64_t)niff * nt; ++i)
    DMM_REQUIRE(col[i] >= 0 && col[i] < ncol, "%s: column index %d of sample %lld outside 0 ... %d", who, col[i], (long long)i, ncol - 1);
  return DMM_OK;
}
int check_ptr(const char* who, const char* what, int n, const int32_t* p) {
  DMM_REQUIRE(p[0] == 0, "%s: %s does not start at 0", who, what);
  for (int i = 0; i < n; ++i) DMM_REQUIRE(p[i + 1] >= p[i], "%s: %s is not monotone at entry %d", who, what, i + 1);
  return DMM_OK;
}
int check_rows(const char* who, int n, int stride, const int32_t* rows, int nstack) {
  for (int i = 0; i < n; ++i)
    DMM_REQUIRE(rows[(int64_t)stride * i] >= 0 && rows[(int64_t)stride * i] < nstack, "%s: row index %d of entry %d outside 0 ... %d", who, rows[(int64_t)stride * i], i, nstack - 1);
  return DMM_OK;
}

}  // namespace

#define SENS_CHECK(call)          \
  do {                            \
    const int rc_ = (call);       \
    if (rc_ != DMM_OK) return rc_; \
  } while (0)

extern "C" {

int dmm_sens_measured(dmm_ctx* ctx, const float* weight, int nf, int nstack, int nt, const float* cnt, int ncol, int niff, const int32_t* col, int npol,
                      const int32_t* pol_ptr, const int32_t* rows, int32_t* tables, float* measured, float* out_weight) {
  const char* who = "dmm_sens_measured";
  DMM_REQUIRE(ctx != nullptr, "dmm_sens_measured: ctx is NULL");
  SENS_CHECK(check_cube(who, nf, nstack, nt));
  DMM_REQUIRE(npol >= 1 && npol <= 65535, "dmm_sens_measured: npol %d outside 1 ... 65535", npol);
  DMM_REQUIRE(weight && cnt && col && pol_ptr && rows && tables && measured && out_weight, "dmm_sens_measured: NULL argument");
  SENS_CHECK(check_cols(who, nf, nt, ncol, niff, col));
  SENS_CHECK(check_ptr(who, "pol_ptr", npol, pol_ptr));
  const int nrows = pol_ptr[npol];
  SENS_CHECK(check_rows(who, nrows, 2, rows, nstack));
  for (int i = 0; i < nrows; ++i) DMM_REQUIRE(rows[2 * i + 1] == 1 || rows[2 * i + 1] == 2, "dmm_sens_measured: factor %d of entry %d is neither 1 nor 2", rows[2 * i + 1], i);
  DMM_HIP(hipSetDevice(ctx->device));
  const size_t ncolidx = (size_t)niff * nt;
  int32_t* col_d = tables;
  int32_t* ptr_d = col_d + ncolidx;
  int32_t* rows_d = ptr_d + npol + 1;
  DMM_HIP(hipMemcpyAsync(col_d, col, sizeof(int32_t) * ncolidx, hipMemcpyHostToDevice, ctx->stream));
  DMM_HIP(hipMemcpyAsync(ptr_d, pol_ptr, sizeof(int32_t) * (size_t)(npol + 1), hipMemcpyHostToDevice, ctx->stream));
  if (nrows) DMM_HIP(hipMemcpyAsync(rows_d, rows, sizeof(int32_t) * 2 * (size_t)nrows, hipMemcpyHostToDevice, ctx->stream));
  MeasArgs a{weight, cnt, col_d, ptr_d, rows_d, measured, out_weight, nf, nstack, nt, ncol, niff, npol};
  hipLaunchKernelGGL(k_sens_measured, dim3(tiles(nt), (unsigned)npol, (unsigned)nf), dim3(kThreads), 0, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_sens_radiometer(dmm_ctx* ctx, const void* vis, const float* weight, int nf, int nstack, int nt, const float* cnt, int ncol, int niff, const int32_t* col,
                        int ngroup, const int32_t* grp_ptr, const int32_t* auto_rows, int npol, const int32_t* pair_ptr, const int32_t* pairs, const float* frac_lost,
                        double dnu_tint, int32_t* tables, float* radiometer, float* frac_out) {
  const char* who = "dmm_sens_radiometer";
  DMM_REQUIRE(ctx != nullptr, "dmm_sens_radiometer: ctx is NULL");
  SENS_CHECK(check_cube(who, nf, nstack, nt));
  DMM_REQUIRE(npol >= 1 && npol <= 65535, "dmm_sens_radiometer: npol %d outside 1 ... 65535", npol);
  DMM_REQUIRE(ngroup >= 0 && ngroup <= DMM_SENS_MAX_GROUP, "dmm_sens_radiometer: ngroup %d outside 0 ... %d", ngroup, DMM_SENS_MAX_GROUP);
  DMM_REQUIRE(vis && weight && cnt && col && grp_ptr && auto_rows && pair_ptr && pairs && tables && radiometer && frac_out, "dmm_sens_radiometer: NULL argument");
  SENS_CHECK(check_cols(who, nf, nt, ncol, niff, col));
  SENS_CHECK(check_ptr(who, "grp_ptr", ngroup, grp_ptr));
  SENS_CHECK(check_ptr(who, "pair_ptr", npol, pair_ptr));
  const int nauto = grp_ptr[ngroup], npair = pair_ptr[npol];
  SENS_CHECK(check_rows(who, nauto, 1, auto_rows, nstack));
  for (int i = 0; i < 2 * npair; ++i) DMM_REQUIRE(pairs[i] >= 0 && pairs[i] < ngroup, "dmm_sens_radiometer: group %d of pair %d outside 0 ... %d", pairs[i], i / 2, ngroup - 1);
  DMM_HIP(hipSetDevice(ctx->device));
  const size_t ncolidx = (size_t)niff * nt;
  int32_t* col_d = tables;
  int32_t* grp_d = col_d + ncolidx;
  int32_t* arows_d = grp_d + ngroup + 1;
  int32_t* pptr_d = arows_d + nauto;
  int32_t* pairs_d = pptr_d + npol + 1;
  DMM_HIP(hipMemcpyAsync(col_d, col, sizeof(int32_t) * ncolidx, hipMemcpyHostToDevice, ctx->stream));
  DMM_HIP(hipMemcpyAsync(grp_d, grp_ptr, sizeof(int32_t) * (size_t)(ngroup + 1), hipMemcpyHostToDevice, ctx->stream));
  if (nauto) DMM_HIP(hipMemcpyAsync(arows_d, auto_rows, sizeof(int32_t) * (size_t)nauto, hipMemcpyHostToDevice, ctx->stream));
  DMM_HIP(hipMemcpyAsync(pptr_d, pair_ptr, sizeof(int32_t) * (size_t)(npol + 1), hipMemcpyHostToDevice, ctx->stream));
  if (npair) DMM_HIP(hipMemcpyAsync(pairs_d, pairs, sizeof(int32_t) * 2 * (size_t)npair, hipMemcpyHostToDevice, ctx->stream));
  RadArgs a{(const float2*)vis, weight, cnt, col_d, grp_d, arows_d, pptr_d, pairs_d, frac_lost, radiometer, frac_out, dnu_tint, nf, nstack, nt, ncol, niff, npol, ngroup};
  const size_t lds = sizeof(double) * 2 * (size_t)(kSplit + ngroup) * kWave;
  DMM_HIP(hipFuncSetAttribute((const void*)k_sens_radiometer, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_sens_radiometer, dim3(tiles(nt), (unsigned)nf), dim3(kThreads), lds, ctx->stream, a);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

int dmm_sens_negative_autos(dmm_ctx* ctx, const void* vis, int nf, int nstack, int nt, int nauto, const int32_t* auto_rows, int32_t* tables, uint8_t* mask) {
  const char* who = "dmm_sens_negative_autos";
  DMM_REQUIRE(ctx != nullptr, "dmm_sens_negative_autos: ctx is NULL");
  SENS_CHECK(check_cube(who, nf, nstack, nt));
  DMM_REQUIRE(nauto >= 0, "dmm_sens_negative_autos: bad row count %d", nauto);
  DMM_REQUIRE(vis && mask && (nauto == 0 || (auto_rows && tables)), "dmm_sens_negative_autos: NULL argument");
  SENS_CHECK(check_rows(who, nauto, 1, auto_rows, nstack));
  DMM_HIP(hipSetDevice(ctx->device));
  if (nauto) DMM_HIP(hipMemcpyAsync(tables, auto_rows, sizeof(int32_t) * (size_t)nauto, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_sens_negative_autos, dim3(tiles(nt), (unsigned)nf), dim3(kThreads), 0, ctx->stream, (const float2*)vis, (const int32_t*)tables, nauto, nstack, nt, mask);
  DMM_HIP(hipGetLastError());
  return DMM_OK;
}

}  // extern "C"
