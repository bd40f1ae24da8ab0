/*
 * draco_amd.h -- C ABI of the MI355X (gfx950) m-mode map-making path.
 *
 * This is the drop-in boundary: every entry point is `extern "C"`, takes plain
 * pointers and sizes (no torch / C++ types) and is what a ctypes binding of the
 * reference's hot path binds (INTEGRATION.md shows the binding).  Each function
 * names the reference interface (radiocosmology/draco, file:line) it replaces.
 *
 * Conventions
 *   - every call returns an int status: 0 = ok, <0 = argument error (DMM_E_*),
 *     >0 = a hipError_t; the message is in dmm_last_error() (thread local);
 *   - the CALLER owns every data buffer; pointers marked [dev] are device pointers
 *     valid on the context's device, [host] are ordinary host pointers; the
 *     library never frees caller memory and keeps no caller pointer after a call
 *     returns (work is enqueued on the context's stream: the caller must keep the
 *     buffers alive until dmm_ctx_sync / a stream sync of its own);
 *   - second-stream rule: an entry point may run part of its work on a stream the
 *     library owns (dmm_ml_run does); that stream is drained before the entry point
 *     returns on every path, error returns included, so after ANY call the caller's
 *     buffers are governed by the context's stream alone; dmm_ctx_sync drains both;
 *   - row-major (C order) everywhere, matching NumPy; complex = interleaved
 *     (re, im); complex64 = 2 x float, complex128 = 2 x double;
 *   - a context is not thread-safe; distinct contexts are independent;
 *   - no exceptions or longjmp cross this boundary.
 */
#ifndef DRACO_AMD_H
#define DRACO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMM_VERSION 100 /* 0.1.0 */

typedef struct dmm_ctx dmm_ctx;
typedef struct dmm_plan dmm_plan;

enum {
  DMM_OK = 0,
  DMM_E_ARG = -1,      /* invalid argument (null pointer, bad size, bad enum) */
  DMM_E_UNSUPPORTED = -2, /* valid request this build cannot serve (e.g. nra too long) */
  DMM_E_NOMEM = -3,
  DMM_E_STATE = -4,
  DMM_E_COMM = -5      /* an RCCL call failed (dmm_comm_*, dmm_allgather_map); RCCL's own code is in dmm_last_error() */
};

/* element types of the beam-transfer pool and of m-mode outputs */
enum { DMM_C64 = 0, DMM_C128 = 1 };

/* layout of one beam-transfer tile B_m[f] (what `bt.beam_m(m, fi=f)` returns,
 * reference mapmaker.py:162, reshaped to [ntel, npol, lmax+1]):
 *   DMM_B_FULL   [ntel, npol, lmax+1]     -- the l<m columns are stored (zeros), never read
 *   DMM_B_PACKED [ntel, npol, lmax+1-m]   -- only the l>=m columns are stored           */
enum { DMM_B_FULL = 0, DMM_B_PACKED = 1 };

/* one (m, freq) solve: which tile, which data column */
typedef struct {
  int64_t b_off; /* element offset of the tile inside the B buffer */
  int32_t m;     /* m of this tile (row of the m axis of mvis/mweight/alm) */
  int32_t f;     /* frequency index into mvis/mweight/alm */
} dmm_tile;

/* ---------------------------------------------------------------- context */
int dmm_version(void);
const char* dmm_last_error(void);
int dmm_ctx_create(int device, dmm_ctx** ctx);
int dmm_ctx_destroy(dmm_ctx* ctx);
/* run on the caller's HIP stream (hipStream_t passed as void*; NULL = default stream) */
int dmm_ctx_set_stream(dmm_ctx* ctx, void* hip_stream);
int dmm_ctx_sync(dmm_ctx* ctx);
/* Options (name, integer value): option, default, meaning.  Every option reads back as "opt_<name>" through
 * dmm_ctx_get_counter.  All but the accuracy-affecting ones change run time only, never results; details: INTEGRATION.md
 * section C.
 *   "dirty_variant"         0  kernel form of the Dirty solve
 *   "grid_mult"             0  size: blocks per CU of the Dirty launch
 *   "dirty_static"          0  1: static striding of the Dirty kernel's task list
 *   "dirty_nofill"          0  1: dmm_dirty_run_multi does not write the structural zeros alm[l < m] (they stay whatever the
 *                              memory held): for an a_lm that only dmm_alm2map reads, which loads l >= m alone; every other entry writes them
 *   "dirty_prio"            0  1: the Dirty kernel's waves raise their issue priority (dmm_dirty_run and every group of dmm_dirty_run_multi)
 *   "project_variant"       0  kernel form of dmm_project_run
 *   "project_grid_mult"     0  size: blocks per CU of the projection launch
 *   "sht_variant"           0  bits: 2 direct ring sums, 3 vector-ALU Legendre kernels, 6 first MFMA synthesis form, 7 pipelined
 *                              synthesis with 4 frequencies per block; the other bits selected A/B forms that are gone: accepted and ignored
 *   "sht_synth_form"        0  1: first MFMA synthesis form, whatever "sht_variant" says
 *   "ringmap_variant"       0  1 three-kernel form, 2 eight elevations per block
 *   "ml_shortcut"           0  0 certificate on, 2 always eigen-decompose, 3 telescope side only
 *   "ml_eigen"              0  0 by batch size, 4 tridiagonal + QL, 1 blocked Jacobi, 2 full-matrix trailing updates, 3 QL made to fail (tests)
 *   "ml_null"               0  0 sampled null certificate, 1 off, 2 every tile
 *   "ml_reduce"             0  0 two-stage with every other update deferred, 3 its reading sweeps as one block per matrix, 2 none deferred, 1 one-stage
 *   "ml_rank_stop"          0  accuracy-affecting (positive semi-definite input only): 0 on at 1e-13 of lambda_max, 1 off, v >= 11 on at 10^-v
 *   "ml_chase_split"        0  1: one chase launch with the full band image
 *   "ml_inner_sweeps"       0  accuracy-affecting: iteration cap of the Jacobi fallback (0: the built-in cap)
 *   "ml_outer_sweeps"       0  accuracy-affecting: iteration cap of the Jacobi fallback (0: the built-in cap)
 *   "gram_stage"            0  1: LDS-DMA operand staging of the Gram kernel
 *   "wiener_overlap"        1  0: the batches of dmm_wiener_run on one stream
 *   "ml_workspace_mib"      0  size the ML solve plans its batches for (0 = 20 GiB; negative values are stored as 0)
 *   "regrid_workspace_mib"  0  scratch the regridder sizes its row chunks for (0 = 12 GiB: a cfg-3 day in one launch; negative: 0)
 *   "wiener_workspace_mib"  0  size the Wiener solve plans its batches for (0 = 6 GiB; negative: 0)
 *   "profile"               0  1: HIP-event timing of the dense solvers' kernel classes; every set collects the open spans and
 *                              clears the sums; reads back as 0 or 1 */
int dmm_ctx_set_option(dmm_ctx* ctx, const char* name, int64_t value);
/* diagnostics counters, cumulative per context ("opt_<name>": the current value of option <name>, no wait): "ml_tiles_direct" (tiles whose pseudo-inverse was
 * certified to cut no mode and solved by Cholesky), "ml_tiles_eigen" (tiles eigen-decomposed), "ml_tiles_null" (tiles answered with zero by the null certificate: every
 * singular value at or below acond), "ml_tiles_stopped" / "ml_stop_cols" (eigen-decomposed tiles whose reduction the rank stop cut off,
 * and the sum of their effective orders), "ml_gram_flops" / "ml_band_bytes" (useful flops 4 k^2 K of the
 * Gram matrices dmm_ml_run formed, algorithmic bytes of stage 1 of its two-stage reductions: the numerators of
 * bench.py's rooflines), "ml_tiles_ql_failed"
 * (of those: tridiagonal QL did not converge, the tile was redone by the blocked Jacobi solver), "ml_early_chunks"
 * (chunks of early-known rejects decomposed beside the remaining certificate batches); read-only properties of the build:
 * "ml_two_stage_max_order" (the largest matrix order the two-stage reduction takes: telescopes above it have no basis route),
 * "build_ab" (1: built with -DDMM_AB, "ml_reduce" = 5 selects the one-kernel stage 1; 0: it runs the default form); with the "profile" option on,
 * "prof_<class>_us" / "prof_<class>_n" = summed HIP-event time (microseconds) and number of spans of a kernel class,
 * class = gram (Hermitian products B B^H / B^H N B), chol (factorisations + triangular solves), tridiag (Householder
 * reduction), band (two-stage reduction, stage 1: dense -> band), chase (stage 2: band -> tridiagonal), ql
 * (tridiagonal eigen-solve + replay), backproj (a = B^H w), null (the null certificate's pass over B), solve (dmm_wiener_run from its first launch to its last: the
 * batches of that call alternate between two streams, so its class sums overlap in time and this span is the wall).  Reading a counter waits for the spans still running. */
int dmm_ctx_get_counter(dmm_ctx* ctx, const char* name, int64_t* value);
/* Validation hook for pinv_svd's rank decision (mapmaker.py:296: keep sigma > rcond*sigma_max and sigma > acond).
 * While `diag` [dev] is non-NULL every tile that dmm_ml_run eigen-decomposes writes four doubles at
 * diag[(f * n_m + m) * 4]: the number of singular values it kept, sigma_max, the smallest kept sigma and the largest
 * cut sigma (sigma = sqrt(lambda) of the smaller-side Gram matrix; exact zero modes -- padding, zero-weight rows,
 * l < m -- count as cut with sigma 0).  Tiles solved by the certified full-rank shortcut write nothing (initialise
 * the buffer to -1 to tell them apart).  f, m as in dmm_tile; n_m = the plan's.  NULL switches it off. */
int dmm_ctx_set_ml_diag(dmm_ctx* ctx, double* diag);
/* Resident beam Gram products for dmm_ml_run (multi-day processing: the beam transfers are the telescope's, the weights
 * the day's).  The telescope-side Gram matrix of a tile is D (B B^H) D with D = sqrt(N^-1) of the day (mapmaker.py:190-198
 * whitens B with it): B B^H does not change from day to day.  While `cache` [dev] is non-NULL, dmm_ml_run keeps the
 * products B B^H of the plan's telescope-side tiles there -- slot s = the s-th such tile in plan order, T (T + 1) / 2
 * lower-triangle blocks of 64 x 64 complex128 each (T = ceil(2 npairs / 64)): dmm_ml_gram_cache_bytes(plan) bytes --
 * computing a slot the first time it meets it (`valid` [dev, one int32 per slot] says which are there) and forming the
 * day's Gram matrix from the slot by the same scaling its Gram kernel applies (bit-identical matrices) ever after.
 * The caller owns both arrays, keeps them with the B block they were computed from and passes reset = 1 whenever that
 * block's contents change (the library then clears `valid`).  cache = NULL: off (default).
 * dmm_wiener_run honours the same arrays for its telescope-side systems I + D (B S B^H) D (mapmaker.py:267-272): the
 * products are then B S B^H -- a cache belongs to ONE maker and ONE prior; hand each its own. */
int dmm_ctx_set_ml_gram_cache(dmm_ctx* ctx, void* cache, int32_t* valid, int64_t nslots, int reset);
/* Resident singular bases of the beam transfers for dmm_ml_run (multi-day processing, one step further than the Gram
 * products).  B B^H = U Sigma^2 U^H does not change from day to day: with U and Sigma of a telescope-side tile resident
 * (numerical rank r = 150 ... 400 of 758 at cfg 3) the day's Gram matrix D B B^H D = A A^H, A = D U Sigma, has the non-zero
 * spectrum of the r x r matrix M = A^H A = Sigma U^H D^2 U Sigma, and pinv_svd's solution (mapmaker.py:190-201, 287-300) is
 * A W diag(keep / lambda^2) W^H A^H (D v) with M = W Lambda W^H -- an order-r eigenproblem per tile and day instead of
 * an order-758 one, and no Gram product of B at all.
 *   build = 1: the next dmm_ml_run calls do NOT solve: they decompose B B^H of every telescope-side tile of their plan (pass
 *              unit weights) and leave, per slot (= the tile's rank among the plan's telescope-side tiles, as for the Gram
 *              cache): U^H as rmax rows of 2 npairs complex128 (`U`), the singular values (`sigma`, rmax doubles) and
 *              their count (`rank`, -1: more than rmax above 1e-15 of the largest eigenvalue -- the tile keeps the
 *              full-order path).  alm is not written.
 *   build = 0: dmm_ml_run takes the basis route for every chunk whose tiles all have a basis -- and whose small problem fits
 *              the workspace beside the basis product (otherwise the chunk keeps the full-order path).  The library sizes the
 *              chunks from a host copy of `rank`, taken when the array is first used through this context and kept until a
 *              build through this context; build = 2: as 0, and take the copy again.  The copy is keyed on the `rank`
 *              POINTER alone: build = 2 is MANDATORY after the array was written by other means (another context, a
 *              copy) or freed and allocated again at the same address.
 * U = NULL: off.  The arrays are the caller's and live with the B block they were computed from.
 * Accuracy: the bases are truncated at 1e-15 of the largest eigenvalue of the UNWEIGHTED B B^H; a day whose non-zero noise
 * weights span more than six decades should use the full-order path (the dropped modes enter the day's Gram matrix at up to
 * 1e-15 (d_max / d_min)^2 of its lambda_max, pinv_svd's relative cut is 1e-6): MaximumLikelihoodMapMaker.cache_beam_basis
 * checks the day's weights and falls back by itself. */
int dmm_ctx_set_ml_basis(dmm_ctx* ctx, void* U, double* sigma, int32_t* rank, int64_t nslots, int rmax, int build);
int64_t dmm_ml_gram_cache_slots(const dmm_plan* plan);
int64_t dmm_ml_gram_cache_bytes(const dmm_plan* plan);
/* HIP-event stopwatch on the context's stream (bench.py's kernel timing) */
int dmm_timer_start(dmm_ctx* ctx);
int dmm_timer_stop(dmm_ctx* ctx, float* elapsed_ms); /* synchronises on the stop event */

/* ------------------------------------------------- m-mode transform (a2, a3)
 * dmm_mfft_pack replaces `_make_marray` (reference transform.py:644-705) together
 * with the zero fill at :623 and the optional window at :630-636:
 *   F = fft(ts, axis=-1) in single precision; for every row r
 *     out[m, 0, r] = F[r, m] / nra              0 <= m <= mlim
 *     out[m, 1, r] = conj(F[r, nra-m]) / nra    1 <= m <= mlim_neg
 *     out[.]       = 0 elsewhere                (mlim, mlim_neg: transform.py:678-679)
 *   then out[m, :, :] *= mscale[m] if mscale != NULL.
 * ts      [dev] complex64 [nrow, nra]
 * out     [dev] complex  [mmax+1, 2, nrow] of out_dtype (DMM_C128 = MModes.vis)
 * mscale  [dev] double [mmax+1] or NULL
 * Any nra >= 1 up to DMM_MAX_NRA is served (power of two: in-LDS radix FFT;
 * otherwise Bluestein).                                                          */
#define DMM_MAX_NRA 8192
int dmm_mfft_pack(dmm_ctx* ctx, const void* ts, int64_t nrow, int nra, void* out,
                  int mmax, int out_dtype, const double* mscale);

/* dmm_mmode_weight replaces transform.py:599-602 + :627 (+ :638-639):
 *   ws[r] = nra^2 * inz( sum_ra inz(weight[r, ra]) ),  out[m, s, r] = ws[r] * wscale[m]
 * weight [dev] float32 [nrow, nra]; out [dev] double [mmax+1, 2, nrow];
 * wscale [dev] double [mmax+1] or NULL.                                           */
int dmm_mmode_weight(dmm_ctx* ctx, const float* weight, int64_t nrow, int nra,
                     double* out, int mmax, const double* wscale);

/* inverse: `_unpack_marray` + `_make_ssarray` (transform.py:814-851) and the weight
 * rule of MModeInverseTransform.process (:790).
 * mvis [dev] complex128 [n_m, 2, nrow]; vis_out [dev] complex64 [nrow, nra];
 * mmax_plus/mmax_minus are the limits computed by the caller per :825-836
 * (the "is the top -m row all zero" test of :826 is done by dmm_mrow_is_zero).     */
int dmm_mifft_unpack(dmm_ctx* ctx, const void* mvis, int n_m, int64_t nrow, int nra,
                     int mmax_plus, int mmax_minus, const double* mscale, void* vis_out);
int dmm_mrow_is_zero(dmm_ctx* ctx, const void* mvis, int n_m, int64_t nrow, int m,
                     int sign, int* is_zero /*[host]*/);

/* MaskMModeData.process (reference flagging.py:113-173), in place on MModes.weight
 * [n_m, 2, nfreq, nstack] double: zero the weights of auto-correlations (is_auto[nstack] != 0;
 * NULL = keep), of m = 0 unless m_zero, of +m / -m (m >= 1) unless positive_m / negative_m, and
 * of every m < mask_low_m.                                                            */
int dmm_mask_mmode_weight(dmm_ctx* ctx, double* mweight, int n_m, int64_t nfreq, int nstack,
                          const unsigned char* is_auto /*[dev]*/, int m_zero, int positive_m,
                          int negative_m, int mask_low_m);

/* CollateProducts.process, the stacking loop (reference transform.py:277-320): every output
 * (freq, unique baseline, time) sample is the weighted mean of its contributing input products
 *   vis = sum wss * (conj?) v / sum wss,  weight = (sum wss)^2 / sum(wss^2 / w)
 *   wss = w                      if red == NULL  ("inverse_variance")
 *       = (w > 0) * red[prod, t]  otherwise       ("natural": redundancy; "uniform": 0/1)
 * ssv [dev] complex64 [nf_in, nprod_in, nt], ssw [dev] float32 same; freq_ind [dev] int [nf_out]
 * (input frequency of each output frequency); CSR over output baselines: csr_ptr [nstack_out+1],
 * csr_src / csr_conj [nnz] (input product, conjugate it?); outputs complex64 / float32
 * [nf_out, nstack_out, nt].                                                             */
int dmm_collate_products(dmm_ctx* ctx, const void* ssv, const float* ssw, int nf_in, int nprod_in, int nt,
                         int nf_out, const int* freq_ind, int nstack_out, const int* csr_ptr,
                         const int* csr_src, const unsigned char* csr_conj, const float* red,
                         void* out_vis, float* out_w);

/* ExpandProducts.process (reference synthesis/stream.py:193-246): stacked stream -> full product triangle.
 * vis_in [dev] complex64 [nfreq, nstack, nt]; src [dev] int [nprod] = unique-baseline index of each product
 * (telescope.feedmap, < 0: masked pair, output 0 with weight 0); conj [dev] uint8 [nprod] (telescope.feedconj);
 * outputs complex64 / float32 [nfreq, nprod, nt], weight 1 where the pair exists.                              */
int dmm_expand_products(dmm_ctx* ctx, const void* vis_in, int nfreq, int nstack, int nt, int nprod,
                        const int* src, const unsigned char* conj, void* out_vis, float* out_w);

/* ------------------------------------------------------ map-maker solves (a5-a8)
 * A plan fixes the batch of (m, f) solves (the double loop at mapmaker.py:79-94)
 * and the shapes; it owns a device copy of the tile table.
 *   mvis    [dev] complex128 [n_m, 2, nfreq, npairs]   (MModes.vis,    containers.py:1178)
 *   mweight [dev] double     [n_m, 2, nfreq, npairs]   (MModes.weight)
 *   alm     [dev] complex128 [nfreq, npol, n_m, lmax+1]  (m-major: l is the fast axis;
 *           the reference's [nfreq, 4, lmax+1, mmax+1] at mapmaker.py:70 is its
 *           transpose, produced by the Python layer on request)
 *   B       [dev] pool of tiles, dtype/layout fixed by the plan, tile i at b_off.
 * Only entries alm[f, :, m, :] of tiles in the plan are written (l<m -> 0).         */
int dmm_solve_plan_create(dmm_ctx* ctx, const dmm_tile* tiles /*[host]*/, int64_t ntile,
                          int npairs, int npol, int lmax, int nfreq, int n_m, int b_dtype,
                          int b_layout, dmm_plan** plan);
int dmm_plan_destroy(dmm_plan* plan);
/* bytes of B the plan's tiles cover (algorithmic: l>=m columns only) */
int64_t dmm_plan_b_bytes(const dmm_plan* plan);

/* DirtyMapMaker._solve_m (mapmaker.py:156-168): a = B^H (Ni o v) for every tile */
int dmm_dirty_run(dmm_plan* plan, const void* B, const void* mvis, const double* mweight,
                  void* alm);

/* The same for `nday` sidereal days against ONE read of B: alm[d] = B^H (Ni_d o v_d).  The reference's loop
 * (mapmaker.py:79-94) is run once per pipeline item (doc/tutorial.rst:110-120) against the same beam transfers; here
 * up to 8 days share every tile read (4 ND f64 FMAs per 16 bytes of B instead of 4).  mvis / mweight / alm: [host]
 * arrays of `nday` device pointers, each as in dmm_dirty_run; the alm arrays must be distinct.  Every day's result is
 * bit-identical to dmm_dirty_run's on that day (same accumulation order).  With the context option "dirty_nofill" = 1
 * the entries l < m of every alm are left unwritten instead of zeroed. */
int dmm_dirty_run_multi(dmm_plan* plan, const void* B, const void* const* mvis, const double* const* mweight,
                        void* const* alm, int nday);

/* WienerMapMaker._solve_m (mapmaker.py:235-284):
 *   a = (S^-1 + B~^H B~)^-1 B~^H v~,  B~ = sqrt(Ni) o B[:, l>=m],  S = amp^2 l^-tilt (l[0]:=1)
 * factored on whichever side is smaller (the two branches at :267/:275 are the same
 * estimator).  workspace [dev]: dmm_wiener_workspace_bytes() bytes.                 */
int64_t dmm_wiener_workspace_bytes(const dmm_plan* plan);
int dmm_wiener_run(dmm_plan* plan, const void* B, const void* mvis, const double* mweight,
                   double prior_amp, double prior_tilt, void* workspace, void* alm);

/* MaximumLikelihoodMapMaker._solve_m (mapmaker.py:184-201) with pinv_svd's rank rule
 * (mapmaker.py:287-300): keep sigma > rcond*sigma_max and sigma > acond.           */
int64_t dmm_ml_workspace_bytes(const dmm_plan* plan);
int dmm_ml_run(dmm_plan* plan, const void* B, const void* mvis, const double* mweight,
               double acond, double rcond, void* workspace, void* alm);

/* forward: bt.project_vector_sky_to_telescope (stream.py:109-112): v = B a per tile.
 *   alm_in [dev] complex128 [nfreq, npol, n_m, lmax+1]; vis_out [dev] complex128
 *   [n_m, 2, nfreq, npairs]                                                         */
int dmm_project_run(dmm_plan* plan, const void* B, const void* alm_in, void* vis_out);

/* --------------------------------------------- spherical-harmonic transforms (a10)
 * hputil.sphtrans_inv_sky(alm, nside) (mapmaker.py:112) and hputil.sphtrans_sky
 * (stream.py:85) [cora -> healpy], HEALPix RING ordering.
 *   alm [dev] complex128 [nfreq, npol, mmax+1, lmax+1] (m-major)
 *   map [dev] double     [nfreq, npol, 12*nside^2]
 * npol = 1 (T) or 4 (T,E,B,V <-> I,Q,U,V).                                          */
int dmm_alm2map(dmm_ctx* ctx, const void* alm, int nfreq, int npol, int lmax, int mmax,
                int nside, double* map);
int dmm_map2alm(dmm_ctx* ctx, const double* map, int nfreq, int npol, int lmax, int mmax,
                int nside, int niter, void* alm);

/* ------------------------------------------------ deconvolving ring-map makers
 * The per-frequency loop of DeconvolveHybridMBase.process (reference ringmapmaker.py:744-823)
 * with the TikhonovRingMapMaker / WienerRingMapMaker weights (:1096-1118, :1178-1183).
 *   hv [dev] complex64 [nm, 2, npol, nfreq, new, nel]   HybridVisMModes.vis
 *   hw [dev] float32   [nm, 2, npol, nfreq, new]        HybridVisMModes.weight (inverse variance)
 *   bv [dev] complex64 [nm_beam >= nm, 2, npol, nfreq, new, nel]  beam m-modes (rows >= nm ignored)
 *   weight_mode 0: w = ew_table[ew] * (hw > 0)   ("natural" / "uniform", table already normalised,
 *                                                 excluded cylinders zero)
 *               1: w = hw*keep / sum_ew(hw*keep)  (Tikhonov "inverse_variance"; ew_table = keep mask)
 *               2: w = hw*keep                    (Wiener; ew_table = keep mask)
 *   eps    [dev] double [nfreq, nm]  regularisation (ignored if skip_deconvolution)
 *   window [dev] float32 [nfreq, nm, nel] or NULL
 *   nra = 2*(nm-1) (+1 if oddra); outputs float64:
 *   map [1, npol, nfreq, nra, nel], weight [npol, nfreq, nra, nel],
 *   dirty_beam_power [1, npol, nfreq, nel], dirty_beam [1, npol, nfreq, nra, nel] or NULL.     */
int dmm_ringmap_deconvolve(dmm_ctx* ctx, int nm, int nm_beam, int npol, int nfreq, int new_, int nel,
                           int nra, int weight_mode, int skip_deconvolution, int iref, const void* hv,
                           const float* hw, const void* bv, const double* ew_table, const double* eps,
                           const float* window, double* map, double* weight, double* dirty_beam_power,
                           double* dirty_beam);

/* dmm_ringmap_window: the cosine-sum window over (freq, m, el) that shapes the EW synthesised beam
 * (DeconvolveHybridMBase._get_window, reference ringmapmaker.py:842-930 with window_generalised,
 * util/tools.py:547-601): window[f, m, el] = sum_i coef[i] cos(2 pi i x) for 0 <= x <= 1, else 0,
 * x = (m - min_m[f, el]) / (max_m[f, el] - min_m[f, el]).
 * min_m, max_m [dev] double [nfreq, nel]; coef [host] 4 doubles; window [dev] float32 [nfreq, nm, nel].  */
int dmm_ringmap_window(dmm_ctx* ctx, int nfreq, int nm, int nel, const double* min_m, const double* max_m,
                       const double* coef, float* window);

/* dmm_analytic_beam_mmodes replaces DeconvolveAnalyticalBeam._get_beam_mmodes (reference
 * ringmapmaker.py:1004-1072): for every (pol, freq, ew, el) the conjugated transit of the analytic
 * beam  exp(2 pi i u cos(dec) sin(phi)) * exp(-(2 tan(phi/2))^2 / (2 sigma^2)),  phi = 2 pi k / nra,
 * u = ew / wavelength, sigma = sa*sb/sqrt(sa^2+sb^2) with s = coef / freq / cos(dec) per feed of the pol
 * pair (:1009-1017,1057-1060), is generated in float64 and m-transformed (double-precision FFT, the
 * _make_marray packing of dmm_mfft_pack) into
 *   out [dev] complex64 [mmax+1, 2, npol, nfreq, new, nel]            (HybridVisMModes.vis layout).
 * freq [nfreq] MHz, ew [new] metres, dec [nel] radians, coef_a/coef_b [npol]: all [dev] double.   */
int dmm_analytic_beam_mmodes(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, int mmax,
                             const double* freq, const double* ew, const double* dec, const double* coef_a,
                             const double* coef_b, void* out);

/* ------------------------------------------------ the map all-gather (the north star's one collective)
 * The reference leaves the Map distributed over frequency (mapmaker.py:113-116: an MPIArray); a caller that wants every
 * frequency on every rank gathers the rank-local shards [nfreq_local, 4, 12 nside^2] with ONE RCCL all-gather over xGMI.
 * RCCL is loaded at run time (librccl.so); a single-GPU user never needs it.
 *   dmm_comm_unique_id  rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by the caller's
 *                       own means (MPI_Bcast, a file, torch.distributed ...)
 *   dmm_comm_init       every rank: its context's device joins the communicator (ncclCommInitRank) -> *comm
 *   dmm_allgather_map   full[r * count .. (r+1) * count) = rank r's shard[0 .. count), float64, on the context's stream
 *                       (asynchronous like every kernel launch: dmm_ctx_sync before the host reads `full`); equal
 *                       counts on all ranks (pad uneven frequency slabs)
 *   dmm_comm_destroy    ncclCommDestroy                                                        */
#define DMM_COMM_ID_BYTES 128
int dmm_comm_unique_id(void* id_out /*[host, DMM_COMM_ID_BYTES]*/);
int dmm_comm_init(dmm_ctx* ctx, const void* id /*[host]*/, int rank, int world, void** comm_out);
int dmm_comm_destroy(void* comm);
int dmm_allgather_map(dmm_ctx* ctx, void* comm, const double* shard /*[dev]*/, int64_t count, double* full /*[dev]*/);

/* ------------------------------------------------ ring-map chain: MakeVisGrid -> BeamformNS -> BeamformEW
 * (reference ringmapmaker.py:38-534; the producers of the HybridVisStream the deconvolving makers start from).
 * dmm_calc_redundancy: tools.calculate_redundancy (tools.py:313-356): redundancy[s, t] = sum over the products stacked into
 *   s of flags[a, t] flags[b, t] (all_good: every flag counts as 1, the reference's rule when no flag is set).
 *   input_flags [dev] float [ninput, nra]; prod_a / prod_b / stack_index [dev] int32 [nprod]; redundancy [dev] float [nstack, nra]
 * dmm_vis_grid: the grid of MakeVisGrid.process (:166-176) as a gather: cell c of polarisation pol takes stack src[c]
 *   (conjugated where conj[c]) or stays empty (src < 0).
 *   vis [dev] complex64 [nfreq, nstack, nra], weight float same; src / conj [dev] [npol * ncell_pol];
 *   grid_vis [dev] complex64 [npol, nfreq, ncell_pol (= ew x ns), nra], grid_weight float same, grid_red int32 [npol, ncell_pol, nra] or NULL
 * dmm_beamform_ns: BeamformNS.process (:299-346) for all frequencies of the slab. weight_mode 0 inverse variance, 1 natural
 *   (redundancy), 2 a window table ns_window [dev] double [nfreq, ny] (window_generalised of the scaled baseline, made by the
 *   caller); the weights are masked by weight > 0, the autos dropped unless include_auto, normalised over ns.
 *   nspos [dev] double [ny] metres, el [dev] double [npix], inv_wavelength [host] double [nfreq] (1/m);
 *   hv [dev] complex64 [npol, nfreq, nx, npix, nra], hw float [npol, nfreq, nx, nra], dirty_beam float like hv or NULL.
 *   float64 arithmetic (the reference's `precision = 64`), float32 stores like the reference's containers.
 * dmm_beamform_ew: BeamformEW.process (:455-495): pol_rotation [dev] complex128 [npol_out, npol_in], weight_ew [dev] double
 *   [nx] (normalised; single_beam: the central beam only); map [dev] double [nbeam, npol_out, nfreq, nra, nel],
 *   weight [npol_out, nfreq, nra, nel], rms [npol_out, nfreq, nra]; dirty beam in (float, real) / out (like map) or both NULL.
 *   Limits: nx <= 8 and npol_in <= 4 (DMM_E_ARG beyond).  A row of pol_rotation may have at most two non-zero entries: the
 *   kernel keeps the first two it finds and silently drops the rest (BeamformEW._get_pol never makes more). */
int dmm_calc_redundancy(dmm_ctx* ctx, const float* input_flags, int ninput, int nra, const int32_t* prod_a, const int32_t* prod_b,
                        const int32_t* stack_index, int64_t nprod, int nstack, int all_good, float* redundancy);
int dmm_vis_grid(dmm_ctx* ctx, const void* vis, const float* weight, const float* redundancy, int nfreq, int nstack, int nra, int npol,
                 int ncell_pol, const int32_t* src, const uint8_t* conj, void* grid_vis, float* grid_weight, int32_t* grid_red);
int dmm_beamform_ns(dmm_ctx* ctx, int npol, int nfreq, int nx, int ny, int nra, int npix, int weight_mode, int include_auto,
                    const void* grid_vis, const float* grid_weight, const int32_t* grid_red, const double* ns_window,
                    const double* nspos, const double* el, const double* inv_wavelength /*[host]*/, void* hv, float* hw,
                    float* dirty_beam);
int dmm_beamform_ew(dmm_ctx* ctx, int npol_in, int npol_out, int nfreq, int nx, int nel, int nra, int single_beam, const void* hv,
                    const float* hw, const float* dirty_beam_in, const void* pol_rotation, const double* weight_ew, double* map,
                    double* weight, double* rms, double* dirty_beam_out);

/* ------------------------------------------------ synthetic beam-transfer tiles
 * Fill tiles with the counter-hash generator shared with oracle/synth.py
 * (bit-identical in float64): value(seed, m, f, row, pol, l) with l<m -> 0.
 * Used by SyntheticProvider / bench.py; not part of the reference.                  */
int dmm_synth_beam_fill(dmm_ctx* ctx, const dmm_tile* tiles /*[host]*/, int64_t ntile,
                        int npairs, int npol, int lmax, int b_dtype, int b_layout,
                        uint64_t seed, void* B);

/* ------------------------------------------------ physically structured synthetic beam transfers
 * Stand-in for the beam transfers driftscan computes from a telescope model [3P; what the reference reads through
 * bt.beam_m(m, fi=f), mapmaker.py:160-162]: a transit telescope at latitude `lat`, two feed polarisation types with one
 * complex Jones screen each, a primary beam of widths sigma_e / sigma_n (direction cosines), baselines sep_e / sep_n
 * (metres east / north).  dmm_beam_screen_maps writes the response maps (A_I, A_Q, A_U, A_V; npol = 1: A_I only) of
 * `npair` baselines at one wavelength, real parts then imaginary parts:
 *   maps [dev] double [2, npair, npol, 12 nside^2]  -- the layout dmm_map2alm takes with nfreq = 2 npair.
 * After dmm_map2alm(niter = 0) of those maps, dmm_beam_screen_pack writes rows s0 .. s0+nc-1 (both signs of m) of every
 * tile of the list into the pool:  B+ = conj(a_re) + i conj(a_im),  B- = conj(a_re) - i conj(a_im)  (0 for m = 0).
 *   alm [dev] complex128 [2, nc, npol, mmax_alm+1, lmax+1]
 * dmm_beam_screen_coeffs returns the 16 plane waves of the screens of a seed (host twin: oracle/synth.py).
 * sep_e, sep_n, pol_a, pol_b, tiles: host arrays.                                        */
int dmm_beam_screen_coeffs(uint64_t seed, int32_t* ka /*[16]*/, int32_t* kb, double* cr, double* ci);
int dmm_beam_screen_maps(dmm_ctx* ctx, int nside, int npol, double wavelength, double lat, uint64_t seed,
                         double sigma_e, double sigma_n, double eps_gain, double eps_leak, const double* sep_e,
                         const double* sep_n, const int32_t* pol_a, const int32_t* pol_b, int npair, double* maps);
int dmm_beam_screen_pack(dmm_ctx* ctx, const void* alm, int nc, int s0, const dmm_tile* tiles /*[host]*/,
                         int64_t ntile, int npairs, int npol, int lmax, int mmax_alm, int b_dtype, int b_layout,
                         void* B);

/* dmm_mmode_fill0: for every m the complex median (NumPy's order: real part, then imaginary) of the entries
 * whose weight is non-zero -- the first guess svd_em puts into the missing ones (reference
 * svdfilter.py:176); 0 where nothing is present.  mvis/mweight as below, viewed as [n_m, per_m];
 * fill0 [dev] complex128 [n_m].                                                                   */
int dmm_mmode_fill0(dmm_ctx* ctx, const void* mvis, const double* mweight, int n_m, int64_t per_m, void* fill0);

/* ------------------------------------------------- m-mode SVD filter
 * dmm_mmode_svd replaces the per-m loops of SVDSpectrumEstimator.process (reference
 * svdfilter.py:22-57) and SVDFilter.process (:79-149) including svd_em (:152-187): for every m
 * the matrix [freq, (msign, base)] of the MModes array, missing entries (weight == 0) refilled
 * `niter` times from its rank-`rank` approximation, is decomposed (frequency-side Gram matrix,
 * f64 MFMA + blocked Jacobi).  mvis/mweight: [n_m, 2, nfreq, nbase] complex128 / float64 (device).
 * fill0: [n_m] complex128 first guess of the missing entries (np.median of the present ones,
 * :176) or NULL when no weight is zero.  spectrum: [n_m, min(2 nbase, nfreq)] float64 (device).
 * mode 0: spectrum only; if u_out / uha_out are given (both or neither) the left singular vectors
 * [n_m, nfreq, nmode] and U^H A = diag(sigma) V^H [n_m, nmode, 2 nbase] of the last decomposition
 * are returned too (svd_em's factors).  mode 1: mvis is overwritten with the data whose
 * cut = max(#(sigma > global_thr*global_max), #(sigma > local_thr*sigma_0)) largest modes are removed. */
int dmm_mmode_svd(dmm_ctx* ctx, void* mvis, const double* mweight, int n_m, int nfreq, int nbase, int niter, int rank,
                  const void* fill0, int mode, double global_max, double global_thr, double local_thr, double* spectrum,
                  void* u_out, void* uha_out);

/* ------------------------------------------------- basis projections of m-modes (fgfilter.py)
 * SVDModeProject / KLModeProject (reference fgfilter.py:53-239) are, per m, matrix-vector products with a basis the
 * beam-transfer products hold [driftscan, 3P]: bt.project_vector_telescope_to_svd (:87), project_vector_svd_to_telescope
 * (:132), kl.project_vector_svd_to_kl (:193), project_vector_kl_to_svd (:229).  dmm_gemv_batch runs all of a
 * container's products in one launch: task t computes y[y_off .. y_off+nrow) = A_t x[x_off .. x_off+ncol) with
 * A_t = A[a_off ..], row-major [nrow, ncol], element type a_dtype (DMM_C64 / DMM_C128); x, y complex128.
 * A, x, y: [dev]; desc: [host].  Offsets are in elements. */
typedef struct {
  int64_t a_off;
  int64_t x_off;
  int64_t y_off;
  int32_t nrow;
  int32_t ncol;
} dmm_gemv_desc;
int dmm_gemv_batch(dmm_ctx* ctx, const void* A, int a_dtype, const dmm_gemv_desc* desc, int64_t ntask, const void* x, void* y);
/* out[r] = np.median(x[r, :]) for a [nrow, per_row] float64 array [dev] -- the weight the reference carries over to
 * the projected container (fgfilter.py:94,141,200,236: `np.median(mmodes.weight[mi])`). */
int dmm_row_median(dmm_ctx* ctx, const double* x, int64_t nrow, int64_t per_row, double* out);

/* ------------------------------------------------- sidereal regridding and day stacking
 * dmm_regrid_band_wiener replaces regrid.band_wiener (reference draco/util/regrid.py:14-89, with the compiled
 * _fast_tools._linear_covariance_banded, _fast_tools.pyx:59-88, and scipy's solveh_banded) as LanczosRegridder._regrid
 * calls it (draco/analysis/transform.py:951-986), the mix-down / mix-up of SiderealRegridder.process
 * (draco/analysis/sidereal.py:221-234, 256-278) fused into its load and store.  Per row k of `nrow` (one (frequency,
 * stack) pair), with R [ngrid, nt] the Lanczos matrix of the padded grid and bw = 2 kernel_width - 1:
 *   d = R (Ni_k o y_k),  C = band_bw(R diag(Ni_k) R^T),  nw = diag(C),  x = (C + eps I)^-1 d   (banded Cholesky)
 * all in float64 from the float32 / complex64 inputs; the first and last `pad` grid points are dropped, x is returned
 * as complex64 and nw as float32 (the reference's dtypes).  A row whose weights are all zero comes out as exact zeros.
 *
 * A plan holds R, which depends on the times only: per grid point g its span [span_start[g], span_end[g]) of time
 * samples with non-zero kernel values (empty where no sample is in reach: span_start = span_end) and, concatenated in
 * grid order, those values R[g, span_start[g] .. span_end[g]) as float64 -- lanczos_forward_matrix(grid, times).T
 * (regrid.py:109-135) evaluated on the host, no sinc on the device.  All three [host].  kernel_width 1 ... 6; a span
 * may hold at most 210 samples (the kernel's LDS tile) -- DMM_E_UNSUPPORTED otherwise.
 *
 * vis [nrow, nt] complex64, weight [nrow, nt] float32, out_vis [nrow, samples] complex64, out_weight [nrow, samples]
 * float32: [dev].  samples + 2 pad = the plan's ngrid.  mask_zero_weight: zero the weight of rows that had no non-zero
 * weight among the samples the grid reaches (transform.py:981-984).  Mixing (all four arrays [dev], or all NULL):
 * omega [nrow] float64 fringe rate, feed_mask [nrow] float32, dphi_in [nt] / dphi_out [samples] float64 sidereal
 * angle of the input samples / of the kept grid points (sidereal.py:256-278): the input is multiplied by
 * feed_mask exp(-i omega dphi_in) as it is loaded (rounded to complex64, as the reference's in-place product is),
 * the output by the conjugate factor at dphi_out as it is stored, and the weight of rows with feed_mask = 0 is zeroed.
 * The factor rows go through the context's scratch, rows in chunks sized by the "regrid_workspace_mib" option. */
typedef struct dmm_regrid_plan dmm_regrid_plan;
int dmm_regrid_plan_create(dmm_ctx* ctx, int nt, int ngrid, int kernel_width, const int32_t* span_start, const int32_t* span_end,
                           const double* kernel_values, dmm_regrid_plan** plan);
int dmm_regrid_plan_destroy(dmm_regrid_plan* plan);
int dmm_regrid_band_wiener(dmm_ctx* ctx, const dmm_regrid_plan* plan, const void* vis, const float* weight, int64_t nrow, double eps,
                           int pad, int samples, int mask_zero_weight, const double* omega, const float* feed_mask,
                           const double* dphi_in, const double* dphi_out, void* out_vis, float* out_weight);
/* SiderealStacker (draco/analysis/sidereal.py:834-1080), one fused element-wise launch per day: West's update of the
 * running mean `stack_vis` (complex64) and, with_variance, of the three sums of squared differences
 * `sample_variance` [3, n] float32 and of `sum_coeff_sq` [n] float32 (:975-1030), float32 state and the reference's
 * order of operations.  mode: DMM_STACK_UNIFORM / DMM_STACK_INVERSE_VARIANCE.  day_nsample [n] uint16 or NULL (the day
 * is a single day: count = weight > 0).  Divisions are invert_no_zero (0 where the divisor is 0).  The caller zeroes
 * the state before the first day.  dmm_sidereal_stack_finish is process_finish (:1032-1065): the weight normalisation
 * of the uniform mode and Bessel's correction of the sample variance.  All arrays [dev], n elements = freq * stack * ra. */
enum { DMM_STACK_UNIFORM = 0, DMM_STACK_INVERSE_VARIANCE = 1 };
int dmm_sidereal_stack_add(dmm_ctx* ctx, int mode, int with_variance, const void* day_vis, const float* day_weight,
                           const uint16_t* day_nsample, void* stack_vis, float* stack_weight, uint16_t* stack_nsample,
                           float* sum_coeff_sq, float* sample_variance, int64_t n);
int dmm_sidereal_stack_finish(dmm_ctx* ctx, int mode, int with_variance, float* stack_weight, const uint16_t* stack_nsample,
                              const float* sum_coeff_sq, float* sample_variance, int64_t n);

/* Sidereal rebinning, its gradient correction and the direct interpolators, csrc/rebin.hip (draco/analysis/sidereal.py:
 * 550-731 SiderealRebinner, :734-831 RebinGradientCorrection, :349-547 SiderealRegridderNearest / Linear / Cubic).
 * Float64 arithmetic from the float32 / complex64 inputs, every output rounded once; no atomics: two runs agree bit
 * for bit.
 *
 * dmm_rebin: one pass over vis [nrow, nt] complex64 and weight [nrow / fold, nt] float32 (row k reads weight row
 * k / fold: fold = 1 for a stream, the length of the `el` axis for a HybridVisStream).  The rebinning matrix
 * R [nra, nt] (regrid.py:161-211) comes in CSR form by output bin: row_ptr [nra + 1], sample_index [nnz] ascending
 * within a bin, value [nnz] float64; tile_span [ceil(nra / 64), 2] holds, per tile of 64 bins, the first and one past
 * the last sample its bins read (0, 0 for a tile without samples).  lsd [nt] float64 are the samples' sidereal days,
 * ra [nra] float64 the bin centres in degrees, start the day's LSD.  Per row and bin g, with (w, v) = (weight, weight)
 * for DMM_REBIN_INVERSE_VARIANCE and (weight > 0, float32(invert_no_zero(weight))) for DMM_REBIN_UNIFORM, summed in
 * ascending sample order:
 *   norm = inz(sum R w),  out_vis = norm sum R w vis,  out_nsample = sum R (weight > 0),
 *   out_weight = inz(norm^2 sum R^2 v),  out_effective_ra = 360 (norm sum R w lsd - start), ra[g] where out_weight = 0
 * out_vis [nrow, nra] complex64; out_weight, out_effective_ra [nrow / fold, nra] float32; out_nsample [nrow / fold,
 * nra] uint16 (truncated toward zero) or, with nsample_f32, float32.  All arrays [dev]; vis and weight 16-byte aligned
 * (DMM_E_ARG otherwise).  Limits: nra <= 64 * 65535 (DMM_E_UNSUPPORTED beyond); a bin may hold any number of samples.
 *
 * dmm_rebin_gradient, in place on vis / weight [nrow, nra]: per row that has a non-zero weight, the gradient of the
 * reference row ref_vis (flagged where ref_weight = 0) over its positions -- ref_effective_ra [nrow, nra] float32 or
 * ref_ra [nra] float64, exactly one of the two non-NULL -- wrapped with period 360 (regrid.py:214-270, np.gradient's
 * second-order formula for uneven spacing); a gradient that touches a flagged sample, an interval of zero length or is
 * not finite is flagged and zero.  Then vis -= gradient (weight > 0) (effective_ra - ra), weight *= !flagged.  The
 * reference arrays may be the arrays being corrected.  All [dev].  nra <= DMM_MAX_NRA (DMM_E_UNSUPPORTED beyond).
 *
 * dmm_regrid_interp: out_vis[k, o] = sum_t coeff[t, o] vis[k, tap[t, o]] for ntap = 1 (nearest), 2 (linear) or 4
 * (cubic) taps; tap [ntap, nout] int32, coeff [ntap, nout] float64, bad [nout] uint8 as the host evaluates them
 * (sidereal.py:365-547).  ntap = 1 copies the weight; otherwise out_weight = inz(sum coeff^2 float32(inz(weight)))
 * where every tap has weight > 0, else 0.  out_weight = 0 where bad.  Mixing arrays as for dmm_regrid_band_wiener,
 * dphi_out [nout].  vis, weight [nrow, nt]; out_vis, out_weight [nrow, nout]; all [dev]. */
enum { DMM_REBIN_UNIFORM = 0, DMM_REBIN_INVERSE_VARIANCE = 1 };
int dmm_rebin(dmm_ctx* ctx, int mode, int nsample_f32, const void* vis, const float* weight, int64_t nrow, int fold, int nt, int nra,
              const int32_t* row_ptr, const int32_t* sample_index, const double* value, int nnz, const int32_t* tile_span,
              const double* lsd, double start, const double* ra, void* out_vis, float* out_weight, void* out_nsample,
              float* out_effective_ra);
int dmm_rebin_gradient(dmm_ctx* ctx, void* vis, float* weight, const float* effective_ra, const double* ra, const void* ref_vis,
                       const float* ref_weight, const float* ref_effective_ra, const double* ref_ra, int64_t nrow, int nra);
int dmm_regrid_interp(dmm_ctx* ctx, int ntap, const void* vis, const float* weight, int64_t nrow, int nt, int nout,
                      const int32_t* tap, const double* coeff, const uint8_t* bad, const double* omega, const float* feed_mask,
                      const double* dphi_in, const double* dphi_out, void* out_vis, float* out_weight);

/* DAYENU delay filter (draco/analysis/dayenu.py:20-193, 776-975, 1125-1232), csrc/dayenu.hip.
 *
 * dmm_dayenu_build: nmat filters of order nfreq (1 ... 1024) at once.  freq [nfreq] float64 (MHz), bands
 * [nmat][nband][2] float64 = (half width tw in micro-seconds, eps) of each stop band (centre 0), mask [nmat][nfreq]
 * bytes (non-zero: channel kept), all [dev].  Per matrix: C = I + sum_k sinc(2 tw_k (nu_f - nu_f')) / eps_k on the kept
 * channels (1 on the diagonal of the others), Cholesky-factored and inverted in float64, nf [nmat][nfreq][nfreq] =
 * C^-1 o (mask x mask) [dev].  status [nmat] int32 [dev]: 0, or 1 where a pivot was not positive (that matrix is
 * left zero, nothing else is touched).  One more nfreq^2 float64 per matrix comes from the context's scratch.
 *
 * A container side (dmm_dayenu_side) describes one dataset as seen by the filter, in ELEMENTS of the real dtype: the
 * value of frequency f, column c of item (outer o, inner i) is ptr[o stride_outer + i stride_inner + c stride_col +
 * f stride_freq]; ncol columns per item.  A complex dataset is a real one with twice the columns.  layout:
 * DMM_DAYENU_COLS = the columns of an item are contiguous (stride_col 1: vis [freq, stack, ra]), DMM_DAYENU_ITEMS =
 * the inner items are (stride_inner 1: map [beam, pol, freq, ra, el], items el, columns ra).
 *
 * dmm_dayenu_mask: flag [nouter][ninner][nfreq] bytes [dev] = all_c(weight > 0), and weight *= flag in the same pass.
 *
 * dmm_dayenu_apply (in place): data <- NF data and weight <- inz((NF o NF) inz(weight)) for every item, NF =
 * nf[item_matrix[item]], on the f64 matrix cores, rounded once to dtype on the store.  item_matrix [nouter][ninner]
 * int32 [dev]: -1 = leave the item alone, -2 = leave its data alone and zero its weight (a failed build).  atten
 * [nmat][nfreq] bytes [dev] or NULL: where zero, the weight of that frequency is stored as 0.  units [nunit] int32
 * [dev] or NULL: the units the launch covers (NULL: unit u = u, nunit of them) -- an item o ninner + i for
 * DMM_DAYENU_COLS, a group of adjacent items o ngroup + g for DMM_DAYENU_ITEMS (groups of 32 for DMM_DAYENU_F32, of 16
 * for DMM_DAYENU_F64; ngroup = ceil(ninner / group)).  data or weight may be NULL (that side is skipped). */
enum { DMM_DAYENU_F32 = 0, DMM_DAYENU_F64 = 1 };
enum { DMM_DAYENU_COLS = 0, DMM_DAYENU_ITEMS = 1 };
typedef struct dmm_dayenu_side {
  void* ptr;
  int64_t ncol, stride_freq, stride_col, stride_inner, stride_outer;
} dmm_dayenu_side;
int dmm_dayenu_build(dmm_ctx* ctx, int nfreq, int nmat, int nband, const double* freq, const double* bands, const uint8_t* mask,
                     double* nf, int32_t* status);
int dmm_dayenu_mask(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, const dmm_dayenu_side* weight, uint8_t* flag);
int dmm_dayenu_apply(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, const double* nf, int nmat,
                     const int32_t* item_matrix, const uint8_t* atten, const int32_t* units, int64_t nunit,
                     const dmm_dayenu_side* data, const dmm_dayenu_side* weight);

/* Delay null-space filter (draco/util/filters.py:133-212, draco/analysis/delay.py:29-339), csrc/nullfilter.hip.
 *
 * dmm_nullfilter_build: nmat filters of order nfreq (1 ... 1024) in one launch, one block per matrix.  num_modes (2 ...
 * 1024) is the pitch of the per-matrix tables; nmodes [nmat] int32 [dev] holds each matrix's own number of Fourier modes
 * (2 ... num_modes; anything else sets status 2 and leaves nf of that matrix with no mode projected), NULL: all num_modes.
 * samples [nfreq] float64, modes [nmat][num_modes] float64 = numpy.linspace(-cutoff, cutoff, num_modes) of each matrix
 * (ascending and symmetric about zero: only the positive half of the first nmodes entries is read), mask [nmat][nfreq] bytes (non-zero: channel
 * kept), window [nfreq] float64 or NULL, all [dev].  Per matrix the real form Fr [nfreq][num_modes] of the masked,
 * windowed Fourier matrix (columns sqrt2 cos / sqrt2 sin of the positive modes, ones for the zero mode of an odd
 * num_modes) is factored by a one-sided Jacobi SVD in float64; sig [nmat][num_modes] [dev] = its singular values (in
 * the order the columns end in, which is not sorted), nkeep [nmat] int32 [dev] = #(sig > tol max sig),
 * U = the left singular vectors of those, and nf [nmat][nfreq][nfreq] [dev] = (I - U U^T) o (1 x mask) o (1 x window)
 * for low = 0, (U U^T) o (1 x mask) o (1 x window) for low = 1: mask and window scale the columns only.  status [nmat]
 * int32 [dev]: 0, or 1 where the sweeps did not converge within the cap of 60 (nf of that matrix is not to be used).
 * sweeps [nmat] int32 [dev] or NULL: the sweeps each matrix took.  nmat num_modes nfreq float64 of the context's
 * scratch hold the factors.
 *
 * dmm_nullfilter_mask: the weight as a dmm_dayenu_side (above), dtype and layout as for dmm_dayenu_mask.  Per item
 * f_samp[f] = #c(weight > 0), flag [nouter][ninner][nfreq] bytes [dev] = (f_samp == max_f f_samp), t_mask[c] likewise
 * from t_samp[c] = #f(weight > 0), and weight *= flag x t_mask in place (an item without weight keeps both masks full
 * and its zeros).  join_outer = 1: the nouter items of one inner index are one item with nouter ncol samples (the two
 * polarisations of a ring map's el): f_samp is summed over them, both maxima are joint, and they get the same flag.
 * nitem (nfreq + ncol) int32 of the context's scratch hold the counts.
 *
 * The filters are applied with dmm_dayenu_apply (weight and atten NULL). */
int dmm_nullfilter_build(dmm_ctx* ctx, int nfreq, int nmat, int num_modes, const int32_t* nmodes, int low, double tol, const double* samples, const double* modes,
                         const uint8_t* mask, const double* window, double* nf, double* sig, int32_t* nkeep, int32_t* status, int32_t* sweeps);
int dmm_nullfilter_mask(dmm_ctx* ctx, int dtype, int layout, int nfreq, int ninner, int nouter, int join_outer, const dmm_dayenu_side* weight,
                        uint8_t* flag);

/* DAYENU filter of hybrid beam-formed visibilities (draco/analysis/dayenu.py:407-572) and the east-west averages of
 * RADependentWeights (draco/analysis/ringmapmaker.py:1202-1315), csrc/dayenu_hybrid.hip.  All arrays [dev]; weight is
 * the stream's vis_weight [npol][nfreq][new][nra] float32, and there is one filter per (ew, ra) sample: item_matrix
 * [new][nra] int32 indexes nf [nmat][nfreq][nfreq] float64 (negative or >= nmat: no filter).  The filters come from
 * dmm_dayenu_build and are applied with dmm_dayenu_apply (DMM_DAYENU_F32, DMM_DAYENU_ITEMS: items along ra).
 *
 * dmm_dayenu_hybrid_mask: flag [nfreq][new][nra] bytes = all_pol(weight > 0).  The weights are not changed.
 *
 * dmm_dayenu_hybrid_save: out [npol][nfreq][nfreq][new][nra] float64 = nf[item_matrix[x][t]][f][f'] for every pol.
 * dmm_dayenu_hybrid_cov: out (same shape) = sum_k nf[m][f][k] nf[m][f'][k] inz(weight[p][k][x][t]), m =
 * item_matrix[x][t], inz taken in float32, the sum in float64 on the matrix cores in an order that depends on the
 * sample alone; symmetric in (f, f') bit for bit.
 * Both: a sample without a filter is stored as zero if skip_negative is 0 and left untouched otherwise (the later
 * launches of a build in batches).
 *
 * dmm_ew_coef, per (pol, freq): mean [x] = mean_ra inz(weight); w [x] = table[x] (DMM_EW_TABLE: the natural or uniform
 * weights, excluded baselines zero) or inz(mean[x]) table[x] (DMM_EW_INVERSE_VARIANCE: table 1 or 0); coef_filter
 * [npol][nfreq][new] = w inz(sum w), coef_cov = w^2 inz((sum w)^2), w2 = w^2, num [npol][nfreq] = sum w^2 mean.
 * 1 <= new <= 64.
 * dmm_ew_scale: ringmap_weight [npol][nfreq][nra][nel] float64 *= num inz(sum_x w2[x] inz(weight[p][f][x][t])).
 * dmm_ew_average: out [nrow][nra] = sum_x coef[row / rows_per_coef][x] in[row][x][t], float64, in ew order (one
 * rounding per product and per addition). */
enum { DMM_EW_TABLE = 0, DMM_EW_INVERSE_VARIANCE = 1 };
int dmm_dayenu_hybrid_mask(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const float* weight, uint8_t* flag);
int dmm_dayenu_hybrid_save(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const double* nf, int nmat, const int32_t* item_matrix,
                           int skip_negative, double* out);
int dmm_dayenu_hybrid_cov(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, const double* nf, int nmat, const int32_t* item_matrix,
                          const float* weight, int skip_negative, double* out);
int dmm_ew_coef(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int scheme, const double* table, const float* weight,
                double* coef_filter, double* coef_cov, double* w2, double* num);
int dmm_ew_scale(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int nel, const float* weight, const double* w2, const double* num,
                 double* ringmap_weight);
int dmm_ew_average(dmm_ctx* ctx, int64_t nrow, int64_t rows_per_coef, int new_, int nra, const double* coef, const double* in, double* out);

/* Stored per-sample delay filters on hybrid visibilities (draco/analysis/dayenu.py:575-773) and the HyFoReS bandpass
 * estimate (draco/analysis/hyforesbandpass.py), csrc/hyfores.hip.  All arrays [dev]: filter / freq_cov
 * [npol][nfreq][nfreq][new][nra] float64 (real filters only), vis / post / vis_out [npol][nfreq][new][nel][nra]
 * complex64, weight / weight_out [npol][nfreq][new][nra] float32.  1 <= nfreq <= 1024, npol * new <= 65535,
 * nel <= 65535.  Every sum is float64 in an order fixed by the shapes: two calls agree bit for bit.
 *
 * dmm_hybrid_filter_apply, per (pol, ew, ra) sample with flag[k] = weight[k] > 0 (per polarisation):
 *   status [npol][new][nra] bytes = DMM_HFA_SKIPPED (no flag set), DMM_HFA_ZERO_FILTER (the filter is entirely zero),
 *   DMM_HFA_MISSING_FREQ (a column k of the filter is non-zero where flag[k] is not set) or DMM_HFA_OK;
 *   OK:  vis_out[f][l] = sum_k filter[f][k] d[k] vis[k][l], rounded to complex64 at the end; d = 1 - gain[p][x][k]
 *        (gain [npol][new][nfreq] complex128) or 1 where gain is NULL; with var[k] = inz(weight[k]) |d[k]|^2 (inz in
 *        float32): weight_out[f] = inz(sum_k filter[f][k]^2 var[k]) atten[f] and freq_cov[f][f'] = sum_k (filter[f][k]
 *        filter[f'][k]) var[k], symmetric bit for bit; atten [npol][nfreq][new][nra] bytes (0 or 1) or NULL, applied to
 *        vis_out too if atten_vis is set;
 *   otherwise: vis_out = vis (keep_input set) or 0, freq_cov = 0, weight_out = weight (skipped) or 0.
 *   weight_out and freq_cov may be NULL (not computed).  Works out of place: vis_out != vis, weight_out != weight.
 *   bits [npol][new][nra] uint32 is scratch.
 *
 * The estimate, with m[f][l][t] = (weight[f][t] > 0) && elm[l] && !pix[p][f][l][t] (elm [nel] bytes, pix
 * [npol][nfreq][nel][nra] bytes or NULL), g = (vis - post) m and s = post m formed in float64:
 * dmm_hyfores_gain: yn [npol][new][nfreq] complex128 = sum_{l, t} conj(g) s, d [npol][new][nfreq] float64 =
 *   sum_{l, t} |g|^2.
 * dmm_hyfores_window: window [npol][new][nfreq][nfreq] complex128, [f][f'] = sum_t filter[f][f'][t] sum_l conj(g[f][l][t])
 *   g[f'][l][t]; partial is scratch of ceil(nra / DMM_HYFORES_RUN) * npol * new * nfreq * nfreq complex128: the sums of
 *   each run of RA, added in run order by a second pass. */
enum { DMM_HFA_OK = 0, DMM_HFA_SKIPPED = 1, DMM_HFA_ZERO_FILTER = 2, DMM_HFA_MISSING_FREQ = 3 };
#define DMM_HYFORES_RUN 64
int dmm_hybrid_filter_apply(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const double* filter, const void* vis, const float* weight,
                            const double* gain, const uint8_t* atten, int atten_vis, int keep_input, void* vis_out, float* weight_out, double* freq_cov,
                            uint32_t* bits, uint8_t* status);
int dmm_hyfores_gain(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const void* vis, const void* post, const float* weight,
                     const uint8_t* elm, const uint8_t* pix, double* yn, double* d);
int dmm_hyfores_window(dmm_ctx* ctx, int npol, int nfreq, int new_, int nel, int nra, const double* filter, const void* vis, const void* post,
                       const float* weight, const uint8_t* elm, const uint8_t* pix, double* partial, double* window);

/* Frequency-correlated noise (draco/analysis/ringmapmaker.py:1318-1712, draco/synthesis/noise.py:377-470),
 * csrc/noisemodel.hip.  All arrays [dev].  cov [npol][nfreq][nfreq][new][nra] float64 (real covariances only), scale
 * [npol][nfreq][nfreq][new] float64, weight / weight_out [npol][nfreq][new][nra] float32.  1 <= nfreq <= 1024,
 * npol * new <= 65535.  A sample is s = (pol new + ew) nra + ra; a call takes the nsample <= 65535 samples from `first`
 * on, and no result depends on how the samples are split over calls.  A channel is valid where weight > 0.
 *
 * dmm_noisemodel_pack: G [nsample][nfreq][nfreq], upper triangle only: G[i][j] = cov[j][i] scale[j][i] (the input's lower
 *   triangle) where i and j are valid, the identity's entry where one is not; weight_out[f] = inz(G[f][f]) rounded to
 *   float32, 0 on invalid channels.
 * dmm_noisemodel_factor: G = U^T U in place (upper triangle); status [nsample] int32 is cleared, then set to
 *   DMM_NOISE_NOT_POSDEF where a pivot is not positive.
 * dmm_noisemodel_store: freq_cov [npol][new][nra][nfreq][nfreq] (the whole array; the call writes its samples):
 *   [r][c] = U[c][r] for c <= r both valid, 0 elsewhere and in every sample whose status is set.
 * dmm_noisemodel_weight: vis_weight [nfreq][nstack][nra] float32 = float(nbaseline[stack] (double(weight[p][f][x][ra])
 *   noise_factor[p][f][x])) with p new + x = cell[stack] (int32), 0 where cell[stack] < 0; noise_factor [npol][nfreq][new]
 *   and nbaseline [nstack] float64.
 * dmm_noise_colour, for the slab (pol, ew): vis[pol][f][ew][ns][ra] = (sum_{k <= f} chol[pol][ew][ra][f][k] z[ra][k][ns])
 *   inv_sqrt_red[pol][ew][ns], z [nra][nfreq][nns] complex64, sums in float64 with k ascending, rounded once to
 *   complex64 (chol is taken as lower triangular: its strict upper triangle is not read);
 *   vis_weight[pol][f][ew][ns][ra] = float(double(weight[pol][f][ew][ra]) redundancy[pol][ew][ns]).  chol is
 *   the whole [npol][new][nra][nfreq][nfreq] array, vis / vis_weight the whole [npol][nfreq][new][nns][nra] arrays,
 *   redundancy int32 and inv_sqrt_red float64 [npol][new][nns].
 * dmm_noise_hermitian, in place on ew = 0, nns odd: vis[pconj[p]][f][0][nns - k][ra] = conj(vis[p][f][0][k][ra]) for
 *   k = 1 ... nns / 2, and where pconj[p] == p the auto k = 0 becomes (sqrt(2) Re, 0) in float32; pconj [npol] int32 with
 *   entries in 0 ... npol - 1; npol * nfreq <= 65535. */
enum { DMM_NOISE_OK = 0, DMM_NOISE_NOT_POSDEF = 1 };
int dmm_noisemodel_pack(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int64_t first, int nsample, const double* cov, const double* scale, const float* weight,
                        double* G, float* weight_out);
int dmm_noisemodel_factor(dmm_ctx* ctx, int nfreq, int nsample, double* G, int32_t* status);
int dmm_noisemodel_store(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int64_t first, int nsample, const double* G, const float* weight, const int32_t* status,
                         double* freq_cov);
int dmm_noisemodel_weight(dmm_ctx* ctx, int npol, int nfreq, int new_, int nra, int nstack, const float* weight, const double* noise_factor, const int32_t* cell,
                          const double* nbaseline, float* vis_weight);
int dmm_noise_colour(dmm_ctx* ctx, int npol, int nfreq, int new_, int nns, int nra, int pol, int ew, const double* chol, const void* z, const float* weight,
                     const int32_t* redundancy, const double* inv_sqrt_red, void* vis, float* vis_weight);
int dmm_noise_hermitian(dmm_ctx* ctx, int npol, int nfreq, int new_, int nns, int nra, const int32_t* pconj, void* vis);

/* Delay spectrum estimators (draco/analysis/delay.py:347-1106, 2102-2201), csrc/delay.hip.  All arrays [dev] unless
 * noted, everything float64.  ndelay = N; order = N in the real time domain, 2 N (alternating real and imaginary) in
 * the complex one; nchan channels with indices chan [nchan] int32 in the full set; baselines are batched, at most
 * 65535 per call.
 *
 * dmm_delay_fourier: F [2 nchan][order], rows 2 f and 2 f + 1 the real and imaginary row of channel chan[f]
 * (fourier_matrix_r2c / fourier_matrix_c2c); the arguments are reduced as (chan t) mod N in integers.
 *
 * A view (dmm_delay_view) describes a dataset as [baseline, sample, freq] in ELEMENTS of its dtype (a complex element
 * is one element): baseline base0 + b is split over the nfold folded axes of lengths fold_n [host], slowest first, and
 * lies at sum_q index_q stride_fold[q]; a weight dataset that lacks a folded axis has stride 0 there.
 *
 * dmm_delay_prepare: per baseline the sample mask nzt [nbase][nsample] bytes (share of channels with weight > 0 above
 * time_frac), the channel mask over the retained samples (above freq_frac), status [nbase] int32 (DMM_DELAY_SKIPPED:
 * no positive weight, nothing retained, or all-zero data after mean removal; DMM_DELAY_CUT: a channel is cut and
 * wiener = 0), and X [nbase][nrow][2 nchan] = c o (d - mean) on the retained samples, zero rows elsewhere.  wiener = 1:
 * nrow = nsample + 1, c = coef[f] x (average weight x weight_boost) x (1 on the real row and 0 on the imaginary row of
 * channels 0 and N / 2 in the real time domain, 2 elsewhere), zero on cut channels, and the last row of X is c on the
 * real rows; wiener = 0: nrow = nsample, c = coef[f].  The inputs are not modified.
 *
 * dmm_delay_project: Y [nbase][nrow][order] = X F on the f64 matrix cores.
 *
 * dmm_delay_solve (order 1 ... 2048): G [nbase][order][order] (workspace) = circ(last row of Y) + diag(Si), Si
 * [nbase][order]; G = U^T U blocked, then each of the nsample rows of Y is replaced by the solution of G x = y.  A non-positive
 * pivot sets status to DMM_DELAY_NOT_POSDEF and nothing further is computed for that baseline.
 *
 * dmm_delay_store: spectrum [nbase][nsample][ndelay] complex128 = numpy.fft.fftshift of the rows of Y (zero imaginary
 * part in the real time domain), zeros where nzt is 0 or status is set; mask [nbase][nsample] bytes (or NULL): 1
 * there. */
enum { DMM_DELAY_F32 = 0, DMM_DELAY_F64 = 1, DMM_DELAY_C64 = 2, DMM_DELAY_C128 = 3 };
enum { DMM_DELAY_OK = 0, DMM_DELAY_SKIPPED = 1, DMM_DELAY_NOT_POSDEF = 2, DMM_DELAY_CUT = 3 };
typedef struct dmm_delay_view {
  const void* ptr;
  int dtype;
  int64_t stride_sample, stride_freq, stride_fold[4];
} dmm_delay_view;
int dmm_delay_fourier(dmm_ctx* ctx, int ndelay, int nchan, int complex_td, const int32_t* chan, double* F);
int dmm_delay_prepare(dmm_ctx* ctx, int ndelay, int nchan, int nsample, int nbase, int64_t base0, int nfold, const int64_t* fold_n,
                      const dmm_delay_view* data, const dmm_delay_view* weight, int complex_td, int wiener, int remove_mean,
                      double time_frac, double freq_frac, double weight_boost, const double* coef, const int32_t* chan, double* X,
                      uint8_t* nzt, int32_t* status);
int dmm_delay_project(dmm_ctx* ctx, int order, int nchan, int nrow, int nbase, const double* X, const double* F, double* Y,
                      const int32_t* status);
int dmm_delay_solve(dmm_ctx* ctx, int order, int complex_td, int nsample, int nbase, double* Y, const double* Si, double* G,
                    int32_t* status);
int dmm_delay_store(dmm_ctx* ctx, int ndelay, int complex_td, int nsample, int nrow, int nbase, const double* Y, const uint8_t* nzt,
                    const int32_t* status, void* spectrum, uint8_t* mask);

/* Delay power spectrum by NRML (draco/analysis/delayopt.py:61-355, delay.py:1270-1301), csrc/nrml.hip: value, gradient,
 * Hessian and Newton-CG direction of the maximum a posteriori problem in x = log S, batched over baselines (at most
 * 65535 per call).  All arrays [dev], float64.  nchan = n <= 1024 channels, ndelay = N <= 2048 delays.  A complex
 * n-vector is held as the real 2n-vector [Re ; Im], a Hermitian matrix as its real embedding [[A, -B], [B, A]] of
 * order 2n.  Every call leaves a baseline alone whose status word (the DMM_DELAY_* values) is set.
 *
 * dmm_nrml_start: from two calls of dmm_delay_prepare with complex_td = 1 and coef = 1: Xp [nbase][nsample + 1][2 n],
 * nzt and status of wiener = 1 (its last row is twice the averaged weight) and Xd [nbase][nsample][2 n] of wiener = 0
 * (the mean-removed data themselves).  win [n] is the window at chan / N.  Writes tw [N][2] = (cos, sin)(2 pi m / N), wv [nbase][n] (the window, zero on a
 * channel without weight), Nm [nbase][n] (the noise variance), Xe [nbase][2n][2n] (the covariance of the windowed
 * data over the retained samples), nsv [nbase] (their number) and S0 [nbase][N], the starting spectrum: the variance
 * over the samples of the unwindowed data of the channels with |w| > 1e-3 max |w|, transformed to delay.  Scratch: work
 * [nbase][3][nsample][2 n], F2 [2 n][2 N], Z [nbase][nsample][2 N].
 *
 * dmm_nrml_eval: value [nbase] and grad [nbase][N] at x [nbase][N]; the likelihood sees x clipped to [lo, hi], the
 * prior (Ci [N][N], the inverse kernel) sees x.  Leaves U, Y (= C^-1 U in its first N rows) and R in the workspace.
 * A non-positive pivot sets status to DMM_DELAY_NOT_POSDEF.  Workspace: S [nbase][N], sh [nbase][N][2], G and D
 * [nbase][2n][2n], U and R [nbase][N][2n], Y [nbase][N + n][2n], t and cix [nbase][N].
 *
 * dmm_nrml_hessian: H [nbase][N][N] (symmetric, both triangles) from that workspace, with the reference's Re(P_ab^2)
 * as first term; exact = 0 gives the Fisher form.
 * P and Q are formed by matrix products into the planes PQ [nbase][4][N][N] (Re P, Im P, Re Q, Im Q) of the workspace
 * and combined element-wise.
 *
 * dmm_nrml_direction: scipy's truncated conjugate gradient for H p = -g, p [nbase][N]; info [nbase][2] = (passes, flag),
 * flag 3 when the 20 N passes ran out. */
typedef struct dmm_nrml_ws {
  const int32_t* chan;
  const double *tw, *wv, *Nm, *Xe, *nsv, *Ci;
  double *S, *sh, *G, *D, *U, *Y, *R, *t, *cix, *PQ;
} dmm_nrml_ws;
int dmm_nrml_start(dmm_ctx* ctx, int ndelay, int nchan, int nsample, int nbase, const int32_t* chan, const double* win,
                   const double* Xp, const double* Xd, const uint8_t* nzt, const int32_t* status, double* work, double* F2, double* Z, double* tw,
                   double* wv, double* Nm, double* Xe, double* nsv, double* S0);
int dmm_nrml_eval(dmm_ctx* ctx, int ndelay, int nchan, int nbase, const dmm_nrml_ws* ws, const double* x, double lo, double hi,
                  int32_t* status, double* value, double* grad);
int dmm_nrml_hessian(dmm_ctx* ctx, int ndelay, int nchan, int nbase, const dmm_nrml_ws* ws, int exact, const int32_t* status,
                     double* H);
int dmm_nrml_direction(dmm_ctx* ctx, int ndelay, int nbase, const double* H, const double* g, const int32_t* status, double* p,
                       int32_t* info);

/* DAYENU m-mode filter along right ascension (draco/analysis/dayenu.py:977-1122, 1235-1427), csrc/mfilter.hip.  All
 * arrays [dev]; the order nra is 1 ... 4096 in every call, matrices are batched, at most 65535 per call.
 *
 * dmm_mfilter_mask: weight [nfreq][nstack][nra] float32 (in place), nfreq <= 65535.  Per frequency, with gb = the stack
 * entries that have any weight > 0: flag [nfreq][nra] bytes = (number of gb entries with weight > 0 at that RA) >
 * 0.90 * len(gb), compared in float64; state [nfreq] int32 = DMM_MFILTER_UNTOUCHED (gb is empty: weight not written,
 * flag 0), DMM_MFILTER_WEIGHT_ONLY (no RA is kept) or DMM_MFILTER_FILTER; unless untouched, weight *= flag.  nfreq x
 * nstack bytes come from the context's scratch.
 *
 * dmm_mfilter_cov: ra [nra] float64 (radians), params [nmat][4] float64 = (diag, coef, m_cut, m_center), mask
 * [nmat][nra] bytes (non-zero: RA kept).  G [nmat][nra][nra] float64 = diag d_ij + coef sinc(m_cut (ra_i - ra_j) / pi)
 * cos(m_center (ra_i - ra_j)) (sinc(x) = sin(pi x) / (pi x), sinc(0) = 1) on the kept RAs, identity on the rows and
 * columns of the others.  status [nmat] int32 is reset to 0.
 *
 * dmm_mfilter_pack / dmm_mfilter_unpack: vis [.][nstack][nra] complex64; matrix t belongs to frequency mat_freq[t]
 * (int32 [nmat]) and carries the nent stack entries entry [nent] int32.  Y [nmat][2 nent][nra] float64: rows 2 e and
 * 2 e + 1 are the real and imaginary part of vis[mat_freq[t]][entry[e]] x exp(-i mix[t][e] ra), zero where mask is 0;
 * mix [nmat][nent] float64 or NULL (no mixer).  Unpack multiplies by the conjugate mixer, rounds once to complex64 and
 * stores exact zeros where mask is 0.  Both leave a matrix whose status is non-zero alone.
 *
 * dmm_mfilter_solve: G = U^T U in place (blocked, float64 matrix cores), then each of the nrow rows of Y
 * [nmat][nrow][nra] is replaced by the solution of G x = y; nrow may be 0.  A pivot that is not positive sets status to
 * DMM_MFILTER_NOT_POSDEF and nothing further is computed for that matrix.
 *
 * dmm_mfilter_eye, on Y [nmat][nra][nra]: stage 0 writes the masked identity (the right-hand sides that give the
 * filter matrix itself), stage 1 zeroes the rows and columns where mask is 0 (the whole matrix where status is set). */
enum { DMM_MFILTER_UNTOUCHED = 0, DMM_MFILTER_WEIGHT_ONLY = 1, DMM_MFILTER_FILTER = 2 };
enum { DMM_MFILTER_OK = 0, DMM_MFILTER_NOT_POSDEF = 1 };
int dmm_mfilter_mask(dmm_ctx* ctx, int nfreq, int nstack, int nra, float* weight, uint8_t* flag, int32_t* state);
int dmm_mfilter_cov(dmm_ctx* ctx, int nra, int nmat, const double* ra, const double* params, const uint8_t* mask, double* G,
                    int32_t* status);
int dmm_mfilter_pack(dmm_ctx* ctx, int nra, int nstack, int nmat, int nent, const int32_t* mat_freq, const int32_t* entry,
                     const double* mix, const double* ra, const uint8_t* mask, const int32_t* status, const void* vis, double* Y);
int dmm_mfilter_unpack(dmm_ctx* ctx, int nra, int nstack, int nmat, int nent, const int32_t* mat_freq, const int32_t* entry,
                       const double* mix, const double* ra, const uint8_t* mask, const int32_t* status, const double* Y, void* vis);
int dmm_mfilter_solve(dmm_ctx* ctx, int nra, int nrow, int nmat, double* G, double* Y, int32_t* status);
int dmm_mfilter_eye(dmm_ctx* ctx, int nra, int nmat, int stage, const uint8_t* mask, double* Y, const int32_t* status);

/* DPSS gap inpainting (draco/util/dpss.py:121-443, draco/analysis/interpolate.py), csrc/dpss.hip.  A batch is nb <=
 * 65535 columns of n = 1 ... 4096 samples that share one real basis A [n][k] float64 row-major, k = 1 ... n (At [k][n]
 * is its transpose).  All arrays [dev] except `layout`; everything between pack and store is float64 in packed rows:
 * X [nb][2][n] (real row, imaginary row), Ni [nb][n], W [nb][n] bytes, xhat [nb][2], B [nb][2][k], C [nb][k][k] (only
 * the upper triangle is written and read), Z [nb][n][k], var / wout [nb][n], F [nb][2][n], status [nb] int32.
 *
 * layout [4] int64 (host) = (ninner, stride_outer, stride_inner, stride_samp), in elements of vis (complex64) and of
 * weight (float32) alike: column c starts at (c / ninner) stride_outer + (c % ninner) stride_inner and its samples are
 * stride_samp apart; cols [nb] int64 names the column of every slot.  With stride_samp = 1 the lanes of a wave run along
 * the samples, otherwise along adjacent slots (which should then be adjacent columns).
 *
 * dmm_dpss_pack: X, Ni = the column's values, W = wext (bytes in the weights' layout) or weight > 0 where wext is NULL,
 * xhat = sum(W x) / sum(W) (0 where no W), status = DMM_DPSS_SKIPPED where every weight is zero, else DMM_DPSS_OK.
 * dmm_dpss_gram: C = A^T diag(Ni) A + eps I (f64 MFMA).  dmm_dpss_project: B = A^T (Ni o (x - xhat)), the mean
 * removed on load.  dmm_dpss_solve: C = U^T U in place, then B <- C^-1 B; a pivot that is not positive sets status to
 * DMM_DPSS_NOT_POSDEF; slots whose status is set are left alone (B of a skipped slot is already zero).
 * dmm_dpss_variance (after solve): Z <- C^-1 a_i for the rows a_i of A, var_i = a_i . z_i - eps |z_i|^2, the diagonal
 * of F N F^H with F = A C^-1 A^T Ni (dpss.py:236-246).  dmm_dpss_synth: F = A B.
 * dmm_dpss_gapflag: keep [nb][n] bytes = flag_above_cutoff(valid, fc) of dpss.py:307-356 along n (nb unbounded).
 * dmm_dpss_pchip: wout = inz(var + max(p, 0)), p SciPy's PchipInterpolator of inz(Ni) through the samples where W is
 * set, evaluated (and extrapolated) at every sample index; no p with fewer than two such samples; var counts as zero
 * in a skipped slot; wout = 0 in a slot that is not positive definite (nb unbounded).
 * dmm_dpss_store: vis = F + xhat, weight = wout, rounded once to complex64 / float32; with inpaint != 0 the samples
 * where W is set get X and Ni back; weight = 0 where keep (may be NULL) is 0; a slot that is not positive definite
 * gets X back and weight 0.  vis / weight may be the arrays pack read or others of the same layout. */
enum { DMM_DPSS_OK = 0, DMM_DPSS_SKIPPED = 1, DMM_DPSS_NOT_POSDEF = 2 };
int dmm_dpss_pack(dmm_ctx* ctx, int n, int nb, const int64_t* layout, const int64_t* cols, const void* vis, const float* weight,
                  const uint8_t* wext, double* X, double* Ni, uint8_t* W, double* xhat, int32_t* status);
int dmm_dpss_gram(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* Ni, double eps, double* C, const int32_t* status);
int dmm_dpss_project(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* X, const double* Ni, const double* xhat, double* B);
int dmm_dpss_solve(dmm_ctx* ctx, int k, int nb, double* C, double* B, int32_t* status);
int dmm_dpss_variance(dmm_ctx* ctx, int n, int k, int nb, const double* A, const double* C, double eps, double* Z, double* var,
                      const int32_t* status);
int dmm_dpss_synth(dmm_ctx* ctx, int n, int k, int nb, const double* At, const double* B, double* F);
int dmm_dpss_gapflag(dmm_ctx* ctx, int n, int nb, const uint8_t* valid, double fc, uint8_t* keep);
int dmm_dpss_pchip(dmm_ctx* ctx, int n, int nb, const double* Ni, const uint8_t* W, const double* var, const int32_t* status, double* wout);
int dmm_dpss_store(dmm_ctx* ctx, int n, int nb, const int64_t* layout, const int64_t* cols, const double* F, const double* xhat,
                   const double* X, const double* Ni, const uint8_t* W, const double* wout, const uint8_t* keep, const int32_t* status,
                   int inpaint, void* vis, float* weight);

/* Source beamforming (draco/analysis/beamform.py:139-385, draco/util/_fast_tools.pyx:211-290), csrc/srcbeam.hip.  All
 * arrays [dev].  A dataset is vis [nfreq][nstack][nra] complex64 and weight of the same shape float32; one processed
 * polarisation is the nsel stacks sel [nsel] int32 of it.
 *
 * dmm_srcbeam_prepare: visT [nfreq][nra][nsel] complex64 = the polarisation's visibilities with the stacks contiguous,
 * ws (same shape, float32) = the weight of the sum: the visibility weight (DMM_SRCBEAM_INVERSE_VARIANCE),
 * (weight > 0) redundancy [nstack][nra] (DMM_SRCBEAM_NATURAL) or (weight > 0)(redundancy > 0) (DMM_SRCBEAM_UNIFORM);
 * SW [nfreq][nra] = sum_k ws, SW2 = sum_k ws^2 inz(weight), float64.  redundancy may be NULL for inverse variance;
 * sel, visT and ws may be NULL when nsel = 0 (a polarisation without stacks: SW = SW2 = 0).
 *
 * dmm_srcbeam_form: for a chunk of nsrc sources with windows of nha slots,
 *   F [nsrc][nfreq][nha] = sum_k ws[f][ra][k] Re(visT[f][ra][k] exp(2 pi i (u[f][k] ut[s][j] + v[f][k] vt[s][j])))
 * float64, u / v [nfreq][nsel] the baselines in wavelengths, ut = cos(dec) sin(ha), vt = -(cos(lat) sin(dec) -
 * sin(lat) cos(dec) cos(ha)) [nsrc][nha].  ws is float32 (DMM_SRCBEAM_W_F32) or float64 (DMM_SRCBEAM_W_F64).  Which
 * slots exist and which sample each reads is the inverted window list: pair_id [npair] int32 = s nha + j sorted by the
 * sample they read, pair_start [nra + 1] int32 the first pair of every sample.  fmask [nsrc][nfreq] bytes (may be NULL):
 * frequencies a source does not process stay zero, as do slots no pair names.  nha <= nra.
 *
 * dmm_srcbeam_collapse: F and pb [npol][nsrc][nfreq][nha] (pb NULL: ones), SW / SW2 [npol][nfreq][nra], ra_index
 * [nsrc][nha] int32 the sample of every slot (outside 0 ... nra - 1: no such slot), rows [nsrc] int64 the output row of
 * every source (< nobj).  With collapse_ha: beam [nobj][npo][nfreq] = sum_j F pb inz(sum_j SW pb^2), weight = 2 (sum_j SW
 * pb^2)^2 inz(sum_j SW2 pb^2), or 2 sum_j SW pb^2 with inverse_variance; without: beam [nobj][npo][nfreq][nha] = F inz(SW),
 * weight = 2 SW^2 inz(SW2) or 2 SW, zero where there is no slot.  Weight is zero where fmask is.  With stokes_i npo = 1
 * and beam = sum_p beam_p weight_p inz(sum_p weight_p), weight = sum_p weight_p; otherwise npo = npol. */
enum { DMM_SRCBEAM_INVERSE_VARIANCE = 0, DMM_SRCBEAM_NATURAL = 1, DMM_SRCBEAM_UNIFORM = 2 };
enum { DMM_SRCBEAM_W_F32 = 0, DMM_SRCBEAM_W_F64 = 1 };
int dmm_srcbeam_prepare(dmm_ctx* ctx, int nfreq, int nstack, int nra, int nsel, const int32_t* sel, int mode, const void* vis, const float* weight,
                        const float* redundancy, void* visT, float* ws, double* SW, double* SW2);
int dmm_srcbeam_form(dmm_ctx* ctx, int nfreq, int nra, int nsel, int wtype, const void* visT, const void* ws, const double* u, const double* v, int nsrc, int nha,
                     const double* ut, const double* vt, const uint8_t* fmask, int64_t npair, const int32_t* pair_start, const int32_t* pair_id, double* F);
int dmm_srcbeam_collapse(dmm_ctx* ctx, int nfreq, int nra, int npol, int nsrc, int nha, int collapse_ha, int inverse_variance, int stokes_i, const double* F,
                         const double* pb, const double* SW, const double* SW2, const int32_t* ra_index, const uint8_t* fmask, const int64_t* rows, int64_t nobj,
                         double* beam, double* weight);

/* Gaussian-process regridding (draco/util/gaussian_process.py:71-226, draco/analysis/sidereal.py:281-346), csrc/gp.hip.
 * A group is one distinct (input mask, kept output rows) pair; frequencies that share it share its projection.  Sizes
 * of group g: dims[g] = (n, M, nk, 0) int32 [host], n compressed input samples, M band rows (1 ... n, decided by the
 * caller), nk kept output rows; dims_dev [ngroup][4] int32 [dev] receives a copy.  ngroup <= 65535.  Arrays [dev]:
 *   pos [ngroup][nmax] f64 compressed sample positions, xout [ngroup][nkpad] f64 kept output positions,
 *   Kb [ngroup][nmax][Mmax] f64, Kb[i][d] = K[i][i - d] (the lower band; whatever lies beyond it is dropped),
 *   Y [ngroup][nmax][nkpad] f64, Y[j][b] = Kstar[b][j]; nkpad a multiple of 64,
 *   status [ngroup], start / end [ngroup][nkpad] int32, Ac [ngroup][width][nkpad] f64.
 * dmm_gp_masks: mask_pos / mask_nonzero [nfreq][nt] bytes = any over the stacks of weight > 0 / != 0; rowflag
 * [nfreq nstack] bytes = any over time of weight > 0.  weight [nfreq][nstack][nt].
 * dmm_gp_fill: Kb and Y from the positions: the product of nspec <= 4 kernels, types [nspec] and params [nspec][3] =
 * (width, alpha, a or 0) [host], of |xa / width - xb / width| with NumPy's expressions; epsilon is added to the diagonal.
 * dmm_gp_project: K = L L^T in place on the band, Y <- K^-1 Y (f64 MFMA), then start / end of every column b < nk of Y:
 * the first and one past the last j with |Y[j][b]| > tol, (0, 0) if none.  A pivot that is not positive sets status to
 * DMM_GP_NOT_POSDEF and nothing further is computed for that group (its start = end = 0).  Kb and Y may come from
 * dmm_gp_fill or from the caller.
 * dmm_gp_compact: Ac[w][b] = Y[start_b + w][b] for start_b + w < end_b, else 0; width >= every end - start.
 * dmm_gp_apply: per frequency f of group freq_group[f] (-1: left alone), stack s with rowflag set and kept row b whose
 * out_index[b] - pad lies in [0, samples): out_vis = sum_j A[b][j] x[j] over [start_b, end_b) in float64 (real and
 * imaginary part apart, rounded to complex64), out_weight = inz(float32(sum_j A[b][j]^2 float32(inz(w[j])))) in float32,
 * both zero where that is negative; x[j] = vis[f][s][sample_index[j]].  Mixing arrays as for dmm_regrid_band_wiener
 * (omega, feed_mask [nfreq nstack], dphi_in [nt], dphi_out [samples]).  Entries it does not write are left alone (the
 * caller zeroes the outputs).  vis, weight [nfreq][nstack][nt]; out_vis, out_weight [nfreq][nstack][samples]. */
enum { DMM_GP_GAUSSIAN = 0, DMM_GP_RATIONAL = 1, DMM_GP_MATERN15 = 2, DMM_GP_MATERN25 = 3 };
enum { DMM_GP_OK = 0, DMM_GP_NOT_POSDEF = 1 };
int dmm_gp_masks(dmm_ctx* ctx, const float* weight, int nfreq, int nstack, int nt, uint8_t* mask_pos, uint8_t* mask_nonzero, uint8_t* rowflag);
int dmm_gp_fill(dmm_ctx* ctx, int nspec, const int32_t* types, const double* params, double epsilon, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax,
                int Mmax, int nkpad, const double* pos, const double* xout, double* Kb, double* Y);
int dmm_gp_project(dmm_ctx* ctx, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int Mmax, int nkpad, double* Kb, double* Y, double tol, int32_t* status,
                   int32_t* start, int32_t* end);
int dmm_gp_compact(dmm_ctx* ctx, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int nkpad, int width, const double* Y, const int32_t* start,
                   const int32_t* end, double* Ac);
int dmm_gp_apply(dmm_ctx* ctx, int nfreq, int nstack, int nt, int samples, int pad, int ngroup, const int32_t* dims, int32_t* dims_dev, int nmax, int nkpad, int width,
                 const int32_t* freq_group, const int32_t* sample_index, const int32_t* out_index, const int32_t* start, const int32_t* end, const double* Ac,
                 const uint8_t* rowflag, const void* vis, const float* weight, const double* omega, const float* feed_mask, const double* dphi_in,
                 const double* dphi_out, void* out_vis, float* out_weight);

/* RFI flagging (draco/util/filters.py:99-130, draco/util/rfi.py:8-257, draco/analysis/flagging.py:1808-2377 and
 * :3231-3381), csrc/rfi.hip.  Planes are [nf][nt] row-major [dev]: float64 data, flags and masks one byte per sample
 * (non-zero = flagged).  Nothing here uses a floating-point atomic; every result is independent of the launch shape.
 * dmm_rfi_medfilt: masked moving median of nplane planes.  The window of (size_f, size_t) samples is centred on the
 * sample and clipped at the plane's edge; the result is 0.5 (v[(n-1)/2] + v[n/2]) of the n unflagged samples v of the
 * window in ascending order, NaN for n = 0.  Supported: both sizes odd, each <= DMM_RFI_MAX_WINDOW, their product <=
 * DMM_RFI_MAX_STRIP (one block's strip of sorted columns lives in LDS); anything else is DMM_E_ARG.  Signed zeros are
 * equal numbers: which of them comes out is not promised.  An unflagged NaN sorts above +inf.
 * dmm_rfi_quantile: per row of y [nrow][n] the "split" quantile of the n' unflagged samples: t = q n', 0.5 (v[lo] +
 * v[hi]) with lo = ceil(t) - 1, hi = floor(t) clamped to 0 ... n' - 1, NaN for n' = 0; count [nrow] int32 (may be NULL)
 * receives n'.  n <= DMM_RFI_MAX_ROW.
 * dmm_rfi_sumthreshold: flag <- flag | !finite(data), then nstep steps, step s with window[s] samples along axis[s]
 * (0: frequency, 1: time) against threshold[s] [all three host arrays]: sums of data (0 where flagged) and of the
 * count (!flag, times variance if given) over samples j - m + 1 ... j (below 0: sample 0), the count sum square-rooted
 * with correct_for_missing; |sum| (sum with only_positive) > count threshold flags j - m + 1 ... j.  A step completes
 * before the next reads the flags.  hit [nf][nt] bytes is scratch.  window[s] <= DMM_RFI_MAX_ST_WINDOW.
 * dmm_rfi_sir: out = flag | SIR(flag) along the axis (accumulate: out |= that): per line the strictly sequential
 * float64 running sum S of flag + (eta - 1), flagged where max(S after the sample) >= min(S before it) with the
 * reference's ranges.  work: 2 nf nt float64.  out may not be flag.
 * dmm_rfi_absdev: dy = y - med (dy may be NULL), ady = |dy|, or the modulus when the imaginary parts are given.
 * dmm_rfi_nsigma: s = scale mad, ratio = ady (1 / s) with 1 / 0 = 0 (divide: ratio = ady / s), a NaN ratio replaced by
 * nan_fill unless that is NaN itself, variance = s s and mask = ratio > nsigma (either may be NULL).
 * dmm_rfi_tv_flag: frac = float32(count / N) of x > chan_thr[c] over the N rows chan_rows[chan_ptr[c] ... chan_ptr[c+1])
 * of the channel c = row_chan[row] the row keeps (1 where row_chan < 0), mask = frac > float32(f).  frac may be NULL.
 * dmm_rfi_mask_op: out = a | b (DMM_RFI_OR), c ? a : b (DMM_RFI_SELECT); out may be an input.
 * dmm_rfi_rows: y[f][t] -= row_sub[f], flag[f][t] |= row_flag[f] (either pair may be NULL).
 * dmm_rfi_radiometer: measured, radiometer, weight [nf][npol][nt] float32 -> y [npol][nf][nt] = float64(measured
 * float32(1 / radiometer)) with 1 / 0 = 0, flag = weight == 0.
 * dmm_rfi_apply_mask: weight [dims...][nt] float32 *= !mask for the nsel samples data_index [dev] of the last axis,
 * each reading sample mask_index [dev] of the mask's nmask; the mask element of leading coordinates (i0, ...) lies at
 * sum_d i_d mask_stride[d] + sample mask_stride_t (a stride of 0 broadcasts).  dims, mask_stride [ndim <= 4, host]. */
#define DMM_RFI_MAX_WINDOW 255
#define DMM_RFI_MAX_STRIP 8192
#define DMM_RFI_MAX_ROW 16384
#define DMM_RFI_MAX_ST_WINDOW 4096
enum { DMM_RFI_OR = 0, DMM_RFI_SELECT = 1 };
int dmm_rfi_medfilt(dmm_ctx* ctx, const double* x, const uint8_t* flag, int nplane, int nf, int nt, int size_f, int size_t_, double* out);
int dmm_rfi_quantile(dmm_ctx* ctx, const double* y, const uint8_t* flag, int64_t nrow, int n, double q, double* out, int32_t* count);
int dmm_rfi_sumthreshold(dmm_ctx* ctx, const double* data, const double* variance, uint8_t* flag, uint8_t* hit, int nf, int nt, int nstep, const int32_t* window,
                         const int32_t* axis, const double* threshold, int correct_for_missing, int only_positive);
int dmm_rfi_sir(dmm_ctx* ctx, const uint8_t* flag, int nf, int nt, int axis, double eta, int accumulate, double* work, uint8_t* out);
int dmm_rfi_absdev(dmm_ctx* ctx, const double* y, const double* med, const double* y_imag, const double* med_imag, int64_t n, double* dy, double* ady);
int dmm_rfi_nsigma(dmm_ctx* ctx, const double* ady, const double* mad, double scale, double nsigma, double nan_fill, int divide, int64_t n, double* ratio,
                   double* variance, uint8_t* mask);
int dmm_rfi_tv_flag(dmm_ctx* ctx, const double* x, int nf, int nt, const int32_t* row_chan, int nchan, const int32_t* chan_ptr, const int32_t* chan_rows, int nrows,
                    const double* chan_thr, double f, float* frac, uint8_t* mask);
int dmm_rfi_mask_op(dmm_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, const uint8_t* c, int64_t n, uint8_t* out);
int dmm_rfi_rows(dmm_ctx* ctx, double* y, uint8_t* flag, const double* row_sub, const uint8_t* row_flag, int nf, int nt);
int dmm_rfi_radiometer(dmm_ctx* ctx, const float* measured, const float* radiometer, const float* weight, int nf, int npol, int nt, double* y, uint8_t* flag);
int dmm_rfi_apply_mask(dmm_ctx* ctx, float* weight, int ndim, const int64_t* dims, int nt, const uint8_t* mask, const int64_t* mask_stride, int64_t mask_stride_t,
                       int nmask, int nsel, const int32_t* data_index, const int32_t* mask_index);

/* Weighted moving median (caput's moving_weighted_median as draco/analysis/flagging.py:1670-1773 uses it; the
 * convention is pinned in DESIGN.md section 7s), csrc/rfi.hip.  x, w, out float64 [nplane][nf][nt] [dev].
 * dmm_rfi_wmedfilt: the window of (size_f, size_t) samples is centred on the sample and clipped at the plane's edge;
 * the samples with w > 0 take part.  In ascending order, W their total weight and c(v) the weight of the samples <= v:
 * lo the smallest sample with c(lo) >= W / 2, hi the smallest with c(hi) > W / 2, the result 0.5 (lo + hi); NaN for a
 * window without a sample.  With 0/1 weights that is dmm_rfi_medfilt's result.  Weight sums are float64, per column of
 * the window in sorted order and then over the columns in a fixed order that depends on the window alone: where every
 * partial sum is exact the result is exact for any launch shape, elsewhere it is the stated one wherever c(v) misses
 * W / 2 by more than the rounding of those sums.  A negative or NaN weight drops the sample (callers reject them).
 * Signed zeros and NaN samples as for dmm_rfi_medfilt.
 * Supported: both sizes odd, each <= DMM_RFI_WMED_MAX_WINDOW, their product <= DMM_RFI_WMED_MAX_STRIP; anything else is
 * DMM_E_ARG.  A block keeps min(size_f, nf) x (T + size_t - 1) <= DMM_RFI_WMED_MAX_STRIP samples of 16 bytes (key and
 * prefix weight) and 4 bytes per column in LDS, T <= DMM_RFI_WMED_TILE output times: at most 128 KiB + 4.3 KiB of the
 * 160 KiB of a CU, one block per CU at the bound.
 * dmm_rfi_wdev: dy = (y - med) sqrt(w), ady = |dy| (may be NULL), n samples: the deviation from the median in expected
 * standard deviations, w the inverse variance. */
#define DMM_RFI_WMED_MAX_WINDOW 1023
#define DMM_RFI_WMED_MAX_STRIP 8192
#define DMM_RFI_WMED_TILE 64
int dmm_rfi_wmedfilt(dmm_ctx* ctx, const double* x, const double* w, int nplane, int nf, int nt, int size_f, int size_t_, double* out);
int dmm_rfi_wdev(dmm_ctx* ctx, const double* y, const double* med, const double* w, int64_t n, double* dy, double* ady);

/* Weighted reductions over adjacent axes (draco/analysis/transform.py:1904-2117 and the collapse of
 * draco/analysis/flagging.py:1548-1579), csrc/reduce.hip.  x [nouter][nred][ninner] [dev] of type dtype; the weight w
 * [dev] (float32 or float64 by wdtype; NULL: all ones) of sample (o, r, i) lies at o ws_outer + (r / nred2) ws_red1 +
 * (r % nred2) ws_red2 + i ws_inner elements, a stride of 0 for an axis the weight lacks; nred2 divides nred.  Sums are
 * float64 in ascending r, one rounding at the store; inz(v) = 1 / v, 0 for v = 0.  out, out_w [nouter][ninner] [dev].
 * DMM_REDUCE_CHISQ: num = max(#(w > 0) - 1, 0), mu = sum(w x) inz(sum w), out = sum(w |x - mu|^2) inz(num) in x's
 * type, out_w = num in the weight's type.
 * DMM_REDUCE_VAR_NONE: out = mean |x - mean x|^2, out_w = 1.  _MASKED (w <- w > 0) and _WEIGHTED: ws = sum w, mu =
 * sum(w x) inz(ws), out = sum(w (x - mu)^2) inz(ws) (the square of a complex number, as the reference has it), out_w =
 * ws.  Both need w.
 * DMM_REDUCE_WMEAN: s = factor sum w, out = sum(w Re x) inz(s), out_w = s, both float64. */
enum { DMM_REDUCE_CHISQ = 0, DMM_REDUCE_VAR_NONE = 1, DMM_REDUCE_VAR_MASKED = 2, DMM_REDUCE_VAR_WEIGHTED = 3, DMM_REDUCE_WMEAN = 4 };
enum { DMM_REDUCE_F32 = 0, DMM_REDUCE_F64 = 1, DMM_REDUCE_C64 = 2, DMM_REDUCE_C128 = 3 };
int dmm_axis_reduce(dmm_ctx* ctx, int op, int dtype, const void* x, int64_t nouter, int64_t nred, int64_t ninner, const void* w, int wdtype, int64_t ws_outer,
                    int64_t nred2, int64_t ws_red1, int64_t ws_red2, int64_t ws_inner, double factor, void* out, void* out_w);

/* System sensitivity of a time stream (draco/analysis/sensitivity.py:11-261) and the mask of negative autocorrelations
 * (draco/analysis/flagging.py:666-699), csrc/sensitivity.hip.  vis complex64 and weight float32 are [nf][nstack][nt]
 * [dev] and are read once; sums run in float64 in a fixed order (no atomics: two runs give the same bits) and are
 * rounded to float32 at the store.  inv0(x) = 1 / x, 0 for x = 0.
 * Index tables are [host] pointers, checked before anything is launched (a row index outside the stack axis, a column
 * index outside cnt, a *_ptr table that does not start at 0 or decreases: DMM_E_ARG); the library copies them to
 * `tables` [dev], int32 scratch of the caller's with room for every table of the call, in the order of the argument
 * list.  Everything else is [dev].
 * cnt [nstack][ncol] float32: the redundancy of every stack entry under every distinct column of input flags; col
 * [niff][nt] [host]: the column of the sample (f % niff, t), niff = 1 or nf.
 * dmm_sens_measured: the rows of polarisation p are rows[pol_ptr[p] ... pol_ptr[p+1]) [host], each a pair (stack entry
 * s, factor k = 1 for an autocorrelation, else 2).  With c = cnt[s][col], w = weight[f][s][t]: V = sum c c k [w > 0] / w,
 * C = sum c k [w > 0]; measured [nf][npol][nt] = sqrt(2 V inv0(C C)), out_weight = C.  tables: niff nt + npol + 1 +
 * 2 pol_ptr[npol] words.  A polarisation without rows gives zeros.
 * dmm_sens_radiometer: the autocorrelation rows of group g (one polarisation of the inputs at one east-west position)
 * are auto_rows[grp_ptr[g] ... grp_ptr[g+1]) [host], ngroup <= DMM_SENS_MAX_GROUP; the ordered group pairs (g, h) of
 * polarisation p are pairs[pair_ptr[p] ... pair_ptr[p+1]) [host].  With n = c [w > 0], a = Re vis: S_g = sum n a, N_g =
 * sum n, R = sum S_g S_h, K = sum N_g N_h, nint = dnu_tint (1 - frac_lost[f][t]) (frac_lost [nf][nt] float32 or NULL
 * for 0): radiometer [nf][npol][nt] = sqrt(2 R inv0(nint K K)), NaN for R < 0 or a NaN dnu_tint; frac_out [nf][nt] receives frac_lost.
 * tables: niff nt + ngroup + 1 + grp_ptr[ngroup] + npol + 1 + 2 pair_ptr[npol] words.
 * dmm_sens_negative_autos: mask [nf][nt] bytes = 1 where Re vis[f][s][t] < 0 for any s of auto_rows [nauto] [host];
 * tables: nauto words. */
#define DMM_SENS_MAX_GROUP 64
int dmm_sens_measured(dmm_ctx* ctx, const float* weight, int nf, int nstack, int nt, const float* cnt, int ncol, int niff, const int32_t* col, int npol,
                      const int32_t* pol_ptr, const int32_t* rows, int32_t* tables, float* measured, float* out_weight);
int dmm_sens_radiometer(dmm_ctx* ctx, const void* vis, const float* weight, int nf, int nstack, int nt, const float* cnt, int ncol, int niff, const int32_t* col,
                        int ngroup, const int32_t* grp_ptr, const int32_t* auto_rows, int npol, const int32_t* pair_ptr, const int32_t* pairs, const float* frac_lost,
                        double dnu_tint, int32_t* tables, float* radiometer, float* frac_out);
int dmm_sens_negative_autos(dmm_ctx* ctx, const void* vis, int nf, int nstack, int nt, int nauto, const int32_t* auto_rows, int32_t* tables, uint8_t* mask);

/* 3-D power spectrum of a ring-map delay cube (draco/analysis/powerspec.py:539-1017), csrc/powerspec.hip.  float64
 * throughout, no floating-point atomics: two runs give the same bits.  Everything is [dev] unless marked [host].
 * dmm_uv_fft2: spectrum [npol][nel][nra][ndelay] complex128 (the delay transform of a ring map, baseline = pol x el) ->
 * vis [npol][ndelay][nra][nel] complex128 = fftshift(fft2(x * (w_ra (x) w_el))) / (nra nel) per (pol, delay) plane; w_ra
 * [nra] and w_el [nel] float64, both NULL for no taper.  Two in-LDS row transforms (along el, then along ra in place in
 * vis), run slab by slab of about slab_mib MiB of vis (0: 128); spectrum is not modified.  dmm_uv_fft2_supported(n):
 * 1 if an axis of length n can be transformed (powers of two to 8192, other lengths to 4096); a longer axis is
 * DMM_E_UNSUPPORTED, before anything is launched.
 * dmm_ps3d_cross: out [npol1 npol2][ncell] = ps_norm vis1[p1] conj(vis2[p2]), p = p1 npol2 + p2, vis1 [npol1][ncell],
 * vis2 [npol2][ncell] complex128 (they may be the same array: the imaginary part of an auto spectrum is exactly 0).
 * dmm_ps_cyl_bin: per plane (pol, delay) of spec [nplane][nu nv] complex128 and per bin b of binmap [nu nv] int16
 * [host] (-1: the cell belongs to no bin; a value >= nbins is DMM_E_ARG), with w = 1 (sigma NULL) or 1 / |sigma|^2, 0
 * where sigma [nplane][nu nv] complex128 is 0:  out_spec [nplane][nbins] = sum w p / sum w, out_weight = sum w, out_neff
 * = (sum w)^2 / sum w^2, summed in a fixed order; an empty bin gives NaN, 0, NaN.  Synchronises the context's stream. */
#define DMM_PS_MAX_BINS 4096
int dmm_uv_fft2_supported(int n);
int dmm_uv_fft2(dmm_ctx* ctx, const void* spectrum, int npol, int nel, int nra, int ndelay, const double* w_ra, const double* w_el, void* vis, int64_t slab_mib);
int dmm_ps3d_cross(dmm_ctx* ctx, const void* vis1, const void* vis2, int npol1, int npol2, int64_t ncell, double ps_norm, void* out);
int dmm_ps_cyl_bin(dmm_ctx* ctx, const void* spec, const void* sigma, const int16_t* binmap, int nplane, int nu, int nv, int nbins, void* out_spec, double* out_weight,
                   double* out_neff);

/* Source stacking (draco/analysis/sourcestack.py:17-211, draco/analysis/beamform.py:915-1302), csrc/sourcestack.hip.
 * float64 throughout, no floating-point atomics: sums run over chunks of DMM_STACK_SRC_CHUNK sources in catalogue
 * order and the chunks' partial sums are added one after the other, so two runs give the same bits whatever
 * partial_chunks is.  Everything is [dev].  Nothing here synchronises.
 *
 * dmm_ringmap_extract: beam [nsrc][npol][nfreq] = map [npol][nfreq][nra][nel] at (ra_ind[s], el_ind[s]); weight
 * likewise from wsrc [npol][nfreq][nra][nel] (rms = 0) or inz(wsrc [npol][nfreq][nra])^2 (rms = 1).  order [nsrc]
 * (may be NULL) is the order in which sources are visited (a permutation, sorted by pixel); a source whose indices are
 * outside the map gets zeros.  nsrc = 0 launches nothing.
 *
 * dmm_source_stack: beam / weight [nsrc][npol][nfreq], freq [nfreq] strictly monotonic (freq_descending says which
 * way), sfreq [nsrc] the sources' line frequencies, smask [nsrc] bytes (NULL: every source), bins [nstack + 1] the
 * strictly monotonic bin edges (bins_ascending).  Channel f of source s is in bin np.digitize(freq[f] - sfreq[s], bins)
 * - 1; with w_eff = weight, or (weight > 0) when uniform, stack [npol][nstack] = S inz(W), out_weight = W, S = sum w_eff
 * beam, W = sum w_eff over sources and the channels of a bin.  partial holds partial_chunks x 2 npol nstack doubles,
 * running 2 npol nstack.
 *
 * dmm_ringmap_stack3d: around the pixel (ra_ind[s], el_ind[s]) of each source the patch of (2 num_ra + 1) x (2 num_dec
 * + 1) pixels, clipped at both ends of el, and in ra wrapped (ra_wraps) or clipped; channel f of source s is in bin
 * np.digitize(freq[f] - sfreq[s], edges) - 1 of edges [nbins + 1] ascending, the two overflow bins dropped.  The weight w
 * of a pixel is the map's (mode DMM_STACK3D_INPUT; wsrc and rms as above, the rms spread over el), (w != 0) wdec [npol]
 * [nfreq][nel] (DMM_STACK3D_DEC) or (w != 0) inz(population variance of the clipped patch) (DMM_STACK3D_PATCH).  stack
 * [npol][2 num_ra + 1][2 num_dec + 1][nbins] = sum(map w) inz(sum w), out_weight = sum w.  partial holds partial_chunks x
 * 2 n doubles and running 2 n, n = npol nbins (2 num_ra + 1)(2 num_dec + 1). */
#define DMM_STACK_SRC_CHUNK 256
#define DMM_STACK_MAX_FREQ 2048
enum { DMM_STACK3D_INPUT = 0, DMM_STACK3D_DEC = 1, DMM_STACK3D_PATCH = 2 };
int dmm_ringmap_extract(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, const double* map, const double* wsrc, int rms, int64_t nsrc, const int32_t* ra_ind,
                        const int32_t* el_ind, const int32_t* order, double* beam, double* weight);
int dmm_source_stack(dmm_ctx* ctx, int64_t nsrc, int npol, int nfreq, int nstack, const double* beam, const double* weight, const double* freq, int freq_descending,
                     const double* sfreq, const uint8_t* smask, const double* bins, int bins_ascending, int uniform, double* partial, int64_t partial_chunks,
                     double* running, double* stack, double* out_weight);
int dmm_ringmap_stack3d(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, const double* map, const double* wsrc, int rms, int mode, const double* wdec, int64_t nsrc,
                        const int32_t* ra_ind, const int32_t* el_ind, const double* sfreq, const double* freq, int freq_descending, int nbins, const double* edges,
                        int num_ra, int num_dec, int ra_wraps, double* partial, int64_t partial_chunks, double* running, double* stack, double* out_weight);

/* Wiener delay transform of a filtered ring map (draco/analysis/powerspec.py:118-458), csrc/wienerdelay.hip.  float64
 * arithmetic in a fixed order, no floating-point atomics: the results are the same bits whatever workspace_mib is.
 * Everything is [dev] unless marked [host].  1 <= nfreq <= DMM_WD_MAX_FREQ, 1 <= ndelay <= nfreq; a count of zero pixels
 * launches nothing.
 *
 * dmm_wienerdelay_build: filter, freq_cov [npol][nfreq][nfreq][nra], weight [npol][nfreq][nra][nel], beam_power [npol]
 * [nfreq][nel] (beam 0 of dirty_beam_power), prior [nfreq][2 nfreq] = [Re | Im] of F S F^H, fourier [2][nfreq][ndelay]
 * = Re, Im of F, sdiag [ndelay] = S, window [nfreq].  Per pixel, with K, C the [freq, freq] slices at this RA, w the
 * weights, b = sqrt(beam_power), win_mask = window > 0:  M = win_mask and (w > 0), H = diag(M) K, r = sqrt(inv0(w diag C))
 * win_mask, A = H (F S F^H o b b^T) H^T + C o r r^T, out [npol][nra][nel][ndelay][nfreq] = diag(S) F^H H^T A^-1 window, the
 * inverse taken on the channels of M and zero elsewhere (only the upper triangle of A is used).  out_dtype DMM_C64 or
 * DMM_C128: one computation, cast at the store.  A pixel without a valid channel gives zeros.  The pixels are worked on
 * in slabs of about workspace_mib MiB (0: 1024) of library scratch; after every slab the stream is synchronised and the
 * call ends at the first slab with a pixel whose A is not positive definite: *first_bad [host] = (pol nra + ra) nel + el
 * of the lowest such pixel of that slab (-1: none), whose part of out, and every later slab's, is not meaningful.
 *
 * dmm_wienerdelay_apply: op [npol][nra][nel][ndelay][nfreq] (op_dtype DMM_C64, widened on load, or DMM_C128), map and
 * weight [npol][nfreq][nra][nel] float64: spectrum [npol nel][nra][ndelay] complex128 = sum_f op[d][f] map[f], sweight
 * (float32, same shape) = inv0(sum_f |op[d][f]|^2 inv0(weight[f])), in a fixed order.  Does not synchronise. */
#define DMM_WD_MAX_FREQ 1024
int dmm_wienerdelay_build(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, int ndelay, const double* filter, const double* freq_cov, const double* weight, const double* beam_power,
                          const double* prior, const double* fourier, const double* sdiag, const double* window, void* out, int out_dtype, int64_t workspace_mib, int64_t* first_bad);
int dmm_wienerdelay_apply(dmm_ctx* ctx, int npol, int nfreq, int nra, int nel, int ndelay, const void* op, int op_dtype, const double* map, const double* weight, void* spectrum,
                          float* sweight);

/* Transient RFI mask from visibilities (draco/analysis/flagging.py:1042-1277, draco/analysis/transform.py:1382-1448,
 * draco/util/filters.py:22-96), csrc/vismask.hip.  No floating-point atomics: two runs give the same bits.  Everything
 * is [dev] unless marked [host]; every argument is checked before anything is launched.
 * dmm_stokes_i_sum: vis [nf][nprod][nt] complex64 and weight float32 -> vis_i [nf][nbase][nt] = the sum over the rows
 * rows[ptr[b] ... ptr[b+1]) of baseline b, in ascending order of the table, in complex64 / float32 from a zero (the
 * reference's `+=`, bit for bit); weight_i likewise.  A baseline without rows is a zero row.  ptr [nbase + 1], rows
 * [nrows] int32; an index outside its axis is clamped.
 * dmm_wconv_filter: per row of data [nrow][n] (dtype DMM_REDUCE_C64 with float32 weight, DMM_REDUCE_C128 or
 * DMM_REDUCE_F64 with float64 weight) and taps [ntap] float64, ntap odd, c = (ntap - 1) / 2, samples outside the row
 * zero: vw[t] = sum_j taps[j] (d w)[t + c - j], ww[t] = sum_j taps[j] w[t + c - j], lp = vw inz(ww), inz(v) = 1 / v and
 * 0 for v = 0 -- the centred slice of the full convolution, also for ntap > n.  Sums are float64 in ascending j, one
 * rounding at the store.  out [nrow][n] complex128 / float64 = lp, or d - lp with highpass.  ntap <= DMM_WCONV_MAX_TAPS.
 * dmm_beam_abs_fft: x [nplane][nstack][nt] complex128 -> out (float64, same shape) [p][k][t] = |sum_s x[p][s][t]
 * exp(-2 pi i k s / nstack)|, one in-LDS transform per column.  dmm_beam_abs_fft_supported(n): as dmm_uv_fft2_supported
 * (powers of two to 8192, other lengths to 4096); a longer axis is DMM_E_UNSUPPORTED, before anything is launched.
 * dmm_rfi_hysteresis: x [nplane][nf][nt] float64, low <- min(low, high): out (bytes) = 1 at every sample with x > low
 * whose 4-connected component of {x > low} within its plane holds a sample with x > high; comparisons are strict, a NaN
 * is in neither set.  accumulate: out |= that.  state [nplane nf nt] bytes and changed [1] int32 are scratch.  *sweeps
 * [host] (may be NULL) receives the number of sweeps (rows both ways, then columns both ways), the last of which
 * changed nothing; DMM_E_STATE, and an unfinished out left unwritten, if DMM_RFI_HYST_MAX_SWEEPS did not reach the fixed
 * point.  Synchronises the context's stream once per sweep.
 * dmm_rfi_beam_count: count [nf][nt] int32 += #{b : flag[f][b][t] != 0}, flag [nf][nb][nt] bytes. */
#define DMM_WCONV_MAX_TAPS 1023
#define DMM_RFI_HYST_MAX_SWEEPS 4096
int dmm_stokes_i_sum(dmm_ctx* ctx, const void* vis, const float* weight, int nf, int nprod, int nt, const int32_t* ptr, const int32_t* rows, int nbase, int nrows,
                     void* vis_i, float* weight_i);
int dmm_wconv_filter(dmm_ctx* ctx, int dtype, const void* data, const void* weight, int64_t nrow, int n, const double* taps, int ntap, int highpass, void* out);
int dmm_beam_abs_fft_supported(int n);
int dmm_beam_abs_fft(dmm_ctx* ctx, const void* x, int nplane, int nstack, int nt, double* out);
int dmm_rfi_hysteresis(dmm_ctx* ctx, const double* x, int nplane, int nf, int nt, double low, double high, int accumulate, uint8_t* state, int32_t* changed, uint8_t* out,
                       int32_t* sweeps);
int dmm_rfi_beam_count(dmm_ctx* ctx, const uint8_t* flag, int nf, int nb, int nt, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* DRACO_AMD_H */
