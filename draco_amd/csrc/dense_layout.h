// Workspace layout of the dense solvers (solve_dense.hip): sizes, batch capacity and the carving of the caller's
// workspace, for the Wiener and the maximum-likelihood maker alike.  Plain integer arithmetic, no HIP: the header
// compiles on the host alone (tools/probe/dense_layout_sweep.cpp sweeps it against the arithmetic it replaced).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dense_layout {

constexpr int kTB = 64, kKC = 16;            // tile edge and staged chunk of dense_kernels.h (solve_dense.hip asserts them equal)
constexpr size_t kC128 = 16, kTileRec = 16;  // sizeof(double2), sizeof(dmm_tile)

struct Layout {
  int N, Np, T;
  size_t per_mat;        // bytes per matrix (A + Linv/V + wbuf)
  size_t per_mat_extra;  // pair rotations W^H / inverted diagonal blocks, flags, scale (kept behind the wbuf region)
  size_t header;         // Sl table, then the table expanded per packed column (Wiener Gram)
  size_t sl_bytes;       // offset of the expanded table inside the header
  int sk_pitch;
};

// aux_slots: matrix-sized regions behind A: 1 = Wiener (X / Cholesky copy), 2 = ML (also the rotation log of the
// tridiagonal eigen path, herm_tridiag.h)
inline Layout layout_of(int npairs, int npol, int lmax, int aux_slots) {
  Layout L;
  L.N = 2 * npairs;
  L.Np = (L.N + kTB - 1) / kTB * kTB;
  L.T = L.Np / kTB;
  const size_t a = (size_t)L.Np * L.Np * kC128;
  L.per_mat = a + (size_t)aux_slots * a + (size_t)L.N * kC128;
  L.per_mat_extra = (size_t)(L.Np / 64) * kTB * kTB * kC128 + (size_t)(L.Np / 64) * sizeof(int) + 32 + 64;  // + theta, tile, work, fail, msel
  L.sl_bytes = ((size_t)(lmax + 1) * sizeof(double) + 255) / 256 * 256;
  L.sk_pitch = (npol * (lmax + 1) + kKC - 1) / kKC * kKC;
  L.header = L.sl_bytes + ((size_t)(lmax + 1) * L.sk_pitch * sizeof(double) + 255) / 256 * 256;
  return L;
}

// matrices in flight per sub-batch: ~6 GiB for the Wiener solve; the ML eigen path has a per-batch latency floor (the
// serial QL chases, ~0.1 s at order 768 whatever the batch size), so its batches are made larger
constexpr size_t kTargetWs = (size_t)6 << 30, kTargetWsMl = (size_t)20 << 30;

// the caller may offer more (or less): opt_mib = "ml_workspace_mib" / "wiener_workspace_mib" (dmm_ctx_set_option, 0: the
// targets above).  The eigen pass pays a fixed cost per Householder column and launch -- the more matrices share it, the better
inline int batch_cap(const Layout& L, int aux_slots, int64_t ntile, int64_t opt_mib) {
  size_t target = aux_slots >= 2 ? kTargetWsMl : kTargetWs;
  if (opt_mib > 0) target = (size_t)opt_mib << 20;
  size_t nmat = target / (L.per_mat + L.per_mat_extra);
  if (nmat < 1) nmat = 1;
  if (nmat > (size_t)ntile) nmat = ntile > 0 ? ntile : 1;
  return (int)nmat;
}
inline int64_t workspace_bytes(const Layout& L, int cap) { return (int64_t)(L.header + (size_t)cap * (L.per_mat + L.per_mat_extra) + 1024); }

// Byte offsets of the regions of a workspace for `cap` matrices (the workspace itself is 256-byte aligned).  The three
// per-matrix regions come first; the small per-batch arrays live behind them (sized in layout_of).
struct Carve {
  size_t A, aux, wbuf;        // [cap] matrices; [cap] x aux_slots matrices (Wiener: X; ML: X, Cholesky copies, eigenvectors, logs); [cap][N]
  size_t blocks;              // [cap][Np / 64] blocks of 64 x 64: inverted diagonal blocks (Cholesky) / pair rotations (Jacobi)
  size_t flag, scale, theta;  // ML: [cap][Np / 64] ints, [cap] doubles, [cap] doubles
  size_t tiles, work;         // [cap] tiles of the batch; column-block prefix sums of the back-projections (work_first)
  size_t slots;               // Wiener: [cap] slots of the resident products
  size_t fail, msel, any_rot; // ML: [cap], [cap], one int
  size_t end;                 // first byte behind the last region (<= workspace_bytes)
};
inline Carve carve(const Layout& L, int cap, int aux_slots) {
  const size_t n = (size_t)cap, a = (size_t)L.Np * L.Np * kC128;
  Carve c = {};
  c.A = L.header;
  c.aux = c.A + n * a;
  c.wbuf = c.aux + n * (L.per_mat - a - (size_t)L.N * kC128);
  c.blocks = (c.wbuf + n * L.N * kC128 + 255) & ~(size_t)255;
  size_t q = c.blocks + n * (L.Np / 64) * kTB * kTB * kC128;
  const bool ml = aux_slots >= 2;
  if (ml) {
    c.flag = q;
    c.scale = c.flag + ((n * (L.Np / 64) + 1) & ~(size_t)1) * sizeof(int);
    c.theta = c.scale + n * sizeof(double);
    q = c.theta + n * sizeof(double);
  }
  c.tiles = q;
  c.work = c.tiles + n * kTileRec;
  q = c.work + ((n + (ml ? 4 : 8)) & ~(size_t)1) * sizeof(int32_t);  // ML: cap + 3 entries at least (work_first)
  if (ml) {
    c.fail = q;
    c.msel = c.fail + ((n + 1) & ~(size_t)1) * sizeof(int);
    c.any_rot = c.msel + ((n + 1) & ~(size_t)1) * sizeof(int);
    c.end = c.any_rot + sizeof(int);
  } else {
    c.slots = q;  // (the per-matrix extras leave room: layout_of)
    c.end = c.slots + n * sizeof(int);
  }
  return c;
}

// Column-block prefix sums of the back-projections (the `work` array): nmat + 1 entries per user, and users that can be
// in flight together get disjoint ranges.  A batch in the matrix slots from `off` on (either maker; Wiener's second half
// and the ML batches) uses [first, first + nmat] with first = off, one entry later when off > 0; the pipelined chunk in
// chunk slot h (ML) one entry later again per slot.  With the two halves (off = 0 and capE) that is [1, capE + 1] and
// [capE + 2, 2 capE + 2]; with the early-reject layout (direct batches in [0, cap_direct), two chunk slots of E behind) a
// FULL direct batch ends at work[cap_direct] and chunk slot 0 starts one entry later: cap + 3 entries in all.
enum WorkUser { kBatch, kChunk0, kChunk1 };
inline size_t work_first(size_t off, WorkUser u) { return u == kBatch ? off + (off ? 1 : 0) : off + 1 + (u == kChunk1 ? 1 : 0); }

}  // namespace dense_layout
