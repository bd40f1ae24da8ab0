// Host-only sweep of draco_amd/csrc/dense_layout.h against the carving arithmetic that solve_dense.hip carried before
// the layout moved there (kept below as it was written, on a fictitious 256-byte aligned base address).  Every offset
// and size must agree, the last region must end inside the workspace, and the work ranges of users that can be in flight
// together must not overlap.  Build and run (no GPU, no HIP):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I draco_amd/csrc tools/probe/dense_layout_sweep.cpp -o dense_layout_sweep && ./dense_layout_sweep
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "dense_layout.h"

namespace old_form {
constexpr int TB = 64, KC = 16;
struct double2 { double x, y; };
struct dmm_tile { int64_t b_off; int32_t m, f; };
struct Layout {
  int N, Np, T;
  size_t per_mat, per_mat_extra, header, sl_bytes;
  int sk_pitch;
};
Layout layout_of(int npairs, int npol, int lmax, int aux_slots) {
  const bool ml = aux_slots > 0;
  Layout L;
  L.N = 2 * npairs;
  L.Np = (L.N + TB - 1) / TB * TB;
  L.T = L.Np / TB;
  const size_t a = (size_t)L.Np * L.Np * sizeof(double2);
  const size_t aux = ml ? (size_t)aux_slots * a : (size_t)L.T * TB * TB * sizeof(double2);
  L.per_mat = a + aux + (size_t)L.N * sizeof(double2);
  L.per_mat_extra = ml ? (size_t)(L.Np / 64) * TB * TB * sizeof(double2) + (size_t)(L.Np / 64) * sizeof(int) + 32 + 64 : 0;
  L.sl_bytes = ((size_t)(lmax + 1) * sizeof(double) + 255) / 256 * 256;
  L.sk_pitch = (npol * (lmax + 1) + KC - 1) / KC * KC;
  L.header = L.sl_bytes + ((size_t)(lmax + 1) * L.sk_pitch * sizeof(double) + 255) / 256 * 256;
  return L;
}
constexpr size_t kTargetWs = (size_t)6 << 30, kTargetWsMl = (size_t)20 << 30;
int64_t workspace_bytes(const Layout& L, int aux_slots, int64_t ntile, int64_t opt) {
  size_t target = aux_slots >= 2 ? kTargetWsMl : kTargetWs;
  if (opt > 0) target = (size_t)opt << 20;
  size_t nmat = target / (L.per_mat + L.per_mat_extra);
  if (nmat < 1) nmat = 1;
  if (nmat > (size_t)ntile) nmat = ntile > 0 ? ntile : 1;
  return (int64_t)(L.header + nmat * (L.per_mat + L.per_mat_extra) + 1024);
}
struct Ptrs {
  uintptr_t A, Linv, wbuf, blocks, flag, scale, theta, tiles, work, slots, fail, msel, any_rot;
};
Ptrs carve(const Layout& L, uintptr_t ws, int cap, bool ml_maker) {
  Ptrs r = {};
  uintptr_t q = ws + L.header;  // make_params
  r.A = q;
  q += (size_t)cap * L.Np * L.Np * sizeof(double2);
  r.Linv = q;
  q += (size_t)cap * (L.per_mat - (size_t)L.Np * L.Np * sizeof(double2) - (size_t)L.N * sizeof(double2));
  r.wbuf = q;
  uintptr_t extra = r.wbuf + (size_t)cap * L.N * sizeof(double2);
  extra = (extra + 255) & ~(uintptr_t)255;
  r.blocks = extra;
  q = r.blocks + (size_t)cap * (L.Np / 64) * TB * TB * sizeof(double2);
  if (!ml_maker) {  // dmm_wiener_run
    r.tiles = q;
    q += (size_t)cap * sizeof(dmm_tile);
    r.work = q;
    r.slots = r.work + (((size_t)cap + 8) & ~(size_t)1) * sizeof(int32_t);
    return r;
  }
  r.flag = q;  // dmm_ml_run
  q += (((size_t)cap * (L.Np / 64) + 1) & ~(size_t)1) * sizeof(int);
  r.scale = q;
  q += (size_t)cap * sizeof(double);
  r.theta = q;
  q += (size_t)cap * sizeof(double);
  r.tiles = q;
  q += (size_t)cap * sizeof(dmm_tile);
  r.work = q;
  q += (((size_t)cap + 4) & ~(size_t)1) * sizeof(int32_t);
  r.fail = q;
  q += (((size_t)cap + 1) & ~(size_t)1) * sizeof(int);
  r.msel = q;
  q += (((size_t)cap + 1) & ~(size_t)1) * sizeof(int);
  r.any_rot = q;
  return r;
}
}  // namespace old_form

static long long ncase = 0, nbad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (nbad++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond);   \
    }                                                                   \
  } while (0)

int main() {
  namespace dl = dense_layout;
  const uintptr_t ws = (uintptr_t)1 << 40;
  const int lmaxs[] = {0, 1, 7, 12, 60, 63, 64, 255, 511, 767, 1024};
  const int64_t ntiles[] = {1, 2, 5, 64, 122, 1000, 131328};
  const int64_t opts[] = {0, 1, 6, 24, 1024, 65536};
  for (int npairs = 1; npairs <= 600; ++npairs)
    for (int npol : {1, 2, 4})
      for (int lmax : lmaxs)
        for (int aux = 1; aux <= 2; ++aux) {
          const old_form::Layout O = old_form::layout_of(npairs, npol, lmax, aux);
          const dl::Layout L = dl::layout_of(npairs, npol, lmax, aux);
          CHECK(O.N == L.N && O.Np == L.Np && O.T == L.T && O.per_mat == L.per_mat && O.per_mat_extra == L.per_mat_extra && O.header == L.header &&
                O.sl_bytes == L.sl_bytes && O.sk_pitch == L.sk_pitch);
          for (int64_t ntile : ntiles)
            for (int64_t opt : opts) {
              ++ncase;
              const int64_t wsb = old_form::workspace_bytes(O, aux, ntile, opt);
              const int cap_old = (int)((wsb - O.header - 1024) / (O.per_mat + O.per_mat_extra));  // as the run functions derived it
              const int cap = dl::batch_cap(L, aux, ntile, opt);
              CHECK(cap == cap_old && dl::workspace_bytes(L, cap) == wsb);
              const old_form::Ptrs P = old_form::carve(O, ws, cap_old, aux == 2);
              const dl::Carve C = dl::carve(L, cap, aux);
              CHECK(ws + C.A == P.A && ws + C.aux == P.Linv && ws + C.wbuf == P.wbuf && ws + C.blocks == P.blocks && ws + C.tiles == P.tiles &&
                    ws + C.work == P.work);
              if (aux == 2) CHECK(ws + C.flag == P.flag && ws + C.scale == P.scale && ws + C.theta == P.theta && ws + C.fail == P.fail &&
                                  ws + C.msel == P.msel && ws + C.any_rot == P.any_rot);
              else CHECK(ws + C.slots == P.slots);
              CHECK((int64_t)C.end <= wsb);
              // the work ranges: [first, first + nmat] per user
              const size_t nwork = (aux == 2 ? C.fail : C.slots) - C.work, n4 = nwork / 4;
              if (aux == 1) {  // Wiener: two halves of caph in flight together
                const int caph = cap / 2;
                if (caph >= 1) {
                  const size_t a0 = dl::work_first(0, dl::kBatch), a1 = dl::work_first(caph, dl::kBatch);
                  CHECK(a0 == 0 && a1 == (size_t)caph + 1);                   // the old form: off + h
                  CHECK(a0 + caph < a1 && a1 + caph < n4);
                }
                CHECK(dl::work_first(0, dl::kBatch) + cap < n4);
                continue;
              }
              const int capE = cap / 2, E = std::min(128, cap / 8), cap_direct = E >= 8 ? cap - 2 * E : cap;
              for (int off : {0, capE, cap_direct, cap_direct + E}) {
                CHECK(dl::work_first(off, dl::kBatch) == (size_t)off + (off ? 1 : 0));  // the three old forms
                CHECK(dl::work_first(off, dl::kChunk0) == (size_t)off + 1 + 0);
                CHECK(dl::work_first(off, dl::kChunk1) == (size_t)off + 1 + 1);
              }
              CHECK(dl::work_first(0, dl::kBatch) + cap < n4);  // a synchronous batch alone
              if (capE >= 1) {  // the two halves
                const size_t c0 = dl::work_first(0, dl::kChunk0), c1 = dl::work_first(capE, dl::kChunk1);
                CHECK(c0 + capE < c1 && c1 + capE < n4);
              }
              if (E >= 8) {  // a full direct batch and the two early slots
                const size_t b = dl::work_first(0, dl::kBatch), c0 = dl::work_first(cap_direct, dl::kChunk0), c1 = dl::work_first(cap_direct + E, dl::kChunk1);
                CHECK(b + cap_direct < c0 && c0 + E < c1 && c1 + E < n4);
              }
            }
        }
  printf("dense_layout sweep: %lld cases, %lld failed checks\n", ncase, nbad);
  return nbad ? 1 : 0;
}
