// remap.hip -- MOM_remapping's remapping_core_h (OM4-era reconstructions PCM / PLM / PPM_H4, answer dates >= 20190101)
// and the remapping half of MOM_ALE on gfx950; the regridding half is regrid.hip, the reconstructions ale_dev.h.
//
//   remapping_core_h :234, intersect_src_tgt_grids :642, remap_src_to_sub_grid_om4 :845, remap_src_to_sub_grid :962,
//   remap_sub_to_tgt_grid_om4 :1103, average_value_ppoly :1391   (src/ALE/MOM_remapping.F90)
//   ALE_remap_tracers :760, ALE_remap_set_h_vel :882, ALE_remap_velocities :1089, ALE_PLM_edge_values :1520, TS_PPM_edge_values :1581   (MOM_ALE.F90)
//
// One thread per column, two kernels:
//  k_remap_recon   the reconstruction (edge values, PLM slope) of every source cell in one sweep over k (ale_dev.h: reconstruct_column).
//  k_remap_apply   the reference builds the n0+n1+1 sub-cells of the two grids' intersection in arrays, integrates the
//                  reconstruction over each, corrects the thickest sub-cell of every source cell so that the cell's
//                  integral is conserved to the last bit, and sums the sub-cells of each target cell.  Per-thread arrays
//                  of that size would live in scratch memory; here the merge is STREAMED instead: the sub-cells of one
//                  source cell are replayed three times from a saved merge state (1: effective width and the thickest
//                  sub-cell, 2: the sum of the other sub-cells' integrals, 3: emission into the running target sums),
//                  so a thread carries O(1) state.  Every quantity is formed by the reference's expression in the
//                  reference's order, so the results are bit-identical to orc_remap.c (which keeps the arrays).
#include "ale_dev.h"
#include <cstring>

namespace {

enum { INTEGRATION_PCM = 0, INTEGRATION_PLM = 1, INTEGRATION_PPM = 3 };

// average_value_ppoly :1391-1494 for PCM / PLM / PPM; a_L, a_R, u_c, p2 = E(i0,1), E(i0,2), u0(i0), coefs(i0,2) [PLM]
__device__ __forceinline__ double average_value(int method, double a_L, double a_R, double u_c, double p2, double xa, double xb) {
  if (xb > xa) {
    if (method == INTEGRATION_PCM) return u_c;
    if (method == INTEGRATION_PLM) return (a_L + p2 * 0.5 * (xb + xa));
    const double mx = 0.5 * (xa + xb);
    const double a_c = 0.5 * ((u_c - a_L) + (u_c - a_R));
    if (mx < 0.5) {
      const double xa2b2ab = (xa * xa + xb * xb) + xa * xb;
      return a_L + ((a_R - a_L) * mx + a_c * (3. * (xb + xa) - 2. * xa2b2ab));
    }
    const double Ya = 1. - xa, Yb = 1. - xb, my = 0.5 * (Ya + Yb);
    const double Ya2b2ab = (Ya * Ya + Yb * Yb) + Ya * Yb;
    return a_R + ((a_L - a_R) * my + a_c * (3. * (Yb + Ya) - 2. * Ya2b2ab));
  }
  if (method == INTEGRATION_PCM) return u_c;       // ppoly0_coefs(i0,1) of PCM = u0(i0)
  const double Ya = 1. - xa;
  if (method == INTEGRATION_PLM) {
    if (xa < 0.5) return a_L + xa * (a_R - a_L);
    return a_R + Ya * (a_L - a_R);
  }
  const double a_c = 3. * ((u_c - a_L) + (u_c - a_R));
  if (xa < 0.5) return a_L + xa * ((a_R - a_L) + a_c * Ya);
  return a_R + Ya * ((a_L - a_R) + a_c * xa);
}

struct Merge {            // the running state of intersect_src_tgt_grids' loop :688-795
  double h0s, h1s;        // h0_supply, h1_supply
  double h1full;          // h1(i1), the whole width of the current target cell
  int i0, i1;
  bool src, tgt;          // src_has_volume, tgt_has_volume
};
enum { EV_SRC = 1, EV_TGT = 2 };

struct ApplyArgs {
  int n0, n1, method, om4, fb_sub, fb_tgt;
};

// one iteration of the loop: the new sub-cell's raw width dh (for h0_eff and the thickest-sub-cell test), its stored
// width h_sub, and which cell it closes
__device__ __forceinline__ int merge_step(Merge &m, const double *__restrict__ h0, View v0, const double *__restrict__ h1, View v1,
                                          int n0, int n1, double &dh, double &h_sub, double &eff) {
  dh = dmin(m.h0s, m.h1s);
  eff = dmin(dh, m.h0s);
  h_sub = dh;
  int ev;
  if (m.h0s <= m.h1s && m.src) { m.h1s = m.h1s - dh; ev = EV_SRC; }
  else if (m.h0s >= m.h1s && m.tgt) { m.h0s = m.h0s - dh; ev = EV_TGT; }
  else if (m.src) { h_sub = m.h0s; ev = EV_SRC; }
  else { h_sub = m.h1s; ev = EV_TGT; }
  if (ev == EV_SRC) {
    if (m.i0 < n0) { m.i0 = m.i0 + 1; m.h0s = AT(h0, v0, m.i0); }
    else { m.h0s = 0.; m.src = false; }
  } else {
    if (m.i1 < n1) { m.i1 = m.i1 + 1; m.h1s = AT(h1, v1, m.i1); m.h1full = m.h1s; }
    else { m.h1s = 0.; m.tgt = false; }
  }
  return ev;
}

struct Target {           // remap_sub_to_tgt_grid_om4 :1125-1160, one target cell at a time
  double dh, duh, umin, umax, ufirst;
  bool started;
};
__device__ __forceinline__ void tgt_reset(Target &t) { t.dh = 0.; t.duh = 0.; t.umin = 0.; t.umax = 0.; t.ufirst = 0.; t.started = false; }
__device__ __forceinline__ void tgt_feed(Target &t, double hs, double u, double uh, int fb) {
  if (!t.started) { t.ufirst = u; t.umin = u; t.umax = u; t.started = true; }
  if (fb) { t.umin = dmin(t.umin, u); t.umax = dmax(t.umax, u); }
  t.dh = t.dh + hs;
  t.duh = t.duh + uh;
}
__device__ __forceinline__ double tgt_close(Target &t, double h1, int fb) {
  double r;
  if (h1 > 0.) {
    r = t.duh / t.dh;
    if (fb) r = dmax(t.umin, dmin(t.umax, r));
  } else r = t.ufirst;
  tgt_reset(t);
  return r;
}

// remapping_core_h :234 for one column (after reconstruct_column).  u1 may alias the array the source values came from
// as long as `u0` points to a copy.
// CFG = 1: the OM4 switch set (PPM reconstruction, remap_src_to_sub_grid_om4, target values bounded, sub-cell values not) known at
// compile time -- the merge is issue-bound, and every sub-cell otherwise tests the method and the integrator again.
template <int CFG>
__device__ void apply_column(const ApplyArgs &A0, const double *__restrict__ h0, const double *__restrict__ u0, View v0,
                             const double *__restrict__ E1, const double *__restrict__ E2, const double *__restrict__ C2, View vw,
                             const double *__restrict__ h1, double *u1, View v1) {
  ApplyArgs A = A0;
  if (CFG == 1) { A.method = INTEGRATION_PPM; A.om4 = 1; A.fb_sub = 0; A.fb_tgt = 1; }   // (constants from here on)
  const int n0 = A.n0, n1 = A.n1, ns = n0 + n1 + 1, method = A.method;
  int last_thick = 0;
  for (int k = 1; k <= n0; k++) if (AT(h0, v0, k) > 0.) last_thick = k;          // i0_last_thick_cell :884-889
  Merge m; m.h0s = AT(h0, v0, 1); m.h1s = AT(h1, v1, 1); m.i0 = 1; m.i1 = 1; m.src = true; m.tgt = true;
  m.h1full = m.h1s;
  Target T; tgt_reset(T);
  int i_sub = 1;            // the index of the last sub-cell made
  // the source cell being integrated
  double a_L = AT(E1, vw, 1), a_R = AT(E2, vw, 1), u_c = AT(u0, v0, 1), p2 = (method == INTEGRATION_PLM) ? AT(C2, vw, 1) : 0.;
  double hsrc = AT(h0, v0, 1);
  // sub-cell 1 (zero width, top edge): :716-720, :893-894 / :1012-1030
  double u_s1 = A.om4 ? a_L : ((hsrc > 0.) ? average_value(method, a_L, a_R, u_c, p2, 0., 0.) : u_c);
  if (A.fb_sub && !A.om4) { u_s1 = dmax(u_s1, dmin(a_L, a_R)); u_s1 = dmin(u_s1, dmax(a_L, a_R)); }
  const double uh_s1 = A.om4 ? 0. : 0. * u_s1;
  tgt_feed(T, 0., u_s1, uh_s1, A.fb_tgt);
  double xa = 0., cum = 0., h0_eff_last = 0.;
  // xa, cum after the zero-width sub-cell: non-OM4 runs it through the loop (dh0_eff += 0, xb = 0 or, for a vanished
  // first cell, 1); OM4 starts the loop at sub-cell 2 with xa = 0
  if (!A.om4) { xa = (hsrc > 0.) ? dmin(1., 0. / hsrc) : 1.; }
  while (m.src) {
    const Merge s = m;
    const int i0 = m.i0;
    const double umin0 = dmin(a_L, a_R), umax0 = dmax(a_L, a_R);
    // ---- pass 1: the cell's sub-cells, its effective width h0_eff :722-747 and the thickest sub-cell :726-729.
    // The first NB sub-cells are also kept in registers: a source cell rarely has more, and then passes 2 and 3 work
    // from that buffer instead of replaying the merge.
    constexpr int NB = 4;
    double b_hs[NB], b_h1[NB]; int b_i1[NB]; bool b_has[NB], b_tev[NB];
    Merge t = s;
    int cnt = 0, imax = -1;
    double dh_max = 0., h0_eff = 0., hsub_imax = 0.;
    {
      int ev;
      do {
        const bool has = t.tgt;
        const int i1 = t.i1;
        const double h1f = t.h1full;
        double dh, hs, eff;
        ev = merge_step(t, h0, v0, h1, v1, n0, n1, dh, hs, eff);
        h0_eff = h0_eff + eff;
        if (dh >= dh_max) { imax = cnt; dh_max = dh; hsub_imax = hs; }
#pragma unroll
        for (int q = 0; q < NB; q++)
          if (q == cnt) { b_hs[q] = hs; b_h1[q] = h1f; b_i1[q] = i1; b_has[q] = has; b_tev[q] = (ev == EV_TGT); }
        cnt++;
      } while (ev != EV_SRC);
    }
    const double den = A.om4 ? h0_eff : hsrc;
    h0_eff_last = h0_eff;
    const bool adjust = (i0 <= last_thick) && (hsub_imax > 0.);
    double duh = 0.;
    if (i0 == 1) duh = duh + uh_s1;
    if (cnt <= NB) {
      // ---- passes 2 and 3 from the register buffer
      double b_u[NB], b_uh[NB];
#pragma unroll
      for (int c = 0; c < NB; c++) {
        if (c < cnt) {
          const double hs = b_hs[c];
          double u, uh;
          if (A.om4 && (i_sub + 1 + c) == ns) { u = AT(E2, vw, n0); uh = u * hs; }
          else {
            cum = cum + hs;
            double xb;
            if (den > 0.) { xb = dmin(1., cum / den); u = average_value(method, a_L, a_R, u_c, p2, xa, xb); }
            else { xb = 1.; u = u_c; }
            if (A.fb_sub) { u = dmax(u, umin0); u = dmin(u, umax0); }
            uh = hs * u;
            xa = xb;
          }
          b_u[c] = u; b_uh[c] = uh;
          if (c != imax) duh = duh + uh;
        }
      }
      const double uh_adj = u_c * hsrc - duh;
#pragma unroll
      for (int c = 0; c < NB; c++) {
        if (c < cnt) {
          double uh = b_uh[c];
          if (adjust && c == imax) uh = uh_adj;
          if (b_has[c]) {
            tgt_feed(T, b_hs[c], b_u[c], uh, A.fb_tgt);
            if (b_tev[c]) AT(u1, v1, b_i1[c]) = tgt_close(T, b_h1[c], A.fb_tgt);
          }
        }
      }
      i_sub += cnt;
    } else {
      // ---- pass 2: sum of u*h over the sub-cells other than the thickest :939-957
      {
        t = s;
        double xa2 = xa, cum2 = cum;
        for (int c = 0; c < cnt; c++) {
          double dh, hs, eff;
          merge_step(t, h0, v0, h1, v1, n0, n1, dh, hs, eff);
          double u, uh;
          if (A.om4 && (i_sub + 1 + c) == ns) { u = AT(E2, vw, n0); uh = u * hs; }
          else {
            cum2 = cum2 + hs;
            double xb;
            if (den > 0.) { xb = dmin(1., cum2 / den); u = average_value(method, a_L, a_R, u_c, p2, xa2, xb); }
            else { xb = 1.; u = u_c; }
            if (A.fb_sub) { u = dmax(u, umin0); u = dmin(u, umax0); }
            uh = hs * u;
            xa2 = xb;
          }
          if (c != imax) duh = duh + uh;
        }
      }
      const double uh_adj = u_c * hsrc - duh;
      // ---- pass 3: emit the sub-cells into the target sums
      {
        t = s;
        for (int c = 0; c < cnt; c++) {
          const bool has_tgt = t.tgt;
          const int i1 = t.i1;
          const double h1f = t.h1full;
          double dh, hs, eff;
          const int ev = merge_step(t, h0, v0, h1, v1, n0, n1, dh, hs, eff);
          i_sub++;
          double u, uh;
          if (A.om4 && i_sub == ns) { u = AT(E2, vw, n0); uh = u * hs; }
          else {
            cum = cum + hs;
            double xb;
            if (den > 0.) { xb = dmin(1., cum / den); u = average_value(method, a_L, a_R, u_c, p2, xa, xb); }
            else { xb = 1.; u = u_c; }
            if (A.fb_sub) { u = dmax(u, umin0); u = dmin(u, umax0); }
            uh = hs * u;
            xa = xb;
          }
          if (adjust && c == imax) uh = uh_adj;
          if (has_tgt) {
            tgt_feed(T, hs, u, uh, A.fb_tgt);
            if (ev == EV_TGT) AT(u1, v1, i1) = tgt_close(T, h1f, A.fb_tgt);
          }
        }
      }
    }
    m = t;
    if (m.src) {          // the next source cell: "dh0_eff = 0 ; xa = 0" :932-934
      xa = 0.; cum = 0.;
      a_L = AT(E1, vw, m.i0); a_R = AT(E2, vw, m.i0); u_c = AT(u0, v0, m.i0); hsrc = m.h0s;
      if (method == INTEGRATION_PLM) p2 = AT(C2, vw, m.i0);
    }
  }
  // ---- the target column is deeper than the source column: the remaining sub-cells continue the last source cell
  {
    const double dd = A.om4 ? h0_eff_last : hsrc;   // h0_eff(n0) | h0(n0)
    const double umin0 = dmin(a_L, a_R), umax0 = dmax(a_L, a_R);
    while (m.tgt) {
      const int i1 = m.i1;
      const double h1f = m.h1full;
      double dh, hs, eff;
      merge_step(m, h0, v0, h1, v1, n0, n1, dh, hs, eff);
      i_sub++;
      double u, uh;
      if (A.om4 && i_sub == ns) { u = AT(E2, vw, n0); uh = u * hs; }
      else {
        cum = cum + hs;
        double xb;
        if (dd > 0.) { xb = dmin(1., cum / dd); u = average_value(method, a_L, a_R, u_c, p2, xa, xb); }
        else { xb = 1.; u = u_c; }
        if (A.fb_sub) { u = dmax(u, umin0); u = dmin(u, umax0); }
        uh = hs * u;
        xa = xb;
      }
      tgt_feed(T, hs, u, uh, A.fb_tgt);
      AT(u1, v1, i1) = tgt_close(T, h1f, A.fb_tgt);
    }
  }
}

// the 3-D form: columns (i0..i1, j0..j1) with mask > 0; h_old / h_new / fields on the same staggering
template <bool IL, bool PAIR = false>
__global__ void __launch_bounds__(256, PAIR ? 2 : RECON_WAVES)
k_remap_recon(Dm d, const double *__restrict__ mask, ReconArgs A, const double *__restrict__ h_old, const double *__restrict__ f,
              double *E1, double *E2, double *C2, double *Ucopy, int i0, int i1, int j0, int j1, int hst) {
  const int i = I_BASE(i0) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < i0 || i > i1 || j > j1) return;
  const size_t x = ix2(d, i, j);
  if (mask && !(mask[x] > 0.)) return;
  View v; v.base = x; v.lev = (size_t)d.slab;
  reconstruct_column<IL, PAIR>(A, h_old, f, v, E1, E2, C2, Ucopy, v, hst);
}
template <int CFG>
__global__ void __launch_bounds__(256)
k_remap_apply(Dm d, const double *__restrict__ mask, ApplyArgs A, const double *__restrict__ h_old, const double *__restrict__ h_new,
              const double *__restrict__ E1, const double *__restrict__ E2, const double *__restrict__ C2,
              const double *__restrict__ Ucopy, double *f, int i0, int i1, int j0, int j1) {
  const int i = I_BASE(i0) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < i0 || i > i1 || j > j1) return;
  const size_t x = ix2(d, i, j);
  if (!(mask[x] > 0.)) return;
  View v; v.base = x; v.lev = (size_t)d.slab;
  apply_column<CFG>(A, h_old, Ucopy, v, E1, E2, C2, v, h_new, f, v);
}
// ---- the merge for the OM4 switch set, shared by the fields that live on one pair of grids --------------------------------
// REMAPPING_SCHEME = PPM_*, remap_src_to_sub_grid_om4 :845, target values bounded, sub-cell values not (what
// `k_remap_apply<1>` is compiled for), with the same results bit for bit.  k_remap_apply spends two thirds of a wavefront's
// life waiting for memory (SQ_WAIT_ANY / SQ_WAVE_CYCLES = 0.64): every step of the merge needs h1 at an index that differs
// from lane to lane, and needs it at once.  Here
//  * the target column goes through a sliding window in LDS (MG_W levels per lane, the level MG_LEAD below the source cell
//    enters at the top of every iteration from a load issued one iteration earlier; a lane whose target index has left the
//    window reads global memory as before), and the source cell's values are loaded one iteration ahead, so a wavefront
//    waits at one place per source cell, for loads that are an iteration old;
//  * what the sub-cells of a source cell share between fields -- their widths, the positions xa, xb in the cell and the
//    polynomial weights that follow from them (two thirds of average_value_ppoly's arithmetic and its division) -- is formed
//    once and used by NF fields (T and S; tracers in pairs);
//  * a cell's sub-cells are kept as (width, two weights, form), from which a field's sub-cell mean costs four operations,
//    so the pass that sums u*h for the conservation fix and the pass that feeds the targets both evaluate it instead of
//    storing it; a cell with more than MG_NB sub-cells replays the merge from its saved start as k_remap_apply does.
// Three facts about the merge, for thicknesses >= 0, are used: (1) inside the source loop the sub-cells of a source cell are
// the closings of consecutive target cells followed by its own closing; a target cell closed by the 2nd, 3rd, ... of them
// lies inside the source cell and its whole width is the sub-cell's; (2) a sub-cell of positive width exists only in a
// source cell of positive thickness, which is then not below i0_last_thick_cell, so `adjust` is (hsub_imax > 0) alone;
// (3) the column's last sub-cell (u = E2(n0), :926-929) is the closing of source cell n0 when the targets are exhausted, or
// else the closing of target n1.
constexpr int MG_NT = 3, MG_W = 16, MG_LEAD = 8;
template <int NF> struct MergeFields { const double2 *E12[NF]; const double *Uc[NF]; double *out[NF]; };   // E12: (E1, E2) of a cell side by side
struct SubW { double p, q; int mode; };   // 0 / 1: xb > xa, left / right form; 2 / 3: a point, left / right; 4: u0(i0); 5: E2(n0)

// xa, xb of the next sub-cell (:900-912) and the weights of average_value_ppoly's PPM branches :1420-1437, :1470-1480
__device__ __forceinline__ SubW sub_weights(double &xa, double &cum, double hs, double den, bool last) {
  SubW w; w.p = 0.; w.q = 0.;
  if (last) { w.mode = 5; return w; }
  cum = cum + hs;
  if (den > 0.) {
    const double xb = dmin(1., cum / den);
    if (xb > xa) {
      const double mx = 0.5 * (xa + xb);
      if (mx < 0.5) { w.mode = 0; w.p = mx; w.q = 3. * (xb + xa) - 2. * ((xa * xa + xb * xb) + xa * xb); }
      else {
        const double Ya = 1. - xa, Yb = 1. - xb;
        w.mode = 1; w.p = 0.5 * (Ya + Yb); w.q = 3. * (Yb + Ya) - 2. * ((Ya * Ya + Yb * Yb) + Ya * Yb);
      }
    } else {
      const double Ya = 1. - xa;
      if (xa < 0.5) { w.mode = 2; w.p = xa; w.q = Ya; }
      else { w.mode = 3; w.p = Ya; w.q = xa; }
    }
    xa = xb;
  } else { w.mode = 4; xa = 1.; }
  return w;
}
// the same for the sub-cell that closes its source cell when it is not the column's last: cum >= den (the same sums, with
// hs >= dh in the last term), so xb = min(1, cum / den) is 1 without the division, which leaves the two right-hand forms
// with Yb = 0 (and x + 0 = x, x * 0 = 0 for the finite x >= 0 here)
__device__ __forceinline__ SubW sub_weights_closing(double &xa, double &cum, double hs, double den) {
  SubW w;
  cum = cum + hs;
  if (den > 0.) {
    const double Ya = 1. - xa;
    if (1. > xa) { w.mode = 1; w.p = 0.5 * Ya; w.q = 3. * Ya - 2. * (Ya * Ya); }
    else { w.mode = 3; w.p = Ya; w.q = xa; }
  } else { w.mode = 4; w.p = 0.; w.q = 0.; }
  xa = 1.;
  return w;
}
struct CellPoly { double aL, aR, uc, dLR, dRL, ac, ac3; };
__device__ __forceinline__ CellPoly cell_poly(double aL, double aR, double uc) {
  CellPoly c; c.aL = aL; c.aR = aR; c.uc = uc; c.dLR = aR - aL; c.dRL = aL - aR;
  const double s = (uc - aL) + (uc - aR);
  c.ac = 0.5 * s; c.ac3 = 3. * s;
  return c;
}
__device__ __forceinline__ double sub_mean(const SubW &w, const CellPoly &c) {
  const bool right = (w.mode & 1);
  const double B = right ? c.aR : c.aL, D = right ? c.dRL : c.dLR;
  if (w.mode < 2) return B + (D * w.p + c.ac * w.q);
  if (w.mode < 4) return B + w.p * (D + c.ac3 * w.q);
  return (w.mode == 4) ? c.uc : c.aR;
}
__device__ __forceinline__ double sub_mean_right(const SubW &w, const CellPoly &c) {   // modes 1, 3, 4, 5
  if (w.mode == 1) return c.aR + (c.dRL * w.p + c.ac * w.q);
  if (w.mode == 3) return c.aR + w.p * (c.dRL + c.ac3 * w.q);
  return (w.mode == 4) ? c.uc : c.aR;
}

template <int NF, bool PAIR = false>
__global__ void __launch_bounds__(256)
k_remap_merge(Dm d, const double *__restrict__ mask, const double *__restrict__ h0p, const double *__restrict__ h1p, MergeFields<NF> F,
              int i0, int i1, int j0, int j1, int hst) {
  __shared__ double win_all[4][MG_W][64];
  const int i = I_BASE(i0) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < i0 || i > i1 || j > j1) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  if (!(mask[x] > 0.)) return;
  const int n = d.nk;
  double *win = &win_all[threadIdx.y][0][threadIdx.x];
#define WIN(L) win[((L) & (MG_W - 1)) * 64]
#define LEV(p, L) (p)[x + (size_t)((L) - 1) * slab]
  // (hst != 0: velocity columns on the cells' thicknesses, see reconstruct_column)
#define HLEV(p, L) (PAIR ? 0.5 * (LEV(p, L) + LEV((p) + hst, L)) : LEV(p, L))
  // the window holds the levels k + MG_LEAD - MG_W + 1 .. k + MG_LEAD of h1 during iteration k
  auto next_target = [&](int &it, double &h1s, double &h1full, bool &tgt, int k) {     // :765-771
    if (it < n) {
      it = it + 1;
      h1s = WIN(it);                   // (the slot exists whatever it holds)
      if ((unsigned)(it - (k + MG_LEAD - MG_W + 1)) >= (unsigned)MG_W) {
        h1s = HLEV(h1p, it);
        asm volatile("" : "+v"(h1s));  // (the wait for this load belongs here, not where the paths meet: there it would also
      }                                //  hold the lanes that read the window until this iteration's prefetches are back)
      h1full = h1s;
    } else { h1s = 0.; tgt = false; }
  };
  double h1s, h1_pf;
  {
    double t[MG_LEAD];
#pragma unroll
    for (int L = 1; L <= MG_LEAD; L++) t[L - 1] = (L <= n) ? HLEV(h1p, L) : 0.;
    h1_pf = (MG_LEAD + 1 <= n) ? HLEV(h1p, MG_LEAD + 1) : 0.;
#pragma unroll
    for (int L = 1; L <= MG_LEAD; L++) WIN(L) = t[L - 1];
    h1s = t[0];
  }
  double n_h0 = HLEV(h0p, 1), n_aL[NF], n_aR[NF], n_uc[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) { const double2 e = LEV(F.E12[f], 1); n_aL[f] = e.x; n_aR[f] = e.y; n_uc[f] = LEV(F.Uc[f], 1); }
  double h1full = h1s;
  int it = 1;
  bool tgt = true;
  // The running target cell (remap_sub_to_tgt_grid_om4 :1125-1160).  It always holds a sub-cell when a source cell begins:
  // the zero-width first one :893-894, later the closing sub-cell of the previous source cell.
  double Tdh = 0. + 0., Tduh[NF], Tmin[NF], Tmax[NF], Tfirst[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) { Tfirst[f] = n_aL[f]; Tmin[f] = n_aL[f]; Tmax[f] = n_aL[f]; Tduh[f] = 0. + 0.; }
  double xa = 0., cum = 0., h0_eff_last = 0.;
  CellPoly P[NF];
  // one more sub-cell of the running target / the first sub-cell of the next one / the target's value :1146-1158
  auto feed = [&](bool fresh, double hs, const double *u, const double *uh) {
    Tdh = (fresh ? 0. : Tdh) + hs;
#pragma unroll
    for (int f = 0; f < NF; f++) {
      if (fresh) { Tfirst[f] = u[f]; Tmin[f] = u[f]; Tmax[f] = u[f]; Tduh[f] = 0. + uh[f]; }
      else { Tmin[f] = dmin(Tmin[f], u[f]); Tmax[f] = dmax(Tmax[f], u[f]); Tduh[f] = Tduh[f] + uh[f]; }
    }
  };
  auto close = [&](int lev, double h1f) {
#pragma unroll
    for (int f = 0; f < NF; f++) {
      double r;
      if (h1f > 0.) { r = Tduh[f] / Tdh; r = dmax(Tmin[f], dmin(Tmax[f], r)); }
      else r = Tfirst[f];
      LEV(F.out[f], lev) = r;
    }
  };
  for (int k = 1; k <= n; k++) {
    // ---- what was asked for during the previous iteration arrives, the next requests leave
    const double hsrc = n_h0;
#pragma unroll
    for (int f = 0; f < NF; f++) P[f] = cell_poly(n_aL[f], n_aR[f], n_uc[f]);
    WIN(k + MG_LEAD) = h1_pf;
    if (k + 1 <= n) {
      n_h0 = HLEV(h0p, k + 1);
#pragma unroll
      for (int f = 0; f < NF; f++) { const double2 e = LEV(F.E12[f], k + 1); n_aL[f] = e.x; n_aR[f] = e.y; n_uc[f] = LEV(F.Uc[f], k + 1); }
    }
    if (k + MG_LEAD + 1 <= n) h1_pf = HLEV(h1p, k + MG_LEAD + 1);
    // ---- the cell's sub-cells (intersect_src_tgt_grids' loop :700-795): the target cells that end inside it, then its own
    // closing; their widths, the effective width h0_eff :722-747 and the thickest one :726-729
    double h0s = hsrc;
    const double s_h1s = h1s, s_h1full = h1full;
    const int s_it = it;
    double b_hs[MG_NT];
    int nt = 0, imax = -1;
    double dh_max = 0., h0_eff = 0., hsub_imax = 0.;
    bool more = tgt && !(h0s <= h1s);
#pragma unroll
    for (int c = 0; c < MG_NT; c++) {
      if (more) {
        const double dh = dmin(h0s, h1s);
        h0_eff = h0_eff + dh;
        if (dh >= dh_max) { imax = c; dh_max = dh; hsub_imax = dh; }
        b_hs[c] = dh; nt = c + 1;
        h0s = h0s - dh;
        next_target(it, h1s, h1full, tgt, k);
        more = tgt && !(h0s <= h1s);
      }
    }
    while (more) {           // more of them than the buffer holds
      const double dh = dmin(h0s, h1s);
      h0_eff = h0_eff + dh;
      if (dh >= dh_max) { imax = nt; dh_max = dh; hsub_imax = dh; }
      nt++;
      h0s = h0s - dh;
      next_target(it, h1s, h1full, tgt, k);
      more = tgt && !(h0s <= h1s);
    }
    double hs_l;
    {
      const double dh = dmin(h0s, h1s);
      hs_l = dh;
      if (h0s <= h1s) h1s = h1s - dh;
      else hs_l = h0s;
      h0_eff = h0_eff + dh;
      if (dh >= dh_max) { imax = nt; dh_max = dh; hsub_imax = hs_l; }
    }
    const bool has_last = tgt, col_last = (k == n) && !tgt, adjust = (hsub_imax > 0.);
    const double den = h0_eff;
    h0_eff_last = h0_eff;
    xa = 0.; cum = 0.;
    if (nt <= MG_NT) {
      SubW w[MG_NT], w_l;
#pragma unroll
      for (int c = 0; c < MG_NT; c++) if (c < nt) w[c] = sub_weights(xa, cum, b_hs[c], den, false);
      if (col_last) { w_l.mode = 5; w_l.p = 0.; w_l.q = 0.; }
      else w_l = sub_weights_closing(xa, cum, hs_l, den);
      double u[MG_NT][NF], u_l[NF], uh_adj[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) {
        double duh = 0. + 0.;
#pragma unroll
        for (int c = 0; c < MG_NT; c++)
          if (c < nt) { u[c][f] = sub_mean(w[c], P[f]); if (c != imax) duh = duh + b_hs[c] * u[c][f]; }
        u_l[f] = sub_mean_right(w_l, P[f]);
        if (nt != imax) duh = duh + hs_l * u_l[f];
        uh_adj[f] = P[f].uc * hsrc - duh;
      }
      double uh[NF];
#pragma unroll
      for (int c = 0; c < MG_NT; c++) {
        if (c < nt) {
#pragma unroll
          for (int f = 0; f < NF; f++) uh[f] = (adjust && c == imax) ? uh_adj[f] : b_hs[c] * u[c][f];
          feed(c > 0, b_hs[c], u[c], uh);
          close(s_it + c, (c == 0) ? s_h1full : b_hs[c]);
        }
      }
      if (has_last) {
#pragma unroll
        for (int f = 0; f < NF; f++) uh[f] = (adjust && nt == imax) ? uh_adj[f] : hs_l * u_l[f];
        feed(nt > 0, hs_l, u_l, uh);
      }
    } else {
      // the merge is replayed from the cell's start, once for the sum :939-957 ...
      double duh[NF], uh_adj[NF], u1[NF], uh1[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) duh[f] = 0. + 0.;
      double r_h0s = hsrc, r_h1s = s_h1s, r_h1full = s_h1full, xa2 = 0., cum2 = 0.;
      int r_it = s_it;
      bool r_tgt = true;
      for (int c = 0; c <= nt; c++) {
        double hs = hs_l;
        SubW w;
        if (c < nt) {
          hs = dmin(r_h0s, r_h1s);
          r_h0s = r_h0s - hs;
          next_target(r_it, r_h1s, r_h1full, r_tgt, k);
          w = sub_weights(xa2, cum2, hs, den, false);
        } else if (col_last) { w.mode = 5; w.p = 0.; w.q = 0.; }
        else w = sub_weights_closing(xa2, cum2, hs, den);
#pragma unroll
        for (int f = 0; f < NF; f++) { const double t = hs * sub_mean(w, P[f]); if (c != imax) duh[f] = duh[f] + t; }
      }
#pragma unroll
      for (int f = 0; f < NF; f++) uh_adj[f] = P[f].uc * hsrc - duh[f];
      // ... and once to feed the targets
      r_h0s = hsrc; r_h1s = s_h1s; r_h1full = s_h1full; r_it = s_it; r_tgt = true;
      for (int c = 0; c <= nt; c++) {
        const int lev = r_it;
        const double h1f = r_h1full;
        double hs = hs_l;
        SubW w;
        if (c < nt) {
          hs = dmin(r_h0s, r_h1s);
          r_h0s = r_h0s - hs;
          next_target(r_it, r_h1s, r_h1full, r_tgt, k);
          w = sub_weights(xa, cum, hs, den, false);
        } else if (col_last) { w.mode = 5; w.p = 0.; w.q = 0.; }
        else w = sub_weights_closing(xa, cum, hs, den);
#pragma unroll
        for (int f = 0; f < NF; f++) { u1[f] = sub_mean(w, P[f]); uh1[f] = (adjust && c == imax) ? uh_adj[f] : hs * u1[f]; }
        if (c < nt || has_last) feed(c > 0, hs, u1, uh1);
        if (c < nt) close(lev, h1f);
      }
    }
  }
  // ---- the target column is deeper than the source column: the remaining sub-cells continue the last source cell
  bool fresh = false;
  while (tgt) {
    const int lev = it;
    const double h1f = h1full, hs = h1s;
    next_target(it, h1s, h1full, tgt, n);
    const SubW w = sub_weights(xa, cum, hs, h0_eff_last, !tgt);
    double u1[NF], uh1[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) { u1[f] = sub_mean(w, P[f]); uh1[f] = hs * u1[f]; }
    feed(fresh, hs, u1, uh1);
    close(lev, h1f);
    fresh = true;
  }
#undef WIN
#undef LEV
}

// the packed form of the unit tests: column c holds n0 | n1 values back to back; work arrays are [k][ncol]
__global__ void __launch_bounds__(64)
k_remap_packed(int ncol, ReconArgs R, ApplyArgs A, const double *__restrict__ h0, const double *__restrict__ u0,
               const double *__restrict__ h1, double *u1, double *E1, double *E2, double *C2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  View v0, v1, vw;
  v0.base = (size_t)c * A.n0; v0.lev = 1; v1.base = (size_t)c * A.n1; v1.lev = 1; vw.base = c; vw.lev = ncol;
  reconstruct_column(R, h0, u0, v0, E1, E2, C2, nullptr, vw);
  apply_column<0>(A, h0, u0, v0, E1, E2, C2, vw, h1, u1, v1);
}

__global__ void __launch_bounds__(256)
k_set_h_vel(Dm d, const double *__restrict__ G, const double *__restrict__ h_new, double *__restrict__ h_u, double *__restrict__ h_v) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni - 1 || j > d.nj - 1) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const bool do_u = (j >= 0) && (gm(G, d, MOM6X_G_mask2dCu)[x] > 0.), do_v = (i >= 0) && (gm(G, d, MOM6X_G_mask2dCv)[x] > 0.);
  const int k0 = blockIdx.z * KCHUNK, k1 = min(k0 + KCHUNK, d.nk);
  for (int k = k0; k < k1; k++) {
    const size_t c = x + (size_t)k * slab;
    const double hc = h_new[c];
    if (do_u) h_u[c] = 0.5 * (hc + h_new[c + 1]);
    if (do_v) h_v[c] = 0.5 * (hc + h_new[c + d.pitch]);
  }
}

int check_params(const mom6x_remapping_params *p, int n0, ReconArgs &R, ApplyArgs &A, int n1) {
  REQUIRE(p, MOM6X_EINVAL, "remapping: null parameters");
  REQUIRE(p->scheme == MOM6X_REMAP_PCM || p->scheme == MOM6X_REMAP_PLM || p->scheme == MOM6X_REMAP_PPM_H4 ||
          p->scheme == MOM6X_REMAP_PPM_IH4, MOM6X_EUNSUPPORTED,
          "MOM_remapping, build_reconstructions_1d: The selected remapping method is invalid");
  REQUIRE(p->answer_date >= 20190101, MOM6X_EUNSUPPORTED, "remapping: REMAPPING_ANSWER_DATE < 20190101 is not on the device path");
  REQUIRE(n0 >= 1 && n1 >= 1, MOM6X_EINVAL, "remapping: empty column");
  int scheme = p->scheme;                                   // :441-447
  if (n0 <= 1) scheme = MOM6X_REMAP_PCM;
  else if (n0 <= 3) scheme = std::min(scheme, (int)MOM6X_REMAP_PLM);
  else if (n0 <= 4) scheme = std::min(scheme, (int)MOM6X_REMAP_PPM_H4);
  R.scheme = scheme; R.boundary_extrapolation = p->boundary_extrapolation; R.h_neglect = p->h_neglect;
  R.h_neglect_edge = p->h_neglect_edge; R.n0 = n0;
  A.n0 = n0; A.n1 = n1; A.om4 = p->om4_remap_via_sub_cells; A.fb_sub = p->force_bounds_in_subcell; A.fb_tgt = p->force_bounds_in_target;
  A.method = (scheme == MOM6X_REMAP_PCM) ? INTEGRATION_PCM : (scheme == MOM6X_REMAP_PLM ? INTEGRATION_PLM : INTEGRATION_PPM);
  return MOM6X_OK;
}

// OM4's switch set (what k_remap_apply<1> is compiled for), and whether the shared-field kernel k_remap_merge serves it:
// MOM6X_REMAP_MERGE=apply asks for the one-field streamed merge k_remap_apply for every switch set
bool om4_switch_set(const ApplyArgs &A) { return A.method == INTEGRATION_PPM && A.om4 && !A.fb_sub && A.fb_tgt; }
bool merge_usable(const ApplyArgs &A) {
  static const bool merge_off = [] { const char *e = getenv("MOM6X_REMAP_MERGE"); return e && !strcmp(e, "apply"); }();
  return om4_switch_set(A) && !merge_off;
}
// remap nf (1 or 2) 3-D fields that live on the same pair of grids, in place, on the points (i0..i1, j0..j1) where mask > 0
// (R, A: check_params' for nk layers on both grids).  hst != 0: h_old / h_new are the CELLS' thicknesses and the fields live at
// velocity points hst elements apart from their second cell (merge_usable only)
int remap_fields(mom6x_ctx *c, const ReconArgs &R, const ApplyArgs &A, int mask_id, int i0, int i1, int j0, int j1, const double *h_old,
                 const double *h_new, double *const *f, int nf, int hst = 0) {
  const Dm d = c->d;
  int rc;
  const bool shared = merge_usable(A);
  REQUIRE(shared || hst == 0, MOM6X_EUNSUPPORTED, "remap_fields: velocity columns on the cells' thicknesses need the OM4 switch set");
  if (!shared && nf > 1) {
    for (int m = 0; m < nf; m++) if ((rc = remap_fields(c, R, A, mask_id, i0, i1, j0, j1, h_old, h_new, f + m, 1))) return rc;
    return MOM6X_OK;
  }
  static const Scr work[2][4] = {{SCR_t0, SCR_t1, SCR_t3, SCR_t2}, {SCR_KE, SCR_q, SCR_absv, SCR_t2}};   // E1 (| E1 and E2 side by side), E2, Ucopy, C2 (PLM only)
  double *W[2][4];
  for (int m = 0; m < nf; m++)
    for (int a = 0; a < 4; a++) if ((rc = ctx_scratch(c, work[m][a], (shared && a == 0) ? 2 * d.nk : d.nk, &W[m][a]))) return rc;
  const dim3 b = blk2(), g = grid3(nxa(i1 - i0 + 1, i0), j1 - j0 + 1, 1, b);
  const double *mask = c->G + (size_t)mask_id * d.slab;
  const auto recon = !shared ? k_remap_recon<false> : hst ? k_remap_recon<true, true> : k_remap_recon<true>;   // (hst = 0 unless shared)
  for (int m = 0; m < nf; m++)
    KLAUNCH(c, "k_remap_recon", recon, g, b, d, mask, R, h_old, (const double *)f[m], W[m][0], W[m][1], W[m][3], W[m][2], i0, i1, j0, j1, hst);
  if (shared && nf == 2) {
    MergeFields<2> F;
    for (int m = 0; m < 2; m++) { F.E12[m] = (const double2 *)W[m][0]; F.Uc[m] = W[m][2]; F.out[m] = f[m]; }
    REQUIRE(hst == 0, MOM6X_EINVAL, "remap_fields: velocity columns go one field at a time");
    KLAUNCH(c, "k_remap_merge<2>", k_remap_merge<2>, g, b, d, mask, h_old, h_new, F, i0, i1, j0, j1, 0);
  } else if (shared) {
    MergeFields<1> F;
    F.E12[0] = (const double2 *)W[0][0]; F.Uc[0] = W[0][2]; F.out[0] = f[0];
    if (hst) KLAUNCH(c, "k_remap_merge<1>", (k_remap_merge<1, true>), g, b, d, mask, h_old, h_new, F, i0, i1, j0, j1, hst);
    else KLAUNCH(c, "k_remap_merge<1>", k_remap_merge<1>, g, b, d, mask, h_old, h_new, F, i0, i1, j0, j1, 0);
  } else
    KLAUNCH(c, "k_remap_apply", (om4_switch_set(A) ? k_remap_apply<1> : k_remap_apply<0>), g, b, d, mask, A, h_old, h_new,
            (const double *)W[0][0], (const double *)W[0][1], (const double *)W[0][3], (const double *)W[0][2], f[0], i0, i1, j0, j1);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
int remap_fields(mom6x_ctx *c, const mom6x_remapping_params *p, int mask_id, int i0, int i1, int j0, int j1, const double *h_old,
                 const double *h_new, double *const *f, int nf) {   // ... from the parameters themselves
  ReconArgs R; ApplyArgs A;
  const int rc = check_params(p, c->d.nk, R, A, c->d.nk);
  return rc ? rc : remap_fields(c, R, A, mask_id, i0, i1, j0, j1, h_old, h_new, f, nf);
}

// ALE_PLM_edge_values, MOM_ALE.F90:1520-1577: one thread per column; slp(k-1), slp(k), slp(k+1) are carried in registers so
// that the column is read once (h, Q) and written once (Q_t, Q_b).
__global__ void __launch_bounds__(256)
k_plm_edge_values(Dm d, const double *__restrict__ h, const double *__restrict__ Q, int bdry_extrap, double hn,
                  double *__restrict__ Q_t, double *__restrict__ Q_b) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni || j > d.nj) return;
  const int N = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
#define HK(k) h[x + (size_t)((k) - 1) * slab]
#define QK(k) Q[x + (size_t)((k) - 1) * slab]
  if (N >= 3) {
    double hm = HK(1), hc = HK(2), um = QK(1), uc = QK(2);
    double s_m = 0.0, s_c, s_p;
    {
      const double hp = HK(3), up = QK(3);
      s_c = PLM_slope_wa(hm, hc, hp, hn, um, uc, up);                                   // slp(2)
    }
    for (int k = 2; k <= N - 1; k++) {
      const double hp = HK(k + 1), up = QK(k + 1);
      s_p = (k + 1 <= N - 1) ? PLM_slope_wa(hc, hp, HK(k + 2), hn, uc, up, QK(k + 2)) : 0.;   // slp(k+1) (slp(N) = 0)
      const double mslp = PLM_monotonized_slope(um, uc, up, s_m, s_c, s_p);
      Q_t[x + (size_t)(k - 1) * slab] = uc - 0.5 * mslp;
      Q_b[x + (size_t)(k - 1) * slab] = uc + 0.5 * mslp;
      hm = hc; hc = hp; um = uc; uc = up; s_m = s_c; s_c = s_p;
    }
  }
  if (bdry_extrap && N >= 2) {
    double mslp = -PLM_extrapolate_slope(HK(2), HK(1), hn, QK(2), QK(1));
    Q_t[x] = QK(1) - 0.5 * mslp; Q_b[x] = QK(1) + 0.5 * mslp;
    mslp = PLM_extrapolate_slope(HK(N - 1), HK(N), hn, QK(N - 1), QK(N));
    Q_t[x + (size_t)(N - 1) * slab] = QK(N) - 0.5 * mslp; Q_b[x + (size_t)(N - 1) * slab] = QK(N) + 0.5 * mslp;
  } else {
    Q_t[x] = QK(1); Q_b[x] = QK(1);
    Q_t[x + (size_t)(N - 1) * slab] = QK(N); Q_b[x + (size_t)(N - 1) * slab] = QK(N);
  }
#undef HK
#undef QK
}
}  // namespace

// ALE_PLM_edge_values(CS, G, GV, h, Q, bdry_extrap, Q_t, Q_b), MOM_ALE.F90:1520 (answer dates >= 20190101)
extern "C" int mom6x_ALE_PLM_edge_values(mom6x_ctx *c, const double *h, const double *Q, int bdry_extrap, double *Q_t, double *Q_b) {
  REQUIRE(c && h && Q && Q_t && Q_b, MOM6X_EINVAL, "mom6x_ALE_PLM_edge_values: null argument");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2();
  KLAUNCH(c, "k_plm_edge_values", k_plm_edge_values, grid3(nxa(d.ni + 2, -1), d.nj + 2, 1, b), b, d, h, Q, bdry_extrap,
          c->GV.H_subroundoff, Q_t, Q_b);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

// One field of TS_PPM_edge_values, MOM_ALE.F90:1581-1663 (answer dates >= 20190101): edge_values_implicit_h4 + PPM_reconstruction
// (+ PPM_boundary_extrapolation) of every column of (isc-1..iec+1, jsc-1..jec+1) -- the PPM_IH4 reconstruction of the remapping
// kernels with h_neglect = h_neglect_edge = GV%H_subroundoff and no land mask; Q_t, Q_b = ppol_E(:,1), ppol_E(:,2).
extern "C" int mom6x_ALE_PPM_edge_values(mom6x_ctx *c, const double *h, const double *Q, int bdry_extrap, double *Q_t, double *Q_b) {
  REQUIRE(c && h && Q && Q_t && Q_b, MOM6X_EINVAL, "mom6x_ALE_PPM_edge_values: null argument");
  REQUIRE(c->dims.nk >= 4, MOM6X_EUNSUPPORTED, "mom6x_ALE_PPM_edge_values: edge_values_implicit_h4 needs at least 4 layers");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  double *C2;
  int rc;
  if ((rc = ctx_scratch(c, SCR_KE, d.nk, &C2))) return rc;   // the tridiagonal solve's c1 column
  ReconArgs R;
  R.scheme = MOM6X_REMAP_PPM_IH4; R.boundary_extrapolation = bdry_extrap; R.h_neglect = c->GV.H_subroundoff;
  R.h_neglect_edge = c->GV.H_subroundoff; R.n0 = d.nk;
  const dim3 b = blk2();
  KLAUNCH(c, "k_remap_recon", k_remap_recon<false>, grid3(nxa(d.ni + 2, -1), d.nj + 2, 1, b), b, d, (const double *)nullptr, R, h, Q, Q_t, Q_b,
          C2, (double *)nullptr, -1, d.ni, -1, d.nj, 0);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_ALE_remap_tracers(mom6x_ctx *c, const mom6x_remapping_params *p, const double *h_old, const double *h_new,
                                       double *const *fields, int nfields) {
  REQUIRE(c && p && h_old && h_new && (fields || nfields == 0), MOM6X_EINVAL, "ALE_remap_tracers: null argument");
  HIPCHK(hipSetDevice(c->device));
  for (int m = 0; m < nfields; m++) REQUIRE(fields[m], MOM6X_EINVAL, "ALE_remap_tracers: null tracer array");
  for (int m = 0; m < nfields; m += 2) {     // the tracers share their grids: two at a time through one merge
    int rc = remap_fields(c, p, MOM6X_G_mask2dT, 0, c->d.ni - 1, 0, c->d.nj - 1, h_old, h_new, fields + m, std::min(2, nfields - m));
    if (rc) return rc;
  }
  return MOM6X_OK;
}

extern "C" int mom6x_ALE_remap_set_h_vel(mom6x_ctx *c, const double *h_new, double *h_u, double *h_v) {
  REQUIRE(c && h_new && h_u && h_v, MOM6X_EINVAL, "ALE_remap_set_h_vel: null argument");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2();
  KLAUNCH(c, "k_set_h_vel", k_set_h_vel, grid3(nxa(d.ni + 1, -1), d.nj + 1, nchunks(d.nk), b), b, d, c->G, h_new, h_u, h_v);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

// The KE-conserving correction of ALE_remap_velocities :1166-1195 (REMAP_VEL_CONSERVE_KE with allow_preserve_variance): one thread
// per velocity column, three walks over k in the reference's order (u_bt and sum(h2); the two baroclinic KE integrals; the rescaling).
__global__ void __launch_bounds__(256)
k_remap_conserve_ke(Dm d, const double *__restrict__ G, int mask_plane, int i0, int i1, int j0, int j1, const double *__restrict__ h1,
                    const double *__restrict__ h2, const double *__restrict__ u_src, double *__restrict__ u_tgt, double H_subroundoff) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > i1 || j > j1) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  if (!(gm(G, d, mask_plane)[x] > 0.0)) return;
  const int nz = d.nk;
  double u_bt = 0.0, hsum = 0.0;
  for (int k = 0; k < nz; k++) { const size_t c = x + (size_t)k * slab; u_bt = u_bt + h2[c] * u_tgt[c]; hsum = hsum + h2[c]; }
  u_bt = u_bt / (hsum + H_subroundoff);
  double ke_c_src = 0.0, ke_c_tgt = 0.0;
  for (int k = 0; k < nz; k++) {
    const size_t c = x + (size_t)k * slab;
    const double a = u_src[c] - u_bt, b = u_tgt[c] - u_bt;
    ke_c_src = ke_c_src + h1[c] * (a * a);
    ke_c_tgt = ke_c_tgt + h2[c] * (b * b);
  }
  // (the 25 % cap on the amplification of the baroclinic part, :1182-1191)
  const double rescale_coef = (ke_c_src < 1.5625 * ke_c_tgt) ? sqrt(ke_c_src / ke_c_tgt) : 1.25;
  for (int k = 0; k < nz; k++) { const size_t c = x + (size_t)k * slab; u_tgt[c] = u_bt + rescale_coef * (u_tgt[c] - u_bt); }
}

void ALE_free(mom6x_ctx *c) {
  AleState *S = c->ale;
  if (!S) return;
  (void)hipFree(S->regrid_res); (void)hipFree(S->regrid_vec); (void)hipFree(S->remap_src); (void)hipFree(S->remap_hvel);
  delete S;
  c->ale = nullptr;
}

static int remap_velocities(mom6x_ctx *c, const mom6x_remapping_params *p, const double *h_old_u, const double *h_old_v,
                            const double *h_new_u, const double *h_new_v, double *u, double *v, bool conserve_ke) {
  REQUIRE(c && p && h_old_u && h_old_v && h_new_u && h_new_v && u && v, MOM6X_EINVAL, "ALE_remap_velocities: null argument");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const size_t n3 = (size_t)d.slab * d.nk;
  // The source column of the correction: allocated by the FIRST call with REMAP_VEL_CONSERVE_KE (a synchronising hipMalloc, once per
  // context; the entry point has no initialisation of its own), kept until the context goes.
  // ORDER: the reference masks the near-bottom velocities (mask_near_bottom_vel, BBL_h_vel_mask / h_vel_mask; MOM_ALE.F90:1194-1200)
  // AFTER the correction.  The device carries neither mask (both default to 0: nothing is masked); whoever adds them must apply them
  // after k_remap_conserve_ke, not inside remap_fields.
  AleState *A = ale_state(c);
  if (conserve_ke && !A->remap_src) HIPCHK(hipMalloc(&A->remap_src, n3 * sizeof(double)));
  const dim3 b = blk2();
  if (conserve_ke) HIPCHK(hipMemcpyAsync(A->remap_src, u, n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  int rc = remap_fields(c, p, MOM6X_G_mask2dCu, -1, d.ni - 1, 0, d.nj - 1, h_old_u, h_new_u, &u, 1);
  if (rc) return rc;
  if (conserve_ke)
    KLAUNCH(c, "k_remap_conserve_ke", k_remap_conserve_ke, grid3(d.ni + 1, d.nj, 1, b), b, d, c->G, (int)MOM6X_G_mask2dCu, -1, d.ni - 1, 0, d.nj - 1,
            h_old_u, h_new_u, (const double *)A->remap_src, u, c->GV.H_subroundoff);
  if (conserve_ke) HIPCHK(hipMemcpyAsync(A->remap_src, v, n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  rc = remap_fields(c, p, MOM6X_G_mask2dCv, 0, d.ni - 1, -1, d.nj - 1, h_old_v, h_new_v, &v, 1);
  if (rc) return rc;
  if (conserve_ke)
    KLAUNCH(c, "k_remap_conserve_ke", k_remap_conserve_ke, grid3(d.ni, d.nj + 1, 1, b), b, d, c->G, (int)MOM6X_G_mask2dCv, 0, d.ni - 1, -1, d.nj - 1,
            h_old_v, h_new_v, (const double *)A->remap_src, v, c->GV.H_subroundoff);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_ALE_remap_velocities(mom6x_ctx *c, const mom6x_remapping_params *p, const double *h_old_u, const double *h_old_v,
                                          const double *h_new_u, const double *h_new_v, double *u, double *v) {
  return remap_velocities(c, p, h_old_u, h_old_v, h_new_u, h_new_v, u, v, false);
}
// ALE_remap_set_h_vel(h_old) + ALE_remap_set_h_vel(h_new) + ALE_remap_velocities as MOM.F90 calls them one after the other
// (ALE_regridding_and_remapping), from the CELLS' thicknesses: with OM4's switch set the thicknesses at the velocity points are
// formed where the remapping reads them (the same expression: the same bits) and the four h_u / h_v arrays are never written or
// read -- 6 words per cell-layer less.  Any other switch set: the arrays are made in work space and the call above follows.
extern "C" int mom6x_ALE_remap_velocities_from_h(mom6x_ctx *c, const mom6x_remapping_params *p, const double *h_old, const double *h_new,
                                                 double *u, double *v) {
  REQUIRE(c && p && h_old && h_new && u && v, MOM6X_EINVAL, "ALE_remap_velocities: null argument");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  ReconArgs R; ApplyArgs M;
  int rc = check_params(p, d.nk, R, M, d.nk);
  if (rc) return rc;
  if (merge_usable(M)) {
    if ((rc = remap_fields(c, R, M, MOM6X_G_mask2dCu, -1, d.ni - 1, 0, d.nj - 1, h_old, h_new, &u, 1, 1))) return rc;
    return remap_fields(c, R, M, MOM6X_G_mask2dCv, 0, d.ni - 1, -1, d.nj - 1, h_old, h_new, &v, 1, d.pitch);
  }
  const size_t n3 = (size_t)d.slab * d.nk;
  AleState *A = ale_state(c);
  if (!A->remap_hvel) { HIPCHK(hipMalloc(&A->remap_hvel, 4 * n3 * sizeof(double))); HIPCHK(hipMemsetAsync(A->remap_hvel, 0, 4 * n3 * sizeof(double), c->stream)); }
  double *hu0 = A->remap_hvel, *hv0 = hu0 + n3, *hu1 = hv0 + n3, *hv1 = hu1 + n3;
  if ((rc = mom6x_ALE_remap_set_h_vel(c, h_old, hu0, hv0)) || (rc = mom6x_ALE_remap_set_h_vel(c, h_new, hu1, hv1))) return rc;
  return remap_velocities(c, p, hu0, hv0, hu1, hv1, u, v, false);
}
// ... with allow_preserve_variance = .true. and REMAP_VEL_CONSERVE_KE (CS%conserve_ke, MOM_ALE.F90:331): MOM.F90's call in the time step
extern "C" int mom6x_ALE_remap_velocities_conserve_ke(mom6x_ctx *c, const mom6x_remapping_params *p, const double *h_old_u,
                                                      const double *h_old_v, const double *h_new_u, const double *h_new_v, double *u,
                                                      double *v) {
  return remap_velocities(c, p, h_old_u, h_old_v, h_new_u, h_new_v, u, v, true);
}

extern "C" int mom6x_remapping_core_h(mom6x_ctx *c, const mom6x_remapping_params *p, int ncol, int n0, const double *h0,
                                      const double *u0, int n1, const double *h1, double *u1) {
  REQUIRE(c && h0 && u0 && h1 && u1 && ncol >= 1, MOM6X_EINVAL, "remapping_core_h: null argument");
  HIPCHK(hipSetDevice(c->device));
  ReconArgs R; ApplyArgs A;
  int rc = check_params(p, n0, R, A, n1);
  if (rc) return rc;
  double *w = nullptr;
  const size_t per = (size_t)n0 * ncol;
  HIPCHK(hipMalloc(&w, 3 * per * sizeof(double)));
  KLAUNCH(c, "k_remap_packed", k_remap_packed, dim3((ncol + 63) / 64), dim3(64), ncol, R, A, h0, u0, h1, u1, w, w + per, w + 2 * per);
  hipError_t e = hipStreamSynchronize(c->stream);
  (void)hipFree(w);
  HIPCHK(e);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
