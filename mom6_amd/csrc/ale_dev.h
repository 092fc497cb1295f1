// ale_dev.h -- what the two files of MOM_ALE share (remap.hip: MOM_remapping; regrid.hip: MOM_regridding): the module's state and the
// reconstructions -- PLM_functions.F90, PPM_functions.F90, regrid_edge_values.F90 (bound_edge_values :39, check_discontinuous_edge_values
// :132, edge_values_explicit_h4 :213, edge_values_implicit_h4 :473, end_value_h4 :634), build_reconstructions_1d MOM_remapping.F90:410.
#pragma once
#include "mom6x_dev.h"
#include <cfloat>

namespace {

struct View { size_t base, lev; };                       // element k (1-based) of a column: p[base + (k-1)*lev]
#define AT(p, v, k) (p)[(v).base + (size_t)((k) - 1) * (v).lev]

__device__ __forceinline__ double fsign(double a, double b) { return copysign(fabs(a), b); }   // Fortran sign()
__device__ __forceinline__ double dmax3(double a, double b, double c) { return dmax(dmax(a, b), c); }
__device__ __forceinline__ double dmin3(double a, double b, double c) { return dmin(dmin(a, b), c); }

// ---- PLM_functions.F90 --------------------------------------------------------------------------------------------
__device__ double PLM_slope_wa(double h_l, double h_c, double h_r, double h_neglect, double u_l, double u_c, double u_r) {   // :27-66
  const double sigma_r = u_r - u_c, sigma_l = u_c - u_l;
  const double sigma_c = 2.0 * (u_r - u_l) * (h_c / (h_l + 2.0 * h_c + h_r + h_neglect));
  const double u_min = dmin3(u_l, u_c, u_r), u_max = dmax3(u_l, u_c, u_r);
  double s;
  if ((sigma_l * sigma_r) > 0.0) s = fsign(dmin(fabs(sigma_c), 2. * dmin(u_c - u_min, u_max - u_c)), sigma_c);
  else s = 0.0;
  if (u_c - 0.5 * fabs(s) < u_min || u_c + 0.5 * fabs(s) > u_max) s = s * (1. - DBL_EPSILON);
  if (fabs(s) < 1.E-140) s = 0.;
  return s;
}
__device__ double PLM_monotonized_slope(double u_l, double u_c, double u_r, double s_l, double s_c, double s_r) {   // :124-162
  const double almost_two = 2. * (1. - DBL_EPSILON);
  const double e_r = u_l + 0.5 * s_l, e_l = u_r - 0.5 * s_r;
  double slp = fabs(s_c);
  double edge = u_c - 0.5 * s_c;
  if ((edge - e_r) * (u_c - edge) < 0.) { edge = 0.5 * (edge + e_r); slp = dmin(slp, fabs(edge - u_c) * almost_two); }
  edge = u_c + 0.5 * s_c;
  if ((edge - u_c) * (e_l - edge) < 0.) { edge = 0.5 * (edge + e_l); slp = dmin(slp, fabs(edge - u_c) * almost_two); }
  return fsign(slp, s_c);
}
__device__ double PLM_extrapolate_slope(double h_l, double h_c, double h_neglect, double u_l, double u_c) {   // :170-191
  const double hl = h_l + h_neglect, hc = h_c + h_neglect;
  const double left_edge = (u_l * hc + u_c * hl) / (hl + hc);
  return 2.0 * (u_c - left_edge);
}

// ---- regrid_edge_values.F90: end_value_h4 :634-747 ------------------------------------------------------------------
__device__ void end_value_h4(const double *dz, const double *u, double *Csys) {
  const double min_frac = 1.0e-6;
  double h1 = dz[0], h2 = dz[1], h3 = dz[2], h4 = dz[3];
  if ((h2 + h3) < min_frac * h1) h3 = min_frac * h1 - h2;
  if ((h3 + h4) < min_frac * h1) h4 = min_frac * h1 - h3;
  const double h12 = h1 + h2, h23 = h2 + h3, h34 = h3 + h4;
  const double h123 = h12 + h3, h234 = h2 + h34, h1234 = h12 + h34;
  const double I_denB3 = 1.0 / (h123 * h12 * h23);
  const double I_h12 = (h123 * h23) * I_denB3;
  const double I_h23 = (h12 * h123) * I_denB3;
  const double I_h123 = (h12 * h23) * I_denB3;
  const double I_denom = 1.0 / (h1234 * (h234 * h34));
  const double I_h234 = (h1234 * h34) * I_denom;
  const double I_h1234 = (h234 * h34) * I_denom;
  const double W11 = -h1 * (I_h1234 + I_h123 + I_h12);
  const double W21 = h1 * h12 * (I_h234 * I_h1234 + I_h23 * (I_h234 + I_h123));
  const double W31 = -h1 * h12 * h123 * I_denom;
  const double W12 = 2.0 * (I_h12 * (1.0 + (h1 + h12) * (I_h1234 + I_h123)) + h1 * I_h1234 * I_h123);
  const double W22 = -2.0 * ((h1 * h12 * I_h1234) * (I_h23 * (I_h234 + I_h123)) + (h1 + h12) * (I_h1234 * I_h234 + I_h23 * (I_h234 + I_h123)));
  const double W32 = 2.0 * ((h1 + h12) * h123 + h1 * h12) * I_denom;
  const double W13 = -3.0 * I_h12 * I_h123 * (1.0 + I_h1234 * ((h1 + h12) + h123));
  const double W23 = 3.0 * I_h23 * (I_h123 + I_h1234 * ((h1 + h12) + h123) * (I_h123 + I_h234));
  const double W33 = -3.0 * ((h1 + h12) + h123) * I_denom;
  const double W14 = 4.0 * I_h1234 * I_h123 * I_h12;
  const double W24 = -4.0 * I_h1234 * (I_h23 * (I_h123 + I_h234));
  const double W34 = 4.0 * I_denom;
  Csys[0] = ((u[0] + (W11 * (u[1] - u[0]))) + (W21 * (u[2] - u[1]))) + (W31 * (u[3] - u[2]));
  Csys[1] = ((W12 * (u[1] - u[0])) + (W22 * (u[2] - u[1]))) + (W32 * (u[3] - u[2]));
  Csys[2] = ((W13 * (u[1] - u[0])) + (W23 * (u[2] - u[1]))) + (W33 * (u[3] - u[2]));
  Csys[3] = ((W14 * (u[1] - u[0])) + (W24 * (u[2] - u[1]))) + (W34 * (u[3] - u[2]));
}

struct ReconArgs {
  int scheme;                 // the scheme after build_reconstructions_1d's small-n0 demotion
  int boundary_extrapolation;
  double h_neglect, h_neglect_edge;
  int n0;
};

// interior edge value of edge_values_explicit_h4 :246-279 between cells (h1,u1) and (h2,u2), with their outer neighbours
__device__ __forceinline__ double edge_h4(double h0, double h1, double h2, double h3, double u0, double u1, double u2, double u3, double hne) {
  const double hMinFrac = 1.e-5;
  if (h0 + h1 == 0.0 || h1 + h2 == 0.0 || h2 + h3 == 0.0) {
    const double h_min = hMinFrac * dmax(hne, (h0 + h1) + (h2 + h3));
    h0 = dmax(h_min, h0); h1 = dmax(h_min, h1); h2 = dmax(h_min, h2); h3 = dmax(h_min, h3);
  }
  const double I_h12 = 1.0 / (h1 + h2);
  const double I_den_et2 = 1.0 / (((h0 + h1) + h2) * (h0 + h1)), I_h012 = (h0 + h1) * I_den_et2;
  const double I_den_et3 = 1.0 / ((h1 + (h2 + h3)) * (h2 + h3)), I_h123 = (h2 + h3) * I_den_et3;
  const double et1 = (1.0 + (h1 * I_h012 + (h0 + h1) * I_h123)) * I_h12 * (h2 * (h2 + h3)) * u1 +
                     (1.0 + (h2 * I_h123 + (h2 + h3) * I_h012)) * I_h12 * (h1 * (h0 + h1)) * u2;
  const double et2 = (h1 * (h2 * (h2 + h3)) * I_den_et2) * (u1 - u0);
  const double et3 = (h2 * (h1 * (h0 + h1)) * I_den_et3) * (u2 - u3);
  return (et1 + (et2 + et3)) / ((h0 + h1) + (h2 + h3));
}
// bound_edge_values :39-101 for one cell (a, b: its edge values; m / p: the neighbour, or the cell itself at the ends)
__device__ __forceinline__ void bound_edges(double um, double uk, double up, double hm, double hk, double hp, double &a, double &b) {
  double slope_x_h = 0.0;
  if (((hm + hp) + 2.0 * hk) > 0.0) {
    const double sigma_l = (uk - um);
    const double sigma_c = (up - um) * (hk / ((hm + hp) + 2.0 * hk));
    const double sigma_r = (up - uk);
    if ((sigma_l * sigma_r) > 0.0) slope_x_h = fsign(dmin3(fabs(sigma_l), fabs(sigma_c), fabs(sigma_r)), sigma_c);
  }
  if ((um - a) * (a - uk) < 0.0) a = uk - fsign(dmin(fabs(slope_x_h), fabs(a - uk)), slope_x_h);
  if ((up - b) * (b - uk) < 0.0) b = uk + fsign(dmin(fabs(slope_x_h), fabs(b - uk)), slope_x_h);
  a = dmax(dmin(a, dmax(um, uk)), dmin(um, uk));
  b = dmax(dmin(b, dmax(up, uk)), dmin(up, uk));
}
// the interior-cell part of PPM_limiter_standard :80-116
__device__ __forceinline__ void ppm_limit(double u_l, double u_c, double u_r, double &edge_l, double &edge_r) {
  if ((u_r - u_c) * (u_c - u_l) <= 0.0) {
    edge_l = u_c; edge_r = u_c;
  } else {
    const double expr1 = 3.0 * (edge_r - edge_l) * ((u_c - edge_l) + (u_c - edge_r));
    const double expr2 = (edge_r - edge_l) * (edge_r - edge_l);
    if (expr1 > expr2) {
      edge_l = u_c + 2.0 * (u_c - edge_r);
      edge_l = dmax(dmin(edge_l, dmax(u_l, u_c)), dmin(u_l, u_c));
    } else if (expr1 < -expr2) {
      edge_r = u_c + 2.0 * (u_c - edge_l);
      edge_r = dmax(dmin(edge_r, dmax(u_r, u_c)), dmin(u_r, u_c));
    }
  }
  if (fabs(edge_r - edge_l) < dmax(1.e-60, DBL_EPSILON * fabs(u_c))) { edge_l = u_c; edge_r = u_c; }
}

#ifndef RECON_RING
#define RECON_RING 4
#endif
#ifndef RECON_WAVES
#define RECON_WAVES 4
#endif
// build_reconstructions_1d :410-550 for one column.  h, u: the source column; E1, E2, C2: outputs (C2 only for PLM);
// Ucopy: a copy of u (the field itself may be overwritten by the remapped values).  All 1-based.
// The reference makes one pass over the column per stage (edge values, bounding, discontinuity check, limiter; first-guess
// slopes, monotonized slopes, coefficients).  Every stage only looks one or two cells away, so here ONE sweep carries a
// register window of the cells and of the intermediate values and finishes cell k-1 when cell k has been bounded: the
// column arrays are read once and the results written once, all with the same k in every lane (coalesced).
// IL: the two edge values of a cell next to each other in ONE array (E1[2 n], E1[2 n + 1]; E2 unused) -- what k_remap_merge reads:
// one 16-byte store and load per lane instead of two 8-byte ones.
// hst != 0: the column is a VELOCITY column and h holds the thicknesses of the CELLS: the thickness at the velocity point is formed
// where it is read, 0.5 * (h(cell) + h(cell + hst)) -- ALE_remap_set_h_vel's expression (MOM_ALE.F90:882; k_set_h_vel), so the bits
// are those of the h_u / h_v arrays it would have written and the remapping would have read back.
template <bool IL = false, bool PAIR = false>
__device__ void reconstruct_column(const ReconArgs &A, const double *__restrict__ h, const double *__restrict__ u, View vs,
                                   double *E1, double *E2, double *C2, double *Ucopy, View vw, int hst = 0) {
  const int N = A.n0;
#define H(k) (PAIR ? 0.5 * (AT(h, vs, k) + AT(h + hst, vs, k)) : AT(h, vs, k))
#define U(k) AT(u, vs, k)
#define e1(k) E1[(IL ? 2 : 1) * (vw.base + (size_t)((k) - 1) * vw.lev)]
#define e2(k) (IL ? E1 + 1 : E2)[(IL ? 2 : 1) * (vw.base + (size_t)((k) - 1) * vw.lev)]
#define c2(k) AT(C2, vw, k)
  if (A.scheme == MOM6X_REMAP_PCM) {                                          // PCM_functions.F90:16-35
    for (int k = 1; k <= N; k++) { const double v = U(k); e1(k) = v; e2(k) = v; if (Ucopy) AT(Ucopy, vw, k) = v; }
    return;
  }
  if (A.scheme == MOM6X_REMAP_PLM) {                                          // PLM_reconstruction :197-262 (N >= 2)
    const double almost_one = 1. - DBL_EPSILON, hn = A.h_neglect;
    // window at step k: cells k-1 (m), k (c), k+1 (p), k+2 (q); slopes slp(k-1..k+1), mslp(k-1..k)
    double um = U(1), uc = U(1), up = (N >= 2) ? U(2) : 0., hc = H(1), hp = (N >= 2) ? H(2) : 0.;
    double s_m = 0., s_c = 0., s_p = 0., ms_m = 0., ms_c = 0.;   // slp(k-1), slp(k), slp(k+1), mslp(k-1), mslp(k)
    // step k finishes cell k-1; cell 1 and N are written explicitly
    // prime: k = 1: slp(1) = 0, slp(2)
    if (N >= 3) s_p = PLM_slope_wa(H(1), H(2), H(3), hn, U(1), U(2), U(3));
    e1(1) = uc; e2(1) = uc; c2(1) = 0.;
    if (Ucopy) AT(Ucopy, vw, 1) = uc;
    for (int k = 2; k <= N - 1; k++) {
      // shift the window to cell k
      um = uc; uc = up; hc = hp; up = U(k + 1); hp = H(k + 1);
      s_m = s_c; s_c = s_p; ms_m = ms_c;
      s_p = (k + 1 <= N - 1) ? PLM_slope_wa(hc, hp, H(k + 2), hn, uc, up, U(k + 2)) : 0.;     // slp(k+1)
      ms_c = PLM_monotonized_slope(um, uc, up, s_m, s_c, s_p);                                   // mslp(k)
      if (Ucopy) AT(Ucopy, vw, k) = uc;
      if (k >= 3) {   // finish cell k-1 (an interior cell): needs mslp(k-1), mslp(k), slp(k)
        const double slope = ms_m, ukm = um;
        const double u_l = ukm - 0.5 * slope, u_r = ukm + 0.5 * slope;
        e1(k - 1) = u_l; e2(k - 1) = u_r;
        double p2 = (u_r - u_l);
        const double edge = p2 + u_l;
        const double e_r = uc - 0.5 * fsign(ms_c, s_c);
        if ((edge - ukm) * (e_r - edge) < 0.) p2 = p2 * almost_one;
        c2(k - 1) = p2;
      }
    }
    if (N >= 3) {   // finish cell N-1: mslp(N) = slp(N) = 0
      const double slope = ms_c, ukm = uc;
      const double u_l = ukm - 0.5 * slope, u_r = ukm + 0.5 * slope;
      e1(N - 1) = u_l; e2(N - 1) = u_r;
      double p2 = (u_r - u_l);
      const double edge = p2 + u_l;
      const double e_r = up - 0.5 * fsign(0., 0.);
      if ((edge - ukm) * (e_r - edge) < 0.) p2 = p2 * almost_one;
      c2(N - 1) = p2;
    }
    const double uN = U(N);
    e1(N) = uN; e2(N) = uN; c2(N) = 0.;
    if (Ucopy) AT(Ucopy, vw, N) = uN;
    if (A.boundary_extrapolation) {                                           // PLM_boundary_extrapolation :274-308
      double slope = -PLM_extrapolate_slope(H(2), H(1), hn, U(2), U(1));
      e1(1) = U(1) - 0.5 * slope; e2(1) = U(1) + 0.5 * slope;
      c2(1) = e2(1) - e1(1);
      slope = PLM_extrapolate_slope(H(N - 1), H(N), hn, U(N - 1), U(N));
      e1(N) = U(N) - 0.5 * slope; e2(N) = U(N) + 0.5 * slope;
      c2(N) = e2(N) - e1(N);
    }
    return;
  }
  // ---- PPM_H4 / PPM_IH4 (N >= 4): edge_values_explicit_h4 :213-348 or edge_values_implicit_h4 :473-630, then
  // PPM_limiter_standard :62-121
  const double hne = A.h_neglect_edge;
  const bool implicit = (A.scheme == MOM6X_REMAP_PPM_IH4);
  double edge_1, edge_2, edge_N, edge_N1;        // the two edge values at either end come from end_value_h4 :314-346
  {
    double dz[4], ut[4], C[4];
    for (int i = 1; i <= 4; i++) { dz[i - 1] = dmax(hne, H(i)); ut[i - 1] = U(i); }
    end_value_h4(dz, ut, C);
    edge_1 = C[0];
    edge_2 = C[0] + dz[0] * (C[1] + dz[0] * (C[2] + dz[0] * C[3]));
    for (int i = 1; i <= 4; i++) { dz[i - 1] = dmax(hne, H(N + 1 - i)); ut[i - 1] = U(N + 1 - i); }
    end_value_h4(dz, ut, C);
    edge_N1 = C[0];
    edge_N = C[0] + dz[0] * (C[1] + dz[0] * (C[2] + dz[0] * C[3]));
  }
  if (implicit) {
    // The N+1 interface values solve a diagonally dominant tridiagonal system (solve_diag_dominant_tridiag,
    // regrid_solvers.F90:246-280): the forward sweep leaves X(1..N) in the E1 column and c1(1..N) in the C2 column (free
    // for a PPM scheme), X(N+1) stays in a register; the backward sweep turns E1 into the final interface values, which
    // the limiter sweep below then reads one interface ahead of the cell it overwrites.
    double I_pivot = 1.0 / (1.0 + 0.0);                                       // tri_c(1) = 1, tri_u(1) = 0 :573-575
    double d1 = 1.0 * I_pivot, x_prev = edge_1 * I_pivot;
    c2(1) = 0.0 * I_pivot; e1(1) = x_prev;
    double h_a = H(1), u_a = U(1);
    for (int k = 2; k <= N; k++) {                                            // row k couples cells k-1 and k :528-552
      const double h_b = H(k), u_b = U(k);
      double h0 = dmax(h_a, hne), h1 = dmax(h_b, hne);
      if (fabs(h0) < 1.0e-12 * fabs(h1)) h0 = 1.0e-12 * h1;
      if (fabs(h1) < 1.0e-12 * fabs(h0)) h1 = 1.0e-12 * h0;
      const double I_h2 = 1.0 / ((h0 + h1) * (h0 + h1));
      const double alpha = (h1 * h1) * I_h2, beta = (h0 * h0) * I_h2, abmix = (h0 * h1) * I_h2;
      const double a = 2.0 * alpha * (alpha + 2.0 * beta + 3.0 * abmix);
      const double b = 2.0 * beta * (beta + 2.0 * alpha + 3.0 * abmix);
      const double Ac = 2.0 * abmix, R = a * u_a + b * u_b;
      const double denom_t1 = Ac + d1 * alpha;
      I_pivot = 1.0 / (denom_t1 + beta);
      d1 = denom_t1 * I_pivot;
      c2(k) = beta * I_pivot;
      x_prev = (R - alpha * x_prev) * I_pivot;
      e1(k) = x_prev;
      h_a = h_b; u_a = u_b;
    }
    I_pivot = 1.0 / (1.0 + d1 * 0.0);                                         // tri_c(N+1) = 1, tri_l(N+1) = 0 :608-613
    edge_N1 = (edge_N1 - 0.0 * x_prev) * I_pivot;
    double x_next = edge_N1;
    for (int k = N; k >= 1; k--) { x_next = e1(k) - c2(k) * x_next; e1(k) = x_next; }
    edge_1 = x_next;
  }
  // window at step k (bounding cell k, finishing cell k-1): cells k-2 (mm), k-1 (m), k (c), k+1 (p), k+2 (q)
  double umm = 0., um = 0., uc = 0., up = U(1), uq = U(2), hm = 0., hc = 0., hp = H(1), hq = H(2);
  double ed_c = 0., ed_p = edge_1;               // edge(k), edge(k+1)
  double a_m = 0., b_m = 0.;                     // bounded edge values of cell k-1 (a_m already through its pair check with k-2)
  // The column is read four cells ahead of its use (a ring of registers indexed by the level mod 4, the loop unrolled by
  // four so that the index is static and nothing is copied): a lane that asked for cell k+2 and used it in the same step
  // kept two loads in flight, and the sweep ran at the latency of a load per step.
  double ru[RECON_RING], rh[RECON_RING];
#pragma unroll
  for (int L = 3; L <= 2 + RECON_RING; L++) { ru[L % RECON_RING] = (L <= N) ? U(L) : 0.; rh[L % RECON_RING] = (L <= N) ? H(L) : 0.; }
  for (int k0 = 1; k0 <= N; k0 += RECON_RING)
#pragma unroll
  for (int kq = 0; kq < RECON_RING; kq++) {
    const int k = k0 + kq;
    if (k > N) break;
    umm = um; um = uc; uc = up; up = uq; hm = hc; hc = hp; hp = hq;
    if (k + 2 <= N) {
      uq = ru[(kq + 3) % RECON_RING]; hq = rh[(kq + 3) % RECON_RING];                      // level k + 2 (k0 = 1 mod RECON_RING)
      if (k + 2 + RECON_RING <= N) { ru[(kq + 3) % RECON_RING] = U(k + 2 + RECON_RING); rh[(kq + 3) % RECON_RING] = H(k + 2 + RECON_RING); }
    }
    ed_c = ed_p;
    const int e = k + 1;                         // the edge below cell k
    if (implicit) {
      ed_p = edge_N1;
      if (e <= N) { ed_p = e1(e); asm volatile("" : "+v"(ed_p)); }   // (its wait stays on this path: the explicit scheme's loads run ahead)
    }
    else if (e <= 2) ed_p = edge_2;
    else if (e >= N) ed_p = (e == N) ? edge_N : edge_N1;
    else ed_p = edge_h4(hm, hc, hp, hq, um, uc, up, uq, hne);      // i = e: cells e-2 .. e+1 = k-1 .. k+2
    if (Ucopy) AT(Ucopy, vw, k) = uc;
    double a = ed_c, b = ed_p;
    bound_edges((k > 1) ? um : uc, uc, (k < N) ? up : uc, (k > 1) ? hm : hc, hc, (k < N) ? hp : hc, a, b);
    if (k > 1) {
      // check_discontinuous_edge_values :132-150 for the pair (k-1, k)
      if ((a - b_m) * (uc - um) < 0.0) {
        double u0_avg = 0.5 * (b_m + a);
        u0_avg = dmax(dmin(u0_avg, dmax(um, uc)), dmin(um, uc));
        b_m = u0_avg; a = u0_avg;
      }
      // cell k-1 is complete
      if (k - 1 == 1) { e1(1) = um; e2(1) = um; }
      else {
        ppm_limit(umm, um, uc, a_m, b_m);
        e1(k - 1) = a_m; e2(k - 1) = b_m;
      }
    }
    a_m = a; b_m = b;
  }
  e1(N) = uc; e2(N) = uc;
  if (A.boundary_extrapolation) {                                             // PPM_boundary_extrapolation :166-296
    const double hn = A.h_neglect;
    {
      const double h0 = H(1), h1 = H(2), u0 = U(1), u1 = U(2);
      const double b = 4.0 * (u1 - e1(2)) + 2.0 * (u1 - e2(2));               // ppoly_coef(2,2) of PPM_reconstruction :49
      double u1_r = b * ((h0 + hn) / (h1 + hn));
      const double slope = 2.0 * (u1 - u0);
      if (fabs(u1_r) > fabs(slope)) u1_r = slope;
      double u0_r = e1(2);
      double u0_l = 3.0 * u0 + 0.5 * u1_r - 2.0 * u0_r;
      const double exp1 = (u0_r - u0_l) * (u0 - 0.5 * (u0_l + u0_r));
      const double exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
      if (exp1 > exp2) u0_l = 3.0 * u0 - 2.0 * u0_r;
      if (exp1 < -exp2) u0_r = 3.0 * u0 - 2.0 * u0_l;
      e1(1) = u0_l; e2(1) = u0_r;
    }
    {
      const double h0 = H(N - 1), h1 = H(N), u0 = U(N - 1), u1 = U(N);
      const double b = 4.0 * (u0 - e1(N - 1)) + 2.0 * (u0 - e2(N - 1));       // ppoly_coef(N-1,2)
      const double c = 3.0 * ((e2(N - 1) - u0) + (e1(N - 1) - u0));           // ppoly_coef(N-1,3)
      double u1_l = (b + 2 * c);
      u1_l = u1_l * ((h1 + hn) / (h0 + hn));
      const double slope = 2.0 * (u1 - u0);
      if (fabs(u1_l) > fabs(slope)) u1_l = slope;
      double u0_l = e2(N - 1);
      double u0_r = 3.0 * u1 - 0.5 * u1_l - 2.0 * u0_l;
      const double exp1 = (u0_r - u0_l) * (u1 - 0.5 * (u0_l + u0_r));
      const double exp2 = (u0_r - u0_l) * (u0_r - u0_l) / 6.0;
      if (exp1 > exp2) u0_l = 3.0 * u1 - 2.0 * u0_r;
      if (exp1 < -exp2) u0_r = 3.0 * u1 - 2.0 * u0_l;
      e1(N) = u0_l; e2(N) = u0_r;
    }
  }
#undef H
#undef U
#undef e1
#undef e2
#undef c2
}
}  // namespace

// The arrays the ALE entry points allocate on first use (they have no initialisation of their own) and keep until the context goes
struct AleState {
  double *regrid_res;   // coordinateResolution of the z* coordinate (nk)
  double *regrid_vec;   // the host vectors of the density coordinates (resolution | targets | max depths | max thicknesses)
  double *remap_src;    // the un-remapped velocity of ALE_remap_velocities' KE-conserving correction
  double *remap_hvel;   // h_u, h_v of both grids for mom6x_ALE_remap_velocities_from_h outside OM4's switch set
};
static AleState *ale_state(mom6x_ctx *c) {
  if (!c->ale) c->ale = new AleState();
  return c->ale;
}
