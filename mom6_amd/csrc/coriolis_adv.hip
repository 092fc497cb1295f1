// coriolis_adv.hip -- Coriolis/momentum advection on gfx950.
//
//   CorAdCalc + gradKE        <- MOM_CoriolisAdv.F90:125-1052
//
// Horizontal-stencil kernels are "column-walk" kernels: lane index = i (coalesced), each thread keeps
// the 2-D metric coefficients of its point in registers and walks KCHUNK layers, so the metric planes
// are read nk/KCHUNK times instead of nk times.
#include "mom6x_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------
// CorAdCalc, pass 1: potential vorticity q (and abs_vort) at vertices, kinetic energy at cells.
__global__ void __launch_bounds__(256)
k_corad_q(Dm d, const double *__restrict__ G, const double *__restrict__ u, const double *__restrict__ v,
          const double *__restrict__ h, double *__restrict__ q, double *__restrict__ absv, double *__restrict__ KE,
          int no_slip, int ke_scheme, double vol_neglect, double *__restrict__ Ihq) {
  const int i = I_BASE(-2) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -2 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni || j > d.nj) return;
  if (i < (-2)) return;
  const int st = d.pitch;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int k0 = blockIdx.z * KCHUNK, k1 = min(k0 + KCHUNK, d.nk);
  const double *mT = gm(G, d, MOM6X_G_mask2dT), *areaT = gm(G, d, MOM6X_G_areaT);
  // Area_h :239-241, Area_q :265-268
  const double A00 = mT[x] * areaT[x], A10 = mT[x + 1] * areaT[x + 1];
  const double A01 = mT[x + st] * areaT[x + st], A11 = mT[x + 1 + st] * areaT[x + 1 + st];
  const double Area_q = (A00 + A11) + (A10 + A01);
  const double dyCv0 = gm(G, d, MOM6X_G_dyCv)[x], dyCv1 = gm(G, d, MOM6X_G_dyCv)[x + 1];
  const double dxCu0 = gm(G, d, MOM6X_G_dxCu)[x], dxCu1 = gm(G, d, MOM6X_G_dxCu)[x + st];
  const double mBu = gm(G, d, MOM6X_G_mask2dBu)[x], IareaBu = gm(G, d, MOM6X_G_IareaBu)[x];
  const double fBu = gm(G, d, MOM6X_G_CoriolisBu)[x];
  const double vfac = no_slip ? (2.0 - mBu) : mBu;
  const bool do_KE = (i >= -1 && j >= -1);
  double aCu0 = 0, aCu1 = 0, aCv0 = 0, aCv1 = 0, IareaT = 0;
  if (do_KE) {
    aCu0 = gm(G, d, MOM6X_G_areaCu)[x]; aCu1 = gm(G, d, MOM6X_G_areaCu)[x - 1];
    aCv0 = gm(G, d, MOM6X_G_areaCv)[x]; aCv1 = gm(G, d, MOM6X_G_areaCv)[x - st];
    IareaT = gm(G, d, MOM6X_G_IareaT)[x];
  }
  for (int k = k0; k < k1; k++) {
    const size_t c = x + (size_t)k * slab;
    const double u0 = u[c], v0 = v[c];
    const double dvdx = (v[c + 1] * dyCv1) - (v0 * dyCv0);
    const double dudy = (u[c + st] * dxCu1) - (u0 * dxCu0);
    const double h00 = h[c], h10 = h[c + 1], h01 = h[c + st], h11 = h[c + 1 + st];
    const double hAu0 = 0.5 * ((A00 * h00) + (A10 * h10));      // hArea_u(I,j)
    const double hAu1 = 0.5 * ((A01 * h01) + (A11 * h11));      // hArea_u(I,j+1)
    const double hAv0 = 0.5 * ((A00 * h00) + (A01 * h01));      // hArea_v(i,J)
    const double hAv1 = 0.5 * ((A10 * h10) + (A11 * h11));      // hArea_v(i+1,J)
    const double rel_vort = vfac * (dvdx - dudy) * IareaBu;
    const double abs_vort = fBu + rel_vort;
    const double hArea_q = (hAu0 + hAu1) + (hAv0 + hAv1);
    const double Ih_q = Area_q / (hArea_q + vol_neglect);
    q[c] = abs_vort * Ih_q;
    if (absv) absv[c] = abs_vort;
    if (Ihq) Ihq[c] = Ih_q;   // ARAKAWA_LAMB_BLEND weighs its three schemes by the spread of Ih_q around a cell (:550-573)
    if (do_KE) {
      const double um1 = u[c - 1], vm1 = v[c - st];
      double ke;
      if (ke_scheme == MOM6X_KE_ARAKAWA) {
        ke = (((aCu0 * (u0 * u0)) + (aCu1 * (um1 * um1))) + ((aCv0 * (v0 * v0)) + (aCv1 * (vm1 * vm1)))) * 0.25 * IareaT;
      } else if (ke_scheme == MOM6X_KE_SIMPLE_GUDONOV) {
        const double up = 0.5 * (um1 + fabs(um1)), up2 = up * up;
        const double um = 0.5 * (u0 - fabs(u0)), um2 = um * um;
        const double vp = 0.5 * (vm1 + fabs(vm1)), vp2 = vp * vp;
        const double vm = 0.5 * (v0 - fabs(v0)), vm2 = vm * vm;
        ke = (dmax(up2, um2) + dmax(vp2, vm2)) * 0.5;
      } else {
        const double up = 0.5 * (um1 + fabs(um1)), up2a = up * up * aCu1;
        const double um = 0.5 * (u0 - fabs(u0)), um2a = um * um * aCu0;
        const double vp = 0.5 * (vm1 + fabs(vm1)), vp2a = vp * vp * aCv1;
        const double vm = 0.5 * (v0 - fabs(v0)), vm2a = vm * vm * aCv0;
        ke = (dmax(um2a, up2a) + dmax(vm2a, vp2a)) * 0.5 * IareaT;
      }
      KE[c] = ke;
    }
  }
}

__device__ __forceinline__ double max4(double a, double b, double c, double d) { return dmax(dmax(dmax(a, b), c), d); }
__device__ __forceinline__ double min4(double a, double b, double c, double d) { return dmin(dmin(dmin(a, b), c), d); }

// CorAdCalc, pass 2: the accelerations CAu (I=-1..ni-1, j=0..nj-1) and CAv (i=0..ni-1, J=-1..nj-1).
// One layer of one point, shared by the two-kernel form (q, KE, abs_vort read from HBM: k_corad_acc) and the one-kernel form
// (from the work-group's LDS tile: k_corad_fused) through the accessors Q(di, dj), KEf(di, dj), AVf(di, dj).
struct CoradAcc {
  const double *u, *v, *uh, *vh, *h, *PFu, *PFv, *diffu, *diffv;
  double *CAu, *CAv, *u_bc, *v_bc;
  double IdxCu, IdyCv, Lv[4], Lu[4];
  int scheme, bound, en_dis;
  bool do_u, do_v;
  // ARAKAWA_LAMB_BLEND (:544-548), ROBUST_ENSTRO (:242-243; IdxCv / IdyCu of the four faces in Lv / Lu)
  double Fe_m2, rat_lin, wt_lin, eps_vel, h_tiny;
  int pv_upwind;
};
// The Arakawa & Lamb (1981) weights of one thickness cell from the potential vorticity at its four corners (NE = q(I,J),
// SW = q(I-1,J-1), NW = q(I-1,J), SE = q(I,J-1)): a(I-1,j), d(I-1,j), b(I,j), c(I,j), ep_u(i,j), ep_v(i,j)  :534-542, and their
// ARAKAWA_LAMB_BLEND form :543-588 (ih* = Ih_q at the same corners).
struct ALCell { double a, d, b, c, ep_u, ep_v; };
__device__ __forceinline__ ALCell al_cell(const CoradAcc &X, double qNE, double qSW, double qNW, double qSE, double ihNE,
                                          double ihSW, double ihNW, double ihSE) {
  const double C1_24 = 1.0 / 24.0;
  ALCell r;
  if (X.scheme == MOM6X_ARAKAWA_LAMB81) {
    r.a = (2.0 * (qNE + qSW) + (qNW + qSE)) * C1_24;
    r.d = ((qNE + qSW) + 2.0 * (qNW + qSE)) * C1_24;
    r.b = ((qNE + qSW) + 2.0 * (qNW + qSE)) * C1_24;
    r.c = (2.0 * (qNE + qSW) + (qNW + qSE)) * C1_24;
    r.ep_u = ((qNE - qSW) + (qNW - qSE)) * C1_24;
    r.ep_v = (-(qNE - qSW) + (qNW - qSE)) * C1_24;
  } else {
    const double min_Ihq = dmin(dmin(dmin(ihSW, ihSE), ihNW), ihNE), max_Ihq = dmax(dmax(dmax(ihSW, ihSE), ihNW), ihNE);
    double rat_m1 = 1.0e15, AL_wt, Sad_wt;
    if (max_Ihq < 1.0e15 * min_Ihq) rat_m1 = max_Ihq / min_Ihq - 1.0;
    if (rat_m1 <= X.Fe_m2) AL_wt = 1.0;
    else if (rat_m1 < 1.5 * X.Fe_m2) AL_wt = 3.0 * X.Fe_m2 / rat_m1 - 2.0;
    else AL_wt = 0.0;
    if (rat_m1 <= 1.5 * X.Fe_m2) Sad_wt = 0.0;
    else if (rat_m1 <= X.rat_lin) Sad_wt = 1.0 - (1.5 * X.Fe_m2) / rat_m1;
    else if (rat_m1 < 2.0 * X.rat_lin) Sad_wt = 1.0 - (X.wt_lin / X.rat_lin) * (rat_m1 - 2.0 * X.rat_lin);
    else Sad_wt = 1.0;
    r.a = Sad_wt * 0.25 * qNW + (1.0 - Sad_wt) * (((2.0 - AL_wt) * qNW + AL_wt * qSE) + 2.0 * (qNE + qSW)) * C1_24;
    r.d = Sad_wt * 0.25 * qSW + (1.0 - Sad_wt) * (((2.0 - AL_wt) * qSW + AL_wt * qNE) + 2.0 * (qNW + qSE)) * C1_24;
    r.b = Sad_wt * 0.25 * qNE + (1.0 - Sad_wt) * (((2.0 - AL_wt) * qNE + AL_wt * qSW) + 2.0 * (qNW + qSE)) * C1_24;
    r.c = Sad_wt * 0.25 * qSE + (1.0 - Sad_wt) * (((2.0 - AL_wt) * qSE + AL_wt * qNW) + 2.0 * (qNE + qSW)) * C1_24;
    r.ep_u = AL_wt * ((qNE - qSW) + (qNW - qSE)) * C1_24;
    r.ep_v = AL_wt * (-(qNE - qSW) + (qNW - qSE)) * C1_24;
  }
  return r;
}
// Heff of ROBUST_ENSTRO (:692-703, :813-824): the transport's own thickness, kept between the two cells' thicknesses
__device__ __forceinline__ double robust_heff(double tr, double Idl, double vel, double eps_vel, double hA, double hB) {
  double He = fabs(tr * Idl) / (eps_vel + fabs(vel));
  He = dmax(He, dmin(hA, hB));
  return dmin(He, dmax(hA, hB));
}
struct NoIhq { __device__ double operator()(int, int) const { return 0.0; } };
// ALL: with the three schemes only the two-kernel form runs (ROBUST_ENSTRO, ARAKAWA_LAMB81, ARAKAWA_LAMB_BLEND).  k_corad_fused
// compiles them OUT: merely present, never taken, they cost it 14 spilled registers (3.6 instead of 2.0 ms per call).
// LEAN: the default configuration known at compile time (SADOURNY75_ENERGY without BOUND_CORIOLIS and CORIOLIS_EN_DIS).
template <bool ALL, bool LEAN = false, class QF, class KF, class AF, class IF = NoIhq>
__device__ __forceinline__ void corad_acc_layer(const CoradAcc &X, size_t c, int st, const QF &Q, const KF &KEf, const AF &AVf,
                                                const IF &IH = NoIhq()) {
  const double *__restrict__ u = X.u, *__restrict__ v = X.v, *__restrict__ uh = X.uh, *__restrict__ vh = X.vh, *__restrict__ h = X.h;
  const double *__restrict__ PFu = X.PFu, *__restrict__ PFv = X.PFv, *__restrict__ diffu = X.diffu, *__restrict__ diffv = X.diffv;
  double *__restrict__ CAu = X.CAu, *__restrict__ CAv = X.CAv, *__restrict__ u_bc = X.u_bc, *__restrict__ v_bc = X.v_bc;
  const double IdxCu = X.IdxCu, IdyCv = X.IdyCv;
  const double *Lv = X.Lv, *Lu = X.Lu;
  const int scheme = LEAN ? (int)MOM6X_SADOURNY75_ENERGY : X.scheme, bound = LEAN ? 0 : X.bound, en_dis = LEAN ? 0 : X.en_dis;
  const bool do_u = X.do_u, do_v = X.do_v;
  const double C1_12 = 1.0 / 12.0;
  auto ihq = [&](int di, int dj) { return (scheme == MOM6X_AL_BLEND) ? IH(di, dj) : 0.0; };   // only the blend has (and reads) Ih_q
  // CORIOLIS_EN_DIS (:326-333, :590-635): the centred thickness transport of a face and the one the continuity solver
  // gave bracket the transport used by the energy-dissipating scheme; recomputed here for the four faces each point needs
  auto bracket = [](double Lf, double vel, double hsum, double hm_in, double &mn, double &mx) {
    const double c1 = 1.0 - 1.5 * 0.5, c2 = 1.0 - 0.5, c3 = 2.0, slope = 0.5;
    double uhc = 0.5 * ((Lf * 1.0) * vel) * hsum, uhm = hm_in;
    if (Lf == 0.0) uhc = uhm;
    if (fabs(uhc) < 0.1 * fabs(uhm)) uhm = 10.0 * uhc;
    else if (fabs(uhc) > c1 * fabs(uhm)) {
      if (fabs(uhc) < c2 * fabs(uhm)) uhc = (3.0 * uhc + (1.0 - c2 * 3.0) * uhm);
      else if (fabs(uhc) <= c3 * fabs(uhm)) uhc = uhm;
      else uhc = slope * uhc + (1.0 - c3 * slope) * uhm;
    }
    if (uhc > uhm) { mn = uhm; mx = uhc; } else { mx = uhm; mn = uhc; }
  };
    const double q00 = Q(0, 0);
    if (do_u) {
      const double q0m = Q(0, -1);
      double ca;
      if (scheme == MOM6X_SADOURNY75_ENERGY && en_dis) {   // :665-684
        double mn0, mx0, mn1, mx1, mn2, mx2, mn3, mx3;      // v faces (i,J), (i+1,J), (i,J-1), (i+1,J-1)
        bracket(Lv[0], v[c], h[c] + h[c + st], vh[c], mn0, mx0);
        bracket(Lv[1], v[c + 1], h[c + 1] + h[c + 1 + st], vh[c + 1], mn1, mx1);
        bracket(Lv[2], v[c - st], h[c - st] + h[c], vh[c - st], mn2, mx2);
        bracket(Lv[3], v[c + 1 - st], h[c + 1 - st] + h[c + 1], vh[c + 1 - st], mn3, mx3);
        const double uk = u[c];
        double temp1, temp2;
        if (q00 * uk == 0.0) temp1 = q00 * ((mx0 + mx1) + (mn0 + mn1)) * 0.5;
        else if (q00 * uk < 0.0) temp1 = q00 * (mx0 + mx1);
        else temp1 = q00 * (mn0 + mn1);
        if (q0m * uk == 0.0) temp2 = q0m * ((mx2 + mx3) + (mn2 + mn3)) * 0.5;
        else if (q0m * uk < 0.0) temp2 = q0m * (mx2 + mx3);
        else temp2 = q0m * (mn2 + mn3);
        ca = 0.25 * IdxCu * (temp1 + temp2);
      } else if (scheme == MOM6X_SADOURNY75_ENERGY) {
        ca = 0.25 * ((q00 * (vh[c + 1] + vh[c])) + (q0m * (vh[c - st] + vh[c + 1 - st]))) * IdxCu;
      } else if (scheme == MOM6X_SADOURNY75_ENSTRO) {
        ca = 0.125 * (IdxCu * (q00 + q0m)) * ((vh[c + 1] + vh[c]) + (vh[c - st] + vh[c + 1 - st]));
      } else if (!ALL || scheme == MOM6X_ARAKAWA_HSU90) {   // :523-533, :683-686
        const double a = (q00 + (Q(1, 0) + q0m)) * C1_12;
        const double dd = ((q00 + Q(1, -1)) + q0m) * C1_12;
        const double b = (q00 + (Q(-1, 0) + q0m)) * C1_12;
        const double cc = ((q00 + Q(-1, -1)) + q0m) * C1_12;
        ca = (((a * vh[c + 1]) + (cc * vh[c - st])) + ((b * vh[c]) + (dd * vh[c + 1 - st]))) * IdxCu;
      } else if (scheme == MOM6X_ROBUST_ENSTRO) {   // :687-714; Lv = IdxCv of the v faces (i,J), (i+1,J), (i,J-1), (i+1,J-1)
        const double Heff1 = robust_heff(vh[c], Lv[0], v[c], X.eps_vel, h[c], h[c + st]);
        const double Heff2 = robust_heff(vh[c - st], Lv[2], v[c - st], X.eps_vel, h[c - st], h[c]);
        const double Heff3 = robust_heff(vh[c + 1], Lv[1], v[c + 1], X.eps_vel, h[c + 1], h[c + 1 + st]);
        const double Heff4 = robust_heff(vh[c + 1 - st], Lv[3], v[c + 1 - st], X.eps_vel, h[c + 1 - st], h[c + 1]);
        const double av0 = AVf(0, 0), avm = AVf(0, -1);
        const double VHeff = ((vh[c] + vh[c + 1 - st]) + (vh[c - st] + vh[c + 1]));
        if (X.pv_upwind) {
          const double QVHeff = 0.5 * (((av0 + avm) * VHeff) - ((av0 - avm) * fabs(VHeff)));
          ca = (QVHeff / (X.h_tiny + ((Heff1 + Heff4) + (Heff2 + Heff3)))) * IdxCu;
        } else
          ca = 0.5 * (av0 + avm) * VHeff / (X.h_tiny + ((Heff1 + Heff4) + (Heff2 + Heff3))) * IdxCu;
      } else {   // ARAKAWA_LAMB81 / ARAKAWA_LAMB_BLEND: the cells (i+1,j) and (i,j) either side of the face  :534-588, :683-686, :716-721
        const double q10 = Q(1, 0), q1m = Q(1, -1), qm0 = Q(-1, 0), qmm = Q(-1, -1);
        const ALCell E = al_cell(X, q10, q0m, q00, q1m, ihq(1, 0), ihq(0, -1), ihq(0, 0), ihq(1, -1));
        const ALCell W = al_cell(X, q00, qmm, qm0, q0m, ihq(0, 0), ihq(-1, -1), ihq(-1, 0), ihq(0, -1));
        ca = (((E.a * vh[c + 1]) + (W.c * vh[c - st])) + ((W.b * vh[c]) + (E.d * vh[c + 1 - st]))) * IdxCu;
        ca = ca + ((W.ep_u * uh[c - 1]) - (E.ep_u * uh[c + 1])) * IdxCu;
      }
      if (bound) {   // :734-747
        const double av0 = AVf(0, 0), avm = AVf(0, -1);
        const double fv1 = av0 * v[c + 1], fv2 = av0 * v[c], fv3 = avm * v[c + 1 - st], fv4 = avm * v[c - st];
        ca = dmin(ca, max4(fv1, fv2, fv3, fv4));
        ca = dmax(ca, min4(fv1, fv2, fv3, fv4));
      }
      const double cau = ca - (KEf(1, 0) - KEf(0, 0)) * IdxCu;
      CAu[c] = cau;
      if (u_bc) u_bc[c] = (cau + PFu[c]) + diffu[c];   // u_bc_accel of the RK2 step (:900-907) while CAu is at hand
    }
    if (do_v) {
      const double qm0 = Q(-1, 0);
      double ca;
      if (scheme == MOM6X_SADOURNY75_ENERGY && en_dis) {   // :776-795
        double mn0, mx0, mn1, mx1, mn2, mx2, mn3, mx3;      // u faces (I-1,j), (I-1,j+1), (I,j), (I,j+1)
        bracket(Lu[0], u[c - 1], h[c - 1] + h[c], uh[c - 1], mn0, mx0);
        bracket(Lu[1], u[c - 1 + st], h[c - 1 + st] + h[c + st], uh[c - 1 + st], mn1, mx1);
        bracket(Lu[2], u[c], h[c] + h[c + 1], uh[c], mn2, mx2);
        bracket(Lu[3], u[c + st], h[c + st] + h[c + 1 + st], uh[c + st], mn3, mx3);
        const double vk = v[c];
        double temp1, temp2;
        if (qm0 * vk == 0.0) temp1 = qm0 * ((mx0 + mx1) + (mn0 + mn1)) * 0.5;
        else if (qm0 * vk > 0.0) temp1 = qm0 * (mx0 + mx1);
        else temp1 = qm0 * (mn0 + mn1);
        if (q00 * vk == 0.0) temp2 = q00 * ((mx2 + mx3) + (mn2 + mn3)) * 0.5;
        else if (q00 * vk > 0.0) temp2 = q00 * (mx2 + mx3);
        else temp2 = q00 * (mn2 + mn3);
        ca = -0.25 * IdyCv * (temp1 + temp2);
      } else if (scheme == MOM6X_SADOURNY75_ENERGY) {
        ca = -0.25 * ((qm0 * (uh[c - 1] + uh[c - 1 + st])) + (q00 * (uh[c] + uh[c + st]))) * IdyCv;
      } else if (scheme == MOM6X_SADOURNY75_ENSTRO) {
        ca = -0.125 * (IdyCv * (qm0 + q00)) * ((uh[c - 1] + uh[c - 1 + st]) + (uh[c] + uh[c + st]));
      } else if (!ALL || scheme == MOM6X_ARAKAWA_HSU90) {
        // a(I-1,j), c(I,j+1), b(I,j), d(I-1,j+1)
        const double a_m = (qm0 + (q00 + Q(-1, -1))) * C1_12;
        const double c_p = ((Q(0, 1) + Q(-1, 0)) + q00) * C1_12;
        const double b_0 = (q00 + (qm0 + Q(0, -1))) * C1_12;
        const double d_mp = ((Q(-1, 1) + q00) + qm0) * C1_12;
        ca = -(((a_m * uh[c - 1]) + (c_p * uh[c + st])) + ((b_0 * uh[c]) + (d_mp * uh[c - 1 + st]))) * IdyCv;
      } else if (scheme == MOM6X_ROBUST_ENSTRO) {   // :808-838; Lu = IdyCu of the u faces (I-1,j), (I-1,j+1), (I,j), (I,j+1)
        const double Heff1 = robust_heff(uh[c], Lu[2], u[c], X.eps_vel, h[c], h[c + 1]);
        const double Heff2 = robust_heff(uh[c - 1], Lu[0], u[c - 1], X.eps_vel, h[c - 1], h[c]);
        const double Heff3 = robust_heff(uh[c + st], Lu[3], u[c + st], X.eps_vel, h[c + st], h[c + 1 + st]);
        const double Heff4 = robust_heff(uh[c - 1 + st], Lu[1], u[c - 1 + st], X.eps_vel, h[c - 1 + st], h[c + st]);
        const double av0 = AVf(0, 0), avm = AVf(-1, 0);
        const double UHeff = ((uh[c] + uh[c - 1 + st]) + (uh[c - 1] + uh[c + st]));
        if (X.pv_upwind) {
          const double QUHeff = 0.5 * (((av0 + avm) * UHeff) - ((av0 - avm) * fabs(UHeff)));
          ca = -(QUHeff / (X.h_tiny + ((Heff1 + Heff4) + (Heff2 + Heff3))) * IdyCv);
        } else
          ca = -(0.5 * (av0 + avm) * UHeff / (X.h_tiny + ((Heff1 + Heff4) + (Heff2 + Heff3))) * IdyCv);
      } else {   // ARAKAWA_LAMB81 / ARAKAWA_LAMB_BLEND: the cells (i,j) and (i,j+1) either side of the face  :796-801, :840-845
        const double qmm = Q(-1, -1), q0m = Q(0, -1), q01 = Q(0, 1), qm1 = Q(-1, 1);
        const ALCell S = al_cell(X, q00, qmm, qm0, q0m, ihq(0, 0), ihq(-1, -1), ihq(-1, 0), ihq(0, -1));
        const ALCell N = al_cell(X, q01, qm0, qm1, q00, ihq(0, 1), ihq(-1, 0), ihq(-1, 1), ihq(0, 0));
        ca = -(((S.a * uh[c - 1]) + (N.c * uh[c + st])) + ((S.b * uh[c]) + (N.d * uh[c - 1 + st]))) * IdyCv;
        ca = ca + ((S.ep_v * vh[c - st]) - (N.ep_v * vh[c + st])) * IdyCv;
      }
      if (bound) {
        const double av0 = AVf(0, 0), avm = AVf(-1, 0);
        const double fu1 = -av0 * u[c + st], fu2 = -av0 * u[c], fu3 = -avm * u[c - 1 + st], fu4 = -avm * u[c - 1];
        ca = dmin(ca, max4(fu1, fu2, fu3, fu4));
        ca = dmax(ca, min4(fu1, fu2, fu3, fu4));
      }
      const double cav = ca - (KEf(0, 1) - KEf(0, 0)) * IdyCv;
      CAv[c] = cav;
      if (v_bc) v_bc[c] = (cav + PFv[c]) + diffv[c];
    }
}

__global__ void __launch_bounds__(256)
k_corad_acc(Dm d, const double *__restrict__ G, const double *__restrict__ u, const double *__restrict__ v,
            const double *__restrict__ uh, const double *__restrict__ vh, const double *__restrict__ q,
            const double *__restrict__ absv, const double *__restrict__ KE, double *__restrict__ CAu,
            double *__restrict__ CAv, int scheme, int bound, const double *__restrict__ h, int en_dis,
            const double *__restrict__ PFu, const double *__restrict__ PFv, const double *__restrict__ diffu,
            const double *__restrict__ diffv, double *__restrict__ u_bc, double *__restrict__ v_bc,
            double *__restrict__ uhtr, double *__restrict__ vhtr, double dt_tr, const double *__restrict__ Ihq, CoradAcc X0) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < (-1)) return;
  const int st = d.pitch;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int k0 = blockIdx.z * KCHUNK, k1 = min(k0 + KCHUNK, d.nk);
  CoradAcc X = X0;   // the scheme's constants (Fe_m2, rat_lin, wt_lin, eps_vel, h_tiny, pv_upwind)
  X.u = u; X.v = v; X.uh = uh; X.vh = vh; X.h = h; X.PFu = PFu; X.PFv = PFv; X.diffu = diffu; X.diffv = diffv;
  X.CAu = CAu; X.CAv = CAv; X.u_bc = u_bc; X.v_bc = v_bc; X.scheme = scheme; X.bound = bound; X.en_dis = en_dis;
  X.do_u = (j >= 0); X.do_v = (i >= 0);
  X.IdxCu = gm(G, d, MOM6X_G_IdxCu)[x]; X.IdyCv = gm(G, d, MOM6X_G_IdyCv)[x];
  for (int n = 0; n < 4; n++) { X.Lv[n] = 0.; X.Lu[n] = 0.; }
  if (en_dis) {
    const double *dx_Cv = gm(G, d, MOM6X_G_dx_Cv), *dy_Cu = gm(G, d, MOM6X_G_dy_Cu);
    if (X.do_u) { X.Lv[0] = dx_Cv[x]; X.Lv[1] = dx_Cv[x + 1]; X.Lv[2] = dx_Cv[x - st]; X.Lv[3] = dx_Cv[x + 1 - st]; }
    if (X.do_v) { X.Lu[0] = dy_Cu[x - 1]; X.Lu[1] = dy_Cu[x - 1 + st]; X.Lu[2] = dy_Cu[x]; X.Lu[3] = dy_Cu[x + st]; }
  }
  if (scheme == MOM6X_ROBUST_ENSTRO) {
    const double *IdxCv = gm(G, d, MOM6X_G_IdxCv), *IdyCu = gm(G, d, MOM6X_G_IdyCu);
    if (X.do_u) { X.Lv[0] = IdxCv[x]; X.Lv[1] = IdxCv[x + 1]; X.Lv[2] = IdxCv[x - st]; X.Lv[3] = IdxCv[x + 1 - st]; }
    if (X.do_v) { X.Lu[0] = IdyCu[x - 1]; X.Lu[1] = IdyCu[x - 1 + st]; X.Lu[2] = IdyCu[x]; X.Lu[3] = IdyCu[x + st]; }
  }
  // uhtr = uhtr + uh*dt, vhtr = vhtr + vh*dt (RK2.F90:1072-1079) for the points of this kernel's box (-1..ni-1, -1..nj-1), whose
  // uh(I,j), vh(i,J) it reads anyway; k_uhtr does the ring around the box
  if (uhtr)
    for (int k = k0; k < k1; k++) {
      const size_t c = x + (size_t)k * slab;
      uhtr[c] = uhtr[c] + uh[c] * dt_tr;
      vhtr[c] = vhtr[c] + vh[c] * dt_tr;
    }
  for (int k = k0; k < k1; k++) {
    const size_t c = x + (size_t)k * slab;
    corad_acc_layer<true>(X, c, st, [&](int di, int dj) { return q[c + di + dj * st]; }, [&](int di, int dj) { return KE[c + di + dj * st]; },
                          [&](int di, int dj) { return absv[c + di + dj * st]; }, [&](int di, int dj) { return Ihq[c + di + dj * st]; });
  }
}

// CorAdCalc in ONE kernel: the potential vorticity, the kinetic energy (and abs_vort) of a layer go from the threads that
// computed them to their neighbours through LDS instead of through HBM (2 writes + ~4.6 reads per cell-layer less).  A work-group
// of CF_X x CF_Y = 32 x 16 threads owns a tile of points; every thread evaluates k_corad_q's expressions for its own point,
// the accelerations are evaluated by the tile minus a frame of one point (q is read at -1..+1, KE at 0..+1): 30 x 14 outputs per
// tile.  Two LDS buffers alternate between layers: one barrier per layer.  Same expressions, same bits as k_corad_q + k_corad_acc.
#define CF_X 32
#ifndef CF_Y
#define CF_Y 16
#endif
#ifndef CF_MINW
#define CF_MINW 4
#endif
#define CF_LDW (CF_X + 2)
#define CF_LDN ((CF_Y + 2) * CF_LDW)
template <bool LEAN>
__global__ void __launch_bounds__(CF_X * CF_Y, CF_MINW)   // 4: two work-groups (16 wavefronts) per CU, at most 128 registers
k_corad_fused(Dm d, const double *__restrict__ G, const double *__restrict__ u, const double *__restrict__ v,
              const double *__restrict__ uh, const double *__restrict__ vh, double *__restrict__ CAu,
              double *__restrict__ CAv, int scheme, int bound, const double *__restrict__ h, int en_dis,
              const double *__restrict__ PFu, const double *__restrict__ PFv, const double *__restrict__ diffu,
              const double *__restrict__ diffv, double *__restrict__ u_bc, double *__restrict__ v_bc,
              double *__restrict__ uhtr, double *__restrict__ vhtr, double dt_tr, int no_slip, int ke_scheme, double vol_neglect,
              int kc, int gx, int gy, int gz, int xcd_order) {
  __shared__ double lds[2 * 3 * CF_LDN];
  const int tx = threadIdx.x, ty = threadIdx.y;
  // A 1-D grid of gx * gy * gz work-groups.  The hardware deals consecutive work-groups round-robin to the 8 XCDs (each with its
  // own L2).  A tile row of 32 doubles starts anywhere in a 128-byte line (the tiles advance by 30), so a tile touches the lines of
  // its x neighbours: with the plain order those neighbours sit on other XCDs and the shared lines come from HBM once per tile
  // (measured 18.2 words per cell-layer for ~12 algorithmic).  xcd_order: XCD n walks a CONTIGUOUS run of tiles (x fastest), so
  // the neighbour's lines are L2 hits.
  int b = (int)blockIdx.x;
  const int nb = gx * gy * gz;
  if (xcd_order) {
    const int per = (nb + 7) / 8;
    b = (b % 8) * per + b / 8;
  }
  if (b >= nb) return;   // (the grid is padded to a multiple of 8; the whole work-group leaves)
  const int bxi = b % gx, byi = (b / gx) % gy, bzi = b / (gx * gy);
  const int i = -2 + bxi * (CF_X - 2) + tx;
  const int j = -2 + byi * (CF_Y - 2) + ty;
  const int st = d.pitch;
  const size_t slab = (size_t)d.slab;
  const int k0 = bzi * kc, k1 = min(k0 + kc, d.nk);
  const int l = (ty + 1) * CF_LDW + (tx + 1);
  const bool live = (i <= d.ni) && (j <= d.nj);                 // the range of k_corad_q: (-2..ni, -2..nj)
  const size_t x = live ? ix2(d, i, j) : ix2(d, 0, 0);
  const bool out = live && tx >= 1 && tx <= CF_X - 2 && ty >= 1 && ty <= CF_Y - 2 && i <= d.ni - 1 && j <= d.nj - 1;   // (i, j >= -1)
  // ---- the coefficients of k_corad_q
  const double *mT = gm(G, d, MOM6X_G_mask2dT), *areaT = gm(G, d, MOM6X_G_areaT);
  const double A00 = mT[x] * areaT[x], A10 = mT[x + 1] * areaT[x + 1];
  const double A01 = mT[x + st] * areaT[x + st], A11 = mT[x + 1 + st] * areaT[x + 1 + st];
  const double Area_q = (A00 + A11) + (A10 + A01);
  const double dyCv0 = gm(G, d, MOM6X_G_dyCv)[x], dyCv1 = gm(G, d, MOM6X_G_dyCv)[x + 1];
  const double dxCu0 = gm(G, d, MOM6X_G_dxCu)[x], dxCu1 = gm(G, d, MOM6X_G_dxCu)[x + st];
  const double mBu = gm(G, d, MOM6X_G_mask2dBu)[x], IareaBu = gm(G, d, MOM6X_G_IareaBu)[x];
  const double fBu = gm(G, d, MOM6X_G_CoriolisBu)[x];
  const double vfac = no_slip ? (2.0 - mBu) : mBu;
  const bool do_KE = live && (i >= -1 && j >= -1);
  double aCu0 = 0, aCu1 = 0, aCv0 = 0, aCv1 = 0, IareaT = 0;
  if (do_KE) {
    aCu0 = gm(G, d, MOM6X_G_areaCu)[x]; aCu1 = gm(G, d, MOM6X_G_areaCu)[x - 1];
    aCv0 = gm(G, d, MOM6X_G_areaCv)[x]; aCv1 = gm(G, d, MOM6X_G_areaCv)[x - st];
    IareaT = gm(G, d, MOM6X_G_IareaT)[x];
  }
  // ---- and of k_corad_acc
  CoradAcc X;
  X.u = u; X.v = v; X.uh = uh; X.vh = vh; X.h = h; X.PFu = PFu; X.PFv = PFv; X.diffu = diffu; X.diffv = diffv;
  X.CAu = CAu; X.CAv = CAv; X.u_bc = u_bc; X.v_bc = v_bc; X.scheme = scheme; X.bound = bound; X.en_dis = en_dis;
  X.do_u = out && (j >= 0); X.do_v = out && (i >= 0);
  X.IdxCu = gm(G, d, MOM6X_G_IdxCu)[x]; X.IdyCv = gm(G, d, MOM6X_G_IdyCv)[x];
  for (int n = 0; n < 4; n++) { X.Lv[n] = 0.; X.Lu[n] = 0.; }
  if (!LEAN && en_dis && out) {
    const double *dx_Cv = gm(G, d, MOM6X_G_dx_Cv), *dy_Cu = gm(G, d, MOM6X_G_dy_Cu);
    if (X.do_u) { X.Lv[0] = dx_Cv[x]; X.Lv[1] = dx_Cv[x + 1]; X.Lv[2] = dx_Cv[x - st]; X.Lv[3] = dx_Cv[x + 1 - st]; }
    if (X.do_v) { X.Lu[0] = dy_Cu[x - 1]; X.Lu[1] = dy_Cu[x - 1 + st]; X.Lu[2] = dy_Cu[x]; X.Lu[3] = dy_Cu[x + st]; }
  }
  for (int k = k0; k < k1; k++) {
    const size_t c = x + (size_t)k * slab;
    double *sq = lds + ((k - k0) & 1) * 3 * CF_LDN, *sk = sq + CF_LDN, *sa = sq + 2 * CF_LDN;
    double qv = 0.0, kev = 0.0, av = 0.0;
    if (live) {
      const double u0 = u[c], v0 = v[c];
      const double dvdx = (v[c + 1] * dyCv1) - (v0 * dyCv0);
      const double dudy = (u[c + st] * dxCu1) - (u0 * dxCu0);
      const double h00 = h[c], h10 = h[c + 1], h01 = h[c + st], h11 = h[c + 1 + st];
      const double hAu0 = 0.5 * ((A00 * h00) + (A10 * h10));      // hArea_u(I,j)
      const double hAu1 = 0.5 * ((A01 * h01) + (A11 * h11));      // hArea_u(I,j+1)
      const double hAv0 = 0.5 * ((A00 * h00) + (A01 * h01));      // hArea_v(i,J)
      const double hAv1 = 0.5 * ((A10 * h10) + (A11 * h11));      // hArea_v(i+1,J)
      const double rel_vort = vfac * (dvdx - dudy) * IareaBu;
      const double abs_vort = fBu + rel_vort;
      const double hArea_q = (hAu0 + hAu1) + (hAv0 + hAv1);
      const double Ih_q = Area_q / (hArea_q + vol_neglect);
      qv = abs_vort * Ih_q;
      av = abs_vort;
      if (do_KE) {
        const double um1 = u[c - 1], vm1 = v[c - st];
        if (ke_scheme == MOM6X_KE_ARAKAWA) {
          kev = (((aCu0 * (u0 * u0)) + (aCu1 * (um1 * um1))) + ((aCv0 * (v0 * v0)) + (aCv1 * (vm1 * vm1)))) * 0.25 * IareaT;
        } else if (ke_scheme == MOM6X_KE_SIMPLE_GUDONOV) {
          const double up = 0.5 * (um1 + fabs(um1)), up2 = up * up;
          const double um = 0.5 * (u0 - fabs(u0)), um2 = um * um;
          const double vp = 0.5 * (vm1 + fabs(vm1)), vp2 = vp * vp;
          const double vm = 0.5 * (v0 - fabs(v0)), vm2 = vm * vm;
          kev = (dmax(up2, um2) + dmax(vp2, vm2)) * 0.5;
        } else {
          const double up = 0.5 * (um1 + fabs(um1)), up2a = up * up * aCu1;
          const double um = 0.5 * (u0 - fabs(u0)), um2a = um * um * aCu0;
          const double vp = 0.5 * (vm1 + fabs(vm1)), vp2a = vp * vp * aCv1;
          const double vm = 0.5 * (v0 - fabs(v0)), vm2a = vm * vm * aCv0;
          kev = (dmax(um2a, up2a) + dmax(vm2a, vp2a)) * 0.5 * IareaT;
        }
      }
    }
    sq[l] = qv; sk[l] = kev; if (!LEAN && bound) sa[l] = av;
    __syncthreads();
    if (out) {
      if (uhtr) {   // :1072-1079 for the box (-1..ni-1, -1..nj-1): see k_corad_acc
        uhtr[c] = uhtr[c] + uh[c] * dt_tr;
        vhtr[c] = vhtr[c] + vh[c] * dt_tr;
      }
      corad_acc_layer<false, LEAN>(X, c, st, [&](int di, int dj) { return sq[l + di + dj * CF_LDW]; }, [&](int di, int dj) { return sk[l + di + dj * CF_LDW]; },
                             [&](int di, int dj) { return sa[l + di + dj * CF_LDW]; });
    }
    // (the layer after next writes this buffer again: the barrier of the next layer lies in between)
  }
}

// k_corad_fused<LEAN> with its INPUTS through LDS too (the default configuration only: SADOURNY75_ENERGY, no bound, no EN_DIS).
// k_corad_fused's threads each ask the vector memory unit for 22 values per layer, 9 of them their own point's (u, v, h, uh, vh and
// the four arrays of the folded u_bc_accel) and 13 a neighbour's, which a neighbouring thread asks for as well: at 8 wavefronts of
// 22 loads per layer and tile the L1's 64 bytes per clock are busy for 1.3 ms of the kernel's 2.8, and every load is used at once.
// Here a thread loads its own point's five values one layer AHEAD into registers (the next layer's requests are in flight during
// the whole of this one), hands them to the tile through LDS, and the neighbours' values are LDS reads; the tile's inputs one point
// beyond its last column / row (q needs them) are loaded the same way by designated threads.  Two barriers per layer: inputs ->
// q, KE -> accelerations; the input planes alternate between layers (the accelerations still read uh, vh when a fast wavefront
// writes the next layer's), q and KE need one buffer.  Same expressions, same bits.
__global__ void __launch_bounds__(CF_X * CF_Y, 4)
k_corad_lds(Dm d, const double *__restrict__ G, const double *__restrict__ u, const double *__restrict__ v,
            const double *__restrict__ uh, const double *__restrict__ vh, double *__restrict__ CAu, double *__restrict__ CAv,
            const double *__restrict__ h, const double *__restrict__ PFu, const double *__restrict__ PFv,
            const double *__restrict__ diffu, const double *__restrict__ diffv, double *__restrict__ u_bc, double *__restrict__ v_bc,
            double *__restrict__ uhtr, double *__restrict__ vhtr, double dt_tr, int no_slip, int ke_scheme, double vol_neglect,
            int kc, int gx, int gy, int gz, int xcd_order) {
  __shared__ double lds[12 * CF_LDN];
  const int tx = threadIdx.x, ty = threadIdx.y;
  int b = (int)blockIdx.x;
  const int nb = gx * gy * gz;
  if (xcd_order) {
    const int per = (nb + 7) / 8;
    b = (b % 8) * per + b / 8;
  }
  if (b >= nb) return;
  const int bxi = b % gx, byi = (b / gx) % gy, bzi = b / (gx * gy);
  const int i = -2 + bxi * (CF_X - 2) + tx;
  const int j = -2 + byi * (CF_Y - 2) + ty;
  const int st = d.pitch;
  const size_t slab = (size_t)d.slab;
  const int k0 = bzi * kc, k1 = min(k0 + kc, d.nk);
  const int l = (ty + 1) * CF_LDW + (tx + 1);
  const bool live = (i <= d.ni) && (j <= d.nj);                 // the range of k_corad_q: (-2..ni, -2..nj)
  const bool inb = (i <= d.ni + 1) && (j <= d.nj + 1);          // the points a live thread reads (halo >= 3: inside the arrays)
  const size_t x = inb ? ix2(d, i, j) : ix2(d, 0, 0);
  const bool out = live && tx >= 1 && tx <= CF_X - 2 && ty >= 1 && ty <= CF_Y - 2 && i <= d.ni - 1 && j <= d.nj - 1;   // (i, j >= -1)
  // the tile's inputs one point beyond its last column and row: (kind 1) v, h east of column CF_X-1, (2) u, h north of row
  // CF_Y-1, (3) h at the corner
  int eKind = 0, eL = 0, ei = 0, ej = 0;
  if (tx == CF_X - 1) { eKind = 1; ei = i + 1; ej = j; eL = (ty + 1) * CF_LDW + CF_X + 1; }
  else if (ty == CF_Y - 1) { eKind = 2; ei = i; ej = j + 1; eL = (CF_Y + 1) * CF_LDW + tx + 1; }
  else if (tx == 0 && ty == 0) { eKind = 2; ei = i + CF_X - 1; ej = j + CF_Y; eL = (CF_Y + 1) * CF_LDW + CF_X; }
  else if (tx == 1 && ty == 0) { eKind = 3; ei = i - 1 + CF_X; ej = j + CF_Y; eL = (CF_Y + 1) * CF_LDW + CF_X + 1; }
  if (ei > d.ni + 1 || ej > d.nj + 1) eKind = 0;
  const size_t xe = eKind ? ix2(d, ei, ej) : x;
  const double *eA = (eKind == 1) ? v : ((eKind == 2) ? u : h);
  // ---- the coefficients of k_corad_q
  const double *mT = gm(G, d, MOM6X_G_mask2dT), *areaT = gm(G, d, MOM6X_G_areaT);
  const size_t xq = live ? x : ix2(d, 0, 0);
  const double A00 = mT[xq] * areaT[xq], A10 = mT[xq + 1] * areaT[xq + 1];
  const double A01 = mT[xq + st] * areaT[xq + st], A11 = mT[xq + 1 + st] * areaT[xq + 1 + st];
  const double Area_q = (A00 + A11) + (A10 + A01);
  const double dyCv0 = gm(G, d, MOM6X_G_dyCv)[xq], dyCv1 = gm(G, d, MOM6X_G_dyCv)[xq + 1];
  const double dxCu0 = gm(G, d, MOM6X_G_dxCu)[xq], dxCu1 = gm(G, d, MOM6X_G_dxCu)[xq + st];
  const double mBu = gm(G, d, MOM6X_G_mask2dBu)[xq], IareaBu = gm(G, d, MOM6X_G_IareaBu)[xq];
  const double fBu = gm(G, d, MOM6X_G_CoriolisBu)[xq];
  const double vfac = no_slip ? (2.0 - mBu) : mBu;
  const bool do_KE = live && (i >= -1 && j >= -1) && tx >= 1 && ty >= 1;   // (the accelerations read KE of threads 1.. only)
  double aCu0 = 0, aCu1 = 0, aCv0 = 0, aCv1 = 0, IareaT = 0;
  if (do_KE) {
    aCu0 = gm(G, d, MOM6X_G_areaCu)[xq]; aCu1 = gm(G, d, MOM6X_G_areaCu)[xq - 1];
    aCv0 = gm(G, d, MOM6X_G_areaCv)[xq]; aCv1 = gm(G, d, MOM6X_G_areaCv)[xq - st];
    IareaT = gm(G, d, MOM6X_G_IareaT)[xq];
  }
  const bool do_u = out && (j >= 0), do_v = out && (i >= 0);
  const double IdxCu = gm(G, d, MOM6X_G_IdxCu)[xq], IdyCv = gm(G, d, MOM6X_G_IdyCv)[xq];
  double *sq = lds + 10 * CF_LDN, *sk = sq + CF_LDN;
  // the first layer's values
  double r_u = 0., r_v = 0., r_h = 0., r_uh = 0., r_vh = 0., r_eA = 0., r_eB = 0.;
  {
    const size_t c = x + (size_t)k0 * slab, ce = xe + (size_t)k0 * slab;
    if (inb) { r_u = u[c]; r_v = v[c]; r_h = h[c]; r_uh = uh[c]; r_vh = vh[c]; }
    if (eKind) { r_eA = eA[ce]; if (eKind != 3) r_eB = h[ce]; }
  }
  for (int k = k0; k < k1; k++) {
    const size_t c = x + (size_t)k * slab;
    double *su = lds + ((k - k0) & 1) * 5 * CF_LDN, *sv = su + CF_LDN, *sh = su + 2 * CF_LDN, *suh = su + 3 * CF_LDN, *svh = su + 4 * CF_LDN;
    su[l] = r_u; sv[l] = r_v; sh[l] = r_h; suh[l] = r_uh; svh[l] = r_vh;
    if (eKind == 1) { sv[eL] = r_eA; sh[eL] = r_eB; }
    else if (eKind == 2) { su[eL] = r_eA; sh[eL] = r_eB; }
    else if (eKind == 3) sh[eL] = r_eA;
    if (k + 1 < k1) {          // the next layer's requests leave before this layer's work
      const size_t cn = c + slab, ce = xe + (size_t)(k + 1) * slab;
      if (inb) { r_u = u[cn]; r_v = v[cn]; r_h = h[cn]; r_uh = uh[cn]; r_vh = vh[cn]; }
      if (eKind) { r_eA = eA[ce]; if (eKind != 3) r_eB = h[ce]; }
    }
    __syncthreads();
    double qv = 0.0, kev = 0.0;
    if (live) {
      const double u0 = su[l], v0 = sv[l];
      const double dvdx = (sv[l + 1] * dyCv1) - (v0 * dyCv0);
      const double dudy = (su[l + CF_LDW] * dxCu1) - (u0 * dxCu0);
      const double h00 = sh[l], h10 = sh[l + 1], h01 = sh[l + CF_LDW], h11 = sh[l + 1 + CF_LDW];
      const double hAu0 = 0.5 * ((A00 * h00) + (A10 * h10));      // hArea_u(I,j)
      const double hAu1 = 0.5 * ((A01 * h01) + (A11 * h11));      // hArea_u(I,j+1)
      const double hAv0 = 0.5 * ((A00 * h00) + (A01 * h01));      // hArea_v(i,J)
      const double hAv1 = 0.5 * ((A10 * h10) + (A11 * h11));      // hArea_v(i+1,J)
      const double rel_vort = vfac * (dvdx - dudy) * IareaBu;
      const double abs_vort = fBu + rel_vort;
      const double hArea_q = (hAu0 + hAu1) + (hAv0 + hAv1);
      const double Ih_q = Area_q / (hArea_q + vol_neglect);
      qv = abs_vort * Ih_q;
      if (do_KE) {
        const double um1 = su[l - 1], vm1 = sv[l - CF_LDW];
        if (ke_scheme == MOM6X_KE_ARAKAWA) {
          kev = (((aCu0 * (u0 * u0)) + (aCu1 * (um1 * um1))) + ((aCv0 * (v0 * v0)) + (aCv1 * (vm1 * vm1)))) * 0.25 * IareaT;
        } else if (ke_scheme == MOM6X_KE_SIMPLE_GUDONOV) {
          const double up = 0.5 * (um1 + fabs(um1)), up2 = up * up;
          const double um = 0.5 * (u0 - fabs(u0)), um2 = um * um;
          const double vp = 0.5 * (vm1 + fabs(vm1)), vp2 = vp * vp;
          const double vm = 0.5 * (v0 - fabs(v0)), vm2 = vm * vm;
          kev = (dmax(up2, um2) + dmax(vp2, vm2)) * 0.5;
        } else {
          const double up = 0.5 * (um1 + fabs(um1)), up2a = up * up * aCu1;
          const double um = 0.5 * (u0 - fabs(u0)), um2a = um * um * aCu0;
          const double vp = 0.5 * (vm1 + fabs(vm1)), vp2a = vp * vp * aCv1;
          const double vm = 0.5 * (v0 - fabs(v0)), vm2a = vm * vm * aCv0;
          kev = (dmax(um2a, up2a) + dmax(vm2a, vp2a)) * 0.5 * IareaT;
        }
      }
    }
    sq[l] = qv; sk[l] = kev;
    __syncthreads();
    if (out) {
      if (uhtr) {   // :1072-1079 for the box (-1..ni-1, -1..nj-1): see k_corad_acc
        uhtr[c] = uhtr[c] + suh[l] * dt_tr;
        vhtr[c] = vhtr[c] + svh[l] * dt_tr;
      }
      const double q00 = sq[l];
      if (do_u) {   // :646-650, :723-731 (SADOURNY75_ENERGY)
        const double q0m = sq[l - CF_LDW];
        const double ca = 0.25 * ((q00 * (svh[l + 1] + svh[l])) + (q0m * (svh[l - CF_LDW] + svh[l + 1 - CF_LDW]))) * IdxCu;
        const double cau = ca - (sk[l + 1] - sk[l]) * IdxCu;
        CAu[c] = cau;
        if (u_bc) u_bc[c] = (cau + PFu[c]) + diffu[c];
      }
      if (do_v) {   // :757-761, :847-855
        const double qm0 = sq[l - 1];
        const double ca = -0.25 * ((qm0 * (suh[l - 1] + suh[l - 1 + CF_LDW])) + (q00 * (suh[l] + suh[l + CF_LDW]))) * IdyCv;
        const double cav = ca - (sk[l + CF_LDW] - sk[l]) * IdyCv;
        CAv[c] = cav;
        if (v_bc) v_bc[c] = (cav + PFv[c]) + diffv[c];
      }
    }
  }
}

}  // namespace

// the points by which the tiles of k_corad_lds / k_corad_fused advance (mom6x_tile_steps, ctx.hip)
void corad_tile_steps(int *sx, int *sy) { *sx = CF_X - 2; *sy = CF_Y - 2; }

// ---------------------------------------------------------------------------------------------
struct CorState { mom6x_coriolis_params P; };   // CoriolisAdv_CS, with the overrides of CoriolisAdv_init applied

extern "C" int mom6x_CoriolisAdv_init(mom6x_ctx *c, const mom6x_coriolis_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_CoriolisAdv_init: null argument");
  REQUIRE(p->Coriolis_Scheme >= MOM6X_SADOURNY75_ENERGY && p->Coriolis_Scheme <= MOM6X_AL_BLEND, MOM6X_EINVAL,
          "CoriolisAdv_init: Unrecognized setting of CORIOLIS_SCHEME");
  REQUIRE(p->KE_Scheme >= MOM6X_KE_ARAKAWA && p->KE_Scheme <= MOM6X_KE_GUDONOV, MOM6X_EINVAL, "CoriolisAdv: bad KE_SCHEME");
  REQUIRE(p->PV_Adv_Scheme == 0 || p->PV_Adv_Scheme == MOM6X_PV_ADV_CENTERED || p->PV_Adv_Scheme == MOM6X_PV_ADV_UPWIND1, MOM6X_EINVAL,
          "CoriolisAdv_init: PV_ADV_SCHEME is invalid");
  if (!c->cor) c->cor = new CorState();
  mom6x_coriolis_params &P = c->cor->P;
  P = *p;
  if (P.Coriolis_Scheme == MOM6X_ROBUST_ENSTRO) { P.Coriolis_En_Dis = 0; P.bound_Coriolis = 0; }   // :1118, :1158
  // CoriolisAdv_init :1158: with CORIOLIS_EN_DIS and SADOURNY75_ENERGY the bound is always effectively off
  if (P.Coriolis_En_Dis && P.Coriolis_Scheme == MOM6X_SADOURNY75_ENERGY) P.bound_Coriolis = 0;
  return MOM6X_OK;
}

void CoriolisAdv_free(mom6x_ctx *c) { delete c->cor; c->cor = nullptr; }
bool CoriolisAdv_ready(const mom6x_ctx *c) { return c->cor != nullptr; }

extern "C" int mom6x_CorAdCalc(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *uh,
                               const double *vh, double *CAu, double *CAv) {
  return CorAdCalc_bc(c, u, v, h, uh, vh, CAu, CAv, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0);
}

// CorAdCalc, and -- for the RK2 step -- u_bc_accel = (CAu + PFu) + diffu (:900-907) formed where CAu is made
int CorAdCalc_bc(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *uh, const double *vh, double *CAu,
                 double *CAv, const double *PFu, const double *PFv, const double *diffu, const double *diffv, double *u_bc,
                 double *v_bc, double *uhtr, double *vhtr, double dt_tr) {
  REQUIRE(c && c->cor, MOM6X_EINVAL, "MOM_CoriolisAdv: Module must be initialized before it is used.");
  REQUIRE(u && v && h && uh && vh && CAu && CAv, MOM6X_EINVAL, "CorAdCalc: null array");
  REQUIRE(c->dims.halo >= 3, MOM6X_EINVAL, "CorAdCalc: halo >= 3 required");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_coriolis_params &P = c->cor->P;
  double *q, *KE, *absv = nullptr;
  int rc;
  if ((rc = ctx_scratch(c, SCR_q, d.nk, &q))) return rc;
  if ((rc = ctx_scratch(c, SCR_KE, d.nk, &KE))) return rc;
  const int scheme = P.Coriolis_Scheme;
  // the schemes of the default k_corad_fused; ROBUST_ENSTRO, ARAKAWA_LAMB81 and ARAKAWA_LAMB_BLEND take the two-kernel form
  const bool fusable = (scheme == MOM6X_SADOURNY75_ENERGY || scheme == MOM6X_SADOURNY75_ENSTRO || scheme == MOM6X_ARAKAWA_HSU90);
  if ((P.bound_Coriolis || scheme == MOM6X_ROBUST_ENSTRO) && (rc = ctx_scratch(c, SCR_absv, d.nk, &absv))) return rc;
  double *Ihq = nullptr;
  if (scheme == MOM6X_AL_BLEND && (rc = ctx_scratch(c, SCR_t0, d.nk, &Ihq))) return rc;
  CoradAcc X0 = {};
  X0.Fe_m2 = P.F_eff_max_blend - 2.0;                                            // :544-548
  X0.wt_lin = P.wt_lin_blend < 1e-16 ? 1e-16 : (P.wt_lin_blend > 1.0 ? 1.0 : P.wt_lin_blend);   // :1139
  X0.rat_lin = 1.5 * X0.Fe_m2 / (X0.wt_lin > 1.0e-16 ? X0.wt_lin : 1.0e-16);
  if (P.F_eff_max_blend <= 2.0) { X0.Fe_m2 = -1.; X0.rat_lin = -1.0; }
  X0.eps_vel = 1.0e-10 * 1.0; X0.h_tiny = c->GV.Angstrom_H;                              // :242-243
  X0.pv_upwind = (P.PV_Adv_Scheme == MOM6X_PV_ADV_UPWIND1);
  const dim3 b = blk2();
  const double vol_neglect = c->GV.H_subroundoff * ((1e-4 * 1.0) * (1e-4 * 1.0));
  // (A barrier-free form -- every thread evaluating q at its own vertex and the one to the south, the western one by a lane
  //  shuffle -- was measured too: 200 registers, 7.1 ms per step against 5.9 for k_corad_fused and 6.5 for the two kernels.)
  static const bool two_kernels = [] { const char *e = getenv("MOM6X_CORAD"); return e && !strcmp(e, "legacy"); }();
  if (!two_kernels && fusable && d.halo >= 3) {   // q, KE, abs_vort through LDS (k_corad_fused); MOM6X_CORAD=legacy: through HBM
    const int kc = (d.nk % 25 == 0) ? 25 : ((d.nk >= KCHUNK) ? KCHUNK : d.nk);
    const dim3 bt(CF_X, CF_Y, 1);
    const int gx = (d.ni + 1 + (CF_X - 2) - 1) / (CF_X - 2), gy = (d.nj + 1 + (CF_Y - 2) - 1) / (CF_Y - 2), gz = (d.nk + kc - 1) / kc;
    constexpr int xcd_order = 1;   // (the launch-order walk of the tiles lost in round 4 and is gone: profiles/README.md)
    const dim3 gt((unsigned)(((gx * gy * gz + 7) / 8) * 8), 1, 1);
    // the default configuration has its own kernel (inputs, q and KE through LDS); every other one the generic k_corad_fused
    const bool lean = (scheme == MOM6X_SADOURNY75_ENERGY) && !P.bound_Coriolis && !P.Coriolis_En_Dis;
    if (lean)
      KLAUNCH(c, "k_corad_lds", k_corad_lds, gt, bt, d, c->G, u, v, uh, vh, CAu, CAv, h, PFu, PFv, diffu, diffv, u_bc, v_bc, uhtr, vhtr, dt_tr,
              P.no_slip, P.KE_Scheme, vol_neglect, kc, gx, gy, gz, xcd_order);
    else
      KLAUNCH(c, "k_corad_fused", k_corad_fused<false>, gt, bt, d, c->G, u, v, uh, vh, CAu, CAv, P.Coriolis_Scheme, P.bound_Coriolis, h,
              P.Coriolis_En_Dis, PFu, PFv, diffu, diffv, u_bc, v_bc, uhtr, vhtr, dt_tr, P.no_slip, P.KE_Scheme, vol_neglect, kc, gx, gy, gz,
              xcd_order);
    HIPCHK(hipGetLastError());
    return MOM6X_OK;
  }
  KLAUNCH(c, "k_corad_q", k_corad_q, gridk(nxa(d.ni + 3, -2), d.nj + 3, d.nk, b), b, d, c->G, u, v, h, q, absv, KE,
          P.no_slip, P.KE_Scheme, vol_neglect, Ihq);
  KLAUNCH(c, "k_corad_acc", k_corad_acc, gridk(nxa(d.ni + 1, -1), d.nj + 1, d.nk, b), b, d, c->G, u, v, uh, vh, q, absv, KE,
          CAu, CAv, P.Coriolis_Scheme, P.bound_Coriolis, h, P.Coriolis_En_Dis, PFu, PFv, diffu, diffv, u_bc, v_bc,
          uhtr, vhtr, dt_tr, (const double *)Ihq, X0);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
