// isopycnal_slopes_dev.h -- what thickness_diffuse.hip and lateral_mixing_coeffs.hip both take from MOM_isopycnal_slopes.F90
// (device code): the column solve of vert_fill_TS and the density gradients at an interface of a face.
#pragma once
#include "mom6x_dev.h"
#include "eos_dev.h"

// The tridiagonal solve of vert_fill_TS (:668-697, kap_dt_x2 > 0) on one column, for the column passes k_td_cols (larger_h_denom:
// h0 = 1e-16*sqrt(0.5*kap_dt_x2)) and k_vm_cols (h0 = h_neglect).  Any layer count >= 2: the solve's c1 goes through a work array.
__device__ __forceinline__ void vert_fill_TS_col(const double *__restrict__ h, const double *__restrict__ T,
                                                 const double *__restrict__ S, double *Tf, double *Sf, double *c1, size_t x,
                                                 size_t slab, int nz, double kap_dt_x2, double h0, double h_neglect) {
  double hk = h[x], hn = h[slab + x];
  double ent = kap_dt_x2 / ((hk + hn) + h0);
  double h_tr = hk + h_neglect;
  double b1 = 1.0 / (h_tr + ent);
  double d1 = b1 * h_tr;
  double Tp = (b1 * h_tr) * T[x], Sp = (b1 * h_tr) * S[x];
  Tf[x] = Tp; Sf[x] = Sp;
  for (int k = 1; k < nz - 1; ++k) {
    const size_t o = (size_t)k * slab + x;
    hk = hn; hn = h[o + slab];
    const double entn = kap_dt_x2 / ((hk + hn) + h0);
    h_tr = hk + h_neglect;
    c1[o] = ent * b1;
    const double t = h_tr + d1 * ent;
    b1 = 1.0 / (t + entn);
    d1 = b1 * t;
    Tp = b1 * (h_tr * T[o] + ent * Tp);
    Sp = b1 * (h_tr * S[o] + ent * Sp);
    Tf[o] = Tp; Sf[o] = Sp;
    ent = entn;
  }
  {
    const size_t o = (size_t)(nz - 1) * slab + x;
    c1[o] = ent * b1;
    h_tr = hn + h_neglect;
    b1 = 1.0 / (h_tr + d1 * ent);
    Tp = b1 * (h_tr * T[o] + ent * Tp);
    Sp = b1 * (h_tr * S[o] + ent * Sp);
    Tf[o] = Tp; Sf[o] = Sp;
  }
  for (int k = nz - 2; k >= 0; --k) {
    const size_t o = (size_t)k * slab + x;
    const double c = c1[o + slab];
    Tp = Tf[o] + c * Tp;
    Sp = Sf[o] + c * Sp;
    Tf[o] = Tp; Sf[o] = Sp;
  }
}

// The density gradients at the interface between layers m (above, "A") and k (below, "B") of the face between cells L and R:
// calc_isoneutral_slopes :271-273, :323-395, which thickness_diffuse_full repeats at MOM_thickness_diffuse.F90:930-1044.  In the
// reference's expression order, parentheses kept.  K: the kernel's scalars (h_neglect, h_neglect2, H_to_Z, Z_to_L, dRho_dT, dRho_dS).
// FORM: the EOS form; 0: layers of constant density -- drdkL, drdkR come in from GV%Rlay, only the weights and drdz are formed.
struct IsoGrad { double drdkL, drdkR, dzaL, dzaR, wtL, wtR, drdz, drdx, mag_grad2; };

template <int FORM, class K>
__device__ __forceinline__ void isoneutral_grads(const K &P, double hLm, double hRm, double hLk, double hRk, double TLm, double TRm,
                                                 double TLk, double TRk, double SLm, double SRm, double SLk, double SRk, double pres_u,
                                                 double eL, double eR, double Igrad, IsoGrad &g) {
  double drdiA = 0.0, drdiB = 0.0;
  if constexpr (FORM != 0) {
    const double T_u = 0.25 * ((TLk + TRk) + (TLm + TRm));
    const double S_u = 0.25 * ((SLk + SRk) + (SLm + SRm));
    double dR_dT, dR_dS;
    eos_density_derivs<FORM>(P, T_u, S_u, pres_u, dR_dT, dR_dS);
    drdiA = dR_dT * (TRm - TLm) + dR_dS * (SRm - SLm);
    drdiB = dR_dT * (TRk - TLk) + dR_dS * (SRk - SLk);
    g.drdkL = (dR_dT * (TLk - TLm) + dR_dS * (SLk - SLm));
    g.drdkR = (dR_dT * (TRk - TRm) + dR_dS * (SRk - SRm));
  }
  const double hg2A = hLm * hRm + P.h_neglect2, hg2B = hLk * hRk + P.h_neglect2;
  const double hg2L = hLm * hLk + P.h_neglect2, hg2R = hRm * hRk + P.h_neglect2;
  const double haA = 0.5 * (hLm + hRm) + P.h_neglect, haB = 0.5 * (hLk + hRk) + P.h_neglect;
  const double haL = 0.5 * (hLm + hLk) + P.h_neglect, haR = 0.5 * (hRm + hRk) + P.h_neglect;
  g.dzaL = haL * P.H_to_Z; g.dzaR = haR * P.H_to_Z;
  const double wtA = hg2A * haB, wtB = hg2B * haA;
  g.wtL = hg2L * (haR * g.dzaR); g.wtR = hg2R * (haL * g.dzaL);
  g.drdz = ((g.wtL * g.drdkL) + (g.wtR * g.drdkR)) / ((g.dzaL * g.wtL) + (g.dzaR * g.wtR));
  g.drdx = 0.0; g.mag_grad2 = 0.0;
  if constexpr (FORM != 0) {
    g.drdx = ((wtA * drdiA + wtB * drdiB) / (wtA + wtB) - g.drdz * (eL - eR)) * Igrad;
    const double zx = P.Z_to_L * g.drdx;
    g.mag_grad2 = zx * zx + g.drdz * g.drdz;
  }
}
