// vert_fill_dev.h -- the tridiagonal solve of vert_fill_TS (MOM_isopycnal_slopes.F90:668-697, kap_dt_x2 > 0) on one column, shared by
// the column passes of thickness_diffuse.hip (larger_h_denom: h0 = 1e-16*sqrt(0.5*kap_dt_x2)) and lateral_mixing_coeffs.hip
// (h0 = h_neglect).  Any layer count >= 2: the solve's c1 goes through a work array.
#pragma once
#include "mom6x_dev.h"

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
