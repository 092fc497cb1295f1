// energetic_PBL.hip -- the ePBL surface boundary layer scheme of MOM_energetic_PBL on gfx950: the diffusivity Kd_ePBL that the
// turbulent kinetic energy of wind and convection can support, with the depth of active mixing.
//
//   energetic_PBL      <- src/parameterizations/vertical/MOM_energetic_PBL.F90:326-884, Boussinesq, fluxes%ustar, no BBL mixing
//   ePBL_column        <- :890-1950 without Langmuir turbulence, equation discovery, the direct calculation and stochastics
//   find_mstar         <- :3519-3613    find_PE_chg_orig <- :3365-3516    find_PE_chg <- :3072-3213
//   cuberoot           <- src/framework/MOM_intrinsic_functions.F90:48-114 (dev_cuberoot, mom6x_dev.h)
//   thickness_to_dz    <- the Boussinesq arm: dz = GV%H_to_Z * h
//   find_uv_at_h       <- MOM_diabatic_aux.F90:546-571, :606-611, the arm without vertical mixing (with MKE_to_TKE_effic > 0 only)
//   the driver's loop  <- MOM_diabatic_driver.F90:1570-1581 (k_epbl_augment), energetic_PBL_get_MLD :3707 (k_epbl_scale)
//
// k_epbl_cols<ORIG, DIAG, MKE>: one lane per column of the computational domain, consecutive lanes along i; templated on what is
// uniform for a run (orig_PE_calc, TKE_diagnostics, MKE conversion).  The downward walk :1345-1865 is a recurrence: interface K
// needs layers k, k-1, k-2 and a dozen running scalars, which live in registers (hp_a, the four dX_to_dY_a, dTe | Te, dSe | Se of
// the layer above, Kddt_h(K-1), pres_Z, htot, dztot, uhtot, vhtot, mech_TKE, conv_PErel, sfc_connected, MLD_output); dT_to_dPE,
// dT_to_dColHt, MixLen_shape and pres_Z are formed on the fly in the reference's order.  There are no per-column arrays.  hb_hs is
// a bottom-up sum (:1206-1211): one pre-pass writes it to the module's work array.  Every iteration of the mixed-layer depth walks
// the column again from memory and overwrites Kd, mixvel and mixlen in place; the walk never stops early (:1452).  A lane that has
// converged idles until the slowest lane of its wavefront has.
//
// Integer powers are products: x**2 = x*x, x**3 = (x*x)*x, UStar**5 = ((u*u)*(u*u))*u.  MAX and MIN are fmax1 and fmin1; where the
// result can be a zero whose sign matters (:1317, :3568, :3596 and the driver's max(Kd_ePBL - Kd_shear, 0.)) the zero is the run-time
// value K.zero: against a literal 0.0 the compiler emits v_max_f64 / v_min_f64, which return the other signed zero.
#include "mom6x_dev.h"

namespace {

struct EpK {
  double dt, I_dtdiag, Rho0, H_to_Z, Z_to_H, H_to_RZ, H_sub, dZ_sub, g_Z, SpV_dt, zero;
  double omega, omega_frac, Ekman, vonKar, MKE_eff, TKE_decay, fixed_mstar, mstar_cap, mstar_coef, C_Ek, cn1, cn2, cn3, cs1, cs2;
  double nstar, conv_coef, transLay, MLD_tol, min_mix_len, MixLenExp, wstar, vfac, vsurf, ustar_min, m_to_Z, T_to_s, vus;
  int old2019, old2024, mstar_scheme, use_iter, guess, bisect, bug, max_its, wT, shape_one;
};
struct EpP {
  const double *h, *u, *v, *T, *S, *dSV_dT, *dSV_dS, *TKE, *ustar, *bflux;
  double *Kd, *MLD, *hb_hs, *dwork, *mixvel, *mixlen;   // hb_hs (nk + 1 levels), dwork (7 planes, with TKE_diagnostics): the module's work arrays
  double *mstar, *ustar_d, *its;
};
// the seven diag_TKE_* planes, filled from dwork by k_epbl_diag_out
struct EpD { double *p[7]; };

// find_mstar :3519-3613, the surface scheme without Langmuir turbulence
__device__ __forceinline__ double ep_find_mstar(const EpK &K, double B, double UStar, double BLD, double absf) {
  const double u2 = UStar * UStar, u3 = u2 * UStar;
  double mstar;
  if (K.mstar_scheme == MOM6X_EPBL_MSTAR_CONSTANT) {
    mstar = K.fixed_mstar;
  } else if (K.mstar_scheme == MOM6X_EPBL_MSTAR_OM4) {
    double mstar_S, mstar_N;
    if (K.old2019) {
      mstar_S = K.mstar_coef * sqrt(fmax1(K.zero, B) / u2 / (absf + 1.e-10 * K.T_to_s));
      mstar_N = K.C_Ek * log(fmax1(1., UStar / (absf + 1.e-10 * K.T_to_s) / BLD));
    } else {
      mstar_S = K.mstar_coef * sqrt(fmax1(K.zero, B) / (u2 * fmax1(absf, 1.e-20 * K.T_to_s)));
      mstar_N = 0.0;
      if (UStar > absf * BLD) mstar_N = K.C_Ek * log(UStar / (absf * BLD));
    }
    mstar = fmax1(mstar_S, fmin1(1.25, mstar_N));
    if (K.mstar_cap > 0.0) mstar = fmin1(K.mstar_cap, mstar);
  } else {
    double mstar_N;
    if (K.old2019) {
      mstar_N = K.cn1 * (1.0 - 1.0 / (1. + K.cn2 * exp(K.cn3 * BLD * absf / UStar)));
    } else {
      const double MSN_term = K.cn2 * exp(K.cn3 * BLD * absf / UStar);
      mstar_N = (K.cn1 * MSN_term) / (1. + MSN_term);
    }
    const double mb = fmax1(K.zero, B);
    const double u5 = (u2 * u2) * UStar;
    const double mstar_S = K.cs1 * pow((mb * mb) * BLD / (u5 * fmax1(absf, 1.e-20 * K.T_to_s)), K.cs2);
    mstar = mstar_N + mstar_S;
  }
  double mstar_Conv_Red;
  if (K.old2019) {
    const double eps = 1.e-10 * ((K.T_to_s * K.T_to_s) * K.T_to_s) * (K.m_to_Z * K.m_to_Z);
    const double mB = -fmin1(K.zero, B);
    mstar_Conv_Red = 1. - K.conv_coef * (mB + eps) / ((mB + eps) + 2.0 * mstar * u3 / BLD);
  } else {
    const double MSCR_term1 = -(BLD * fmin1(K.zero, B));
    const double MSCR_term2 = 2.0 * mstar * u3;
    if (fabs(MSCR_term2) > 0.0) mstar_Conv_Red = ((1. - K.conv_coef) * MSCR_term1 + MSCR_term2) / (MSCR_term1 + MSCR_term2);
    else mstar_Conv_Red = 1. - K.conv_coef;
  }
  return mstar * mstar_Conv_Red;
}

// :1525-1541 and its twin :1600-1616
__device__ __forceinline__ double ep_vstar(const EpK &K, double TKE_here, double conv_PErel, double dztot, double MLD_guess, double u_star) {
  if (K.old2024) {
    if (K.wT == MOM6X_EPBL_WT_CUBE_ROOT_TKE) return K.vfac * K.vus * pow(K.SpV_dt * TKE_here, 1.0 / 3.0);
    const double Surface_Scale = fmax1(0.05, 1.0 - dztot / MLD_guess);
    return K.vfac * Surface_Scale * (K.vsurf * u_star + K.vus * pow(K.wstar * conv_PErel * K.SpV_dt, 1.0 / 3.0));
  }
  if (K.wT == MOM6X_EPBL_WT_CUBE_ROOT_TKE) return K.vfac * dev_cuberoot(K.SpV_dt * TKE_here);
  const double Surface_Scale = fmax1(0.05, 1.0 - dztot / MLD_guess);
  return (K.vfac * Surface_Scale) * (K.vsurf * u_star + dev_cuberoot((K.wstar * conv_PErel) * K.SpV_dt));
}

// find_PE_chg_orig :3365-3516 (ORIG; q1..q4 = dTe_term, dSe_term, dT_km1_t2, dS_km1_t2) or find_PE_chg :3072-3213 with Kddt_h0 = 0
// (q1..q4 = Th_a, Sh_a, Th_b, Sh_b).  DER: dPEc_dKd; LIM: dPE_max and dPEc_dKd_0.  hk: h(k) | hp_b; ha: hp_a(k-1) | b_den_1;
// Pk, Sk: dT_to_dPE(k), dS_to_dPE(k); Pa, Sa: dT_to_dPE_a(k-1), dS_to_dPE_a(k-1); Ck, Dk, Ca, Da: the dX_to_dColHt likewise
template <bool ORIG, bool DER, bool LIM>
__device__ __forceinline__ void ep_PE_chg(double Kddt_h, double hk, double ha, double q1, double q2, double q3, double q4, double Pk,
                                          double Sk, double Pa, double Sa, double pres_Z, double Ck, double Dk, double Ca, double Da,
                                          double &PE_chg, double &dPEc_dKd, double &dPE_max, double &dPEc_dKd_0) {
  if constexpr (ORIG) {
    const double b1 = 1.0 / (ha + Kddt_h);
    const double b1Kd = Kddt_h * b1;
    const double I_Kr_denom = 1.0 / (hk * ha + (ha + hk) * Kddt_h);
    const double dT_k = (Kddt_h * I_Kr_denom) * q1;
    const double dS_k = (Kddt_h * I_Kr_denom) * q2;
    const double dT_km1 = b1Kd * (dT_k + q3);
    const double dS_km1 = b1Kd * (dS_k + q4);
    PE_chg = (Pk * dT_k + Pa * dT_km1) + (Sk * dS_k + Sa * dS_km1);
    const double ColHt_chg = (Ck * dT_k + Ca * dT_km1) + (Dk * dS_k + Da * dS_km1);
    if (ColHt_chg < 0.0) PE_chg = PE_chg - pres_Z * ColHt_chg;
    if constexpr (DER) {
      const double dKr_dKd = (hk * ha) * (I_Kr_denom * I_Kr_denom);
      const double ddT_k_dKd = dKr_dKd * q1;
      const double ddS_k_dKd = dKr_dKd * q2;
      const double ddT_km1_dKd = ((b1 * b1) * ha) * (dT_k + q3) + b1Kd * ddT_k_dKd;
      const double ddS_km1_dKd = ((b1 * b1) * ha) * (dS_k + q4) + b1Kd * ddS_k_dKd;
      dPEc_dKd = (Pk * ddT_k_dKd + Pa * ddT_km1_dKd) + (Sk * ddS_k_dKd + Sa * ddS_km1_dKd);
      const double dColHt_dKd = (Ck * ddT_k_dKd + Ca * ddT_km1_dKd) + (Dk * ddS_k_dKd + Da * ddS_km1_dKd);
      if (dColHt_dKd < 0.0) dPEc_dKd = dPEc_dKd - pres_Z * dColHt_dKd;
    }
    if constexpr (LIM) {
      dPE_max = (Pa * q3 + Sa * q4) + ((Pk + Pa) * q1 + (Sk + Sa) * q2) / (ha + hk);
      const double dColHt_max = (Ca * q3 + Da * q4) + ((Ck + Ca) * q1 + (Dk + Da) * q2) / (ha + hk);
      if (dColHt_max < 0.0) dPE_max = dPE_max - pres_Z * dColHt_max;
      dPEc_dKd_0 = (Pa * q3 + Sa * q4) / (ha) + (Pk * q1 + Sk * q2) / (hk * ha);
      const double dColHt_dKd = (Ca * q3 + Da * q4) / (ha) + (Ck * q1 + Dk * q2) / (hk * ha);
      if (dColHt_dKd < 0.0) dPEc_dKd_0 = dPEc_dKd_0 - pres_Z * dColHt_dKd;
    }
  } else {
    const double hps = ha + hk;
    const double bdt1 = ha * hk;   // + Kddt_h0 * hps with Kddt_h0 = 0
    const double dT_c = ha * q3 - hk * q1;
    const double dS_c = ha * q4 - hk * q2;
    const double PEc_core = hk * (Pa * dT_c + Sa * dS_c) - ha * (Pk * dT_c + Sk * dS_c);
    const double ColHt_core = hk * (Ca * dT_c + Da * dS_c) - ha * (Ck * dT_c + Dk * dS_c);
    double y1_3 = Kddt_h / (bdt1 * (bdt1 + Kddt_h * hps));
    PE_chg = PEc_core * y1_3;
    double ColHt_chg = ColHt_core * y1_3;
    if (ColHt_chg < 0.0) PE_chg = PE_chg - pres_Z * ColHt_chg;
    if constexpr (DER) {
      const double t = bdt1 + Kddt_h * hps;
      const double y1_4 = 1.0 / (t * t);
      dPEc_dKd = PEc_core * y1_4;
      ColHt_chg = ColHt_core * y1_4;
      if (ColHt_chg < 0.0) dPEc_dKd = dPEc_dKd - pres_Z * ColHt_chg;
    }
    if constexpr (LIM) {
      y1_3 = 1.0 / (bdt1 * hps);
      dPE_max = PEc_core * y1_3;
      ColHt_chg = ColHt_core * y1_3;
      if (ColHt_chg < 0.0) dPE_max = dPE_max - pres_Z * ColHt_chg;
      const double y1_4 = 1.0 / (bdt1 * bdt1);
      dPEc_dKd_0 = PEc_core * y1_4;
      ColHt_chg = ColHt_core * y1_4;
      if (ColHt_chg < 0.0) dPEc_dKd_0 = dPEc_dKd_0 - pres_Z * ColHt_chg;
    }
  }
}

// find_uv_at_h without vertical mixing (MOM_diabatic_aux.F90:546-571, :606-611) for one cell: x its column, o its layer.  The
// weights are formed again for every layer, not kept: the column walk has no registers to spare for them.
__device__ __forceinline__ void ep_uv_at_h(const Dm &d, const double *__restrict__ G, const EpP &P, size_t x, size_t o, double &u_h, double &v_h) {
  const double *aCu = gm(G, d, MOM6X_G_areaCu), *aCv = gm(G, d, MOM6X_G_areaCv);
  const double IaT = gm(G, d, MOM6X_G_IareaT)[x];
  double a_w = 0.0, a_e = 0.0, a_s = 0.0, a_n = 0.0;
  double sum_area = aCu[x - 1] + aCu[x];
  if (sum_area > 0.0) { const double Idenom = sqrt(0.5 * IaT / sum_area); a_w = aCu[x - 1] * Idenom; a_e = aCu[x] * Idenom; }
  sum_area = aCv[x - d.pitch] + aCv[x];
  if (sum_area > 0.0) { const double Idenom = sqrt(0.5 * IaT / sum_area); a_s = aCv[x - d.pitch] * Idenom; a_n = aCv[x] * Idenom; }
  u_h = (a_e * P.u[o]) + (a_w * P.u[o - 1]);
  v_h = (a_n * P.v[o]) + (a_s * P.v[o - d.pitch]);
}

// ORIG: orig_PE_calc; DIAG: TKE_diagnostics; MKE: MKE_to_TKE_effic > 0
template <bool ORIG, bool DIAG, bool MKE>
__global__ void __launch_bounds__(256) k_epbl_cols(Dm d, const double *__restrict__ G, EpK K, EpP P) {
  static_assert(!(DIAG && MKE), "k_epbl_cols<., true, true> does not fit a lane's registers; mom6x_energetic_PBL_init refuses the combination");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;

  if (!(gm(G, d, MOM6X_G_mask2dT)[x] > 0.0)) {   // :819-823
    for (int k = 0; k <= nz; ++k) {
      P.Kd[(size_t)k * slab + x] = 0.0;
      if (P.mixvel) P.mixvel[(size_t)k * slab + x] = 0.0;
      if (P.mixlen) P.mixlen[(size_t)k * slab + x] = 0.0;
    }
    P.MLD[x] = 0.0;
    if constexpr (DIAG) {   // :533-538
#pragma unroll
      for (int n = 0; n < 7; ++n) P.dwork[(size_t)n * slab + x] = 0.0;
    }
    if (P.mstar) P.mstar[x] = 0.0;
    if (P.ustar_d) P.ustar_d[x] = 0.0;
    if (P.its) P.its[x] = 0.0;
    return;
  }

#define DW_wind P.dwork[0 * slab + x]
#define DW_mke P.dwork[1 * slab + x]
#define DW_conv P.dwork[2 * slab + x]
#define DW_forcing P.dwork[3 * slab + x]
#define DW_mixing P.dwork[4 * slab + x]
#define DW_mech_decay P.dwork[5 * slab + x]
#define DW_conv_decay P.dwork[6 * slab + x]
  // energetic_PBL :631-673
  double u_star = P.ustar[x];
  if (P.ustar_d) P.ustar_d[x] = u_star;
  if (u_star < K.ustar_min) u_star = K.ustar_min;
  double absf;
  if (K.omega_frac >= 1.0) {
    absf = 2.0 * K.omega;
  } else {
    const double *f = gm(G, d, MOM6X_G_CoriolisBu);
    absf = 0.25 * ((fabs(f[x]) + fabs(f[x - d.pitch - 1])) + (fabs(f[x - d.pitch]) + fabs(f[x - 1])));
    if (K.omega_frac > 0.0) absf = sqrt(K.omega_frac * 4.0 * (K.omega * K.omega) + (1.0 - K.omega_frac) * (absf * absf));
  }
  double MLD_guess = -1.0;
  if (K.guess) { const double m0 = P.MLD[x]; if (m0 > 0.0) MLD_guess = m0; }


  // ePBL_column :1203-1224: dz_sum and max_MLD top-down, hb_hs bottom-up into the work array
  double dz_sum = K.dZ_sub, max_MLD = 0.0;
  for (int k = 0; k < nz; ++k) {
    const double dzk = K.H_to_Z * P.h[(size_t)k * slab + x] + K.dZ_sub;
    dz_sum = dz_sum + dzk;
    max_MLD = max_MLD + dzk;
  }
  double I_dzsum = 0.0;
  if (dz_sum > 0.0) I_dzsum = 1.0 / dz_sum;
  {
    double dz_bot = 0.0;
    P.hb_hs[(size_t)nz * slab + x] = 0.0;
    for (int k = nz - 1; k >= 0; --k) {
      dz_bot = dz_bot + (K.H_to_Z * P.h[(size_t)k * slab + x] + K.dZ_sub);
      P.hb_hs[(size_t)k * slab + x] = dz_bot * I_dzsum;
    }
  }
  double MLD_output = K.H_to_Z * P.h[x] + K.dZ_sub;
  double min_MLD = 0.0;
  double dMLD_min = -1.0 * K.m_to_Z, dMLD_max = 1.0 * K.m_to_Z;
  if (MLD_guess <= min_MLD) MLD_guess = 0.5 * (min_MLD + max_MLD);
  const double h_dz_int = K.Z_to_H;

  // with DIAG the seven terms of the TKE budget are accumulated in the module's work planes (one base address), not in registers;
  // k_epbl_diag_out hands them to the caller's planes
  double mstar_total = 0.0;
  int OBL_it = 0;
  while (OBL_it < K.max_its) {
    ++OBL_it;
    // the surface layer is read again in every iteration: nothing of it is kept across the walk
    const double h0 = P.h[x] + K.H_sub, dz0 = K.H_to_Z * P.h[x] + K.dZ_sub;
    const double T00 = P.T[x], S00 = P.S[x], TKE0 = P.TKE[x];
    const double dSVdT0 = P.dSV_dT[x], dSVdS0 = P.dSV_dS[x];
    MLD_output = dz0;
    bool sfc_connected = true;
    const double B_flux = P.bflux[x];
    const double us0 = P.ustar[x];
    const double mech_TKE_in = K.dt * K.Rho0 * ((us0 * us0) * us0);   // :634, from fluxes%ustar before ustar_min
    mstar_total = ep_find_mstar(K, B_flux, u_star, MLD_guess, absf);
    double mech_TKE;
    if (K.old2019 && (K.mstar_scheme == MOM6X_EPBL_MSTAR_CONSTANT)) mech_TKE = (K.dt * mstar_total * K.Rho0) * ((u_star * u_star) * u_star);
    else mech_TKE = mstar_total * mech_TKE_in;
    if constexpr (DIAG) {
      DW_conv = 0.0;
      DW_mixing = 0.0;
      DW_mke = 0.0;   // eCD%dTKE_MKE stays 0: DIAG is built without MKE (the static_assert above), so MKE_src is 0 throughout
      DW_mech_decay = 0.0;
      DW_conv_decay = 0.0;
      DW_wind = mech_TKE * K.I_dtdiag;
      {
        if (TKE0 <= 0.0) DW_forcing = fmax1(-mech_TKE, TKE0) * K.I_dtdiag;
        else DW_forcing = K.nstar * TKE0 * K.I_dtdiag;
      }
    }
    double conv_PErel;
    if (TKE0 <= 0.0) {
      mech_TKE = mech_TKE + TKE0;
      if (mech_TKE < 0.0) mech_TKE = 0.0;
      conv_PErel = 0.0;
    } else {
      conv_PErel = TKE0;
    }
    // the mixing shape function :1293-1324 is formed at each interface
    const int shape = K.shape_one ? 0 : ((MLD_guess <= 0.0) ? 1 : 2);
    double I_MLD = 0.0;
    if (shape == 2) I_MLD = 1.0 / MLD_guess;
    double dz_rsum = 0.0;
    P.Kd[x] = 0.0;
    if (P.mixvel) P.mixvel[x] = 0.0;
    if (P.mixlen) P.mixlen[x] = 0.0;
    double Kddt_h_prev = 0.0;
    double hp_a = h0;
    double dMass = K.H_to_RZ * h0;
    double dPres = K.g_Z * dMass;
    double pres_Z = 0.0;
    double dT_to_dPE_a = (dMass * (pres_Z + 0.5 * dPres)) * dSVdT0;
    double dS_to_dPE_a = (dMass * (pres_Z + 0.5 * dPres)) * dSVdS0;
    double dT_to_dColHt_a = dMass * dSVdT0;
    double dS_to_dColHt_a = dMass * dSVdS0;
    double dT_to_dColHt_km1 = dT_to_dColHt_a, dS_to_dColHt_km1 = dS_to_dColHt_a;
    pres_Z = pres_Z + dPres;
    double htot = h0, dztot = dz0, uhtot = 0.0, vhtot = 0.0;
    if constexpr (MKE) { double u0, v0; ep_uv_at_h(d, G, P, x, x, u0, v0); uhtot = u0 * h0; vhtot = v0 * h0; }
    double Xe_km2 = 0.0, Ye_km2 = 0.0;   // dTe(k-2), dSe(k-2) | Te(k-2), Se(k-2)
    double T_km2 = 0.0, S_km2 = 0.0, T_km1 = T00, S_km1 = S00, h_km1 = h0, dz_km1 = dz0;
    for (int k = 1; k < nz; ++k) {   // interface K = k + 1 of the reference, between layers k - 1 and k
      const size_t o = (size_t)k * slab + x;
      const double hk = P.h[o] + K.H_sub, dzk = K.H_to_Z * P.h[o] + K.dZ_sub;
      const double Tk = P.T[o], Sk = P.S[o], TKEk = P.TKE[o];
      const double dSVdT = P.dSV_dT[o], dSVdS = P.dSV_dS[o];
      // :1192-1201 for the layer below
      dMass = K.H_to_RZ * hk;
      dPres = K.g_Z * dMass;
      const double dT_to_dPE = (dMass * (pres_Z + 0.5 * dPres)) * dSVdT;
      const double dS_to_dPE = (dMass * (pres_Z + 0.5 * dPres)) * dSVdS;
      const double dT_to_dColHt = dMass * dSVdT;
      const double dS_to_dColHt = dMass * dSVdS;
      double MixLen_shape;
      if (shape == 0) {
        MixLen_shape = 1.0;
      } else if (shape == 1) {
        MixLen_shape = (K.transLay > 0.0) ? K.transLay : 1.0;
      } else {
        dz_rsum = dz_rsum + dz_km1;
        const double xs = fmax1(K.zero, (MLD_guess - dz_rsum) * I_MLD);
        if (K.MixLenExp == 2.0) MixLen_shape = K.transLay + (1.0 - K.transLay) * (xs * xs);
        else MixLen_shape = K.transLay + (1.0 - K.transLay) * pow(xs, K.MixLenExp);
      }
      const double Idecay_len_TKE = (K.TKE_decay * absf / u_star) * K.H_to_Z;
      double exp_kh = 1.0;
      if (Idecay_len_TKE > 0.0) exp_kh = exp(-h_km1 * Idecay_len_TKE);
      if constexpr (DIAG) DW_mech_decay = DW_mech_decay + (exp_kh - 1.0) * mech_TKE * K.I_dtdiag;
      mech_TKE = mech_TKE * exp_kh;
      if (TKEk > 0.0) {
        conv_PErel = conv_PErel + TKEk;
        if constexpr (DIAG) DW_forcing = DW_forcing + K.nstar * TKEk * K.I_dtdiag;
      }
      double nstar_FC = K.nstar;
      if (K.nstar * conv_PErel > 0.0) {
        const double t = absf * dztot;
        nstar_FC = K.nstar * conv_PErel / (conv_PErel + 0.2 * sqrt(0.5 * K.dt * K.Rho0 * ((t * t) * t) * conv_PErel));
      }
      double tot_TKE = mech_TKE + nstar_FC * conv_PErel;
      if (TKEk < 0.0) {   // :1401-1424
        if (TKEk + tot_TKE < 0.0) {
          if constexpr (DIAG) {
            DW_mixing = DW_mixing + tot_TKE * K.I_dtdiag;
            DW_forcing = DW_forcing - tot_TKE * K.I_dtdiag;
            DW_conv_decay = DW_conv_decay + (K.nstar - nstar_FC) * conv_PErel * K.I_dtdiag;
          }
          tot_TKE = 0.0; mech_TKE = 0.0; conv_PErel = 0.0;
        } else {
          const double TKE_reduc = (tot_TKE + TKEk) / tot_TKE;
          if constexpr (DIAG) {
            DW_mixing = DW_mixing - TKEk * K.I_dtdiag;
            DW_forcing = DW_forcing + TKEk * K.I_dtdiag;
            DW_conv_decay = DW_conv_decay + (1.0 - TKE_reduc) * (K.nstar - nstar_FC) * conv_PErel * K.I_dtdiag;
          }
          tot_TKE = TKE_reduc * tot_TKE;
          mech_TKE = TKE_reduc * mech_TKE;
          conv_PErel = TKE_reduc * conv_PErel;
        }
      }
      double dTe_t2 = 0.0, dSe_t2 = 0.0;
      if constexpr (ORIG) {
        if (k > 1) {
          dTe_t2 = Kddt_h_prev * ((T_km2 - T_km1) + Xe_km2);
          dSe_t2 = Kddt_h_prev * ((S_km2 - S_km1) + Ye_km2);
        }
      }
      const double dt_h = K.dt / fmax1(0.5 * (dz_km1 + dzk), 1e-15 * dz_sum);
      const bool Convectively_stable = (0.0 <= ((dT_to_dColHt + dT_to_dColHt_km1) * (T_km1 - Tk) +
                                                (dS_to_dColHt + dS_to_dColHt_km1) * (S_km1 - Sk)));
      double Kd_k = 0.0, Kddt_h = 0.0, b1, hp_a_new;
      if (P.mixvel) P.mixvel[o] = 0.0;   // :1290
      if (P.mixlen) P.mixlen[o] = 0.0;
      double Xe_km1 = 0.0, Ye_km1 = 0.0;
      bool sfc_disconnect;
      if (((mech_TKE + conv_PErel) <= 0.0) && Convectively_stable) {   // :1447-1470
        tot_TKE = 0.0; mech_TKE = 0.0; conv_PErel = 0.0;
        Kd_k = 0.0; Kddt_h = 0.0;
        sfc_disconnect = true;
        b1 = 1.0 / hp_a;
        if constexpr (ORIG) { Xe_km1 = b1 * (dTe_t2); Ye_km1 = b1 * (dSe_t2); }
        hp_a_new = hk;
        dT_to_dPE_a = dT_to_dPE; dS_to_dPE_a = dS_to_dPE;
        dT_to_dColHt_a = dT_to_dColHt; dS_to_dColHt_a = dS_to_dColHt;
      } else {
        sfc_disconnect = false;
        double q1, q2, q3, q4;
        if constexpr (ORIG) {
          if (k == 1) {
            q3 = (Tk - T_km1);
            q4 = (Sk - S_km1);
          } else {
            q3 = (Tk - T_km1) - (Kddt_h_prev / hp_a) * ((T_km2 - T_km1) + Xe_km2);
            q4 = (Sk - S_km1) - (Kddt_h_prev / hp_a) * ((S_km2 - S_km1) + Ye_km2);
          }
          q1 = dTe_t2 + hp_a * (T_km1 - Tk);
          q2 = dSe_t2 + hp_a * (S_km1 - Sk);
        } else {
          if (k <= 1) {
            q1 = h_km1 * T_km1; q2 = h_km1 * S_km1;
          } else {
            q1 = h_km1 * T_km1 + Kddt_h_prev * Xe_km2;
            q2 = h_km1 * S_km1 + Kddt_h_prev * Ye_km2;
          }
          q3 = hk * Tk; q4 = hk * Sk;
        }
#define EP_PE(DER, LIM, Kddt, PE, DPE, PMAX, DPE0) \
        ep_PE_chg<ORIG, DER, LIM>(Kddt, hk, hp_a, q1, q2, q3, q4, dT_to_dPE, dS_to_dPE, dT_to_dPE_a, dS_to_dPE_a, pres_Z, dT_to_dColHt, \
                                  dS_to_dColHt, dT_to_dColHt_a, dS_to_dColHt_a, PE, DPE, PMAX, DPE0)
        double dMKE_max = 0.0, MKE2_Hharm = 0.0;
        if constexpr (MKE) {
          if (htot * hk > 0.0) {
            double uk, vk;
            ep_uv_at_h(d, G, P, x, o, uk, vk);
            const double du = uhtot - uk * htot, dv = vhtot - vk * htot;
            dMKE_max = (K.H_to_RZ * K.MKE_eff) * 0.5 * (hk / ((htot + hk) * htot)) * ((du * du) + (dv * dv));
            MKE2_Hharm = (htot + hk + 2.0 * K.H_sub) / ((htot + K.H_sub) * (hk + K.H_sub));
          }
        }
        const double dz_tt = dztot + 0.0;
        const double hbs_here = fmin1(P.hb_hs[o], MixLen_shape);
        double TKE_here = mech_TKE + K.wstar * conv_PErel;
        double vstar, Kd_guess0;
        if (TKE_here > 0.0) {
          vstar = ep_vstar(K, TKE_here, conv_PErel, dztot, MLD_guess, u_star);
          const double mixlen_k = fmax1(K.min_mix_len, ((dz_tt * hbs_here) * vstar) / ((K.Ekman * absf) * (dz_tt * hbs_here) + vstar));
          if (P.mixlen) P.mixlen[o] = mixlen_k;
          if (!K.use_iter) Kd_guess0 = (h_dz_int * vstar) * K.vonKar * ((dz_tt * hbs_here) * vstar) / ((K.Ekman * absf) * (dz_tt * hbs_here) + vstar);
          else Kd_guess0 = (h_dz_int * vstar) * K.vonKar * mixlen_k;
        } else {
          vstar = 0.0; Kd_guess0 = 0.0;
        }
        if (P.mixvel) P.mixvel[o] = vstar;
        const double Kddt_h_g0 = Kd_guess0 * dt_h;
        double PE_chg_g0, PE_chg_max, dPEc_dKd_Kd0, dum;
        EP_PE(false, true, Kddt_h_g0, PE_chg_g0, dum, PE_chg_max, dPEc_dKd_Kd0);
        const bool convectively_unstable = (PE_chg_g0 < 0.0) || ((vstar == 0.0) && (dPEc_dKd_Kd0 < 0.0));
        double MKE_src = 0.0;
        if constexpr (MKE) MKE_src = dMKE_max * (1.0 - exp(-Kddt_h_g0 * MKE2_Hharm));
        if (convectively_unstable) {   // :1594-1671
          double dPE_conv;
          if (PE_chg_max <= 0.0) {
            TKE_here = mech_TKE + K.wstar * (conv_PErel - PE_chg_max);
            if (TKE_here > 0.0) {
              vstar = ep_vstar(K, TKE_here, conv_PErel, dztot, MLD_guess, u_star);
              const double mixlen_k = fmax1(K.min_mix_len, ((dz_tt * hbs_here) * vstar) / ((K.Ekman * absf) * (dz_tt * hbs_here) + vstar));
              if (P.mixlen) P.mixlen[o] = mixlen_k;
              if (!K.use_iter) Kd_k = (h_dz_int * vstar) * K.vonKar * ((dz_tt * hbs_here) * vstar) / ((K.Ekman * absf) * (dz_tt * hbs_here) + vstar);
              else Kd_k = (h_dz_int * vstar) * K.vonKar * mixlen_k;
            } else {
              vstar = 0.0; Kd_k = 0.0;
            }
            if (P.mixvel) P.mixvel[o] = vstar;
            double d1, d2, d3;
            EP_PE(false, false, Kd_k * dt_h, dPE_conv, d1, d2, d3);
            if (dPE_conv > 0.0) {
              Kd_k = Kd_guess0; dPE_conv = PE_chg_g0;
            } else {
              if constexpr (MKE) MKE_src = dMKE_max * (1.0 - exp(-(Kd_k * dt_h) * MKE2_Hharm));
            }
          } else {
            Kd_k = Kd_guess0; dPE_conv = PE_chg_g0;
          }
          conv_PErel = conv_PErel - dPE_conv;
          mech_TKE = mech_TKE + MKE_src;
          if constexpr (DIAG) {
            DW_conv = DW_conv - K.nstar * dPE_conv * K.I_dtdiag;
          }
          if (sfc_connected) MLD_output = MLD_output + dzk;
        } else if (tot_TKE + (MKE_src - PE_chg_g0) >= 0.0) {   // :1697-1718
          Kd_k = Kd_guess0;
          tot_TKE = tot_TKE + MKE_src;
          double TKE_reduc = 0.0;
          if (tot_TKE > 0.0) TKE_reduc = (tot_TKE - PE_chg_g0) / tot_TKE;
          if constexpr (DIAG) {
            DW_mixing = DW_mixing - PE_chg_g0 * K.I_dtdiag;
            DW_conv_decay = DW_conv_decay + (1.0 - TKE_reduc) * (K.nstar - nstar_FC) * conv_PErel * K.I_dtdiag;
          }
          tot_TKE = TKE_reduc * tot_TKE;
          mech_TKE = TKE_reduc * (mech_TKE + MKE_src);
          conv_PErel = TKE_reduc * conv_PErel;
          if (sfc_connected) MLD_output = MLD_output + dzk;
        } else if (tot_TKE == 0.0) {   // :1720-1724
          Kd_k = 0.0;
          tot_TKE = 0.0; conv_PErel = 0.0; mech_TKE = 0.0;
          sfc_disconnect = true;
        } else {   // :1725-1820: the bracketed Newton solve
          double Kddt_h_max = Kddt_h_g0, Kddt_h_min = 0.0, PE_chg = 0.0;
          double TKE_left_max = tot_TKE + (MKE_src - PE_chg_g0);
          double TKE_left_min = tot_TKE;
          double Kddt_h_guess = tot_TKE * Kddt_h_max / fmax1(PE_chg_g0 - MKE_src, Kddt_h_max * (dPEc_dKd_Kd0 - dMKE_max * MKE2_Hharm));
          for (int itt = 1; itt <= 20; ++itt) {
            double dPEc_dKd, d2, d3;
            EP_PE(true, false, Kddt_h_guess, PE_chg, dPEc_dKd, d2, d3);
            double dMKE_src_dK = 0.0;
            if constexpr (MKE) {
              const double ex = exp(-MKE2_Hharm * Kddt_h_guess);   // (the reference evaluates it twice)
              MKE_src = dMKE_max * (1.0 - ex);
              dMKE_src_dK = dMKE_max * MKE2_Hharm * ex;
            }
            const double TKE_left = tot_TKE + (MKE_src - PE_chg);
            if (TKE_left >= 0.0) { Kddt_h_min = Kddt_h_guess; TKE_left_min = TKE_left; }
            else { Kddt_h_max = Kddt_h_guess; TKE_left_max = TKE_left; }
            bool use_Newt = true;
            double dKddt_h_Newt = 0.0;
            if (dPEc_dKd - dMKE_src_dK <= 0.0) {
              use_Newt = false;
            } else {
              dKddt_h_Newt = TKE_left / (dPEc_dKd - dMKE_src_dK);
              const double Kddt_h_Newt = Kddt_h_guess + dKddt_h_Newt;
              if ((Kddt_h_Newt > Kddt_h_max) || (Kddt_h_Newt < Kddt_h_min)) use_Newt = false;
            }
            double Kddt_h_next, dKddt_h;
            if (use_Newt) {
              Kddt_h_next = Kddt_h_guess + dKddt_h_Newt;
              dKddt_h = dKddt_h_Newt;
            } else {
              Kddt_h_next = (TKE_left_max * Kddt_h_min - Kddt_h_max * TKE_left_min) / (TKE_left_max - TKE_left_min);
              dKddt_h = Kddt_h_next - Kddt_h_guess;
            }
            if ((fabs(dKddt_h) < 1e-9 * Kddt_h_guess) || (itt == 20)) break;
            Kddt_h_guess = Kddt_h_next;
          }
          Kd_k = Kddt_h_guess / dt_h;
          if constexpr (DIAG) {
            DW_mixing = DW_mixing - (tot_TKE + MKE_src) * K.I_dtdiag;
            DW_conv_decay = DW_conv_decay + (K.nstar - nstar_FC) * conv_PErel * K.I_dtdiag;
          }
          if (sfc_connected) MLD_output = MLD_output + (PE_chg / (PE_chg_g0)) * dzk;
          tot_TKE = 0.0; mech_TKE = 0.0; conv_PErel = 0.0;
          sfc_disconnect = true;
        }
#undef EP_PE
        Kddt_h = Kd_k * dt_h;
        b1 = 1.0 / (hp_a + Kddt_h);
        const double c1 = Kddt_h * b1;
        if constexpr (ORIG) {
          Xe_km1 = b1 * (Kddt_h * (Tk - T_km1) + dTe_t2);
          Ye_km1 = b1 * (Kddt_h * (Sk - S_km1) + dSe_t2);
        }
        hp_a_new = hk + (hp_a * b1) * Kddt_h;
        dT_to_dPE_a = dT_to_dPE + c1 * dT_to_dPE_a;
        dS_to_dPE_a = dS_to_dPE + c1 * dS_to_dPE_a;
        dT_to_dColHt_a = dT_to_dColHt + c1 * dT_to_dColHt_a;
        dS_to_dColHt_a = dS_to_dColHt + c1 * dS_to_dColHt_a;
      }
      P.Kd[o] = Kd_k;
      double uk = 0.0, vk = 0.0;
      if constexpr (MKE) ep_uv_at_h(d, G, P, x, o, uk, vk);   // formed again: not kept across the solve above
      if (sfc_disconnect) {   // :1842-1854
        if constexpr (MKE) { uhtot = uk * hk; vhtot = vk * hk; }
        htot = hk;
        dztot = dzk;
        sfc_connected = false;
      } else {
        if constexpr (MKE) { uhtot = uhtot + uk * hk; vhtot = vhtot + vk * hk; }
        htot = htot + hk;
        dztot = dztot + dzk;
      }
      if constexpr (!ORIG) {   // calc_Te :1856-1864
        if (k == 1) {
          Xe_km1 = b1 * (h_km1 * T_km1);
          Ye_km1 = b1 * (h_km1 * S_km1);
        } else {
          Xe_km1 = b1 * (h_km1 * T_km1 + Kddt_h_prev * Xe_km2);
          Ye_km1 = b1 * (h_km1 * S_km1 + Kddt_h_prev * Ye_km2);
        }
      }
      Xe_km2 = Xe_km1; Ye_km2 = Ye_km1;
      hp_a = hp_a_new;
      Kddt_h_prev = Kddt_h;
      dT_to_dColHt_km1 = dT_to_dColHt; dS_to_dColHt_km1 = dS_to_dColHt;
      pres_Z = pres_Z + dPres;
      T_km2 = T_km1; S_km2 = S_km1; T_km1 = Tk; S_km1 = Sk; h_km1 = hk; dz_km1 = dzk;
    }
    P.Kd[(size_t)nz * slab + x] = 0.0;
    if (P.mixvel) P.mixvel[(size_t)nz * slab + x] = 0.0;
    if (P.mixlen) P.mixlen[(size_t)nz * slab + x] = 0.0;

    if (OBL_it >= K.max_its) break;   // :1890
    const double MLD_found = MLD_output;
    if (K.bug) {   // :1901-1918
      if (MLD_found - MLD_guess > K.MLD_tol) { min_MLD = MLD_guess; dMLD_min = MLD_found - MLD_guess; }
      else if (fabs(MLD_found - MLD_guess) < K.MLD_tol) break;
      else { max_MLD = MLD_guess; dMLD_max = MLD_found - MLD_guess; }
    } else {
      if (fabs(MLD_found - MLD_guess) < K.MLD_tol) break;
      else if (MLD_found > MLD_guess) { min_MLD = MLD_guess; dMLD_min = MLD_found - MLD_guess; }
      else { max_MLD = MLD_guess; dMLD_max = MLD_found - MLD_guess; }
    }
    if (K.bisect) {   // :1921-1936
      MLD_guess = 0.5 * (min_MLD + max_MLD);
    } else if ((dMLD_min > 0.0) && (dMLD_max < 0.0) && (OBL_it > 2) && (((OBL_it - 1) % 4) > 0)) {
      MLD_guess = (dMLD_min * max_MLD - dMLD_max * min_MLD) / (dMLD_min - dMLD_max);
    } else if ((MLD_found > min_MLD) && (MLD_found < max_MLD)) {
      MLD_guess = MLD_found;
    } else {
      MLD_guess = 0.5 * (min_MLD + max_MLD);
    }
  }

  P.MLD[x] = MLD_output;
  if (P.mstar) P.mstar[x] = mstar_total;
  if (P.its) P.its[x] = (double)OBL_it;
#undef DW_wind
#undef DW_mke
#undef DW_conv
#undef DW_forcing
#undef DW_mixing
#undef DW_mech_decay
#undef DW_conv_decay
}

// :740-748: the column's eCD%dTKE_* (dwork) accumulated into the diag_TKE_* planes, which :533-538 zeroed
__global__ void __launch_bounds__(256) k_epbl_diag_out(Dm d, const double *__restrict__ dwork, EpD D, double zero) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
#pragma unroll
  for (int n = 0; n < 7; ++n)
    if (D.p[n]) D.p[n][x] = zero + dwork[(size_t)n * d.slab + x];
}

// energetic_PBL_get_MLD :3721-3723
__global__ void __launch_bounds__(256) k_epbl_scale(Dm d, const double *__restrict__ src, double *__restrict__ dst, double scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  dst[x] = scale * src[x];
}

// MOM_diabatic_driver.F90:1570-1581, one lane per point of levels 2..nk (blockIdx.z + 1); level 2 also writes visc%h_ML
__global__ void __launch_bounds__(256) k_epbl_augment(Dm d, const double *__restrict__ Kd_ePBL, const double *__restrict__ Kd_shear,
                                                      double *__restrict__ Kv_shear, double *__restrict__ Kd_heat,
                                                      double *__restrict__ Kd_salt, int additive, double Prandtl, double zero,
                                                      const double *__restrict__ MLD, double *__restrict__ h_ML, double Z_to_H) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  if (blockIdx.z == 0 && h_ML) h_ML[x] = Z_to_H * MLD[x];
  const int k = blockIdx.z + 1;
  if (k >= d.nk) return;
  const size_t o = (size_t)k * d.slab + x;
  const double Ke = Kd_ePBL[o];
  double Kd_add_here;
  if (additive) {
    Kd_add_here = Ke;
    Kv_shear[o] = Kv_shear[o] + Prandtl * Ke;
  } else {
    Kd_add_here = fmax1(Ke - Kd_shear[o], zero);
    Kv_shear[o] = fmax1(Kv_shear[o], Prandtl * Ke);
  }
  Kd_heat[o] = Kd_heat[o] + Kd_add_here;
  Kd_salt[o] = Kd_salt[o] + Kd_add_here;
}

}  // namespace

// energetic_PBL_CS as the surface scheme reads it, and the work array of hb_hs
struct EpblState {
  mom6x_energetic_PBL_params P;
  double *hb_hs;   // nk + 1 levels, on the device
  double *dwork;   // 7 planes with TKE_diagnostics: the accumulators of eCD%dTKE_*
};

void energetic_PBL_free(mom6x_ctx *c) {
  if (!c->epbl) return;
  (void)hipFree(c->epbl->hb_hs);
  (void)hipFree(c->epbl->dwork);
  delete c->epbl;
  c->epbl = nullptr;
}

extern "C" int mom6x_energetic_PBL_init(mom6x_ctx *c, const mom6x_energetic_PBL_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_energetic_PBL_init: null argument");
  HIPCHK(hipSetDevice(c->device));
  energetic_PBL_free(c);   // first: a refused or invalid init leaves no module behind, whatever was initialized before
  REFUSE(p->SpV_avg || !c->GV.Boussinesq, "energetic_PBL_init", "non-Boussinesq mode (tv%SpV_avg)");
  REFUSE(p->ePBL_BBL_effic > 0.0, "energetic_PBL_init", "bottom boundary layer ePBL (EPBL_BBL_EFFIC)");
  REFUSE(p->ePBL_tidal_effic > 0.0, "energetic_PBL_init", "bottom boundary layer ePBL (EPBL_BBL_TIDAL_EFFIC)");
  REFUSE(p->ePBL_BBL_use_mstar, "energetic_PBL_init", "bottom boundary layer ePBL (EPBL_BBL_USE_MSTAR)");
  REFUSE(p->use_LT, "energetic_PBL_init", "Langmuir turbulence (USE_LA_LI2016, EPBL_LT)");
  REFUSE(p->eqdisc, "energetic_PBL_init", "EPBL_EQD_DIFFUSIVITY_SHAPE");
  REFUSE(p->eqdisc_v0, "energetic_PBL_init", "EPBL_EQD_DIFFUSIVITY_VELOCITY");
  REFUSE(p->eqdisc_v0h, "energetic_PBL_init", "EPBL_EQD_DIFFUSIVITY_VELOCITY_H");
  REFUSE(p->direct_calc, "energetic_PBL_init", "DIRECT_EPBL_MIXING_CALC");
  REFUSE(p->options_diff > 0, "energetic_PBL_init", "EPBL_OPTIONS_DIFF");
  REFUSE(p->pert_epbl, "energetic_PBL_init", "stochastic perturbations (stoch_CS%pert_epbl)");
  REFUSE(p->ustar_shelf, "energetic_PBL_init", "an ice shelf's fluxes%ustar_shelf");
  REFUSE(p->tau_mag, "energetic_PBL_init", "fluxes%tau_mag in place of fluxes%ustar");
  // (k_epbl_cols<., true, true> needs 6 registers more than a lane has: the instantiation would keep values in scratch memory)
  REFUSE(p->TKE_diagnostics && p->MKE_to_TKE_effic > 0.0, "energetic_PBL_init", "TKE_diagnostics together with MKE_TO_TKE_EFFIC > 0");
  REQUIRE(p->mstar_scheme == MOM6X_EPBL_MSTAR_CONSTANT || p->mstar_scheme == MOM6X_EPBL_MSTAR_OM4 ||
          p->mstar_scheme == MOM6X_EPBL_MSTAR_REICHL_H18, MOM6X_EINVAL, "energetic_PBL_init: unknown EPBL_MSTAR_SCHEME");
  REQUIRE(p->wT_scheme == MOM6X_EPBL_WT_CUBE_ROOT_TKE || p->wT_scheme == MOM6X_EPBL_WT_REICHL_H18, MOM6X_EINVAL,
          "energetic_PBL_init: unknown EPBL_VEL_SCALE_SCHEME");
  REQUIRE(p->max_MLD_its >= 1, MOM6X_EINVAL, "energetic_PBL_init: EPBL_MLD_MAX_ITS must be at least 1");
  REQUIRE(p->Use_MLD_iteration || p->max_MLD_its == 1, MOM6X_EINVAL,
          "energetic_PBL_init: max_MLD_its must be 1 without USE_MLD_ITERATION (MOM_energetic_PBL.F90:3999)");
  REQUIRE(p->m_to_Z > 0.0 && p->T_to_s > 0.0 && p->ustar_min > 0.0, MOM6X_EINVAL,
          "energetic_PBL_init: m_to_Z, T_to_s and ustar_min must be positive");
  EpblState *s = new EpblState();
  c->epbl = s;
  s->P = *p;
  s->hb_hs = nullptr; s->dwork = nullptr;
  const size_t n = (size_t)(c->d.nk + 1) * c->d.slab * sizeof(double);
  HIPCHK(hipMalloc(&s->hb_hs, n));
  HIPCHK(hipMemsetAsync(s->hb_hs, work_fill_byte(), n, c->stream));
  if (p->TKE_diagnostics) {
    const size_t nd = (size_t)7 * c->d.slab * sizeof(double);
    HIPCHK(hipMalloc(&s->dwork, nd));
    HIPCHK(hipMemsetAsync(s->dwork, work_fill_byte(), nd, c->stream));
  }
  return MOM6X_OK;
}

extern "C" int mom6x_energetic_PBL(mom6x_ctx *c, const double *h, const double *u, const double *v, const double *T, const double *S,
                                   const double *dSV_dT, const double *dSV_dS, const double *TKE_forced, const double *ustar,
                                   const double *buoy_flux, double dt, double *Kd_int, double *ML_depth, double *Velocity_Scale,
                                   double *Mixing_Length, double *diag_TKE_wind, double *diag_TKE_MKE, double *diag_TKE_conv,
                                   double *diag_TKE_forcing, double *diag_TKE_mixing, double *diag_TKE_mech_decay,
                                   double *diag_TKE_conv_decay, double *mstar_sfc, double *ustar_diag, double *OBL_its) {
  REQUIRE(c && c->epbl, MOM6X_EINVAL, "energetic_PBL: Module must be initialized before it is used.");
  const EpblState *s = c->epbl;
  const mom6x_energetic_PBL_params &Q = s->P;
  const mom6x_vgrid &GV = c->GV;
  REQUIRE(Q.has_eos, MOM6X_EINVAL, "energetic_PBL: Temperature, salinity and an equation of state must now be used.");
  REQUIRE(ustar, MOM6X_EINVAL, "energetic_PBL: No surface friction velocity (ustar or tau_mag) defined in fluxes type.");
  REQUIRE(h && T && S && dSV_dT && dSV_dS && TKE_forced && buoy_flux, MOM6X_EINVAL,
          "energetic_PBL: null h, tv%T, tv%S, dSV_dT, dSV_dS, TKE_forced or buoy_flux");
  REQUIRE(Kd_int && ML_depth, MOM6X_EINVAL, "energetic_PBL: null Kd_int or ML_depth");
  const bool mke = Q.MKE_to_TKE_effic > 0.0;
  REQUIRE(!mke || (u && v), MOM6X_EINVAL, "energetic_PBL: MKE_TO_TKE_EFFIC > 0 needs u and v");
  const bool any_diag = diag_TKE_wind || diag_TKE_MKE || diag_TKE_conv || diag_TKE_forcing || diag_TKE_mixing || diag_TKE_mech_decay ||
                        diag_TKE_conv_decay;
  REQUIRE(!any_diag || Q.TKE_diagnostics, MOM6X_EINVAL, "energetic_PBL: a diag_TKE_* plane needs TKE_diagnostics");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "energetic_PBL: dt must be positive");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;

  EpK K;
  memset(&K, 0, sizeof(K));
  K.dt = dt; K.I_dtdiag = 1.0 / dt; K.Rho0 = GV.Rho0; K.H_to_Z = GV.H_to_Z; K.Z_to_H = GV.Z_to_H; K.H_to_RZ = GV.H_to_RZ;
  K.H_sub = GV.H_subroundoff; K.dZ_sub = GV.dZ_subroundoff; K.g_Z = Q.g_Earth_Z_T2; K.zero = 0.0;
  K.old2019 = Q.answer_date < 20190101; K.old2024 = Q.answer_date < 20240101;
  if (K.old2024) {   // :604, :680
    const double Z_to_m = 1.0 / Q.m_to_Z, s_to_T = 1.0 / Q.T_to_s;
    K.SpV_dt = (((Z_to_m * Z_to_m) * Z_to_m) * ((s_to_T * s_to_T) * s_to_T)) * (1.0 / (dt * GV.Rho0));
  } else {
    K.SpV_dt = 1.0 / (GV.Rho0 * dt);   // I_rho0dt :527
  }
  K.omega = Q.omega; K.omega_frac = Q.omega_frac; K.Ekman = Q.Ekman_scale_coef; K.vonKar = Q.vonKar; K.MKE_eff = Q.MKE_to_TKE_effic;
  K.TKE_decay = Q.TKE_decay; K.fixed_mstar = Q.fixed_mstar; K.mstar_cap = Q.mstar_cap; K.mstar_coef = Q.mstar_coef; K.C_Ek = Q.C_Ek;
  K.cn1 = Q.RH18_mstar_cn1; K.cn2 = Q.RH18_mstar_cn2; K.cn3 = Q.RH18_mstar_cn3; K.cs1 = Q.RH18_mstar_cs1; K.cs2 = Q.RH18_mstar_cs2;
  K.nstar = Q.nstar; K.conv_coef = Q.mstar_convect_coef; K.transLay = Q.transLay_scale; K.MLD_tol = Q.MLD_tol;
  K.min_mix_len = Q.min_mix_len; K.MixLenExp = Q.MixLenExponent; K.wstar = Q.wstar_ustar_coef; K.vfac = Q.vstar_scale_fac;
  K.vsurf = Q.vstar_surf_fac; K.ustar_min = Q.ustar_min; K.m_to_Z = Q.m_to_Z; K.T_to_s = Q.T_to_s; K.vus = Q.m_to_Z * Q.T_to_s;
  K.mstar_scheme = Q.mstar_scheme; K.use_iter = Q.Use_MLD_iteration != 0; K.guess = Q.MLD_iteration_guess != 0;
  K.bisect = Q.MLD_bisection != 0; K.bug = Q.MLD_iter_bug != 0; K.max_its = Q.max_MLD_its; K.wT = Q.wT_scheme;
  K.shape_one = (!Q.Use_MLD_iteration) || (Q.transLay_scale >= 1.0) || (Q.transLay_scale < 0.0);

  EpP A;
  memset(&A, 0, sizeof(A));
  A.h = h; A.u = u; A.v = v; A.T = T; A.S = S; A.dSV_dT = dSV_dT; A.dSV_dS = dSV_dS; A.TKE = TKE_forced; A.ustar = ustar;
  A.bflux = buoy_flux; A.Kd = Kd_int; A.MLD = ML_depth; A.hb_hs = s->hb_hs; A.dwork = s->dwork; A.mixvel = Velocity_Scale; A.mixlen = Mixing_Length;
  A.mstar = mstar_sfc; A.ustar_d = ustar_diag; A.its = OBL_its;

  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
  const bool orig = Q.orig_PE_calc != 0, diag = Q.TKE_diagnostics != 0;
#define EPC(O, D, M) KLAUNCH(c, "k_epbl_cols<" #O ", " #D ", " #M ">", (k_epbl_cols<O, D, M>), g, b, d, c->G, K, A)
  if (orig) { if (diag) EPC(true, true, false); else if (mke) EPC(true, false, true); else EPC(true, false, false); }
  else { if (diag) EPC(false, true, false); else if (mke) EPC(false, false, true); else EPC(false, false, false); }
#undef EPC
  if (any_diag) {   // the order of DW_* in k_epbl_cols
    EpD D;
    D.p[0] = diag_TKE_wind; D.p[1] = diag_TKE_MKE; D.p[2] = diag_TKE_conv; D.p[3] = diag_TKE_forcing; D.p[4] = diag_TKE_mixing;
    D.p[5] = diag_TKE_mech_decay; D.p[6] = diag_TKE_conv_decay;
    KLAUNCH(c, "k_epbl_diag_out", k_epbl_diag_out, g, b, d, s->dwork, D, 0.0);
  }
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_energetic_PBL_get_MLD(mom6x_ctx *c, const double *ML_depth, double *MLD, double scale) {
  REQUIRE(c && c->epbl, MOM6X_EINVAL, "energetic_PBL_get_MLD: Module must be initialized before it is used.");
  REQUIRE(ML_depth && MLD, MOM6X_EINVAL, "energetic_PBL_get_MLD: null ML_depth or MLD");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
  KLAUNCH(c, "k_epbl_scale", k_epbl_scale, g, b, d, ML_depth, MLD, scale);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_ePBL_augment_Kd(mom6x_ctx *c, const double *Kd_ePBL, const double *Kd_shear, double *Kv_shear, double *Kd_heat,
                                     double *Kd_salt, int ePBL_is_additive, double ePBL_Prandtl, const double *MLD, double *h_ML) {
  REQUIRE(c, MOM6X_EINVAL, "ePBL_augment_Kd: null context");
  REQUIRE(Kd_ePBL && Kv_shear && Kd_heat && Kd_salt, MOM6X_EINVAL, "ePBL_augment_Kd: null Kd_ePBL, visc%Kv_shear, Kd_heat or Kd_salt");
  REQUIRE(ePBL_is_additive || Kd_shear, MOM6X_EINVAL, "ePBL_augment_Kd: without EPBL_IS_ADDITIVE visc%Kd_shear is needed");
  REQUIRE((MLD != nullptr) == (h_ML != nullptr), MOM6X_EINVAL, "ePBL_augment_Kd: MLD and visc%h_ML go together");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2(), g = grid3(d.ni, d.nj, d.nk > 1 ? d.nk - 1 : 1, b);
  KLAUNCH(c, "k_epbl_augment", k_epbl_augment, g, b, d, Kd_ePBL, Kd_shear, Kv_shear, Kd_heat, Kd_salt, ePBL_is_additive != 0,
          ePBL_Prandtl, 0.0, MLD, h_ML, c->GV.Z_to_H);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
