// MEKE.hip -- the mesoscale eddy kinetic energy equation on gfx950, the EKE_SOURCE = prog arm.
//
//   step_forward_MEKE      <- src/parameterizations/lateral/MOM_MEKE.F90:174-982 (:289-853 and :870-927)
//   MEKE_equilibrium       <- :987-1143
//   MEKE_equilibrium_restoring <- :1148-1178
//   MEKE_lengthScales      <- :1183-1253
//   MEKE_lengthScales_0d   <- :1258-1325
//   MEKE_init              <- :1329-1750, the members of mom6x_MEKE_params
//
// Boussinesq, no open boundaries (G%OBCmaskCu/v are mask2dCu/v), G%Z_ref = 0.  The launches of one call, each one lane per cell or
// face with lanes along i:
//   k_meke_cols    the only 3-D traffic: h, hu, hv once each, k = 1..nz in order, into mass, I_mass, depth_tot (isc-1..iec+1) and
//                  baroHu, baroHv (their faces); hu, hv are skipped without advection, one layer of them is read with the bug arm
//   k_meke_equil   the first call while CS%initialize is set: MEKE_equilibrium, one lane per column, the reference's loops as written
//   k_meke_lscale  MEKE_lengthScales into the planes bottomFac2, barotrFac2, LmixScale (kept for :903-918), MEKE%Le
//   k_meke_src     drag_rate_visc, the sources, the full step of source and the first Strang stage (:329-357, :415-606)
//   -- pass_MEKE :611 (with kh_flux_enabled or MEKE_K4 >= 0)
//   k_meke_flux    one lane per face, both directions in one launch: the biharmonic flux from del2MEKE formed where it is read
//                  (:615-668), the Laplacian flux with its CFL limiter and the upwind advection (:681-738)
//   k_meke_update  the two flux divergences, the second Strang stage and MEKE_POSITIVE (:669-678, :740-849, :870-875)
//   -- pass_MEKE :878
//   k_meke_diff    MEKE%Kh, Ku, Au and the velocity-scale diagnostics (:881-920, :933-980)
//   -- pass_Kh :925 of the planes given
// The fluxes go through planes between k_meke_flux and k_meke_update because a cell's update reads its neighbours' MEKE as it was
// after the first stage; the length scales and the root find have kernels of their own so that their pow and their loops do not
// take registers from the step kernels.  MAX and MIN are fmax1 and fmin1 of mom6x_dev.h with the reference's argument order; x**2 is
// x*x and x**3 is (x*x)*x.  The one departure from the reference (Kh_here without MEKE%Kh, :683-711) is described in include/mom6x.h.
#include "mom6x_dev.h"

// MEKE_CS, G%dF_dx, G%dF_dy and the work planes of mom6x_MEKE_init
enum { MW_mass = 0, MW_Imass, MW_depth, MW_baroHu, MW_baroHv, MW_drv, MW_bf2, MW_tf2, MW_Lmix, MW_cur, MW_s1, MW_uf, MW_vf, MW_uf4, MW_vf4,
       MW_COUNT };
struct MekeState {
  mom6x_MEKE_params p;
  bool initialize;        // CS%initialize :1720
  bool kh_flux_enabled;   // :1617-1619
  double *dF_dx, *dF_dy;  // device copies (null with use_old_lscale and none given)
  double *work;           // MW_COUNT planes
};

namespace {

struct MekeK {
  double damping, Cd_scale, Cb, min_gamma, Ct, GMcoeff, GEOMETRIC_alpha, restoring_rate, FrCoeff, bhFrCoeff, bh_coeff, GMECoeff, BGsrc;
  double Kh, K4, KhCoeff, Uscale, min_depth_tot, KhMEKE_Fac, lscale_maxval, Ku, Au, Lfixed, aDeform, aRhines, aEady, aFrict, aGrid;
  double topographic_beta, cdrag, cdrag2, T_to_s, L_to_m, m_s_to_L_T;
  double H_to_RZ, RZ_to_H, Z_to_H, h_neglect, mass_neglect, sdt, sdt_damp, damp_step, advFac;
  int GEOMETRIC, equilibrium_alt, restoring, positive, GM_src_alt, visc_drag, old_lscale, min_lscale, Rd_as_max_scale, fixed_total_depth;
  int adv, adv_bug, use_drag_rate, split, kh_flux, any_s1, any_damp;
};
struct MekeVisc { const double *Kv_u, *Kv_v, *thick_u, *thick_v; };   // all four, or all null (drag_rate_visc = 0)
struct MekeSrc { const double *GM_src, *mom_src, *mom_src_bh, *GME_snk; };
struct MekeDiag { double *src, *src_adv, *src_mom_K4, *src_btm_drag, *src_GM, *src_mom_lp, *src_mom_bh, *decay; };

// :329-357 at one cell
__device__ __forceinline__ double meke_drag_vel(double mask, double thick, double Kv) {
  double dv = 0.0;
  if ((mask > 0.0) && (thick > 0.0)) dv = Kv / thick;
  return dv;
}
__device__ __forceinline__ double meke_drag_rate_visc(const Dm &d, const double *__restrict__ G, const MekeVisc &V, size_t x) {
  if (!V.Kv_u) return 0.;
  const size_t p = (size_t)d.pitch;
  const double *mu = gm(G, d, MOM6X_G_mask2dCu), *mv = gm(G, d, MOM6X_G_mask2dCv);
  const double *aCu = gm(G, d, MOM6X_G_areaCu), *aCv = gm(G, d, MOM6X_G_areaCv);
  const double uW = meke_drag_vel(mu[x - 1], V.thick_u[x - 1], V.Kv_u[x - 1]), uE = meke_drag_vel(mu[x], V.thick_u[x], V.Kv_u[x]);
  const double vS = meke_drag_vel(mv[x - p], V.thick_v[x - p], V.Kv_v[x - p]), vN = meke_drag_vel(mv[x], V.thick_v[x], V.Kv_v[x]);
  return (0.25 * gm(G, d, MOM6X_G_IareaT)[x] * (((aCu[x - 1] * uW) + (aCu[x] * uE)) + ((aCv[x - p] * vS) + (aCv[x] * vN))));
}

// MEKE_lengthScales_0d :1258-1325.  Lrhines and Leady are set on the arm that is not use_old_lscale only, as in the reference.
__device__ __forceinline__ void meke_lscales_0d(const MekeK &K, double area, double beta, double depth_tot, double Rd_dx, double SN,
                                                double EKE, double &bottomFac2, double &barotrFac2, double &LmixScale, double &Lrhines,
                                                double &Leady) {
  const double Lgrid = sqrt(area);
  const double Ldeform = Lgrid * Rd_dx;
  const double Lfrict = depth_tot / K.cdrag;
  bottomFac2 = K.Cd_scale * K.Cd_scale;
  if (Lfrict * K.Cb > 0.) bottomFac2 = bottomFac2 + 1. / pow(1. + K.Cb * (Ldeform / Lfrict), 0.8);
  bottomFac2 = fmax1(bottomFac2, K.min_gamma);
  barotrFac2 = 1.;
  if (Lfrict * K.Ct > 0.) barotrFac2 = 1. / pow(1. + K.Ct * (Ldeform / Lfrict), 0.25);
  barotrFac2 = fmax1(barotrFac2, K.min_gamma);
  if (K.old_lscale) {
    if (K.Rd_as_max_scale) LmixScale = fmin1(Ldeform, Lgrid);
    else LmixScale = Lgrid;
  } else {
    const double Ue = sqrt(2.0 * fmax1(0., barotrFac2 * EKE));
    Lrhines = sqrt(Ue / fmax1(beta, 1.e-30 * K.T_to_s * K.L_to_m));
    if (K.aEady > 0.) Leady = Ue / fmax1(SN, 1.e-15 * K.T_to_s);
    else Leady = 0.;
    if (K.min_lscale) {
      LmixScale = K.lscale_maxval;
      if (K.aDeform * Ldeform > 0.) LmixScale = fmin1(LmixScale, K.aDeform * Ldeform);
      if (K.aFrict * Lfrict > 0.) LmixScale = fmin1(LmixScale, K.aFrict * Lfrict);
      if (K.aRhines * Lrhines > 0.) LmixScale = fmin1(LmixScale, K.aRhines * Lrhines);
      if (K.aEady * Leady > 0.) LmixScale = fmin1(LmixScale, K.aEady * Leady);
      if (K.aGrid * Lgrid > 0.) LmixScale = fmin1(LmixScale, K.aGrid * Lgrid);
      if (K.Lfixed > 0.) LmixScale = fmin1(LmixScale, K.Lfixed);
    } else {
      LmixScale = 0.;
      if (K.aDeform * Ldeform > 0.) LmixScale = LmixScale + 1. / (K.aDeform * Ldeform);
      if (K.aFrict * Lfrict > 0.) LmixScale = LmixScale + 1. / (K.aFrict * Lfrict);
      if (K.aRhines * Lrhines > 0.) LmixScale = LmixScale + 1. / (K.aRhines * Lrhines);
      if (K.aEady * Leady > 0.) LmixScale = LmixScale + 1. / (K.aEady * Leady);
      if (K.aGrid * Lgrid > 0.) LmixScale = LmixScale + 1. / (K.aGrid * Lgrid);
      if (K.Lfixed > 0.) LmixScale = LmixScale + 1. / K.Lfixed;
      if (LmixScale > 0.) LmixScale = 1. / LmixScale;
    }
  }
}

// beta of :1039-1059 | :1217-1239 (not formed with use_old_lscale, where MEKE_lengthScales_0d does not read it)
__device__ __forceinline__ double meke_beta(const MekeK &K, const Dm &d, const double *__restrict__ G, const double *__restrict__ depth_tot,
                                            const double *__restrict__ dF_dx, const double *__restrict__ dF_dy, size_t x) {
  const size_t p = (size_t)d.pitch;
  const double *Cor = gm(G, d, MOM6X_G_CoriolisBu);
  const double FatH = 0.25 * ((Cor[x] + Cor[x - 1 - p]) + (Cor[x - 1] + Cor[x - p]));
  const double D = depth_tot[x];
  double beta_topo_x, beta_topo_y;
  if (K.topographic_beta == 0. || (D == 0.0)) {
    beta_topo_x = 0.; beta_topo_y = 0.;
  } else {
    const double *IdxCu = gm(G, d, MOM6X_G_IdxCu), *IdyCv = gm(G, d, MOM6X_G_IdyCv);
    const double DE = depth_tot[x + 1], DW = depth_tot[x - 1], DN = depth_tot[x + p], DS = depth_tot[x - p];
    beta_topo_x = -K.topographic_beta * FatH * 0.5 * ((DE - D) * IdxCu[x] / fmax1(fmax1(DE, D), K.h_neglect) +
                                                      (D - DW) * IdxCu[x - 1] / fmax1(fmax1(D, DW), K.h_neglect));
    beta_topo_y = -K.topographic_beta * FatH * 0.5 * ((DN - D) * IdyCv[x] / fmax1(fmax1(DN, D), K.h_neglect) +
                                                      (D - DS) * IdyCv[x - p] / fmax1(fmax1(D, DS), K.h_neglect));
  }
  const double bx = dF_dx[x] + beta_topo_x, by = dF_dy[x] + beta_topo_y;
  return sqrt((bx * bx) + (by * by));
}

// SN = min(SN_u(I,j), SN_u(I-1,j), SN_v(i,J), SN_v(i,J-1)) :1034 | :1173
__device__ __forceinline__ double meke_SN_min(const Dm &d, const double *__restrict__ SN_u, const double *__restrict__ SN_v, size_t x) {
  return fmin1(fmin1(fmin1(SN_u[x], SN_u[x - 1]), SN_v[x]), SN_v[x - (size_t)d.pitch]);
}

// :299-327 and :359-388 on cells isc-1..iec+1, jsc-1..jec+1.  Lanes start at i = -IAL.
__global__ void __launch_bounds__(256)
k_meke_cols(Dm d, const double *__restrict__ G, MekeK K, const double *__restrict__ h, const double *__restrict__ hu,
            const double *__restrict__ hv, double *__restrict__ mass, double *__restrict__ I_mass, double *__restrict__ depth_tot,
            double *__restrict__ baroHu, double *__restrict__ baroHv) {
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni || j > d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  const double mask = gm(G, d, MOM6X_G_mask2dT)[x];
  double m = 0.0;
  size_t o = x;
  for (int k = 0; k < nz; ++k, o += slab) m = m + mask * (K.H_to_RZ * h[o]);
  mass[x] = m;
  double Im = 0.0;
  if (m > 0.0) Im = 1.0 / m;
  I_mass[x] = Im;
  if (K.fixed_total_depth) depth_tot[x] = (gm(G, d, MOM6X_G_bathyT)[x] + 0.0) * K.Z_to_H;   // G%Z_ref = 0
  else depth_tot[x] = m * K.RZ_to_H;
  if (!K.adv) return;
  if (i <= d.ni - 1 && j >= 0 && j <= d.nj - 1) {      // I = isc-1..iec, j = jsc..jec
    double b;
    if (K.adv_bug) {
      b = hu[x + (size_t)(nz - 1) * slab] * K.H_to_RZ;
    } else {
      b = 0.;
      o = x;
      for (int k = 0; k < nz; ++k, o += slab) b = b + hu[o] * K.H_to_RZ;
    }
    baroHu[x] = b;
  }
  if (i >= 0 && i <= d.ni - 1 && j <= d.nj - 1) {      // i = isc..iec, J = jsc-1..jec
    double b;
    if (K.adv_bug) {
      b = hv[x + (size_t)(nz - 1) * slab] * K.H_to_RZ;
    } else {
      b = 0.;
      o = x;
      for (int k = 0; k < nz; ++k, o += slab) b = b + hv[o] * K.H_to_RZ;
    }
    baroHv[x] = b;
  }
}

// MEKE_equilibrium :987-1143 on the computational domain.  The two `stop`s of the reference (a bracket beyond 2e17 m2 s-2 for the
// second time, :1095; more than 200 bisections, :1133) raise the context's numeric flag instead and leave the column.
__global__ void __launch_bounds__(256)
k_meke_equil(Dm d, const double *__restrict__ G, MekeK K, MekeVisc V, const double *__restrict__ SN_u, const double *__restrict__ SN_v,
             const double *__restrict__ I_mass, const double *__restrict__ depth_tot, const double *__restrict__ Rd_dx_h,
             const double *__restrict__ dF_dx, const double *__restrict__ dF_dy, double *__restrict__ MEKE, int *flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  const double SN = meke_SN_min(d, SN_u, SN_v, x);
  const double cd2 = K.cdrag2, D = depth_tot[x];
  if (K.equilibrium_alt) {
    const double t = K.GEOMETRIC_alpha * SN * D;
    MEKE[x] = (t * t) / cd2;
    return;
  }
  const double KhCoeff = K.KhCoeff, Ubg2 = K.Uscale * K.Uscale;
  const double tolerance = 1.0e-12 * (K.m_s_to_L_T * K.m_s_to_L_T);
  const double beta = K.old_lscale ? 0. : meke_beta(K, d, G, depth_tot, dF_dx, dF_dy, x);
  const double Im = I_mass[x];
  double EKE;
  if (KhCoeff * SN * Im > 0.) {
    const double area = gm(G, d, MOM6X_G_areaT)[x], Rd = Rd_dx_h ? Rd_dx_h[x] : 0.0;
    const double drv = meke_drag_rate_visc(d, G, V, x);
    double EKEmin = 0., ResMin = 0., EKEmax = 0.01 * (K.m_s_to_L_T * K.m_s_to_L_T);
    bool useSecant = false, debugIteration = false;
    double bottomFac2 = 0., barotrFac2 = 0., LmixScale = 0., LRhines = 0., LEady = 0.;
    double resid = 1.0;
    EKE = EKEmax;
    while (resid > 0.) {                                // :1070-1103
      EKE = EKEmax;
      meke_lscales_0d(K, area, beta, D, Rd, SN, EKE, bottomFac2, barotrFac2, LmixScale, LRhines, LEady);
      const double Kh = (KhCoeff * sqrt(2. * barotrFac2 * EKE) * LmixScale);
      const double src = Kh * (SN * SN);
      const double drag_rate = (K.H_to_RZ * Im) * sqrt(drv * drv + cd2 * (2.0 * bottomFac2 * EKE + Ubg2));
      const double ldamping = K.damping + drag_rate * bottomFac2;
      resid = src - ldamping * EKE;
      if (resid > 0.) {
        EKEmin = EKE;
        EKEmax = 10. * EKE;
        if (resid < ResMin) useSecant = true;
        ResMin = resid;
        if (EKEmax > 2.e17 * (K.m_s_to_L_T * K.m_s_to_L_T)) {
          if (debugIteration) { atomicOr(flag, MOM6X_FLAG_MEKE_EQUILIBRIUM); MEKE[x] = EKE; return; }
          debugIteration = true;
          resid = 1.;
          EKEmin = 0.; ResMin = 0.;
          EKEmax = 0.01 * (K.m_s_to_L_T * K.m_s_to_L_T);
          useSecant = false;
        }
      }
    }
    double ResMax = resid;
    int n2 = 0;
    double EKEerr = EKEmax - EKEmin;
    while (EKEerr > tolerance) {                        // :1108-1134
      n2 = n2 + 1;
      if (useSecant) EKE = EKEmin + (EKEmax - EKEmin) * (ResMin / (ResMin - ResMax));
      else EKE = 0.5 * (EKEmin + EKEmax);
      EKEerr = fmin1(EKE - EKEmin, EKEmax - EKE);
      const double Kh = (KhCoeff * sqrt(2. * barotrFac2 * EKE) * LmixScale);
      const double src = Kh * (SN * SN);
      const double drag_rate = (K.H_to_RZ * Im) * sqrt(drv * drv + cd2 * (2.0 * bottomFac2 * EKE + Ubg2));
      const double ldamping = K.damping + drag_rate * bottomFac2;
      resid = src - ldamping * EKE;
      if (useSecant && resid > ResMin) useSecant = false;
      if (resid > 0.) {
        EKEmin = EKE;
        if (resid < ResMin) useSecant = true;
        ResMin = resid;
      } else if (resid < 0.) {
        EKEmax = EKE;
        ResMax = resid;
      } else {
        break;
      }
      if (n2 > 200) { atomicOr(flag, MOM6X_FLAG_MEKE_EQUILIBRIUM); break; }
    }
  } else {
    EKE = 0.;
  }
  MEKE[x] = EKE;
}

// MEKE_lengthScales :1183-1253 and MEKE%Le :408-413 on the computational domain
__global__ void __launch_bounds__(256)
k_meke_lscale(Dm d, const double *__restrict__ G, MekeK K, const double *__restrict__ SN_u, const double *__restrict__ SN_v,
              const double *__restrict__ MEKE, const double *__restrict__ depth_tot, const double *__restrict__ Rd_dx_h,
              const double *__restrict__ dF_dx, const double *__restrict__ dF_dy, double *__restrict__ bottomFac2,
              double *__restrict__ barotrFac2, double *__restrict__ LmixScale, double *__restrict__ Le, double *__restrict__ LmixScale_out,
              double *__restrict__ LRhines_out, double *__restrict__ LEady_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  double SN = 0., beta = 0.;
  if (!K.old_lscale) {
    if (K.aEady > 0.) SN = 0.25 * ((SN_u[x] + SN_u[x - 1]) + (SN_v[x] + SN_v[x - (size_t)d.pitch]));
    beta = meke_beta(K, d, G, depth_tot, dF_dx, dF_dy, x);
  }
  double bf2, tf2, L, Lrh = 0., Led = 0.;
  meke_lscales_0d(K, gm(G, d, MOM6X_G_areaT)[x], beta, depth_tot[x], Rd_dx_h ? Rd_dx_h[x] : 0.0, SN, MEKE[x], bf2, tf2, L, Lrh, Led);
  bottomFac2[x] = bf2; barotrFac2[x] = tf2; LmixScale[x] = L;
  if (Le) Le[x] = L;
  if (LmixScale_out) LmixScale_out[x] = L;
  if (!K.old_lscale) {
    if (LRhines_out) LRhines_out[x] = Lrh;
    if (LEady_out) LEady_out[x] = Led;
  }
}

// the drag rate of :528-529 | :771-772
__device__ __forceinline__ double meke_drag_rate(const MekeK &K, double Im, double drv, double bf2, double M) {
  return (K.H_to_RZ * Im) * sqrt(drv * drv + K.cdrag2 * (fmax1(0.0, 2.0 * bf2 * M) + K.Uscale * K.Uscale));
}

// :329-357 and :415-606 on the computational domain
__global__ void __launch_bounds__(256)
k_meke_src(Dm d, const double *__restrict__ G, MekeK K, MekeVisc V, MekeSrc S, const double *__restrict__ SN_u,
           const double *__restrict__ SN_v, const double *__restrict__ I_mass, const double *__restrict__ depth_tot,
           const double *__restrict__ bottomFac2, double *__restrict__ MEKE, double *__restrict__ drv_out, double *__restrict__ cur_out,
           double *__restrict__ s1_out, MekeDiag D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  const double drv = meke_drag_rate_visc(d, G, V, x);
  drv_out[x] = drv;
  const double Im = I_mass[x], bf2 = bottomFac2[x];
  double src = K.BGsrc;
  double gmd = 0., lp = 0., bh = 0.;
  if (K.FrCoeff > 0.) src = src - K.FrCoeff * Im * S.mom_src[x];
  if (S.mom_src_bh) {
    src = src - K.bh_coeff * Im * S.mom_src_bh[x];
    if (D.src_mom_lp) lp = -K.FrCoeff * Im * (S.mom_src[x] - S.mom_src_bh[x]);
    if (D.src_mom_bh) bh = -K.bhFrCoeff * Im * S.mom_src_bh[x];
  }
  if (S.GME_snk) src = src - K.GMECoeff * Im * S.GME_snk[x];
  if (S.GM_src) {
    if (K.GM_src_alt) {
      src = src - K.GMcoeff * S.GM_src[x] / (K.H_to_RZ * fmax1(K.min_depth_tot, depth_tot[x]));
    } else {
      src = src - K.GMcoeff * Im * S.GM_src[x];
      gmd = -K.GMcoeff * Im * S.GM_src[x];
    }
  }
  double M = MEKE[x];
  if (K.restoring) {                                   // MEKE_equilibrium_restoring :1148-1178
    const double t = K.GEOMETRIC_alpha * meke_SN_min(d, SN_u, SN_v, x) * depth_tot[x];
    src = src - K.restoring_rate * (M - (t * t) / K.cdrag2);
  }
  if (D.src) D.src[x] = src;
  const double mask = gm(G, d, MOM6X_G_mask2dT)[x];
  const double cur = M;
  cur_out[x] = cur;
  M = (M + K.sdt * src) * mask;
  double drag_rate = 0.;
  if (K.use_drag_rate) drag_rate = meke_drag_rate(K, Im, drv, bf2, M);
  double damp_rate = K.damping + drag_rate * bf2;
  if (M < 0.) damp_rate = 0.;
  M = M / (1. + K.sdt_damp * damp_rate);
  MEKE[x] = M;
  double btm = 0.;
  if (K.any_s1) {
    const double damping = 1. / (1. + K.sdt_damp * damp_rate);
    if (D.decay) D.decay[x] = damp_rate * mask;
    gmd = gmd * damping; lp = lp * damping; bh = bh * damping;
    btm = -cur * (K.damp_step * (damp_rate * damping));
    if (D.src_btm_drag && K.split) s1_out[x] = damp_rate * damping;
  }
  if (D.src_GM) D.src_GM[x] = gmd;
  if (D.src_mom_lp) D.src_mom_lp[x] = lp;
  if (D.src_mom_bh) D.src_mom_bh[x] = bh;
  if (D.src_btm_drag) D.src_btm_drag[x] = btm;
  if (D.src_adv) D.src_adv[x] = 0.;
  if (D.src_mom_K4) D.src_mom_K4[x] = 0.;
}

// del2MEKE :617-642 at one cell (MEKE_uflux, MEKE_vflux as work space :620, :630)
__device__ __forceinline__ double meke_del2(const Dm &d, const double *__restrict__ G, const double *__restrict__ M, size_t x) {
  const size_t p = (size_t)d.pitch;
  const double *dy_Cu = gm(G, d, MOM6X_G_dy_Cu), *IdxCu = gm(G, d, MOM6X_G_IdxCu), *mu = gm(G, d, MOM6X_G_mask2dCu);
  const double *dx_Cv = gm(G, d, MOM6X_G_dx_Cv), *IdyCv = gm(G, d, MOM6X_G_IdyCv), *mv = gm(G, d, MOM6X_G_mask2dCv);
  const double c = M[x];
  const double uE = ((dy_Cu[x] * IdxCu[x]) * mu[x]) * (M[x + 1] - c);
  const double uW = ((dy_Cu[x - 1] * IdxCu[x - 1]) * mu[x - 1]) * (c - M[x - 1]);
  const double vN = ((dx_Cv[x] * IdyCv[x]) * mv[x]) * (M[x + p] - c);
  const double vS = ((dx_Cv[x - p] * IdyCv[x - p]) * mv[x - p]) * (c - M[x - p]);
  return gm(G, d, MOM6X_G_IareaT)[x] * ((uE - uW) + (vN - vS));
}

// :644-668 and :681-738 on the faces of face_lane<0>
__global__ void __launch_bounds__(256)
k_meke_flux(Dm d, const double *__restrict__ G, MekeK K, const double *__restrict__ MEKE, const double *__restrict__ mass,
            const double *__restrict__ Kh, const double *__restrict__ baroHu, const double *__restrict__ baroHv, double *__restrict__ uf,
            double *__restrict__ vf, double *__restrict__ uf4, double *__restrict__ vf4, double *__restrict__ Kh_u, double *__restrict__ Kh_v) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t x = f.x, y = f.y;
  const double r = dir ? (gm(G, d, MOM6X_G_dx_Cv)[x] * gm(G, d, MOM6X_G_IdyCv)[x]) : (gm(G, d, MOM6X_G_dy_Cu)[x] * gm(G, d, MOM6X_G_IdxCu)[x]);
  const double *IareaT = gm(G, d, MOM6X_G_IareaT);
  const double IA = fmax1(IareaT[x], IareaT[y]);
  const double mx = mass[x], my = mass[y];
  const double mh = (2.0 * mx * my) / ((mx + my) + K.mass_neglect);
  if (K.K4 >= 0.0) {
    double K4_here = K.K4;
    const double t = r * IA;
    const double Inv_K4_max = 64.0 * K.sdt * (t * t);
    if (K4_here * Inv_K4_max > 0.3) K4_here = 0.3 / Inv_K4_max;
    (dir ? vf4 : uf4)[x] = ((K4_here * r) * mh) * (meke_del2(d, G, MEKE, y) - meke_del2(d, G, MEKE, x));
  }
  if (K.kh_flux) {
    const double Mx = MEKE[x], My = MEKE[y];
    double Kh_here = fmax1(0., K.Kh);
    if (Kh) Kh_here = fmax1(0., K.Kh) + K.KhMEKE_Fac * 0.5 * (Kh[x] + Kh[y]);
    const double Inv_Kh_max = 2.0 * K.sdt * (r * IA);
    if (Kh_here * Inv_Kh_max > 0.25) Kh_here = 0.25 / Inv_Kh_max;
    double *Kd = dir ? Kh_v : Kh_u;
    if (Kd) Kd[x] = Kh_here;
    double fl = ((Kh_here * r) * mh) * (Mx - My);
    if (K.adv) {
      const double b = (dir ? baroHv : baroHu)[x];
      if (b > 0.) fl = fl + b * Mx * K.advFac;
      else if (b < 0.) fl = fl + b * My * K.advFac;
    }
    (dir ? vf : uf)[x] = fl;
  }
}

// :669-678, :740-849 and :870-875 on the computational domain
__global__ void __launch_bounds__(256)
k_meke_update(Dm d, const double *__restrict__ G, MekeK K, const double *__restrict__ I_mass, const double *__restrict__ bottomFac2,
              const double *__restrict__ drv_in, const double *__restrict__ cur_in, const double *__restrict__ s1_in,
              const double *__restrict__ uf, const double *__restrict__ vf, const double *__restrict__ uf4, const double *__restrict__ vf4,
              double *__restrict__ MEKE, MekeDiag D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), p = (size_t)d.pitch;
  const double Im = I_mass[x];
  const double a = gm(G, d, MOM6X_G_IareaT)[x] * Im;
  double M = MEKE[x];
  double del4 = 0., k4 = 0., adv = 0.;
  if (K.K4 >= 0.0) {
    const double div = (uf4[x - 1] - uf4[x]) + (vf4[x - p] - vf4[x]);
    del4 = (K.sdt * a) * div;
    k4 = a * div;
  }
  if (K.kh_flux) {
    const double div = (uf[x - 1] - uf[x]) + (vf[x - p] - vf[x]);
    M = M + (K.sdt * a) * div;
    adv = a * div;
  }
  if (K.K4 >= 0.0) M = M + del4;
  if (K.split) {                                       // the second stage of the Strang splitting :766-849
    const double bf2 = bottomFac2[x];
    double drag_rate = 0.;
    if (K.use_drag_rate) drag_rate = meke_drag_rate(K, Im, drv_in[x], bf2, M);
    double damp_rate = K.damping + drag_rate * bf2;
    if (M < 0.) damp_rate = 0.;
    M = M / (1. + K.sdt_damp * damp_rate);
    if (K.any_damp) {
      const double damping = 1. / (1. + K.sdt_damp * damp_rate);
      if (D.decay) D.decay[x] = damp_rate * gm(G, d, MOM6X_G_mask2dT)[x];
      if (D.src_GM) D.src_GM[x] = D.src_GM[x] * damping;
      if (D.src_mom_lp) D.src_mom_lp[x] = D.src_mom_lp[x] * damping;
      if (D.src_mom_bh) D.src_mom_bh[x] = D.src_mom_bh[x] * damping;
      adv = adv * damping;
      k4 = k4 * damping;
      if (D.src_btm_drag) D.src_btm_drag[x] = -cur_in[x] * (K.damp_step * ((damp_rate + s1_in[x]) * damping));
    }
  }
  if (D.src_adv && K.kh_flux) D.src_adv[x] = adv;
  if (D.src_mom_K4) D.src_mom_K4[x] = k4;
  if (K.positive) M = fmax1(0., M);
  MEKE[x] = M;
}

// :881-920 and :933-980 on the computational domain
__global__ void __launch_bounds__(256)
k_meke_diff(Dm d, const double *__restrict__ G, MekeK K, const double *__restrict__ MEKE, const double *__restrict__ bottomFac2,
            const double *__restrict__ barotrFac2, const double *__restrict__ LmixScale, const double *__restrict__ Rd_dx_h,
            double *__restrict__ Kh, double *__restrict__ Ku, double *__restrict__ Au, double *__restrict__ Ue, double *__restrict__ Ub,
            double *__restrict__ Ut, double *__restrict__ gamma_b, double *__restrict__ gamma_t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j);
  const double M = MEKE[x], bf2 = bottomFac2[x], tf2 = barotrFac2[x], L = LmixScale[x];
  if (K.KhCoeff > 0. && !K.GEOMETRIC) {
    if (K.old_lscale) {
      const double v = K.KhCoeff * sqrt(2. * fmax1(0., tf2 * M) * gm(G, d, MOM6X_G_areaT)[x]);
      if (K.Rd_as_max_scale) Kh[x] = v * fmin1(Rd_dx_h ? Rd_dx_h[x] : 0.0, 1.0);
      else Kh[x] = v;
    } else {
      Kh[x] = K.KhCoeff * sqrt(2. * fmax1(0., tf2 * M)) * L;
    }
  }
  if (K.Ku != 0.) Ku[x] = K.Ku * sqrt(2. * fmax1(0., M)) * L;
  if (K.Au != 0.) Au[x] = K.Au * sqrt(2. * fmax1(0., M)) * ((L * L) * L);
  if (Ue) Ue[x] = sqrt(fmax1(0., 2. * M));
  if (Ub) Ub[x] = sqrt(fmax1(0., 2. * M * bf2));
  if (Ut) Ut[x] = sqrt(fmax1(0., 2. * M * tf2));
  if (gamma_b) gamma_b[x] = sqrt(bf2);
  if (gamma_t) gamma_t[x] = sqrt(tf2);
}

}  // namespace

void MEKE_free(mom6x_ctx *c) {
  MekeState *s = c->meke;
  if (!s) return;
  (void)hipFree(s->dF_dx); (void)hipFree(s->dF_dy); (void)hipFree(s->work);
  delete s;
  c->meke = nullptr;
}

extern "C" int mom6x_MEKE_init(mom6x_ctx *c, const mom6x_MEKE_params *p, const double *dF_dx, const double *dF_dy) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_MEKE_init: null argument");
  REFUSE(p->eke_source_file, "MEKE_init", "EKE_SOURCE = file (time_interp_external)");
  REFUSE(p->eke_source_dbclient, "MEKE_init", "EKE_SOURCE = dbclient (the machine-learning inference)");
  REFUSE(p->use_Kh_diff, "MEKE_init", "USE_KH_IN_MEKE (MEKE%Kh_diff)");
  REFUSE(p->non_Boussinesq || !c->GV.Boussinesq, "MEKE_init", "non-Boussinesq mode (MEKE_TOTAL_DEPTH_RHO)");
  REFUSE(p->open_bcs, "MEKE_init", "open boundary conditions (G%OBCmaskCu, G%OBCmaskCv)");
  REFUSE(p->debug, "MEKE_init", "DEBUG (the checksums of step_forward_MEKE)");
  REQUIRE(p->use_old_lscale || (dF_dx && dF_dy), MOM6X_EINVAL, "MEKE_init: G%dF_dx and G%dF_dy are needed unless MEKE_OLD_LSCALE");
  REQUIRE(p->cdrag > 0., MOM6X_EINVAL, "MEKE_init: MEKE_CDRAG must be positive");
  REQUIRE(p->MEKE_dtScale > 0., MOM6X_EINVAL, "MEKE_init: MEKE_DTSCALE must be positive");
  REQUIRE(c->d.halo >= 1, MOM6X_EINVAL, "MEKE_init: step_forward_MEKE needs a halo of one");
  REQUIRE(p->MEKE_K4 < 0. || c->d.halo >= 2, MOM6X_EINVAL, "MEKE_init: MEKE_K4 >= 0 (the biharmonic of MEKE) needs a halo of two");
  HIPCHK(hipSetDevice(c->device));
  MEKE_free(c);
  MekeState *s = new MekeState();
  s->p = *p;
  s->initialize = !p->cold_start;                                          // :1720-1721
  s->kh_flux_enabled = (p->MEKE_Kh >= 0.0) || (p->KhMEKE_Fac > 0.0) || (p->MEKE_advection_factor > 0.0);   // :1617-1619
  s->dF_dx = s->dF_dy = s->work = nullptr;
  c->meke = s;
  const size_t n2 = (size_t)c->d.slab * sizeof(double);
  HIPCHK(hipMalloc(&s->work, MW_COUNT * n2));
  HIPCHK(hipMemsetAsync(s->work, work_fill_byte(), MW_COUNT * n2, c->stream));
  if (dF_dx && dF_dy) {
    HIPCHK(hipMalloc(&s->dF_dx, n2));
    HIPCHK(hipMalloc(&s->dF_dy, n2));
    HIPCHK(hipMemcpy(s->dF_dx, dF_dx, n2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->dF_dy, dF_dy, n2, hipMemcpyHostToDevice));
  }
  return MOM6X_OK;
}

extern "C" int mom6x_MEKE_set_initialized(mom6x_ctx *c, int initialized) {
  REQUIRE(c && c->meke, MOM6X_EINVAL, "MOM_MEKE: Module must be initialized before it is used.");
  c->meke->initialize = !initialized && !c->meke->p.cold_start;            // query_initialized(MEKE%MEKE) :1720-1721
  return MOM6X_OK;
}

extern "C" int mom6x_step_forward_MEKE(mom6x_ctx *c, double *MEKE, const double *h, const double *SN_u, const double *SN_v,
                                       const double *Kv_bbl_u, const double *Kv_bbl_v, const double *bbl_thick_u,
                                       const double *bbl_thick_v, double dt, const double *hu, const double *hv, const double *Rd_dx_h,
                                       const double *GM_src, const double *mom_src, const double *mom_src_bh, const double *GME_snk,
                                       double *Kh, double *Ku, double *Au, double *Le, double *src, double *src_adv, double *src_mom_K4,
                                       double *src_btm_drag, double *src_GM, double *src_mom_lp, double *src_mom_bh, double *decay,
                                       double *Kh_u, double *Kh_v, double *LmixScale, double *LRhines, double *LEady, double *Ue, double *Ub,
                                       double *Ut, double *gamma_b, double *gamma_t) {
  REQUIRE(c && c->meke, MOM6X_EINVAL, "MOM_MEKE: Module must be initialized before it is used.");
  MekeState *s = c->meke;
  const mom6x_MEKE_params &P = s->p;
  REQUIRE(MEKE && h && SN_u && SN_v, MOM6X_EINVAL, "step_forward_MEKE: null array (MEKE%MEKE, h, SN_u, SN_v)");
  REQUIRE(dt > 0., MOM6X_EINVAL, "step_forward_MEKE: dt must be positive");
  REQUIRE(!(P.MEKE_advection_factor > 0.) || (hu && hv), MOM6X_EINVAL, "step_forward_MEKE: hu and hv are needed with MEKE_ADVECTION_FACTOR > 0");
  REQUIRE(!(P.MEKE_FrCoeff > 0.) || mom_src, MOM6X_EINVAL, "step_forward_MEKE: MEKE%mom_src is needed with MEKE_FRCOEFF > 0");
  const bool geo = P.MEKE_GEOMETRIC != 0;
  REQUIRE(!(P.MEKE_KhCoeff > 0. && !geo) || Kh, MOM6X_EINVAL, "step_forward_MEKE: MEKE%Kh is needed with MEKE_KHCOEFF > 0");
  REQUIRE(P.viscosity_coeff_Ku == 0. || Ku, MOM6X_EINVAL, "step_forward_MEKE: MEKE%Ku is needed with MEKE_VISCOSITY_COEFF_KU");
  REQUIRE(P.viscosity_coeff_Au == 0. || Au, MOM6X_EINVAL, "step_forward_MEKE: MEKE%Au is needed with MEKE_VISCOSITY_COEFF_AU");
  // a diagnostic the reference does not register is not posted: the plane is left alone
  if (!(P.MEKE_K4 >= 0.)) src_mom_K4 = nullptr;        // :1653
  if (!(P.MEKE_GMcoeff >= 0.)) src_GM = nullptr;       // :1658
  if (!(P.MEKE_FrCoeff >= 0.)) src_mom_lp = nullptr;   // :1663
  if (!(P.MEKE_bhFrCoeff >= 0.)) src_mom_bh = nullptr; // :1668
  if (!s->kh_flux_enabled) { Kh_u = nullptr; Kh_v = nullptr; }   // :1702
  REQUIRE(!(src_mom_lp && mom_src_bh) || mom_src, MOM6X_EINVAL, "step_forward_MEKE: MEKE%mom_src is needed for MEKE_src_mom_lp");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_vgrid &GV = c->GV;

  MekeK K;
  K.damping = P.MEKE_damping; K.Cd_scale = P.MEKE_Cd_scale; K.Cb = P.MEKE_Cb; K.min_gamma = P.MEKE_min_gamma; K.Ct = P.MEKE_Ct;
  K.GMcoeff = P.MEKE_GMcoeff; K.GEOMETRIC = geo; K.GEOMETRIC_alpha = P.MEKE_GEOMETRIC_alpha;
  K.equilibrium_alt = P.MEKE_equilibrium_alt != 0; K.restoring = P.MEKE_equilibrium_restoring != 0; K.restoring_rate = P.MEKE_restoring_rate;
  K.FrCoeff = P.MEKE_FrCoeff; K.bhFrCoeff = P.MEKE_bhFrCoeff; K.GMECoeff = P.MEKE_GMECoeff; K.BGsrc = P.MEKE_BGsrc;
  K.bh_coeff = (P.MEKE_bhFrCoeff > 0. && P.MEKE_FrCoeff > 0.) ? P.MEKE_bhFrCoeff - P.MEKE_FrCoeff : P.MEKE_bhFrCoeff;   // :452-456
  K.Kh = P.MEKE_Kh; K.K4 = P.MEKE_K4; K.positive = P.MEKE_positive != 0; K.KhCoeff = P.MEKE_KhCoeff; K.Uscale = P.MEKE_Uscale;
  K.GM_src_alt = P.GM_src_alt != 0; K.min_depth_tot = P.MEKE_min_depth_tot; K.visc_drag = P.visc_drag != 0; K.KhMEKE_Fac = P.KhMEKE_Fac;
  K.old_lscale = P.use_old_lscale != 0; K.min_lscale = P.use_min_lscale != 0; K.lscale_maxval = P.lscale_maxval;
  K.Rd_as_max_scale = P.Rd_as_max_scale != 0; K.Ku = P.viscosity_coeff_Ku; K.Au = P.viscosity_coeff_Au; K.Lfixed = P.Lfixed;
  K.fixed_total_depth = P.fixed_total_depth != 0;
  K.aDeform = P.aDeform; K.aRhines = P.aRhines; K.aEady = P.aEady; K.aFrict = P.aFrict; K.aGrid = P.aGrid;
  K.topographic_beta = P.MEKE_topographic_beta; K.cdrag = P.cdrag; K.cdrag2 = P.cdrag * P.cdrag;                     // :291
  K.T_to_s = P.T_to_s; K.L_to_m = P.L_to_m; K.m_s_to_L_T = P.m_s_to_L_T;
  K.H_to_RZ = GV.H_to_RZ; K.RZ_to_H = GV.RZ_to_H; K.Z_to_H = GV.Z_to_H; K.h_neglect = GV.H_subroundoff;
  K.mass_neglect = GV.H_to_RZ * GV.H_subroundoff;                                                                    // :290
  K.sdt = dt * P.MEKE_dtScale;                                                                                       // :289
  K.split = (P.MEKE_Kh >= 0. || P.MEKE_K4 >= 0.);                                                                    // :295-297
  K.damp_step = K.split ? 0.5 : 1.;
  K.sdt_damp = K.sdt * K.damp_step;
  K.adv = P.MEKE_advection_factor > 0.; K.adv_bug = P.MEKE_advection_bug != 0;
  K.advFac = P.MEKE_advection_factor / K.sdt;                                                                        // :719
  K.use_drag_rate = (P.MEKE_Cd_scale > 0.0) || (P.MEKE_Cb > 0.) || P.visc_drag;                                      // :258
  K.kh_flux = s->kh_flux_enabled;
  K.any_s1 = src_GM || src_mom_lp || src_mom_bh || src_btm_drag;                                                     // :430-435
  K.any_damp = K.any_s1 || src_adv || src_mom_K4;                                                                    // :438-442

  MekeVisc V = { nullptr, nullptr, nullptr, nullptr };
  if (P.visc_drag && Kv_bbl_u && Kv_bbl_v && bbl_thick_u && bbl_thick_v) V = { Kv_bbl_u, Kv_bbl_v, bbl_thick_u, bbl_thick_v };   // :330
  const MekeSrc S = { GM_src, mom_src, mom_src_bh, GME_snk };
  const MekeDiag D = { src, src_adv, src_mom_K4, src_btm_drag, src_GM, src_mom_lp, src_mom_bh, decay };
  const size_t n2 = (size_t)d.slab;
  double *W = s->work;
  double *mass = W + MW_mass * n2, *I_mass = W + MW_Imass * n2, *depth_tot = W + MW_depth * n2, *baroHu = W + MW_baroHu * n2;
  double *baroHv = W + MW_baroHv * n2, *drv = W + MW_drv * n2, *bf2 = W + MW_bf2 * n2, *tf2 = W + MW_tf2 * n2, *Lmix = W + MW_Lmix * n2;
  double *cur = W + MW_cur * n2, *s1 = W + MW_s1 * n2, *uf = W + MW_uf * n2, *vf = W + MW_vf * n2, *uf4 = W + MW_uf4 * n2;
  double *vf4 = W + MW_vf4 * n2;
  const dim3 b = blk2();
  const dim3 gdom = grid3(d.ni, d.nj, 1, b);
  const int stg[4] = { 0, 0, 0, 0 }, nks[4] = { 1, 1, 1, 1 };
  c->halo_error = false;

  KLAUNCH(c, "k_meke_cols", k_meke_cols, grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, c->G, K, h, hu, hv, mass, I_mass, depth_tot, baroHu,
          baroHv);
  if (s->initialize) {                                                                                               // :390-393
    KLAUNCH(c, "k_meke_equil", k_meke_equil, gdom, b, d, c->G, K, V, SN_u, SN_v, (const double *)I_mass, (const double *)depth_tot, Rd_dx_h,
            (const double *)s->dF_dx, (const double *)s->dF_dy, MEKE, c->flag);
    s->initialize = false;
  }
  KLAUNCH(c, "k_meke_lscale", k_meke_lscale, gdom, b, d, c->G, K, SN_u, SN_v, (const double *)MEKE, (const double *)depth_tot, Rd_dx_h,
          (const double *)s->dF_dx, (const double *)s->dF_dy, bf2, tf2, Lmix, Le, LmixScale, LRhines, LEady);
  KLAUNCH(c, "k_meke_src", k_meke_src, gdom, b, d, c->G, K, V, S, SN_u, SN_v, (const double *)I_mass, (const double *)depth_tot,
          (const double *)bf2, MEKE, drv, cur, s1, D);
  const bool fluxes = s->kh_flux_enabled || P.MEKE_K4 >= 0.0;
  if (fluxes) {
    double *f[1] = { MEKE };
    halo_wrap(c, f, stg, nks, 1);                                                                                    // pass_MEKE :611
    KLAUNCH(c, "k_meke_flux", k_meke_flux, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, c->G, K, (const double *)MEKE, (const double *)mass,
            (const double *)Kh, (const double *)baroHu, (const double *)baroHv, uf, vf, uf4, vf4, Kh_u, Kh_v);
  }
  if (fluxes || K.split || K.positive)
    KLAUNCH(c, "k_meke_update", k_meke_update, gdom, b, d, c->G, K, (const double *)I_mass, (const double *)bf2, (const double *)drv,
            (const double *)cur, (const double *)s1, (const double *)uf, (const double *)vf, (const double *)uf4, (const double *)vf4, MEKE, D);
  {
    double *f[1] = { MEKE };
    halo_wrap(c, f, stg, nks, 1);                                                                                    // pass_MEKE :878
  }
  KLAUNCH(c, "k_meke_diff", k_meke_diff, gdom, b, d, c->G, K, (const double *)MEKE, (const double *)bf2, (const double *)tf2,
          (const double *)Lmix, Rd_dx_h, Kh, Ku, Au, Ue, Ub, Ut, gamma_b, gamma_t);
  {
    double *f[4];
    int n = 0;
    if (Kh) f[n++] = Kh;
    if (Ku) f[n++] = Ku;
    if (Au) f[n++] = Au;
    if (Le) f[n++] = Le;
    if (n) halo_wrap(c, f, stg, nks, n);                                                                             // pass_Kh :925
  }
  HIPCHK(hipGetLastError());
  REQUIRE(!c->halo_error, MOM6X_EHIP, mom6x_last_error());
  return MOM6X_OK;
}
