// pressure_force.hip -- finite-volume pressure-gradient force on gfx950.
//
//   PressureForce_FV_Bouss    <- MOM_PressureForce_FV.F90:947-2017
//     + Set_pbce_Bouss        <- MOM_PressureForce_Montgomery.F90:649-748
//
// "Column-walk" kernels: lane index = i (coalesced), one thread per column with sequential k.
#include "mom6x_dev.h"
#include "eos_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------
// PressureForce_FV_Bouss, pass 1: interface heights bottom-up (:1200-1202) on (-1..ni, -1..nj).
__global__ void __launch_bounds__(256)
k_pgf_e(Dm d, const double *__restrict__ G, const double *__restrict__ h, double *__restrict__ e, double H_to_Z) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni || j > d.nj) return;
  if (i < (-1)) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  double ek = -gm(G, d, MOM6X_G_bathyT)[x];
  e[x + (size_t)d.nk * slab] = ek;
  for (int k = d.nk - 1; k >= 0; k--) {
    ek = ek + h[x + (size_t)k * slab] * H_to_Z;
    e[x + (size_t)k * slab] = ek;
  }
}

// pass 2: top-down pressure anomalies and the accelerations (:1323-1345, :1539-1552, :1794-1813),
// Set_pbce_Bouss (no-EOS :735-746) and eta (:1886).
__global__ void __launch_bounds__(256)
k_pgf_main(Dm d, const double *__restrict__ G, const double *__restrict__ h, const double *__restrict__ e,
           const double *__restrict__ Rlay, const double *__restrict__ g_prime, double *__restrict__ PFu,
           double *__restrict__ PFv, double *__restrict__ pbce, double *__restrict__ eta, double g_Earth,
           double H_to_Z, double Z_to_H, double rho_ref, double GxRho_ref, double Z_ref, double I_Rho0,
           double h_neglect, double dz_neglect, BcFold B) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni || j > d.nj) return;
  if (i < (-1)) return;
  const int st = d.pitch, nz = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const bool do_u = (i <= d.ni - 1) && (j >= 0) && (j <= d.nj - 1);
  const bool do_v = (j <= d.nj - 1) && (i >= 0) && (i <= d.ni - 1);
  const double e_top = e[x], e_bot = e[x + (size_t)nz * slab];
  if (eta) eta[x] = e_top * Z_to_H;
  const double Ihtot = 1.0 / ((e_top - e_bot) + dz_neglect);
  double pa0 = GxRho_ref * (e_top - Z_ref), pa1 = 0.0, pa2 = 0.0, intx_pa = 0.0, inty_pa = 0.0;
  double cu = 0.0, cv = 0.0;
  if (do_u) { pa1 = GxRho_ref * (e[x + 1] - Z_ref); intx_pa = 0.5 * (pa0 + pa1); cu = (2.0 * I_Rho0 * gm(G, d, MOM6X_G_IdxCu)[x]); }
  if (do_v) { pa2 = GxRho_ref * (e[x + st] - Z_ref); inty_pa = 0.5 * (pa0 + pa2); cv = (2.0 * I_Rho0 * gm(G, d, MOM6X_G_IdyCv)[x]); }
  double pb = 0.0;
  // bt_mass_source's eta_h (MOM_barotropic.F90:5268-5272: h summed from the top, less the depth) of the same h, while it passes
  const bool do_eh = (B.eta_h != nullptr) && i >= 0 && i <= d.ni - 1 && j >= 0 && j <= d.nj - 1;
  double eta_h = 0.0;
  for (int k = 0; k < nz; k++) {
    const size_t c = x + (size_t)k * slab, cb = c + slab;
    const double R = Rlay[k] - rho_ref;
    const double h0 = h[c];
    if (do_eh) eta_h = (k == 0) ? (h0 - gm(G, d, MOM6X_G_bathyT)[x] * Z_to_H) : (eta_h + h0);
    const double dz0 = g_Earth * H_to_Z * h0;
    const double dpa0 = R * dz0, iz0 = 0.5 * R * dz0 * h0;
    const double eb0 = e[cb];
    if (do_u) {
      const double h1 = h[c + 1];
      const double dz1 = g_Earth * H_to_Z * h1;
      const double iz1 = 0.5 * R * dz1 * h1;
      const double intx_dpa = 0.5 * R * (dz0 + dz1);
      const double pf = (((pa0 * h0 + iz0) - (pa1 * h1 + iz1)) + ((h1 - h0) * intx_pa - (e[cb + 1] - eb0) * intx_dpa * Z_to_H)) *
                        (cu / ((h0 + h1) + h_neglect));
      PFu[c] = pf;
      if (B.u_bc) B.u_bc[c] = (B.CAu[c] + pf) + B.diffu[c];   // u_bc_accel of the predictor (RK2.F90:565-572) while PFu is at hand
      pa1 = pa1 + R * dz1;
      intx_pa = intx_pa + intx_dpa;
    }
    if (do_v) {
      const double h2 = h[c + st];
      const double dz2 = g_Earth * H_to_Z * h2;
      const double iz2 = 0.5 * R * dz2 * h2;
      const double inty_dpa = 0.5 * R * (dz0 + dz2);
      const double pf = (((pa0 * h0 + iz0) - (pa2 * h2 + iz2)) + ((h2 - h0) * inty_pa - (e[cb + st] - eb0) * inty_dpa * Z_to_H)) *
                        (cv / ((h0 + h2) + h_neglect));
      PFv[c] = pf;
      if (B.v_bc) B.v_bc[c] = (B.CAv[c] + pf) + B.diffv[c];
      pa2 = pa2 + R * dz2;
      inty_pa = inty_pa + inty_dpa;
    }
    pa0 = pa0 + dpa0;
    if (pbce) {
      if (k == 0) pb = g_prime[0] * H_to_Z;
      else pb = pb + (g_prime[k] * H_to_Z) * ((e[c] - e_bot) * Ihtot);
      pbce[c] = pb;
    }
  }
  if (do_eh) B.eta_h[x] = eta_h;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// PressureForce_FV_Bouss with an equation of state (:1206, :1289-1316): analytic_int_density_dz
// (MOM_EOS.F90:1384) for EOS_LINEAR (MOM_EOS_linear.F90:275-475) and EOS_WRIGHT (MOM_EOS_Wright.F90:389-655),
// and the use_EOS branch of Set_pbce_Bouss (MOM_PressureForce_Montgomery.F90:704-733).
struct EosDev { int form; double Rho_T0_S0, dRho_dT, dRho_dS, dRho_dp; int do_mw, top_mw, ssh_z0; int van_only; double dz_nv; };

namespace {

// dpa and intz_dpa of one cell (the first loop of int_density_dz_linear :373-384 / _wright :554-577)
template <int FORM>
__device__ __forceinline__ void cell_int(const EosDev &E, double rho_ref, double G_e, double GxRho, double I_Rho, double T,
                                         double S, double zt, double zb, double z0, double &dpa, double &intz) {
  const double dz = zt - zb;
  const double p_ave = -GxRho * (0.5 * (zt + zb) - z0);
  if (FORM == MOM6X_EOS_LINEAR) {
    const double C1_6 = 1.0 / 6.0;
    const double rho_anom = (E.Rho_T0_S0 - rho_ref) + E.dRho_dT * T + E.dRho_dS * S + E.dRho_dp * p_ave;
    dpa = G_e * rho_anom * dz;
    intz = 0.5 * G_e * (rho_anom - C1_6 * E.dRho_dp * (GxRho * dz)) * (dz * dz);
  } else {
    const double C1_3 = 1.0 / 3.0, C1_7 = 1.0 / 7.0, C1_9 = 1.0 / 9.0;
    double al0, p0, lambda;
    wright_coefs<FORM>(T, S, al0, p0, lambda);
    const double I_al0 = 1.0 / al0;
    if (FORM == MOM6X_EOS_WRIGHT) {   // int_density_dz_wright, MOM_EOS_Wright.F90:554-577
      const double I_Lzz = 1.0 / (p0 + (lambda * I_al0) + p_ave);
      const double eps = 0.5 * GxRho * dz * I_Lzz, eps2 = eps * eps;
      const double rho_anom = (p0 + p_ave) * (I_Lzz * I_al0) - rho_ref;
      const double rem = I_Rho * (lambda * (I_al0 * I_al0)) * eps2 * (C1_3 + eps2 * (0.2 + eps2 * (C1_7 + C1_9 * eps2)));
      dpa = 1.0 * (G_e * rho_anom * dz - 2.0 * eps * rem);
      intz = 1.0 * (0.5 * G_e * rho_anom * (dz * dz) - dz * (1.0 + eps) * rem);
    } else {                          // int_density_dz_wright_full / _red, MOM_EOS_Wright_full.F90:550-572
      const double I_Lzz = 1.0 / ((p0 + p_ave) + lambda * I_al0);
      const double eps = 0.5 * (GxRho * dz) * I_Lzz, eps2 = eps * eps;
      const double rho_anom = (p0 + p_ave) * (I_Lzz * I_al0) - rho_ref;
      const double rem = (I_Rho * (lambda * (I_al0 * I_al0))) * (eps2 * (C1_3 + eps2 * (0.2 + eps2 * (C1_7 + C1_9 * eps2))));
      dpa = 1.0 * ((G_e * rho_anom) * dz - 2.0 * eps * rem);
      intz = 1.0 * (0.5 * (G_e * rho_anom) * (dz * dz) - dz * ((1.0 + eps) * rem));
    }
  }
}

// intx_dpa | inty_dpa of the face between columns L and R (:386-430 / :560-607)
template <int FORM>
__device__ __forceinline__ double face_int(const EosDev &E, double rho_ref, double G_e, double GxRho, double I_Rho, double TL,
                                           double SL, double TR, double SR, double ztL, double zbL, double ztR, double zbR,
                                           double z0L, double z0R, double bathyL, double bathyR, double sshL, double sshR,
                                           double dz_neglect, double dpaL, double dpaR) {
  const double C1_90 = 1.0 / 90.0;
  double hWght = 0.0;
  if (E.do_mw) hWght = dmax(dmax(0., -bathyL - ztR), -bathyR - ztL);
  if (E.top_mw) hWght = dmax(dmax(hWght, zbR - sshL), zbL - sshR);
  if (FORM == MOM6X_EOS_LINEAR && hWght <= 0.0) {
    const double C1_6 = 1.0 / 6.0;
    const double dzL = ztL - zbL, dzR = ztR - zbR;
    double p_ave = -GxRho * (0.5 * (ztL + zbL) - z0L);
    const double raL = (E.Rho_T0_S0 - rho_ref) + ((E.dRho_dT * TL + E.dRho_dS * SL) + E.dRho_dp * p_ave);
    p_ave = -GxRho * (0.5 * (ztR + zbR) - z0R);
    const double raR = (E.Rho_T0_S0 - rho_ref) + ((E.dRho_dT * TR + E.dRho_dS * SR) + E.dRho_dp * p_ave);
    return G_e * C1_6 * ((dzL * (2.0 * raL + raR)) + (dzR * (2.0 * raR + raL)));
  }
  double LL = 1.0, LR = 0.0, RR = 1.0, RL = 0.0;
  if (hWght > 0.) {
    const double hL = (ztL - zbL) + dz_neglect, hR = (ztR - zbR) + dz_neglect;
    const double q = (hL - hR) / (hL + hR);
    hWght = hWght * (q * q);
    const double iDenom = 1.0 / (hWght * (hR + hL) + hL * hR);
    LL = (hWght * hL + hR * hL) * iDenom; LR = (hWght * hR) * iDenom;
    RR = (hWght * hR + hR * hL) * iDenom; RL = (hWght * hL) * iDenom;
  }
  double al0L = 0., p0L = 0., lamL = 0., al0R = 0., p0R = 0., lamR = 0.;
  if (FORM != MOM6X_EOS_LINEAR) { wright_coefs<FORM>(TL, SL, al0L, p0L, lamL); wright_coefs<FORM>(TR, SR, al0R, p0R, lamR); }
  double intz[5];
  intz[0] = dpaL; intz[4] = dpaR;
#pragma unroll
  for (int m = 2; m <= 4; m++) {
    const double wt_L = 0.25 * (double)(5 - m), wt_R = 1.0 - wt_L;
    const double wtT_L = (wt_L * LL) + (wt_R * RL), wtT_R = (wt_L * LR) + (wt_R * RR);
    const double dz = (wt_L * (ztL - zbL)) + (wt_R * (ztR - zbR));
    const double p_ave = -GxRho * ((wt_L * (0.5 * (ztL + zbL) - z0L)) + (wt_R * (0.5 * (ztR + zbR) - z0R)));
    if (FORM == MOM6X_EOS_LINEAR) {
      const double rho_anom = (E.Rho_T0_S0 - rho_ref) +
                              ((E.dRho_dT * ((wtT_L * TL) + (wtT_R * TR)) + E.dRho_dS * ((wtT_L * SL) + (wtT_R * SR))) + E.dRho_dp * p_ave);
      intz[m - 1] = G_e * rho_anom * dz;
    } else {
      const double C1_3 = 1.0 / 3.0, C1_7 = 1.0 / 7.0, C1_9 = 1.0 / 9.0;
      const double al0 = (wtT_L * al0L) + (wtT_R * al0R);
      const double p0 = (wtT_L * p0L) + (wtT_R * p0R);
      const double lambda = (wtT_L * lamL) + (wtT_R * lamR);
      const double I_al0 = 1.0 / al0;
      if (FORM == MOM6X_EOS_WRIGHT) {   // MOM_EOS_Wright.F90:601-605
        const double I_Lzz = 1.0 / (p0 + (lambda * I_al0) + p_ave);
        const double eps = 0.5 * GxRho * dz * I_Lzz, eps2 = eps * eps;
        intz[m - 1] = 1.0 * (G_e * dz * ((p0 + p_ave) * (I_Lzz * I_al0) - rho_ref) - 2.0 * eps *
                             I_Rho * (lambda * (I_al0 * I_al0)) * eps2 * (C1_3 + eps2 * (0.2 + eps2 * (C1_7 + C1_9 * eps2))));
      } else {                          // MOM_EOS_Wright_full.F90:606-610
        const double I_Lzz = 1.0 / ((p0 + p_ave) + lambda * I_al0);
        const double eps = 0.5 * (GxRho * dz) * I_Lzz, eps2 = eps * eps;
        intz[m - 1] = 1.0 * ((G_e * dz) * ((p0 + p_ave) * (I_Lzz * I_al0) - rho_ref) - 2.0 * eps *
                             (I_Rho * (lambda * (I_al0 * I_al0))) * (eps2 * (C1_3 + eps2 * (0.2 + eps2 * (C1_7 + C1_9 * eps2)))));
      }
    }
  }
  return C1_90 * (7.0 * (intz[0] + intz[4]) + 32.0 * (intz[1] + intz[3]) + 12.0 * intz[2]);
}


// ---- use_ALE with PRESSURE_RECONSTRUCTION_SCHEME = 1 (PressureForce_FV.F90:1235-1236, :1287-1296) ---------------------
// density_anomaly_elem_linear (MOM_EOS_linear.F90:74-84) / density_anomaly_elem_buggy_Wright (MOM_EOS_Wright.F90:101-129):
// calculate_density(..., rho_ref=rho_ref) of the quadratures of int_density_dz_generic_plm
template <int FORM>
__device__ __forceinline__ double density_anomaly(const EosDev &E, double T, double S, double pressure, double rho_ref) {
  if (FORM == MOM6X_EOS_LINEAR)
    return (E.Rho_T0_S0 - rho_ref) + ((E.dRho_dT * T + E.dRho_dS * S) + E.dRho_dp * pressure);
  if (FORM == MOM6X_EOS_UNESCO) return unesco::density_anomaly(T, S, pressure, rho_ref);
  if (FORM == MOM6X_EOS_ROQUET_RHO) return roquet::roquet_density_anomaly(T, S, pressure, rho_ref);
  if (FORM == MOM6X_EOS_JACKETT06) return jackett::jackett_density_anomaly(T, S, pressure, rho_ref);
  if (FORM == MOM6X_EOS_ROQUET_SPV) return roquet::roquet_spv_density_anomaly(T, S, pressure, rho_ref);
  typedef WC<FORM> W;   // the same expression in MOM_EOS_Wright.F90:119-128, _full.F90:108-119, _red.F90:108-119
  const double pa_000 = (W::b0 * (1.0 - W::a0 * rho_ref) - rho_ref * W::c0);
  const double al_TS = W::a1 * T + W::a2 * S;
  const double al0 = W::a0 + al_TS;
  const double p_TSp = pressure + (W::b4 * S + T * (W::b1 + (T * (W::b2 + W::b3 * T) + W::b5 * S)));
  const double lam_TS = W::c4 * S + T * (W::c1 + (T * (W::c2 + W::c3 * T) + W::c5 * S));
  return (pa_000 + (p_TSp - rho_ref * (p_TSp * al0 + (W::b0 * al_TS + lam_TS)))) / ((W::c0 + lam_TS) + al0 * (W::b0 + p_TSp));
}

// section 1 of int_density_dz_generic_plm (MOM_density_integrals.F90:587-637): dpa and intz_dpa of one cell by Boole's rule
// MODE 1: linear T, S between the edge values (int_density_dz_generic_plm); 2: parabolic through the edge values and the mean
// (int_density_dz_generic_ppm :1047-1073); 3: the layer mean (int_density_dz_generic_pcm :243-262)
template <int FORM, int MODE>
__device__ __forceinline__ void cell_int_plm(const EosDev &E, double rho_ref, double G_e, double GxRho, double Tt, double Tb,
                                             double St, double Sb, double zt, double zb, double z0, double &dpa, double &intz,
                                             double Tm = 0., double Sm = 0.) {
  const double C1_90 = 1.0 / 90.0;
  const double dz = zt - zb;
  double r5[6];
  double s6 = 0., t6 = 0.;
  if (MODE == 2) { s6 = 3.0 * (2.0 * Sm - (St + Sb)); t6 = 3.0 * (2.0 * Tm - (Tt + Tb)); }
#pragma unroll
  for (int n = 1; n <= 5; n++) {
    const double wt_t = 0.25 * (double)(5 - n), wt_b = 1.0 - wt_t;
    const double p5 = -GxRho * ((zt - z0) - 0.25 * (double)(n - 1) * dz);
    double S5, T5;
    if (MODE == 2) { S5 = wt_t * St + wt_b * (Sb + s6 * wt_t); T5 = wt_t * Tt + wt_b * (Tb + t6 * wt_t); }
    else if (MODE == 3) { S5 = Sm; T5 = Tm; }
    else { S5 = wt_t * St + wt_b * Sb; T5 = wt_t * Tt + wt_b * Tb; }
    r5[n] = density_anomaly<FORM>(E, T5, S5, p5, rho_ref);
  }
  const double rho_anom = C1_90 * (7.0 * (r5[1] + r5[5]) + 32.0 * (r5[2] + r5[4]) + 12.0 * r5[3]);
  dpa = G_e * dz * rho_anom;
  intz = 0.5 * G_e * (dz * dz) * (rho_anom - C1_90 * (16.0 * (r5[4] - r5[2]) + 7.0 * (r5[5] - r5[1])));
}

// sections 2 / 3 (:640-742 / :745-868): intx_dpa | inty_dpa of the face between columns L and R
template <int FORM>
__device__ __forceinline__ double face_int_plm(const EosDev &E, double rho_ref, double G_e, double GxRho, double dz_subroundoff,
                                               double TtL, double TbL, double StL, double SbL, double TtR, double TbR, double StR,
                                               double SbR, double ztL, double zbL, double ztR, double zbR, double z0L, double z0R,
                                               double bathyL, double bathyR, double sshL, double sshR, double dpaL, double dpaR) {
  const double C1_90 = 1.0 / 90.0;
  const double mwT = E.do_mw ? 1. : 0., topT = E.top_mw ? 1. : 0., nvT = E.van_only ? 0. : 1.;
  double hWght = mwT * dmax(dmax(0., -bathyL - ztR), -bathyR - ztL);
  const double hWghtTop = topT * dmax(dmax(0., zbR - sshL), zbL - sshR);
  hWght = dmax(hWght, hWghtTop);
  if (((ztL - zbL) > E.dz_nv) && ((ztR - zbR) > E.dz_nv)) hWght = nvT * hWght;
  double Ttl = TtL, Tbl = TbL, Ttr = TtR, Tbr = TbR, Stl = StL, Sbl = SbL, Str = StR, Sbr = SbR;
  if (hWght > 0.) {
    const double hL = (ztL - zbL) + dz_subroundoff, hR = (ztR - zbR) + dz_subroundoff;
    const double q = (hL - hR) / (hL + hR);
    hWght = hWght * (q * q);
    const double iDenom = 1. / (hWght * (hR + hL) + hL * hR);
    Ttl = ((hWght * hR) * TtR + (hWght * hL + hR * hL) * TtL) * iDenom;
    Ttr = ((hWght * hL) * TtL + (hWght * hR + hR * hL) * TtR) * iDenom;
    Tbl = ((hWght * hR) * TbR + (hWght * hL + hR * hL) * TbL) * iDenom;
    Tbr = ((hWght * hL) * TbL + (hWght * hR + hR * hL) * TbR) * iDenom;
    Stl = ((hWght * hR) * StR + (hWght * hL + hR * hL) * StL) * iDenom;
    Str = ((hWght * hL) * StL + (hWght * hR + hR * hL) * StR) * iDenom;
    Sbl = ((hWght * hR) * SbR + (hWght * hL + hR * hL) * SbL) * iDenom;
    Sbr = ((hWght * hL) * SbL + (hWght * hR + hR * hL) * SbR) * iDenom;
  }
  double intz[6];
  intz[1] = dpaL; intz[5] = dpaR;
#pragma unroll
  for (int m = 2; m <= 4; m++) {
    const double w_left = 0.25 * (double)(5 - m), w_right = 1.0 - w_left;
    const double dz_x = (w_left * (ztL - zbL)) + (w_right * (ztR - zbR));
    double T15[6], S15[6], p15[6], r15[6];
    T15[1] = (w_left * Ttl) + (w_right * Ttr); T15[5] = (w_left * Tbl) + (w_right * Tbr);
    S15[1] = (w_left * Stl) + (w_right * Str); S15[5] = (w_left * Sbl) + (w_right * Sbr);
    p15[1] = -GxRho * ((w_left * (ztL - z0L)) + (w_right * (ztR - z0R)));
#pragma unroll
    for (int n = 2; n <= 5; n++) p15[n] = p15[n - 1] + GxRho * 0.25 * dz_x;
#pragma unroll
    for (int n = 2; n <= 4; n++) {
      const double wt_t = 0.25 * (double)(5 - n), wt_b = 1.0 - wt_t;
      S15[n] = wt_t * S15[1] + wt_b * S15[5];
      T15[n] = wt_t * T15[1] + wt_b * T15[5];
    }
#pragma unroll
    for (int n = 1; n <= 5; n++) r15[n] = density_anomaly<FORM>(E, T15[n], S15[n], p15[n], rho_ref);
    intz[m] = (G_e * dz_x * (C1_90 * (7.0 * (r15[1] + r15[5]) + 32.0 * (r15[2] + r15[4]) + 12.0 * r15[3])));
  }
  return C1_90 * (7.0 * (intz[1] + intz[5]) + 32.0 * (intz[2] + intz[4]) + 12.0 * intz[3]);
}

// sections 2 / 3 of int_density_dz_generic_ppm (:1075-1183 / :1186-1308): the face between columns L and R, T and S parabolic in
// the vertical through the (thickness-weighted) top, mean and bottom values
template <int FORM>
__device__ __forceinline__ double face_int_ppm(const EosDev &E, double rho_ref, double G_e, double GxRho, double dz_subroundoff,
                                               double TtL, double TbL, double TmL, double StL, double SbL, double SmL, double TtR,
                                               double TbR, double TmR, double StR, double SbR, double SmR, double ztL, double zbL,
                                               double ztR, double zbR, double z0L, double z0R, double bathyL, double bathyR,
                                               double sshL, double sshR, double dpaL, double dpaR) {
  const double C1_90 = 1.0 / 90.0;
  const double mwT = E.do_mw ? 1. : 0., topT = E.top_mw ? 1. : 0., nvT = E.van_only ? 0. : 1.;
  double hWght = mwT * dmax(dmax(0., -bathyL - ztR), -bathyR - ztL);
  const double hWghtTop = topT * dmax(dmax(0., zbR - sshL), zbL - sshR);
  hWght = dmax(hWght, hWghtTop);
  if (((ztL - zbL) > E.dz_nv) && ((ztR - zbR) > E.dz_nv)) hWght = nvT * hWght;
  double Ttl = TtL, Tbl = TbL, Tml = TmL, Ttr = TtR, Tbr = TbR, Tmr = TmR;
  double Stl = StL, Sbl = SbL, Sml = SmL, Str = StR, Sbr = SbR, Smr = SmR;
  if (hWght > 0.) {
    const double hL = (ztL - zbL) + dz_subroundoff, hR = (ztR - zbR) + dz_subroundoff;
    const double q = (hL - hR) / (hL + hR);
    hWght = hWght * (q * q);
    const double iDenom = 1. / (hWght * (hR + hL) + hL * hR);
    const double wR = (hWght * hR), wLL = (hWght * hL + hR * hL), wL = (hWght * hL), wRR = (hWght * hR + hR * hL);
    Ttl = (wR * TtR + wLL * TtL) * iDenom; Tbl = (wR * TbR + wLL * TbL) * iDenom; Tml = (wR * TmR + wLL * TmL) * iDenom;
    Ttr = (wL * TtL + wRR * TtR) * iDenom; Tbr = (wL * TbL + wRR * TbR) * iDenom; Tmr = (wL * TmL + wRR * TmR) * iDenom;
    Stl = (wR * StR + wLL * StL) * iDenom; Sbl = (wR * SbR + wLL * SbL) * iDenom; Sml = (wR * SmR + wLL * SmL) * iDenom;
    Str = (wL * StL + wRR * StR) * iDenom; Sbr = (wL * SbL + wRR * SbR) * iDenom; Smr = (wL * SmL + wRR * SmR) * iDenom;
  }
  double intz[6];
  intz[1] = dpaL; intz[5] = dpaR;
#pragma unroll
  for (int m = 2; m <= 4; m++) {
    const double w_left = 0.25 * (double)(5 - m), w_right = 1.0 - w_left;
    const double T_top = (w_left * Ttl) + (w_right * Ttr), T_mn = (w_left * Tml) + (w_right * Tmr), T_bot = (w_left * Tbl) + (w_right * Tbr);
    const double S_top = (w_left * Stl) + (w_right * Str), S_mn = (w_left * Sml) + (w_right * Smr), S_bot = (w_left * Sbl) + (w_right * Sbr);
    const double dz_x = (w_left * (ztL - zbL)) + (w_right * (ztR - zbR));
    double p15[6], r15[6];
    p15[1] = -GxRho * ((w_left * (ztL - z0L)) + (w_right * (ztR - z0R)));
#pragma unroll
    for (int n = 2; n <= 5; n++) p15[n] = p15[n - 1] + GxRho * 0.25 * dz_x;
    const double s6 = 3.0 * (2.0 * S_mn - (S_top + S_bot)), t6 = 3.0 * (2.0 * T_mn - (T_top + T_bot));
#pragma unroll
    for (int n = 1; n <= 5; n++) {
      const double wt_t = 0.25 * (double)(5 - n), wt_b = 1.0 - wt_t;
      const double S15 = wt_t * S_top + wt_b * (S_bot + s6 * wt_t);
      const double T15 = wt_t * T_top + wt_b * (T_bot + t6 * wt_t);
      r15[n] = density_anomaly<FORM>(E, T15, S15, p15[n], rho_ref);
    }
    intz[m] = (G_e * dz_x * (C1_90 * (7.0 * (r15[1] + r15[5]) + 32.0 * (r15[2] + r15[4]) + 12.0 * r15[3])));
  }
  return C1_90 * (7.0 * (intz[1] + intz[5]) + 32.0 * (intz[2] + intz[4]) + 12.0 * intz[3]);
}

// int_density_dz_generic_pcm (EOS_QUADRATURE), :265-339 / :342-414: layer-mean T, S carried across the face with the
// (possibly thickness-weighted) weights hWt_LL ... hWt_RL
template <int FORM>
__device__ __forceinline__ double face_int_pcm(const EosDev &E, double rho_ref, double G_e, double GxRho, double dz_neglect, double TL,
                                               double SL, double TR, double SR, double ztL, double zbL, double ztR, double zbR, double z0L,
                                               double z0R, double bathyL, double bathyR, double sshL, double sshR, double dpaL,
                                               double dpaR) {
  const double C1_90 = 1.0 / 90.0;
  const double nvT = E.van_only ? 0. : 1.;
  double hWght = 0.0;
  if (E.do_mw) hWght = dmax(dmax(0., -bathyL - ztR), -bathyR - ztL);
  if (E.top_mw) hWght = dmax(dmax(hWght, zbR - sshL), zbL - sshR);
  if (((ztL - zbL) > E.dz_nv) && ((ztR - zbR) > E.dz_nv)) hWght = nvT * hWght;
  double hWt_LL = 1.0, hWt_LR = 0.0, hWt_RR = 1.0, hWt_RL = 0.0;
  if (hWght > 0.) {
    const double hL = (ztL - zbL) + dz_neglect, hR = (ztR - zbR) + dz_neglect;
    const double q = (hL - hR) / (hL + hR);
    hWght = hWght * (q * q);
    const double iDenom = 1.0 / (hWght * (hR + hL) + hL * hR);
    hWt_LL = (hWght * hL + hR * hL) * iDenom; hWt_LR = (hWght * hR) * iDenom;
    hWt_RR = (hWght * hR + hR * hL) * iDenom; hWt_RL = (hWght * hL) * iDenom;
  }
  double intz[6];
  intz[1] = dpaL; intz[5] = dpaR;
#pragma unroll
  for (int m = 2; m <= 4; m++) {
    const double wt_L = 0.25 * (double)(5 - m), wt_R = 1.0 - wt_L;
    const double wtT_L = (wt_L * hWt_LL) + (wt_R * hWt_RL), wtT_R = (wt_L * hWt_LR) + (wt_R * hWt_RR);
    const double dz_x = (wt_L * (ztL - zbL)) + (wt_R * (ztR - zbR));
    const double T15 = (wtT_L * TL) + (wtT_R * TR), S15 = (wtT_L * SL) + (wtT_R * SR);
    double p15[6], r15[6];
    p15[1] = -GxRho * ((wt_L * (ztL - z0L)) + (wt_R * (ztR - z0R)));
#pragma unroll
    for (int n = 2; n <= 5; n++) p15[n] = p15[n - 1] + GxRho * 0.25 * dz_x;
#pragma unroll
    for (int n = 1; n <= 5; n++) r15[n] = density_anomaly<FORM>(E, T15, S15, p15[n], rho_ref);
    intz[m] = (G_e * dz_x * (C1_90 * (7.0 * (r15[1] + r15[5]) + 32.0 * (r15[2] + r15[4]) + 12.0 * r15[3])));
  }
  return C1_90 * (7.0 * (intz[1] + intz[5]) + 32.0 * (intz[2] + intz[4]) + 12.0 * intz[3]);
}

// One thread per (i,j) column, top-down like k_pgf_main; the integrals of the east and north neighbours are
// recomputed by this thread (no 3-D dpa / intz_dpa / intx_dpa arrays).  PLM: the T, S edge values of TS_PLM_edge_values
// (Tt, Tb, St, Sb) and the generic quadratures instead of the layer means and the analytic integrals.
template <int FORM, int MODE>   // MODE 0: analytic integrals; 1: PLM; 2: PPM; 3: layer means by quadrature (EOS_QUADRATURE)
__global__ void __launch_bounds__(256)
k_pgf_main_eos(Dm d, const double *__restrict__ G, const double *__restrict__ h, const double *__restrict__ e,
               const double *__restrict__ Tv, const double *__restrict__ Sv, const double *__restrict__ Tt,
               const double *__restrict__ Tb, const double *__restrict__ St, const double *__restrict__ Sb, EosDev E,
               double *__restrict__ PFu,
               double *__restrict__ PFv, double *__restrict__ pbce, double *__restrict__ eta, double g_Earth, double H_to_Z,
               double Z_to_H, double rho_ref, double GxRho_ref, double Z_ref, double Rho0, double rho0_alt, double h_neglect,
               double dz_neglect, BcFold B) {
  const int i = I_BASE(-1) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni || j > d.nj) return;
  if (i < (-1)) return;
  const int st = d.pitch, nz = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const bool do_u = (i <= d.ni - 1) && (j >= 0) && (j <= d.nj - 1);
  const bool do_v = (j <= d.nj - 1) && (i >= 0) && (i <= d.ni - 1);
  const double *bathyT = gm(G, d, MOM6X_G_bathyT);
  const double I_Rho0 = 1.0 / Rho0;
  const double G_e = g_Earth, GxRho = G_e * rho0_alt, I_Rho = 1.0 / rho0_alt;   // rho0_int_density :1134-1144
  const double e_top = e[x], e_bot = e[x + (size_t)nz * slab];
  if (eta) eta[x] = e_top * Z_to_H;
  const double ssh0 = e_top, ssh1 = do_u ? e[x + 1] : 0.0, ssh2 = do_v ? e[x + st] : 0.0;
  const double z00 = E.ssh_z0 ? ssh0 : Z_ref, z01 = E.ssh_z0 ? ssh1 : Z_ref, z02 = E.ssh_z0 ? ssh2 : Z_ref;   // Z_0p :1264-1276
  const double b0 = bathyT[x], b1 = do_u ? bathyT[x + 1] : 0.0, b2 = do_v ? bathyT[x + st] : 0.0;
  double pa0 = GxRho_ref * (e_top - Z_ref), pa1 = 0.0, pa2 = 0.0, intx_pa = 0.0, inty_pa = 0.0;
  double cu = 0.0, cv = 0.0;
  if (do_u) { pa1 = GxRho_ref * (ssh1 - Z_ref); intx_pa = 0.5 * (pa0 + pa1); cu = (2.0 * I_Rho0 * gm(G, d, MOM6X_G_IdxCu)[x]); }
  if (do_v) { pa2 = GxRho_ref * (ssh2 - Z_ref); inty_pa = 0.5 * (pa0 + pa2); cv = (2.0 * I_Rho0 * gm(G, d, MOM6X_G_IdyCv)[x]); }
  // Set_pbce_Bouss, use_EOS, no rho_star :704-733 (Rho0 argument = rho0_set_pbce = rho0_alt)
  const double Rho0xG = rho0_alt * g_Earth, G_Rho0 = g_Earth / Rho0;
  const double Ihtot = H_to_Z / ((e_top - e_bot) + dz_neglect);
  double pb = 0.0, T_prev = 0.0, S_prev = 0.0;
  double zt0 = e_top, zt1 = ssh1, zt2 = ssh2;
  for (int k = 0; k < nz; k++) {
    const size_t c = x + (size_t)k * slab, cb = c + slab;
    const double h0 = h[c], T0 = Tv[c], S0 = Sv[c];
    const double zb0 = e[cb];
    double dpa0, iz0;
    double Tt0 = 0., Tb0 = 0., St0 = 0., Sb0 = 0.;
    if (MODE != 0) {
      if (MODE != 3) { Tt0 = Tt[c]; Tb0 = Tb[c]; St0 = St[c]; Sb0 = Sb[c]; }
      cell_int_plm<FORM, MODE>(E, rho_ref, G_e, GxRho, Tt0, Tb0, St0, Sb0, zt0, zb0, z00, dpa0, iz0, T0, S0);
    } else {
      cell_int<FORM>(E, rho_ref, G_e, GxRho, I_Rho, T0, S0, zt0, zb0, z00, dpa0, iz0);
    }
    if (Z_to_H != 1.0) iz0 = iz0 * Z_to_H;
    if (do_u) {
      const double h1 = h[c + 1], T1 = Tv[c + 1], S1 = Sv[c + 1], zb1 = e[cb + 1];
      double dpa1, iz1, intx_dpa;
      if (MODE != 0) {
        double Tt1 = 0., Tb1 = 0., St1 = 0., Sb1 = 0.;
        if (MODE != 3) { Tt1 = Tt[c + 1]; Tb1 = Tb[c + 1]; St1 = St[c + 1]; Sb1 = Sb[c + 1]; }
        cell_int_plm<FORM, MODE>(E, rho_ref, G_e, GxRho, Tt1, Tb1, St1, Sb1, zt1, zb1, z01, dpa1, iz1, T1, S1);
        if (MODE == 1)
          intx_dpa = face_int_plm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, Tt0, Tb0, St0, Sb0, Tt1, Tb1, St1, Sb1, zt0, zb0, zt1, zb1,
                                        z00, z01, b0, b1, ssh0, ssh1, dpa0, dpa1);
        else if (MODE == 2)
          intx_dpa = face_int_ppm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, Tt0, Tb0, T0, St0, Sb0, S0, Tt1, Tb1, T1, St1, Sb1, S1, zt0, zb0,
                                        zt1, zb1, z00, z01, b0, b1, ssh0, ssh1, dpa0, dpa1);
        else
          intx_dpa = face_int_pcm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, T0, S0, T1, S1, zt0, zb0, zt1, zb1, z00, z01, b0, b1, ssh0, ssh1,
                                        dpa0, dpa1);
      } else {
        cell_int<FORM>(E, rho_ref, G_e, GxRho, I_Rho, T1, S1, zt1, zb1, z01, dpa1, iz1);
        intx_dpa = face_int<FORM>(E, rho_ref, G_e, GxRho, I_Rho, T0, S0, T1, S1, zt0, zb0, zt1, zb1, z00, z01, b0, b1,
                                  ssh0, ssh1, dz_neglect, dpa0, dpa1);
      }
      if (Z_to_H != 1.0) iz1 = iz1 * Z_to_H;
      const double pf = (((pa0 * h0 + iz0) - (pa1 * h1 + iz1)) + ((h1 - h0) * intx_pa - (zb1 - zb0) * intx_dpa * Z_to_H)) *
                        (cu / ((h0 + h1) + h_neglect));
      PFu[c] = pf;
      if (B.u_bc) B.u_bc[c] = (B.CAu[c] + pf) + B.diffu[c];
      pa1 = pa1 + dpa1;
      intx_pa = intx_pa + intx_dpa;
      zt1 = zb1;
    }
    if (do_v) {
      const double h2 = h[c + st], T2 = Tv[c + st], S2 = Sv[c + st], zb2 = e[cb + st];
      double dpa2, iz2, inty_dpa;
      if (MODE != 0) {
        double Tt2 = 0., Tb2 = 0., St2 = 0., Sb2 = 0.;
        if (MODE != 3) { Tt2 = Tt[c + st]; Tb2 = Tb[c + st]; St2 = St[c + st]; Sb2 = Sb[c + st]; }
        cell_int_plm<FORM, MODE>(E, rho_ref, G_e, GxRho, Tt2, Tb2, St2, Sb2, zt2, zb2, z02, dpa2, iz2, T2, S2);
        if (MODE == 1)
          inty_dpa = face_int_plm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, Tt0, Tb0, St0, Sb0, Tt2, Tb2, St2, Sb2, zt0, zb0, zt2, zb2,
                                        z00, z02, b0, b2, ssh0, ssh2, dpa0, dpa2);
        else if (MODE == 2)
          inty_dpa = face_int_ppm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, Tt0, Tb0, T0, St0, Sb0, S0, Tt2, Tb2, T2, St2, Sb2, S2, zt0, zb0,
                                        zt2, zb2, z00, z02, b0, b2, ssh0, ssh2, dpa0, dpa2);
        else
          inty_dpa = face_int_pcm<FORM>(E, rho_ref, G_e, GxRho, dz_neglect, T0, S0, T2, S2, zt0, zb0, zt2, zb2, z00, z02, b0, b2, ssh0, ssh2,
                                        dpa0, dpa2);
      } else {
        cell_int<FORM>(E, rho_ref, G_e, GxRho, I_Rho, T2, S2, zt2, zb2, z02, dpa2, iz2);
        inty_dpa = face_int<FORM>(E, rho_ref, G_e, GxRho, I_Rho, T0, S0, T2, S2, zt0, zb0, zt2, zb2, z00, z02, b0, b2,
                                  ssh0, ssh2, dz_neglect, dpa0, dpa2);
      }
      if (Z_to_H != 1.0) iz2 = iz2 * Z_to_H;
      const double pf = (((pa0 * h0 + iz0) - (pa2 * h2 + iz2)) + ((h2 - h0) * inty_pa - (zb2 - zb0) * inty_dpa * Z_to_H)) *
                        (cv / ((h0 + h2) + h_neglect));
      PFv[c] = pf;
      if (B.v_bc) B.v_bc[c] = (B.CAv[c] + pf) + B.diffv[c];
      pa2 = pa2 + dpa2;
      inty_pa = inty_pa + inty_dpa;
      zt2 = zb2;
    }
    pa0 = pa0 + dpa0;
    if (pbce) {
      const double press = -Rho0xG * (zt0 - Z_ref);
      if (k == 0) {
        double rho_in_situ;
        if (FORM == MOM6X_EOS_LINEAR) rho_in_situ = E.Rho_T0_S0 + E.dRho_dT * T0 + E.dRho_dS * S0 + E.dRho_dp * press;
        else if (FORM == MOM6X_EOS_UNESCO) rho_in_situ = unesco::density(T0, S0, press);
        else if (FORM == MOM6X_EOS_ROQUET_RHO) rho_in_situ = roquet::roquet_density(T0, S0, press);
        else if (FORM == MOM6X_EOS_JACKETT06) rho_in_situ = jackett::jackett_density(T0, S0, press);
        else if (FORM == MOM6X_EOS_ROQUET_SPV) rho_in_situ = roquet::roquet_spv_density(T0, S0, press);
        else {
          rho_in_situ = wright_density<FORM>(T0, S0, press);
        }
        pb = G_Rho0 * (1.0 * rho_in_situ) * H_to_Z;
      } else {
        const double T_int = 0.5 * (T_prev + T0), S_int = 0.5 * (S_prev + S0);
        double dR_dT, dR_dS;
        eos_density_derivs<FORM>(E, T_int, S_int, press, dR_dT, dR_dS);
        pb = pb + G_Rho0 * ((zt0 - e_bot) * Ihtot) * (dR_dT * (T0 - T_prev) + dR_dS * (S0 - S_prev));
      }
      pbce[c] = pb;
    }
    T_prev = T0; S_prev = S0;
    zt0 = zb0;
  }
}
}  // namespace

// PressureForce_FV_CS and what tv hands it.  mom6x_PressureForce_set_tv may come before mom6x_PressureForce_init: whichever is first
// creates the state
struct PgfState {
  mom6x_pgf_params P; bool init;
  double *Rlay, *g_prime;                             // device copies of GV%Rlay, GV%g_prime (nk), owned
  const double *tv_T, *tv_S; mom6x_eos_params eos;    // tv%T, tv%S (caller-owned), tv%eqn_of_state (tv_T null: the layered path)
};
static PgfState *pgf_state(mom6x_ctx *c) {
  if (!c->pgf) c->pgf = new PgfState();
  return c->pgf;
}
void PressureForce_free(mom6x_ctx *c) {
  PgfState *S = c->pgf;
  if (!S) return;
  (void)hipFree(S->Rlay); (void)hipFree(S->g_prime);
  delete S;
  c->pgf = nullptr;
}
bool PressureForce_ready(const mom6x_ctx *c) { return c->pgf && c->pgf->init; }
const double *PressureForce_Rlay(const mom6x_ctx *c) { return c->pgf ? c->pgf->Rlay : nullptr; }

extern "C" int mom6x_PressureForce_set_tv(mom6x_ctx *c, const double *T, const double *S, const mom6x_eos_params *eos) {
  REQUIRE(c, MOM6X_EINVAL, "mom6x_PressureForce_set_tv: null ctx");
  if (!T) { if (c->pgf) c->pgf->tv_T = c->pgf->tv_S = nullptr; return MOM6X_OK; }
  REQUIRE(S && eos, MOM6X_EINVAL, "mom6x_PressureForce_set_tv: tv%T without tv%S or tv%eqn_of_state");
  REQUIRE(eos->form >= MOM6X_EOS_LINEAR && eos->form <= MOM6X_EOS_ROQUET_SPV, MOM6X_EUNSUPPORTED,
          "PressureForce: EQN_OF_STATE must be LINEAR, WRIGHT, WRIGHT_FULL, WRIGHT_REDUCED, UNESCO, ROQUET_RHO (NEMO), JACKETT_06 or ROQUET_SPV");
  // analytic_int_density_dz, MOM_EOS.F90:1495-1496
  REQUIRE(eos->form < MOM6X_EOS_UNESCO || eos->EOS_quadrature || eos->Recon_Scheme, MOM6X_EUNSUPPORTED,
          "No analytic integration option is available with this EOS!");
  REQUIRE(eos->Recon_Scheme >= 0 && eos->Recon_Scheme <= 2, MOM6X_EINVAL,
          "PressureForce_FV_init: PRESSURE_RECONSTRUCTION_SCHEME must be 1 (PLM) or 2 (PPM), or 0 without RECONSTRUCT_FOR_PRESSURE");
  REQUIRE(eos->Recon_Scheme != 2 || c->dims.nk >= 4, MOM6X_EUNSUPPORTED,
          "PressureForce_FV: PRESSURE_RECONSTRUCTION_SCHEME = 2 (edge_values_implicit_h4) needs NK >= 4");
  PgfState *S_ = pgf_state(c);
  S_->tv_T = T; S_->tv_S = S; S_->eos = *eos;
  return MOM6X_OK;
}

extern "C" int mom6x_PressureForce_init(mom6x_ctx *c, const mom6x_pgf_params *p, const double *Rlay, const double *g_prime) {
  REQUIRE(c && p && Rlay && g_prime, MOM6X_EINVAL, "mom6x_PressureForce_init: null argument");
  HIPCHK(hipSetDevice(c->device));
  PgfState *S = pgf_state(c);
  S->P = *p;
  const size_t n = (size_t)c->dims.nk * sizeof(double);
  if (!S->Rlay) HIPCHK(hipMalloc(&S->Rlay, n));
  if (!S->g_prime) HIPCHK(hipMalloc(&S->g_prime, n));
  HIPCHK(hipMemcpy(S->Rlay, Rlay, n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(S->g_prime, g_prime, n, hipMemcpyHostToDevice));
  S->init = true;
  return MOM6X_OK;
}

extern "C" int mom6x_PressureForce(mom6x_ctx *c, const double *h, double *PFu, double *PFv, double *pbce, double *eta) {
  bool eta_h_written;
  return PressureForce_bc(c, h, PFu, PFv, pbce, eta, BcFold{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr }, &eta_h_written);
}

int PressureForce_bc(mom6x_ctx *c, const double *h, double *PFu, double *PFv, double *pbce, double *eta, const BcFold &fold,
                     bool *eta_h_written) {
  *eta_h_written = false;
  REQUIRE(c && PressureForce_ready(c), MOM6X_EINVAL, "MOM_PressureForce_FV_Bouss: Module must be initialized before it is used.");
  REQUIRE(h && PFu && PFv, MOM6X_EINVAL, "PressureForce: null array");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const PgfState &S = *c->pgf;
  const mom6x_pgf_params &pgf = S.P;
  const mom6x_eos_params &eos = S.eos;
  double *e;
  int rc;
  if ((rc = ctx_scratch(c, SCR_e, d.nk + 1, &e))) return rc;
  const dim3 b = blk2();
  const mom6x_vgrid &GV = c->GV;
  const double GxRho0 = GV.g_Earth * GV.Rho0;
  const double GxRho_ref = pgf.rho_ref_bug ? GxRho0 : GV.g_Earth * pgf.rho_ref;
  KLAUNCH(c, "k_pgf_e", k_pgf_e, grid3(nxa(d.ni + 2, -1), d.nj + 2, 1, b), b, d, c->G, h, e, GV.H_to_Z);
  if (S.tv_T) {   // use_EOS = associated(tv%eqn_of_state) :1125
    EosDev E;
    E.form = eos.form; E.Rho_T0_S0 = eos.Rho_T0_S0; E.dRho_dT = eos.dRho_dT; E.dRho_dS = eos.dRho_dS;
    E.dRho_dp = eos.dRho_dp; E.do_mw = eos.MassWghtInterp & 1; E.top_mw = (eos.MassWghtInterp >> 1) & 1;
    E.ssh_z0 = eos.use_SSH_in_Z0p;
    E.van_only = eos.MassWghtInterpVanOnly; E.dz_nv = GV.H_to_Z * eos.h_nonvanished;   // dz_nonvanished :1128
    const double rho0_alt = pgf.rho_ref_bug ? pgf.rho_ref : GV.Rho0;   // rho0_int_density = rho0_set_pbce
    const dim3 g = grid3(nxa(d.ni + 2, -1), d.nj + 2, 1, b);
    // 0: analytic_int_density_dz; 1: TS_PLM_edge_values + int_density_dz_generic_plm; 2: TS_PPM_edge_values + ..._generic_ppm;
    // 3: EOS_QUADRATURE without a reconstruction: int_density_dz_generic_pcm (int_density_dz, MOM_density_integrals.F90:95-99)
    const int mode = eos.Recon_Scheme ? eos.Recon_Scheme : (eos.EOS_quadrature ? 3 : 0);
    double *Tt = nullptr, *Tb = nullptr, *St = nullptr, *Sb = nullptr;
    if (mode == 1 || mode == 2) {   // TS_PLM_edge_values (MOM_ALE.F90:1495) | TS_PPM_edge_values (:1581): S first, then T
      if ((rc = ctx_scratch(c, SCR_t0, d.nk, &Tt)) || (rc = ctx_scratch(c, SCR_t1, d.nk, &Tb)) ||
          (rc = ctx_scratch(c, SCR_t2, d.nk, &St)) || (rc = ctx_scratch(c, SCR_t3, d.nk, &Sb))) return rc;
      if (mode == 1) {
        if ((rc = mom6x_ALE_PLM_edge_values(c, h, S.tv_S, eos.boundary_extrap, St, Sb))) return rc;
        if ((rc = mom6x_ALE_PLM_edge_values(c, h, S.tv_T, eos.boundary_extrap, Tt, Tb))) return rc;
      } else {
        if ((rc = mom6x_ALE_PPM_edge_values(c, h, S.tv_S, eos.boundary_extrap, St, Sb))) return rc;
        if ((rc = mom6x_ALE_PPM_edge_values(c, h, S.tv_T, eos.boundary_extrap, Tt, Tb))) return rc;
      }
    }
#define PGF_EOS(F, P, NAME) KLAUNCH(c, NAME, (k_pgf_main_eos<F, P>), g, b, d, c->G, h, e, S.tv_T, S.tv_S, Tt, Tb, St, Sb, E, PFu, PFv,   \
                                    pbce, eta, GV.g_Earth, GV.H_to_Z, GV.Z_to_H, pgf.rho_ref, GxRho_ref, pgf.Z_ref, GV.Rho0, \
                                    rho0_alt, GV.H_subroundoff, GV.dZ_subroundoff, fold)
#define PGF_FORM(F, N) do { if (mode == 1) PGF_EOS(F, 1, "k_pgf_main_plm<" N ">"); else if (mode == 2) PGF_EOS(F, 2, "k_pgf_main_ppm<" N ">"); \
                            else if (mode == 3) PGF_EOS(F, 3, "k_pgf_main_pcm<" N ">"); else PGF_EOS(F, 0, "k_pgf_main_eos<" N ">"); } while (0)
    if (E.form == MOM6X_EOS_UNESCO) {   // quadratures only
      if (mode == 1) PGF_EOS(MOM6X_EOS_UNESCO, 1, "k_pgf_main_plm<unesco>");
      else if (mode == 2) PGF_EOS(MOM6X_EOS_UNESCO, 2, "k_pgf_main_ppm<unesco>");
      else PGF_EOS(MOM6X_EOS_UNESCO, 3, "k_pgf_main_pcm<unesco>");
    } else if (E.form == MOM6X_EOS_ROQUET_RHO) {
      if (mode == 1) PGF_EOS(MOM6X_EOS_ROQUET_RHO, 1, "k_pgf_main_plm<roquet_rho>");
      else if (mode == 2) PGF_EOS(MOM6X_EOS_ROQUET_RHO, 2, "k_pgf_main_ppm<roquet_rho>");
      else PGF_EOS(MOM6X_EOS_ROQUET_RHO, 3, "k_pgf_main_pcm<roquet_rho>");
    } else if (E.form == MOM6X_EOS_ROQUET_SPV) {
      if (mode == 1) PGF_EOS(MOM6X_EOS_ROQUET_SPV, 1, "k_pgf_main_plm<roquet_spv>");
      else if (mode == 2) PGF_EOS(MOM6X_EOS_ROQUET_SPV, 2, "k_pgf_main_ppm<roquet_spv>");
      else PGF_EOS(MOM6X_EOS_ROQUET_SPV, 3, "k_pgf_main_pcm<roquet_spv>");
    } else if (E.form == MOM6X_EOS_JACKETT06) {
      if (mode == 1) PGF_EOS(MOM6X_EOS_JACKETT06, 1, "k_pgf_main_plm<jackett06>");
      else if (mode == 2) PGF_EOS(MOM6X_EOS_JACKETT06, 2, "k_pgf_main_ppm<jackett06>");
      else PGF_EOS(MOM6X_EOS_JACKETT06, 3, "k_pgf_main_pcm<jackett06>");
    } else if (E.form == MOM6X_EOS_LINEAR) PGF_FORM(MOM6X_EOS_LINEAR, "linear");
    else if (E.form == MOM6X_EOS_WRIGHT_FULL) PGF_FORM(MOM6X_EOS_WRIGHT_FULL, "wright_full");
    else if (E.form == MOM6X_EOS_WRIGHT_REDUCED) PGF_FORM(MOM6X_EOS_WRIGHT_REDUCED, "wright_red");
    else PGF_FORM(MOM6X_EOS_WRIGHT, "wright");
#undef PGF_FORM
#undef PGF_EOS
    HIPCHK(hipGetLastError());
    return MOM6X_OK;
  }
  KLAUNCH(c, "k_pgf_main", k_pgf_main, grid3(nxa(d.ni + 2, -1), d.nj + 2, 1, b), b, d, c->G, h, e, S.Rlay, S.g_prime, PFu, PFv,
          pbce, eta, GV.g_Earth, GV.H_to_Z, GV.Z_to_H, pgf.rho_ref, GxRho_ref, pgf.Z_ref, 1.0 / GV.Rho0,
          GV.H_subroundoff, GV.dZ_subroundoff, fold);
  *eta_h_written = (fold.eta_h != nullptr);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
