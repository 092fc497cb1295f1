// set_diffusivity.hip -- the diapycnal diffusivities of the ALE-coordinate (non-layered) path of MOM_set_diffusivity on gfx950.
//
//   set_BBL_TKE               <- MOM_set_diffusivity.F90:1947-2152, the arm without open boundaries
//   set_diffusivity           <- :243-868: the fills :369-374, :452-453, the split of double diffusion :504-523, Kd_int from Kd_lay
//                                :571-589, the dissipation floors :682-695, :710-723, Kd_add :698-701, :732-736
//   find_N2                   <- :1095-1270 with h_amp = 0 (no tidal mixing)
//   double_diffusion          <- :1279-1361
//   add_LOTW_BBL_diffusivity  <- :1606-1789, both arms of LOTW_BBL_ANSWER_DATE
//   calculate_bkgnd_mixing    <- MOM_bkgnd_mixing.F90:323-518, the `else` arm :450-516
//   vert_fill_TS              <- MOM_isopycnal_slopes.F90:612-700 (isopycnal_slopes_dev.h), thickness_to_dz: dz = H_to_Z*h (Boussinesq)
//
// set_BBL_TKE: ONE launch, one lane per cell, which recomputes the bottom-up walks of its four faces (each face is walked by its
// two cells; the walk covers bbl_thick, a few layers, and the second cell finds the lines in L2).  No work array, no combine pass.
//
// set_diffusivity: TWO launches.  k_sd_fill writes the reference's whole-array fills into the halos (and wherever k_sd_cols will not
// write in the same call).  k_sd_cols<FORM>: one lane
// per column of the computational domain, consecutive lanes along i, four sweeps of the same lane --
//   1. vert_fill_TS_col: the elimination top-down, the back substitution bottom-up (c1 and the un-substituted T, S in work arrays);
//   2. top-down: pres of find_N2 and of double_diffusion, dRho_int, N2_lay, N2_int, the Hmix ramp's running depth, Kd_lay of the
//      background and of double diffusion, Kv_slow, dz_above of the newer LOTW answers, the depth sums;
//   3. the two bottom-up passes of find_N2 that put N2_bot into the deepest interfaces and layers (they climb while dz == 0);
//   4. bottom-up: Kd_int from Kd_lay, the law of the wall, the floors, Kd_add, and the stores of Kd_int and Kd_lay.
// What crosses sweeps (T_f, S_f, c1 | Kd_lay_2d, dRho_int, N2_int, N2_lay, dz_above) goes through the work arrays of
// mom6x_set_diffusivity_init; a lane reads back only what it wrote itself.  The call allocates nothing and does not synchronise.
//
// Not formed, because nothing on this path reads them: dRho_int_unfilt (find_TKE_to_Kd only) and find_rho_bottom (Boussinesq:
// Rho_bot = Rho0; h_bot, k_bot go to the internal-tide code).  MAX and MIN are fmax1 and fmin1 (mom6x_dev.h); x**2 is x*x.
#include "mom6x_dev.h"
#include "eos_dev.h"
#include "isopycnal_slopes_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// set_BBL_TKE

// ustar | vstar and u2_bbl | v2_bbl of the face between cells x and y (:2031-2079 | :2083-2129): vel, Kv, bt at the face's index xf
__device__ __forceinline__ void bbl_face(const double *__restrict__ h, const double *__restrict__ vel, double mask, double Kv, double bt,
                                         double cdrag_sqrt, double H_to_Z, size_t xf, size_t x, size_t y, size_t slab, int nz,
                                         double &ustar, double &u2) {
  ustar = 0.0; u2 = 0.0;
  if (!((mask > 0.0) && (cdrag_sqrt * bt > 0.0))) return;
  ustar = Kv / (cdrag_sqrt * bt);
  double htot = 0.0, uhtot = 0.0;
  for (int k = nz - 1; k >= 0; --k) {
    const size_t o = (size_t)k * slab;
    const double hvel = 0.5 * (H_to_Z * h[o + x] + H_to_Z * h[o + y]);
    if ((htot + hvel) >= bt) {
      uhtot = uhtot + (bt - htot) * vel[o + xf];
      htot = bt;
      break;
    }
    uhtot = uhtot + hvel * vel[o + xf];
    htot = htot + hvel;
  }
  if (htot > 0.0) u2 = (uhtot * uhtot) / (htot * htot);
}

// zero != 0: the early return :2007-2019
__global__ void __launch_bounds__(256)
k_set_BBL_TKE(Dm d, const double *__restrict__ G, double cdrag_sqrt, double H_to_Z, int zero, const double *__restrict__ u,
              const double *__restrict__ v, const double *__restrict__ h, const double *__restrict__ Kv_u,
              const double *__restrict__ Kv_v, const double *__restrict__ bt_u, const double *__restrict__ bt_v,
              double *__restrict__ ustar_BBL, double *__restrict__ KE_loss, double *__restrict__ KE_loss_sqrtCd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), p = (size_t)d.pitch, slab = (size_t)d.slab;
  if (zero) {
    if (ustar_BBL) ustar_BBL[x] = 0.0;
    if (KE_loss) KE_loss[x] = 0.0;
    if (KE_loss_sqrtCd) KE_loss_sqrtCd[x] = 0.0;
    return;
  }
  const int nz = d.nk;
  const double *mCu = gm(G, d, MOM6X_G_mask2dCu), *mCv = gm(G, d, MOM6X_G_mask2dCv);
  const double *aCu = gm(G, d, MOM6X_G_areaCu), *aCv = gm(G, d, MOM6X_G_areaCv);
  double usW, u2W, usE, u2E, vsS, v2S, vsN, v2N;
  bbl_face(h, u, mCu[x - 1], Kv_u[x - 1], bt_u[x - 1], cdrag_sqrt, H_to_Z, x - 1, x - 1, x, slab, nz, usW, u2W);
  bbl_face(h, u, mCu[x], Kv_u[x], bt_u[x], cdrag_sqrt, H_to_Z, x, x, x + 1, slab, nz, usE, u2E);
  bbl_face(h, v, mCv[x - p], Kv_v[x - p], bt_v[x - p], cdrag_sqrt, H_to_Z, x - p, x - p, x, slab, nz, vsS, v2S);
  bbl_face(h, v, mCv[x], Kv_v[x], bt_v[x], cdrag_sqrt, H_to_Z, x, x, x + p, slab, nz, vsN, v2N);
  const double Ia = gm(G, d, MOM6X_G_IareaT)[x];
  // :2132-2147
  ustar_BBL[x] = sqrt(0.5 * Ia * (((aCu[x - 1] * (usW * usW)) + (aCu[x] * (usE * usE))) +
                                  ((aCv[x - p] * (vsS * vsS)) + (aCv[x] * (vsN * vsN)))));
  const double loss = (((aCu[x - 1] * (usW * u2W)) + (aCu[x] * (usE * u2E))) + ((aCv[x - p] * (vsS * v2S)) + (aCv[x] * (vsN * v2N)))) * Ia;
  KE_loss[x] = cdrag_sqrt * loss;
  if (KE_loss_sqrtCd) KE_loss_sqrtCd[x] = loss;
}

// ---------------------------------------------------------------------------------------------------------------------------
// set_diffusivity

// Kd_sfc of calculate_bkgnd_mixing :452-472 over the whole plane, in place on the latitudes; mode 0 constant, 1 Henyey, 2 tanh
__global__ void k_sd_Kd_sfc(int n, int mode, double Kd, double Kd_min, double N0_2Omega, double Henyey_max_lat, double I_x30,
                            double deg_to_rad, double tanh_scale, double *__restrict__ plane) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n) return;
  const double lat = plane[x], min_sinlat = 1.e-10;
  double Kd_sfc = Kd;
  if (mode == 1) {
    double abs_sinlat = fabs(sin(lat * deg_to_rad));
    if (fabs(lat) > Henyey_max_lat) abs_sinlat = min_sinlat;
    const double r = N0_2Omega / fmax1(min_sinlat, abs_sinlat);
    Kd_sfc = fmax1(Kd_min, Kd * ((abs_sinlat * log(r + sqrt(r * r - 1.0))) * I_x30));   // invcosh :304-308
  } else if (mode == 2) {
    Kd_sfc = fmax1(Kd_min, Kd * (1.0 + tanh_scale * 0.5 * tanh((fabs(lat) - 35.0) / 5.0)));
  }
  plane[x] = Kd_sfc;
}

// The arrays of :369-374 and :452-453, nullable; lay: nk levels, the others nk + 1.  A point of the computational domain that
// k_sd_cols overwrites in the same call is skipped (Kd_int, Kd_lay and Kv_slow at every level, Kd_extra_T | _S at K = 2..nz with
// DOUBLE_DIFFUSION): the fill is the halo's, and the two launches together leave what the reference's two assignments leave.
struct SdFill { double *Kd_int, *Kd_lay, *Kd_extra_T, *Kd_extra_S, *Kv_slow, *Kv_shear; double Kd, Kv; size_t n_lay, n_int; int dd; };
__global__ void __launch_bounds__(256) k_sd_fill(Dm d, SdFill f) {
  const size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= f.n_int) return;
  const int k = (int)(x / (size_t)d.slab), r = (int)(x - (size_t)k * d.slab);
  const int j = r / d.pitch - d.joff, i = r - (j + d.joff) * d.pitch - d.ioff;
  const bool own = i >= 0 && i < d.ni && j >= 0 && j < d.nj;
  if (!own) {
    if (f.Kd_lay && x < f.n_lay) f.Kd_lay[x] = f.Kd;
    f.Kd_int[x] = f.Kd;
    if (f.Kv_slow) f.Kv_slow[x] = f.Kv;
  }
  if (!(own && f.dd && k >= 1 && k < d.nk)) {
    if (f.Kd_extra_T) f.Kd_extra_T[x] = 0.0;
    if (f.Kd_extra_S) f.Kd_extra_S[x] = 0.0;
  }
  if (f.Kv_shear) f.Kv_shear[x] = 0.0;
}

// the scalars of the column kernel, formed once on the host in the reference's order
struct SdK {
  double H_to_Z, Z_to_H, RZ_to_H, H_to_RZ, h_neglect, dz_neglect, gH, G_Rho0, p_to_Pa;
  double kap_dt_x2, h0;                                   // vert_fill_TS
  double Kd, Kv, Kd_tot_ml, Hmix, I_Hmix, prandtl;        // background
  double Max_Rrho, Max_salt_diff, Kv_molecular;           // double diffusion
  double BBL_effic, IMax_decay, von_Karm, N2_min, Kd_max; // law of the wall
  double dissip_min, dissip_N0, dissip_N1, dissip_N2, FluxRi_max, Omega2, Kd_add;
  double dRho_dT, dRho_dS;                                // the linear EOS (eos_density_derivs)
  int fill, ramp, ramp_bug, double_diffusion, use_shear, lotw, lotw_new, limit_dissipation;
};
struct SdP {   // the planes and fields of a call (nullable unless said otherwise) and the work arrays
  const double *u, *v, *h, *T, *S, *p_surf, *tv_p_surf, *Kd_shear, *ustar_BBL, *KE_loss, *ustar_tidal, *tidal_dis, *Ray_u, *Ray_v;
  const double *Kd_sfc, *Rlay;
  double *Kd_int, *Kd_lay, *Kd_extra_T, *Kd_extra_S, *Kv_slow, *N2_3d, *Kd_BBL, *Kd_bkgnd, *Kv_bkgnd, *KT_extra, *KS_extra;
  double *Tf, *Sf, *Kdl, *drho, *N2i, *N2l, *dza;   // Kdl doubles as vert_fill_TS's c1; Tf, Sf = T, S when nothing is filled
};

// FORM: the EOS form, 0 for layers of constant density (GV%Rlay)
template <int FORM>
__global__ void __launch_bounds__(256) k_sd_cols(Dm d, const double *__restrict__ G, SdK K, SdP P) {
  constexpr bool EOS = FORM != 0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), p = (size_t)d.pitch, slab = (size_t)d.slab;
  const int nz = d.nk;
  const double *h = P.h;

  // 1. vert_fill_TS(h, tv%T, tv%S, kappa_dt_fill, T_f, S_f, larger_h_denom=.true.) (:463)
  if (EOS && K.fill) vert_fill_TS_col(h, P.T, P.S, P.Tf, P.Sf, P.Kdl, x, slab, nz, K.kap_dt_x2, K.h0, K.h_neglect);
  const double *Tf = P.Tf, *Sf = P.Sf;

  // 2. top-down: find_N2 :1156-1200, calculate_bkgnd_mixing :475-515, double_diffusion :1321-1358 and its split :508-523
  const double Kd_sfc = P.Kd_sfc[x];
  double pres = P.p_surf ? P.p_surf[x] : 0.0, pdd = P.tv_p_surf ? P.tv_p_surf[x] : 0.0;
  double depth = 0.0, sumdz = 0.0, dza = K.dz_neglect;
  double hm = 0.0, Tm = 0.0, Sm = 0.0, dRm = 0.0, basem = 0.0, pend = 0.0;
  P.N2i[x] = 0.0; P.drho[x] = 0.0;
  if (K.lotw_new) P.dza[x] = dza;
  if (P.Kv_slow) P.Kv_slow[x] = K.Kv + 0.0;
  if (P.Kd_bkgnd) P.Kd_bkgnd[x] = 0.0;
  if (P.Kv_bkgnd) P.Kv_bkgnd[x] = 0.0;
  if (K.double_diffusion) {
    if (P.KT_extra) P.KT_extra[x] = 0.0;
    if (P.KS_extra) P.KS_extra[x] = 0.0;
  }
  for (int k = 0; k < nz; ++k) {
    const size_t o = (size_t)k * slab + x;
    const double hk = h[o];
    double Tk = 0.0, Sk = 0.0;
    if constexpr (EOS) { Tk = Tf[o]; Sk = Sf[o]; }
    // Kd_lay of the background (:475-505)
    double base;
    if (K.ramp) {
      const double depth_c = depth + 0.5 * hk;
      const double mid = ((Kd_sfc - K.Kd_tot_ml) * K.I_Hmix) * depth_c + (2.0 * K.Kd_tot_ml - Kd_sfc);
      if (depth_c <= K.Hmix) base = K.ramp_bug ? K.Kd : K.Kd_tot_ml;
      else if (depth_c >= 2.0 * K.Hmix) base = K.ramp_bug ? K.Kd : Kd_sfc;
      else base = mid;
      depth = depth + hk;
    } else {
      base = Kd_sfc;
    }
    double lay = base;
    if (k >= 1) {   // the interface between layers k-1 and k
      pres = pres + K.gH * hm;
      double dR, dR_dT = 0.0, dR_dS = 0.0;
      if constexpr (EOS) {
        eos_density_derivs<FORM>(K, 0.5 * (Tk + Tm), 0.5 * (Sk + Sm), K.p_to_Pa * pres, dR_dT, dR_dS);
        dR = fmax1(dR_dT * (Tk - Tm) + dR_dS * (Sk - Sm), 0.0);
      } else {
        dR = P.Rlay[k] - P.Rlay[k - 1];
      }
      P.drho[o] = dR;
      P.N2i[o] = K.G_Rho0 * dR / (0.5 * (hm + hk + K.h_neglect));
      P.N2l[o - slab] = K.G_Rho0 * 0.5 * (dRm + dR) / (hm + K.h_neglect);
      dRm = dR;
      const double Kd_bk = 0.5 * (basem + base), Kv_bk = Kd_bk * K.prandtl;   // :513-514
      if (P.Kv_slow) P.Kv_slow[o] = K.Kv + Kv_bk;
      if (P.Kd_bkgnd) P.Kd_bkgnd[o] = Kd_bk;
      if (P.Kv_bkgnd) P.Kv_bkgnd[o] = Kv_bk;
      if constexpr (EOS) {
        if (K.double_diffusion) {
          pdd = pdd + K.gH * hm;
          double aT = dR_dT, bS = dR_dS;
          if (pdd != pres) eos_density_derivs<FORM>(K, 0.5 * (Tm + Tk), 0.5 * (Sm + Sk), K.p_to_Pa * pdd, aT, bS);
          const double alpha_dT = -1.0 * aT * (Tm - Tk), beta_dS = bS * (Sm - Sk);
          double KT = 0.0, KS = 0.0;
          if ((alpha_dT > beta_dS) && (beta_dS > 0.0)) {   // salt fingers
            const double Rrho = fmin1(alpha_dT / beta_dS, K.Max_Rrho);
            const double diff_dd = 1.0 - ((Rrho - 1.0) / (K.Max_Rrho - 1.0));
            const double Kd_dd = K.Max_salt_diff * diff_dd * diff_dd * diff_dd;
            KT = 0.7 * Kd_dd; KS = Kd_dd;
          } else if ((alpha_dT < 0.) && (beta_dS < 0.) && (alpha_dT > beta_dS)) {   // diffusive convection
            const double Rrho = alpha_dT / beta_dS;
            const double Kd_dd = K.Kv_molecular * 0.909 * exp(4.6 * exp(-0.54 * (1.0 / Rrho - 1.0)));
            double prandtl = 0.15 * Rrho;
            if (Rrho > 0.5) prandtl = (1.85 - 0.85 / Rrho) * Rrho;
            KT = Kd_dd; KS = prandtl * Kd_dd;
          }
          if (KS > KT) {
            pend = pend + 0.5 * KT; lay = lay + 0.5 * KT;
            P.Kd_extra_S[o] = KS - KT; P.Kd_extra_T[o] = 0.0;
          } else if (KT > 0.0) {
            pend = pend + 0.5 * KS; lay = lay + 0.5 * KS;
            P.Kd_extra_T[o] = KT - KS; P.Kd_extra_S[o] = 0.0;
          } else {
            P.Kd_extra_T[o] = 0.0; P.Kd_extra_S[o] = 0.0;
          }
          if (P.KT_extra) P.KT_extra[o] = KT;
          if (P.KS_extra) P.KS_extra[o] = KS;
        }
      }
      P.Kdl[o - slab] = pend;
    }
    const double dzk = K.H_to_Z * hk;
    sumdz = sumdz + dzk;
    dza = dza + dzk;
    if (K.lotw_new) P.dza[o + slab] = dza;
    pend = lay; basem = base; hm = hk; Tm = Tk; Sm = Sk;
  }
  {
    const size_t o = (size_t)nz * slab + x;
    P.Kdl[o - slab] = pend;
    P.N2l[o - slab] = K.G_Rho0 * 0.5 * (dRm + 0.0) / (hm + K.h_neglect);
    P.N2i[o] = 0.0; P.drho[o] = 0.0;
    if (P.Kv_slow) P.Kv_slow[o] = K.Kv + 0.0;
    if (P.Kd_bkgnd) P.Kd_bkgnd[o] = 0.0;
    if (P.Kv_bkgnd) P.Kv_bkgnd[o] = 0.0;
    if (K.double_diffusion) {
      if (P.KT_extra) P.KT_extra[o] = 0.0;
      if (P.KS_extra) P.KS_extra[o] = 0.0;
    }
  }

  // 3. N2_bot and its two bottom-up passes with h_amp = 0 (:1203-1258)
  if (gm(G, d, MOM6X_G_mask2dT)[x] > 0.0) {
    const double dz_nz = K.H_to_Z * h[(size_t)(nz - 1) * slab + x];
    double z_from_bot = 0.5 * dz_nz, hb = 0.0, drho_bot = 0.0;
    for (int k = nz - 1; k >= 1; --k) {
      const size_t o = (size_t)k * slab + x;
      const double hk = h[o], hkm = h[o - slab];
      z_from_bot = z_from_bot + 0.5 * (K.H_to_Z * hk + K.H_to_Z * hkm);
      hb = hb + 0.5 * (hk + hkm);
      drho_bot = drho_bot + P.drho[o];
      if (z_from_bot > 0.0) {
        if (k > 1) {   // always include at least one full layer
          hb = hb + 0.5 * (hkm + h[o - 2 * slab]);
          drho_bot = drho_bot + P.drho[o - slab];
        }
        break;
      }
    }
    const double N2_bot = (hb > 0.0) ? (K.G_Rho0 * drho_bot) / hb : 0.0;
    z_from_bot = 0.5 * dz_nz;
    for (int k = nz - 1; k >= 1; --k) {
      const size_t o = (size_t)k * slab + x;
      z_from_bot = z_from_bot + 0.5 * (K.H_to_Z * h[o] + K.H_to_Z * h[o - slab]);
      P.N2i[o] = N2_bot;
      if (k > 1) P.N2l[o - slab] = N2_bot;
      if (z_from_bot > 0.0) {
        if (k > 1) P.N2i[o - slab] = N2_bot;
        break;
      }
    }
  }

  // 4. bottom-up: Kd_int from Kd_lay :571-589, add_LOTW_BBL_diffusivity :1677-1786, the floors and Kd_add :682-736
  double ustar2 = 0.0, absf = 0.0, Idecay = 0.0, TKE_remaining = 0.0, ustar_D = 0.0, total_depth = 0.0, Ia_eff = 0.0;
  const bool Rayleigh = K.lotw && P.Ray_u != nullptr;
  if (K.lotw) {
    const double *q = gm(G, d, MOM6X_G_CoriolisBu);
    absf = 0.25 * ((fabs(q[x - 1 - p]) + fabs(q[x])) + (fabs(q[x - 1]) + fabs(q[x - p])));
    double ustar = P.ustar_BBL[x];
    ustar2 = ustar * ustar;
    if (P.ustar_tidal) ustar = ustar + K.Z_to_H * P.ustar_tidal[x];
    Idecay = K.IMax_decay;
    if ((ustar > 0.0) && (absf > K.IMax_decay * ustar)) Idecay = absf / ustar;
    double dis = P.KE_loss[x];
    if (P.tidal_dis) dis = dis + P.tidal_dis[x] * K.RZ_to_H;
    TKE_remaining = K.BBL_effic * dis;
    total_depth = K.lotw_new ? dza : (sumdz + K.dz_neglect);
    ustar_D = ustar * total_depth;
    if (Rayleigh) Ia_eff = 0.5 * K.BBL_effic * gm(G, d, MOM6X_G_IareaT)[x];
  }
  const double *aCu = gm(G, d, MOM6X_G_areaCu), *aCv = gm(G, d, MOM6X_G_areaCv);
  double h_bot = 0.0, z_bot = 0.0, Kd_lower = 0.0;
  double lk = P.Kdl[(size_t)(nz - 1) * slab + x];
  for (int k = nz - 1; k >= 1; --k) {   // interface k, between layers k-1 and k
    const size_t o = (size_t)k * slab + x;
    const double lm = P.Kdl[o - slab];
    double kint, klay = lk;
    if (K.use_shear) {
      kint = P.Kd_shear[o] + 0.5 * (lm + lk);
      klay = lk + 0.5 * (P.Kd_shear[o] + P.Kd_shear[o + slab]);
    } else {
      kint = 0.5 * (lm + lk);
    }
    const double N2_int = P.N2i[o];
    if (K.lotw) {
      const double hk = h[o], dzk = K.H_to_Z * hk;
      const double dz_int = 0.5 * (K.H_to_Z * h[o - slab] + dzk);
      if (Rayleigh) {
        const double uW = P.u[o - 1], uE = P.u[o], vS = P.v[o - p], vN = P.v[o];
        TKE_remaining = TKE_remaining + Ia_eff * (((aCu[x - 1] * P.Ray_u[o - 1] * (uW * uW)) + (aCu[x] * P.Ray_u[o] * (uE * uE))) +
                                                  ((aCv[x - p] * P.Ray_v[o - p] * (vS * vS)) + (aCv[x] * P.Ray_v[o] * (vN * vN))));
      }
      TKE_remaining = exp(-Idecay * hk) * TKE_remaining;
      z_bot = z_bot + dzk;
      h_bot = h_bot + hk;
      const double D_minus_z = K.lotw_new ? P.dza[o] : fmax1(total_depth - z_bot, 0.);
      double Kd_wall, TKE_consumed;
      if (ustar_D + absf * (h_bot * D_minus_z) == 0.) Kd_wall = 0.;
      else Kd_wall = ((K.von_Karm * ustar2) * (z_bot * D_minus_z)) / (ustar_D + absf * (h_bot * D_minus_z));
      const double TKE_Kd_wall = Kd_wall * dz_int * fmax1(N2_int, K.N2_min);
      if (TKE_Kd_wall > 0.) {
        TKE_consumed = fmin1(TKE_Kd_wall, TKE_remaining);
        Kd_wall = (TKE_consumed / TKE_Kd_wall) * Kd_wall;
      } else {
        Kd_wall = (TKE_remaining > 0.) ? K.Kd_max : 0.;
        TKE_consumed = 0.;
      }
      TKE_remaining = TKE_remaining - TKE_consumed;
      kint = kint + Kd_wall;
      klay = klay + 0.5 * (Kd_wall + Kd_lower);
      Kd_lower = Kd_wall;
      if (P.Kd_BBL) P.Kd_BBL[o] = Kd_wall;
    }
    if (K.limit_dissipation) {
      const double dissip = fmax1(fmax1(K.dissip_min, K.dissip_N0 + K.dissip_N1 * sqrt(N2_int)), K.dissip_N2 * N2_int);
      kint = fmax1(kint, dissip * (K.FluxRi_max / (K.H_to_RZ * (N2_int + K.Omega2))));
    }
    if (K.Kd_add > 0.0) kint = kint + K.Kd_add;
    P.Kd_int[o] = kint;
    if (P.N2_3d) P.N2_3d[o] = N2_int;
    if (P.Kd_lay) {
      if (K.limit_dissipation && k <= nz - 2) {
        const double N2_lay = P.N2l[o];
        const double dissip = fmax1(fmax1(K.dissip_min, K.dissip_N0 + K.dissip_N1 * sqrt(N2_lay)), K.dissip_N2 * N2_lay);
        klay = fmax1(klay, dissip * (K.FluxRi_max / (K.H_to_RZ * (N2_lay + K.Omega2))));
      }
      if (K.Kd_add > 0.0) klay = klay + K.Kd_add;
      P.Kd_lay[o] = klay;
    }
    lk = lm;
  }
  {   // layer 1 and the two outer interfaces
    const size_t ob = (size_t)nz * slab + x;
    double kint = K.use_shear ? P.Kd_shear[x] : lk, kbot = 0.0;
    if (K.Kd_add > 0.0) { kint = kint + K.Kd_add; kbot = kbot + K.Kd_add; }
    P.Kd_int[x] = kint;
    P.Kd_int[ob] = kbot;
    if (P.N2_3d) { P.N2_3d[x] = P.N2i[x]; P.N2_3d[ob] = P.N2i[ob]; }
    if (P.Kd_lay) {
      double klay = lk;
      if (K.use_shear) klay = lk + 0.5 * (P.Kd_shear[x] + P.Kd_shear[x + slab]);
      if (K.Kd_add > 0.0) klay = klay + K.Kd_add;
      P.Kd_lay[x] = klay;
    }
  }
}

}  // namespace

// set_diffusivity_CS with its bkgnd_mixing_CS, tv%eqn_of_state, the device copy of GV%Rlay, the Kd_sfc plane and the work arrays
struct SdState {
  mom6x_set_diffusivity_params P;
  bool use_eos; mom6x_eos_params eos;
  double IMax_decay, dissip_N2; bool limit_dissipation;   // :2441-2442, :2566-2570
  double *Rlay;     // nk, null with an EOS
  double *Kd_sfc;   // one plane
  double *work;     // [T_f | S_f | c1, Kd_lay_2d | dRho_int | N2_int | N2_lay | dz_above], nk + 1 levels each
};

void set_diffusivity_free(mom6x_ctx *c) {
  if (!c->sd) return;
  (void)hipFree(c->sd->Rlay); (void)hipFree(c->sd->Kd_sfc); (void)hipFree(c->sd->work);
  delete c->sd;
  c->sd = nullptr;
}

extern "C" int mom6x_set_diffusivity_init(mom6x_ctx *c, const mom6x_set_diffusivity_params *p, const mom6x_eos_params *eos,
                                          const double *Rlay, const double *geoLatT) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_set_diffusivity_init: null argument");
  REFUSE(p->ML_radiation, "set_diffusivity_init", "ML_RADIATION (add_MLrad_diffusivity)");
  REFUSE(p->use_tidal_mixing, "set_diffusivity_init", "tidal mixing (INT_TIDE_DISSIPATION, USE_CVMix_TIDAL, LEE_WAVE_DISSIPATION)");
  REFUSE(p->use_int_tides, "set_diffusivity_init", "INTERNAL_TIDES (get_lowmode_diffusivity)");
  REFUSE(p->use_CVMix_ddiff, "set_diffusivity_init", "USE_CVMIX_DDIFF");
  REFUSE(p->Bryan_Lewis_diffusivity, "set_diffusivity_init", "BRYAN_LEWIS_DIFFUSIVITY");
  REFUSE(p->horiz_varying_background, "set_diffusivity_init", "HORIZ_VARYING_BACKGROUND");
  REFUSE(p->user_change_diff, "set_diffusivity_init", "USER_CHANGE_DIFFUSIVITY");
  REFUSE(p->nkml != 0, "set_diffusivity_init", "a bulk mixed layer (GV%nkml > 0)");
  REFUSE(p->SpV_avg || !c->GV.Boussinesq, "set_diffusivity_init", "non-Boussinesq mode (tv%SpV_avg)");
  REFUSE(p->open_bcs, "set_diffusivity_init", "open boundary conditions (set_BBL_TKE)");
  REFUSE(p->bottomdraglaw && p->BBL_effic > 0.0 && !p->use_LOTW_BBL_diffusivity, "set_diffusivity_init",
         "bottom-drag mixing without USE_LOTW_BBL_DIFFUSIVITY (add_drag_diffusivity, find_TKE_to_Kd)");
  REQUIRE(!(p->bottomdraglaw && p->use_LOTW_BBL_diffusivity && p->Kd_max <= 0.), MOM6X_EINVAL,
          "set_diffusivity_init: KD_MAX must be set (positive) when USE_LOTW_BBL_DIFFUSIVITY=True.");
  REQUIRE(!p->double_diffusion || eos, MOM6X_EINVAL,
          "set_diffusivity_init: DOUBLE_DIFFUSION needs an equation of state (the reference leaves Kd_T_dd, Kd_S_dd unset)");
  REQUIRE(!(p->Henyey_IGW_background && p->Kd_tanh_lat_fn), MOM6X_EINVAL,
          "MOM_bkgnd_mixing: KD_TANH_LAT_FN can not be used with HENYEY_IGW_BACKGROUND.");
  REQUIRE(!(p->Henyey_IGW_background || p->Kd_tanh_lat_fn) || geoLatT, MOM6X_EINVAL,
          "set_diffusivity_init: HENYEY_IGW_BACKGROUND and KD_TANH_LAT_FN need G%geoLatT");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "set_diffusivity_init: unknown EQN_OF_STATE form");
  REQUIRE(!eos || c->d.nk >= 2, MOM6X_EINVAL, "set_diffusivity_init: vert_fill_TS needs two layers");
  REQUIRE(eos || Rlay, MOM6X_EINVAL, "set_diffusivity_init: without an equation of state find_N2 needs GV%Rlay");
  HIPCHK(hipSetDevice(c->device));
  set_diffusivity_free(c);
  SdState *s = new SdState();
  c->sd = s;
  s->P = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  s->IMax_decay = 0.0;
  if (p->bottomdraglaw && p->BBL_mixing_max_decay > 0.0) s->IMax_decay = 1.0 / p->BBL_mixing_max_decay;
  s->limit_dissipation = (p->dissip_min > 0.) || (p->dissip_N1 > 0.) || (p->dissip_N0 > 0.) || (p->dissip_Kd_min > 0.);
  s->dissip_N2 = 0.0;
  if (p->FluxRi_max > 0.0) s->dissip_N2 = p->dissip_Kd_min * c->GV.H_to_RZ / p->FluxRi_max;
  const Dm d = c->d;
  const size_t slab = (size_t)d.slab, nw = (size_t)7 * (d.nk + 1) * slab * sizeof(double);
  s->Rlay = nullptr; s->Kd_sfc = nullptr; s->work = nullptr;
  HIPCHK(hipMalloc(&s->work, nw));
  HIPCHK(hipMemsetAsync(s->work, work_fill_byte(), nw, c->stream));
  if (!eos) {
    HIPCHK(hipMalloc(&s->Rlay, (size_t)d.nk * sizeof(double)));
    HIPCHK(hipMemcpy(s->Rlay, Rlay, (size_t)d.nk * sizeof(double), hipMemcpyHostToDevice));
  }
  // Kd_sfc depends on latitude only: formed once, on the device (sin, log and tanh are the device's)
  HIPCHK(hipMalloc(&s->Kd_sfc, slab * sizeof(double)));
  const int mode = p->Henyey_IGW_background ? 1 : (p->Kd_tanh_lat_fn ? 2 : 0);
  if (mode) HIPCHK(hipMemcpy(s->Kd_sfc, geoLatT, slab * sizeof(double), hipMemcpyHostToDevice));
  else HIPCHK(hipMemsetAsync(s->Kd_sfc, 0, slab * sizeof(double), c->stream));
  const double x30 = p->N0_2Omega * 2.0;
  const double I_x30 = (mode == 1) ? 2.0 / log(x30 + sqrt(x30 * x30 - 1.0)) : 0.0;   // :453
  const double deg_to_rad = atan(1.0) / 45.0;
  KLAUNCH(c, "k_sd_Kd_sfc", k_sd_Kd_sfc, dim3((unsigned)((slab + 255) / 256)), dim3(256), (int)slab, mode, p->Kd, p->Kd_min, p->N0_2Omega,
          p->Henyey_max_lat, I_x30, deg_to_rad, p->Kd_tanh_lat_scale, s->Kd_sfc);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" double *mom6x_set_diffusivity_field(mom6x_ctx *c, int which) {
  if (!c || !c->sd) return nullptr;
  return which == 0 ? c->sd->Kd_sfc : nullptr;
}

extern "C" int mom6x_set_BBL_TKE(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *Kv_bbl_u,
                                 const double *Kv_bbl_v, const double *bbl_thick_u, const double *bbl_thick_v, double *ustar_BBL,
                                 double *BBL_meanKE_loss, double *BBL_meanKE_loss_sqrtCd) {
  REQUIRE(c && c->sd, MOM6X_EINVAL, "set_BBL_TKE: Module must be initialized before it is used.");
  const mom6x_set_diffusivity_params &P = c->sd->P;
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
  const bool zero = !P.bottomdraglaw || (P.BBL_effic <= 0.0 && P.ePBL_BBL_effic <= 0.0 && !P.ePBL_BBL_mstar);   // :2007
  if (zero) {
    if (!ustar_BBL && !BBL_meanKE_loss && !BBL_meanKE_loss_sqrtCd) return MOM6X_OK;
  } else {
    REQUIRE(u && v && h, MOM6X_EINVAL, "set_BBL_TKE: null u, v or h");
    REQUIRE(Kv_bbl_u && Kv_bbl_v && bbl_thick_u && bbl_thick_v, MOM6X_EINVAL,
            "set_BBL_TKE: visc%Kv_bbl_u, Kv_bbl_v, bbl_thick_u and bbl_thick_v (mom6x_set_viscous_BBL) are needed");
    REQUIRE(ustar_BBL && BBL_meanKE_loss, MOM6X_EINVAL, "set_BBL_TKE: visc%ustar_BBL and visc%BBL_meanKE_loss are needed");
  }
  KLAUNCH(c, "k_set_BBL_TKE", k_set_BBL_TKE, g, b, d, c->G, sqrt(P.cdrag), c->GV.H_to_Z, zero ? 1 : 0, u, v, h, Kv_bbl_u, Kv_bbl_v,
          bbl_thick_u, bbl_thick_v, ustar_BBL, BBL_meanKE_loss, BBL_meanKE_loss_sqrtCd);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_set_diffusivity(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *T, const double *S,
                                     const double *p_surf, const double *tv_p_surf, const double *Kd_shear, const double *ustar_BBL,
                                     const double *BBL_meanKE_loss, const double *ustar_tidal, const double *BBL_tidal_dis,
                                     const double *Ray_u, const double *Ray_v, double dt, double *Kd_int, double *Kd_lay,
                                     double *Kd_extra_T, double *Kd_extra_S, double *Kv_slow, double *Kv_shear, double *N2_3d,
                                     double *Kd_BBL, double *Kd_bkgnd, double *Kv_bkgnd, double *KT_extra, double *KS_extra) {
  REQUIRE(c && c->sd, MOM6X_EINVAL, "set_diffusivity: Module must be initialized before it is used.");
  const SdState *s = c->sd;
  const mom6x_set_diffusivity_params &P = s->P;
  const mom6x_vgrid &GV = c->GV;
  REQUIRE(h && Kd_int, MOM6X_EINVAL, "set_diffusivity: null h or Kd_int");
  REQUIRE(!s->use_eos || (T && S), MOM6X_EINVAL, "set_diffusivity: an equation of state needs tv%T and tv%S");
  REQUIRE((Kd_extra_T != nullptr) == (Kd_extra_S != nullptr), MOM6X_EINVAL, "set_diffusivity: Kd_extra_T and Kd_extra_S come together");
  REQUIRE(!P.double_diffusion || Kd_extra_T, MOM6X_EINVAL,
          "set_diffusivity: both Kd_extra_T and Kd_extra_S must be present when USE_CVMIX_DDIFF or DOUBLE_DIFFUSION are true.");
  REQUIRE(!P.use_Kd_shear || Kd_shear, MOM6X_EINVAL, "set_diffusivity: USE_JACKSON_PARAM / USE_CVMix_SHEAR need visc%Kd_shear");
  const bool lotw = P.bottomdraglaw && P.BBL_effic > 0.0 && P.use_LOTW_BBL_diffusivity;
  REQUIRE(!lotw || (ustar_BBL && BBL_meanKE_loss), MOM6X_EINVAL,
          "set_diffusivity: USE_LOTW_BBL_DIFFUSIVITY needs visc%ustar_BBL and visc%BBL_meanKE_loss (mom6x_set_BBL_TKE)");
  REQUIRE((Ray_u != nullptr) == (Ray_v != nullptr), MOM6X_EINVAL, "set_diffusivity: Ray_u and Ray_v come together");
  REQUIRE(!(lotw && Ray_u) || (u && v), MOM6X_EINVAL, "set_diffusivity: with visc%Ray_u, Ray_v the law of the wall reads u and v");
  REQUIRE(dt > 0.0 || P.answer_date < 20190101, MOM6X_EINVAL, "set_diffusivity: dt must be positive");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const size_t slab = (size_t)d.slab, n3 = (size_t)(d.nk + 1) * slab;

  SdFill f;
  f.Kd_int = Kd_int; f.Kd_lay = Kd_lay; f.Kd_extra_T = Kd_extra_T; f.Kd_extra_S = Kd_extra_S; f.Kv_slow = Kv_slow;
  f.Kv_shear = P.use_Kd_shear ? nullptr : Kv_shear;   // :452-453
  f.Kd = P.Kd; f.Kv = P.Kv; f.n_lay = (size_t)d.nk * slab; f.n_int = n3; f.dd = P.double_diffusion;
  KLAUNCH(c, "k_sd_fill", k_sd_fill, dim3((unsigned)((n3 + 255) / 256)), dim3(256), d, f);

  SdK K;
  K.H_to_Z = GV.H_to_Z; K.Z_to_H = GV.Z_to_H; K.RZ_to_H = GV.RZ_to_H; K.H_to_RZ = GV.H_to_RZ;
  K.h_neglect = GV.H_subroundoff; K.dz_neglect = GV.dZ_subroundoff;
  K.gH = GV.g_Earth * GV.H_to_RZ;                              // :1169, :1330
  K.G_Rho0 = P.g_Earth_Z_T2 / GV.H_to_RZ;                      // :1152
  K.p_to_Pa = P.RL2_T2_to_Pa;
  double kappa_dt_fill;                                        // :350-355
  if (P.answer_date < 20190101) kappa_dt_fill = 1.e-3 * P.m2_s_to_HZ_T * 7200. * P.s_to_T;
  else kappa_dt_fill = P.Kd_smooth * dt;
  K.kap_dt_x2 = (2.0 * kappa_dt_fill) * P.Z_to_H_fill;         // MOM_isopycnal_slopes.F90:655
  K.h0 = 1.0e-16 * sqrt(0.5 * K.kap_dt_x2);                    // :658
  K.fill = s->use_eos && K.kap_dt_x2 > 0.0;                    // else T_f = T_in (:661-665): read in place
  K.Kd = P.Kd; K.Kv = P.Kv; K.Kd_tot_ml = P.Kd_tot_ml; K.Hmix = P.Hmix; K.prandtl = P.prandtl_bkgnd;
  K.ramp = (!P.physical_OBL_scheme) && (P.Kd != P.Kd_tot_ml);  // MOM_bkgnd_mixing.F90:475
  K.I_Hmix = K.ramp ? 1.0 / (P.Hmix + GV.H_subroundoff) : 0.0;
  K.ramp_bug = P.Kd_via_Kdml_bug;
  K.double_diffusion = P.double_diffusion;
  K.Max_Rrho = P.Max_Rrho_salt_fingers; K.Max_salt_diff = P.Max_salt_diff_salt_fingers; K.Kv_molecular = P.Kv_molecular;
  K.use_shear = P.use_Kd_shear;
  K.lotw = lotw; K.lotw_new = lotw && P.LOTW_BBL_answer_date > 20240630;
  K.BBL_effic = P.BBL_effic; K.IMax_decay = s->IMax_decay; K.von_Karm = P.von_Karm; K.Kd_max = P.Kd_max;
  K.N2_min = P.LOTW_BBL_use_omega ? P.omega * P.omega : 0.;    // :1666-1667
  K.limit_dissipation = s->limit_dissipation;
  K.dissip_min = P.dissip_min; K.dissip_N0 = P.dissip_N0; K.dissip_N1 = P.dissip_N1; K.dissip_N2 = s->dissip_N2;
  K.FluxRi_max = P.FluxRi_max; K.Omega2 = P.omega * P.omega; K.Kd_add = P.Kd_add;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;

  SdP A;
  A.u = u; A.v = v; A.h = h; A.T = T; A.S = S; A.p_surf = p_surf; A.tv_p_surf = tv_p_surf; A.Kd_shear = Kd_shear;
  A.ustar_BBL = ustar_BBL; A.KE_loss = BBL_meanKE_loss; A.ustar_tidal = ustar_tidal; A.tidal_dis = BBL_tidal_dis;
  A.Ray_u = Ray_u; A.Ray_v = Ray_v; A.Kd_sfc = s->Kd_sfc; A.Rlay = s->Rlay;
  A.Kd_int = Kd_int; A.Kd_lay = Kd_lay; A.Kd_extra_T = Kd_extra_T; A.Kd_extra_S = Kd_extra_S; A.Kv_slow = Kv_slow;
  A.N2_3d = N2_3d; A.Kd_BBL = Kd_BBL; A.Kd_bkgnd = Kd_bkgnd; A.Kv_bkgnd = Kv_bkgnd; A.KT_extra = KT_extra; A.KS_extra = KS_extra;
  double *W = s->work;
  A.Tf = K.fill ? W : const_cast<double *>(T); A.Sf = K.fill ? W + n3 : const_cast<double *>(S);
  A.Kdl = W + 2 * n3; A.drho = W + 3 * n3; A.N2i = W + 4 * n3; A.N2l = W + 5 * n3; A.dza = W + 6 * n3;
  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
#define SDC(F) KLAUNCH(c, "k_sd_cols<" #F ">", k_sd_cols<F>, g, b, d, c->G, K, A)
  if (!s->use_eos) SDC(0);
  else EOS_FORM_DISPATCH(s->eos.form, SDC);
#undef SDC
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
