// diabatic_aux.hip -- applyBoundaryFluxesInOut of MOM_diabatic_aux on gfx950: the surface fluxes of heat, salt and water into h, tv%T
// and tv%S, with the energetics that energetic_PBL reads (cTKE, dSV_dT, dSV_dS, SkinBuoyFlux).
//
//   applyBoundaryFluxesInOut  <- MOM_diabatic_aux.F90:682-1346, the Boussinesq path without brine plumes
//   extractFluxes1d           <- MOM_forcing_type.F90:447-948 with do_enthalpy = .true. (MOM6 computes the enthalpy terms itself),
//                                the four _rate outputs with their deliberate omissions :724-728, :745-749
//   absorbRemainingSW         <- MOM_opacity.F90:600-867 as this caller uses it: adjustAbsorptionProfile = .false.,
//                                absorbAllSW = .true., no eps | ksort | htot | Ttot, TKE and dSV_dT with energetics
//   calculate_specific_vol_derivs, calculate_density_derivs <- eos_dev.h
//
// k_da_fill writes the reference's whole-array fills (:808-809) into the halos, and into the computational domain where k_da_cols
// will not write in the same call.  k_da_cols<NSW, ENER>: one lane per column of the computational domain, consecutive lanes along
// i.  The reference runs the derivatives :886-895, step A :1005-1073, step B :1077-1175 and the downward loop of absorbRemainingSW
// :724-815 as separate k loops over a j slice; they couple the layers of a column only through scalars (pres, netMassOut, netHeat,
// netSalt, Pen_SW_bnd(n), h_heat), so here they are ONE top-down walk: for layer k the derivatives on the original h, T, S, then A
// if k = 1, then B, then the absorption.  The expressions and their order within a layer are the reference's, so are the results.
// Before the walk a lane sums h top-down for extractFluxes1d's htot (:589-590): a second read of h.  After it, the upward loop
// :845-861 runs only in a lane with T_chg > 0 (shortwave reached the bottom); T_chg_above is 0 throughout, so a wavefront none of
// whose lanes has shortwave left skips it.  SkinBuoyFlux comes last, from the final T(1), S(1) (:1296-1318).
//
// The bands are compile-time (NSW = 0..4, unrolled): Pen_SW_bnd(n) and Pen_SW_bnd_rate(n) stay in registers.  The equation of
// state is a wavefront-uniform switch inside the kernel (two sites per column), not a template argument.
//
// What the device cannot do as the reference does is stop: see include/mom6x.h.  MAX and MIN are fmax1 and fmin1; x**2 is x*x.
#include "mom6x_dev.h"
#include "eos_dev.h"

namespace {

struct DaFill { double *cTKE, *Skin; int own_cTKE, own_Skin; };
// one lane per point of a plane; own_*: k_da_cols writes the computational domain of that array in this call
__global__ void __launch_bounds__(256) k_da_fill(Dm d, DaFill f) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= d.slab) return;
  const int j = r / d.pitch - d.joff, i = r - (j + d.joff) * d.pitch - d.ioff;
  const bool own = i >= 0 && i < d.ni && j >= 0 && j < d.nj;
  if (f.cTKE && !(own && f.own_cTKE))
    for (int k = 0; k < d.nk; ++k) f.cTKE[(size_t)k * d.slab + r] = 0.0;
  if (f.Skin && !(own && f.own_Skin)) f.Skin[r] = 0.0;
}

// the scalars of the column kernel, formed once on the host in the reference's order
struct DaK {
  double dt, Idt, H_to_Z, H_to_RZ, RZ_to_H, C_p, I_Cp, I_Cp_Hc;
  double Ih_limit;                 // extractFluxes1d :553
  double Ih_limit_sw, h_min_heat;  // absorbRemainingSW :832, :707
  double gH, p_to_Pa, g_Hconv2, g_Hconv2_sw, GoRho_H_to_Z, RivermixConst, ppt1000, dSalt_frac_max, H_subroundoff;
  double min_depth, evap_CFL, min_SW_heat, I_Habs;
  double zero;   // 0.0 as a run-time value.  MIN(0., x) and `if (x < 0.) s = s + x` from s = 0. against the LITERAL 0.0 are compiled to
                 // v_min_f64(x, 0), which returns -0 for x = -0 where the reference's compare-and-select returns +0
  double Rho_T0_S0, dRho_dT, dRho_dS, dRho_dp;   // the linear EOS
  int form, forcing, agg, buoy, rivermix, river_heat, calving_heat, ignore_land, old_optics;
};
struct DaP {
  mom6x_surface_fluxes F;
  const double *opac, *swpen, *p_surf;
  double *h, *T, *S, *cTKE, *dSV_dT, *dSV_dS, *Skin, *createdH, *penSW, *penSWflux, *nonpenSW;
  unsigned long long *cnt;   // groundings, columns with a negative thickness, fluxes over land
};

__device__ __forceinline__ void da_specvol_derivs(const DaK &K, double T, double S, double p, double &a, double &b) {
  switch (K.form) {
    case MOM6X_EOS_LINEAR: eos_specvol_derivs<MOM6X_EOS_LINEAR>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT: eos_specvol_derivs<MOM6X_EOS_WRIGHT>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT_FULL: eos_specvol_derivs<MOM6X_EOS_WRIGHT_FULL>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT_REDUCED: eos_specvol_derivs<MOM6X_EOS_WRIGHT_REDUCED>(K, T, S, p, a, b); break;
    default: eos_specvol_derivs<MOM6X_EOS_ROQUET_SPV>(K, T, S, p, a, b); break;
  }
}
__device__ __forceinline__ void da_density_derivs(const DaK &K, double T, double S, double p, double &a, double &b) {
  switch (K.form) {
    case MOM6X_EOS_LINEAR: eos_density_derivs<MOM6X_EOS_LINEAR>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT: eos_density_derivs<MOM6X_EOS_WRIGHT>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT_FULL: eos_density_derivs<MOM6X_EOS_WRIGHT_FULL>(K, T, S, p, a, b); break;
    case MOM6X_EOS_WRIGHT_REDUCED: eos_density_derivs<MOM6X_EOS_WRIGHT_REDUCED>(K, T, S, p, a, b); break;
    case MOM6X_EOS_UNESCO: eos_density_derivs<MOM6X_EOS_UNESCO>(K, T, S, p, a, b); break;
    case MOM6X_EOS_ROQUET_RHO: eos_density_derivs<MOM6X_EOS_ROQUET_RHO>(K, T, S, p, a, b); break;
    case MOM6X_EOS_JACKETT06: eos_density_derivs<MOM6X_EOS_JACKETT06>(K, T, S, p, a, b); break;
    default: eos_density_derivs<MOM6X_EOS_ROQUET_SPV>(K, T, S, p, a, b); break;
  }
}

// NSW: the number of bands of penetrating shortwave; ENER: calculate_energetics
template <int NSW, bool ENER>
__global__ void __launch_bounds__(256) k_da_cols(Dm d, const double *__restrict__ G, DaK K, DaP P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  double *h = P.h, *T = P.T, *S = P.S;

  if (!K.forcing) {   // .not.associated(fluxes%sw): the derivatives :877-897, then `cycle` (:900)
    if constexpr (ENER) {
      double pres = P.p_surf ? P.p_surf[x] : 0.0;
      for (int k = 0; k < nz; ++k) {
        const size_t o = (size_t)k * slab + x;
        const double d_pres = K.gH * h[o], p_lay = pres + 0.5 * d_pres;
        pres = pres + d_pres;
        double a, b;
        da_specvol_derivs(K, T[o], S[o], K.p_to_Pa * p_lay, a, b);
        P.dSV_dT[o] = a; P.dSV_dS[o] = b; P.cTKE[o] = 0.0;
      }
    }
    return;
  }
  const bool wet = gm(G, d, MOM6X_G_mask2dT)[x] > 0.0;
  const mom6x_surface_fluxes &F = P.F;

  // extractFluxes1d (MOM_forcing_type.F90:589-946); T(i,1) is the temperature before step A
  double htot = h[x];
  for (int k = 1; k < nz; ++k) htot = htot + h[(size_t)k * slab + x];
  const double T1 = T[x];
  double scale = 1.0;
  if ((K.Ih_limit > 0.0) && (htot * K.Ih_limit < 1.0)) scale = htot * K.Ih_limit;
  double Pen[NSW > 0 ? NSW : 1], Pen_rate[NSW > 0 ? NSW : 1];
  double Pen_tot = 0.0, Pen_tot_rate = 0.0;
  Pen[0] = 0.0; Pen_rate[0] = 0.0;
#pragma unroll
  for (int n = 0; n < NSW; ++n) {
    const double top = P.swpen[(size_t)n * slab + x];
    Pen[n] = K.I_Cp_Hc * scale * K.dt * fmax1(0.0, top);
    Pen_tot = Pen_tot + Pen[n];
    Pen_rate[n] = K.I_Cp_Hc * scale * fmax1(0.0, top);
    Pen_tot_rate = Pen_tot_rate + Pen_rate[n];
  }
  const double lprec = F.lprec[x], fprec = F.fprec[x], evap = F.evap[x], lrunoff = F.lrunoff[x], lrunoff_glc = F.lrunoff_glc[x];
  const double vprec = F.vprec[x], seaice_melt = F.seaice_melt[x], frunoff = F.frunoff[x], frunoff_glc = F.frunoff_glc[x];
  const double water = ((((((((lprec + fprec) + evap) + lrunoff) + lrunoff_glc) + vprec) + seaice_melt) + frunoff) + frunoff_glc);
  double netMassInOut = K.dt * (scale * water), netMassInOut_rate = (scale * water);
  double netMassOut = K.zero;
  if (evap < 0.0) netMassOut = netMassOut + evap;
  if (lprec < 0.0) netMassOut = netMassOut + lprec;
  if (seaice_melt < 0.0) netMassOut = netMassOut + seaice_melt;
  if (vprec < 0.0) netMassOut = netMassOut + vprec;
  netMassOut = K.dt * scale * netMassOut;
  netMassInOut = K.RZ_to_H * netMassInOut;
  netMassInOut_rate = K.RZ_to_H * netMassInOut_rate;
  netMassOut = K.RZ_to_H * netMassOut;
  const double sw = F.sw[x];
  double rad;
  if (F.seaice_melt_heat) rad = sw + (((F.lw[x] + F.latent[x]) + F.sens[x]) + F.seaice_melt_heat[x]);
  else rad = sw + ((F.lw[x] + F.latent[x]) + F.sens[x]);
  double netHeat = scale * K.dt * K.I_Cp_Hc * rad, netHeat_rate = scale * K.I_Cp_Hc * rad;
  if (F.heat_added) {
    const double ha = F.heat_added[x];
    netHeat = netHeat + (scale * (K.dt * K.I_Cp_Hc)) * ha;
    netHeat_rate = netHeat_rate + (scale * K.I_Cp_Hc) * ha;
  }
  double TempxPmE = F.TempxPmE ? F.TempxPmE[x] : 0.0;
  if (K.river_heat) {   // the _rate twin is left out on purpose (:724-728)
    const double hl = F.heat_content_lrunoff[x], hg = F.heat_content_lrunoff_glc[x];
    netHeat = (netHeat + (scale * (K.dt * K.I_Cp_Hc)) * hl) - (K.RZ_to_H * (scale * K.dt)) * lrunoff * T1;
    netHeat = (netHeat + (scale * (K.dt * K.I_Cp_Hc)) * hg) - (K.RZ_to_H * (scale * K.dt)) * lrunoff_glc * T1;
    if (F.TempxPmE) {
      TempxPmE = TempxPmE + (scale * K.dt) * (K.I_Cp * hl - lrunoff * T1);
      TempxPmE = TempxPmE + (scale * K.dt) * (K.I_Cp * hg - lrunoff_glc * T1);
    }
  }
  if (K.calving_heat) {   // likewise (:745-749)
    const double hf = F.heat_content_frunoff[x], hg = F.heat_content_frunoff_glc[x];
    netHeat = netHeat + (scale * (K.dt * K.I_Cp_Hc)) * hf - (K.RZ_to_H * (scale * K.dt)) * frunoff * T1;
    netHeat = netHeat + (scale * (K.dt * K.I_Cp_Hc)) * hg - (K.RZ_to_H * (scale * K.dt)) * frunoff_glc * T1;
    if (F.TempxPmE) {
      TempxPmE = TempxPmE + (scale * K.dt) * (K.I_Cp * hf - frunoff * T1);
      TempxPmE = TempxPmE + (scale * K.dt) * (K.I_Cp * hg - frunoff_glc * T1);
    }
  }
  netHeat = netHeat - Pen_tot;
  netHeat_rate = netHeat_rate - Pen_tot_rate;
  const double nonpenSW = scale * K.dt * K.I_Cp_Hc * sw - Pen_tot;
  double netSalt = 0.0, netSalt_rate = 0.0;
  if (F.salt_flux) {
    const double sf = F.salt_flux[x];
    netSalt = (scale * K.dt * (K.ppt1000 * sf)) * K.RZ_to_H;
    netSalt_rate = (scale * 1. * (K.ppt1000 * sf)) * K.RZ_to_H;
  }
  // the diagnostics of :819-920
  double hc_in = 0.0, hc_out = 0.0;
  if (K.agg) {
    if (netMassInOut > 0.0) {
      hc_in = -K.C_p * netMassOut * T1 * K.H_to_RZ / K.dt;
      hc_out = K.C_p * netMassOut * T1 * K.H_to_RZ / K.dt;
    } else {
      hc_in = K.C_p * (netMassInOut - netMassOut) * T1 * K.H_to_RZ / K.dt;
      hc_out = -K.C_p * (netMassInOut - netMassOut) * T1 * K.H_to_RZ / K.dt;
    }
  }
  if (F.heat_content_lprec) F.heat_content_lprec[x] = (lprec > 0.0) ? K.C_p * lprec * T1 : 0.0;
  if (F.heat_content_fprec) F.heat_content_fprec[x] = (fprec > 0.0) ? K.C_p * fprec * T1 : 0.0;
  if (F.heat_content_vprec) F.heat_content_vprec[x] = (vprec > 0.0) ? K.C_p * vprec * T1 : 0.0;
  if (F.heat_content_cond) F.heat_content_cond[x] = (evap > 0.0) ? K.C_p * evap * T1 : 0.0;
  if (!K.river_heat) {
    if (F.heat_content_lrunoff) F.heat_content_lrunoff[x] = K.C_p * lrunoff * T1;
    if (F.heat_content_lrunoff_glc) F.heat_content_lrunoff_glc[x] = K.C_p * lrunoff_glc * T1;
  }
  if (!K.calving_heat) {
    if (F.heat_content_frunoff) F.heat_content_frunoff[x] = K.C_p * frunoff * T1;
    if (F.heat_content_frunoff_glc) F.heat_content_frunoff_glc[x] = K.C_p * frunoff_glc * T1;
  }

  // MOM_diabatic_aux.F90:968-983
  double netMassIn;
  if (K.agg) {
    netMassOut = netMassInOut;
    netMassIn = 0.;
  } else {
    netMassIn = netMassInOut - netMassOut;
  }
  if (F.netMassOut) F.netMassOut[x] = wet ? netMassOut : 0.0;
  if (F.netMassIn) F.netMassIn[x] = wet ? netMassIn : 0.0;

  // the walk
  const double C1_6 = 1.0 / 6.0, C1_60 = 1.0 / 60.0;
  double pres = 0.0;
  if constexpr (ENER) pres = P.p_surf ? P.p_surf[x] : 0.0;
  double h_heat = 0.0, T_sfc = 0.0, S_sfc = 0.0;
  bool negative = false;
  for (int k = 0; k < nz; ++k) {
    const size_t o = (size_t)k * slab + x;
    double hk = h[o], Tk = T[o], Sk = 0.0;
    if (ENER || wet || k == 0) Sk = S[o];
    double dSVdT = 0.0, dSVdS = 0.0, cT = 0.0;
    if constexpr (ENER) {   // :886-895, on the original h, T, S
      const double d_pres = K.gH * hk, p_lay = pres + 0.5 * d_pres;
      pres = pres + d_pres;
      da_specvol_derivs(K, Tk, Sk, K.p_to_Pa * p_lay, dSVdT, dSVdS);
      P.dSV_dT[o] = dSVdT; P.dSV_dS[o] = dSVdS;
    }
    if (wet) {
      if (k == 0) {   // A/ the incoming mass flux :1005-1073
        const double dThickness = netMassIn;
        double dTemp = 0., dSalt = 0.;
        netMassIn = netMassIn - dThickness;
        const double Temp_in = Tk, Salin_in = 0.0;
        dTemp = dTemp + dThickness * Temp_in;
        if (F.heat_content_massin) hc_in = hc_in + Tk * fmax1(0., dThickness) * K.H_to_RZ * K.C_p * K.Idt;
        if (F.heat_content_massout) hc_out = hc_out + Tk * fmin1(K.zero, dThickness) * K.H_to_RZ * K.C_p * K.Idt;
        if (F.TempxPmE) TempxPmE = TempxPmE + Tk * dThickness * K.H_to_RZ;
        if constexpr (ENER) {
          if (K.rivermix)
            cT = cT + fmax1(0.0, K.RivermixConst * dSVdS * ((lrunoff + frunoff) + (lrunoff_glc + frunoff_glc)) * Sk);
        }
        const double hOld = hk;
        hk = hk + dThickness;
        if (hk > 0.0) {
          if constexpr (ENER) {
            if (dThickness > 0.)
              cT = cT + 0.5 * K.g_Hconv2 * (hOld * dThickness) * ((Tk - Temp_in) * dSVdT + (Sk - Salin_in) * dSVdS);
          }
          const double Ithickness = 1.0 / hk;
          if (dThickness != 0. || dTemp != 0.) Tk = (hOld * Tk + dTemp) * Ithickness;
          if (dThickness != 0. || dSalt != 0.) Sk = (hOld * Sk + dSalt) * Ithickness;
        }
      }
      {   // B/ the mass leaving the ocean and the other fluxes of heat and salt :1077-1175
        const double IforcingDepthScale = 1. / fmax1(K.H_subroundoff, K.min_depth - netMassOut);
        double fractionOfForcing = fmin1(1.0, hk * IforcingDepthScale);
        if (-fractionOfForcing * netMassOut > K.evap_CFL * hk) fractionOfForcing = -K.evap_CFL * hk / netMassOut;
        const double dThickness = fmax1(fractionOfForcing * netMassOut, -hk);
        double dTemp = fractionOfForcing * netHeat;
        const double dSalt = fmax1(fractionOfForcing * netSalt, -K.dSalt_frac_max * hk * Sk);
        netMassOut = netMassOut - dThickness;
        netHeat = netHeat - dTemp;
        netSalt = netSalt - dSalt;
        dTemp = dTemp + dThickness * Tk;
        if (F.heat_content_massin) hc_in = hc_in + Tk * fmax1(0., dThickness) * K.H_to_RZ * K.C_p * K.Idt;
        if (F.heat_content_massout) hc_out = hc_out + Tk * fmin1(K.zero, dThickness) * K.H_to_RZ * K.C_p * K.Idt;
        if (F.TempxPmE) TempxPmE = TempxPmE + Tk * dThickness * K.H_to_RZ;
        const double hOld = hk;
        hk = hk + dThickness;
        if (hk > 0.) {
          if constexpr (ENER)
            cT = cT - (0.5 * hk * K.g_Hconv2) * ((dTemp - dThickness * Tk) * dSVdT + (dSalt - dThickness * Sk) * dSVdS);
          const double Ithickness = 1.0 / hk;
          Tk = (hOld * Tk + dTemp) * Ithickness;
          Sk = (hOld * Sk + dSalt + 0.0) * Ithickness;   // + plume_flux
        } else if (hk < 0.0) {
          negative = true;   // the reference stops here (:1163-1172); T and S of the layer stay
        }
      }
      h[o] = hk; S[o] = Sk;
    }
    if (P.penSW) P.penSW[o] = Tk;   // :1215, the temperature before the shortwave heating
    // C/ the downward loop of absorbRemainingSW (MOM_opacity.F90:724-815) with the new thickness
    double pen_TKE = 0.0;
    if constexpr (NSW > 0) {
      if (hk > 0.0) {   // h > 1.5*epsilon, epsilon = 0
#pragma unroll
        for (int n = 0; n < NSW; ++n) {
          if (Pen[n] > 0.0) {
            const double opt_depth = hk * P.opac[((size_t)n * nz + k) * slab + x];
            const double exp_OD = exp(-opt_depth);
            double SW_trans = exp_OD;
            const double nPen = (double)NSW * Pen[n];
            if (K.old_optics) {
              if (nPen * SW_trans < K.min_SW_heat * fmin1(1.0, K.I_Habs * hk)) SW_trans = 0.0;
            } else if ((nPen * SW_trans < K.min_SW_heat) && (hk > K.h_min_heat)) {
              if (nPen <= K.min_SW_heat * (K.I_Habs * (hk - K.h_min_heat))) SW_trans = 0.0;
              else SW_trans = fmin1(SW_trans, 1.0 - (K.min_SW_heat * (K.I_Habs * (hk - K.h_min_heat))) / nPen);
            }
            const double Heat_bnd = Pen[n] * (1.0 - SW_trans);
            Tk = Tk + Pen[n] * (1.0 - SW_trans) / hk;
            if constexpr (ENER) {   // coSWa_frac = 1
              if (opt_depth > 1e-2)
                pen_TKE = pen_TKE - Heat_bnd * dSVdT * (0.5 * hk * K.g_Hconv2_sw) *
                                        (opt_depth * (1.0 + exp_OD) - 2.0 * (1.0 - exp_OD)) / (opt_depth * (1.0 - exp_OD));
              else
                pen_TKE = pen_TKE - Heat_bnd * dSVdT * (0.5 * hk * K.g_Hconv2_sw) *
                                        (C1_6 * opt_depth * (1.0 - C1_60 * (opt_depth * opt_depth)));
            }
            Pen[n] = Pen[n] * SW_trans;
          }
        }
      }
      if (hk >= 2.0 * K.h_min_heat) h_heat = h_heat + hk;
      else if (hk > K.h_min_heat) h_heat = h_heat + (2.0 * hk - 2.0 * K.h_min_heat);
    }
    if constexpr (ENER) P.cTKE[o] = cT + pen_TKE;   // :1227-1229
    T[o] = Tk;
    if (k == 0) { T_sfc = Tk; S_sfc = Sk; }
  }

  // what is left of the shortwave goes back through the column (MOM_opacity.F90:820-861); T_chg_above = 0
  if constexpr (NSW > 0) {
    double Pen_SW_rem = Pen[0];
#pragma unroll
    for (int n = 1; n < NSW; ++n) Pen_SW_rem = Pen_SW_rem + Pen[n];
    double T_chg = 0.0;
    if ((Pen_SW_rem > 0.0) && (h_heat > 0.0)) {
      if (h_heat * K.Ih_limit_sw >= 1.0) T_chg = Pen_SW_rem / h_heat;
      else T_chg = Pen_SW_rem * K.Ih_limit_sw;
    }
    if (T_chg > 0.0) {
      for (int k = nz - 1; k >= 0; --k) {
        const size_t o = (size_t)k * slab + x;
        const double hk = h[o];
        if (hk >= 2.0 * K.h_min_heat) T[o] = T[o] + T_chg;
        else if (hk > K.h_min_heat) T[o] = T[o] + T_chg * (2.0 - 2.0 * K.h_min_heat / hk);
      }
      T_sfc = T[x];
    }
  }

  // the diagnostics :1245-1272
  if (P.penSW) {
    double flux = 0.0;
    if (P.penSWflux) P.penSWflux[(size_t)nz * slab + x] = 0.0;
    for (int k = nz - 1; k >= 0; --k) {
      const size_t o = (size_t)k * slab + x;
      const double conv = (T[o] - P.penSW[o]) * h[o] * K.Idt * K.C_p * K.H_to_RZ;
      P.penSW[o] = conv;
      flux = conv + flux;
      if (P.penSWflux) P.penSWflux[o] = flux;
    }
  }
  if (P.nonpenSW) P.nonpenSW[x] = nonpenSW * K.Idt * K.C_p * K.H_to_RZ;
  if (F.heat_content_massin) F.heat_content_massin[x] = hc_in;
  if (F.heat_content_massout) F.heat_content_massout[x] = hc_out;
  if (F.TempxPmE) F.TempxPmE[x] = TempxPmE;

  // :1178-1203: the reference's two fatal errors and its warning are counts here
  if (negative) atomicAdd(&P.cnt[1], 1ull);
  if (!wet && ((fabs(netHeat) + fabs(netSalt) + fabs(netMassIn) + fabs(netMassOut)) > 0.) && !K.ignore_land) atomicAdd(&P.cnt[2], 1ull);
  const double grounded = netMassIn + netMassOut;
  if (grounded != 0.0) atomicAdd(&P.cnt[0], 1ull);
  if (P.createdH) P.createdH[x] = (grounded != 0.0) ? 0. - grounded / K.dt : 0.;

  // SkinBuoyFlux :1279-1318, the Boussinesq arm, from the final T(1), S(1)
  if (K.buoy) {
    double netPen_rate = 0.0;
#pragma unroll
    for (int n = 0; n < NSW; ++n) netPen_rate = netPen_rate + Pen_rate[n];
    double dRhodT, dRhodS;
    da_density_derivs(K, T_sfc, S_sfc, K.p_to_Pa * (P.p_surf ? P.p_surf[x] : 0.0), dRhodT, dRhodS);
    P.Skin[x] = -K.GoRho_H_to_Z * (dRhodS * (netSalt_rate - S_sfc * netMassInOut_rate) + dRhodT * (netHeat_rate + netPen_rate));
  }
}

const char *eos_form_name(int form) {
  switch (form) {
    case MOM6X_EOS_UNESCO: return "UNESCO";
    case MOM6X_EOS_ROQUET_RHO: return "ROQUET_RHO";
    case MOM6X_EOS_JACKETT06: return "JACKETT_06";
    default: return "this";
  }
}

}  // namespace

// diabatic_aux_CS with the members of tv, US and optics the routine reads, tv%eqn_of_state and the counters
struct DaState {
  mom6x_diabatic_aux_params P;
  bool use_eos; mom6x_eos_params eos;
  unsigned long long *cnt;   // 3, on the device
};

void diabatic_aux_free(mom6x_ctx *c) {
  if (!c->da) return;
  (void)hipFree(c->da->cnt);
  delete c->da;
  c->da = nullptr;
}

extern "C" int mom6x_diabatic_aux_init(mom6x_ctx *c, const mom6x_diabatic_aux_params *p, const mom6x_eos_params *eos) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_diabatic_aux_init: null argument");
  REFUSE(p->SpV_avg || !c->GV.Boussinesq, "diabatic_aux_init", "non-Boussinesq mode (tv%SpV_avg)");
  REFUSE(p->do_brine_plume, "diabatic_aux_init", "DO_BRINE_PLUME");
  REFUSE(p->enthalpy_from_coupler, "diabatic_aux_init", "enthalpy from the coupler (fluxes%heat_content_evap, do_enthalpy = .false.)");
  REFUSE(p->nkml != 0, "diabatic_aux_init", "a bulk mixed layer (GV%nkml > 0)");
  REQUIRE(p->C_p > 0.0, MOM6X_EINVAL, "diabatic_aux_init: C_p must be positive");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "diabatic_aux_init: unknown EQN_OF_STATE form");
  HIPCHK(hipSetDevice(c->device));
  diabatic_aux_free(c);
  DaState *s = new DaState();
  c->da = s;
  s->P = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  s->cnt = nullptr;
  HIPCHK(hipMalloc(&s->cnt, 3 * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(s->cnt, 0, 3 * sizeof(unsigned long long), c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_diabatic_aux_status(mom6x_ctx *c, long *groundings, long *negative_h, long *land_fluxes) {
  REQUIRE(c && c->da, MOM6X_EINVAL, "diabatic_aux_status: Module must be initialized before it is used.");
  HIPCHK(hipSetDevice(c->device));
  unsigned long long n[3];
  HIPCHK(hipMemcpyAsync(n, c->da->cnt, sizeof(n), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemsetAsync(c->da->cnt, 0, sizeof(n), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (groundings) *groundings = (long)n[0];
  if (negative_h) *negative_h = (long)n[1];
  if (land_fluxes) *land_fluxes = (long)n[2];
  return MOM6X_OK;
}

extern "C" int mom6x_applyBoundaryFluxesInOut(mom6x_ctx *c, double dt, const mom6x_surface_fluxes *fluxes, int nsw,
                                              const double *opacity_band, const double *sw_pen_band, double *h, double *T, double *S,
                                              const double *tv_p_surf, int aggregate_FW_forcing, double evap_CFL_limit,
                                              double minimum_forcing_depth, double *cTKE, double *dSV_dT, double *dSV_dS,
                                              double *SkinBuoyFlux, double *createdH, double *penSW_diag, double *penSWflux_diag,
                                              double *nonpenSW_diag) {
  REQUIRE(c && c->da, MOM6X_EINVAL, "applyBoundaryFluxesInOut: Module must be initialized before it is used.");
  const DaState *s = c->da;
  const mom6x_diabatic_aux_params &P = s->P;
  const mom6x_vgrid &GV = c->GV;
  const bool ener = cTKE && dSV_dT && dSV_dS, buoy = SkinBuoyFlux != nullptr;
  const bool forcing = fluxes && fluxes->sw;
  REQUIRE(!ener || s->use_eos, MOM6X_EINVAL, "applyBoundaryFluxesInOut: cTKE, dSV_dT and dSV_dS need an equation of state");
  REQUIRE(!buoy || s->use_eos, MOM6X_EINVAL, "applyBoundaryFluxesInOut: SkinBuoyFlux needs an equation of state");
  if (ener && !eos_specvol_form_known(s->eos.form)) {
    mom6x_set_error("applyBoundaryFluxesInOut: the specific-volume derivatives of EQN_OF_STATE = %s are not on the device "
                    "(calculate_energetics)", eos_form_name(s->eos.form));
    return MOM6X_EUNSUPPORTED;
  }
  if (forcing || ener) REQUIRE(h && T && S, MOM6X_EINVAL, "applyBoundaryFluxesInOut: null h, tv%T or tv%S");
  if (forcing) {
    const mom6x_surface_fluxes &F = *fluxes;
    REQUIRE(dt > 0.0, MOM6X_EINVAL, "applyBoundaryFluxesInOut: dt must be positive");
    REQUIRE(nsw >= 0, MOM6X_EINVAL, "applyBoundaryFluxesInOut: nsw must not be negative");
    REFUSE(nsw > 4, "applyBoundaryFluxesInOut", "more than 4 bands of penetrating shortwave (nsw > 4)");
    REQUIRE(F.lw, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: fluxes%lw is not associated.");
    REQUIRE(F.latent, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: fluxes%latent is not associated.");
    REQUIRE(F.sens, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: fluxes%sens is not associated.");
    REQUIRE(F.evap, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: No evaporation defined.");
    REQUIRE(F.vprec, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: fluxes%vprec not defined.");
    REQUIRE(F.lprec && F.fprec, MOM6X_EINVAL, "MOM_forcing_type extractFluxes1d: No precipitation defined.");
    REQUIRE(F.lrunoff && F.frunoff && F.lrunoff_glc && F.frunoff_glc, MOM6X_EINVAL,
            "applyBoundaryFluxesInOut: fluxes%lrunoff, frunoff, lrunoff_glc and frunoff_glc are needed");
    REQUIRE(F.seaice_melt, MOM6X_EINVAL, "applyBoundaryFluxesInOut: fluxes%seaice_melt is needed");
    REQUIRE(nsw == 0 || (opacity_band && sw_pen_band), MOM6X_EINVAL,
            "applyBoundaryFluxesInOut: nsw > 0 needs optics%opacity_band and optics%sw_pen_band");
    REQUIRE(!P.use_river_heat_content || (F.heat_content_lrunoff && F.heat_content_lrunoff_glc), MOM6X_EINVAL,
            "applyBoundaryFluxesInOut: USE_RIVER_HEAT_CONTENT needs fluxes%heat_content_lrunoff and heat_content_lrunoff_glc");
    REQUIRE(!P.use_calving_heat_content || (F.heat_content_frunoff && F.heat_content_frunoff_glc), MOM6X_EINVAL,
            "applyBoundaryFluxesInOut: USE_CALVING_HEAT_CONTENT needs fluxes%heat_content_frunoff and heat_content_frunoff_glc");
    REQUIRE(!penSWflux_diag || penSW_diag, MOM6X_EINVAL, "applyBoundaryFluxesInOut: penSWflux_diag needs penSW_diag");
  }
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const bool cols = forcing || ener;   // :814

  if (cTKE || SkinBuoyFlux) {
    DaFill f;
    f.cTKE = cTKE; f.Skin = SkinBuoyFlux; f.own_cTKE = cols && ener; f.own_Skin = forcing && buoy;
    KLAUNCH(c, "k_da_fill", k_da_fill, dim3((unsigned)((d.slab + 255) / 256)), dim3(256), d, f);
  }
  if (!cols) { HIPCHK(hipGetLastError()); return MOM6X_OK; }

  DaK K;
  memset(&K, 0, sizeof(K));
  K.dt = dt; K.Idt = forcing ? 1.0 / dt : 0.0;
  K.H_to_Z = GV.H_to_Z; K.H_to_RZ = GV.H_to_RZ; K.RZ_to_H = GV.RZ_to_H;
  K.C_p = P.C_p; K.I_Cp = 1.0 / P.C_p; K.I_Cp_Hc = 1.0 / (GV.H_to_RZ * P.C_p);            // MOM_forcing_type.F90:554-555
  const double H_limit_fluxes = (GV.H_subroundoff > GV.Angstrom_H) ? GV.H_subroundoff : GV.Angstrom_H;   // :844
  K.Ih_limit = 0.0; if (H_limit_fluxes > 0.0) K.Ih_limit = 1.0 / H_limit_fluxes;           // MOM_forcing_type.F90:553
  K.Ih_limit_sw = 1.0 / H_limit_fluxes;                                                    // MOM_opacity.F90:832
  K.h_min_heat = 2.0 * GV.Angstrom_H + GV.H_subroundoff;                                   // MOM_opacity.F90:707
  K.gH = GV.g_Earth * GV.H_to_RZ;                                                          // :888
  K.p_to_Pa = P.RL2_T2_to_Pa;
  K.g_Hconv2 = (P.g_Earth_Z_T2 * GV.H_to_RZ) * GV.H_to_RZ;                                 // :810
  K.old_optics = P.optics_answer_date < 20190101;
  K.g_Hconv2_sw = K.old_optics ? K.g_Hconv2 : P.g_Earth_Z_T2 * (GV.H_to_RZ * GV.H_to_RZ);  // MOM_opacity.F90:713-717
  K.GoRho_H_to_Z = (P.g_Earth_Z_T2 / GV.Rho0) * GV.H_to_Z;                                 // :821, :1314
  K.RivermixConst = -0.5 * (P.rivermix_depth * dt) * P.g_Earth_Z_T2 * GV.Rho0;             // :1045
  K.ppt1000 = 1000.0 * P.ppt_to_S;
  K.dSalt_frac_max = P.dSalt_frac_max; K.H_subroundoff = GV.H_subroundoff;
  K.min_depth = minimum_forcing_depth; K.evap_CFL = evap_CFL_limit;
  K.zero = 0.0;
  K.min_SW_heat = P.PenSW_flux_absorb * dt; K.I_Habs = P.PenSW_absorb_Invlen;              // MOM_opacity.F90:704-705
  K.Rho_T0_S0 = s->eos.Rho_T0_S0; K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS; K.dRho_dp = s->eos.dRho_dp;
  K.form = s->use_eos ? s->eos.form : 0;
  K.forcing = forcing; K.agg = aggregate_FW_forcing != 0; K.buoy = buoy;
  K.rivermix = P.do_rivermix; K.river_heat = P.use_river_heat_content; K.calving_heat = P.use_calving_heat_content;
  K.ignore_land = P.ignore_fluxes_over_land;

  DaP A;
  memset(&A, 0, sizeof(A));
  if (forcing) A.F = *fluxes;
  A.opac = opacity_band; A.swpen = sw_pen_band; A.p_surf = tv_p_surf;
  A.h = h; A.T = T; A.S = S; A.cTKE = cTKE; A.dSV_dT = dSV_dT; A.dSV_dS = dSV_dS; A.Skin = SkinBuoyFlux;
  A.createdH = createdH; A.penSW = penSW_diag; A.penSWflux = penSWflux_diag; A.nonpenSW = nonpenSW_diag;
  A.cnt = s->cnt;

  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
  const int nb = forcing ? nsw : 0;
#define DAC(N, E) KLAUNCH(c, "k_da_cols<" #N ", " #E ">", (k_da_cols<N, E>), g, b, d, c->G, K, A)
#define DAN(N) do { if (ener) DAC(N, true); else DAC(N, false); } while (0)
  switch (nb) {
    case 0: DAN(0); break;
    case 1: DAN(1); break;
    case 2: DAN(2); break;
    case 3: DAN(3); break;
    default: DAN(4); break;
  }
#undef DAN
#undef DAC
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
