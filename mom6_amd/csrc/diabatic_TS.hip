// diabatic_TS.hip -- the in-place modifiers of tv%T and tv%S around the column physics of diabatic on gfx950: make_frazil and
// adjust_salt of MOM_diabatic_aux, geothermal_in_place of MOM_geothermal.
//
//   k_frazil_cols<PDF>   <- make_frazil, MOM_diabatic_aux.F90:110-230: the mid-layer pressures :158-165 (PDF:
//                           PRESSURE_DEPENDENT_FRAZIL), the reclaim arm :167-189, the walk :191-220, the sum :221-223
//   eos_TFreeze          <- calculate_TFreeze_1d, MOM_EOS.F90:664-744 (eos_dev.h)
//   k_salt_cols          <- adjust_salt, MOM_diabatic_aux.F90:339-390
//   k_geo_fill           <- geothermal_in_place, MOM_geothermal.F90:434, :436 (the whole-array fills) and :520-524 (the heat
//                           tendency of the layers that take no heat)
//   k_geo_cols<BF>       <- geothermal_in_place, MOM_geothermal.F90:439-513 (BF: BFlx_geothermal :440-460), :500, :523
//   calculate_density_derivs <- eos_dev.h
//
// Every column kernel is one lane per column, consecutive lanes along i.  The reference walks a j slice layer by layer; the layers
// of a column are coupled only through per-column scalars (fraz_col, salt_add_col, heat_rem, h_geo_rem), and the freezing point
// of a row is computed from S and the pressure, which the routine does not change, so one lane's walk gives the reference's
// results.  The walks read T (or S) of every layer and the other operands only where the reference's gate lets a layer through.
//
// make_frazil's pressures are a top-down recurrence (:160-163) that a bottom-up walk cannot recover bit for bit by subtraction:
// with the switch the lane writes them into the module's nk-level work array and reads its own words back, in the one kernel.
//
// geothermal_in_place departs from the reference in one place, the j-row skip :476: see include/mom6x.h.
// MAX is fmax1; x**2 is x*x.
#include "mom6x_dev.h"
#include "eos_dev.h"

namespace {

// the lane of a kernel over the computational domain widened by `halo`: rows from j = -halo, lanes along i from -IAL when the range
// starts below 0 (mom6x_dev.h)
__device__ __forceinline__ bool wide_lane(const Dm &d, int halo, int &i, int &j) {
  i = (halo > 0 ? -IAL : 0) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  j = -halo + (int)(blockIdx.y * blockDim.y + threadIdx.y);
  return i >= -halo && i < d.ni + halo && j < d.nj + halo;
}
inline dim3 wide_grid(const Dm &d, int halo, dim3 b) { return grid3(nxa(d.ni + 2 * halo, -halo), d.nj + 2 * halo, 1, b); }

// the scalars of make_frazil, formed once on the host in the reference's order, and what eos_TFreeze reads
struct FzK {
  double CpH;          // tv%C_p*GV%H_to_RZ :179, :202
  double half_H_to_p;  // 0.5*H_to_RL2_T2 :160
  double h_thin;       // 10.0*(GV%Angstrom_H + GV%H_subroundoff) :203
  double zero;         // 0.0 as a run-time value (eos_TFreeze)
  double RL2_T2_to_Pa, S_to_ppt, degC_to_C, TFr_S0_P0, dTFr_dS, dTFr_dp;
  int form_of_TFreeze, reclaim, halo;
};

// PDF: pressure_dependent_frazil.  pres: the work array (PDF only)
template <bool PDF>
__global__ void __launch_bounds__(256) k_frazil_cols(Dm d, const double *__restrict__ G, FzK K, const double *__restrict__ h,
                                                     double *__restrict__ T, const double *__restrict__ S,
                                                     double *__restrict__ frazil, const double *__restrict__ p_surf,
                                                     double *__restrict__ pres) {
  int i, j;
  if (!wide_lane(d, K.halo, i, j)) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;

  double p1 = 0.0;
  if constexpr (PDF) {   // :158-165
    const double ps = p_surf ? p_surf[x] : 0.0;
    double h_above = h[x];
    double p = ps + K.half_H_to_p * h_above;
    pres[x] = p; p1 = p;
    for (int k = 1; k < nz; ++k) {
      const size_t o = (size_t)k * slab + x;
      const double hk = h[o];
      p = p + K.half_H_to_p * (hk + h_above);
      pres[o] = p;
      h_above = hk;
    }
  }

  double fraz = frazil[x];
  if (K.reclaim && fraz > 0.0) {   // :167-189, land columns too
    const double T_freeze = eos_TFreeze(K, S[x], p1);
    const double T1 = T[x];
    if (T1 > T_freeze) {
      const double hc = K.CpH * h[x];
      if (fraz - hc * (T1 - T_freeze) <= 0.0) {
        T[x] = T1 - fraz / hc;
        fraz = 0.0;
      } else {
        fraz = fraz - hc * (T1 - T_freeze);
        T[x] = T_freeze;
      }
    }
  }

  double fraz_col = 0.0;
  if (gm(G, d, MOM6X_G_mask2dT)[x] > 0.0) {   // :191-220
    for (int k = nz - 1; k >= 0; --k) {
      const size_t o = (size_t)k * slab + x;
      const double Tk = T[o];
      if ((Tk < 0.0) || (fraz_col > 0.0)) {
        double pk = 0.0;
        if constexpr (PDF) pk = pres[o];
        const double T_freeze = eos_TFreeze(K, S[o], pk);
        const double hk = h[o];
        const double hc = K.CpH * hk;
        if (hk <= K.h_thin) {
          if (Tk < T_freeze) {
            fraz_col = fraz_col + hc * (T_freeze - Tk);
            T[o] = T_freeze;
          }
        } else if ((fraz_col > 0.0) || (Tk < T_freeze)) {
          if (fraz_col + hc * (T_freeze - Tk) < 0.0) {
            T[o] = Tk - fraz_col / hc;
            fraz_col = 0.0;
          } else {
            fraz_col = fraz_col + hc * (T_freeze - Tk);
            T[o] = T_freeze;
          }
        }
      }
    }
  }
  frazil[x] = fraz + fraz_col;   // :221-223
}

// adjust_salt: the computational domain only
__global__ void __launch_bounds__(256) k_salt_cols(Dm d, const double *__restrict__ G, double H_to_RZ, double h_thin, double S_min,
                                                   const double *__restrict__ h, double *__restrict__ S,
                                                   double *__restrict__ salt_deficit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  double salt_add_col = 0.0;
  if (gm(G, d, MOM6X_G_mask2dT)[x] > 0.0) {   // :365-383
    for (int k = d.nk - 1; k >= 0; --k) {
      const size_t o = (size_t)k * slab + x;
      const double Sk = S[o];
      if ((Sk < S_min) || (salt_add_col > 0.0)) {
        const double hk = h[o];
        const double mc = H_to_RZ * hk;
        if (hk <= h_thin) {
          if (Sk < S_min) {
            salt_add_col = salt_add_col + mc * (S_min - Sk);
            S[o] = S_min;
          }
        } else if (salt_add_col + mc * (S_min - Sk) <= 0.0) {
          S[o] = Sk - salt_add_col / mc;
          salt_add_col = 0.0;
        } else {
          salt_add_col = salt_add_col + mc * (S_min - Sk);
          S[o] = S_min;
        }
      }
    }
  }
  salt_deficit[x] = salt_deficit[x] + salt_add_col;   // :384-386
}

// the scalars of geothermal_in_place
struct GeoK {
  double dtIrho_cp;    // dt*Irho_cp :472
  double thick, Angstrom, H_neglect, Idt, H_to_pres, H_to_RZ;
  double HCp;          // GV%H_to_RZ*tv%C_p :523
  double gI_Rho0sq;    // GV%g_Earth_Z_T2*I_Rho0squared :458
  double I_Cp, p_to_Pa;
  double dRho_dT, dRho_dS;   // the linear EOS
  int form, halo;
};
struct GeoP { double *internal_heat, *BFlx, *dTdt, *tend; };

// one lane per point of a plane: the fills of the arrays that k_geo_cols does not write as a whole.  Inside the range of the
// call BFlx is k_geo_cols's; the heat tendency of a layer there is the product :523 with dTdt_diag = 0.0, rewritten by
// k_geo_cols where the layer takes heat
__global__ void __launch_bounds__(256) k_geo_fill(Dm d, GeoK K, GeoP P, const double *__restrict__ h) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= d.slab) return;
  const int j = r / d.pitch - d.joff, i = r - (j + d.joff) * d.pitch - d.ioff;
  const bool in = i >= -K.halo && i < d.ni + K.halo && j >= -K.halo && j < d.nj + K.halo;
  if (P.BFlx && !in) P.BFlx[r] = 0.0;
  if (P.dTdt)
    for (int k = 0; k < d.nk; ++k) P.dTdt[(size_t)k * d.slab + r] = 0.0;
  if (P.tend)
    for (int k = 0; k < d.nk; ++k) {
      const size_t o = (size_t)k * d.slab + r;
      P.tend[o] = in ? K.HCp * (h[o] * 0.0) : 0.0;
    }
}

__device__ __forceinline__ void geo_density_derivs(const GeoK &K, double T, double S, double p, double &a, double &b) {
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

// BF: BFlx_geothermal is asked for
template <bool BF>
__global__ void __launch_bounds__(256) k_geo_cols(Dm d, const double *__restrict__ G, GeoK K, GeoP P,
                                                  const double *__restrict__ geo_heat, const double *__restrict__ h,
                                                  double *__restrict__ T, const double *__restrict__ S) {
  int i, j;
  if (!wide_lane(d, K.halo, i, j)) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  const double mask = gm(G, d, MOM6X_G_mask2dT)[x], gh = geo_heat[x];

  if constexpr (BF) {   // :440-460
    double bottom_pressure = 0.0;
    for (int k = 0; k < nz; ++k) bottom_pressure = bottom_pressure + K.H_to_pres * h[(size_t)k * slab + x];
    double dRhodT = 0.0, dRhodS = 0.0;   // :453-454; EOSdom :423 is the computational domain along i
    if (i >= 0 && i < d.ni) {
      const size_t o = (size_t)(nz - 1) * slab + x;
      geo_density_derivs(K, T[o], S[o], K.p_to_Pa * bottom_pressure, dRhodT, dRhodS);
    }
    P.BFlx[x] = -((K.gI_Rho0sq * ((K.I_Cp * dRhodT) * gh)) * mask);
  }

  const double heat_in = mask * (gh * K.dtIrho_cp);   // :472
  double heat_rem = heat_in, h_geo_rem = K.thick;
  for (int k = nz - 1; k >= 0 && heat_rem > 0.0; --k) {   // :482-507
    const size_t o = (size_t)k * slab + x;
    const double hk = h[o];
    if (hk > K.Angstrom) {
      double heat_here;
      if ((hk - K.Angstrom) >= h_geo_rem) {
        heat_here = heat_rem;
        h_geo_rem = 0.0;
        heat_rem = 0.0;
      } else {
        heat_here = heat_rem * ((hk - K.Angstrom) / (h_geo_rem + K.H_neglect));
        h_geo_rem = h_geo_rem - (hk - K.Angstrom);
        heat_rem = heat_rem - heat_here;
      }
      const double dTemp = heat_here / (hk + K.H_neglect);
      T[o] = T[o] + dTemp;
      if (P.dTdt) P.dTdt[o] = dTemp * K.Idt;
      if (P.tend) P.tend[o] = K.HCp * (hk * (dTemp * K.Idt));
    }
  }
  if (P.internal_heat) P.internal_heat[x] = P.internal_heat[x] + K.H_to_RZ * (heat_in - heat_rem);   // :509-512, in every row
}

}  // namespace

// what make_frazil reads of diabatic_aux_CS, tv and tv%eqn_of_state with its `pressure` work array; geothermal_CS with CS%geo_heat on
// the device and tv%eqn_of_state
struct DtsState {
  bool frazil_init; mom6x_frazil_params F; double *pres;   // nk levels, with pressure_dependent_frazil only
  bool geo_init; mom6x_geothermal_params Geo; double *geo_heat; bool use_eos; mom6x_eos_params eos;
};

void diabatic_TS_free(mom6x_ctx *c) {
  if (!c->dts) return;
  (void)hipFree(c->dts->pres);
  (void)hipFree(c->dts->geo_heat);
  delete c->dts;
  c->dts = nullptr;
}

static DtsState *dts_state(mom6x_ctx *c) {
  if (!c->dts) c->dts = new DtsState();   // (all members zero)
  return c->dts;
}

static bool halo_ok(const mom6x_ctx *c, int halo) { return halo >= 0 && halo <= c->d.halo; }

extern "C" int mom6x_make_frazil_init(mom6x_ctx *c, const mom6x_frazil_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_make_frazil_init: null argument");
  REFUSE(p->form_of_TFreeze == MOM6X_TFREEZE_TEOS10, "make_frazil_init", "TFREEZE_FORM = TEOS10 (it needs the GSW library)");
  REFUSE(p->use_conT_absS, "make_frazil_init", "use_conT_absS (the gsw_sp_from_sr and gsw_ct_from_pt conversions)");
  REQUIRE(p->form_of_TFreeze == MOM6X_TFREEZE_LINEAR || p->form_of_TFreeze == MOM6X_TFREEZE_MILLERO ||
          p->form_of_TFreeze == MOM6X_TFREEZE_TEOSPOLY, MOM6X_EINVAL, "make_frazil_init: form_of_TFreeze is not valid.");
  REQUIRE(p->C_p > 0.0, MOM6X_EINVAL, "make_frazil_init: C_p must be positive");
  HIPCHK(hipSetDevice(c->device));
  DtsState *s = dts_state(c);
  s->frazil_init = false;
  if (s->pres) { HIPCHK(hipFree(s->pres)); s->pres = nullptr; }
  if (p->pressure_dependent_frazil) {
    const size_t n = (size_t)c->dims.slab * c->dims.nk;
    HIPCHK(hipMalloc(&s->pres, n * sizeof(double)));
    HIPCHK(hipMemsetAsync(s->pres, work_fill_byte(), n * sizeof(double), c->stream));
  }
  s->F = *p;
  s->frazil_init = true;
  return MOM6X_OK;
}

extern "C" int mom6x_make_frazil(mom6x_ctx *c, const double *h, double *T, const double *S, double *frazil, const double *p_surf,
                                 int halo) {
  REQUIRE(c && c->dts && c->dts->frazil_init, MOM6X_EINVAL, "make_frazil: Module must be initialized before it is used.");
  REQUIRE(h && T && S && frazil, MOM6X_EINVAL, "make_frazil: null h, tv%T, tv%S or tv%frazil");
  REQUIRE(halo_ok(c, halo), MOM6X_EINVAL, "make_frazil: halo must be between 0 and the context's halo");
  const DtsState *s = c->dts;
  const mom6x_frazil_params &P = s->F;
  const mom6x_vgrid &GV = c->GV;
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  FzK K;
  memset(&K, 0, sizeof(K));
  K.CpH = P.C_p * GV.H_to_RZ;
  const double H_to_RL2_T2 = GV.H_to_RZ * GV.g_Earth;   // :146
  K.half_H_to_p = 0.5 * H_to_RL2_T2;
  K.h_thin = 10.0 * (GV.Angstrom_H + GV.H_subroundoff);
  K.zero = 0.0;
  K.RL2_T2_to_Pa = P.RL2_T2_to_Pa; K.S_to_ppt = P.S_to_ppt; K.degC_to_C = P.degC_to_C;
  K.TFr_S0_P0 = P.TFr_S0_P0; K.dTFr_dS = P.dTFr_dS; K.dTFr_dp = P.dTFr_dp;
  K.form_of_TFreeze = P.form_of_TFreeze; K.reclaim = P.reclaim_frazil; K.halo = halo;
  const dim3 b = blk2(), g = wide_grid(d, halo, b);
  if (P.pressure_dependent_frazil)
    KLAUNCH(c, "k_frazil_cols<true>", k_frazil_cols<true>, g, b, d, c->G, K, h, T, S, frazil, p_surf, s->pres);
  else
    KLAUNCH(c, "k_frazil_cols<false>", k_frazil_cols<false>, g, b, d, c->G, K, h, T, S, frazil, p_surf, s->pres);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_adjust_salt(mom6x_ctx *c, const double *h, double *S, double *salt_deficit, double min_salinity) {
  REQUIRE(c, MOM6X_EINVAL, "adjust_salt: null ctx");
  REQUIRE(h && S && salt_deficit, MOM6X_EINVAL, "adjust_salt: null h, tv%S or tv%salt_deficit");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
  KLAUNCH(c, "k_salt_cols", k_salt_cols, g, b, d, c->G, c->GV.H_to_RZ, 10.0 * c->GV.Angstrom_H, min_salinity, h, S, salt_deficit);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_geothermal_init(mom6x_ctx *c, const mom6x_geothermal_params *p, const double *geo_heat_host_plane,
                                     const mom6x_eos_params *eos) {
  REQUIRE(c && p && geo_heat_host_plane, MOM6X_EINVAL, "mom6x_geothermal_init: null argument");
  REFUSE(!c->GV.Boussinesq, "geothermal_init", "non-Boussinesq mode (calculate_specific_vol_derivs, MOM_geothermal.F90:444-451)");
  REQUIRE(p->C_p > 0.0, MOM6X_EINVAL, "geothermal_init: C_p must be positive");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "geothermal_init: unknown EQN_OF_STATE form");
  HIPCHK(hipSetDevice(c->device));
  DtsState *s = dts_state(c);
  s->geo_init = false;
  const size_t n = (size_t)c->dims.slab * sizeof(double);
  if (!s->geo_heat) HIPCHK(hipMalloc(&s->geo_heat, n));
  HIPCHK(hipMemcpyAsync(s->geo_heat, geo_heat_host_plane, n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));   // the host plane is the caller's again
  s->Geo = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  s->geo_init = true;
  return MOM6X_OK;
}

extern "C" int mom6x_geothermal_in_place(mom6x_ctx *c, const double *h, double *T, const double *S, double dt, double *internal_heat,
                                         double *BFlx_geothermal, double *dTdt_diag, double *heat_tend_diag, int halo) {
  REQUIRE(c && c->dts && c->dts->geo_init, MOM6X_EINVAL, "MOM_geothermal: Module must be initialized before it is used.");
  const DtsState *s = c->dts;
  const mom6x_geothermal_params &P = s->Geo;
  const mom6x_vgrid &GV = c->GV;
  REQUIRE(h && T, MOM6X_EINVAL, "geothermal_in_place: null h or tv%T");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "geothermal_in_place: dt must be positive");
  REQUIRE(halo_ok(c, halo), MOM6X_EINVAL, "geothermal_in_place: halo must be between 0 and the context's halo");
  REQUIRE(!BFlx_geothermal || s->use_eos, MOM6X_EINVAL, "geothermal_in_place: BFlx_geothermal needs an equation of state");
  REQUIRE(!BFlx_geothermal || S, MOM6X_EINVAL, "geothermal_in_place: BFlx_geothermal needs tv%S");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  GeoK K;
  memset(&K, 0, sizeof(K));
  const double Irho_cp = 1.0 / (GV.H_to_RZ * P.C_p);   // :416
  K.dtIrho_cp = dt * Irho_cp;
  K.thick = P.geothermal_thick; K.Angstrom = GV.Angstrom_H; K.H_neglect = GV.H_subroundoff;
  K.Idt = 1.0 / dt;
  K.H_to_pres = GV.H_to_RZ * GV.g_Earth;               // :420
  K.H_to_RZ = GV.H_to_RZ;
  K.HCp = GV.H_to_RZ * P.C_p;
  K.I_Cp = 1. / P.C_p;
  const double I_Rho0squared = 1. / (GV.Rho0 * GV.Rho0);   // :422
  K.gI_Rho0sq = P.g_Earth_Z_T2 * I_Rho0squared;
  K.p_to_Pa = P.RL2_T2_to_Pa;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;
  K.form = s->use_eos ? s->eos.form : 0;
  K.halo = halo;
  GeoP A;
  A.internal_heat = internal_heat; A.BFlx = BFlx_geothermal; A.dTdt = dTdt_diag; A.tend = heat_tend_diag;

  if (BFlx_geothermal || dTdt_diag || heat_tend_diag)
    KLAUNCH(c, "k_geo_fill", k_geo_fill, dim3((unsigned)((d.slab + 255) / 256)), dim3(256), d, K, A, h);
  const dim3 b = blk2(), g = wide_grid(d, halo, b);
  if (BFlx_geothermal) KLAUNCH(c, "k_geo_cols<true>", k_geo_cols<true>, g, b, d, c->G, K, A, s->geo_heat, h, T, S);
  else KLAUNCH(c, "k_geo_cols<false>", k_geo_cols<false>, g, b, d, c->G, K, A, s->geo_heat, h, T, S);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
