// set_visc.hip -- the bottom boundary layer viscosity of the drag law on gfx950.
//
//   set_viscous_BBL  <- MOM_set_viscosity.F90:135-1115, the non-channel path of a Boussinesq grid:
//                       thickness at the face :465-509, background velocity :609-621, the near-bottom walk :623-700,
//                       pressure and EOS derivatives :701-711, the density walk :720-840, thickness :842-876,
//                       viscosity and Rayleigh drag :1019-1086; set_v_at_u / set_u_at_v :1819-1906.
//
// One lane per face, lanes along i, both face directions in one launch (blockIdx.z).  A lane keeps no column in
// registers: each walk re-reads h, T, S and the velocities of its two cells, which sit in L2 after the first walk.  MIN: dmin.
#include "mom6x_dev.h"
#include "eos_dev.h"

namespace {

// the scalars of set_viscous_BBL :331-348, formed once on the host
struct SvK {
  double cdrag, cdrag_sqrt, cdrag_sqrt_H, cdrag_L_to_H, drag_bg_vel, Hbbl, dz_bbl, BBL_thick_min, Kv_BBL_min, BBL_thick_max;
  double Rho0x400_G, HRg, H_to_Z, h_neglect, dz_neglect, Angstrom_H, dRho_dT, dRho_dS;
  int linear_drag, tidal_bg, body_force, correct_bounds, RiNo_mix;
};

// h_at_vel / dz_at_vel (:470-479): upwind-biased harmonic mean where the flow goes from thin to thick, else the plain mean
__device__ __forceinline__ void at_vel(double vel, double hL, double hR, double H_to_Z, double h_neglect, double dz_neglect,
                                       double &h_at, double &dz_at) {
  const double dzL = H_to_Z * hL, dzR = H_to_Z * hR;   // thickness_to_dz (MOM_interface_heights.F90), Boussinesq
  if (vel * (hR - hL) >= 0) {
    h_at = 2.0 * hL * hR / (hL + hR + h_neglect);
    dz_at = 2.0 * dzL * dzR / (dzL + dzR + dz_neglect);
  } else {
    h_at = 0.5 * (hL + hR);
    dz_at = 0.5 * (dzL + dzR);
  }
}

// set_v_at_u (:1819-1860) at u face (i, j), layer plane hk / vk (no open boundaries)
__device__ __forceinline__ double v_at_u(const double *hk, const double *vk, const double *mCv, size_t x, size_t p) {
  const double w0m = (hk[x - p] + hk[x]) * mCv[x - p];             // hwt(0,-1)
  const double w1m = (hk[x + 1 - p] + hk[x + 1]) * mCv[x + 1 - p]; // hwt(1,-1)
  const double w00 = (hk[x] + hk[x + p]) * mCv[x];                 // hwt(0,0)
  const double w10 = (hk[x + 1] + hk[x + 1 + p]) * mCv[x + 1];     // hwt(1,0)
  const double tot = (w0m + w10) + (w1m + w00);
  if (!(tot > 0.0)) return 0.0;
  return (((w00 * vk[x]) + (w1m * vk[x + 1 - p])) + ((w10 * vk[x + 1]) + (w0m * vk[x - p]))) / tot;
}

// set_u_at_v (:1863-1906) at v face (i, J)
__device__ __forceinline__ double u_at_v(const double *hk, const double *uk, const double *mCu, size_t x, size_t p) {
  const double wm0 = (hk[x - 1] + hk[x]) * mCu[x - 1];             // hwt(-1,0)
  const double w00 = (hk[x] + hk[x + 1]) * mCu[x];                 // hwt(0,0)
  const double wm1 = (hk[x - 1 + p] + hk[x + p]) * mCu[x - 1 + p]; // hwt(-1,1)
  const double w01 = (hk[x + p] + hk[x + 1 + p]) * mCu[x + p];     // hwt(0,1)
  const double tot = (wm0 + w01) + (w00 + wm1);
  if (!(tot > 0.0)) return 0.0;
  return (((w00 * uk[x]) + (wm1 * uk[x - 1 + p])) + ((wm0 * uk[x - 1]) + (w01 * uk[x + p]))) / tot;
}

// FORM: the EOS form of use_BBL_EOS, 0 for the GV%Rlay walk.  The lane: face_lane<0> (mom6x_dev.h) written out, 0.6 % faster so.
template <int FORM>
__global__ void __launch_bounds__(256)
k_set_viscous_BBL(Dm d, const double *__restrict__ G, SvK K, const double *__restrict__ u, const double *__restrict__ v,
                  const double *__restrict__ h, const double *__restrict__ T, const double *__restrict__ S,
                  const double *__restrict__ p_surf, const double *__restrict__ tideamp, const double *__restrict__ Rlay,
                  double *__restrict__ Kv_u, double *__restrict__ Kv_v, double *__restrict__ bt_u, double *__restrict__ bt_v,
                  double *__restrict__ Ray_u, double *__restrict__ Ray_v) {
  constexpr bool EOS = FORM != 0;
  const int dir = blockIdx.z;
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (dir == 0 ? (i < -1 || j < 0) : (i < 0)) return;
  const size_t x = ix2(d, i, j), p = (size_t)d.pitch, st = dir ? p : 1, y = x + st, slab = (size_t)d.slab;
  if (!(gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x] > 0.0)) return;   // do_i (:453-464)
  const int nz = d.nk;
  const double *vel = dir ? v : u, *oth = dir ? u : v;
  const double *mO = gm(G, d, dir ? MOM6X_G_mask2dCu : MOM6X_G_mask2dCv);
  double *Ray = dir ? Ray_v : Ray_u;

  // u2_bg (:609-621)
  double u2_bg;
  if (K.tidal_bg) {
    const double *mT = gm(G, d, MOM6X_G_mask2dT);
    u2_bg = 0.5 * (mT[x] * (tideamp[x] * tideamp[x]) + mT[y] * (tideamp[y] * tideamp[y]));
  } else {
    u2_bg = K.drag_bg_vel * K.drag_bg_vel;
  }

  // the near-bottom walk over at most Hbbl (:623-700)
  double ustar, umag_avg = 0.0, h_bbl_drag = 0.0, dz_bbl_drag = 0.0, T_EOS = 0.0, S_EOS = 0.0;
  if (EOS || K.body_force || !K.linear_drag) {
    double htot_vel = 0.0, hwtot = 0.0, hutot = 0.0, dztot_vel = 0.0, dzwtot = 0.0, Thtot = 0.0, Shtot = 0.0;
    for (int k = nz - 1; k >= 0; --k) {
      if (htot_vel >= K.Hbbl) break;
      const size_t o = (size_t)k * slab;
      double h_at, dz_at;
      at_vel(vel[o + x], h[o + x], h[o + y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
      const double hweight = dmin(K.Hbbl - htot_vel, h_at);
      if (hweight < 1.5 * K.Angstrom_H + K.h_neglect) continue;
      const double dzweight = dmin(K.dz_bbl - dztot_vel, dz_at);
      htot_vel = htot_vel + h_at;
      hwtot = hwtot + hweight;
      dztot_vel = dztot_vel + dz_at;
      dzwtot = dzwtot + dzweight;
      if (!K.linear_drag && hweight >= 0.0) {
        const double w = vel[o + x];
        const double a = dir ? u_at_v(h + o, oth + o, mO, x, p) : v_at_u(h + o, oth + o, mO, x, p);
        hutot = hutot + hweight * sqrt(w * w + a * a + u2_bg);
      }
      if (EOS && hweight >= 0.0) {
        Thtot = Thtot + hweight * (0.5 * (T[o + x] + T[o + y]));
        Shtot = Shtot + hweight * (0.5 * (S[o + x] + S[o + y]));
      }
    }
    const double I_hwtot = (hwtot > 0.0) ? 1.0 / hwtot : 0.0;
    if (hwtot <= 0.0 || K.linear_drag) ustar = K.cdrag_sqrt_H * K.drag_bg_vel;
    else ustar = K.cdrag_sqrt_H * hutot / hwtot;
    umag_avg = hutot * I_hwtot;
    h_bbl_drag = hwtot;
    dz_bbl_drag = dzwtot;
    if (EOS && hwtot > 0.0) { T_EOS = Thtot / hwtot; S_EOS = Shtot / hwtot; }
  } else {
    ustar = K.cdrag_sqrt_H * K.drag_bg_vel;
  }

  // pressure at the bottom, summed top-down, and the density derivatives there (:701-711)
  double dR_dT = 0.0, dR_dS = 0.0;
  if constexpr (EOS) {
    double press = p_surf ? 0.5 * (p_surf[x] + p_surf[y]) : 0.0;
    for (int k = 0; k < nz; ++k) {
      const size_t o = (size_t)k * slab;
      press = press + K.HRg * (0.5 * (h[o + x] + h[o + y]));
    }
    eos_density_derivs<FORM>(K, T_EOS, S_EOS, press, dR_dT, dR_dS);
  }

  // the stratification-limited thickness, bottom-up (:720-840)
  const double ustarsq = K.Rho0x400_G * (ustar * ustar);
  double htot = 0.0, dztot = 0.0;
  if (EOS) {
    double Thtot = 0.0, Shtot = 0.0, oldfn = 0.0;
    for (int k = nz - 1; k >= 1; --k) {
      const size_t o = (size_t)k * slab, om = o - slab;
      double h_at, dz_at;
      at_vel(vel[o + x], h[o + x], h[o + y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
      if (h_at <= 0.0) continue;
      const double Tk = 0.5 * (T[o + x] + T[o + y]), Sk = 0.5 * (S[o + x] + S[o + y]);
      oldfn = dR_dT * (Thtot - Tk * htot) + dR_dS * (Shtot - Sk * htot);
      if (oldfn >= ustarsq) break;
      const double Tm = 0.5 * (T[om + x] + T[om + y]), Sm = 0.5 * (S[om + x] + S[om + y]);
      const double Dfn = (dR_dT * (Tk - Tm) + dR_dS * (Sk - Sm)) * (h_at + htot);
      double Dh, Ddz;
      if ((oldfn + Dfn) <= ustarsq) { Dh = h_at; Ddz = dz_at; }
      else {
        const double frac_used = sqrt((ustarsq - oldfn) / (Dfn));
        Dh = h_at * frac_used; Ddz = dz_at * frac_used;
      }
      htot = htot + Dh;
      dztot = dztot + Ddz;
      Thtot = Thtot + Tk * Dh; Shtot = Shtot + Sk * Dh;
    }
    double h_at, dz_at;
    at_vel(vel[x], h[x], h[y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
    if ((oldfn < ustarsq) && h_at > 0.0) {   // layer 1 might be part of the BBL
      const double T1 = 0.5 * (T[x] + T[y]), S1 = 0.5 * (S[x] + S[y]);
      if (dR_dT * (Thtot - T1 * htot) + dR_dS * (Shtot - S1 * htot) < ustarsq) { htot = htot + h_at; dztot = dztot + dz_at; }
    }
  } else {   // GV%Rlay, nkml = 0: K2 = 2
    double Rhtot = 0.0;
    for (int k = nz - 1; k >= 1; --k) {
      const size_t o = (size_t)k * slab;
      double h_at, dz_at;
      at_vel(vel[o + x], h[o + x], h[o + y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
      const double Rk = Rlay[k];
      const double oldfn = Rhtot - Rk * htot;
      const double Dfn = (Rk - Rlay[k - 1]) * (h_at + htot);
      double Dh, Ddz;
      if (oldfn >= ustarsq) continue;
      else if ((oldfn + Dfn) <= ustarsq) { Dh = h_at; Ddz = dz_at; }
      else {
        const double frac_used = sqrt((ustarsq - oldfn) / (Dfn));
        Dh = h_at * frac_used; Ddz = dz_at * frac_used;
      }
      htot = htot + Dh;
      dztot = dztot + Ddz;
      Rhtot = Rhtot + Rk * Dh;
    }
    if (Rhtot - Rlay[0] * htot < ustarsq) {
      double h_at, dz_at;
      at_vel(vel[x], h[x], h[y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
      htot = htot + h_at; dztot = dztot + dz_at;
    }
  }

  // Killworth and Edwards (1999) eq. 2.20 with the rotation of 2f at the face (:842-876)
  const double *q = gm(G, d, MOM6X_G_CoriolisBu);
  const double C2f = dir ? q[x - 1] + q[x] : q[x - p] + q[x];
  double bbl_thick;
  if (K.cdrag * u2_bg <= 0.0) {
    const double ustH = ustar, root = sqrt(0.25 * (ustH * ustH) + (htot * C2f) * (htot * C2f));
    if (dztot * ustH <= (K.BBL_thick_min + K.dz_neglect) * (0.5 * ustH + root)) bbl_thick = K.BBL_thick_min;
    else bbl_thick = (dztot * ustH) / (0.5 * ustH + root);
  } else {
    bbl_thick = dztot / (0.5 + sqrt(0.25 + htot * htot * C2f * C2f / (ustar * ustar)));
    if (bbl_thick < K.BBL_thick_min) bbl_thick = K.BBL_thick_min;
  }
  if ((bbl_thick > 0.5 * K.dz_bbl) && K.RiNo_mix) bbl_thick = 0.5 * K.dz_bbl;
  if (K.body_force) bbl_thick = dz_bbl_drag;

  // viscosity (:1019-1047)
  double kv_bbl;
  if (K.correct_bounds && K.cdrag_sqrt * ustar * bbl_thick <= K.Kv_BBL_min) {
    kv_bbl = K.Kv_BBL_min;
    if ((K.cdrag_sqrt * ustar) * K.BBL_thick_max > kv_bbl) bbl_thick = kv_bbl / (K.cdrag_sqrt * ustar);
    else bbl_thick = K.BBL_thick_max;
  } else {
    kv_bbl = (K.cdrag_sqrt * ustar) * bbl_thick;
  }

  // DRAG_AS_BODY_FORCE: Rayleigh drag over the bottommost h_bbl_drag, bottom-up (:1049-1070)
  if (K.body_force && h_bbl_drag > 0.0) {
    double h_sum = 0.0;
    const double I_hwtot = 1.0 / h_bbl_drag;
    for (int k = nz - 1; k >= 0; --k) {
      const size_t o = (size_t)k * slab;
      double h_at, dz_at;
      at_vel(vel[o + x], h[o + x], h[o + y], K.H_to_Z, K.h_neglect, K.dz_neglect, h_at, dz_at);
      const double h_bbl_fr = dmin(h_bbl_drag - h_sum, h_at) * I_hwtot;
      Ray[o + x] = Ray[o + x] + (K.cdrag_L_to_H * umag_avg) * h_bbl_fr;
      h_sum = h_sum + h_at;
      if (h_sum >= h_bbl_drag) break;
    }
    kv_bbl = K.Kv_BBL_min;
  }
  kv_bbl = dmax(K.Kv_BBL_min, kv_bbl);
  (dir ? bt_v : bt_u)[x] = bbl_thick;
  double *Kv = dir ? Kv_v : Kv_u;
  if (Kv) Kv[x] = kv_bbl;
}

}  // namespace

// set_visc_CS of set_viscous_BBL, tv%eqn_of_state when use_BBL_EOS, CS%tideamp (caller-owned device array); owns no device memory
struct SvState { mom6x_set_visc_params P; bool use_eos; mom6x_eos_params eos; const double *tideamp; };
void set_visc_free(mom6x_ctx *c) { delete c->sv; c->sv = nullptr; }

extern "C" int mom6x_set_visc_init(mom6x_ctx *c, const mom6x_set_visc_params *p, const mom6x_eos_params *eos, const double *tideamp) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_set_visc_init: null argument");
  REQUIRE(!p->channel_drag, MOM6X_EINVAL, "set_visc_init: CHANNEL_DRAG (find_L_open_*) is not on the device");
  REQUIRE(p->nkml == 0, MOM6X_EINVAL, "set_visc_init: a bulk mixed layer (nkml > 0) is not on the device");
  REQUIRE(!p->open_bcs, MOM6X_EINVAL, "set_visc_init: open boundary conditions are not on the device path of set_viscous_BBL");
  REQUIRE(!p->ice_shelf, MOM6X_EINVAL, "set_visc_init: ice shelves are not on the device path of set_viscous_BBL");
  REQUIRE(!p->SpV_avg && c->GV.Boussinesq, MOM6X_EINVAL, "set_visc_init: the non-Boussinesq tv%SpV_avg forms are not on the device");
  REQUIRE(!(p->bottomdraglaw && p->BBL_use_tidal_bg) || tideamp, MOM6X_EINVAL, "set_visc_init: BBL_USE_TIDAL_BG needs CS%tideamp");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "set_visc_init: unknown EQN_OF_STATE form");
  if (!c->sv) c->sv = new SvState();
  SvState *s = c->sv;
  s->P = *p;
  s->use_eos = eos && p->BBL_use_EOS;   // use_BBL_EOS (:340)
  if (eos) s->eos = *eos;
  s->tideamp = tideamp;
  return MOM6X_OK;
}

extern "C" int mom6x_set_viscous_BBL(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *T, const double *S,
                                     const double *p_surf, double *Kv_bbl_u, double *Kv_bbl_v, double *bbl_thick_u, double *bbl_thick_v,
                                     double *Ray_u, double *Ray_v) {
  REQUIRE(c && c->sv, MOM6X_EINVAL, "MOM_set_viscosity(BBL): Module must be initialized before it is used.");
  const SvState *s = c->sv;
  const mom6x_set_visc_params &P = s->P;
  const double *Rlay = PressureForce_Rlay(c);   // the device copy of GV%Rlay
  if (!P.bottomdraglaw) return MOM6X_OK;   // :323
  REQUIRE(u && v && h && bbl_thick_u && bbl_thick_v, MOM6X_EINVAL, "set_viscous_BBL: null array");
  REQUIRE((Kv_bbl_u != nullptr) == (Kv_bbl_v != nullptr), MOM6X_EINVAL, "set_viscous_BBL: Kv_bbl_u and Kv_bbl_v come together");
  REQUIRE((Ray_u != nullptr) == (Ray_v != nullptr), MOM6X_EINVAL, "set_viscous_BBL: Ray_u and Ray_v come together");
  REQUIRE(!P.body_force_drag || Ray_u, MOM6X_EINVAL, "set_viscous_BBL: DRAG_AS_BODY_FORCE needs visc%Ray_u/v");
  REQUIRE(!s->use_eos || (T && S), MOM6X_EINVAL, "set_viscous_BBL: BBL_USE_EOS needs tv%T and tv%S");
  REQUIRE(s->use_eos || Rlay, MOM6X_EINVAL, "set_viscous_BBL: without BBL_USE_EOS the walk needs GV%Rlay (mom6x_PressureForce_init)");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_vgrid &GV = c->GV;
  SvK K;
  K.cdrag = P.cdrag;
  K.cdrag_sqrt = sqrt(P.cdrag);
  K.cdrag_sqrt_H = K.cdrag_sqrt * P.L_to_H;
  K.cdrag_L_to_H = P.cdrag * P.L_to_H;
  K.drag_bg_vel = P.drag_bg_vel;
  K.Hbbl = P.Hbbl; K.dz_bbl = P.dz_bbl; K.BBL_thick_min = P.BBL_thick_min; K.Kv_BBL_min = P.Kv_BBL_min;
  K.BBL_thick_max = P.Rad_Earth * P.L_to_Z;
  K.Rho0x400_G = 400.0 * (GV.H_to_RZ / ((P.L_to_Z * P.L_to_Z) * GV.g_Earth));
  K.HRg = GV.H_to_RZ * GV.g_Earth;
  K.H_to_Z = GV.H_to_Z; K.h_neglect = GV.H_subroundoff; K.dz_neglect = GV.dZ_subroundoff; K.Angstrom_H = GV.Angstrom_H;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;
  K.linear_drag = P.linear_drag; K.tidal_bg = P.BBL_use_tidal_bg; K.body_force = P.body_force_drag;
  K.correct_bounds = P.correct_BBL_bounds; K.RiNo_mix = P.RiNo_mix;
  if (Ray_u) {   // :442-443
    HIPCHK(hipMemsetAsync(Ray_u, 0, (size_t)d.nk * d.slab * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(Ray_v, 0, (size_t)d.nk * d.slab * sizeof(double), c->stream));
  }
  const dim3 b = blk2(), g = grid3(d.ni + IAL, d.nj + 1, 2, b);
#define SVB(F)                                                                                                              \
  KLAUNCH(c, "k_set_viscous_BBL<" #F ">", k_set_viscous_BBL<F>, g, b, d, c->G, K, u, v, h, T, S, p_surf, s->tideamp,      \
          Rlay, Kv_bbl_u, Kv_bbl_v, bbl_thick_u, bbl_thick_v, Ray_u, Ray_v)
  if (!s->use_eos) SVB(0);
  else EOS_FORM_DISPATCH(s->eos.form, SVB);
#undef SVB
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
