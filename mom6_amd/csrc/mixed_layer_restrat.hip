// mixed_layer_restrat.hip -- the mixed-layer eddy restratification of Fox-Kemper et al. on gfx950, general-coordinate (OM4) branch.
//
//   mixedlayer_restrat      <- MOM_mixed_layer_restrat.F90:149-186, the arm :183
//   mixedlayer_restrat_OM4  <- :189-714 (Boussinesq, no Stanley term, no open boundaries: G%OBCmaskCu/v are mask2dCu/v)
//   detect_mld              <- :1504-1571
//   mu                      <- :717-751
//   find_ustar(H_T_units)   <- MOM_forcing_type.F90:1271, the Boussinesq arm
//
// k_mle_cols: one lane per cell of the domain widened by one: MLD_fast (detect_mld, or MLE_MLD_STRETCH*h_MLD), the two running-mean
// filters in place, then the walk down that sums htot_fast | slow and Rml_int_fast | slow and stops once both sums are full (the
// reference stops a whole row at once; a column does not use the density after its own sums are full).  k_mle_faces: one lane per
// face, both directions in one launch (blockIdx.z): the two timescales, uDml | uDml_slow, the three walks with the CFL limiter, uhml
// and uhtr += uhml*dt.  a(k) and b(k) are not kept per thread (they would be arrays of nk in scratch memory): the later walks form
// them again from the same zpa | zpb recurrence.  h_avail (:394) is formed from h and areaT where it is read.  Once both interfaces
// of a layer lie below the (extended) mixed layer, mu is +0 there and in every layer further down, a(k) = b(k) = +0: the limiter
// walks stop and the last walk writes uhml = (+0*uDml) + (+0*uDml_slow) (the sign of that zero is the reference's) without reading
// h.  k_mle_cells: :667-671.  MAX and MIN are fmax1 and fmin1 of mom6x_dev.h with the reference's argument order.
#include "mom6x_dev.h"
#include "eos_dev.h"

// mixedlayer_restrat_CS, tv%eqn_of_state and the work array of mom6x_mixedlayer_restrat_init
struct MleState {
  mom6x_mixedlayer_restrat_params p;
  mom6x_eos_params eos;
  double *work;   // [htot_fast | htot_slow | Rml_av_fast | Rml_av_slow (2-D) | uhml | vhml (nk each)]
};

namespace {

struct MleK {
  double coef, coef2, front_length, aFac1, bFac1, aFac2, bFac2, density_diff, tail_dh, stretch, vonKar_x_pi2, ustar_min;
  double Angstrom_H, h_neglect, Z_to_H, g_Rho0, I4dt, dt;
  double Rho_T0_S0, dRho_dT, dRho_dS, dRho_dp;
  int detect, filt1, filt2, res_upscale;
};
struct MleDiag { double *ts[2], *Dml[2]; };

// mu(sigma, dh) :717-751.  below: sigma is at or under the base of the extended mixed layer in a way that holds for every smaller
// sigma as well (2*sigma+1 <= -1 and the un-clamped xp >= 1; both are monotone in sigma in floating point): mu is +0 there.
// TAIL false: MLE_TAIL_DH = 0, the exponent of :744 is 1 and x**1. is x.
template <bool TAIL>
__device__ __forceinline__ double mle_mu(double sigma, double dh, bool &below) {
  const double t = 2. * sigma + 1.;
  const double t2 = t * t;
  const double m = fmax1(0., (1. - t2) * (1. + (5. / 21.) * t2));
  const double raw = (-sigma - 0.5) * 2. / (1. + 2. * dh);
  const double xp = fmax1(0., fmin1(1., raw));
  double dd = fmax1(1. - (xp * xp) * (3. - 2. * xp), 0.);
  if (TAIL) dd = pow(dd, 1. + 2. * dh);
  const double bottop = 0.5 * (1. - copysign(1., sigma + 0.5));
  below = (t <= -1.) && (raw >= 1.);
  return fmax1(m, dd * bottop);
}

template <int FORM>
__device__ __forceinline__ double mle_rho(const MleK &K, double T, double S) {
  return eos_density(FORM, K.Rho_T0_S0, K.dRho_dT, K.dRho_dS, K.dRho_dp, T, S, 0.0);
}

// :300-348 and :384-426 on cells isc-1..iec+1, jsc-1..jec+1.  Lanes start at i = -IAL.
template <int FORM>
__global__ void __launch_bounds__(256)
k_mle_cols(Dm d, MleK K, const double *__restrict__ h, const double *__restrict__ T, const double *__restrict__ S,
           const double *__restrict__ h_MLD, double *__restrict__ MLD_filt, double *__restrict__ MLD_filt_slow,
           double *__restrict__ htot_f, double *__restrict__ htot_s, double *__restrict__ Rml_f, double *__restrict__ Rml_s,
           double *__restrict__ MLD_fast_out, double *__restrict__ MLD_slow_out, double *__restrict__ Rml_out) {
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni || j > d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  double MLD_fast;
  if (K.detect) {                                   // detect_mld :1532-1570
    double hm = h[x];
    double dK = 0.5 * hm;
    const double rhoSurf = mle_rho<FORM>(K, T[x], S[x]);
    double dRhoK = 0., MLD = 0.;
    size_t o = slab + x;
    for (int k = 1; k < nz; ++k, o += slab) {
      const double hk = h[o];
      const double dKm1 = dK;
      dK = dK + 0.5 * (hk + hm);
      const double dRhoKm1 = dRhoK;
      dRhoK = mle_rho<FORM>(K, T[o], S[o]) - rhoSurf;
      const double ddRho = dRhoK - dRhoKm1;
      if ((MLD == 0.) && (ddRho > 0.) && (dRhoKm1 < K.density_diff) && (dRhoK >= K.density_diff)) {
        const double aFac = (K.density_diff - dRhoKm1) / ddRho;
        MLD = dK * aFac + dKm1 * (1. - aFac);
      }
      hm = hk;
    }
    MLD_fast = K.stretch * MLD;
    if ((MLD_fast == 0.) && (dRhoK < K.density_diff)) MLD_fast = dK;   // mixing to the bottom
  } else {
    MLD_fast = K.stretch * h_MLD[x];                // :304
  }
  if (K.filt1) {                                    // :317-325
    const double f = fmax1(MLD_fast, K.bFac1 * MLD_fast + K.aFac1 * MLD_filt[x]);
    MLD_filt[x] = f;
    MLD_fast = f;
  }
  double MLD_slow = MLD_fast;
  if (K.filt2) {                                    // :335-343
    MLD_slow = fmax1(MLD_fast, K.bFac2 * MLD_fast + K.aFac2 * MLD_filt_slow[x]);
    MLD_filt_slow[x] = MLD_slow;
  }
  double hf = 0.0, hs = 0.0, Rf = 0.0, Rs = 0.0;    // :388-420
  size_t o = x;
  for (int k = 0; k < nz; ++k, o += slab) {
    const bool nf = hf < MLD_fast, ns = hs < MLD_slow;
    if (!nf && !ns) break;
    const double hk = h[o];
    const double rho = mle_rho<FORM>(K, T[o], S[o]);
    if (nf) {
      const double dh = fmin1(hk, MLD_fast - hf);
      Rf = Rf + dh * rho;
      hf = hf + dh;
    }
    if (ns) {
      const double dh = fmin1(hk, MLD_slow - hs);
      Rs = Rs + dh * rho;
      hs = hs + dh;
    }
  }
  const double Rav = -(K.g_Rho0 * Rf) / (hf + K.h_neglect);            // :423-424
  htot_f[x] = hf; htot_s[x] = hs;
  Rml_f[x] = Rav;
  Rml_s[x] = -(K.g_Rho0 * Rs) / (hs + K.h_neglect);
  if (MLD_fast_out) MLD_fast_out[x] = MLD_fast;
  if (MLD_slow_out) MLD_slow_out[x] = MLD_slow;
  if (Rml_out) Rml_out[x] = Rav;
}

// :486-574 | :578-664 on the faces of face_lane<0>.
template <bool TAIL>
__global__ void __launch_bounds__(256)
k_mle_faces(Dm d, const double *__restrict__ G, MleK K, const double *__restrict__ h, double *__restrict__ uhtr,
            double *__restrict__ vhtr, const double *__restrict__ ustar, const double *__restrict__ Rd, const double *__restrict__ fl,
            const double *__restrict__ htot_f, const double *__restrict__ htot_s, const double *__restrict__ Rml_f,
            const double *__restrict__ Rml_s, double *__restrict__ uhml, double *__restrict__ vhml, MleDiag D) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t x = f.x, y = f.y, ot = f.ot, slab = (size_t)d.slab;
  const int nz = d.nk;
  double *htr = dir ? vhtr : uhtr, *hml = dir ? vhml : uhml;
  const double hn = K.h_neglect, tdh = K.tail_dh;
  const double u_star = fmax1(K.ustar_min, 0.5 * (K.Z_to_H * ustar[x] + K.Z_to_H * ustar[y]));
  const double *Cor = gm(G, d, MOM6X_G_CoriolisBu);
  const double absf = 0.5 * (fabs(Cor[x - ot]) + fabs(Cor[x]));
  double res_fac = 0.0;
  if (K.res_upscale) {                               // :492-498 | :581-588
    const double lfront = 0.5 * ((fl ? fl[x] : K.front_length) + (fl ? fl[y] : K.front_length));
    double I_LFront = 0.0;
    if (lfront != 0.0) I_LFront = 1.0 / lfront;
    const double dx = gm(G, d, dir ? MOM6X_G_dxCv : MOM6X_G_dxCu)[x], dy = gm(G, d, dir ? MOM6X_G_dyCv : MOM6X_G_dyCu)[x];
    res_fac = (sqrt(0.5 * ((dx * dx) + (dy * dy))) * I_LFront) * fmin1(1., 0.5 * (Rd[x] + Rd[y]));
  }
  const double mask = gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  const double len = gm(G, d, dir ? MOM6X_G_dxCv : MOM6X_G_dyCu)[x], Ilen = gm(G, d, dir ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  const double hfs = htot_f[x] + htot_f[y], hss = htot_s[x] + htot_s[y];

  double h_vel = 0.5 * (hfs + hn);                   // :502-514
  double mom_mixrate = K.vonKar_x_pi2 * (u_star * u_star) / (absf * (h_vel * h_vel) + 4.0 * (h_vel + hn) * u_star);
  double timescale = 0.0625 * (absf + 2.0 * mom_mixrate) / (absf * absf + mom_mixrate * mom_mixrate);
  timescale = timescale * K.coef;
  if (K.res_upscale) timescale = timescale * res_fac;
  double Dml = timescale * mask * len * Ilen * (Rml_f[y] - Rml_f[x]) * (h_vel * h_vel);

  h_vel = 0.5 * (hss + hn);                          // :517-529
  mom_mixrate = K.vonKar_x_pi2 * (u_star * u_star) / (absf * (h_vel * h_vel) + 4.0 * (h_vel + hn) * u_star);
  timescale = 0.0625 * (absf + 2.0 * mom_mixrate) / (absf * absf + mom_mixrate * mom_mixrate);
  timescale = timescale * K.coef2;
  if (K.res_upscale) timescale = timescale * res_fac;
  double Dml_slow = timescale * mask * len * Ilen * (Rml_s[y] - Rml_s[x]) * (h_vel * h_vel);

  if (Dml + Dml_slow == 0.) {                        // :531-532
    size_t o = x;
    for (int k = 0; k < nz; ++k, o += slab) hml[o] = 0.0;
  } else {
    const double IhTot = 2.0 / (hfs + hn), IhTot_slow = 2.0 / (hss + hn);
    const double *areaT = gm(G, d, MOM6X_G_areaT);
    const double qL = K.I4dt * areaT[x], qR = K.I4dt * areaT[y];   // h_avail = max(I4dt*areaT*(h-Angstrom_H), 0.) :394
    bool bel;
    const double mu0 = mle_mu<TAIL>(0.0, tdh, bel);
    {                                                // :539-550
      double zpa = 0.0, mu_up = mu0;
      size_t o = x;
      for (int k = 0; k < nz; ++k, o += slab) {
        const double hL = h[o], hR = h[o + (y - x)];
        const double hAtVel = 0.5 * (hL + hR);
        zpa = zpa - (hAtVel * IhTot);
        const double mu_dn = mle_mu<TAIL>(zpa, tdh, bel);
        const double a = mu_up - mu_dn;
        if (a * Dml > 0.0) {
          const double ha = fmax1(qL * (hL - K.Angstrom_H), 0.0);
          if (a * Dml > ha) Dml = ha / a;
        } else if (a * Dml < 0.0) {
          const double ha = fmax1(qR * (hR - K.Angstrom_H), 0.0);
          if (-a * Dml > ha) Dml = -ha / a;
        }
        mu_up = mu_dn;
        if (bel) break;
      }
    }
    {                                                // :551-565
      double zpa = 0.0, zpb = 0.0, mua_up = mu0, mub_up = mu0;
      size_t o = x;
      for (int k = 0; k < nz; ++k, o += slab) {
        const double hL = h[o], hR = h[o + (y - x)];
        const double hAtVel = 0.5 * (hL + hR);
        zpa = zpa - (hAtVel * IhTot);
        const double mua_dn = mle_mu<TAIL>(zpa, tdh, bel);
        const double a = mua_up - mua_dn;
        zpb = zpb - (hAtVel * IhTot_slow);
        const double mub_dn = mle_mu<TAIL>(zpb, tdh, bel);
        const double b = mub_up - mub_dn;
        if (b * Dml_slow > 0.0) {
          const double lim = fmax1(qL * (hL - K.Angstrom_H), 0.0) - a * Dml;
          if (b * Dml_slow > lim) Dml_slow = fmax1(0., lim) / b;
        } else if (b * Dml_slow < 0.0) {
          const double lim = fmax1(qR * (hR - K.Angstrom_H), 0.0) + a * Dml;
          if (-b * Dml_slow > lim) Dml_slow = -fmax1(0., lim) / b;
        }
        mua_up = mua_dn; mub_up = mub_dn;
        if (bel) break;                              // (zpb is below: b = +0 from here on)
      }
    }
    {                                                // :566-569
      double zpa = 0.0, zpb = 0.0, mua_up = mu0, mub_up = mu0;
      size_t o = x;
      int k = 0;
      for (; k < nz; ++k, o += slab) {
        const double hAtVel = 0.5 * (h[o] + h[o + (y - x)]);
        bool bela, belb;
        zpa = zpa - (hAtVel * IhTot);
        const double mua_dn = mle_mu<TAIL>(zpa, tdh, bela);
        const double a = mua_up - mua_dn;
        zpb = zpb - (hAtVel * IhTot_slow);
        const double mub_dn = mle_mu<TAIL>(zpb, tdh, belb);
        const double b = mub_up - mub_dn;
        const double val = a * Dml + b * Dml_slow;
        hml[o] = val;
        htr[o] = htr[o] + val * K.dt;
        mua_up = mua_dn; mub_up = mub_dn;
        if (bela && belb) { ++k; o += slab; break; }
      }
      const double z = 0.0 * Dml + 0.0 * Dml_slow, zdt = z * K.dt;   // a(k) = b(k) = +0 below both mixed layers
      for (; k < nz; ++k, o += slab) {
        hml[o] = z;
        htr[o] = htr[o] + zdt;
      }
    }
  }
  if (D.ts[dir]) D.ts[dir][x] = timescale;           // :572-573
  if (D.Dml[dir]) D.Dml[dir][x] = Dml;
}

// :667-671 on the computational domain, one lane per cell and layer.
__global__ void __launch_bounds__(256)
k_mle_cells(Dm d, const double *__restrict__ G, double dt, double h_min, double *__restrict__ h, const double *__restrict__ uhml,
            const double *__restrict__ vhml) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), o = (size_t)blockIdx.z * (size_t)d.slab + x, p = (size_t)d.pitch;
  double hv = h[o] - dt * gm(G, d, MOM6X_G_IareaT)[x] * ((uhml[o] - uhml[o - 1]) + (vhml[o] - vhml[o - p]));
  if (hv < h_min) hv = h_min;
  h[o] = hv;
}

// the device's mu at n values (mom6x_mixedlayer_restrat_mu)
__global__ void __launch_bounds__(256)
k_mle_mu(const double *__restrict__ sigma, const double *__restrict__ dh, double *__restrict__ out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  bool bel;
  out[t] = (dh[t] == 0.) ? mle_mu<false>(sigma[t], 0., bel) : mle_mu<true>(sigma[t], dh[t], bel);
}

}  // namespace

void mixedlayer_restrat_free(mom6x_ctx *c) {
  MleState *s = c->mle;
  if (!s) return;
  (void)hipFree(s->work);
  delete s;
  c->mle = nullptr;
}

extern "C" int mom6x_mixedlayer_restrat_init(mom6x_ctx *c, const mom6x_mixedlayer_restrat_params *p, const mom6x_eos_params *eos) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_mixedlayer_restrat_init: null argument");
  REFUSE(p->use_Bodner, "mixedlayer_restrat_init", "MLE%USE_BODNER23 (mixedlayer_restrat_Bodner)");
  REFUSE(p->nkml, "mixedlayer_restrat_init", "a bulk mixed layer (NKML > 0, mixedlayer_restrat_BML)");
  REFUSE(p->use_Stanley_ML, "mixedlayer_restrat_init", "USE_STANLEY_ML");
  REFUSE(p->non_Boussinesq || !c->GV.Boussinesq, "mixedlayer_restrat_init", "non-Boussinesq mode (calculate_spec_vol, tau_mag)");
  REFUSE(p->open_bcs, "mixedlayer_restrat_init", "open boundary conditions (OBC)");
  REFUSE(p->debug, "mixedlayer_restrat_init", "DEBUG (the checksums of mixedlayer_restrat_OM4)");
  REQUIRE(eos, MOM6X_EINVAL, "mixedlayer_restrat_OM4: An equation of state must be used with this module.");
  REQUIRE(eos_form_known(eos), MOM6X_EINVAL, "mixedlayer_restrat_init: unknown EQN_OF_STATE form");
  REQUIRE(p->MLE_density_diff > 0. || p->MLE_use_PBL_MLD, MOM6X_EINVAL,
          "mixedlayer_restrat_OM4: No MLD to use for MLE parameterization.");
  REQUIRE(c->d.halo >= 1, MOM6X_EINVAL, "mixedlayer_restrat_init: mixedlayer_restrat needs a halo of one");
  HIPCHK(hipSetDevice(c->device));
  mixedlayer_restrat_free(c);
  const size_t n = (4 + 2 * (size_t)c->d.nk) * c->d.slab * sizeof(double);
  double *work = nullptr;
  HIPCHK(hipMalloc(&work, n));
  MleState *s = new MleState();
  s->p = *p;
  s->eos = *eos;
  s->work = work;
  c->mle = s;
  HIPCHK(hipMemsetAsync(s->work, work_fill_byte(), n, c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_mixedlayer_restrat(mom6x_ctx *c, double *h, double *uhtr, double *vhtr, const double *T, const double *S,
                                        const double *ustar, double dt, const double *h_MLD, const double *Rd_dx_h,
                                        const double *mle_fl, double *MLD_filtered, double *MLD_filtered_slow, double *uhml,
                                        double *vhml, double *utimescale, double *vtimescale, double *uDml, double *vDml,
                                        double *MLD_fast_out, double *MLD_slow_out, double *Rml_av_fast_out) {
  REQUIRE(c && c->mle, MOM6X_EINVAL, "mixedlayer_restrat: Module must be initialized before it is used.");
  const MleState *s = c->mle;
  const mom6x_mixedlayer_restrat_params &P = s->p;
  REQUIRE(h && uhtr && vhtr && T && S && ustar, MOM6X_EINVAL, "mixedlayer_restrat: null array (h, uhtr, vhtr, tv%T, tv%S, forces%ustar)");
  REQUIRE(dt > 0., MOM6X_EINVAL, "mixedlayer_restrat: dt must be positive");
  MleK K;
  K.detect = P.MLE_density_diff > 0.;
  REQUIRE(K.detect || h_MLD, MOM6X_EINVAL, "mixedlayer_restrat_OM4: h_MLD is needed with MLE_USE_PBL_MLD");
  K.filt1 = P.MLE_MLD_decay_time > 0.; K.filt2 = P.MLE_MLD_decay_time2 > 0.;
  REQUIRE(!K.filt1 || MLD_filtered, MOM6X_EINVAL, "mixedlayer_restrat_OM4: MLD_filtered is needed with MLE_MLD_DECAY_TIME > 0");
  REQUIRE(!K.filt2 || MLD_filtered_slow, MOM6X_EINVAL,
          "mixedlayer_restrat_OM4: MLD_filtered_slow is needed with MLE_MLD_DECAY_TIME2 > 0");
  const double *fl = nullptr;
  if (P.front_length > 0.) K.res_upscale = 1;                            // :355-374
  else if (P.front_length == 0. && mle_fl) { K.res_upscale = 1; fl = mle_fl; }
  else K.res_upscale = 0;
  REQUIRE(!K.res_upscale || Rd_dx_h, MOM6X_EINVAL,
          "mixedlayer_restrat_OM4: The resolution argument, Rd/dx (VarMix%Rd_dx_h), was not associated.");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_vgrid &GV = c->GV;
  K.coef = P.ml_restrat_coef; K.coef2 = P.ml_restrat_coef2; K.front_length = P.front_length;
  K.aFac1 = P.MLE_MLD_decay_time / (dt + P.MLE_MLD_decay_time); K.bFac1 = dt / (dt + P.MLE_MLD_decay_time);       // :317-318
  K.aFac2 = P.MLE_MLD_decay_time2 / (dt + P.MLE_MLD_decay_time2); K.bFac2 = dt / (dt + P.MLE_MLD_decay_time2);   // :335-336
  K.density_diff = P.MLE_density_diff; K.tail_dh = P.MLE_tail_dh; K.stretch = P.MLE_MLD_stretch;
  K.vonKar_x_pi2 = P.vonKar * 9.8696;                                     // :286
  K.ustar_min = P.ustar_min;
  K.Angstrom_H = GV.Angstrom_H; K.h_neglect = GV.H_subroundoff; K.Z_to_H = GV.Z_to_H;
  K.g_Rho0 = GV.H_to_Z * GV.g_Earth / GV.Rho0;                            // :353
  K.I4dt = 0.25 / dt; K.dt = dt;
  K.Rho_T0_S0 = s->eos.Rho_T0_S0; K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS; K.dRho_dp = s->eos.dRho_dp;
  const size_t n2 = (size_t)d.slab, n3 = (size_t)d.nk * n2;
  double *W = s->work;
  double *htot_f = W, *htot_s = W + n2, *Rml_f = W + 2 * n2, *Rml_s = W + 3 * n2;
  if (!uhml) uhml = W + 4 * n2;
  if (!vhml) vhml = W + 4 * n2 + n3;
  const dim3 b = blk2();
#define MLC(F)                                                                                                                   \
  KLAUNCH(c, "k_mle_cols<" #F ">", (k_mle_cols<F>), grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, K, h, T, S, h_MLD, MLD_filtered, \
          MLD_filtered_slow, htot_f, htot_s, Rml_f, Rml_s, MLD_fast_out, MLD_slow_out, Rml_av_fast_out)
  EOS_FORM_DISPATCH(s->eos.form, MLC);
#undef MLC
  MleDiag D;
  D.ts[0] = utimescale; D.ts[1] = vtimescale; D.Dml[0] = uDml; D.Dml[1] = vDml;
  const dim3 g = grid3(d.ni + IAL, d.nj + 1, 2, b);
  if (P.MLE_tail_dh == 0.)
    KLAUNCH(c, "k_mle_faces<0>", (k_mle_faces<false>), g, b, d, c->G, K, h, uhtr, vhtr, ustar, Rd_dx_h, fl, htot_f, htot_s, Rml_f, Rml_s,
            uhml, vhml, D);
  else
    KLAUNCH(c, "k_mle_faces<1>", (k_mle_faces<true>), g, b, d, c->G, K, h, uhtr, vhtr, ustar, Rd_dx_h, fl, htot_f, htot_s, Rml_f, Rml_s,
            uhml, vhml, D);
  KLAUNCH(c, "k_mle_cells", k_mle_cells, grid3(d.ni, d.nj, d.nk, b), b, d, c->G, dt, 0.5 * GV.Angstrom_H, h, uhml, vhml);   // h_min :282
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

extern "C" int mom6x_mixedlayer_restrat_mu(mom6x_ctx *c, const double *sigma, const double *dh, double *out, int n) {
  REQUIRE(c && sigma && dh && out && n >= 0, MOM6X_EINVAL, "mom6x_mixedlayer_restrat_mu: null argument");
  if (n == 0) return MOM6X_OK;
  HIPCHK(hipSetDevice(c->device));
  KLAUNCH(c, "k_mle_mu", k_mle_mu, dim3((n + 255) / 256), dim3(256), sigma, dh, out, n);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
