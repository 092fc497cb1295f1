// thickness_diffuse.hip -- isopycnal height diffusion (the Gent-McWilliams closure) on gfx950.
//
//   thickness_diffuse       <- MOM_thickness_diffuse.F90:134-630: the diffusivities :224-233, :240-250, :291-325, :343-353, :392-429,
//                              the update of uhtr, vhtr and h :600-615
//   thickness_diffuse_full  <- :635-1671 without the FGNV streamfunction: the column pass :864-882, the face pass :916-1213 /
//                              :1231-1530, layer 1 :1533-1535
//   find_eta                <- MOM_interface_heights.F90:91-97 (Boussinesq), vert_fill_TS <- MOM_isopycnal_slopes.F90:612-700
//
// Three launches.  k_td_cols: one lane per cell of the domain widened by one, top-down: h_avail_rsum, h_frac, pres and the
// tridiagonal solve of vert_fill_TS (any layer count: the solve's c1 goes through a work array).  k_td_faces: one lane per face,
// both directions in one launch (blockIdx.z), ONE bottom-up walk -- without the FGNV solver the two K = nz..2 loops of a face row
// carry only uhtot -- that forms e from h as it climbs (find_eta's own order), h_avail pointwise, writes uhD | vhD and adds them
// to uhtr | vhtr.  k_td_update: h.  MAX and MIN are fmax1 and fmin1 of mom6x_dev.h, but the limiter of uhD | vhD (:1160-1161, :1479) is
// dmax(dmin()): where no transport meets no available mass beyond the face, MAX(+0.0, -0.0), the compiled reference answers
// with its second argument, -0.0, which shows in uhGM | vhGM (found by tests/test_ref_parity_cpu.py on every grid).  The density
// gradients of MODE 1 (isoneutral_grads) and the vert_fill_TS solve come from isopycnal_slopes_dev.h, which
// lateral_mixing_coeffs.hip shares; the lane of a face from face_lane (mom6x_dev.h), the EOS form's kernel from EOS_FORM_DISPATCH.
#include "mom6x_dev.h"
#include "eos_dev.h"
#include "isopycnal_slopes_dev.h"

namespace {

// the scalars of :818-824 and vert_fill_TS :649-659, formed once on the host in the reference's order
struct TdK {
  double dt, I4dt, I_slope_max2, h_neglect, h_neglect2, dz_neglect, H_to_Z, Z_to_H, Angstrom_H, gH, Z_to_L, int_slope;
  double Khth, Khth_Min, Khth_Max, qCFL, kap_dt_x2, h0;
  double dRho_dT, dRho_dS;
};

// The column pass :864-882 on cells is-1..ie+1, js-1..je+1 and, with Tf, vert_fill_TS(halo_here=1, larger_h_denom=.true.).
// rsum[k], pres[k]: h_avail_rsum and pres at the interface ABOVE layer k.  Lanes start at i = -IAL (whole lines per wavefront).
__global__ void __launch_bounds__(256)
k_td_cols(Dm d, const double *__restrict__ G, TdK K, const double *__restrict__ h, const double *__restrict__ T,
          const double *__restrict__ S, const double *__restrict__ p_surf, double *__restrict__ rsum, double *__restrict__ hfrac,
          double *__restrict__ pres, double *Tf, double *Sf, double *c1) {
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni || j > d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  const double Ia = K.I4dt * gm(G, d, MOM6X_G_areaT)[x];
  double rs = 0.0, pr = p_surf ? p_surf[x] : 0.0;
  for (int k = 0; k < nz; ++k) {
    const size_t o = (size_t)k * slab + x;
    const double hk = h[o];
    const double ha = fmax1(Ia * (hk - K.Angstrom_H), 0.0);
    rsum[o] = rs;
    if (pres) pres[o] = pr;
    const double rn = k ? rs + ha : ha;
    if (hfrac) hfrac[o] = k ? ((ha > 0.0) ? ha / rn : 0.0) : 1.0;
    pr = pr + K.gH * hk;
    rs = rn;
  }
  if (!Tf) return;
  // vert_fill_TS :668-697, kap_dt_x2 > 0
  vert_fill_TS_col(h, T, S, Tf, Sf, c1, x, slab, nz, K.kap_dt_x2, K.h0, K.h_neglect);
}

// MODE 0: layers of constant density (:1085-1094); 1: an EOS of form FORM, slopes from the filled T, S; 2: an EOS with stored
// slopes (no density derivative, calc_derivatives :924); 3: constant density with stored slopes.
template <int FORM, int MODE>
__global__ void __launch_bounds__(256)
k_td_faces(Dm d, const double *__restrict__ G, TdK K, const double *__restrict__ h, double *__restrict__ uhtr,
           double *__restrict__ vhtr, const double *__restrict__ khth2d, const double *__restrict__ slope_x,
           const double *__restrict__ slope_y, const double *__restrict__ rsum, const double *__restrict__ hfrac,
           const double *__restrict__ pres, const double *__restrict__ Tf, const double *__restrict__ Sf,
           double *__restrict__ uhD, double *__restrict__ vhD) {
  constexpr bool EOS = (MODE == 1 || MODE == 2);
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t x = f.x, y = f.y, slab = (size_t)d.slab;
  const int nz = d.nk;
  double *htr = dir ? vhtr : uhtr, *hD = dir ? vhD : uhD;
  const double *slope = dir ? slope_y : slope_x;

  // KH_u_CFL, Khth_loc_u, KH_u(:,:,1) (:224-233, :240-250, :291-305) and their v twins
  const double Idx = gm(G, d, dir ? MOM6X_G_IdxCv : MOM6X_G_IdxCu)[x], Idy = gm(G, d, dir ? MOM6X_G_IdyCv : MOM6X_G_IdyCu)[x];
  const double KH_CFL = K.qCFL / (K.dt * ((Idx * Idx) + (Idy * Idy)));
  double Kh_loc = khth2d ? 0.5 * (khth2d[x] + khth2d[y]) : K.Khth;
  if (K.Khth_Max > 0) Kh_loc = fmax1(K.Khth_Min, fmin1(Kh_loc, K.Khth_Max));
  else Kh_loc = fmax1(K.Khth_Min, Kh_loc);
  const double KHlen = fmin1(KH_CFL, Kh_loc) * gm(G, d, dir ? MOM6X_G_dx_Cv : MOM6X_G_dy_Cu)[x];
  const double Igrad = dir ? Idy : Idx;
  const double mask = gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];   // OBCmaskCu/v without open boundaries
  const double *aT = gm(G, d, MOM6X_G_areaT), *bT = gm(G, d, MOM6X_G_bathyT);
  const double IaL = K.I4dt * aT[x], IaR = K.I4dt * aT[y];
  const double ebL = -(bT[x] + 0.0), ebR = -(bT[y] + 0.0);   // find_eta :91, dZ_ref = 0

  double elL = ebL, elR = ebR;   // e(:,K+1)
  double uhtot = 0.0;
  size_t o = (size_t)(nz - 1) * slab;
  double hLk = h[o + x], hRk = h[o + y];
  double TLk = 0.0, TRk = 0.0, SLk = 0.0, SRk = 0.0;
  if constexpr (MODE == 1) { TLk = Tf[o + x]; TRk = Tf[o + y]; SLk = Sf[o + x]; SRk = Sf[o + y]; }
  for (int k = nz - 1; k >= 1; --k, o -= slab) {
    const size_t om = o - slab;
    const double eL = elL + hLk * K.H_to_Z, eR = elR + hRk * K.H_to_Z;   // e(:,K), find_eta :96
    const double hLm = h[om + x], hRm = h[om + y];
    double TLm = 0.0, TRm = 0.0, SLm = 0.0, SRm = 0.0;
    double Slope, ratio = 0.0, Sfn_unlim;
    if constexpr (EOS) {
      if constexpr (MODE == 1) {
        TLm = Tf[om + x]; TRm = Tf[om + y]; SLm = Sf[om + x]; SRm = Sf[om + y];
        IsoGrad g;
        isoneutral_grads<FORM>(K, hLm, hRm, hLk, hRk, TLm, TRm, TLk, TRk, SLm, SRm, SLk, SRk, 0.5 * (pres[o + x] + pres[o + y]),
                               eL, eR, Igrad, g);
        if (g.mag_grad2 > 0.0) {
          Slope = g.drdx / sqrt(g.mag_grad2);
          ratio = Slope * Slope * K.I_slope_max2;
        } else {
          Slope = 0.0;
          ratio = 1.0e20;
        }
      } else {
        Slope = slope[o + x];
        ratio = Slope * Slope * K.I_slope_max2;
      }
      // :1049-1051 with int_slope_u = 0 (kept: it decides the sign of a zero slope)
      Slope = (1.0 - K.int_slope) * Slope + K.int_slope * ((eR - eL) * Igrad);
      ratio = (1.0 - K.int_slope) * ratio;
      Sfn_unlim = -(KHlen)*Slope;
      // no dense water upslope from below the bottom of the receiving side (:1067-1083)
      if (Sfn_unlim > 0.0) {
        if (eL < ebR) Sfn_unlim = 0.0;
        else if (ebR > elL) Sfn_unlim = Sfn_unlim * ((eL - ebR) / ((eL - elL) + K.dz_neglect));
      } else {
        if (eR < ebL) Sfn_unlim = 0.0;
        else if (ebL > elR) Sfn_unlim = Sfn_unlim * ((eR - ebL) / ((eR - elR) + K.dz_neglect));
      }
    } else {
      if constexpr (MODE == 3) Slope = slope[o + x];
      else Slope = ((eR - eL) * Igrad) * mask;
      Sfn_unlim = -(KHlen)*Slope;
    }

    // the second K loop (:1125-1190)
    const double haL_ = fmax1(IaL * (hLk - K.Angstrom_H), 0.0), haR_ = fmax1(IaR * (hRk - K.Angstrom_H), 0.0);
    double Sfn_est;
    if constexpr (EOS) {
      const double Sfn_safe = (uhtot <= 0.0) ? uhtot * (1.0 - hfrac[o + x]) : uhtot * (1.0 - hfrac[o + y]);
      Sfn_est = (K.Z_to_H * Sfn_unlim + ratio * Sfn_safe) / (1.0 + ratio);
    } else {
      Sfn_est = K.Z_to_H * Sfn_unlim;
    }
    const double Sfn_in_H = fmin1(fmax1(Sfn_est, -rsum[o + x]), rsum[o + y]);
    const double D = dmax(dmin((Sfn_in_H - uhtot), haL_), -haR_);   // :1160-1161, :1479: a tie here shows (see the header)
    uhtot = uhtot + D;
    hD[o + x] = D;
    htr[o + x] = htr[o + x] + D * K.dt;
    elL = eL; elR = eR; hLk = hLm; hRk = hRm;
    TLk = TLm; TRk = TRm; SLk = SLm; SRk = SRm;
  }
  // layer 1 (:1534-1535)
  const double D = -uhtot;
  hD[x] = D;
  htr[x] = htr[x] + D * K.dt;
}

// h(i,j,k) -= dt*IareaT*div(uhD, vhD) with the floor at Angstrom_H (:610-614)
__global__ void __launch_bounds__(256)
k_td_update(Dm d, const double *__restrict__ G, double dt, double Angstrom_H, double *__restrict__ h,
            const double *__restrict__ uhD, const double *__restrict__ vhD) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix3(d, i, j, blockIdx.z), p = (size_t)d.pitch;
  double hn = h[x] - dt * gm(G, d, MOM6X_G_IareaT)[ix2(d, i, j)] * ((uhD[x] - uhD[x - 1]) + (vhD[x] - vhD[x - p]));
  if (hn < Angstrom_H) hn = Angstrom_H;
  h[x] = hn;
}

}  // namespace

// thickness_diffuse_CS, tv%eqn_of_state, CS%khth2d and the work arrays of mom6x_thickness_diffuse_init
struct TdState {
  mom6x_thickness_diffuse_params P;
  bool use_eos; mom6x_eos_params eos;
  const double *khth2d;   // caller-owned device array (READ_KHTH)
  double *work;           // [uhD | vhD | h_avail_rsum] and, with an EOS, [h_frac | pres | T_f | S_f], nk levels each; null: nothing to diffuse
};

void thickness_diffuse_free(mom6x_ctx *c) {
  if (!c->td) return;
  (void)hipFree(c->td->work);
  delete c->td;
  c->td = nullptr;
}

extern "C" int mom6x_thickness_diffuse_init(mom6x_ctx *c, const mom6x_thickness_diffuse_params *p, const mom6x_eos_params *eos,
                                            const double *khth2d) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_thickness_diffuse_init: null argument");
  REFUSE(p->use_FGNV_streamfn, "thickness_diffuse_init", "KHTH_USE_FGNV_STREAMFUNCTION");
  REFUSE(p->use_stanley_gm, "thickness_diffuse_init", "USE_STANLEY_GM");
  REFUSE(p->detangle_interfaces, "thickness_diffuse_init", "DETANGLE_INTERFACES");
  REFUSE(p->Kh_eta_bg > 0.0, "thickness_diffuse_init", "KH_ETA_CONST > 0");
  REFUSE(p->Kh_eta_vel > 0.0, "thickness_diffuse_init", "KH_ETA_VEL_SCALE > 0");
  REFUSE(p->use_GME, "thickness_diffuse_init", "USE_GME");
  REFUSE(p->use_variable_mixing, "thickness_diffuse_init", "variable mixing (VarMix%use_variable_mixing)");
  REFUSE(p->use_MEKE, "thickness_diffuse_init", "MEKE (MEKE%Kh, MEKE%GM_src)");
  REFUSE(p->use_Kh_in_MEKE, "thickness_diffuse_init", "USE_KH_IN_MEKE");
  REFUSE(p->GMwork, "thickness_diffuse_init", "the GMwork diagnostic (find_work)");
  REFUSE(p->skeb_use_gm, "thickness_diffuse_init", "SKEB (STOCH%skeb_use_gm)");
  REFUSE(p->nkml != 0, "thickness_diffuse_init", "a bulk mixed layer (GV%nkml > 0)");
  REFUSE(p->open_bcs, "thickness_diffuse_init", "open boundary conditions");
  REFUSE(p->non_Boussinesq || !c->GV.Boussinesq, "thickness_diffuse_init", "non-Boussinesq mode (tv%SpV_avg, semi_Boussinesq)");
  REQUIRE(p->max_Khth_CFL > 0.0, MOM6X_EINVAL, "thickness_diffuse_init: KHTH_MAX_CFL <= 0 leaves KH_v unset in the reference");
  REQUIRE(!(p->read_khth && p->Khth > 0.0), MOM6X_EINVAL,
          "thickness_diffuse_init: KHTH > 0 is not compatible with READ_KHTH = TRUE. ");
  REQUIRE((p->read_khth != 0) == (khth2d != nullptr), MOM6X_EINVAL, "thickness_diffuse_init: khth2d comes with READ_KHTH");
  REQUIRE(p->slope_max > 0.0, MOM6X_EINVAL, "thickness_diffuse_init: KHTH_SLOPE_MAX must be positive");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "thickness_diffuse_init: unknown EQN_OF_STATE form");
  REQUIRE(!eos || c->d.nk >= 2, MOM6X_EINVAL, "thickness_diffuse_init: vert_fill_TS needs two layers");
  HIPCHK(hipSetDevice(c->device));
  thickness_diffuse_free(c);
  double *work = nullptr;
  const size_t n = (size_t)(eos ? 7 : 3) * c->d.nk * c->d.slab * sizeof(double);
  const bool active = p->thickness_diffuse && (p->Khth > 0.0 || p->read_khth);
  if (active) HIPCHK(hipMalloc(&work, n));
  TdState *s = new TdState();
  s->P = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  s->khth2d = khth2d;
  s->work = work;
  c->td = s;
  if (active) HIPCHK(hipMemsetAsync(work, work_fill_byte(), n, c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_thickness_diffuse(mom6x_ctx *c, double *h, double *uhtr, double *vhtr, const double *T, const double *S,
                                       const double *p_surf, const double *slope_x, const double *slope_y, double dt,
                                       double *uhGM, double *vhGM) {
  REQUIRE(c && c->td, MOM6X_EINVAL, "MOM_thickness_diffuse: Module must be initialized before it is used.");
  const TdState *s = c->td;
  const mom6x_thickness_diffuse_params &P = s->P;
  if (!P.thickness_diffuse || !(P.Khth > 0.0 || P.read_khth)) return MOM6X_OK;   // :195-197
  REQUIRE(h && uhtr && vhtr, MOM6X_EINVAL, "thickness_diffuse: null array");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "thickness_diffuse: dt must be positive");
  REQUIRE((slope_x != nullptr) == (slope_y != nullptr), MOM6X_EINVAL, "thickness_diffuse: slope_x and slope_y come together");
  REQUIRE((uhGM != nullptr) == (vhGM != nullptr), MOM6X_EINVAL, "thickness_diffuse: uhGM and vhGM come together");
  const bool use_eos = s->use_eos, stored = slope_x != nullptr;
  REQUIRE(!use_eos || stored || (T && S), MOM6X_EINVAL, "thickness_diffuse: an equation of state needs tv%T and tv%S");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_vgrid &GV = c->GV;
  TdK K;
  K.dt = dt;
  K.I4dt = 0.25 / dt;                                          // :818
  K.I_slope_max2 = 1.0 / (P.slope_max * P.slope_max);          // :819
  K.h_neglect = GV.H_subroundoff; K.h_neglect2 = K.h_neglect * K.h_neglect; K.dz_neglect = GV.dZ_subroundoff;   // :821-822
  K.H_to_Z = GV.H_to_Z; K.Z_to_H = GV.Z_to_H; K.Angstrom_H = GV.Angstrom_H;
  K.gH = GV.g_Earth * GV.H_to_RZ;                              // :872
  K.Z_to_L = P.Z_to_L; K.int_slope = 0.0;                      // :472-474
  K.Khth = P.Khth; K.Khth_Min = P.Khth_Min; K.Khth_Max = P.Khth_Max;
  K.qCFL = 0.25 * P.max_Khth_CFL;                              // :226
  K.kap_dt_x2 = (2.0 * (P.kappa_smooth * dt)) * P.Z_to_H_fill;  // MOM_isopycnal_slopes.F90:655
  K.h0 = 1.0e-16 * sqrt(0.5 * K.kap_dt_x2);                    // :658
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;
  const size_t n3 = (size_t)d.nk * d.slab;
  double *W = s->work;
  double *uD = uhGM ? uhGM : W, *vD = vhGM ? vhGM : W + n3, *rsum = W + 2 * n3;
  double *hfrac = use_eos ? W + 3 * n3 : nullptr;
  const bool derivs = use_eos && !stored;                      // calc_derivatives :924-925
  double *pres = derivs ? W + 4 * n3 : nullptr;
  const bool fill = derivs && K.kap_dt_x2 > 0.0;               // else T_f = T_in (MOM_isopycnal_slopes.F90:661-665): read in place
  double *Tf = fill ? W + 5 * n3 : nullptr, *Sf = fill ? W + 6 * n3 : nullptr;
  const dim3 b = blk2();
  KLAUNCH(c, "k_td_cols", k_td_cols, grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, c->G, K, h, T, S, p_surf, rsum, hfrac, pres, Tf,
          Sf, W);   // (c1 lives in the uhD work array until the face pass)
  const double *Tr = fill ? Tf : T, *Sr = fill ? Sf : S;
  const dim3 g = grid3(d.ni + IAL, d.nj + 1, 2, b);
#define TDF(F, M)                                                                                                            \
  KLAUNCH(c, "k_td_faces<" #F "," #M ">", (k_td_faces<F, M>), g, b, d, c->G, K, h, uhtr, vhtr, s->khth2d, slope_x, slope_y, \
          rsum, hfrac, pres, Tr, Sr, uD, vD)
  if (!use_eos) {
    if (stored) TDF(0, 3); else TDF(0, 0);
  } else if (stored) {
    TDF(0, 2);
  } else {
#define TDF_1(F) TDF(F, 1)
    EOS_FORM_DISPATCH(s->eos.form, TDF_1);
#undef TDF_1
  }
#undef TDF
  KLAUNCH(c, "k_td_update", k_td_update, grid3(d.ni, d.nj, d.nk, b), b, d, c->G, dt, GV.Angstrom_H, h, uD, vD);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
