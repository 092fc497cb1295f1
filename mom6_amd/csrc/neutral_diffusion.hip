// neutral_diffusion.hip -- epineutral tracer mixing of MOM_neutral_diffusion on gfx950, continuous reconstruction (NDIFF_CONTINUOUS).
//
//   neutral_diffusion_calc_coeffs              <- src/tracer/MOM_neutral_diffusion.F90:351-616, continuous arm
//   neutral_diffusion                          <- :619-1032 without vertical structure or tapering
//   interface_scalar, ppm_edge, ppm_ave        <- :1091-1130 (i_method = 2), :1135-1177, :1181-1211
//   signum, PLM_diff, fv_diff                  <- :1215-1222, :1226-1291 (c_method = 2, b_method = 1), :1297-1321
//   find_neutral_surface_positions_continuous  <- :1368-1573      interpolate_for_nondim_position <- :1578-1619
//   absolute_position                          <- :2279-2295      neutral_surface_flux <- :2318-2496, continuous arm
//   ppm_left_right_edge_values                 <- :2562-2585
//   calculate_density_derivs                   <- MOM_EOS.F90:781-829, every form of eos_dev.h
//
// Every per-column and per-face array of the reference lives in the module's resident arrays, as stacks of pitched planes with the
// column or face index fastest: the lanes of a wavefront touch one level of one array in consecutive words.  Scalars live in
// registers; no lane holds an array, so nothing is kept in scratch memory.
//   k_ndiff_interface  one lane per column of isc-1..iec+1 x jsc-1..jec+1: Pint, Tint, Sint, dRdT, dRdS.  interface_scalar streams
//                      down the column (nd_interface_scalar): it needs diff(k-1) and diff(k) only, which are formed from the layers
//                      as it goes.
//   k_ndiff_positions  one lane per face, both directions in one launch (face_lane): the walk over the 2 nk + 2 surfaces, which is
//                      sequential, with kl, kr, the last position and the last absolute positions in registers; the interface
//                      columns are indexed by the data-dependent kl, kr in global memory.  hEff leaves with the factor :592-597.
//   k_ndiff_edges      per tracer, one lane per column: Til, aL, aR.
//   k_ndiff_flux       per tracer, one lane per face: Flx on the 2 nk + 1 sublayers, and trans_x_2d | trans_y_2d.
//   k_ndiff_update     per tracer, one lane per cell: the divergence :894-937, the underflow, tendency.  With ndiff_answer_date >
//                      20240330 the four directional sums of a layer are running sums over the surfaces whose Ko is that layer
//                      (Ko is monotone in the surface index), which is the reference's order of additions.  The earlier arm adds
//                      the four directions surface by surface into dTracer(:), which is a column of the workspace.
// Every loop is bounded by nk.  There is no barrier.  bl_kl = bl_kr = 1 and bl_zl = bl_zr = 0 as the reference passes them (:543):
// the clamp :1541-1554 then sets KoL = 1 where KoL <= 1 and PoL = 0 where PoL < 0, which is what they already are.
//
// The reference's `stop` and FATAL sites cannot be reached with h >= 0.  A lane that does reach one adds to the module's counter of
// the site, raises MOM6X_FLAG_NEUTRAL_DIFFUSION in the context's flag (mom6x_ctx_sync then returns MOM6X_ENUMERIC) and goes on with
// an index inside the column.  `stop 'Else what?'` (:1539) has no counter: the first surface always sets one of the two search
// flags (:1434-1450) and every later statement keeps exactly one of them set.
//
// x**2 is x*x.  MAX and MIN are fmax1 and fmin1; SIGN is copysign (the sign of a negative zero counts, as in the compiled
// reference).  The literal 0. of max(0., x) :1588 is the run-time K.zero (see energetic_PBL.hip).  The EOS form is a
// wavefront-uniform switch (EOS_FORM_DISPATCH).
#include "mom6x_dev.h"
#include "eos_dev.h"
#include <cmath>
#include <vector>

namespace {

enum { ND_ERR_KM1 = 0, ND_ERR_PPOS, ND_ERR_DX_NEG, ND_ERR_DX_BIG, ND_NERR };

struct NdK {
  double gHRZ, pa_to_H, ref_pres, h_neglect, zero, p_to_Pa, C_to_degC, S_to_ppt, dRdT_scale, dRdS_scale, dRho_dT, dRho_dS;
  int form;
};
// the coefficients of one face direction, [surface][slab]
struct NdCoef { double *PoL, *PoR, *hEff; short *KoL, *KoR; };

__device__ __forceinline__ void nd_stop(int *flag, int *err, int site) {
  atomicOr(flag, MOM6X_FLAG_NEUTRAL_DIFFUSION);
  atomicAdd(err + site, 1);
}

// signum(1., x) :1215
__device__ __forceinline__ double nd_sgn1(double x) { return (x == 0.) ? 0. : copysign(1., x); }

// fv_diff :1297
__device__ __forceinline__ double nd_fv_diff(double hkm1, double hk, double hkp1, double Skm1, double Sk, double Skp1) {
  double h_sum = (hkm1 + hkp1) + hk;
  if (h_sum != 0.) h_sum = 1. / h_sum;
  double hm = hkm1 + hk;
  if (hm != 0.) hm = 1. / hm;
  double hp = hkp1 + hk;
  if (hp != 0.) hp = 1. / hp;
  return (hk * h_sum) * (((2. * hkm1 + hk) * hp) * (Skp1 - Sk) + ((2. * hkp1 + hk) * hm) * (Sk - Skm1));
}

// diff(k) of PLM_diff :1248-1282 for an interior layer, c_method = 2
__device__ __forceinline__ double nd_plm_diff(double hkm1, double hk, double hkp1, double Skm1, double Sk, double Skp1) {
  if ((hkp1 + hk) * (hkm1 + hk) > 0.) {
    const double diff_c = nd_fv_diff(hkm1, hk, hkp1, Skm1, Sk, Skp1);
    const double diff_l = 2. * (Sk - Skm1);
    const double diff_r = 2. * (Skp1 - Sk);
    if (nd_sgn1(diff_l) * nd_sgn1(diff_r) <= 0.) return 0.;   // PCM for local extrema
    return copysign(fmin1(fmin1(fabs(diff_l), fabs(diff_c)), fabs(diff_r)), diff_c);
  }
  return 0.;   // PCM next to vanished layers
}

// ppm_edge :1135
__device__ __forceinline__ double nd_ppm_edge(double hkm1, double hk, double hkp1, double hkp2, double Ak, double Akp1, double Pk,
                                              double Pkp1, double h_neglect) {
  double R_hk_hkp1 = hk + hkp1;
  if (R_hk_hkp1 <= 0.) return 0.5 * (Ak + Akp1);
  R_hk_hkp1 = 1. / R_hk_hkp1;
  double edge;
  if (hk < hkp1) edge = Ak + (hk * R_hk_hkp1) * (Akp1 - Ak);
  else edge = Akp1 + (hkp1 * R_hk_hkp1) * (Ak - Akp1);
  const double R_2hk_hkp1 = 1. / ((2. * hk + hkp1) + h_neglect);
  const double R_hk_2hkp1 = 1. / ((hk + 2. * hkp1) + h_neglect);
  const double f1 = 1. / ((hk + hkp1) + (hkm1 + hkp2));
  const double f2 = ((2. * (hkp1 * hk)) * R_hk_hkp1) * ((hkm1 + hk) * R_2hk_hkp1 - (hkp2 + hkp1) * R_hk_2hkp1);
  const double f3 = (hk * (hkm1 + hk)) * R_2hk_hkp1;
  const double f4 = (hkp1 * (hkp1 + hkp2)) * R_hk_2hkp1;
  return edge + f1 * (f2 * (Akp1 - Ak) - (f3 * Pkp1 - f4 * Pk));
}

// interface_scalar :1091-1130 with i_method = 2 down one column: h and S point at layer 1, st is the stride between layers, and
// put(K, Si(K)) is called for K = 1 .. nk + 1 in turn.  PLM_diff(nk, h, S, 2, 1, diff): diff(1) = diff(nk) = 0 (b_method = 1).
template <class Put>
__device__ __forceinline__ void nd_interface_scalar(const double *h, const double *S, size_t st, int nk, double h_neglect, Put put) {
  double diff_km1 = 0.;
  put(1, S[0] - 0.5 * diff_km1);
  for (int k = 2; k <= nk; ++k) {
    double diff_k = 0.;
    if (k <= nk - 1)
      diff_k = nd_plm_diff(h[(size_t)(k - 2) * st], h[(size_t)(k - 1) * st], h[(size_t)k * st], S[(size_t)(k - 2) * st],
                           S[(size_t)(k - 1) * st], S[(size_t)k * st]);
    const int km2 = (k - 2 > 1) ? k - 2 : 1, kp1 = (k + 1 < nk) ? k + 1 : nk;
    put(k, nd_ppm_edge(h[(size_t)(km2 - 1) * st], h[(size_t)(k - 2) * st], h[(size_t)(k - 1) * st], h[(size_t)(kp1 - 1) * st],
                       S[(size_t)(k - 2) * st], S[(size_t)(k - 1) * st], diff_km1, diff_k, h_neglect));
    diff_km1 = diff_k;
  }
  put(nk + 1, S[(size_t)(nk - 1) * st] + 0.5 * diff_km1);
}

// the lane of a column of isc-1..iec+1 x jsc-1..jec+1
__device__ __forceinline__ bool nd_column_lane(const Dm &d, int &i, int &j) {
  i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  return i >= -1 && i <= d.ni && j <= d.nj;
}

// :436-445, :472-473, :492-496
__global__ void __launch_bounds__(256)
k_ndiff_interface(Dm d, NdK K, const double *__restrict__ h, const double *__restrict__ T, const double *__restrict__ S,
                  const double *__restrict__ p_surf, double *Pint, double *Tint, double *Sint, double *__restrict__ dRdT,
                  double *__restrict__ dRdS) {
  int i, j;
  if (!nd_column_lane(d, i, j)) return;
  const size_t x = ix2(d, i, j), sl = (size_t)d.slab;
  const int nk = d.nk;
  double P = p_surf ? p_surf[x] : 0.;
  Pint[x] = P;
  for (int k = 1; k <= nk; ++k) {
    P = P + h[x + (size_t)(k - 1) * sl] * K.gHRZ;
    Pint[x + (size_t)k * sl] = P;
  }
  nd_interface_scalar(h + x, T + x, sl, nk, K.h_neglect, [&](int k, double v) { Tint[x + (size_t)(k - 1) * sl] = v; });
  nd_interface_scalar(h + x, S + x, sl, nk, K.h_neglect, [&](int k, double v) { Sint[x + (size_t)(k - 1) * sl] = v; });
  for (int k = 1; k <= nk + 1; ++k) {
    const size_t o = x + (size_t)(k - 1) * sl;
    const double pres = (K.ref_pres >= 0.) ? K.ref_pres : Pint[o];
    const double Ta = K.C_to_degC * Tint[o], Sa = K.S_to_ppt * Sint[o], pPa = K.p_to_Pa * pres;   // MOM_EOS.F90:813-815
    double dR_dT = 0., dR_dS = 0.;
#define ND_EOS(F) eos_density_derivs<F>(K, Ta, Sa, pPa, dR_dT, dR_dS)
    EOS_FORM_DISPATCH(K.form, ND_EOS);
#undef ND_EOS
    dRdT[o] = K.dRdT_scale * dR_dT;   // :820-827
    dRdS[o] = K.dRdS_scale * dR_dS;
  }
}

// interpolate_for_nondim_position :1578
__device__ __forceinline__ double nd_interpolate(double dRhoNeg, double Pneg, double dRhoPos, double Ppos, double zero, int *flag,
                                                 int *err) {
  if ((Ppos > Pneg) && (dRhoPos - dRhoNeg >= 0.)) {
    if (dRhoPos - dRhoNeg > 0.) return fmin1(1., fmax1(zero, -dRhoNeg / (dRhoPos - dRhoNeg)));
    if (dRhoPos - dRhoNeg == 0.) {
      if (dRhoNeg > 0.) return 0.;
      if (dRhoNeg < 0.) return 1.;
      return 0.5;
    }
    return 0.5;
  }
  if (Ppos == Pneg) return 0.5;   // vanished or inverted layers
  nd_stop(flag, err, ND_ERR_PPOS);   // :1616 (the caller comes with dRhoNeg < dRhoPos: this is Ppos < Pneg)
  return 0.5;
}

// 0.5 * ( ( dRdTa + dRdTb ) * ( Ta - Tb ) + ( dRdSa + dRdSb ) * ( Sa - Sb ) ) of :1431, :1455-1459, :1498-1502
__device__ __forceinline__ double nd_drho(double aTa, double aTb, double Ta, double Tb, double aSa, double aSb, double Sa, double Sb) {
  return 0.5 * ((aTa + aTb) * (Ta - Tb) + (aSa + aSb) * (Sa - Sb));
}

// find_neutral_surface_positions_continuous :1368-1573 at every face, :524-554, :592-597
__global__ void __launch_bounds__(256)
k_ndiff_positions(Dm d, const double *__restrict__ G, NdK K, const double *__restrict__ Pint, const double *__restrict__ Tint,
                  const double *__restrict__ Sint, const double *__restrict__ dRdT, const double *__restrict__ dRdS, NdCoef cu,
                  NdCoef cv, int *flag, int *err) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const NdCoef C = f.dir ? cv : cu;
  const int nk = d.nk, ns = 2 * nk + 2;
  const size_t sl = (size_t)d.slab;
  if (!(gm(G, d, f.dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[f.x] > 0.0)) {   // :524-533
    for (int ks = 1; ks <= ns; ++ks) {
      const size_t o = f.x + (size_t)(ks - 1) * sl;
      C.PoL[o] = 0.; C.PoR[o] = 0.; C.KoL[o] = 1; C.KoR[o] = 1;
      if (ks < ns) C.hEff[o] = 0.;
    }
    return;
  }
#define ND_L(A, k) A[f.x + (size_t)((k) - 1) * sl]
#define ND_R(A, k) A[f.y + (size_t)((k) - 1) * sl]
  int kr = 1, kl = 1, lastK_right = 1, lastK_left = 1;
  double lastP_right = 0., lastP_left = 0., absL_last = 0., absR_last = 0.;
  bool reached_bottom = false, searching_left_column = false, searching_right_column = false;
  for (int k_surface = 1; k_surface <= ns; ++k_surface) {
    int klm1 = (kl - 1 > 1) ? kl - 1 : 1;
    int krm1 = (kr - 1 > 1) ? kr - 1 : 1;
    if (klm1 > nk || krm1 > nk) {   // :1426, :1428
      nd_stop(flag, err, ND_ERR_KM1);
      if (klm1 > nk) klm1 = nk;
      if (krm1 > nk) krm1 = nk;
    }
    const double Tl_kl = ND_L(Tint, kl), Sl_kl = ND_L(Sint, kl), aTl_kl = ND_L(dRdT, kl), aSl_kl = ND_L(dRdS, kl);
    const double Tr_kr = ND_R(Tint, kr), Sr_kr = ND_R(Sint, kr), aTr_kr = ND_R(dRdT, kr), aSr_kr = ND_R(dRdS, kr);
    const double dRho = nd_drho(aTr_kr, aTl_kl, Tr_kr, Tl_kl, aSr_kr, aSl_kl, Sr_kr, Sl_kl);
    if (!reached_bottom) {
      if (dRho < 0.) {
        searching_left_column = true; searching_right_column = false;
      } else if (dRho > 0.) {
        searching_right_column = true; searching_left_column = false;
      } else if (kl + kr == 2) {   // still at the surface
        searching_left_column = true; searching_right_column = false;
      } else {                     // change direction
        searching_left_column = !searching_left_column; searching_right_column = !searching_right_column;
      }
    }
    double PoL = 0., PoR = 0.;
    int KoL = 1, KoR = 1;
    if (searching_left_column) {
      const double dRhoTop = nd_drho(ND_L(dRdT, klm1), aTr_kr, ND_L(Tint, klm1), Tr_kr, ND_L(dRdS, klm1), aSr_kr, ND_L(Sint, klm1), Sr_kr);
      const double dRhoBot = nd_drho(ND_L(dRdT, klm1 + 1), aTr_kr, ND_L(Tint, klm1 + 1), Tr_kr, ND_L(dRdS, klm1 + 1), aSr_kr,
                                     ND_L(Sint, klm1 + 1), Sr_kr);
      if (dRhoTop > 0. || kr + kl == 2) PoL = 0.;
      else if (dRhoTop >= dRhoBot) PoL = 1.;
      else PoL = nd_interpolate(dRhoTop, ND_L(Pint, klm1), dRhoBot, ND_L(Pint, klm1 + 1), K.zero, flag, err);
      if (PoL >= 1. && klm1 < nk) { klm1 = klm1 + 1; PoL = PoL - 1.; }
      if ((double)(klm1 - lastK_left) + (PoL - lastP_left) < 0.) { PoL = lastP_left; klm1 = lastK_left; }
      KoL = klm1;
      if (kr <= nk) { PoR = 0.; KoR = kr; } else { PoR = 1.; KoR = nk; }
      if (kr <= nk) kr = kr + 1;
      else { reached_bottom = true; searching_right_column = true; searching_left_column = false; }
    } else if (searching_right_column) {
      const double dRhoTop = nd_drho(ND_R(dRdT, krm1), aTl_kl, ND_R(Tint, krm1), Tl_kl, ND_R(dRdS, krm1), aSl_kl, ND_R(Sint, krm1), Sl_kl);
      const double dRhoBot = nd_drho(ND_R(dRdT, krm1 + 1), aTl_kl, ND_R(Tint, krm1 + 1), Tl_kl, ND_R(dRdS, krm1 + 1), aSl_kl,
                                     ND_R(Sint, krm1 + 1), Sl_kl);
      if (dRhoTop >= 0. || kr + kl == 2) PoR = 0.;
      else if (dRhoTop >= dRhoBot) PoR = 1.;
      else PoR = nd_interpolate(dRhoTop, ND_R(Pint, krm1), dRhoBot, ND_R(Pint, krm1 + 1), K.zero, flag, err);
      if (PoR >= 1. && krm1 < nk) { krm1 = krm1 + 1; PoR = PoR - 1.; }
      if ((double)(krm1 - lastK_right) + (PoR - lastP_right) < 0.) { PoR = lastP_right; krm1 = lastK_right; }
      KoR = krm1;
      if (kl <= nk) { PoL = 0.; KoL = kl; } else { PoL = 1.; KoL = nk; }
      if (kl <= nk) kl = kl + 1;
      else { reached_bottom = true; searching_right_column = false; searching_left_column = true; }
    }
    // (:1541-1554 with bl_kl = bl_kr = 1, bl_zl = bl_zr = 0: KoL >= 1 and PoL >= 0 already)
    lastK_left = KoL; lastP_left = PoL;
    lastK_right = KoR; lastP_right = PoR;
    const size_t o = f.x + (size_t)(k_surface - 1) * sl;
    C.PoL[o] = PoL; C.PoR[o] = PoR; C.KoL[o] = (short)KoL; C.KoR[o] = (short)KoR;
    // absolute_position :2279 of this surface; that of the surface before is what the last pass formed from the same operands
    const double absL = ND_L(Pint, KoL) + PoL * (ND_L(Pint, KoL + 1) - ND_L(Pint, KoL));
    const double absR = ND_R(Pint, KoR) + PoR * (ND_R(Pint, KoR + 1) - ND_R(Pint, KoR));
    if (k_surface > 1) {
      const double hL = absL - absL_last, hR = absR - absR_last;
      double hEff = 0.;
      if (hL + hR > 0.) hEff = 2. * hL * hR / (hL + hR);
      C.hEff[o - sl] = hEff * K.pa_to_H;   // :592-597
    }
    absL_last = absL; absR_last = absR;
  }
#undef ND_L
#undef ND_R
}

// interface_scalar and ppm_left_right_edge_values :2562 of one tracer at every column, :2411-2414
__global__ void __launch_bounds__(256)
k_ndiff_edges(Dm d, double h_neglect, const double *__restrict__ h, const double *__restrict__ tr, double *__restrict__ Til,
              double *__restrict__ aL, double *__restrict__ aR) {
  int i, j;
  if (!nd_column_lane(d, i, j)) return;
  const size_t x = ix2(d, i, j), sl = (size_t)d.slab;
  double Ti_above = 0.;
  nd_interface_scalar(h + x, tr + x, sl, d.nk, h_neglect, [&](int K, double Ti) {
    Til[x + (size_t)(K - 1) * sl] = Ti;
    if (K >= 2) {
      const size_t o = x + (size_t)(K - 2) * sl;   // layer k = K - 1
      const double Tl = tr[o];
      double a_l = Ti_above, a_r = Ti;
      if (nd_sgn1(a_r - Tl) * nd_sgn1(Tl - a_l) <= 0.0) {
        a_l = Tl; a_r = Tl;
      } else if (copysign(3., a_r - a_l) * ((Tl - a_l) + (Tl - a_r)) > fabs(a_r - a_l)) {
        a_l = Tl + 2.0 * (Tl - a_r);
      } else if (copysign(3., a_r - a_l) * ((Tl - a_l) + (Tl - a_r)) < -fabs(a_r - a_l)) {
        a_r = Tl + 2.0 * (Tl - a_l);
      }
      aL[o] = a_l; aR[o] = a_r;
    }
    Ti_above = Ti;
  });
}

// ppm_ave :1181
__device__ __forceinline__ double nd_ppm_ave(double xL, double xR, double aL, double aR, double aMean, int *flag, int *err) {
  const double dx = xR - xL;
  const double xave = 0.5 * (xR + xL);
  const double a6o3 = 2. * aMean - (aL + aR);
  const double a6 = 3. * a6o3;
  if (dx < 0.) nd_stop(flag, err, ND_ERR_DX_NEG);        // :1203
  else if (dx > 1.) nd_stop(flag, err, ND_ERR_DX_BIG);   // :1205
  else if (dx == 0.) return aL + (aR - aL) * xR + a6 * xR * (1. - xR);
  return (aL + xave * ((aR - aL) + a6)) - a6o3 * (xR * xR + xR * xL + xL * xL);
}

__device__ __forceinline__ int nd_layer(int k, int nk) { return (k < 1) ? 1 : ((k > nk) ? nk : k); }   // (an index inside the column, whatever the array holds)

// neutral_surface_flux :2427-2494 of one tracer at every face, and the sums :962-970 | :991-999
__global__ void __launch_bounds__(256)
k_ndiff_flux(Dm d, const double *__restrict__ G, const double *__restrict__ tr, const double *__restrict__ Til,
             const double *__restrict__ aL, const double *__restrict__ aR, NdCoef cu, NdCoef cv, double *__restrict__ uFlx,
             double *__restrict__ vFlx, const double *__restrict__ Coef_x, const double *__restrict__ Coef_y,
             double *__restrict__ trans_x, double *__restrict__ trans_y, double Idt, int *flag, int *err) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const NdCoef C = f.dir ? cv : cu;
  double *Flx = f.dir ? vFlx : uFlx;
  double *trans = f.dir ? trans_y : trans_x;
  const int nk = d.nk, ns = 2 * nk + 2;
  const size_t sl = (size_t)d.slab;
  if (!(gm(G, d, f.dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[f.x] > 0.0)) {   // :713-714, :953 | :982
    for (int ks = 1; ks < ns; ++ks) Flx[f.x + (size_t)(ks - 1) * sl] = 0.;
    if (trans) trans[f.x] = 0.;
    return;
  }
  const double coef = (f.dir ? Coef_y : Coef_x)[f.x];   // Coef_x(I,j,1) | Coef_y(i,J,1)
  double sum = 0.;
  double PiL_t = C.PoL[f.x], PiR_t = C.PoR[f.x];
  int klt = nd_layer(C.KoL[f.x], nk), krt = nd_layer(C.KoR[f.x], nk);
  for (int ks = 1; ks < ns; ++ks) {
    const size_t o = f.x + (size_t)(ks - 1) * sl;
    const double PiL_b = C.PoL[o + sl], PiR_b = C.PoR[o + sl];
    const int klb = nd_layer(C.KoL[o + sl], nk), krb = nd_layer(C.KoR[o + sl], nk);
    const double hEff = C.hEff[o];
    double F = 0.;
    if (!(hEff == 0.)) {
#define ND_L(A, k) A[f.x + (size_t)((k) - 1) * sl]
#define ND_R(A, k) A[f.y + (size_t)((k) - 1) * sl]
      const double T_left_bottom = (1. - PiL_b) * ND_L(Til, klb) + PiL_b * ND_L(Til, klb + 1);
      const double T_left_top = (1. - PiL_t) * ND_L(Til, klt) + PiL_t * ND_L(Til, klt + 1);
      const double T_left_layer = nd_ppm_ave(PiL_t, PiL_b + (double)(klb - klt), ND_L(aL, klt), ND_L(aR, klt), ND_L(tr, klt), flag, err);
      const double T_right_bottom = (1. - PiR_b) * ND_R(Til, krb) + PiR_b * ND_R(Til, krb + 1);
      const double T_right_top = (1. - PiR_t) * ND_R(Til, krt) + PiR_t * ND_R(Til, krt + 1);
      const double T_right_layer = nd_ppm_ave(PiR_t, PiR_b + (double)(krb - krt), ND_R(aL, krt), ND_R(aR, krt), ND_R(tr, krt), flag, err);
#undef ND_L
#undef ND_R
      const double dT_top = T_right_top - T_left_top;
      const double dT_bottom = T_right_bottom - T_left_bottom;
      double dT_ave = 0.5 * (dT_top + dT_bottom);
      const double dT_layer = T_right_layer - T_left_layer;
      if (nd_sgn1(dT_top) * nd_sgn1(dT_bottom) <= 0. || nd_sgn1(dT_ave) * nd_sgn1(dT_layer) <= 0.) dT_ave = 0.;
      else dT_ave = dT_layer;
      F = dT_ave * hEff;   // (khtr_ave = 1.0 :2407)
    }
    Flx[o] = F;
    sum = sum - coef * F;
    PiL_t = PiL_b; PiR_t = PiR_b; klt = klb; krt = krb;
  }
  if (trans) trans[f.x] = sum * Idt;
}

// :894-937 and :941-945 of one tracer at every cell of the computational domain
__global__ void __launch_bounds__(256)
k_ndiff_update(Dm d, const double *__restrict__ G, const double *__restrict__ h, double *__restrict__ tr, NdCoef cu, NdCoef cv,
               const double *__restrict__ uFlx, const double *__restrict__ vFlx, const double *__restrict__ Coef_x,
               const double *__restrict__ Coef_y, double *__restrict__ dTracer, double *__restrict__ tendency, double H_subroundoff,
               double Idt, double conc_underflow, int new_order) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const int nk = d.nk, nsub = 2 * nk + 1;
  const size_t x = ix2(d, i, j), sl = (size_t)d.slab, xw = x - 1, xs = x - (size_t)d.pitch;
  if (!(gm(G, d, MOM6X_G_mask2dT)[x] > 0.)) {
    for (int k = 0; k < nk; ++k) {
      const size_t o = x + (size_t)k * sl;
      if (tendency) tendency[o] = 0.;   // :710
      if (conc_underflow > 0.0 && fabs(tr[o]) < conc_underflow) tr[o] = 0.0;   // :941-945 has no mask
    }
    return;
  }
  const double IareaT = gm(G, d, MOM6X_G_IareaT)[x];
  const double CE = Coef_x[x], CW = Coef_x[xw], CN = Coef_y[x], CS = Coef_y[xs];
  if (!new_order) {   // :897-907
    for (int k = 0; k < nk; ++k) dTracer[x + (size_t)k * sl] = 0.;
    for (int ks = 0; ks < nsub; ++ks) {
      const size_t o = (size_t)ks * sl;
      size_t a = x + (size_t)(nd_layer(cu.KoL[x + o], nk) - 1) * sl;
      dTracer[a] = dTracer[a] + CE * uFlx[x + o];
      a = x + (size_t)(nd_layer(cu.KoR[xw + o], nk) - 1) * sl;
      dTracer[a] = dTracer[a] - CW * uFlx[xw + o];
      a = x + (size_t)(nd_layer(cv.KoL[x + o], nk) - 1) * sl;
      dTracer[a] = dTracer[a] + CN * vFlx[x + o];
      a = x + (size_t)(nd_layer(cv.KoR[xs + o], nk) - 1) * sl;
      dTracer[a] = dTracer[a] - CS * vFlx[xs + o];
    }
  }
  int pE = 0, pW = 0, pN = 0, pS = 0;   // the next surface of each direction
  for (int k = 1; k <= nk; ++k) {
    const size_t o = x + (size_t)(k - 1) * sl;
    double dTr;
    if (new_order) {   // :909-922: each directional sum of layer k over the surfaces whose Ko is k, in their order
      double dTracer_E = 0.0, dTracer_W = 0.0, dTracer_N = 0.0, dTracer_S = 0.0;
      for (; pE < nsub && cu.KoL[x + (size_t)pE * sl] <= k; ++pE)
        if (cu.KoL[x + (size_t)pE * sl] == k) dTracer_E = dTracer_E + CE * uFlx[x + (size_t)pE * sl];
      for (; pW < nsub && cu.KoR[xw + (size_t)pW * sl] <= k; ++pW)
        if (cu.KoR[xw + (size_t)pW * sl] == k) dTracer_W = dTracer_W - CW * uFlx[xw + (size_t)pW * sl];
      for (; pN < nsub && cv.KoL[x + (size_t)pN * sl] <= k; ++pN)
        if (cv.KoL[x + (size_t)pN * sl] == k) dTracer_N = dTracer_N + CN * vFlx[x + (size_t)pN * sl];
      for (; pS < nsub && cv.KoR[xs + (size_t)pS * sl] <= k; ++pS)
        if (cv.KoR[xs + (size_t)pS * sl] == k) dTracer_S = dTracer_S - CS * vFlx[xs + (size_t)pS * sl];
      dTr = (dTracer_N + dTracer_S) + (dTracer_E + dTracer_W);
    } else {
      dTr = dTracer[o];
    }
    double t = tr[o] + dTr * (IareaT / (h[o] + H_subroundoff));
    if (fabs(t) < conc_underflow) t = 0.0;   // :927
    tr[o] = t;
    if (tendency) tendency[o] = dTr * IareaT * Idt;   // :932
  }
}

}  // namespace

// neutral_diffusion_CS with tv%eqn_of_state and every array of the two calls
struct NdState {
  mom6x_neutral_diffusion_params P;
  mom6x_eos_params eos;
  double *iface = nullptr;              // Pint | Tint | Sint | dRdT | dRdS, nk + 1 planes each
  double *Po[2] = {nullptr, nullptr};   // per direction PoL | PoR, 2 nk + 2 planes each
  short *Ko[2] = {nullptr, nullptr};    // per direction KoL | KoR, 2 nk + 2 planes each
  double *hEff[2] = {nullptr, nullptr}; // 2 nk + 1 planes
  double *Flx[2] = {nullptr, nullptr};  // uFlx, vFlx: 2 nk + 1 planes
  double *col = nullptr;                // Til (nk + 1) | aL (nk) | aR (nk) | dTracer (nk)
  double *coef = nullptr;               // Coef_x | Coef_y of tracer_hordiff's neutral branch, nk + 1 planes each
  int *err = nullptr;                   // ND_NERR counters
  long long bytes = 0;
  bool have_coeffs = false;             // calc_coeffs has run: KoL, KoR hold layer indices
};

void neutral_diffusion_free(mom6x_ctx *c) {
  NdState *s = c->nd;
  if (!s) return;
  (void)hipFree(s->iface); (void)hipFree(s->col); (void)hipFree(s->coef); (void)hipFree(s->err);
  for (int dir = 0; dir < 2; dir++) { (void)hipFree(s->Po[dir]); (void)hipFree(s->Ko[dir]); (void)hipFree(s->hEff[dir]); (void)hipFree(s->Flx[dir]); }
  delete s;
  c->nd = nullptr;
}

bool neutral_diffusion_ready(const mom6x_ctx *c) { return c->nd != nullptr; }
bool neutral_diffusion_recalc(const mom6x_ctx *c) { return c->nd && c->nd->P.recalc_neutral_surf != 0; }
void neutral_diffusion_coef_arrays(const mom6x_ctx *c, double **Coef_x, double **Coef_y) {
  *Coef_x = c->nd->coef;
  *Coef_y = c->nd->coef + (size_t)(c->d.nk + 1) * (size_t)c->d.slab;
}

extern "C" int mom6x_neutral_diffusion_tile(int *bx, int *by, int *i_first) {
  if (bx) *bx = LANE_BX;
  if (by) *by = LANE_BY;
  if (i_first) *i_first = -IAL;
  return MOM6X_OK;
}

// one array of a state, filled as the work arrays are
template <class T>
static int nd_alloc(mom6x_ctx *c, NdState *s, T **p, size_t planes) {
  const size_t n = planes * (size_t)c->d.slab * sizeof(T);
  HIPCHK(hipMalloc(p, n));
  HIPCHK(hipMemsetAsync(*p, work_fill_byte(), n, c->stream));
  s->bytes += (long long)n;
  return MOM6X_OK;
}

static int neutral_diffusion_alloc(mom6x_ctx *c, NdState *s) {
  const size_t nk = (size_t)c->d.nk, ns = 2 * nk + 2;
  if (const int rc = nd_alloc(c, s, &s->iface, 5 * (nk + 1))) return rc;
  for (int dir = 0; dir < 2; dir++) {
    if (const int rc = nd_alloc(c, s, &s->Po[dir], 2 * ns)) return rc;
    if (const int rc = nd_alloc(c, s, &s->Ko[dir], 2 * ns)) return rc;
    if (const int rc = nd_alloc(c, s, &s->hEff[dir], ns - 1)) return rc;
    if (const int rc = nd_alloc(c, s, &s->Flx[dir], ns - 1)) return rc;
  }
  if (const int rc = nd_alloc(c, s, &s->col, 4 * nk + 1)) return rc;
  if (const int rc = nd_alloc(c, s, &s->coef, 2 * (nk + 1))) return rc;
  HIPCHK(hipMalloc(&s->err, ND_NERR * sizeof(int)));
  HIPCHK(hipMemsetAsync(s->err, 0, ND_NERR * sizeof(int), c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_neutral_diffusion_init(mom6x_ctx *c, const mom6x_neutral_diffusion_params *p, const mom6x_eos_params *eos) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_neutral_diffusion_init: null argument");
  HIPCHK(hipSetDevice(c->device));
  neutral_diffusion_free(c);   // first: a refused or invalid init leaves no module behind, whatever was initialized before
  REFUSE(!p->continuous_reconstruction, "neutral_diffusion_init", "NDIFF_CONTINUOUS = False (the discontinuous reconstruction)");
  REFUSE(p->interior_only, "neutral_diffusion_init", "NDIFF_INTERIOR_ONLY");
  REFUSE(p->tapering, "neutral_diffusion_init", "NDIFF_TAPERING");
  REFUSE(p->KhTh_use_vert_struct, "neutral_diffusion_init", "KHTR_USE_EBT_STRUCT or KHTR_USE_SQG_STRUCT");
  REFUSE(p->use_unmasked_transport_bug, "neutral_diffusion_init", "NDIFF_USE_UNMASKED_TRANSPORT_BUG");
  REFUSE(!c->GV.Boussinesq, "neutral_diffusion_init", "non-Boussinesq mode");
  REFUSE(!eos, "neutral_diffusion_init", "a run without an equation of state (tv%eqn_of_state)");
  REQUIRE(eos_form_known(eos), MOM6X_EINVAL, "neutral_diffusion_init: unknown EQN_OF_STATE form");
  REQUIRE(c->d.nk <= 32766, MOM6X_EINVAL, "neutral_diffusion_init: KoL and KoR are 16-bit, at most 32766 layers");
  NdState *s = new NdState;
  c->nd = s;
  s->P = *p;
  s->eos = *eos;
  if (const int rc = neutral_diffusion_alloc(c, s)) { neutral_diffusion_free(c); return rc; }   // (no state without its arrays)
  return MOM6X_OK;
}

extern "C" long long mom6x_neutral_diffusion_work_bytes(mom6x_ctx *c) {
  if (!c || !c->nd) return 0;
  return c->nd->bytes;
}

static NdCoef nd_coef(const mom6x_ctx *c, int dir) {
  const NdState *s = c->nd;
  const size_t n = (size_t)(2 * c->d.nk + 2) * (size_t)c->d.slab;
  NdCoef C;
  C.PoL = s->Po[dir]; C.PoR = s->Po[dir] + n; C.KoL = s->Ko[dir]; C.KoR = s->Ko[dir] + n; C.hEff = s->hEff[dir];
  return C;
}

extern "C" int mom6x_neutral_diffusion_coeffs(mom6x_ctx *c, int dir, const double **PoL, const double **PoR, const short **KoL,
                                              const short **KoR, const double **hEff) {
  REQUIRE(c && c->nd, MOM6X_EINVAL, "neutral_diffusion_coeffs: neutral_diffusion_init must be called first");
  REQUIRE(dir == 0 || dir == 1, MOM6X_EINVAL, "neutral_diffusion_coeffs: dir must be 0 (u faces) or 1 (v faces)");
  const NdCoef C = nd_coef(c, dir);
  if (PoL) *PoL = C.PoL;
  if (PoR) *PoR = C.PoR;
  if (KoL) *KoL = C.KoL;
  if (KoR) *KoR = C.KoR;
  if (hEff) *hEff = C.hEff;
  return MOM6X_OK;
}

extern "C" int mom6x_neutral_diffusion_status(mom6x_ctx *c, long long counts[4]) {
  REQUIRE(c && c->nd && counts, MOM6X_EINVAL, "neutral_diffusion_status: neutral_diffusion_init must be called first");
  HIPCHK(hipSetDevice(c->device));
  int e[ND_NERR];
  HIPCHK(hipMemcpyAsync(e, c->nd->err, sizeof(e), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int n = 0; n < ND_NERR; n++) counts[n] = e[n];
  return MOM6X_OK;
}

extern "C" int mom6x_neutral_diffusion_calc_coeffs(mom6x_ctx *c, const double *h, const double *T, const double *S,
                                                   const double *p_surf) {
  REQUIRE(c && c->nd, MOM6X_EINVAL, "neutral_diffusion_calc_coeffs: neutral_diffusion_init must be called first");
  REQUIRE(h && T && S, MOM6X_EINVAL, "neutral_diffusion_calc_coeffs: null h, T or S");
  NdState *s = c->nd;
  const mom6x_neutral_diffusion_params &Q = s->P;
  const mom6x_vgrid &GV = c->GV;
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  NdK K;
  memset(&K, 0, sizeof(K));
  K.gHRZ = GV.g_Earth * GV.H_to_RZ;              // :444
  K.pa_to_H = 1. / (GV.H_to_RZ * GV.g_Earth);    // :382
  K.ref_pres = Q.ref_pres; K.h_neglect = GV.H_subroundoff; K.zero = 0.0;
  K.p_to_Pa = Q.RL2_T2_to_Pa; K.C_to_degC = Q.C_to_degC; K.S_to_ppt = Q.S_to_ppt;
  K.dRdT_scale = Q.kg_m3_to_R * Q.C_to_degC;     // MOM_EOS.F90:820-823
  K.dRdS_scale = Q.kg_m3_to_R * Q.S_to_ppt;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS; K.form = s->eos.form;
  const size_t n1 = (size_t)(d.nk + 1) * (size_t)d.slab;
  double *Pint = s->iface, *Tint = Pint + n1, *Sint = Tint + n1, *dRdT = Sint + n1, *dRdS = dRdT + n1;
  const dim3 b = blk2();
  KLAUNCH(c, "k_ndiff_interface", k_ndiff_interface, grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, K, h, T, S, p_surf, Pint, Tint, Sint,
          dRdT, dRdS);
  KLAUNCH(c, "k_ndiff_positions", k_ndiff_positions, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, (const double *)c->G, K,
          (const double *)Pint, (const double *)Tint, (const double *)Sint, (const double *)dRdT, (const double *)dRdS, nd_coef(c, 0),
          nd_coef(c, 1), c->flag, s->err);
  HIPCHK(hipGetLastError());
  s->have_coeffs = true;
  return MOM6X_OK;
}

extern "C" int mom6x_neutral_diffusion(mom6x_ctx *c, const double *h, const double *Coef_x, const double *Coef_y, double dt,
                                       double *const *tracers, const double *conc_underflow, int ntr, double *const *tendency,
                                       double *const *trans_x_2d, double *const *trans_y_2d) {
  REQUIRE(c && c->nd, MOM6X_EINVAL, "neutral_diffusion: neutral_diffusion_init must be called first");
  NdState *s = c->nd;
  REQUIRE(s->have_coeffs, MOM6X_EINVAL, "neutral_diffusion: neutral_diffusion_calc_coeffs must be called first");
  REQUIRE(ntr >= 0, MOM6X_EINVAL, "neutral_diffusion: negative tracer count");
  if (ntr == 0) return MOM6X_OK;
  REQUIRE(h && Coef_x && Coef_y && tracers, MOM6X_EINVAL, "neutral_diffusion: null h, Coef_x, Coef_y or tracers");
  for (int m = 0; m < ntr; m++) REQUIRE(tracers[m], MOM6X_EINVAL, "neutral_diffusion: null tracer array");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "neutral_diffusion: dt must be positive");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const size_t sl = (size_t)d.slab, nk = (size_t)d.nk;
  double *Til = s->col, *aL = Til + (nk + 1) * sl, *aR = aL + nk * sl, *dTracer = aR + nk * sl;
  const NdCoef cu = nd_coef(c, 0), cv = nd_coef(c, 1);
  const double Idt = 1.0 / dt;   // :709
  const int new_order = s->P.ndiff_answer_date > 20240330;
  const dim3 b = blk2();
  for (int m = 0; m < ntr; m++) {
    double *tr = tracers[m];
    KLAUNCH(c, "k_ndiff_edges", k_ndiff_edges, grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, c->GV.H_subroundoff, h, (const double *)tr,
            Til, aL, aR);
    KLAUNCH(c, "k_ndiff_flux", k_ndiff_flux, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, (const double *)c->G, (const double *)tr,
            (const double *)Til, (const double *)aL, (const double *)aR, cu, cv, s->Flx[0], s->Flx[1], Coef_x, Coef_y,
            trans_x_2d ? trans_x_2d[m] : nullptr, trans_y_2d ? trans_y_2d[m] : nullptr, Idt, c->flag, s->err);
    KLAUNCH(c, "k_ndiff_update", k_ndiff_update, grid3(d.ni, d.nj, 1, b), b, d, (const double *)c->G, h, tr, cu, cv,
            (const double *)s->Flx[0], (const double *)s->Flx[1], Coef_x, Coef_y, dTracer, tendency ? tendency[m] : nullptr,
            c->GV.H_subroundoff, Idt, conc_underflow ? conc_underflow[m] : 0.0, new_order);
  }
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
