// kappa_shear.hip -- the Jackson et al. (2008) shear-driven mixing of MOM_kappa_shear on gfx950: visc%Kd_shear, visc%TKE_turb and
// visc%Kv_shear at the tracer columns, from the C-grid velocities.
//
//   Calculate_kappa_shear     <- src/parameterizations/vertical/MOM_kappa_shear.F90:133-411 (massless-layer elimination :252-314,
//                                the interpolation back :332-380, land :382-391)
//   kappa_shear_column        <- :864-1372, Boussinesq (dz_h_Int = GV%H_to_Z :1110)
//   calculate_projected_state <- :1377-1504 (ks_proj)        find_kappa_tke <- :1507-2067 (ks_find)
//   find_uv_at_h              <- MOM_diabatic_aux.F90:546-571 with :607-610 (the plain average) or :595-605 (zero_mix)
//   calculate_density_derivs  <- MOM_EOS.F90:781-829 with scale = -g_R0, every form of eos_dev.h
//
// k_kappa_shear: one lane per column.  A launch has work_columns lanes, one wavefront per work-group; lane `slot` walks the columns
// slot, slot + work_columns, ... of the computational domain (consecutive lanes along i) and keeps every per-column array of the
// reference in its slot of the module's workspace, laid out [array][K][slot] with the slot fastest: the lanes of a wavefront touch
// one level of one array in consecutive doubles.  Scalars live in registers; there are no per-lane arrays, so nothing is kept in
// scratch memory.  The workspace is sized by the lanes in flight, not by the grid.  A slot's contents are dead between columns:
// every value a column reads it has written before (the test with a poisoned workspace holds that).
//
// Fewer arrays than the reference where the bits allow it: dz_h_Int is the constant GV%H_to_Z; pressure, T_int and Sal_int are
// consumed interface by interface as dbuoy_dT, dbuoy_dS are formed; tol_min, tol_max, tol_chg are formed again where they are
// compared; a1 = k0dt*I_dz_int is a product formed again; u0xdz, v0xdz, T0xdz, S0xdz are overwritten in place by u, v, T, Sal;
// dist_from_top and h_from_top borrow u_test and v_test, which are not yet in use.  The constants tke_noflux_top_BC,
// tke_noflux_bottom_BC and debug_soln of find_kappa_tke are .false. in the reference: their arms are not here.
//
// Every loop is bounded by a parameter: the outer iteration by max_KS_it, the halving by (max_KS_it + 1 - itt)/2, the refinement by
// 5, find_kappa_tke by max_RiNo_it, every K loop by nzc <= nk.  A column without an interface of Ri < Ri_crit leaves after its first
// find_kappa_tke (:1303); a wavefront of such columns goes on to its next columns at once (there is no barrier in the kernel).  In a
// mixed wavefront the lanes that are done idle behind the slowest column until the wavefront moves on.
//
// x**2 is x*x.  MAX and MIN are fmax1 and fmin1, but N2 = MAX(0.0, ...) of :1492-1502 is dmax: with an argument of -0.0 the compiled
// reference returns -0.0 (the case `tie`).  A literal 0.0 operand is the run-time K.zero (see energetic_PBL.hip).  The EOS form
// is a wavefront-uniform switch inside the one kernel (EOS_FORM_DISPATCH): the kernel is not instantiated per form.
#include "mom6x_dev.h"
#include "eos_dev.h"

namespace {

// the per-column arrays of a slot
enum { A_hlay = 0, A_dzlay, A_u, A_v, A_T, A_S, A_ut, A_vt, A_Tt, A_St, A_Idz, A_Idzi, A_hInt, A_dzInt, A_IL2, A_dbT, A_dbS, A_N2,
       A_S2, A_kappa, A_tke, A_kout, A_ksrc, A_lsrc, A_KQ, A_KQt, A_tkep, A_kpred, A_kmid, A_kavg, A_tkeavg, A_N2m, A_S2m, A_N2i,
       A_S2i, A_lsavg, A_c1, A_aQ, A_dQdz, A_dK, A_dQ, A_cQ, A_cK, A_ILd2, A_decay, A_fsrc, A_dQmdK, A_dKdQ, A_e1, A_kc, A_kf,
       KS_NARR };

struct KsK {
  double dt, zero, H_to_Z, gR0, g_R0, k0dt, dz_massless, h_neglect, rho_scale, p_to_Pa, dRho_dT, dRho_dS;
  double Ri_crit, Shearmix_rate, FRi_curvature, c_N2, c_S2, Ilambda2, I_lz_rescale_sqr, q0, TKE_min, kappa0, kappa_seed, kappa_trunc;
  double tol_err, tol_dksrc, tol_dksrc_low, tol2, Prandtl, vel_under, m_to_Z, L_to_Z;
  int max_RiNo_it, max_KS_it, nkml, elim, dKdQ_bug, all_layer_bug, restrictive, zero_mix, form, diag;
  int ni, ncol;
};
struct KsP {
  const double *u, *v, *h, *T, *S, *p_surf, *Rlay;
  double *kappa_io, *tke_io, *kv_io, *N2_init, *S2_init, *N2_mean, *S2_mean, *its;
};
// a slot of the workspace: (array, K) with K = 1 .. nk + 1 as in the Fortran
struct Ws {
  double *p; size_t ns, nkp, slot;
  __device__ __forceinline__ double &operator()(int a, int K) const { return p[((size_t)a * nkp + (size_t)(K - 1)) * ns + slot]; }
};

__device__ __forceinline__ double ks_sq(double x) { return x * x; }

// K_src of :1241, :1274, :1646
__device__ __forceinline__ double ks_ksrc(const KsK &K, double N2, double S2) {
  return (2.0 * K.Shearmix_rate * sqrt(S2)) * ((K.Ri_crit * S2 - N2) / (K.Ri_crit * S2 + K.FRi_curvature * N2));
}

// calculate_projected_state :1377-1504.  The initial state is u, v, T, Sal of the slot; a_kap: the diffusivity; ou, ov, oT, oS: where
// the projected state goes (the state itself or the test arrays); ks, ke: the layer range, 1 and nz without ks_int and ke_int.
__device__ __forceinline__ void ks_proj(const Ws &W, const KsK &K, int a_kap, double dt, int nz, int ou, int ov, int oT, int oS, int ks,
                                        int ke) {
  if (ks > ke) return;
  if (dt > 0.0) {
    double a_b = dt * (W(a_kap, ks + 1) * W(A_Idzi, ks + 1));
    double dzk = W(A_hlay, ks);
    double b1 = 1.0 / (dzk + a_b);
    W(A_c1, ks + 1) = a_b * b1;
    double d1 = dzk * b1;
    double up = (b1 * dzk) * W(A_u, ks), vp = (b1 * dzk) * W(A_v, ks), Tp = (b1 * dzk) * W(A_T, ks), Sp = (b1 * dzk) * W(A_S, ks);
    W(ou, ks) = up; W(ov, ks) = vp; W(oT, ks) = Tp; W(oS, ks) = Sp;
    double a_a;
    for (int k = ks + 1; k <= ke - 1; ++k) {
      a_a = a_b;
      a_b = dt * (W(a_kap, k + 1) * W(A_Idzi, k + 1));
      dzk = W(A_hlay, k);
      const double bd1 = dzk + d1 * a_a;
      b1 = 1.0 / (bd1 + a_b);
      W(A_c1, k + 1) = a_b * b1; d1 = bd1 * b1;
      up = b1 * (dzk * W(A_u, k) + a_a * up);
      vp = b1 * (dzk * W(A_v, k) + a_a * vp);
      Tp = b1 * (dzk * W(A_T, k) + a_a * Tp);
      Sp = b1 * (dzk * W(A_S, k) + a_a * Sp);
      W(ou, k) = up; W(ov, k) = vp; W(oT, k) = Tp; W(oS, k) = Sp;
    }
    a_a = a_b;
    dzk = W(A_hlay, ke);
    // (ks < ke wherever dt > 0: a range given by ks_int and ke_int has ks = ks_int - 1 < ks_int <= ke_int = ke, since kappa is 0 at
    //  interfaces 1 and nz + 1, and the whole column is projected only after mixing, which needs nz >= 2)
    b1 = 1.0 / (dzk + d1 * a_a);
    double Tk = b1 * (dzk * W(A_T, ke) + a_a * Tp);
    double Sk = b1 * (dzk * W(A_S, ke) + a_a * Sp);
    double b1nz_0;
    if (ke == nz) {
      a_b = dt * (W(a_kap, nz + 1) * W(A_Idzi, nz + 1));
      b1nz_0 = 1.0 / ((dzk + d1 * a_a) + a_b);
    } else {
      b1nz_0 = b1;
    }
    double uk = b1nz_0 * (dzk * W(A_u, ke) + a_a * up);
    double vk = b1nz_0 * (dzk * W(A_v, ke) + a_a * vp);
    if (fabs(uk) < K.vel_under) uk = 0.0;
    if (fabs(vk) < K.vel_under) vk = 0.0;
    W(ou, ke) = uk; W(ov, ke) = vk; W(oT, ke) = Tk; W(oS, ke) = Sk;
    for (int k = ke - 1; k >= ks; --k) {
      const double c1 = W(A_c1, k + 1);
      uk = W(ou, k) + c1 * uk;
      vk = W(ov, k) + c1 * vk;
      if (fabs(uk) < K.vel_under) uk = 0.0;
      if (fabs(vk) < K.vel_under) vk = 0.0;
      Tk = W(oT, k) + c1 * Tk;
      Sk = W(oS, k) + c1 * Sk;
      W(ou, k) = uk; W(ov, k) = vk; W(oT, k) = Tk; W(oS, k) = Sk;
    }
  } else {
    for (int k = 1; k <= nz; ++k) {
      double uk = W(A_u, k), vk = W(A_v, k);
      if (fabs(uk) < K.vel_under) uk = 0.0;
      if (fabs(vk) < K.vel_under) vk = 0.0;
      W(ou, k) = uk; W(ov, k) = vk; W(oT, k) = W(A_T, k); W(oS, k) = W(A_S, k);
    }
  }
  // the squared shear and the buoyancy frequency at the interfaces ks .. ke + 1
  W(A_S2, 1) = 0.0; W(A_S2, nz + 1) = 0.0;
  W(A_N2, 1) = 0.0; W(A_N2, nz + 1) = 0.0;
  double um, vm, Tm, Sm;
  if (ks > 1) {
    const double I = W(A_Idzi, ks);
    um = W(ou, ks); vm = W(ov, ks); Tm = W(oT, ks); Sm = W(oS, ks);
    W(A_S2, ks) = (ks_sq(um - W(A_u, ks - 1)) + ks_sq(vm - W(A_v, ks - 1))) * ks_sq(K.L_to_Z * I);
    W(A_N2, ks) = dmax(K.zero, I * (W(A_dbT, ks) * (W(A_T, ks - 1) - Tm) + W(A_dbS, ks) * (W(A_S, ks - 1) - Sm)));
  } else {
    um = W(ou, 1); vm = W(ov, 1); Tm = W(oT, 1); Sm = W(oS, 1);
  }
  for (int k = ks + 1; k <= ke; ++k) {
    const double I = W(A_Idzi, k);
    const double uk = W(ou, k), vk = W(ov, k), Tk = W(oT, k), Sk = W(oS, k);
    W(A_S2, k) = (ks_sq(uk - um) + ks_sq(vk - vm)) * ks_sq(K.L_to_Z * I);
    W(A_N2, k) = dmax(K.zero, I * (W(A_dbT, k) * (Tm - Tk) + W(A_dbS, k) * (Sm - Sk)));
    um = uk; vm = vk; Tm = Tk; Sm = Sk;
  }
  if (ke < nz) {
    const double I = W(A_Idzi, ke + 1);
    W(A_S2, ke + 1) = (ks_sq(W(A_u, ke + 1) - um) + ks_sq(W(A_v, ke + 1) - vm)) * ks_sq(K.L_to_Z * I);
    W(A_N2, ke + 1) = dmax(K.zero, I * (W(A_dbT, ke + 1) * (Tm - W(A_T, ke + 1)) + W(A_dbS, ke + 1) * (Sm - W(A_S, ke + 1))));
  }
}

// find_kappa_tke :1507-2067.  a_kin: kappa_in; a_KQ: K_Q; a_tke: tke; a_kap: kappa; SRC: kappa_src and local_src are formed
template <bool SRC>
__device__ __forceinline__ void ks_find(const Ws &W, const KsK &K, int nz, double f2, int a_kin, int a_KQ, int a_tke, int a_kap) {
  const double roundoff = 1.0e-16;
  const double dzh = K.H_to_Z, q0 = K.q0, kappa0 = K.kappa0, TKE_min = K.TKE_min, kappa_trunc = K.kappa_trunc, Ilambda2 = K.Ilambda2;
  bool do_Newton = false, abort_Newton = false;
  double Newton_err = 0.2;
  int ks_kappa = 2, ke_kappa = nz, ks_kappa_prev = 2, ke_kappa_prev = nz;
  int ke_src = 0, ks_src = nz + 1;
  for (int k = 2; k <= nz; ++k) {
    const double N2 = W(A_N2, k), S2 = W(A_S2, k);
    if (N2 < K.Ri_crit * S2) {
      W(A_fsrc, k) = ks_ksrc(K, N2, S2);
      ke_src = k;
      if (ks_src > k) ks_src = k;
    } else {
      W(A_fsrc, k) = 0.0;
    }
  }
  if (ks_src > ke_src) {   // :1656
    for (int k = 1; k <= nz + 1; ++k) {
      W(a_kap, k) = 0.0; W(a_KQ, k) = 0.0; W(a_tke, k) = TKE_min;
      if (SRC) { W(A_ksrc, k) = 0.0; W(A_lsrc, k) = 0.0; }
    }
    return;
  }
  for (int k = 1; k <= nz + 1; ++k) {
    const double kap = W(a_kin, k), KQ = W(a_KQ, k);
    W(a_kap, k) = kap;
    W(A_decay, k) = sqrt(K.c_N2 * W(A_N2, k) + K.c_S2 * W(A_S2, k));
    W(a_tke, k) = ((kap > 0.0) && (KQ > 0.0)) ? kap / KQ : TKE_min;
  }
  W(a_kap, 1) = 0.0; W(a_kap, nz + 1) = 0.0;
  {   // e1 :1681-1695
    double eden2 = kappa0 * W(A_Idz, nz), ome = 1.0;
    W(A_e1, nz + 1) = 0.0;
    for (int k = nz; k >= 2; --k) {
      const double eden1 = W(A_hInt, k) * W(A_decay, k) + ome * eden2;
      eden2 = kappa0 * W(A_Idz, k - 1);
      const double I_eden = 1.0 / (eden2 + eden1);
      W(A_e1, k) = eden2 * I_eden; ome = eden1 * I_eden;
    }
    W(A_e1, 1) = 0.0;
  }

  for (int itt = 1; itt <= K.max_RiNo_it; ++itt) {
    if (!do_Newton) {
      const int ke_tke = ((ke_kappa > ke_kappa_prev) ? ke_kappa : ke_kappa_prev) + 1;
      const int kaq = (ke_tke < nz) ? ke_tke : nz;
      for (int k = 1; k <= kaq; ++k) W(A_aQ, k) = (0.5 * (W(a_kap, k) + W(a_kap, k + 1)) + kappa0) * W(A_Idz, k);
      W(A_dQ, 1) = -W(a_tke, 1);
      W(a_tke, 1) = q0; W(A_cQ, 2) = 0.0;
      double cQcomp = 1.0;
      for (int k = 2; k <= ke_tke - 1; ++k) {
        W(A_dQ, k) = -W(a_tke, k);
        const double decay = W(A_decay, k), hI = W(A_hInt, k), aQm = W(A_aQ, k - 1), aQk = W(A_aQ, k);
        const double tke_src = dzh * (W(a_kap, k) + kappa0) * W(A_S2, k) + q0 * decay;
        const double bQd1 = hI * (decay + dzh * W(A_N2, k) * W(a_KQ, k)) + cQcomp * aQm;
        const double bQ = 1.0 / (bQd1 + aQk);
        W(a_tke, k) = bQ * (hI * tke_src + aQm * W(a_tke, k - 1));
        W(A_cQ, k + 1) = aQk * bQ; cQcomp = bQd1 * bQ;
      }
      if (ke_tke == nz + 1) {
        W(a_tke, nz + 1) = TKE_min;
        W(A_dQ, nz + 1) = 0.0;
      } else {
        int k = ke_tke;
        const double decay = W(A_decay, k), hI = W(A_hInt, k), aQm = W(A_aQ, k - 1), aQk = W(A_aQ, k);
        const double tke_src = dzh * kappa0 * W(A_S2, k) + q0 * decay;
        const double bQ = 1.0 / ((hI * decay + cQcomp * aQm) + aQk);
        const double cQn = aQk * bQ;
        W(A_cQ, k + 1) = cQn;
        const double told = W(a_tke, k), e1n = W(A_e1, k + 1);
        double dQk = -told;
        const double tnew = fmax1((bQ * (hI * tke_src + aQm * W(a_tke, k - 1)) + cQn * (W(a_tke, k + 1) - e1n * told)) / (1.0 - cQn * e1n), TKE_min);
        W(a_tke, k) = tnew;
        dQk = tnew + dQk;
        W(A_dQ, k) = dQk;
        for (k = ke_tke + 1; k <= nz + 1; ++k) {   // :1758-1762; k is nz + 2 when the loop runs out
          dQk = W(A_e1, k) * dQk;
          W(A_dQ, k) = dQk;
          const double t = fmax1(W(a_tke, k) + dQk, TKE_min);
          W(a_tke, k) = t;
          if (fabs(dQk) < roundoff * t) break;
        }
        for (int k2 = k + 1; k2 <= nz; ++k2) {
          if (W(A_dQ, k2) == 0.0) break;
          W(A_dQ, k2) = 0.0;
        }
      }
      {
        double tn = W(a_tke, ke_tke);
        for (int k = ke_tke - 1; k >= 1; --k) {
          tn = fmax1(W(a_tke, k) + W(A_cQ, k + 1) * tn, TKE_min);
          W(a_tke, k) = tn;
          W(A_dQ, k) = tn + W(A_dQ, k);
        }
      }

      // kappa :1778-1821
      ke_kappa_prev = ke_kappa; ks_kappa_prev = ks_kappa;
      W(A_dK, 1) = 0.0;
      W(A_cK, 2) = 0.0;
      double cKcomp = 1.0;
      if (itt == 1) {
        for (int k = 2; k <= nz; ++k) W(A_ILd2, k) = dzh * (W(A_N2, k) * Ilambda2 + f2) / W(a_tke, k) + W(A_IL2, k);
      }
      double kapm = W(a_kap, 1);
      for (int k = 2; k <= nz; ++k) {
        double kap = W(a_kap, k);
        W(A_dK, k) = -kap;
        if (itt > 1) W(A_ILd2, k) = dzh * (W(A_N2, k) * Ilambda2 + f2) / W(a_tke, k) + W(A_IL2, k);
        const double hI = W(A_hInt, k), Im = W(A_Idz, k - 1), Ik = W(A_Idz, k);
        const double bKd1 = hI * W(A_ILd2, k) + cKcomp * Im;
        const double bK = 1.0 / (bKd1 + Ik);
        kap = bK * (Im * kapm + hI * W(A_fsrc, k));
        W(A_cK, k + 1) = Ik * bK; cKcomp = bKd1 * bK;
        bool leave = false;
        if (kap < cKcomp * kappa_trunc) {
          kap = 0.0;
          if (k > ke_src) { ke_kappa = k - 1; W(a_KQ, k) = 0.0; leave = true; }
        } else if (kap < 2.0 * cKcomp * kappa_trunc) {
          kap = 2.0 * (kap - cKcomp * kappa_trunc);
        }
        W(a_kap, k) = kap;
        kapm = kap;
        if (leave) break;
      }
      {
        const double kap = W(a_kap, ke_kappa);
        W(a_KQ, ke_kappa) = kap / W(a_tke, ke_kappa);
        W(A_dK, ke_kappa) = W(A_dK, ke_kappa) + kap;
      }
      for (int k = ke_kappa + 2; k <= ke_kappa_prev; ++k) { W(A_dK, k) = -W(a_kap, k); W(a_kap, k) = 0.0; W(a_KQ, k) = 0.0; }
      {
        double kapn = W(a_kap, ke_kappa);
        for (int k = ke_kappa - 1; k >= 2; --k) {
          double kap = W(a_kap, k) + W(A_cK, k + 1) * kapn;
          bool leave = false;
          if (kap <= kappa_trunc) {
            kap = 0.0;
            if (k < ks_src) { ks_kappa = k + 1; W(a_KQ, k) = 0.0; leave = true; }
          } else if (kap < 2.0 * kappa_trunc) {
            kap = 2.0 * (kap - kappa_trunc);
          }
          W(a_kap, k) = kap;
          kapn = kap;
          if (leave) break;
          W(A_dK, k) = W(A_dK, k) + kap;
          W(a_KQ, k) = kap / W(a_tke, k);
        }
      }
      for (int k = ks_kappa_prev; k <= ks_kappa - 2; ++k) { W(a_kap, k) = 0.0; W(a_KQ, k) = 0.0; }
    } else {
      // Newton's method on the whole system :1826-1969
      ks_kappa_prev = ks_kappa; ke_kappa_prev = ke_kappa; ke_kappa = nz;
      ks_kappa = 2;
      W(A_dK, 1) = 0.0; W(A_cK, 2) = 0.0; W(A_dKdQ, 1) = 0.0;
      double cKcomp = 1.0;
      W(A_aQ, 1) = (0.5 * (W(a_kap, 1) + W(a_kap, 2)) + kappa0) * W(A_Idz, 1);
      W(A_dQdz, 1) = 0.5 * (W(a_tke, 1) - W(a_tke, 2)) * W(A_Idz, 1);
      W(A_dQ, 1) = 0.0; W(A_cQ, 2) = 0.0; W(A_dQmdK, 2) = 0.0;
      double cQcomp = 1.0;
      for (int k = 2; k <= nz; ++k) {
        const double tk = W(a_tke, k), tm = W(a_tke, k - 1), tp = W(a_tke, k + 1);
        const double kap = W(a_kap, k), kapm = W(a_kap, k - 1), kapp = W(a_kap, k + 1);
        const double N2 = W(A_N2, k), S2 = W(A_S2, k), hI = W(A_hInt, k), Im = W(A_Idz, k - 1), Ik = W(A_Idz, k);
        const double I_Q = 1.0 / tk;
        const double ILd2 = (N2 * Ilambda2 + f2) * dzh * I_Q + W(A_IL2, k);
        W(A_ILd2, k) = ILd2;
        const double kap_src = hI * (W(A_fsrc, k) - ILd2 * kap) + Im * (kapm - kap) - Ik * (kap - kapp);
        const double dQmdK = W(A_dQmdK, k), dKdQm = W(A_dKdQ, k - 1), cQk = W(A_cQ, k);
        const double decay_term_k = -Im * dQmdK * dKdQm + hI * ILd2;
        if (decay_term_k < 0.0) { abort_Newton = true; break; }
        const double bK = 1.0 / (Ik + Im * cKcomp + decay_term_k);
        const double cKn = bK * Ik;
        W(A_cK, k + 1) = cKn;
        cKcomp = bK * (Im * cKcomp + decay_term_k);
        double dKdQ;
        if (K.dKdQ_bug) dKdQ = bK * (Im * dKdQm * cQk + K.m_to_Z * (N2 * Ilambda2 + f2) * (I_Q * I_Q) * kap);
        else dKdQ = bK * (Im * dKdQm * cQk + W(A_dzInt, k) * (N2 * Ilambda2 + f2) * (I_Q * I_Q) * kap);
        W(A_dKdQ, k) = dKdQ;
        const double dKm = W(A_dK, k - 1), dQm = W(A_dQ, k - 1);
        double dK = bK * (kap_src + Im * dKm + Im * dKdQm * dQm);
        if (dK <= cKcomp * (kappa_trunc - kap)) dK = -cKcomp * kap;
        else if (dK < cKcomp * (2.0 * kappa_trunc - kap)) dK = 2.0 * dK - cKcomp * (2.0 * kappa_trunc - kap);
        W(A_dK, k) = dK;
        const double aQk = (0.5 * (kap + kapp) + kappa0) * Ik, aQm = W(A_aQ, k - 1);
        W(A_aQ, k) = aQk;
        const double dQdzk = 0.5 * (tk - tp) * Ik, dQdzm = W(A_dQdz, k - 1);
        W(A_dQdz, k) = dQdzk;
        const double decay = W(A_decay, k);
        const double tke_src = hI * ((dzh * ((kap + kappa0) * S2 - kap * N2)) - (tk - q0) * decay) - (aQk * (tk - tp) - aQm * (tm - tk));
        const double v1 = aQm + dQdzm * dKdQm;
        const double v2 = (v1 * dQmdK + dQdzm * W(A_cK, k)) + ((dQdzm - dQdzk) + W(A_dzInt, k) * (S2 - N2));
        const double decay_term_Q = hI * decay - dQdzm * dKdQm * cQk - v2 * dKdQ;
        if (decay_term_Q < 0.0) { abort_Newton = true; break; }
        const double bQ = 1.0 / (aQk + (cQcomp * aQm + decay_term_Q));
        W(A_cQ, k + 1) = aQk * bQ;
        cQcomp = (cQcomp * aQm + decay_term_Q) * bQ;
        W(A_dQmdK, k + 1) = (v2 * cKn - dQdzk) * bQ;
        W(A_dQ, k) = fmax1(bQ * ((v1 * dQm + dQdzm * dKm) + (v2 * dK + tke_src)), cQcomp * (-0.5 * tk));
        if ((itt > 1) && (k > ke_src) && (dK == 0.0) && ((kap + kapp) == 0.0)) { ke_kappa = k - 1; break; }
      }
      if ((ke_kappa == nz) && !abort_Newton) {
        W(A_dK, nz + 1) = 0.0; W(A_dKdQ, nz + 1) = 0.0;
        W(A_dQ, nz + 1) = 0.0;
      } else if (!abort_Newton) {
        double dQk = W(A_dQ, ke_kappa + 1) / (1.0 - W(A_cQ, ke_kappa + 2) * W(A_e1, ke_kappa + 2));
        W(A_dQ, ke_kappa + 1) = dQk;
        W(a_tke, ke_kappa + 1) = fmax1(W(a_tke, ke_kappa + 1) + dQk, TKE_min);
        for (int k = ke_kappa + 2; k <= nz + 1; ++k) {
          W(A_dK, k) = 0.0;
          const double told = W(a_tke, k);
          dQk = fmax1(W(A_e1, k) * dQk, -0.5 * told);
          W(A_dQ, k) = dQk;
          const double t = fmax1(told + dQk, TKE_min);
          W(a_tke, k) = t;
          if (fabs(dQk) < roundoff * t) break;
        }
      }
      if (!abort_Newton) {
        double dQn = W(A_dQ, ke_kappa + 1), dKn = W(A_dK, ke_kappa + 1);
        for (int k = ke_kappa; k >= 2; --k) {
          const double told = W(a_tke, k), kap = W(a_kap, k);
          const double dQk = fmax1(W(A_dQ, k) + (W(A_cQ, k + 1) * dQn + W(A_dQmdK, k + 1) * dKn), -0.5 * told);
          W(A_dQ, k) = dQk;
          W(a_tke, k) = fmax1(told + dQk, TKE_min);
          double dK = W(A_dK, k) + (W(A_cK, k + 1) * dKn + W(A_dKdQ, k) * dQk);
          if (dK <= kappa_trunc - kap) {
            dK = -kap;
            W(a_kap, k) = 0.0;
            if ((k < ks_src) && (k + 1 > ks_kappa)) ks_kappa = k + 1;
          } else if (dK < 2.0 * kappa_trunc - kap) {
            dK = 2.0 * dK - (2.0 * kappa_trunc - kap);
            W(a_kap, k) = fmax1(kap + dK, K.zero);
            if (k <= ks_kappa) ks_kappa = 2;
          } else {
            W(a_kap, k) = kap + dK;
            if (k <= ks_kappa) ks_kappa = 2;
          }
          W(A_dK, k) = dK;
          dQn = dQk; dKn = dK;
        }
        const double t1 = W(a_tke, 1);
        const double dQ1 = fmax1(W(A_dQ, 1) + W(A_cQ, 2) * dQn + W(A_dQmdK, 2) * dKn, TKE_min - t1);
        W(A_dQ, 1) = dQ1;
        W(a_tke, 1) = fmax1(t1 + dQ1, TKE_min);
        W(A_dK, 1) = 0.0;
      }
    }

    // the convergence test :2001-2028
    bool within_tolerance = true;
    const int k0 = (ks_kappa < ks_kappa_prev) ? ks_kappa : ks_kappa_prev, k1 = (ke_kappa > ke_kappa_prev) ? ke_kappa : ke_kappa_prev;
    if ((K.tol_err < Newton_err) && !abort_Newton) {
      const double Newton_test = do_Newton ? 2.0 * Newton_err : Newton_err;
      do_Newton = true;
      for (int k = k0; k <= k1; ++k) {
        const double dK = W(A_dK, k), dQ = W(A_dQ, k);
        const double kappa_mean = kappa0 + (W(a_kap, k) - 0.5 * dK);
        if (fabs(dK) > Newton_test * kappa_mean) {
          if (do_Newton) abort_Newton = true;
          within_tolerance = false; do_Newton = false;
          break;
        } else if (fabs(dK) > K.tol_err * kappa_mean) {
          within_tolerance = false;
          if (!do_Newton) break;
        }
        if (fabs(dQ) > Newton_test * (W(a_tke, k) - 0.5 * dQ)) {
          if (do_Newton) abort_Newton = true;
          do_Newton = false;
          if (!within_tolerance) break;
        }
      }
    } else {
      for (int k = k0; k <= k1; ++k) {
        const double dK = W(A_dK, k);
        if (fabs(dK) > K.tol_err * (kappa0 + (W(a_kap, k) - 0.5 * dK))) { within_tolerance = false; break; }
      }
    }
    if (abort_Newton) {
      do_Newton = false; abort_Newton = false;
      Newton_err = 0.5 * Newton_err;
      ke_kappa_prev = nz;
      for (int k = 2; k <= nz; ++k) W(a_KQ, k) = W(a_kap, k) / fmax1(W(a_tke, k), TKE_min);
    }
    if (within_tolerance) break;
  }

  if (do_Newton) {   // :2042-2046
    for (int k = 1; k <= ks_kappa - 1; ++k) W(a_KQ, k) = 0.0;
    for (int k = ks_kappa; k <= ke_kappa; ++k) W(a_KQ, k) = W(a_kap, k) / W(a_tke, k);
    for (int k = ke_kappa + 1; k <= nz + 1; ++k) W(a_KQ, k) = 0.0;
  }
  if (SRC) {
    W(A_lsrc, 1) = 0.0; W(A_lsrc, nz + 1) = 0.0;
    W(A_ksrc, 1) = 0.0; W(A_ksrc, nz + 1) = 0.0;
    for (int k = 2; k <= nz; ++k) {
      const double kap = W(a_kap, k), Im = W(A_Idz, k - 1), Ik = W(A_Idz, k), hI = W(A_hInt, k), src = W(A_fsrc, k);
      const double diffusive_src = Im * (W(a_kap, k - 1) - kap) + Ik * (W(a_kap, k + 1) - kap);
      const double chg_by_k0 = kappa0 * ((Im + Ik) / hI + W(A_ILd2, k));
      if (diffusive_src <= 0.0) W(A_lsrc, k) = src + chg_by_k0;
      else W(A_lsrc, k) = (src + chg_by_k0) + diffusive_src / hI;
      W(A_ksrc, k) = src;
    }
  }
}

// the validity scan of a trial time step :1239-1259 (restrictive: CS%restrictive_tolerance_check) and :1272-1285
__device__ __forceinline__ bool ks_scan(const Ws &W, const KsK &K, int nzc, int ks_kappa, int ke_kappa, double Idtt, bool restrictive) {
  const int k0 = (ks_kappa - 1 > 2) ? ks_kappa - 1 : 2, k1 = (ke_kappa + 1 < nzc) ? ke_kappa + 1 : nzc;
  for (int k = k0; k <= k1; ++k) {
    const double N2 = W(A_N2, k), S2 = W(A_S2, k), ksrc = W(A_ksrc, k), lsrc = W(A_lsrc, k);
    const double tol_max = ksrc + K.tol_dksrc * lsrc, tol_min = ksrc - K.tol_dksrc_low * lsrc, tol_chg = K.tol2 * W(A_lsavg, k);
    if (N2 < K.Ri_crit * S2) {
      const double src = ks_ksrc(K, N2, S2);
      if (restrictive) {
        if ((src > fmin1(tol_max, ksrc + Idtt * tol_chg)) || (src < fmax1(tol_min, ksrc - Idtt * tol_chg))) return false;
      } else {
        if ((src > fmax1(tol_max, ksrc + Idtt * tol_chg)) || (src < fmin1(tol_min, ksrc - Idtt * tol_chg))) return false;
      }
    } else {
      if (0.0 < fmin1(tol_min, ksrc - Idtt * tol_chg)) return false;
    }
  }
  return true;
}

__global__ void __launch_bounds__(64) k_kappa_shear(Dm d, const double *__restrict__ G, KsK K, KsP P, double *__restrict__ ws, int nslots) {
  Ws W;
  W.p = ws; W.ns = (size_t)nslots; W.nkp = (size_t)(d.nk + 1); W.slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (W.slot >= W.ns) return;
  const int nz = d.nk;
  const size_t slab = (size_t)d.slab;
  const double *aCu = gm(G, d, MOM6X_G_areaCu), *aCv = gm(G, d, MOM6X_G_areaCv), *IareaT = gm(G, d, MOM6X_G_IareaT);
  const double *f2B = gm(G, d, MOM6X_G_Coriolis2Bu), *mask2dT = gm(G, d, MOM6X_G_mask2dT);
  const bool use_T = P.T != nullptr;

  for (long long n = (long long)W.slot; n < (long long)K.ncol; n += (long long)nslots) {
    const int i = (int)(n % K.ni), j = (int)(n / K.ni);
    const size_t x = ix2(d, i, j);
    const double mask = mask2dT[x];
    if (!(mask > 0.0)) {   // :382-391
      for (int k = 0; k <= nz; ++k) {
        const size_t o = (size_t)k * slab + x;
        P.kappa_io[o] = mask * K.zero; P.tke_io[o] = mask * K.zero; P.kv_io[o] = (mask * K.zero) * K.Prandtl;
        if (P.N2_init) P.N2_init[o] = 0.0;
        if (P.S2_init) P.S2_init[o] = 0.0;
        if (P.N2_mean) P.N2_mean[o] = 0.0;
        if (P.S2_mean) P.S2_mean[o] = 0.0;
      }
      if (P.its) P.its[x] = 0.0;
      continue;
    }

    // find_uv_at_h's weights, MOM_diabatic_aux.F90:548-570
    double a_w = 0.0, a_e = 0.0, a_s = 0.0, a_n = 0.0;
    {
      const double IaT = IareaT[x];
      double sum_area = aCu[x - 1] + aCu[x];
      if (sum_area > 0.0) { const double Idenom = sqrt(0.5 * IaT / sum_area); a_w = aCu[x - 1] * Idenom; a_e = aCu[x] * Idenom; }
      sum_area = aCv[x - d.pitch] + aCv[x];
      if (sum_area > 0.0) { const double Idenom = sqrt(0.5 * IaT / sum_area); a_s = aCv[x - d.pitch] * Idenom; a_n = aCv[x] * Idenom; }
    }

    // the load pass :232-314: u_h, v_h, thickness_to_dz and the merging of massless layers
    int nzc = 1;
    {
      double hs = K.zero, dzs = K.zero, us = K.zero, vs = K.zero, Ts = K.zero, Ss = K.zero;
      for (int k = 1; k <= nz; ++k) {
        const size_t o = (size_t)(k - 1) * slab + x;
        const double hk = P.h[o], dzk = K.H_to_Z * hk;
        const double ua = (a_e * P.u[o]) + (a_w * P.u[o - 1]), va = (a_n * P.v[o]) + (a_s * P.v[o - d.pitch]);
        double uk, vk;
        if (K.zero_mix) {
          const double b1 = 1.0 / (hk + K.h_neglect);
          if (k == 1) { uk = (hk * b1) * ua; vk = (hk * b1) * va; }
          else { uk = (hk * ua) * b1; vk = (hk * va) * b1; }
        } else {
          uk = ua; vk = va;
        }
        double Tk, Sk;
        if (use_T) { Tk = P.T[o]; Sk = P.S[o]; }
        else { Tk = P.Rlay[k - 1]; Sk = Tk; }
        if (K.elim) {
          if ((k > K.nkml) && (hs > 0.0) && (hk > K.dz_massless)) {
            W(A_hlay, nzc) = hs; W(A_dzlay, nzc) = dzs; W(A_u, nzc) = us; W(A_v, nzc) = vs; W(A_T, nzc) = Ts; W(A_S, nzc) = Ss;
            nzc = nzc + 1;
            hs = K.zero; dzs = K.zero; us = K.zero; vs = K.zero; Ts = K.zero; Ss = K.zero;
          }
          W(A_kc, k) = (double)nzc;
          hs = hs + hk; dzs = dzs + dzk; us = us + uk * hk; vs = vs + vk * hk; Ts = Ts + Tk * hk; Ss = Ss + Sk * hk;
        } else {
          W(A_hlay, k) = hk; W(A_dzlay, k) = dzk; W(A_u, k) = uk * hk; W(A_v, k) = vk * hk; W(A_T, k) = Tk * hk; W(A_S, k) = Sk * hk;
        }
      }
      if (K.elim) {
        W(A_hlay, nzc) = hs; W(A_dzlay, nzc) = dzs; W(A_u, nzc) = us; W(A_v, nzc) = vs; W(A_T, nzc) = Ts; W(A_S, nzc) = Ss;
        W(A_kc, nz + 1) = (double)(nzc + 1);
        if (nzc != nz) {   // kf :288-296, read only where layers were merged (:353)
          W(A_kf, 1) = 0.0;
          double dz_in_lay = P.h[x];
          int kcm = (int)W(A_kc, 1);
          for (int k = 2; k <= nz; ++k) {
            const double hk = P.h[(size_t)(k - 1) * slab + x];
            const int kck = (int)W(A_kc, k);
            if (kck > kcm) { W(A_kf, k) = 0.0; dz_in_lay = hk; }
            else { W(A_kf, k) = dz_in_lay * (1.0 / W(A_hlay, kck)); dz_in_lay = dz_in_lay + hk; }
            kcm = kck;
          }
          W(A_kf, nz + 1) = 0.0;
        }
      } else {
        nzc = nz;
      }
    }
    const double f2 = 0.25 * ((f2B[x] + f2B[x - d.pitch - 1]) + (f2B[x - d.pitch] + f2B[x - 1]));
    const double surface_pres = P.p_surf ? P.p_surf[x] : 0.0;
    for (int k = 1; k <= nzc + 1; ++k) W(A_kappa, k) = K.kappa_seed;   // :323

    // kappa_shear_column :1024-1047
    {
      double dzm = W(A_dzlay, 1);
      W(A_Idz, 1) = 1.0 / dzm;
      W(A_Idzi, 1) = 2.0 / dzm;
      double dft = 0.0, hft = 0.0;
      W(A_ut, 1) = 0.0; W(A_vt, 1) = 0.0;   // dist_from_top, h_from_top
      for (int k = 2; k <= nzc; ++k) {
        const double dzk = W(A_dzlay, k);
        W(A_Idz, k) = 1.0 / dzk;
        W(A_Idzi, k) = 2.0 / (dzm + dzk);
        dft = dft + dzm;
        hft = hft + W(A_hlay, k - 1);
        W(A_ut, k) = dft; W(A_vt, k) = hft;
        dzm = dzk;
      }
      W(A_Idzi, nzc + 1) = 2.0 / dzm;
      double dist_from_bot = 0.0, h_from_bot = 0.0;
      for (int k = nzc; k >= 2; --k) {
        dist_from_bot = dist_from_bot + W(A_dzlay, k);
        h_from_bot = h_from_bot + W(A_hlay, k);
        const double t = W(A_ut, k), ht = W(A_vt, k);
        const double v = ((t + dist_from_bot) * (ht + h_from_bot)) / ((t * dist_from_bot) * (ht * h_from_bot));
        W(A_IL2, k) = K.I_lz_rescale_sqr * v;
      }
    }
    // a time step of the background diffusivity :1051-1087, in place on u0xdz, v0xdz, T0xdz, S0xdz
    if (nzc > 1) {
      double a1k = K.k0dt * W(A_Idzi, 2);
      const double h1 = W(A_hlay, 1);
      double b1 = 1.0 / (h1 + a1k);
      double up = b1 * W(A_u, 1), vp = b1 * W(A_v, 1), Tp = b1 * W(A_T, 1), Sp = b1 * W(A_S, 1);
      W(A_u, 1) = up; W(A_v, 1) = vp; W(A_T, 1) = Tp; W(A_S, 1) = Sp;
      W(A_c1, 2) = a1k * b1;
      double d1 = h1 * b1;
      for (int k = 2; k <= nzc - 1; ++k) {
        const double bd1 = W(A_hlay, k) + d1 * a1k;
        const double a1n = K.k0dt * W(A_Idzi, k + 1);
        b1 = 1.0 / (bd1 + a1n);
        up = b1 * (W(A_u, k) + a1k * up);
        vp = b1 * (W(A_v, k) + a1k * vp);
        Tp = b1 * (W(A_T, k) + a1k * Tp);
        Sp = b1 * (W(A_S, k) + a1k * Sp);
        W(A_u, k) = up; W(A_v, k) = vp; W(A_T, k) = Tp; W(A_S, k) = Sp;
        W(A_c1, k + 1) = a1n * b1; d1 = bd1 * b1;
        a1k = a1n;
      }
      const double hn = W(A_hlay, nzc);
      b1 = 1.0 / ((hn + d1 * a1k) + K.k0dt * W(A_Idzi, nzc + 1));
      double un = b1 * (W(A_u, nzc) + a1k * up), vn = b1 * (W(A_v, nzc) + a1k * vp);
      b1 = 1.0 / (hn + d1 * a1k);
      double Tn = b1 * (W(A_T, nzc) + a1k * Tp), Sn = b1 * (W(A_S, nzc) + a1k * Sp);
      W(A_u, nzc) = un; W(A_v, nzc) = vn; W(A_T, nzc) = Tn; W(A_S, nzc) = Sn;
      for (int k = nzc - 1; k >= 1; --k) {
        const double c1 = W(A_c1, k + 1);
        un = W(A_u, k) + c1 * un; vn = W(A_v, k) + c1 * vn; Tn = W(A_T, k) + c1 * Tn; Sn = W(A_S, k) + c1 * Sn;
        W(A_u, k) = un; W(A_v, k) = vn; W(A_T, k) = Tn; W(A_S, k) = Sn;
      }
    } else {
      const double h1 = W(A_hlay, 1);
      double b1 = 1.0 / (h1 + K.k0dt * W(A_Idzi, 2));
      W(A_u, 1) = b1 * W(A_u, 1); W(A_v, 1) = b1 * W(A_v, 1);
      b1 = 1.0 / h1;
      W(A_T, 1) = b1 * W(A_T, 1); W(A_S, 1) = b1 * W(A_S, 1);
    }
    // h_Int, dz_Int :1095-1107
    {
      W(A_hInt, 1) = 0.0; W(A_hInt, 2) = W(A_hlay, 1);
      W(A_dzInt, 1) = 0.0; W(A_dzInt, 2) = W(A_dzlay, 1);
      for (int k = 2; k <= nzc - 1; ++k) {
        const double hk = W(A_hlay, k), hm = W(A_hlay, k - 1), hp = W(A_hlay, k + 1), dzk = W(A_dzlay, k);
        const double Norm = 1.0 / (hk * (hm + hp) + 2.0 * hm * hp);
        const double wt_a = ((hk + hp) * hm) * Norm, wt_b = ((hm + hk) * hp) * Norm;
        W(A_hInt, k) = W(A_hInt, k) + hk * wt_a;
        W(A_hInt, k + 1) = hk * wt_b;
        W(A_dzInt, k) = W(A_dzInt, k) + dzk * wt_a;
        W(A_dzInt, k + 1) = dzk * wt_b;
      }
      W(A_hInt, nzc) = W(A_hInt, nzc) + W(A_hlay, nzc); W(A_hInt, nzc + 1) = 0.0;
      W(A_dzInt, nzc) = W(A_dzInt, nzc) + W(A_dzlay, nzc); W(A_dzInt, nzc + 1) = 0.0;
    }
    // dbuoy_dT, dbuoy_dS :1125-1147
    if (use_T) {
      double pres = surface_pres, Tm = W(A_T, 1), Sm = W(A_S, 1);
      for (int k = 2; k <= nzc; ++k) {
        pres = pres + K.gR0 * W(A_hlay, k - 1);
        const double Tk = W(A_T, k), Sk = W(A_S, k);
        const double T_int = 0.5 * (Tm + Tk), Sal_int = 0.5 * (Sm + Sk), pPa = K.p_to_Pa * pres;
        double dR_dT = 0.0, dR_dS = 0.0;
#define KS_EOS(F) eos_density_derivs<F>(K, T_int, Sal_int, pPa, dR_dT, dR_dS)
        EOS_FORM_DISPATCH(K.form, KS_EOS);
#undef KS_EOS
        W(A_dbT, k) = K.rho_scale * dR_dT;
        W(A_dbS, k) = K.rho_scale * dR_dS;
        Tm = Tk; Sm = Sk;
      }
    } else {
      for (int k = 1; k <= nzc + 1; ++k) { W(A_dbT, k) = -K.g_R0; W(A_dbS, k) = 0.0; }
    }

    // N2 and S2 of the initial state :1165-1184
    ks_proj(W, K, A_kappa, 0.0, nzc, A_u, A_v, A_T, A_S, 1, nzc);
    double dt_rem = K.dt;
    for (int k = 1; k <= nzc + 1; ++k) {
      if (K.diag) { W(A_N2i, k) = W(A_N2, k); W(A_S2i, k) = W(A_S2, k); W(A_N2m, k) = 0.0; W(A_S2m, k) = 0.0; }
      W(A_KQ, k) = 0.0;
      W(A_kavg, k) = 0.0; W(A_tkeavg, k) = 0.0;
      const double hI = W(A_hInt, k);
      double lsa = 0.0;
      if (hI > 0.0) lsa = 0.1 * K.k0dt * W(A_Idzi, k) / hI;
      W(A_lsavg, k) = lsa;
    }

    int its = 0;
    for (int itt = 1; itt <= K.max_KS_it; ++itt) {
      its = itt;
      ks_find<true>(W, K, nzc, f2, A_kappa, A_KQ, A_tke, A_kout);
      int ks_kappa = nz + 1, ke_kappa = 0;   // GV%ke + 1
      for (int k = 2; k <= nzc; ++k) if (W(A_kout, k) > 0.0) { ks_kappa = k; break; }
      for (int k = nzc; k >= ks_kappa; --k) if (W(A_kout, k) > 0.0) { ke_kappa = k; break; }
      if (ke_kappa == nzc) W(A_kout, nzc + 1) = 0.0;

      double dt_now;
      if ((ke_kappa < ks_kappa) || (itt == K.max_KS_it)) {
        dt_now = dt_rem;
      } else {
        const int pks = (ks_kappa - 1 > 1) ? ks_kappa - 1 : 1, pke = (ke_kappa < nzc) ? ke_kappa : nzc;
        double dt_test = dt_rem, dt_inc;
        bool valid_dt = false;
        const int nhalf = (K.max_KS_it + 1 - itt) / 2;
        for (int itt_dt = 1; itt_dt <= nhalf; ++itt_dt) {
          ks_proj(W, K, A_kout, 0.5 * dt_test, nzc, A_ut, A_vt, A_Tt, A_St, pks, pke);
          valid_dt = ks_scan(W, K, nzc, ks_kappa, ke_kappa, 1.0 / dt_test, K.restrictive != 0);
          if (valid_dt) break;
          dt_test = 0.5 * dt_test;
        }
        if ((dt_test < dt_rem) && valid_dt) {
          dt_inc = 0.5 * dt_test;
          for (int itt_dt = 1; itt_dt <= 5; ++itt_dt) {   // dt_refinements
            ks_proj(W, K, A_kout, 0.5 * (dt_test + dt_inc), nzc, A_ut, A_vt, A_Tt, A_St, pks, pke);
            valid_dt = ks_scan(W, K, nzc, ks_kappa, ke_kappa, 1.0 / (dt_test + dt_inc), false);
            if (valid_dt) dt_test = dt_test + dt_inc;
            dt_inc = 0.5 * dt_inc;
          }
        } else {
          dt_inc = 0.0;
        }
        dt_now = fmin1(dt_test * (1.0 + K.tol_err) + dt_inc, dt_rem);
        for (int k = 2; k <= nzc; ++k) W(A_lsavg, k) = W(A_lsavg, k) + dt_now * W(A_lsrc, k);
      }

      if (ke_kappa < ks_kappa) {   // :1303: there is no mixing now, and will not be again
        const double dt_wt = dt_rem / K.dt;
        dt_rem = 0.0;
        for (int k = 1; k <= nzc + 1; ++k) {
          W(A_kmid, k) = 0.0;
          W(A_tkeavg, k) = W(A_tkeavg, k) + dt_wt * W(A_tke, k);
        }
      } else {
        // the predictor with kappa_out and a copy of K_Q, then the corrector with kappa_mid :1316-1343
        for (int k = 1; k <= nzc + 1; ++k) W(A_KQt, k) = W(A_KQ, k);
        for (int pass = 0; pass < 2; ++pass) {
          const int pks = (ks_kappa - 1 > 1) ? ks_kappa - 1 : 1, pke = (ke_kappa < nzc) ? ke_kappa : nzc;
          ks_proj(W, K, pass ? A_kmid : A_kout, dt_now, nzc, A_ut, A_vt, A_Tt, A_St, pks, pke);
          ks_find<false>(W, K, nzc, f2, A_kout, pass ? A_KQ : A_KQt, A_tkep, A_kpred);
          if (pass == 0) {
            ks_kappa = nz + 1; ke_kappa = 0;
            for (int k = 1; k <= nzc + 1; ++k) {
              const double km = 0.5 * (W(A_kout, k) + W(A_kpred, k));
              W(A_kmid, k) = km;
              if ((km > 0.0) && (k < ks_kappa)) ks_kappa = k;
              if (km > 0.0) ke_kappa = k;
            }
          }
        }
        const double dt_wt = dt_now / K.dt;
        dt_rem = dt_rem - dt_now;
        for (int k = 1; k <= nzc + 1; ++k) {
          const double kp = W(A_kpred, k);
          const double km = 0.5 * (W(A_kout, k) + kp);
          W(A_kmid, k) = km;
          W(A_kavg, k) = W(A_kavg, k) + km * dt_wt;
          W(A_tkeavg, k) = W(A_tkeavg, k) + dt_wt * 0.5 * (W(A_tkep, k) + W(A_tke, k));
          if (K.diag) {
            W(A_N2m, k) = W(A_N2m, k) + dt_wt * W(A_N2, k);
            W(A_S2m, k) = W(A_S2m, k) + dt_wt * W(A_S2, k);
          }
          W(A_kappa, k) = kp;
        }
      }
      if (dt_rem > 0.0) ks_proj(W, K, A_kmid, dt_now, nzc, A_u, A_v, A_T, A_S, 1, nzc);   // :1359-1366
      if (dt_rem <= 0.0) break;
    }

    // back to the model's layers :332-380 and the masked stores :388-392
    const bool whole = (nz == nzc);
    const int a_tk = (whole && K.all_layer_bug) ? A_tke : A_tkeavg;
    for (int k = 1; k <= nz + 1; ++k) {
      const size_t o = (size_t)(k - 1) * slab + x;
      double kap, tk, n2i = 0.0, s2i = 0.0, n2m = 0.0, s2m = 0.0;
      if (whole) {
        kap = W(A_kavg, k); tk = W(a_tk, k);
        if (K.diag) { n2i = W(A_N2i, k); s2i = W(A_S2i, k); n2m = W(A_N2m, k); s2m = W(A_S2m, k); }
      } else {
        const int c = (int)W(A_kc, k);
        const double kf = W(A_kf, k);
        if (kf == 0.0) {
          kap = W(A_kavg, c); tk = W(A_tkeavg, c);
          if (K.diag) { n2i = W(A_N2i, c); s2i = W(A_S2i, c); n2m = W(A_N2m, c); s2m = W(A_S2m, c); }
        } else {
          kap = (1.0 - kf) * W(A_kavg, c) + kf * W(A_kavg, c + 1);
          tk = (1.0 - kf) * W(A_tkeavg, c) + kf * W(A_tkeavg, c + 1);
          if (K.diag) {
            n2i = (1.0 - kf) * W(A_N2i, c) + kf * W(A_N2i, c + 1); s2i = (1.0 - kf) * W(A_S2i, c) + kf * W(A_S2i, c + 1);
            n2m = (1.0 - kf) * W(A_N2m, c) + kf * W(A_N2m, c + 1); s2m = (1.0 - kf) * W(A_S2m, c) + kf * W(A_S2m, c + 1);
          }
        }
      }
      P.kappa_io[o] = mask * kap;
      P.tke_io[o] = mask * tk;
      P.kv_io[o] = (mask * kap) * K.Prandtl;
      if (P.N2_init) P.N2_init[o] = n2i;
      if (P.S2_init) P.S2_init[o] = s2i;
      if (P.N2_mean) P.N2_mean[o] = n2m;
      if (P.S2_mean) P.S2_mean[o] = s2m;
    }
    if (P.its) P.its[x] = (double)its;
  }
}

constexpr int KS_DEFAULT_WORK_COLUMNS = 65536;   // 256 compute units x 4 SIMDs x one wavefront of 64: 2.0 GB at 75 layers

}  // namespace

// Kappa_shear_CS, tv%eqn_of_state, the device copy of GV%Rlay and the workspace of the lanes in flight
struct KsState {
  mom6x_kappa_shear_params P;
  bool use_eos; mom6x_eos_params eos;
  double *Rlay;    // nk, null when init got none
  double *work;    // [KS_NARR][nk + 1][nslots]
  int nslots;
};

void kappa_shear_free(mom6x_ctx *c) {
  if (!c->ks) return;
  (void)hipFree(c->ks->Rlay);
  (void)hipFree(c->ks->work);
  delete c->ks;
  c->ks = nullptr;
}

extern "C" int mom6x_kappa_shear_init(mom6x_ctx *c, const mom6x_kappa_shear_params *p, const mom6x_eos_params *eos, const double *Rlay) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_kappa_shear_init: null argument");
  HIPCHK(hipSetDevice(c->device));
  kappa_shear_free(c);   // first: a refused or invalid init leaves no module behind, whatever was initialized before
  REFUSE(p->KS_at_vertex, "kappa_shear_init", "VERTEX_SHEAR (Calc_kappa_shear_vertex)");
  REFUSE(!c->GV.Boussinesq, "kappa_shear_init", "non-Boussinesq mode");
  REQUIRE(p->max_KS_it >= 1, MOM6X_EINVAL, "kappa_shear_init: MAX_KAPPA_SHEAR_IT must be at least 1");
  REQUIRE(p->max_RiNo_it >= 1, MOM6X_EINVAL, "kappa_shear_init: MAX_RINO_IT must be at least 1");
  REQUIRE(p->RiNo_crit > 0.0, MOM6X_EINVAL, "kappa_shear_init: RINO_CRIT must be positive");
  REQUIRE(p->kappa_src_max_chg > 1.0, MOM6X_EINVAL, "kappa_shear_init: KAPPA_SHEAR_MAX_KAP_SRC_CHG must be greater than 1");
  REQUIRE(p->work_columns >= 0, MOM6X_EINVAL, "kappa_shear_init: work_columns must not be negative");
  REQUIRE(p->nkml >= 1, MOM6X_EINVAL, "kappa_shear_init: nkml must be at least 1");
  REQUIRE(p->lambda != 0.0, MOM6X_EINVAL, "kappa_shear_init: KAPPA_BUOY_SCALE_COEF must not be 0");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "kappa_shear_init: unknown EQN_OF_STATE form");
  KsState *s = new KsState();
  c->ks = s;
  s->P = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  s->Rlay = nullptr; s->work = nullptr;
  const Dm d = c->d;
  const long long ncol = (long long)d.ni * d.nj;
  long long ns = p->work_columns > 0 ? p->work_columns : (ncol < KS_DEFAULT_WORK_COLUMNS ? ncol : KS_DEFAULT_WORK_COLUMNS);
  ns = (ns + 63) / 64 * 64;   // whole wavefronts
  s->nslots = (int)ns;
  const size_t nw = (size_t)KS_NARR * (size_t)(d.nk + 1) * (size_t)ns * sizeof(double);
  HIPCHK(hipMalloc(&s->work, nw));
  HIPCHK(hipMemsetAsync(s->work, work_fill_byte(), nw, c->stream));
  if (Rlay) {
    HIPCHK(hipMalloc(&s->Rlay, (size_t)d.nk * sizeof(double)));
    HIPCHK(hipMemcpy(s->Rlay, Rlay, (size_t)d.nk * sizeof(double), hipMemcpyHostToDevice));
  }
  return MOM6X_OK;
}

extern "C" long long mom6x_kappa_shear_work_bytes(mom6x_ctx *c) {
  if (!c || !c->ks) return 0;
  return (long long)KS_NARR * (long long)(c->d.nk + 1) * (long long)c->ks->nslots * (long long)sizeof(double);
}

extern "C" int mom6x_Calculate_kappa_shear(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *T,
                                           const double *S, const double *p_surf, double dt, int zero_mix, double *kappa_io,
                                           double *tke_io, double *kv_io, double *N2_init, double *S2_init, double *N2_mean,
                                           double *S2_mean, double *KS_its) {
  REQUIRE(c && c->ks, MOM6X_EINVAL, "Calculate_kappa_shear: Module must be initialized before it is used.");
  const KsState *s = c->ks;
  const mom6x_kappa_shear_params &Q = s->P;
  const mom6x_vgrid &GV = c->GV;
  REQUIRE(u && v && h, MOM6X_EINVAL, "Calculate_kappa_shear: null u, v or h");
  REQUIRE(kappa_io && tke_io && kv_io, MOM6X_EINVAL, "Calculate_kappa_shear: null kappa_io, tke_io or kv_io");
  REQUIRE((T != nullptr) == (S != nullptr), MOM6X_EINVAL, "Calculate_kappa_shear: tv%T and tv%S are given together or not at all");
  REQUIRE(!T || s->use_eos, MOM6X_EINVAL, "Calculate_kappa_shear: tv%T and tv%S need the equation of state given to init");
  REQUIRE(T || s->Rlay, MOM6X_EINVAL, "Calculate_kappa_shear: without tv%T and tv%S the layered arm needs the GV%Rlay given to init");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "Calculate_kappa_shear: dt must be positive");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;

  KsK K;
  memset(&K, 0, sizeof(K));
  K.dt = dt; K.zero = 0.0; K.H_to_Z = GV.H_to_Z;
  K.gR0 = GV.H_to_RZ * GV.g_Earth;                 // :1006
  K.g_R0 = Q.g_Earth_Z_T2 / GV.Rho0;               // :1007
  K.k0dt = dt * Q.kappa_0;                         // :218, :1008
  K.dz_massless = 0.1 * sqrt(Q.Z_to_m_m_to_H * K.k0dt);   // :219
  K.h_neglect = GV.H_subroundoff;
  K.rho_scale = Q.kg_m3_to_R * (-K.g_R0);          // MOM_EOS.F90:820-823 with scale = -g_R0
  K.p_to_Pa = Q.RL2_T2_to_Pa;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;
  K.Ri_crit = Q.RiNo_crit; K.Shearmix_rate = Q.Shearmix_rate; K.FRi_curvature = Q.FRi_curvature;
  K.c_N2 = Q.C_N * Q.C_N; K.c_S2 = Q.C_S * Q.C_S;  // :1628
  K.Ilambda2 = 1.0 / (Q.lambda * Q.lambda);        // :1632
  K.I_lz_rescale_sqr = 1.0;                        // :1010
  if (Q.lz_rescale > 0) K.I_lz_rescale_sqr = 1 / (Q.lz_rescale * Q.lz_rescale);
  K.q0 = Q.TKE_bg; K.kappa0 = Q.kappa_0; K.kappa_seed = Q.kappa_seed; K.kappa_trunc = Q.kappa_trunc;
  {                                                // :1630
    const double floor_ = 1.0E-20 * (Q.m_to_Z * Q.m_to_Z) * (Q.T_to_s * Q.T_to_s);
    K.TKE_min = (floor_ > Q.TKE_bg) ? floor_ : Q.TKE_bg;
  }
  K.tol_err = Q.kappa_tol_err;
  K.tol_dksrc = Q.kappa_src_max_chg;               // :1012-1019
  K.tol_dksrc_low = (K.tol_dksrc == 10.0) ? 0.95 : (K.tol_dksrc - 0.5) / K.tol_dksrc;
  K.tol2 = 2.0 * Q.kappa_tol_err;
  K.Prandtl = Q.Prandtl_turb; K.vel_under = Q.vel_underflow; K.m_to_Z = Q.m_to_Z; K.L_to_Z = Q.L_to_Z;
  K.max_RiNo_it = Q.max_RiNo_it; K.max_KS_it = Q.max_KS_it; K.nkml = Q.nkml; K.elim = Q.eliminate_massless != 0;
  K.dKdQ_bug = Q.dKdQ_iteration_bug != 0; K.all_layer_bug = Q.all_layer_TKE_bug != 0; K.restrictive = Q.restrictive_tolerance_check != 0;
  K.zero_mix = zero_mix != 0; K.form = T ? s->eos.form : 0;
  K.diag = (N2_init || S2_init || N2_mean || S2_mean) ? 1 : 0;
  K.ni = d.ni; K.ncol = d.ni * d.nj;

  KsP A;
  A.u = u; A.v = v; A.h = h; A.T = T; A.S = S; A.p_surf = p_surf; A.Rlay = s->Rlay;
  A.kappa_io = kappa_io; A.tke_io = tke_io; A.kv_io = kv_io; A.N2_init = N2_init; A.S2_init = S2_init; A.N2_mean = N2_mean;
  A.S2_mean = S2_mean; A.its = KS_its;
  KLAUNCH(c, "k_kappa_shear", k_kappa_shear, dim3((unsigned)(s->nslots / 64)), dim3(64), d, c->G, K, A, s->work, s->nslots);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
