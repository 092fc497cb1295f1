// lateral_mixing_coeffs.hip -- the isopycnal slopes and the Eady growth rate of variable mixing on gfx950.
//
//   calc_slope_functions              <- MOM_lateral_mixing_coeffs.F90:686-738, its three branches :708-723
//   calc_isoneutral_slopes            <- MOM_isopycnal_slopes.F90:31-608 (halo = 1, Boussinesq, no open boundaries, no Stanley term),
//                                        vert_fill_TS :612-700 WITHOUT larger_h_denom (h0 = h_neglect), find_eta(halo_size=2)
//   calc_Eady_growth_rate_2D          <- :962-1112
//   calc_Visbeck_coeffs_old           <- :743-959, the arm without open boundaries
//   calc_slope_functions_using_just_e <- :1116-1275
//   VarMix_init                       <- :1759-1772 (L2u, L2v)
//
// k_vm_cols: one lane per cell of the domain widened by two: e bottom-up (find_eta's order), pres top-down, the vert_fill_TS solve.
// k_vm_faces: one lane per face, both directions in one launch (blockIdx.z), walks K = 2..nz; with use_simpler_Eady_growth_rate it
// carries vint_SN and sum_dz of calc_Eady_growth_rate_2D along (the reference's summation order), so dzu, dzSxN and N2 only go to
// memory when a diagnostic asks for them.  k_vm_eady_combine: the four-neighbour combination from the un-combined planes.
// k_vm_visbeck: the sums of calc_Visbeck_coeffs_old, h4_u | h4_v formed from h as the walk goes.  k_vm_just_e: the third branch in
// one launch, the neighbours' E_x | E_y recomputed from e.  MAX and MIN are fmax1 and fmin1 of mom6x_dev.h, but the radicand of
// dzSxN | dzSyN (MOM_isopycnal_slopes.F90:418, :602) is dmax: max(0.0, -0.0), which both vertical density differences being -0.0
// make of it, the compiled reference answers with its second argument, and sqrt(-0.0) = -0.0 shows in the diagnostic (found by
// tests/test_ref_parity_cpu.py with the case eady_tie).  The density gradients (isoneutral_grads) and the vert_fill_TS solve come from isopycnal_slopes_dev.h, which
// thickness_diffuse.hip shares; the lane of a face from face_lane (mom6x_dev.h), the EOS form's kernel from EOS_FORM_DISPATCH.
#include "mom6x_dev.h"
#include "eos_dev.h"
#include "isopycnal_slopes_dev.h"

// VarMix_CS and the work arrays of mom6x_varmix_init
struct VmState {
  mom6x_varmix_params p;
  bool use_eos;
  mom6x_eos_params eos;
  double *Rlay, *g_prime;   // device copies (nk): one allocation, Rlay owns it
  double *work;             // [e (nk+1) | pres, T_f, S_f, c1 (nk each, with an EOS) | N2_u, N2_v (nk+1 each, Visbeck) | SN raw u, v (2 planes, Eady)]
};

namespace {

struct VmK {
  double h_neglect, h_neglect2, dz_neglect, H_to_Z, gH, Z_to_L, G_Rho0, kap_dt_x2, h0;
  double D_scale, r_crp_dist, S2max, hsub4, H_cutoff, dZ_cutoff, h_min_N2;
  double dRho_dT, dRho_dS;
  int crop, Ktop, use_dztot;
};
struct VmDiag { double *N2[2], *dz[2], *dzSN[2]; };

// find_eta(halo_size=2) :91-97, pres (MOM_isopycnal_slopes.F90:231-247) and vert_fill_TS(halo+1) on cells isc-2..iec+2,
// jsc-2..jec+2.  e[K], pres[K]: at the interface ABOVE layer K (e has nk+1 planes).  Lanes start at i = -IAL.
__global__ void __launch_bounds__(256)
k_vm_cols(Dm d, const double *__restrict__ G, VmK K, const double *__restrict__ h, const double *__restrict__ T,
          const double *__restrict__ S, const double *__restrict__ p_surf, double *__restrict__ e, double *__restrict__ pres,
          double *Tf, double *Sf, double *c1) {
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -2 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -2 || i > d.ni + 1 || j > d.nj + 1) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const int nz = d.nk;
  double el = -(gm(G, d, MOM6X_G_bathyT)[x] + 0.0);
  e[(size_t)nz * slab + x] = el;
  for (int k = nz - 1; k >= 0; --k) {
    const size_t o = (size_t)k * slab + x;
    el = el + h[o] * K.H_to_Z;
    e[o] = el;
  }
  if (!pres) return;
  double pr = p_surf ? p_surf[x] : 0.0;
  for (int k = 0; k < nz; ++k) {
    const size_t o = (size_t)k * slab + x;
    pres[o] = pr;
    pr = pr + K.gH * h[o];
  }
  if (!Tf) return;
  vert_fill_TS_col(h, T, S, Tf, Sf, c1, x, slab, nz, K.kap_dt_x2, K.h0, K.h_neglect);
}

// calc_isoneutral_slopes(halo=1) and, with BR == 1, the vertical sums of calc_Eady_growth_rate_2D.  FORM 0: no EOS (GV%Rlay).
// The faces of face_lane<1>: one wider than the other face kernels'.
template <int FORM, int BR>
__global__ void __launch_bounds__(256)
k_vm_faces(Dm d, const double *__restrict__ G, VmK K, const double *__restrict__ h, const double *__restrict__ e,
           const double *__restrict__ pres, const double *__restrict__ Tf, const double *__restrict__ Sf,
           const double *__restrict__ Rlay, double *__restrict__ slope_x, double *__restrict__ slope_y, VmDiag D,
           double *__restrict__ raw_u, double *__restrict__ raw_v) {
  constexpr bool EOS = FORM != 0;
  const FaceLane f = face_lane<1>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t x = f.x, y = f.y, slab = (size_t)d.slab;
  const int nz = d.nk;
  double *slope = dir ? slope_y : slope_x;
  double *N2 = D.N2[dir], *dzo = D.dz[dir], *dzs = D.dzSN[dir];
  const double Igrad = gm(G, d, dir ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  const double mask = gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  const size_t ob = (size_t)nz * slab;
  if (N2) { N2[x] = 0.0; N2[ob + x] = 0.0; }      // MOM_isopycnal_slopes.F90:174-209
  if (dzo) { dzo[x] = 0.0; dzo[ob + x] = 0.0; }
  if (dzs) { dzs[x] = 0.0; dzs[ob + x] = 0.0; }

  double e1L = 0.0, e1R = 0.0, ebL = 0.0, ebR = 0.0, vint_SN = 0.0, sum_dz = K.dz_neglect;
  if constexpr (BR == 1) { e1L = e[x]; e1R = e[y]; ebL = e[ob + x]; ebR = e[ob + y]; }
  double hLm = h[x], hRm = h[y];
  double TLm = 0.0, TRm = 0.0, SLm = 0.0, SRm = 0.0;
  if constexpr (EOS) { TLm = Tf[x]; TRm = Tf[y]; SLm = Sf[x]; SRm = Sf[y]; }
  size_t o = slab;
  for (int k = 1; k < nz; ++k, o += slab) {       // K = 2..nz; layers k-1 (A, m) and k (B, k)
    const double hLk = h[o + x], hRk = h[o + y];
    const double eL = e[o + x], eR = e[o + y];
    // g.drdkL, g.drdkR go IN without an EOS (FORM 0, from GV%Rlay) and come OUT with one; T, S and pres_u are then not read
    double TLk = 0.0, TRk = 0.0, SLk = 0.0, SRk = 0.0, pres_u = 0.0;
    IsoGrad g;
    if constexpr (EOS) {
      TLk = Tf[o + x]; TRk = Tf[o + y]; SLk = Sf[o + x]; SRk = Sf[o + y];
      pres_u = 0.5 * (pres[o + x] + pres[o + y]);
    } else {
      g.drdkL = Rlay[k] - Rlay[k - 1]; g.drdkR = g.drdkL;
    }
    isoneutral_grads<FORM>(K, hLm, hRm, hLk, hRk, TLm, TRm, TLk, TRk, SLm, SRm, SLk, SRk, pres_u, eL, eR, Igrad, g);
    const double dzu = 0.5 * (g.dzaL + g.dzaR);
    if (N2) N2[o + x] = K.G_Rho0 * g.drdz * mask;
    double sl;
    if constexpr (EOS) {
      sl = (g.mag_grad2 > 0.0) ? g.drdx / sqrt(g.mag_grad2) : 0.0;
    } else {
      sl = (eR - eL) * Igrad;
    }
    slope[o + x] = sl;
    if (dzo) dzo[o + x] = dzu;
    bool want_dzSN = dzs != nullptr;
    if constexpr (BR == 1) want_dzSN = true;
    if (want_dzSN) {
      const double dzSN = sqrt(K.G_Rho0 * dmax(0.0, (g.wtL * (g.dzaL * g.drdkL)) + (g.wtR * (g.dzaR * g.drdkR))) / (g.wtL + g.wtR)) * fabs(sl) * mask;
      if (dzs) dzs[o + x] = dzSN;
      if constexpr (BR == 1) {                    // :1014-1041 | :1057-1085
        double dnew = sum_dz + dzu;
        dnew = fmin1(dnew, K.D_scale);
        const double dz = fmax1(0.0, dnew - sum_dz);
        double weight = dz / (dzu + K.dz_neglect);
        if (K.crop) {
          double dT = fmin1(e1L, e1R), dB = fmax1(eL, eR);
          weight = weight * fmin1(fmax1(0.0, (dT - dB) * K.r_crp_dist), 1.0);
          dT = fmin1(eL, eR); dB = fmax1(ebL, ebR);
          weight = weight * fmin1(fmax1(0.0, (dT - dB) * K.r_crp_dist), 1.0);
        }
        // weight at the u faces, weight**2 at the v faces (:1028 | :1071, :1083): the reference's own asymmetry
        vint_SN = vint_SN + (dir ? weight * weight : weight) * dzSN;
        sum_dz = sum_dz + weight * dzu;
      }
    }
    hLm = hLk; hRm = hRk; TLm = TLk; TRm = TRk; SLm = SLk; SRm = SRk;
  }
  if constexpr (BR == 1) {
    // :1045-1046 at I = -1..ni-1, j = -1..nj | :1088 at i = -1..ni, J = -1..nj-1
    const bool in = dir ? (f.j >= -1 && f.j <= d.nj - 1) : (f.i >= -1 && f.i <= d.ni - 1);
    if (in) (dir ? raw_v : raw_u)[x] = mask * (vint_SN / sum_dz);
  }
}

// :1002-1005 and :1092-1105 on isc-1..iec+1 x jsc-1..jec+1: SN_u from the un-combined SN_v, SN_v from SN_cpy.
__global__ void __launch_bounds__(256)
k_vm_eady_combine(Dm d, const double *__restrict__ ru, const double *__restrict__ rv, double *__restrict__ SN_u,
                  double *__restrict__ SN_v) {
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i < -1 || i > d.ni || j > d.nj) return;
  const size_t x = ix2(d, i, j), p = (size_t)d.pitch;
  double su = 0.0, sv = 0.0;
  if (i <= d.ni - 1) {
    su = ru[x];
    if (j >= 0 && j <= d.nj - 1) {
      const double a = rv[x], b = rv[x + 1 - p], c = rv[x + 1], e_ = rv[x - p];
      su = sqrt(su * su + 0.25 * (((a * a) + (b * b)) + ((c * c) + (e_ * e_))));
    }
  }
  if (j <= d.nj - 1) {                            // J = jsc-1..jec: the row jsc-1 is combined too (:1099)
    sv = rv[x];
    if (i >= 0 && i <= d.ni - 1) {
      const double a = ru[x], b = ru[x - 1 + p], c = ru[x + p], e_ = ru[x - 1];
      sv = sqrt(sv * sv + 0.25 * (((a * a) + (b * b)) + ((c * c) + (e_ * e_))));
    }
  }
  SN_u[x] = su;
  SN_v[x] = sv;
}

// The four faces of the other direction around a face at x (own stride st, other stride ot), in the order the reference adds them:
// u: NW, SE, NE, SW (:879-880); v: SE, NW, NE, SW (:922-923).  Each has its two cells at f and f + ot.
#define VM_NBR_FACES const size_t f1 = x, f2 = x + st - ot, f3 = x + st, f4 = x - ot

// calc_Visbeck_coeffs_old :856-940 on the faces of face_lane<0>.
__global__ void __launch_bounds__(256)
k_vm_visbeck(Dm d, const double *__restrict__ G, VmK K, const double *__restrict__ h, const double *__restrict__ slope_x,
             const double *__restrict__ slope_y, const double *__restrict__ N2_u, const double *__restrict__ N2_v,
             double *__restrict__ SN_u, double *__restrict__ SN_v, double *__restrict__ S2_u, double *__restrict__ S2_v) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t st = f.st, ot = f.ot, x = f.x, y = f.y, slab = (size_t)d.slab;
  const int nz = d.nk;
  VM_NBR_FACES;
  const double *so = dir ? slope_y : slope_x, *sn = dir ? slope_x : slope_y, *N2 = dir ? N2_v : N2_u;
  const double *mo = gm(G, d, dir ? MOM6X_G_mask2dCu : MOM6X_G_mask2dCv);
  const double mask = gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  const double m1 = mo[f1], m2 = mo[f2], m3 = mo[f3], m4 = mo[f4];
  // the products of the two thicknesses across each face in the layer above
  double a0 = h[x], b0 = h[y];
  double qo = a0 * b0, q1 = a0 * h[f1 + ot], q2 = h[f2] * b0, q3 = b0 * h[f3 + ot], q4 = h[f4] * a0;
  double SN = 0.0, S2s = 0.0, Hs = 0.0;
  size_t o = slab;
  for (int k = 1; k < nz; ++k, o += slab) {
    const double a = h[o + x], b = h[o + y];
    const double po = a * b, p1 = a * h[o + f1 + ot], p2 = h[o + f2] * b, p3 = b * h[o + f3 + ot], p4 = h[o + f4] * a;
    const double Hdn = sqrt(po), Hup = sqrt(qo);
    const double H_geom = sqrt(Hdn * Hup);
    const double w1 = m1 * (p1 * q1), w2 = m2 * (p2 * q2), w3 = m3 * (p3 * q3), w4 = m4 * (p4 * q4);   // h4_v | h4_u :844-847
    const double s0 = so[o + x], s1 = sn[o + f1], s2 = sn[o + f2], s3 = sn[o + f3], s4 = sn[o + f4];
    double S2 = s0 * s0 + (((w1 * (s1 * s1)) + (w2 * (s2 * s2))) + ((w3 * (s3 * s3)) + (w4 * (s4 * s4)))) /
                              (((w1 + w2) + (w3 + w4)) + K.hsub4);
    if (K.S2max > 0.0) S2 = S2 * K.S2max / (S2 + K.S2max);
    const double N2p = fmax1(0.0, N2[o + x]);
    SN = SN + sqrt(S2 * N2p) * H_geom;
    S2s = S2s + S2 * H_geom;
    Hs = Hs + H_geom;
    qo = po; q1 = p1; q2 = p2; q3 = p3; q4 = p4;
  }
  if (Hs > 0.0) {
    SN = mask * SN / Hs;
    S2s = mask * S2s / Hs;
  } else {
    SN = 0.0;
  }
  (dir ? SN_v : SN_u)[x] = SN;
  double *S2o = dir ? S2_v : S2_u;
  if (S2o) S2o[x] = S2s;
}

// calc_slope_functions_using_just_e :1185-1273.  The same face ranges as k_vm_visbeck.
__global__ void __launch_bounds__(256)
k_vm_just_e(Dm d, const double *__restrict__ G, VmK K, const double *__restrict__ h, const double *__restrict__ e,
            const double *__restrict__ g_prime, double *__restrict__ SN_u, double *__restrict__ SN_v) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const int dir = f.dir;
  const size_t st = f.st, ot = f.ot, x = f.x, y = f.y, slab = (size_t)d.slab;
  const int nz = d.nk;
  VM_NBR_FACES;
  const double Io = gm(G, d, dir ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  const double *In = gm(G, d, dir ? MOM6X_G_IdxCu : MOM6X_G_IdyCv);
  const double I1 = In[f1], I2 = In[f2], I3 = In[f3], I4 = In[f4];
  double SN = 0.0;
  for (int k = nz - 1; k >= K.Ktop - 1; --k) {
    const size_t o = (size_t)k * slab;
    const double hL = h[o + x], hR = h[o + y], eL = e[o + x], eR = e[o + y];
    double Eo = (eR - eL) * Io;
    if (fmin1(hL, hR) < K.H_cutoff) Eo = 0.0;
    // the cells of the neighbouring faces: f1: x, x+ot; f2: y-ot, y; f3: y, y+ot; f4: x-ot, x
    const double h1 = h[o + f1 + ot], h2 = h[o + f2], h3 = h[o + f3 + ot], h4 = h[o + f4];
    double E1 = (e[o + f1 + ot] - eL) * I1, E2 = (eR - e[o + f2]) * I2, E3 = (e[o + f3 + ot] - eR) * I3, E4 = (eL - e[o + f4]) * I4;
    if (fmin1(hL, h1) < K.H_cutoff) E1 = 0.0;
    if (fmin1(h2, hR) < K.H_cutoff) E2 = 0.0;
    if (fmin1(hR, h3) < K.H_cutoff) E3 = 0.0;
    if (fmin1(h4, hL) < K.H_cutoff) E4 = 0.0;
    double S2 = (Eo * Eo + 0.25 * (((E1 * E1) + (E2 * E2)) + ((E3 * E3) + (E4 * E4))));
    const double hLm = h[o - slab + x], hRm = h[o - slab + y];
    if (fmin1(fmin1(fmin1(hLm, hRm), hL), hR) < K.H_cutoff) S2 = 0.0;
    const double Hdn = 2.0 * hL * hLm / (hL + hLm + K.h_neglect);
    const double Hup = 2.0 * hR * hRm / (hR + hRm + K.h_neglect);
    const double H_geom = sqrt(Hdn * Hup);
    SN = SN + (H_geom * S2) * (g_prime[k] / fmax1(fmax1(Hdn, Hup), K.h_min_N2));
  }
  const double mask = gm(G, d, dir ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  if (K.use_dztot) {
    const size_t ob = (size_t)nz * slab;
    const double dzL = e[x] - e[ob + x], dzR = e[y] - e[ob + y];
    SN = mask * sqrt(SN / fmax1(fmax1(dzL, dzR), K.dz_neglect));
  } else {
    const double *bT = gm(G, d, MOM6X_G_bathyT);
    const double bL = bT[x], bR = bT[y];                         // (the v loop's corrected index: bathyT(i,j+1), :1265)
    if (fmin1(bL, bR) + 0.0 > K.dZ_cutoff) SN = mask * sqrt(SN / (fmax1(bL, bR) + 0.0));   // G%Z_ref = 0
    else SN = 0.0;
  }
  (dir ? SN_v : SN_u)[x] = SN;
}

// CS%L2u, CS%L2v :1759-1772 over the whole arrays
__global__ void __launch_bounds__(256)
k_vm_L2(Dm d, const double *__restrict__ G, double L2, int by_area, int nrows, double *__restrict__ L2u, double *__restrict__ L2v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y;
  if (c >= d.pitch || r >= nrows) return;
  const size_t x = (size_t)r * d.pitch + c;
  const int i = c - d.ioff, j = r - d.joff;
  double u = L2, v = L2;
  if (by_area) {
    u = (i >= -1 && i <= d.ni - 1 && j >= 0 && j <= d.nj - 1) ? L2 * gm(G, d, MOM6X_G_areaCu)[x] : 0.0;
    v = (i >= 0 && i <= d.ni - 1 && j >= -1 && j <= d.nj - 1) ? L2 * gm(G, d, MOM6X_G_areaCv)[x] : 0.0;
  }
  if (L2u) L2u[x] = u;
  if (L2v) L2v[x] = v;
}

}  // namespace

void varmix_free(mom6x_ctx *c) {
  VmState *s = c->vm;
  if (!s) return;
  (void)hipFree(s->work);
  (void)hipFree(s->Rlay);
  delete s;
  c->vm = nullptr;
}

// the device copies and work arrays of a state whose parameters are set
static int varmix_alloc(mom6x_ctx *c, VmState *s, const double *Rlay, const double *g_prime) {
  const mom6x_varmix_params *p = &s->p;
  const Dm d = c->d;
  const bool slopes = p->calculate_Eady_growth_rate && p->use_stored_slopes;
  if (p->calculate_Eady_growth_rate) {
    const size_t nk = (size_t)d.nk;
    HIPCHK(hipMalloc(&s->Rlay, 2 * nk * sizeof(double)));
    s->g_prime = s->Rlay + nk;
    HIPCHK(hipMemsetAsync(s->Rlay, 0, 2 * nk * sizeof(double), c->stream));
    if (Rlay) HIPCHK(hipMemcpyAsync(s->Rlay, Rlay, nk * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (g_prime) HIPCHK(hipMemcpyAsync(s->g_prime, g_prime, nk * sizeof(double), hipMemcpyHostToDevice, c->stream));
    size_t planes = nk + 1;
    if (slopes && s->use_eos) planes += 4 * nk;
    if (slopes && !p->use_simpler_Eady_growth_rate) planes += 2 * (nk + 1);
    if (p->use_simpler_Eady_growth_rate) planes += 2;
    const size_t n = planes * d.slab * sizeof(double);
    HIPCHK(hipMalloc(&s->work, n));
    HIPCHK(hipMemsetAsync(s->work, work_fill_byte(), n, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the host arrays may go once the call returns)
  }
  return MOM6X_OK;
}

extern "C" int mom6x_varmix_init(mom6x_ctx *c, const mom6x_varmix_params *p, const mom6x_eos_params *eos, const double *Rlay,
                                 const double *g_prime, double *L2u, double *L2v) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_varmix_init: null argument");
  REFUSE(p->use_stanley_iso, "VarMix_init", "USE_STANLEY_ISO");
  REFUSE(p->open_bcs, "VarMix_init", "open boundary conditions (OBC)");
  REFUSE(p->non_Boussinesq || !c->GV.Boussinesq, "VarMix_init", "non-Boussinesq mode (tv%SpV_avg, semi_Boussinesq)");
  REFUSE(p->debug, "VarMix_init", "DEBUG (the checksums of calc_slope_functions)");
  REQUIRE(!p->use_simpler_Eady_growth_rate || p->use_stored_slopes, MOM6X_EINVAL,
          "MOM_lateral_mixing_coeffs.F90, VarMix_init:When USE_SIMPLER_EADY_GROWTH_RATE=True, USE_STORED_SLOPES must also be True.");
  REQUIRE(p->VarMix_Ktop >= 2, MOM6X_EINVAL, "VarMix_init: VARMIX_KTOP must be at least 2");
  REQUIRE(!eos || eos_form_known(eos), MOM6X_EINVAL, "VarMix_init: unknown EQN_OF_STATE form");
  const bool slopes = p->calculate_Eady_growth_rate && p->use_stored_slopes;
  REQUIRE(!p->calculate_Eady_growth_rate || c->d.halo >= 2, MOM6X_EINVAL, "VarMix_init: calc_slope_functions needs a halo of two");
  REQUIRE(!p->calculate_Eady_growth_rate || (slopes && eos) || (Rlay && g_prime), MOM6X_EINVAL,
          "VarMix_init: GV%Rlay and GV%g_prime are needed without an equation of state");
  HIPCHK(hipSetDevice(c->device));
  varmix_free(c);
  VmState *s = new VmState();
  s->p = *p;
  s->use_eos = eos != nullptr;
  if (eos) s->eos = *eos;
  c->vm = s;
  const Dm d = c->d;
  if (const int rc = varmix_alloc(c, s, Rlay, g_prime)) { varmix_free(c); return rc; }   // (no state without its arrays)
  if (L2u || L2v) {
    const int nrows = d.slab / d.pitch;
    double L2;
    if (p->Visbeck_L_scale < 0) { const double t = p->L_to_m * p->Visbeck_L_scale; L2 = t * t; }
    else L2 = p->Visbeck_L_scale * p->Visbeck_L_scale;
    const dim3 b = blk2();
    KLAUNCH(c, "k_vm_L2", k_vm_L2, grid3(d.pitch, nrows, 1, b), b, d, c->G, L2, p->Visbeck_L_scale < 0 ? 1 : 0, nrows, L2u, L2v);
    HIPCHK(hipGetLastError());
  }
  return MOM6X_OK;
}

extern "C" int mom6x_calc_slope_functions(mom6x_ctx *c, const double *h, const double *T, const double *S, const double *p_surf,
                                          double dt, double *SN_u, double *SN_v, double *slope_x, double *slope_y, double *N2_u,
                                          double *N2_v, double *dzu, double *dzv, double *dzSxN, double *dzSyN, double *S2_u,
                                          double *S2_v) {
  REQUIRE(c && c->vm, MOM6X_EINVAL,
          "MOM_lateral_mixing_coeffs.F90, calc_slope_functions: Module must be initialized before it is used.");
  const VmState *s = c->vm;
  const mom6x_varmix_params &P = s->p;
  if (!P.calculate_Eady_growth_rate) return MOM6X_OK;   // :708
  REQUIRE(h, MOM6X_EINVAL, "calc_slope_functions: null array");
  REQUIRE(SN_u && SN_v, MOM6X_EINVAL, "calc_slope_function:%SN_u is not associated with use_variable_mixing.");
  const bool simpler = P.use_simpler_Eady_growth_rate != 0, stored = P.use_stored_slopes != 0;
  const bool slopes = simpler || stored, use_eos = slopes && s->use_eos;
  REQUIRE(!slopes || (slope_x && slope_y), MOM6X_EINVAL, "calc_slope_functions: slope_x and slope_y are needed with USE_STORED_SLOPES");
  REQUIRE(!use_eos || (T && S), MOM6X_EINVAL, "calc_slope_functions: an equation of state needs tv%T and tv%S");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const mom6x_vgrid &GV = c->GV;
  const int nz = d.nk;
  VmK K;
  K.h_neglect = GV.H_subroundoff; K.h_neglect2 = K.h_neglect * K.h_neglect; K.dz_neglect = GV.dZ_subroundoff;
  K.H_to_Z = P.H_to_Z;
  K.gH = P.g_Earth * P.H_to_RZ;                                 // MOM_isopycnal_slopes.F90:245
  K.Z_to_L = P.Z_to_L;
  K.G_Rho0 = P.g_Earth / P.Rho0;                                // :173
  K.kap_dt_x2 = (2.0 * (dt * P.kappa_smooth)) * P.Z_to_H_fill;  // :655 with kappa_dt = dt*CS%kappa_smooth (:711)
  K.h0 = K.h_neglect;                                           // :656: no larger_h_denom
  K.D_scale = P.Eady_GR_D_scale;
  if (K.D_scale <= 0.) K.D_scale = 64. * P.max_depth;           // :991
  K.r_crp_dist = 1. / ((P.cropping_distance > K.dz_neglect) ? P.cropping_distance : K.dz_neglect);   // :992
  K.crop = P.cropping_distance >= 0.;
  K.S2max = P.Visbeck_S_max * P.Visbeck_S_max;                  // :796
  { const double t = GV.H_subroundoff * GV.H_subroundoff; K.hsub4 = t * t; }
  K.H_cutoff = (double)(2 * nz) * (GV.Angstrom_H + K.h_neglect);   // :1159
  K.dZ_cutoff = (double)(2 * nz) * (P.Angstrom_Z + GV.dZ_subroundoff);
  K.h_min_N2 = P.h_min_N2;
  K.Ktop = P.VarMix_Ktop; K.use_dztot = P.full_depth_Eady_growth_rate;
  K.dRho_dT = s->eos.dRho_dT; K.dRho_dS = s->eos.dRho_dS;
  const size_t n3 = (size_t)nz * d.slab, n3p = n3 + d.slab;
  double *W = s->work, *e = W;
  W += n3p;
  double *pres = nullptr, *Tf = nullptr, *Sf = nullptr, *c1 = nullptr;
  if (slopes && s->use_eos) { pres = W; Tf = W + n3; Sf = W + 2 * n3; c1 = W + 3 * n3; W += 4 * n3; }
  const bool fill = use_eos && K.kap_dt_x2 > 0.0;               // else T_f = T_in (:661-665): read in place
  REQUIRE(!fill || nz >= 2, MOM6X_EINVAL, "calc_slope_functions: vert_fill_TS needs two layers");
  const dim3 b = blk2();
  KLAUNCH(c, "k_vm_cols", k_vm_cols, grid3(d.ni + 2 + IAL, d.nj + 4, 1, b), b, d, c->G, K, h, T, S, p_surf, e, use_eos ? pres : nullptr,
          fill ? Tf : nullptr, Sf, c1);
  if (!slopes) {
    KLAUNCH(c, "k_vm_just_e", k_vm_just_e, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, c->G, K, h, e, s->g_prime, SN_u, SN_v);
    HIPCHK(hipGetLastError());
    return MOM6X_OK;
  }
  const double *Tr = fill ? Tf : T, *Sr = fill ? Sf : S;
  VmDiag D;
  double *raw_u = nullptr, *raw_v = nullptr;
  if (simpler) {
    D.N2[0] = N2_u; D.N2[1] = N2_v; D.dz[0] = dzu; D.dz[1] = dzv; D.dzSN[0] = dzSxN; D.dzSN[1] = dzSyN;
    raw_u = W; raw_v = W + d.slab;
  } else {
    D.N2[0] = N2_u ? N2_u : W; D.N2[1] = N2_v ? N2_v : W + n3p;
    D.dz[0] = D.dz[1] = D.dzSN[0] = D.dzSN[1] = nullptr;
    // :798-799: CS%SN_u(:,:) = 0 ; CS%SN_v(:,:) = 0
    HIPCHK(hipMemsetAsync(SN_u, 0, (size_t)d.slab * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(SN_v, 0, (size_t)d.slab * sizeof(double), c->stream));
  }
  const dim3 g = grid3(d.ni + 1 + IAL, d.nj + 3, 2, b);
#define VMF(F)                                                                                                              \
  do {                                                                                                                      \
    if (simpler) KLAUNCH(c, "k_vm_faces<" #F ",1>", (k_vm_faces<F, 1>), g, b, d, c->G, K, h, e, pres, Tr, Sr, s->Rlay, slope_x, \
                         slope_y, D, raw_u, raw_v);                                                                         \
    else KLAUNCH(c, "k_vm_faces<" #F ",2>", (k_vm_faces<F, 2>), g, b, d, c->G, K, h, e, pres, Tr, Sr, s->Rlay, slope_x, slope_y, \
                 D, raw_u, raw_v);                                                                                          \
  } while (0)
  if (!use_eos) VMF(0);
  else EOS_FORM_DISPATCH(s->eos.form, VMF);
#undef VMF
  if (simpler) {
    KLAUNCH(c, "k_vm_eady_combine", k_vm_eady_combine, grid3(d.ni + 1 + IAL, d.nj + 2, 1, b), b, d, raw_u, raw_v, SN_u, SN_v);
  } else {
    KLAUNCH(c, "k_vm_visbeck", k_vm_visbeck, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, c->G, K, h, slope_x, slope_y, D.N2[0], D.N2[1],
            SN_u, SN_v, S2_u, S2_v);
  }
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
