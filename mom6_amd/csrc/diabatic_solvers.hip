// diabatic_solvers.hip -- the vertical tridiagonal solves of MOM_diabatic_aux and MOM_tracer_diabatic on gfx950.
//   triDiagTS, triDiagTS_Eulerian         <- src/parameterizations/vertical/MOM_diabatic_aux.F90:394-488
//   tracer_vertdiff(_Eulerian)            <- src/tracer/MOM_tracer_diabatic.F90:25-420
#include "mom6x_dev.h"

namespace {

// sfc_src / btm_src of tracer_vertdiff :89-113 (convert_flux_in: flux_scale = dt RZ_to_H; 0: the flux is a source already); none without the array
__device__ __forceinline__ double flux_src(const double *__restrict__ flux, size_t x, double flux_scale) {
  return !flux ? 0.0 : (flux_scale != 0.0) ? (flux[x] * flux_scale) : flux[x];
}

// One layer of the forward elimination of triDiagTS (:411-432) and tracer_vertdiff (tracer_diabatic.F90:151-176 with sinking, :189-209
// without) and one of the back substitution, for the two walking kernels (k_tridiag_cols keeps them written out: as calls the compiler
// schedules it otherwise): b1, d1 and the un-substituted tracer t are carried down the column.  The denominators come from the caller:
// triDiagTS, vertdiff and the sinking form sum them in three orders.  (Operands by reference: see ThomasFwd, vert_friction.hip.)
struct TriDiagFwd {
  double b1, d1, t;
  // denom: the first layer's whole denominator, dnum: the part of it that d1 keeps; src: tracer_vertdiff's surface source.  Returns t
  __device__ __forceinline__ double first(const double &denom, const double &dnum, const double &h_tr, const double &T0, bool src, const double &sfc_src) {
    b1 = 1.0 / denom; d1 = dnum * b1;
    t = (b1 * h_tr) * T0; if (src) t = t + b1 * sfc_src;
    return t;
  }
  // layers 2..nz; e: ea (with sinking: + sink(K)); btm: tracer_vertdiff's last layer, which takes the bottom source.  Returns c1(k)
  __device__ __forceinline__ double next(const double &b_denom_1, const double &eb_above, const double &eb, const double &h_tr, const double &Tk, const double &e, bool btm, const double &btm_src) {
    const double c1 = eb_above * b1;
    b1 = 1.0 / (b_denom_1 + eb); d1 = b_denom_1 * b1;
    t = b1 * (btm ? (h_tr * Tk + btm_src) + e * t : h_tr * Tk + e * t);
    return c1;
  }
  __device__ __forceinline__ double back(const double &Tk, const double &c1_below) { return t = Tk + c1_below * t; }
};

// triDiagTS :394-440 / triDiagTS_Eulerian :444-488 / tracer_vertdiff(_Eulerian) no-sink branch, one column per thread.
// vertdiff = 1 adds the land mask, ea(1) in the first denominator and the surface/bottom sources.
__global__ void __launch_bounds__(256)
k_tridiag(Dm d, const double *__restrict__ G, const double *__restrict__ hold, const double *__restrict__ ea,
          const double *__restrict__ eb, double *__restrict__ T, double *__restrict__ S, double *__restrict__ c1, double h_neglect,
          int vertdiff, const double *__restrict__ sfc_flux, const double *__restrict__ btm_flux, double flux_scale, int i0, int i1,
          int j0, int j1) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > i1 || j > j1) return;
  const int nz = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const bool two = (S != nullptr);   // triDiagTS solves for T and S with the same b1, c1, d1 (:411-438) -- one sweep for both
  double sfc_src = 0.0, btm_src = 0.0;
  if (vertdiff) {
    if (!(gm(G, d, MOM6X_G_mask2dT)[x] > 0.0)) return;
    sfc_src = flux_src(sfc_flux, x, flux_scale); btm_src = flux_src(btm_flux, x, flux_scale);
  }
  double h_tr = hold[x] + h_neglect;
  TriDiagFwd F; double prevS = 0.0;
  T[x] = F.first(vertdiff ? (h_tr + ea[x]) + eb[x] : h_tr + eb[x], h_tr, h_tr, T[x], vertdiff, sfc_src);
  if (two) { prevS = (F.b1 * h_tr) * S[x]; S[x] = prevS; }
  for (int k = 1; k < nz; k++) {
    const size_t c = x + (size_t)k * slab;
    h_tr = hold[c] + h_neglect;
    const double eak = ea[c];
    c1[c] = F.next(h_tr + F.d1 * eak, eb[c - slab], eb[c], h_tr, T[c], eak, vertdiff && k == nz - 1, btm_src);
    T[c] = F.t;
    if (two) { prevS = F.b1 * (h_tr * S[c] + eak * prevS); S[c] = prevS; }
  }
  for (int k = nz - 2; k >= 0; k--) {
    const size_t c = x + (size_t)k * slab;
    const double c1k = c1[c + slab];
    T[c] = F.back(T[c], c1k);
    if (two) { prevS = S[c] + c1k * prevS; S[c] = prevS; }
  }
}

// tracer_vertdiff with sink_rate :123-179 (and tracer_vertdiff_Eulerian's :315-380 with ea = ent(K), eb = ent(K+1)): one column per
// thread.  The limited sinking distances are a bottom-up recurrence and the solve runs top-down, so the first sweep leaves sink(K)
// and h_minus_dsink(k) in two scratch arrays (a tracer package's call, not on the benchmark's path: the plain form of k_tridiag).
__global__ void __launch_bounds__(256)
k_tridiag_sink(Dm d, const double *__restrict__ G, const double *__restrict__ hold, const double *__restrict__ ea,
               const double *__restrict__ eb, double *__restrict__ T, double *__restrict__ c1, double *__restrict__ snk, double *__restrict__ hmd,
               double h_neglect, const double *__restrict__ sfc_flux, const double *__restrict__ btm_flux, double flux_scale,
               double *__restrict__ btm_reservoir, double sink_dist, double H_to_RZ) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  const int nz = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  if (!(gm(G, d, MOM6X_G_mask2dT)[x] > 0.0)) return;      // (the reference forms sink on land too; nothing there reads it)
  const double sfc_src = flux_src(sfc_flux, x, flux_scale), btm_src = flux_src(btm_flux, x, flux_scale);
  // ---- sinking distances at the interfaces K = nz .. 1 (snk[k] <-> the top of layer k) :127-149
  double s_below = btm_reservoir ? sink_dist : 0.0;        // sink(nz+1)
  const double s_bottom = s_below;
  for (int k = nz - 1; k >= 1; k--) {
    const size_t c = x + (size_t)k * slab;
    const double h = hold[c];
    double sk, hm;
    if (btm_reservoir) { sk = sink_dist; hm = h; }
    else if (s_below >= sink_dist) { sk = sink_dist; hm = h + (s_below - sk); }
    else if (s_below + h < sink_dist) { sk = s_below + h; hm = 0.0; }
    else { sk = sink_dist; hm = (h + s_below) - sk; }
    snk[c] = sk; hmd[c] = hm;
    s_below = sk;
  }
  // ---- the solve :155-179
  const double b_denom_top = (hold[x] + s_below) + ea[x] + h_neglect;   // h_minus_dsink(1) = h_old(1) + sink(2)
  TriDiagFwd F;
  T[x] = F.first(b_denom_top + eb[x], b_denom_top, hold[x] + h_neglect, T[x], true, sfc_src);
  for (int k = 1; k < nz; k++) {
    const size_t c = x + (size_t)k * slab;
    const double es = ea[c] + snk[c];
    c1[c] = F.next(hmd[c] + F.d1 * es + h_neglect, eb[c - slab], eb[c], hold[c] + h_neglect, T[c], es, k == nz - 1, btm_src);
    T[c] = F.t;
  }
  if (btm_reservoir) btm_reservoir[x] = btm_reservoir[x] + (s_bottom * F.t) * H_to_RZ;
  for (int k = nz - 2; k >= 0; k--) {
    const size_t c = x + (size_t)k * slab;
    T[c] = F.back(T[c], c1[c + slab]);
  }
}

}  // namespace

// k_tridiag with the whole column on chip (the technique of k_vertvisc_cols, vert_friction.hip): c1 and the un-substituted T in
// registers, the un-substituted S of triDiagTS in LDS, one wavefront per work-group, inputs fetched TD_G layers ahead into a
// double buffer.  4 (5) words read and 1 (2) written per cell-layer instead of 9 (13); the same operations in the same order.
template <int NKT, bool TWO>   // (NKT: mom6x_dev.h NK_OF / NK_EXACT -- the layer count itself, or a bound on it)
__global__ void __launch_bounds__(64)
k_tridiag_cols(Dm d, const double *__restrict__ G, const double *__restrict__ hold, const double *__restrict__ ea,
               const double *__restrict__ eb, double *T, double *S, double h_neglect, int vertdiff,
               const double *__restrict__ sfc_flux, const double *__restrict__ btm_flux, double flux_scale, int i0, int i1, int j0,
               int j1) {
  constexpr int NK = NK_OF(NKT);
  const int nk = NK_EXACT(NKT) ? NK : d.nk;
  extern __shared__ double td_lds[];
  const int i = i0 + blockIdx.x * 64 + threadIdx.x;
  const int j = j0 + blockIdx.y;
  if (i > i1 || j > j1) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  double *ss = td_lds + threadIdx.x;
  double sfc_src = 0.0, btm_src = 0.0;
  if (vertdiff) {
    if (!(gm(G, d, MOM6X_G_mask2dT)[x] > 0.0)) return;
    sfc_src = flux_src(sfc_flux, x, flux_scale); btm_src = flux_src(btm_flux, x, flux_scale);
  }
  constexpr int TD_G = TWO ? 3 : 5, NG = (NK + TD_G - 1) / TD_G;
  double tt[NK], cc[NK];
  double q_h[2][TD_G], q_a[2][TD_G], q_b[2][TD_G], q_t[2][TD_G], q_s[2][TD_G];
  auto fetch = [&](int g, int b) {
#pragma unroll
    for (int m = 0; m < TD_G; m++) {
      const int k = g * TD_G + m;
      if (k < NK && k < nk) {
        const size_t c = x + (size_t)k * slab;
        q_h[b][m] = hold[c]; q_a[b][m] = ea[c]; q_b[b][m] = eb[c]; q_t[b][m] = T[c];
        if (TWO) q_s[b][m] = S[c];
      }
    }
  };
  double b1 = 0., d1 = 0., prev = 0., prevS = 0., eb_prev = 0.;
  fetch(0, 0);
#pragma unroll
  for (int g = 0; g < NG; g++) {
    if (g + 1 < NG) fetch(g + 1, (g + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < TD_G; m++) {
      const int k = g * TD_G + m;
      if (k < NK && k < nk) {
        const double h_tr = q_h[g & 1][m] + h_neglect, eak = q_a[g & 1][m], ebk = q_b[g & 1][m], Tk = q_t[g & 1][m];
        if (k == 0) {
          b1 = vertdiff ? 1.0 / ((h_tr + eak) + ebk) : 1.0 / (h_tr + ebk);
          d1 = h_tr * b1;
          prev = (b1 * h_tr) * Tk;
          if (vertdiff) prev = prev + b1 * sfc_src;
          if (TWO) prevS = (b1 * h_tr) * q_s[g & 1][m];
        } else {
          cc[k] = eb_prev * b1;
          const double b_denom_1 = h_tr + d1 * eak;
          b1 = 1.0 / (b_denom_1 + ebk);
          d1 = b_denom_1 * b1;
          if (vertdiff && k == nk - 1) prev = b1 * ((h_tr * Tk + btm_src) + eak * prev);
          else prev = b1 * (h_tr * Tk + eak * prev);
          if (TWO) prevS = b1 * (h_tr * q_s[g & 1][m] + eak * prevS);
        }
        eb_prev = ebk;
        tt[k] = prev;
        if (TWO) ss[k * 64] = prevS;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  T[x + (size_t)(nk - 1) * slab] = prev;
  if (TWO) S[x + (size_t)(nk - 1) * slab] = prevS;
  asm volatile("" ::: "memory");   // (S comes back from LDS, not from NK more live registers)
#pragma unroll
  for (int k = NK - 2; k >= 0; k--) {
    if (k >= nk - 1) continue;
    const size_t c = x + (size_t)k * slab;
    const double c1k = cc[k + 1];
    prev = tt[k] + c1k * prev;
    T[c] = prev;
    if (TWO) { prevS = ss[k * 64] + c1k * prevS; S[c] = prevS; }
    if (TWO && (k % 8) == 0) __builtin_amdgcn_sched_barrier(0);   // (or all 74 LDS reads are hoisted to the top: 150 registers)
  }
}

static int tridiag(mom6x_ctx *c, const double *hold, const double *ea, const double *eb, double *T, double *S, int vertdiff,
                   const double *sfc_flux, const double *btm_flux, double flux_scale, int is, int ie, int js, int je) {
  REQUIRE(c && hold && ea && eb && T, MOM6X_EINVAL, "tridiagonal solve: null array");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  double *c1; int rc;
  if ((rc = ctx_scratch(c, SCR_c1, d.nk, &c1))) return rc;
  static const bool walk = [] { const char *e = getenv("MOM6X_TRIDIAG"); return e && !strcmp(e, "walk"); }();
  if (d.nk <= COLS_NK_BOUND && !walk) {   // the layer counts the on-chip column kernel is built for
    const dim3 bc(64, 1, 1), gc((unsigned)((ie - is + 1 + 63) / 64), (unsigned)(je - js + 1), 1);
    // triDiagTS: T and S share the matrix (hold, ea, eb, and with them b1, d1, c1): ONE sweep for both, S's un-substituted values in
    // LDS -- 7 words per cell-layer instead of 10 (3.6 -> 3.1 ms per thermodynamic step at 1440 x 1080 x 75).  The instantiation with
    // a BOUND on the layer count serves 75 layers too: with the layer count itself the compiler schedules the fully unrolled,
    // branch-free column into 512 registers + 138 spilled; the uniform tests on the layer index keep its loads where they are.
    // (the profile label carries the template argument, so that a test can see which instantiation ran)
#define TDC(NKT, TWO) KLAUNCH_LDS(c, "k_tridiag_cols<" #NKT ">", (k_tridiag_cols<NKT, TWO>), gc, bc, TWO ? (size_t)NK_OF(NKT) * 64 * sizeof(double) : (size_t)0, \
                d, c->G, hold, ea, eb, T, S, c->GV.H_subroundoff, vertdiff, sfc_flux, btm_flux, flux_scale, is, ie, js, je)
#define TDC1(NKT) TDC(NKT, false)
    if (S) { if (d.nk <= 52) TDC(-52, true); else if (d.nk <= 66) TDC(-66, true); else TDC(-COLS_NK_BOUND, true); }
    else COLS_NK_DISPATCH(d.nk, TDC1);
#undef TDC1
#undef TDC
  } else {
    const dim3 b = blk2();
    KLAUNCH(c, "k_tridiag", k_tridiag, grid3(ie - is + 1, je - js + 1, 1, b), b, d, c->G, hold, ea, eb, T, S, c1, c->GV.H_subroundoff,
            vertdiff, sfc_flux, btm_flux, flux_scale, is, ie, js, je);
  }
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

// triDiagTS(G, GV, is, ie, js, je, hold, ea, eb, T, S)  diabatic_aux.F90:394 (one field per call; S = second call)
extern "C" int mom6x_triDiagTS(mom6x_ctx *c, int is, int ie, int js, int je, const double *hold, const double *ea,
                               const double *eb, double *T, double *S) {
  return tridiag(c, hold, ea, eb, T, S, 0, nullptr, nullptr, 0.0, is, ie, js, je);
}
// triDiagTS_Eulerian(G, GV, is, ie, js, je, hold, ent, T, S)  :444 ; ent has nk+1 interfaces
extern "C" int mom6x_triDiagTS_Eulerian(mom6x_ctx *c, int is, int ie, int js, int je, const double *hold, const double *ent,
                                        double *T, double *S) {
  REQUIRE(ent, MOM6X_EINVAL, "triDiagTS_Eulerian: null ent");
  return mom6x_triDiagTS(c, is, ie, js, je, hold, ent, ent + c->dims.slab, T, S);
}
// tracer_vertdiff(h_old, ea, eb, dt, tr, G, GV, sfc_flux, btm_flux, ..., convert_flux_in)  tracer_diabatic.F90:25
extern "C" int mom6x_tracer_vertdiff(mom6x_ctx *c, const double *h_old, const double *ea, const double *eb, double dt,
                                     double *tr, const double *sfc_flux, const double *btm_flux, int convert_flux) {
  if (c && c->dims.nk == 1) return MOM6X_OK;   // the reference warns and returns
  const double scale = convert_flux ? dt * c->GV.RZ_to_H : 0.0;
  return tridiag(c, h_old, ea, eb, tr, nullptr, 1, sfc_flux, btm_flux, scale, 0, c->dims.ni - 1, 0, c->dims.nj - 1);
}
extern "C" int mom6x_tracer_vertdiff_Eulerian(mom6x_ctx *c, const double *h_old, const double *ent, double dt, double *tr,
                                              const double *sfc_flux, const double *btm_flux, int convert_flux) {
  REQUIRE(ent, MOM6X_EINVAL, "tracer_vertdiff_Eulerian: null ent");
  return mom6x_tracer_vertdiff(c, h_old, ent, ent + c->dims.slab, dt, tr, sfc_flux, btm_flux, convert_flux);
}
// tracer_vertdiff(..., btm_reservoir, sink_rate, ...) with sink_rate present (:123-179); btm_reservoir may be null
extern "C" int mom6x_tracer_vertdiff_sink(mom6x_ctx *c, const double *h_old, const double *ea, const double *eb, double dt, double *tr,
                                          const double *sfc_flux, const double *btm_flux, double *btm_reservoir, double sink_rate,
                                          int convert_flux) {
  REQUIRE(c && h_old && ea && eb && tr, MOM6X_EINVAL, "tracer_vertdiff: null array");
  if (c->dims.nk == 1) return MOM6X_OK;   // the reference warns and returns
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  double *c1, *snk, *hmd; int rc;
  if ((rc = ctx_scratch(c, SCR_c1, d.nk, &c1)) || (rc = ctx_scratch(c, SCR_t0, d.nk, &snk)) || (rc = ctx_scratch(c, SCR_t1, d.nk, &hmd))) return rc;
  const double scale = convert_flux ? dt * c->GV.RZ_to_H : 0.0;
  const double sink_dist = (dt * sink_rate) * c->GV.Z_to_H;
  const dim3 b = blk2();
  KLAUNCH(c, "k_tridiag_sink", k_tridiag_sink, grid3(d.ni, d.nj, 1, b), b, d, c->G, h_old, ea, eb, tr, c1, snk, hmd, c->GV.H_subroundoff,
          sfc_flux, btm_flux, scale, btm_reservoir, sink_dist, c->GV.H_to_RZ);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
extern "C" int mom6x_tracer_vertdiff_Eulerian_sink(mom6x_ctx *c, const double *h_old, const double *ent, double dt, double *tr,
                                                   const double *sfc_flux, const double *btm_flux, double *btm_reservoir,
                                                   double sink_rate, int convert_flux) {
  REQUIRE(c && ent, MOM6X_EINVAL, "tracer_vertdiff_Eulerian: null ent");
  return mom6x_tracer_vertdiff_sink(c, h_old, ent, ent + c->dims.slab, dt, tr, sfc_flux, btm_flux, btm_reservoir, sink_rate, convert_flux);
}
// diabatic(u, v, h, tv, BLD, fluxes, visc, ADp, CDp, dt, Time_end, G, GV, US, CS, ...)  diabatic_driver.F90:277
// The dispatcher stays with the host.  With GV%ke == 1 it returns immediately (:330); otherwise set_BBL_TKE and set_diffusivity
// (set_diffusivity.hip, the ALE-coordinate path) give Kd_int on the device, the caller forms ea/eb or ent from it and calls the
// solvers above; kappa shear, the boundary layer schemes and tidal mixing are still the host's.
extern "C" int mom6x_diabatic_is_trivial(const mom6x_ctx *c) { return (c && c->dims.nk == 1) ? 1 : 0; }
