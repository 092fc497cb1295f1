// vert_friction.hip -- the vertical-viscosity coefficients and tridiagonal solves on gfx950.
//
//   vertvisc, vertvisc_remnant<- MOM_vert_friction.F90:557-1356
//   vertvisc_coef             <- MOM_vert_friction.F90:1357-1900, find_coupling_coef :2314-2560
//
// Vertical solves are one thread per column with sequential k (Thomas algorithm in the Schopf & Loughe
// form used by the reference), lane index = i (coalesced).
#include "mom6x_dev.h"

// vertvisc_CS and what visc hands it.  The setters (mom6x_vertvisc_set_visc, _set_coef, _set_direct_stress) may come before
// mom6x_vertvisc_init: whichever is first creates the state
struct VvState {
  mom6x_vertvisc_params P; bool init;                      // init: mom6x_vertvisc_init has run (vertvisc_coef is on the device)
  const double *a_u, *a_v, *h_u, *h_v, *Ray_u, *Ray_v;     // the coefficients in use: own_* below, or a host's (mom6x_vertvisc_set_coef)
  const double *Kv_bbl_u, *Kv_bbl_v, *bbl_thick_u, *bbl_thick_v, *Kv_shear;   // vertvisc_type inputs (caller-owned)
  double *own_a_u, *own_a_v, *own_h_u, *own_h_v;           // CS%a_u .. CS%h_v of mom6x_vertvisc_init, owned
  double ds_Hmix; const double *ds_h;                      // DIRECT_STRESS: HMIX_STRESS (0 = off) and the thicknesses of the public vertvisc
};
static VvState *vv_state(mom6x_ctx *c) {
  if (!c->vv) c->vv = new VvState();
  return c->vv;
}
void vertvisc_free(mom6x_ctx *c) {
  VvState *S = c->vv;
  if (!S) return;
  (void)hipFree(S->own_a_u); (void)hipFree(S->own_a_v); (void)hipFree(S->own_h_u); (void)hipFree(S->own_h_v);
  delete S;
  c->vv = nullptr;
}
bool vertvisc_ready(const mom6x_ctx *c) { return c->vv && c->vv->init; }
bool vertvisc_has_coef(const mom6x_ctx *c) { return c->vv && c->vv->a_u; }

namespace {

// DIRECT_STRESS (:707-720 / :958-971): the wind stress as a body force over the topmost HMIX_STRESS instead of a stress
// boundary condition.  The increment of layer k is added where the sweep picks the layer's velocity up.
struct DirectStress { double Hmix, I_Hmix, h_neglect; const double *h; };
struct DSWalk {
  bool on; double zDS, stress;
  __device__ __forceinline__ void start(const DirectStress &S, double dt_Rho0, double tau) { on = (S.Hmix > 0.0); zDS = 0.0; stress = dt_Rho0 * tau; }
  __device__ __forceinline__ double add(const DirectStress &S, double uk, size_t x3, int st) {
    if (!on) return uk;
    const double h_a = 0.5 * (S.h[x3] + S.h[x3 + st]) + S.h_neglect;
    double hfr = 1.0; if ((zDS + h_a) > S.Hmix) hfr = (S.Hmix - zDS) / h_a;
    uk = uk + S.I_Hmix * hfr * stress;
    zDS = zDS + h_a; if (zDS >= S.Hmix) on = false;
    return uk;
  }
};
// h: vertvisc's thickness argument (the RK2 step's), or null: what mom6x_vertvisc_set_direct_stress stored (the public vertvisc)
static DirectStress direct_stress_of(const mom6x_ctx *c, const double *h) {
  const double Hmix = c->vv->ds_Hmix;
  DirectStress S; S.Hmix = Hmix; S.I_Hmix = (Hmix > 0.0) ? 1.0 / Hmix : 0.0; S.h_neglect = c->GV.H_subroundoff;
  S.h = (Hmix > 0.0) ? (h ? h : c->vv->ds_h) : nullptr;
  return S;
}

// One layer of the forward elimination of vertvisc (:763-790 / :988-1015) and vertvisc_remnant (:1279-1298 / :1319-1338): b1 and d1
// are carried down the column, u (VEL) is the un-substituted velocity and r (REM) the un-substituted remnant of the layer just done.
// Shared by every kernel that walks the solve, so they cannot differ in arithmetic.  The on-chip kernels, which have no Rayleigh
// drag, pass the literal 0. for Ray: the sum with it is part of the bit pattern.
// (The operands come by reference: by value the compiler settles the order of the commutative operands inside these two functions
//  before it inlines them, and most kernels' instruction streams change -- same results, other registers.  This way every kernel keeps
//  its registers and occupancy, and the on-chip ones their instructions up to one exchanged pair of source operands.)
template <bool VEL, bool REM>
struct ThomasFwd {
  double b1, d1, u, r;
  __device__ __forceinline__ void first(const double &hu, const double &a_k, const double &a_kp, const double &Ray, const double &dt, const double &u0,
                                       const double &surface_stress) {
    const double b_denom_1 = hu + dt * (Ray + a_k);
    const double b = 1.0 / (b_denom_1 + dt * a_kp);
    b1 = b;
    d1 = b_denom_1 * b;
    if (VEL) u = b * (hu * u0 + surface_stress);
    if (REM) r = b * hu;
  }
  // layers 2..nz; returns c1(k)
  __device__ __forceinline__ double next(const double &hu, const double &a_k, const double &a_kp, const double &Ray, const double &dt, const double &u0) {
    const double c1 = dt * a_k * b1;
    const double b_denom_1 = hu + dt * (Ray + a_k * d1);
    b1 = 1.0 / (b_denom_1 + dt * a_kp);
    d1 = b_denom_1 * b1;
    if (VEL) u = (hu * u0 + dt * a_k * u) * b1;
    if (REM) r = (hu + dt * a_k * r) * b1;
    return c1;
  }
};

// ---------------------------------------------------------------------------------------------
// vertvisc_remnant :1229-1356 (one direction)
template <int DIR>
__global__ void __launch_bounds__(256)
k_vertvisc_remnant(Dm d, const double *__restrict__ G, double *__restrict__ vr, const double *__restrict__ a_u,
                   const double *__restrict__ h_u, const double *__restrict__ Ray_u, double *__restrict__ c1, double dt) {
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const int nz = d.nk;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  if (!(mC > 0.)) return;
  double Ray = Ray_u ? Ray_u[x] : 0.;
  double a_k = a_u[x], a_kp = a_u[x + slab];
  ThomasFwd<false, true> T;
  T.first(h_u[x], a_k, a_kp, Ray, dt, 0., 0.);
  vr[x] = T.r;
  for (int k = 1; k < nz; k++) {
    const size_t x3 = x + (size_t)k * slab;
    if (Ray_u) Ray = Ray_u[x3];
    a_k = a_kp; a_kp = a_u[x3 + slab];
    c1[x3] = T.next(h_u[x3], a_k, a_kp, Ray, dt, 0.);
    vr[x3] = T.r;
  }
  double prev = T.r;
  for (int k = nz - 2; k >= 0; k--) {
    const size_t x3 = x + (size_t)k * slab;
    prev = vr[x3] + c1[x3 + slab] * prev;
    vr[x3] = prev;
  }
}

// vertvisc_remnant with the column on chip (see k_vertvisc_cols): c1 and the un-substituted remnant stay in
// registers, 2 words read and 1 written per face-layer instead of 6.  No Ray_u (that goes through
// k_vertvisc_remnant); same operations in the same order.
// (NKT: mom6x_dev.h NK_OF / NK_EXACT -- the layer count itself, or a bound on it)
template <int DIR, int NKT>
__global__ void __launch_bounds__(64)
k_vertvisc_remnant_cols(Dm d, const double *__restrict__ G, double *__restrict__ vr, const double *__restrict__ a_u,
                        const double *__restrict__ h_u, double dt) {
  constexpr int NK = NK_OF(NKT);
  const int nk = NK_EXACT(NKT) ? NK : d.nk;
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * 64 + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  if (!(mC > 0.)) return;
  constexpr int VV_G = 8, NG = (NK + VV_G - 1) / VV_G;
  double rr[NK], cu[NK];
  double q_a[2][VV_G], q_h[2][VV_G];
  auto fetch = [&](int g, int b) {
#pragma unroll
    for (int m = 0; m < VV_G; m++) {
      const int k = g * VV_G + m;
      if (k < NK && k < nk) { const size_t x3 = x + (size_t)k * slab; q_a[b][m] = a_u[x3 + slab]; q_h[b][m] = h_u[x3]; }
    }
  };
  double a_kp = a_u[x];
  ThomasFwd<false, true> T = { 0., 0., 0., 0. };
  fetch(0, 0);
#pragma unroll
  for (int g = 0; g < NG; g++) {
    if (g + 1 < NG) fetch(g + 1, (g + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < VV_G; m++) {
      const int k = g * VV_G + m;
      if (k < NK && k < nk) {
        const double a_k = a_kp; a_kp = q_a[g & 1][m];
        const double hu = q_h[g & 1][m];
        if (k == 0) T.first(hu, a_k, a_kp, 0., dt, 0., 0.);
        else cu[k] = T.next(hu, a_k, a_kp, 0., dt, 0.);
        rr[k] = T.r;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  double prev = T.r;
  vr[x + (size_t)(nk - 1) * slab] = prev;
#pragma unroll
  for (int k = NK - 2; k >= 0; k--) {
    if (k >= nk - 1) continue;
    prev = rr[k] + cu[k + 1] * prev;
    vr[x + (size_t)k * slab] = prev;
  }
}

}  // namespace

// The velocity update of the RK2 step (:681-694 / :957-966), vertvisc (:557) and vertvisc_remnant (:1231)
// of one direction in ONE column sweep.  The three share the tridiagonal coefficients (b1, d1, c1 depend
// only on a, h, Ray and dt), so the fused kernel reads a_u and h_u once instead of twice, never writes
// and re-reads the un-diffused velocity, and keeps a single c1 array.  Each quantity goes through
// exactly the operations of the separate kernels, in the same order: results are bit-identical.
//   UPD: u_start = mask * (u_in + dtx * (u_bc + u_abt)) is formed on the fly (else u is updated in place)
//   REM: visc_rem is computed alongside (needs the same dt as the velocity solve)
template <int DIR, bool UPD, bool REM>
__global__ void __launch_bounds__(256)
k_vertvisc_fused(Dm d, const double *__restrict__ G, const double *u_in, const double *__restrict__ u_bc,
                 const double *__restrict__ u_abt, double dtx, double *u, double *__restrict__ vr,
                 const double *__restrict__ a_u, const double *__restrict__ h_u, const double *__restrict__ Ray_u,
                 const double *__restrict__ tau, double *__restrict__ c1, double dt, double dt_Rho0, double H_to_RZ,
                 double *__restrict__ tau_bot, DirectStress S) {
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const int nz = d.nk, st = DIR ? d.pitch : 1;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  if (mC > 0.) {
    const double surface_stress = (S.Hmix > 0.0) ? 0.0 : dt_Rho0 * (mC * tau[x]);
    DSWalk W; W.start(S, dt_Rho0, tau[x]);
    double Ray = Ray_u ? Ray_u[x] : 0.;
    double a_k = a_u[x], a_kp = a_u[x + slab];
    double hu = h_u[x];
    double u0 = UPD ? mC * (u_in[x] + dtx * (u_bc[x] + u_abt[x])) : u_in[x];
    u0 = W.add(S, u0, x, st);
    ThomasFwd<true, REM> T;
    T.first(hu, a_k, a_kp, Ray, dt, u0, surface_stress);
    u[x] = T.u;
    if (REM) vr[x] = T.r;
#pragma unroll 4
    for (int k = 1; k < nz; k++) {
      const size_t x3 = x + (size_t)k * slab;
      if (Ray_u) Ray = Ray_u[x3];
      a_k = a_kp; a_kp = a_u[x3 + slab];
      hu = h_u[x3];
      u0 = UPD ? mC * (u_in[x3] + dtx * (u_bc[x3] + u_abt[x3])) : u_in[x3];
      u0 = W.add(S, u0, x3, st);
      c1[x3] = T.next(hu, a_k, a_kp, Ray, dt, u0);
      u[x3] = T.u;
      if (REM) vr[x3] = T.r;
    }
    double uprev = T.u, rprev = REM ? T.r : 0.;
#pragma unroll 4
    for (int k = nz - 2; k >= 0; k--) {
      const size_t x3 = x + (size_t)k * slab;
      const double ck = c1[x3 + slab];
      uprev = u[x3] + ck * uprev;
      u[x3] = uprev;
      if (REM) { rprev = vr[x3] + ck * rprev; vr[x3] = rprev; }
    }
  } else if (UPD) {
    for (int k = 0; k < nz; k++) {
      const size_t x3 = x + (size_t)k * slab;
      u[x3] = mC * (u_in[x3] + dtx * (u_bc[x3] + u_abt[x3]));
    }
  }
  if (tau_bot) {
    double tb = H_to_RZ * (u[x + (size_t)(nz - 1) * slab] * a_u[x + (size_t)nz * slab]);
    if (Ray_u) for (int k = 0; k < nz; k++) tb = tb + H_to_RZ * (Ray_u[x + (size_t)k * slab] * u[x + (size_t)k * slab]);
    tau_bot[x] = tb;
  }
}

// k_vertvisc_fused with the whole column on chip: the forward sweep keeps c1 and the un-substituted velocity
// in registers (2*NK doubles; the 512-entry unified VGPR/AGPR file of a wave that runs alone on its SIMD)
// and the un-substituted remnant in LDS (NK*8 B per lane, lane-minor: conflict-free), so the backward sweep
// never goes back to HBM: 5 words read and 2 written per face-layer against 12.7 with the c1 / u / visc_rem
// round trips.  One wave per work-group; four work-groups (4 * 64 * NK * 8 B of LDS) fill a CU.  With one
// wave per SIMD nothing else hides the HBM latency, so the inputs are fetched VV_G layers ahead into a
// double buffer (3..5 * VV_G loads in flight per lane while the previous group is solved); the scheduling
// fences keep the compiler from hoisting every load of the unrolled column to the top (which spills).
// Same operations in the same order as k_vertvisc_fused: bit-identical.  Ray_u and the direct-stress
// option go through k_vertvisc_fused.
template <int DIR, bool UPD, bool REM, int NKT>
__global__ void __launch_bounds__(64)
k_vertvisc_cols(Dm d, const double *__restrict__ G, const double *u_in, const double *__restrict__ u_bc,
                const double *__restrict__ u_abt, double dtx, double *u, double *__restrict__ vr,
                const double *__restrict__ a_u, const double *__restrict__ h_u,
                const double *__restrict__ tau, double dt, double dt_Rho0, double H_to_RZ,
                double *__restrict__ tau_bot) {
  constexpr int NK = NK_OF(NKT);
  const int nk = NK_EXACT(NKT) ? NK : d.nk;
  extern __shared__ double vv_lds[];
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * 64 + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab;
  double *rr = vv_lds + threadIdx.x;
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  constexpr int VV_G = UPD ? 4 : 6;
  constexpr int NG = (NK + VV_G - 1) / VV_G;
  double uu[NK], cu[NK];
  double q_a[2][VV_G], q_h[2][VV_G], q_u[2][VV_G], q_b[2][VV_G], q_t[2][VV_G];
  auto fetch = [&](int g, int b) {
#pragma unroll
    for (int m = 0; m < VV_G; m++) {
      const int k = g * VV_G + m;
      if (k < NK && k < nk) {
        const size_t x3 = x + (size_t)k * slab;
        q_a[b][m] = a_u[x3 + slab];
        q_h[b][m] = h_u[x3];
        q_u[b][m] = u_in[x3];
        if (UPD) { q_b[b][m] = u_bc[x3]; q_t[b][m] = u_abt[x3]; }
      }
    }
  };
  if (mC > 0.) {
    const double surface_stress = dt_Rho0 * (mC * tau[x]);
    double a_kp = a_u[x];
    ThomasFwd<true, REM> T = { 0., 0., 0., 0. };
    fetch(0, 0);
#pragma unroll
    for (int g = 0; g < NG; g++) {
      if (g + 1 < NG) fetch(g + 1, (g + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < VV_G; m++) {
        const int k = g * VV_G + m;
        if (k < NK && k < nk) {
          const double a_k = a_kp; a_kp = q_a[g & 1][m];
          const double hu = q_h[g & 1][m];
          const double u0 = UPD ? mC * (q_u[g & 1][m] + dtx * (q_b[g & 1][m] + q_t[g & 1][m])) : q_u[g & 1][m];
          if (k == 0) T.first(hu, a_k, a_kp, 0., dt, u0, surface_stress);
          else cu[k] = T.next(hu, a_k, a_kp, 0., dt, u0);
          uu[k] = T.u;
          if (REM) rr[k * 64] = T.r;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    double uprev = T.u, rprev = T.r;
    u[x + (size_t)(nk - 1) * slab] = uprev;
    if (REM) vr[x + (size_t)(nk - 1) * slab] = rprev;
    const double u_bottom = uprev;   // (uu[nk - 1])
    asm volatile("" ::: "memory");   // the remnant comes back from LDS, not from 75 more live registers
#pragma unroll
    for (int k = NK - 2; k >= 0; k--) {
      if (k >= nk - 1) continue;
      const size_t x3 = x + (size_t)k * slab;
      const double ck = cu[k + 1];
      uprev = uu[k] + ck * uprev;
      u[x3] = uprev;
      if (REM) { rprev = rr[k * 64] + ck * rprev; vr[x3] = rprev; }
    }
    if (tau_bot) tau_bot[x] = H_to_RZ * (u_bottom * a_kp);
  } else {
    if (UPD) {
      for (int k = 0; k < nk; k++) {
        const size_t x3 = x + (size_t)k * slab;
        u[x3] = mC * (u_in[x3] + dtx * (u_bc[x3] + u_abt[x3]));
      }
    }
    if (tau_bot) tau_bot[x] = H_to_RZ * (u[x + (size_t)(nk - 1) * slab] * a_u[x + (size_t)nk * slab]);
  }
}

// MOM6X_VERTVISC, read once per process: `walk` keeps every solve on the kernels that walk the column through HBM, `pair` keeps the
// on-chip solve but not the one-kernel form of coefficients + solve (k_vertvisc_coef_cols); anything else: the default.
enum VertviscForm { VV_DEFAULT, VV_PAIR, VV_WALK };
static VertviscForm vertvisc_form() {
  static const VertviscForm form = [] {
    const char *e = getenv("MOM6X_VERTVISC");
    return (e && !strcmp(e, "walk")) ? VV_WALK : ((e && !strcmp(e, "pair")) ? VV_PAIR : VV_DEFAULT);
  }();
  return form;
}

// The coefficient walk compiled for the common switch set (CoefWalk::layer<true>) where a run's constants allow it, the general one
// otherwise.  MOM6X_VV_WALK=general, read once per process: always the general one (tests/test_vertvisc_walk_gpu.py).
static bool vertvisc_walk_lean(const mom6x_vertvisc_params &P, const mom6x_vgrid &GV) {
  static const bool general_env = [] { const char *e = getenv("MOM6X_VV_WALK"); return e && !strcmp(e, "general"); }();
  return !general_env && !P.harmonic_visc && P.bottomdraglaw && P.harm_BL_val == 0.0 && !(P.Kvml_invZ2 > 0.0) && GV.H_to_Z == 1.0 &&
         GV.dZ_subroundoff == GV.H_subroundoff;
}

// The layer counts the on-chip column kernels are built for (anything deeper walks through HBM): 75 as such (the headline's), any
// other count up to the bound with uniform tests on the layer index (mom6x_dev.h COLS_NK_BOUND, COLS_NK_DISPATCH).
static bool vertvisc_cols_usable(int nk, const double *Ray, const DirectStress &S) {
  return vertvisc_form() != VV_WALK && nk <= COLS_NK_BOUND && !Ray && !(S.Hmix > 0.0);
}

template <int DIR, bool UPD, bool REM>
static void launch_vertvisc_fused(mom6x_ctx *c, const double *u_in, const double *u_bc, const double *u_abt, double dtx, double *u,
                                  double *vr, const double *a, const double *h, const double *Ray, const double *tau, double *c1,
                                  double dt, double *tau_bot, const double *h_ds) {
  const Dm d = c->d;
  const double dt_Rho0 = dt / c->GV.H_to_RZ, HR = c->GV.H_to_RZ;
  const DirectStress S = direct_stress_of(c, h_ds);
  if (vertvisc_cols_usable(d.nk, Ray, S)) {
    const dim3 bc(64, 1, 1);
    const dim3 gc((unsigned)(((DIR ? d.ni : nxa(d.ni + 1, -1)) + 63) / 64), (unsigned)(DIR ? d.nj + 1 : d.nj), 1);
#define VVC(NKT) KLAUNCH_LDS(c, DIR ? "k_vertvisc_cols<1>" : "k_vertvisc_cols<0>", (k_vertvisc_cols<DIR, UPD, REM, NKT>), gc, bc,           \
                             (REM ? (size_t)NK_OF(NKT) * 64 * sizeof(double) : (size_t)0), d, c->G, u_in, u_bc, u_abt, dtx, u, vr, a, h, tau, \
                             dt, dt_Rho0, HR, tau_bot)
    COLS_NK_DISPATCH(d.nk, VVC);
#undef VVC
    return;
  }
  const dim3 b = blk2();
  const dim3 g = DIR ? grid3(d.ni, d.nj + 1, 1, b) : grid3(nxa(d.ni + 1, -1), d.nj, 1, b);
  KLAUNCH(c, DIR ? "k_vertvisc_fused<1>" : "k_vertvisc_fused<0>", (k_vertvisc_fused<DIR, UPD, REM>), g, b, d, c->G, u_in, u_bc, u_abt, dtx,
          u, vr, a, h, Ray, tau, c1, dt, dt_Rho0, HR, tau_bot, S);
}

// [u = mask*(u_in + dtx*(u_bc + u_abt));] vertvisc(u, dt); [vertvisc_remnant(vr, dt)] -- see k_vertvisc_fused.
// u_bc == nullptr: no velocity update (u_in is ignored, u is updated in place); vr_u == nullptr: no remnant.
template <bool UPD, bool REM>
static int vertvisc_fused_as(mom6x_ctx *c, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                             const double *u_abt, const double *v_abt, double dtx, double *u, double *v, const double *taux,
                             const double *tauy, double dt, double *taux_bot, double *tauy_bot, double *vr_u, double *vr_v,
                             const double *h) {
  REQUIRE(c && vertvisc_has_coef(c), MOM6X_EINVAL, "MOM_vert_friction(visc): Module must be initialized before it is used.");
  HIPCHK(hipSetDevice(c->device));
  const VvState &S = *c->vv;
  double *c1;
  int rc;
  if ((rc = ctx_scratch(c, SCR_c1, c->d.nk, &c1))) return rc;
  launch_vertvisc_fused<0, UPD, REM>(c, UPD ? u_in : u, u_bc, u_abt, dtx, u, vr_u, S.a_u, S.h_u, S.Ray_u, taux, c1, dt, taux_bot, h);
  launch_vertvisc_fused<1, UPD, REM>(c, UPD ? v_in : v, v_bc, v_abt, dtx, v, vr_v, S.a_v, S.h_v, S.Ray_v, tauy, c1, dt, tauy_bot, h);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
int vertvisc_fused(mom6x_ctx *c, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                   const double *u_abt, const double *v_abt, double dtx, double *u, double *v, const double *taux,
                   const double *tauy, double dt, double *taux_bot, double *tauy_bot, double *vr_u, double *vr_v, const double *h) {
  const bool upd = (u_bc != nullptr), rem = (vr_u != nullptr);
  auto *f = upd ? (rem ? vertvisc_fused_as<true, true> : vertvisc_fused_as<true, false>)
                : (rem ? vertvisc_fused_as<false, true> : vertvisc_fused_as<false, false>);
  return f(c, u_in, v_in, u_bc, v_bc, u_abt, v_abt, dtx, u, v, taux, tauy, dt, taux_bot, tauy_bot, vr_u, vr_v, h);
}

// One layer of the bottom-up walk of vertvisc_coef :1357 + find_coupling_coef :2314 (see k_vertvisc_coef): the thickness at the velocity
// point (CS%h_u) of layer K-1 (0-based k = K-1) and the coupling coefficient (CS%a_u) of the interface K below it, from the two cells'
// thicknesses, the velocity the upwinding looks at, and what the walk carries up from the bottom.  Shared by k_vertvisc_coef and
// k_vertvisc_coef_cols, so the two cannot differ in arithmetic.
struct CoefWalk {
  mom6x_vertvisc_params CS;
  double I_Hbbl, I_valBL, kv_bbl, bbl_thick, hn, H_to_Z, h_neglect, dz_neglect, a_cpl_max, I_amax, Dmin;
  double zh, zcol0, zcol1, z_i_below, dz_vel_below;
  __device__ __forceinline__ void init(const mom6x_vertvisc_params &CS_, double bathy0, double bathy1, double I_Hbbl_, double I_valBL_, double kv_bbl_,
                                       double bbl_thick_, double hn_, double H_to_Z_, double h_neglect_, double dz_neglect_, double a_cpl_max_,
                                       double I_amax_) {
    CS = CS_; I_Hbbl = I_Hbbl_; I_valBL = I_valBL_; kv_bbl = kv_bbl_; bbl_thick = bbl_thick_; hn = hn_; H_to_Z = H_to_Z_;
    h_neglect = h_neglect_; dz_neglect = dz_neglect_; a_cpl_max = a_cpl_max_; I_amax = I_amax_;
    Dmin = dmin(bathy0, bathy1);
    zh = 0.; zcol0 = -bathy0; zcol1 = -bathy1;
    z_i_below = 0.;          // z_i(k+1): the interface below the layer being worked on
    dz_vel_below = 0.;       // dz_vel(k+1)
    botfn_below = 1.;        // botfn(0): the bottom interface's coupling has its own expression and does not read it
  }
  // LEAN (vertvisc_walk_lean): harmonic_visc off, bottomdraglaw on, harm_BL_val == 0, no KV_ML_INVZ2, H_to_Z == 1 and dz_neglect ==
  // h_neglect, all constants of a run.  Then dz IS h (1.0 * h and the same neglect: dz_harm, dz_arith and the blend dz_vel are h_harm,
  // h_arith and hvel in every bit), and in the upwinding arm z2_wt is exactly 1 (zh * I_Hbbl < 2 * 0 only where zh * I_Hbbl < 0 already
  // chose h_harm), so its z2 = 1.0 * (dmax(zh, z_clear) * I_Hbbl) is this layer's z_i_top: the operand the coupling of the layer above
  // reads as z_i_below.  One botfn per layer, carried up, serves both sites; three divisions per layer where the general form has five.
  double botfn_below;        // LEAN: botfn(z_i(k+1))
  template <bool LEAN>
  __device__ __forceinline__ void layer(int K, int nz, double h0, double h1, double uk, double z_t, bool have_Kv_add, double Kv_add,
                                        double &h_u_out, double &a_out) {
    if (LEAN) {
      const double h_harm = 2. * h0 * h1 / (h0 + h1 + h_neglect);
      const double h_arith = 0.5 * (h1 + h0);
      const double h_delta = h1 - h0;
      zcol0 = zcol0 + h0; zcol1 = zcol1 + h1;
      zh = zh + h_harm;
      const double z_clear = dmax(zcol0, zcol1) + Dmin;
      const double z2 = dmax(zh, z_clear) * I_Hbbl;                // z_i_top
      const double botfn_top = 1. / (1. + 0.09 * z2 * z2 * z2 * z2 * z2 * z2);
      double hvel = h_arith;
      if (uk * h_delta > 0.) {
        if (zh * I_Hbbl < 0.) hvel = h_harm;                       // (negative thicknesses: as the general form has them)
        else hvel = (1. - botfn_top) * h_arith + botfn_top * h_harm;
      }
      h_u_out = hvel + h_neglect;
      double a_cpl;
      if (K == nz) {
        const double dhc = hvel * 0.5;
        a_cpl = kv_bbl / ((dmin(dhc, bbl_thick) + hn) + I_amax * kv_bbl);
      } else {
        double Kv_tot = CS.Kv;
        if (have_Kv_add) Kv_tot = Kv_tot + Kv_add;
        const double botfn = botfn_below;
        Kv_tot = Kv_tot + (kv_bbl - CS.Kv) * botfn;
        const double dhc = 0.5 * (dz_vel_below + hvel);
        double h_shear;
        if (dhc > bbl_thick) h_shear = ((1. - botfn) * dhc + botfn * bbl_thick) + hn;
        else h_shear = dhc + hn;
        a_cpl = Kv_tot / (h_shear + (I_amax * Kv_tot));
      }
      a_out = dmin(a_cpl_max, a_cpl);
      botfn_below = botfn_top; dz_vel_below = hvel;
      return;
    }
    const double dz0 = H_to_Z * h0, dz1 = H_to_Z * h1;
    const double h_harm = 2. * h0 * h1 / (h0 + h1 + h_neglect);
    const double h_arith = 0.5 * (h1 + h0);
    const double h_delta = h1 - h0;
    const double dz_harm = 2. * dz0 * dz1 / (dz0 + dz1 + dz_neglect);
    const double dz_arith = 0.5 * (dz1 + dz0);
    double hvel, dz_vel, z_i_top;
    if (CS.harmonic_visc) {
      hvel = h_harm; dz_vel = dz_harm;
      if (uk * h_delta < 0) {
        const double z2 = z_i_below;
        const double botfn = 1. / (1. + 0.09 * z2 * z2 * z2 * z2 * z2 * z2);
        hvel = (1. - botfn) * h_harm + botfn * h_arith;
        dz_vel = (1. - botfn) * dz_harm + botfn * dz_arith;
      }
      z_i_top = z_i_below + dz_harm * I_Hbbl;
    } else {
      zcol0 = zcol0 + dz0; zcol1 = zcol1 + dz1;
      zh = zh + dz_harm;
      const double z_clear = dmax(zcol0, zcol1) + Dmin;
      z_i_top = dmax(zh, z_clear) * I_Hbbl;
      hvel = h_arith; dz_vel = dz_arith;
      if (uk * h_delta > 0.) {
        if (zh * I_Hbbl < CS.harm_BL_val) {
          hvel = h_harm; dz_vel = dz_harm;
        } else {
          double z2_wt = 1.;
          if (zh * I_Hbbl < 2. * CS.harm_BL_val) z2_wt = dmax(0., dmin(1., zh * I_Hbbl * I_valBL - 1.));
          const double z2 = z2_wt * (dmax(zh, z_clear) * I_Hbbl);
          const double botfn = 1. / (1. + 0.09 * z2 * z2 * z2 * z2 * z2 * z2);
          hvel = (1. - botfn) * h_arith + botfn * h_harm;
          dz_vel = (1. - botfn) * dz_arith + botfn * dz_harm;
        }
      }
    }
    h_u_out = hvel + h_neglect;                                    // CS%h_u :1868-1872
    double a_cpl;
    if (K == nz) {                                                 // :2543-2558
      if (CS.bottomdraglaw) {
        const double dhc = dz_vel * 0.5;
        a_cpl = kv_bbl / ((dmin(dhc, bbl_thick) + hn) + I_amax * kv_bbl);
      } else if (fabs(CS.Kv_extra_bbl) > 0.0) {
        a_cpl = (CS.Kv + CS.Kv_extra_bbl) / ((0.5 * dz_vel + hn) + I_amax * (CS.Kv + CS.Kv_extra_bbl));
      } else {
        a_cpl = CS.Kv / ((0.5 * dz_vel + hn) + I_amax * CS.Kv);
      }
    } else {                                                       // :2418-2540, Fortran K+1 between layers k and k+1
      double Kv_tot = CS.Kv;
      if (CS.Kvml_invZ2 > 0.) Kv_tot = CS.Kv + CS.Kvml_invZ2 / ((z_t * z_t) * (1. + 0.09 * z_t * z_t * z_t * z_t * z_t * z_t));
      if (have_Kv_add) Kv_tot = Kv_tot + Kv_add;
      if (CS.bottomdraglaw) {
        const double z2 = z_i_below;
        const double botfn = 1. / (1. + 0.09 * z2 * z2 * z2 * z2 * z2 * z2);
        Kv_tot = Kv_tot + (kv_bbl - CS.Kv) * botfn;
        const double dhc = 0.5 * (dz_vel_below + dz_vel);
        double h_shear;
        if (dhc > bbl_thick) h_shear = ((1. - botfn) * dhc + botfn * bbl_thick) + hn;
        else h_shear = dhc + hn;
        a_cpl = Kv_tot / (h_shear + (I_amax * Kv_tot));
      } else if (fabs(CS.Kv_extra_bbl) > 0.0) {
        const double z2 = z_i_below;
        const double botfn = 1. / (1. + 0.09 * z2 * z2 * z2 * z2 * z2 * z2);
        Kv_tot = Kv_tot + CS.Kv_extra_bbl * botfn;
        const double h_shear = 0.5 * (dz_vel_below + dz_vel + hn);
        a_cpl = Kv_tot / (h_shear + I_amax * Kv_tot);
      } else {
        const double h_shear = 0.5 * (dz_vel_below + dz_vel + hn);
        a_cpl = Kv_tot / (h_shear + I_amax * Kv_tot);
      }
    }
    a_out = dmin(a_cpl_max, a_cpl);                                // CS%a_u :1863-1867
    z_i_below = z_i_top; dz_vel_below = dz_vel;
  }
};

// ---------------------------------------------------------------------------------------------
// vertvisc_coef :1357 + find_coupling_coef :2314 for one direction: one thread per face column.
// Everything the coupling coefficient of interface K needs (z_i(K), dz_vel of the layers above and below) is
// available while the column is walked bottom-up, so a_cpl is formed in the same sweep and no 3-D temporaries
// (hvel, dz_vel, dz_harm, z_i, a_cpl of the reference) exist.  The only top-down quantity is the mixed-layer
// coordinate z_t of KV_ML_INVZ2 (:2420-2436): when that option is on, a first top-down walk leaves z_t(K) in
// the a array, where the main sweep picks it up before overwriting it.
// dz = H_to_Z*h (thickness_to_dz, MOM_interface_heights.F90:892).
// MODE selects the velocity the upwinding looks at: 0: u as given; 1: the predictor estimate of :591-598,
// mask*(u + dtx*u_bc); 2: that of :681-694 / :957-966, mask*(u + dtx*(u_bc + u_abt)) -- formed on the fly with the
// reference's expression, so the step never has to write and re-read up/vp just for this routine.
template <int DIR, int MODE, bool LEAN>
__global__ void __launch_bounds__(256)
k_vertvisc_coef(Dm d, const double *__restrict__ G, mom6x_vertvisc_params CS, const double *u, double *u_out,
                const double *__restrict__ u_bc, const double *__restrict__ u_abt, double dtx,
                const double *__restrict__ h, const double *__restrict__ Kv_bbl, const double *__restrict__ bbl_thick_in,
                const double *__restrict__ Kv_shear, double *__restrict__ a_out, double *__restrict__ h_out, double H_to_Z,
                double h_neglect, double dz_neglect, double a_cpl_max, double I_amax, LayerAccelSrc LA) {
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const int nz = d.nk, st = DIR ? d.pitch : 1;
  const size_t x = ix2(d, i, j), y = x + st, slab = (size_t)d.slab;
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  // MODE 3: accel_layer_u of btstep_layer_accel (MOM_barotropic.F90:3432-3504) formed here from pbce and the barotropic solver's
  // 2-D results (the expression of k_layer_accel, barotropic.hip) instead of being read as u_abt
  double la_e0 = 0., la_e1 = 0., la_g0 = 0., la_g1 = 0., la_a = 0., la_Idx = 0.;
  if (MODE == 3) {
    la_e0 = LA.e_anom[x]; la_e1 = LA.e_anom[y]; la_g0 = LA.g_own[x]; la_g1 = LA.g_nbr[y]; la_a = LA.a2d[x];
    la_Idx = gm(G, d, DIR ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  }
  auto abt = [&](size_t c) -> double {
    if (MODE != 3) return u_abt[c];
    double a = (la_a - (((LA.pbce[c + st] - la_g1) * la_e1) - ((LA.pbce[c] - la_g0) * la_e0)) * la_Idx);
    if (fabs(a) < LA.underflow) a = 0.0;
    return a;
  };
  if (!(mC > 0.)) {   // do_i :1514-1516
    if (u_out && MODE >= 2)   // (the velocity estimate the solve that follows starts from, see below: masked faces too)
      for (int k = 0; k < nz; k++) { const size_t c = x + (size_t)k * slab; u_out[c] = mC * (u[c] + dtx * (u_bc[c] + abt(c))); }
    return;
  }
  const double *bathyT = gm(G, d, MOM6X_G_bathyT);
  double I_valBL = 0.0; if (CS.harm_BL_val > 0.0) I_valBL = 1.0 / CS.harm_BL_val;
  double I_Hbbl = 1. / (CS.Hbbl + dz_neglect), kv_bbl = 0.0, bbl_thick = 0.0;
  if (CS.bottomdraglaw) {
    kv_bbl = Kv_bbl[x];
    bbl_thick = bbl_thick_in[x] + dz_neglect;
    I_Hbbl = 1. / bbl_thick;
  }
  const double hn = dz_neglect;   // h_neglect of find_coupling_coef :2390
  if (CS.Kvml_invZ2 > 0.) {       // z_t(K), K = 2..nz, top-down
    const double I_Hmix = 1. / (CS.Hmix + hn);
    double z_t = hn * I_Hmix;
    for (int K = 1; K < nz; K++) {
      const double dz0 = H_to_Z * h[x + (size_t)(K - 1) * slab], dz1 = H_to_Z * h[y + (size_t)(K - 1) * slab];
      z_t = z_t + (2. * dz0 * dz1 / (dz0 + dz1 + dz_neglect)) * I_Hmix;
      a_out[x + (size_t)K * slab] = z_t;
    }
  }
  CoefWalk W;
  W.init(CS, bathyT[x], bathyT[y], I_Hbbl, I_valBL, kv_bbl, bbl_thick, hn, H_to_Z, h_neglect, dz_neglect, a_cpl_max, I_amax);
  for (int k = nz - 1; k >= 0; k--) {
    const size_t c = x + (size_t)k * slab;
    const double h0 = h[c], h1 = h[c + st];
    double uk = u[c];
    if (MODE == 1) uk = mC * (uk + dtx * u_bc[c]);
    if (MODE >= 2) {
      uk = mC * (uk + dtx * (u_bc[c] + abt(c)));
      // u_out: this IS the velocity the RK2 step hands to vertvisc next (:681-694 / :957-966); written here, the solve reads one
      // array instead of three (u_out may be u itself: every thread reads and writes its own column only)
      if (u_out) u_out[c] = uk;
    }
    const int K = k + 1;   // the interface below this layer (bottom: K = nz)
    double z_t = 0.0, Kv_add = 0.0;
    if (K < nz) {
      if (CS.Kvml_invZ2 > 0.) z_t = a_out[x + (size_t)K * slab];
      if (Kv_shear) Kv_add = 0.5 * (Kv_shear[x + (size_t)K * slab] + Kv_shear[y + (size_t)K * slab]);
    }
    double hu, a;
    W.layer<LEAN>(K, nz, h0, h1, uk, z_t, Kv_shear != nullptr, Kv_add, hu, a);
    h_out[c] = hu;                                                 // CS%h_u :1868-1872
    a_out[x + (size_t)K * slab] = a;                               // CS%a_u :1863-1867
  }
  a_out[x] = dmin(a_cpl_max, 0.0);   // a_cpl(:,:,1) stays 0 without shelves / dynamic mixed-layer viscosity
}

#ifndef CC_GROUP
#define CC_GROUP 5
#endif
#ifndef CC_GROUP1
#define CC_GROUP1 8   // (MODE 1 holds no pbce pair and no velocity: 8 layers ahead, 1.53-1.58 against 1.60-1.62 ms per launch on average; profiles/r05_ab_vv.txt)
#endif
#ifndef CC_UG
#define CC_UG 8
#endif
// k_vertvisc_coef_cols, pass 1: the coefficients of the pair P of layer groups (2P and 2P+1, G layers each, counted from the bottom) go
// to their registers -- every index a constant.
template <int NK, int G, int P>
__device__ __forceinline__ void cc_file(double (&aa)[NK + 1], const double (&t_a)[2][G]) {
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int m = 0; m < G; m++) {
      const int k = NK - 1 - ((2 * P + b) * G + m);
      if (k >= 0) aa[k + 1] = t_a[b][m];
    }
}
template <int NK, int G>
__device__ __forceinline__ void cc_file_switch(int p, double (&aa)[NK + 1], const double (&t_a)[2][G]) {
  static_assert((NK + G - 1) / G <= 40, "cc_file_switch: at most 20 pairs of groups");
  switch (p) {
#define CC_CASE(P) case P: cc_file<NK, G, P>(aa, t_a); break;
    CC_CASE(0) CC_CASE(1) CC_CASE(2) CC_CASE(3) CC_CASE(4) CC_CASE(5) CC_CASE(6) CC_CASE(7) CC_CASE(8) CC_CASE(9)
    CC_CASE(10) CC_CASE(11) CC_CASE(12) CC_CASE(13) CC_CASE(14) CC_CASE(15) CC_CASE(16) CC_CASE(17) CC_CASE(18) CC_CASE(19)
#undef CC_CASE
    default: break;
  }
}

// vertvisc_coef + vertvisc [+ vertvisc_remnant] (MODE 3: :737-767 and :1002-1022 of the RK2 step) or vertvisc_coef + vertvisc_remnant
// (MODE 1: :602-610) in ONE kernel per direction.  k_vertvisc_coef writes a_u (NK+1 levels) and h_u for k_vertvisc_cols /
// k_vertvisc_remnant_cols to read straight back.  The coefficients are a bottom-up recurrence (z_i counts from the bottom) and the Thomas
// sweep runs top-down, so the column of coefficients has to wait on chip: a_u in registers, h_u in LDS -- and as the forward sweep consumes
// them it puts c1 into a_u's registers and the un-substituted remnant into h_u's LDS words, so the kernel holds what k_vertvisc_cols holds
// (2 NK doubles in the 512-entry register file of a wave alone on its SIMD, NK in LDS).
//   pass 1 (bottom-up): velocity estimate, h_u, a_u, the inputs fetched CC_G layers ahead.  The walk is a LOOP over pairs of groups (75
//     copies of the layer's ~300 instructions would not fit the instruction cache), but a_u can only live in registers if every index
//     is a constant: each pair leaves its coefficients in temporaries and a switch over the pair's number files them (cc_file<P>).
//     The velocity estimate goes to its place in the result array and comes back in pass 2 (150 more registers would spill:
//     measured, 2.1 against 1.75 ms); u may be u_in: a layer's inputs are read before its estimate is written.
//   pass 2 / 3: k_vertvisc_cols's sweeps from the chip.
// WRITE_COEF: a_u and h_u are also written (CS%a_u, CS%h_u stay what the step's LAST vertvisc_coef made them; the coefficients of the
// earlier stages are replaced before anybody can look, unless a vertvisc_remnant of their own follows).
// Words per face-layer: MODE 3: u, u_bc, pbce, h in; the estimate out and in; u [, visc_rem] out [; a_u, h_u out] = 8-10 where the
// pair moves 12-13; MODE 1: u, u_bc, h in, visc_rem out = 4 against 8.  The same expressions in the same order as the kernels it
// replaces (CoefWalk; the sweeps are copies): bit-identical.  KV_ML_INVZ2 (a top-down pre-pass through a_u), Rayleigh drag and the
// direct-stress option stay with the separate kernels.
template <int DIR, int MODE, bool REM, bool WRITE_COEF, int NKT, bool LEAN>
__global__ void __launch_bounds__(64)
k_vertvisc_coef_cols(Dm d, const double *__restrict__ G, mom6x_vertvisc_params CS, const double *u_in, const double *__restrict__ u_bc,
                     double dtx, const double *__restrict__ h, const double *__restrict__ Kv_bbl, const double *__restrict__ bbl_thick_in,
                     const double *__restrict__ Kv_shear, double *__restrict__ a_out, double *h_out, double H_to_Z,
                     double h_neglect, double dz_neglect, double a_cpl_max, double I_amax, LayerAccelSrc LA,
                     double *u, double *__restrict__ vr, const double *__restrict__ tau, double dt, double dt_Rho0, double H_to_RZ,
                     double *__restrict__ tau_bot) {
  static_assert(MODE == 1 || MODE == 3, "k_vertvisc_coef_cols: MODE 1 (coefficients + remnant) or 3 (coefficients + solve)");
  static_assert(MODE == 3 || REM, "k_vertvisc_coef_cols: MODE 1 makes the remnant");
  constexpr int NK = NK_OF(NKT);
  const int nk = NK_EXACT(NKT) ? NK : d.nk;   // (NKT < 0: the arrays and unrolled loops have NK slots, the column nk <= NK layers)
  extern __shared__ double cc_lds[];
  // (DIR = 1: a block column's rows on ONE XCD, so that the row north of a face column -- the next work-group's own row -- meets it in
  //  that XCD's L2, was measured: 1.77-1.81 against 1.56 ms per launch; rows along blockIdx.y it is.)
  const int i = I_BASE((DIR ? 0 : -1)) + blockIdx.x * 64 + threadIdx.x;
  const int j = (DIR ? -1 : 0) + blockIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (i < ((DIR ? 0 : -1))) return;
  const int st = DIR ? d.pitch : 1;
  const size_t x = ix2(d, i, j), y = x + st, slab = (size_t)d.slab;
  double *hh = cc_lds + threadIdx.x;               // h_u(k) at hh[k * 64], later the un-substituted remnant
  const double mC = gm(G, d, DIR ? MOM6X_G_mask2dCv : MOM6X_G_mask2dCu)[x];
  // accel_layer_u of btstep_layer_accel formed here (k_vertvisc_coef, MODE 3)
  double la_e0 = 0., la_e1 = 0., la_g0 = 0., la_g1 = 0., la_a = 0., la_Idx = 0.;
  if (MODE == 3) {
    la_e0 = LA.e_anom[x]; la_e1 = LA.e_anom[y]; la_g0 = LA.g_own[x]; la_g1 = LA.g_nbr[y]; la_a = LA.a2d[x];
    la_Idx = gm(G, d, DIR ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  }
  auto abt_of = [&](double pb0, double pb1) -> double {
    double a = (la_a - (((pb1 - la_g1) * la_e1) - ((pb0 - la_g0) * la_e0)) * la_Idx);
    if (fabs(a) < LA.underflow) a = 0.0;
    return a;
  };
  if (!(mC > 0.)) {   // do_i :1514-1516: (MODE 3) the velocity estimate of the masked faces too; no coefficients, no solve
    if (MODE == 3) {
      double ul = 0.0;
      for (int k = 0; k < nk; k++) {
        const size_t c = x + (size_t)k * slab;
        ul = mC * (u_in[c] + dtx * (u_bc[c] + abt_of(LA.pbce[c], LA.pbce[c + st])));
        u[c] = ul;
      }
      if (tau_bot) tau_bot[x] = H_to_RZ * (ul * a_out[x + (size_t)nk * slab]);
    }
    return;
  }
  const double *bathyT = gm(G, d, MOM6X_G_bathyT);
  double I_valBL = 0.0; if (CS.harm_BL_val > 0.0) I_valBL = 1.0 / CS.harm_BL_val;
  double I_Hbbl = 1. / (CS.Hbbl + dz_neglect), kv_bbl = 0.0, bbl_thick = 0.0;
  if (CS.bottomdraglaw) {
    kv_bbl = Kv_bbl[x];
    bbl_thick = bbl_thick_in[x] + dz_neglect;
    I_Hbbl = 1. / bbl_thick;
  }
  CoefWalk W;
  W.init(CS, bathyT[x], bathyT[y], I_Hbbl, I_valBL, kv_bbl, bbl_thick, dz_neglect, H_to_Z, h_neglect, dz_neglect, a_cpl_max, I_amax);
  double aa[NK + 1];                               // a_u(K), then c1(k)
  constexpr bool EST_LDS = (MODE == 3) && WRITE_COEF;
  // ---- pass 1
  constexpr int CC_G = (MODE == 1) ? CC_GROUP1 : CC_GROUP;   // layers per group of the walk (MODE 1 holds no pbce pair)
  constexpr int NG = (NK + CC_G - 1) / CC_G, NP = (NG + 1) / 2;
  double q_u[2][CC_G], q_b[2][CC_G], q_p0[2][CC_G], q_p1[2][CC_G], q_h0[2][CC_G], q_h1[2][CC_G];
  double t_a[2][CC_G];
  double a_bot = 0.;
  auto fetch = [&](int g, const int b) {
#pragma unroll
    for (int m = 0; m < CC_G; m++) {
      const int k = NK - 1 - (g * CC_G + m);
      if (k >= 0) {
        // (NKT < 0: a slot below the column's bottom fetches the bottom layer once more instead of standing under a test on the
        //  layer index: the number of loads in flight stays a constant of the code and the waits for them stay partial)
        const size_t c = x + (size_t)(NK_EXACT(NKT) ? k : min(k, nk - 1)) * slab;
        q_u[b][m] = u_in[c]; q_b[b][m] = u_bc[c];
        if (MODE == 3) { q_p0[b][m] = LA.pbce[c]; q_p1[b][m] = LA.pbce[c + st]; }
        q_h0[b][m] = h[c]; q_h1[b][m] = h[c + st];
      }
    }
  };
  auto group = [&](int g, const int b) {
#pragma unroll
    for (int m = 0; m < CC_G; m++) {
      const int k = NK - 1 - (g * CC_G + m);
      if (k >= 0 && k < nk) {
        const size_t c = x + (size_t)k * slab;
        const double uk = (MODE == 3) ? mC * (q_u[b][m] + dtx * (q_b[b][m] + abt_of(q_p0[b][m], q_p1[b][m])))
                                      : mC * (q_u[b][m] + dtx * q_b[b][m]);
        const int K = k + 1;
        double Kv_add = 0.0;
        if (K < nk && Kv_shear) Kv_add = 0.5 * (Kv_shear[x + (size_t)K * slab] + Kv_shear[y + (size_t)K * slab]);
        double hu, a;
        W.layer<LEAN>(K, nk, q_h0[b][m], q_h1[b][m], uk, 0.0, Kv_shear != nullptr, Kv_add, hu, a);
        t_a[b][m] = a;
        if (k == nk - 1) a_bot = a;                  // a_u at the bottom interface (aa[nk]): the walk's first layer
        // between the passes: h_u in LDS and the estimate through the result array -- or, when h_u is written anyway, the estimate
        // in LDS and h_u back from its array (a word less)
        if (EST_LDS) hh[k * 64] = uk; else { hh[k * 64] = hu; if (MODE == 3) u[c] = uk; }
        if (WRITE_COEF) { h_out[c] = hu; a_out[x + (size_t)K * slab] = a; }
      }
      __builtin_amdgcn_sched_barrier(0);             // (one layer's temporaries at a time)
    }
  };
  fetch(0, 0);
#pragma unroll 1
  for (int p = 0; p < NP; p++) {
    if (2 * p + 1 < NG) fetch(2 * p + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    group(2 * p, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (2 * p + 2 < NG) fetch(2 * p + 2, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (2 * p + 1 < NG) group(2 * p + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    cc_file_switch<NK, CC_G>(p, aa, t_a);
  }
  aa[0] = dmin(a_cpl_max, 0.0);                    // a_cpl(:,:,1) stays 0 without shelves / dynamic mixed-layer viscosity
  if (WRITE_COEF) a_out[x] = aa[0];
  asm volatile("" ::: "memory");
  // ---- pass 2: the forward sweep of k_vertvisc_cols / k_vertvisc_remnant_cols from the chip; the velocity estimate comes back
  //      (written a column's walk ago: mostly from the L2) U_G layers ahead of the sweep
  const double surface_stress = (MODE == 3) ? dt_Rho0 * (mC * tau[x]) : 0.0;
  ThomasFwd<MODE == 3, REM> T = { 0., 0., 0., 0. };
  double uu[(MODE == 3) ? NK : 1];
  constexpr int U_G = CC_UG;
  const double *back = EST_LDS ? (const double *)h_out : (const double *)u;   // what comes back from memory: h_u or the estimate
  if (MODE == 3) {
#pragma unroll
    for (int k = 0; k < U_G && k < NK; k++) uu[k] = back[x + (size_t)min(k, nk - 1) * slab];
  }
#pragma unroll
  for (int k = 0; k < NK; k++) {
    // (NKT < 0: the loads are NOT under the test on the layer index -- a slot beyond the column reads the bottom layer again --, so
    //  that the memory counter of the loads in flight stays exact across the tests; with them inside, the compiler waits for every
    //  load at every join: 70 instead of 15 s_waitcnt vmcnt(0), and the kernel ran at half its speed)
    if (MODE == 3 && k + U_G < NK) uu[(MODE == 3) ? k + U_G : 0] = back[x + (size_t)min(k + U_G, nk - 1) * slab];
    if (k < nk) {
    const double a_k = aa[k], a_kp = aa[k + 1];
    const double from_lds = hh[k * 64], from_mem = (MODE == 3) ? uu[(MODE == 3) ? k : 0] : 0.0;
    const double hu = EST_LDS ? from_mem : from_lds;
    const double u0 = EST_LDS ? from_lds : from_mem;
    if (k == 0) T.first(hu, a_k, a_kp, 0., dt, u0, surface_stress);
    else aa[k] = T.next(hu, a_k, a_kp, 0., dt, u0);   // c1(k)
    if (MODE == 3) uu[(MODE == 3) ? k : 0] = T.u;
    if (REM) hh[k * 64] = T.r;
    }
    if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  }
  double uprev = T.u, rprev = T.r;
  if (MODE == 3) u[x + (size_t)(nk - 1) * slab] = uprev;
  if (REM) vr[x + (size_t)(nk - 1) * slab] = rprev;
  const double u_bot = uprev;   // uu[nk - 1]
  asm volatile("" ::: "memory");
  // ---- pass 3: back substitution
#pragma unroll
  for (int k = NK - 2; k >= 0; k--) {
    if (k >= nk - 1) continue;
    const size_t x3 = x + (size_t)k * slab;
    const double ck = aa[k + 1];
    if (MODE == 3) { uprev = uu[(MODE == 3) ? k : 0] + ck * uprev; u[x3] = uprev; }
    if (REM) { rprev = hh[k * 64] + ck * rprev; vr[x3] = rprev; }
  }
  if (MODE == 3 && tau_bot) tau_bot[x] = H_to_RZ * (u_bot * a_bot);
}

extern "C" int mom6x_vertvisc_init(mom6x_ctx *c, const mom6x_vertvisc_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_vertvisc_init: null argument");
  HIPCHK(hipSetDevice(c->device));
  VvState *S = vv_state(c);
  S->P = *p;
  const size_t n3 = (size_t)c->dims.slab * c->dims.nk, n3i = (size_t)c->dims.slab * (c->dims.nk + 1);
  if (!S->own_a_u) HIPCHK(hipMalloc(&S->own_a_u, n3i * sizeof(double)));
  if (!S->own_a_v) HIPCHK(hipMalloc(&S->own_a_v, n3i * sizeof(double)));
  if (!S->own_h_u) HIPCHK(hipMalloc(&S->own_h_u, n3 * sizeof(double)));
  if (!S->own_h_v) HIPCHK(hipMalloc(&S->own_h_v, n3 * sizeof(double)));
  HIPCHK(hipMemsetAsync(S->own_a_u, 0, n3i * sizeof(double), c->stream)); HIPCHK(hipMemsetAsync(S->own_a_v, 0, n3i * sizeof(double), c->stream));
  HIPCHK(hipMemsetAsync(S->own_h_u, 0, n3 * sizeof(double), c->stream)); HIPCHK(hipMemsetAsync(S->own_h_v, 0, n3 * sizeof(double), c->stream));
  S->a_u = S->own_a_u; S->a_v = S->own_a_v; S->h_u = S->own_h_u; S->h_v = S->own_h_v;
  S->init = true;
  return MOM6X_OK;
}

extern "C" int mom6x_vertvisc_set_visc(mom6x_ctx *c, const double *Kv_bbl_u, const double *Kv_bbl_v, const double *bbl_thick_u,
                                       const double *bbl_thick_v, const double *Kv_shear, const double *Ray_u, const double *Ray_v) {
  REQUIRE(c, MOM6X_EINVAL, "mom6x_vertvisc_set_visc: null ctx");
  REQUIRE((Ray_u != nullptr) == (Ray_v != nullptr), MOM6X_EINVAL, "mom6x_vertvisc_set_visc: Ray_u and Ray_v come together");
  VvState *S = vv_state(c);
  S->Kv_bbl_u = Kv_bbl_u; S->Kv_bbl_v = Kv_bbl_v; S->bbl_thick_u = bbl_thick_u; S->bbl_thick_v = bbl_thick_v;
  S->Kv_shear = Kv_shear; S->Ray_u = Ray_u; S->Ray_v = Ray_v;
  return MOM6X_OK;
}

extern "C" double *mom6x_vertvisc_field(mom6x_ctx *c, int which) {
  if (!c || !vertvisc_ready(c)) return nullptr;
  double *t[] = { c->vv->own_a_u, c->vv->own_a_v, c->vv->own_h_u, c->vv->own_h_v };
  return (which >= 0 && which < 4) ? t[which] : nullptr;
}

// vertvisc_coef on u, v themselves (mode 0) or on the velocity estimates the RK2 step would hand over: mask*(u + dtx*u_bc) (1),
// mask*(u + dtx*(u_bc + u_abt)) (2), or that with u_abt formed on the fly from the barotropic solver's results (3: LayerAccelSrc,
// mom6x_dev.h); modes 2 and 3 leave the estimate in u_out, v_out
static int vertvisc_coef_launch(mom6x_ctx *c, int mode, const double *u, const double *v, const double *u_bc, const double *v_bc,
                                const double *u_abt, const double *v_abt, const LayerAccelSrc &LAu, const LayerAccelSrc &LAv, double dtx,
                                const double *h, double dt, double *u_out, double *v_out) {
  REQUIRE(c && vertvisc_ready(c), MOM6X_EINVAL, "MOM_vert_friction(coef): Module must be initialized before it is used.");
  REQUIRE(u && v && h, MOM6X_EINVAL, "vertvisc_coef: null array");
  const VvState &S = *c->vv;
  REQUIRE(!S.P.bottomdraglaw || (S.Kv_bbl_u && S.Kv_bbl_v && S.bbl_thick_u && S.bbl_thick_v), MOM6X_EINVAL,
          "vertvisc_coef: BOTTOMDRAGLAW needs visc%Kv_bbl_u/v and visc%bbl_thick_u/v (mom6x_vertvisc_set_visc)");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const dim3 b = blk2();
  const mom6x_vgrid &GV = c->GV;
  const double a_cpl_max = 1.0e37 * GV.Z_to_H;
  const double I_amax = (S.P.answer_date < 20190101) ? (1.0e-10 * GV.H_to_Z) * dt : 0.0;
  const dim3 gu = grid3(nxa(d.ni + 1, -1), d.nj, 1, b), gv = grid3(d.ni, d.nj + 1, 1, b);
  const bool lean = vertvisc_walk_lean(S.P, GV);
#define VVC_AS(M, L)                                                                                                            \
  KLAUNCH(c, "k_vertvisc_coef<0>", (k_vertvisc_coef<0, M, L>), gu, b, d, c->G, S.P, u, u_out, u_bc, u_abt, dtx, h, S.Kv_bbl_u, S.bbl_thick_u, \
          S.Kv_shear, S.own_a_u, S.own_h_u, GV.H_to_Z, GV.H_subroundoff, GV.dZ_subroundoff, a_cpl_max, I_amax, LAu);           \
  KLAUNCH(c, "k_vertvisc_coef<1>", (k_vertvisc_coef<1, M, L>), gv, b, d, c->G, S.P, v, v_out, v_bc, v_abt, dtx, h, S.Kv_bbl_v, S.bbl_thick_v, \
          S.Kv_shear, S.own_a_v, S.own_h_v, GV.H_to_Z, GV.H_subroundoff, GV.dZ_subroundoff, a_cpl_max, I_amax, LAv)
#define VVC(M) do { if (lean) { VVC_AS(M, true); } else { VVC_AS(M, false); } } while (0)
  if (mode == 0) { VVC(0); } else if (mode == 1) { VVC(1); } else if (mode == 2) { VVC(2); } else { VVC(3); }
#undef VVC
#undef VVC_AS
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

// vertvisc_coef + the solve of the RK2 step as one kernel per direction (k_vertvisc_coef_cols) where it exists: up to COLS_NK_BOUND
// layers, no Rayleigh drag, no direct stress, no KV_ML_INVZ2.  MOM6X_VERTVISC=walk|pair: the two kernels.
static bool vertvisc_coef_solve_usable(mom6x_ctx *c) {
  if (!vertvisc_ready(c)) return false;
  const VvState &S = *c->vv;
  return vertvisc_form() == VV_DEFAULT && c->d.nk <= COLS_NK_BOUND && !S.Ray_u && !(S.ds_Hmix > 0.0) && !(S.P.Kvml_invZ2 > 0.0) &&
         S.a_u == S.own_a_u && S.a_v == S.own_a_v && S.h_u == S.own_h_u && S.h_v == S.own_h_v &&   // (the solve reads what vertvisc_coef writes)
         (!S.P.bottomdraglaw || (S.Kv_bbl_u && S.Kv_bbl_v && S.bbl_thick_u && S.bbl_thick_v));
}
static int vertvisc_coef_cols_launch(mom6x_ctx *c, int mode, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                                     const LayerAccelSrc &LAu, const LayerAccelSrc &LAv, double dtx, const double *h, double dt_coef,
                                     double *u, double *v, const double *taux, const double *tauy, double dt, double *taux_bot, double *tauy_bot,
                                     double *vr_u, double *vr_v, bool keep_coef) {
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const VvState &S = *c->vv;
  const mom6x_vgrid &GV = c->GV;
  const double a_cpl_max = 1.0e37 * GV.Z_to_H;
  const double I_amax = (S.P.answer_date < 20190101) ? (1.0e-10 * GV.H_to_Z) * dt_coef : 0.0;
  const double dt_Rho0 = dt / GV.H_to_RZ, HR = GV.H_to_RZ;
  const dim3 bc(64, 1, 1);
  const dim3 gu((unsigned)((nxa(d.ni + 1, -1) + 63) / 64), (unsigned)d.nj, 1), gv((unsigned)((d.ni + 63) / 64), (unsigned)(d.nj + 1), 1);
  const bool rem = (vr_u != nullptr), lean = vertvisc_walk_lean(S.P, GV);
#define VCS(DIR, M, R, WC, NKT, L, g, uin, ubc, LA, uo, vro, tau, taub, Kb, bt, ao, ho)                                                  \
  KLAUNCH_LDS(c, DIR ? "k_vertvisc_coef_cols<1>" : "k_vertvisc_coef_cols<0>", (k_vertvisc_coef_cols<DIR, M, R, WC, NKT, L>), g, bc,    \
              (size_t)NK_OF(NKT) * 64 * sizeof(double), d, c->G, S.P, uin, ubc,                                                       \
              dtx, h, Kb, bt, S.Kv_shear, ao, ho, GV.H_to_Z, GV.H_subroundoff, GV.dZ_subroundoff, a_cpl_max, I_amax, LA, uo, vro, tau, dt, dt_Rho0, HR, taub)
#define VCS2L(M, R, WC, NKT, L) do { \
    VCS(0, M, R, WC, NKT, L, gu, u_in, u_bc, LAu, u, vr_u, taux, taux_bot, S.Kv_bbl_u, S.bbl_thick_u, S.own_a_u, S.own_h_u); \
    VCS(1, M, R, WC, NKT, L, gv, v_in, v_bc, LAv, v, vr_v, tauy, tauy_bot, S.Kv_bbl_v, S.bbl_thick_v, S.own_a_v, S.own_h_v); } while (0)
#define VCS2(M, R, WC, NKT) do { if (lean) VCS2L(M, R, WC, NKT, true); else VCS2L(M, R, WC, NKT, false); } while (0)
#define VCS_ALL(NKT) do {                                                                                                               \
    if (mode == 1) VCS2(1, true, false, NKT);   /* (nobody sees the coefficients of :602-609: :737 replaces them) */                    \
    else if (rem && keep_coef) VCS2(3, true, true, NKT);                                                                                \
    else if (rem) VCS2(3, true, false, NKT);                                                                                            \
    else if (keep_coef) VCS2(3, false, true, NKT);                                                                                      \
    else VCS2(3, false, false, NKT); } while (0)
  COLS_NK_DISPATCH(d.nk, VCS_ALL);
#undef VCS_ALL
#undef VCS2
#undef VCS2L
#undef VCS
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}

// The RK2 step's :591-610: vertvisc_coef on mask * (u + dt * u_bc_accel), then vertvisc_remnant -- in one kernel per direction where
// that exists (nobody sees these coefficients: :737 replaces them), else as the two routines; a context without device coefficients
// (no vertvisc_init) takes the remnant of the coefficients it was given.
int vertvisc_stage_remnant(mom6x_ctx *c, const double *u, const double *v, const double *u_bc, const double *v_bc, const double *h,
                           double dt, double *vr_u, double *vr_v) {
  REQUIRE(c, MOM6X_EINVAL, "vertvisc_stage_remnant: null context");
  int rc;
  const LayerAccelSrc none = {};
  if (vertvisc_coef_solve_usable(c)) {
    REQUIRE(u && v && u_bc && v_bc && h && vr_u && vr_v, MOM6X_EINVAL, "vertvisc_stage_remnant: null array");
    return vertvisc_coef_cols_launch(c, 1, u, v, u_bc, v_bc, none, none, dt, h, dt, nullptr, nullptr, nullptr, nullptr, dt, nullptr, nullptr,
                                     vr_u, vr_v, false);
  }
  if (vertvisc_ready(c) && (rc = vertvisc_coef_launch(c, 1, u, v, u_bc, v_bc, nullptr, nullptr, none, none, dt, h, dt, nullptr, nullptr))) return rc;
  return mom6x_vertvisc_remnant(c, vr_u, vr_v, dt);
}

// The RK2 step's :681-767 and :957-1022: the velocity estimate u = mask * (u_in + dt * (u_bc + u_abt)) -- u_abt read from the arrays or,
// where a LayerAccelSrc pair is given, formed on the fly from that --, vertvisc_coef on it, vertvisc(u, v, dt) and, with vr_u, vertvisc_remnant(dt).  One kernel per
// direction where that exists, else vertvisc_coef (which leaves the estimate in u, v) + the fused solve; a context without device
// coefficients: the fused solve alone, which forms the estimate itself.  keep_coef: CS%a_u, CS%h_u are written even by the one-kernel
// form (the step's LAST vertvisc_coef, or a vertvisc_remnant of its own follows).
int vertvisc_stage_solve(mom6x_ctx *c, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                         const double *u_abt, const double *v_abt, const LayerAccelSrc *LAu, const LayerAccelSrc *LAv, double dt,
                         const double *h, double *u, double *v, const double *taux, const double *tauy, double *taux_bot, double *tauy_bot,
                         double *vr_u, double *vr_v, bool keep_coef) {
  REQUIRE(c && u_in && v_in && u_bc && v_bc && h && u && v && taux && tauy, MOM6X_EINVAL, "vertvisc_stage_solve: null array");
  REQUIRE((LAu != nullptr) == (LAv != nullptr) && (LAu || (u_abt && v_abt)), MOM6X_EINVAL,
          "vertvisc_stage_solve: the barotropic accelerations come as two arrays or as two LayerAccelSrc");
  REQUIRE((vr_u != nullptr) == (vr_v != nullptr), MOM6X_EINVAL, "vertvisc_stage_solve: visc_rem_u and visc_rem_v come together");
  if (!vertvisc_ready(c)) {
    REQUIRE(u_abt && v_abt, MOM6X_EINVAL, "vertvisc_stage_solve: without device coefficients the accelerations come as arrays");
    return vertvisc_fused(c, u_in, v_in, u_bc, v_bc, u_abt, v_abt, dt, u, v, taux, tauy, dt, taux_bot, tauy_bot, vr_u, vr_v, h);
  }
  if (LAu && vertvisc_coef_solve_usable(c))
    return vertvisc_coef_cols_launch(c, 3, u_in, v_in, u_bc, v_bc, *LAu, *LAv, dt, h, dt, u, v, taux, tauy, dt, taux_bot, tauy_bot, vr_u, vr_v,
                                     keep_coef);
  int rc;
  const LayerAccelSrc none = {};
  if ((rc = vertvisc_coef_launch(c, LAu ? 3 : 2, u_in, v_in, u_bc, v_bc, LAu ? nullptr : u_abt, LAu ? nullptr : v_abt, LAu ? *LAu : none,
                                 LAu ? *LAv : none, dt, h, dt, u, v))) return rc;
  return vertvisc_fused(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, u, v, taux, tauy, dt, taux_bot, tauy_bot, vr_u, vr_v, h);
}

extern "C" int mom6x_vertvisc_coef(mom6x_ctx *c, const double *u, const double *v, const double *h, double dt) {
  const LayerAccelSrc none = {};
  return vertvisc_coef_launch(c, 0, u, v, nullptr, nullptr, nullptr, nullptr, none, none, 0.0, h, dt, nullptr, nullptr);
}

extern "C" int mom6x_vertvisc_set_coef(mom6x_ctx *c, const double *a_u, const double *a_v, const double *h_u,
                                       const double *h_v, const double *Ray_u, const double *Ray_v) {
  REQUIRE(c && a_u && a_v && h_u && h_v, MOM6X_EINVAL, "mom6x_vertvisc_set_coef: null mandatory array");
  REQUIRE((Ray_u != nullptr) == (Ray_v != nullptr), MOM6X_EINVAL, "mom6x_vertvisc_set_coef: Ray_u and Ray_v come together");
  VvState *S = vv_state(c);
  S->a_u = a_u; S->a_v = a_v; S->h_u = h_u; S->h_v = h_v; S->Ray_u = Ray_u; S->Ray_v = Ray_v;
  return MOM6X_OK;
}

extern "C" int mom6x_vertvisc(mom6x_ctx *c, double *u, double *v, const double *taux, const double *tauy, double dt,
                              double *taux_bot, double *tauy_bot) {
  REQUIRE(c && vertvisc_has_coef(c), MOM6X_EINVAL, "MOM_vert_friction(visc): Module must be initialized before it is used.");
  REQUIRE(u && v && taux && tauy, MOM6X_EINVAL, "vertvisc: null array");
  return vertvisc_fused(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, u, v, taux, tauy, dt, taux_bot, tauy_bot, nullptr, nullptr,
                        nullptr);
}

extern "C" int mom6x_vertvisc_set_direct_stress(mom6x_ctx *c, double Hmix_stress, const double *h) {
  REQUIRE(c, MOM6X_EINVAL, "vertvisc_set_direct_stress: null context");
  REQUIRE(!(Hmix_stress > 0.0) || h, MOM6X_EINVAL, "vertvisc: DIRECT_STRESS needs the layer thicknesses");
  VvState *S = vv_state(c);
  S->ds_Hmix = (Hmix_stress > 0.0) ? Hmix_stress : 0.0;
  S->ds_h = (Hmix_stress > 0.0) ? h : nullptr;
  return MOM6X_OK;
}

extern "C" int mom6x_vertvisc_remnant(mom6x_ctx *c, double *visc_rem_u, double *visc_rem_v, double dt) {
  REQUIRE(c && vertvisc_has_coef(c), MOM6X_EINVAL, "MOM_vert_friction(remant): Module must be initialized before it is used.");
  REQUIRE(visc_rem_u && visc_rem_v, MOM6X_EINVAL, "vertvisc_remnant: null array");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  const VvState &S = *c->vv;
  double *c1;
  int rc;
  if (vertvisc_cols_usable(d.nk, S.Ray_u, DirectStress{}) && !S.Ray_v) {
    const dim3 bc(64, 1, 1);
#define VRC(NKT) do {                                                                                                                   \
    KLAUNCH(c, "k_vertvisc_remnant_cols<0>", (k_vertvisc_remnant_cols<0, NKT>), dim3((unsigned)((nxa(d.ni + 1, -1) + 63) / 64), (unsigned)d.nj, 1), bc, \
            d, c->G, visc_rem_u, S.a_u, S.h_u, dt);                                                                                    \
    KLAUNCH(c, "k_vertvisc_remnant_cols<1>", (k_vertvisc_remnant_cols<1, NKT>), dim3((unsigned)((d.ni + 63) / 64), (unsigned)(d.nj + 1), 1), bc, \
            d, c->G, visc_rem_v, S.a_v, S.h_v, dt); } while (0)
    COLS_NK_DISPATCH(d.nk, VRC);
#undef VRC
    HIPCHK(hipGetLastError());
    return MOM6X_OK;
  }
  if ((rc = ctx_scratch(c, SCR_c1, d.nk, &c1))) return rc;
  const dim3 b = blk2();
  KLAUNCH(c, "k_vertvisc_remnant<0>", k_vertvisc_remnant<0>, grid3(nxa(d.ni + 1, -1), d.nj, 1, b), b, d, c->G, visc_rem_u, S.a_u, S.h_u,
          S.Ray_u, c1, dt);
  KLAUNCH(c, "k_vertvisc_remnant<1>", k_vertvisc_remnant<1>, grid3(d.ni, d.nj + 1, 1, b), b, d, c->G, visc_rem_v, S.a_v, S.h_v,
          S.Ray_v, c1, dt);
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
