// mom6x_dev.h -- device-side helpers shared by all HIP kernels of the dycore (gfx950 only).
//
// Layout: see include/mom6x.h.  Every kernel gets the tile dims by value (`Dm`), a pointer to
// the metric block and plain FP64 device pointers.  i is the coalesced (lane) index in every
// kernel, exactly as the reference's inner `do i` loops; columns (k) are walked per thread.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../include/mom6x.h"

struct Dm {            // device copy of the layout part of mom6x_dims
  int ni, nj, nk, halo, ioff, joff, pitch, slab;
};

__host__ __device__ inline Dm make_dm(const mom6x_dims &d) {
  Dm m; m.ni = d.ni; m.nj = d.nj; m.nk = d.nk; m.halo = d.halo; m.ioff = d.ioff; m.joff = d.joff;
  m.pitch = d.pitch; m.slab = d.slab; return m;
}

__device__ __forceinline__ size_t ix2(const Dm &d, int i, int j) {
  return (size_t)(i + d.ioff) + (size_t)(j + d.joff) * (size_t)d.pitch;
}
__device__ __forceinline__ size_t ix3(const Dm &d, int i, int j, int k) {
  return ix2(d, i, j) + (size_t)k * (size_t)d.slab;
}
__device__ __forceinline__ const double *gm(const double *G, const Dm &d, int m) {
  return G + (size_t)m * (size_t)d.slab;
}

// Two families of MAX and MIN.  They differ only on a tie, where dmax / dmin return the SECOND argument and fmax1 / fmin1 the
// FIRST, as the reference's compiler evaluates MAX(a, b) and MIN(a, b): between +0 and -0 that decides the sign of the zero.
// Every call site keeps the family it was held to the reference with; do not convert one into the other.
__device__ __forceinline__ double dmax(double a, double b) { return (a > b) ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return (a < b) ? a : b; }
__device__ __forceinline__ double fmax1(double a, double b) { return (b > a) ? b : a; }
__device__ __forceinline__ double fmin1(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double dsign(double a, double b) { return (b >= 0.0) ? fabs(a) : -fabs(a); }

// cuberoot of MOM_intrinsic_functions.F90:48-114 with rescale_cbrt (:118-159) and descale (:163-184): the argument's fraction is moved
// into [0.125, 1) by an integer power of 8, two Halley steps on a fraction num / den, one division, one Newton step, and the exponent
// put back.  Pure arithmetic in the reference's order: bit for bit, and exact under a scaling of x by 8**n.
__device__ __forceinline__ double dev_cuberoot(double x) {
  if ((x >= 0.0) == (x <= 0.0)) return x;   // 0 or NaN
  long long xb = __double_as_longlong(x);
  const long long s_a = (xb >> 63) & 1ll;
  const long long e_a = ((xb >> 52) & 0x7FFll) - 1023ll;
  long long e_mod = e_a % 3ll; if (e_mod < 0) e_mod += 3ll;   // modulo(): floor
  const long long e_r = (e_a - e_mod) / 3ll + 1ll;
  xb = (xb & 0x000FFFFFFFFFFFFFll) | ((e_mod - 3ll + 1023ll) << 52);
  const double asx = __longlong_as_double(xb);
  const double r0 = 0.707106;
  const double r0_3 = r0 * r0 * r0;
  double num = r0 * (r0_3 + 2.0 * asx);
  double den = 2.0 * r0_3 + asx;
#pragma unroll
  for (int itt = 0; itt < 2; ++itt) {
    const double num_prev = num, den_prev = den;
    const double np_3 = num_prev * num_prev * num_prev;
    const double dp_3 = den_prev * den_prev * den_prev;
    num = num_prev * (np_3 + 2.0 * asx * dp_3);
    den = den_prev * (2.0 * np_3 + asx * dp_3);
  }
  double root_asx = num / den;
  const double ra_3 = root_asx * root_asx * root_asx;
  root_asx = root_asx - (ra_3 - asx) / (3.0 * (root_asx * root_asx));
  long long rb = __double_as_longlong(root_asx);
  const long long e = (rb >> 52) & 0x7FFll;
  rb = (rb & ~(0x7FFll << 52)) | (((e_r + e) & 0x7FFll) << 52);
  rb = (rb & 0x7FFFFFFFFFFFFFFFll) | (s_a << 63);
  return __longlong_as_double(rb);
}

// a bit of the context's device-side error flag (mom6x_ctx::flag) with a message of its own in mom6x_ctx_sync: MEKE_equilibrium left a
// column at one of the reference's two `stop`s (MOM_MEKE.F90:1095 the bracket, :1133 more than 200 bisections)
#define MOM6X_FLAG_MEKE_EQUILIBRIUM 64
// neutral_diffusion.hip: a face or a column reached one of the reference's `stop` / FATAL sites (MOM_neutral_diffusion.F90:1426, :1428
// klm1, krm1 out of bounds; :1616 Ppos < Pneg; :1203, :1205 ppm_ave's dx outside [0, 1]); mom6x_neutral_diffusion_status has the counts
#define MOM6X_FLAG_NEUTRAL_DIFFUSION 128

// ---------------------------------------------------------------------------------------------
// host-side error plumbing
void mom6x_set_error(const char *fmt, ...);
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      mom6x_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return MOM6X_EHIP;                                                                   \
    }                                                                                      \
  } while (0)
#define REQUIRE(cond, code, msg)                  \
  do {                                            \
    if (!(cond)) { mom6x_set_error("%s", msg); return code; } \
  } while (0)
// an option of the reference that the device path of an init call (`who`) does not have
#define REFUSE(cond, who, what) REQUIRE(!(cond), MOM6X_EUNSUPPORTED, who ": " what " is not on the device")

// ---------------------------------------------------------------------------------------------
// The context (opaque to C callers).
#define MOM6X_NSCR 12
enum Scr { SCR_q = 0, SCR_KE, SCR_absv, SCR_e, SCR_c1, SCR_t0, SCR_t1, SCR_t2, SCR_t3 };
// One state struct per module, defined in the module's own file (ContState: continuity_dev.h, the module has three files).  It holds
// the module's parameter copy, its caller-owned pointers, the device arrays it allocates and an `init` flag where a setter may come
// before the init call.  The context only owns them: a typed pointer each, null until the module is first touched.
struct ContState; struct BTState; struct CorState; struct PgfState; struct VvState; struct HvState; struct RK2State; struct AleState;
struct TAState; struct DiagState; struct SvState; struct TdState; struct ThdState; struct VmState; struct MleState; struct MekeState; struct SdState; struct DaState; struct EpblState; struct DtsState; struct OpState; struct KsState; struct NdState;
struct Comm;   // halo.hip: tile layout + RCCL communicator (null: single tile, wrap only)

// u_bc_accel = (CAu + PFu) + diffu of the RK2 predictor (RK2.F90:565-572) formed by the pressure-force kernel that has just made
// PFu (all null: PressureForce on its own); the RK2 step hands it to PressureForce_bc
struct BcFold { const double *CAu, *CAv, *diffu, *diffv; double *u_bc, *v_bc; double *eta_h; };   // eta_h: bt_mass_source's column sum (h summed top-down, less the depth), a by-product
struct mom6x_ctx {
  // what every module shares
  mom6x_dims dims;
  Dm d;
  int device;
  hipStream_t stream;       // compute stream
  hipStream_t halo_stream;  // halo pack / RCCL send-recv / unpack
  double *G;                // device metric block [MOM6X_G_COUNT][slab]
  mom6x_vgrid GV;
  int first_direction;
  int *flag;                // device-side error flag (NaN / negative thickness; MOM6X_FLAG_* bits of single modules)
  // lazily allocated 3-D scratch arrays (slot -> nlev levels)
  double *scr[MOM6X_NSCR]; int scr_nlev[MOM6X_NSCR];
  bool prof_on;
  struct Prof *prof;
  // halo.hip: the bookkeeping of the group passes
  bool bt_overlap;          // btstep's own group pass of eta, ubt, vbt overlapped with the own-points half of the next sub-step (mom6x_comm_overlap_btstep)
  bool halo_error;          // set by a failed halo exchange inside a stream-ordered sequence
  hipEvent_t ev_ready, ev_done; bool pass_pending;   // the group pass in flight on the halo stream (start_/complete_group_pass)
  // the base width of the RK2 step's own group passes (0: the context's halo) -- a context whose halo was widened for the
  // barotropic solver (BTHALO) still sends NIHALO rows of the 3-D fields (mom6x_set_dyn_pass_width)
  int dyn_pass_width;
  long long n_exchanges, n_exchange_bytes;
  // the modules' states
  ContState *cont; BTState *bts; CorState *cor; PgfState *pgf; VvState *vv; HvState *hv; RK2State *rk2; AleState *ale;
  TAState *ta; DiagState *diag; SvState *sv; TdState *td; ThdState *thd; VmState *vm; MleState *mle; MekeState *meke; SdState *sd; DaState *da; EpblState *epbl; DtsState *dts; OpState *op; KsState *ks; NdState *nd; Comm *comm;
};
// Each frees every device pointer its struct owns, deletes the struct and nulls the context's pointer (a null pointer: nothing to
// do).  mom6x_ctx_destroy calls them all; apart from them it frees only what mom6x_ctx_create allocated.
void continuity_free(mom6x_ctx *c);  void bt_state_free(mom6x_ctx *c);          void CoriolisAdv_free(mom6x_ctx *c);
void PressureForce_free(mom6x_ctx *c);  void vertvisc_free(mom6x_ctx *c);       void hor_visc_free(mom6x_ctx *c);
void rk2_state_free(mom6x_ctx *c);   void ALE_free(mom6x_ctx *c);               void ta_state_free(mom6x_ctx *c);
void diag_sums_free(mom6x_ctx *c);   void set_visc_free(mom6x_ctx *c);          void thickness_diffuse_free(mom6x_ctx *c);
void tracer_hor_diff_free(mom6x_ctx *c);  void varmix_free(mom6x_ctx *c);       void mixedlayer_restrat_free(mom6x_ctx *c);
void MEKE_free(mom6x_ctx *c);  void set_diffusivity_free(mom6x_ctx *c);  void diabatic_aux_free(mom6x_ctx *c);  void energetic_PBL_free(mom6x_ctx *c);  void diabatic_TS_free(mom6x_ctx *c);  void opacity_free(mom6x_ctx *c);  void kappa_shear_free(mom6x_ctx *c);  void neutral_diffusion_free(mom6x_ctx *c);
void comm_free(mom6x_ctx *c);
// The widths of one group pass (create_group_pass(..., halo=)).  w: rows / columns of halo filled for its 3-D fields (0: the context's
// halo); wf[0 .. nwf - 1]: the widths of single 3-D fields (0 entries and fields beyond nwf: w).  The default is what every pass but the
// RK2 step's own asks for; the step sends the reference's own 2-3 rows instead of NIHALO = 4 (RK2.F90:484-495).
struct PassWidth { int w = 0; const int *wf = nullptr; int nwf = 0; };
void halo_wrap(mom6x_ctx *c, double *const *fields, const int *staggers, const int *nks, int n, PassWidth pw = {});    // do_group_pass
void halo_start(mom6x_ctx *c, double *const *fields, const int *staggers, const int *nks, int n, PassWidth pw = {});   // start_group_pass
void halo_complete(mom6x_ctx *c);                                     // complete_group_pass
bool halo_start_packed(mom6x_ctx *c, double *const *fields, const int *staggers, const int *nks, int n, PassWidth pw = {});   // ... packed on the compute stream
bool halo_can_overlap(const mom6x_ctx *c);
int comm_allreduce_scalar(mom6x_ctx *c, double *value, int op);       // halo.hip: 0 min, 1 max, 2 sum

// ---------------------------------------------------------------------------------------------
// Per-kernel timing with HIP events on the compute stream (mom6x_prof_* in include/mom6x.h).
// Off by default; when on, every KLAUNCH is bracketed by two events from a pool.
void prof_begin(mom6x_ctx *c, const char *name);
void prof_end(mom6x_ctx *c);
#define KLAUNCH(c, name, kern, grid, blk, ...)                              \
  do {                                                                      \
    if ((c)->prof_on) prof_begin((c), name);                                \
    hipLaunchKernelGGL(kern, grid, blk, 0, (c)->stream, __VA_ARGS__);       \
    if ((c)->prof_on) prof_end((c));                                        \
  } while (0)

#define KLAUNCH_LDS(c, name, kern, grid, blk, lds, ...)                     \
  do {                                                                      \
    if ((c)->prof_on) prof_begin((c), name);                                \
    hipLaunchKernelGGL(kern, grid, blk, lds, (c)->stream, __VA_ARGS__);     \
    if ((c)->prof_on) prof_end((c));                                        \
  } while (0)

int ctx_scratch(mom6x_ctx *c, int slot, int nlev, double **out);
int work_fill_byte();   // 0, or 0xFF with MOM6X_POISON_WORK=1 (ctx.hip): the initial contents of work arrays   // ctx.hip
// what mom6x_tile_steps (ctx.hip) reports, each defined next to the constants of its kernels
void corad_tile_steps(int *sx, int *sy);                           // coriolis_adv.hip: CF_X - 2, CF_Y - 2
void hor_visc_tile_steps(int *sx, int *sy);                        // hor_visc.hip: HV_TX - 2 * HT_H, HV_TY - 2 * HT_H
void tracer_advect_tile_steps(int *sx, int *sy);                   // tracer_advect.hip: TX, SEGY
// What one module asks of another (each lives in the file that owns the state).  xxx_ready: the module's init call has run
bool continuity_ready(const mom6x_ctx *c);  bool barotropic_ready(const mom6x_ctx *c);  bool CoriolisAdv_ready(const mom6x_ctx *c);
bool PressureForce_ready(const mom6x_ctx *c);  bool hor_visc_ready(const mom6x_ctx *c);
// neutral_diffusion.hip, for tracer_hordiff's neutral branch (tracer_hor_diff.hip): the module is initialised; RECALC_NEUTRAL_SURF; the
// module's Coef_x | Coef_y of nk + 1 planes each (the reference's locals of tracer_hordiff, MOM_tracer_hor_diff.F90:150-153)
bool neutral_diffusion_ready(const mom6x_ctx *c);  bool neutral_diffusion_recalc(const mom6x_ctx *c);
void neutral_diffusion_coef_arrays(const mom6x_ctx *c, double **Coef_x, double **Coef_y);
bool vertvisc_ready(const mom6x_ctx *c);                           // vert_friction.hip: vertvisc_coef is on the device (mom6x_vertvisc_init)
bool vertvisc_has_coef(const mom6x_ctx *c);                        // vert_friction.hip: there are coefficients to solve with (vertvisc_init or _set_coef)
int continuity_stencil(const mom6x_ctx *c);                        // continuity.hip: 3, SIMPLE_2ND 2, UPWIND_1ST 1 (needs continuity_ready)
int hor_visc_vel_stencil(const mom6x_ctx *c);                      // hor_visc.hip: 3 with a Leith viscosity, else 2
const double *PressureForce_Rlay(const mom6x_ctx *c);              // pressure_force.hip: the device copy of GV%Rlay (nk), or null before its init
int CorAdCalc_bc(mom6x_ctx *c, const double *u, const double *v, const double *h, const double *uh, const double *vh, double *CAu,
                 double *CAv, const double *PFu, const double *PFv, const double *diffu, const double *diffv, double *u_bc,
                 double *v_bc, double *uhtr, double *vhtr, double dt_tr);   // coriolis_adv.hip
// btstep_layer_accel (MOM_barotropic.F90:3432-3504) evaluated by the CONSUMER of accel_layer_u / _v instead of being written to
// HBM and read back: what a face column needs of the barotropic solver's 2-D results (barotropic.hip keeps them in its work block
// until the next btstep).
struct LayerAccelSrc {
  const double *pbce;      // 3-D
  const double *e_anom;    // 2-D, h points
  const double *g_own;     // gtot_E | gtot_N at the cell of the face's own index
  const double *g_nbr;     // gtot_W | gtot_S at the next cell
  const double *a2d;       // u_accel_bt | v_accel_bt (2-D)
  double underflow;        // accel_underflow = vel_underflow / dt
};
// pressure_force.hip, for the RK2 step: PressureForce whose kernel also forms what `fold` names.  *eta_h_written: fold.eta_h has been
// filled (the layered path only; with an equation of state nothing of the fold is formed)
int PressureForce_bc(mom6x_ctx *c, const double *h, double *PFu, double *PFv, double *pbce, double *eta, const BcFold &fold,
                     bool *eta_h_written);
// continuity.hip, for the RK2 step: continuity_PPM with the step's extras.  av_kind: the time average of the thicknesses that the
// convergence kernels write to `av` on the tile's own cells -- 1: av = 0.5 * (av_src + h) (RK2.F90:808-810); 2: av = 0.5 * (h_old +
// h_new) of an in-place call (:1025-1027 + :1064-1066); 0: none.  h_unused: the caller does not look at the new thicknesses
// (:646: hp is overwritten at :781 before anybody reads it), the convergence of the second direction is not computed.
struct ContFold { int av_kind; double *av; const double *av_src; bool h_unused; };
int continuity_PPM_fold(mom6x_ctx *c, const double *u, const double *v, const double *hin, double *h, double *uh, double *vh, double dt,
                        const double *uhbt, const double *vhbt, const double *visc_rem_u, const double *visc_rem_v, double *u_cor,
                        double *v_cor, const mom6x_BT_cont *BT, double *du_cor, double *dv_cor, const ContFold &fold);
int bt_mass_source_from(mom6x_ctx *c, const double *eta_h, const double *eta, int set_cor);   // bt_mass_source with the column sum given
int set_dtbt_eta(mom6x_ctx *c, const double *pbce, const double *eta);      // barotropic.hip: set_dtbt(pbce, eta=eta) RK2.F90:667
// barotropic.hip, for the RK2 step.  btcalc with h_u, h_v and `defer`: only the operands are noted, the next btstep's column pass
// forms the thickness fractions from them.  btstep with `defer_layer_accel`: k_layer_accel is skipped and accel_layer_u / _v are
// not written; the result stays pending in the work block (bt_layer_accel_src / _materialize).  The public entries pass false.
int btcalc_deferrable(mom6x_ctx *c, const double *h, const double *h_u, const double *h_v, bool defer);
int btstep_deferrable(mom6x_ctx *c, const double *U_in, const double *V_in, const double *eta_in, double dt, const double *bc_accel_u,
                      const double *bc_accel_v, const double *taux, const double *tauy, const double *pbce, const double *eta_PF_in,
                      const double *U_Cor, const double *V_Cor, double *accel_layer_u, double *accel_layer_v, double *eta_out,
                      double *uhbtav, double *vhbtav, const double *visc_rem_u, const double *visc_rem_v, const mom6x_BT_cont *BT_cont,
                      const double *taux_bot, const double *tauy_bot, const double *uh0, const double *vh0, const double *u_uh0,
                      const double *v_vh0, double *etaav, bool defer_layer_accel);
int bt_frhat_materialize(mom6x_ctx *c);                                 // writes frhatu / frhatv if a deferred btcalc is pending
bool bt_layer_accel_src(mom6x_ctx *c, LayerAccelSrc *u, LayerAccelSrc *v);   // false if no deferred result is pending
int bt_layer_accel_materialize(mom6x_ctx *c, double *accel_layer_u, double *accel_layer_v);
// vert_friction.hip, for the RK2 step.  Which kernels serve a call (one per direction with the column on chip, vertvisc_coef + the
// fused solve, or the fused solve alone in a context without device coefficients) is decided there.
// :591-610: vertvisc_coef on mask*(u + dt*u_bc), then vertvisc_remnant(vr_u, vr_v, dt)
int vertvisc_stage_remnant(mom6x_ctx *c, const double *u, const double *v, const double *u_bc, const double *v_bc, const double *h,
                           double dt, double *vr_u, double *vr_v);
// :681-767 / :957-1022: u = mask*(u_in + dt*(u_bc + u_abt)), u_abt from the arrays or, if given, from the LayerAccelSrc pair; vertvisc_coef
// on it; vertvisc(u, v, dt); [vertvisc_remnant(vr_u, vr_v, dt)].  keep_coef: CS%a_u, CS%h_u must hold these coefficients afterwards
int vertvisc_stage_solve(mom6x_ctx *c, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                         const double *u_abt, const double *v_abt, const LayerAccelSrc *LAu, const LayerAccelSrc *LAv, double dt,
                         const double *h, double *u, double *v, const double *taux, const double *tauy, double *taux_bot, double *tauy_bot,
                         double *vr_u, double *vr_v, bool keep_coef);
// [u = mask*(u_in + dtx*(u_bc + u_abt));] vertvisc(u, v, dt); [vertvisc_remnant(vr_u, vr_v, dt)] in one sweep, with the coefficients
// the context holds (the step's host-callback arms, which call back between the pieces).  h: vertvisc's thickness argument, read
// under DIRECT_STRESS only (null: the array mom6x_vertvisc_set_direct_stress was given -- the public vertvisc)
int vertvisc_fused(mom6x_ctx *c, const double *u_in, const double *v_in, const double *u_bc, const double *v_bc,
                   const double *u_abt, const double *v_abt, double dtx, double *u, double *v, const double *taux,
                   const double *tauy, double dt, double *taux_bot, double *tauy_bot, double *vr_u, double *vr_v, const double *h);

// k-chunking for "column-walk" kernels: a thread keeps its 2-D coefficients in registers and walks
// KCHUNK consecutive layers, so the 2-D metric planes are read nk/KCHUNK times instead of nk times.
#define KCHUNK 15
inline int nchunks(int nk) { return (nk + KCHUNK - 1) / KCHUNK; }

// The i-parallel kernels whose first index I0 is negative (u-points start at -1, widened loops at -2, -3) start
// their blocks at i = -IAL, a 128-byte line of the pitched rows (ioff = 16): every wavefront then reads and writes
// whole cache lines instead of sharing its first and last line with the neighbouring block (which usually runs
// on another XCD, i.e. behind another L2).  Lanes below I0 exit.  nxa() is the matching grid extent.
#define IAL 16
// The work-group of those kernels and of the other i-parallel ones (blk2()): a wavefront along i, LANE_BY rows.  With IAL it fixes
// where a launch extent rounds up to another block; mom6x_lane_launch_shape() hands the three to the tests that sit on those edges.
#define LANE_BX 64
#define LANE_BY 4
#define I_BASE(I0) (((I0) < 0) ? -IAL : (I0))
inline int nxa(int nx, int I0) { return (I0 < 0) ? nx + IAL + I0 : nx; }

// The lane of a kernel that serves the faces of both directions in one launch (blockIdx.z): one lane per face, lanes along i from
// i = -IAL, rows from j = -1 - W.  dir 0: u faces I = -1..ni-1, j = 0..nj-1; dir 1: v faces i = 0..ni-1, J = -1..nj-1; with W = 1
// every range is one face wider at either end (I = -2..ni, j = -1..nj | i = -1..ni, J = -2..nj).  x: the face and its own cell,
// y = x + st: the cell on its far side, ot: the stride across the face's direction.  A lane outside the ranges (!in) returns.
struct FaceLane { int dir, i, j; size_t x, y, st, ot; bool in; };
template <int W>
__device__ __forceinline__ FaceLane face_lane(const Dm &d) {
  FaceLane f;
  f.dir = blockIdx.z;
  f.i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  f.j = -1 - W + blockIdx.y * blockDim.y + threadIdx.y;
  f.in = f.i <= d.ni - 1 + W && f.j <= d.nj - 1 + W && (f.dir == 0 ? (f.i >= -1 - W && f.j >= -W) : (f.i >= -W));
  f.st = f.dir ? (size_t)d.pitch : 1; f.ot = f.dir ? 1 : (size_t)d.pitch;
  f.x = ix2(d, f.i, f.j); f.y = f.x + f.st;
  return f;
}

inline dim3 grid3(int nx, int ny, int nz, dim3 b) {
  return dim3((nx + b.x - 1) / b.x, (ny + b.y - 1) / b.y, (nz + b.z - 1) / b.z);
}
inline dim3 blk2() { return dim3(LANE_BX, LANE_BY, 1); }   // the work-group of the i-parallel kernels: a wavefront along i, four rows
inline dim3 gridk(int nx, int ny, int nk, dim3 b) { return dim3((nx + b.x - 1) / b.x, (ny + b.y - 1) / b.y, nchunks(nk)); }

// The kernels that keep a whole column on chip (registers + LDS: k_vertvisc_coef_cols, k_vertvisc_cols, k_vertvisc_remnant_cols,
// k_tridiag_cols, k_btcalc_cols, k_regrid_zstar_cols) unroll the column at compile time.  Their template argument NKT is the layer
// count itself (NKT > 0: 75, the headline's) or, negated, a BOUND on it: the register arrays and unrolled loops have -NKT slots and
// a wavefront-uniform test `k < nk` skips the ones beyond the column, so any nk <= -NKT runs the same code.
#define NK_OF(NKT) ((NKT) > 0 ? (NKT) : -(NKT))
#define NK_EXACT(NKT) ((NKT) > 0)
constexpr int COLS_NK_BOUND = 76;   // (k_vertvisc_coef_cols holds 4 x NK registers of column state next to ~190 others: 76 slots fit the 512 of a wavefront alone on its SIMD,
                                    //  78 spill, at 80 the coefficient column stays in scratch; k_regrid_zstar_cols spills at 80 too)
// (three bounds, so that a column fills at least 4/5 of the slots it pays for once it has more than 41 layers.  Not 64: with a bound
//  that is a multiple of the walk's group size, k_vertvisc_coef_cols' switch over the group pairs (cc_file_switch) is affine in the
//  pair's number, the compiler turns it into one store with a computed index, and the coefficient column lives in scratch memory.)
#define COLS_NK_DISPATCH(nk, CALL) do { if ((nk) == 75) { CALL(75); } else if ((nk) <= 52) { CALL(-52); } else if ((nk) <= 66) { CALL(-66); } \
                                        else { CALL(-COLS_NK_BOUND); } } while (0)
