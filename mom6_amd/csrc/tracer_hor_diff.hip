// tracer_hor_diff.hip -- along-layer diffusion of all tracers on gfx950.
//
//   tracer_hordiff        <- MOM_tracer_hor_diff.F90:119-699 on its along-layer path: the face diffusivities and khdt_x, khdt_y
//                            :237-357, the iteration count :371-390, the zeroing of df_x, df_y :392-402, the iteration :544-612
//   tracer_hor_diff_init  <- :1630-1779
//   tracer_hordiff_neutral <- the neutral branch :479-539, an entry of its own on the same state: khdt_x, khdt_y and the iteration
//                            count come from the helper both entries call (thd_khdt_and_itts), the rest is neutral_diffusion.hip's
//
// The 2-D part is two small launches: k_thd_khdt (both face directions, blockIdx.z; MAX and MIN are fmax1 and fmin1 of
// mom6x_dev.h, the reference compiler's) and, with CHECK_DIFFUSIVE_CFL, k_thd_cfl (the cell CFL and its maximum).  The iteration is
// k_thd_tile: the coefficients do not depend on the tracer, so h, khdt_x, khdt_y and IareaT are read once for up to eight tracers.
// The update is in place and every dTr of a layer is formed from the values BEFORE the iteration, so a work item may only read what
// its own work-group will overwrite.  A work-group owns HD_TX consecutive columns of a segment of HD_TY rows of one layer and walks
// the segment along j, one thread per column: the row below is the thread's own old value, kept in a register; the row above has
// not been written yet; the neighbours in i go through LDS.  What lies beyond the tile (one column on either side of every row,
// one row below and one above the segment) belongs to another work-group, which may have overwritten it already: it comes from
// the copies k_thd_save_x and k_thd_save_y made before the pass (tracer_advect.hip's k_ta_save_x/y, for a five-point stencil).
// h is only read and needs no copy.
#include "mom6x_dev.h"
#include <cmath>
#include <cfloat>
#include <vector>

constexpr int HD_TX = 240;     // columns of a work-group's tile (15 x 128 B: tiles start on cache lines); threads HD_TX and HD_TX + 1
                               // fetch the column west and east of the tile
constexpr int HD_TY = 64;      // rows of a work-group's segment
constexpr int HD_MAXT = 8;     // tracers per launch

namespace {

struct ThdK {       // tracer_hor_diff_CS and the switches of :221-227
  double dt, KhTr, KhTr_Slope_Cff, KhTr_min, KhTr_max, passivity_coeff, passivity_min, KhTr_fac, max_diff_CFL;
  int use_VarMix, Resoln_scaled, use_Eady, use_MEKE;
};

// khdt_x at the u faces and khdt_y at the v faces, :237-357.  The lane: face_lane<0> (mom6x_dev.h) written out, as measured faster.
__global__ void __launch_bounds__(256)
k_thd_khdt(Dm d, const double *__restrict__ G, ThdK K, const double *__restrict__ L2u, const double *__restrict__ SN_u,
           const double *__restrict__ L2v, const double *__restrict__ SN_v, const double *__restrict__ Res_fn_h,
           const double *__restrict__ Rd_dx_h, const double *__restrict__ MEKE_Kh, double *__restrict__ khdt_x,
           double *__restrict__ khdt_y) {
  const int dir = blockIdx.z;
  const int i = -IAL + blockIdx.x * blockDim.x + threadIdx.x;
  const int j = -1 + blockIdx.y * blockDim.y + threadIdx.y;
  if (i > d.ni - 1 || j > d.nj - 1) return;
  if (dir == 0 ? (i < -1 || j < 0) : (i < 0)) return;
  const size_t x = ix2(d, i, j), y = x + (dir ? (size_t)d.pitch : 1);
  const double len = gm(G, d, dir ? MOM6X_G_dx_Cv : MOM6X_G_dy_Cu)[x] * gm(G, d, dir ? MOM6X_G_IdyCv : MOM6X_G_IdxCu)[x];
  double khdt;
  if (K.use_VarMix) {                                                          // :238-281
    double Kh_loc = K.KhTr;
    if (K.use_Eady) Kh_loc = Kh_loc + K.KhTr_Slope_Cff * (dir ? L2v : L2u)[x] * (dir ? SN_v : SN_u)[x];
    if (K.use_MEKE) Kh_loc = Kh_loc + K.KhTr_fac * sqrt(MEKE_Kh[x] * MEKE_Kh[y]);
    if (K.KhTr_max > 0.) Kh_loc = fmin1(Kh_loc, K.KhTr_max);
    if (K.Resoln_scaled) Kh_loc = Kh_loc * 0.5 * (Res_fn_h[x] + Res_fn_h[y]);
    double Kh = fmax1(Kh_loc, K.KhTr_min);
    if (K.passivity_coeff > 0.) {
      const double Rd_dx = 0.5 * (Rd_dx_h[x] + Rd_dx_h[y]);
      Kh_loc = Kh * fmax1(K.passivity_min, K.passivity_coeff * Rd_dx);
      if (K.KhTr_max > 0.) Kh_loc = fmin1(Kh_loc, K.KhTr_max);
      Kh = fmax1(Kh_loc, K.KhTr_min);
    }
    khdt = K.dt * (Kh * len);
  } else if (K.Resoln_scaled) {                                                // :282-294
    const double Res_fn = 0.5 * (Res_fn_h[x] + Res_fn_h[y]);
    khdt = K.dt * (K.KhTr * len) * Res_fn;
  } else {
    khdt = K.dt * (K.KhTr * len);                                              // :305, :317
  }
  if (K.max_diff_CFL > 0.0) {                                                  // :322-357
    const double *aT = gm(G, d, MOM6X_G_areaT);
    const double khdt_max = 0.125 * K.max_diff_CFL * fmin1(aT[x], aT[y]);
    khdt = fmin1(khdt, khdt_max);
  }
  (dir ? khdt_y : khdt_x)[x] = khdt;
}

// CFL(i,j) and its maximum :373-378.  The maximum starts at 0.0 and only a larger value replaces it, so the bit patterns of the
// candidates order as unsigned integers.
__global__ void __launch_bounds__(256)
k_thd_cfl(Dm d, const double *__restrict__ G, const double *__restrict__ khdt_x, const double *__restrict__ khdt_y,
          double *__restrict__ CFL, unsigned long long *__restrict__ max_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  double cfl = 0.0;
  if (i < d.ni && j < d.nj) {
    const size_t x = ix2(d, i, j);
    cfl = 2.0 * ((khdt_x[x - 1] + khdt_x[x]) + (khdt_y[x - d.pitch] + khdt_y[x])) * gm(G, d, MOM6X_G_IareaT)[x];
    CFL[x] = cfl;
  }
  if (!(cfl > 0.0)) cfl = 0.0;
  for (int o = 32; o > 0; o >>= 1) { const double v = __shfl_xor(cfl, o); if (v > cfl) cfl = v; }
  if ((threadIdx.x & 63) == 0 && cfl > 0.0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(cfl));
}

struct HdList { double *t[HD_MAXT]; double *dfx[HD_MAXT]; double *dfy[HD_MAXT]; double underflow[HD_MAXT]; int n; };

// layouts of the copies: x: [k][m][boundary][side][j], boundaries nb = 0..ntx at the columns B = min(HD_TX*nb, ni), side 0 the
// column B-1, 1 the column B; y: [k][boundary][m][side][i], boundaries nb = 0..nseg at the rows B = min(HD_TY*nb, nj)
__device__ __forceinline__ size_t save_x_at(const Dm &d, int ntr, int ntx, int k, int m, int nb, int q) {
  return ((((size_t)k * ntr + m) * (size_t)(ntx + 1) + nb) * 2 + q) * (size_t)d.nj;
}
__device__ __forceinline__ size_t save_y_at(const Dm &d, int ntr, int nseg, int k, int m, int nb, int q) {
  return ((((size_t)k * (size_t)(nseg + 1) + nb) * ntr + m) * 2 + q) * (size_t)d.ni;
}

__global__ void __launch_bounds__(256)
k_thd_save_x(Dm d, HdList L, double *__restrict__ save, int ntx) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, nb = blockIdx.y, k = blockIdx.z;
  if (j >= d.nj) return;
  const int B = min(HD_TX * nb, d.ni);
  const size_t a = ix3(d, B - 1, j, k);
  for (int m = 0; m < L.n; m++) {
    save[save_x_at(d, L.n, ntx, k, m, nb, 0) + j] = L.t[m][a];
    save[save_x_at(d, L.n, ntx, k, m, nb, 1) + j] = L.t[m][a + 1];
  }
}

__global__ void __launch_bounds__(256)
k_thd_save_y(Dm d, HdList L, double *__restrict__ save, int nseg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, nb = blockIdx.y, k = blockIdx.z;
  if (i >= d.ni) return;
  const int B = min(HD_TY * nb, d.nj);
  const size_t a = ix3(d, i, B - 1, k);
  for (int m = 0; m < L.n; m++) {
    save[save_y_at(d, L.n, nseg, k, m, nb, 0) + i] = L.t[m][a];
    save[save_y_at(d, L.n, nseg, k, m, nb, 1) + i] = L.t[m][a + d.pitch];
  }
}

// Coef_x | Coef_y of :557-566 for the face between the cells with thicknesses ha and hb
__device__ __forceinline__ double hd_coef(double scale, double khdt, double ha, double hb, double h_neglect) {
  return ((scale * khdt) * 2.0 * (ha * hb)) / (ha + hb + h_neglect);
}

// One iteration of :547-610 for the tracers of L.  DF: some tracer has a flux diagnostic; first: this is the first iteration, whose
// df_x, df_y start from the zero of :392-402 (added, not read: a call of one iteration neither clears nor reads them).
template <int MAXT, bool DF>
__global__ void __launch_bounds__(256)
k_thd_tile(Dm d, const double *__restrict__ G, const double *__restrict__ h, HdList L, const double *__restrict__ khdt_x,
           const double *__restrict__ khdt_y, const double *__restrict__ save_x, const double *__restrict__ save_y, double scale,
           double h_neglect, double Idt, int first, int ntx, int nseg) {
  const int n = blockIdx.x, s = blockIdx.y, k = blockIdx.z, t = threadIdx.x, ntr = L.n;
  const int C0 = HD_TX * n, ncell = min(HD_TX, d.ni - C0);
  const int R0 = HD_TY * s, R1 = min(R0 + HD_TY, d.nj) - 1;
  const bool cell = t < ncell, west = (t == HD_TX), east = (t == HD_TX + 1), edge = west || east;
  const int i = cell ? C0 + t : (west ? C0 - 1 : C0 + ncell);
  const int slot = cell ? t + 1 : (west ? 0 : ncell + 1);
  const size_t p = (size_t)d.pitch;
  __shared__ double sT[2][MAXT][HD_TX + 2];          // the row's old values at the cells C0-1 .. C0+ncell (slot q <-> cell C0-1+q)
  __shared__ double s_h[2][HD_TX + 2];

  // a cell thread walks its column of the tracer arrays, an edge thread its column of the copy
  const double *hp = h + ix3(d, i, 0, k);
  const double *tp[MAXT];
  const size_t tstride = cell ? p : 1;
#pragma unroll
  for (int m = 0; m < MAXT; m++) {
    tp[m] = nullptr;
    if (m < ntr) tp[m] = cell ? L.t[m] + ix3(d, i, 0, k) : save_x + save_x_at(d, ntr, ntx, k, m, west ? n : n + 1, west ? 0 : 1);
  }
  double Ts[MAXT], Tc[MAXT], Tn[MAXT], hc = 0., hn = 0., Cs = 0.;
#pragma unroll
  for (int m = 0; m < MAXT; m++) { Ts[m] = 0.; Tc[m] = 0.; Tn[m] = 0.; }
  if (cell || edge) {
    hc = hp[(long)R0 * (long)p];
#pragma unroll
    for (int m = 0; m < MAXT; m++) if (m < ntr) Tc[m] = tp[m][(size_t)R0 * tstride];
  }
  if (cell) {
    const double hs = hp[((long)R0 - 1) * (long)p];
#pragma unroll
    for (int m = 0; m < MAXT; m++) if (m < ntr) Ts[m] = save_y[save_y_at(d, ntr, nseg, k, m, s, 0) + i];
    Cs = hd_coef(scale, khdt_y[ix2(d, i, R0 - 1)], hs, hc, h_neglect);
  }
  const double *IareaT = gm(G, d, MOM6X_G_IareaT);

  for (int j = R0; j <= R1; j++) {
    const int b = (j - R0) & 1;
    // ask for the next row, then hand this one over to LDS
    if (cell) {
      hn = hp[((long)j + 1) * (long)p];
#pragma unroll
      for (int m = 0; m < MAXT; m++)
        if (m < ntr) Tn[m] = (j < R1) ? tp[m][(size_t)(j + 1) * tstride] : save_y[save_y_at(d, ntr, nseg, k, m, s + 1, 1) + i];
    } else if (edge && j < R1) {
      hn = hp[((long)j + 1) * (long)p];
#pragma unroll
      for (int m = 0; m < MAXT; m++) if (m < ntr) Tn[m] = tp[m][(size_t)(j + 1) * tstride];
    }
    if (cell || edge) {
      s_h[b][slot] = hc;
#pragma unroll
      for (int m = 0; m < MAXT; m++) if (m < ntr) sT[b][m][slot] = Tc[m];
    }
    __syncthreads();   // (one barrier per row: the row after the next reuses this buffer, and nobody gets there before all have read it)
    if (cell) {
      const size_t x2 = ix2(d, i, j), x3 = x2 + (size_t)k * (size_t)d.slab;
      const double hw = s_h[b][t], he = s_h[b][t + 2];
      const double Cw = hd_coef(scale, khdt_x[x2 - 1], hw, hc, h_neglect);
      const double Ce = hd_coef(scale, khdt_x[x2], hc, he, h_neglect);
      const double Cn = hd_coef(scale, khdt_y[x2], hc, hn, h_neglect);
      const double Ihdxdy = IareaT[x2] / (hc + h_neglect);
#pragma unroll
      for (int m = 0; m < MAXT; m++) if (m < ntr) {
        const double Tw = sT[b][m][t], Te = sT[b][m][t + 2], T0 = Tc[m];
        const double fw = Cw * (Tw - T0), fe = Ce * (T0 - Te), fs = Cs * (Ts[m] - T0), fn = Cn * (T0 - Tn[m]);
        const double dTr = Ihdxdy * ((fw - fe) + (fs - fn));
        if constexpr (DF) {
          double *fx = L.dfx[m], *fy = L.dfy[m];
          if (fx) {
            fx[x3] = (first ? 0.0 : fx[x3]) + fe * Idt;
            if (i == 0) fx[x3 - 1] = (first ? 0.0 : fx[x3 - 1]) + fw * Idt;
          }
          if (fy) {
            fy[x3] = (first ? 0.0 : fy[x3]) + fn * Idt;
            if (j == 0) fy[x3 - p] = (first ? 0.0 : fy[x3 - p]) + fs * Idt;
          }
        }
        double Tnew = T0 + dTr;
        if (L.underflow[m] > 0.0 && fabs(Tnew) < L.underflow[m]) Tnew = 0.0;   // :605-610
        L.t[m][x3] = Tnew;
        Ts[m] = T0;
      }
      Cs = Cn;
    }
    hc = hn;
#pragma unroll
    for (int m = 0; m < MAXT; m++) Tc[m] = Tn[m];
  }
}

}  // namespace

struct ThdState {
  mom6x_tracer_hor_diff_params P;
  double *planes = nullptr;               // khdt_x | khdt_y | CFL
  unsigned long long *max_bits = nullptr; // the bit pattern of max_CFL
  double *save_x = nullptr, *save_y = nullptr;
  int ntx = 0, nseg = 0;
};

void tracer_hor_diff_free(mom6x_ctx *c) {
  ThdState *s = c->thd;
  if (!s) return;
  (void)hipFree(s->planes); (void)hipFree(s->max_bits); (void)hipFree(s->save_x); (void)hipFree(s->save_y);
  delete s;
  c->thd = nullptr;
}

// the kernel's tile extents, for tests that place a grid's edges around them
extern "C" int mom6x_tracer_hordiff_tile(int *tx, int *ty, int *max_tracers) {
  if (tx) *tx = HD_TX;
  if (ty) *ty = HD_TY;
  if (max_tracers) *max_tracers = HD_MAXT;
  return MOM6X_OK;
}

// the work arrays of a state whose parameters are set
static int tracer_hor_diff_alloc(mom6x_ctx *c, ThdState *s) {
  const Dm d = c->d;
  s->ntx = (d.ni + HD_TX - 1) / HD_TX; s->nseg = (d.nj + HD_TY - 1) / HD_TY;
  const size_t n2 = 3 * (size_t)d.slab * sizeof(double);
  const size_t nx = (size_t)d.nk * HD_MAXT * (s->ntx + 1) * 2 * d.nj * sizeof(double);
  const size_t ny = (size_t)d.nk * (s->nseg + 1) * HD_MAXT * 2 * d.ni * sizeof(double);
  HIPCHK(hipMalloc(&s->planes, n2));
  HIPCHK(hipMalloc(&s->max_bits, sizeof(unsigned long long)));
  HIPCHK(hipMalloc(&s->save_x, nx));
  HIPCHK(hipMalloc(&s->save_y, ny));
  HIPCHK(hipMemsetAsync(s->planes, work_fill_byte(), n2, c->stream));
  HIPCHK(hipMemsetAsync(s->save_x, work_fill_byte(), nx, c->stream));
  HIPCHK(hipMemsetAsync(s->save_y, work_fill_byte(), ny, c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_tracer_hor_diff_init(mom6x_ctx *c, const mom6x_tracer_hor_diff_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_tracer_hor_diff_init: null argument");
  REFUSE(p->use_neutral_diffusion, "tracer_hor_diff_init", "USE_NEUTRAL_DIFFUSION");
  REFUSE(p->use_hor_bnd_diffusion, "tracer_hor_diff_init", "USE_HORIZONTAL_BOUNDARY_DIFFUSION");
  REFUSE(p->Diffuse_ML_interior, "tracer_hor_diff_init", "DIFFUSE_ML_TO_INTERIOR (tracer_epipycnal_ML_diff)");
  REFUSE(p->offline, "tracer_hor_diff_init", "offline tracer transport (do_online_flag = .false., read_khdt_x, read_khdt_y)");
  REFUSE(p->open_bcs, "tracer_hor_diff_init", "open boundary conditions");
  REQUIRE(c->d.halo >= 1, MOM6X_EINVAL, "tracer_hor_diff_init: the stencil needs a halo of one");
  HIPCHK(hipSetDevice(c->device));
  tracer_hor_diff_free(c);
  ThdState *s = new ThdState;
  c->thd = s;
  s->P = *p;
  if (const int rc = tracer_hor_diff_alloc(c, s)) { tracer_hor_diff_free(c); return rc; }   // (no state without its arrays)
  return MOM6X_OK;
}

// khdt_x, khdt_y :237-357 and the iteration count :371-390 of a call whose arguments are checked, for both entries
struct ThdPlan { double *khx, *khy; int num_itts; double I_numitts, Idt; };
static int thd_khdt_and_itts(mom6x_ctx *c, ThdState *s, double dt, const double *L2u, const double *SN_u, const double *L2v,
                             const double *SN_v, const double *Res_fn_h, const double *Rd_dx_h, const double *MEKE_Kh, double *khdt_x_out,
                             double *khdt_y_out, double *cfl_out, int *num_itts_out, ThdPlan *plan) {
  const mom6x_tracer_hor_diff_params &P = s->P;
  ThdK K;
  K.dt = dt; K.KhTr = P.KhTr; K.KhTr_Slope_Cff = P.KhTr_Slope_Cff; K.KhTr_min = P.KhTr_min; K.KhTr_max = P.KhTr_max;
  K.passivity_coeff = P.KhTr_passivity_coeff; K.passivity_min = P.KhTr_passivity_min; K.KhTr_fac = P.MEKE_KhTr_fac;
  K.max_diff_CFL = P.max_diff_CFL;
  K.use_VarMix = P.use_variable_mixing != 0;
  K.Resoln_scaled = P.Resoln_scaled_KhTr != 0;
  K.use_Eady = K.use_VarMix && P.KhTr_Slope_Cff > 0.;                          // :225
  K.use_MEKE = K.use_VarMix && P.use_MEKE_Kh;                                   // :243
  REQUIRE(!K.use_Eady || L2u, MOM6X_EINVAL, "tracer_hordiff: KHTR_SLOPE_CFF > 0 needs VarMix%L2u");
  REQUIRE(!K.use_Eady || SN_u, MOM6X_EINVAL, "tracer_hordiff: KHTR_SLOPE_CFF > 0 needs VarMix%SN_u");
  REQUIRE(!K.use_Eady || L2v, MOM6X_EINVAL, "tracer_hordiff: KHTR_SLOPE_CFF > 0 needs VarMix%L2v");
  REQUIRE(!K.use_Eady || SN_v, MOM6X_EINVAL, "tracer_hordiff: KHTR_SLOPE_CFF > 0 needs VarMix%SN_v");
  REQUIRE(!K.use_MEKE || MEKE_Kh, MOM6X_EINVAL, "tracer_hordiff: the MEKE term needs MEKE%Kh (MEKE_Kh)");
  REQUIRE(!K.Resoln_scaled || Res_fn_h, MOM6X_EINVAL, "tracer_hordiff: RESOLN_SCALED_KHTR needs VarMix%Res_fn_h");
  REQUIRE(!(K.use_VarMix && P.KhTr_passivity_coeff > 0.) || Rd_dx_h, MOM6X_EINVAL,
          "tracer_hordiff: KHTR_PASSIVITY_COEFF > 0 needs VarMix%Rd_dx_h");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;
  double *khx = khdt_x_out ? khdt_x_out : s->planes, *khy = khdt_y_out ? khdt_y_out : s->planes + d.slab;
  const dim3 b = blk2();
  KLAUNCH(c, "k_thd_khdt", k_thd_khdt, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, c->G, K, L2u, SN_u, L2v, SN_v, Res_fn_h, Rd_dx_h,
          MEKE_Kh, khx, khy);

  int num_itts = 1;                                                            // :371-390
  if (P.check_diffusive_CFL) {
    double *cfl = cfl_out ? cfl_out : s->planes + 2 * (size_t)d.slab;
    HIPCHK(hipMemsetAsync(s->max_bits, 0, sizeof(unsigned long long), c->stream));
    KLAUNCH(c, "k_thd_cfl", k_thd_cfl, grid3(d.ni, d.nj, 1, b), b, d, c->G, (const double *)khx, (const double *)khy, cfl, s->max_bits);
    double max_CFL = 0.0;
    HIPCHK(hipMemcpyAsync(&max_CFL, s->max_bits, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the count decides the launches
    { const int rc = comm_allreduce_scalar(c, &max_CFL, 1); if (rc) return rc; }   // max_across_PEs
    REQUIRE(max_CFL < 1.0e6, MOM6X_EINVAL, "tracer_hordiff: the diffusive CFL number asks for more than a million iterations");
    num_itts = (int)ceil(max_CFL - 4.0 * DBL_EPSILON);
    if (num_itts < 1) num_itts = 1;
  } else if (P.max_diff_CFL > 0.0) {
    REQUIRE(P.max_diff_CFL < 1.0e6, MOM6X_EINVAL, "tracer_hordiff: MAX_TR_DIFFUSION_CFL asks for more than a million iterations");
    num_itts = (int)ceil(P.max_diff_CFL - 4.0 * DBL_EPSILON);
    if (num_itts < 1) num_itts = 1;
  }
  const double I_numitts = 1.0 / (double)num_itts, Idt = 1.0 / dt;
  if (num_itts_out) *num_itts_out = num_itts;
  plan->khx = khx; plan->khy = khy; plan->num_itts = num_itts; plan->I_numitts = I_numitts; plan->Idt = Idt;
  return MOM6X_OK;
}

extern "C" int mom6x_tracer_hordiff(mom6x_ctx *c, const double *h, double dt, double *const *tracers, const double *conc_underflow,
                                    int ntr, const double *L2u, const double *SN_u, const double *L2v, const double *SN_v,
                                    const double *Res_fn_h, const double *Rd_dx_h, const double *MEKE_Kh, double *const *df_x,
                                    double *const *df_y, double *khdt_x_out, double *khdt_y_out, double *cfl_out, int *num_itts_out) {
  REQUIRE(c && c->thd, MOM6X_EINVAL, "MOM_tracer_hor_diff: tracer_hor_diff_init must be called before tracer_hordiff.");
  ThdState *s = c->thd;
  const mom6x_tracer_hor_diff_params &P = s->P;
  REQUIRE(ntr >= 0, MOM6X_EINVAL, "tracer_hordiff: negative tracer count");
  if (num_itts_out) *num_itts_out = 0;
  if (ntr == 0 || (P.KhTr <= 0.0 && !P.use_variable_mixing)) return MOM6X_OK;   // :199
  REQUIRE(h && tracers, MOM6X_EINVAL, "tracer_hordiff: null array");
  for (int m = 0; m < ntr; m++) REQUIRE(tracers[m], MOM6X_EINVAL, "tracer_hordiff: null tracer array");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "tracer_hordiff: dt must be positive");
  ThdPlan plan;
  if (const int rc = thd_khdt_and_itts(c, s, dt, L2u, SN_u, L2v, SN_v, Res_fn_h, Rd_dx_h, MEKE_Kh, khdt_x_out, khdt_y_out, cfl_out, num_itts_out,
                                       &plan)) return rc;
  const Dm d = c->d;
  double *khx = plan.khx, *khy = plan.khy;
  const int num_itts = plan.num_itts;
  const double I_numitts = plan.I_numitts, Idt = plan.Idt;

  // The kernel carries up to HD_MAXT tracers through one pass over h and the coefficients; a longer registry goes HD_MAXT at a
  // time, each group through all iterations: tracers do not interact, so every tracer gets the bits of one pass.
  c->halo_error = false;
  for (int m0 = 0; m0 < ntr; m0 += HD_MAXT) {
    HdList L;
    L.n = (ntr - m0 < HD_MAXT) ? (ntr - m0) : HD_MAXT;
    bool any_df = false;
    int stg[HD_MAXT], nks[HD_MAXT];
    for (int m = 0; m < HD_MAXT; m++) {
      const bool on = m < L.n;
      L.t[m] = on ? tracers[m0 + m] : nullptr;
      L.dfx[m] = (on && df_x) ? df_x[m0 + m] : nullptr;
      L.dfy[m] = (on && df_y) ? df_y[m0 + m] : nullptr;
      L.underflow[m] = (on && conc_underflow) ? conc_underflow[m0 + m] : 0.0;
      any_df = any_df || L.dfx[m] || L.dfy[m];
      stg[m] = 0; nks[m] = d.nk;
    }
    const dim3 g(s->ntx, s->nseg, d.nk);
    for (int itt = 0; itt < num_itts; itt++) {
      halo_wrap(c, L.t, stg, nks, L.n);                                        // do_group_pass(CS%pass_t) :545
      KLAUNCH(c, "k_thd_save_x", k_thd_save_x, dim3((d.nj + 255) / 256, s->ntx + 1, d.nk), dim3(256), d, L, s->save_x, s->ntx);
      KLAUNCH(c, "k_thd_save_y", k_thd_save_y, dim3((d.ni + 255) / 256, s->nseg + 1, d.nk), dim3(256), d, L, s->save_y, s->nseg);
#define THD(M, DF)                                                                                                                  \
  KLAUNCH(c, "k_thd_tile<" #M "," #DF ">", (k_thd_tile<M, DF>), g, dim3(256), d, c->G, h, L, (const double *)khx, (const double *)khy, \
          (const double *)s->save_x, (const double *)s->save_y, I_numitts, c->GV.H_subroundoff, Idt, (int)(itt == 0), s->ntx, s->nseg)
#define THD_M(M) do { if (any_df) THD(M, true); else THD(M, false); } while (0)
      if (L.n <= 1) THD_M(1); else if (L.n <= 2) THD_M(2); else if (L.n <= 4) THD_M(4); else THD_M(8);
#undef THD_M
#undef THD
    }
  }
  HIPCHK(hipGetLastError());
  REQUIRE(!c->halo_error, MOM6X_EHIP, mom6x_last_error());
  return MOM6X_OK;
}

namespace {

// Coef_x(I,j,K) = I_numitts * khdt_x(I,j) and Coef_y(i,J,K) = I_numitts * khdt_y(i,J) on all nk + 1 planes, :494-507
__global__ void __launch_bounds__(256)
k_thd_ndiff_coef(Dm d, double I_numitts, const double *__restrict__ khdt_x, const double *__restrict__ khdt_y, double *__restrict__ Coef_x,
                 double *__restrict__ Coef_y) {
  const FaceLane f = face_lane<0>(d);
  if (!f.in) return;
  const double coef = I_numitts * (f.dir ? khdt_y : khdt_x)[f.x];
  double *Coef = f.dir ? Coef_y : Coef_x;
  for (int K = 0; K <= d.nk; K++) Coef[f.x + (size_t)K * (size_t)d.slab] = coef;
}

}  // namespace

// The neutral branch :479-539.  The registry's group pass is the context's, as in mom6x_tracer_hordiff.
extern "C" int mom6x_tracer_hordiff_neutral(mom6x_ctx *c, const double *h, double dt, double *const *tracers, const double *conc_underflow,
                                            int ntr, const double *L2u, const double *SN_u, const double *L2v, const double *SN_v,
                                            const double *Res_fn_h, const double *Rd_dx_h, const double *MEKE_Kh, const double *T,
                                            const double *S, const double *p_surf, double *const *tendency, double *const *trans_x_2d,
                                            double *const *trans_y_2d, double *khdt_x_out, double *khdt_y_out, double *cfl_out,
                                            int *num_itts_out) {
  REQUIRE(c && c->thd, MOM6X_EINVAL, "MOM_tracer_hor_diff: tracer_hor_diff_init must be called before tracer_hordiff_neutral.");
  REQUIRE(neutral_diffusion_ready(c), MOM6X_EINVAL, "tracer_hordiff_neutral: neutral_diffusion_init must be called first");
  ThdState *s = c->thd;
  const mom6x_tracer_hor_diff_params &P = s->P;
  REQUIRE(ntr >= 0, MOM6X_EINVAL, "tracer_hordiff_neutral: negative tracer count");
  if (num_itts_out) *num_itts_out = 0;
  if (ntr == 0 || (P.KhTr <= 0.0 && !P.use_variable_mixing)) return MOM6X_OK;   // :199
  REQUIRE(h && tracers && T && S, MOM6X_EINVAL, "tracer_hordiff_neutral: null array");
  for (int m = 0; m < ntr; m++) REQUIRE(tracers[m], MOM6X_EINVAL, "tracer_hordiff_neutral: null tracer array");
  REQUIRE(dt > 0.0, MOM6X_EINVAL, "tracer_hordiff_neutral: dt must be positive");
  ThdPlan plan;
  if (const int rc = thd_khdt_and_itts(c, s, dt, L2u, SN_u, L2v, SN_v, Res_fn_h, Rd_dx_h, MEKE_Kh, khdt_x_out, khdt_y_out, cfl_out, num_itts_out,
                                       &plan)) return rc;
  const Dm d = c->d;
  std::vector<int> stg(ntr, 0), nks(ntr, d.nk);
  c->halo_error = false;
  halo_wrap(c, tracers, stg.data(), nks.data(), ntr);                            // do_group_pass(CS%pass_t) :483
  if (const int rc = mom6x_neutral_diffusion_calc_coeffs(c, h, T, S, p_surf)) return rc;
  double *Coef_x, *Coef_y;
  neutral_diffusion_coef_arrays(c, &Coef_x, &Coef_y);
  const dim3 b = blk2();
  KLAUNCH(c, "k_thd_ndiff_coef", k_thd_ndiff_coef, grid3(d.ni + IAL, d.nj + 1, 2, b), b, d, plan.I_numitts, (const double *)plan.khx,
          (const double *)plan.khy, Coef_x, Coef_y);
  for (int itt = 0; itt < plan.num_itts; itt++) {
    if (itt > 0) {
      halo_wrap(c, tracers, stg.data(), nks.data(), ntr);                        // :528
      if (neutral_diffusion_recalc(c)) {
        if (const int rc = mom6x_neutral_diffusion_calc_coeffs(c, h, T, S, p_surf)) return rc;
      }
    }
    if (const int rc = mom6x_neutral_diffusion(c, h, Coef_x, Coef_y, plan.I_numitts * dt, tracers, conc_underflow, ntr, tendency,
                                               trans_x_2d, trans_y_2d)) return rc;
  }
  HIPCHK(hipGetLastError());
  REQUIRE(!c->halo_error, MOM6X_EHIP, mom6x_last_error());
  return MOM6X_OK;
}
