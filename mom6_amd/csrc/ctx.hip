// ctx.hip -- context, layout and host<->device transfer entry points of the C ABI.
#include <cstdarg>
#include <vector>
#include "mom6x_dev.h"
#include <cstdlib>

#include <map>
static thread_local char g_err[512] = "";

struct ProfRec { int id; hipEvent_t a, b; };
struct Prof {
  std::vector<std::string> names;
  std::map<std::string, int> ids;
  std::vector<ProfRec> recs;
  std::vector<double> ms;
  std::vector<long> count;
  std::vector<hipEvent_t> pool;
  hipEvent_t cur_a;
  int cur_id;
  std::string filter;   // record only kernels whose name starts with this prefix ("" = all)
};

static hipEvent_t prof_event(Prof *p) {
  if (!p->pool.empty()) { hipEvent_t e = p->pool.back(); p->pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

extern "C" int mom6x_prof_filter(mom6x_ctx *c, const char *prefix) {
  REQUIRE(c, MOM6X_EINVAL, "mom6x_prof_filter: null ctx");
  if (!c->prof) c->prof = new Prof();
  c->prof->filter = prefix ? prefix : "";
  return MOM6X_OK;
}

void prof_begin(mom6x_ctx *c, const char *name) {
  Prof *p = c->prof;
  p->cur_id = -1;
  if (!p->filter.empty() && strncmp(name, p->filter.c_str(), p->filter.size()) != 0) return;
  auto it = p->ids.find(name);
  int id;
  if (it == p->ids.end()) {
    id = (int)p->names.size();
    p->names.push_back(name); p->ids[name] = id; p->ms.push_back(0.0); p->count.push_back(0);
  } else id = it->second;
  p->cur_id = id;
  p->cur_a = prof_event(p);
  (void)hipEventRecord(p->cur_a, c->stream);
}

void prof_end(mom6x_ctx *c) {
  Prof *p = c->prof;
  if (p->cur_id < 0) return;
  ProfRec r; r.id = p->cur_id; r.a = p->cur_a; r.b = prof_event(p);
  (void)hipEventRecord(r.b, c->stream);
  p->recs.push_back(r);
}

static void prof_collect(mom6x_ctx *c) {
  Prof *p = c->prof;
  (void)hipStreamSynchronize(c->stream);
  for (auto &r : p->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { p->ms[r.id] += ms; p->count[r.id] += 1; }
    p->pool.push_back(r.a); p->pool.push_back(r.b);
  }
  p->recs.clear();
}

static void prof_free(mom6x_ctx *c) {
  Prof *p = c->prof;
  if (!p) return;
  for (auto &r : p->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (hipEvent_t e : p->pool) (void)hipEventDestroy(e);
  delete p;
  c->prof = nullptr;
}

extern "C" int mom6x_prof_enable(mom6x_ctx *c, int on) {
  REQUIRE(c, MOM6X_EINVAL, "mom6x_prof_enable: null ctx");
  HIPCHK(hipSetDevice(c->device));
  if (!c->prof) c->prof = new Prof();
  if (!on && c->prof_on) prof_collect(c);
  c->prof_on = (on != 0);
  return MOM6X_OK;
}

extern "C" int mom6x_prof_reset(mom6x_ctx *c) {
  REQUIRE(c, MOM6X_EINVAL, "mom6x_prof_reset: null ctx");
  if (!c->prof) return MOM6X_OK;
  prof_collect(c);
  for (auto &m : c->prof->ms) m = 0.0;
  for (auto &n : c->prof->count) n = 0;
  return MOM6X_OK;
}

// Writes "name\tcount\ttotal_ms\n" lines into buf; returns the number of bytes needed.
extern "C" int mom6x_prof_report(mom6x_ctx *c, char *buf, int buflen) {
  if (!c || !c->prof) { if (buf && buflen > 0) buf[0] = 0; return 0; }
  prof_collect(c);
  std::string out;
  char line[256];
  for (size_t i = 0; i < c->prof->names.size(); i++) {
    snprintf(line, sizeof(line), "%s\t%ld\t%.6f\n", c->prof->names[i].c_str(), c->prof->count[i], c->prof->ms[i]);
    out += line;
  }
  if (buf && buflen > 0) { strncpy(buf, out.c_str(), (size_t)buflen - 1); buf[buflen - 1] = 0; }
  return (int)out.size() + 1;
}

void mom6x_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *mom6x_last_error(void) { return g_err; }
extern "C" int mom6x_abi_version(void) { return MOM6X_ABI_VERSION; }

// the work-group and the first lane of the one-lane-per-face kernels (mom6x_dev.h), for tests that place a grid's edges around them
extern "C" int mom6x_lane_launch_shape(int *bx, int *by, int *i_first) {
  if (bx) *bx = LANE_BX;
  if (by) *by = LANE_BY;
  if (i_first) *i_first = -IAL;
  return MOM6X_OK;
}

// the steps of the tiled kernels of the dynamics, for tests that place a grid's edges on a whole number of tiles and one point more:
// which = 0 CorAdCalc (k_corad_lds, k_corad_fused), 1 horizontal_viscosity (k_hv_fused), 2 advect_tracer (cells of an x tile, rows
// of a y segment)
extern "C" int mom6x_tile_steps(int which, int *sx, int *sy) {
  REQUIRE(which >= 0 && which <= 2, MOM6X_EINVAL, "mom6x_tile_steps: which must be 0 (CorAdCalc), 1 (hor_visc) or 2 (tracer advection)");
  int x = 0, y = 0;
  if (which == 0) corad_tile_steps(&x, &y);
  else if (which == 1) hor_visc_tile_steps(&x, &y);
  else tracer_advect_tile_steps(&x, &y);
  if (sx) *sx = x;
  if (sy) *sy = y;
  return MOM6X_OK;
}

extern "C" int mom6x_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { mom6x_set_error("mom6x_device_count: hipGetDeviceCount failed"); return -1; }
  return n;
}

// sizeof() of the public structs, so that non-C hosts (ctypes, ISO_C_BINDING) can verify their mirrors.
extern "C" int mom6x_struct_size(int which) {
  switch (which) {
    case 0: return (int)sizeof(mom6x_dims);
    case 1: return (int)sizeof(mom6x_vgrid);
    case 2: return (int)sizeof(mom6x_continuity_params);
    case 3: return (int)sizeof(mom6x_BT_cont);
    case 4: return (int)sizeof(mom6x_barotropic_params);
    case 5: return (int)sizeof(mom6x_coriolis_params);
    case 6: return (int)sizeof(mom6x_pgf_params);
    case 7: return (int)sizeof(mom6x_rk2_params);
    case 8: return (int)sizeof(mom6x_rk2_hooks);
    case 9: return (int)sizeof(mom6x_eos_params);
    case 10: return (int)sizeof(mom6x_vertvisc_params);
    case 11: return (int)sizeof(mom6x_hor_visc_params);
    case 12: return (int)sizeof(mom6x_remapping_params);
    case 13: return (int)sizeof(mom6x_regrid_zstar_params);
    case 14: return (int)sizeof(mom6x_chksum_result);
    case 15: return (int)sizeof(mom6x_sum_output_params);
    case 16: return (int)sizeof(mom6x_energy_sums);
    case 17: return (int)sizeof(mom6x_regrid_rho_params);
    case 18: return (int)sizeof(mom6x_set_visc_params);
    case 19: return (int)sizeof(mom6x_thickness_diffuse_params);
    case 20: return (int)sizeof(mom6x_tracer_hor_diff_params);
    case 21: return (int)sizeof(mom6x_varmix_params);
    case 22: return (int)sizeof(mom6x_mixedlayer_restrat_params);
    case 23: return (int)sizeof(mom6x_MEKE_params);
    case 25: return (int)sizeof(mom6x_set_diffusivity_params);
    case 27: return (int)sizeof(mom6x_diabatic_aux_params);
    case 28: return (int)sizeof(mom6x_surface_fluxes);
    case 30: return (int)sizeof(mom6x_energetic_PBL_params);
    case 32: return (int)sizeof(mom6x_frazil_params);
    case 33: return (int)sizeof(mom6x_geothermal_params);
    case 34: return (int)sizeof(mom6x_opacity_params);
    case 35: return (int)sizeof(mom6x_kappa_shear_params);
    case 36: return (int)sizeof(mom6x_neutral_diffusion_params);
    default: return -1;
  }
}

extern "C" int mom6x_dims_init(mom6x_dims *d, int ni, int nj, int nk, int halo) {
  REQUIRE(d && ni > 0 && nj > 0 && nk > 0, MOM6X_EINVAL, "mom6x_dims_init: bad sizes");
  REQUIRE(halo >= 1 && halo + 1 <= 16, MOM6X_EINVAL, "mom6x_dims_init: halo must be in 1..15");
  d->ni = ni; d->nj = nj; d->nk = nk; d->halo = halo;
  d->ioff = 16;               // local i = 0 starts a 128-byte line
  d->joff = halo + 1;
  d->pitch = ((d->ioff + ni + halo + 15) / 16) * 16;
  d->slab = d->pitch * (nj + 2 * halo + 1);
  d->i_glob0 = 0; d->j_glob0 = 0; d->ni_glob = ni; d->nj_glob = nj;
  d->reentrant_x = 0; d->reentrant_y = 0;
  return MOM6X_OK;
}

// the streams and arrays of a context whose members are otherwise set (on failure mom6x_ctx_create destroys what there is)
static int ctx_alloc(mom6x_ctx *c, const double *metrics_host) {
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&c->halo_stream, hipStreamNonBlocking));
  const size_t nG = (size_t)MOM6X_G_COUNT * c->dims.slab;
  HIPCHK(hipMalloc(&c->G, nG * sizeof(double)));
  HIPCHK(hipMemcpy(c->G, metrics_host, nG * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&c->flag, sizeof(int)));
  HIPCHK(hipMemset(c->flag, 0, sizeof(int)));
  return MOM6X_OK;
}

extern "C" int mom6x_ctx_create(mom6x_ctx **out, const mom6x_dims *dims, int device,
                                const double *metrics_host, const mom6x_vgrid *GV,
                                int first_direction) {
  REQUIRE(out && dims && metrics_host && GV, MOM6X_EINVAL, "mom6x_ctx_create: null argument");
  REQUIRE(dims->halo >= 3, MOM6X_EINVAL, "mom6x_ctx_create: halo >= 3 is required by continuity_PPM");
  REQUIRE(dims->ioff >= dims->halo + 1 && dims->joff >= dims->halo + 1 &&
          dims->pitch >= dims->ioff + dims->ni + dims->halo &&
          dims->slab == dims->pitch * (dims->nj + 2 * dims->halo + 1),
          MOM6X_EINVAL, "mom6x_ctx_create: inconsistent layout in dims");
  REQUIRE(GV->Boussinesq == 1, MOM6X_EUNSUPPORTED, "mom6x: only BOUSSINESQ=True is supported");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  REQUIRE(ndev > 0 && device >= 0 && device < ndev, MOM6X_EHIP,
          "mom6x_ctx_create: no such HIP device (the product path has no CPU fallback)");
  HIPCHK(hipSetDevice(device));
  mom6x_ctx *c = new mom6x_ctx();   // (all members zero: no stream, no array, no module state)
  c->dims = *dims;
  c->d = make_dm(*dims);
  c->device = device;
  c->GV = *GV;
  c->first_direction = first_direction;
  const int rc = ctx_alloc(c, metrics_host);
  if (rc) { (void)mom6x_ctx_destroy(c); return rc; }
  *out = c;
  return MOM6X_OK;
}

extern "C" int mom6x_ctx_destroy(mom6x_ctx *c) {
  if (!c) return MOM6X_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->halo_stream) (void)hipStreamSynchronize(c->halo_stream);
  bt_state_free(c);    // (before the step's: with no barotropic state left, a deferred btcalc is dropped, not completed)
  rk2_state_free(c);
  continuity_free(c);
  CoriolisAdv_free(c);
  PressureForce_free(c);
  vertvisc_free(c);
  hor_visc_free(c);
  ALE_free(c);
  ta_state_free(c);
  diag_sums_free(c);
  set_visc_free(c);
  thickness_diffuse_free(c);
  tracer_hor_diff_free(c);
  varmix_free(c);
  mixedlayer_restrat_free(c);
  MEKE_free(c);
  set_diffusivity_free(c);
  diabatic_aux_free(c);
  energetic_PBL_free(c);
  diabatic_TS_free(c);
  opacity_free(c);
  kappa_shear_free(c);
  neutral_diffusion_free(c);
  comm_free(c);
  for (int m = 0; m < MOM6X_NSCR; m++) (void)hipFree(c->scr[m]);
  (void)hipFree(c->G); (void)hipFree(c->flag);
  if (c->ev_ready) { (void)hipEventDestroy(c->ev_ready); (void)hipEventDestroy(c->ev_done); }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->halo_stream) (void)hipStreamDestroy(c->halo_stream);
  prof_free(c);
  delete c;
  return MOM6X_OK;
}

// The reference's test.nan (.testing/Makefile:399-408: every allocation initialised with signalling NaNs): with MOM6X_POISON_WORK=1 in
// the environment the WORK arrays of the device -- the scratch slots, the PPM edge arrays, the tracer advection's remainders, whatever a
// host asks mom6x_dev_alloc for -- start as NaNs (all bits set) instead of zeros.  A step that reads a word of them it has not
// written differs from the un-poisoned run or trips the numeric flag (tests/test_invariants_gpu.py).  Arrays the reference zeroes
// explicitly after allocating them (the restart fields of the RK2 and barotropic modules) are not work arrays.
int work_fill_byte() {
  const char *e = getenv("MOM6X_POISON_WORK");   // (read at every allocation: a test switches it between two models of one process)
  return (e && atoi(e) != 0) ? 0xFF : 0;
}

int ctx_scratch(mom6x_ctx *c, int slot, int nlev, double **out) {
  REQUIRE(slot >= 0 && slot < MOM6X_NSCR, MOM6X_EINVAL, "ctx_scratch: bad slot");
  if (c->scr[slot] && c->scr_nlev[slot] < nlev) { HIPCHK(hipFree(c->scr[slot])); c->scr[slot] = nullptr; }
  if (!c->scr[slot]) {
    const size_t n = (size_t)c->dims.slab * nlev;
    HIPCHK(hipMalloc(&c->scr[slot], n * sizeof(double)));
    HIPCHK(hipMemsetAsync(c->scr[slot], work_fill_byte(), n * sizeof(double), c->stream));
    c->scr_nlev[slot] = nlev;
  }
  *out = c->scr[slot];
  return MOM6X_OK;
}

extern "C" void *mom6x_ctx_stream(mom6x_ctx *c) { return (void *)c->stream; }
extern "C" const mom6x_dims *mom6x_ctx_dims(const mom6x_ctx *c) { return &c->dims; }
extern "C" const double *mom6x_ctx_metrics_dev(const mom6x_ctx *c) { return c->G; }

extern "C" int mom6x_ctx_sync(mom6x_ctx *c) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->halo_stream));
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, c->flag, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) {
    HIPCHK(hipMemset(c->flag, 0, sizeof(int)));
    if (flag & MOM6X_FLAG_NEUTRAL_DIFFUSION)
      mom6x_set_error("device-side numeric error flag = %d (bit %d: neutral diffusion reached one of the reference's stop sites, "
                      "MOM_neutral_diffusion.F90:1203, :1205, :1426, :1428, :1616, see mom6x_neutral_diffusion_status; other bits: NaN or "
                      "negative thickness)", flag, MOM6X_FLAG_NEUTRAL_DIFFUSION);
    else if (flag & MOM6X_FLAG_MEKE_EQUILIBRIUM)
      mom6x_set_error("device-side numeric error flag = %d (bit %d: MEKE_equilibrium found no bracket below 2e17 m2 s-2 or did not "
                      "converge in 200 bisections, MOM_MEKE.F90:1095, :1133; other bits: NaN or negative thickness)", flag,
                      MOM6X_FLAG_MEKE_EQUILIBRIUM);
    else
      mom6x_set_error("device-side numeric error flag = %d (NaN or negative thickness)", flag);
    return MOM6X_ENUMERIC;
  }
  return MOM6X_OK;
}

extern "C" int mom6x_dev_alloc(mom6x_ctx *c, double **p, size_t n) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMalloc(p, n * sizeof(double)));
  HIPCHK(hipMemsetAsync(*p, work_fill_byte(), n * sizeof(double), c->stream));
  return MOM6X_OK;
}
// device -> device on the context's stream (the Fortran shims: a result that lands in a scratch slot although its host array is resident)
extern "C" int mom6x_dev_copy(mom6x_ctx *c, double *dst, const double *src, size_t n) {
  REQUIRE(c && dst && src, MOM6X_EINVAL, "mom6x_dev_copy: null argument");
  HIPCHK(hipSetDevice(c->device));
  if (dst != src) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return MOM6X_OK;
}
extern "C" int mom6x_dev_free(mom6x_ctx *c, double *p) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipFree(p));
  return MOM6X_OK;
}

// Fortran symmetric-memory extents of the four staggerings (MOM_memory_macros.h, dynamic
// symmetric branch): h (isd:ied, jsd:jed), u (isd-1:ied, jsd:jed), v (isd:ied, jsd-1:jed),
// q (isd-1:ied, jsd-1:jed).
static void f_extent(const mom6x_dims &d, int stagger, int &nx, int &ny, int &i0, int &j0) {
  const int xB = (stagger == 1 || stagger == 3), yB = (stagger == 2 || stagger == 3);
  nx = d.ni + 2 * d.halo + xB; ny = d.nj + 2 * d.halo + yB;
  i0 = -d.halo - xB; j0 = -d.halo - yB;
}

static int xfer(mom6x_ctx *c, double *dev, double *host, int stagger, int nk, bool up) {
  REQUIRE(stagger >= 0 && stagger <= 3 && nk >= 1, MOM6X_EINVAL, "mom6x_upload/download: bad stagger or nk");
  HIPCHK(hipSetDevice(c->device));
  const mom6x_dims &d = c->dims;
  int nx, ny, i0, j0;
  f_extent(d, stagger, nx, ny, i0, j0);
  const int nrows = d.nj + 2 * d.halo + 1;
  hipMemcpy3DParms p;
  memset(&p, 0, sizeof(p));
  hipPitchedPtr hp = make_hipPitchedPtr(host, (size_t)nx * sizeof(double), nx, ny);
  hipPitchedPtr dp = make_hipPitchedPtr(dev, (size_t)d.pitch * sizeof(double), d.pitch, nrows);
  hipPos hpos = make_hipPos(0, 0, 0);
  hipPos dpos = make_hipPos((size_t)(i0 + d.ioff) * sizeof(double), (size_t)(j0 + d.joff), 0);
  if (up) { p.srcPtr = hp; p.srcPos = hpos; p.dstPtr = dp; p.dstPos = dpos; p.kind = hipMemcpyHostToDevice; }
  else    { p.srcPtr = dp; p.srcPos = dpos; p.dstPtr = hp; p.dstPos = hpos; p.kind = hipMemcpyDeviceToHost; }
  p.extent = make_hipExtent((size_t)nx * sizeof(double), ny, nk);
  HIPCHK(hipMemcpy3DAsync(&p, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MOM6X_OK;
}

extern "C" int mom6x_upload(mom6x_ctx *c, double *dev, const double *host_f, int stagger, int nk) {
  return xfer(c, dev, const_cast<double *>(host_f), stagger, nk, true);
}
extern "C" int mom6x_download(mom6x_ctx *c, double *host_f, const double *dev, int stagger, int nk) {
  return xfer(c, const_cast<double *>(dev), host_f, stagger, nk, false);
}
