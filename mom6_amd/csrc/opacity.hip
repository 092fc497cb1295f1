// opacity.hip -- the shortwave optics of the water column on gfx950: set_pen_shortwave of MOM_diabatic_aux with set_opacity of
// MOM_opacity, the producer of optics%opacity_band and optics%sw_pen_band that applyBoundaryFluxesInOut (diabatic_aux.hip) reads.
//
//   mom6x_opacity_init   <- opacity_init, MOM_opacity.F90:1151-1160 (the band-count rules), :1243-1283 (coefficients per band,
//                           chl_dep_bands, the fold of a coefficient with zero power), :1310-1313 with init_ohlmann_table :1321-1430
//   k_opacity_cols       <- set_pen_shortwave, MOM_diabatic_aux.F90:621-677 (the negative-chlorophyll test :649 as a counter);
//                           set_opacity, MOM_opacity.F90:118-240 (the exponential arms :152-193, the diagnostics :197-237);
//                           opacity_from_chl :245-477; opacity_morel and SW_pen_frac_morel :481-513; lookup_ohlmann_swpen and
//                           lookup_ohlmann_opacity :1433-1485; the product of extract_optics_slice :559
//
// One lane per column of the computational domain, consecutive lanes along i, one launch per call.  The lane reads mask2dT, the
// shortwave planes and the chlorophyll of its column once, forms sw_pen_band and then walks down the layers storing nbands words
// per layer, each store coalesced across the wavefront.  With chl_2d or without chlorophyll the reference evaluates the same
// expression with the same operands at every layer: the lane evaluates it once, which gives the same bits and leaves one pow (or
// log10) per band and column instead of one per band and cell.  With chl_3d the layer's chlorophyll is loaded PF layers ahead of
// its use and the transcendental is evaluated per cell, as in the reference.
//
// Where the reference stops on a negative chlorophyll (MOM_diabatic_aux.F90:649, MOM_opacity.F90:328, :338) the lane counts and
// stores what the formulas give: see include/mom6x.h.  No contraction (the build's -ffp-contract=off); every sum keeps the
// reference's association.
#include "mom6x_dev.h"

#define OP_NLUT 401   // nval_lut, MOM_opacity.F90:1389
#define OP_PF 4       // layers by which the load of chl_3d runs ahead of its use

namespace {

// the scalars of a call, formed on the host in the reference's order
struct OpK {
  double c1[4], c2[4], pw[4];       // CS%opacity_coef(1:2,n), CS%chl_power(n) (MANIZZA_05)
  double mo[6], mp[6];              // CS%opacity_coef(1:6,1), CS%sw_pen_frac_coef (MOREL_88)
  double blue_frac, one_m_blue;     // :369, :372
  double land;                      // CS%opacity_land_value
  double inv_scale, inv_scale_2nd;  // :157, :163
  double ratio1, one_m_ratio1;      // :174, :175
  double frac_inv_nbands;           // CS%pen_SW_frac * Inv_nbands :190
  double Inv_nbands, Inv_nbands_nir;   // :304-308
  double Z_to_m;                    // :469
  double op_diag_len;               // :228
  double opacity_scale;             // extract_optics_slice :549
  double chl_min, log10chl_min, log10chl_max, dlog10chl;   // :1400-1403
  int nbands, chl_dep_bands;
  int vis_in, nir_in, tot_in;       // multiband_vis_input, multiband_nir_input, total_sw_input :320-322
  int pen_zero;                     // .not.associated(sw_total) .or. (CS%pen_SW_scale <= 0.0) :166, :182
};
struct OpP {
  const double *sw, *vis_dir, *vis_dif, *nir_dir, *nir_dif, *chl_2d, *chl_3d, *lut;
  double *opacity_band, *sw_pen_band, *SW_pen, *SW_vis_pen, *opac_diag;
  unsigned long long *cnt;
};

// Chl of opacity_morel :488 and SW_pen_frac_morel :509
__device__ __forceinline__ double morel_log10chl(double chl) { return log10(fmin1(fmax1(chl, 0.02), 60.0)); }
__device__ __forceinline__ double morel_poly(const double *c, double Chl) {   // the nesting of :490-492 and :510-512
  const double Chl2 = Chl * Chl;
  return (c[0] + c[1] * Chl) + Chl2 * ((c[2] + Chl * c[3]) + Chl2 * (c[4] + Chl * c[5]));
}
// the 0-based table entry of lookup_ohlmann_swpen | _opacity :1447-1453; nint rounds a half away from zero, as round does
__device__ __forceinline__ int ohlmann_index(const OpK &K, double chl) {
  double log10chl;
  if (chl > K.chl_min) log10chl = fmin1(log10(chl), K.log10chl_max);
  else log10chl = K.log10chl_min;
  int n = (int)round((log10chl - K.log10chl_min) / K.dlog10chl);
  return n < 0 ? 0 : (n > OP_NLUT - 1 ? OP_NLUT - 1 : n);   // (never taken by a finite table: keeps the load inside it)
}

// the opacities of the bands from one chlorophyll value, before opacity_scale
template <int SCH>
__device__ __forceinline__ void band_opacities(const OpK &K, const double *__restrict__ lut, double mask, double chl, double (&op)[4]) {
  if constexpr (SCH == MOM6X_OPACITY_MANIZZA_05) {   // :436-451
    if (mask <= 0.5) {
#pragma unroll
      for (int n = 0; n < 4; ++n) op[n] = K.land;
    } else {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if (n < K.chl_dep_bands) op[n] = K.c1[n] + K.c2[n] * pow(chl, K.pw[n]);
        else op[n] = K.c1[n];
      }
    }
  } else if constexpr (SCH == MOM6X_OPACITY_MOREL_88) {   // :453-461
    double o = K.land;
    if (mask > 0.0) o = 1.0 / morel_poly(K.mo, morel_log10chl(chl));
#pragma unroll
    for (int n = 0; n < 4; ++n) op[n] = o;
  } else {   // OHLMANN_03 :464-471
    if (mask <= 0.5) {
      op[0] = K.land; op[1] = K.land;
    } else {
      const int m = ohlmann_index(K, chl);
      op[0] = lut[2 * OP_NLUT + m] * K.Z_to_m;
      op[1] = lut[3 * OP_NLUT + m] * K.Z_to_m;
    }
    op[2] = op[3] = 0.0;
  }
}

// one layer's stores: the product :559 into opacity_band, the remapped opacity :234 into the diagnostic
__device__ __forceinline__ void store_layer(const OpK &K, const OpP &P, size_t o, size_t band, const double (&op)[4]) {
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (n < K.nbands) {
      P.opacity_band[(size_t)n * band + o] = K.opacity_scale * op[n];
      if (P.opac_diag) P.opac_diag[(size_t)n * band + o] = tanh(K.op_diag_len * op[n]) / K.op_diag_len;
    }
}

// SCH: enum mom6x_opacity_scheme.  CHL: 0 no chlorophyll (the exponential schemes), 1 chl_2d, 2 chl_3d
template <int SCH, int CHL>
__global__ void __launch_bounds__(256) k_opacity_cols(Dm d, const double *__restrict__ G, OpK K, OpP P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= d.ni || j >= d.nj) return;
  const size_t x = ix2(d, i, j), slab = (size_t)d.slab, band = slab * (size_t)d.nk;
  const int nz = d.nk;
  const double mask = gm(G, d, MOM6X_G_mask2dT)[x];

  double chl = 0.0;   // chl_data of the surface: chl_2d, or chl_3d(:,:,1) :326
  double buf[OP_PF];
  if constexpr (CHL == 1) {
    chl = P.chl_2d[x];
    if ((mask > 0.0) && (chl < 0.0)) atomicAdd(P.cnt, 1ull);   // :338, MOM_diabatic_aux.F90:649
  }
  if constexpr (CHL == 2) {
#pragma unroll
    for (int q = 0; q < OP_PF; ++q) buf[q] = q < nz ? P.chl_3d[(size_t)q * slab + x] : 0.0;
    chl = buf[0];
  }

  // optics%sw_pen_band
  double pen[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (SCH == MOM6X_OPACITY_MANIZZA_05) {   // :352-377
    double SW_vis_tot = 0.0, SW_nir_tot = 0.0;
    if (mask > 0.0) {
      if (K.vis_in) SW_vis_tot = P.vis_dir[x] + P.vis_dif[x];
      else if (K.tot_in) SW_vis_tot = 0.42 * P.sw[x];
      if (K.nir_in) SW_nir_tot = P.nir_dir[x] + P.nir_dif[x];
      else if (K.tot_in) SW_nir_tot = P.sw[x] - SW_vis_tot;
    }
    pen[0] = K.blue_frac * SW_vis_tot;
    pen[1] = K.one_m_blue * SW_vis_tot;
    pen[2] = K.Inv_nbands_nir * SW_nir_tot;
    pen[3] = pen[2];
  } else if constexpr (SCH == MOM6X_OPACITY_MOREL_88) {   // :380-393
    double SW_pen_tot = 0.0;
    if (mask > 0.0) {
      if (K.vis_in) SW_pen_tot = (1.0 - morel_poly(K.mp, morel_log10chl(chl))) * (P.vis_dir[x] + P.vis_dif[x]);
      else if (K.tot_in) SW_pen_tot = (1.0 - morel_poly(K.mp, morel_log10chl(chl))) * 0.5 * P.sw[x];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) pen[n] = K.Inv_nbands * SW_pen_tot;
  } else if constexpr (SCH == MOM6X_OPACITY_OHLMANN_03) {   // :400-416
    if (!(mask < 0.5)) {
      double SW_vis_tot;
      if (K.vis_in) SW_vis_tot = ((P.vis_dir[x] + P.vis_dif[x]) + P.nir_dir[x]) + P.nir_dif[x];
      else SW_vis_tot = P.sw[x];
      const int m = ohlmann_index(K, chl);
      pen[0] = P.lut[m] * SW_vis_tot;
      pen[1] = P.lut[OP_NLUT + m] * SW_vis_tot;
    }
  } else if constexpr (SCH == MOM6X_OPACITY_DOUBLE_EXP) {   // :166-177
    if (!K.pen_zero) {
      const double s = P.sw[x];
      pen[0] = K.ratio1 * s;
      pen[1] = K.one_m_ratio1 * s;
    }
  } else {   // SINGLE_EXP :182-192
    if (!K.pen_zero) {
      const double s = P.sw[x];
#pragma unroll
      for (int n = 0; n < 4; ++n) pen[n] = K.frac_inv_nbands * s;
    }
  }
#pragma unroll
  for (int n = 0; n < 4; ++n)
    if (n < K.nbands) P.sw_pen_band[(size_t)n * slab + x] = pen[n];

  if (P.SW_pen) {   // :199-204
    double tot = 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (n < K.nbands) tot = tot + pen[n];
    P.SW_pen[x] = tot;
  }
  if (P.SW_vis_pen) {   // :208-224
    const int nv = (SCH == MOM6X_OPACITY_MANIZZA_05 && K.nbands > 2) ? 2 : K.nbands;
    double tot = 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (n < nv) tot = tot + pen[n];
    P.SW_vis_pen[x] = tot;
  }

  // optics%opacity_band
  double op[4];
  if constexpr (CHL == 0) {   // :153-181
    op[0] = K.inv_scale;
    op[1] = SCH == MOM6X_OPACITY_DOUBLE_EXP ? K.inv_scale_2nd : K.inv_scale;
    op[2] = op[3] = K.inv_scale;
    for (int k = 0; k < nz; ++k) store_layer(K, P, (size_t)k * slab + x, band, op);
  } else if constexpr (CHL == 1) {
    band_opacities<SCH>(K, P.lut, mask, chl, op);
    for (int k = 0; k < nz; ++k) store_layer(K, P, (size_t)k * slab + x, band, op);
  } else {
    const bool wet = mask > 0.0;
    for (int k0 = 0; k0 < nz; k0 += OP_PF) {
#pragma unroll
      for (int q = 0; q < OP_PF; ++q) {
        const int k = k0 + q;
        if (k < nz) {
          const double c = buf[q];
          buf[q] = (k + OP_PF < nz) ? P.chl_3d[(size_t)(k + OP_PF) * slab + x] : 0.0;
          if (wet && (c < 0.0)) atomicAdd(P.cnt, 1ull);   // :328
          band_opacities<SCH>(K, P.lut, mask, c, op);
          store_layer(K, P, (size_t)k * slab + x, band, op);
        }
      }
    }
  }
}

}  // namespace

// opacity_CS and the members of optics_type that set_opacity reads, as opacity_init leaves them; the Ohlmann table and the counter
// of negative chlorophyll on the device
struct OpState {
  bool init;
  mom6x_opacity_params P;
  double c1[4], c2[4], pw[4];
  int chl_dep_bands;
  double chl_min, log10chl_min, log10chl_max, dlog10chl;
  double *lut;                 // a1 | a2 | b1 | b2, OP_NLUT entries each (OHLMANN_03 only)
  unsigned long long *cnt;     // 1, on the device
};

void opacity_free(mom6x_ctx *c) {
  if (!c->op) return;
  (void)hipFree(c->op->lut);
  (void)hipFree(c->op->cnt);
  delete c->op;
  c->op = nullptr;
}

// init_ohlmann_table :1321-1430: Ohlmann (2003) Table 1a with the additional values of CESM-POP, interpolated linearly in
// chlorophyll onto OP_NLUT points spaced evenly in log10(chlorophyll)
static void ohlmann_table(OpState *s, double *lut) {
  const int nt = 31;
  static const double chl_t[nt] = {.001, .005, .01, .02, .03, .05, .10, .15, .20, .25, .30, .35, .40, .45, .50, .60,
                                   .70, .80, .90, 1.00, 1.50, 2.00, 2.50, 3.00, 4.00, 5.00, 6.00, 7.00, 8.00, 9.00, 10.00};
  static const double tab[4][nt] = {
      {0.4421, 0.4451, 0.4488, 0.4563, 0.4622, 0.4715, 0.4877, 0.4993, 0.5084, 0.5159, 0.5223, 0.5278, 0.5326, 0.5369, 0.5408, 0.5474,
       0.5529, 0.5576, 0.5615, 0.5649, 0.5757, 0.5802, 0.5808, 0.5788, 0.56965, 0.55638, 0.54091, 0.52442, 0.50766, 0.49110, 0.47505},
      {0.2981, 0.2963, 0.2940, 0.2894, 0.2858, 0.2800, 0.2703, 0.2628, 0.2571, 0.2523, 0.2481, 0.2444, 0.2411, 0.2382, 0.2356, 0.2309,
       0.2269, 0.2235, 0.2206, 0.2181, 0.2106, 0.2089, 0.2113, 0.2167, 0.23357, 0.25504, 0.27829, 0.30274, 0.32698, 0.35056, 0.37303},
      {0.0287, 0.0301, 0.0319, 0.0355, 0.0384, 0.0434, 0.0532, 0.0612, 0.0681, 0.0743, 0.0800, 0.0853, 0.0902, 0.0949, 0.0993, 0.1077,
       0.1154, 0.1227, 0.1294, 0.1359, 0.1640, 0.1876, 0.2082, 0.2264, 0.25808, 0.28498, 0.30844, 0.32932, 0.34817, 0.36540, 0.38132},
      {0.3192, 0.3243, 0.3306, 0.3433, 0.3537, 0.3705, 0.4031, 0.4262, 0.4456, 0.4621, 0.4763, 0.4889, 0.4999, 0.5100, 0.5191, 0.5347,
       0.5477, 0.5588, 0.5682, 0.5764, 0.6042, 0.6206, 0.6324, 0.6425, 0.66172, 0.68144, 0.70086, 0.72144, 0.74178, 0.76190, 0.78155}};
  s->chl_min = chl_t[0];
  s->log10chl_min = log10(chl_t[0]);
  s->log10chl_max = log10(chl_t[nt - 1]);
  s->dlog10chl = (s->log10chl_max - s->log10chl_min) / (OP_NLUT - 1);
  int m = 1;
  for (int n = 0; n < OP_NLUT; ++n) {
    const double log10chl_lut = s->log10chl_min + n * s->dlog10chl;
    double chl = pow(10.0, log10chl_lut);
    chl = fmax(chl_t[0], fmin(chl, chl_t[nt - 1]));
    while (chl > chl_t[m]) ++m;
    const double w2 = (chl - chl_t[m - 1]) / (chl_t[m] - chl_t[m - 1]);
    const double w1 = 1. - w2;
    for (int t = 0; t < 4; ++t) lut[t * OP_NLUT + n] = w1 * tab[t][m - 1] + w2 * tab[t][m];
  }
}

extern "C" int mom6x_opacity_init(mom6x_ctx *c, const mom6x_opacity_params *p) {
  REQUIRE(c && p, MOM6X_EINVAL, "mom6x_opacity_init: null argument");
  REFUSE(!c->GV.Boussinesq, "opacity_init", "non-Boussinesq mode (the SpV_avg scaling of extract_optics_slice)");
  const int sch = p->opacity_scheme, nb = p->nbands;
  REQUIRE(sch == MOM6X_OPACITY_MANIZZA_05 || sch == MOM6X_OPACITY_MOREL_88 || sch == MOM6X_OPACITY_SINGLE_EXP ||
          sch == MOM6X_OPACITY_DOUBLE_EXP || sch == MOM6X_OPACITY_OHLMANN_03, MOM6X_EINVAL, "opacity_init: opacity_scheme is not valid.");
  REQUIRE(nb >= 0, MOM6X_EINVAL, "opacity_init: PEN_SW_NBANDS must not be negative");
  REQUIRE(sch != MOM6X_OPACITY_DOUBLE_EXP || nb == 2, MOM6X_EINVAL, "set_opacity: Cannot use a double_exp opacity scheme with nbands!=2.");
  REQUIRE(sch != MOM6X_OPACITY_SINGLE_EXP || nb == 1, MOM6X_EINVAL, "set_opacity: Cannot use a single_exp opacity scheme with nbands!=1.");
  REQUIRE(sch != MOM6X_OPACITY_OHLMANN_03 || nb == 2, MOM6X_EINVAL, "set_opacity: OHLMANN_03 scheme requires nbands==2");
  REFUSE(nb > 4, "opacity_init", "more than 4 bands of penetrating shortwave radiation");
  HIPCHK(hipSetDevice(c->device));
  opacity_free(c);
  OpState *s = new OpState();   // (all members zero)
  c->op = s;
  s->P = *p;
  if (sch == MOM6X_OPACITY_MANIZZA_05) {   // :1246-1269
    for (int n = 0; n < (nb < 3 ? nb : 3); ++n) {
      s->c1[n] = p->manizza_coef[2 * n]; s->c2[n] = p->manizza_coef[2 * n + 1];
      s->pw[n] = p->manizza_power[n];
    }
    for (int n = 3; n < nb; ++n) { s->c1[n] = s->c1[n - 1]; s->c2[n] = s->c2[n - 1]; s->pw[n] = s->pw[n - 1]; }
    s->chl_dep_bands = nb;
    for (int n = nb - 1; n >= 0; --n) {
      if (s->pw[n] != 0.0) break;
      s->chl_dep_bands = n;
    }
    for (int n = s->chl_dep_bands; n < nb; ++n)
      if (s->c2[n] != 0.0) { s->c1[n] = s->c1[n] + s->c2[n]; s->c2[n] = 0.0; }
  }
  HIPCHK(hipMalloc(&s->cnt, sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(s->cnt, 0, sizeof(unsigned long long), c->stream));
  if (sch == MOM6X_OPACITY_OHLMANN_03) {
    double lut[4 * OP_NLUT];
    ohlmann_table(s, lut);
    HIPCHK(hipMalloc(&s->lut, sizeof(lut)));
    HIPCHK(hipMemcpyAsync(s->lut, lut, sizeof(lut), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the table on the stack is no longer read
  }
  s->init = true;
  return MOM6X_OK;
}

extern "C" int mom6x_opacity_status(mom6x_ctx *c, long *negative_chl) {
  REQUIRE(c && c->op && c->op->init, MOM6X_EINVAL, "opacity_status: Module must be initialized before it is used.");
  HIPCHK(hipSetDevice(c->device));
  unsigned long long n = 0;
  HIPCHK(hipMemcpyAsync(&n, c->op->cnt, sizeof(n), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemsetAsync(c->op->cnt, 0, sizeof(n), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (negative_chl) *negative_chl = (long)n;
  return MOM6X_OK;
}

extern "C" int mom6x_set_pen_shortwave(mom6x_ctx *c, const double *sw, const double *sw_vis_dir, const double *sw_vis_dif,
                                       const double *sw_nir_dir, const double *sw_nir_dif, const double *chl_2d, const double *chl_3d,
                                       double opacity_scale, double *opacity_band, double *sw_pen_band, double *SW_pen,
                                       double *SW_vis_pen, double *opac_diag) {
  REQUIRE(c && c->op && c->op->init, MOM6X_EINVAL, "set_pen_shortwave: Module must be initialized before it is used.");
  const OpState *s = c->op;
  const mom6x_opacity_params &P = s->P;
  const mom6x_vgrid &GV = c->GV;
  const int sch = P.opacity_scheme, nb = P.nbands;
  const bool chl_scheme = sch == MOM6X_OPACITY_MANIZZA_05 || sch == MOM6X_OPACITY_MOREL_88 || sch == MOM6X_OPACITY_OHLMANN_03;
  REQUIRE(!(chl_2d && chl_3d), MOM6X_EINVAL, "set_pen_shortwave: chl_2d and chl_3d are both given");
  REQUIRE(!chl_scheme || chl_2d || chl_3d, MOM6X_EINVAL,
          "set_pen_shortwave: OPACITY_SCHEME = MANIZZA_05, MOREL_88 or OHLMANN_03 needs chl_2d or chl_3d (VAR_PEN_SW)");
  REQUIRE(chl_scheme || !(chl_2d || chl_3d), MOM6X_EINVAL,
          "set_pen_shortwave: EXP_OPACITY_SCHEME = SINGLE_EXP or DOUBLE_EXP takes no chlorophyll");
  const bool vis_in = sw_vis_dir && sw_vis_dif, nir_in = sw_nir_dir && sw_nir_dif;
  REQUIRE(sch != MOM6X_OPACITY_OHLMANN_03 || (vis_in && nir_in) || (!vis_in && sw), MOM6X_EINVAL,
          "opacity_from_chl: No shortwave input was provided (OHLMANN_03 needs sw, or all of sw_vis_dir, sw_vis_dif, sw_nir_dir, sw_nir_dif).");
  if (nb == 0) return MOM6X_OK;
  REQUIRE(opacity_band && sw_pen_band, MOM6X_EINVAL, "set_pen_shortwave: null optics%opacity_band or optics%sw_pen_band");
  HIPCHK(hipSetDevice(c->device));
  const Dm d = c->d;

  OpK K;
  memset(&K, 0, sizeof(K));
  for (int n = 0; n < 4; ++n) { K.c1[n] = s->c1[n]; K.c2[n] = s->c2[n]; K.pw[n] = s->pw[n]; }
  for (int n = 0; n < 6; ++n) { K.mo[n] = P.morel_coef[n]; K.mp[n] = P.morel_pen_coef[n]; }
  K.blue_frac = P.blue_frac; K.one_m_blue = 1.0 - P.blue_frac;
  K.land = P.opacity_land_value;
  // GV%Angstrom_Z as H_to_Z*Angstrom_H (Boussinesq: both are the same length)
  const double floor_Z = fmax(0.1 * (GV.H_to_Z * GV.Angstrom_H), GV.dZ_subroundoff);
  K.inv_scale = 1.0 / fmax(P.pen_sw_scale, floor_Z);
  K.inv_scale_2nd = 1.0 / fmax(P.pen_sw_scale_2nd, floor_Z);
  K.ratio1 = P.sw_1st_exp_ratio; K.one_m_ratio1 = 1. - P.sw_1st_exp_ratio;
  K.Inv_nbands = nb <= 1 ? 1.0 : 1.0 / (double)nb;
  K.Inv_nbands_nir = nb <= 2 ? 0.0 : 1.0 / ((double)nb - 2.0);
  K.frac_inv_nbands = P.pen_sw_frac * K.Inv_nbands;
  K.Z_to_m = P.Z_to_m;
  K.op_diag_len = 1.0e-10 * P.m_to_Z;
  K.opacity_scale = opacity_scale;
  K.chl_min = s->chl_min; K.log10chl_min = s->log10chl_min; K.log10chl_max = s->log10chl_max; K.dlog10chl = s->dlog10chl;
  K.nbands = nb; K.chl_dep_bands = s->chl_dep_bands;
  K.vis_in = vis_in; K.nir_in = nir_in; K.tot_in = sw != nullptr;
  K.pen_zero = !sw || (P.pen_sw_scale <= 0.0);
  OpP A;
  A.sw = sw; A.vis_dir = sw_vis_dir; A.vis_dif = sw_vis_dif; A.nir_dir = sw_nir_dir; A.nir_dif = sw_nir_dif;
  A.chl_2d = chl_2d; A.chl_3d = chl_3d; A.lut = s->lut;
  A.opacity_band = opacity_band; A.sw_pen_band = sw_pen_band; A.SW_pen = SW_pen; A.SW_vis_pen = SW_vis_pen; A.opac_diag = opac_diag;
  A.cnt = s->cnt;

  const dim3 b = blk2(), g = grid3(d.ni, d.nj, 1, b);
#define OP_LAUNCH(SCH, CHL) KLAUNCH(c, "k_opacity_cols<" #SCH ", " #CHL ">", (k_opacity_cols<MOM6X_OPACITY_##SCH, CHL>), g, b, d, c->G, K, A)
  const bool c3 = chl_3d != nullptr;
  switch (sch) {
    case MOM6X_OPACITY_MANIZZA_05: if (c3) OP_LAUNCH(MANIZZA_05, 2); else OP_LAUNCH(MANIZZA_05, 1); break;
    case MOM6X_OPACITY_MOREL_88: if (c3) OP_LAUNCH(MOREL_88, 2); else OP_LAUNCH(MOREL_88, 1); break;
    case MOM6X_OPACITY_OHLMANN_03: if (c3) OP_LAUNCH(OHLMANN_03, 2); else OP_LAUNCH(OHLMANN_03, 1); break;
    case MOM6X_OPACITY_DOUBLE_EXP: OP_LAUNCH(DOUBLE_EXP, 0); break;
    default: OP_LAUNCH(SINGLE_EXP, 0); break;
  }
#undef OP_LAUNCH
  HIPCHK(hipGetLastError());
  return MOM6X_OK;
}
