/*
 * mom6x.h -- C ABI of the MI355X-native MOM6 split-explicit dynamical core.
 *
 * This is the drop-in boundary: every entry point below
 * is what a Fortran `bind(C)` interface in MOM6 binds to replace one module
 * procedure of the reference.  Each declaration cites the reference interface
 * (file:line under /root/reference) that it stands in for.  No torch / C++ types
 * appear in any signature: plain pointers, ints and doubles only.
 *
 * Memory model
 * ------------
 * All field pointers handed to the `mom6x_*` compute entry points are DEVICE
 * pointers (HBM) to FP64 arrays in the "pitched tile layout" described by
 * mom6x_dims.  The Fortran host keeps its own (i,j,k) column-major arrays
 * (i fastest); mom6x_upload_* / mom6x_download_* convert between a Fortran array
 * with MOM6's symmetric-memory extents and the pitched device layout with one
 * strided DMA (hipMemcpy3DAsync), so i stays the coalesced index on the device
 * exactly as in the reference's `do i` inner loops.
 *
 * Pitched tile layout (one layout for h-, u-, v- and q-point arrays):
 *   local C indices: compute domain i = 0..ni-1, j = 0..nj-1 (MOM6 isc..iec,
 *   jsc..jec); data domain i = -halo..ni-1+halo; the symmetric-memory extra
 *   row/column of u-, v-, q-point arrays is I = -halo-1 (MOM6 IsdB = isd-1).
 *   A vertex/face index I (capital in MOM6) refers to the east/north face of
 *   cell i, as in MOM6.
 *   flat(i,j,k) = (i + ioff) + (j + joff)*pitch + k*slab,
 *   with ioff >= halo+1, joff = halo+1, pitch >= ioff+ni+halo (multiple of 16
 *   doubles so that i = 0 starts a 128-byte line), slab = pitch*(nj+2*halo+1).
 *   All four staggerings use the same flat(); 2-D arrays are one slab.
 */
#ifndef MOM6X_H
#define MOM6X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mom6x_continuity_params.sum_order, the Leith members of mom6x_hor_visc_params, Recon_Scheme / boundary_extrap /
 * h_nonvanished of mom6x_eos_params, mom6x_device_count.
 * 3: mom6x_coriolis_params grew (CORIOLIS_SCHEME ARAKAWA_LAMB81 / AL_BLEND / ROBUST_ENSTRO: wt_lin_blend, F_eff_max_blend, PV_Adv_Scheme),
 * mom6x_eos_params.EOS_quadrature and the EOS forms beyond LINEAR / WRIGHT, mom6x_barotropic_params' wide-halo members
 * (use_wide_halos, BTHALO, min_stencil) (round 3).
 * 5: (round 5) mom6x_barotropic_params.nonlinear_continuity / nonlin_cont_update_period; btstep accepts BT_cont == NULL;
 *    mom6x_continuity_params.sum_order = MOM6X_SUM_TREE16_FMA.
 * 6: (round 6) mom6x_barotropic_params.bt_thick_scheme / maxvel (BT_THICK_SCHEME without a BT_cont_type; BOUND_BT_CORRECTION through
 *    eta_cor_bound), mom6x_set_dtbt_pbce_eta.
 * 4: (round 4) mom6x_dyn_split_RK2_restart_fills + MOM6X_RK2_HAVE_*, mom6x_rk2_diag_*; see the end of this comment's list in
 * DESIGN.md section 1.  Hosts compare mom6x_abi_version() with the value they were
 * built against (fortran/mom6x_c_api.F90 MOM6X_ABI_BUILT_FOR, mom6_amd/abi.py ABI_VERSION) and refuse to run on a mismatch. */
#define MOM6X_ABI_VERSION 6

/* ------------------------------------------------------------------------- */
/* Tile dimensions and layout (MOM_hor_index.F90:14-44 hor_index_type +
 * config_src/memory/dynamic_symmetric/MOM_memory.h extents).                */
typedef struct mom6x_dims {
  int ni, nj, nk;   /* compute-domain size of this tile and number of layers  */
  int halo;         /* NIHALO = NJHALO (MOM_domains.F90:221), >= 4 for PPM+BT */
  int ioff, joff;   /* memory column/row of local index i = 0 / j = 0         */
  int pitch;        /* doubles per memory row                                 */
  int slab;         /* doubles per 2-D plane = pitch * (nj + 2*halo + 1)      */
  /* Position of this tile in the global (ni_glob x nj_glob) domain and the
   * 2-D processor layout (MOM_domains LAYOUT = npx,npy).                     */
  int i_glob0, j_glob0;       /* global index of local (0,0)                  */
  int ni_glob, nj_glob;
  int reentrant_x, reentrant_y; /* REENTRANT_X / REENTRANT_Y                  */
} mom6x_dims;

/* Fill ioff/joff/pitch/slab from ni,nj,nk,halo.  Returns 0 on success.       */
int mom6x_dims_init(mom6x_dims *d, int ni, int nj, int nk, int halo);

/* ------------------------------------------------------------------------- */
/* Grid metrics: ocean_grid_type (src/core/MOM_grid.F90:30-200).  All planes
 * live in ONE contiguous block `metrics[MOM6X_G_COUNT][slab]`.               */
enum mom6x_metric {
  MOM6X_G_mask2dT = 0, MOM6X_G_mask2dCu, MOM6X_G_mask2dCv, MOM6X_G_mask2dBu,
  MOM6X_G_dxT, MOM6X_G_dyT, MOM6X_G_IdxT, MOM6X_G_IdyT,
  MOM6X_G_dxCu, MOM6X_G_dyCu, MOM6X_G_IdxCu, MOM6X_G_IdyCu,
  MOM6X_G_dxCv, MOM6X_G_dyCv, MOM6X_G_IdxCv, MOM6X_G_IdyCv,
  MOM6X_G_dxBu, MOM6X_G_dyBu, MOM6X_G_IdxBu, MOM6X_G_IdyBu,
  MOM6X_G_areaT, MOM6X_G_IareaT, MOM6X_G_areaBu, MOM6X_G_IareaBu,
  MOM6X_G_areaCu, MOM6X_G_areaCv, MOM6X_G_IareaCu, MOM6X_G_IareaCv,
  MOM6X_G_dy_Cu, MOM6X_G_dx_Cv,     /* open face widths                      */
  MOM6X_G_bathyT,                   /* depth of the bottom, positive down [Z] */
  MOM6X_G_CoriolisBu, MOM6X_G_Coriolis2Bu,
  MOM6X_G_COUNT
};

/* ------------------------------------------------------------------------- */
/* verticalGrid_type (src/core/MOM_verticalGrid.F90:25-90) -- scalars only;
 * Rlay/g_prime are passed as arrays of nk doubles where needed.              */
typedef struct mom6x_vgrid {
  double g_Earth;        /* G_EARTH [L2 Z-1 T-2]                              */
  double Rho0;           /* RHO_0                                             */
  double Angstrom_H;     /* ANGSTROM in thickness units                       */
  double H_subroundoff;  /* verticalGrid.F90:214-218                          */
  double dZ_subroundoff;
  double H_to_Z, Z_to_H, H_to_RZ, RZ_to_H;  /* all 1 / 1 / Rho0 / 1/Rho0 (Bouss) */
  int    Boussinesq;     /* only 1 is supported            */
} mom6x_vgrid;

/* ------------------------------------------------------------------------- */
/* continuity_PPM_CS (src/core/MOM_continuity_PPM.F90:35-68); defaults from
 * continuity_PPM_init :2674-2754.                                            */
typedef struct mom6x_continuity_params {
  int    upwind_1st;       /* UPWIND_1ST_CONTINUITY      (F)                  */
  int    monotonic;        /* MONOTONIC_CONTINUITY       (F)                  */
  int    simple_2nd;       /* SIMPLE_2ND_PPM_CONTINUITY  (F)                  */
  double tol_eta;          /* ETA_TOLERANCE  (0.5*NK*ANGSTROM)                */
  double tol_vel;          /* VELOCITY_TOLERANCE (3e8 m/s)                    */
  double CFL_limit_adjust; /* CONTINUITY_CFL_LIMIT (0.5)                      */
  int    aggress_adjust;   /* CONT_PPM_AGGRESS_ADJUST (F).  With this or vol_CFL set the thread-per-column kernels run, whose column sums are in the reference's order whatever sum_order says */
  int    vol_CFL;          /* CONT_PPM_VOLUME_BASED_CFL (default = aggress_adjust, MOM_continuity_PPM.F90:2728) */
  int    better_iter;      /* CONT_PPM_BETTER_ITER (T)                        */
  int    use_visc_rem_max; /* CONT_PPM_USE_VISC_REM_MAX (T)                   */
  int    marginal_faces;   /* CONT_PPM_MARGINAL_FACE_AREAS (T)                */
  int    sum_order;        /* order of the column (k) sums of zonal/meridional_mass_flux, *_flux_adjust and
                            * set_*_BT_cont -- no counterpart in the reference, which sums sequentially in k:
                            *   MOM6X_SUM_REFERENCE (0): the reference's order, results bit-identical to the Fortran loop nest;
                            *   MOM6X_SUM_TREE16    (1): sixteen partial sums over k = q, q+16, q+32, ... (q = 0..15, each
                            *     in increasing k) combined by a balanced binary tree in q order, and the duL / duR
                            *     recurrences of set_*_BT_cont (:1293-1316) taken as the min / max they compute in exact
                            *     arithmetic.  Results agree with the reference order to round-off (<= 1e-13 of each
                            *     field's range); this is the order of a 16-lane wavefront row and lets one wavefront own a
                            *     face column (continuity_wave.hip).  Requires nk <= 128.
                            *   MOM6X_SUM_TREE16_FMA (2): the sums of TREE16, and fused multiply-adds at FIXED sites (what a Fortran
                            *     compiler's -ffp-contract does where it pleases): a + CFL * (p + q * r) of *_flux_layer and
                            *     *_flux_thickness (:936-955, :1017-1030) as fma(CFL, fma(q, r, p), a); u + du * visc_rem as
                            *     fma(du, visc_rem, u); the masked neighbours and the edge values of PPM_reconstruction_x/y
                            *     (:2396-2405).  oracle/orc_continuity.c restates the same sites; against the reference order the
                            *     results agree to round-off (bound and 10-step drift: tests/test_sum_order_gpu.py).  The default of the
                            *     hosts since round 6 (mom6_amd/abi.py default_sum_order, MOM6X_CONTINUITY_SUMS of the Fortran shim).       */
} mom6x_continuity_params;
#define MOM6X_SUM_REFERENCE  0
#define MOM6X_SUM_TREE16     1
#define MOM6X_SUM_TREE16_FMA 2

/* BT_cont_type (src/core/MOM_variables.F90:315-350): 12 2-D planes + h_u,h_v.
 * Any pointer may be NULL only if the whole struct pointer is NULL.          */
typedef struct mom6x_BT_cont {
  double *FA_u_EE, *FA_u_E0, *FA_u_W0, *FA_u_WW, *uBT_WW, *uBT_EE;
  double *FA_v_NN, *FA_v_N0, *FA_v_S0, *FA_v_SS, *vBT_SS, *vBT_NN;
  double *h_u, *h_v;   /* 3-D; may be NULL (allocated(BT_cont%h_u) false)     */
} mom6x_BT_cont;

/* barotropic_CS parameters (src/core/MOM_barotropic.F90:108-330, read in
 * barotropic_init :5403-5713).  Only the default-path flags listed in
 * SURVEY.md 8(b.1) are implemented; others must keep their default.          */
typedef struct mom6x_barotropic_params {
  double bebt;                 /* BEBT (0.1)                                  */
  double dtbt;                 /* CS%dtbt [T]: the stable BT step (set_dtbt)  */
  double dt_bt_filter;         /* DT_BT_FILTER (-0.25)                        */
  int    BT_project_velocity;  /* BT_PROJECT_VELOCITY (F)                     */
  int    Sadourny;             /* SADOURNY (T)                                */
  int    strong_drag;          /* BT_STRONG_DRAG (F)                          */
  int    wt_uv_bug;            /* VISC_REM_BT_WEIGHT_BUG (T)                  */
  int    use_old_coriolis_bracket_bug; /* BT_USE_OLD_CORIOLIS_BRACKET_BUG (F) */
  int    visc_rem_u_uh0;       /* BT_USE_VISC_REM_U_UH0 (F)                   */
  int    clip_velocity;        /* CLIP_BT_VELOCITY (F)                        */
  double CFL_trunc;            /* CFL_TRUNCATE (0.5)                          */
  double vel_underflow;        /* VEL_UNDERFLOW (0)                           */
  double G_extra;              /* G_BT_EXTRA (0)                              */
  double BT_Coriolis_scale;    /* BT_CORIOLIS_SCALE (1)                       */
  double maxCFL_BT_cont;       /* MAXCFL_BT_CONT (0.25)                       */
  int    bound_BT_corr;        /* BOUND_BT_CORRECTION (F)                     */
  int    BT_cont_bounds;       /* BT_CONT_CORR_BOUNDS (T)                     */
  double dtbt_fraction;        /* |DTBT| when DTBT<0 (0.98)                   */
  double Z_ref;                /* G%Z_ref (0)                                 */
  /* The wide-halo cycle of btstep (MOM_barotropic.F90:766-794, :2505-2512): with BT_USE_WIDE_HALOS the solver marches in from its
   * wide halo and exchanges every (halo / stencil) sub-steps.  On the device the barotropic domain's halo IS the context's halo
   * (mom6x_dims.halo): a host that wants BTHALO > NIHALO creates the context with halo = max(NIHALO, BTHALO) (and may keep the
   * 3-D passes at NIHALO rows: mom6x_set_dyn_pass_width).  The answers do not depend on any of the three.                    */
  int    use_wide_halos;       /* BT_USE_WIDE_HALOS (T); F: an exchange every sub-step                                       */
  int    BTHALO;               /* BTHALO (0): refused if it exceeds the context's halo                                        */
  int    min_stencil;          /* BT_WIDE_HALO_MIN_STENCIL (0)                                                                */
  /* Without a BT_cont_type (btstep's BT_cont argument NULL; USE_BT_CONT_TYPE = False), ABI 5: the face areas of the linear barotropic
   * continuity equation from the bathymetry alone, or (NONLINEAR_BT_CONTINUITY) from bathymetry + eta, recomputed every
   * NONLIN_BT_CONT_UPDATE_PERIOD sub-steps with a stencil of 2 (MOM_barotropic.F90:767-768, :1131-1136, :2539-2543, :5146-5237).     */
  int    nonlinear_continuity;       /* NONLINEAR_BT_CONTINUITY (F); ignored when BT_cont is given                                  */
  int    nonlin_cont_update_period;  /* NONLIN_BT_CONT_UPDATE_PERIOD (1); 0: the face areas of the step's first eta throughout      */
  /* ABI 6.  BT_THICK_SCHEME (:5566-5591) for btcalc calls without h_u / h_v: MOM6X_BT_THICK_*.  FROM_BT_CONT (the reference's default)
   * needs the BT_cont_type: btcalc without h_u then falls back to HYBRID only where the reference passes may_use_default (:4419-4430,
   * barotropic_init :6127), and the step without a BT_cont_type refuses it as barotropic_init does (:5589-5591).                       */
  int    bt_thick_scheme;
  /* MAXVEL (3e8 m/s) [L T-1]: only in eta_cor_bound = IareaT 0.1 maxvel (Datu + Datu + Datv + Datv) (:6164-6173), the bound of
   * BOUND_BT_CORRECTION when the BT_cont fits are not used for it (no BT_cont_type, or BT_CONT_CORR_BOUNDS = False) :1582-1585.       */
  double maxvel;
} mom6x_barotropic_params;
#define MOM6X_BT_THICK_FROM_BT_CONT 0
#define MOM6X_BT_THICK_HYBRID       1
#define MOM6X_BT_THICK_HARMONIC     2
#define MOM6X_BT_THICK_ARITHMETIC   3

/* CoriolisAdv_CS (src/core/MOM_CoriolisAdv.F90:29-100; CoriolisAdv_init :1054).            */
enum mom6x_coriolis_scheme {       /* CORIOLIS_SCHEME, values as in MOM_CoriolisAdv.F90:82-90       */
  MOM6X_SADOURNY75_ENERGY = 1,     /* default                                                   */
  MOM6X_ARAKAWA_HSU90 = 2,
  MOM6X_ROBUST_ENSTRO = 3,         /* :687-714, :808-838; switches CORIOLIS_EN_DIS and BOUND_CORIOLIS off (:1118, :1158) */
  MOM6X_SADOURNY75_ENSTRO = 4,
  MOM6X_ARAKAWA_LAMB81 = 5,        /* :534-542 + the ep_u / ep_v terms :716-721, :840-845       */
  MOM6X_AL_BLEND = 6               /* ARAKAWA_LAMB_BLEND :543-588                               */
};
enum mom6x_ke_scheme { MOM6X_KE_ARAKAWA = 10, MOM6X_KE_SIMPLE_GUDONOV = 11, MOM6X_KE_GUDONOV = 12 };
enum mom6x_pv_adv_scheme { MOM6X_PV_ADV_CENTERED = 21, MOM6X_PV_ADV_UPWIND1 = 22 };   /* MOM_CoriolisAdv.F90:115-119 */
typedef struct mom6x_coriolis_params {
  int Coriolis_Scheme;   /* SADOURNY75_ENERGY                                                   */
  int KE_Scheme;         /* KE_ARAKAWA                                                          */
  int bound_Coriolis;    /* BOUND_CORIOLIS (F; tc1/p0: T)                                       */
  int no_slip;           /* NOSLIP (F)                                                          */
  int Coriolis_En_Dis;   /* CORIOLIS_EN_DIS (F): the energy-dissipating biased SADOURNY75_ENERGY scheme  */
  int PV_Adv_Scheme;     /* PV_ADV_SCHEME (PV_ADV_CENTERED); read by ROBUST_ENSTRO only; 0 = the default   */
  double F_eff_max_blend;/* CORIOLIS_BLEND_F_EFF_MAX (4.0), ARAKAWA_LAMB_BLEND only                      */
  double wt_lin_blend;   /* CORIOLIS_BLEND_WT_LIN (0.125), ARAKAWA_LAMB_BLEND only; clipped to [1e-16, 1] as :1139 does */
} mom6x_coriolis_params;

/* PressureForce_FV_CS (src/core/MOM_PressureForce_FV.F90:40-110; PressureForce_FV_init :2020). */
typedef struct mom6x_pgf_params {
  double rho_ref;        /* RHO_PGF_REF (= RHO_0)                                               */
  int    rho_ref_bug;    /* RHO_PGF_REF_BUG (T)                                                 */
  double Z_ref;          /* G%Z_ref (0)                                                         */
} mom6x_pgf_params;

/* vertvisc_CS (src/parameterizations/vertical/MOM_vert_friction.F90:39-180; vertvisc_init :3135).  The
 * branches of vertvisc_coef / find_coupling_coef that are on the device path: HARMONIC_VISC on or off,
 * BOTTOMDRAGLAW on (visc%Kv_bbl_u/v, visc%bbl_thick_u/v from set_viscous_BBL are inputs) or off
 * (KV_EXTRA_BBL), KV_ML_INVZ2, visc%Kv_shear.  Ice shelves, open boundaries, GL90, visc%Kv_shear_Bu and
 * the dynamic / law-of-the-wall mixed-layer viscosities (DYNAMIC_VISCOUS_ML, FIXED_DEPTH_LOTW_ML,
 * LOTW_VISCOUS_ML_FLOOR, a bulk mixed layer) are not.                                               */
typedef struct mom6x_vertvisc_params {
  double Kv;            /* KV           [H Z T-1]                                                 */
  double Kvml_invZ2;    /* KV_ML_INVZ2  (0)                                                       */
  double Hmix;          /* HMIX_FIXED   [Z]                                                       */
  double Hbbl;          /* HBBL         [Z]                                                       */
  double harm_BL_val;   /* HARMONIC_BL_SCALE (0)                                                  */
  double Kv_extra_bbl;  /* KV_EXTRA_BBL (0); only without BOTTOMDRAGLAW                           */
  int    harmonic_visc; /* HARMONIC_VISC (F)                                                      */
  int    bottomdraglaw; /* BOTTOMDRAGLAW (T)                                                      */
  int    answer_date;   /* VERT_FRICTION_ANSWER_DATE (99991231)                                   */
} mom6x_vertvisc_params;

/* hor_visc_CS (src/parameterizations/lateral/MOM_hor_visc.F90:36-259; hor_visc_init :2322).  On the device path:
 * LAPLACIAN and/or BIHARMONIC with constant / velocity-scale / time-scale background coefficients, SMAGORINSKY_KH,
 * SMAGORINSKY_AH (+ BOUND_CORIOLIS_BIHARM), BOUND_KH / BOUND_AH in both the "better" and the legacy form,
 * ADD_LES_VISCOSITY, USE_LAND_MASK_FOR_HVISC, NOSLIP (Laplacian only, as in the reference).  Not on it (rejected):
 * Leith / Leith+E, MEKE, GME, backscatter, anisotropic viscosity, KH_SIN_LAT, 2-D background files, RE_AH,
 * USE_CONT_THICKNESS, open boundaries, the FrictWork diagnostics.                                              */
typedef struct mom6x_hor_visc_params {
  int    Laplacian;        /* LAPLACIAN (F)                                                     */
  int    biharmonic;       /* BIHARMONIC (T)                                                    */
  double Kh;               /* KH (0)              [L2 T-1]                                      */
  double Kh_bg_min;        /* KH_BG_MIN (0)                                                     */
  double Kh_vel_scale;     /* KH_VEL_SCALE (0)    [L T-1]                                       */
  int    Smagorinsky_Kh;   /* SMAGORINSKY_KH (F)                                                */
  double Smag_Lap_const;   /* SMAG_LAP_CONST (0)                                                */
  int    bound_Kh;         /* BOUND_KH (T)                                                      */
  int    better_bound_Kh;  /* BETTER_BOUND_KH (= BOUND_KH)                                      */
  int    add_LES_viscosity;/* ADD_LES_VISCOSITY (F)                                             */
  double Ah;               /* AH (0)              [L4 T-1]                                      */
  double Ah_vel_scale;     /* AH_VEL_SCALE (0)                                                  */
  double Ah_time_scale;    /* AH_TIME_SCALE (0)                                                 */
  int    Smagorinsky_Ah;   /* SMAGORINSKY_AH (F)                                                */
  double Smag_bi_const;    /* SMAG_BI_CONST (0)                                                 */
  int    bound_Ah;         /* BOUND_AH (T)                                                      */
  int    better_bound_Ah;  /* BETTER_BOUND_AH (= BOUND_AH)                                      */
  int    bound_Coriolis;   /* BOUND_CORIOLIS_BIHARM (= BOUND_CORIOLIS, F); only with SMAGORINSKY_AH */
  double bound_Cor_vel;    /* BOUND_CORIOLIS_VEL (= MAXVEL = 3e8)                               */
  int    use_land_mask;    /* USE_LAND_MASK_FOR_HVISC (T)                                       */
  double bound_coef;       /* HORVISC_BOUND_COEF (0.8)                                          */
  int    no_slip;          /* NOSLIP (F)                                                        */
  int    backscatter_underbound; /* BACKSCATTER_UNDERBOUND (T)                                  */
  double dt;               /* DT: the time step the stability bounds are made for (:2714)       */
  /* Leith (1996) viscosities from the gradient of the vertical vorticity (:80-85, :987-1113);
   * USE_LEITHY (Leith+E) and USE_QG_LEITH_VISC are not carried                                  */
  int    Leith_Kh;         /* LEITH_KH (F); needs LAPLACIAN                                     */
  double Leith_Lap_const;  /* LEITH_LAP_CONST (0)                                               */
  int    Leith_Ah;         /* LEITH_AH (F); needs BIHARMONIC                                    */
  double Leith_bi_const;   /* LEITH_BI_CONST (0)                                                */
  int    modified_Leith;   /* MODIFIED_LEITH (F): add the gradient of the divergence            */
  int    use_beta_in_Leith;/* USE_BETA_IN_LEITH (= LEITH_KH): grad f (G%dF_dx, G%dF_dy of
                            * MOM_calculate_grad_Coriolis, MOM_shared_initialization.F90:91) joins grad(vorticity) */
} mom6x_hor_visc_params;

/* tv%eqn_of_state (EOS_type, src/equation_of_state/MOM_EOS.F90:99-150) and the switches of
 * PressureForce_FV_CS that only matter with an equation of state.  Analytic density integrals
 * (analytic_int_density_dz, MOM_EOS.F90:1384) exist for EOS_LINEAR and the WRIGHT family: LINEAR, WRIGHT (the default,
 * MOM_EOS_Wright.F90), WRIGHT_FULL (MOM_EOS_Wright_full.F90) and WRIGHT_REDUCED (MOM_EOS_Wright_red.F90) are carried, each
 * with the analytic integrals and, with EOS_QUADRATURE or a pressure reconstruction, the generic quadratures.  UNESCO
 * (MOM_EOS_UNESCO.F90) has no analytic integrals: it needs EOS_QUADRATURE or a pressure reconstruction, as in the reference
 * ("No analytic integration option is available with this EOS!"); likewise ROQUET_RHO (= NEMO, MOM_EOS_Roquet_rho.F90).
 * JACKETT_06 (MOM_EOS_Jackett06.F90) and ROQUET_SPV (MOM_EOS_Roquet_SpV.F90).  TEOS10 (the gsw library, whose sources are not in
 * the reference tree) is refused.   */
enum mom6x_eos_form { MOM6X_EOS_LINEAR = 1, MOM6X_EOS_WRIGHT = 2, MOM6X_EOS_WRIGHT_FULL = 3, MOM6X_EOS_WRIGHT_REDUCED = 4, MOM6X_EOS_UNESCO = 5,
                      MOM6X_EOS_ROQUET_RHO = 6, /* "ROQUET_RHO" = "NEMO": MOM_EOS_Roquet_rho.F90; quadratures only, like UNESCO */
                      MOM6X_EOS_JACKETT06 = 7,  /* "JACKETT_06": MOM_EOS_Jackett06.F90; quadratures only ("JACKETT_MCD" is UNESCO) */
                      MOM6X_EOS_ROQUET_SPV = 8  /* "ROQUET_SPV": MOM_EOS_Roquet_SpV.F90; quadratures only */ };
typedef struct mom6x_eos_params {
  int    form;            /* EQN_OF_STATE                                                       */
  double Rho_T0_S0;       /* RHO_T0_S0 (1000)  } EOS_LINEAR                                     */
  double dRho_dT;         /* DRHO_DT (-0.2)    }                                                */
  double dRho_dS;         /* DRHO_DS (0.8)     }                                                */
  double dRho_dp;         /* linear_EOS%dRho_dp (0)                                             */
  int    MassWghtInterp;  /* bit 0: MASS_WEIGHT_IN_PRESSURE_GRADIENT, bit 1: ..._TOP (F, F)     */
  int    use_SSH_in_Z0p;  /* SSH_IN_EOS_PRESSURE_FOR_PGF (F)                                    */
  /* With ALE (USE_REGRIDDING): RECONSTRUCT_FOR_PRESSURE + PRESSURE_RECONSTRUCTION_SCHEME (PressureForce_FV_init :2172-2184)  */
  int    Recon_Scheme;    /* 0: layer-mean T, S (analytic integrals); 1: PLM edge values (TS_PLM_edge_values, MOM_ALE.F90:1495)
                           *    and the 5-point quadrature of int_density_dz_generic_plm (MOM_density_integrals.F90:418);
                           *    2: PPM edge values (TS_PPM_edge_values, MOM_ALE.F90:1581: edge_values_implicit_h4 + PPM_reconstruction)
                           *    and int_density_dz_generic_ppm (:874); needs NK >= 4                    */
  int    boundary_extrap; /* BOUNDARY_EXTRAPOLATION_PRESSURE (T)                                   */
  int    MassWghtInterpVanOnly; /* MASS_WEIGHT_IN_PGF_VANISHED_ONLY (F)                            */
  double h_nonvanished;   /* RESET_INTXPA_H_NONVANISHED (1e-6 m) [H]: the thickness below which a side counts as vanished */
  int    EOS_quadrature;  /* EOS_QUADRATURE (F, MOM_EOS.F90:1654): with Recon_Scheme = 0 the layer integrals come from the 5-point
                           * quadratures of int_density_dz_generic_pcm (MOM_density_integrals.F90:108) instead of the analytic forms */
} mom6x_eos_params;

/* MOM_dyn_split_RK2_CS parameters (src/core/MOM_dynamics_split_RK2.F90:85-273, read in
 * initialize_dyn_split_RK2 :1427-1495).                                                     */
typedef struct mom6x_rk2_params {
  double be;                   /* BE (0.6)                                                    */
  double begw;                 /* BEGW (0)                                                    */
  int    split_bottom_stress;  /* SPLIT_BOTTOM_STRESS (F)                                     */
  int    BT_use_layer_fluxes;  /* BT_USE_LAYER_FLUXES (T) -- only T supported                 */
  int    store_CAu;            /* STORE_CORIOLIS_ACCEL (T) -- only T supported                */
  int    visc_rem_dt_bug;      /* VISC_REM_TIMESTEP_BUG (T with ENABLE_BUGS_BY_DEFAULT)       */
  int    remap_aux;            /* REMAP_AUXILIARY_VARS (F): mom6x_remap_dyn_split_RK2_aux_vars */
  int    no_BT_cont;           /* 1: USE_BT_CONT_TYPE = False (MOM_barotropic.F90 barotropic_init: CS%BT_cont stays unassociated) --
                                * RK2.F90:467-469, :627, :644-652, :662-668, :867: btcalc from h (BT_THICK_SCHEME = HYBRID), the
                                * continuity calls and both btstep calls without a BT_cont_type, set_dtbt with eta (ABI 5)    */
} mom6x_rk2_params;

/* ------------------------------------------------------------------------- */
/* Context: owns the device copy of the metrics, the parameter structs, scratch
 * HBM, two HIP streams (compute + halo) and the RCCL communicator handle.    */
typedef struct mom6x_ctx mom6x_ctx;

/* Status codes.  The reference calls MOM_error(FATAL,...) (never returns); the
 * C side returns nonzero and mom6x_last_error() holds the message the Fortran
 * shim forwards to MOM_error.                                                */
#define MOM6X_OK          0
#define MOM6X_EINVAL      1
#define MOM6X_EHIP        2
#define MOM6X_EUNSUPPORTED 3
#define MOM6X_ENUMERIC    4   /* device-side flag (a NaN reached the thicknesses in continuity; NaN / overflow in the reproducing sums), returned by mom6x_ctx_sync */

const char *mom6x_last_error(void);
int  mom6x_abi_version(void);
/* The work-group (lanes along i, rows) of the kernels that give each cell or face of a plane a lane, and the i of their first lane
 * (a cache line before the first own point).  For tests that place a grid's edges where a launch extent rounds up to another block. */
int  mom6x_lane_launch_shape(int *bx, int *by, int *i_first);
/* The points along i and j by which the tiles of a tiled kernel advance: which = 0 CorAdCalc (k_corad_lds, k_corad_fused: the tile
 * minus its frame), 1 horizontal_viscosity (k_hv_fused), 2 advect_tracer (the cells of a tile of the x passes, the rows of a segment
 * of the y passes).  For tests that place a grid's edges on a whole number of tiles and one point more. */
int  mom6x_tile_steps(int which, int *sx, int *sy);
/* hipGetDeviceCount: lets a host with one process per GPU pick its device as (local rank) mod (count).  < 0 on error. */
int  mom6x_device_count(void);
/* sizeof() of the public structs (0 dims, 1 vgrid, 2 continuity_params, 3 BT_cont, 4 barotropic_params,
 * 5 coriolis_params, 6 pgf_params, 7 rk2_params, 8 rk2_hooks, 9 eos_params, 10 vertvisc_params, 11 hor_visc_params,
 * 12 remapping_params, 13 regrid_zstar_params, 14 chksum_result, 15 sum_output_params, 16 energy_sums, 17 regrid_rho_params,
 * 18 set_visc_params, 19 thickness_diffuse_params, 20 tracer_hor_diff_params, 21 varmix_params,
 * 22 mixedlayer_restrat_params, 23 MEKE_params, 25 set_diffusivity_params, 27 diabatic_aux_params, 28 surface_fluxes, 30 energetic_PBL_params, 32 frazil_params,
 * 33 geothermal_params, 34 opacity_params, 35 kappa_shear_params, 36 neutral_diffusion_params; 24, 26, 29 and 31 are not assigned and
 * return -1): lets ctypes /
 * ISO_C_BINDING mirrors be checked at start-up.  */
int  mom6x_struct_size(int which);

/* Create a context for one tile on HIP device `device`.  `metrics_host` is a
 * HOST block of MOM6X_G_COUNT pitched planes (copied to HBM once; replaces the
 * `G` argument of every reference routine).                                  */
int mom6x_ctx_create(mom6x_ctx **ctx, const mom6x_dims *dims, int device,
                     const double *metrics_host, const mom6x_vgrid *GV,
                     int first_direction);
int mom6x_ctx_destroy(mom6x_ctx *ctx);
/* The stream all compute entry points launch on (a hipStream_t).            */
void *mom6x_ctx_stream(mom6x_ctx *ctx);
int  mom6x_ctx_sync(mom6x_ctx *ctx);
const mom6x_dims *mom6x_ctx_dims(const mom6x_ctx *ctx);
const double *mom6x_ctx_metrics_dev(const mom6x_ctx *ctx);

/* Per-kernel timing (HIP events on the compute stream around every launch).  Mirrors the
 * reference's cpu_clock_begin/end brackets (e.g. MOM_dynamics_split_RK2.F90:502/538) at kernel
 * granularity.  mom6x_prof_report writes "name<TAB>count<TAB>total_ms" lines into buf.       */
int mom6x_prof_enable(mom6x_ctx *ctx, int on);
int mom6x_prof_reset(mom6x_ctx *ctx);
int mom6x_prof_filter(mom6x_ctx *ctx, const char *prefix);  /* time only kernels named prefix*; NULL = all */
int mom6x_prof_report(mom6x_ctx *ctx, char *buf, int buflen);

/* Device memory helpers for non-torch hosts (Fortran).                       */
int mom6x_dev_alloc(mom6x_ctx *ctx, double **p, size_t n_doubles);
int mom6x_dev_free(mom6x_ctx *ctx, double *p);
int mom6x_dev_copy(mom6x_ctx *ctx, double *dst, const double *src, size_t n_doubles);   /* device -> device, on the context's stream */
/* Fortran array <-> pitched device array.  `stagger`: 0 = h-point
 * (SZI_,SZJ_), 1 = u-point (SZIB_,SZJ_), 2 = v-point (SZI_,SZJB_), 3 = q-point
 * (SZIB_,SZJB_), with MOM6 symmetric-memory extents; nk = 1 for 2-D.         */
int mom6x_upload(mom6x_ctx *ctx, double *dev, const double *host_f, int stagger, int nk);
int mom6x_download(mom6x_ctx *ctx, double *host_f, const double *dev, int stagger, int nk);

/* ------------------------------------------------------------------------- */
/* MOM_continuity_PPM                                                          */

int mom6x_continuity_init(mom6x_ctx *ctx, const mom6x_continuity_params *p);
  /* continuity_PPM_init, MOM_continuity_PPM.F90:2674                          */

/* Newton statistics of the mass-flux kernel (sum_order TREE16 only): out3[0] = flux re-evaluations inside
 * zonal/meridional_flux_adjust and set_*_BT_cont (whole-column sweeps, per wavefront of four face columns), out3[1] = Newton solves
 * (per wavefront), out3[2] = solves repeated with the exact CFL limits, accumulated while collection is on.  mode: 1 = switch
 * collection on and reset the counters, 0 = switch it off, -1 = just read.  The collecting variant of the kernel is slower (the
 * counters cost it registers): a diagnostic, not for timed runs.  Synchronises the context's stream.  out3 nullable.   */
int mom6x_continuity_stats(mom6x_ctx *ctx, int mode, unsigned long long *out3);

/* continuity_PPM(u, v, hin, h, uh, vh, dt, G, GV, US, CS, OBC, pbv, uhbt, vhbt,
 *   visc_rem_u, visc_rem_v, u_cor, v_cor, BT_cont, du_cor, dv_cor)
 * MOM_continuity_PPM.F90:86-194.  Optional Fortran arguments are nullable
 * pointers; presence changes behaviour exactly as in the reference
 * (:590-592, :637, :737, :756).  OBC must be unassociated and pbv all ones
 * (USE_POROUS_BARRIER=False).  h may alias hin.                              */
int mom6x_continuity_PPM(mom6x_ctx *ctx,
    const double *u, const double *v, const double *hin, double *h,
    double *uh, double *vh, double dt,
    const double *uhbt, const double *vhbt,
    const double *visc_rem_u, const double *visc_rem_v,
    double *u_cor, double *v_cor, const mom6x_BT_cont *BT_cont,
    double *du_cor, double *dv_cor);

/* ------------------------------------------------------------------------- */
/* MOM_barotropic                                                              */

int mom6x_barotropic_init(mom6x_ctx *ctx, const mom6x_barotropic_params *p);
  /* barotropic_init, MOM_barotropic.F90:5301 (static fields :5784-5896,
   * :6146-6163).                                                              */

/* btcalc(h, G, GV, CS, h_u, h_v, may_use_default, OBC)  :4360.  h_u/h_v are the
 * BT_cont%h_u/h_v face thicknesses (BT_THICK_SCHEME=FROM_BT_CONT, the default);
 * when NULL the scheme of mom6x_barotropic_params.bt_thick_scheme (ARITHMETIC :4448, HYBRID :4453,
 * HARMONIC :4476) and, for FROM_BT_CONT, the HYBRID default of `may_use_default`.  Writes the
 * context's frhatu/frhatv.  mom6x_btcalc_strict is the call without may_use_default: FROM_BT_CONT
 * without h_u / h_v is the reference's "Inconsistent settings" error (:4426-4429).               */
int mom6x_btcalc(mom6x_ctx *ctx, const double *h, const double *h_u, const double *h_v);
int mom6x_btcalc_strict(mom6x_ctx *ctx, const double *h, const double *h_u, const double *h_v);

/* bt_mass_source(h, eta, set_cor, G, GV, CS)  :5243                           */
int mom6x_bt_mass_source(mom6x_ctx *ctx, const double *h, const double *eta, int set_cor);

/* set_dtbt(G, GV, US, CS, pbce=, gtot_est=, SSH_add=)  :3509.  Result goes to
 * the context's dtbt (and *dtbt_out if non-NULL).                            */
int mom6x_set_dtbt(mom6x_ctx *ctx, const double *pbce, double gtot_est, double SSH_add,
                   double *dtbt_out);

/* set_dtbt(G, GV, US, CS, pbce, eta=, SSH_add=) without a BT_cont argument, MOM_barotropic.F90:3576-3582: face areas
 * from find_face_areas(eta=eta) :5171-5186 when NONLINEAR_BT_CONTINUITY is set and eta is not NULL, otherwise from
 * find_face_areas(add_max=SSH_add) :5208-5219 (the deeper of the two neighbouring columns).  mom6x_set_dtbt_pbce is the call
 * of MOM_dynamics_split_RK2.F90:667 behind a BT_cont_type (= eta NULL, SSH_add 0).                                     */
int mom6x_set_dtbt_pbce_eta(mom6x_ctx *ctx, const double *pbce, const double *eta, double SSH_add, double *dtbt_out);
int mom6x_set_dtbt_pbce(mom6x_ctx *ctx, const double *pbce, double *dtbt_out);

/* btstep(U_in, V_in, eta_in, dt, bc_accel_u, bc_accel_v, forces, pbce, eta_PF_in,
 *   U_Cor, V_Cor, accel_layer_u, accel_layer_v, eta_out, uhbtav, vhbtav, G, GV, US,
 *   CS, visc_rem_u, visc_rem_v, SpV_avg, ADp, OBC, BT_cont, eta_PF_start, taux_bot,
 *   tauy_bot, uh0, vh0, u_uh0, v_vh0, etaav)          MOM_barotropic.F90:455-459.
 * forces%taux/tauy are passed as 2-D planes; SpV_avg/ADp/OBC/eta_PF_start are
 * not supported (must be absent in the caller); taux_bot/tauy_bot, the uh0 quad
 * and etaav are nullable.  Mutates the context's ubtav, vbtav, eta_cor.      */
int mom6x_btstep(mom6x_ctx *ctx,
    const double *U_in, const double *V_in, const double *eta_in, double dt,
    const double *bc_accel_u, const double *bc_accel_v,
    const double *taux, const double *tauy, const double *pbce,
    const double *eta_PF_in, const double *U_Cor, const double *V_Cor,
    double *accel_layer_u, double *accel_layer_v, double *eta_out,
    double *uhbtav, double *vhbtav,
    const double *visc_rem_u, const double *visc_rem_v,
    const mom6x_BT_cont *BT_cont,
    const double *taux_bot, const double *tauy_bot,
    const double *uh0, const double *vh0, const double *u_uh0, const double *v_vh0,
    double *etaav);

/* The warnings btstep issues for an unphysical sea surface height ("btstep: eta has
 * dropped below bathyT", MOM_barotropic.F90:2738-2745; the reference prints the first two
 * per call and counts the rest).  The device counts them over all sub-steps since the last
 * reset and keeps the first: info[4] = eta [H], -bathyT [Z], i, j (tile indices, 0-based).
 * Synchronises the context's stream.  `info` is nullable.                          */
int mom6x_btstep_warnings(mom6x_ctx *ctx, int reset, long long *count, double *info);

/* Access to barotropic_CS state that MOM_restart registers by pointer
 * (register_barotropic_restarts :6253: ubtav, vbtav) and that tests inspect.
 * `which`: 0 ubtav, 1 vbtav, 2 eta_cor, 3 frhatu (3-D), 4 frhatv (3-D),
 * 5 IDatu, 6 IDatv.  Returns a device pointer owned by the context.          */
double *mom6x_barotropic_field(mom6x_ctx *ctx, int which);
/* CS%dtbt, the scalar restart variable "DTBT" (register_barotropic_restarts :6290): *get (nullable) receives it, *set
 * (nullable, > 0) replaces it -- a restarted run keeps the file's DTBT as barotropic_init :5962-5970 does.         */
int mom6x_barotropic_dtbt(mom6x_ctx *ctx, double *get, const double *set);

/* ------------------------------------------------------------------------- */
/* MOM_CoriolisAdv                                                             */
int mom6x_CoriolisAdv_init(mom6x_ctx *ctx, const mom6x_coriolis_params *p);
  /* CoriolisAdv_init, MOM_CoriolisAdv.F90:1054                                */
/* CorAdCalc(u, v, h, uh, vh, CAu, CAv, OBC, AD, G, GV, US, CS, pbv, Waves)   :125.
 * OBC unassociated, no Stokes drift, pbv == 1.  Input halos as documented at :229-233. */
int mom6x_CorAdCalc(mom6x_ctx *ctx, const double *u, const double *v, const double *h,
                    const double *uh, const double *vh, double *CAu, double *CAv);

/* ------------------------------------------------------------------------- */
/* MOM_PressureForce (dispatcher :41 -> PressureForce_FV_Bouss, FV.F90:947)    */
int mom6x_PressureForce_init(mom6x_ctx *ctx, const mom6x_pgf_params *p, const double *Rlay,
                             const double *g_prime);
  /* PressureForce_init :85; Rlay/g_prime are HOST arrays of nk doubles
   * (GV%Rlay, GV%g_prime of verticalGrid_type).                               */
/* PressureForce(h, tv, PFu, PFv, G, GV, US, CS, ALE_CSp, ADp, p_atm, pbce, eta).  Layered
 * (tv%eqn_of_state unassociated) Boussinesq path; p_atm absent; pbce/eta nullable.       */
int mom6x_PressureForce(mom6x_ctx *ctx, const double *h, double *PFu, double *PFv,
                        double *pbce, double *eta);
/* The thermo_var_ptrs argument `tv` of PressureForce (:947): tv%T, tv%S (device, 3-D h-point arrays that
 * stay owned by the caller) and tv%eqn_of_state.  Once set, mom6x_PressureForce -- and the PressureForce
 * calls inside mom6x_step_dyn_split_RK2 -- take the use_EOS branch (:1206, :1289-1309: int_density_dz,
 * and Set_pbce_Bouss :692-722).  T == NULL dissociates tv%eqn_of_state again (layered path).  Bulk mixed
 * layers (GV%nk_rho_varies > 0) and ALE reconstructions are not on this path.                        */
/* ALE_PLM_edge_values(CS, G, GV, h, Q, bdry_extrap, Q_t, Q_b), MOM_ALE.F90:1520-1577: the values of a PLM reconstruction of the
 * tracer Q at the top and the bottom of every layer (TS_PLM_edge_values :1495 calls it for S and T); boundary cells PCM unless
 * bdry_extrap.  Answer dates >= 20190101 (h_neglect = GV%H_subroundoff).                                                   */
int mom6x_ALE_PLM_edge_values(mom6x_ctx *ctx, const double *h, const double *Q, int bdry_extrap, double *Q_t, double *Q_b);
/* One field of TS_PPM_edge_values (MOM_ALE.F90:1581): edge_values_implicit_h4 + PPM_reconstruction (+ PPM_boundary_extrapolation),
 * the edge values PRESSURE_RECONSTRUCTION_SCHEME = 2 hands to int_density_dz_generic_ppm.  NK >= 4. */
int mom6x_ALE_PPM_edge_values(mom6x_ctx *ctx, const double *h, const double *Q, int bdry_extrap, double *Q_t, double *Q_b);
int mom6x_PressureForce_set_tv(mom6x_ctx *ctx, const double *T, const double *S, const mom6x_eos_params *eos);

/* ------------------------------------------------------------------------- */
/* MOM_hor_visc                                                    */
/* hor_visc_init :2322: the 2-D coefficient fields (background and maximum viscosities, Smagorinsky
 * constants, metric products) are computed on the device from the metric block.                 */
int mom6x_hor_visc_init(mom6x_ctx *ctx, const mom6x_hor_visc_params *p);
/* horizontal_viscosity(u, v, h, uh, vh, diffu, diffv, MEKE, VarMix, G, GV, US, CS, tv, dt, ...) :266.
 * uh, vh only feed the FrictWork diagnostics and are not arguments here.  After mom6x_hor_visc_init,
 * mom6x_step_dyn_split_RK2 calls this itself at :886 (and the new-run initialisation at :1601) unless a
 * horizontal_viscosity callback is given.                                                      */
int mom6x_horizontal_viscosity(mom6x_ctx *ctx, const double *u, const double *v, const double *h,
                               double *diffu, double *diffv);

/* ------------------------------------------------------------------------- */
/* MOM_remapping / the remapping half of MOM_ALE                   */
/* remapping_CS (src/ALE/MOM_remapping.F90:47-84) as set by initialize_remapping :1654 / remapping_set_param :122.
 * On the device path: the OM4-era reconstruction functions PCM, PLM, PPM_H4, PPM_IH4 (build_reconstructions_1d :410) with
 * REMAPPING_ANSWER_DATE >= 20190101, with or without boundary extrapolation, both sub-cell integrators
 * (remap_src_to_sub_grid_om4 :845 / remap_src_to_sub_grid :962) and remap_sub_to_tgt_grid_om4 :1103.
 * Not on it (rejected): PPM_CW, the hybgen and PQM schemes, the Recon1d class ("C_*") schemes,
 * the 2018 answers, PCM_cell masks, check_reconstruction / check_remapping.                        */
enum mom6x_remap_scheme { MOM6X_REMAP_PCM = 0, MOM6X_REMAP_PLM = 2, MOM6X_REMAP_PPM_H4 = 4, MOM6X_REMAP_PPM_IH4 = 5 };   /* :86-96 */
typedef struct mom6x_remapping_params {
  int    scheme;                    /* REMAPPING_SCHEME: PCM, PLM (the module default), PPM_H4, PPM_IH4   */
  int    boundary_extrapolation;    /* REMAP_BOUNDARY_EXTRAP (type default .true.; ALE_init passes F)     */
  int    force_bounds_in_subcell;   /* REMAP_BOUND_INTERMEDIATE_VALUES (F)                                */
  int    force_bounds_in_target;    /* (T)                                                                */
  int    om4_remap_via_sub_cells;   /* REMAPPING_USE_OM4_SUBCELLS (type default F; ALE_init default T)    */
  int    answer_date;               /* REMAPPING_ANSWER_DATE; must be >= 20190101                         */
  double h_neglect;                 /* GV%H_subroundoff (or GV%kg_m2_to_H*1e-30 ...)                      */
  double h_neglect_edge;            /* = h_neglect for answer dates >= 20190101                           */
} mom6x_remapping_params;

/* ALE_remap_scalar-style column remap of `nfields` T-point fields in place (MOM_ALE.F90:760 ALE_remap_tracers,
 * without the diagnostics): for every wet column remapping_core_h(CS, nk, h_old, field, nk, h_new, field).   */
int mom6x_ALE_remap_tracers(mom6x_ctx *ctx, const mom6x_remapping_params *p, const double *h_old, const double *h_new,
                            double *const *fields, int nfields);
/* ALE_remap_set_h_vel :882 (no partial cells, no OBC): h_u = 0.5*(h(i)+h(i+1)) at open faces, else untouched.  */
int mom6x_ALE_remap_set_h_vel(mom6x_ctx *ctx, const double *h_new, double *h_u, double *h_v);
/* ALE_remap_velocities :1089 (REMAP_VEL_CONSERVE_KE off, no near-bottom masking, no diagnostics).              */
int mom6x_ALE_remap_velocities(mom6x_ctx *ctx, const mom6x_remapping_params *p, const double *h_old_u, const double *h_old_v,
                               const double *h_new_u, const double *h_new_v, double *u, double *v);
/* The three calls MOM.F90 makes in a row (ALE_regridding_and_remapping: ALE_remap_set_h_vel of the old and of the new grid, then
 * ALE_remap_velocities) as one, from the CELLS' thicknesses: the same bits; with OM4's switch set h_u / h_v are never stored. */
int mom6x_ALE_remap_velocities_from_h(mom6x_ctx *ctx, const mom6x_remapping_params *p, const double *h_old, const double *h_new,
                                      double *u, double *v);
/* ... with the KE-conserving correction of its baroclinic part (REMAP_VEL_CONSERVE_KE = True and allow_preserve_variance,
 * MOM_ALE.F90:1166-1195, :1240-1270): what MOM.F90 asks for inside the time step.                                          */
int mom6x_ALE_remap_velocities_conserve_ke(mom6x_ctx *ctx, const mom6x_remapping_params *p, const double *h_old_u,
                                           const double *h_old_v, const double *h_new_u, const double *h_new_v,
                                           double *u, double *v);
/* ALE_regrid (MOM_ALE.F90:518) -> regridding_main (MOM_regridding.F90:862) for REGRIDDING_ZSTAR without ice shelves
 * and with CS%nk == GV%ke (Boussinesq): nom_depth_H :920-922, build_zstar_grid :1257 (build_zstar_column,
 * coord_zlike.F90:63; filtered_grid_motion :1105 incl. the old-grid weight and its depth-dependent transition),
 * calc_h_new_by_dz :1008.  h needs one valid halo point (the reference regrids isc-1..iec+1).
 * coordinateResolution: nk host values (the nominal layer thicknesses ALE_COORDINATE_CONFIG gives, in Z units). */
typedef struct mom6x_regrid_zstar_params {
  double min_thickness;                 /* MIN_THICKNESS (0.001 m) [H]                                        */
  double old_grid_weight;               /* from REGRID_TIME_SCALE: exp(-dt/timescale) or 0 (:96)              */
  double depth_of_time_filter_shallow;  /* REGRID_FILTER_SHALLOW_DEPTH (0) [H]                                */
  double depth_of_time_filter_deep;     /* REGRID_FILTER_DEEP_DEPTH (0) [H]                                   */
  double Z_ref;                         /* G%Z_ref (0)                                                        */
} mom6x_regrid_zstar_params;
int mom6x_ALE_regrid_zstar(mom6x_ctx *ctx, const mom6x_regrid_zstar_params *p, const double *coordinateResolution,
                           const double *h, double *h_new, double *dzRegrid);

/* The density-following coordinate generators of regridding_main (MOM_regridding.F90:862): REGRIDDING_RHO
 * (build_rho_grid :1472 -> build_rho_column coord_rho.F90:92) and REGRIDDING_HYCOM1 (build_grid_HyCOM1 :1638 ->
 * build_hycom1_column coord_hycom.F90:106; Bleck 2002), CS%nk == GV%ke, no ice shelf.  Both find the positions of the
 * target interface densities in the column's (potential) density profile with regrid_interp.F90's
 * build_and_interpolate_grid :331 (regridding_set_ppolys :80, interpolate_grid :295, the Newton iteration of
 * get_polynomial_coordinate :376), blend old and new positions with filtered_grid_motion :1105 and hand back
 * dzInterface and h_new = calc_h_new_by_dz :1008.  REGRIDDING_RHO wants the column statically stable first
 * (regridding_preadjust_reqs :966): mom6x_ALE_convective_adjustment = convective_adjustment :1905.            */
enum mom6x_interp_scheme {            /* INTERPOLATION_SCHEME (regrid_interp.F90:38-49); others are not carried */
  MOM6X_INTERP_P1M_H2 = 0,            /* the default */
  MOM6X_INTERP_PLM = 3, MOM6X_INTERP_PPM_H4 = 5
};
typedef struct mom6x_regrid_rho_params {
  mom6x_regrid_zstar_params f;       /* MIN_THICKNESS, the time filter of filtered_grid_motion, G%Z_ref           */
  int    interp_scheme;              /* INTERPOLATION_SCHEME (P1M_H2)                                             */
  int    boundary_extrapolation;     /* BOUNDARY_EXTRAPOLATION (F)                                                */
  double ref_pressure;               /* P_REF (2e7 Pa): CS%ref_pressure of REGRIDDING_RHO, tv%P_Ref of HYCOM1     */
  double compressibility_fraction;   /* REGRID_COMPRESSIBILITY_FRACTION (0): HYCOM1 only                          */
  int    integrate_downward_for_e;   /* CS%integrate_downward_for_e (T): REGRIDDING_RHO only                      */
} mom6x_regrid_rho_params;
/* target_density: nk+1 host values (the interface densities set_target_densities :2297 makes from the layer ones).  */
int mom6x_ALE_regrid_rho(mom6x_ctx *ctx, const mom6x_regrid_rho_params *p, const mom6x_eos_params *eos,
                         const double *target_density, const double *h, const double *T, const double *S,
                         double *h_new, double *dzRegrid);
/* coordinateResolution: nk host values [Z]; max_interface_depths (nk+1) and max_layer_thickness (nk): host, nullable
 * (MAXIMUM_INT_DEPTH_CONFIG / MAX_LAYER_THICKNESS_CONFIG).  HYCOM1's "only improves" option is not carried.       */
int mom6x_ALE_regrid_hycom1(mom6x_ctx *ctx, const mom6x_regrid_rho_params *p, const mom6x_eos_params *eos,
                            const double *coordinateResolution, const double *target_density,
                            const double *max_interface_depths, const double *max_layer_thickness,
                            const double *h, const double *T, const double *S, double *h_new, double *dzRegrid);
/* convective_adjustment :1905: adjacent layers swap (h, T, S) until the density at the surface pressure increases downward */
int mom6x_ALE_convective_adjustment(mom6x_ctx *ctx, const mom6x_eos_params *eos, double *h, double *T, double *S);

/* remapping_core_h :234 for `ncol` independent columns stored back to back (n0 | n1 values each): the entry the
 * reference's own unit tests (remapping_unit_tests :2072) exercise.  Device pointers.                          */
int mom6x_remapping_core_h(mom6x_ctx *ctx, const mom6x_remapping_params *p, int ncol, int n0, const double *h0,
                           const double *u0, int n1, const double *h1, double *u1);

/* ------------------------------------------------------------------------- */
/* MOM_vert_friction                                                           */
/* The coupling coefficients CS%a_u, CS%a_v [(nk+1) levels], CS%h_u, CS%h_v and the optional
 * visc%Ray_u/Ray_v are produced by vertvisc_coef (:1357, not ported: SURVEY 8f-1); the host
 * hands their DEVICE copies to the context before vertvisc / vertvisc_remnant.             */
int mom6x_vertvisc_set_coef(mom6x_ctx *ctx, const double *a_u, const double *a_v,
                            const double *h_u, const double *h_v,
                            const double *Ray_u, const double *Ray_v);
/* vertvisc(u, v, h, forces, visc, dt, OBC, ADp, CDp, G, GV, US, CS, taux_bot, tauy_bot)  :557 */
/* vertvisc_init :3135: keeps the parameters and allocates CS%a_u, CS%a_v [(nk+1) levels], CS%h_u, CS%h_v on
 * the device; the context's coefficient set (mom6x_vertvisc_set_coef) then points at them.           */
int mom6x_vertvisc_init(mom6x_ctx *ctx, const mom6x_vertvisc_params *p);
/* The members of vertvisc_type (MOM_variables.F90) that vertvisc_coef / vertvisc read: visc%Kv_bbl_u/v and
 * visc%bbl_thick_u/v (2-D; required with BOTTOMDRAGLAW), visc%Kv_shear (3-D, nk+1 interfaces at h points,
 * nullable), visc%Ray_u/v (3-D, nullable).  Device arrays owned by the caller: mom6x_set_viscous_BBL below
 * fills the first four (and Ray_u/v) on the device; the shear-mixing schemes stay on the host.       */
int mom6x_vertvisc_set_visc(mom6x_ctx *ctx, const double *Kv_bbl_u, const double *Kv_bbl_v, const double *bbl_thick_u,
                            const double *bbl_thick_v, const double *Kv_shear, const double *Ray_u, const double *Ray_v);
/* vertvisc_coef(u, v, h, dz, forces, visc, tv, dt, G, GV, US, CS, OBC, VarMix) :1357, with dz = H_to_Z*h
 * (thickness_to_dz, MOM_interface_heights.F90:855, Boussinesq).  Fills CS%a_u, a_v, h_u, h_v.  After
 * mom6x_vertvisc_init, mom6x_step_dyn_split_RK2 calls this itself at :609, :738 and :1003 unless a
 * vertvisc_coef callback is given.                                                                   */
int mom6x_vertvisc_coef(mom6x_ctx *ctx, const double *u, const double *v, const double *h, double dt);
/* CS%a_u (0), CS%a_v (1) [nk+1 levels], CS%h_u (2), CS%h_v (3) of the device vertvisc_CS (diagnostics, restarts of Kv_u). */
double *mom6x_vertvisc_field(mom6x_ctx *ctx, int which);
int mom6x_vertvisc(mom6x_ctx *ctx, double *u, double *v, const double *taux, const double *tauy,
                   double dt, double *taux_bot, double *tauy_bot);
/* DIRECT_STRESS / HMIX_STRESS (vertvisc_init :3208, :3258-3268; vertvisc :707-720, :958-971): with Hmix_stress > 0 the wind
 * stress is distributed as a body force over the topmost Hmix_stress [H] of fluid instead of entering as the surface
 * boundary condition.  h is vertvisc's third argument (device pointer, kept); mom6x_step_dyn_split_RK2 uses its own h. */
int mom6x_vertvisc_set_direct_stress(mom6x_ctx *ctx, double Hmix_stress, const double *h);
/* vertvisc_remnant(visc, visc_rem_u, visc_rem_v, dt, G, GV, US, CS)  :1229                   */
int mom6x_vertvisc_remnant(mom6x_ctx *ctx, double *visc_rem_u, double *visc_rem_v, double dt);

/* ------------------------------------------------------------------------- */
/* MOM_set_viscosity: set_viscous_BBL                                          */
/* set_visc_CS (src/parameterizations/vertical/MOM_set_viscosity.F90:46-133; set_visc_init :2876-3204): the members the
 * non-channel, Boussinesq path of set_viscous_BBL (:135-1115) reads.  CHANNEL_DRAG (find_L_open_*, :878-1018), open
 * boundaries, ice shelves, a bulk mixed layer (nkml > 0) and the non-Boussinesq tv%SpV_avg forms are refused.      */
typedef struct mom6x_set_visc_params {
  int    bottomdraglaw;      /* BOTTOMDRAGLAW (T, :2941); F: mom6x_set_viscous_BBL returns at once (:323)             */
  double cdrag;              /* CDRAG (0.003, :3025)                                                                 */
  double drag_bg_vel;        /* DRAG_BG_VEL (0 m s-1, :3047) [L T-1]; 1e30 with BBL_USE_TIDAL_BG (:3045)             */
  double Hbbl;               /* CS%Hbbl = dz_bbl*(Z_to_m*m_to_H) (:3140) [H]                                         */
  double dz_bbl;             /* HBBL (required, :3018) [Z]                                                           */
  double BBL_thick_min;      /* BBL_THICK_MIN (0, :3068) [Z]                                                         */
  double Kv_BBL_min;         /* KV_BBL_MIN (KV, :3094) [H Z T-1]                                                     */
  int    linear_drag;        /* LINEAR_DRAG (F, :2957)                                                               */
  int    BBL_use_EOS;        /* BBL_USE_EOS (USE_EOS, :3060); used only with an EOS (use_BBL_EOS, :340)              */
  int    BBL_use_tidal_bg;   /* BBL_USE_TIDAL_BG (F, :3029): u2_bg from the tideamp field of mom6x_set_visc_init     */
  int    body_force_drag;    /* DRAG_AS_BODY_FORCE (F, :2947): needs visc%Ray_u/v                                    */
  int    correct_BBL_bounds; /* CORRECT_BBL_BOUNDS (F, :3100)                                                        */
  int    RiNo_mix;           /* CS%RiNo_mix = kappa_shear_is_used (F, :2970)                                         */
  int    channel_drag;       /* CHANNEL_DRAG (F, :2953): must be 0                                                   */
  double Rad_Earth;          /* G%Rad_Earth_L (6.378e6 m) [L]: BBL_thick_max = Rad_Earth*L_to_Z (:348)               */
  double L_to_Z;             /* US%L_to_Z (1): GV%g_Earth_Z_T2 = L_to_Z**2*g_Earth (MOM_verticalGrid.F90:178)        */
  double L_to_H;             /* US%L_to_m*GV%m_to_H (1): cdrag_sqrt_H, cdrag_L_to_H (:344-347)                       */
  int    nkml;               /* GV%nkml (0): must be 0                                                               */
  int    open_bcs;           /* CS%OBC associated (0): must be 0                                                     */
  int    ice_shelf;          /* an ice shelf (0): must be 0                                                          */
  int    SpV_avg;            /* tv%SpV_avg allocated (0, non-Boussinesq): must be 0                                  */
} mom6x_set_visc_params;
/* set_visc_init :2876: keeps the parameters.  eos: tv%eqn_of_state (NULL: none; use_BBL_EOS = eos && BBL_use_EOS, :340);
 * without it the density walk uses GV%Rlay as given to mom6x_PressureForce_init.  tideamp: CS%tideamp (:3175-3179), a
 * 2-D h-point DEVICE array [Z T-1] with a valid halo of one (required with BBL_USE_TIDAL_BG, kept).                    */
int mom6x_set_visc_init(mom6x_ctx *ctx, const mom6x_set_visc_params *p, const mom6x_eos_params *eos, const double *tideamp);
/* set_viscous_BBL(u, v, h, tv, visc, G, GV, US, CS, pbv) :135 on the context's stream, dz = H_to_Z*h.  u, v, h, T, S and
 * tv%p_surf (nullable) need a valid halo of one.  Writes visc%bbl_thick_u/v and visc%Kv_bbl_u/v (nullable) at the unmasked
 * faces I = isc-1..iec, j = jsc..jec and i = isc..iec, J = jsc-1..jec (:450-460), the range vertvisc_coef reads; masked
 * faces and all other points are left as they are.  visc%Ray_u/v (3-D, nullable; required with DRAG_AS_BODY_FORCE) are
 * zeroed everywhere first (:442-443), as the reference does whenever they are allocated.  T, S: required with use_BBL_EOS. */
int mom6x_set_viscous_BBL(mom6x_ctx *ctx, const double *u, const double *v, const double *h, const double *T, const double *S,
                          const double *p_surf, double *Kv_bbl_u, double *Kv_bbl_v, double *bbl_thick_u, double *bbl_thick_v,
                          double *Ray_u, double *Ray_v);

/* ------------------------------------------------------------------------- */
/* MOM_thickness_diffuse: thickness_diffuse                                    */
/* thickness_diffuse_CS (src/parameterizations/lateral/MOM_thickness_diffuse.F90:41-128; thickness_diffuse_init :2175-2500):
 * the members thickness_diffuse (:134-630) and thickness_diffuse_full (:635-1671) read on a Boussinesq grid with the plain
 * (Gent-McWilliams) streamfunction.  The members marked "must be 0" are refused with MOM6X_EUNSUPPORTED.
 * The reference's own thickness_diffuse_init (compiled, tests/test_ref_parity_cpu.py LATERAL_REFUSALS) stops on only one of
 * them: USE_STANLEY_GM without STANLEY_COEFF >= 0 (:2334), and accepts it with one.  KH_ETA_CONST, KH_ETA_VEL_SCALE,
 * DETANGLE_INTERFACES, USE_GME, KHTH_USE_FGNV_STREAMFUNCTION and USE_MEKE it accepts (the last two make VarMix_init ask for wave
 * speeds); the device refuses them because their paths are not on the device.  use_variable_mixing is not a parameter of this
 * init: it is VarMix%use_variable_mixing, which the reference's VarMix_init sets TRUE by default (INTERPOLATED_SQG_STRUCTURE with
 * SQG_EXPO > 0 allocates the stored slopes, MOM_lateral_mixing_coeffs.F90:1699-1701, :2053); with KHTH_SLOPE_CFF = 0 and nothing
 * else switched on that changes no arithmetic (:206-221), and the device takes stored slopes as arguments instead.  Both inits
 * stop on KHTH > 0 with READ_KHTH (:2218), as the device does.                                                              */
typedef struct mom6x_thickness_diffuse_params {
  int    thickness_diffuse;   /* THICKNESSDIFFUSE (F, :2207); F: mom6x_thickness_diffuse returns at once (:195)            */
  double Khth;                /* KHTH (0, :2210) [L2 T-1]; 0 without khth2d: returns at once (:196)                         */
  int    read_khth;           /* READ_KHTH (F, :2213): CS%khth2d is the khth2d of the init call; with KHTH > 0 an error (:2218) */
  double Khth_Min;            /* KHTH_MIN (0, :2242) [L2 T-1]                                                               */
  double Khth_Max;            /* KHTH_MAX (0, :2256) [L2 T-1]; used when > 0 (:291)                                         */
  double max_Khth_CFL;        /* KHTH_MAX_CFL (0.8, :2259); must be > 0 (:2291 and :404 leave KH_v unset otherwise)         */
  double slope_max;           /* KHTH_SLOPE_MAX (0.01, :2302) [Z L-1]                                                       */
  double kappa_smooth;        /* KD_SMOOTH (1e-6 m2 s-1, :2305) [H Z T-1]                                                   */
  double Z_to_L;              /* US%Z_to_L (1): mag_grad2 (:1037)                                                           */
  double Z_to_H_fill;         /* US%Z_to_m*GV%m_to_H (1) of vert_fill_TS (MOM_isopycnal_slopes.F90:655) [H Z-1]             */
  double Kh_eta_bg;           /* KH_ETA_CONST (0, :2266): must be 0                                                         */
  double Kh_eta_vel;          /* KH_ETA_VEL_SCALE (0, :2272): must be 0                                                     */
  int    use_FGNV_streamfn;   /* KHTH_USE_FGNV_STREAMFUNCTION (F, :2309): must be 0                                         */
  int    use_stanley_gm;      /* USE_STANLEY_GM (F, :2327): must be 0                                                       */
  int    detangle_interfaces; /* DETANGLE_INTERFACES (F, :2292): must be 0                                                  */
  int    use_GME;             /* USE_GME (F, :2397): must be 0                                                              */
  int    use_variable_mixing; /* VarMix%use_variable_mixing (Visbeck, resolution / depth scaling, khth_struct, QG Leith; :210): must be 0 */
  int    use_MEKE;            /* MEKE%Kh or MEKE%GM_src allocated (USE_MEKE, :2386; :262, :846): must be 0                  */
  int    use_Kh_in_MEKE;      /* USE_KH_IN_MEKE (F, :2388): must be 0                                                       */
  int    GMwork;              /* the GMwork diagnostic (CS%GMwork allocated: find_work, :847): must be 0                    */
  int    skeb_use_gm;         /* STOCH%skeb_use_gm (:509): must be 0                                                        */
  int    nkml;                /* GV%nkml (0; nk_linear, :839): must be 0                                                    */
  int    open_bcs;            /* open boundaries (G%OBCmaskCu/v differ from mask2dCu/v): must be 0                          */
  int    non_Boussinesq;      /* tv%SpV_avg allocated or GV%semi_Boussinesq: must be 0                                      */
} mom6x_thickness_diffuse_params;
/* thickness_diffuse_init :2175: keeps the parameters and allocates the work arrays (seven 3-D arrays with an EOS, three
 * without).  eos: tv%eqn_of_state (NULL: layers of constant density, :1085-1094).  khth2d: CS%khth2d (:2235), a 2-D h-point
 * DEVICE array [L2 T-1] with a valid halo of one, owned by the caller and kept (required with READ_KHTH, else NULL).         */
int mom6x_thickness_diffuse_init(mom6x_ctx *ctx, const mom6x_thickness_diffuse_params *p, const mom6x_eos_params *eos,
                                 const double *khth2d);
/* thickness_diffuse(h, uhtr, vhtr, tv, dt, G, GV, US, MEKE, VarMix, CDp, CS, STOCH) :134 on the context's stream, without a
 * host synchronisation or an allocation.  h, T, S, tv%p_surf (nullable) and khth2d need a valid halo of one; T, S are
 * required with an EOS.  slope_x, slope_y: VarMix%slope_x/y with use_stored_slopes, two nullable 3-D interface arrays of
 * nk+1 planes [Z L-1] that come together.  uhGM, vhGM: CDp%uhGM / vhGM, two nullable 3-D outputs that receive uhD, vhD
 * (:604, :608) and come together.  uhtr and uhGM are written at I = isc-1..iec, j = jsc..jec, vhtr and vhGM at i = isc..iec,
 * J = jsc-1..jec, h on the computational domain only; all other points are left as they are.  Faces are not masked by the
 * routine: a closed face gives a zero flux because G%dy_Cu / G%dx_Cv is zero there.  The caller still owes pass_var(h).     */
int mom6x_thickness_diffuse(mom6x_ctx *ctx, double *h, double *uhtr, double *vhtr, const double *T, const double *S,
                            const double *p_surf, const double *slope_x, const double *slope_y, double dt, double *uhGM,
                            double *vhGM);

/* ------------------------------------------------------------------------- */
/* MOM_tracer_hor_diff: tracer_hordiff                                        */
/* tracer_hor_diff_CS (src/tracer/MOM_tracer_hor_diff.F90:41-97; tracer_hor_diff_init :1630-1779) and the switches of VarMix and
 * MEKE that tracer_hordiff (:119-699) reads on its along-layer path (:541-612).  The members marked "must be 0" are refused
 * with MOM6X_EUNSUPPORTED.                                                                                                   */
typedef struct mom6x_tracer_hor_diff_params {
  double KhTr;                 /* KHTR (0, :1659) [L2 T-1]; <= 0 without variable mixing: mom6x_tracer_hordiff returns at once (:199) */
  double KhTr_Slope_Cff;       /* KHTR_SLOPE_CFF (0, :1666): the Eady term, with variable mixing, when > 0 (:225, :242)              */
  double KhTr_min;             /* KHTR_MIN (0, :1671) [L2 T-1]                                                                       */
  double KhTr_max;             /* KHTR_MAX (0, :1681) [L2 T-1]; used when > 0 (:245)                                                 */
  double KhTr_passivity_coeff; /* KHTR_PASSIVITY_COEFF (0, :1684); used with variable mixing when > 0 (:249)                         */
  double KhTr_passivity_min;   /* KHTR_PASSIVITY_MIN (0.5, :1690)                                                                    */
  int    check_diffusive_CFL;  /* CHECK_DIFFUSIVE_CFL (F, :1697): the iteration count from the cell CFL (:371-384), one stream
                                  synchronisation and one all-reduce per call                                                        */
  double max_diff_CFL;         /* MAX_TR_DIFFUSION_CFL (-1, :1702): when > 0 limits khdt_x, khdt_y (:322-357) and, without
                                  CHECK_DIFFUSIVE_CFL, gives the iteration count (:386)                                              */
  int    use_variable_mixing;  /* VarMix%use_variable_mixing (:222): the branch :238-281                                             */
  int    Resoln_scaled_KhTr;   /* VarMix%Resoln_scaled_KhTr (RESOLN_SCALED_KHTR): Res_fn_h scales the diffusivity (:246, :282-294).
                                  The reference reads it only with variable mixing; here the branch :282-294 runs as written when
                                  it is set without                                                                                  */
  int    use_MEKE_Kh;          /* MEKE%Kh is allocated (:243): the MEKE term, with variable mixing                                   */
  double MEKE_KhTr_fac;        /* MEKE%KhTr_fac (MEKE_KHTR_FAC, 0)                                                                   */
  int    use_neutral_diffusion; /* USE_NEUTRAL_DIFFUSION (F, :1738): must be 0                                                       */
  int    use_hor_bnd_diffusion; /* USE_HORIZONTAL_BOUNDARY_DIFFUSION (F, :1742): must be 0                                           */
  int    Diffuse_ML_interior;  /* DIFFUSE_ML_TO_INTERIOR (F, :1694; tracer_epipycnal_ML_diff needs a bulk mixed layer): must be 0    */
  int    offline;              /* do_online_flag = .false. with read_khdt_x, read_khdt_y (:359-369): must be 0                       */
  int    open_bcs;             /* open boundary conditions: must be 0                                                                */
} mom6x_tracer_hor_diff_params;
/* tracer_hor_diff_init(Time, G, GV, US, param_file, diag, EOS, diabatic_CSp, CS) :1630: keeps the parameters and allocates the
 * work arrays (three 2-D planes and the copies of the tile edges for eight tracers).                                           */
int mom6x_tracer_hor_diff_init(mom6x_ctx *ctx, const mom6x_tracer_hor_diff_params *p);
/* tracer_hordiff(h, dt, MEKE, VarMix, visc, G, GV, US, CS, Reg, tv) :119 on the context's stream.  tracers: the registry, a HOST
 * array of ntr 3-D device arrays, updated in place on the computational domain; each iteration starts with the context's group
 * pass of all of them (:545), so their halos are filled on return from the values before the last iteration.  h is read one
 * point into the halo and never passed: the caller owes that halo.  conc_underflow: ntr HOST values (Reg%Tr(m)%conc_underflow,
 * :605) or NULL for none.  L2u, SN_u, L2v, SN_v, Res_fn_h, Rd_dx_h (VarMix) and MEKE_Kh (MEKE%Kh): 2-D device planes owned by
 * the caller, h-point ones valid one point into the halo; NULL when absent, and a term that is switched on without its plane is
 * an error that names the field.  df_x, df_y: NULL or HOST arrays of ntr nullable 3-D device arrays (Reg%Tr(m)%df_x / df_y,
 * :581-588) that receive the fluxes summed over the iterations at I = isc-1..iec, j = jsc..jec | i = isc..iec, J = jsc-1..jec;
 * other points keep what they held.  khdt_x_out, khdt_y_out (2-D, the same face ranges), cfl_out (2-D, the computational domain,
 * written with CHECK_DIFFUSIVE_CFL only) and num_itts_out are optional outputs.  Without CHECK_DIFFUSIVE_CFL the call neither
 * synchronises nor allocates.  With no tracers, or KHTR <= 0 without variable mixing, nothing is written (:199).
 * Not carried: the 2-D flux diagnostics df2d_x / df2d_y, the Kh_u / Kh_v / Kh_h diagnostics, DEBUG checksums.                   */
int mom6x_tracer_hordiff(mom6x_ctx *ctx, const double *h, double dt, double *const *tracers, const double *conc_underflow, int ntr,
                         const double *L2u, const double *SN_u, const double *L2v, const double *SN_v, const double *Res_fn_h,
                         const double *Rd_dx_h, const double *MEKE_Kh, double *const *df_x, double *const *df_y, double *khdt_x_out,
                         double *khdt_y_out, double *cfl_out, int *num_itts_out);
/* The extents of the iteration kernel's tile (columns, rows) and the number of tracers it carries per launch.                   */
int mom6x_tracer_hordiff_tile(int *tx, int *ty, int *max_tracers);
/* The neutral branch of tracer_hordiff (:479-539), an entry of its own: a host that uses neutral diffusion LEAVES
 * use_neutral_diffusion = 0 (mom6x_tracer_hor_diff_init goes on refusing it) and calls this in place of mom6x_tracer_hordiff.  It
 * needs mom6x_tracer_hor_diff_init and mom6x_neutral_diffusion_init.  khdt_x, khdt_y and the iteration count are formed exactly as
 * in mom6x_tracer_hordiff (one code path); then the group pass of the registry (:483), neutral_diffusion_calc_coeffs with T, S (tv%T,
 * tv%S, which may be members of `tracers`) and p_surf (tv%p_surf or NULL), Coef_x, Coef_y = I_numitts * khdt on nk + 1 planes
 * (:494-507) and, per iteration, the group pass for itt > 1, calc_coeffs again under recalc_neutral_surf, and neutral_diffusion with
 * I_numitts * dt (:525-539).  tendency, trans_x_2d, trans_y_2d: as in mom6x_neutral_diffusion; they hold the LAST iteration's values,
 * as the reference's posted diagnostics do.  The other arguments are mom6x_tracer_hordiff's.                                      */
int mom6x_tracer_hordiff_neutral(mom6x_ctx *ctx, const double *h, double dt, double *const *tracers, const double *conc_underflow,
                                 int ntr, const double *L2u, const double *SN_u, const double *L2v, const double *SN_v,
                                 const double *Res_fn_h, const double *Rd_dx_h, const double *MEKE_Kh, const double *T, const double *S,
                                 const double *p_surf, double *const *tendency, double *const *trans_x_2d, double *const *trans_y_2d,
                                 double *khdt_x_out, double *khdt_y_out, double *cfl_out, int *num_itts_out);

/* ------------------------------------------------------------------------- */
/* MOM_lateral_mixing_coeffs: calc_slope_functions                            */
/* VarMix_CS (src/parameterizations/lateral/MOM_lateral_mixing_coeffs.F90:38-215; VarMix_init :1445-2054): the members that
 * calc_slope_functions (:686-738) and its callees read: calc_isoneutral_slopes (src/core/MOM_isopycnal_slopes.F90:31-608),
 * calc_Eady_growth_rate_2D (:962-1112), calc_Visbeck_coeffs_old (:743-959, without open boundaries) and
 * calc_slope_functions_using_just_e (:1116-1275), on a Boussinesq grid.  The members marked "must be 0" are refused with
 * MOM6X_EUNSUPPORTED.                                                                                                      */
/* Of the members marked "must be 0" the reference's own VarMix_init (compiled, tests/test_ref_parity_cpu.py LATERAL_REFUSALS)
 * stops only on USE_STANLEY_ISO without STANLEY_COEFF >= 0 (:1621) and accepts it with one; DEBUG it accepts; open_bcs and
 * non_Boussinesq are no parameters of it (the OBC pointer, GV%Boussinesq).  Both stop on USE_SIMPLER_EADY_GROWTH_RATE without
 * USE_STORED_SLOPES (:1722).                                                                                                */
typedef struct mom6x_varmix_params {
  int    calculate_Eady_growth_rate;   /* CS%calculate_Eady_growth_rate (:1604); 0: mom6x_calc_slope_functions writes nothing (:708) */
  int    use_stored_slopes;            /* USE_STORED_SLOPES (F, :1589)                                                              */
  int    use_simpler_Eady_growth_rate; /* USE_SIMPLER_EADY_GROWTH_RATE (F, :1718); needs use_stored_slopes (:1722)                  */
  int    full_depth_Eady_growth_rate;  /* FULL_DEPTH_EADY_GROWTH_RATE (F when Boussinesq, :1743)                                    */
  double kappa_smooth;                 /* KD_SMOOTH (1e-6 m2 s-1, :1704) [H Z T-1]                                                  */
  double Visbeck_S_max;                /* VISBECK_MAX_SLOPE (0, :1689) [Z L-1]; the limiter acts when its square is > 0 (:882)      */
  double Visbeck_L_scale;              /* VISBECK_L_SCALE (0, :1755) [L], or when negative a nondimensional factor on the face areas */
  double Eady_GR_D_scale;              /* EADY_GROWTH_RATE_D_SCALE (0, :1725) [Z]; <= 0: 64*max_depth (:991)                        */
  double cropping_distance;            /* EADY_GROWTH_RATE_CROPPING_DISTANCE (0, :1729) [Z]; negative: no cropping (:993)           */
  int    VarMix_Ktop;                  /* VARMIX_KTOP (2, :1734); must be >= 2 (layer k-1 is read, :1203)                           */
  double h_min_N2;                     /* MIN_DZ_FOR_SLOPE_N2 (1 m, :1738) [H]                                                      */
  double max_depth;                    /* GV%max_depth [Z] (:991)                                                                   */
  double H_to_Z;                       /* GV%H_to_Z (1): find_eta, dzaL / dzaR                                                      */
  double Z_to_L;                       /* US%Z_to_L (1): mag_grad2 (MOM_isopycnal_slopes.F90:390)                                   */
  double L_to_m;                       /* US%L_to_m (1): L2u, L2v with a negative VISBECK_L_SCALE (:1764)                           */
  double H_to_RZ;                      /* GV%H_to_RZ (Rho0): pres (MOM_isopycnal_slopes.F90:245)                                    */
  double Z_to_H_fill;                  /* US%Z_to_m*GV%m_to_H (1) of vert_fill_TS (MOM_isopycnal_slopes.F90:655) [H Z-1]            */
  double Angstrom_Z;                   /* GV%Angstrom_Z (1e-10 m) [Z]: dZ_cutoff (:1160)                                            */
  double g_Earth;                      /* GV%g_Earth [L2 Z-1 T-2]                                                                   */
  double Rho0;                         /* GV%Rho0 [R]: G_Rho0 (MOM_isopycnal_slopes.F90:173)                                        */
  int    use_stanley_iso;              /* USE_STANLEY_ISO (F, :1614): must be 0                                                     */
  int    open_bcs;                     /* open boundaries (OBC associated; G%OBCmaskCu/v differ from mask2dCu/v): must be 0         */
  int    non_Boussinesq;               /* tv%SpV_avg allocated or GV%semi_Boussinesq: must be 0                                     */
  int    debug;                        /* DEBUG (F): the checksums of :948-957, :995-999, :1107-1110: must be 0                     */
} mom6x_varmix_params;
/* VarMix_init :1445 for the members above: checks them (use_simpler_Eady_growth_rate without use_stored_slopes is the reference's
 * own fatal error, :1722), keeps them and allocates every work array calc_slope_functions will need.  The context's halo must be
 * at least two wide.  eos: tv%eqn_of_state (NULL: layers of constant density, slopes from GV%Rlay).  Rlay, g_prime: GV%Rlay,
 * GV%g_prime, HOST arrays of nk values, copied.  L2u, L2v: nullable 2-D DEVICE planes that receive CS%L2u, CS%L2v (:1759-1772):
 * Visbeck_L_scale**2 at every point of the array or, when the scale is negative, (L_to_m*Visbeck_L_scale)**2 * areaCu | areaCv at
 * I = isc-1..iec, j = jsc..jec | i = isc..iec, J = jsc-1..jec and zero elsewhere.                                                 */
int mom6x_varmix_init(mom6x_ctx *ctx, const mom6x_varmix_params *p, const mom6x_eos_params *eos, const double *Rlay,
                      const double *g_prime, double *L2u, double *L2v);
/* calc_slope_functions(h, tv, dt, G, GV, US, CS, OBC) :686 on the context's stream, without an exchange, a host synchronisation
 * or an allocation.  h, T, S and tv%p_surf (nullable) need TWO valid halo points (find_eta(halo_size=2), vert_fill_TS(halo+1));
 * T, S are required with an EOS.  SN_u, SN_v: CS%SN_u, CS%SN_v, 2-D planes.  slope_x, slope_y: CS%slope_x, CS%slope_y, the 3-D
 * interface arrays of nk+1 planes that mom6x_thickness_diffuse takes; required with use_stored_slopes (both branches that call
 * calc_isoneutral_slopes), not touched otherwise.  Nullable diagnostics, each of nk+1 planes unless noted: N2_u, N2_v (the
 * use_stored_slopes branch posts them; filled in both slope branches), dzu, dzv, dzSxN, dzSyN (use_simpler_Eady_growth_rate),
 * S2_u, S2_v (2-D planes, calc_Visbeck_coeffs_old :944-945).
 * What is written, everything else keeps its value:
 *   calc_isoneutral_slopes(halo=1): slope_x, N2_u, dzu, dzSxN at I = isc-2..iec+1, j = jsc-1..jec+1 and slope_y, N2_v, dzv, dzSyN
 *     at i = isc-1..iec+1, J = jsc-2..jec+1, interfaces 2..nk; planes 1 and nk+1 of N2 and dz* are zeroed there, those of the
 *     slopes are not touched;
 *   use_simpler_Eady_growth_rate: SN_u and SN_v on isc-1..iec+1 x jsc-1..jec+1 (:1002-1005, :1045, :1088, :1094, :1101);
 *   use_stored_slopes alone: SN_u, SN_v zeroed at every point of the array (:798-799), then set at I = isc-1..iec, j = jsc..jec |
 *     i = isc..iec, J = jsc-1..jec, as are S2_u, S2_v;
 *   neither: SN_u, SN_v at I = isc-1..iec, j = jsc..jec | i = isc..iec, J = jsc-1..jec.
 * With calculate_Eady_growth_rate = 0 nothing is written.                                                                       */
int mom6x_calc_slope_functions(mom6x_ctx *ctx, const double *h, const double *T, const double *S, const double *p_surf, double dt,
                               double *SN_u, double *SN_v, double *slope_x, double *slope_y, double *N2_u, double *N2_v,
                               double *dzu, double *dzv, double *dzSxN, double *dzSyN, double *S2_u, double *S2_v);

/* ------------------------------------------------------------------------- */
/* MOM_mixed_layer_restrat: mixedlayer_restrat (Fox-Kemper, the OM4 path)     */
/* mixedlayer_restrat_CS (src/parameterizations/lateral/MOM_mixed_layer_restrat.F90:37-140; mixedlayer_restrat_init :1617-1958):
 * the members that mixedlayer_restrat_OM4 (:189-714), detect_mld (:1504-1571) and mu (:717-751) read on a Boussinesq grid in
 * general coordinates.  GV%Angstrom_H, GV%H_subroundoff, GV%H_to_Z, GV%Z_to_H, GV%g_Earth and GV%Rho0 are the context's
 * (mom6x_vgrid).  The members marked "must be 0" are refused with MOM6X_EUNSUPPORTED.                                          */
typedef struct mom6x_mixedlayer_restrat_params {
  double ml_restrat_coef;      /* FOX_KEMPER_ML_RESTRAT_COEF (0, :1786): scales the fast timescale (:510)                        */
  double ml_restrat_coef2;     /* FOX_KEMPER_ML_RESTRAT_COEF2 (0, :1812): scales the slow timescale (:525)                       */
  double front_length;         /* MLE_FRONT_LENGTH (0, :1815) [L]; > 0: the resolution upscaling with this length (:355-359);
                                  0 with an mle_fl plane: MLE_FRONT_LENGTH_FROM_FILE (:360-363); otherwise no upscaling          */
  int    MLE_use_PBL_MLD;      /* MLE_USE_PBL_MLD (F, :1844): MLD_fast = MLE_MLD_stretch*h_MLD (:304) when MLE_density_diff <= 0  */
  double MLE_MLD_decay_time;   /* MLE_MLD_DECAY_TIME (0, :1849) [T]; > 0: the running mean of :317-325 on MLD_filtered           */
  double MLE_MLD_decay_time2;  /* MLE_MLD_DECAY_TIME2 (0, :1854) [T]; > 0: the slow running mean of :335-343                     */
  double MLE_density_diff;     /* MLE_DENSITY_DIFF (0.03 kg m-3, :1860; not read with MLE_USE_PBL_MLD) [R]; > 0: detect_mld      */
  double MLE_tail_dh;          /* MLE_TAIL_DH (0, :1865): the extension of the stream function below the mixed layer (mu :739)    */
  double MLE_MLD_stretch;      /* MLE_MLD_STRETCH (1, :1869)                                                                     */
  double vonKar;               /* VON_KARMAN_CONST (0.41, :1806)                                                                 */
  double ustar_min;            /* RESTRAT_USTAR_MIN as :1882-1887 leave it in CS%ustar_min [H T-1]                               */
  int    use_Bodner;           /* MLE%USE_BODNER23 (mixedlayer_restrat_Bodner): must be 0                                        */
  int    nkml;                 /* GV%nkml (mixedlayer_restrat_BML): must be 0                                                    */
  int    use_Stanley_ML;       /* USE_STANLEY_ML (F, :1796): must be 0                                                           */
  int    non_Boussinesq;       /* not GV%Boussinesq, or semi-Boussinesq (calculate_spec_vol :427-471, tau_mag in find_ustar): must be 0 */
  int    open_bcs;             /* open boundaries (G%OBCmaskCu/v differ from mask2dCu/v): must be 0                              */
  int    debug;                /* DEBUG (F, :1671): the checksums of :313-334, :473-479: must be 0                               */
} mom6x_mixedlayer_restrat_params;
/* mixedlayer_restrat_init :1617 for the members above: checks them, keeps them and allocates every work array the step needs
 * (four 2-D planes and uhml, vhml).  eos: tv%eqn_of_state, required (the reference's fatal error, :288).  MOM6X_EINVAL when
 * MLE_density_diff <= 0 without MLE_use_PBL_MLD (:306).                                                                         */
int mom6x_mixedlayer_restrat_init(mom6x_ctx *ctx, const mom6x_mixedlayer_restrat_params *p, const mom6x_eos_params *eos);
/* mixedlayer_restrat(h, uhtr, vhtr, tv, forces, dt, MLD, h_MLD, bflux, VarMix, G, GV, US, CS) :149 on the context's stream, without
 * an exchange, a host synchronisation or an allocation.  h, uhtr, vhtr are updated in place; T, S are tv%T, tv%S; ustar is
 * forces%ustar [Z T-1] (the device forms GV%Z_to_H*ustar as find_ustar(H_T_units=.true.) does, MOM_forcing_type.F90:1271).
 * h_MLD: the boundary-layer scheme's mixed-layer thickness [H], required with MLE_use_PBL_MLD when MLE_density_diff <= 0.
 * Rd_dx_h: VarMix%Rd_dx_h, required whenever the resolution upscaling is on.  mle_fl: nullable plane of the frontal length [L]
 * (with front_length == 0 it is the MLE_FRONT_LENGTH_FROM_FILE arm; the host keeps time_interp_external, its halo pass and the
 * sign check :364-371).  MLD_filtered, MLD_filtered_slow: CS%MLD_filtered, CS%MLD_filtered_slow (the restart fields
 * MLD_MLE_filtered and MLD_MLE_filtered_slow), the caller's resident planes, each required when its decay time is > 0 and
 * updated in place on isc-1..iec+1 x jsc-1..jec+1.  The remaining arguments are nullable diagnostics as the reference posts them:
 * uhml, vhml (3-D), utimescale, vtimescale (the value the reference stores, the slow one: :572, :662), uDml, vDml (after the
 * limiter), MLD_fast_out (id_BLD), MLD_slow_out (id_MLD), Rml_av_fast_out (id_Rml), the last three on isc-1..iec+1 x jsc-1..jec+1.
 * h, T, S, ustar, h_MLD, Rd_dx_h, mle_fl and the two filtered planes need ONE valid halo point.
 * Written: uhtr, uhml, utimescale, uDml at I = isc-1..iec, j = jsc..jec; vhtr, vhml, vtimescale, vDml at i = isc..iec,
 * J = jsc-1..jec (uhtr, vhtr keep their bits at a face whose uDml + uDml_slow is zero, :531); h on the computational domain.
 * Every other point keeps its value, and the caller still owes pass_var(h).
 * Not carried: the id_uml / id_vml diagnostics, DEBUG checksums, diag_update_remap_grids.                                        */
int mom6x_mixedlayer_restrat(mom6x_ctx *ctx, double *h, double *uhtr, double *vhtr, const double *T, const double *S,
                             const double *ustar, double dt, const double *h_MLD, const double *Rd_dx_h, const double *mle_fl,
                             double *MLD_filtered, double *MLD_filtered_slow, double *uhml, double *vhml, double *utimescale,
                             double *vtimescale, double *uDml, double *vDml, double *MLD_fast_out, double *MLD_slow_out,
                             double *Rml_av_fast_out);
/* A test hook: the device's mu(sigma, dh) (:717) at n values; sigma, dh and out are DEVICE arrays of n.                          */
int mom6x_mixedlayer_restrat_mu(mom6x_ctx *ctx, const double *sigma, const double *dh, double *out, int n);

/* ------------------------------------------------------------------------- */
/* MOM_MEKE: step_forward_MEKE (mesoscale eddy kinetic energy, EKE_SOURCE = prog) */
/* MEKE_CS (src/parameterizations/lateral/MOM_MEKE.F90:54-168; MEKE_init :1329-1750): the members that the EKE_SOURCE = prog arm of
 * step_forward_MEKE (:174-982), MEKE_equilibrium (:987), MEKE_equilibrium_restoring (:1148), MEKE_lengthScales (:1183) and
 * MEKE_lengthScales_0d (:1258) read on a Boussinesq grid with G%Z_ref = 0.  GV%H_to_RZ, GV%RZ_to_H, GV%Z_to_H and GV%H_subroundoff
 * are the context's (mom6x_vgrid).  Logicals are ints.  The members marked "must be 0" are refused with MOM6X_EUNSUPPORTED.     */
typedef struct mom6x_MEKE_params {
  double MEKE_damping;          /* MEKE_DAMPING (0, :1400) [T-1]: the depth-independent dissipation rate (:542)                    */
  double MEKE_Cd_scale;         /* MEKE_CD_SCALE (0, :1403): gamma_b of :1283                                                      */
  double MEKE_Cb;               /* MEKE_CB (25, :1408): > 0 brings the **0.8 of :1284                                              */
  double MEKE_min_gamma;        /* MEKE_MIN_GAMMA2 (1e-4, :1412)                                                                   */
  double MEKE_Ct;               /* MEKE_CT (50, :1415): > 0 brings the **0.25 of :1289                                             */
  double MEKE_GMcoeff;          /* MEKE_GMCOEFF (-1, :1419): scales MEKE%GM_src (:486-503); < 0: MEKE_src_GM is not registered     */
  int    MEKE_GEOMETRIC;        /* MEKE_GEOMETRIC (F, :1424): MEKE%Kh is not written (:883)                                        */
  double MEKE_GEOMETRIC_alpha;  /* MEKE_GEOMETRIC_ALPHA (0.05, :1427): the two equilibrium formulas :1037, :1174                   */
  int    MEKE_equilibrium_alt;  /* MEKE_EQUILIBRIUM_ALT (F, :1430): the closed form :1037 instead of the root find                 */
  int    MEKE_equilibrium_restoring; /* MEKE_EQUILIBRIUM_RESTORING (F, :1433): the nudging of :505-511                            */
  double MEKE_restoring_rate;   /* 1 / MEKE_RESTORING_TIMESCALE (1e6 s, :1437-1440) [T-1]                                          */
  double MEKE_FrCoeff;          /* MEKE_FRCOEFF (-1, :1443): > 0 reads MEKE%mom_src (:444)                                         */
  double MEKE_bhFrCoeff;        /* MEKE_BHFRCOEFF (-1, :1447): scales MEKE%mom_src_bh (:451-461)                                   */
  double MEKE_GMECoeff;         /* MEKE_GMECOEFF (-1, :1451): scales MEKE%GME_snk (:479-484)                                       */
  double MEKE_BGsrc;            /* MEKE_BGSRC (0, :1455) [L2 T-3]                                                                  */
  double MEKE_Kh;               /* MEKE_KH (-1, :1458) [L2 T-1]; >= 0: Laplacian diffusion and the Strang split                    */
  double MEKE_K4;               /* MEKE_K4 (-1, :1462) [L4 T-1]; >= 0: biharmonic diffusion (needs a halo of two)                  */
  double MEKE_dtScale;          /* MEKE_DTSCALE (1, :1466)                                                                         */
  int    MEKE_positive;         /* MEKE_POSITIVE (F, :1469): MEKE = MAX(0, MEKE) at :870                                           */
  double MEKE_KhCoeff;          /* MEKE_KHCOEFF (1, :1480): > 0 writes MEKE%Kh (:882)                                              */
  double MEKE_Uscale;           /* MEKE_USCALE (0, :1487) [L T-1]                                                                  */
  int    GM_src_alt;            /* MEKE_GM_SRC_ALT (F, :1490): the GM source over the total depth (:487-492)                       */
  double MEKE_min_depth_tot;    /* MEKE_MIN_DEPTH_TOT (1 m, :1493) [H]                                                             */
  int    visc_drag;             /* MEKE_VISC_DRAG (T, :1497): drag_rate_visc from visc%Kv_bbl_u/v, visc%bbl_thick_u/v (:330-351)    */
  double KhMEKE_Fac;            /* MEKE_KHMEKE_FAC (0, :1504): MEKE%Kh in the diffusivity of MEKE itself (:687-689)                */
  int    use_old_lscale;        /* MEKE_OLD_LSCALE (F, :1507)                                                                      */
  int    use_min_lscale;        /* MEKE_MIN_LSCALE (F, :1511)                                                                      */
  double lscale_maxval;         /* MEKE_LSCALE_MAX_VAL (1e7 m, :1515) [L]                                                          */
  int    Rd_as_max_scale;       /* MEKE_RD_MAX_SCALE (F, :1520)                                                                    */
  double viscosity_coeff_Ku;    /* MEKE_VISCOSITY_COEFF_KU (0, :1524): /= 0 writes MEKE%Ku (:910)                                  */
  double viscosity_coeff_Au;    /* MEKE_VISCOSITY_COEFF_AU (0, :1530): /= 0 writes MEKE%Au (:916)                                  */
  double Lfixed;                /* MEKE_FIXED_MIXING_LENGTH (0, :1536) [L]                                                         */
  int    fixed_total_depth;     /* MEKE_FIXED_TOTAL_DEPTH (T, :1540): depth_tot from G%bathyT (:371-376) instead of the mass       */
  double aDeform;               /* MEKE_ALPHA_DEFORM (0, :1550)                                                                    */
  double aRhines;               /* MEKE_ALPHA_RHINES (0, :1554)                                                                    */
  double aEady;                 /* MEKE_ALPHA_EADY (0, :1558)                                                                      */
  double aFrict;                /* MEKE_ALPHA_FRICT (0, :1562)                                                                     */
  double aGrid;                 /* MEKE_ALPHA_GRID (0, :1566)                                                                      */
  double MEKE_advection_factor; /* MEKE_ADVECTION_FACTOR (0, :1580): > 0 reads hu, hv                                              */
  int    MEKE_advection_bug;    /* MEKE_ADVECTION_BUG (F, :1585): the transports of layer nz only (:317-326)                       */
  double MEKE_topographic_beta; /* MEKE_TOPOGRAPHIC_BETA (0, :1589)                                                                */
  double cdrag;                 /* MEKE_CDRAG (CDRAG = 0.003) times US%L_to_m*GV%m_to_H, as :1602-1604 leave it [H L-1]             */
  double T_to_s;                /* US%T_to_s (1): the floors of :1299, :1301                                                       */
  double L_to_m;                /* US%L_to_m (1): the floor of :1299                                                               */
  double m_s_to_L_T;            /* US%m_s_to_L_T (1): the bracket and the tolerance of MEKE_equilibrium (:1027, :1065, :1094)      */
  int    cold_start;            /* MEKE_COLD_START (F, :1570): CS%initialize is false from the start (:1721)                       */
  int    eke_source_file;       /* EKE_SOURCE = file (:1385-1396): must be 0                                                       */
  int    eke_source_dbclient;   /* EKE_SOURCE = dbclient (ML_MEKE_init): must be 0                                                 */
  int    use_Kh_diff;           /* USE_KH_IN_MEKE, MEKE%Kh_diff allocated (:690, :707, :1734): must be 0                           */
  int    non_Boussinesq;        /* not GV%Boussinesq (:377-381, MEKE_TOTAL_DEPTH_RHO): must be 0                                   */
  int    open_bcs;              /* open boundaries (G%OBCmaskCu/v differ from mask2dCu/v, :620, :630): must be 0                   */
  int    debug;                 /* DEBUG (F, :1614): the checksums of :272-287, :397-406, :513, :851: must be 0                    */
} mom6x_MEKE_params;
/* MEKE_init :1329 for the members above: checks them, keeps them, sets CS%kh_flux_enabled (:1617-1619) and CS%initialize =
 * .not. cold_start (:1720-1721: a new run), and allocates every work plane the step needs.  dF_dx, dF_dy: G%dF_dx, G%dF_dy, HOST
 * planes at h points in the tile layout, copied; read at i = isc..iec, j = jsc..jec; required unless use_old_lscale.  The context
 * needs a halo of two with MEKE_K4 >= 0 and of one otherwise.  Left to the host: the checks of LAPLACIAN / BIHARMONIC against the
 * two viscosity coefficients (:1608-1612), MEKE%Le = sqrt(areaT) of a new run (:1724-1729) and the two group passes of
 * :1735, :1742-1744 (mom6x_pass_fields).                                                                                          */
int mom6x_MEKE_init(mom6x_ctx *ctx, const mom6x_MEKE_params *p, const double *dF_dx, const double *dF_dy);
/* The restart arm of :1720: initialized != 0 says that MEKE%MEKE came from a restart file, CS%initialize is cleared and the next
 * step does not call MEKE_equilibrium; the host then owes the halo update of :1735.  initialized = 0 sets it again (unless
 * cold_start).                                                                                                                   */
int mom6x_MEKE_set_initialized(mom6x_ctx *ctx, int initialized);
/* step_forward_MEKE(MEKE, h, SN_u, SN_v, visc, dt, G, GV, US, CS, hu, hv, ...) :174 on the context's stream, without a host
 * synchronisation or an allocation; the reference's group passes (:611 with kh_flux_enabled or MEKE_K4 >= 0, :878 always, :925 of
 * whichever of Kh, Ku, Au, Le are given) run inside through the context's halo layer.  All arrays are DEVICE arrays.
 * MEKE, Kh, Ku, Au, Le: MEKE%MEKE, MEKE%Kh, MEKE%Ku, MEKE%Au, MEKE%Le, the caller's resident planes (the restart fields MEKE,
 * MEKE_Kh, MEKE_Ku, MEKE_Au, MEKE_Le), updated in place; the last four are nullable, NULL meaning "not allocated"
 * (MEKE_alloc_register_restart :2074-2113).  GM_src, mom_src, mom_src_bh, GME_snk: MEKE%GM_src ..., nullable with the same
 * meaning.  Rd_dx_h: MEKE%Rd_dx_h, NULL stands for the zeros of :2088.  Kv_bbl_u, Kv_bbl_v, bbl_thick_u, bbl_thick_v: the members
 * of visc; with visc_drag off or any of them NULL drag_rate_visc is 0 (:330, :352).  hu, hv: the accumulated mass fluxes (uhtr,
 * vhtr), read with MEKE_advection_factor > 0 only.  MOM6X_EINVAL, naming the plane, when a coefficient asks for an absent one
 * (mom_src with MEKE_FrCoeff > 0 or with MEKE_src_mom_lp wanted; Kh with MEKE_KhCoeff > 0 unless MEKE_GEOMETRIC; Ku, Au with their
 * coefficients; hu, hv): the reference would fault there.
 * Read: h at i = isc-1..iec+1, j = jsc-1..jec+1 (ONE valid halo point), all layers in the order k = 1..nz; hu at I = isc-1..iec,
 * j = jsc..jec, hv at i = isc..iec, J = jsc-1..jec; SN_u, Kv_bbl_u, bbl_thick_u and SN_v, Kv_bbl_v, bbl_thick_v on the same
 * faces; the four sources, Rd_dx_h and MEKE on the computational domain; Kh on isc-1..iec+1 x jsc-1..jec+1 when given and
 * kh_flux_enabled (its halo is the previous call's).
 * Written: MEKE on the computational domain and then its whole halo by the passes (with MEKE_K4 >= 0 two halo points are read
 * after the first pass); Kh (unless MEKE_GEOMETRIC or MEKE_KhCoeff <= 0), Ku, Au (with their coefficients) and Le (always, :411) on
 * the computational domain and then their halos by the pass of :925.  Every other point keeps its value.
 * The remaining arguments are nullable diagnostics, written on the computational domain (Kh_u at I = isc-1..iec, j = jsc..jec,
 * Kh_v at i = isc..iec, J = jsc-1..jec) as the reference posts them; a given plane plays the role of id_* > 0, so the `damping`
 * factors of :556-606 and :792-848 are applied exactly when src_GM, src_mom_lp, src_mom_bh or src_btm_drag (first stage) or any of
 * those, src_adv or src_mom_K4 (second stage) is given.  As in the reference, decay is written only inside those two blocks.  A
 * plane whose diagnostic the reference does not register is left alone: src_mom_K4 with MEKE_K4 < 0 (:1653), src_GM with
 * MEKE_GMcoeff < 0, src_mom_lp with MEKE_FrCoeff < 0, src_mom_bh with MEKE_bhFrCoeff < 0, Kh_u, Kh_v without kh_flux_enabled; so are
 * LRhines and LEady with use_old_lscale, where MEKE_lengthScales_0d does not set them.  Ue, Ub, Ut: :933-949; gamma_b, gamma_t:
 * the square roots of :969-979.
 * MEKE_equilibrium runs on the first call while CS%initialize is set; its two `stop`s (:1095, :1133) raise the context's numeric
 * flag (bit 64; MOM6X_ENUMERIC at the next mom6x_ctx_sync, whose message names MEKE_equilibrium) instead.
 * ONE DELIBERATE DEPARTURE.  When neither MEKE%Kh nor MEKE%Kh_diff is allocated, the reference sets Kh_here = max(0, MEKE_Kh) once
 * before each face loop (:683, :703 firstprivate) and the CFL limiter of :695 | :710 overwrites it: once the limiter has fired at
 * one face its result is carried to every later face of a serial sweep, or of one thread's share with OpenMP, so the reference's
 * answer there depends on the traversal order and on the layout.  The device forms max(0, MEKE_Kh) at every face and limits it
 * there.  The two agree wherever the limiter does not fire in that arm; with MEKE%Kh given the reference resets Kh_here at every
 * face and there is no difference.
 * Not carried: EKE_SOURCE = file | dbclient, MEKE%Kh_diff, the DEBUG checksums, the id_MEKE_equilibrium diagnostic.               */
int mom6x_step_forward_MEKE(mom6x_ctx *ctx, double *MEKE, const double *h, const double *SN_u, const double *SN_v,
                            const double *Kv_bbl_u, const double *Kv_bbl_v, const double *bbl_thick_u, const double *bbl_thick_v,
                            double dt, const double *hu, const double *hv, const double *Rd_dx_h, const double *GM_src,
                            const double *mom_src, const double *mom_src_bh, const double *GME_snk, double *Kh, double *Ku, double *Au,
                            double *Le, double *src, double *src_adv, double *src_mom_K4, double *src_btm_drag, double *src_GM,
                            double *src_mom_lp, double *src_mom_bh, double *decay, double *Kh_u, double *Kh_v, double *LmixScale,
                            double *LRhines, double *LEady, double *Ue, double *Ub, double *Ut, double *gamma_b, double *gamma_t);

/* ------------------------------------------------------------------------- */
/* MOM_set_diffusivity: set_BBL_TKE and set_diffusivity (diapycnal diffusivities, the ALE-coordinate path)                       */
/* set_diffusivity_CS (src/parameterizations/vertical/MOM_set_diffusivity.F90:57-228; set_diffusivity_init :2262-2700) and the
 * bkgnd_mixing_cs it owns (MOM_bkgnd_mixing.F90:40-100; bkgnd_mixing_init :107-320): the members that set_BBL_TKE (:1947-2152),
 * set_diffusivity (:243-868), find_N2 (:1095), double_diffusion (:1279), add_LOTW_BBL_diffusivity (:1606) and the `else` arm of
 * calculate_bkgnd_mixing (MOM_bkgnd_mixing.F90:450-516) read on a Boussinesq grid in general coordinates.  Values are in the
 * reference's scaled units, as its get_param calls leave them; GV%H_to_Z, Z_to_H, H_to_RZ, RZ_to_H, g_Earth, H_subroundoff and
 * dZ_subroundoff are the context's (mom6x_vgrid).  Logicals are ints.  The members marked "must be 0" are refused with
 * MOM6X_EUNSUPPORTED.                                                                                                           */
typedef struct mom6x_set_diffusivity_params {
  double Kd;                    /* KD (0, :2508-2512) [H Z T-1]: the fill of Kd_int, Kd_lay (:370-371) and the background            */
  double Kd_min;                /* KD_MIN (0.01*KD, :2513) [H Z T-1]: the floor of Kd_sfc (MOM_bkgnd_mixing.F90:457, :465)           */
  double Kd_max;                /* KD_MAX (-1, :2516) [H Z T-1]: Kd_wall where no TKE is consumed (:1771); > 0 with the law of the wall */
  double Kd_add;                /* KD_ADD (0, :2529) [H Z T-1]: added to every interface and layer (:698-701, :732-736)              */
  double Kv;                    /* KV (none, :2503) [H Z T-1]: the fill of visc%Kv_slow (:374)                                       */
  double Kd_smooth;             /* KD_SMOOTH (1e-6, :2536) [H Z T-1]: kappa_dt_fill = Kd_smooth*dt (:354)                            */
  double FluxRi_max;            /* FLUX_RI_MAX (0.2, :2339): the floors (:693, :721) and dissip_N2 (:2569)                           */
  double omega;                 /* OMEGA (7.2921e-5, :2344) [T-1]: Omega2 (:356), N2_min of the law of the wall (:1667)              */
  int    answer_date;           /* SET_DIFF_ANSWER_DATE (99991231, :2350): < 20190101 takes kappa_dt_fill of :352                    */
  int    bottomdraglaw;         /* BOTTOMDRAGLAW (T, :2417); F: set_BBL_TKE zeroes its planes (:2007), no bottom-drag mixing         */
  double cdrag;                 /* CDRAG (0.003, :2423): cdrag_sqrt of set_BBL_TKE (:2021)                                           */
  double BBL_effic;             /* BBL_EFFIC (0.2, :2427) times US%L_to_Z**2: TKE_column (:1709), the Rayleigh term (:1733)          */
  double ePBL_BBL_effic;        /* EPBL_BBL_EFFIC (0, :2431): only in the early return of set_BBL_TKE (:2007)                        */
  int    ePBL_BBL_mstar;        /* EPBL_BBL_USE_MSTAR (F, :2433): likewise                                                           */
  double BBL_mixing_max_decay;  /* BBL_MIXING_MAX_DECAY (200 m, :2435) [H]: IMax_decay = 1/it when > 0, else 0 (:2441-2442)          */
  int    use_LOTW_BBL_diffusivity; /* USE_LOTW_BBL_DIFFUSIVITY (F, :2448); F with BOTTOMDRAGLAW and BBL_EFFIC > 0 is refused         */
  int    LOTW_BBL_use_omega;    /* LOTW_BBL_USE_OMEGA (T, :2453): N2_min = omega**2 (:1667)                                          */
  double von_Karm;              /* VON_KARMAN_BBL (VON_KARMAN_CONST = 0.41, :2456-2461)                                              */
  int    LOTW_BBL_answer_date;  /* LOTW_BBL_ANSWER_DATE (20190101, :2466): > 20240630 takes dz_above (:1712-1717, :1745)             */
  double dissip_min;            /* DISSIPATION_MIN (0, :2548) [R Z2 T-3 scaled as :2551]                                             */
  double dissip_N0;             /* DISSIPATION_N0 (0, :2552)                                                                         */
  double dissip_N1;             /* DISSIPATION_N1 (0, :2557)                                                                         */
  double dissip_Kd_min;         /* DISSIPATION_KD_MIN (0, :2562) [H Z T-1]; limit_dissipation and dissip_N2 are derived (:2566-2570) */
  int    double_diffusion;      /* DOUBLE_DIFFUSION (F, :2626): needs an EOS and Kd_extra_T, Kd_extra_S                              */
  double Max_Rrho_salt_fingers; /* MAX_RRHO_SALT_FINGERS (1.9, :2632)                                                                */
  double Max_salt_diff_salt_fingers; /* MAX_SALT_DIFF_SALT_FINGERS (1e-4, :2635) [H Z T-1]                                            */
  double Kv_molecular;          /* KV_MOLECULAR (1.5e-6, :2638) [H Z T-1]                                                            */
  int    use_Kd_shear;          /* useKappaShear .or. use_CVMix_shear (:2656, :2663): the host hands in visc%Kd_shear (:571-581)       */
  int    physical_OBL_scheme;   /* a physically based boundary layer scheme is on (MOM_bkgnd_mixing.F90:157): no Hmix ramp (:475)    */
  double Kd_tot_ml;             /* KD_ML_TOT | KDML (KD, MOM_bkgnd_mixing.F90:171-181) [H Z T-1]; /= Kd brings the ramp of :475-499  */
  double Hmix;                  /* HMIX_FIXED (none, MOM_bkgnd_mixing.F90:191) [H]                                                   */
  int    Kd_via_Kdml_bug;       /* KD_BACKGROUND_VIA_KDML_BUG (F, MOM_bkgnd_mixing.F90:312): the two outer arms leave Kd_lay alone   */
  double prandtl_bkgnd;         /* PRANDTL_BKGND (1, MOM_bkgnd_mixing.F90:252): Kv_bkgnd (:514)                                      */
  int    Henyey_IGW_background; /* HENYEY_IGW_BACKGROUND (F, MOM_bkgnd_mixing.F90:267): Kd_sfc of :452-459, needs geoLatT            */
  double N0_2Omega;             /* HENYEY_N0_2OMEGA (20, MOM_bkgnd_mixing.F90:280)                                                   */
  double Henyey_max_lat;        /* HENYEY_MAX_LAT (95, MOM_bkgnd_mixing.F90:287) [degN]                                              */
  int    Kd_tanh_lat_fn;        /* KD_TANH_LAT_FN (F, MOM_bkgnd_mixing.F90:293): Kd_sfc of :460-467, needs geoLatT                   */
  double Kd_tanh_lat_scale;     /* KD_TANH_LAT_SCALE (0, MOM_bkgnd_mixing.F90:300)                                                   */
  double g_Earth_Z_T2;          /* GV%g_Earth_Z_T2 (g_Earth) [Z T-2]: G_Rho0 of find_N2 (:1152)                                      */
  double Z_to_H_fill;           /* US%Z_to_m*GV%m_to_H (1): kap_dt_x2 of vert_fill_TS (MOM_isopycnal_slopes.F90:655)                 */
  double m2_s_to_HZ_T;          /* GV%m2_s_to_HZ_T (1): kappa_dt_fill of :352                                                        */
  double s_to_T;                /* US%s_to_T (1): likewise                                                                           */
  double RL2_T2_to_Pa;          /* US%RL2_T2_to_Pa (1): the pressure handed to the equation of state (MOM_EOS.F90 calculate_density_derivs_1d) */
  int    ML_radiation;          /* ML_RADIATION (F, :2363; add_MLrad_diffusivity): must be 0                                         */
  int    use_tidal_mixing;      /* tidal_mixing_init (:2360: INT_TIDE_DISSIPATION, LEE_WAVE_DISSIPATION, USE_CVMix_TIDAL): must be 0 */
  int    use_int_tides;         /* INTERNAL_TIDES (F, :2496; get_lowmode_diffusivity): must be 0                                     */
  int    use_CVMix_ddiff;       /* USE_CVMIX_DDIFF (:2666): must be 0                                                                */
  int    Bryan_Lewis_diffusivity;  /* BRYAN_LEWIS_DIFFUSIVITY (F, MOM_bkgnd_mixing.F90:201): must be 0                               */
  int    horiz_varying_background; /* HORIZ_VARYING_BACKGROUND (F, MOM_bkgnd_mixing.F90:227): must be 0                              */
  int    user_change_diff;      /* USER_CHANGE_DIFFUSIVITY (F, :2545): must be 0                                                     */
  int    nkml;                  /* GV%nkml, a bulk mixed layer (:2332): must be 0                                                    */
  int    SpV_avg;               /* tv%SpV_avg allocated, non-Boussinesq (:1690, thickness_to_dz): must be 0                          */
  int    open_bcs;              /* open boundary conditions (set_BBL_TKE :1992-1997): must be 0                                      */
} mom6x_set_diffusivity_params;
/* set_diffusivity_init :2262 with bkgnd_mixing_init for the members above: checks them, keeps them, derives IMax_decay,
 * limit_dissipation and dissip_N2, allocates the seven work arrays of the column kernel (nk + 1 levels each) and forms the
 * Kd_sfc plane.  eos: tv%eqn_of_state (NULL: layers of constant density, dRho_int from Rlay).  Rlay: GV%Rlay, a HOST array of
 * nk values, read without an EOS only.  geoLatT: G%geoLatT [degrees], a HOST plane of the tile in the pitched layout, read with
 * HENYEY_IGW_BACKGROUND or KD_TANH_LAT_FN only (required then; the metric block carries no latitude).
 * MOM6X_EUNSUPPORTED, naming the setting: every "must be 0" member, and BOTTOMDRAGLAW with BBL_EFFIC > 0 but without
 * USE_LOTW_BBL_DIFFUSIVITY (add_drag_diffusivity with find_TKE_to_Kd and set_density_ratios, the layered-mode physics).
 * MOM6X_EINVAL: USE_LOTW_BBL_DIFFUSIVITY with KD_MAX <= 0 (:2533), DOUBLE_DIFFUSION without an EOS (the reference leaves the
 * arrays unset), an EOS with nk < 2, both latitude functions at once (MOM_bkgnd_mixing.F90:305), a missing Rlay or geoLatT. */
int mom6x_set_diffusivity_init(mom6x_ctx *ctx, const mom6x_set_diffusivity_params *p, const mom6x_eos_params *eos,
                               const double *Rlay, const double *geoLatT);
/* Device arrays of the module: which = 0 the Kd_sfc plane of calculate_bkgnd_mixing :452-472 (one plane, formed over the whole
 * array at init; the constant KD without a latitude function).  NULL before init or for another index.                        */
double *mom6x_set_diffusivity_field(mom6x_ctx *ctx, int which);
/* set_BBL_TKE(u, v, h, tv, fluxes, visc, G, GV, US, CS, OBC) :1947 on the context's stream, one launch, no host synchronisation.
 * Kv_bbl_u, Kv_bbl_v, bbl_thick_u, bbl_thick_v: the planes mom6x_set_viscous_BBL leaves on the device.
 * Read: h at i = isc-1..iec+1, j = jsc-1..jec+1 (ONE valid halo point), bottom-up over bbl_thick; u, Kv_bbl_u, bbl_thick_u at
 * I = isc-1..iec, j = jsc..jec; v, Kv_bbl_v, bbl_thick_v at i = isc..iec, J = jsc-1..jec (what mom6x_set_viscous_BBL writes).
 * Written on the computational domain: ustar_BBL, BBL_meanKE_loss (visc%ustar_BBL, visc%BBL_meanKE_loss) and, when given,
 * BBL_meanKE_loss_sqrtCd.  Without BOTTOMDRAGLAW, or with BBL_EFFIC <= 0, EPBL_BBL_EFFIC <= 0 and no EPBL_BBL_USE_MSTAR, the
 * planes that are given are zeroed there and nothing is read (:2007-2019).                                                  */
int mom6x_set_BBL_TKE(mom6x_ctx *ctx, const double *u, const double *v, const double *h, const double *Kv_bbl_u,
                      const double *Kv_bbl_v, const double *bbl_thick_u, const double *bbl_thick_v, double *ustar_BBL,
                      double *BBL_meanKE_loss, double *BBL_meanKE_loss_sqrtCd);
/* set_diffusivity(u, v, h, u_h, v_h, tv, fluxes, optics, visc, dt, Kd_int, G, GV, US, CS, VBF, Kd_lay, Kd_extra_T, Kd_extra_S) :243
 * on the context's stream: two launches, no allocation, no host synchronisation, no halo exchange.
 * Inputs.  h, T, S (tv%T, tv%S, with an EOS): 3-D.  p_surf: fluxes%p_surf (find_N2 :1161), tv_p_surf: tv%p_surf
 * (double_diffusion :1326): two separately nullable planes.  Kd_shear: visc%Kd_shear (nk + 1 levels), required with use_Kd_shear.
 * ustar_BBL, BBL_meanKE_loss: the planes of mom6x_set_BBL_TKE, required with the law of the wall.  ustar_tidal, BBL_tidal_dis:
 * fluxes%ustar_tidal, fluxes%BBL_tidal_dis, nullable planes.  Ray_u, Ray_v: visc%Ray_u, visc%Ray_v (3-D, nullable, together):
 * when given the law of the wall adds the Rayleigh-drag term :1732-1737 and reads u and v, otherwise u and v may be NULL.
 * Outputs.  Kd_int (nk + 1 levels) is required.  Nullable: Kd_lay (nk levels); Kd_extra_T and Kd_extra_S (nk + 1, together,
 * required with DOUBLE_DIFFUSION, :360-363); Kv_slow, Kv_shear (visc%Kv_slow, visc%Kv_shear, nk + 1).  Nullable diagnostics,
 * nk + 1 levels each: N2_3d, Kd_BBL, Kd_bkgnd, Kv_bkgnd, KT_extra, KS_extra (dd%...).
 * Read: everything at the computational domain only (i = isc..iec, j = jsc..jec), u and Ray_u also at I = isc-1, v and Ray_v
 * at J = jsc-1, CoriolisBu at the four corners.
 * Written over the WHOLE array, halos included (:369-374, :452-453): Kd_int = Kd_lay = KD, Kd_extra_T = Kd_extra_S = 0,
 * Kv_slow = KV, and Kv_shear = 0 unless use_Kd_shear.  Then on the computational domain: Kd_int and Kd_lay at every level;
 * Kd_extra_T, Kd_extra_S at K = 2..nz with DOUBLE_DIFFUSION; Kv_slow, N2_3d, Kd_bkgnd, Kv_bkgnd at every interface; KT_extra,
 * KS_extra at every interface with DOUBLE_DIFFUSION; Kd_BBL at K = 2..nz when the law of the wall runs.  A diagnostic plane is
 * otherwise left alone (the reference allocates its own with zeros: the caller's K = 1 and K = nz+1 planes of Kd_BBL and the
 * halos keep what the caller put there).
 * The call of Calculate_kappa_shear (:413-444) is the host's: mom6x_Calculate_kappa_shear writes the visc%Kd_shear and
 * visc%Kv_shear that are handed in here.  Not carried: CVMix shear (the host may hand in its visc%Kd_shear), ML_RADIATION, tidal mixing,
 * INTERNAL_TIDES, USE_CVMIX_DDIFF, the Bryan-Lewis and horizontally varying backgrounds, USER_CHANGE_DIFFUSIVITY,
 * add_drag_diffusivity, dRho_int_unfilt and find_rho_bottom (nothing on this path reads them), the Kd_Work diagnostics and VBF. */
int mom6x_set_diffusivity(mom6x_ctx *ctx, const double *u, const double *v, const double *h, const double *T, const double *S,
                          const double *p_surf, const double *tv_p_surf, const double *Kd_shear, const double *ustar_BBL,
                          const double *BBL_meanKE_loss, const double *ustar_tidal, const double *BBL_tidal_dis,
                          const double *Ray_u, const double *Ray_v, double dt, double *Kd_int, double *Kd_lay,
                          double *Kd_extra_T, double *Kd_extra_S, double *Kv_slow, double *Kv_shear, double *N2_3d,
                          double *Kd_BBL, double *Kd_bkgnd, double *Kv_bkgnd, double *KT_extra, double *KS_extra);

/* ------------------------------------------------------------------------- */
/* MOM_diabatic_aux: applyBoundaryFluxesInOut (surface heat, salt and water into h, tv%T, tv%S)                                  */
/* diabatic_aux_CS (src/parameterizations/vertical/MOM_diabatic_aux.F90:43-98; diabatic_aux_init :1349), the members of tv, US
 * and optics_type (MOM_opacity.F90:25-61) that applyBoundaryFluxesInOut (:682-1346) and its callees extractFluxes1d
 * (src/core/MOM_forcing_type.F90:447-948) and absorbRemainingSW (MOM_opacity.F90:600-867) read on a Boussinesq grid.  Values
 * are in the reference's scaled units; GV%g_Earth, Rho0, Angstrom_H, H_subroundoff, H_to_Z, H_to_RZ and RZ_to_H are the
 * context's (mom6x_vgrid).  Logicals are ints.  The members marked "must be 0" are refused with MOM6X_EUNSUPPORTED.           */
typedef struct mom6x_diabatic_aux_params {
  double C_p;                   /* tv%C_p [Q C-1]: I_Cp, I_Cp_Hconvert (MOM_forcing_type.F90:554-555) and the heat-content diagnostics */
  double g_Earth_Z_T2;          /* GV%g_Earth_Z_T2 [Z T-2]: g_Hconv2 (:810, MOM_opacity.F90:713-717), GoRho (:821), RivermixConst (:1045) */
  double RL2_T2_to_Pa;          /* US%RL2_T2_to_Pa (1): the pressure handed to the equation of state                                 */
  double ppt_to_S;              /* US%ppt_to_S (1): net_salt (MOM_forcing_type.F90:813)                                              */
  double rivermix_depth;        /* RIVERMIX_DEPTH (0, :1423) [Z]: read with DO_RIVERMIX                                              */
  double dSalt_frac_max;        /* the largest fraction of a layer's salt that a step may take out (SALT_EXTRACTION_LIMIT, 0.9999, :1400-1404; :1122) */
  double PenSW_flux_absorb;     /* PEN_SW_FLUX_ABSORB (2.5e-11, MOM_opacity.F90:1172) [C H T-1]: min_SW_heat = PenSW_flux_absorb*dt (MOM_opacity.F90:704)       */
  double PenSW_absorb_Invlen;   /* 1/(PEN_SW_ABSORB_MINTHICK + H_subroundoff) (MOM_opacity.F90:1184) [H-1]: I_Habs (:705)                             */
  int    optics_answer_date;    /* OPTICS_ANSWER_DATE (MOM_opacity.F90:1165): < 20190101 takes MOM_opacity.F90:714 and :744            */
  int    do_rivermix;           /* DO_RIVERMIX (F, :1418): the river TKE source :1033-1054 (with energetics)                         */
  int    use_river_heat_content;   /* USE_RIVER_HEAT_CONTENT (F, :1431): MOM_forcing_type.F90:718-735; needs heat_content_lrunoff, _glc */
  int    use_calving_heat_content; /* USE_CALVING_HEAT_CONTENT (F, :1435): MOM_forcing_type.F90:739-756; needs heat_content_frunoff, _glc */
  int    ignore_fluxes_over_land;  /* IGNORE_FLUXES_OVER_LAND (F, :1412): a flux over land (:1178) is not counted                    */
  int    do_brine_plume;        /* DO_BRINE_PLUME (F, :1444): must be 0 (needs the mixed layer depth of the boundary layer scheme)   */
  int    enthalpy_from_coupler; /* fluxes%heat_content_evap associated, do_enthalpy = .false. (MOM_forcing_type.F90:551): must be 0  */
  int    SpV_avg;               /* tv%SpV_avg allocated, non-Boussinesq (:903, :1046): must be 0                                     */
  int    nkml;                  /* GV%nkml, a bulk mixed layer (its own bulkmixedlayer applies the fluxes): must be 0                */
} mom6x_diabatic_aux_params;
/* The members of `forcing` (MOM_forcing_type.F90:80-256) that the routine touches, as DEVICE planes of the tile, NULL where the
 * reference's pointer is not associated.  Fluxes are in [R Z T-1] (water, salt) and [Q R Z T-1] (heat).
 * Required inputs (extractFluxes1d's fatal errors :567-587 and the sums :626-635): sw .. seaice_melt.
 * Nullable inputs: seaice_melt_heat (:694), heat_added (:711), salt_flux (:812).  heat_content_lrunoff, _lrunoff_glc, _frunoff,
 * _frunoff_glc are INPUTS with USE_RIVER_HEAT_CONTENT | USE_CALVING_HEAT_CONTENT (required then) and diagnostics written at
 * :902-920 without.
 * Nullable outputs, written on the computational domain: netMassIn, netMassOut (:976-982, 0 over land); heat_content_massin,
 * heat_content_massout (set at :823-849, accumulated at MOM_diabatic_aux.F90:1021-1027 and :1134-1140); heat_content_lprec,
 * _fprec, _vprec, _cond (:858-900).  TempxPmE (tv%TempxPmE) is accumulated into (:729-755, MOM_diabatic_aux.F90:1028, :1141):
 * the caller zeroes it.                                                                                                       */
typedef struct mom6x_surface_fluxes {
  const double *sw, *lw, *latent, *sens, *evap, *lprec, *fprec, *vprec, *lrunoff, *frunoff, *lrunoff_glc, *frunoff_glc, *seaice_melt;
  const double *seaice_melt_heat, *heat_added, *salt_flux;
  double *heat_content_lrunoff, *heat_content_lrunoff_glc, *heat_content_frunoff, *heat_content_frunoff_glc;
  double *netMassIn, *netMassOut, *heat_content_massin, *heat_content_massout;
  double *heat_content_lprec, *heat_content_fprec, *heat_content_vprec, *heat_content_cond;
  double *TempxPmE;
} mom6x_surface_fluxes;
/* diabatic_aux_init :1349 for the members above: checks them, keeps them with the equation of state and allocates the three
 * device counters of mom6x_diabatic_aux_status.  eos: tv%eqn_of_state, NULL without one (then neither the energetics nor
 * SkinBuoyFlux can be asked for).
 * MOM6X_EUNSUPPORTED, naming the setting: every "must be 0" member and a non-Boussinesq context.  MOM6X_EINVAL: an unknown
 * EQN_OF_STATE form, C_p <= 0.                                                                                                */
int mom6x_diabatic_aux_init(mom6x_ctx *ctx, const mom6x_diabatic_aux_params *p, const mom6x_eos_params *eos);
/* applyBoundaryFluxesInOut(CS, G, GV, US, dt, fluxes, optics, nsw, h, tv, aggregate_FW_forcing, evap_CFL_limit,
 * minimum_forcing_depth, cTKE, dSV_dT, dSV_dS, SkinBuoyFlux) :682 with extractFluxes1d (MOM_forcing_type.F90:447, do_enthalpy)
 * and absorbRemainingSW (MOM_opacity.F90:600; adjustAbsorptionProfile = .false., absorbAllSW = .true., no eps, ksort, htot,
 * Ttot) on the context's stream: at most two launches, no allocation, no host synchronisation, no halo exchange.  One lane per
 * column; the derivatives :886-895, steps A and B :1001-1175 and the downward loop of absorbRemainingSW run as ONE top-down
 * walk, which gives the reference's results bit for bit (the steps couple layers only through per-column scalars).
 * fluxes: NULL, or one whose sw is NULL, is .not.associated(fluxes%sw): with energetics only the derivatives and the fills are
 * made, otherwise only the fills (:814, :900).
 * nsw: the number of bands of penetrating shortwave, 0..4.  opacity_band: optics%opacity_band as nsw 3-D arrays, band-major
 * (band n at offset n * (nk * slab)), in [H-1]: the caller has applied opacity_scale = GV%H_to_Z (:904).  sw_pen_band:
 * optics%sw_pen_band as nsw planes, band-major.  Both are required with nsw > 0.
 * h, T, S (tv%T, tv%S): 3-D, rewritten in place on the computational domain.  tv_p_surf: tv%p_surf, a nullable plane.
 * Energetics (calculate_energetics, :806) are on when cTKE, dSV_dT and dSV_dS are all given; SkinBuoyFlux (a plane) turns
 * calculate_buoyancy on; both need an equation of state, the energetics one of LINEAR, WRIGHT, WRIGHT_FULL, WRIGHT_REDUCED,
 * ROQUET_SPV (the forms whose specific-volume derivatives are on the device; the others are MOM6X_EUNSUPPORTED by name).
 * Nullable diagnostics: createdH (CS%createdH, a plane [H T-1]: 0, or less what grounded over dt, :1202), penSW_diag (nk
 * levels), penSWflux_diag (nk + 1 levels, needs penSW_diag), nonpenSW_diag (a plane) (:1213-1272).
 * Written over the WHOLE array, halos included (:808-809): cTKE = 0 and SkinBuoyFlux = 0.  Everything else is written on the
 * computational domain only: dSV_dT, dSV_dS and every other array keep the caller's halo.  Land columns of the computational
 * domain do what the reference does with them: no step A or B, but the derivatives and the shortwave absorption run.
 * WHERE THE DEVICE DEPARTS FROM THE REFERENCE: it cannot stop.  A negative layer thickness after step B (:1163, FATAL in the
 * reference) leaves T and S of that layer as they were and is counted; a flux over land without IGNORE_FLUXES_OVER_LAND
 * (:1178, FATAL) is counted; a grounding (:1193, a WARNING) is counted and goes into createdH.  mom6x_diabatic_aux_status
 * reads the counts.  Results equal the reference's wherever the reference would have run to completion.
 * MOM6X_EINVAL: a required plane missing, nsw > 0 without the optics arrays, energetics or SkinBuoyFlux without an equation of
 * state, USE_RIVER_HEAT_CONTENT | USE_CALVING_HEAT_CONTENT without their heat-content planes, dt <= 0.  MOM6X_EUNSUPPORTED:
 * nsw > 4, energetics with UNESCO, ROQUET_RHO or JACKETT_06.
 * Not carried: DO_BRINE_PLUME, enthalpy from the coupler (fluxes%heat_content_evap), non-Boussinesq mode, the bulk mixed layer. */
int mom6x_applyBoundaryFluxesInOut(mom6x_ctx *ctx, double dt, const mom6x_surface_fluxes *fluxes, int nsw,
                                   const double *opacity_band, const double *sw_pen_band, double *h, double *T, double *S,
                                   const double *tv_p_surf, int aggregate_FW_forcing, double evap_CFL_limit,
                                   double minimum_forcing_depth, double *cTKE, double *dSV_dT, double *dSV_dS, double *SkinBuoyFlux,
                                   double *createdH, double *penSW_diag, double *penSWflux_diag, double *nonpenSW_diag);
/* Synchronises the context's stream and returns how many columns, since the last status call, grounded (:1193), were left with
 * a negative thickness (:1163) and had a flux over land without IGNORE_FLUXES_OVER_LAND (:1178).  Each pointer may be NULL.   */
int mom6x_diabatic_aux_status(mom6x_ctx *ctx, long *groundings, long *negative_h, long *land_fluxes);

/* ------------------------------------------------------------------------- */
/* The in-place modifiers of tv%T and tv%S around the column physics of diabatic (MOM_diabatic_driver.F90): make_frazil before
 * and after it (:371-391, :437-444), geothermal_in_place as the first call of diabatic_ALE (:1373), adjust_salt just before the
 * tridiagonal solve (:1633).  Each is one lane per column on the context's stream with no allocation, no host synchronisation and
 * no halo exchange, and gives the reference's results bit for bit.                                                            */
enum mom6x_tfreeze_form { MOM6X_TFREEZE_LINEAR = 1, MOM6X_TFREEZE_MILLERO = 2, MOM6X_TFREEZE_TEOS10 = 3,
                          MOM6X_TFREEZE_TEOSPOLY = 4 };   /* MOM_EOS.F90:184-187; TFREEZE_FORM = LINEAR, MILLERO_78, TEOS10, TEOS_POLY */
/* What make_frazil (src/parameterizations/vertical/MOM_diabatic_aux.F90:110-230) reads of diabatic_aux_CS, tv and of
 * tv%eqn_of_state for calculate_TFreeze (src/equation_of_state/MOM_EOS.F90:664-744).  GV%H_to_RZ, g_Earth, Angstrom_H and
 * H_subroundoff are the context's.  Logicals are ints.                                                                        */
typedef struct mom6x_frazil_params {
  double C_p;                       /* tv%C_p [Q C-1]: hc = (C_p*H_to_RZ)*h (:179, :202)                                       */
  double RL2_T2_to_Pa;              /* EOS%RL2_T2_to_Pa (1) } with both 1 the freezing point is taken from S and the pressure  */
  double S_to_ppt;                  /* EOS%S_to_ppt (1)     } as they are (MOM_EOS.F90:699), otherwise from their products (:715-716) */
  double degC_to_C;                 /* EOS%degC_to_C (1): applied to the freezing point when it is not 1 (:740)                */
  double TFr_S0_P0;                 /* TFREEZE_S0_P0 (0.0) [degC]       }                                                     */
  double dTFr_dS;                   /* DTFREEZE_DS (-0.054) [degC ppt-1] } TFREEZE_FORM = LINEAR (MOM_TFreeze.F90:82)         */
  double dTFr_dp;                   /* DTFREEZE_DP (0.0) [degC Pa-1]    }                                                     */
  int    form_of_TFreeze;           /* enum mom6x_tfreeze_form; TEOS10 needs the GSW library: MOM6X_EUNSUPPORTED               */
  int    reclaim_frazil;            /* RECLAIM_FRAZIL (T): the arm on layer 1 (:167-189)                                       */
  int    pressure_dependent_frazil; /* PRESSURE_DEPENDENT_FRAZIL (F): the mid-layer pressures (:158-165) instead of 0          */
  int    use_conT_absS;             /* EOS%use_conT_absS (gsw_sp_from_sr, gsw_ct_from_pt, MOM_EOS.F90:687-694, :733): must be 0 */
} mom6x_frazil_params;
/* Keeps the members above; with pressure_dependent_frazil it allocates the routine's `pressure` work array (nk levels), without
 * it nothing.  MOM6X_EUNSUPPORTED, naming the setting: TFREEZE_FORM = TEOS10, use_conT_absS.  MOM6X_EINVAL: an unknown
 * form_of_TFreeze, C_p <= 0.                                                                                                  */
int mom6x_make_frazil_init(mom6x_ctx *ctx, const mom6x_frazil_params *p);
/* make_frazil(h, tv, G, GV, US, CS, p_surf, halo) :110-230.  h, T (tv%T), S (tv%S): 3-D; frazil (tv%frazil): a plane; p_surf:
 * a nullable plane, read with pressure_dependent_frazil only; halo: 0 .. the context's halo, the width by which the
 * computational domain is widened (anything else is MOM6X_EINVAL).  One launch, one lane per column of that range, in the
 * reference's order: the mid-layer pressures top-down into the work array (:160-163, with the switch only); the reclaim arm on
 * layer 1 (:167-189), which has no land mask in the reference and none here; the walk from layer nk up to 1 in wet columns
 * (:191-220), where a layer with T >= 0 and no heat pending reads neither S nor h nor a pressure (:194-195); and
 * frazil = frazil + fraz_col in every column of the range, land included (:221-223), which turns a stored -0 into +0.
 * Reads h, S, p_surf; rewrites T and frazil inside the range only.  tv%frazil_was_reset (:226) is the host's flag.            */
int mom6x_make_frazil(mom6x_ctx *ctx, const double *h, double *T, const double *S, double *frazil, const double *p_surf, int halo);
/* adjust_salt(h, tv, G, GV, CS) :339-390 with S_min = tv%min_salinity: needs no init call.  h, S (tv%S): 3-D; salt_deficit
 * (tv%salt_deficit): a plane.  The computational domain only; wet columns are walked from layer nk up to 1, where a layer with
 * S >= S_min and no deficit pending reads no h (:366-367); the thin-layer test is h <= 10*Angstrom_H (:369, no H_subroundoff)
 * and the absorbing arm tests <= 0 (:375); salt_deficit = salt_deficit + salt_add_col in every column of the domain (:384-386).
 * Reads h; rewrites S and salt_deficit on the computational domain only.                                                      */
int mom6x_adjust_salt(mom6x_ctx *ctx, const double *h, double *S, double *salt_deficit, double min_salinity);
/* What geothermal_in_place (src/parameterizations/vertical/MOM_geothermal.F90:364-535) reads of geothermal_CS, tv, GV and US.
 * GV%H_to_RZ, g_Earth, Rho0, Angstrom_H and H_subroundoff are the context's.                                                  */
typedef struct mom6x_geothermal_params {
  double C_p;                /* tv%C_p [Q C-1]: Irho_cp (:416), I_Cp (:421), the heat tendency (:523)                          */
  double geothermal_thick;   /* GEOTHERMAL_THICKNESS (0.1 m, :579) [H]                                                         */
  double g_Earth_Z_T2;       /* GV%g_Earth_Z_T2 [Z T-2]: BFlx_geothermal (:458)                                                */
  double RL2_T2_to_Pa;       /* US%RL2_T2_to_Pa (1): the bottom pressure handed to the equation of state                       */
} mom6x_geothermal_params;
/* geothermal_init :538 for the in-place mode.  geo_heat_host_plane: CS%geo_heat [Q R Z T-1], a HOST plane of the tile as the
 * caller has scaled and masked it (:600-606), copied to the device once.  eos: tv%eqn_of_state, NULL without one (then
 * BFlx_geothermal cannot be asked for).  MOM6X_EUNSUPPORTED: a non-Boussinesq context (:444-451).  MOM6X_EINVAL: a null
 * argument, an unknown EQN_OF_STATE form, C_p <= 0.  Not carried: geothermal_entraining (:41-359, the layered mode) has no
 * entry point.                                                                                                                */
int mom6x_geothermal_init(mom6x_ctx *ctx, const mom6x_geothermal_params *p, const double *geo_heat_host_plane,
                          const mom6x_eos_params *eos);
/* geothermal_in_place(h, tv, dt, G, GV, US, CS, BFlx_geothermal, halo) :364-535.  h, T (tv%T), S (tv%S): 3-D; internal_heat
 * (tv%internal_heat) and BFlx_geothermal: nullable planes; dTdt_diag (internal_heat_temp_tendency) and heat_tend_diag
 * (internal_heat_heat_tendency, the product at :523): nullable, nk levels, either without the other; halo as in make_frazil.
 * One lane per column of the widened domain.  With BFlx_geothermal the lane sums H_to_pres*h top-down (:441-443) and takes
 * the bottom layer's density derivatives, from any EQN_OF_STATE form, at RL2_T2_to_Pa times that pressure (:455-458; as the
 * reference's EOS domain has it, they are 0 in the columns of the i halo); this needs an equation of state and S.  Without it
 * the column of h is not summed.  The walk from the bottom (:482-507) reads and writes only the layers that take heat.
 * Written over the WHOLE array, halos included: BFlx_geothermal = 0 (:434), dTdt_diag = 0 and heat_tend_diag = 0 (:436);
 * inside the range heat_tend_diag is the product :523 of every layer.  T and internal_heat are rewritten inside the range only.
 * WHERE THE DEVICE DEPARTS FROM THE REFERENCE: the reference skips a whole j-row of its tile when no column of it is heated
 * (:476), and with it that row's internal_heat = internal_heat + H_to_RZ*(...) (:509-512).  For an unheated column the addend
 * is +0, so the skip shows only in an internal_heat of -0, and it depends on the tile layout in the reference itself.  The
 * device makes the addition in every column of the range.
 * MOM6X_EINVAL: dt <= 0, a halo outside 0 .. the context's, null h or T, BFlx_geothermal without an equation of state or S.  */
int mom6x_geothermal_in_place(mom6x_ctx *ctx, const double *h, double *T, const double *S, double dt, double *internal_heat,
                              double *BFlx_geothermal, double *dTdt_diag, double *heat_tend_diag, int halo);

/* ------------------------------------------------------------------------- */
/* The shortwave optics: set_pen_shortwave (src/parameterizations/vertical/MOM_diabatic_aux.F90:621-677) with set_opacity
 * (src/parameterizations/vertical/MOM_opacity.F90:118-240), called in diabatic_ALE before applyBoundaryFluxesInOut
 * (MOM_diabatic_driver.F90).  They produce the optics%opacity_band and optics%sw_pen_band that
 * mom6x_applyBoundaryFluxesInOut reads, from the shortwave planes of `forcing` and, at most, one field of chlorophyll.           */
enum mom6x_opacity_scheme { MOM6X_OPACITY_MANIZZA_05 = 1, MOM6X_OPACITY_MOREL_88 = 2, MOM6X_OPACITY_SINGLE_EXP = 3,
                            MOM6X_OPACITY_DOUBLE_EXP = 4, MOM6X_OPACITY_OHLMANN_03 = 5 };   /* MOM_opacity.F90:105-106 */
/* What opacity_init (MOM_opacity.F90:1041-1315) reads into opacity_CS and optics_type for set_opacity.  GV%Angstrom_Z is taken
 * as H_to_Z*Angstrom_H of the context (the same length in a Boussinesq model), GV%dZ_subroundoff is the context's.              */
typedef struct mom6x_opacity_params {
  double pen_sw_scale;        /* PEN_SW_SCALE (0.0) [Z]: :157, :166, :182                                                       */
  double pen_sw_scale_2nd;    /* PEN_SW_SCALE_2ND (0.0) [Z]: DOUBLE_EXP, :163                                                   */
  double sw_1st_exp_ratio;    /* SW_1ST_EXP_RATIO (0.0): DOUBLE_EXP, :174-175                                                   */
  double pen_sw_frac;         /* PEN_SW_FRAC (0.0): SINGLE_EXP, :190                                                            */
  double blue_frac;           /* BLUE_FRAC_SW (0.5): MANIZZA_05, :369-372                                                       */
  double opacity_land_value;  /* OPACITY_LAND_VALUE (10 m-1) [Z-1]: :439, :454, :466                                            */
  double manizza_coef[6];     /* OPACITY_VALUES_MANIZZA (0.0232, 0.074, 0.225, 0.037, 2.86, 0.0) [Z-1]: coef_1, coef_2 per band */
  double manizza_power[3];    /* CHOROPHYLL_POWER_MANIZZA (0.674, 0.629, 0.0)                                                   */
  double morel_coef[6];       /* OPACITY_VALUES_MOREL (7.925, -6.644, 3.662, -1.815, -0.218, 0.502) [Z]: :490-492               */
  double morel_pen_coef[6];   /* SW_PEN_FRAC_COEFS_MOREL (0.321, 0.008, 0.132, 0.038, -0.017, -0.007): :510-512                 */
  double Z_to_m;              /* US%Z_to_m (1): the Ohlmann opacities, :469                                                     */
  double m_to_Z;              /* US%m_to_Z (1): the length of the opacity diagnostic, :228                                      */
  int    opacity_scheme;      /* enum mom6x_opacity_scheme: OPACITY_SCHEME with VAR_PEN_SW, EXP_OPACITY_SCHEME without          */
  int    nbands;              /* PEN_SW_NBANDS (1): 0 .. 4                                                                      */
} mom6x_opacity_params;
/* What opacity_init does with the parameters, on the host: the band-count rules (:1151-1160: DOUBLE_EXP and OHLMANN_03 need 2
 * bands, SINGLE_EXP 1); the coefficients of MANIZZA_05 per band, band 3's for the bands from 4 on (:1246-1254); chl_dep_bands
 * and the fold of a chlorophyll coefficient whose power is 0 into the constant (:1256-1269); with OHLMANN_03 the table of 401
 * entries (init_ohlmann_table :1321-1430), uploaded once.  It allocates one device counter.  nbands = 0 is accepted where the
 * rules allow it, and mom6x_set_pen_shortwave then does nothing.  MOM6X_EINVAL: a null argument, an unknown scheme, a negative
 * nbands, a broken band-count rule.  MOM6X_EUNSUPPORTED, naming the setting: more than 4 bands (the limit of
 * mom6x_applyBoundaryFluxesInOut), a non-Boussinesq context (the SpV_avg scaling of extract_optics_slice :555).  Not carried:
 * sumSWoverBands, the band wavelengths, and the once-only warning of :310-318 (the host knows which pointers it passes).       */
int mom6x_opacity_init(mom6x_ctx *ctx, const mom6x_opacity_params *p);
/* set_pen_shortwave(optics, fluxes, G, GV, US, CS, opacity, tracer_flow_CSp) MOM_diabatic_aux.F90:621-677 with set_opacity
 * MOM_opacity.F90:118-240, opacity_from_chl :245-477, opacity_morel and SW_pen_frac_morel :481-513, lookup_ohlmann_swpen and
 * lookup_ohlmann_opacity :1433-1485, and the product of extract_optics_slice :559.  All arrays are device pointers.
 * sw (fluxes%sw), sw_vis_dir, sw_vis_dif, sw_nir_dir, sw_nir_dif: planes, NULL where the reference's pointer is not associated.
 * chl_2d: the plane time_interp_external gave the host (CHL_FROM_FILE); chl_3d: the model's own chlorophyll, nk levels
 * (get_chl_from_model); both NULL: the exponential arm :152-193.  opacity_band: nbands 3-D arrays, band n at offset
 * n*nk*slab; sw_pen_band: nbands planes, band n at offset n*slab: the layout mom6x_applyBoundaryFluxesInOut reads, so the two
 * pointers pass straight on.  The value stored in opacity_band is opacity_scale*opacity, the single product of :559: the caller
 * passes GV%H_to_Z, and with 1.0 the array is optics%opacity_band itself.  Nullable diagnostics: SW_pen (:197-206) and
 * SW_vis_pen (:207-226, bands 1 and 2 only under MANIZZA_05), planes; opac_diag, nbands 3-D arrays laid out as opacity_band, of
 * tanh(op_diag_len*op)/op_diag_len from the unscaled opacity (:227-237).
 * One launch on the context's stream, one lane per column, no allocation, no host synchronisation, no halo exchange.  Every
 * output is written on the computational domain only; the caller's halo is kept.  With chl_2d or without chlorophyll the
 * opacity of a column is evaluated once and stored at every layer (the reference evaluates the same expression nk times).
 * WHERE THE DEVICE DEPARTS FROM THE REFERENCE: a negative chlorophyll at a wet point (mask2dT > 0) is FATAL in the reference
 * (MOM_diabatic_aux.F90:649, MOM_opacity.F90:328, :338).  The device cannot stop: it counts such points
 * (mom6x_opacity_status) and stores there what the formulas give; everywhere else the results are the reference's.
 * MOM6X_EINVAL: a call before init; both chl_2d and chl_3d; MANIZZA_05, MOREL_88 or OHLMANN_03 without chlorophyll; SINGLE_EXP
 * or DOUBLE_EXP with it; OHLMANN_03 with neither sw nor all four band planes, or with the visible pair but not the near-infrared
 * one (:410 and the dereference at :406); nbands > 0 with a null opacity_band or sw_pen_band.                                  */
int mom6x_set_pen_shortwave(mom6x_ctx *ctx, const double *sw, const double *sw_vis_dir, const double *sw_vis_dif,
                            const double *sw_nir_dir, const double *sw_nir_dif, const double *chl_2d, const double *chl_3d,
                            double opacity_scale, double *opacity_band, double *sw_pen_band, double *SW_pen, double *SW_vis_pen,
                            double *opac_diag);
/* Synchronises the stream.  *negative_chl: the wet points (mask2dT > 0) with negative chlorophyll since the last status call,
 * one per (i,j) for chl_2d and one per cell for chl_3d.  The pointer may be NULL.                                              */
int mom6x_opacity_status(mom6x_ctx *ctx, long *negative_chl);

/* ------------------------------------------------------------------------- */
/* MOM_energetic_PBL: energetic_PBL (the ePBL surface boundary layer scheme), between applyBoundaryFluxesInOut and the tridiagonal
 * solve of diabatic_ALE (src/parameterizations/vertical/MOM_diabatic_driver.F90:1559-1581).                                     */
enum mom6x_epbl_mstar_scheme { MOM6X_EPBL_MSTAR_CONSTANT = 0, MOM6X_EPBL_MSTAR_OM4 = 2, MOM6X_EPBL_MSTAR_REICHL_H18 = 3 };   /* MOM_energetic_PBL.F90:279-282 */
enum mom6x_epbl_wT_scheme { MOM6X_EPBL_WT_CUBE_ROOT_TKE = 0, MOM6X_EPBL_WT_REICHL_H18 = 1 };                                 /* :288-290 */
/* What energetic_PBL_init (src/parameterizations/vertical/MOM_energetic_PBL.F90:3729-4429) leaves in energetic_PBL_CS (:38-276)
 * for the surface boundary layer, scaled as CS holds it, with the members of GV and US that energetic_PBL and ePBL_column read.
 * GV%Rho0, H_to_Z, Z_to_H, H_to_RZ, H_subroundoff and dZ_subroundoff are the context's (mom6x_vgrid).  Logicals are ints.  The
 * members marked "must be 0" are refused with MOM6X_EUNSUPPORTED.                                                              */
typedef struct mom6x_energetic_PBL_params {
  double omega;              /* OMEGA [T-1]                                                                                      */
  double omega_frac;         /* ML_OMEGA_FRAC: absf :662-669                                                                     */
  double Ekman_scale_coef;   /* EKMAN_SCALE_COEF                                                                                 */
  double vonKar;             /* VON_KARMAN_CONST                                                                                 */
  double MKE_to_TKE_effic;   /* MKE_TO_TKE_EFFIC * US%L_to_Z**2: > 0 needs u and v                                               */
  double TKE_decay;          /* TKE_DECAY (2.5)                                                                                  */
  double fixed_mstar;        /* MSTAR, EPBL_MSTAR_SCHEME = CONSTANT                                                              */
  double mstar_cap;          /* MSTAR_CAP (-1: none), OM4                                                                        */
  double mstar_coef, C_Ek;   /* MSTAR2_COEF1, MSTAR2_COEF2, OM4                                                                  */
  double RH18_mstar_cn1, RH18_mstar_cn2, RH18_mstar_cn3, RH18_mstar_cs1, RH18_mstar_cs2;   /* REICHL_H18                        */
  double nstar;              /* NSTAR                                                                                            */
  double mstar_convect_coef; /* MSTAR_CONV_ADJ                                                                                   */
  double transLay_scale;     /* EPBL_TRANSITION_SCALE (outside (0, 1) with Use_MLD_iteration the reference stops, :3969; taken here) */
  double MLD_tol;            /* EPBL_MLD_TOLERANCE [Z]                                                                           */
  double min_mix_len;        /* EPBL_MIN_MIX_LEN [Z]                                                                             */
  double MixLenExponent;     /* MIX_LEN_EXPONENT                                                                                 */
  double wstar_ustar_coef;   /* WSTAR_USTAR_COEF                                                                                 */
  double vstar_scale_fac;    /* EPBL_VEL_SCALE_FACTOR                                                                            */
  double vstar_surf_fac;     /* VSTAR_SURF_FAC                                                                                   */
  double ustar_min;          /* 2e-4*omega*(Angstrom_Z + dZ_subroundoff) (:4328) [Z T-1]                                         */
  double g_Earth_Z_T2;       /* GV%g_Earth_Z_T2 [Z T-2]: dPres :1194                                                             */
  double m_to_Z, T_to_s;     /* US%m_to_Z, US%T_to_s (1): dMLD_min, dMLD_max :1221 and the answers before 20240101               */
  double ePBL_BBL_effic;     /* EPBL_BBL_EFFIC: must be 0 (ePBL_BBL_column is not on the device)                                 */
  double ePBL_tidal_effic;   /* EPBL_BBL_TIDAL_EFFIC: must be 0                                                                  */
  int    answer_date;        /* EPBL_ANSWER_DATE: < 20190101, < 20240101 (A**(1./3.)) or later (cuberoot)                        */
  int    orig_PE_calc;       /* EPBL_ORIGINAL_PE_CALC (T): find_PE_chg_orig, else find_PE_chg                                    */
  int    mstar_scheme;       /* enum mom6x_epbl_mstar_scheme                                                                     */
  int    Use_MLD_iteration;  /* USE_MLD_ITERATION (T)                                                                            */
  int    MLD_iteration_guess;/* MLD_ITERATION_GUESS (F): the first guess is ML_depth of the call before                          */
  int    MLD_bisection;      /* EPBL_MLD_BISECTION (F)                                                                           */
  int    MLD_iter_bug;       /* EPBL_MLD_ITER_BUG                                                                                */
  int    max_MLD_its;        /* EPBL_MLD_MAX_ITS (20); 1 without USE_MLD_ITERATION (:3999)                                       */
  int    wT_scheme;          /* enum mom6x_epbl_wT_scheme                                                                        */
  int    TKE_diagnostics;    /* CS%TKE_diagnostics: the seven diag_TKE_* planes are formed                                       */
  int    has_eos;            /* associated(tv%eqn_of_state) (:512): what dSV_dT and dSV_dS came from                             */
  int    ePBL_BBL_use_mstar; /* EPBL_BBL_USE_MSTAR: must be 0                                                                    */
  int    use_LT;             /* USE_LA_LI2016 | EPBL_LT, Langmuir turbulence (needs MOM_wave_interface): must be 0               */
  int    eqdisc, eqdisc_v0, eqdisc_v0h;   /* EPBL_EQD_DIFFUSIVITY_SHAPE, _VELOCITY, _VELOCITY_H: must be 0                      */
  int    direct_calc;        /* DIRECT_EPBL_MIXING_CALC: must be 0                                                               */
  int    options_diff;       /* EPBL_OPTIONS_DIFF: must be 0                                                                     */
  int    pert_epbl;          /* stoch_CS%pert_epbl, stochastic perturbations: must be 0                                          */
  int    ustar_shelf;        /* fluxes%ustar_shelf and frac_shelf_h associated (:656): must be 0                                 */
  int    tau_mag;            /* fluxes%tau_mag in place of fluxes%ustar (:635-643): must be 0                                    */
  int    SpV_avg;            /* tv%SpV_avg allocated, non-Boussinesq: must be 0                                                  */
} mom6x_energetic_PBL_params;
/* energetic_PBL_init :3729: checks the members, keeps them and allocates the work array of hb_hs (nk + 1 levels).
 * A refused or invalid call leaves no module behind, also where an earlier call had succeeded.
 * MOM6X_EUNSUPPORTED, naming the setting: every "must be 0" member, a non-Boussinesq context, and TKE_diagnostics together with
 * MKE_to_TKE_effic > 0 (that instantiation of the kernel does not fit a lane's registers).  MOM6X_EINVAL: an unknown scheme,
 * max_MLD_its < 1.                                                                                                     */
int mom6x_energetic_PBL_init(mom6x_ctx *ctx, const mom6x_energetic_PBL_params *p);
/* energetic_PBL(h_3d, u_3d, v_3d, tv, fluxes, visc, dt, Kd_int, G, GV, US, CS, stoch_CS, dSV_dT, dSV_dS, TKE_forced, buoy_flux)
 * :326-884 with ePBL_column :890-1950, find_mstar :3519-3613, find_PE_chg_orig :3365-3516, find_PE_chg :3072-3213, cuberoot
 * (src/framework/MOM_intrinsic_functions.F90:48-114) and the Boussinesq thickness_to_dz, in one launch on the context's stream (a second,
 * small one with diag_TKE_* planes): no allocation, no host synchronisation, no halo exchange.  One lane per column of the computational domain; the lanes of a
 * wavefront leave the mixed-layer-depth iteration together, after the slowest of them.
 * h, T, S (tv%T, tv%S), dSV_dT, dSV_dS, TKE_forced: 3-D, only read.  ustar (fluxes%ustar), buoy_flux: planes, only read.
 * u, v: the C-GRID velocities; the kernel forms u_h, v_h with the no-mixing arm of find_uv_at_h (MOM_diabatic_aux.F90:546-571,
 * :606-611).  Read only with MKE_to_TKE_effic > 0, NULL otherwise.
 * Kd_int: nk + 1 levels, written on the computational domain, 0 in land columns (:819-823).
 * ML_depth: CS%ML_depth [Z], the caller's resident plane: read with MLD_iteration_guess (:673), written on the computational
 * domain always (0 over land).
 * Nullable outputs, on the computational domain (0 over land): Velocity_Scale, Mixing_Length (nk + 1 levels); the seven
 * diag_TKE_* planes (with TKE_diagnostics only; diag_TKE_MKE is then always 0, since TKE_diagnostics excludes MKE conversion); mstar_sfc; ustar_diag (diag_ustar :645: fluxes%ustar before ustar_min); OBL_its
 * (eCD%OBL_its as a real, the per-column value behind CS%sum_its).
 * MOM6X_EINVAL: a required array missing, MKE_to_TKE_effic > 0 without u and v, no equation of state (has_eos = 0), a diag_TKE_*
 * plane without TKE_diagnostics, dt <= 0.
 * Not carried: bottom-boundary-layer ePBL (ePBL_BBL_column), Langmuir turbulence, the equation-discovery switches,
 * DIRECT_EPBL_MIXING_CALC, EPBL_OPTIONS_DIFF, stochastic perturbations, ustar_shelf, tau_mag, non-Boussinesq mode.             */
int mom6x_energetic_PBL(mom6x_ctx *ctx, const double *h, const double *u, const double *v, const double *T, const double *S,
                        const double *dSV_dT, const double *dSV_dS, const double *TKE_forced, const double *ustar,
                        const double *buoy_flux, double dt, double *Kd_int, double *ML_depth, double *Velocity_Scale,
                        double *Mixing_Length, double *diag_TKE_wind, double *diag_TKE_MKE, double *diag_TKE_conv,
                        double *diag_TKE_forcing, double *diag_TKE_mixing, double *diag_TKE_mech_decay, double *diag_TKE_conv_decay,
                        double *mstar_sfc, double *ustar_diag, double *OBL_its);
/* energetic_PBL_get_MLD(CS, MLD, G, US, m_to_MLD_units) :3707: MLD = scale * ML_depth on the computational domain.            */
int mom6x_energetic_PBL_get_MLD(mom6x_ctx *ctx, const double *ML_depth, double *MLD, double scale);
/* The driver's loop MOM_diabatic_driver.F90:1570-1581 over levels 2..nk of the computational domain: with ePBL_is_additive
 * Kv_shear += ePBL_Prandtl*Kd_ePBL and Kd_add = Kd_ePBL, otherwise Kv_shear = max(Kv_shear, ePBL_Prandtl*Kd_ePBL) and Kd_add =
 * max(Kd_ePBL - Kd_shear, 0.) (Kd_shear is read in this arm only); Kd_heat += Kd_add, Kd_salt += Kd_add.  MLD and h_ML, both
 * or neither: visc%h_ML = GV%Z_to_H * MLD (:1565, the Boussinesq convert_MLD_to_ML_thickness).                                  */
int mom6x_ePBL_augment_Kd(mom6x_ctx *ctx, const double *Kd_ePBL, const double *Kd_shear, double *Kv_shear, double *Kd_heat,
                          double *Kd_salt, int ePBL_is_additive, double ePBL_Prandtl, const double *MLD, double *h_ML);

/* ------------------------------------------------------------------------- */
/* MOM_kappa_shear: Calculate_kappa_shear, the Jackson et al. (2008) shear-driven mixing (USE_JACKSON_PARAM), called by
 * set_diffusivity (src/parameterizations/vertical/MOM_set_diffusivity.F90:413-444) after the driver's find_uv_at_h
 * (MOM_diabatic_driver.F90:1391-1398).  It produces the visc%Kd_shear and visc%Kv_shear that mom6x_set_diffusivity reads.        */
/* What kappa_shear_init (src/parameterizations/vertical/MOM_kappa_shear.F90:2070-2330) leaves in Kappa_shear_CS (:34-126), scaled
 * as CS holds it, with the members of US, GV and the EOS type that Calculate_kappa_shear (:133-411), kappa_shear_column
 * (:864-1372), calculate_projected_state (:1377-1504) and find_kappa_tke (:1507-2067) read and the context does not hold.
 * GV%g_Earth, Rho0, H_to_Z, H_to_RZ and H_subroundoff are the context's (mom6x_vgrid).  Logicals are ints.  (struct 35)           */
typedef struct mom6x_kappa_shear_params {
  double RiNo_crit;          /* RINO_CRIT (0.25)                                                                                 */
  double Shearmix_rate;      /* SHEARMIX_RATE (0.089)                                                                            */
  double FRi_curvature;      /* FRI_CURVATURE (-0.97)                                                                            */
  double C_N;                /* TKE_N_DECAY_CONST (0.24)                                                                         */
  double C_S;                /* TKE_SHEAR_DECAY_CONST (0.14)                                                                     */
  double lambda;             /* KAPPA_BUOY_SCALE_COEF (0.82)                                                                     */
  double lambda2_N_S;        /* KAPPA_N_OVER_S_SCALE_COEF2 (0): kept in CS, read by no routine                                   */
  double lz_rescale;         /* LZ_RESCALE (1): :1010                                                                            */
  double TKE_bg;             /* TKE_BACKGROUND (0) [Z2 T-2]                                                                      */
  double kappa_0;            /* KD_KAPPA_SHEAR_0 (max(KD, 1e-7 m2 s-1)) [H Z T-1]                                                */
  double kappa_seed;         /* KD_SEED_KAPPA_SHEAR (1 m2 s-1) [H Z T-1]: the first guess :323                                   */
  double kappa_trunc;        /* KD_TRUNC_KAPPA_SHEAR (0.01*kappa_0) [H Z T-1]                                                    */
  double kappa_tol_err;      /* KAPPA_SHEAR_TOL_ERR (0.1)                                                                        */
  double Prandtl_turb;       /* PRANDTL_TURB (1): kv_io :391                                                                     */
  double vel_underflow;      /* VEL_UNDERFLOW (0) [L T-1]                                                                        */
  double kappa_src_max_chg;  /* KAPPA_SHEAR_MAX_KAP_SRC_CHG (10): must be greater than 1                                         */
  double m_to_Z, T_to_s;     /* US%m_to_Z, US%T_to_s (1): TKE_min :1630, the KAPPA_SHEAR_ITER_BUG arm :1860                      */
  double L_to_Z;             /* US%L_to_Z (1): the squared shear :1484-1489                                                      */
  double Z_to_m_m_to_H;      /* US%Z_to_m*GV%m_to_H (1): dz_massless :219                                                        */
  double g_Earth_Z_T2;       /* GV%g_Earth_Z_T2 [Z T-2]: g_R0 :1007                                                              */
  double RL2_T2_to_Pa;       /* EOS%RL2_T2_to_Pa (1): the pressure handed to the equation of state, MOM_EOS.F90:813               */
  double kg_m3_to_R;         /* EOS%kg_m3_to_R (1): the density derivatives, MOM_EOS.F90:820                                     */
  int    max_RiNo_it;        /* MAX_RINO_IT (50): the iterations of find_kappa_tke, at least 1                                   */
  int    max_KS_it;          /* MAX_KAPPA_SHEAR_IT (13): the outer iterations of a column, at least 1                            */
  int    nkml;               /* CS%nkml: GV%nkml with a bulk mixed layer and KAPPA_SHEAR_MERGE_ML, else 1 (:2283-2289)           */
  int    eliminate_massless; /* KAPPA_SHEAR_ELIM_MASSLESS (T)                                                                    */
  int    dKdQ_iteration_bug; /* KAPPA_SHEAR_ITER_BUG (F)                                                                         */
  int    all_layer_TKE_bug;  /* KAPPA_SHEAR_ALL_LAYER_TKE_BUG (F)                                                                */
  int    restrictive_tolerance_check;   /* USE_RESTRICTIVE_TOLERANCE_CHECK (F)                                                   */
  int    KS_at_vertex;       /* VERTEX_SHEAR: must be 0 (Calc_kappa_shear_vertex is not on the device)                           */
  int    work_columns;       /* the columns in flight, each with a slot of the workspace; 0: the library's default (the columns
                              * of the tile, at most 65536).  Rounded up to whole wavefronts of 64.  A small value makes a small
                              * grid reuse its slots (for tests)                                                                 */
} mom6x_kappa_shear_params;
/* kappa_shear_init :2070: checks the members, keeps them with the equation of state (tv%eqn_of_state; NULL: none) and a device
 * copy of GV%Rlay (a HOST array of nk values; NULL: none), and allocates the workspace: 51 arrays of nk + 1 levels for each of
 * work_columns slots, on the device.  A refused or invalid call leaves no module behind, also where an earlier call had succeeded.
 * MOM6X_EUNSUPPORTED, naming the setting: KS_at_vertex (VERTEX_SHEAR), a non-Boussinesq context.  MOM6X_EINVAL: max_KS_it < 1,
 * max_RiNo_it < 1, RiNo_crit <= 0, kappa_src_max_chg <= 1, work_columns < 0, nkml < 1, lambda = 0, an unknown EQN_OF_STATE form.
 * The reference's kappa_shear_init has no FATAL of its own: the compiled init takes every one of these values as given
 * (KAPPA_BUOY_SCALE_COEF = 0 then divides by zero at :1632); GV%nkml = 0 is its spelling of nkml = 1 (:2283-2289) and
 * work_columns is not a setting of its.  The refusals above are the device's alone; only an unknown EQN_OF_STATE is FATAL there
 * too (MOM_EOS.F90:1591).  tests/test_ref_parity_cpu.py holds this list to the compiled init.                                   */
int mom6x_kappa_shear_init(mom6x_ctx *ctx, const mom6x_kappa_shear_params *p, const mom6x_eos_params *eos, const double *Rlay);
/* The bytes of the workspace that mom6x_kappa_shear_init allocated (0 before it). */
long long mom6x_kappa_shear_work_bytes(mom6x_ctx *ctx);
/* Calculate_kappa_shear(u_in, v_in, h, tv, p_surf, kappa_io, tke_io, kv_io, dt, G, GV, US, CS) :133-411 with kappa_shear_column
 * :864-1372, calculate_projected_state :1377-1504, find_kappa_tke :1507-2067 and the Boussinesq thickness_to_dz, in one launch on
 * the context's stream: no allocation, no host synchronisation, no halo exchange.  All arrays are device pointers.
 * u, v: the C-GRID velocities, only read.  The kernel forms u_h, v_h as the driver's find_uv_at_h does
 * (MOM_diabatic_driver.F90:1391-1398; MOM_diabatic_aux.F90:546-611, without ea and eb): the plain average (:607-610), or with
 * zero_mix != 0 the arm of :595-605 with GV%H_subroundoff, which the driver takes when geothermal heating is on.
 * h, T, S (tv%T, tv%S): 3-D, only read; p_surf: a plane or NULL.  T and S are given together (and need the equation of state
 * given to init: calculate_density_derivs at interfaces 2..nzc with scale = -g_R0, every form of mom6x_eos_form) or both NULL (the
 * layered arm, GV%Rlay as the state :241, :1146-1147, needs the Rlay given to init).
 * kappa_io (visc%Kd_shear), tke_io (visc%TKE_turb), kv_io (visc%Kv_shear): nk + 1 levels, written on the computational domain
 * only, 0 in land columns (:382-391); halos are left alone.  kappa_io is NOT READ: although the reference declares it intent(inout)
 * ("the value from the previous timestep"), every column starts from kappa_seed (:323), and so does the device.
 * N2_init, S2_init, N2_mean, S2_mean: nullable diagnostics of nk + 1 levels (0 in land columns).  KS_its: a nullable plane, the
 * outer iterations (:1189) each column used, as a real (0 over land).
 * One lane per column; a lane walks its share of the columns and reuses its slot of the workspace.  The lanes of a wavefront
 * leave a column together, after the slowest of them; a wavefront of columns without an interface of Ri < Ri_crit (:1303) does
 * not wait for any other.
 * MOM6X_EINVAL: a call before init, null u, v, h, kappa_io, tke_io or kv_io, dt <= 0, T without S, T and S without an equation of
 * state at init, no T and S when init got no Rlay.
 * Not carried: Calc_kappa_shear_vertex (:415-860, VERTEX_SHEAR) with full_convection and the vertex averages, CVMix shear
 * (MOM_CVMix_shear), non-Boussinesq mode, the debug checksums (:397-402), VBF%Kd_KS.                                            */
int mom6x_Calculate_kappa_shear(mom6x_ctx *ctx, const double *u, const double *v, const double *h, const double *T, const double *S,
                                const double *p_surf, double dt, int zero_mix, double *kappa_io, double *tke_io, double *kv_io,
                                double *N2_init, double *S2_init, double *N2_mean, double *S2_mean, double *KS_its);

/* ------------------------------------------------------------------------- */
/* MOM_neutral_diffusion: epineutral tracer mixing (USE_NEUTRAL_DIFFUSION), continuous reconstruction (NDIFF_CONTINUOUS = True) */
/* What neutral_diffusion_init (src/tracer/MOM_neutral_diffusion.F90:134-345) leaves in neutral_diffusion_CS (:44-126), with
 * RECALC_NEUTRAL_SURF of tracer_hor_diff_CS and the members of the EOS type that calculate_density_derivs reads
 * (MOM_EOS.F90:809-827).  GV%g_Earth, H_to_RZ and H_subroundoff are the context's.  Logicals are ints.  The members marked "must
 * be" are refused with MOM6X_EUNSUPPORTED and the parameter's name.  (struct 36)                                                 */
typedef struct mom6x_neutral_diffusion_params {
  int    continuous_reconstruction;  /* NDIFF_CONTINUOUS (T, :181): must be 1 (the discontinuous reconstruction is not on the device) */
  double ref_pres;                   /* NDIFF_REF_PRES (-1, :187) [R L2 T-2]: negative: the local interface pressure (:493)           */
  int    interior_only;              /* NDIFF_INTERIOR_ONLY (F, :191): must be 0                                                       */
  int    tapering;                   /* NDIFF_TAPERING (F, :196): must be 0                                                            */
  int    KhTh_use_vert_struct;       /* KHTR_USE_EBT_STRUCT or KHTR_USE_SQG_STRUCT (F, :201-208): must be 0                            */
  int    use_unmasked_transport_bug; /* NDIFF_USE_UNMASKED_TRANSPORT_BUG (F, :209): must be 0                                          */
  int    ndiff_answer_date;          /* NDIFF_ANSWER_DATE (20240101, :217): <= 20240330 the interleaved sum :897-907, later the four
                                      * directional sums :909-922                                                                      */
  int    recalc_neutral_surf;        /* RECALC_NEUTRAL_SURF (F, MOM_tracer_hor_diff.F90:1747): read by mom6x_tracer_hordiff_neutral
                                      * alone, which has no other home for it                                                          */
  double RL2_T2_to_Pa;               /* EOS%RL2_T2_to_Pa (1): the pressure handed to the equation of state, MOM_EOS.F90:813            */
  double C_to_degC;                  /* EOS%C_to_degC (1): the temperature, MOM_EOS.F90:814, and dRdT :822                             */
  double S_to_ppt;                   /* EOS%S_to_ppt (1): the salinity, MOM_EOS.F90:815, and dRdS :823                                 */
  double kg_m3_to_R;                 /* EOS%kg_m3_to_R (1): the density derivatives, MOM_EOS.F90:820                                   */
} mom6x_neutral_diffusion_params;
/* neutral_diffusion_init :134: checks the members, keeps them with the equation of state and allocates every array the calls below
 * use, so that none of them allocates: Pint, Tint, Sint, dRdT, dRdS of nk + 1 planes; per face direction PoL, PoR (doubles) and
 * KoL, KoR (16-bit integers) on 2 nk + 2 surfaces and hEff on 2 nk + 1; the two flux arrays of 2 nk + 1 planes; Til, aL, aR and the
 * accumulator of the update (4 nk + 1 planes); Coef_x, Coef_y of mom6x_tracer_hordiff_neutral (2 nk + 2 planes).  A refused or
 * invalid call leaves no module behind, also where an earlier call had succeeded.  MOM6X_EUNSUPPORTED, naming the setting:
 * NDIFF_CONTINUOUS = False, NDIFF_INTERIOR_ONLY, NDIFF_TAPERING, KHTR_USE_EBT_STRUCT / KHTR_USE_SQG_STRUCT,
 * NDIFF_USE_UNMASKED_TRANSPORT_BUG, a non-Boussinesq context, a NULL equation of state (the module is only created with
 * temperature and salinity, :134).  MOM6X_EINVAL: an unknown EQN_OF_STATE form, more than 32766 layers.
 * The reference's neutral_diffusion_init refuses none of these settings: the compiled init has no FATAL and no WARNING for
 * NDIFF_CONTINUOUS = False (it goes on to set up MOM_remapping, :248-251), KHTR_USE_EBT_STRUCT / KHTR_USE_SQG_STRUCT (it allocates
 * Coef_h, :306-308) or NDIFF_USE_UNMASKED_TRANSPORT_BUG; it does not even read NDIFF_TAPERING unless NDIFF_INTERIOR_ONLY is set
 * (:195-200), so a lone NDIFF_TAPERING, which the device refuses, changes nothing there; and under NDIFF_INTERIOR_ONLY it is FATAL
 * only where the diabatic driver holds neither KPP nor ePBL (:296-298).  The refusals above are the device's alone; only an unknown
 * EQN_OF_STATE is FATAL there too (MOM_EOS.F90:1591).  tests/test_ref_parity_cpu.py holds this list to the compiled init.       */
int mom6x_neutral_diffusion_init(mom6x_ctx *ctx, const mom6x_neutral_diffusion_params *p, const mom6x_eos_params *eos);
/* The bytes that mom6x_neutral_diffusion_init allocated (0 before it). */
long long mom6x_neutral_diffusion_work_bytes(mom6x_ctx *ctx);
/* neutral_diffusion_calc_coeffs(G, GV, US, h, T, S, visc, CS, p_surf) :351-616, continuous arm, on the context's stream: no
 * allocation, no host synchronisation, no halo exchange.  h, T, S: 3-D device arrays, p_surf: a plane or NULL; each is read on
 * isc-1..iec+1 x jsc-1..jec+1 and nowhere else: the caller owes a halo of one.  Fills the module's interface state (Pint :436-445;
 * Tint, Sint by interface_scalar :1091 with PLM_diff(.., 2, 1, ..) and ppm_edge; dRdT, dRdS by calculate_density_derivs of every
 * form of mom6x_eos_form at Pint or ref_pres) and, at every u face I = isc-1..iec, j = jsc..jec and v face i = isc..iec,
 * J = jsc-1..jec, the positions of find_neutral_surface_positions_continuous :1368-1573 (bl_kl = bl_kr = 1, bl_zl = bl_zr = 0 as the
 * reference passes them, :543: the clamp :1541-1554 is the identity), hEff times 1 / (H_to_RZ g_Earth) (:592-597).  Dry faces
 * hold Po = hEff = 0 and Ko = 1 (:524-533).  The reference's `stop` and FATAL sites -- klm1, krm1 out of bounds :1426-1428,
 * Ppos < Pneg :1616 -- are unreachable with h >= 0; the device counts them (mom6x_neutral_diffusion_status), raises
 * the context's numeric flag, which makes mom6x_ctx_sync return MOM6X_ENUMERIC, and goes on with the value clamped.               */
int mom6x_neutral_diffusion_calc_coeffs(mom6x_ctx *ctx, const double *h, const double *T, const double *S, const double *p_surf);
/* neutral_diffusion(G, GV, h, Coef_x, Coef_y, dt, Reg, US, CS) :619-1032 without vertical structure or tapering, on the context's
 * stream: no allocation, no host synchronisation, no halo exchange -- the caller owes a halo of one on h and on every tracer.
 * tracers: the registry, a HOST array of ntr 3-D device arrays, updated in place on the computational domain only, one after the
 * other: neutral_surface_flux :2318-2496 (interface_scalar, ppm_left_right_edge_values :2562, ppm_ave :1181, the limiter :2457) at
 * the wet faces, then the update :894-937 in the order of additions ndiff_answer_date selects, with the underflow :927 and
 * :941-945.  conc_underflow: ntr HOST values or NULL.  Coef_x, Coef_y: device arrays of nk + 1 planes as the reference declares
 * them; ONLY PLANE 1 IS READ in this configuration (KhTh_use_vert_struct = 0).  dt: the time step times I_numitts, read only for
 * the diagnostics (Idt = 1 / dt).  tendency (3-D, the computational domain, 0 over land, :932), trans_x_2d (2-D, the u faces,
 * :962-970) and trans_y_2d (2-D, the v faces, :991-999): NULL or HOST arrays of ntr nullable device outputs.
 * MOM6X_EINVAL: a call before init or before the first calc_coeffs, a null array, dt <= 0 (whether or not a diagnostic is given).
 * ppm_ave's dx outside [0, 1] (:1203, :1205) is counted like the sites of calc_coeffs.
 * Not carried: dfxy_conc, dfxy_cont_2d, uhEff_2d, vhEff_2d (a host derives them from what is returned).                           */
int mom6x_neutral_diffusion(mom6x_ctx *ctx, const double *h, const double *Coef_x, const double *Coef_y, double dt,
                            double *const *tracers, const double *conc_underflow, int ntr, double *const *tendency,
                            double *const *trans_x_2d, double *const *trans_y_2d);
/* The module's resident coefficients, read only: dir 0 the u faces (uPoL, uPoR, uKoL, uKoR, uhEff), 1 the v faces.  Each is a stack
 * of pitched planes [surface][j + joff][i + ioff] like a 2-D field of the context, the face (I, j) | (i, J) at the index of the cell
 * it bounds to the east | north; Po: doubles, 2 nk + 2 planes; Ko: 16-bit integers (1-based layer indices), 2 nk + 2 planes; hEff:
 * doubles, 2 nk + 1 planes.  Words outside the face ranges of calc_coeffs are not defined.  Any pointer argument may be NULL.      */
int mom6x_neutral_diffusion_coeffs(mom6x_ctx *ctx, int dir, const double **PoL, const double **PoR, const short **KoL,
                                   const short **KoR, const double **hEff);
/* Waits for the context's stream and hands out how often each stop site was reached since init: counts[0] klm1 or krm1 out of bounds,
 * [1] Ppos < Pneg, [2] ppm_ave dx < 0, [3] ppm_ave dx > 1.                                                                       */
int mom6x_neutral_diffusion_status(mom6x_ctx *ctx, long long counts[4]);
/* The work-group (lanes along i, rows) of the module's kernels and the i of their first lane, for tests that place a grid's edges
 * where a launch extent rounds up to another block.                                                                              */
int mom6x_neutral_diffusion_tile(int *bx, int *by, int *i_first);

/* ------------------------------------------------------------------------- */
/* MOM_dynamics_split_RK2                                                    */

/* Host callbacks for the callees of step_MOM_dyn_split_RK2 that are NOT on the ported hot path
 * (SURVEY.md 8f).  All array arguments are DEVICE pointers.  A NULL callback means "keep what the
 * context already holds" (coefficients / diffu,diffv frozen over the step).                    */
typedef struct mom6x_rk2_hooks {
  void *user;
  /* set_viscous_ML + thickness_to_dz + vertvisc_coef (RK2.F90:602-609 stage 0, :737-738 stage 1,
   * :1002-1003 stage 2): must leave updated coefficients behind via mom6x_vertvisc_set_coef.   */
  int (*vertvisc_coef)(void *user, int stage, const double *u, const double *v, const double *h, double dt);
  /* horizontal_viscosity (RK2.F90:886): fills diffu, diffv.                                     */
  int (*horizontal_viscosity)(void *user, const double *u_av, const double *v_av, const double *h_av,
                              const double *uh, const double *vh, double *diffu, double *diffv);
} mom6x_rk2_hooks;

/* initialize_dyn_split_RK2 (RK2.F90:1346): allocates MOM_dyn_split_RK2_CS on the device (incl. the
 * BT_cont_type).  continuity, barotropic, CoriolisAdv, PressureForce must be initialised first,
 * as in :1552-1596.                                                                           */
int mom6x_initialize_dyn_split_RK2(mom6x_ctx *ctx, const mom6x_rk2_params *p);
/* The new-run fills of initialize_dyn_split_RK2 :1577-1650 (eta from h; u_av,v_av = u,v; h_av and
 * CAu_pred from one continuity + CorAdCalc pass).  A restarted run uploads the fields instead
 * (mom6x_rk2_field) and calls mom6x_rk2_set_CAu_pred_stored.                                   */
int mom6x_dyn_split_RK2_new_run(mom6x_ctx *ctx, const double *u, const double *v, const double *h,
                                double *uh, double *vh, double dt);
int mom6x_rk2_set_CAu_pred_stored(mom6x_ctx *ctx, int stored);
/* The same routine for a RESTARTED run (initialize_dyn_split_RK2 :1577-1668), field by field as the reference decides
 * with query_initialized: the host uploads the variables the restart file held (mom6x_rk2_field) and names them in
 * `have`; every other one is formed as the reference forms it -- eta from h (:1578-1590), diffu, diffv by
 * horizontal_viscosity (:1599-1606), u_av, v_av = u, v (:1608-1614), and, when CAu / CAv are absent, h_av from one
 * continuity call (or the file's uh, vh, h2: HAVE_UH + HAVE_H2, an older restart format) and CAu_pred, CAv_pred by
 * CorAdCalc (:1620-1640) -- followed by the group pass of :1670-1679.  have = 0 is mom6x_dyn_split_RK2_new_run.      */
#define MOM6X_RK2_HAVE_ETA   1   /* "sfc"            */
#define MOM6X_RK2_HAVE_DIFFU 2   /* "diffu", "diffv" */
#define MOM6X_RK2_HAVE_U2    4   /* "u2", "v2"       */
#define MOM6X_RK2_HAVE_CAU   8   /* "CAu", "CAv"     */
#define MOM6X_RK2_HAVE_UH    16  /* "uh", "vh"       */
#define MOM6X_RK2_HAVE_H2    32  /* "h2"             */
int mom6x_dyn_split_RK2_restart_fills(mom6x_ctx *ctx, const double *u, const double *v, const double *h,
                                      double *uh, double *vh, double dt, int have);
/* remap_dyn_split_RK2_aux_vars (RK2.F90:1302): after an ALE regridding the auxiliary restart variables move to the
 * new grid too -- u_av, v_av and CAu_pred, CAv_pred (STORE_CORIOLIS_ACCEL), then diffu, diffv, each pair with
 * ALE_remap_velocities and the first two followed by their pass_vector.  Returns at once unless REMAP_AUXILIARY_VARS.
 * p stands for ALE_CSp%vel_remapCS; the face thicknesses are those of mom6x_ALE_remap_set_h_vel.                  */
int mom6x_remap_dyn_split_RK2_aux_vars(mom6x_ctx *ctx, const mom6x_remapping_params *p, const double *h_old_u,
                                       const double *h_old_v, const double *h_new_u, const double *h_new_v);
/* Device pointers to the CS arrays MOM_restart registers (register_restarts_dyn_split_RK2 :1210:
 * sfc=eta, u2=u_av, v2=v_av, CAu, CAv, diffu, diffv) and the others, by name index:
 * 0 CAu, 1 CAv, 2 CAu_pred, 3 CAv_pred, 4 PFu, 5 PFv, 6 diffu, 7 diffv, 8 visc_rem_u, 9 visc_rem_v,
 * 10 u_accel_bt, 11 v_accel_bt, 12 u_av, 13 v_av, 14 h_av, 15 pbce, 16 eta, 17 eta_PF, 18 uhbt,
 * 19 vhbt, 20 taux_bot, 21 tauy_bot, 22 BT_cont%h_u, 23 BT_cont%h_v.                            */
double *mom6x_rk2_field(mom6x_ctx *ctx, int which);

/* step_MOM_dyn_split_RK2(u_inst, v_inst, h, tv, visc, Time_local, dt, forces, p_surf_begin,
 *   p_surf_end, uh, vh, uhtr, vhtr, eta_av, G, GV, US, CS, calc_dtbt, VarMix, MEKE,
 *   thickness_diffuse_CSp, pbv, STOCH, Waves)                       RK2.F90:294-296.
 * forces%taux/tauy are planes; tv (layered: no T,S), p_surf_*, VarMix, MEKE, STOCH, Waves absent. */
int mom6x_step_dyn_split_RK2(mom6x_ctx *ctx, double *u_inst, double *v_inst, double *h,
                             double *uh, double *vh, double *uhtr, double *vhtr, double *eta_av,
                             const double *taux, const double *tauy, double dt, int calc_dtbt,
                             const mom6x_rk2_hooks *hooks);

/* ------------------------------------------------------------------------- */
/* MOM_tracer_advect / MOM_diabatic_aux / MOM_tracer_diabatic                    */

/* TRACER_ADVECTION_SCHEME values (MOM_tracer_advect_schemes.F90:11-13)          */
#define MOM6X_ADVECT_PLM   0
#define MOM6X_ADVECT_PPMH3 1
#define MOM6X_ADVECT_PPM   2
/* tracer_advect_init (MOM_tracer_advect.F90:1155): DT, TRACER_ADVECTION_SCHEME ('PLM' default),
 * USE_HUYNH_STENCIL_BUG (F).                                                                       */
int mom6x_tracer_advect_init(mom6x_ctx *ctx, double dt_dyn, int default_scheme, int useHuynhStencilBug);
/* advect_tracer(h_end, uhtr, vhtr, OBC, dt, G, GV, US, CS, Reg, x_first_in, vol_prev, max_iter_in,
 *   update_vol_prev, uhr_out, vhr_out)                                MOM_tracer_advect.F90:53-54.
 * The registry Reg is an array of ntr device pointers (Reg%Tr(m)%t) with per-tracer schemes
 * (Reg%Tr(m)%advect_scheme; < 0 = the default).  x_first_in: -1 absent; max_iter_in: 0 absent;
 * uhr_out/vhr_out/iters_out nullable.  OBC unassociated; the offline-transport arguments (vol_prev,
 * update_vol_prev) are not supported.                                                              */
int mom6x_advect_tracer(mom6x_ctx *ctx, const double *h_end, const double *uhtr, const double *vhtr, double dt,
                        double *const *tracers, const int *schemes, int ntr, int x_first_in, int max_iter_in,
                        double *uhr_out, double *vhr_out, int *iters_out);
/* triDiagTS(G, GV, is, ie, js, je, hold, ea, eb, T, S)            MOM_diabatic_aux.F90:394; S may be NULL.
 * is..je are LOCAL 0-based indices (MOM6 is-isc etc.).                                             */
int mom6x_triDiagTS(mom6x_ctx *ctx, int is, int ie, int js, int je, const double *hold, const double *ea,
                    const double *eb, double *T, double *S);
/* triDiagTS_Eulerian(G, GV, is, ie, js, je, hold, ent, T, S)      :444; ent has nk+1 interfaces.     */
int mom6x_triDiagTS_Eulerian(mom6x_ctx *ctx, int is, int ie, int js, int je, const double *hold, const double *ent,
                             double *T, double *S);
/* tracer_vertdiff(h_old, ea, eb, dt, tr, G, GV, sfc_flux, btm_flux, btm_reservoir, sink_rate, convert_flux_in)
 * MOM_tracer_diabatic.F90:25 -- the branch without sink_rate (:181-214; btm_reservoir is only read with sink_rate).   */
int mom6x_tracer_vertdiff(mom6x_ctx *ctx, const double *h_old, const double *ea, const double *eb, double dt,
                          double *tr, const double *sfc_flux, const double *btm_flux, int convert_flux);
/* tracer_vertdiff_Eulerian(h_old, ent, dt, tr, G, GV, ...)         :224 (no-sink branch :382-414).     */
int mom6x_tracer_vertdiff_Eulerian(mom6x_ctx *ctx, const double *h_old, const double *ent, double dt, double *tr,
                                   const double *sfc_flux, const double *btm_flux, int convert_flux);
/* The same two routines WITH sink_rate (:123-179 / :315-380): the tracer sinks through the interfaces by up to sink_rate * dt,
 * limited so that characteristics do not cross within the step; with btm_reservoir (nullable = not present) the sinking is not
 * limited and what leaves the bottom layer is added to btm_reservoir [CU R Z].                                           */
int mom6x_tracer_vertdiff_sink(mom6x_ctx *ctx, const double *h_old, const double *ea, const double *eb, double dt,
                               double *tr, const double *sfc_flux, const double *btm_flux, double *btm_reservoir,
                               double sink_rate, int convert_flux);
int mom6x_tracer_vertdiff_Eulerian_sink(mom6x_ctx *ctx, const double *h_old, const double *ent, double dt, double *tr,
                                        const double *sfc_flux, const double *btm_flux, double *btm_reservoir,
                                        double sink_rate, int convert_flux);
/* diabatic (MOM_diabatic_driver.F90:277) is a host-side dispatcher.  Of what it calls, set_BBL_TKE and set_diffusivity
 * (mom6x_set_BBL_TKE, mom6x_set_diffusivity: the ALE-coordinate path), applyBoundaryFluxesInOut (mom6x_applyBoundaryFluxesInOut:
 * the surface fluxes) and the solvers above are on the device, so a resident, forced run forms ent = dt*Kd_int/dz there and
 * keeps h, T and S there; kappa shear, the boundary layer schemes (energetic_PBL now has its inputs cTKE, dSV_dT, dSV_dS and
 * SkinBuoyFlux on the device) and tidal mixing stay with the host.  Its early return for GV%ke == 1 (:330) is below.  */
int mom6x_diabatic_is_trivial(const mom6x_ctx *ctx);

/* ------------------------------------------------------------------------- */
/* MOM_domains: 2-D tile decomposition and halo updates over RCCL / xGMI         */

/* Index range (inclusive, local indices) of the region of a `stagger` field that is SENT to (send=1)
 * or RECEIVED from (send=0) the neighbour in direction dir = 0..7 (W,E,S,N,SW,SE,NW,NE).  Host-only,
 * no GPU needed: this is the exchange plan, tested on CPU with gloo.                              */
int mom6x_halo_region(const mom6x_dims *d, int stagger, int dir, int send, int *i0, int *i1, int *j0, int *j1);
/* Rank (px + npx*py) of the neighbour of tile (px,py) in direction dir, or -1 at a closed boundary. */
int mom6x_halo_neighbor(int npx, int npy, int px, int py, int dir, int reentrant_x, int reentrant_y);
/* A transport of the host's own instead of the process's RCCL: nine functions with RCCL's meaning (ncclGetUniqueId,
 * ncclCommInitRank, ncclCommDestroy, ncclSend, ncclRecv, ncclGroupStart, ncclGroupEnd, ncclAllReduce,
 * ncclGetErrorString), opaque handles as void*, return 0 for success.  For a host that wants its halo traffic in one
 * library (GPU-aware MPI: MOM6's own FMS domains) -- and how the layout tests run several tiles as threads of one
 * process on one GPU (tests/transport/).  Communicators made after the call use it; NULL returns to RCCL.           */
enum { MOM6X_T_INT32 = 0, MOM6X_T_INT64 = 1, MOM6X_T_FLOAT64 = 2 };
enum { MOM6X_OP_SUM = 0, MOM6X_OP_MIN = 1, MOM6X_OP_MAX = 2 };
typedef struct mom6x_transport {
  int (*get_unique_id)(char *id128);
  int (*comm_init_rank)(void **comm, int nranks, const char *id128, int rank);
  int (*comm_destroy)(void *comm);
  int (*send)(const void *buf, size_t count, int dtype, int peer, void *comm, void *stream);
  int (*recv)(void *buf, size_t count, int dtype, int peer, void *comm, void *stream);
  int (*group_start)(void);
  int (*group_end)(void);
  int (*all_reduce)(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *comm, void *stream);
  const char *(*error_string)(int rc);       /* nullable */
} mom6x_transport;
int mom6x_comm_set_transport(const mom6x_transport *t);
/* ncclGetUniqueId on the calling rank: 128 bytes the host broadcasts (MPI_Bcast / torch.distributed). */
int mom6x_comm_unique_id(char *id128);
/* Attach LAYOUT = npx,npy (MOM_domains.F90:155) with this tile at (px,py) and create the RCCL
 * communicator (clone of MOM_domains_init / create_group_pass's message plan).  After this call every
 * halo update inside the mom6x_* routines is a packed ncclSend/ncclRecv group exchange.            */
int mom6x_comm_init(mom6x_ctx *ctx, int npx, int npy, int px, int py, const char *id128, int force_nccl_self);
int mom6x_comm_rank(const mom6x_ctx *ctx);
/* do_group_pass of n fields (pass_var / pass_vector, MOM_domain_infra.F90:171-560, :1141).          */
int mom6x_pass_fields(mom6x_ctx *ctx, double *const *fields, const int *staggers, const int *nks, int n);
/* The halo width of the 3-D fields in the RK2 step's own group passes (the reference's create_group_pass calls of
 * MOM_dynamics_split_RK2.F90 run on G%Domain, i.e. with NIHALO).  For a context whose halo was widened for the barotropic solver
 * -- BT_USE_WIDE_HALOS with BTHALO > NIHALO, MOM_barotropic.F90:5446-5461: create the context with halo = max(NIHALO, BTHALO);
 * btstep then exchanges every halo / stencil sub-steps (:2505-2512) -- this keeps the 3-D messages at NIHALO rows.
 * width = 0: the context's halo (the default); otherwise 4 <= width <= the context's halo.  2-D fields (eta) always travel at
 * the context's width: btstep reads them over its wide halo.                                                          */
int mom6x_set_dyn_pass_width(mom6x_ctx *ctx, int width);
/* btstep's own group pass of eta, ubt, vbt (pass_eta_ubt, MOM_barotropic.F90:2505-2512) started on the second stream -- packed on the
 * compute stream, messages and unpack behind it -- while the compute stream runs the half of the next sub-step that reads the tile's
 * own points only, completed before the other half (start_group_pass / complete_group_pass around interior work).  Off by default
 * (see halo.hip: it loses on the one-GPU model); the answers do not depend on it.                                       */
int mom6x_comm_overlap_btstep(mom6x_ctx *ctx, int on);
/* Packed group exchanges (one message per neighbour each) this tile has made since the last reset; reset != 0 clears the count. */
long long mom6x_comm_exchange_count(mom6x_ctx *ctx, int reset);
/* ... and the bytes this tile sent in them (all neighbours together): what the per-pass halo widths of the RK2 step
 * (create_group_pass(..., halo=), RK2.F90:484-495) save over NIHALO rows of every field.                             */
long long mom6x_comm_exchange_bytes(mom6x_ctx *ctx, int reset);

/* ------------------------------------------------------------------------- */
/* The order-invariant sums and checksums of the reference's regression artefacts (ocean.stats, the debugging
 * checksum lines, the restart files' `checksum` attributes), evaluated on the device-resident fields.  Index
 * ranges are local compute indices, inclusive (h-point computational domain: 0..ni-1, 0..nj-1).  Across tiles
 * the integers are summed over RCCL unless only_on_PE is set.                                              */

/* reproducing_sum_3d (MOM_coms.F90:349): array = nk pitched planes.  sum: the result; sums (nullable, [nk]): the
 * sums by layer -- their presence changes how `sum` is formed (:470-477 vs :541-542), exactly as in the reference;
 * EFP_sum (nullable, [6]) and EFP_lay_sums (nullable, [6*nk]): the extended-fixed-point integers (EFP_type%v);
 * err (nullable): the reference's error code instead of a failure (+1 conversion overflow, +2 overflow, +2 NaN). */
int mom6x_reproducing_sum_3d(mom6x_ctx *ctx, const double *array, int nk, int is, int ie, int js, int je, double unscale,
                             int only_on_PE, double *sum, double *sums, int64_t *EFP_sum, int64_t *EFP_lay_sums, int *err);
/* reproducing_sum_2d (:235, reproducing = .true.) of one pitched plane; err: +2 overflow, +4 NaN (:205-209).   */
int mom6x_reproducing_sum_2d(mom6x_ctx *ctx, const double *array, int is, int ie, int js, int je, double unscale,
                             int only_on_PE, double *sum, int64_t *EFP_sum, int *err);

/* chksum_{h,u,v,B}_{2d,3d} (MOM_checksums.F90:387/:1413 h, :1005/:1782 u, :1209/:1986 v, :688/:1586 B; the pair
 * routines hchksum_pair / uvchksum / Bchksum_pair are two of these calls).  rank = 2 or 3 as the reference's 2-d and
 * 3-d routines differ for B points; stagger as in mom6x_upload; scale: nullable (absent).  The numbers of the two
 * message lines are returned; the host prints them (chk_sum_msg :2563-2640).                                   */
enum mom6x_chksum_kind { MOM6X_CHK_NONE = 0,      /* " c="                          (chk_sum_msg1)     */
                         MOM6X_CHK_CORNERS = 1,   /* " c=" "sw=" "se=" "nw=" "ne="  (chk_sum_msg5)     */
                         MOM6X_CHK_NSEW = 2,      /* " c=" "N=" "S=" "E=" "W="      (chk_sum_msg_NSEW) */
                         MOM6X_CHK_W = 3,         /* " c=" "W="                     (chk_sum_msg_W)    */
                         MOM6X_CHK_S = 4 };       /* " c=" "S="                     (chk_sum_msg_S)    */
typedef struct mom6x_chksum_result {
  double mean, amin, amax;   /* subStats: reproducing mean over the h-point domain, min and max (as printed: 0. + x) */
  int    bc0;                /* bit count of the unshifted computational domain, mod 1 000 000 000                    */
  int    bc[4];              /* the shifted bit counts in the order of the message                                    */
  int    nbc;                /* how many of bc[] are set: 0, 1 or 4                                                  */
  int    bc_kind;            /* enum mom6x_chksum_kind                                                               */
} mom6x_chksum_result;
int mom6x_chksum(mom6x_ctx *ctx, const double *array, int nk, int rank, int stagger, int haloshift, int symmetric,
                 int omit_corners, const double *scale, mom6x_chksum_result *out);

/* field_checksum_real_3d (MOM_checksums.F90:2480) -> field_chksum -> FMS mpp_chksum: the wrapping 64-bit integer sum
 * of the bit patterns of unscale*field over (is..ie, js..je, all k), the value MOM_restart.F90:1741-1749 stores as
 * the `checksum` attribute (written with Z16, MOM_io_infra.F90:1986) of every restart variable.                    */
int mom6x_field_chksum(mom6x_ctx *ctx, const double *array, int nk, int is, int ie, int js, int je, double unscale,
                       int64_t *chksum);

/* write_energy (MOM_sum_output.F90:321): the globally summed diagnostics behind ocean.stats (and ocean.stats.nc).
 * The members of Sum_output_CS that the sums read; the write schedule (ENERGYSAVEDAYS), the values of the previous
 * call (mass_prev_EFP ...), the accumulated surface inputs and the files stay with the host, which formats the line
 * from the numbers returned here (:871-905).                                                                     */
typedef struct mom6x_sum_output_params {
  int    do_APE_calc;       /* CALCULATE_APE (T)                                                       */
  int    use_temperature;   /* ENABLE_THERMODYNAMICS: salt and heat content from tv%T, tv%S            */
  double dt_in_T;           /* DT: the baroclinic time step of the CFL numbers                         */
  double D_list_min_inc;    /* DEPTH_LIST_MIN_INC (1e-10 m)                                            */
  double Z_ref;             /* G%Z_ref                                                                 */
  double C_p;               /* tv%C_p                                                                  */
} mom6x_sum_output_params;
/* MOM_sum_output_init :147 + depth_list_setup :1161 (READ_DEPTH_LIST = False: create_depth_list :1203 from the
 * context's bathyT, areaT, mask2dT; with several tiles the global list is summed over RCCL).  g_prime: GV%g_prime(1:nk). */
int mom6x_sum_output_init(mom6x_ctx *ctx, const mom6x_sum_output_params *p, const double *g_prime);
/* The Depth_List (DL%depth, DL%area, DL%vol_below); the arrays (nullable) must hold listsize entries -- call once
 * with null arrays to learn listsize.                                                                           */
int mom6x_depth_list(const mom6x_ctx *ctx, int *listsize, double *depth, double *area, double *vol_below);
typedef struct mom6x_energy_sums {
  double  mass_tot, KE_tot, PE_tot;   /* :509, :674, :660                                               */
  double  max_CFL[2];                 /* max_CFL_trans, max_CFL_lin :701-727                            */
  int64_t mass_EFP[6];                /* mass_EFP, for mass_chg_EFP = mass_EFP - CS%mass_prev_EFP :749  */
  int64_t salt_EFP[6], heat_EFP[6];   /* :683-686 (zero without ENABLE_THERMODYNAMICS)                  */
} mom6x_energy_sums;
/* u, v, h (and tv%T, tv%S, nullable without ENABLE_THERMODYNAMICS) on the device; mass_lay[nk], KE[nk], PE[nk+1],
 * Z_0APE[nk+1] on the host: the vectors of ocean.stats.nc (Mass_lay, KE, APE, H0).                          */
int mom6x_write_energy(mom6x_ctx *ctx, const double *u, const double *v, const double *h, const double *T, const double *S,
                       mom6x_energy_sums *out, double *mass_lay, double *KE, double *PE, double *Z_0APE);

#ifdef __cplusplus
}
#endif
#endif /* MOM6X_H */
