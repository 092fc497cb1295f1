"""ctypes mirror of include/mom6x.h and loader of the HIP C-ABI library.

The product path has NO CPU fallback: `load_library()` raises if
mom6_amd/lib/libmom6x.so is missing, and every compute entry point needs a GPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmom6x.so")

c_double_p = C.POINTER(C.c_double)


class Dims(C.Structure):
    """mom6x_dims (include/mom6x.h); MOM_hor_index.F90:14-44 extents."""
    _fields_ = [
        ("ni", C.c_int), ("nj", C.c_int), ("nk", C.c_int), ("halo", C.c_int),
        ("ioff", C.c_int), ("joff", C.c_int), ("pitch", C.c_int), ("slab", C.c_int),
        ("i_glob0", C.c_int), ("j_glob0", C.c_int), ("ni_glob", C.c_int), ("nj_glob", C.c_int),
        ("reentrant_x", C.c_int), ("reentrant_y", C.c_int),
    ]

    @property
    def nrows(self):
        return self.nj + 2 * self.halo + 1

    def shape2(self):
        return (self.nrows, self.pitch)

    def shape3(self, nk=None):
        return (self.nk if nk is None else nk, self.nrows, self.pitch)

    def sl(self, i0, i1, j0, j1):
        """numpy slices [j, i] for local inclusive ranges i0..i1, j0..j1."""
        return (slice(j0 + self.joff, j1 + self.joff + 1), slice(i0 + self.ioff, i1 + self.ioff + 1))


def dims_init(ni, nj, nk, halo=4, ni_glob=None, nj_glob=None, i_glob0=0, j_glob0=0,
              reentrant_x=False, reentrant_y=False):
    """Python twin of mom6x_dims_init (tested equal to the C one)."""
    if halo + 1 > 16:
        raise ValueError("halo too wide")
    d = Dims()
    d.ni, d.nj, d.nk, d.halo = ni, nj, nk, halo
    d.ioff = 16
    d.joff = halo + 1
    d.pitch = ((d.ioff + ni + halo + 15) // 16) * 16
    d.slab = d.pitch * (nj + 2 * halo + 1)
    d.ni_glob = ni if ni_glob is None else ni_glob
    d.nj_glob = nj if nj_glob is None else nj_glob
    d.i_glob0, d.j_glob0 = i_glob0, j_glob0
    d.reentrant_x, d.reentrant_y = int(reentrant_x), int(reentrant_y)
    return d


class VGrid(C.Structure):
    """mom6x_vgrid; MOM_verticalGrid.F90:25-90."""
    _fields_ = [
        ("g_Earth", C.c_double), ("Rho0", C.c_double), ("Angstrom_H", C.c_double),
        ("H_subroundoff", C.c_double), ("dZ_subroundoff", C.c_double),
        ("H_to_Z", C.c_double), ("Z_to_H", C.c_double), ("H_to_RZ", C.c_double),
        ("RZ_to_H", C.c_double), ("Boussinesq", C.c_int),
    ]


def vgrid_default(g_Earth=9.80, Rho0=1035.0, Angstrom=1e-10):
    """Defaults of verticalGridInit (MOM_verticalGrid.F90:100-230) with all US scalings = 1."""
    gv = VGrid()
    gv.g_Earth, gv.Rho0, gv.Angstrom_H = g_Earth, Rho0, Angstrom
    # verticalGrid.F90:214-218: H_subroundoff = 1e-20 * max(Angstrom_H, m_to_H*1e-17)
    gv.H_subroundoff = 1e-20 * max(Angstrom, 1e-17)
    gv.dZ_subroundoff = 1e-20 * max(Angstrom, 1e-17)
    gv.H_to_Z = gv.Z_to_H = 1.0
    gv.H_to_RZ = Rho0
    gv.RZ_to_H = 1.0 / Rho0
    gv.Boussinesq = 1
    return gv


class ContinuityParams(C.Structure):
    """mom6x_continuity_params; continuity_PPM_CS (MOM_continuity_PPM.F90:35-68)."""
    _fields_ = [
        ("upwind_1st", C.c_int), ("monotonic", C.c_int), ("simple_2nd", C.c_int),
        ("tol_eta", C.c_double), ("tol_vel", C.c_double), ("CFL_limit_adjust", C.c_double),
        ("aggress_adjust", C.c_int), ("vol_CFL", C.c_int), ("better_iter", C.c_int),
        ("use_visc_rem_max", C.c_int), ("marginal_faces", C.c_int), ("sum_order", C.c_int),
    ]


def continuity_params_default(nk, Angstrom=1e-10):
    """Defaults of continuity_PPM_init (MOM_continuity_PPM.F90:2674-2754)."""
    p = ContinuityParams()
    p.upwind_1st = p.monotonic = p.simple_2nd = 0
    p.tol_eta = 0.5 * nk * Angstrom
    p.tol_vel = 3.0e8
    p.CFL_limit_adjust = 0.5
    p.aggress_adjust = p.vol_CFL = 0
    p.better_iter = p.use_visc_rem_max = p.marginal_faces = 1
    p.sum_order = default_sum_order(nk)
    return p


SUM_REFERENCE, SUM_TREE16, SUM_TREE16_FMA = 0, 1, 2


def default_sum_order(nk):
    """Order of the column sums of the mass-flux kernels (mom6x_continuity_params.sum_order): the 16-lane tree of the
    wave-owned kernel with fused multiply-adds at fixed sites (MOM6X_SUM_TREE16_FMA, the default since round 6: 4 % faster, the
    same distance from the reference's arithmetic as the un-fused tree) unless MOM6X_SUMS=tree asks for the un-fused tree,
    MOM6X_SUMS=exact for the reference's sequential order (bit-identical to the Fortran loop nest, slower), or the column is
    deeper than the wave-owned kernel carries."""
    want = os.environ.get("MOM6X_SUMS", "").lower()
    if want in ("exact", "reference", "0") or nk > 128:
        return SUM_REFERENCE
    if want in ("tree", "tree16", "1"):
        return SUM_TREE16
    return SUM_TREE16_FMA


class BTCont(C.Structure):
    """mom6x_BT_cont; BT_cont_type (MOM_variables.F90:315-350)."""
    _names = ["FA_u_EE", "FA_u_E0", "FA_u_W0", "FA_u_WW", "uBT_WW", "uBT_EE",
              "FA_v_NN", "FA_v_N0", "FA_v_S0", "FA_v_SS", "vBT_SS", "vBT_NN", "h_u", "h_v"]
    _fields_ = [(n, C.c_void_p) for n in _names]


BT_THICK_FROM_BT_CONT, BT_THICK_HYBRID, BT_THICK_HARMONIC, BT_THICK_ARITHMETIC = 0, 1, 2, 3   # MOM6X_BT_THICK_*


class BarotropicParams(C.Structure):
    """mom6x_barotropic_params; barotropic_CS (MOM_barotropic.F90:108-330)."""
    _fields_ = [
        ("bebt", C.c_double), ("dtbt", C.c_double), ("dt_bt_filter", C.c_double),
        ("BT_project_velocity", C.c_int), ("Sadourny", C.c_int), ("strong_drag", C.c_int),
        ("wt_uv_bug", C.c_int), ("use_old_coriolis_bracket_bug", C.c_int),
        ("visc_rem_u_uh0", C.c_int), ("clip_velocity", C.c_int),
        ("CFL_trunc", C.c_double), ("vel_underflow", C.c_double), ("G_extra", C.c_double),
        ("BT_Coriolis_scale", C.c_double), ("maxCFL_BT_cont", C.c_double),
        ("bound_BT_corr", C.c_int), ("BT_cont_bounds", C.c_int),
        ("dtbt_fraction", C.c_double), ("Z_ref", C.c_double),
        ("use_wide_halos", C.c_int), ("BTHALO", C.c_int), ("min_stencil", C.c_int),
        ("nonlinear_continuity", C.c_int), ("nonlin_cont_update_period", C.c_int),
        ("bt_thick_scheme", C.c_int), ("maxvel", C.c_double),
    ]


def barotropic_params_default(dtbt):
    """Defaults read in barotropic_init (MOM_barotropic.F90:5403-5713)."""
    p = BarotropicParams()
    p.bebt, p.dtbt, p.dt_bt_filter = 0.1, dtbt, -0.25
    p.use_wide_halos, p.BTHALO, p.min_stencil = 1, 0, 0
    p.nonlinear_continuity, p.nonlin_cont_update_period = 0, 1
    p.bt_thick_scheme, p.maxvel = BT_THICK_FROM_BT_CONT, 3.0e8
    p.BT_project_velocity = 0
    p.Sadourny = 1
    p.strong_drag = 0
    p.wt_uv_bug = 1
    p.use_old_coriolis_bracket_bug = 0
    p.visc_rem_u_uh0 = 0
    p.clip_velocity = 0
    p.CFL_trunc, p.vel_underflow, p.G_extra = 0.5, 0.0, 0.0
    p.BT_Coriolis_scale, p.maxCFL_BT_cont = 1.0, 0.25
    p.bound_BT_corr, p.BT_cont_bounds = 0, 1
    p.dtbt_fraction, p.Z_ref = 0.98, 0.0
    return p


SADOURNY75_ENERGY, ARAKAWA_HSU90, ROBUST_ENSTRO, SADOURNY75_ENSTRO, ARAKAWA_LAMB81, AL_BLEND = 1, 2, 3, 4, 5, 6
KE_ARAKAWA, KE_SIMPLE_GUDONOV, KE_GUDONOV = 10, 11, 12
PV_ADV_CENTERED, PV_ADV_UPWIND1 = 21, 22


class CoriolisParams(C.Structure):
    """mom6x_coriolis_params; CoriolisAdv_CS (MOM_CoriolisAdv.F90:29-100)."""
    _fields_ = [("Coriolis_Scheme", C.c_int), ("KE_Scheme", C.c_int), ("bound_Coriolis", C.c_int),
                ("no_slip", C.c_int), ("Coriolis_En_Dis", C.c_int), ("PV_Adv_Scheme", C.c_int),
                ("F_eff_max_blend", C.c_double), ("wt_lin_blend", C.c_double)]


def coriolis_params_default():
    """Defaults of CoriolisAdv_init (MOM_CoriolisAdv.F90:1054-1320)."""
    p = CoriolisParams()
    p.Coriolis_Scheme, p.KE_Scheme = SADOURNY75_ENERGY, KE_ARAKAWA
    p.bound_Coriolis = p.no_slip = p.Coriolis_En_Dis = 0
    p.PV_Adv_Scheme, p.F_eff_max_blend, p.wt_lin_blend = PV_ADV_CENTERED, 4.0, 0.125   # :1126-1139, :1178-1192
    return p


class PGFParams(C.Structure):
    """mom6x_pgf_params; PressureForce_FV_CS (MOM_PressureForce_FV.F90:40-110)."""
    _fields_ = [("rho_ref", C.c_double), ("rho_ref_bug", C.c_int), ("Z_ref", C.c_double)]


class VertviscParams(C.Structure):
    """mom6x_vertvisc_params; vertvisc_CS (MOM_vert_friction.F90:39-180)."""
    _fields_ = [("Kv", C.c_double), ("Kvml_invZ2", C.c_double), ("Hmix", C.c_double), ("Hbbl", C.c_double),
                ("harm_BL_val", C.c_double), ("Kv_extra_bbl", C.c_double), ("harmonic_visc", C.c_int),
                ("bottomdraglaw", C.c_int), ("answer_date", C.c_int)]


def vertvisc_params_default(Kv=1.0e-4, Hmix=20.0, Hbbl=10.0):
    """vertvisc_init :3135 defaults; KV, HMIX_FIXED and HBBL have none in MOM6 (fail_if_missing)."""
    p = VertviscParams()
    p.Kv = Kv; p.Kvml_invZ2 = 0.0; p.Hmix = Hmix; p.Hbbl = Hbbl; p.harm_BL_val = 0.0; p.Kv_extra_bbl = 0.0
    p.harmonic_visc = 0; p.bottomdraglaw = 1; p.answer_date = 99991231
    return p


class SetViscParams(C.Structure):
    """mom6x_set_visc_params; the set_visc_CS members of set_viscous_BBL (MOM_set_viscosity.F90:46-133)."""
    _fields_ = [("bottomdraglaw", C.c_int), ("cdrag", C.c_double), ("drag_bg_vel", C.c_double), ("Hbbl", C.c_double),
                ("dz_bbl", C.c_double), ("BBL_thick_min", C.c_double), ("Kv_BBL_min", C.c_double), ("linear_drag", C.c_int),
                ("BBL_use_EOS", C.c_int), ("BBL_use_tidal_bg", C.c_int), ("body_force_drag", C.c_int),
                ("correct_BBL_bounds", C.c_int), ("RiNo_mix", C.c_int), ("channel_drag", C.c_int), ("Rad_Earth", C.c_double),
                ("L_to_Z", C.c_double), ("L_to_H", C.c_double), ("nkml", C.c_int), ("open_bcs", C.c_int), ("ice_shelf", C.c_int),
                ("SpV_avg", C.c_int)]


def set_visc_params_default(HBBL=10.0, Kv=1.0e-4, BBL_use_EOS=True):
    """set_visc_init :2876-3204 defaults (Boussinesq, unscaled units); HBBL and KV have none in MOM6 (fail_if_missing), and
    BBL_USE_EOS defaults to USE_EOS (:3060)."""
    p = SetViscParams()
    p.bottomdraglaw = 1; p.cdrag = 0.003; p.drag_bg_vel = 0.0
    p.dz_bbl = HBBL; p.Hbbl = HBBL          # CS%Hbbl = CS%dz_bbl * (US%Z_to_m * GV%m_to_H) (:3140)
    p.BBL_thick_min = 0.0; p.Kv_BBL_min = Kv
    p.linear_drag = 0; p.BBL_use_EOS = int(BBL_use_EOS); p.BBL_use_tidal_bg = 0; p.body_force_drag = 0
    p.correct_BBL_bounds = 0; p.RiNo_mix = 0; p.channel_drag = 0
    p.Rad_Earth = 6.378e6; p.L_to_Z = 1.0; p.L_to_H = 1.0
    p.nkml = 0; p.open_bcs = 0; p.ice_shelf = 0; p.SpV_avg = 0
    return p


class ThicknessDiffuseParams(C.Structure):
    """mom6x_thickness_diffuse_params; the thickness_diffuse_CS members of thickness_diffuse (MOM_thickness_diffuse.F90:41-128)."""
    _fields_ = [("thickness_diffuse", C.c_int), ("Khth", C.c_double), ("read_khth", C.c_int), ("Khth_Min", C.c_double),
                ("Khth_Max", C.c_double), ("max_Khth_CFL", C.c_double), ("slope_max", C.c_double), ("kappa_smooth", C.c_double),
                ("Z_to_L", C.c_double), ("Z_to_H_fill", C.c_double), ("Kh_eta_bg", C.c_double), ("Kh_eta_vel", C.c_double),
                ("use_FGNV_streamfn", C.c_int), ("use_stanley_gm", C.c_int), ("detangle_interfaces", C.c_int), ("use_GME", C.c_int),
                ("use_variable_mixing", C.c_int), ("use_MEKE", C.c_int), ("use_Kh_in_MEKE", C.c_int), ("GMwork", C.c_int),
                ("skeb_use_gm", C.c_int), ("nkml", C.c_int), ("open_bcs", C.c_int), ("non_Boussinesq", C.c_int)]


THICKNESS_DIFFUSE_MUST_BE_0 = ("use_FGNV_streamfn", "use_stanley_gm", "detangle_interfaces", "Kh_eta_bg", "Kh_eta_vel", "use_GME",
                               "use_variable_mixing", "use_MEKE", "use_Kh_in_MEKE", "GMwork", "skeb_use_gm", "nkml", "open_bcs",
                               "non_Boussinesq")


def thickness_diffuse_params_default(KHTH=600.0):
    """thickness_diffuse_init :2207-2401 defaults (Boussinesq, unscaled units) with THICKNESSDIFFUSE = True; KHTH defaults to 0 in
    MOM6, which switches the routine off (:196)."""
    p = ThicknessDiffuseParams()
    p.thickness_diffuse = 1; p.Khth = KHTH; p.read_khth = 0
    p.Khth_Min = 0.0; p.Khth_Max = 0.0; p.max_Khth_CFL = 0.8
    p.slope_max = 0.01; p.kappa_smooth = 1.0e-6
    p.Z_to_L = 1.0; p.Z_to_H_fill = 1.0
    for n in THICKNESS_DIFFUSE_MUST_BE_0:
        setattr(p, n, 0)
    return p


class TracerHorDiffParams(C.Structure):
    """mom6x_tracer_hor_diff_params; tracer_hor_diff_CS (MOM_tracer_hor_diff.F90:41-97) and the VarMix / MEKE switches of tracer_hordiff."""
    _fields_ = [("KhTr", C.c_double), ("KhTr_Slope_Cff", C.c_double), ("KhTr_min", C.c_double), ("KhTr_max", C.c_double),
                ("KhTr_passivity_coeff", C.c_double), ("KhTr_passivity_min", C.c_double), ("check_diffusive_CFL", C.c_int),
                ("max_diff_CFL", C.c_double), ("use_variable_mixing", C.c_int), ("Resoln_scaled_KhTr", C.c_int),
                ("use_MEKE_Kh", C.c_int), ("MEKE_KhTr_fac", C.c_double), ("use_neutral_diffusion", C.c_int),
                ("use_hor_bnd_diffusion", C.c_int), ("Diffuse_ML_interior", C.c_int), ("offline", C.c_int), ("open_bcs", C.c_int)]


TRACER_HOR_DIFF_MUST_BE_0 = ("use_neutral_diffusion", "use_hor_bnd_diffusion", "Diffuse_ML_interior", "offline", "open_bcs")


def tracer_hor_diff_params_default(KHTR=0.0, **kw):
    """tracer_hor_diff_init :1659-1707 defaults (unscaled units), no variable mixing, no MEKE; KHTR defaults to 0 in MOM6, which
    switches the routine off (:199)."""
    p = TracerHorDiffParams()
    p.KhTr = KHTR; p.KhTr_Slope_Cff = 0.0; p.KhTr_min = 0.0; p.KhTr_max = 0.0
    p.KhTr_passivity_coeff = 0.0; p.KhTr_passivity_min = 0.5
    p.check_diffusive_CFL = 0; p.max_diff_CFL = -1.0
    p.use_variable_mixing = 0; p.Resoln_scaled_KhTr = 0; p.use_MEKE_Kh = 0; p.MEKE_KhTr_fac = 0.0
    for n in TRACER_HOR_DIFF_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class VarMixParams(C.Structure):
    """mom6x_varmix_params; the VarMix_CS members of calc_slope_functions (MOM_lateral_mixing_coeffs.F90:38-215)."""
    _fields_ = [("calculate_Eady_growth_rate", C.c_int), ("use_stored_slopes", C.c_int), ("use_simpler_Eady_growth_rate", C.c_int),
                ("full_depth_Eady_growth_rate", C.c_int), ("kappa_smooth", C.c_double), ("Visbeck_S_max", C.c_double),
                ("Visbeck_L_scale", C.c_double), ("Eady_GR_D_scale", C.c_double), ("cropping_distance", C.c_double),
                ("VarMix_Ktop", C.c_int), ("h_min_N2", C.c_double), ("max_depth", C.c_double), ("H_to_Z", C.c_double),
                ("Z_to_L", C.c_double), ("L_to_m", C.c_double), ("H_to_RZ", C.c_double), ("Z_to_H_fill", C.c_double),
                ("Angstrom_Z", C.c_double), ("g_Earth", C.c_double), ("Rho0", C.c_double), ("use_stanley_iso", C.c_int),
                ("open_bcs", C.c_int), ("non_Boussinesq", C.c_int), ("debug", C.c_int)]


VARMIX_MUST_BE_0 = ("use_stanley_iso", "open_bcs", "non_Boussinesq", "debug")


def varmix_params_default(GV=None, max_depth=4000.0, **kw):
    """VarMix_init :1589-1758 defaults (Boussinesq, unscaled units) with the Eady growth rate wanted (KHTR_SLOPE_CFF or
    KHTH_SLOPE_CFF > 0, or MEKE, :1604): USE_STORED_SLOPES and USE_SIMPLER_EADY_GROWTH_RATE off, KD_SMOOTH = 1e-6,
    VISBECK_MAX_SLOPE = 0, VISBECK_L_SCALE = 0, EADY_GROWTH_RATE_D_SCALE = 0, EADY_GROWTH_RATE_CROPPING_DISTANCE = 0,
    VARMIX_KTOP = 2, MIN_DZ_FOR_SLOPE_N2 = 1 m, FULL_DEPTH_EADY_GROWTH_RATE off; the unit factors from GV; MAXIMUM_DEPTH has no
    default in MOM6."""
    GV = GV if GV is not None else vgrid_default()
    p = VarMixParams()
    p.calculate_Eady_growth_rate = 1; p.use_stored_slopes = 0; p.use_simpler_Eady_growth_rate = 0
    p.full_depth_Eady_growth_rate = 0
    p.kappa_smooth = 1.0e-6; p.Visbeck_S_max = 0.0; p.Visbeck_L_scale = 0.0; p.Eady_GR_D_scale = 0.0; p.cropping_distance = 0.0
    p.VarMix_Ktop = 2; p.h_min_N2 = 1.0 * GV.Z_to_H; p.max_depth = max_depth
    p.H_to_Z = GV.H_to_Z; p.Z_to_L = 1.0; p.L_to_m = 1.0; p.H_to_RZ = GV.H_to_RZ; p.Z_to_H_fill = 1.0
    p.Angstrom_Z = GV.Angstrom_H * GV.H_to_Z; p.g_Earth = GV.g_Earth; p.Rho0 = GV.Rho0
    for n in VARMIX_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class MixedLayerRestratParams(C.Structure):
    """mom6x_mixedlayer_restrat_params; the mixedlayer_restrat_CS members of mixedlayer_restrat_OM4 (MOM_mixed_layer_restrat.F90:37-140)."""
    _fields_ = [("ml_restrat_coef", C.c_double), ("ml_restrat_coef2", C.c_double), ("front_length", C.c_double),
                ("MLE_use_PBL_MLD", C.c_int), ("MLE_MLD_decay_time", C.c_double), ("MLE_MLD_decay_time2", C.c_double),
                ("MLE_density_diff", C.c_double), ("MLE_tail_dh", C.c_double), ("MLE_MLD_stretch", C.c_double), ("vonKar", C.c_double),
                ("ustar_min", C.c_double), ("use_Bodner", C.c_int), ("nkml", C.c_int), ("use_Stanley_ML", C.c_int),
                ("non_Boussinesq", C.c_int), ("open_bcs", C.c_int), ("debug", C.c_int)]


MIXEDLAYER_RESTRAT_MUST_BE_0 = ("use_Bodner", "nkml", "use_Stanley_ML", "non_Boussinesq", "open_bcs", "debug")


def mixedlayer_restrat_params_default(GV=None, omega=7.2921e-5, **kw):
    """mixedlayer_restrat_init :1784-1887 defaults (Boussinesq, unscaled units, NKML = 0): FOX_KEMPER_ML_RESTRAT_COEF and COEF2 = 0
    (the routine then moves nothing), MLE_FRONT_LENGTH = 0, MLE_USE_PBL_MLD off, both decay times 0, MLE_DENSITY_DIFF = 0.03 kg m-3,
    MLE_TAIL_DH = 0, MLE_MLD_STRETCH = 1, VON_KARMAN_CONST = 0.41, RESTRAT_USTAR_MIN = 2e-4*OMEGA*(Angstrom_Z + dZ_subroundoff)
    in thickness units (:1882-1887)."""
    GV = GV if GV is not None else vgrid_default()
    p = MixedLayerRestratParams()
    p.ml_restrat_coef = 0.0; p.ml_restrat_coef2 = 0.0; p.front_length = 0.0; p.MLE_use_PBL_MLD = 0
    p.MLE_MLD_decay_time = 0.0; p.MLE_MLD_decay_time2 = 0.0; p.MLE_density_diff = 0.03; p.MLE_tail_dh = 0.0
    p.MLE_MLD_stretch = 1.0; p.vonKar = 0.41
    p.ustar_min = (2.0e-4 * omega * (GV.Angstrom_H * GV.H_to_Z + GV.dZ_subroundoff)) * GV.Z_to_H
    for n in MIXEDLAYER_RESTRAT_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class MEKEParams(C.Structure):
    """mom6x_MEKE_params; the MEKE_CS members of the EKE_SOURCE = prog arm of step_forward_MEKE (MOM_MEKE.F90:54-168)."""
    _fields_ = [("MEKE_damping", C.c_double), ("MEKE_Cd_scale", C.c_double), ("MEKE_Cb", C.c_double), ("MEKE_min_gamma", C.c_double),
                ("MEKE_Ct", C.c_double), ("MEKE_GMcoeff", C.c_double), ("MEKE_GEOMETRIC", C.c_int), ("MEKE_GEOMETRIC_alpha", C.c_double),
                ("MEKE_equilibrium_alt", C.c_int), ("MEKE_equilibrium_restoring", C.c_int), ("MEKE_restoring_rate", C.c_double),
                ("MEKE_FrCoeff", C.c_double), ("MEKE_bhFrCoeff", C.c_double), ("MEKE_GMECoeff", C.c_double), ("MEKE_BGsrc", C.c_double),
                ("MEKE_Kh", C.c_double), ("MEKE_K4", C.c_double), ("MEKE_dtScale", C.c_double), ("MEKE_positive", C.c_int),
                ("MEKE_KhCoeff", C.c_double), ("MEKE_Uscale", C.c_double), ("GM_src_alt", C.c_int), ("MEKE_min_depth_tot", C.c_double),
                ("visc_drag", C.c_int), ("KhMEKE_Fac", C.c_double), ("use_old_lscale", C.c_int), ("use_min_lscale", C.c_int),
                ("lscale_maxval", C.c_double), ("Rd_as_max_scale", C.c_int), ("viscosity_coeff_Ku", C.c_double),
                ("viscosity_coeff_Au", C.c_double), ("Lfixed", C.c_double), ("fixed_total_depth", C.c_int), ("aDeform", C.c_double),
                ("aRhines", C.c_double), ("aEady", C.c_double), ("aFrict", C.c_double), ("aGrid", C.c_double),
                ("MEKE_advection_factor", C.c_double), ("MEKE_advection_bug", C.c_int), ("MEKE_topographic_beta", C.c_double),
                ("cdrag", C.c_double), ("T_to_s", C.c_double), ("L_to_m", C.c_double), ("m_s_to_L_T", C.c_double), ("cold_start", C.c_int),
                ("eke_source_file", C.c_int), ("eke_source_dbclient", C.c_int), ("use_Kh_diff", C.c_int), ("non_Boussinesq", C.c_int),
                ("open_bcs", C.c_int), ("debug", C.c_int)]


MEKE_MUST_BE_0 = ("eke_source_file", "eke_source_dbclient", "use_Kh_diff", "non_Boussinesq", "open_bcs", "debug")


def MEKE_params_default(GV=None, **kw):
    """MEKE_init :1400-1604 defaults (EKE_SOURCE = prog, Boussinesq, unscaled units): MEKE_DAMPING = 0, MEKE_CD_SCALE = 0, MEKE_CB = 25,
    MEKE_MIN_GAMMA2 = 1e-4, MEKE_CT = 50, MEKE_GMCOEFF = MEKE_FRCOEFF = MEKE_BHFRCOEFF = MEKE_GMECOEFF = -1, MEKE_GEOMETRIC off with
    alpha 0.05, MEKE_RESTORING_TIMESCALE = 1e6 s, MEKE_BGSRC = 0, MEKE_KH = MEKE_K4 = -1, MEKE_DTSCALE = 1, MEKE_KHCOEFF = 1,
    MEKE_USCALE = 0, MEKE_MIN_DEPTH_TOT = 1 m, MEKE_VISC_DRAG on, MEKE_KHMEKE_FAC = 0, MEKE_LSCALE_MAX_VAL = 1e7 m,
    MEKE_FIXED_TOTAL_DEPTH on, every alpha 0, MEKE_ADVECTION_FACTOR = 0, MEKE_TOPOGRAPHIC_BETA = 0, MEKE_CDRAG = CDRAG = 0.003 in the
    units of :1604, MEKE_COLD_START off."""
    GV = GV if GV is not None else vgrid_default()
    p = MEKEParams()
    p.MEKE_damping = 0.0; p.MEKE_Cd_scale = 0.0; p.MEKE_Cb = 25.0; p.MEKE_min_gamma = 1.0e-4; p.MEKE_Ct = 50.0
    p.MEKE_GMcoeff = -1.0; p.MEKE_GEOMETRIC = 0; p.MEKE_GEOMETRIC_alpha = 0.05; p.MEKE_equilibrium_alt = 0
    p.MEKE_equilibrium_restoring = 0; p.MEKE_restoring_rate = 1.0 / 1.0e6
    p.MEKE_FrCoeff = -1.0; p.MEKE_bhFrCoeff = -1.0; p.MEKE_GMECoeff = -1.0; p.MEKE_BGsrc = 0.0
    p.MEKE_Kh = -1.0; p.MEKE_K4 = -1.0; p.MEKE_dtScale = 1.0; p.MEKE_positive = 0; p.MEKE_KhCoeff = 1.0; p.MEKE_Uscale = 0.0
    p.GM_src_alt = 0; p.MEKE_min_depth_tot = 1.0 * GV.Z_to_H; p.visc_drag = 1; p.KhMEKE_Fac = 0.0
    p.use_old_lscale = 0; p.use_min_lscale = 0; p.lscale_maxval = 1.0e7; p.Rd_as_max_scale = 0
    p.viscosity_coeff_Ku = 0.0; p.viscosity_coeff_Au = 0.0; p.Lfixed = 0.0; p.fixed_total_depth = 1
    p.aDeform = 0.0; p.aRhines = 0.0; p.aEady = 0.0; p.aFrict = 0.0; p.aGrid = 0.0
    p.MEKE_advection_factor = 0.0; p.MEKE_advection_bug = 0; p.MEKE_topographic_beta = 0.0
    p.cdrag = 0.003 * (1.0 * GV.Z_to_H)
    p.T_to_s = 1.0; p.L_to_m = 1.0; p.m_s_to_L_T = 1.0; p.cold_start = 0
    for n in MEKE_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class SetDiffusivityParams(C.Structure):
    """mom6x_set_diffusivity_params; set_diffusivity_CS and its bkgnd_mixing_cs (MOM_set_diffusivity.F90:57-228,
    MOM_bkgnd_mixing.F90:40-100) as set_BBL_TKE and the ALE-coordinate path of set_diffusivity read them."""
    _fields_ = [("Kd", C.c_double), ("Kd_min", C.c_double), ("Kd_max", C.c_double), ("Kd_add", C.c_double), ("Kv", C.c_double),
                ("Kd_smooth", C.c_double), ("FluxRi_max", C.c_double), ("omega", C.c_double), ("answer_date", C.c_int),
                ("bottomdraglaw", C.c_int), ("cdrag", C.c_double), ("BBL_effic", C.c_double), ("ePBL_BBL_effic", C.c_double),
                ("ePBL_BBL_mstar", C.c_int), ("BBL_mixing_max_decay", C.c_double), ("use_LOTW_BBL_diffusivity", C.c_int),
                ("LOTW_BBL_use_omega", C.c_int), ("von_Karm", C.c_double), ("LOTW_BBL_answer_date", C.c_int),
                ("dissip_min", C.c_double), ("dissip_N0", C.c_double), ("dissip_N1", C.c_double), ("dissip_Kd_min", C.c_double),
                ("double_diffusion", C.c_int), ("Max_Rrho_salt_fingers", C.c_double), ("Max_salt_diff_salt_fingers", C.c_double),
                ("Kv_molecular", C.c_double), ("use_Kd_shear", C.c_int), ("physical_OBL_scheme", C.c_int), ("Kd_tot_ml", C.c_double),
                ("Hmix", C.c_double), ("Kd_via_Kdml_bug", C.c_int), ("prandtl_bkgnd", C.c_double), ("Henyey_IGW_background", C.c_int),
                ("N0_2Omega", C.c_double), ("Henyey_max_lat", C.c_double), ("Kd_tanh_lat_fn", C.c_int),
                ("Kd_tanh_lat_scale", C.c_double), ("g_Earth_Z_T2", C.c_double), ("Z_to_H_fill", C.c_double),
                ("m2_s_to_HZ_T", C.c_double), ("s_to_T", C.c_double), ("RL2_T2_to_Pa", C.c_double),
                ("ML_radiation", C.c_int), ("use_tidal_mixing", C.c_int), ("use_int_tides", C.c_int), ("use_CVMix_ddiff", C.c_int),
                ("Bryan_Lewis_diffusivity", C.c_int), ("horiz_varying_background", C.c_int), ("user_change_diff", C.c_int),
                ("nkml", C.c_int), ("SpV_avg", C.c_int), ("open_bcs", C.c_int)]


SET_DIFFUSIVITY_MUST_BE_0 = ("ML_radiation", "use_tidal_mixing", "use_int_tides", "use_CVMix_ddiff", "Bryan_Lewis_diffusivity",
                             "horiz_varying_background", "user_change_diff", "nkml", "SpV_avg", "open_bcs")


def set_diffusivity_params_default(GV=None, Kv=1.0e-4, Hmix=20.0, **kw):
    """set_diffusivity_init :2262-2700 and bkgnd_mixing_init defaults (Boussinesq, unscaled units): KD = 0 and with it KD_MIN and
    KD_ML_TOT, KD_MAX = -1, KD_ADD = 0, KD_SMOOTH = 1e-6, FLUX_RI_MAX = 0.2, OMEGA = 7.2921e-5, the newest answers but
    LOTW_BBL_ANSWER_DATE = 20190101, BOTTOMDRAGLAW on with CDRAG = 0.003, BBL_MIXING_MAX_DECAY = 200 m, LOTW_BBL_USE_OMEGA on,
    von Karman 0.41, no dissipation floors, no double diffusion (MAX_RRHO_SALT_FINGERS = 1.9, MAX_SALT_DIFF_SALT_FINGERS = 1e-4,
    KV_MOLECULAR = 1.5e-6), PRANDTL_BKGND = 1, no latitude function (HENYEY_N0_2OMEGA = 20, HENYEY_MAX_LAT = 95).  KV and
    HMIX_FIXED have no default in MOM6 (fail_if_missing).  Two departures, both because the reference's own defaults select a path
    that is not on the device: BBL_EFFIC = 0 instead of 0.2 (with USE_LOTW_BBL_DIFFUSIVITY = F that is add_drag_diffusivity), and a
    physically based boundary layer scheme is assumed (an OM4 run has ePBL), so that KD_ML_TOT plays no part."""
    GV = GV if GV is not None else vgrid_default()
    p = SetDiffusivityParams()
    p.Kd = 0.0; p.Kd_min = 0.0; p.Kd_max = -1.0; p.Kd_add = 0.0; p.Kv = Kv; p.Kd_smooth = 1.0e-6
    p.FluxRi_max = 0.2; p.omega = 7.2921e-5; p.answer_date = 99991231
    p.bottomdraglaw = 1; p.cdrag = 0.003; p.BBL_effic = 0.0; p.ePBL_BBL_effic = 0.0; p.ePBL_BBL_mstar = 0
    p.BBL_mixing_max_decay = 200.0 * GV.Z_to_H; p.use_LOTW_BBL_diffusivity = 0; p.LOTW_BBL_use_omega = 1; p.von_Karm = 0.41
    p.LOTW_BBL_answer_date = 20190101
    p.dissip_min = 0.0; p.dissip_N0 = 0.0; p.dissip_N1 = 0.0; p.dissip_Kd_min = 0.0
    p.double_diffusion = 0; p.Max_Rrho_salt_fingers = 1.9; p.Max_salt_diff_salt_fingers = 1.0e-4; p.Kv_molecular = 1.5e-6
    p.use_Kd_shear = 0; p.physical_OBL_scheme = 1; p.Kd_tot_ml = 0.0; p.Hmix = Hmix; p.Kd_via_Kdml_bug = 0; p.prandtl_bkgnd = 1.0
    p.Henyey_IGW_background = 0; p.N0_2Omega = 20.0; p.Henyey_max_lat = 95.0; p.Kd_tanh_lat_fn = 0; p.Kd_tanh_lat_scale = 0.0
    p.g_Earth_Z_T2 = GV.g_Earth; p.Z_to_H_fill = GV.Z_to_H; p.m2_s_to_HZ_T = 1.0; p.s_to_T = 1.0; p.RL2_T2_to_Pa = 1.0
    for n in SET_DIFFUSIVITY_MUST_BE_0:
        setattr(p, n, 0)
    if "Kd" in kw:                                  # KD_MIN and KD_ML_TOT default from KD (:2513, MOM_bkgnd_mixing.F90:171)
        p.Kd_min = 0.01 * kw["Kd"]; p.Kd_tot_ml = kw["Kd"]
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class DiabaticAuxParams(C.Structure):
    """mom6x_diabatic_aux_params; diabatic_aux_CS (MOM_diabatic_aux.F90:43-98) and the members of tv, US and optics_type
    (MOM_opacity.F90:25-61) that applyBoundaryFluxesInOut, extractFluxes1d and absorbRemainingSW read."""
    _fields_ = [("C_p", C.c_double), ("g_Earth_Z_T2", C.c_double), ("RL2_T2_to_Pa", C.c_double), ("ppt_to_S", C.c_double),
                ("rivermix_depth", C.c_double), ("dSalt_frac_max", C.c_double), ("PenSW_flux_absorb", C.c_double),
                ("PenSW_absorb_Invlen", C.c_double), ("optics_answer_date", C.c_int), ("do_rivermix", C.c_int),
                ("use_river_heat_content", C.c_int), ("use_calving_heat_content", C.c_int), ("ignore_fluxes_over_land", C.c_int),
                ("do_brine_plume", C.c_int), ("enthalpy_from_coupler", C.c_int), ("SpV_avg", C.c_int), ("nkml", C.c_int)]


DIABATIC_AUX_MUST_BE_0 = ("do_brine_plume", "enthalpy_from_coupler", "SpV_avg", "nkml")


def diabatic_aux_params_default(GV=None, **kw):
    """diabatic_aux_init (MOM_diabatic_aux.F90:1392-1452) and opacity_init (MOM_opacity.F90:1162-1184) defaults, Boussinesq and
    unscaled: C_P = 3991.86795711963, SALT_EXTRACTION_LIMIT = 0.9999, no river mixing, no river or calving heat content, fluxes
    over land are checked, the newest optics answers with PEN_SW_FLUX_ABSORB = 2.5e-11 and PEN_SW_ABSORB_MINTHICK = 1 m."""
    GV = GV if GV is not None else vgrid_default()
    p = DiabaticAuxParams()
    p.C_p = 3991.86795711963; p.g_Earth_Z_T2 = GV.g_Earth; p.RL2_T2_to_Pa = 1.0; p.ppt_to_S = 1.0
    p.rivermix_depth = 0.0; p.dSalt_frac_max = 0.9999
    p.optics_answer_date = 99991231
    p.PenSW_flux_absorb = 2.5e-11
    p.do_rivermix = 0; p.use_river_heat_content = 0; p.use_calving_heat_content = 0; p.ignore_fluxes_over_land = 0
    for n in DIABATIC_AUX_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    if "PenSW_absorb_Invlen" not in kw:            # PEN_SW_ABSORB_MINTHICK defaults from the answer date (MOM_opacity.F90:1179-1184)
        p.PenSW_absorb_Invlen = 1.0 / ((0.001 if p.optics_answer_date < 20190101 else 1.0) + GV.H_subroundoff)
    return p


SURFACE_FLUXES_IN = ("sw", "lw", "latent", "sens", "evap", "lprec", "fprec", "vprec", "lrunoff", "frunoff", "lrunoff_glc",
                     "frunoff_glc", "seaice_melt")
SURFACE_FLUXES_IN_NULLABLE = ("seaice_melt_heat", "heat_added", "salt_flux")
SURFACE_FLUXES_RUNOFF_HEAT = ("heat_content_lrunoff", "heat_content_lrunoff_glc", "heat_content_frunoff", "heat_content_frunoff_glc")
SURFACE_FLUXES_OUT = ("netMassIn", "netMassOut", "heat_content_massin", "heat_content_massout", "heat_content_lprec",
                      "heat_content_fprec", "heat_content_vprec", "heat_content_cond")
SURFACE_FLUXES_INOUT = ("TempxPmE",)
SURFACE_FLUXES_NAMES = (SURFACE_FLUXES_IN + SURFACE_FLUXES_IN_NULLABLE + SURFACE_FLUXES_RUNOFF_HEAT + SURFACE_FLUXES_OUT +
                        SURFACE_FLUXES_INOUT)


class SurfaceFluxes(C.Structure):
    """mom6x_surface_fluxes: the members of `forcing` that applyBoundaryFluxesInOut touches, as device planes (None: not associated)."""
    _fields_ = [(n, C.c_void_p) for n in SURFACE_FLUXES_NAMES]


TFREEZE_LINEAR, TFREEZE_MILLERO, TFREEZE_TEOS10, TFREEZE_TEOSPOLY = 1, 2, 3, 4   # enum mom6x_tfreeze_form (MOM_EOS.F90:184-187)


class FrazilParams(C.Structure):
    """mom6x_frazil_params: what make_frazil (MOM_diabatic_aux.F90:110-230) reads of diabatic_aux_CS, tv and tv%eqn_of_state
    (calculate_TFreeze, MOM_EOS.F90:664-744)."""
    _fields_ = ([(n, C.c_double) for n in ("C_p", "RL2_T2_to_Pa", "S_to_ppt", "degC_to_C", "TFr_S0_P0", "dTFr_dS", "dTFr_dp")] +
                [(n, C.c_int) for n in ("form_of_TFreeze", "reclaim_frazil", "pressure_dependent_frazil", "use_conT_absS")])


def frazil_params_default(**kw):
    """diabatic_aux_init (MOM_diabatic_aux.F90:1392-1410) and EOS_init (MOM_EOS.F90:1540-1575) defaults, unscaled:
    C_P = 3991.86795711963, RECLAIM_FRAZIL = True, PRESSURE_DEPENDENT_FRAZIL = False, TFREEZE_FORM = LINEAR with
    TFREEZE_S0_P0 = 0, DTFREEZE_DS = -0.054, DTFREEZE_DP = 0."""
    p = FrazilParams()
    p.C_p = 3991.86795711963; p.RL2_T2_to_Pa = 1.0; p.S_to_ppt = 1.0; p.degC_to_C = 1.0
    p.TFr_S0_P0 = 0.0; p.dTFr_dS = -0.054; p.dTFr_dp = 0.0
    p.form_of_TFreeze = TFREEZE_LINEAR; p.reclaim_frazil = 1; p.pressure_dependent_frazil = 0; p.use_conT_absS = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class GeothermalParams(C.Structure):
    """mom6x_geothermal_params: what geothermal_in_place (MOM_geothermal.F90:364-535) reads of geothermal_CS, tv, GV and US."""
    _fields_ = [(n, C.c_double) for n in ("C_p", "geothermal_thick", "g_Earth_Z_T2", "RL2_T2_to_Pa")]


def geothermal_params_default(GV=None, **kw):
    """geothermal_init (MOM_geothermal.F90:579) defaults, Boussinesq and unscaled: GEOTHERMAL_THICKNESS = 0.1 m."""
    GV = GV if GV is not None else vgrid_default()
    p = GeothermalParams()
    p.C_p = 3991.86795711963; p.geothermal_thick = 0.1 * GV.Z_to_H; p.g_Earth_Z_T2 = GV.g_Earth; p.RL2_T2_to_Pa = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


OPACITY_MANIZZA_05, OPACITY_MOREL_88, OPACITY_SINGLE_EXP, OPACITY_DOUBLE_EXP, OPACITY_OHLMANN_03 = 1, 2, 3, 4, 5   # enum mom6x_opacity_scheme (MOM_opacity.F90:105-106)


class OpacityParams(C.Structure):
    """mom6x_opacity_params: what opacity_init (MOM_opacity.F90:1041-1315) reads into opacity_CS and optics_type for set_opacity."""
    _fields_ = ([(n, C.c_double) for n in ("pen_sw_scale", "pen_sw_scale_2nd", "sw_1st_exp_ratio", "pen_sw_frac", "blue_frac",
                                           "opacity_land_value")] +
                [("manizza_coef", C.c_double * 6), ("manizza_power", C.c_double * 3), ("morel_coef", C.c_double * 6),
                 ("morel_pen_coef", C.c_double * 6), ("Z_to_m", C.c_double), ("m_to_Z", C.c_double),
                 ("opacity_scheme", C.c_int), ("nbands", C.c_int)])


def opacity_params_default(**kw):
    """opacity_init (MOM_opacity.F90:1104-1106, :1125-1145, :1193, :1198, :1205, :1210, :1287) defaults, unscaled, with
    VAR_PEN_SW = True: OPACITY_SCHEME = MANIZZA_05, PEN_SW_NBANDS = 1, BLUE_FRAC_SW = 0.5, PEN_SW_SCALE = PEN_SW_SCALE_2ND =
    SW_1ST_EXP_RATIO = PEN_SW_FRAC = 0, OPACITY_LAND_VALUE = 10 m-1 and the Manizza and Morel coefficients.  Array members take
    a sequence.  SINGLE_EXP carries sw_1st_exp_ratio = 1 in the reference (:1141); it is not read by that scheme."""
    p = OpacityParams()
    p.pen_sw_scale = 0.0; p.pen_sw_scale_2nd = 0.0; p.sw_1st_exp_ratio = 0.0; p.pen_sw_frac = 0.0; p.blue_frac = 0.5
    p.opacity_land_value = 10.0
    p.manizza_coef[:] = (0.0232, 0.074, 0.225, 0.037, 2.86, 0.0)
    p.manizza_power[:] = (0.674, 0.629, 0.0)
    p.morel_coef[:] = (7.925, -6.644, 3.662, -1.815, -0.218, 0.502)
    p.morel_pen_coef[:] = (0.321, 0.008, 0.132, 0.038, -0.017, -0.007)
    p.Z_to_m = 1.0; p.m_to_Z = 1.0
    p.opacity_scheme = OPACITY_MANIZZA_05; p.nbands = 1
    for k, v in kw.items():
        if k in ("manizza_coef", "manizza_power", "morel_coef", "morel_pen_coef"):
            getattr(p, k)[:] = tuple(v)
        else:
            setattr(p, k, v)
    return p


EPBL_MSTAR_CONSTANT, EPBL_MSTAR_OM4, EPBL_MSTAR_REICHL_H18 = 0, 2, 3  # enum mom6x_epbl_mstar_scheme (MOM_energetic_PBL.F90:279-282)
EPBL_WT_CUBE_ROOT_TKE, EPBL_WT_REICHL_H18 = 0, 1                     # enum mom6x_epbl_wT_scheme (:288-290)


class EnergeticPBLParams(C.Structure):
    """mom6x_energetic_PBL_params; what energetic_PBL_init (MOM_energetic_PBL.F90:3729-4429) leaves in energetic_PBL_CS (:38-276)
    for the surface boundary layer, with the members of GV and US that energetic_PBL and ePBL_column read."""
    _fields_ = ([(n, C.c_double) for n in (
        "omega", "omega_frac", "Ekman_scale_coef", "vonKar", "MKE_to_TKE_effic", "TKE_decay", "fixed_mstar", "mstar_cap", "mstar_coef",
        "C_Ek", "RH18_mstar_cn1", "RH18_mstar_cn2", "RH18_mstar_cn3", "RH18_mstar_cs1", "RH18_mstar_cs2", "nstar", "mstar_convect_coef",
        "transLay_scale", "MLD_tol", "min_mix_len", "MixLenExponent", "wstar_ustar_coef", "vstar_scale_fac", "vstar_surf_fac",
        "ustar_min", "g_Earth_Z_T2", "m_to_Z", "T_to_s", "ePBL_BBL_effic", "ePBL_tidal_effic")] +
                [(n, C.c_int) for n in (
                    "answer_date", "orig_PE_calc", "mstar_scheme", "Use_MLD_iteration", "MLD_iteration_guess", "MLD_bisection",
                    "MLD_iter_bug", "max_MLD_its", "wT_scheme", "TKE_diagnostics", "has_eos", "ePBL_BBL_use_mstar", "use_LT", "eqdisc",
                    "eqdisc_v0", "eqdisc_v0h", "direct_calc", "options_diff", "pert_epbl", "ustar_shelf", "tau_mag", "SpV_avg")])


ENERGETIC_PBL_MUST_BE_0 = ("ePBL_BBL_effic", "ePBL_tidal_effic", "ePBL_BBL_use_mstar", "use_LT", "eqdisc", "eqdisc_v0", "eqdisc_v0h",
                           "direct_calc", "options_diff", "pert_epbl", "ustar_shelf", "tau_mag", "SpV_avg")


def energetic_PBL_params_default(GV=None, **kw):
    """energetic_PBL_init (MOM_energetic_PBL.F90:3767-4328) defaults, Boussinesq and unscaled: OMEGA = 7.2921e-5, ML_OMEGA_FRAC = 0,
    the newest answers, EPBL_ORIGINAL_PE_CALC = True, TKE_DECAY = 2.5, EPBL_MSTAR_SCHEME = CONSTANT with MSTAR = 1.2, NSTAR = 0.2,
    USE_MLD_ITERATION with EPBL_TRANSITION_SCALE = 0.1, a tolerance of 1 m, at most 20 iterations and EPBL_MLD_ITER_BUG as
    ENABLE_BUGS_BY_DEFAULT has it, MIX_LEN_EXPONENT = 2, EPBL_VEL_SCALE_SCHEME = CUBE_ROOT_TKE; ustar_min as :4328.  A given
    Use_MLD_iteration = 0 sets max_MLD_its = 1 (:3999)."""
    GV = GV if GV is not None else vgrid_default()
    p = EnergeticPBLParams()
    p.omega = 7.2921e-5; p.omega_frac = 0.0; p.Ekman_scale_coef = 1.0; p.vonKar = 0.41; p.MKE_to_TKE_effic = 0.0; p.TKE_decay = 2.5
    p.fixed_mstar = 1.2; p.mstar_cap = -1.0; p.mstar_coef = 0.3; p.C_Ek = 0.085
    p.RH18_mstar_cn1 = 0.275; p.RH18_mstar_cn2 = 8.0; p.RH18_mstar_cn3 = -5.0; p.RH18_mstar_cs1 = 0.2; p.RH18_mstar_cs2 = 0.4
    p.nstar = 0.2; p.mstar_convect_coef = 0.0; p.transLay_scale = 0.1; p.MLD_tol = 1.0; p.min_mix_len = 0.0; p.MixLenExponent = 2.0
    p.wstar_ustar_coef = 1.0; p.vstar_scale_fac = 1.0; p.vstar_surf_fac = 1.2
    p.g_Earth_Z_T2 = GV.g_Earth; p.m_to_Z = 1.0; p.T_to_s = 1.0
    p.answer_date = 99991231; p.orig_PE_calc = 1; p.mstar_scheme = EPBL_MSTAR_CONSTANT; p.Use_MLD_iteration = 1
    p.MLD_iteration_guess = 0; p.MLD_bisection = 0; p.MLD_iter_bug = 1; p.max_MLD_its = 20; p.wT_scheme = EPBL_WT_CUBE_ROOT_TKE
    p.TKE_diagnostics = 0; p.has_eos = 1
    for n in ENERGETIC_PBL_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    if "ustar_min" not in kw:                      # Angstrom_Z = H_to_Z * Angstrom_H
        p.ustar_min = 2e-4 * p.omega * (GV.H_to_Z * GV.Angstrom_H + GV.dZ_subroundoff)
    if not p.Use_MLD_iteration:
        p.max_MLD_its = 1
    return p


class KappaShearParams(C.Structure):
    """mom6x_kappa_shear_params; what kappa_shear_init (MOM_kappa_shear.F90:2070-2330) leaves in Kappa_shear_CS (:34-126), with the
    members of US, GV and the EOS type that the routines read.  (`lambda` is a Python keyword: getattr(p, "lambda"), or the
    property lambda_.)"""
    _fields_ = ([(n, C.c_double) for n in (
        "RiNo_crit", "Shearmix_rate", "FRi_curvature", "C_N", "C_S", "lambda", "lambda2_N_S", "lz_rescale", "TKE_bg", "kappa_0",
        "kappa_seed", "kappa_trunc", "kappa_tol_err", "Prandtl_turb", "vel_underflow", "kappa_src_max_chg", "m_to_Z", "T_to_s",
        "L_to_Z", "Z_to_m_m_to_H", "g_Earth_Z_T2", "RL2_T2_to_Pa", "kg_m3_to_R")] +
                [(n, C.c_int) for n in (
                    "max_RiNo_it", "max_KS_it", "nkml", "eliminate_massless", "dKdQ_iteration_bug", "all_layer_TKE_bug",
                    "restrictive_tolerance_check", "KS_at_vertex", "work_columns")])

    @property
    def lambda_(self):
        return getattr(self, "lambda")

    @lambda_.setter
    def lambda_(self, v):
        setattr(self, "lambda", v)


KAPPA_SHEAR_MUST_BE_0 = ("KS_at_vertex",)


def kappa_shear_params_default(GV=None, **kw):
    """kappa_shear_init (MOM_kappa_shear.F90:2157-2289) defaults, Boussinesq and unscaled: RINO_CRIT = 0.25, SHEARMIX_RATE = 0.089,
    FRI_CURVATURE = -0.97, TKE_N_DECAY_CONST = 0.24, TKE_SHEAR_DECAY_CONST = 0.14, KAPPA_BUOY_SCALE_COEF = 0.82, LZ_RESCALE = 1,
    KD_KAPPA_SHEAR_0 = 1e-7 (KD = 0), KD_SEED_KAPPA_SHEAR = 1, KAPPA_SHEAR_TOL_ERR = 0.1, MAX_RINO_IT = 50, MAX_KAPPA_SHEAR_IT = 13,
    KAPPA_SHEAR_MAX_KAP_SRC_CHG = 10, massless layers eliminated, no bulk mixed layer (nkml = 1), every bug switch off.
    KD_TRUNC_KAPPA_SHEAR follows kappa_0 (0.01 of it, :2185) unless given.  lambda is given as lambda_."""
    GV = GV if GV is not None else vgrid_default()
    p = KappaShearParams()
    p.RiNo_crit = 0.25; p.Shearmix_rate = 0.089; p.FRi_curvature = -0.97; p.C_N = 0.24; p.C_S = 0.14; p.lambda_ = 0.82
    p.lambda2_N_S = 0.0; p.lz_rescale = 1.0; p.TKE_bg = 0.0; p.kappa_0 = 1.0e-7; p.kappa_seed = 1.0; p.kappa_tol_err = 0.1
    p.Prandtl_turb = 1.0; p.vel_underflow = 0.0; p.kappa_src_max_chg = 10.0
    p.m_to_Z = 1.0; p.T_to_s = 1.0; p.L_to_Z = 1.0; p.Z_to_m_m_to_H = 1.0; p.g_Earth_Z_T2 = GV.g_Earth
    p.RL2_T2_to_Pa = 1.0; p.kg_m3_to_R = 1.0
    p.max_RiNo_it = 50; p.max_KS_it = 13; p.nkml = 1; p.eliminate_massless = 1; p.dKdQ_iteration_bug = 0; p.all_layer_TKE_bug = 0
    p.restrictive_tolerance_check = 0; p.work_columns = 0
    for n in KAPPA_SHEAR_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    if "kappa_trunc" not in kw:
        p.kappa_trunc = 0.01 * p.kappa_0
    return p


class NeutralDiffusionParams(C.Structure):
    """mom6x_neutral_diffusion_params; what neutral_diffusion_init (MOM_neutral_diffusion.F90:134-345) leaves in
    neutral_diffusion_CS, with RECALC_NEUTRAL_SURF of tracer_hor_diff_CS and the unit factors of the EOS type."""
    _fields_ = [("continuous_reconstruction", C.c_int), ("ref_pres", C.c_double), ("interior_only", C.c_int), ("tapering", C.c_int),
                ("KhTh_use_vert_struct", C.c_int), ("use_unmasked_transport_bug", C.c_int), ("ndiff_answer_date", C.c_int),
                ("recalc_neutral_surf", C.c_int), ("RL2_T2_to_Pa", C.c_double), ("C_to_degC", C.c_double), ("S_to_ppt", C.c_double),
                ("kg_m3_to_R", C.c_double)]


NEUTRAL_DIFFUSION_MUST_BE_0 = ("interior_only", "tapering", "KhTh_use_vert_struct", "use_unmasked_transport_bug")


def neutral_diffusion_params_default(**kw):
    """neutral_diffusion_init (MOM_neutral_diffusion.F90:181-217) defaults, unscaled: NDIFF_CONTINUOUS = True, NDIFF_REF_PRES = -1
    (the local interface pressure), NDIFF_ANSWER_DATE = 20240101 (:222: not yet DEFAULT_ANSWER_DATE), RECALC_NEUTRAL_SURF = False;
    everything the device refuses is off."""
    p = NeutralDiffusionParams()
    p.continuous_reconstruction = 1; p.ref_pres = -1.0; p.ndiff_answer_date = 20240101; p.recalc_neutral_surf = 0
    p.RL2_T2_to_Pa = 1.0; p.C_to_degC = 1.0; p.S_to_ppt = 1.0; p.kg_m3_to_R = 1.0
    for n in NEUTRAL_DIFFUSION_MUST_BE_0:
        setattr(p, n, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class HorViscParams(C.Structure):
    """mom6x_hor_visc_params; hor_visc_CS (MOM_hor_visc.F90:36-259)."""
    _fields_ = [("Laplacian", C.c_int), ("biharmonic", C.c_int), ("Kh", C.c_double), ("Kh_bg_min", C.c_double),
                ("Kh_vel_scale", C.c_double), ("Smagorinsky_Kh", C.c_int), ("Smag_Lap_const", C.c_double), ("bound_Kh", C.c_int),
                ("better_bound_Kh", C.c_int), ("add_LES_viscosity", C.c_int), ("Ah", C.c_double), ("Ah_vel_scale", C.c_double),
                ("Ah_time_scale", C.c_double), ("Smagorinsky_Ah", C.c_int), ("Smag_bi_const", C.c_double), ("bound_Ah", C.c_int),
                ("better_bound_Ah", C.c_int), ("bound_Coriolis", C.c_int), ("bound_Cor_vel", C.c_double), ("use_land_mask", C.c_int),
                ("bound_coef", C.c_double), ("no_slip", C.c_int), ("backscatter_underbound", C.c_int), ("dt", C.c_double),
                ("Leith_Kh", C.c_int), ("Leith_Lap_const", C.c_double), ("Leith_Ah", C.c_int), ("Leith_bi_const", C.c_double),
                ("modified_Leith", C.c_int), ("use_beta_in_Leith", C.c_int)]


def hor_visc_params_default(dt, Laplacian=False, biharmonic=True):
    """hor_visc_init :2403-2720 defaults (LAPLACIAN F, BIHARMONIC T, bounds on, everything else off / zero)."""
    p = HorViscParams()
    p.Laplacian = int(Laplacian); p.biharmonic = int(biharmonic)
    p.Kh = 0.0; p.Kh_bg_min = 0.0; p.Kh_vel_scale = 0.0; p.Smagorinsky_Kh = 0; p.Smag_Lap_const = 0.0
    p.bound_Kh = 1; p.better_bound_Kh = 1; p.add_LES_viscosity = 0
    p.Ah = 0.0; p.Ah_vel_scale = 0.0; p.Ah_time_scale = 0.0; p.Smagorinsky_Ah = 0; p.Smag_bi_const = 0.0
    p.bound_Ah = 1; p.better_bound_Ah = 1; p.bound_Coriolis = 0; p.bound_Cor_vel = 3.0e8
    p.use_land_mask = 1; p.bound_coef = 0.8; p.no_slip = 0; p.backscatter_underbound = 1; p.dt = dt
    return p


REMAP_PCM, REMAP_PLM, REMAP_PPM_H4, REMAP_PPM_IH4 = 0, 2, 4, 5   # enum mom6x_remap_scheme


class RemappingParams(C.Structure):
    """mom6x_remapping_params; remapping_CS (MOM_remapping.F90:47-84)."""
    _fields_ = [("scheme", C.c_int), ("boundary_extrapolation", C.c_int), ("force_bounds_in_subcell", C.c_int),
                ("force_bounds_in_target", C.c_int), ("om4_remap_via_sub_cells", C.c_int), ("answer_date", C.c_int),
                ("h_neglect", C.c_double), ("h_neglect_edge", C.c_double)]


def remapping_params_default(scheme=REMAP_PLM, h_neglect=1.0e-30, **kw):
    """initialize_remapping :1654 with the type's defaults (:47-84): boundary extrapolation on, target values bounded,
    sub-cell values not, the non-OM4 sub-cell integrator; h_neglect as in remapping_unit_tests (1e-30 H)."""
    p = RemappingParams()
    p.scheme = scheme; p.boundary_extrapolation = 1; p.force_bounds_in_subcell = 0; p.force_bounds_in_target = 1
    p.om4_remap_via_sub_cells = 0; p.answer_date = 99991231; p.h_neglect = h_neglect; p.h_neglect_edge = h_neglect
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class ChksumResult(C.Structure):
    """mom6x_chksum_result: the numbers of the two message lines of chksum_{h,u,v,B}_{2d,3d} (MOM_checksums.F90)."""
    _fields_ = [("mean", C.c_double), ("amin", C.c_double), ("amax", C.c_double), ("bc0", C.c_int), ("bc", C.c_int * 4),
                ("nbc", C.c_int), ("bc_kind", C.c_int)]


CHK_NONE, CHK_CORNERS, CHK_NSEW, CHK_W, CHK_S = range(5)    # enum mom6x_chksum_kind


class SumOutputParams(C.Structure):
    """mom6x_sum_output_params: the members of Sum_output_CS (MOM_sum_output.F90:60-140) the sums of write_energy read."""
    _fields_ = [("do_APE_calc", C.c_int), ("use_temperature", C.c_int), ("dt_in_T", C.c_double), ("D_list_min_inc", C.c_double),
                ("Z_ref", C.c_double), ("C_p", C.c_double)]


def sum_output_params_default(dt, **kw):
    """CALCULATE_APE = True, ENABLE_THERMODYNAMICS off unless asked, DEPTH_LIST_MIN_INC = 1e-10 m, C_P = 3991.86795711963."""
    p = SumOutputParams()
    p.do_APE_calc = 1; p.use_temperature = 0; p.dt_in_T = dt; p.D_list_min_inc = 1.0e-10; p.Z_ref = 0.0; p.C_p = 3991.86795711963
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class EnergySums(C.Structure):
    """mom6x_energy_sums."""
    _fields_ = [("mass_tot", C.c_double), ("KE_tot", C.c_double), ("PE_tot", C.c_double), ("max_CFL", C.c_double * 2),
                ("mass_EFP", C.c_int64 * 6), ("salt_EFP", C.c_int64 * 6), ("heat_EFP", C.c_int64 * 6)]


class RegridZstarParams(C.Structure):
    """mom6x_regrid_zstar_params; the members of regridding_CS (MOM_regridding.F90:40-140) the z* branch reads."""
    _fields_ = [("min_thickness", C.c_double), ("old_grid_weight", C.c_double), ("depth_of_time_filter_shallow", C.c_double),
                ("depth_of_time_filter_deep", C.c_double), ("Z_ref", C.c_double)]


def regrid_zstar_params_default(**kw):
    """MIN_THICKNESS = 0.001 m, no time filtering (REGRID_TIME_SCALE = 0), Z_ref = 0."""
    p = RegridZstarParams()
    p.min_thickness = 1.0e-3; p.old_grid_weight = 0.0; p.depth_of_time_filter_shallow = 0.0; p.depth_of_time_filter_deep = 0.0
    p.Z_ref = 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


INTERP_P1M_H2, INTERP_PLM, INTERP_PPM_H4 = 0, 3, 5   # enum mom6x_interp_scheme
INTERP_P1M_H4 = 1                                      # (restated in the oracle only)


class RegridRhoParams(C.Structure):
    """mom6x_regrid_rho_params: what REGRIDDING_RHO / REGRIDDING_HYCOM1 read of regridding_CS on top of the z* members."""
    _fields_ = [("f", RegridZstarParams), ("interp_scheme", C.c_int), ("boundary_extrapolation", C.c_int), ("ref_pressure", C.c_double),
                ("compressibility_fraction", C.c_double), ("integrate_downward_for_e", C.c_int)]


def regrid_rho_params_default(**kw):
    """INTERPOLATION_SCHEME = P1M_H2, BOUNDARY_EXTRAPOLATION = F, P_REF = 2e7 Pa, no compressibility, heights integrated
    downward from the surface (MOM_regridding.F90:90, :106, :118, :210-240)."""
    p = RegridRhoParams()
    p.f = regrid_zstar_params_default()
    p.interp_scheme = INTERP_P1M_H2; p.boundary_extrapolation = 0; p.ref_pressure = 2.0e7; p.compressibility_fraction = 0.0
    p.integrate_downward_for_e = 1
    for k, v in kw.items():
        if hasattr(p.f, k):
            setattr(p.f, k, v)
        else:
            setattr(p, k, v)
    return p


LINEAR, WRIGHT, WRIGHT_FULL, WRIGHT_REDUCED, UNESCO, ROQUET_RHO, JACKETT06, ROQUET_SPV = 1, 2, 3, 4, 5, 6, 7, 8   # enum mom6x_eos_form


class EOSParams(C.Structure):
    """mom6x_eos_params: tv%eqn_of_state + the EOS-only switches of PressureForce_FV_CS."""
    _fields_ = [("form", C.c_int), ("Rho_T0_S0", C.c_double), ("dRho_dT", C.c_double), ("dRho_dS", C.c_double),
                ("dRho_dp", C.c_double), ("MassWghtInterp", C.c_int), ("use_SSH_in_Z0p", C.c_int),
                ("Recon_Scheme", C.c_int), ("boundary_extrap", C.c_int), ("MassWghtInterpVanOnly", C.c_int), ("h_nonvanished", C.c_double),
                ("EOS_quadrature", C.c_int)]


def eos_params_default(form=WRIGHT):
    """EQN_OF_STATE (default WRIGHT), RHO_T0_S0 = 1000, DRHO_DT = -0.2, DRHO_DS = 0.8 (MOM_EOS.F90:1562-1600)."""
    p = EOSParams()
    p.form = form
    p.Rho_T0_S0 = 1000.0; p.dRho_dT = -0.2; p.dRho_dS = 0.8; p.dRho_dp = 0.0
    p.MassWghtInterp = 0; p.use_SSH_in_Z0p = 0
    p.Recon_Scheme = 0; p.boundary_extrap = 1; p.MassWghtInterpVanOnly = 0; p.h_nonvanished = 1.0e-6; p.EOS_quadrature = 0   # (Recon_Scheme: 1 with USE_REGRIDDING)
    return p


def pgf_params_default(Rho0=1035.0):
    p = PGFParams()
    p.rho_ref, p.rho_ref_bug, p.Z_ref = Rho0, 1, 0.0
    return p


def layer_densities(nk, Rho0=1035.0, g_Earth=9.80, drho=2.0):
    """GV%Rlay and GV%g_prime for a simple linear layer-density profile (COORD_CONFIG="linear",
    MOM_coord_initialization.F90:126-170): Rlay(k) = Rlay(1) + (k-1)*drho/(nk-1) style spacing and
    g_prime(k) = g*(Rlay(k)-Rlay(k-1))/Rho0, g_prime(1) = g (free surface)."""
    import numpy as np
    Rlay = Rho0 - 0.5 * drho + drho * (np.arange(nk) / max(nk - 1, 1))
    g_prime = np.empty(nk)
    g_prime[0] = g_Earth
    g_prime[1:] = (g_Earth / Rho0) * (Rlay[1:] - Rlay[:-1])
    return np.ascontiguousarray(Rlay), np.ascontiguousarray(g_prime)


class RK2Params(C.Structure):
    """mom6x_rk2_params; MOM_dyn_split_RK2_CS (MOM_dynamics_split_RK2.F90:85-273)."""
    _fields_ = [("be", C.c_double), ("begw", C.c_double), ("split_bottom_stress", C.c_int),
                ("BT_use_layer_fluxes", C.c_int), ("store_CAu", C.c_int), ("visc_rem_dt_bug", C.c_int), ("remap_aux", C.c_int),
                ("no_BT_cont", C.c_int)]


def rk2_params_default():
    """Defaults read in initialize_dyn_split_RK2 (MOM_dynamics_split_RK2.F90:1427-1495)."""
    p = RK2Params()
    p.be, p.begw = 0.6, 0.0
    p.split_bottom_stress = 0
    p.BT_use_layer_fluxes = p.store_CAu = p.visc_rem_dt_bug = 1
    p.remap_aux = 0
    p.no_BT_cont = 0                                                   # USE_BT_CONT_TYPE = True
    return p


VERTVISC_COEF_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double)
HOR_VISC_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p)


class RK2Hooks(C.Structure):
    """mom6x_rk2_hooks."""
    _fields_ = [("user", C.c_void_p), ("vertvisc_coef", VERTVISC_COEF_HOOK), ("horizontal_viscosity", HOR_VISC_HOOK)]


RK2_FIELDS = ["CAu", "CAv", "CAu_pred", "CAv_pred", "PFu", "PFv", "diffu", "diffv", "visc_rem_u", "visc_rem_v",
              "u_accel_bt", "v_accel_bt", "u_av", "v_av", "h_av", "pbce", "eta", "eta_PF", "uhbt", "vhbt",
              "taux_bot", "tauy_bot", "BT_h_u", "BT_h_v"]
# mom6x_dyn_split_RK2_restart_fills: the restart variables the caller has uploaded (include/mom6x.h MOM6X_RK2_HAVE_*)
RK2_HAVE_ETA, RK2_HAVE_DIFFU, RK2_HAVE_U2, RK2_HAVE_CAU, RK2_HAVE_UH, RK2_HAVE_H2 = 1, 2, 4, 8, 16, 32
RK2_FIELDS_2D = {"eta", "eta_PF", "uhbt", "vhbt", "taux_bot", "tauy_bot"}


# Metric plane indices: enum mom6x_metric
METRICS = [
    "mask2dT", "mask2dCu", "mask2dCv", "mask2dBu",
    "dxT", "dyT", "IdxT", "IdyT",
    "dxCu", "dyCu", "IdxCu", "IdyCu",
    "dxCv", "dyCv", "IdxCv", "IdyCv",
    "dxBu", "dyBu", "IdxBu", "IdyBu",
    "areaT", "IareaT", "areaBu", "IareaBu",
    "areaCu", "areaCv", "IareaCu", "IareaCv",
    "dy_Cu", "dx_Cv", "bathyT", "CoriolisBu", "Coriolis2Bu",
]
G = {n: i for i, n in enumerate(METRICS)}
G_COUNT = len(METRICS)

MOM6X_OK = 0

_lib = None


ABI_VERSION = 6   # include/mom6x.h MOM6X_ABI_VERSION


def load_library(path=None):
    """Load the HIP C-ABI shared library.  Raises (never falls back) if it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"mom6_amd: HIP extension {p} is missing; run `python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no CPU fallback for the product path.")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    if lib.mom6x_abi_version() != ABI_VERSION:
        raise RuntimeError(f"mom6_amd: {p} has ABI version {lib.mom6x_abi_version()}, this host mirror was written for "
                           f"{ABI_VERSION} (include/mom6x.h MOM6X_ABI_VERSION); rebuild the library")
    lib.mom6x_last_error.restype = C.c_char_p
    lib.mom6x_ctx_stream.restype = C.c_void_p
    lib.mom6x_ctx_dims.restype = C.POINTER(Dims)
    lib.mom6x_ctx_metrics_dev.restype = C.c_void_p
    for name in ("mom6x_barotropic_field", "mom6x_rk2_field"):
        if hasattr(lib, name):
            getattr(lib, name).restype = C.c_void_p
    if hasattr(lib, "mom6x_step_forward_MEKE"):   # (39 arguments: the types are stated, not inferred from what a call happens to pass)
        vp = C.c_void_p
        lib.mom6x_MEKE_init.argtypes = [vp, C.POINTER(MEKEParams), vp, vp]
        lib.mom6x_MEKE_set_initialized.argtypes = [vp, C.c_int]
        lib.mom6x_step_forward_MEKE.argtypes = [vp] * 9 + [C.c_double] + [vp] * 29
    if hasattr(lib, "mom6x_set_diffusivity"):     # (28 arguments, stated like the MEKE step's)
        vp = C.c_void_p
        lib.mom6x_set_diffusivity_init.argtypes = [vp, C.POINTER(SetDiffusivityParams), C.POINTER(EOSParams), vp, vp]
        lib.mom6x_set_diffusivity_field.argtypes = [vp, C.c_int]
        lib.mom6x_set_diffusivity_field.restype = vp
        lib.mom6x_set_BBL_TKE.argtypes = [vp] * 11
        lib.mom6x_set_diffusivity.argtypes = [vp] * 15 + [C.c_double] + [vp] * 12
    if hasattr(lib, "mom6x_applyBoundaryFluxesInOut"):     # (21 arguments, stated like the MEKE step's)
        vp = C.c_void_p
        lib.mom6x_diabatic_aux_init.argtypes = [vp, C.POINTER(DiabaticAuxParams), C.POINTER(EOSParams)]
        lib.mom6x_applyBoundaryFluxesInOut.argtypes = ([vp, C.c_double, C.POINTER(SurfaceFluxes), C.c_int] + [vp] * 6 +
                                                       [C.c_int, C.c_double, C.c_double] + [vp] * 8)
        lib.mom6x_diabatic_aux_status.argtypes = [vp] + [C.POINTER(C.c_long)] * 3
    if hasattr(lib, "mom6x_energetic_PBL"):       # (26 arguments, stated like the MEKE step's)
        vp = C.c_void_p
        lib.mom6x_energetic_PBL_init.argtypes = [vp, C.POINTER(EnergeticPBLParams)]
        lib.mom6x_energetic_PBL.argtypes = [vp] * 11 + [C.c_double] + [vp] * 14
        lib.mom6x_energetic_PBL_get_MLD.argtypes = [vp, vp, vp, C.c_double]
        lib.mom6x_ePBL_augment_Kd.argtypes = [vp] * 6 + [C.c_int, C.c_double, vp, vp]
    if hasattr(lib, "mom6x_make_frazil"):
        vp = C.c_void_p
        lib.mom6x_make_frazil_init.argtypes = [vp, C.POINTER(FrazilParams)]
        lib.mom6x_make_frazil.argtypes = [vp] * 6 + [C.c_int]
        lib.mom6x_adjust_salt.argtypes = [vp] * 4 + [C.c_double]
        lib.mom6x_geothermal_init.argtypes = [vp, C.POINTER(GeothermalParams), vp, C.POINTER(EOSParams)]
        lib.mom6x_geothermal_in_place.argtypes = [vp] * 4 + [C.c_double] + [vp] * 4 + [C.c_int]
    if hasattr(lib, "mom6x_set_pen_shortwave"):
        vp = C.c_void_p
        lib.mom6x_opacity_init.argtypes = [vp, C.POINTER(OpacityParams)]
        lib.mom6x_set_pen_shortwave.argtypes = [vp] * 8 + [C.c_double] + [vp] * 5
        lib.mom6x_opacity_status.argtypes = [vp, C.POINTER(C.c_long)]
    if hasattr(lib, "mom6x_Calculate_kappa_shear"):
        vp = C.c_void_p
        lib.mom6x_kappa_shear_init.argtypes = [vp, C.POINTER(KappaShearParams), C.POINTER(EOSParams), vp]
        lib.mom6x_kappa_shear_work_bytes.argtypes = [vp]
        lib.mom6x_kappa_shear_work_bytes.restype = C.c_longlong
        lib.mom6x_Calculate_kappa_shear.argtypes = [vp] * 7 + [C.c_double, C.c_int] + [vp] * 8
    if hasattr(lib, "mom6x_neutral_diffusion"):
        vp = C.c_void_p
        lib.mom6x_neutral_diffusion_init.argtypes = [vp, C.POINTER(NeutralDiffusionParams), C.POINTER(EOSParams)]
        lib.mom6x_neutral_diffusion_work_bytes.argtypes = [vp]
        lib.mom6x_neutral_diffusion_work_bytes.restype = C.c_longlong
        lib.mom6x_neutral_diffusion_calc_coeffs.argtypes = [vp] * 5
        lib.mom6x_neutral_diffusion.argtypes = [vp] * 4 + [C.c_double, vp, vp, C.c_int, vp, vp, vp]
        lib.mom6x_neutral_diffusion_coeffs.argtypes = [vp, C.c_int] + [C.POINTER(vp)] * 5
        lib.mom6x_neutral_diffusion_status.argtypes = [vp, C.POINTER(C.c_longlong)]
        lib.mom6x_neutral_diffusion_tile.argtypes = [C.POINTER(C.c_int)] * 3
        lib.mom6x_tracer_hordiff_neutral.argtypes = ([vp, vp, C.c_double, vp, vp, C.c_int] + [vp] * 7 + [vp] * 3 + [vp] * 3 + [vp] * 3 +
                                                     [C.POINTER(C.c_int)])
    if path is None:
        _lib = lib
    return lib


class Mom6xError(RuntimeError):
    pass


def check(lib, rc):
    if rc != MOM6X_OK:
        msg = lib.mom6x_last_error()
        raise Mom6xError(f"mom6x error {rc}: {msg.decode() if msg else ''}")


def lane_launch_shape(lib=None):
    """(lanes along i, rows, i of the first lane) of the work-groups of the one-lane-per-face kernels: mom6x_lane_launch_shape.
    Needs the library, not a GPU."""
    lib = lib or load_library()
    bx, by, i0 = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib, lib.mom6x_lane_launch_shape(C.byref(bx), C.byref(by), C.byref(i0)))
    return bx.value, by.value, i0.value


TILE_CORAD, TILE_HOR_VISC, TILE_TRACER_ADVECT = 0, 1, 2


def tile_steps(which, lib=None):
    """(points along i, points along j) by which the tiles of CorAdCalc's (TILE_CORAD) and horizontal_viscosity's (TILE_HOR_VISC)
    fused kernels advance, or the cells of an x tile and the rows of a y segment of advect_tracer (TILE_TRACER_ADVECT):
    mom6x_tile_steps.  Needs the library, not a GPU."""
    lib = lib or load_library()
    sx, sy = C.c_int(0), C.c_int(0)
    check(lib, lib.mom6x_tile_steps(int(which), C.byref(sx), C.byref(sy)))
    return sx.value, sy.value
