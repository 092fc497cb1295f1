"""The loader of oracle/_ref/libref_param.so -- the reference's own MOM_EOS_Wright*.F90, MOM_EOS_linear.F90,
MOM_intrinsic_functions.F90, MOM_opacity.F90, MOM_energetic_PBL.F90, MOM_kappa_shear.F90, MOM_neutral_diffusion.F90,
MOM_isopycnal_slopes.F90, MOM_lateral_mixing_coeffs.F90 and MOM_thickness_diffuse.F90 (with MOM_EOS.F90 and
MOM_interface_heights.F90) compiled where they
lie against the interface stand-ins of oracle/ref_standins.F90, behind the bind(C) doors of oracle/ref_param_shim.F90 -- and the
one place where the members of abi.OpacityParams, abi.EnergeticPBLParams, abi.KappaShearParams, abi.NeutralDiffusionParams,
abi.VarMixParams and abi.ThicknessDiffuseParams are
mapped to the names the reference reads with get_param.  Of MOM_neutral_diffusion the door hands out the tracers, their content
tendencies and the two transports; the positions and effective thicknesses are private to the compiled module (see
neutral_diffusion below).  Test infrastructure:
tests/test_ref_parity_cpu.py holds the python restatements to these doors, scripts/record_ref_parity.py records their results for
the GPU tests.  The maps below are lists of names; nothing of the reference's text is here."""
import ctypes as C
import hashlib
import os

import numpy as np

from mom6_amd import abi

G = abi.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libref_param.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
_lib = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    """The library, or None where oracle/_ref is not built (it needs the reference's sources and amdflang: make -C oracle ref)."""
    global _lib
    if _lib is None and available():
        _lib = C.CDLL(LIB_PATH)
        _lib.ref_diag_size.restype = C.c_int
        for n in ("ref_opacity", "ref_energetic_PBL", "ref_absorbRemainingSW", "ref_sumSWoverBands", "ref_Calculate_kappa_shear",
                  "ref_neutral_diffusion", "ref_standin_never_count", "ref_calc_slope_functions", "ref_thickness_diffuse"):
            getattr(_lib, n).restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# equations of state and intrinsic functions

EOS_OUT = ("rho", "rho_anom", "spv", "drho_dT", "drho_dS", "dSV_dT", "dSV_dS", "rho_c", "drho_dp")
EOS_DOOR = {abi.WRIGHT: "ref_WRIGHT", abi.WRIGHT_FULL: "ref_WRIGHT_FULL", abi.WRIGHT_REDUCED: "ref_WRIGHT_REDUCED",
            abi.LINEAR: "ref_LINEAR"}


def eos_points(eos, T, S, p, rho_ref):
    """density_elem, density_anomaly_elem, spec_vol_elem, calculate_density_derivs_elem, calculate_specvol_derivs_elem and
    calculate_compress_elem of the reference at n points: a dict of arrays by the names of EOS_OUT."""
    T, S, p = _c(T), _c(S), _c(p)
    n = T.size
    out = {k: np.zeros(n) for k in EOS_OUT}
    args = [C.c_int(n), _p(T), _p(S), _p(p), C.c_double(rho_ref)]
    if eos.form == abi.LINEAR:
        coef = np.array([eos.Rho_T0_S0, eos.dRho_dT, eos.dRho_dS, eos.dRho_dp])
        args.append(_p(coef))
    getattr(lib(), EOS_DOOR[eos.form])(*args, *[_p(out[k]) for k in EOS_OUT])
    return out


def cuberoot(x):
    x = _c(x); y = np.zeros_like(x)
    lib().ref_cuberoot(C.c_int(x.size), _p(x), _p(y))
    return y


def invcosh(x):
    x = _c(x); y = np.zeros_like(x)
    lib().ref_invcosh(C.c_int(x.size), _p(x), _p(y))
    return y


# ------------------------------------------------------------------------------------------------------------------------------
# the parameter table

def _table(entries, powers=None):
    """Fills the stand-in's name -> value table: entries are (NAME, value) with a float, an int or bool, a str or a sequence of
    floats; powers are the *_RESCALE_POWER entries of the reference's own unit_scaling_init."""
    L = lib()
    L.ref_param_clear()
    for name, v in list(entries) + [(k + "_RESCALE_POWER", int(e)) for k, e in (powers or {}).items()]:
        b = name.encode()
        if isinstance(v, str):
            L.ref_set_char(b, v.encode())
        elif isinstance(v, (bool, int, np.integer)):
            L.ref_set_int(b, C.c_int(int(v)))
        elif isinstance(v, float):
            L.ref_set_real(b, C.c_double(v))
        else:
            a = np.array(list(v), dtype=np.float64)
            L.ref_set_reals(b, C.c_int(a.size), _p(a))


def _power_of_two(x, what):
    e = int(round(np.log2(x)))
    assert 2.0 ** e == x, (what, x)
    return e


def vgrid_values(GV, m_to_Z=1.0):
    """The members of verticalGrid_type that the compiled files read, from abi.VGrid (whose g_Earth is g_Earth_Z_T2 and whose
    Angstrom_Z is H_to_Z * Angstrom_H), in the order of oracle/ref_param_shim.F90."""
    H_to_m = GV.H_to_Z / m_to_Z
    return np.array([GV.Rho0, GV.g_Earth, GV.Angstrom_H, GV.H_to_Z * GV.Angstrom_H, GV.H_subroundoff, GV.dZ_subroundoff, GV.H_to_Z,
                     GV.Z_to_H, GV.H_to_RZ, GV.RZ_to_H, H_to_m, 1.0 / H_to_m, H_to_m, 1.0])


def _tile(d):
    nj_mem, ni_mem = d.shape2()
    idx = (C.c_int * 4)(d.ioff + 1, d.ioff + d.ni, d.joff + 1, d.joff + d.nj)
    return ni_mem, nj_mem, idx


def _diag(name, shape):
    """What post_data last copied for a name the door was asked for, as an array of `shape` (whole planes, halo included)."""
    L = lib()
    n = L.ref_diag_size(name.encode())
    assert n == int(np.prod(shape)), (name, n, shape)
    out = np.zeros(shape)
    L.ref_get_diag(name.encode(), C.c_int(out.size), _p(out))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_opacity

OPACITY_SCHEME_NAMES = {abi.OPACITY_MANIZZA_05: "MANIZZA_05", abi.OPACITY_MOREL_88: "MOREL_88", abi.OPACITY_OHLMANN_03: "OHLMANN_03",
                        abi.OPACITY_SINGLE_EXP: "SINGLE_EXP", abi.OPACITY_DOUBLE_EXP: "DOUBLE_EXP"}
OPACITY_CHL_SCHEMES = (abi.OPACITY_MANIZZA_05, abi.OPACITY_MOREL_88, abi.OPACITY_OHLMANN_03)
# member of abi.OpacityParams -> (the name opacity_init reads, the unit of the member: "Z" a length, "Z-1" an inverse length)
OPACITY_PARAM_NAMES = {
    "pen_sw_scale": ("PEN_SW_SCALE", "Z"), "pen_sw_scale_2nd": ("PEN_SW_SCALE_2ND", "Z"), "sw_1st_exp_ratio": ("SW_1ST_EXP_RATIO", ""),
    "pen_sw_frac": ("PEN_SW_FRAC", ""), "blue_frac": ("BLUE_FRAC_SW", ""), "opacity_land_value": ("OPACITY_LAND_VALUE", "Z-1"),
    "manizza_coef": ("OPACITY_VALUES_MANIZZA", "Z-1"), "manizza_power": ("CHOROPHYLL_POWER_MANIZZA", ""),
    "morel_coef": ("OPACITY_VALUES_MOREL", "Z"), "morel_pen_coef": ("SW_PEN_FRAC_COEFS_MOREL", ""),
    "nbands": ("PEN_SW_NBANDS", ""),
}
# opacity_scheme maps to VAR_PEN_SW with OPACITY_SCHEME or EXP_OPACITY_SCHEME; Z_to_m and m_to_Z to Z_RESCALE_POWER.
OPACITY_DIAG_NAMES = {"SW_pen": "SW_pen", "SW_vis_pen": "SW_vis_pen", "opac_diag": "opac_%d"}


def opacity_table(P):
    """The parameter table of a case: members in the model's units go back to the MKS values a parameter file holds."""
    to_mks = {"": 1.0, "Z": P.Z_to_m, "Z-1": P.m_to_Z}
    ent = []
    chl = P.opacity_scheme in OPACITY_CHL_SCHEMES
    ent.append(("VAR_PEN_SW", chl))
    ent.append(("OPACITY_SCHEME" if chl else "EXP_OPACITY_SCHEME", OPACITY_SCHEME_NAMES[P.opacity_scheme]))
    for member, (name, unit) in OPACITY_PARAM_NAMES.items():
        v = getattr(P, member)
        if member == "nbands":
            ent.append((name, int(v)))
        elif hasattr(v, "__len__"):
            ent.append((name, [float(x) * to_mks[unit] for x in v]))
        else:
            ent.append((name, float(v) * to_mks[unit]))
    assert P.Z_to_m * P.m_to_Z == 1.0
    return ent, dict(Z=_power_of_two(P.Z_to_m, "Z_to_m"))


def opacity(d, M, GV, P, opt, inp):
    """opacity_init through the table, then set_opacity on whole arrays, with the arguments of a case of tests/opacity_ref.py.
    Returns the outputs by the names of opacity_ref.outputs (opacity_band times opt["scale"], the one product of
    extract_optics_slice; planes beyond the computational domain are whatever the reference left) and the FATAL count."""
    L = lib()
    ent, powers = opacity_table(P)
    _table(ent, powers)
    nb = max(P.nbands, 1)
    for n in opt["diag"]:
        if n == "opac_diag":
            for b in range(nb):
                L.ref_want_diag((OPACITY_DIAG_NAMES[n] % (b + 1)).encode())
        else:
            L.ref_want_diag(OPACITY_DIAG_NAMES[n].encode())
    ni_mem, nj_mem, idx = _tile(d)
    mask = _c(M[G["mask2dT"]])
    planes = [_c(inp[n]) if n in opt["given"] else None for n in ("sw", "sw_vis_dir", "sw_vis_dif", "sw_nir_dir", "sw_nir_dif")]
    c2 = _c(inp["chl_2d"]) if opt["chl"] == "2d" else None
    c3 = _c(inp["chl_3d"]) if opt["chl"] == "3d" else None
    gv = vgrid_values(GV, P.m_to_Z)
    ob = np.full((nb,) + d.shape3(), np.nan); pen = np.full((nb,) + d.shape2(), np.nan)
    nbo = C.c_int(-1)
    fatal = L.ref_opacity(C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(mask), *[_p(a) for a in planes], _p(c2), _p(c3),
                          C.c_int(nb), C.byref(nbo), _p(ob), _p(pen))
    if fatal:
        return None, fatal
    assert nbo.value == P.nbands, (nbo.value, P.nbands)
    out = dict(opacity_band=opt["scale"] * ob, sw_pen_band=pen)
    for n in opt["diag"]:
        if n == "opac_diag":
            out[n] = np.stack([_diag(OPACITY_DIAG_NAMES[n] % (b + 1), d.shape3()) for b in range(nb)])
        else:
            out[n] = _diag(OPACITY_DIAG_NAMES[n], d.shape2())
    return out, fatal


def absorbRemainingSW(GV, P, h, opacity_band, nsw, dt, H_limit_fluxes, T, Pen_SW_bnd, TKE=None, dSV_dT=None):
    """absorbRemainingSW of the reference on one j-row, with the arguments of tests/bflux_ref.py's (h, T, TKE, dSV_dT [nk, ni];
    opacity_band [n, nk, ni]; Pen_SW_bnd [n, ni]) and adjustAbsorptionProfile false, absorbAllSW true as applyBoundaryFluxesInOut
    calls it (MOM_diabatic_aux.F90:1224-1225); T, Pen_SW_bnd and TKE are changed in place.  Returns the FATAL count."""
    nk, ni = h.shape
    nm = max(nsw, 1)
    ob = np.ascontiguousarray(np.moveaxis(np.asarray(opacity_band, dtype=np.float64)[:nm], 0, -1))          # [nk, ni, n]
    pen = np.ascontiguousarray(np.moveaxis(np.asarray(Pen_SW_bnd, dtype=np.float64)[:nm], 0, -1))           # [ni, n]
    hh, TT = _c(h), _c(T)
    tke, dsv = (_c(TKE), _c(dSV_dT)) if TKE is not None and dSV_dT is not None else (None, None)
    gv = vgrid_values(GV)
    fatal = lib().ref_absorbRemainingSW(C.c_int(ni), C.c_int(nk), _p(gv), C.c_int(nsw), C.c_int(P.optics_answer_date),
                                        C.c_double(P.PenSW_flux_absorb), C.c_double(P.PenSW_absorb_Invlen), _p(hh), _p(ob), C.c_double(dt),
                                        C.c_double(H_limit_fluxes), C.c_int(0), C.c_int(1), _p(TT), _p(pen), _p(tke), _p(dsv))
    T[...] = TT
    Pen_SW_bnd[:nm] = np.moveaxis(pen, -1, 0)
    if tke is not None:
        TKE[...] = tke
    return fatal


def sumSWoverBands(GV, P, h, dz, opacity_band, nsw, dt, H_limit_fluxes, iPen_SW_bnd, absorbAllSW=True):
    """sumSWoverBands of the reference on one j-row (h, dz [nk, ni]; opacity_band [n, nk, ni]; iPen_SW_bnd [n, ni]): netPen
    [nk + 1, ni] and the FATAL count.  The project has no restatement of it (it has no device side); the door is kept for one."""
    nk, ni = h.shape
    nm = max(nsw, 1)
    ob = np.ascontiguousarray(np.moveaxis(np.asarray(opacity_band, dtype=np.float64)[:nm], 0, -1))
    pen = np.ascontiguousarray(np.moveaxis(np.asarray(iPen_SW_bnd, dtype=np.float64)[:nm], 0, -1))
    hh, zz = _c(h), _c(dz)
    net = np.zeros((nk + 1, ni))
    gv = vgrid_values(GV)
    fatal = lib().ref_sumSWoverBands(C.c_int(ni), C.c_int(nk), _p(gv), C.c_int(nsw), C.c_int(P.optics_answer_date),
                                     C.c_double(P.PenSW_flux_absorb), C.c_double(P.PenSW_absorb_Invlen), _p(hh), _p(zz), _p(ob),
                                     C.c_double(dt), C.c_double(H_limit_fluxes), C.c_int(int(absorbAllSW)), _p(pen), _p(net))
    return net, fatal


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_energetic_PBL

EPBL_MSTAR_NAMES = {abi.EPBL_MSTAR_CONSTANT: "CONSTANT", abi.EPBL_MSTAR_OM4: "OM4", abi.EPBL_MSTAR_REICHL_H18: "REICHL_H18"}
EPBL_WT_NAMES = {abi.EPBL_WT_CUBE_ROOT_TKE: "CUBE_ROOT_TKE", abi.EPBL_WT_REICHL_H18: "REICHL_H18"}
# member of abi.EnergeticPBLParams -> (the name energetic_PBL_init reads, kind, the unit of the member)
EPBL_PARAM_NAMES = {
    "omega": ("OMEGA", "real", "T-1"), "omega_frac": ("ML_OMEGA_FRAC", "real", ""), "Ekman_scale_coef": ("EKMAN_SCALE_COEF", "real", ""),
    "vonKar": ("VON_KARMAN_CONST", "real", ""), "MKE_to_TKE_effic": ("MKE_TO_TKE_EFFIC", "real", ""), "TKE_decay": ("TKE_DECAY", "real", ""),
    "fixed_mstar": ("MSTAR", "real", ""), "mstar_cap": ("MSTAR_CAP", "real", ""), "mstar_coef": ("MSTAR2_COEF1", "real", ""),
    "C_Ek": ("MSTAR2_COEF2", "real", ""), "RH18_mstar_cn1": ("RH18_MSTAR_CN1", "real", ""), "RH18_mstar_cn2": ("RH18_MSTAR_CN2", "real", ""),
    "RH18_mstar_cn3": ("RH18_MSTAR_CN3", "real", ""), "RH18_mstar_cs1": ("RH18_MSTAR_CS1", "real", ""),
    "RH18_mstar_cs2": ("RH18_MSTAR_CS2", "real", ""), "nstar": ("NSTAR", "real", ""), "mstar_convect_coef": ("MSTAR_CONV_ADJ", "real", ""),
    "transLay_scale": ("EPBL_TRANSITION_SCALE", "real", ""), "MLD_tol": ("EPBL_MLD_TOLERANCE", "real", "Z"),
    "min_mix_len": ("EPBL_MIN_MIX_LEN", "real", "Z"), "MixLenExponent": ("MIX_LEN_EXPONENT", "real", ""),
    "wstar_ustar_coef": ("WSTAR_USTAR_COEF", "real", ""), "vstar_scale_fac": ("EPBL_VEL_SCALE_FACTOR", "real", ""),
    "vstar_surf_fac": ("VSTAR_SURF_FAC", "real", ""),
    "answer_date": ("EPBL_ANSWER_DATE", "int", ""), "orig_PE_calc": ("EPBL_ORIGINAL_PE_CALC", "bool", ""),
    "mstar_scheme": ("EPBL_MSTAR_SCHEME", EPBL_MSTAR_NAMES, ""), "Use_MLD_iteration": ("USE_MLD_ITERATION", "bool", ""),
    "MLD_iteration_guess": ("MLD_ITERATION_GUESS", "bool", ""), "MLD_bisection": ("EPBL_MLD_BISECTION", "bool", ""),
    "MLD_iter_bug": ("EPBL_MLD_ITER_BUG", "bool", ""), "max_MLD_its": ("EPBL_MLD_MAX_ITS", "int", ""),
    "wT_scheme": ("EPBL_VEL_SCALE_SCHEME", EPBL_WT_NAMES, ""),
}
# Not parameters: ustar_min (derived from OMEGA and GV, :4328), g_Earth_Z_T2 (GV), m_to_Z and T_to_s (the *_RESCALE_POWERs),
# TKE_diagnostics (true where a TKE diagnostic is registered, :4418), has_eos (tv%eqn_of_state is associated), and the members of
# abi.ENERGETIC_PBL_MUST_BE_0, which stay at the reference's defaults (off).
EPBL_DIAG_NAMES = {"Velocity_Scale": "Velocity_Scale", "Mixing_Length": "Mixing_Length", "mstar_sfc": "MSTAR", "ustar_diag": "ePBL_ustar",
                   "diag_TKE_wind": "ePBL_TKE_wind", "diag_TKE_MKE": "ePBL_TKE_MKE", "diag_TKE_conv": "ePBL_TKE_conv",
                   "diag_TKE_forcing": "ePBL_TKE_forcing", "diag_TKE_mixing": "ePBL_TKE_mixing",
                   "diag_TKE_mech_decay": "ePBL_TKE_mech_decay", "diag_TKE_conv_decay": "ePBL_TKE_conv_decay"}
EPBL_NOT_EXPOSED = ("OBL_its",)      # eCD%OBL_its reaches no diagnostic of the reference (only the report_avg_its printout)
EPBL_WET_ONLY = ("mstar_sfc", "ustar_diag")   # diag_mstar_sfc and diag_ustar are set at wet points only (:645, :767): land is not defined


def epbl_table(P):
    to_mks = {"": 1.0, "Z": 1.0 / P.m_to_Z, "T-1": 1.0 / P.T_to_s}
    ent = []
    for member, (name, kind, unit) in EPBL_PARAM_NAMES.items():
        v = getattr(P, member)
        if kind == "real":
            ent.append((name, float(v) * to_mks[unit]))
        elif kind == "int":
            ent.append((name, int(v)))
        elif kind == "bool":
            ent.append((name, bool(v)))
        else:
            ent.append((name, kind[int(v)]))
    for n in abi.ENERGETIC_PBL_MUST_BE_0:
        assert getattr(P, n) == 0, n
    return ent, dict(Z=_power_of_two(1.0 / P.m_to_Z, "Z_to_m"), T=_power_of_two(P.T_to_s, "T_to_s"))


def uv_at_h(d, M, u, v):
    """The velocities at thickness points that energetic_PBL is handed (the no-mixing arm of find_uv_at_h,
    MOM_diabatic_aux.F90:546-571, :606-611, which is not part of the compiled files): the weights of tests/epbl_ref.py."""
    aCu = M[G["areaCu"]]; aCv = M[G["areaCv"]]; IaT = M[G["IareaT"]]
    uh, vh = np.zeros_like(u), np.zeros_like(v)
    with np.errstate(all="ignore"):
        su = aCu[:, :-1] + aCu[:, 1:]
        Iu = np.where(su > 0.0, np.sqrt(0.5 * IaT[:, 1:] / np.where(su > 0.0, su, 1.0)), 0.0)
        a_w, a_e = aCu[:, :-1] * Iu, aCu[:, 1:] * Iu
        uh[:, :, 1:] = (a_e * u[:, :, 1:]) + (a_w * u[:, :, :-1])
        sv = aCv[:-1, :] + aCv[1:, :]
        Iv = np.where(sv > 0.0, np.sqrt(0.5 * IaT[1:, :] / np.where(sv > 0.0, sv, 1.0)), 0.0)
        a_s, a_n = aCv[:-1, :] * Iv, aCv[1:, :] * Iv
        vh[:, 1:, :] = (a_n * v[:, 1:, :]) + (a_s * v[:, :-1, :])
    return uh, vh


def energetic_PBL(d, M, GV, P, opt, inp, ncalls=None):
    """energetic_PBL_init through the table, energetic_PBL `ncalls` times on the same control structure and
    energetic_PBL_get_MLD, with the arguments of a case of tests/epbl_ref.py.  Returns the outputs by the names of
    epbl_ref.outputs, without those of EPBL_NOT_EXPOSED, and the FATAL count."""
    L = lib()
    ent, powers = epbl_table(P)
    _table(ent, powers)
    for n in opt["diag"]:
        if n in EPBL_DIAG_NAMES:
            L.ref_want_diag(EPBL_DIAG_NAMES[n].encode())
    assert bool(P.TKE_diagnostics) == any(n.startswith("diag_TKE_") for n in opt["diag"]), "TKE_diagnostics follows the registered ids"
    ni_mem, nj_mem, idx = _tile(d)
    mask = _c(M[G["mask2dT"]]); cor = _c(M[G["CoriolisBu"]])
    if P.MKE_to_TKE_effic > 0.0:
        uh, vh = uv_at_h(d, M, inp["u"], inp["v"])
    else:
        uh, vh = np.zeros(d.shape3()), np.zeros(d.shape3())
    a = {n: _c(inp[n]).copy() for n in ("h", "T", "S", "dSV_dT", "dSV_dS", "TKE_forced", "ustar", "buoy_flux")}
    gv = vgrid_values(GV, P.m_to_Z)
    Kd = np.full(d.shape3(d.nk + 1), np.nan); MLD = np.full(d.shape2(), np.nan)
    fatal = L.ref_energetic_PBL(C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(mask), _p(cor), _p(a["h"]), _p(uh), _p(vh),
                                _p(a["T"]), _p(a["S"]), _p(a["dSV_dT"]), _p(a["dSV_dS"]), _p(a["TKE_forced"]), _p(a["ustar"]),
                                _p(a["buoy_flux"]), C.c_double(opt["dt"]), C.c_int(ncalls or opt["ncalls"]), _p(Kd), _p(MLD))
    if fatal:
        return None, fatal
    for n in a:
        assert np.array_equal(a[n], inp[n], equal_nan=True), n + " is only read"
    out = dict(Kd_int=Kd, ML_depth=MLD)
    for n in opt["diag"]:
        if n in EPBL_DIAG_NAMES:
            out[n] = _diag(EPBL_DIAG_NAMES[n], d.shape3(d.nk + 1) if n in ("Velocity_Scale", "Mixing_Length") else d.shape2())
    return out, fatal


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_kappa_shear

# member of abi.KappaShearParams -> (the name kappa_shear_init reads (MOM_kappa_shear.F90:2114-2285), kind, the unit of the member)
KSHEAR_PARAM_NAMES = {
    "RiNo_crit": ("RINO_CRIT", "real", ""), "Shearmix_rate": ("SHEARMIX_RATE", "real", ""), "FRi_curvature": ("FRI_CURVATURE", "real", ""),
    "C_N": ("TKE_N_DECAY_CONST", "real", ""), "C_S": ("TKE_SHEAR_DECAY_CONST", "real", ""), "lambda": ("KAPPA_BUOY_SCALE_COEF", "real", ""),
    "lambda2_N_S": ("KAPPA_N_OVER_S_SCALE_COEF2", "real", ""), "lz_rescale": ("LZ_RESCALE", "real", ""),
    "TKE_bg": ("TKE_BACKGROUND", "real", "Z2 T-2"), "kappa_0": ("KD_KAPPA_SHEAR_0", "real", "H Z T-1"),
    "kappa_seed": ("KD_SEED_KAPPA_SHEAR", "real", "H Z T-1"), "kappa_trunc": ("KD_TRUNC_KAPPA_SHEAR", "real", "H Z T-1"),
    "kappa_tol_err": ("KAPPA_SHEAR_TOL_ERR", "real", ""), "Prandtl_turb": ("PRANDTL_TURB", "real", ""),
    "vel_underflow": ("VEL_UNDERFLOW", "real", "L T-1"), "kappa_src_max_chg": ("KAPPA_SHEAR_MAX_KAP_SRC_CHG", "real", ""),
    "max_RiNo_it": ("MAX_RINO_IT", "int", ""), "max_KS_it": ("MAX_KAPPA_SHEAR_IT", "int", ""),
    "eliminate_massless": ("KAPPA_SHEAR_ELIM_MASSLESS", "bool", ""), "dKdQ_iteration_bug": ("KAPPA_SHEAR_ITER_BUG", "bool", ""),
    "all_layer_TKE_bug": ("KAPPA_SHEAR_ALL_LAYER_TKE_BUG", "bool", ""),
    "restrictive_tolerance_check": ("USE_RESTRICTIVE_TOLERANCE_CHECK", "bool", ""), "KS_at_vertex": ("VERTEX_SHEAR", "bool", ""),
}
# Not parameters: nkml (GV%nkml with KAPPA_SHEAR_MERGE_ML, :2283-2289), m_to_Z, T_to_s, L_to_Z, RL2_T2_to_Pa and kg_m3_to_R (the
# *_RESCALE_POWERs), Z_to_m_m_to_H and g_Earth_Z_T2 (GV), work_columns (the device's workspace).  USE_JACKSON_PARAM is true.
KSHEAR_DIAG_NAMES = {"N2_init": "N2_shear_in", "S2_init": "S2_shear_in", "N2_mean": "N2_shear_mean", "S2_mean": "S2_shear_mean"}
KSHEAR_NOT_EXPOSED = ("KS_its",)     # the iteration count reaches no diagnostic of the reference
KSHEAR_EOS_NAMES = {abi.WRIGHT: "WRIGHT", abi.WRIGHT_FULL: "WRIGHT_FULL", abi.WRIGHT_REDUCED: "WRIGHT_REDUCED", abi.LINEAR: "LINEAR"}


def kshear_units(P):
    """The unit factors of a case from the members of abi.KappaShearParams: the powers of unit_scaling_init and the factors of GV."""
    Z_to_m = 1.0 / P.m_to_Z
    L_to_m = P.L_to_Z * Z_to_m
    R_to_kg_m3 = 1.0 / P.kg_m3_to_R
    m_to_H = P.Z_to_m_m_to_H * P.m_to_Z
    powers = dict(Z=_power_of_two(Z_to_m, "Z_to_m"), L=_power_of_two(L_to_m, "L_to_m"), T=_power_of_two(P.T_to_s, "T_to_s"),
                  R=_power_of_two(R_to_kg_m3, "R_to_kg_m3"))
    assert P.RL2_T2_to_Pa == R_to_kg_m3 * (L_to_m / P.T_to_s) ** 2, "RL2_T2_to_Pa is not what US derives"
    _power_of_two(m_to_H, "m_to_H")
    return powers, dict(m_to_H=m_to_H, m2_s_to_HZ_T=m_to_H * P.m_to_Z * P.T_to_s, Z2_T2=(P.m_to_Z * P.T_to_s) ** 2,
                        m_s_to_L_T=P.T_to_s / L_to_m)


def kshear_table(P, eos=None, merge_ml=True):
    """The parameter table of a case: members in the model's units go back to the MKS values a parameter file holds."""
    powers, f = kshear_units(P)
    to_mks = {"": 1.0, "Z2 T-2": 1.0 / f["Z2_T2"], "H Z T-1": 1.0 / f["m2_s_to_HZ_T"], "L T-1": 1.0 / f["m_s_to_L_T"]}
    ent = [("USE_JACKSON_PARAM", True), ("KAPPA_SHEAR_MERGE_ML", bool(merge_ml))]
    for member, (name, kind, unit) in KSHEAR_PARAM_NAMES.items():
        v = getattr(P, member)
        ent.append((name, float(v) * to_mks[unit] if kind == "real" else int(v) if kind == "int" else bool(v)))
    if eos is not None:
        ent.append(("EQN_OF_STATE", KSHEAR_EOS_NAMES[eos.form]))
        if eos.form == abi.LINEAR:
            ent += [("RHO_T0_S0", float(eos.Rho_T0_S0)), ("DRHO_DT", float(eos.dRho_dT)), ("DRHO_DS", float(eos.dRho_dS)),
                    ("DRHO_DP", float(eos.dRho_dp))]
    return ent, powers


def Calculate_kappa_shear(d, M, GV, P, opt, inp, eos=None, table_extra=()):
    """kappa_shear_init and EOS_init through the table, then Calculate_kappa_shear on the whole tile, with the arguments of a case
    of tests/kappa_shear_ref.py.  u_h and v_h are those kappa_shear_ref.find_uv_at_h makes of u and v (find_uv_at_h is not part of
    the compiled files).  Returns kappa_io, tke_io, kv_io and the four 3-D diagnostics by the names of kappa_shear_ref.outputs
    (planes beyond the computational domain are whatever the reference left) and the FATAL count."""
    from tests import kappa_shear_ref as K
    L = lib()
    layered = opt["eos"] is None
    eos = eos if eos is not None else K.case_eos(opt)
    ent, powers = kshear_table(P, None if layered else eos)
    _table(ent + list(table_extra), powers)          # (a later entry of a name replaces an earlier one)
    _, f = kshear_units(P)
    ni_mem, nj_mem, idx = _tile(d)
    H_to_m = 1.0 / f["m_to_H"]
    gv = np.array([GV.Rho0, P.g_Earth_Z_T2, GV.Angstrom_H, GV.H_to_Z * GV.Angstrom_H, GV.H_subroundoff, GV.dZ_subroundoff, GV.H_to_Z,
                   GV.Z_to_H, GV.H_to_RZ, GV.RZ_to_H, H_to_m, f["m_to_H"], H_to_m, 1.0 / f["m2_s_to_HZ_T"]])
    gx = np.array([GV.g_Earth, f["m2_s_to_HZ_T"], 1.0 / f["m2_s_to_HZ_T"], 1.0 / f["m2_s_to_HZ_T"]])
    with np.errstate(all="ignore"):
        u_h, v_h = K.find_uv_at_h(d, M, GV, inp["u"], inp["v"], inp["h"], opt["zero_mix"])
    mask = _c(M[G["mask2dT"]]); f2 = _c(M[G["Coriolis2Bu"]])
    a = {n: _c(inp[n]).copy() for n in ("h", "T", "S", "p_surf") if inp.get(n) is not None and not (layered and n in ("T", "S"))}
    Rlay = _c(inp["Rlay"]) if inp.get("Rlay") is not None else np.zeros(d.nk)
    out = {n: np.full(d.shape3(d.nk + 1), np.nan) for n in ("kappa_io", "tke_io", "kv_io")}
    fatal = L.ref_Calculate_kappa_shear(C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(gx), C.c_int(int(P.nkml)), _p(mask),
                                        _p(f2), _p(Rlay), _p(a["h"]), _p(_c(u_h)), _p(_c(v_h)), _p(a.get("T")), _p(a.get("S")),
                                        _p(a.get("p_surf")), C.c_double(opt["dt"]), _p(out["kappa_io"]), _p(out["tke_io"]),
                                        _p(out["kv_io"]))
    if fatal:
        return None, fatal
    if not opt["dt"] > 0.0:             # the door ran the two inits only
        return {}, fatal
    for n in a:
        assert np.array_equal(a[n], inp[n], equal_nan=True), n + " is only read"
    for n, name in KSHEAR_DIAG_NAMES.items():
        out[n] = _diag(name, d.shape3(d.nk + 1))
    return out, fatal


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_neutral_diffusion

# member of abi.NeutralDiffusionParams -> (the name neutral_diffusion_init reads (MOM_neutral_diffusion.F90:181-222), kind, the unit
# of the member)
NDIFF_PARAM_NAMES = {
    "continuous_reconstruction": ("NDIFF_CONTINUOUS", "bool", ""), "ref_pres": ("NDIFF_REF_PRES", "real", "R L2 T-2"),
    "interior_only": ("NDIFF_INTERIOR_ONLY", "bool", ""), "tapering": ("NDIFF_TAPERING", "bool", ""),
    "KhTh_use_vert_struct": ("KHTR_USE_EBT_STRUCT", "bool", ""),
    "use_unmasked_transport_bug": ("NDIFF_USE_UNMASKED_TRANSPORT_BUG", "bool", ""),
    "ndiff_answer_date": ("NDIFF_ANSWER_DATE", "int", ""),
}
# Not parameters of neutral_diffusion_init: recalc_neutral_surf (RECALC_NEUTRAL_SURF of tracer_hor_diff_init, which is not
# compiled: the door makes no use of it); RL2_T2_to_Pa, C_to_degC, S_to_ppt and kg_m3_to_R, the factors EOS_init takes from the
# unit_scale_type (MOM_EOS.F90:1721-1729), which come from the R, L, T, C and S *_RESCALE_POWERs.  USE_NEUTRAL_DIFFUSION is true.
NDIFF_NOT_PARAMS = ("recalc_neutral_surf", "RL2_T2_to_Pa", "C_to_degC", "S_to_ppt", "kg_m3_to_R")
# output of ndiff_ref.run / the device -> (the member of tracer_type whose id posts it, the stem of the name the door registers
# that id under for tracer m = 1 ..).  Read from MOM_neutral_diffusion.F90:949-1028: `tendency` is dTracer * IareaT * Idt, the
# tendency of the layer's tracer content, posted as id_dfxy_cont (:1006) before :1024-1028 divide it by h for id_dfxy_conc;
# trans_x_2d and trans_y_2d are the vertically summed transports of id_dfx_2d (:973) and id_dfy_2d (:1002).  The device has no
# output for id_dfxy_cont_2d or id_dfxy_conc, and the door leaves both ids at -1.
NDIFF_DIAG_NAMES = {"tendency": ("id_dfxy_cont", "dfxy_cont_%d"), "trans_x_2d": ("id_dfx_2d", "dfx_2d_%d"),
                    "trans_y_2d": ("id_dfy_2d", "dfy_2d_%d")}
# The components of neutral_diffusion_CS are private and id_uhEff_2d / id_vhEff_2d are registered nowhere in the reference: the
# ten coefficient arrays of ndiff_ref.COEFFS cannot be read out of the compiled module.  They are held through the tracers,
# tendencies and transports they produce.
NDIFF_NOT_EXPOSED = ("uPoL", "uPoR", "uKoL", "uKoR", "uhEff", "vPoL", "vPoR", "vKoL", "vKoR", "vhEff")
NDIFF_OUT = ("tracers", "tendency", "trans_x_2d", "trans_y_2d")
NDIFF_EOS_NAMES = KSHEAR_EOS_NAMES


def ndiff_units(P, powers=None):
    """The *_RESCALE_POWERs of a case.  The members of abi.NeutralDiffusionParams fix R, C and S and the ratio of L to T only
    (RL2_T2_to_Pa = R_to_kg_m3 (L_to_m / T_to_s)**2); `powers` names all of Z, L, T, R, C, S where a test rescales them, and is
    checked against the members."""
    if powers is None:
        powers = dict(R=_power_of_two(1.0 / P.kg_m3_to_R, "R_to_kg_m3"), C=_power_of_two(P.C_to_degC, "C_to_degC"),
                      S=_power_of_two(P.S_to_ppt, "S_to_ppt"))
    pw = dict(dict(Z=0, L=0, T=0, R=0, C=0, S=0), **powers)
    assert P.kg_m3_to_R == 2.0 ** -pw["R"] and P.C_to_degC == 2.0 ** pw["C"] and P.S_to_ppt == 2.0 ** pw["S"], "the factors of P are not US's"
    assert P.RL2_T2_to_Pa == 2.0 ** pw["R"] * (2.0 ** pw["L"] / 2.0 ** pw["T"]) ** 2, "RL2_T2_to_Pa is not what US derives"
    return pw


def ndiff_table(P, eos, powers=None):
    """The parameter table of a case: members in the model's units go back to the MKS values a parameter file holds."""
    pw = ndiff_units(P, powers)
    to_mks = {"": 1.0, "R L2 T-2": P.RL2_T2_to_Pa}
    ent = [("USE_NEUTRAL_DIFFUSION", True)]
    for member, (name, kind, unit) in NDIFF_PARAM_NAMES.items():
        v = getattr(P, member)
        ent.append((name, float(v) * to_mks[unit] if kind == "real" else int(v) if kind == "int" else bool(v)))
    assert set(NDIFF_PARAM_NAMES) | set(NDIFF_NOT_PARAMS) == {n for n, _ in abi.NeutralDiffusionParams._fields_}
    ent.append(("EQN_OF_STATE", NDIFF_EOS_NAMES[eos.form]))
    if eos.form == abi.LINEAR:
        ent += [("RHO_T0_S0", float(eos.Rho_T0_S0)), ("DRHO_DT", float(eos.dRho_dT)), ("DRHO_DS", float(eos.dRho_dS)),
                ("DRHO_DP", float(eos.dRho_dp))]
    return ent, pw


def neutral_diffusion(d, M, GV, P, opt, inp, ncalls=1, inp2=None, powers=None, dt=None, coef=None, table_extra=(), diag=NDIFF_OUT[1:]):
    """unit_scaling_init, EOS_init and neutral_diffusion_init through the table, then neutral_diffusion_calc_coeffs (with p_surf
    where the case has one) and neutral_diffusion over a registry of the case's tracers, with the arguments of a case of
    tests/ndiff_ref.py: plane 1 of ndiff_ref.coef_planes (or of `coef`), ndiff_ref.DT (or `dt`), the tracers' conc_underflow.
    ncalls = 2 runs calc_coeffs and neutral_diffusion once more on the same control structure, the coefficients from h, T, S
    (and p_surf) of `inp2` (default: of `inp` again), the tracers going on from the first round's.  dt <= 0: the inits only.
    Returns `tracers`, `tendency`, `trans_x_2d` and `trans_y_2d` by the names of ndiff_ref.run (lists of whole arrays; outside the
    ranges the reference's loops visit they hold whatever the reference left) and the FATAL count.  h, T, S and p_surf are
    asserted to have only been read.

    What the door cannot give: the components of neutral_diffusion_CS are private and id_uhEff_2d / id_vhEff_2d are never
    registered by the reference, so the positions (PoL, PoR, KoL, KoR) and hEff (NDIFF_NOT_EXPOSED) are not handed out; they are
    held through the tracers, tendencies and transports they produce."""
    from tests import ndiff_ref as R
    L = lib()
    ent, pw = ndiff_table(P, R.case_eos(opt), powers)
    _table(ent + list(table_extra), pw)
    dt = R.DT if dt is None else dt
    ntr = len(inp["tracers"])
    for n in diag:
        for m in range(ntr):
            L.ref_want_diag((NDIFF_DIAG_NAMES[n][1] % (m + 1)).encode())
    ni_mem, nj_mem, idx = _tile(d)
    gv = vgrid_values(GV)
    gx = np.array([GV.g_Earth, GV.g_Earth * GV.H_to_RZ])
    masks = np.ascontiguousarray(np.stack([M[G[n]] for n in ("mask2dT", "mask2dCu", "mask2dCv", "IareaT")]), dtype=np.float64)
    rounds = [inp] + [inp2 if inp2 is not None else inp] * (ncalls - 1)
    a = {n: np.ascontiguousarray(np.stack([r[n] for r in rounds]), dtype=np.float64) for n in ("h", "T", "S")}
    if inp.get("p_surf") is not None:
        a["p_surf"] = np.ascontiguousarray(np.stack([r["p_surf"] for r in rounds]), dtype=np.float64)
    before = {n: x.copy() for n, x in a.items()}
    Coef_x, Coef_y = coef if coef is not None else R.coef_planes(d, M)
    cx, cy = _c(Coef_x[0]), _c(Coef_y[0])
    tr = np.ascontiguousarray(np.stack(inp["tracers"]), dtype=np.float64) if ntr else np.zeros((0,) + d.shape3())
    uf = np.array(R.case_uf(opt, ntr) or [0.0] * ntr, dtype=np.float64)
    fatal = L.ref_neutral_diffusion(C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(gx), _p(masks), C.c_int(ncalls),
                                    _p(a["h"]), _p(a["T"]), _p(a["S"]), _p(a.get("p_surf")), _p(cx), _p(cy), C.c_double(dt), C.c_int(ntr),
                                    _p(tr), _p(uf))
    if fatal:
        return None, fatal
    if not dt > 0.0:
        return {}, fatal
    for n in a:
        assert np.array_equal(a[n], before[n], equal_nan=True), n + " is only read"
    out = dict(tracers=[tr[m].copy() for m in range(ntr)])
    for n in diag:
        out[n] = [_diag(NDIFF_DIAG_NAMES[n][1] % (m + 1), d.shape3() if n == "tendency" else d.shape2()) for m in range(ntr)]
    return out, fatal


def standin_never_count():
    """Of the last door's FATALs, those raised by a stand-in procedure that must never run."""
    return int(lib().ref_standin_never_count())


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_lateral_mixing_coeffs (with MOM_isopycnal_slopes) and MOM_thickness_diffuse

# the grid planes the two modules read, in the order of setup_lateral (oracle/ref_param_shim.F90)
LATERAL_METRICS = ("mask2dT", "mask2dCu", "mask2dCv", "IdxCu", "IdyCu", "IdxCv", "IdyCv", "dxCu", "dyCu", "dxCv", "dyCv", "dy_Cu", "dx_Cv",
                   "areaT", "IareaT", "areaCu", "areaCv", "bathyT")
LATERAL_EOS_NAMES = {abi.LINEAR: "LINEAR", abi.WRIGHT: "WRIGHT", abi.WRIGHT_FULL: "WRIGHT_FULL", abi.WRIGHT_REDUCED: "WRIGHT_REDUCED",
                     abi.UNESCO: "UNESCO", abi.ROQUET_RHO: "ROQUET_RHO", abi.JACKETT06: "JACKETT_06", abi.ROQUET_SPV: "ROQUET_SPV"}
# member of abi.VarMixParams -> (the name VarMix_init reads (MOM_lateral_mixing_coeffs.F90:1589-1758), kind, the unit of the member)
VARMIX_PARAM_NAMES = {
    "use_stored_slopes": ("USE_STORED_SLOPES", "bool", ""), "use_simpler_Eady_growth_rate": ("USE_SIMPLER_EADY_GROWTH_RATE", "bool", ""),
    "full_depth_Eady_growth_rate": ("FULL_DEPTH_EADY_GROWTH_RATE", "bool", ""), "kappa_smooth": ("KD_SMOOTH", "real", "H Z T-1"),
    "Visbeck_S_max": ("VISBECK_MAX_SLOPE", "real", "Z L-1"), "Visbeck_L_scale": ("VISBECK_L_SCALE", "real", "L"),
    "Eady_GR_D_scale": ("EADY_GROWTH_RATE_D_SCALE", "real", "Z"), "cropping_distance": ("EADY_GROWTH_RATE_CROPPING_DISTANCE", "real", "Z"),
    "VarMix_Ktop": ("VARMIX_KTOP", "int", ""), "h_min_N2": ("MIN_DZ_FOR_SLOPE_N2", "real", "H"),
    "use_stanley_iso": ("USE_STANLEY_ISO", "bool", ""), "debug": ("DEBUG", "bool", ""),
}
# Not parameters of VarMix_init: calculate_Eady_growth_rate is `use_MEKE or KHTR_SLOPE_CFF > 0 or KHTH_SLOPE_CFF > 0` (:1604): the
# table sets KHTR_SLOPE_CFF = 1 for it (KHTH_SLOPE_CFF stays 0: thickness_diffuse reads it too); VISBECK_MAX_SLOPE and
# VISBECK_L_SCALE are read only then (:1688, :1753).  max_depth is GV%max_depth and Angstrom_Z GV%Angstrom_Z; H_to_Z, H_to_RZ,
# Z_to_H_fill (GV%Z_to_H), g_Earth and Rho0 are GV's; Z_to_L and L_to_m come from the Z and L *_RESCALE_POWERs.  open_bcs is the
# OBC pointer (null in the door) and non_Boussinesq GV%Boussinesq (true in the door).
VARMIX_NOT_PARAMS = ("calculate_Eady_growth_rate", "max_depth", "H_to_Z", "Z_to_L", "L_to_m", "H_to_RZ", "Z_to_H_fill", "Angstrom_Z",
                     "g_Earth", "Rho0", "open_bcs", "non_Boussinesq")
# output of varmix_ref.run / the device -> where the reference has it: a public member of VarMix_CS, or the name of a diagnostic
# that calc_slope_functions (:725-735) or calc_Visbeck_coeffs_old (:943-945) posts
VARMIX_MEMBERS = ("SN_u", "SN_v", "slope_x", "slope_y")
VARMIX_DIAG_NAMES = {"N2_u": "N2_u", "N2_v": "N2_v", "S2_u": "S2_u", "S2_v": "S2_v", "dzu": "dzu_Visbeck", "dzv": "dzv_Visbeck",
                     "dzSxN": "dzSxN", "dzSyN": "dzSyN"}
# dzu, dzv, dzSxN and dzSyN are locals of calc_slope_functions, but it posts them (:726-729, registered :1815-1826): nothing that
# the device or the restatement hands out is hidden in the compiled module.
VARMIX_NOT_EXPOSED = ()
VARMIX_CORE = VARMIX_MEMBERS                        # in every file (slope_x, slope_y where the case stores slopes)
VARMIX_DROP_ORDER = ("dzSyN", "dzSxN", "dzv", "dzu", "N2_v", "N2_u", "S2_v", "S2_u")   # left out of a file over the size limit, in this order
# member of abi.ThicknessDiffuseParams -> (the name thickness_diffuse_init reads (MOM_thickness_diffuse.F90:2207-2404), kind, unit)
THICKDIFF_PARAM_NAMES = {
    "thickness_diffuse": ("THICKNESSDIFFUSE", "bool", ""), "Khth": ("KHTH", "real", "L2 T-1"), "read_khth": ("READ_KHTH", "bool", ""),
    "Khth_Min": ("KHTH_MIN", "real", "L2 T-1"), "Khth_Max": ("KHTH_MAX", "real", "L2 T-1"), "max_Khth_CFL": ("KHTH_MAX_CFL", "real", ""),
    "slope_max": ("KHTH_SLOPE_MAX", "real", "Z L-1"), "kappa_smooth": ("KD_SMOOTH", "real", "H Z T-1"),
    "Kh_eta_bg": ("KH_ETA_CONST", "real", "L2 T-1"), "Kh_eta_vel": ("KH_ETA_VEL_SCALE", "real", "L T-1"),
    "use_FGNV_streamfn": ("KHTH_USE_FGNV_STREAMFUNCTION", "bool", ""), "use_stanley_gm": ("USE_STANLEY_GM", "bool", ""),
    "detangle_interfaces": ("DETANGLE_INTERFACES", "bool", ""), "use_GME": ("USE_GME", "bool", ""), "use_MEKE": ("USE_MEKE", "bool", ""),
}
# Not parameters of thickness_diffuse_init: Z_to_L (the Z and L powers), Z_to_H_fill (GV%Z_to_H), nkml (GV%nkml), open_bcs,
# non_Boussinesq (GV%Boussinesq); use_variable_mixing is VarMix%use_variable_mixing, which VarMix_init sets; use_Kh_in_MEKE is
# read only with USE_MEKE; GMwork is `the diagnostic GMwork is registered`; skeb_use_gm is STOCH%skeb_use_gm (false in the door).
THICKDIFF_NOT_PARAMS = ("Z_to_L", "Z_to_H_fill", "nkml", "open_bcs", "non_Boussinesq", "use_variable_mixing", "use_Kh_in_MEKE", "GMwork",
                        "skeb_use_gm")
THICKDIFF_CORE = ("h", "uhtr", "vhtr")              # in every file
THICKDIFF_DROP_ORDER = ("vhGM", "uhGM")             # left out of a file over the size limit, in this order (the chain: CHAIN_DROP_ORDER)
THICKDIFF_OUT = THICKDIFF_CORE + ("uhGM", "vhGM")
# READ_KHTH: thickness_diffuse_init reads the plane from a file (:2217-2237) into a private member and passes it through
# pass_var: the khth2d case stays outside the comparison (the MOM_read_data stand-in counts as a path out of the compiled files).
THICKDIFF_LEFT_OUT = ("khth2d",)
UNITY = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0)


def lateral_units(GV, sc=None, max_depth=0.0):
    """The *_RESCALE_POWERs, vgr, vgx and the to-MKS factors of a lateral case.  `sc` names the factors by which a quantity in
    seconds, metres (horizontal), thickness units, metres (vertical) and kg m-3 is multiplied (the T, L, H, Z, R of
    tests/test_thickness_diffuse_cpu.scaled): s_to_T, m_to_L, m_to_H, m_to_Z and kg_m3_to_R.  GV is checked against them."""
    sc = dict(UNITY, **(sc or {}))
    T_, L, Hs, Z, Rr = (sc[k] for k in "TLHZR")
    powers = dict(Z=-_power_of_two(Z, "m_to_Z"), L=-_power_of_two(L, "m_to_L"), T=-_power_of_two(T_, "s_to_T"), R=-_power_of_two(Rr, "kg_m3_to_R"))
    _power_of_two(Hs, "m_to_H")
    assert GV.H_to_Z == Z / Hs and GV.Z_to_H == Hs / Z, "GV%H_to_Z is not what the factors give"
    assert GV.H_to_RZ == (GV.Rho0 * Z) / Hs or GV.H_to_RZ == GV.Rho0 * (Z / Hs), "GV%H_to_RZ is not Rho0 * H_to_Z"
    gv = np.array([GV.Rho0, GV.g_Earth * (Z / L) ** 2, GV.Angstrom_H, GV.H_to_Z * GV.Angstrom_H, GV.H_subroundoff, GV.dZ_subroundoff,
                   GV.H_to_Z, GV.Z_to_H, GV.H_to_RZ, GV.RZ_to_H, 1.0 / Hs, Hs, 1.0 / Hs, T_ / (Hs * Z)])
    gx = np.array([GV.g_Earth, Hs * Z / T_, (GV.Rho0 / Rr) / Hs, float(max_depth)])
    to_mks = {"": 1.0, "H Z T-1": T_ / (Hs * Z), "Z L-1": L / Z, "L": 1.0 / L, "Z": 1.0 / Z, "H": 1.0 / Hs, "L2 T-1": T_ / (L * L),
              "L T-1": T_ / L}
    return powers, gv, gx, to_mks, sc


def _entries(P, names, to_mks):
    ent = []
    for member, (name, kind, unit) in names.items():
        v = getattr(P, member)
        ent.append((name, float(v) * to_mks[unit] if kind == "real" else int(v) if kind == "int" else bool(v)))
    return ent


def _eos_entries(eos):
    if eos is None:
        return []
    ent = [("EQN_OF_STATE", LATERAL_EOS_NAMES[eos.form])]
    if eos.form == abi.LINEAR:
        ent += [("RHO_T0_S0", float(eos.Rho_T0_S0)), ("DRHO_DT", float(eos.dRho_dT)), ("DRHO_DS", float(eos.dRho_dS)),
                ("DRHO_DP", float(eos.dRho_dp))]
    return ent


def varmix_table(P, GV, eos=None, sc=None):
    """The parameter table of a calc_slope_functions case: members in the model's units go back to the MKS values a parameter file
    holds.  The unit factors among the members are checked against what unit_scaling_init and GV will give."""
    powers, gv, gx, to_mks, sc = lateral_units(GV, sc, P.max_depth)
    assert set(VARMIX_PARAM_NAMES) | set(VARMIX_NOT_PARAMS) == {n for n, _ in abi.VarMixParams._fields_}
    assert (P.H_to_Z, P.H_to_RZ, P.Z_to_H_fill, P.g_Earth, P.Rho0) == (GV.H_to_Z, GV.H_to_RZ, GV.Z_to_H, GV.g_Earth, GV.Rho0), "not GV's"
    assert P.Z_to_L == sc["L"] / sc["Z"] and P.L_to_m == 1.0 / sc["L"] and P.Angstrom_Z == GV.Angstrom_H * GV.H_to_Z, "not what US derives"
    assert not P.open_bcs and not P.non_Boussinesq
    ent = [("KHTR_SLOPE_CFF", 1.0 if P.calculate_Eady_growth_rate else 0.0), ("KHTH_SLOPE_CFF", 0.0)]
    return ent + _entries(P, VARMIX_PARAM_NAMES, to_mks) + _eos_entries(eos), powers, gv, gx


def thickdiff_table(P, GV, eos=None, sc=None, stored=False):
    """The parameter table of a thickness_diffuse case; USE_STORED_SLOPES (read by VarMix_init) where the case hands slopes over."""
    powers, gv, gx, to_mks, sc = lateral_units(GV, sc)
    assert set(THICKDIFF_PARAM_NAMES) | set(THICKDIFF_NOT_PARAMS) == {n for n, _ in abi.ThicknessDiffuseParams._fields_}
    assert P.Z_to_L == sc["L"] / sc["Z"] and P.Z_to_H_fill == GV.Z_to_H, "not what US and GV derive"
    assert not (P.use_variable_mixing or P.use_Kh_in_MEKE or P.GMwork or P.skeb_use_gm or P.nkml or P.open_bcs or P.non_Boussinesq)
    ent = [("KHTH_SLOPE_CFF", 0.0), ("KHTR_SLOPE_CFF", 0.0), ("USE_STORED_SLOPES", bool(stored))]
    return ent + _entries(P, THICKDIFF_PARAM_NAMES, to_mks) + _eos_entries(eos), powers, gv, gx


def _on_a_large_stack(fn, *args):
    """fn(*args) on a thread with a 1 GiB stack: the lateral routines hold some twenty whole 3-D arrays as automatic variables, which
    at 75 layers pass the 8 MiB a main thread usually has."""
    import threading
    box = []
    old = threading.stack_size(1 << 30)
    try:
        t = threading.Thread(target=lambda: box.append(fn(*args)))
        t.start(); t.join()
    finally:
        threading.stack_size(old)
    return box[0]


def _metrics(M):
    return np.ascontiguousarray(np.stack([M[G[n]] for n in LATERAL_METRICS]), dtype=np.float64)


def _layers(d, GV, Rlay, g_prime):
    if Rlay is None:
        Rlay, g_prime = abi.layer_densities(d.nk, Rho0=GV.Rho0, g_Earth=GV.g_Earth)
    gp = np.zeros(d.nk + 1); gp[:d.nk] = g_prime          # GV%g_prime has nk + 1 entries; the last is never read
    return _c(Rlay), gp


def varmix_ranges(d, P, nk=None):
    """name -> (k, j, i) slices of what calc_slope_functions writes of each output (the ranges of the reference's loops, halo = 1;
    tests/test_ref_parity_cpu.py holds the restatement's written words to exactly these)."""
    nz = d.nk if nk is None else nk
    ni, nj = d.ni, d.nj
    xs, ys = d.sl(-2, ni, -1, nj), d.sl(-1, ni, -2, nj)                 # calc_isoneutral_slopes with halo = 1 (:145, :255, :432)
    ru, rv = d.sl(-1, ni - 1, 0, nj - 1), d.sl(0, ni - 1, -1, nj - 1)
    allk, mid = slice(0, nz + 1), slice(1, nz)
    out = {}
    if not P.calculate_Eady_growth_rate:
        return out
    if P.use_stored_slopes:
        out.update(slope_x=(mid,) + xs, slope_y=(mid,) + ys, N2_u=(allk,) + xs, N2_v=(allk,) + ys)
    if P.use_simpler_Eady_growth_rate:
        box = d.sl(-1, ni, -1, nj)
        out.update(dzu=(allk,) + xs, dzv=(allk,) + ys, dzSxN=(allk,) + xs, dzSyN=(allk,) + ys, SN_u=box, SN_v=box)
    elif P.use_stored_slopes:
        out.update(SN_u=(slice(None), slice(None)), SN_v=(slice(None), slice(None)), S2_u=ru, S2_v=rv)
    else:
        out.update(SN_u=ru, SN_v=rv)
    return out


def thickdiff_ranges(d):
    """name -> (j, i) slices of what thickness_diffuse writes: h on the computational domain, the fluxes on their faces."""
    from tests import helpers as H
    return dict(h=H.interior(d, "h"), uhtr=H.interior(d, "u"), vhtr=H.interior(d, "v"), uhGM=H.interior(d, "u"), vhGM=H.interior(d, "v"))


def calc_slope_functions(d, M, GV, P, inp, dt, eos=None, give_ps=False, ncalls=1, inp2=None, sc=None, Rlay=None, g_prime=None,
                         table_extra=(), diag=tuple(VARMIX_DIAG_NAMES)):
    """unit_scaling_init, EOS_init and VarMix_init through the table, then calc_slope_functions `ncalls` times on the same VarMix_CS
    (round r on the h of `inp2` where given, else of `inp` again), with the arguments of tests/varmix_ref.run.  Returns SN_u, SN_v,
    slope_x, slope_y (the public members, where VarMix_init allocates them), L2u, L2v likewise, and every diagnostic of `diag`
    that was posted, by the names of varmix_ref.outputs: whole arrays, which outside varmix_ranges hold whatever the reference
    left; and the FATAL count.  dt <= 0: the inits only."""
    L = lib()
    ent, powers, gv, gx = varmix_table(P, GV, eos, sc)
    _table(ent + list(table_extra), powers)
    for n in diag:
        L.ref_want_diag(VARMIX_DIAG_NAMES[n].encode())
    ni_mem, nj_mem, idx = _tile(d)
    Rl, gp = _layers(d, GV, Rlay, g_prime)
    rounds = [inp] + [inp2 if inp2 is not None else inp] * (ncalls - 1)
    h = np.ascontiguousarray(np.stack([r["h"] for r in rounds]), dtype=np.float64)
    a = dict(T=_c(inp["T"]), S=_c(inp["S"])) if eos is not None else {}
    if give_ps:
        a["p_surf"] = _c(inp["p_surf"])
    before = dict({n: x.copy() for n, x in a.items()}, h=h.copy())
    o2 = {n: np.full(d.shape2(), np.nan) for n in ("SN_u", "SN_v", "L2u", "L2v")}
    o3 = {n: np.full(d.shape3(d.nk + 1), np.nan) for n in ("slope_x", "slope_y")}
    has = (C.c_int * 3)(0, 0, 0)
    fatal = _on_a_large_stack(L.ref_calc_slope_functions, C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(gx), _p(_metrics(M)), _p(Rl), _p(gp),
                                       C.c_int(ncalls), _p(h), _p(a.get("T")), _p(a.get("S")), _p(a.get("p_surf")), C.c_double(dt),
                                       _p(o2["SN_u"]), _p(o2["SN_v"]), _p(o3["slope_x"]), _p(o3["slope_y"]), _p(o2["L2u"]), _p(o2["L2v"]), has)
    if fatal:
        return None, fatal
    out = {}
    if has[2]:
        out.update(L2u=o2["L2u"], L2v=o2["L2v"])
    if not dt > 0.0:
        return out, fatal
    assert np.array_equal(h, before["h"], equal_nan=True), "h is only read"
    for n in a:
        assert np.array_equal(a[n], before[n], equal_nan=True), n + " is only read"
    if has[0]:
        out.update(SN_u=o2["SN_u"], SN_v=o2["SN_v"])
    if has[1]:
        out.update(o3)
    for n in diag:
        name = VARMIX_DIAG_NAMES[n]
        if L.ref_diag_size(name.encode()) > 0:
            out[n] = _diag(name, d.shape2() if n in ("S2_u", "S2_v") else d.shape3(d.nk + 1))
    return out, fatal


def thickness_diffuse(d, M, GV, P, inp, dt, eos=None, give_ps=False, stored=False, ncalls=1, sc=None, chain=None, table_extra=(),
                      diag=("uhGM", "vhGM"), Rlay=None, g_prime=None):
    """unit_scaling_init, EOS_init, VarMix_init and thickness_diffuse_init through the table, then thickness_diffuse `ncalls` times on
    the same control structures, with the arguments of tests/thickdiff_ref.run.  `stored`: inp["slope_x"], inp["slope_y"] are copied
    into VarMix%slope_x, VarMix%slope_y (USE_STORED_SLOPES true).  `chain`, an abi.VarMixParams: every round first runs
    calc_slope_functions on the same VarMix_CS, whose stored slopes thickness_diffuse reads; slope_x, slope_y, SN_u, SN_v come
    back too.  Returns h, uhtr, vhtr; uhGM, vhGM (CDp's, allocated where the diagnostics of those names are asked for); uhGM_diag,
    vhGM_diag (what the module posts); and the FATAL count.  dt <= 0: the inits only."""
    L = lib()
    assert not (stored and chain is not None)
    if chain is not None:
        ent, powers, gv, gx = varmix_table(chain, GV, eos, sc)
        ent2, powers2, _, _ = thickdiff_table(P, GV, eos, sc, stored=bool(chain.use_stored_slopes))
        assert powers == powers2 and chain.kappa_smooth == P.kappa_smooth and chain.use_stored_slopes, "one table serves both inits"
        ent = [e for e in ent2 if e[0] not in dict(ent)] + ent
    else:
        ent, powers, gv, gx = thickdiff_table(P, GV, eos, sc, stored=stored)
    _table(ent + list(table_extra), powers)
    for n in diag:
        L.ref_want_diag(n.encode())
    ni_mem, nj_mem, idx = _tile(d)
    Rl, gp = _layers(d, GV, Rlay, g_prime)
    a = dict(T=_c(inp["T"]), S=_c(inp["S"])) if eos is not None else {}
    if give_ps:
        a["p_surf"] = _c(inp["p_surf"])
    before = {n: x.copy() for n, x in a.items()}
    io = {n: _c(inp[n]).copy() for n in THICKDIFF_CORE}
    gm = {n: np.full(d.shape3(), np.nan) for n in ("uhGM", "vhGM")}
    sl = {n: (_c(inp[n]).copy() if stored else np.full(d.shape3(d.nk + 1), np.nan)) for n in ("slope_x", "slope_y")}
    sn = {n: np.full(d.shape2(), np.nan) for n in ("SN_u", "SN_v")}
    has = (C.c_int * 2)(0, 0)
    mode = 2 if chain is not None else 1 if stored else 0
    fatal = _on_a_large_stack(L.ref_thickness_diffuse, C.c_int(ni_mem), C.c_int(nj_mem), idx, C.c_int(d.nk), _p(gv), _p(gx), _p(_metrics(M)), _p(Rl), _p(gp),
                                    C.c_int(ncalls), C.c_int(mode), _p(io["h"]), _p(io["uhtr"]), _p(io["vhtr"]), _p(a.get("T")),
                                    _p(a.get("S")), _p(a.get("p_surf")), C.c_double(dt), _p(sl["slope_x"]), _p(sl["slope_y"]),
                                    _p(sn["SN_u"]), _p(sn["SN_v"]), _p(gm["uhGM"]), _p(gm["vhGM"]), has)
    if fatal:
        return None, fatal
    if not dt > 0.0:
        return {}, fatal
    for n in a:
        assert np.array_equal(a[n], before[n], equal_nan=True), n + " is only read"
    out = dict(io)
    for m, n in enumerate(("uhGM", "vhGM")):
        if has[m]:
            out[n] = gm[n]
        if n in diag and L.ref_diag_size(n.encode()) > 0:
            out[n + "_diag"] = _diag(n, d.shape3())
    if chain is not None:
        out.update(sl); out.update(sn)
    return out, fatal


def ndiff_ranges(d):
    """The ranges tests/test_neutral_diffusion_gpu.py's _check compares on, by output."""
    from tests import helpers as H
    return dict(tracers=H.interior(d, "h"), tendency=H.interior(d, "h"), trans_x_2d=H.interior(d, "u"), trans_y_2d=H.interior(d, "v"))


# ------------------------------------------------------------------------------------------------------------------------------
# recorded results (tests/golden/ref_opacity_*.npz, ref_epbl_*.npz, ref_kshear_*.npz, ref_ndiff_*.npz): written by
# scripts/record_ref_parity.py from the doors above

GOLDEN_OPACITY = ("manizza_3", "morel_1", "ohlmann_1")
GOLDEN_EPBL = ("croot_new", "rh18_orig_tl")      # (rh18_orig itself holds a setting the reference stops on: its twin)
# (case, grid, keyword arguments) of MOM_kappa_shear; the torus gets its shape in golden_configs
GOLDEN_KSHEAR = tuple((n, "island_basin", dict(nk=4)) for n in ("shear", "bugs", "nkml2", "layered", "newton", "tie")) + (
    ("shear", "benchmark_small", dict(nk=8)), ("nkml2", "benchmark_small", dict(nk=8)), ("shear", "benchmark_small", dict(nk=2)),
    ("shear", "torus", dict(nk=3)), ("layered", "torus", dict(nk=3)))
KSHEAR_CORE = ("kappa_io", "tke_io", "kv_io")                      # in every file
KSHEAR_DROP_ORDER = ("S2_mean", "N2_mean", "S2_init", "N2_init")   # what a file that would pass the size limit leaves out, in this order
# (case, grid, keyword arguments) of MOM_neutral_diffusion: every case on the island basin at 4 layers, the bowl at 1, 2 and 8, the
# edge torus at 3
GOLDEN_NDIFF = (("flat", "island_basin", dict(nk=4)), ("inverted", "island_basin", dict(nk=4)), ("massless", "island_basin", dict(nk=4)),
                ("new_order", "island_basin", dict(nk=4)), ("psurf", "island_basin", dict(nk=4)), ("refp", "island_basin", dict(nk=4)),
                ("refp_wright", "island_basin", dict(nk=4)), ("slope", "island_basin", dict(nk=4)), ("ties", "island_basin", dict(nk=4)), ("underflow", "island_basin", dict(nk=4)),
                ("unstratified", "island_basin", dict(nk=4)),
                ("slope", "benchmark_small", dict(nk=1)), ("slope", "benchmark_small", dict(nk=2)), ("slope", "benchmark_small", dict(nk=8)),
                ("massless", "benchmark_small", dict(nk=8)), ("slope", "torus", dict(nk=3)), ("new_order", "torus", dict(nk=3)))
NDIFF_CORE = ("tracers",)                                          # in every file
NDIFF_DROP_ORDER = ("tendency", "trans_y_2d", "trans_x_2d")        # what a file that would pass the size limit leaves out, in this order


# (case, EOS form or None, grid, keyword arguments) of calc_slope_functions: every case on the island basin at 4 layers (land, wet halo
# corners, Angstrom bands), eady once per EOS form there (the dispatch); eady, visbeck and just_e on the bowl at 1, 2 and 8 layers
# (no interior interface, exactly one; vert_fill_TS has separate first, middle and last steps; at one layer the reference's
# vert_fill_TS would read layer 2, so the two cases with an equation of state are replaced by their layered twins); eady_diag and
# visbeck_diag on the edge torus at 3
_OTHER_FORMS = (abi.LINEAR, abi.WRIGHT_FULL, abi.WRIGHT_REDUCED, abi.UNESCO, abi.ROQUET_RHO, abi.JACKETT06, abi.ROQUET_SPV)
GOLDEN_VARMIX = tuple((n, abi.WRIGHT, "island_basin", dict(nk=4)) for n in (
    "eady", "eady_diag", "eady_nocrop", "eady_tie", "eady_noeos", "visbeck", "visbeck_diag", "visbeck_neg", "visbeck_noeos", "just_e", "just_e_full")) + tuple(
    ("eady", f, "island_basin", dict(nk=4)) for f in _OTHER_FORMS) + tuple(
    (n, abi.WRIGHT, "benchmark_small", dict(nk=nk)) for nk in (2, 8) for n in ("eady", "visbeck", "just_e")) + tuple(
    (n, abi.WRIGHT, "benchmark_small", dict(nk=1)) for n in ("eady_noeos", "visbeck_noeos", "just_e")) + (
    ("eady_diag", abi.WRIGHT, "torus", dict(nk=3)), ("visbeck_diag", abi.WRIGHT, "torus", dict(nk=3)))
# likewise of thickness_diffuse: every case but khth2d (THICKDIFF_LEFT_OUT) on the island basin at 4, eos once per form; eos and
# noeos on the bowl at 2 and 8, noeos at 1; eos and slopes_noeos on the edge torus at 3; and the chain (calc_slope_functions, whose
# stored slopes thickness_diffuse reads on the same VarMix_CS) on the bowl at 8
GOLDEN_THICKDIFF = tuple((n, abi.WRIGHT, "island_basin", dict(nk=4)) for n in (
    "noeos", "eos", "psurf", "slopes_eos", "slopes_noeos", "kmax", "kmin", "large", "large_noeos", "kd0", "gm", "thin_top")) + tuple(
    ("eos", f, "island_basin", dict(nk=4)) for f in _OTHER_FORMS) + tuple(
    (n, abi.WRIGHT, "benchmark_small", dict(nk=nk)) for nk in (2, 8) for n in ("eos", "noeos")) + (
    ("noeos", abi.WRIGHT, "benchmark_small", dict(nk=1)), ("eos", abi.WRIGHT, "torus", dict(nk=3)),
    ("slopes_noeos", abi.WRIGHT, "torus", dict(nk=3)), ("chain", abi.WRIGHT, "benchmark_small", dict(nk=8)))
CHAIN_OUT = THICKDIFF_CORE + VARMIX_MEMBERS          # what the chain case hands out; h, uhtr, vhtr (which both slopes feed) are in its file,
CHAIN_DROP_ORDER = ("slope_y", "slope_x", "SN_v", "SN_u")   # of the intermediate planes a file over the size limit leaves out these, in this order
CHAIN_DT = 3600.0


def chain_params(GV):
    """The two parameter sets of the chain case (test_chain_into_thickness_diffuse_and_tracer_hordiff of tests/test_varmix_gpu.py)."""
    from tests import varmix_ref
    return abi.varmix_params_default(GV, Visbeck_L_scale=3.0e4, **varmix_ref.VISB), abi.thickness_diffuse_params_default()


def _form_tag(name, form):
    return name if form == abi.WRIGHT else f"{name}-{LATERAL_EOS_NAMES[form].lower()}"


def edge_torus_shape():
    bx, by, _ = abi.lane_launch_shape()
    return bx + 1, by + 1


def golden_configs():
    """(kind, case, grid, keyword arguments of the grid's helper) of every recorded result."""
    ni, nj = edge_torus_shape()
    out = []
    for name in GOLDEN_OPACITY:
        out.append(("opacity", name, "island_basin", dict(nk=4)))
        out.append(("opacity", name, "torus", dict(nk=3, ni=ni, nj=nj)))
    for name in GOLDEN_EPBL:
        out.append(("epbl", name, "benchmark_small", dict(nk=3)))
        out.append(("epbl", name, "benchmark_small", dict(nk=8)))
        out.append(("epbl", name, "torus", dict(nk=3, ni=ni, nj=nj)))
    for name, grid, kw in GOLDEN_KSHEAR:
        out.append(("kshear", name, grid, dict(kw, ni=ni, nj=nj) if grid == "torus" else dict(kw)))
    for name, grid, kw in GOLDEN_NDIFF:
        out.append(("ndiff", name, grid, dict(kw, ni=ni, nj=nj) if grid == "torus" else dict(kw)))
    for kind, configs in (("varmix", GOLDEN_VARMIX), ("thickdiff", GOLDEN_THICKDIFF)):
        for name, form, grid, kw in configs:
            out.append((kind, _form_tag(name, form), grid, dict(kw, ni=ni, nj=nj) if grid == "torus" else dict(kw)))
    return out


def golden_name(kind, name, grid, kw):
    shape = "x".join(str(kw[k]) for k in ("ni", "nj", "nk") if k in kw)
    return f"ref_{kind}_{name}_{grid}_{shape}"


def golden_setup(kind, name, grid, kw):
    """(d, M, GV, P, opt, inp) of a recorded configuration: the inputs are regenerated from the seeded case_inputs."""
    from tests import helpers as H
    from tests import opacity_ref, epbl_ref, kappa_shear_ref, ndiff_ref
    d, M = getattr(H, grid)(**kw)[1:]
    GV = abi.vgrid_default()
    if kind == "ndiff":       # the NaN-beyond-the-first-halo inputs of ndiff_ref.want, without running the restatement
        P, opt = ndiff_ref.case(name)
        return d, M, GV, P, opt, ndiff_ref.nan_halo(d, ndiff_ref.case_inputs(d, M, GV, opt, ntr=3))
    if kind in ("varmix", "thickdiff"):
        return (d, M, GV) + lateral_setup(kind, name, d, M, GV)
    if kind == "kshear":
        P, opt = kappa_shear_ref.case(name, GV)
        opt = dict(opt, diag=kappa_shear_ref.DIAG_3D + kappa_shear_ref.DIAG_2D)       # every diagnostic, whatever the case names
        inp = kappa_shear_ref.case_inputs(d, M, GV, opt)
    elif kind == "opacity":
        P, opt = opacity_ref.case(name)
        inp = opacity_ref.case_inputs(d, M, opt)
    else:
        P, opt = epbl_ref.case(name, GV)
        inp = epbl_ref.case_inputs(d, M, GV, opt)
    return d, M, GV, P, opt, inp


def lateral_setup(kind, tag, d, M, GV):
    """(P, opt, inp) of a recorded varmix or thickdiff configuration.  opt holds the arguments of the case (eos, give_ps, stored,
    dt, chain); the inputs are NaN beyond what the reference reads (nan_beyond)."""
    from tests import thickdiff_ref, varmix_ref
    name, _, ftag = tag.partition("-")
    form = {v.lower(): k for k, v in LATERAL_EOS_NAMES.items()}[ftag] if ftag else abi.WRIGHT
    if kind == "varmix":
        P, eos, ps, dg, dt, opts = varmix_ref.case(name, GV, form=form, nk=d.nk)
        inp = varmix_ref.inputs(d, M, GV, **opts)
        return P, dict(eos=eos, give_ps=ps, dt=dt), nan_beyond(d, inp, "varmix")
    if name == "chain":
        Pv, P = chain_params(GV)
        inp = thickdiff_ref.inputs(d, M, GV)
        return P, dict(eos=abi.eos_params_default(abi.WRIGHT), give_ps=False, stored=False, dt=CHAIN_DT, chain=Pv), nan_beyond(d, inp, "varmix")
    P, eos, ps, stored, gm, dt, opts = thickdiff_ref.case(name, form=form)
    inp = thickdiff_ref.inputs(d, M, GV, **opts)
    return P, dict(eos=eos, give_ps=ps, stored=stored, dt=dt, chain=None), nan_beyond(d, inp, "thickdiff")


def nan_beyond(d, inp, kind):
    """The inputs with NaN where the reference's loops read nothing.  thickness_diffuse reads cells one beyond the computational
    domain in x or in y (a plus shape, no halo corner) and stored slopes on their faces of the domain; calc_slope_functions the box
    one beyond it (the four-face averages and calc_slope_functions_using_just_e read its corners) and a second cell in x or in y
    (calc_isoneutral_slopes with halo = 1).  uhtr and vhtr are read on their faces of the domain."""
    from tests import helpers as H
    ni, nj = d.ni, d.nj
    read = np.zeros(d.shape2(), bool)
    if kind == "varmix":
        for r in ((-2, ni + 1, -1, nj), (-1, ni, -2, nj + 1)):
            read[d.sl(*r)] = True
    else:
        for r in ((-1, ni, 0, nj - 1), (0, ni - 1, -1, nj)):
            read[d.sl(*r)] = True
    out = {}
    for n, a in inp.items():
        if n in ("h", "T", "S", "p_surf", "khth2d"):
            keep = read
        else:
            keep = np.zeros(d.shape2(), bool); keep[H.interior(d, "u" if n in ("uhtr", "slope_x") else "v")] = True
        out[n] = np.ascontiguousarray(np.where(keep, a, np.nan))
    return out


def _varmix_door(d, M, GV, P, opt, inp):
    """The recorded outputs of a varmix configuration, each cut to its range of varmix_ranges (L2u, L2v are not recorded)."""
    got, fatal = calc_slope_functions(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"])
    if fatal:
        return None, fatal
    rng = varmix_ranges(d, P)
    return {n: np.ascontiguousarray(got[n][rng[n]]) for n in rng}, fatal


def _thickdiff_door(d, M, GV, P, opt, inp):
    """Likewise of a thickdiff configuration, each output on its range of thickdiff_ranges (the chain: CHAIN_OUT, the slopes and
    SN_u, SN_v on theirs of varmix_ranges)."""
    got, fatal = thickness_diffuse(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"], stored=opt["stored"],
                                   chain=opt["chain"])
    if fatal:
        return None, fatal
    rng = thickdiff_ranges(d)
    if opt["chain"] is not None:
        rng = dict({n: rng[n] for n in THICKDIFF_CORE}, **{n: varmix_ranges(d, opt["chain"])[n] for n in VARMIX_MEMBERS})
        return {n: np.ascontiguousarray(got[n][(Ellipsis,) + rng[n]]) for n in CHAIN_OUT}, fatal
    assert all(np.array_equal(got[n + "_diag"][(Ellipsis,) + rng[n]], got[n][(Ellipsis,) + rng[n]]) for n in ("uhGM", "vhGM"))
    return {n: np.ascontiguousarray(got[n][(Ellipsis,) + rng[n]]) for n in THICKDIFF_OUT}, fatal


DOORS = dict(opacity=opacity, epbl=energetic_PBL, kshear=Calculate_kappa_shear, ndiff=neutral_diffusion, varmix=_varmix_door,
             thickdiff=_thickdiff_door)     # kind -> its door


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def input_hashes(M, inp, kind=None):
    """SHA-256 of every input array of a case and of the grid planes the modules read."""
    if kind == "ndiff":
        h = {n: sha256(a) for n, a in inp.items() if not isinstance(a, list)}
        h.update({"tracer_%d" % m: sha256(a) for m, a in enumerate(inp["tracers"])})
        for n in ("mask2dT", "mask2dCu", "mask2dCv", "IareaT"):
            h[n] = sha256(M[G[n]])
        return h
    if kind in ("varmix", "thickdiff"):
        h = {n: sha256(a) for n, a in inp.items()}
        h.update({n: sha256(M[G[n]]) for n in LATERAL_METRICS})
        return h
    h = {n: sha256(a) for n, a in inp.items() if a is not None}
    h["mask2dT"] = sha256(M[G["mask2dT"]]); h["CoriolisBu"] = sha256(M[G["CoriolisBu"]])
    if kind == "kshear":
        for n in ("Coriolis2Bu", "areaCu", "areaCv", "IareaT"):
            h[n] = sha256(M[G[n]])
    return h


def dom(d):
    return d.sl(0, d.ni - 1, 0, d.nj - 1)


def load_golden(kind, name, grid, kw, M, inp):
    """The recorded outputs on the computational domain (kind ndiff: each on its range of ndiff_ranges; varmix and thickdiff: each on
    its range of varmix_ranges or thickdiff_ranges), after the stored hashes of the inputs have been checked against the
    regenerated ones."""
    path = os.path.join(GOLDEN, golden_name(kind, name, grid, kw) + ".npz")
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    want = input_hashes(M, inp, kind)
    names = [str(s) for s in got.pop("input_names")]
    hashes = [str(s) for s in got.pop("input_sha256")]
    assert dict(zip(names, hashes)) == want, f"{path}: the seeded inputs are not the recorded ones"
    if kind == "ndiff":       # an output is stored as one array [ntr, ...] on its range of ndiff_ranges; handed back as a list
        got = {n: [x for x in a] for n, a in got.items()}
    return got
