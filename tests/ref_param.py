"""The loader of oracle/_ref/libref_param.so -- the reference's own MOM_EOS_Wright*.F90, MOM_EOS_linear.F90,
MOM_intrinsic_functions.F90, MOM_opacity.F90, MOM_energetic_PBL.F90 and MOM_kappa_shear.F90 (with MOM_EOS.F90) compiled where they
lie against the interface stand-ins of oracle/ref_standins.F90, behind the bind(C) doors of oracle/ref_param_shim.F90 -- and the
one place where the members of abi.OpacityParams, abi.EnergeticPBLParams and abi.KappaShearParams are mapped to the names the
reference reads with get_param.  Test infrastructure:
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
        for n in ("ref_opacity", "ref_energetic_PBL", "ref_absorbRemainingSW", "ref_sumSWoverBands", "ref_Calculate_kappa_shear"):
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
# recorded results (tests/golden/ref_opacity_*.npz, ref_epbl_*.npz, ref_kshear_*.npz): written by scripts/record_ref_parity.py from
# the doors above

GOLDEN_OPACITY = ("manizza_3", "morel_1", "ohlmann_1")
GOLDEN_EPBL = ("croot_new", "rh18_orig_tl")      # (rh18_orig itself holds a setting the reference stops on: its twin)
# (case, grid, keyword arguments) of MOM_kappa_shear; the torus gets its shape in golden_configs
GOLDEN_KSHEAR = tuple((n, "island_basin", dict(nk=4)) for n in ("shear", "bugs", "nkml2", "layered", "newton", "tie")) + (
    ("shear", "benchmark_small", dict(nk=8)), ("nkml2", "benchmark_small", dict(nk=8)), ("shear", "benchmark_small", dict(nk=2)),
    ("shear", "torus", dict(nk=3)), ("layered", "torus", dict(nk=3)))
KSHEAR_CORE = ("kappa_io", "tke_io", "kv_io")                      # in every file
KSHEAR_DROP_ORDER = ("S2_mean", "N2_mean", "S2_init", "N2_init")   # what a file that would pass the size limit leaves out, in this order


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
    return out


def golden_name(kind, name, grid, kw):
    shape = "x".join(str(kw[k]) for k in ("ni", "nj", "nk") if k in kw)
    return f"ref_{kind}_{name}_{grid}_{shape}"


def golden_setup(kind, name, grid, kw):
    """(d, M, GV, P, opt, inp) of a recorded configuration: the inputs are regenerated from the seeded case_inputs."""
    from tests import helpers as H
    from tests import opacity_ref, epbl_ref, kappa_shear_ref
    d, M = getattr(H, grid)(**kw)[1:]
    GV = abi.vgrid_default()
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


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def input_hashes(M, inp, kind=None):
    """SHA-256 of every input array of a case and of the grid planes the modules read."""
    h = {n: sha256(a) for n, a in inp.items() if a is not None}
    h["mask2dT"] = sha256(M[G["mask2dT"]]); h["CoriolisBu"] = sha256(M[G["CoriolisBu"]])
    if kind == "kshear":
        for n in ("Coriolis2Bu", "areaCu", "areaCv", "IareaT"):
            h[n] = sha256(M[G[n]])
    return h


def dom(d):
    return d.sl(0, d.ni - 1, 0, d.nj - 1)


def load_golden(kind, name, grid, kw, M, inp):
    """The recorded outputs on the computational domain, after the stored hashes of the inputs have been checked against the
    regenerated ones."""
    path = os.path.join(GOLDEN, golden_name(kind, name, grid, kw) + ".npz")
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    want = input_hashes(M, inp, kind)
    names = [str(s) for s in got.pop("input_names")]
    hashes = [str(s) for s in got.pop("input_sha256")]
    assert dict(zip(names, hashes)) == want, f"{path}: the seeded inputs are not the recorded ones"
    return got
