"""The checker of mom6x_applyBoundaryFluxesInOut: a numpy restatement of applyBoundaryFluxesInOut
(src/parameterizations/vertical/MOM_diabatic_aux.F90:682-1346, the Boussinesq path without brine plumes) with its callees
extractFluxes1d (src/core/MOM_forcing_type.F90:447-948, do_enthalpy = .true.) and absorbRemainingSW (MOM_opacity.F90:600-867 with
adjustAbsorptionProfile = .false., absorbAllSW = .true., no eps, ksort, htot or Ttot), vectorised over the columns of the
computational domain with loops over k and over the bands and masks for the columns an arm applies to.  Arrays are in the pitched
tile layout of include/mom6x.h ([k, j + joff, i + ioff]).

The steps run as the reference runs them -- the derivatives for every layer, then step A, then step B for every layer, then the
downward and the upward loop of absorbRemainingSW -- not as the device's single walk, so the two orders check each other.  The
arithmetic is the reference's, operation for operation (x**2 written as x*x, MAX and MIN as the reference's compiler evaluates
them), so that the device can be held to it bit for bit wherever no exp is evaluated with an argument other than 0 or below -750.
The density derivatives of SkinBuoyFlux come from the oracle's EOS through ref_common._derivs; the specific-volume derivatives are
restated here from the five reference routines (specvol_derivs).  `counts` (BRANCHES) records how often each arm fired.

Where the reference stops (a negative thickness :1163, a flux over land :1178) the restatement counts, leaves T and S of the layer
alone and goes on, as the device does; `status` returns the three counts."""
import os
import re

import numpy as np

from mom6_amd import abi
from tests.ref_common import _derivs, _max, _min

G = abi.G
BRANCHES = ("scale_full", "scale_reduced", "massout_evap", "massout_lprec", "massout_seaice", "massout_vprec", "agg_fw", "split_fw",
            "river_heat", "calving_heat", "rivermix", "a_energetics", "b_thin_layer", "b_cfl_limited", "b_dsalt_limited",
            "b_layer_emptied", "b_negative_h", "land_flux", "grounding", "sw_skip_thin", "sw_old_cut", "sw_new_zero", "sw_new_min",
            "sw_new_none", "tke_large_od", "tke_taylor", "h_heat_full", "h_heat_partial", "h_heat_none", "bottom_all",
            "bottom_limited", "tchg_full", "tchg_partial", "exp")
OUT3 = ("cTKE", "dSV_dT", "dSV_dS", "penSW_diag", "penSWflux_diag")
OUT2 = ("SkinBuoyFlux", "createdH", "nonpenSW_diag")
FLUX_OUT = abi.SURFACE_FLUXES_OUT
FLUX_REQUIRED = abi.SURFACE_FLUXES_IN


def _dom(d):
    return d.sl(0, d.ni - 1, 0, d.nj - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# calculate_specific_vol_derivs

_WRIGHT = dict(a0=7.057924e-4, a1=3.480336e-7, a2=-1.112733e-7, b0=5.790749e8, b1=3.516535e6, b2=-4.002714e4, b3=2.084372e2,
               b4=5.944068e5, b5=-9.643486e3, c0=1.704853e5, c1=7.904722e2, c2=-7.984422, c3=5.140652e-2, c4=-2.302158e2,
               c5=-3.079464)                                     # MOM_EOS_Wright.F90:23-37, MOM_EOS_Wright_red.F90:18-35
_WRIGHT_FULL = dict(a0=7.133718e-4, a1=2.724670e-7, a2=-1.646582e-7, b0=5.613770e8, b1=3.600337e6, b2=-3.727194e4, b3=1.660557e2,
                    b4=6.844158e5, b5=-8.389457e3, c0=1.609893e5, c1=8.427815e2, c2=-6.931554, c3=3.869318e-2, c4=-1.664201e2,
                    c5=-2.765195)                                # MOM_EOS_Wright_full.F90:18-35
_RS = None


def _roquet_spv_coefs():
    """The ALP and BET coefficients of MOM_EOS_Roquet_SpV.F90 as the library's header states them (mom6_amd/csrc/eos_dev.h, the
    RS_ macros, which follow the reference's parameter statements term by term), evaluated in the header's order."""
    global _RS
    if _RS is None:
        txt = open(os.path.join(os.path.dirname(os.path.abspath(abi.__file__)), "csrc", "eos_dev.h")).read()
        ns = dict(RQ_POW2=lambda x: x * x, RQ_POW3=lambda x: x * (x * x), RQ_POW4=lambda x: (x * x) * (x * x),
                  RQ_POW5=lambda x: x * ((x * x) * (x * x)), RQ_POW6=lambda x: (x * x) * ((x * x) * (x * x)))
        for name, expr in re.findall(r"^#define (RS_\w+) \((.*)\)\s*$", txt, flags=re.M):
            ns[name] = eval(expr, {"__builtins__": {}}, ns)   # noqa: S307 -- arithmetic on the header's own constants
        _RS = {k[3:]: v for k, v in ns.items() if k.startswith("RS_")}
        assert len(_RS) > 120 and _RS["rdeltaS"] == 24.0 and "ALP050" in _RS and "BET003" in _RS
    return _RS


def _roquet_spv_derivs(T, S, pressure):
    """calculate_specvol_derivs_elem_Roquet_SpV, MOM_EOS_Roquet_SpV.F90:352-423."""
    c = _roquet_spv_coefs()
    zt, zs, zp = T, np.sqrt(np.abs(S + c["rdeltaS"]) * c["r1_S0"]), pressure
    out = []
    for X in ("ALP", "BET"):
        q = lambda n, X=X: c[X + n]
        d3 = q("003")
        d2 = q("002") + (zs * q("102") + zt * q("012"))
        d1 = q("001") + (zs * (q("101") + zs * (q("201") + zs * q("301"))) +
                         zt * (q("011") + (zs * (q("111") + zs * q("211")) + zt * (q("021") + (zs * q("121") + zt * q("031"))))))
        d0 = q("000") + (zs * (q("100") + zs * (q("200") + zs * (q("300") + zs * (q("400") + zs * q("500"))))) +
                         zt * (q("010") + (zs * (q("110") + zs * (q("210") + zs * (q("310") + zs * q("410")))) +
                                           zt * (q("020") + (zs * (q("120") + zs * (q("220") + zs * q("320"))) +
                                                             zt * (q("030") + (zt * (q("040") + (zs * q("140") + zt * q("050"))) +
                                                                               zs * (q("130") + zs * q("230")))))))))
        out.append(d0 + zp * (d1 + zp * (d2 + zp * d3)))
    return out[0], out[1] / zs


def specvol_derivs(eos, T, S, pressure):
    """dSV_dT, dSV_dS of calculate_specific_vol_derivs (MOM_EOS.F90:1039) for LINEAR (MOM_EOS_linear.F90:164), WRIGHT
    (MOM_EOS_Wright.F90:270), WRIGHT_FULL (MOM_EOS_Wright_full.F90:275), WRIGHT_REDUCED (MOM_EOS_Wright_red.F90:277) and
    ROQUET_SPV; pressure in Pa."""
    form = eos.form
    if form == abi.LINEAR:
        rho = eos.Rho_T0_S0 + ((eos.dRho_dT * T + eos.dRho_dS * S) + eos.dRho_dp * pressure)
        I_rho2 = 1.0 / (rho * rho)
        return -eos.dRho_dT * I_rho2, -eos.dRho_dS * I_rho2
    if form == abi.ROQUET_SPV:
        return _roquet_spv_derivs(T, S, pressure)
    assert form in (abi.WRIGHT, abi.WRIGHT_FULL, abi.WRIGHT_REDUCED), form
    W = _WRIGHT_FULL if form == abi.WRIGHT_FULL else _WRIGHT
    a1, a2 = W["a1"], W["a2"]
    b0, b1, b2, b3, b4, b5 = (W[n] for n in ("b0", "b1", "b2", "b3", "b4", "b5"))
    c0, c1, c2, c3, c4, c5 = (W[n] for n in ("c0", "c1", "c2", "c3", "c4", "c5"))
    if form == abi.WRIGHT:
        p0 = (b0 + b4 * S) + T * (b1 + T * ((b2 + b3 * T)) + b5 * S)
        lam = (c0 + c4 * S) + T * (c1 + T * ((c2 + c3 * T)) + c5 * S)
        I_denom = 1.0 / (pressure + p0)
        dSV_dT = (a1 + I_denom * (c1 + T * ((2.0 * c2 + 3.0 * c3 * T)) + c5 * S)) - \
            ((I_denom * I_denom) * lam) * (b1 + T * ((2.0 * b2 + 3.0 * b3 * T)) + b5 * S)
        dSV_dS = (a2 + I_denom * (c4 + c5 * T)) - ((I_denom * I_denom) * lam) * (b4 + b5 * T)
        return dSV_dT, dSV_dS
    p0 = b0 + (b4 * S + T * (b1 + (T * (b2 + b3 * T) + b5 * S)))
    lam = c0 + (c4 * S + T * (c1 + (T * (c2 + c3 * T) + c5 * S)))
    I_denom = 1.0 / (pressure + p0)
    dSV_dT = a1 + I_denom * ((c1 + (T * (2.0 * c2 + 3.0 * c3 * T) + c5 * S)) -
                             (I_denom * lam) * (b1 + (T * (2.0 * b2 + 3.0 * b3 * T) + b5 * S)))
    dSV_dS = a2 + I_denom * ((c4 + c5 * T) - (I_denom * lam) * (b4 + b5 * T))
    return dSV_dT, dSV_dS


# ------------------------------------------------------------------------------------------------------------------------------
# absorbRemainingSW

def absorbRemainingSW(GV, P, h, opacity_band, nsw, dt, H_limit_fluxes, T, Pen_SW_bnd, TKE=None, dSV_dT=None, counts=None):
    """MOM_opacity.F90:600-867 on slices [k, j, i] (opacity_band [n, k, j, i], Pen_SW_bnd [n, j, i]); T, Pen_SW_bnd and TKE are
    changed in place."""
    if nsw < 1:
        return
    nz = h.shape[0]
    min_SW_heat = P.PenSW_flux_absorb * dt
    I_Habs = P.PenSW_absorb_Invlen
    h_min_heat = 2.0 * GV.Angstrom_H + GV.H_subroundoff
    C1_6, C1_60 = 1.0 / 6.0, 1.0 / 60.0
    TKE_calc = TKE is not None and dSV_dT is not None
    old = P.optics_answer_date < 20190101
    if old:
        g_Hconv2 = (P.g_Earth_Z_T2 * GV.H_to_RZ) * GV.H_to_RZ
    else:
        g_Hconv2 = P.g_Earth_Z_T2 * (GV.H_to_RZ * GV.H_to_RZ)
    h_heat = np.zeros(h.shape[1:])
    fnsw = float(nsw)
    for k in range(nz):
        hk = h[k]
        thick = hk > 1.5 * 0.0                                    # epsilon = 0
        counts["sw_skip_thin"] += int((~thick).sum())
        for n in range(nsw):
            on = thick & (Pen_SW_bnd[n] > 0.0)
            if not on.any():
                continue
            hs = np.where(on, hk, 1.0)                            # (the lanes that are off compute on harmless values)
            Pen = np.where(on, Pen_SW_bnd[n], 1.0)
            opt_depth = hs * opacity_band[n, k]
            exp_OD = np.exp(-opt_depth)
            counts["exp"] += int((on & (opt_depth != 0.0) & ~(opt_depth > 750.0)).sum())
            SW_trans = exp_OD
            if old:
                cut = on & (fnsw * Pen * SW_trans < min_SW_heat * _min(1.0, I_Habs * hs))
                counts["sw_old_cut"] += int(cut.sum())
                SW_trans = np.where(cut, 0.0, SW_trans)
            else:
                c1 = (fnsw * Pen * SW_trans < min_SW_heat) & (hs > h_min_heat)
                zero = c1 & (fnsw * Pen <= min_SW_heat * (I_Habs * (hs - h_min_heat)))
                lim = c1 & ~zero
                counts["sw_new_zero"] += int((on & zero).sum())
                counts["sw_new_min"] += int((on & lim).sum())
                counts["sw_new_none"] += int((on & ~c1).sum())
                SW_trans = np.where(zero, 0.0, np.where(lim, _min(SW_trans, 1.0 - (min_SW_heat * (I_Habs * (hs - h_min_heat))) /
                                                                  (fnsw * Pen)), SW_trans))
            Heat_bnd = Pen * (1.0 - SW_trans)
            T[k] = np.where(on, T[k] + Pen * (1.0 - SW_trans) / hs, T[k])
            if TKE_calc:
                big = opt_depth > 1e-2
                counts["tke_large_od"] += int((on & big).sum())
                counts["tke_taylor"] += int((on & ~big).sum())
                od = np.where(big, opt_depth, 1.0)
                t_big = TKE[k] - 1.0 * Heat_bnd * dSV_dT[k] * (0.5 * hs * g_Hconv2) * \
                    (od * (1.0 + exp_OD) - 2.0 * (1.0 - exp_OD)) / np.where(big, od * (1.0 - exp_OD), 1.0)
                t_small = TKE[k] - 1.0 * Heat_bnd * dSV_dT[k] * (0.5 * hs * g_Hconv2) * \
                    (C1_6 * opt_depth * (1.0 - C1_60 * (opt_depth * opt_depth)))
                TKE[k] = np.where(on, np.where(big, t_big, t_small), TKE[k])
            Pen_SW_bnd[n] = np.where(on, Pen * SW_trans, Pen_SW_bnd[n])
        full = hk >= 2.0 * h_min_heat
        part = ~full & (hk > h_min_heat)
        counts["h_heat_full"] += int(full.sum()); counts["h_heat_partial"] += int(part.sum())
        counts["h_heat_none"] += int((~full & ~part).sum())
        h_heat = np.where(full, h_heat + hk, np.where(part, h_heat + (2.0 * hk - 2.0 * h_min_heat), h_heat))
    T_chg = np.zeros(h.shape[1:])
    Pen_SW_rem = Pen_SW_bnd[0].copy()
    for n in range(1, nsw):
        Pen_SW_rem = Pen_SW_rem + Pen_SW_bnd[n]
    Ih_limit = 1.0 / H_limit_fluxes
    rem = (Pen_SW_rem > 0.0) & (h_heat > 0.0)
    allw = rem & (h_heat * Ih_limit >= 1.0)
    limw = rem & ~allw
    counts["bottom_all"] += int(allw.sum()); counts["bottom_limited"] += int(limw.sum())
    hh = np.where(rem, h_heat, 1.0)
    T_chg = np.where(allw, Pen_SW_rem / hh, np.where(limw, Pen_SW_rem * Ih_limit, T_chg))
    unabsorbed = np.where(allw, 0.0, 1.0 - hh * Ih_limit)
    for n in range(nsw):
        Pen_SW_bnd[n] = np.where(rem, unabsorbed * Pen_SW_bnd[n], Pen_SW_bnd[n])
    for k in range(nz - 1, -1, -1):
        hk = h[k]
        up = T_chg > 0.0
        full = up & (hk >= 2.0 * h_min_heat)
        part = up & ~full & (hk > h_min_heat)
        counts["tchg_full"] += int(full.sum()); counts["tchg_partial"] += int(part.sum())
        hs = np.where(part, hk, 1.0)
        T[k] = np.where(full, T[k] + T_chg, np.where(part, T[k] + T_chg * (2.0 - 2.0 * h_min_heat / hs), T[k]))
        T_chg = T_chg + 0.0                                       # T_chg_above = 0


# ------------------------------------------------------------------------------------------------------------------------------
# applyBoundaryFluxesInOut

def applyBoundaryFluxesInOut(d, M, GV, P, dt, fluxes, h, T, S, nsw=0, opacity_band=None, sw_pen_band=None, tv_p_surf=None,
                             aggregate_FW_forcing=True, evap_CFL_limit=0.8, minimum_forcing_depth=0.001, eos=None, orc=None,
                             cTKE=None, dSV_dT=None, dSV_dS=None, SkinBuoyFlux=None, createdH=None, penSW_diag=None,
                             penSWflux_diag=None, nonpenSW_diag=None, counts=None):
    """h, T, S, the given planes of `fluxes` (a dict by the names of abi.SURFACE_FLUXES_NAMES, None: not associated) and the
    given outputs are changed in place.  Returns (groundings, negative_h, land_fluxes)."""
    counts = counts if counts is not None else dict.fromkeys(BRANCHES, 0)
    dom = _dom(d)
    D3 = (slice(None),) + dom
    nz = d.nk
    Idt = 1.0 / dt
    energetics = cTKE is not None and dSV_dT is not None and dSV_dS is not None
    buoyancy = SkinBuoyFlux is not None
    if buoyancy:
        SkinBuoyFlux[...] = 0.0                                   # :808-809
    if cTKE is not None:
        cTKE[...] = 0.0
    g_Hconv2 = (P.g_Earth_Z_T2 * GV.H_to_RZ) * GV.H_to_RZ
    forcing = fluxes is not None and fluxes.get("sw") is not None
    if not forcing and not energetics:                           # :814
        return 0, 0, 0
    if (energetics or buoyancy) and orc is None:
        from oracle import orc
    H_limit_fluxes = float(_max(GV.Angstrom_H, GV.H_subroundoff))
    h2d, T2d, S2d = h[D3].copy(), T[D3].copy(), S[D3].copy()
    shp = h2d.shape[1:]
    p_surf = tv_p_surf[dom] if tv_p_surf is not None else None
    with np.errstate(all="ignore"):
        if energetics:                                            # :877-897
            pres = p_surf.copy() if p_surf is not None else np.zeros(shp)
            sT, sS = np.empty_like(h2d), np.empty_like(h2d)
            for k in range(nz):
                d_pres = (GV.g_Earth * GV.H_to_RZ) * h2d[k]
                p_lay = pres + 0.5 * d_pres
                pres = pres + d_pres
                sT[k], sS[k] = specvol_derivs(eos, T2d[k], S2d[k], P.RL2_T2_to_Pa * p_lay)
            dSV_dT[D3] = sT; dSV_dS[D3] = sS
            pen_TKE = np.zeros_like(h2d)
            cT = np.zeros_like(h2d)
        if not forcing:                                           # :900
            return 0, 0, 0
        F = lambda n: fluxes[n][dom]
        has = lambda n: fluxes.get(n) is not None
        wet = M[G["mask2dT"]][dom] > 0.0

        # extractFluxes1d
        Ih_limit = 1.0 / H_limit_fluxes if H_limit_fluxes > 0.0 else 0.0
        I_Cp = 1.0 / P.C_p
        I_Cp_Hconvert = 1.0 / (GV.H_to_RZ * P.C_p)
        htot = h2d[0].copy()
        for k in range(1, nz):
            htot = htot + h2d[k]
        T1 = T2d[0].copy()
        red = (Ih_limit > 0.0) & (htot * Ih_limit < 1.0)
        counts["scale_reduced"] += int(red.sum()); counts["scale_full"] += int((~red).sum())
        scale = np.where(red, htot * Ih_limit, 1.0)
        Pen_SW_bnd = np.zeros((max(nsw, 1),) + shp)
        Pen_SW_bnd_rate = np.zeros((max(nsw, 1),) + shp)
        Pen_sw_tot, pen_sw_tot_rate = np.zeros(shp), np.zeros(shp)
        for n in range(nsw):
            top = sw_pen_band[n][dom]
            Pen_SW_bnd[n] = I_Cp_Hconvert * scale * dt * _max(0.0, top)
            Pen_sw_tot = Pen_sw_tot + Pen_SW_bnd[n]
            Pen_SW_bnd_rate[n] = I_Cp_Hconvert * scale * _max(0.0, top)
            pen_sw_tot_rate = pen_sw_tot_rate + Pen_SW_bnd_rate[n]
        water = ((((((((F("lprec") + F("fprec")) + F("evap")) + F("lrunoff")) + F("lrunoff_glc")) + F("vprec")) +
                   F("seaice_melt")) + F("frunoff")) + F("frunoff_glc"))
        netMassInOut = dt * (scale * water)
        netMassInOut_rate = (scale * water)
        netMassOut = np.zeros(shp)
        for n, arm in (("evap", "massout_evap"), ("lprec", "massout_lprec"), ("seaice_melt", "massout_seaice"), ("vprec", "massout_vprec")):
            neg = F(n) < 0.0
            counts[arm] += int(neg.sum())
            netMassOut = np.where(neg, netMassOut + F(n), netMassOut)
        netMassOut = dt * scale * netMassOut
        netMassInOut = GV.RZ_to_H * netMassInOut
        netMassInOut_rate = GV.RZ_to_H * netMassInOut_rate
        netMassOut = GV.RZ_to_H * netMassOut
        if has("seaice_melt_heat"):
            rad = F("sw") + (((F("lw") + F("latent")) + F("sens")) + F("seaice_melt_heat"))
        else:
            rad = F("sw") + ((F("lw") + F("latent")) + F("sens"))
        net_heat = scale * dt * I_Cp_Hconvert * rad
        net_heat_rate = scale * I_Cp_Hconvert * rad
        if has("heat_added"):
            net_heat = net_heat + (scale * (dt * I_Cp_Hconvert)) * F("heat_added")
            net_heat_rate = net_heat_rate + (scale * I_Cp_Hconvert) * F("heat_added")
        TempxPmE = F("TempxPmE").copy() if has("TempxPmE") else None
        for on, arm, names in ((P.use_river_heat_content, "river_heat", ("lrunoff", "lrunoff_glc")),
                               (P.use_calving_heat_content, "calving_heat", ("frunoff", "frunoff_glc"))):
            if not on:
                continue
            counts[arm] += int(np.prod(shp))
            for n in names:                                       # the _rate twin is left out on purpose (:724-728, :745-749)
                hc = F("heat_content_" + n)
                net_heat = (net_heat + (scale * (dt * I_Cp_Hconvert)) * hc) - (GV.RZ_to_H * (scale * dt)) * F(n) * T1
                if TempxPmE is not None:
                    TempxPmE = TempxPmE + (scale * dt) * (I_Cp * hc - F(n) * T1)
        net_heat = net_heat - Pen_sw_tot
        net_heat_rate = net_heat_rate - pen_sw_tot_rate
        nonpenSW = scale * dt * I_Cp_Hconvert * F("sw") - Pen_sw_tot
        net_salt, net_salt_rate = np.zeros(shp), np.zeros(shp)
        if has("salt_flux"):
            net_salt = (scale * dt * (1000.0 * P.ppt_to_S * F("salt_flux"))) * GV.RZ_to_H
            net_salt_rate = (scale * 1. * (1000.0 * P.ppt_to_S * F("salt_flux"))) * GV.RZ_to_H
        hc_in, hc_out = np.zeros(shp), np.zeros(shp)
        if aggregate_FW_forcing:
            isin = netMassInOut > 0.0
            hc_in = np.where(isin, -P.C_p * netMassOut * T1 * GV.H_to_RZ / dt, P.C_p * (netMassInOut - netMassOut) * T1 * GV.H_to_RZ / dt)
            hc_out = np.where(isin, P.C_p * netMassOut * T1 * GV.H_to_RZ / dt, -P.C_p * (netMassInOut - netMassOut) * T1 * GV.H_to_RZ / dt)
        for n, src in (("heat_content_lprec", "lprec"), ("heat_content_fprec", "fprec"), ("heat_content_vprec", "vprec"),
                       ("heat_content_cond", "evap")):
            if has(n):
                fluxes[n][dom] = np.where(F(src) > 0.0, P.C_p * F(src) * T1, 0.0)
        if not P.use_river_heat_content:
            for n in ("lrunoff", "lrunoff_glc"):
                if has("heat_content_" + n):
                    fluxes["heat_content_" + n][dom] = P.C_p * F(n) * T1
        if not P.use_calving_heat_content:
            for n in ("frunoff", "frunoff_glc"):
                if has("heat_content_" + n):
                    fluxes["heat_content_" + n][dom] = P.C_p * F(n) * T1

        # MOM_diabatic_aux.F90:968-983
        if aggregate_FW_forcing:
            counts["agg_fw"] += int(np.prod(shp))
            netMassOut = netMassInOut.copy()
            netMassIn = np.zeros(shp)
        else:
            counts["split_fw"] += int(np.prod(shp))
            netMassIn = netMassInOut - netMassOut
        if has("netMassOut"):
            fluxes["netMassOut"][dom] = np.where(wet, netMassOut, 0.0)
        if has("netMassIn"):
            fluxes["netMassIn"][dom] = np.where(wet, netMassIn, 0.0)
        netHeat, netSalt = net_heat, net_salt

        def mass_diags(Tk, dThickness):                           # :1021-1030, :1134-1143
            nonlocal hc_in, hc_out, TempxPmE
            hc_in = np.where(wet, hc_in + Tk * _max(0., dThickness) * GV.H_to_RZ * P.C_p * Idt, hc_in)
            hc_out = np.where(wet, hc_out + Tk * _min(0., dThickness) * GV.H_to_RZ * P.C_p * Idt, hc_out)
            if TempxPmE is not None:
                TempxPmE = np.where(wet, TempxPmE + Tk * dThickness * GV.H_to_RZ, TempxPmE)

        # A/ :1005-1073
        k = 0
        dThickness = netMassIn.copy()
        dTemp = np.zeros(shp)
        netMassIn = np.where(wet, netMassIn - dThickness, netMassIn)
        Temp_in, Salin_in = T2d[k].copy(), 0.0
        dTemp = dTemp + dThickness * Temp_in
        mass_diags(T2d[k], dThickness)
        if energetics and P.do_rivermix:
            counts["rivermix"] += int(wet.sum())
            RivermixConst = -0.5 * (P.rivermix_depth * dt) * P.g_Earth_Z_T2 * GV.Rho0
            cT[k] = np.where(wet, cT[k] + _max(0.0, RivermixConst * sS[0] * ((F("lrunoff") + F("frunoff")) +
                                                                             (F("lrunoff_glc") + F("frunoff_glc"))) * S2d[0]), cT[k])
        hOld = h2d[k].copy()
        hnew = hOld + dThickness
        pos = wet & (hnew > 0.0)
        if energetics:
            ae = pos & (dThickness > 0.)
            counts["a_energetics"] += int(ae.sum())
            cT[k] = np.where(ae, cT[k] + 0.5 * g_Hconv2 * (hOld * dThickness) *
                             ((T2d[k] - Temp_in) * sT[k] + (S2d[k] - Salin_in) * sS[k]), cT[k])
        Ithickness = 1.0 / np.where(pos, hnew, 1.0)
        T2d[k] = np.where(pos & ((dThickness != 0.) | (dTemp != 0.)), (hOld * T2d[k] + dTemp) * Ithickness, T2d[k])
        S2d[k] = np.where(pos & (dThickness != 0.), (hOld * S2d[k] + 0.) * Ithickness, S2d[k])
        h2d[k] = np.where(wet, hnew, hOld)

        # B/ :1077-1175
        negative = np.zeros(shp, bool)
        for k in range(nz):
            IforcingDepthScale = 1. / _max(GV.H_subroundoff, minimum_forcing_depth - netMassOut)
            fractionOfForcing = _min(1.0, h2d[k] * IforcingDepthScale)
            counts["b_thin_layer"] += int((wet & (fractionOfForcing < 1.0)).sum())
            cfl = -fractionOfForcing * netMassOut > evap_CFL_limit * h2d[k]
            counts["b_cfl_limited"] += int((wet & cfl).sum())
            fractionOfForcing = np.where(cfl, -evap_CFL_limit * h2d[k] / np.where(cfl, netMassOut, 1.0), fractionOfForcing)
            dThickness = _max(fractionOfForcing * netMassOut, -h2d[k])
            dTemp = fractionOfForcing * netHeat
            slim = -P.dSalt_frac_max * h2d[k] * S2d[k]
            counts["b_dsalt_limited"] += int((wet & (slim > fractionOfForcing * netSalt)).sum())
            dSalt = _max(fractionOfForcing * netSalt, slim)
            netMassOut = np.where(wet, netMassOut - dThickness, netMassOut)
            netHeat = np.where(wet, netHeat - dTemp, netHeat)
            netSalt = np.where(wet, netSalt - dSalt, netSalt)
            dTemp = dTemp + dThickness * T2d[k]
            mass_diags(T2d[k], dThickness)
            hOld = h2d[k].copy()
            hnew = hOld + dThickness
            pos = wet & (hnew > 0.)
            counts["b_layer_emptied"] += int((wet & (hnew == 0.)).sum())
            neg = wet & (hnew < 0.)
            counts["b_negative_h"] += int(neg.sum())
            negative |= neg
            if energetics:
                cT[k] = np.where(pos, cT[k] - (0.5 * hnew * g_Hconv2) * ((dTemp - dThickness * T2d[k]) * sT[k] +
                                                                        (dSalt - dThickness * S2d[k]) * sS[k]), cT[k])
            Ithickness = 1.0 / np.where(pos, hnew, 1.0)
            T2d[k] = np.where(pos, (hOld * T2d[k] + dTemp) * Ithickness, T2d[k])
            S2d[k] = np.where(pos, (hOld * S2d[k] + dSalt + 0.0) * Ithickness, S2d[k])
            h2d[k] = np.where(wet, hnew, hOld)

        # :1178-1203
        land = ~wet & ((np.abs(netHeat) + np.abs(netSalt) + np.abs(netMassIn) + np.abs(netMassOut)) > 0.)
        counts["land_flux"] += int(land.sum())
        n_land = 0 if P.ignore_fluxes_over_land else int(land.sum())
        grounded = (netMassIn + netMassOut) != 0.0
        counts["grounding"] += int(grounded.sum())
        if createdH is not None:
            createdH[dom] = np.where(grounded, 0. - (netMassIn + netMassOut) / dt, 0.)

        # C/ :1213-1233
        T_before = T2d.copy()
        opac = None
        if nsw > 0:
            opac = np.stack([opacity_band[n][D3] for n in range(nsw)])
        absorbRemainingSW(GV, P, h2d, opac, nsw, dt, H_limit_fluxes, T2d, Pen_SW_bnd, TKE=pen_TKE if energetics else None,
                          dSV_dT=sT if energetics else None, counts=counts)
        if energetics:
            cTKE[D3] = cT + pen_TKE
        # D/ :1238-1272
        h[D3] = h2d; T[D3] = T2d; S[D3] = S2d
        if penSW_diag is not None:
            conv = (T2d - T_before) * h2d * Idt * P.C_p * GV.H_to_RZ
            penSW_diag[D3] = conv
            if penSWflux_diag is not None:
                flux = np.zeros((nz + 1,) + shp)
                for k in range(nz - 1, -1, -1):
                    flux[k] = conv[k] + flux[k + 1]
                penSWflux_diag[D3] = flux
        if nonpenSW_diag is not None:
            nonpenSW_diag[dom] = nonpenSW * Idt * P.C_p * GV.H_to_RZ
        if has("heat_content_massin"):
            fluxes["heat_content_massin"][dom] = hc_in
        if has("heat_content_massout"):
            fluxes["heat_content_massout"][dom] = hc_out
        if TempxPmE is not None:
            fluxes["TempxPmE"][dom] = TempxPmE

        # SkinBuoyFlux :1279-1318, the Boussinesq arm
        if buoyancy:
            netPen_rate = np.zeros(shp)
            for n in range(nsw):
                netPen_rate = netPen_rate + Pen_SW_bnd_rate[n]
            SurfPressure = p_surf if p_surf is not None else np.zeros(shp)
            GoRho = P.g_Earth_Z_T2 / GV.Rho0
            dRhodT, dRhodS = _derivs(orc, eos, T2d[0], S2d[0], P.RL2_T2_to_Pa * SurfPressure)
            SkinBuoyFlux[dom] = -GoRho * GV.H_to_Z * (dRhodS * (net_salt_rate - S2d[0] * netMassInOut_rate) +
                                                      dRhodT * (net_heat_rate + netPen_rate))
    return int(grounded.sum()), int(negative.sum()), n_land


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_diabatic_aux_cpu.py and tests/test_diabatic_aux_gpu.py

def _ij(d):
    il = (np.arange(d.pitch) - d.ioff + d.i_glob0)[None, :] * np.ones(d.shape2(), int)
    jl = (np.arange(d.shape2()[0]) - d.joff + d.j_glob0)[:, None] * np.ones(d.shape2(), int)
    return il, jl


def inputs(d, M, GV, seed=5, nsw=0, opacity="zero", dt=3600.0, land_fluxes=False, dry=True, ground=True, thin=True, thin_min=0.0):
    """h, T, S, tv_p_surf, every plane of `forcing` and the optics arrays on a tile, every field laid in global coordinates.
    h: the bowl's layers with, in bands of columns, one to three thin surface layers of 1e-10 .. 1e-3 m (among them 3e-10 m,
    between h_min_heat and twice that), vanished layers (h = 0) at depth and at the surface and, with `dry`, a patch of nearly
    dry columns (one layer of 0.5e-10 or 2.2e-10 m over vanished ones).  The water fluxes have both signs; with `ground` a patch
    evaporates more than its columns hold.  Heat fluxes of both signs; salt_flux strong enough to fire the dSalt limiter in the
    thin layers; runoff with its heat content.  Unless `land_fluxes`, every flux and sw_pen_band are zero over land.
    sw_pen_band: 0..4 bands, mostly positive, negative in a patch, and dim (1e-3 .. 1e-9 W m-2) in another.
    thin_min: the thin layers that are not vanished are at least this thick (the exp cases, see CASES).
    opacity: "zero" (exp(-0) = 1: everything reaches the bottom), "huge" (0 in layers thinner than 0.05 m, 1e6 m-1 in the others:
    the first thick layer takes everything), "mixed" (alternating by band and by rows), or "real" (0.05 .. 3 m-1: the exp cases)."""
    from mom6_amd import synth
    nk = d.nk
    h, _, _ = synth.make_state(d, M, seed=20250808 + seed, u_max=0.3, h_pert=0.01)
    il, jl = _ij(d)
    wetp = M[G["mask2dT"]] > 0.0
    sf = lambda n, **kw: synth.smooth_field(d, seed + n, ox=0.5, oy=0.5, **kw)
    if thin:
        thins = (1.0e-10, 3.0e-10, 1.0e-9, 1.0e-7, 1.0e-5, 1.0e-4, 1.0e-3, 0.0)
        thins = tuple(th if th == 0.0 else max(th, thin_min) for th in thins)
        for m, th in enumerate(thins):                            # columns il % 11 == m of every third row band
            sel = wetp & (il % 11 == m) & (jl % 3 != 0)
            for k in range(min(1 + m % 3, nk - 1) if nk > 1 else 0):
                h[k] = np.where(sel, th, h[k])
        if nk > 2:                                                # vanished layers at depth
            h[nk - 2] = np.where(wetp & (il % 7 == 3), 0.0, h[nk - 2])
    if dry:
        for m, th in enumerate((0.5e-10, 2.2e-10)):
            sel = wetp & (il >= 5 + 3 * m) & (il <= 6 + 3 * m) & (jl >= 5) & (jl <= 7)
            h[0] = np.where(sel, th, h[0])
            for k in range(1, nk):
                h[k] = np.where(sel, 0.0, h[k])
    pT, pS = sf(10), sf(11)
    T = np.zeros_like(h); S = np.zeros_like(h)
    for k in range(nk):
        zf = k / max(nk - 1, 1)
        T[k] = 20.0 - 15.0 * zf + 0.8 * pT * (1.0 - 0.5 * zf)
        S[k] = 34.5 + 1.0 * zf + 0.2 * pS * (1.0 - 0.5 * zf)
    out = dict(h=h, T=T, S=S, tv_p_surf=2.0e4 * (1.0 + 0.2 * sf(21)))
    fl = {}
    fl["sw"] = 150.0 * (1.0 + sf(30))
    fl["lw"] = -60.0 * (1.0 + 0.3 * sf(31))
    fl["latent"] = -90.0 * (1.0 + 0.8 * sf(32))
    fl["sens"] = 15.0 * sf(33)
    fl["evap"] = 1.0e-4 * (sf(34) - 0.3)
    fl["lprec"] = 8.0e-5 * (sf(35) + 0.2)
    fl["fprec"] = 1.0e-5 * np.abs(sf(36))
    fl["vprec"] = 2.0e-5 * sf(37)
    fl["lrunoff"] = 3.0e-5 * np.maximum(sf(38), 0.0)
    fl["frunoff"] = 1.0e-5 * np.maximum(sf(39), 0.0)
    fl["lrunoff_glc"] = 4.0e-6 * np.maximum(sf(40), 0.0)
    fl["frunoff_glc"] = 2.0e-6 * np.maximum(sf(41), 0.0)
    fl["seaice_melt"] = 3.0e-5 * sf(42)
    fl["seaice_melt_heat"] = 20.0 * sf(43)
    fl["heat_added"] = 30.0 * sf(44)
    fl["salt_flux"] = 1.0e-4 * sf(45)
    C_p = 3991.86795711963
    for n in ("lrunoff", "lrunoff_glc", "frunoff", "frunoff_glc"):
        fl["heat_content_" + n] = C_p * fl[n] * (T[0] - 2.0)
    if ground:                                                    # more evaporation than the columns hold
        sel = wetp & (il >= 20) & (il <= 22) & (jl >= 16) & (jl <= 17)
        fl["evap"] = np.where(sel, -3.0 * GV.H_to_RZ * h.sum(axis=0) / dt, fl["evap"])
    pen = []
    for n in range(nsw):
        b = fl["sw"] * (0.25 / (n + 1)) * (1.0 + 0.3 * sf(50 + n))
        b = np.where((il >= 20) & (il <= 23) & (jl >= 3) & (jl <= 5), -1.0, b)                        # max(0, .)
        dim = (il >= 26) & (il <= 33) & (jl >= 8) & (jl <= 14)
        b = np.where(dim, 10.0 ** (-3.0 - 6.0 * ((il - 26) + 8 * (jl - 8)) / 56.0), b)
        pen.append(b)
    if not land_fluxes:
        for n in fl:
            fl[n] = np.where(wetp, fl[n], 0.0)
        pen = [np.where(wetp, b, 0.0) for b in pen]
    out["sw_pen_band"] = np.stack(pen) if nsw else None
    if nsw:
        op = np.zeros((nsw, nk) + d.shape2())
        thick = h >= 0.05
        for n in range(nsw):
            if opacity == "huge":
                op[n] = np.where(thick, 1.0e6, 0.0)
            elif opacity == "mixed":
                op[n] = np.where(thick & (((jl // 4) + n) % 2 == 0)[None], 1.0e6, 0.0)
            elif opacity == "real":
                op[n] = (0.05 + 2.95 * n / max(nsw - 1, 1)) * (1.0 + 0.2 * synth.smooth_field(d, seed + 60 + n, nk=nk, ox=0.5, oy=0.5))
        out["opacity_band"] = op
    else:
        out["opacity_band"] = None
    out = {n: (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None) for n, a in out.items()}
    out["fluxes"] = {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in fl.items()}
    return out


_DIAG = ("createdH", "penSW_diag", "penSWflux_diag", "nonpenSW_diag")
_ALL_FLUX_OUT = FLUX_OUT + ("TempxPmE",)
_EXP_INP = dict(thin_min=1.0e-4, dry=False)
# case -> (params members, options).  Options: eos (an EOS form or None), nsw, opacity, ener (cTKE, dSV_dT, dSV_dS given), buoy
# (SkinBuoyFlux given), agg, p_surf (tv%p_surf given), given (nullable input planes handed in), fout (output planes of `forcing`
# handed in), diag, cfl (evap_CFL_limit), depth (minimum_forcing_depth), inp (keyword arguments of inputs())
CASES = {
    "plain": ({}, dict(nsw=0, agg=True)),
    "split": ({}, dict(nsw=0, agg=False, fout=_ALL_FLUX_OUT, given=("salt_flux",), diag=("createdH", "nonpenSW_diag"))),
    "linear_e": ({}, dict(eos=abi.LINEAR, nsw=1, opacity="huge", ener=True, buoy=True, agg=True, p_surf=True, fout=("netMassIn", "netMassOut"))),
    "wright_3": (dict(do_rivermix=1, rivermix_depth=40.0),
                 dict(eos=abi.WRIGHT, nsw=3, opacity="mixed", ener=True, buoy=True, agg=False, given=("salt_flux", "heat_added"),
                      fout=_ALL_FLUX_OUT, diag=_DIAG)),
    "wright_full_4": (dict(use_river_heat_content=1, use_calving_heat_content=1),
                      dict(eos=abi.WRIGHT_FULL, nsw=4, opacity="huge", ener=True, buoy=False, agg=True, p_surf=True,
                           given=("seaice_melt_heat", "salt_flux") + abi.SURFACE_FLUXES_RUNOFF_HEAT, fout=_ALL_FLUX_OUT, diag=("penSW_diag",))),
    "wright_red_old": (dict(optics_answer_date=20181231),
                       dict(eos=abi.WRIGHT_REDUCED, nsw=3, opacity="mixed", ener=True, buoy=True, agg=False, given=("salt_flux",),
                            fout=abi.SURFACE_FLUXES_RUNOFF_HEAT + ("heat_content_massin", "heat_content_massout"), diag=_DIAG)),
    "roquet_spv": ({}, dict(eos=abi.ROQUET_SPV, nsw=1, opacity="zero", ener=True, buoy=True, agg=True, p_surf=True, cfl=1.0)),
    "buoy_only": ({}, dict(eos=abi.UNESCO, nsw=3, opacity="zero", ener=False, buoy=True, agg=False, given=("salt_flux",), diag=_DIAG)),
    "no_eos_old": (dict(optics_answer_date=20181231), dict(nsw=4, opacity="mixed", agg=True, diag=("penSW_diag", "penSWflux_diag"))),
    "land": (dict(ignore_fluxes_over_land=1), dict(eos=abi.WRIGHT, nsw=1, opacity="zero", ener=True, buoy=True, agg=True,
                                                     inp=dict(land_fluxes=True), diag=("createdH",))),
    # The cases that evaluate exp with an argument other than 0 or below -750.  Their thin layers are 1e-4 m and more, and they
    # have no nearly dry columns: the heating of a layer is Pen*(1 - exp(-h*opacity))/h, and 1 - exp(-x) turns a difference of one
    # unit in the last place of exp into a relative difference of 2.2e-16/x.  Two correct exp functions may differ by two such
    # units, Pen is up to 0.16 degC m here (dt*sw_pen/(Rho0*C_p), three bands), so T of a layer of thickness h may differ by
    # 0.16*4.4e-16/h: within 1e-12 of the range of T (15 degC and more) only for h above 5e-6 m -- whatever computes the exp.
    # (Seen on the device with the 1e-10 m layers in: 2.5e-11 of range in T, every other field below 3e-16.)  The thinner layers
    # have their bit-for-bit coverage in the exp-free cases, where their optical depth is exactly 0.
    "real_3": (dict(do_rivermix=1, rivermix_depth=40.0),
               dict(eos=abi.WRIGHT, nsw=3, opacity="real", ener=True, buoy=True, agg=False, given=("salt_flux",), fout=_ALL_FLUX_OUT, diag=_DIAG,
                    inp=_EXP_INP)),
    "real_old_1": (dict(optics_answer_date=20181231), dict(eos=abi.LINEAR, nsw=1, opacity="real", ener=True, agg=True, diag=("penSW_diag",),
                                                           inp=_EXP_INP)),
    "real_4": ({}, dict(nsw=4, opacity="real", agg=True, diag=_DIAG, inp=_EXP_INP)),
}
CASES_EXP = ("real_3", "real_old_1", "real_4")
CASES_EXP_FREE = tuple(n for n in CASES if n not in CASES_EXP)


def case(name, GV):
    """(params, EOS or None, options)"""
    mods, opt = CASES[name]
    opt = dict(dict(eos=None, nsw=0, opacity="zero", ener=False, buoy=False, agg=True, p_surf=False, given=(), fout=(), diag=(),
                    cfl=0.8, depth=0.001, inp={}, dt=3600.0), **opt)
    P = abi.diabatic_aux_params_default(GV, **mods)
    eos = abi.eos_params_default(opt["eos"]) if opt["eos"] is not None else None
    return P, eos, opt


def case_inputs(d, M, GV, opt, **kw):
    return inputs(d, M, GV, nsw=opt["nsw"], opacity=opt["opacity"], dt=opt["dt"], **dict(opt["inp"], **kw))


def outputs(d, opt, fill=np.nan):
    """The optional outputs of a case, filled with `fill`."""
    out = {}
    if opt["ener"]:
        for n in ("cTKE", "dSV_dT", "dSV_dS"):
            out[n] = np.full(d.shape3(), fill)
    if opt["buoy"]:
        out["SkinBuoyFlux"] = np.full(d.shape2(), fill)
    for n in opt["diag"]:
        out[n] = np.full(d.shape3(d.nk + 1) if n == "penSWflux_diag" else d.shape3() if n == "penSW_diag" else d.shape2(), fill)
    return out


def flux_planes(d, opt, inp, fill=np.nan, forcing=True):
    """The `forcing` of a case: the required planes, the nullable inputs the case hands in, and its output planes filled with
    `fill` (tv%TempxPmE with 0: the caller zeroes it).  The runoff heat contents are inputs where the case gives them, outputs
    where it asks for them."""
    if not forcing:
        return None
    f = {n: inp["fluxes"][n].copy() for n in FLUX_REQUIRED + tuple(opt["given"])}
    for n in opt["fout"]:
        if n not in f:
            f[n] = np.full(d.shape2(), 0.0 if n == "TempxPmE" else fill)
    return f


def run(d, M, GV, P, eos, opt, inp, fill=np.nan, counts=None, orc=None, ncalls=1, forcing=True):
    """applyBoundaryFluxesInOut of a case on copies of the numpy inputs, `ncalls` times in a row on the same arrays.  Returns
    (state: h, T, S and every output and output plane by name, status summed over the calls, counts)."""
    counts = counts if counts is not None else dict.fromkeys(BRANCHES, 0)
    st = dict(h=inp["h"].copy(), T=inp["T"].copy(), S=inp["S"].copy())
    out = outputs(d, opt, fill)
    f = flux_planes(d, opt, inp, fill, forcing)
    status = np.zeros(3, int)
    for _ in range(ncalls):
        status += applyBoundaryFluxesInOut(d, M, GV, P, opt["dt"], f, st["h"], st["T"], st["S"], nsw=opt["nsw"],
                                           opacity_band=inp["opacity_band"], sw_pen_band=inp["sw_pen_band"],
                                           tv_p_surf=inp["tv_p_surf"] if opt["p_surf"] else None, aggregate_FW_forcing=opt["agg"],
                                           evap_CFL_limit=opt["cfl"], minimum_forcing_depth=opt["depth"], eos=eos, orc=orc,
                                           counts=counts, **out)
    st.update(out)
    if f is not None:
        st.update({"fluxes." + n: f[n] for n in opt["fout"]})
    return st, tuple(int(v) for v in status), counts
