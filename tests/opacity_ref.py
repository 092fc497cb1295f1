"""The checker of mom6x_opacity_init and mom6x_set_pen_shortwave: a numpy restatement of set_pen_shortwave
(src/parameterizations/vertical/MOM_diabatic_aux.F90:621-677), set_opacity (src/parameterizations/vertical/MOM_opacity.F90:118-240),
opacity_from_chl (:245-477), opacity_morel and SW_pen_frac_morel (:481-513), lookup_ohlmann_swpen and lookup_ohlmann_opacity
(:1433-1485), the parts of opacity_init that turn parameters into coefficients (:1151-1160, :1243-1283), init_ohlmann_table
(:1321-1430) and the one product of extract_optics_slice (:559).  Arrays are in the pitched tile layout of include/mom6x.h
([k, j + joff, i + ioff], bands first); outputs are written on the computational domain only.

The opacities are evaluated layer by layer as the reference does, not once per column as the device does with chl_2d, so the two
orders check each other.  The arithmetic is the reference's, operation for operation.  The Ohlmann table is built with the C
library's log10 and pow (math.log10, math.pow), as the host side of the device builds it.  `counts` (BRANCHES) records how often
each arm fired; `ohlmann_near_half` counts the lookups whose real-valued index lies within 1e-6 of a half-integer, where the
nearest-neighbour lookup could go either way between two log10 functions.

Where the reference stops on a negative chlorophyll at a wet point (MOM_diabatic_aux.F90:649, MOM_opacity.F90:328, :338) the
restatement counts and stores what the formulas give, as the device does; set_pen_shortwave returns the count.

The case table has two classes.  EXACT: chlorophyll of 0.0 and 1.0 only (1.0 only for MOREL_88, whose clamp turns 0 into
log10(0.02)), for which pow and log10 are exact on both sides, and the chlorophyll-free schemes: bit for bit, except opac_diag
(a tanh).  TRANSCENDENTAL: smooth chlorophyll of 0.01 .. 20 mg m-3, held to 1e-12 of each field's range."""
import math

import numpy as np

from mom6_amd import abi
from tests.ref_common import _max, _min

G = abi.G
MANIZZA, MOREL, SINGLE_EXP, DOUBLE_EXP, OHLMANN = (abi.OPACITY_MANIZZA_05, abi.OPACITY_MOREL_88, abi.OPACITY_SINGLE_EXP,
                                                   abi.OPACITY_DOUBLE_EXP, abi.OPACITY_OHLMANN_03)
CHL_SCHEMES = (MANIZZA, MOREL, OHLMANN)
BRANCHES = ("sch_manizza", "sch_morel", "sch_ohlmann", "sch_single_exp", "sch_double_exp", "chl_2d", "chl_3d", "chl_none",
            "init_band_ge_4", "init_chl_indep_band", "init_coef_folded",
            "man_vis_multiband", "man_vis_from_total", "man_vis_none", "man_nir_multiband", "man_nir_from_total", "man_nir_none",
            "man_pen_wet", "man_pen_land", "man_band_2", "man_band_nir", "man_op_land", "man_op_wet", "man_op_chl_dep", "man_op_chl_indep",
            "morel_multiband", "morel_from_total", "morel_none", "morel_pen_wet", "morel_pen_land", "morel_op_wet", "morel_op_land",
            "morel_more_bands",
            "ohl_multiband", "ohl_from_total", "ohl_pen_wet", "ohl_pen_land", "ohl_op_wet", "ohl_op_land", "ohl_below_table",
            "ohl_in_table",
            "exp_pen_zero", "exp_pen_set", "diag_sw_pen", "diag_vis_manizza", "diag_vis_all", "diag_opac", "negative_chl",
            "ohlmann_near_half")
NLUT = 401


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


def _count(counts, name, mask=True):
    if counts is not None:
        counts[name] += int(np.count_nonzero(mask))


def _dom(d):
    return d.sl(0, d.ni - 1, 0, d.nj - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# opacity_init

_CHL_T = (.001, .005, .01, .02, .03, .05, .10, .15, .20, .25, .30, .35, .40, .45, .50, .60,
          .70, .80, .90, 1.00, 1.50, 2.00, 2.50, 3.00, 4.00, 5.00, 6.00, 7.00, 8.00, 9.00, 10.00)
# Ohlmann (2003) Table 1a with the additional values used by CESM-POP: A1, A2, B1, B2
_TAB = ((0.4421, 0.4451, 0.4488, 0.4563, 0.4622, 0.4715, 0.4877, 0.4993, 0.5084, 0.5159, 0.5223, 0.5278, 0.5326, 0.5369, 0.5408, 0.5474,
         0.5529, 0.5576, 0.5615, 0.5649, 0.5757, 0.5802, 0.5808, 0.5788, 0.56965, 0.55638, 0.54091, 0.52442, 0.50766, 0.49110, 0.47505),
        (0.2981, 0.2963, 0.2940, 0.2894, 0.2858, 0.2800, 0.2703, 0.2628, 0.2571, 0.2523, 0.2481, 0.2444, 0.2411, 0.2382, 0.2356, 0.2309,
         0.2269, 0.2235, 0.2206, 0.2181, 0.2106, 0.2089, 0.2113, 0.2167, 0.23357, 0.25504, 0.27829, 0.30274, 0.32698, 0.35056, 0.37303),
        (0.0287, 0.0301, 0.0319, 0.0355, 0.0384, 0.0434, 0.0532, 0.0612, 0.0681, 0.0743, 0.0800, 0.0853, 0.0902, 0.0949, 0.0993, 0.1077,
         0.1154, 0.1227, 0.1294, 0.1359, 0.1640, 0.1876, 0.2082, 0.2264, 0.25808, 0.28498, 0.30844, 0.32932, 0.34817, 0.36540, 0.38132),
        (0.3192, 0.3243, 0.3306, 0.3433, 0.3537, 0.3705, 0.4031, 0.4262, 0.4456, 0.4621, 0.4763, 0.4889, 0.4999, 0.5100, 0.5191, 0.5347,
         0.5477, 0.5588, 0.5682, 0.5764, 0.6042, 0.6206, 0.6324, 0.6425, 0.66172, 0.68144, 0.70086, 0.72144, 0.74178, 0.76190, 0.78155))


def ohlmann_table():
    """init_ohlmann_table :1321-1430: (lut[4, 401] = a1, a2, b1, b2; chl_min, log10chl_min, log10chl_max, dlog10chl)."""
    nt = len(_CHL_T)
    log10chl_min = math.log10(_CHL_T[0])
    log10chl_max = math.log10(_CHL_T[nt - 1])
    dlog10chl = (log10chl_max - log10chl_min) / (NLUT - 1)
    lut = np.zeros((4, NLUT))
    m = 1
    for n in range(NLUT):
        log10chl_lut = log10chl_min + n * dlog10chl
        chl = math.pow(10.0, log10chl_lut)
        chl = max(_CHL_T[0], min(chl, _CHL_T[nt - 1]))
        while chl > _CHL_T[m]:
            m += 1
        w2 = (chl - _CHL_T[m - 1]) / (_CHL_T[m] - _CHL_T[m - 1])
        w1 = 1. - w2
        for t in range(4):
            lut[t, n] = w1 * _TAB[t][m - 1] + w2 * _TAB[t][m]
    return lut, _CHL_T[0], log10chl_min, log10chl_max, dlog10chl


def init(P, GV, counts=None):
    """What opacity_init leaves in opacity_CS and optics_type; ValueError where the reference (:1151-1160) or the device refuses."""
    sch, nb = P.opacity_scheme, P.nbands
    if sch not in (MANIZZA, MOREL, SINGLE_EXP, DOUBLE_EXP, OHLMANN):
        raise ValueError("opacity_scheme is not valid")
    if nb < 0:
        raise ValueError("negative nbands")
    if (sch == DOUBLE_EXP and nb != 2) or (sch == SINGLE_EXP and nb != 1) or (sch == OHLMANN and nb != 2):
        raise ValueError("band-count rule")
    if nb > 4:
        raise ValueError("more than 4 bands")
    CS = dict(scheme=sch, nbands=nb, P=P, GV=GV, chl_dep_bands=0)
    if sch == MANIZZA:   # :1246-1269
        c1, c2, pw = np.zeros(max(nb, 1)), np.zeros(max(nb, 1)), np.zeros(max(nb, 1))
        for n in range(min(3, nb)):
            c1[n] = P.manizza_coef[2 * n]; c2[n] = P.manizza_coef[2 * n + 1]; pw[n] = P.manizza_power[n]
        for n in range(3, nb):
            c1[n] = c1[n - 1]; c2[n] = c2[n - 1]; pw[n] = pw[n - 1]
            _count(counts, "init_band_ge_4")
        dep = nb
        for n in range(nb - 1, -1, -1):
            if pw[n] != 0.0:
                break
            dep = n
        for n in range(dep, nb):
            _count(counts, "init_chl_indep_band")
            if c2[n] != 0.0:
                _count(counts, "init_coef_folded")
                c1[n] = c1[n] + c2[n]; c2[n] = 0.0
        CS.update(c1=c1, c2=c2, pw=pw, chl_dep_bands=dep)
    elif sch == MOREL:
        CS.update(mo=np.array(P.morel_coef[:]), mp=np.array(P.morel_pen_coef[:]))
    elif sch == OHLMANN:
        lut, chl_min, lmin, lmax, dl = ohlmann_table()
        CS.update(lut=lut, chl_min=chl_min, log10chl_min=lmin, log10chl_max=lmax, dlog10chl=dl)
    return CS


# ------------------------------------------------------------------------------------------------------------------------------
# the functions of chlorophyll

def _morel_poly(c, chl_data):
    Chl = np.log10(_min(_max(chl_data, 0.02), 60.0)); Chl2 = Chl * Chl   # :488, :509
    return (c[0] + c[1] * Chl) + Chl2 * ((c[2] + Chl * c[3]) + Chl2 * (c[4] + Chl * c[5]))


def opacity_morel(chl_data, CS):
    return 1.0 / _morel_poly(CS["mo"], chl_data)   # :490-492


def SW_pen_frac_morel(chl_data, CS):
    return 1.0 - _morel_poly(CS["mp"], chl_data)   # :510-512


def ohlmann_index(chl, CS, counts=None, where=None):
    """The 0-based table entry of :1447-1453 (nint rounds a half away from zero) for an array of chlorophyll."""
    with np.errstate(invalid="ignore", divide="ignore"):
        inside = chl > CS["chl_min"]
        log10chl = np.where(inside, _min(np.log10(np.where(inside, chl, 1.0)), CS["log10chl_max"]), CS["log10chl_min"])
    x = (log10chl - CS["log10chl_min"]) / CS["dlog10chl"]
    fl = np.floor(x)
    fr = x - fl
    sel = np.ones(x.shape, bool) if where is None else where
    _count(counts, "ohlmann_near_half", sel & (np.abs(fr - 0.5) < 1.0e-6))
    _count(counts, "ohl_below_table", sel & ~inside)
    _count(counts, "ohl_in_table", sel & inside)
    return (fl + (fr >= 0.5)).astype(int)


# ------------------------------------------------------------------------------------------------------------------------------
# set_pen_shortwave with set_opacity

def set_pen_shortwave(d, M, CS, opacity_band, sw_pen_band, sw=None, sw_vis_dir=None, sw_vis_dif=None, sw_nir_dir=None, sw_nir_dif=None,
                      chl_2d=None, chl_3d=None, opacity_scale=1.0, SW_pen=None, SW_vis_pen=None, opac_diag=None, counts=None):
    """Writes opacity_band [nbands, nk, j, i] (times opacity_scale), sw_pen_band [nbands, j, i] and the diagnostics given, on
    the computational domain; returns the number of wet points with negative chlorophyll."""
    P, GV, sch, nb = CS["P"], CS["GV"], CS["scheme"], CS["nbands"]
    if chl_2d is not None and chl_3d is not None:
        raise ValueError("both chl_2d and chl_3d")
    has_chl = chl_2d is not None or chl_3d is not None
    if (sch in CHL_SCHEMES) != has_chl:
        raise ValueError("scheme / chlorophyll mismatch")
    multiband_vis_input = sw_vis_dir is not None and sw_vis_dif is not None
    multiband_nir_input = sw_nir_dir is not None and sw_nir_dif is not None
    total_sw_input = sw is not None
    if sch == OHLMANN and not ((multiband_vis_input and multiband_nir_input) or (not multiband_vis_input and total_sw_input)):
        raise ValueError("No shortwave input was provided.")
    if nb == 0:
        return 0
    dom = _dom(d)
    nz = d.nk
    mask = M[G["mask2dT"]][dom]
    sh = mask.shape
    wet, zero = mask > 0.0, np.zeros(sh)
    get = lambda a: a[dom]
    _count(counts, {MANIZZA: "sch_manizza", MOREL: "sch_morel", OHLMANN: "sch_ohlmann", SINGLE_EXP: "sch_single_exp",
                    DOUBLE_EXP: "sch_double_exp"}[sch])
    _count(counts, "chl_3d" if chl_3d is not None else "chl_2d" if chl_2d is not None else "chl_none")
    negative = 0
    pen = [np.zeros(sh) for _ in range(nb)]
    op = np.zeros((nb, nz) + sh)   # the unscaled opacity

    if has_chl:   # opacity_from_chl
        Inv_nbands = 1.0 if nb <= 1 else 1.0 / float(nb)
        Inv_nbands_nir = 0.0 if nb <= 2 else 1.0 / (float(nb) - 2.0)
        if chl_3d is not None:
            chl_data = chl_3d[0][dom]
            negative = int(np.count_nonzero(wet[None] & (chl_3d[(slice(None),) + dom] < 0.0)))   # :328
        else:
            chl_data = chl_2d[dom]
            negative = int(np.count_nonzero(wet & (chl_data < 0.0)))   # :338, MOM_diabatic_aux.F90:649
        _count(counts, "negative_chl", negative)
        with np.errstate(invalid="ignore", divide="ignore"):
            if sch == MANIZZA:   # :352-377
                SW_vis_tot, SW_nir_tot = zero, zero
                _count(counts, "man_pen_wet", wet); _count(counts, "man_pen_land", ~wet)
                if multiband_vis_input:
                    SW_vis_tot = np.where(wet, get(sw_vis_dir) + get(sw_vis_dif), 0.0); _count(counts, "man_vis_multiband")
                elif total_sw_input:
                    SW_vis_tot = np.where(wet, 0.42 * get(sw), 0.0); _count(counts, "man_vis_from_total")
                else:
                    _count(counts, "man_vis_none")
                if multiband_nir_input:
                    SW_nir_tot = np.where(wet, get(sw_nir_dir) + get(sw_nir_dif), 0.0); _count(counts, "man_nir_multiband")
                elif total_sw_input:
                    SW_nir_tot = np.where(wet, get(sw) - SW_vis_tot, 0.0); _count(counts, "man_nir_from_total")
                else:
                    _count(counts, "man_nir_none")
                pen[0] = P.blue_frac * SW_vis_tot
                if nb > 1:
                    pen[1] = (1.0 - P.blue_frac) * SW_vis_tot; _count(counts, "man_band_2")
                for n in range(2, nb):
                    pen[n] = Inv_nbands_nir * SW_nir_tot; _count(counts, "man_band_nir")
            elif sch == MOREL:   # :380-393
                SW_pen_tot = zero
                _count(counts, "morel_pen_wet", wet); _count(counts, "morel_pen_land", ~wet)
                if multiband_vis_input:
                    SW_pen_tot = np.where(wet, SW_pen_frac_morel(chl_data, CS) * (get(sw_vis_dir) + get(sw_vis_dif)), 0.0)
                    _count(counts, "morel_multiband")
                elif total_sw_input:
                    SW_pen_tot = np.where(wet, SW_pen_frac_morel(chl_data, CS) * 0.5 * get(sw), 0.0)
                    _count(counts, "morel_from_total")
                else:
                    _count(counts, "morel_none")
                for n in range(nb):
                    pen[n] = Inv_nbands * SW_pen_tot
            else:   # OHLMANN_03 :400-416
                land = mask < 0.5
                _count(counts, "ohl_pen_wet", ~land); _count(counts, "ohl_pen_land", land)
                if multiband_vis_input:
                    SW_vis_tot = ((get(sw_vis_dir) + get(sw_vis_dif)) + get(sw_nir_dir)) + get(sw_nir_dif); _count(counts, "ohl_multiband")
                else:
                    SW_vis_tot = get(sw); _count(counts, "ohl_from_total")
                m = ohlmann_index(chl_data, CS, counts, ~land)
                pen[0] = np.where(land, 0., CS["lut"][0][m] * SW_vis_tot)
                pen[1] = np.where(land, 0., CS["lut"][1][m] * SW_vis_tot)

            for k in range(nz):   # :422-475
                if chl_3d is not None:
                    chl_data = chl_3d[k][dom]
                if sch == MANIZZA:
                    land = mask <= 0.5
                    _count(counts, "man_op_land", land); _count(counts, "man_op_wet", ~land)
                    for n in range(nb):
                        if n < CS["chl_dep_bands"]:
                            _count(counts, "man_op_chl_dep")
                            op[n, k] = np.where(land, P.opacity_land_value,
                                                CS["c1"][n] + CS["c2"][n] * np.power(chl_data, CS["pw"][n]))
                        else:
                            _count(counts, "man_op_chl_indep")
                            op[n, k] = np.where(land, P.opacity_land_value, CS["c1"][n])
                elif sch == MOREL:
                    _count(counts, "morel_op_wet", wet); _count(counts, "morel_op_land", ~wet)
                    op[0, k] = np.where(wet, opacity_morel(chl_data, CS), P.opacity_land_value)
                    for n in range(1, nb):
                        op[n, k] = op[0, k]; _count(counts, "morel_more_bands")
                else:
                    land = mask <= 0.5
                    _count(counts, "ohl_op_land", land); _count(counts, "ohl_op_wet", ~land)
                    m = ohlmann_index(chl_data, CS, counts, ~land)
                    op[0, k] = np.where(land, P.opacity_land_value, CS["lut"][2][m] * P.Z_to_m)
                    op[1, k] = np.where(land, P.opacity_land_value, CS["lut"][3][m] * P.Z_to_m)
    else:   # :152-193
        Inv_nbands = 1.0 if nb <= 1 else 1.0 / float(nb)
        floor_Z = max(0.1 * (GV.H_to_Z * GV.Angstrom_H), GV.dZ_subroundoff)   # GV%Angstrom_Z as H_to_Z*Angstrom_H
        inv_sw_pen_scale = 1.0 / max(P.pen_sw_scale, floor_Z)
        pen_zero = (not total_sw_input) or (P.pen_sw_scale <= 0.0)
        _count(counts, "exp_pen_zero" if pen_zero else "exp_pen_set")
        if sch == DOUBLE_EXP:
            op[0] = inv_sw_pen_scale
            op[1] = 1.0 / max(P.pen_sw_scale_2nd, floor_Z)
            if not pen_zero:
                pen[0] = (P.sw_1st_exp_ratio) * get(sw)
                pen[1] = (1. - P.sw_1st_exp_ratio) * get(sw)
        else:
            op[:] = inv_sw_pen_scale
            if not pen_zero:
                for n in range(nb):
                    pen[n] = P.pen_sw_frac * Inv_nbands * get(sw)

    for n in range(nb):
        sw_pen_band[(n,) + dom] = pen[n]
        opacity_band[(n, slice(None)) + dom] = opacity_scale * op[n]   # extract_optics_slice :559
    if SW_pen is not None:   # :199-204
        _count(counts, "diag_sw_pen")
        tot = np.zeros(sh)
        for n in range(nb):
            tot = tot + pen[n]
        SW_pen[dom] = tot
    if SW_vis_pen is not None:   # :208-224
        _count(counts, "diag_vis_manizza" if sch == MANIZZA else "diag_vis_all")
        tot = np.zeros(sh)
        for n in range(min(nb, 2) if sch == MANIZZA else nb):
            tot = tot + pen[n]
        SW_vis_pen[dom] = tot
    if opac_diag is not None:   # :227-237
        _count(counts, "diag_opac")
        op_diag_len = 1.0e-10 * P.m_to_Z
        with np.errstate(invalid="ignore"):
            for n in range(nb):
                opac_diag[(n, slice(None)) + dom] = np.tanh(op_diag_len * op[n]) / op_diag_len
    return negative


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and cases

def _ij(d):
    il = (np.arange(d.pitch) - d.ioff + d.i_glob0)[None, :] * np.ones(d.shape2(), int)
    jl = (np.arange(d.shape2()[0]) - d.joff + d.j_glob0)[:, None] * np.ones(d.shape2(), int)
    return il, jl


SW_NAMES = ("sw", "sw_vis_dir", "sw_vis_dif", "sw_nir_dir", "sw_nir_dif")


def inputs(d, M, seed=7, chl="exact", chl_one=False):
    """The five shortwave planes (non-zero over land too, so that the masks are seen to act), chl_2d and chl_3d, laid in global
    coordinates.  chl "exact": a pattern of 0.0 and 1.0 (chl_one: 1.0 everywhere); "smooth": 0.01 .. 20 mg m-3, log-uniform."""
    from mom6_amd import synth
    sf = lambda n, **kw: synth.smooth_field(d, seed + n, ox=0.5, oy=0.5, **kw)
    il, jl = _ij(d)
    out = dict(sw=150.0 * (1.0 + 0.9 * sf(1)), sw_vis_dir=40.0 * (1.0 + 0.8 * sf(2)), sw_vis_dif=25.0 * (1.0 + 0.8 * sf(3)),
               sw_nir_dir=50.0 * (1.0 + 0.8 * sf(4)), sw_nir_dif=30.0 * (1.0 + 0.8 * sf(5)))
    if chl == "exact":
        c2 = np.where((il + 2 * jl) % 3 == 0, 0.0, 1.0)
        c3 = np.stack([np.where((il + 2 * jl + k) % 3 == 0, 0.0, 1.0) for k in range(d.nk)])
        if chl_one:
            c2 = np.ones_like(c2); c3 = np.ones_like(c3)
    else:
        lo, hi = math.log(0.01), math.log(20.0)
        c2 = np.clip(np.exp(lo + (hi - lo) * 0.5 * (1.0 + 1.8 * sf(6))), 0.01, 20.0)
        c3 = np.clip(np.exp(lo + (hi - lo) * 0.5 * (1.0 + 1.8 * sf(7, nk=d.nk))), 0.01, 20.0)
    out["chl_2d"], out["chl_3d"] = c2, c3
    return {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in out.items()}


_ALL, _TOT, _VIS, _NIR = SW_NAMES, ("sw",), ("sw_vis_dir", "sw_vis_dif"), ("sw_nir_dir", "sw_nir_dif")
_SW_SETS = ((), _TOT, _VIS, _NIR, _VIS + _NIR, _TOT + _VIS, _TOT + _NIR, _ALL)
_DIAG = ("SW_pen", "SW_vis_pen", "opac_diag")
SCALES = (1.0, 2.0 ** -11)


def _cases():
    """case -> (params members, options).  Options: given (the shortwave planes handed in), chl (None, "2d", "3d"), chl_kind
    ("exact", "smooth"), chl_one, scale (opacity_scale), diag (the diagnostics handed in)."""
    C = {}
    for m, given in enumerate(_SW_SETS):   # MANIZZA_05: every combination of associated inputs, 1 .. 4 bands, both chlorophylls
        C[f"manizza_{m}"] = (dict(opacity_scheme=MANIZZA, nbands=1 + m % 4),
                             dict(given=given, chl=("2d", "3d")[(m // 4 + m) % 2], scale=SCALES[m % 2], diag=_DIAG if m % 3 == 0 else ()))
    C["manizza_half_pairs"] = (dict(opacity_scheme=MANIZZA, nbands=3), dict(given=("sw", "sw_vis_dir", "sw_nir_dif"), chl="2d"))
    C["manizza_folded"] = (dict(opacity_scheme=MANIZZA, nbands=4, manizza_power=(0.674, 0.0, 0.0), manizza_coef=(0.0232, 0.074, 0.225, 0.037, 2.86, 0.5),
                                blue_frac=0.375, opacity_land_value=3.0),
                           dict(given=_ALL, chl="3d", scale=SCALES[1], diag=_DIAG))
    for m, given in enumerate(((), _TOT, _VIS, _TOT + _VIS, _ALL)):   # MOREL_88: chlorophyll of 1.0 only
        C[f"morel_{m}"] = (dict(opacity_scheme=MOREL, nbands=1 + m % 4),
                           dict(given=given, chl=("2d", "3d")[m % 2], chl_one=True, scale=SCALES[m % 2], diag=_DIAG if m % 2 else ()))
    for m, given in enumerate((_TOT, _VIS + _NIR, _ALL, _TOT + _NIR)):   # OHLMANN_03
        C[f"ohlmann_{m}"] = (dict(opacity_scheme=OHLMANN, nbands=2),
                             dict(given=given, chl=("2d", "3d")[m % 2], scale=SCALES[m % 2], diag=_DIAG if m >= 2 else ()))
    for m, (given, scale) in enumerate(((_TOT, 15.0), ((), 15.0), (_ALL, 0.0), (_TOT, 1.0e-12))):   # the exponential schemes
        C[f"single_{m}"] = (dict(opacity_scheme=SINGLE_EXP, nbands=1, pen_sw_scale=scale, pen_sw_frac=0.42, sw_1st_exp_ratio=1.0),
                            dict(given=given, scale=SCALES[m % 2], diag=_DIAG if m % 2 == 0 else ()))
        C[f"double_{m}"] = (dict(opacity_scheme=DOUBLE_EXP, nbands=2, pen_sw_scale=scale, pen_sw_scale_2nd=0.35, sw_1st_exp_ratio=0.58),
                            dict(given=given, scale=SCALES[(m + 1) % 2], diag=_DIAG if m % 2 else ()))
    # the transcendental class
    for sch, name, nb in ((MANIZZA, "manizza", 3), (MOREL, "morel", 2), (OHLMANN, "ohlmann", 2)):
        for chl in ("2d", "3d"):
            C[f"smooth_{name}_{chl}"] = (dict(opacity_scheme=sch, nbands=nb),
                                         dict(given=_ALL if chl == "2d" else _TOT, chl=chl, chl_kind="smooth", scale=SCALES[chl == "3d"], diag=_DIAG))
    return C


CASES = _cases()
CASES_TRANSCENDENTAL = tuple(n for n in CASES if n.startswith("smooth_"))
CASES_EXACT = tuple(n for n in CASES if n not in CASES_TRANSCENDENTAL)
OUT_TRANSCENDENTAL = ("opac_diag",)   # outside the exact class in every case


def case(name):
    """(params, options)"""
    mods, opt = CASES[name]
    opt = dict(dict(given=(), chl=None, chl_kind="exact", chl_one=False, scale=1.0, diag=()), **opt)
    return abi.opacity_params_default(**mods), opt


def case_inputs(d, M, opt, seed=7):
    return inputs(d, M, seed=seed, chl=opt["chl_kind"], chl_one=opt["chl_one"])


def outputs(d, P, opt, fill=np.nan):
    nb = max(P.nbands, 1)
    out = dict(opacity_band=np.full((nb,) + d.shape3(), fill), sw_pen_band=np.full((nb,) + d.shape2(), fill))
    for n in opt["diag"]:
        out[n] = np.full((nb,) + d.shape3(), fill) if n == "opac_diag" else np.full(d.shape2(), fill)
    return out


def call_args(opt, inp):
    """The keyword arguments of a case's call, from a dict of arrays by name."""
    kw = {n: inp[n] for n in opt["given"]}
    if opt["chl"] is not None:
        kw["chl_" + opt["chl"]] = inp["chl_" + opt["chl"]]
    kw["opacity_scale"] = opt["scale"]
    return kw


def run(d, M, GV, P, opt, inp, fill=np.nan, counts=None, ncalls=1):
    """A case on numpy arrays, `ncalls` times on the same outputs: (outputs by name, negative count summed, counts)."""
    counts = counts if counts is not None else new_counts()
    CS = init(P, GV, counts)
    out = outputs(d, P, opt, fill)
    neg = 0
    for _ in range(ncalls):
        neg += set_pen_shortwave(d, M, CS, counts=counts, **call_args(opt, inp), **out)
    return out, neg, counts
