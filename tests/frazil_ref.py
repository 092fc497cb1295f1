"""The checker of mom6x_make_frazil, mom6x_adjust_salt and mom6x_geothermal_in_place: a numpy restatement of make_frazil
(src/parameterizations/vertical/MOM_diabatic_aux.F90:110-230), adjust_salt (:339-390), geothermal_in_place
(src/parameterizations/vertical/MOM_geothermal.F90:364-535, the Boussinesq arm) and calculate_TFreeze_1d
(src/equation_of_state/MOM_EOS.F90:664-744 with MOM_TFreeze.F90:82, :129, :196-200).  Arrays are in the pitched tile layout of
include/mom6x.h ([k, j + joff, i + ioff]).

The routines run in the reference's own loop order: one j-row at a time, inside a row one layer at a time over the i of the row,
with masks for the columns an arm applies to -- not the device's one lane per column, so the two orders check each other.
geothermal_in_place keeps the reference's row rule (:476): a row without a heated column is left before tv%internal_heat is
added to.  The arithmetic is the reference's, operation for operation (x**2 written as x*x, MAX as the reference's compiler
evaluates it); the only non-arithmetic operation is a square root, so the device is held to it bit for bit.  The density derivatives
of BFlx_geothermal come from the oracle's EOS through ref_common._derivs.  `counts` (BRANCHES) records how often each arm fired."""
import numpy as np

from mom6_amd import abi
from tests.ref_common import _derivs, _max

G = abi.G
BRANCHES = ("tfr_unscaled", "tfr_scaled", "tfr_degC_scaled",
            "fz_reclaim_all", "fz_reclaim_part", "fz_reclaim_cold", "fz_gate_closed", "fz_thin_cold", "fz_thin_warm",
            "fz_thick_freeze", "fz_thick_absorb", "fz_thick_idle", "fz_warm_cooled", "fz_reaches_surface", "fz_land_column",
            "salt_gate_closed", "salt_thin_low", "salt_thin_ok", "salt_absorb", "salt_deficit", "salt_reaches_surface",
            "geo_row_skipped", "geo_fits_layer", "geo_fits_bottom", "geo_partial", "geo_several_layers", "geo_left_over",
            "geo_skip_angstrom", "geo_unheated_column")


def _count(counts, name, mask):
    if counts is not None:
        counts[name] += int(np.count_nonzero(mask))


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# calculate_TFreeze_1d

_TF = dict(TF00=0.017947064327968736, TF20=-6.076099099929818e-2, TF30=4.883198653547851e-3, TF40=-1.188081601230542e-3,
           TF50=1.334658511480257e-4, TF60=-8.722761043208607e-6, TF70=2.082038908808201e-7, TF01=-7.389420998107497e-8,
           TF21=-9.891538123307282e-11, TF31=-8.987150128406496e-13, TF41=1.054318231187074e-12, TF51=3.850133554097069e-14,
           TF61=-2.079022768390933e-14, TF71=1.242891021876471e-15, TF02=-2.110913185058476e-16, TF22=3.831132432071728e-19,
           TF32=1.065556599652796e-19, TF42=-2.078616693017569e-20, TF52=1.596435439942262e-21, TF03=2.295491578006229e-25,
           TF23=-7.997496801694032e-27, TF33=8.756340772729538e-28, TF43=1.338002171109174e-29)


def TFreeze(P, S, pressure, counts=None):
    """calculate_TFreeze_1d without use_conT_absS: S [S], pressure [R L2 T-2] -> the freezing point [C]."""
    S = np.asarray(S, dtype=np.float64); pressure = np.asarray(pressure, dtype=np.float64) + 0.0 * S
    if (P.RL2_T2_to_Pa == 1.0) and (P.S_to_ppt == 1.0):           # :699
        Sa, pres = S, pressure
        _count(counts, "tfr_unscaled", np.ones(S.shape, bool))
    else:                                                         # :714-717
        pres = P.RL2_T2_to_Pa * pressure
        Sa = P.S_to_ppt * S
        _count(counts, "tfr_scaled", np.ones(S.shape, bool))
    with np.errstate(invalid="ignore"):
        if P.form_of_TFreeze == abi.TFREEZE_LINEAR:
            T_fr = (P.TFr_S0_P0 + P.dTFr_dS * Sa) + P.dTFr_dp * pres
        elif P.form_of_TFreeze == abi.TFREEZE_MILLERO:
            cS1, cS3_2, cS2, dTFr_dp = -0.0575, 1.710523e-3, -2.154996e-4, -7.75e-8
            T_fr = Sa * (cS1 + (cS3_2 * np.sqrt(_max(Sa, 0.0)) + cS2 * Sa)) + dTFr_dp * pres
        elif P.form_of_TFreeze == abi.TFREEZE_TEOSPOLY:
            c = _TF
            rS = np.sqrt(_max(Sa, 0.0))
            T_fr = ((c["TF00"] + Sa * (c["TF20"] + rS * (c["TF30"] + rS * (c["TF40"] + rS * (c["TF50"] + rS * (c["TF60"] + rS * c["TF70"])))))) +
                    pres * ((c["TF01"] + Sa * (c["TF21"] + rS * (c["TF31"] + rS * (c["TF41"] + rS * (c["TF51"] + rS * (c["TF61"] + rS * c["TF71"])))))) +
                            pres * ((c["TF02"] + Sa * (c["TF22"] + rS * (c["TF32"] + rS * (c["TF42"] + rS * c["TF52"])))) +
                                    pres * (c["TF03"] + Sa * (c["TF23"] + rS * (c["TF33"] + rS * c["TF43"]))))))
        else:
            raise ValueError("form_of_TFreeze is not valid.")
        if P.degC_to_C != 1.0:                                    # :740
            T_fr = P.degC_to_C * T_fr
            _count(counts, "tfr_degC_scaled", np.ones(S.shape, bool))
    return T_fr


def _range(d, halo):
    return -halo, d.ni - 1 + halo, -halo, d.nj - 1 + halo


# ------------------------------------------------------------------------------------------------------------------------------
def make_frazil(d, M, GV, P, h, T, S, frazil, p_surf=None, halo=0, counts=None):
    """make_frazil: T and frazil are rewritten in place on the computational domain widened by halo."""
    nz = d.nk
    is_, ie, js, je = _range(d, halo)
    ci = slice(is_ + d.ioff, ie + d.ioff + 1)
    n = ie - is_ + 1
    CpH = P.C_p * GV.H_to_RZ
    pressure = np.zeros((nz, n))                                  # :143-144
    H_to_RL2_T2 = GV.H_to_RZ * GV.g_Earth
    h_thin = 10.0 * (GV.Angstrom_H + GV.H_subroundoff)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(js, je + 1):
            r = j + d.joff
            ps = np.zeros(n)
            if p_surf is not None:
                ps = p_surf[r, ci].copy()
            fraz_col = np.zeros(n)
            if P.pressure_dependent_frazil:                       # :158-165
                pressure[0] = ps + (0.5 * H_to_RL2_T2) * h[0, r, ci]
                for k in range(1, nz):
                    pressure[k] = pressure[k - 1] + (0.5 * H_to_RL2_T2) * (h[k, r, ci] + h[k - 1, r, ci])
            if P.reclaim_frazil:                                  # :167-189
                fr = frazil[r, ci].copy()
                pos = fr > 0.0
                if pos.any():
                    T_freeze = TFreeze(P, S[0, r, ci], pressure[0], counts)
                    T1 = T[0, r, ci].copy()
                    warm = pos & (T1 > T_freeze)
                    hc = CpH * h[0, r, ci]
                    allr = warm & (fr - hc * (T1 - T_freeze) <= 0.0)
                    part = warm & ~allr
                    _count(counts, "fz_reclaim_all", allr); _count(counts, "fz_reclaim_part", part)
                    _count(counts, "fz_reclaim_cold", pos & ~warm)
                    T[0, r, ci] = np.where(allr, T1 - fr / hc, np.where(part, T_freeze, T1))
                    frazil[r, ci] = np.where(allr, 0.0, np.where(part, fr - hc * (T1 - T_freeze), fr))
            wet = M[G["mask2dT"]][r, ci] > 0.0
            _count(counts, "fz_land_column", ~wet)
            for k in range(nz - 1, -1, -1):                       # :191-220
                Tk = T[k, r, ci].copy()
                gate = wet & ((Tk < 0.0) | (fraz_col > 0.0))
                _count(counts, "fz_gate_closed", wet & ~gate)
                if not gate.any():
                    continue
                T_freeze = TFreeze(P, S[k, r, ci], pressure[k], counts)
                hk = h[k, r, ci]
                hc = CpH * hk
                thin = gate & (hk <= h_thin)
                t_cold = thin & (Tk < T_freeze)
                thick = gate & ~thin & ((fraz_col > 0.0) | (Tk < T_freeze))
                absorb = thick & (fraz_col + hc * (T_freeze - Tk) < 0.0)
                freeze = thick & ~absorb
                _count(counts, "fz_thin_cold", t_cold); _count(counts, "fz_thin_warm", thin & ~t_cold)
                _count(counts, "fz_thick_absorb", absorb); _count(counts, "fz_thick_freeze", freeze)
                _count(counts, "fz_thick_idle", gate & ~thin & ~thick)
                _count(counts, "fz_warm_cooled", thick & (Tk >= T_freeze))
                more = t_cold | freeze
                T[k, r, ci] = np.where(more, T_freeze, np.where(absorb, Tk - fraz_col / hc, Tk))
                fraz_col = np.where(more, fraz_col + hc * (T_freeze - Tk), np.where(absorb, 0.0, fraz_col))
            _count(counts, "fz_reaches_surface", fraz_col > 0.0)
            frazil[r, ci] = frazil[r, ci] + fraz_col              # :221-223


def adjust_salt(d, M, GV, h, S, salt_deficit, S_min, counts=None):
    """adjust_salt: S and salt_deficit are rewritten in place on the computational domain."""
    nz = d.nk
    ci = slice(d.ioff, d.ioff + d.ni)
    h_thin = 10.0 * GV.Angstrom_H
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(d.nj):
            r = j + d.joff
            col = np.zeros(d.ni)
            wet = M[G["mask2dT"]][r, ci] > 0.0
            for k in range(nz - 1, -1, -1):
                Sk = S[k, r, ci].copy()
                gate = wet & ((Sk < S_min) | (col > 0.0))
                _count(counts, "salt_gate_closed", wet & ~gate)
                if not gate.any():
                    continue
                hk = h[k, r, ci]
                mc = GV.H_to_RZ * hk
                thin = gate & (hk <= h_thin)
                t_low = thin & (Sk < S_min)
                absorb = gate & ~thin & (col + mc * (S_min - Sk) <= 0.0)
                deficit = gate & ~thin & ~absorb
                _count(counts, "salt_thin_low", t_low); _count(counts, "salt_thin_ok", thin & ~t_low)
                _count(counts, "salt_absorb", absorb); _count(counts, "salt_deficit", deficit)
                more = t_low | deficit
                S[k, r, ci] = np.where(more, S_min, np.where(absorb, Sk - col / mc, Sk))
                col = np.where(more, col + mc * (S_min - Sk), np.where(absorb, 0.0, col))
            _count(counts, "salt_reaches_surface", col > 0.0)
            salt_deficit[r, ci] = salt_deficit[r, ci] + col


def geothermal_in_place(d, M, GV, P, geo_heat, h, T, S, dt, internal_heat=None, BFlx_geothermal=None, dTdt_diag=None,
                        heat_tend_diag=None, halo=0, eos=None, orc=None, counts=None):
    """geothermal_in_place, Boussinesq: T and the given outputs are rewritten in place.  BFlx_geothermal is optional here as on
    the device (the reference always forms it); it needs eos and orc."""
    nz = d.nk
    is_, ie, js, je = _range(d, halo)
    ci = slice(is_ + d.ioff, ie + d.ioff + 1)
    n = ie - is_ + 1
    il = np.arange(is_, ie + 1)
    dom = (il >= 0) & (il < d.ni)                                 # EOS_domain(G%HI) :423: the computational domain along i
    Irho_cp = 1.0 / (GV.H_to_RZ * P.C_p)
    Angstrom, H_neglect = GV.Angstrom_H, GV.H_subroundoff
    Idt = 1.0 / dt
    H_to_pres = GV.H_to_RZ * GV.g_Earth
    I_Cp = 1. / P.C_p
    I_Rho0squared = 1. / (GV.Rho0 * GV.Rho0)
    calc_diags = dTdt_diag is not None or heat_tend_diag is not None
    if BFlx_geothermal is not None:
        BFlx_geothermal[...] = 0.0                                # :434
    diag = np.zeros(d.shape3()) if calc_diags else None           # :436
    mask2dT = M[G["mask2dT"]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(js, je + 1):
            r = j + d.joff
            mask, gh = mask2dT[r, ci], geo_heat[r, ci]
            if BFlx_geothermal is not None:                       # :440-460
                bottom_pressure = np.zeros(n)
                for k in range(nz):
                    bottom_pressure = bottom_pressure + H_to_pres * h[k, r, ci]
                dRhodT = np.zeros(n)
                a, _ = _derivs(orc, eos, T[nz - 1, r, ci][dom], S[nz - 1, r, ci][dom], P.RL2_T2_to_Pa * bottom_pressure[dom])
                dRhodT[dom] = a
                BFlx_geothermal[r, ci] = -(((P.g_Earth_Z_T2 * I_Rho0squared) * ((I_Cp * dRhodT) * gh)) * mask)
            heat_rem = mask * (gh * (dt * Irho_cp))               # :472
            h_geo_rem = np.full(n, P.geothermal_thick)
            if not (heat_rem > 0.0).any():                        # :476
                _count(counts, "geo_row_skipped", np.ones(1, bool))
                continue
            _count(counts, "geo_unheated_column", ~(heat_rem > 0.0))
            layers = np.zeros(n, int)
            for k in range(nz - 1, -1, -1):                       # :482-507
                hk = h[k, r, ci]
                act = (heat_rem > 0.0) & (hk > Angstrom)
                _count(counts, "geo_skip_angstrom", (heat_rem > 0.0) & ~act)
                fits = act & ((hk - Angstrom) >= h_geo_rem)
                part = act & ~fits
                _count(counts, "geo_fits_layer", fits); _count(counts, "geo_partial", part)
                if k == nz - 1:
                    _count(counts, "geo_fits_bottom", fits)
                heat_here = np.where(fits, heat_rem, heat_rem * ((hk - Angstrom) / (h_geo_rem + H_neglect)))
                h_geo_new = np.where(fits, 0.0, h_geo_rem - (hk - Angstrom))
                heat_new = np.where(fits, 0.0, heat_rem - heat_here)
                h_geo_rem = np.where(act, h_geo_new, h_geo_rem)
                heat_rem = np.where(act, heat_new, heat_rem)
                dTemp = heat_here / (hk + H_neglect)
                Tk = T[k, r, ci]
                T[k, r, ci] = np.where(act, Tk + dTemp, Tk)
                if calc_diags:
                    diag[k, r, ci] = np.where(act, dTemp * Idt, diag[k, r, ci])
                layers += act
                if not (heat_rem > 0.0).any():
                    break
            _count(counts, "geo_several_layers", layers > 1)
            _count(counts, "geo_left_over", heat_rem > 0.0)
            if internal_heat is not None:                         # :509-512
                internal_heat[r, ci] = internal_heat[r, ci] + GV.H_to_RZ * (mask * (gh * (dt * Irho_cp)) - heat_rem)
        if dTdt_diag is not None:
            dTdt_diag[...] = diag
        if heat_tend_diag is not None:                            # :520-524
            rows = slice(js + d.joff, je + d.joff + 1)
            diag[:, rows, ci] = (GV.H_to_RZ * P.C_p) * (h[:, rows, ci] * diag[:, rows, ci])
            heat_tend_diag[...] = diag


# ------------------------------------------------------------------------------------------------------------------------------
# Shared inputs and cases of tests/test_diabatic_TS_cpu.py and tests/test_diabatic_TS_gpu.py

def _ij(d):
    il = (np.arange(d.pitch) - d.ioff + d.i_glob0)[None, :] * np.ones(d.shape2(), int)
    jl = (np.arange(d.shape2()[0]) - d.joff + d.j_glob0)[:, None] * np.ones(d.shape2(), int)
    return il, jl


def inputs(d, M, GV, seed=3, polar=0.45, geo="patchy", neg_zero=False):
    """h, T, S and the planes frazil, salt_deficit, internal_heat, p_surf, geo_heat on a tile, every field laid in global
    coordinates, halos included.
    h: the bathymetry's layers with, in bands of columns, thin layers (0, 0.5e-10, 5e-10, 1e-9, 2e-9, 1e-6 m: below and above
    Angstrom_H, 10*Angstrom_H and 10*(Angstrom_H + H_subroundoff)) at the bottom, in the middle and at the surface.
    T: -3 .. 12 degC, the rows below `polar` of the way north below freezing throughout, the others warm with cold patches at
    depth and in mid-column (a warm layer above a cold one takes the pending heat).  S: 33 .. 36 with fresh patches (0 .. 30), a
    patch below 0 and, in a band, fresh water at the bottom only (a deficit that a salty layer above absorbs).
    frazil: 0 with positive patches (small enough for a warm surface layer to take all of, and large), also over land.
    salt_deficit, internal_heat: smooth and positive.  geo_heat (scaled by mask2dT as geothermal_init does): `patchy` 0.05 ..
    0.15 W m-2 with every fourth row and a block unheated and one row heated in a single column; `none`: 0.
    neg_zero: -0 planted in blocks of frazil, salt_deficit and T."""
    from mom6_amd import synth
    nk = d.nk
    h, _, _ = synth.make_state(d, M, seed=20250808 + seed, u_max=0.3, h_pert=0.01)
    il, jl = _ij(d)
    wetp = M[G["mask2dT"]] > 0.0
    sf = lambda n, **kw: synth.smooth_field(d, seed + n, ox=0.5, oy=0.5, **kw)
    thins = (0.0, 0.5e-10, 5.0e-10, 1.0e-9, 2.0e-9, 1.0e-6)
    for m, th in enumerate(thins):
        sel = wetp & (il % 9 == m) & (jl % 3 != 1)
        ks = {0: (nk - 1,), 1: (nk - 1, nk - 2), 2: (0,)}[m % 3]
        for k in ks:
            if 0 <= k < nk and nk > 1:
                h[k] = np.where(sel, th, h[k])
    if nk > 3:
        h[nk // 2] = np.where(wetp & (il % 7 == 5), 3.0e-10, h[nk // 2])
    T = np.zeros_like(h); S = np.zeros_like(h)
    pT, pS = sf(10), sf(11)
    cold_rows = jl < polar * d.nj_glob
    for k in range(nk):
        zf = k / max(nk - 1, 1)
        warm = 8.0 - 6.0 * zf + 3.0 * pT
        warm = np.where((il % 5 == 2) & (k >= nk // 2), -1.9 - 0.5 * zf + 0.2 * pT, warm)      # cold at depth under warm water
        warm = np.where((il % 13 == 6) & (k == nk // 2), -2.5, warm)                          # one cold layer in mid-column
        T[k] = np.where(cold_rows, -2.2 - 0.6 * zf + 0.5 * pT, warm)
        S[k] = 34.5 + 1.0 * zf + 0.8 * pS
        S[k] = np.where((il >= 8) & (il <= 13) & (jl >= 4) & (jl <= 9), 15.0 * (1.0 + pS) * (1.0 - 0.5 * zf), S[k])
        S[k] = np.where((il >= 20) & (il <= 22) & (jl >= 10) & (jl <= 12), -0.5 + 0.1 * zf, S[k])
    S[nk - 1] = np.where(il % 6 == 1, 20.0 + pS, S[nk - 1])
    frazil = np.zeros(d.shape2())
    frazil = np.where((il % 4 == 1) & (jl % 2 == 0), 1.0e3 * (1.0 + 0.5 * sf(20)), frazil)
    frazil = np.where((il % 8 == 3) & (jl % 2 == 1), 1.0e9 * (1.5 + sf(21)), frazil)
    salt_deficit = 5.0 * (1.5 + sf(22))
    internal_heat = 1.0e4 * (1.5 + sf(23))
    p_surf = 2.0e4 * (1.0 + 0.2 * sf(24))
    if geo == "none":
        geo_heat = np.zeros(d.shape2())
    else:
        geo_heat = 0.1 * (1.0 + 0.5 * sf(25))
        geo_heat = np.where(jl % 4 == 2, 0.0, geo_heat)
        geo_heat = np.where((il >= 24) & (il <= 30) & (jl >= 14) & (jl <= 19), 0.0, geo_heat)
        geo_heat = np.where((jl % 4 == 2) & (jl % 8 == 2) & (il == 17), 0.08, geo_heat)       # one heated column in its row
    geo_heat = M[G["mask2dT"]] * geo_heat
    if neg_zero:
        frazil[d.sl(3, 9, 2, 8)] = -0.0
        salt_deficit[d.sl(5, 12, 3, 9)] = -0.0
        T[(slice(None),) + d.sl(10, 18, 6, 14)] = -0.0
    out = dict(h=h, T=T, S=S, frazil=frazil, salt_deficit=salt_deficit, internal_heat=internal_heat, p_surf=p_surf, geo_heat=geo_heat)
    return {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in out.items()}


def nan_beyond(d, inp, halo):
    """The inputs with NaN in h, T and S beyond the computational domain widened by halo: nothing out there may be read."""
    inp = dict(inp)
    own = np.zeros(d.shape2(), bool)
    own[d.sl(-halo, d.ni - 1 + halo, -halo, d.nj - 1 + halo)] = True
    for n in ("h", "T", "S"):
        inp[n] = np.where(own[None], inp[n], np.nan)
    return inp


# case -> options.  frazil: members of mom6x_frazil_params; p_surf: handed to make_frazil; S_min: adjust_salt's; geo: members of
# mom6x_geothermal_params; dt; eos: an EOS form or None; out: the nullable outputs of geothermal_in_place handed in; inp: keyword
# arguments of inputs()
_GEO_ALL = ("internal_heat", "BFlx_geothermal", "dTdt_diag", "heat_tend_diag")
CASES = {
    "linear": dict(frazil=dict(), p_surf=False, S_min=0.01, geo=dict(), dt=3600.0, eos=None, out=("internal_heat",)),
    "linear_p": dict(frazil=dict(pressure_dependent_frazil=1, dTFr_dp=-7.6e-8), p_surf=True, S_min=33.0, geo=dict(geothermal_thick=500.0),
                     dt=7200.0, eos=abi.WRIGHT, out=_GEO_ALL),
    "millero": dict(frazil=dict(form_of_TFreeze=abi.TFREEZE_MILLERO, reclaim_frazil=0), p_surf=False, S_min=34.0,
                    geo=dict(geothermal_thick=5000.0), dt=1800.0, eos=None, out=("dTdt_diag",)),
    "millero_p": dict(frazil=dict(form_of_TFreeze=abi.TFREEZE_MILLERO, pressure_dependent_frazil=1), p_surf=False, S_min=20.0,
                      geo=dict(geothermal_thick=1.0e-9), dt=3600.0, eos=abi.LINEAR, out=("BFlx_geothermal", "heat_tend_diag")),
    "teos_poly": dict(frazil=dict(form_of_TFreeze=abi.TFREEZE_TEOSPOLY), p_surf=True, S_min=35.5, geo=dict(geothermal_thick=100.0),
                      dt=3600.0, eos=None, out=()),
    "teos_poly_p": dict(frazil=dict(form_of_TFreeze=abi.TFREEZE_TEOSPOLY, pressure_dependent_frazil=1, reclaim_frazil=0), p_surf=True,
                        S_min=0.01, geo=dict(), dt=3600.0, eos=abi.WRIGHT_FULL, out=("internal_heat", "BFlx_geothermal")),
    "scaled": dict(frazil=dict(form_of_TFreeze=abi.TFREEZE_MILLERO, pressure_dependent_frazil=1, RL2_T2_to_Pa=0.5, S_to_ppt=2.0,
                               degC_to_C=4.0), p_surf=True, S_min=33.0, geo=dict(geothermal_thick=500.0), dt=3600.0, eos=None,
                   out=("internal_heat", "heat_tend_diag")),
    "idle": dict(frazil=dict(), p_surf=False, S_min=-10.0, geo=dict(), dt=3600.0, eos=None, out=("internal_heat", "dTdt_diag"),
                 inp=dict(polar=-1.0, geo="none")),
}


def case(name, GV):
    o = dict(CASES[name])
    o.setdefault("inp", {})
    return abi.frazil_params_default(**o["frazil"]), abi.geothermal_params_default(GV, **o["geo"]), o


def geo_outputs(d, opt, fill=np.nan, inp=None):
    """The nullable outputs of geothermal_in_place a case hands in; internal_heat starts from the inputs'."""
    out = {}
    for n in opt["out"]:
        if n == "internal_heat":
            out[n] = inp["internal_heat"].copy()
        else:
            out[n] = np.full(d.shape2() if n == "BFlx_geothermal" else d.shape3(), fill)
    return out


def run(d, M, GV, opt, Pf, Pg, inp, halo=0, orc=None, ncalls=1, counts=None):
    """`ncalls` times make_frazil, geothermal_in_place and adjust_salt, each on its own copy of the inputs (the routines are
    checked one by one; the chain is the GPU test's).  Returns {routine: {array: result}} and the branch counts."""
    counts = counts if counts is not None else new_counts()
    eos = abi.eos_params_default(opt["eos"]) if opt["eos"] is not None else None
    res = {}
    T, fr = inp["T"].copy(), inp["frazil"].copy()
    for _ in range(ncalls):
        make_frazil(d, M, GV, Pf, inp["h"], T, inp["S"], fr, inp["p_surf"] if opt["p_surf"] else None, halo, counts)
    res["frazil"] = dict(T=T, frazil=fr)
    S, sd = inp["S"].copy(), inp["salt_deficit"].copy()
    for _ in range(ncalls):
        adjust_salt(d, M, GV, inp["h"], S, sd, opt["S_min"], counts)
    res["salt"] = dict(S=S, salt_deficit=sd)
    T = inp["T"].copy()
    out = geo_outputs(d, opt, inp=inp)
    for _ in range(ncalls):
        geothermal_in_place(d, M, GV, Pg, inp["geo_heat"], inp["h"], T, inp["S"], opt["dt"], halo=halo, eos=eos, orc=orc,
                            counts=counts, **out)
    res["geo"] = dict(out, T=T)
    return res, counts
