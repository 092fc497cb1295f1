"""The checker of mom6x_calc_slope_functions: a numpy restatement of calc_slope_functions
(src/parameterizations/lateral/MOM_lateral_mixing_coeffs.F90:686-738) with calc_isoneutral_slopes
(src/core/MOM_isopycnal_slopes.F90:31-608, halo = 1, Boussinesq, no open boundaries, no Stanley term), vert_fill_TS (:612-700,
called WITHOUT larger_h_denom: h0 = h_neglect), find_eta (src/core/MOM_interface_heights.F90:91-97, halo_size = 2),
calc_Eady_growth_rate_2D (:962-1112), calc_Visbeck_coeffs_old (:743-959) and calc_slope_functions_using_just_e (:1116-1275), and
of the L2u, L2v of VarMix_init (:1759-1772).  Written from the Fortran operation for operation (x**2 as x*x, x**4 as (x*x)*(x*x),
nothing reordered), independent of the HIP, vectorised over the faces of one direction with a loop over K.  Arrays are in the
pitched tile layout of include/mom6x.h ([k, j + joff, i + ioff]); local indices are zero based (isc = 0, iec = ni-1).  Density
derivatives come from the oracle's EOS only, one point at a time.  MAX and MIN return their first argument on a tie, except in the
radicand of dzSxN and dzSyN (MOM_isopycnal_slopes.F90:418, :602), where the tie shows: MAX(0.0, -0.0) is -0.0 in the compiled
reference, and so is its square root (the case eady_tie reaches it).  These,
find_eta, the pressure column and vert_fill_TS come from tests/ref_common.py; the slope arithmetic is this module's own.
`counts` records how often each branch fired.

tests/test_varmix_cpu.py holds this module to facts that do not come from it; tests/test_ref_parity_cpu.py holds it bit for bit to
the reference's own MOM_lateral_mixing_coeffs.F90, MOM_isopycnal_slopes.F90 and MOM_interface_heights.F90, compiled into
oracle/_ref/libref_param.so (every case, slopes and every posted diagnostic), and tests/golden/ref_varmix_*.npz hold the device to
what that library gave."""
import numpy as np

from mom6_amd import abi
from tests.ref_common import _A, _derivs, _dmax, _max, _min, find_eta, pressure_column, vert_fill_TS

G = abi.G
BRANCHES = ("mag_grad2_zero", "kap_zero", "dzSN_clip", "N2_clipped", "S2max_applied", "S2max_idle", "Hu_le0", "Dscale_full",
            "Dscale_partial", "Dscale_zero", "crop_top_0", "crop_top_mid", "crop_top_1", "crop_bot_0", "crop_bot_mid", "crop_bot_1",
            "H_cutoff_mask", "bathy_cutoff", "denom_bathy", "denom_dztot")


def calc_isoneutral_slopes(d, M, GV, P, h, e, dt_kappa_smooth, out, T=None, S=None, p_surf=None, eos=None, Rlay=None, counts=None,
                           orc=None):
    """calc_isoneutral_slopes(..., halo=1).  `out` holds slope_x, slope_y and whichever of N2_u, N2_v, dzu, dzv, dzSxN, dzSyN are
    present; they are written in place on the reference's ranges only."""
    nz = d.nk
    is_, ie, js, je = -1, d.ni, -1, d.nj                                                # :145
    h_neglect = GV.H_subroundoff
    h_neglect2 = h_neglect * h_neglect
    use_EOS = eos is not None
    G_Rho0 = P.g_Earth / P.Rho0                                                         # :173
    if use_EOS:
        if orc is None:
            from oracle import orc
        Tf, Sf = vert_fill_TS(h, T, S, dt_kappa_smooth, GV, P.Z_to_H_fill, False, counts)   # :213
        pres = pressure_column(h, p_surf, P.g_Earth * P.H_to_RZ)                        # :231-247
    for dir in (0, 1):
        rng = (is_ - 1, ie, js, je) if dir == 0 else (is_, ie, js - 1, je)
        far = dict(di=1, dj=0) if dir == 0 else dict(di=0, dj=1)
        s = "v" if dir else "u"

        def L(a):
            return _A(d, a, rng)

        def R(a):
            return _A(d, a, rng, **far)

        slope = out["slope_y" if dir else "slope_x"]
        N2 = out.get("N2_" + s)
        dzo = out.get("dz" + s)
        dzs = out.get("dzSyN" if dir else "dzSxN")
        for a in (N2, dzo, dzs):                                                        # :174-209
            if a is not None:
                L(a[0])[...] = 0.0
                L(a[nz])[...] = 0.0
        Igrad = L(M[G["IdyCv" if dir else "IdxCu"]])
        mask = L(M[G["mask2dCv" if dir else "mask2dCu"]])
        for k in range(1, nz):                                                          # K = 2..nz (each K on its own)
            hLm, hRm, hLk, hRk = L(h[k - 1]), R(h[k - 1]), L(h[k]), R(h[k])
            if use_EOS:
                TLk, TRk, TLm, TRm = L(Tf[k]), R(Tf[k]), L(Tf[k - 1]), R(Tf[k - 1])
                SLk, SRk, SLm, SRm = L(Sf[k]), R(Sf[k]), L(Sf[k - 1]), R(Sf[k - 1])
                pres_u = 0.5 * (L(pres[k]) + R(pres[k]))                                # :271-273
                T_u = 0.25 * ((TLk + TRk) + (TLm + TRm))
                S_u = 0.25 * ((SLk + SRk) + (SLm + SRm))
                dR_dT, dR_dS = _derivs(orc, eos, T_u, S_u, pres_u)
                drdiA = dR_dT * (TRm - TLm) + dR_dS * (SRm - SLm)                       # :323-332
                drdiB = dR_dT * (TRk - TLk) + dR_dS * (SRk - SLk)
                drdkL = (dR_dT * (TLk - TLm) + dR_dS * (SLk - SLm))
                drdkR = (dR_dT * (TRk - TRm) + dR_dS * (SRk - SRm))
            else:
                drdkL = np.full(hLm.shape, Rlay[k] - Rlay[k - 1])                        # :265
                drdkR = drdkL
            hg2A = hLm * hRm + h_neglect2                                               # :343-352
            hg2B = hLk * hRk + h_neglect2
            hg2L = hLm * hLk + h_neglect2
            hg2R = hRm * hRk + h_neglect2
            haA = 0.5 * (hLm + hRm) + h_neglect
            haB = 0.5 * (hLk + hRk) + h_neglect
            haL = 0.5 * (hLm + hLk) + h_neglect
            haR = 0.5 * (hRm + hRk) + h_neglect
            dzaL = haL * P.H_to_Z
            dzaR = haR * P.H_to_Z
            if dzo is not None:
                L(dzo[k])[...] = 0.5 * (dzaL + dzaR)                                    # :357
            wtA = hg2A * haB                                                            # :360-363
            wtB = hg2B * haA
            wtL = hg2L * (haR * dzaR)
            wtR = hg2R * (haL * dzaL)
            drdz = ((wtL * drdkL) + (wtR * drdkR)) / ((dzaL * wtL) + (dzaR * wtR))
            if N2 is not None:
                L(N2[k])[...] = G_Rho0 * drdz * mask                                    # :381
            eL, eR = L(e[k]), R(e[k])
            if use_EOS:
                drdx = ((wtA * drdiA + wtB * drdiB) / (wtA + wtB) - drdz * (eL - eR)) * Igrad   # :385-395
                zx = P.Z_to_L * drdx
                mag_grad2 = zx * zx + drdz * drdz
                pos = mag_grad2 > 0.0
                if counts is not None:
                    counts["mag_grad2_zero"] += int((~pos).sum())
                sl = np.where(pos, drdx / np.sqrt(np.where(pos, mag_grad2, 1.0)), 0.0)
            else:
                sl = (eR - eL) * Igrad                                                  # :397
            L(slope[k])[...] = sl                                                       # :416
            if dzs is not None:                                                         # :417-420
                arg = (wtL * (dzaL * drdkL)) + (wtR * (dzaR * drdkR))
                if counts is not None:
                    counts["dzSN_clip"] += int((arg > 0.0).sum() < arg.size)
                L(dzs[k])[...] = np.sqrt(G_Rho0 * _dmax(0.0, arg) / (wtL + wtR)) * np.abs(sl) * mask   # (second argument on a tie)


def calc_Eady_growth_rate_2D(d, M, GV, P, e, dzu, dzv, dzSxN, dzSyN, SN_u, SN_v, counts):
    nz = d.nk
    dz_neglect = GV.dZ_subroundoff
    D_scale = P.Eady_GR_D_scale
    if D_scale <= 0.:
        D_scale = 64. * P.max_depth                                                     # :991
    r_crp_dist = 1. / max(dz_neglect, P.cropping_distance)
    crop = P.cropping_distance >= 0.
    box = (-1, d.ni, -1, d.nj)
    _A(d, SN_u, box)[...] = 0.0                                                         # :1002-1005
    _A(d, SN_v, box)[...] = 0.0
    SN_cpy = np.full(SN_u.shape, np.nan)
    for dir in (0, 1):
        rng = (-1, d.ni - 1, -1, d.nj) if dir == 0 else (-1, d.ni, -1, d.nj - 1)
        far = dict(di=1, dj=0) if dir == 0 else dict(di=0, dj=1)
        dzf, dzSN = (dzv, dzSyN) if dir else (dzu, dzSxN)
        mask = _A(d, M[G["mask2dCv" if dir else "mask2dCu"]], rng)
        vint_SN = np.zeros(mask.shape)
        sum_dz = np.full(mask.shape, dz_neglect)
        e1L, e1R = _A(d, e[0], rng), _A(d, e[0], rng, **far)
        ebL, ebR = _A(d, e[nz], rng), _A(d, e[nz], rng, **far)
        for k in range(1, nz):                                                          # K = 2..nz
            dzk = _A(d, dzf[k], rng)
            dnew = sum_dz + dzk
            clipped = D_scale < dnew
            dnew = _min(dnew, D_scale)
            dz = _max(0., dnew - sum_dz)
            counts["Dscale_full"] += int((~clipped).sum())
            counts["Dscale_partial"] += int((clipped & (dz > 0.)).sum())
            counts["Dscale_zero"] += int((clipped & ~(dz > 0.)).sum())
            weight = dz / (dzk + dz_neglect)
            if crop:
                eL, eR = _A(d, e[k], rng), _A(d, e[k], rng, **far)
                dT = _min(e1L, e1R)
                dB = _max(eL, eR)
                f = _min(_max(0., (dT - dB) * r_crp_dist), 1.)
                counts["crop_top_0"] += int((f == 0.).sum()); counts["crop_top_1"] += int((f == 1.).sum())
                counts["crop_top_mid"] += int(((f > 0.) & (f < 1.)).sum())
                weight = weight * f
                dT = _min(eL, eR)
                dB = _max(ebL, ebR)
                f = _min(_max(0., (dT - dB) * r_crp_dist), 1.)
                counts["crop_bot_0"] += int((f == 0.).sum()); counts["crop_bot_1"] += int((f == 1.).sum())
                counts["crop_bot_mid"] += int(((f > 0.) & (f < 1.)).sum())
                weight = weight * f
            if dir == 0:
                vint_SN = vint_SN + weight * _A(d, dzSN[k], rng)                         # :1028
            else:
                vint_SN = vint_SN + weight * weight * _A(d, dzSN[k], rng)                # :1071: weight**2 at the v faces
            sum_dz = sum_dz + weight * dzk
        if dir == 0:
            _A(d, SN_u, rng)[...] = mask * (vint_SN / sum_dz)                           # :1045-1046
            _A(d, SN_cpy, rng)[...] = mask * (vint_SN / sum_dz)
        else:
            _A(d, SN_v, rng)[...] = mask * (vint_SN / sum_dz)                           # :1088
    ru = (-1, d.ni - 1, 0, d.nj - 1)
    v = SN_v
    _A(d, SN_u, ru)[...] = np.sqrt(_A(d, SN_cpy, ru) * _A(d, SN_cpy, ru)                # :1094-1096
                                   + 0.25 * (((_A(d, v, ru) * _A(d, v, ru)) + (_A(d, v, ru, 1, -1) * _A(d, v, ru, 1, -1)))
                                             + ((_A(d, v, ru, 1, 0) * _A(d, v, ru, 1, 0)) + (_A(d, v, ru, 0, -1) * _A(d, v, ru, 0, -1)))))
    rv = (0, d.ni - 1, -1, d.nj - 1)
    c = SN_cpy
    _A(d, SN_v, rv)[...] = np.sqrt(_A(d, v, rv) * _A(d, v, rv)                          # :1101-1103
                                   + 0.25 * (((_A(d, c, rv) * _A(d, c, rv)) + (_A(d, c, rv, -1, 1) * _A(d, c, rv, -1, 1)))
                                             + ((_A(d, c, rv, 0, 1) * _A(d, c, rv, 0, 1)) + (_A(d, c, rv, -1, 0) * _A(d, c, rv, -1, 0)))))


def calc_Visbeck_coeffs_old(d, M, GV, P, h, slope_x, slope_y, N2_u, N2_v, SN_u, SN_v, counts, S2_u=None, S2_v=None):
    nz = d.nk
    S2max = P.Visbeck_S_max * P.Visbeck_S_max                                           # :796
    SN_u[...] = 0.0                                                                     # :798-799
    SN_v[...] = 0.0
    hs2 = GV.H_subroundoff * GV.H_subroundoff
    hsub4 = hs2 * hs2
    h4_u = np.full((nz + 1,) + h.shape[1:], np.nan)
    h4_v = np.full((nz + 1,) + h.shape[1:], np.nan)
    r4u, r4v = (-1, d.ni - 1, -1, d.nj), (-1, d.ni, -1, d.nj - 1)
    for k in range(1, nz):                                                              # :842-849
        _A(d, h4_u[k], r4u)[...] = _A(d, M[G["mask2dCu"]], r4u) * (
            (_A(d, h[k], r4u) * _A(d, h[k], r4u, 1, 0)) * (_A(d, h[k - 1], r4u) * _A(d, h[k - 1], r4u, 1, 0)))
        _A(d, h4_v[k], r4v)[...] = _A(d, M[G["mask2dCv"]], r4v) * (
            (_A(d, h[k], r4v) * _A(d, h[k], r4v, 0, 1)) * (_A(d, h[k - 1], r4v) * _A(d, h[k - 1], r4v, 0, 1)))
    for dir in (0, 1):
        rng = (-1, d.ni - 1, 0, d.nj - 1) if dir == 0 else (0, d.ni - 1, -1, d.nj - 1)
        far = dict(di=1, dj=0) if dir == 0 else dict(di=0, dj=1)
        shp = _A(d, SN_u, rng).shape
        SN, S2s, H_u = np.zeros(shp), np.zeros(shp), np.zeros(shp)
        own, N2 = (slope_y, N2_v) if dir else (slope_x, N2_u)
        for k in range(1, nz):
            Hdn = np.sqrt(_A(d, h[k], rng) * _A(d, h[k], rng, **far))                   # :862-864
            Hup = np.sqrt(_A(d, h[k - 1], rng) * _A(d, h[k - 1], rng, **far))
            H_geom = np.sqrt(Hdn * Hup)
            s0 = _A(d, own[k], rng)
            if dir == 0:                                                                # :867-881
                w, o = h4_v[k], slope_y[k]
                wSE, wNW, wNE, wSW = _A(d, w, rng, 1, -1), _A(d, w, rng), _A(d, w, rng, 1, 0), _A(d, w, rng, 0, -1)
                sSE, sNW, sNE, sSW = _A(d, o, rng, 1, -1), _A(d, o, rng), _A(d, o, rng, 1, 0), _A(d, o, rng, 0, -1)
                S2 = s0 * s0 + (((wNW * (sNW * sNW)) + (wSE * (sSE * sSE))) + ((wNE * (sNE * sNE)) + (wSW * (sSW * sSW)))) / (
                    ((wSE + wNW) + (wNE + wSW)) + hsub4)
            else:                                                                       # :910-924
                w, o = h4_u[k], slope_x[k]
                wSE, wNW, wNE, wSW = _A(d, w, rng), _A(d, w, rng, -1, 1), _A(d, w, rng, 0, 1), _A(d, w, rng, -1, 0)
                sSE, sNW, sNE, sSW = _A(d, o, rng), _A(d, o, rng, -1, 1), _A(d, o, rng, 0, 1), _A(d, o, rng, -1, 0)
                S2 = s0 * s0 + (((wSE * (sSE * sSE)) + (wNW * (sNW * sNW))) + ((wNE * (sNE * sNE)) + (wSW * (sSW * sSW)))) / (
                    ((wSE + wNW) + (wNE + wSW)) + hsub4)
            if S2max > 0.:                                                              # :882
                lim = S2 * S2max / (S2 + S2max)
                counts["S2max_applied"] += int((lim < S2).sum())
                S2 = lim
            else:
                counts["S2max_idle"] += S2.size
            N2k = _A(d, N2[k], rng)
            counts["N2_clipped"] += int((N2k < 0.).sum())
            N2p = _max(0., N2k)                                                         # :884-887
            SN = SN + np.sqrt(S2 * N2p) * H_geom
            S2s = S2s + S2 * H_geom
            H_u = H_u + H_geom
        mask = _A(d, M[G["mask2dCv" if dir else "mask2dCu"]], rng)
        posH = H_u > 0.                                                                 # :889-896
        counts["Hu_le0"] += int((~posH).sum())
        Hsafe = np.where(posH, H_u, 1.0)
        _A(d, SN_v if dir else SN_u, rng)[...] = np.where(posH, mask * SN / Hsafe, 0.0)
        S2o = S2_v if dir else S2_u
        if S2o is not None:
            _A(d, S2o, rng)[...] = np.where(posH, mask * S2s / Hsafe, S2s)


def calc_slope_functions_using_just_e(d, M, GV, P, h, e, g_prime, SN_u, SN_v, counts):
    nz = d.nk
    h_neglect = GV.H_subroundoff
    H_cutoff = float(2 * nz) * (GV.Angstrom_H + h_neglect)                              # :1159-1160
    dZ_cutoff = float(2 * nz) * (P.Angstrom_Z + GV.dZ_subroundoff)
    use_dztot = bool(P.full_depth_Eady_growth_rate)
    rEx, rEy = (-1, d.ni - 1, -1, d.nj), (-1, d.ni, -1, d.nj - 1)
    ru, rv = (-1, d.ni - 1, 0, d.nj - 1), (0, d.ni - 1, -1, d.nj - 1)
    S2N2 = [np.zeros((nz,) + _A(d, SN_u, ru).shape), np.zeros((nz,) + _A(d, SN_v, rv).shape)]
    ks = list(range(nz - 1, P.VarMix_Ktop - 2, -1))                                     # k = nz..VarMix_Ktop
    for k in ks:
        E_x = np.full(h.shape[1:], np.nan)
        E_y = np.full(h.shape[1:], np.nan)
        ex = (_A(d, e[k], rEx, 1, 0) - _A(d, e[k], rEx)) * _A(d, M[G["IdxCu"]], rEx)    # :1189-1196
        mx = _min(_A(d, h[k], rEx), _A(d, h[k], rEx, 1, 0)) < H_cutoff
        _A(d, E_x, rEx)[...] = np.where(mx, 0., ex)
        ey = (_A(d, e[k], rEy, 0, 1) - _A(d, e[k], rEy)) * _A(d, M[G["IdyCv"]], rEy)
        my = _min(_A(d, h[k], rEy), _A(d, h[k], rEy, 0, 1)) < H_cutoff
        _A(d, E_y, rEy)[...] = np.where(my, 0., ey)
        for dir, rng, far in ((0, ru, dict(di=1, dj=0)), (1, rv, dict(di=0, dj=1))):
            if dir == 0:                                                                # :1201-1202
                o = E_y
                a, b, c, e_ = _A(d, o, rng), _A(d, o, rng, 1, -1), _A(d, o, rng, 1, 0), _A(d, o, rng, 0, -1)
                own = _A(d, E_x, rng)
            else:                                                                       # :1212-1213
                o = E_x
                a, b, c, e_ = _A(d, o, rng), _A(d, o, rng, -1, 1), _A(d, o, rng, 0, 1), _A(d, o, rng, -1, 0)
                own = _A(d, E_y, rng)
            S2 = (own * own + 0.25 * (((a * a) + (b * b)) + ((c * c) + (e_ * e_))))
            hLk, hRk, hLm, hRm = _A(d, h[k], rng), _A(d, h[k], rng, **far), _A(d, h[k - 1], rng), _A(d, h[k - 1], rng, **far)
            cut = _min(_min(_min(hLm, hRm), hLk), hRk) < H_cutoff                       # :1203
            counts["H_cutoff_mask"] += int(cut.sum())
            S2 = np.where(cut, 0.0, S2)
            Hdn = 2. * hLk * hLm / (hLk + hLm + h_neglect)                              # :1205-1209
            Hup = 2. * hRk * hRm / (hRk + hRm + h_neglect)
            H_geom = np.sqrt(Hdn * Hup)
            S2N2[dir][k] = (H_geom * S2) * (g_prime[k] / _max(_max(Hdn, Hup), P.h_min_N2))
    dz_tot = e[0] - e[nz]                                                               # :1167
    bT = M[G["bathyT"]]
    for dir, rng, far in ((0, ru, dict(di=1, dj=0)), (1, rv, dict(di=0, dj=1))):
        SN = np.zeros(S2N2[dir].shape[1:])
        for k in ks:                                                                    # :1228-1230
            SN = SN + S2N2[dir][k]
        mask = _A(d, M[G["mask2dCv" if dir else "mask2dCu"]], rng)
        if use_dztot:                                                                   # :1233-1237
            counts["denom_dztot"] += SN.size
            res = mask * np.sqrt(SN / _max(_max(_A(d, dz_tot, rng), _A(d, dz_tot, rng, **far)), GV.dZ_subroundoff))
        else:                                                                           # :1240-1245 (v: bathyT(i,j+1), :1265)
            bL, bR = _A(d, bT, rng), _A(d, bT, rng, **far)
            deep = _min(bL, bR) + 0.0 > dZ_cutoff
            counts["denom_bathy"] += int(deep.sum()); counts["bathy_cutoff"] += int((~deep).sum())
            res = np.where(deep, mask * np.sqrt(SN / np.where(deep, _max(bL, bR) + 0.0, 1.0)), 0.0)
        _A(d, SN_v if dir else SN_u, rng)[...] = res


def calc_slope_functions(d, M, GV, P, h, dt, SN_u, SN_v, T=None, S=None, p_surf=None, eos=None, Rlay=None, g_prime=None,
                         slope_x=None, slope_y=None, diag=None, counts=None, orc=None):
    """Writes SN_u, SN_v, slope_x, slope_y and the arrays of `diag` (any of N2_u, N2_v, dzu, dzv, dzSxN, dzSyN, S2_u, S2_v) in place,
    as mom6x_calc_slope_functions does; returns the branch counts."""
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    diag = diag or {}
    assert all(getattr(P, n) == 0 for n in abi.VARMIX_MUST_BE_0) and P.VarMix_Ktop >= 2
    if not P.calculate_Eady_growth_rate:                                                # :708
        return counts
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = find_eta(d, M, h, P.H_to_Z)                                                 # :709
        shp = (d.nk + 1,) + h.shape[1:]
        if P.use_simpler_Eady_growth_rate:                                              # :710-714
            assert P.use_stored_slopes
            out = dict(slope_x=slope_x, slope_y=slope_y)
            for n in ("N2_u", "N2_v", "dzu", "dzv", "dzSxN", "dzSyN"):
                out[n] = diag[n] if diag.get(n) is not None else np.full(shp, np.nan)
            calc_isoneutral_slopes(d, M, GV, P, h, e, dt * P.kappa_smooth, out, T=T, S=S, p_surf=p_surf, eos=eos, Rlay=Rlay,
                                   counts=counts, orc=orc)
            calc_Eady_growth_rate_2D(d, M, GV, P, e, out["dzu"], out["dzv"], out["dzSxN"], out["dzSyN"], SN_u, SN_v, counts)
        elif P.use_stored_slopes:                                                       # :715-719
            out = dict(slope_x=slope_x, slope_y=slope_y)
            for n in ("N2_u", "N2_v"):
                out[n] = diag[n] if diag.get(n) is not None else np.full(shp, np.nan)
            calc_isoneutral_slopes(d, M, GV, P, h, e, dt * P.kappa_smooth, out, T=T, S=S, p_surf=p_surf, eos=eos, Rlay=Rlay,
                                   counts=counts, orc=orc)
            calc_Visbeck_coeffs_old(d, M, GV, P, h, slope_x, slope_y, out["N2_u"], out["N2_v"], SN_u, SN_v, counts,
                                    S2_u=diag.get("S2_u"), S2_v=diag.get("S2_v"))
        else:                                                                           # :721
            calc_slope_functions_using_just_e(d, M, GV, P, h, e, g_prime, SN_u, SN_v, counts)
    return counts


def varmix_L2(d, M, P):
    """CS%L2u, CS%L2v of VarMix_init (:1759-1772)."""
    L2u, L2v = np.zeros(d.shape2()), np.zeros(d.shape2())
    if P.Visbeck_L_scale < 0:
        t = P.L_to_m * P.Visbeck_L_scale
        ru, rv = (-1, d.ni - 1, 0, d.nj - 1), (0, d.ni - 1, -1, d.nj - 1)
        _A(d, L2u, ru)[...] = (t * t) * _A(d, M[G["areaCu"]], ru)
        _A(d, L2v, rv)[...] = (t * t) * _A(d, M[G["areaCv"]], rv)
    else:
        L2u[...] = P.Visbeck_L_scale * P.Visbeck_L_scale
        L2v[...] = P.Visbeck_L_scale * P.Visbeck_L_scale
    return L2u, L2v


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_varmix_cpu.py and tests/test_varmix_gpu.py

def inputs(d, M, GV, seed=5, strat=1.0, uniform_patch=False, thin_top=False):
    """h, T (a stratification scaled by `strat`), S and p_surf of tests/setvisc_ref.inputs with its band of Angstrom-thin bottom
    layers taken across the whole width of the array (two halo points are read here; global rows, so that a tile of any layout sees
    its part of the one-tile state); with `uniform_patch` T and S are uniform in a block of columns (mag_grad2 == 0 when nothing is
    smoothed); with `thin_top` the two top layers of a second band of rows are Angstrom thin (interfaces that outcrop: the upper
    cropping factor of calc_Eady_growth_rate_2D reaches 0)."""
    from tests import setvisc_ref
    b = setvisc_ref.inputs(d, M, GV, seed=seed, strat=strat, vanish=False)
    h, T, S = b["h"].copy(), b["T"], b["S"]
    il = np.arange(d.pitch) - d.ioff + d.i_glob0
    jl = np.arange(d.shape2()[0]) - d.joff + d.j_glob0
    if d.nk > 2:
        band = ((jl >= d.nj_glob // 3) & (jl <= d.nj_glob // 2))[:, None] & np.ones(d.pitch, bool)[None, :]
        for k in (d.nk - 2, d.nk - 1):
            h[k] = np.where(band, GV.Angstrom_H, h[k])
    if thin_top and d.nk > 3:
        band = ((jl >= 3) & (jl <= 6))[:, None] & np.ones(d.pitch, bool)[None, :]
        for k in (0, 1):
            h[k] = np.where(band, GV.Angstrom_H, h[k])
    if uniform_patch:
        patch = ((jl >= 8) & (jl <= 14))[:, None] & ((il >= 20) & (il <= 30))[None, :]
        T = np.where(patch[None], 8.0, T)
        S = np.where(patch[None], 35.0, S)
    return dict(h=np.ascontiguousarray(h), T=np.ascontiguousarray(T), S=np.ascontiguousarray(S), p_surf=b["p_surf"])


DIAG3 = ("N2_u", "N2_v", "dzu", "dzv", "dzSxN", "dzSyN")
DIAG2 = ("S2_u", "S2_v")
EADY = dict(use_stored_slopes=1, use_simpler_Eady_growth_rate=1)
VISB = dict(use_stored_slopes=1)
# case -> (params members, EOS form, None or "form" (each of the eight), given p_surf, given diagnostics, dt, input options)
CASES = {
    "eady": (dict(EADY), "form", False, False, 900.0, dict(thin_top=True)),
    "eady_diag": (dict(EADY, Eady_GR_D_scale=500.0, cropping_distance=50.0), abi.WRIGHT, True, True, 900.0, dict(thin_top=True)),
    "eady_nocrop": (dict(EADY, Eady_GR_D_scale=150.0, cropping_distance=-1.0, kappa_smooth=0.0), abi.WRIGHT, False, False, 900.0,
                    dict(uniform_patch=True)),
    # T and S uniform in a patch and never smoothed under a linear equation of state with both coefficients negative: both vertical
    # density differences are -0.0 there, and the radicand of dzSxN is MAX(0.0, -0.0)
    "eady_tie": (dict(EADY, kappa_smooth=0.0), abi.LINEAR, False, True, 900.0, dict(uniform_patch=True, eos_mods=dict(dRho_dT=-0.25, dRho_dS=-0.75))),
    "eady_noeos": (dict(EADY, Eady_GR_D_scale=1000.0, cropping_distance=200.0), None, False, True, 900.0, dict(thin_top=True)),
    "visbeck": (dict(VISB), "form", False, False, 900.0, {}),
    "visbeck_diag": (dict(VISB, Visbeck_S_max=1.0e-3), abi.WRIGHT, True, True, 900.0, {}),
    "visbeck_neg": (dict(VISB, kappa_smooth=0.0), abi.WRIGHT, False, False, 900.0, dict(strat=-1.0, uniform_patch=True)),
    "visbeck_noeos": (dict(VISB, Visbeck_S_max=1.0e-4), None, False, True, 3600.0, {}),
    "just_e": (dict(), None, False, False, 900.0, {}),
    "just_e_full": (dict(full_depth_Eady_growth_rate=1, VarMix_Ktop=3, h_min_N2=50.0), None, False, False, 900.0, {}),
}
FORMS = (abi.LINEAR, abi.WRIGHT, abi.WRIGHT_FULL, abi.WRIGHT_REDUCED, abi.UNESCO, abi.ROQUET_RHO, abi.JACKETT06, abi.ROQUET_SPV)


def case_list(forms=FORMS):
    """(name, form) of every case, the "form" cases once per EOS form."""
    out = []
    for n, c in CASES.items():
        out += [(n, f) for f in forms] if c[1] == "form" else [(n, None)]
    return out


def case(name, GV, form=None, nk=None):
    mods, eos_form, give_ps, give_diag, dt, opts = CASES[name]
    P = abi.varmix_params_default(GV)
    for k, val in mods.items():
        setattr(P, k, val)
    if nk is not None and P.VarMix_Ktop > max(nk, 2):
        P.VarMix_Ktop = max(nk, 2)
    if eos_form == "form":
        eos_form = form
    eos = abi.eos_params_default(eos_form) if eos_form is not None else None
    opts = dict(opts)
    for k, val in opts.pop("eos_mods", {}).items():
        setattr(eos, k, val)
    return P, eos, give_ps, give_diag, dt, opts


def outputs(d, P, give_diag, fill=np.nan):
    """The output arrays of one call, filled with `fill`."""
    out = dict(SN_u=np.full(d.shape2(), fill), SN_v=np.full(d.shape2(), fill))
    if P.use_stored_slopes:
        out.update(slope_x=np.full(d.shape3(d.nk + 1), fill), slope_y=np.full(d.shape3(d.nk + 1), fill))
    if give_diag:
        out.update({n: np.full(d.shape3(d.nk + 1), fill) for n in DIAG3})
        out.update({n: np.full(d.shape2(), fill) for n in DIAG2})
    return out


def run(d, M, GV, P, inp, dt, eos=None, give_ps=False, give_diag=False, fill=np.nan, orc=None, Rlay=None, g_prime=None):
    """The restatement on the inputs; every output starts as `fill`.  Returns (outputs, counts)."""
    if Rlay is None:
        Rlay, g_prime = abi.layer_densities(d.nk, Rho0=GV.Rho0, g_Earth=GV.g_Earth)
    out = outputs(d, P, give_diag, fill)
    counts = calc_slope_functions(d, M, GV, P, inp["h"], dt, out["SN_u"], out["SN_v"], T=inp["T"], S=inp["S"],
                                  p_surf=inp["p_surf"] if give_ps else None, eos=eos, Rlay=Rlay, g_prime=g_prime,
                                  slope_x=out.get("slope_x"), slope_y=out.get("slope_y"),
                                  diag={n: out[n] for n in DIAG3 + DIAG2} if give_diag else None, orc=orc)
    return out, counts
