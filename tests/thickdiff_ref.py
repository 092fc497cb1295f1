"""The checker of mom6x_thickness_diffuse: a numpy restatement of thickness_diffuse and thickness_diffuse_full
(src/parameterizations/lateral/MOM_thickness_diffuse.F90:134-630, :635-1671) on a Boussinesq grid without the FGNV
streamfunction, with find_eta (src/core/MOM_interface_heights.F90:91-97) and vert_fill_TS
(src/core/MOM_isopycnal_slopes.F90:612-700, larger_h_denom = .true.; both from tests/ref_common.py), written from the
Fortran operation for operation (x**2 as x*x, nothing reordered) and vectorised over the faces of one direction with a loop
over K.  Arrays are in the pitched tile layout of include/mom6x.h ([k, j + joff, i + ioff]).  Density derivatives come from the
oracle's EOS only (oracle/orc.py eos_density_derivs), one point at a time.  MAX and MIN return their first argument on a tie,
which decides the sign of a zero, except in the limiter of uhD and vhD (:1160-1161, :1479), where the tie shows: with no
transport and no available mass beyond the face, MAX(+0.0, -0.0), the compiled reference answers with its second argument, -0.0,
in uhGM and vhGM.  `counts` records how often each branch fired.

tests/test_thickness_diffuse_cpu.py holds this module to facts that do not come from it (closed forms, exact column sums,
bounds, the quarter turn, unit scaling); tests/test_ref_parity_cpu.py holds it bit for bit to the reference's own
MOM_thickness_diffuse.F90, compiled into oracle/_ref/libref_param.so with MOM_lateral_mixing_coeffs.F90, MOM_isopycnal_slopes.F90
and MOM_interface_heights.F90 (every case but khth2d, whose plane the reference reads from a file into a private member), and
tests/golden/ref_thickdiff_*.npz hold the device to what that library gave."""
import numpy as np

from mom6_amd import abi
from tests.ref_common import _derivs, _dmax, _dmin, _faces, _max, _min, find_eta, pressure_column, vert_fill_TS

G = abi.G
BRANCHES = ("bottom_zero_pos", "bottom_zero_neg", "bottom_scale_pos", "bottom_scale_neg", "mag_grad2_zero", "rsum_clip_lo",
            "rsum_clip_hi", "havail_clip_hi", "havail_clip_lo", "uhtot_le0", "uhtot_gt0", "hfrac_zero", "KH_cfl", "KH_max",
            "kap_zero", "angstrom_floor")


def thickness_diffuse(d, M, GV, P, h, uhtr, vhtr, dt, T=None, S=None, p_surf=None, eos=None, khth2d=None, slope_x=None,
                      slope_y=None, uhGM=None, vhGM=None, counts=None, orc=None, diag=None):
    """Updates h, uhtr, vhtr (and uhGM, vhGM) in place, as mom6x_thickness_diffuse does; returns the branch counts.  `diag`, a
    dict, receives uhD, vhD and h_avail."""
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    if (not P.thickness_diffuse) or not (P.Khth > 0.0 or P.read_khth):   # :195-197
        return counts
    assert all(getattr(P, n) == 0 for n in abi.THICKNESS_DIFFUSE_MUST_BE_0) and P.max_Khth_CFL > 0.0
    use_EOS = eos is not None
    stored = slope_x is not None
    calc_derivatives = use_EOS and not stored                    # :924-925 (no find_work, FGNV or Stanley)
    if calc_derivatives and orc is None:
        from oracle import orc
    nz = d.nk
    I4dt = 0.25 / dt                                             # :818
    I_slope_max2 = 1.0 / (P.slope_max * P.slope_max)             # :819
    h_neglect = GV.H_subroundoff
    h_neglect2 = h_neglect * h_neglect
    dz_neglect = GV.dZ_subroundoff
    int_slope = 0.0                                              # :472-474
    aT = M[G["areaT"]]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = find_eta(d, M, h, GV.H_to_Z)
        if calc_derivatives:                                     # :850-853
            Tf, Sf = vert_fill_TS(h, T, S, P.kappa_smooth * dt, GV, P.Z_to_H_fill, True, counts)
        # the column pass :864-882
        h_avail = np.empty_like(h)
        h_frac = np.empty_like(h)
        rsum = np.empty_like(e)
        pres = pressure_column(h, p_surf, GV.g_Earth * GV.H_to_RZ)
        rsum[0] = 0.0
        h_avail[0] = _max(I4dt * aT * (h[0] - GV.Angstrom_H), 0.0)
        rsum[1] = h_avail[0]
        h_frac[0] = 1.0
        for k in range(1, nz):
            h_avail[k] = _max(I4dt * aT * (h[k] - GV.Angstrom_H), 0.0)
            rsum[k + 1] = rsum[k] + h_avail[k]
            h_frac[k] = np.where(h_avail[k] > 0.0, h_avail[k] / rsum[k + 1], 0.0)
        counts["hfrac_zero"] += int((h_avail[1:][(slice(None),) + d.sl(0, d.ni - 1, 0, d.nj - 1)] <= 0.0).sum())

        hD = [np.zeros_like(h), np.zeros_like(h)]
        for dir in (0, 1):
            (r0, r1), (c0, c1_), (oj, oi) = _faces(d, dir)

            def F(a, right=False):
                dj, di = (oj, oi) if right else (0, 0)
                return a[..., r0 + dj:r1 + dj, c0 + di:c1_ + di]

            Idx = F(M[G["IdxCv" if dir else "IdxCu"]])
            Idy = F(M[G["IdyCv" if dir else "IdyCu"]])
            KH_CFL = (0.25 * P.max_Khth_CFL) / (dt * ((Idx * Idx) + (Idy * Idy)))   # :226, :231
            if not P.read_khth:
                Kh_loc = np.full(Idx.shape, P.Khth)              # :243
            else:
                Kh_loc = 0.5 * (F(khth2d) + F(khth2d, True))     # :248, :351
            if P.Khth_Max > 0:                                   # :291-301
                counts["KH_max"] += int((Kh_loc > P.Khth_Max).sum())
                Kh_loc = _max(P.Khth_Min, _min(Kh_loc, P.Khth_Max))
            else:
                Kh_loc = _max(P.Khth_Min, Kh_loc)
            counts["KH_cfl"] += int((KH_CFL < Kh_loc).sum())
            KH = _min(KH_CFL, Kh_loc)                            # :304
            KHlen = KH * F(M[G["dx_Cv" if dir else "dy_Cu"]])
            Igrad = Idy if dir else Idx
            mask = F(M[G["mask2dCv" if dir else "mask2dCu"]])
            slope = slope_y if dir else slope_x
            ebL, ebR = F(e[nz]), F(e[nz], True)
            uhtot = np.zeros(Idx.shape)
            D3 = hD[dir]
            for k in range(nz - 1, 0, -1):                       # K = nz..2 (k + 1 in the Fortran's numbering)
                eL, eR, elL, elR = F(e[k]), F(e[k], True), F(e[k + 1]), F(e[k + 1], True)
                hLk, hRk, hLm, hRm = F(h[k]), F(h[k], True), F(h[k - 1]), F(h[k - 1], True)
                if use_EOS:
                    if calc_derivatives:
                        TLk, TRk, TLm, TRm = F(Tf[k]), F(Tf[k], True), F(Tf[k - 1]), F(Tf[k - 1], True)
                        SLk, SRk, SLm, SRm = F(Sf[k]), F(Sf[k], True), F(Sf[k - 1]), F(Sf[k - 1], True)
                        pres_u = 0.5 * (F(pres[k]) + F(pres[k], True))                   # :930-932
                        T_u = 0.25 * ((TLk + TRk) + (TLm + TRm))
                        S_u = 0.25 * ((SLk + SRk) + (SLm + SRm))
                        dR_dT, dR_dS = _derivs(orc, eos, T_u, S_u, pres_u)
                        drdiA = dR_dT * (TRm - TLm) + dR_dS * (SRm - SLm)               # :954-963
                        drdiB = dR_dT * (TRk - TLk) + dR_dS * (SRk - SLk)
                        drdkL = (dR_dT * (TLk - TLm) + dR_dS * (SLk - SLm))
                        drdkR = (dR_dT * (TRk - TRm) + dR_dS * (SRk - SRm))
                        hg2L = hLm * hLk + h_neglect2                                   # :981-1005
                        hg2R = hRm * hRk + h_neglect2
                        haL = 0.5 * (hLm + hLk) + h_neglect
                        haR = 0.5 * (hRm + hRk) + h_neglect
                        dzaL = haL * GV.H_to_Z
                        dzaR = haR * GV.H_to_Z
                        wtL = hg2L * (haR * dzaR)
                        wtR = hg2R * (haL * dzaL)
                        drdz = ((wtL * drdkL) + (wtR * drdkR)) / ((dzaL * wtL) + (dzaR * wtR))
                        hg2A = hLm * hRm + h_neglect2
                        hg2B = hLk * hRk + h_neglect2
                        haA = 0.5 * (hLm + hRm) + h_neglect
                        haB = 0.5 * (hLk + hRk) + h_neglect
                        wtA = hg2A * haB                                                # :1030-1044
                        wtB = hg2B * haA
                        drdx = ((wtA * drdiA + wtB * drdiB) / (wtA + wtB) - drdz * (eL - eR)) * Igrad
                        zx = P.Z_to_L * drdx
                        mag_grad2 = zx * zx + drdz * drdz
                        pos = mag_grad2 > 0.0
                        counts["mag_grad2_zero"] += int((~pos).sum())
                        Slope = np.where(pos, drdx / np.sqrt(mag_grad2), 0.0)
                        ratio = np.where(pos, Slope * Slope * I_slope_max2, 1.0e20)
                    else:
                        Slope = F(slope[k])                                             # :1025-1026
                        ratio = Slope * Slope * I_slope_max2
                    Slope = (1.0 - int_slope) * Slope + int_slope * ((eR - eL) * Igrad)  # :1049-1051
                    ratio = (1.0 - int_slope) * ratio
                    Sfn_unlim = -(KHlen) * Slope                                        # :1063
                    p = Sfn_unlim > 0.0                                                 # :1067-1083
                    zp = p & (eL < ebR)
                    sp = p & ~zp & (ebR > elL)
                    zn = ~p & (eR < ebL)
                    sn = ~p & ~zn & (ebL > elR)
                    neg = Sfn_unlim < 0.0
                    counts["bottom_zero_pos"] += int(zp.sum()); counts["bottom_scale_pos"] += int(sp.sum())
                    counts["bottom_zero_neg"] += int((zn & neg).sum()); counts["bottom_scale_neg"] += int((sn & neg).sum())
                    scp = Sfn_unlim * ((eL - ebR) / ((eL - elL) + dz_neglect))
                    scn = Sfn_unlim * ((eR - ebL) / ((eR - elR) + dz_neglect))
                    Sfn_unlim = np.where(zp | zn, 0.0, np.where(sp, scp, np.where(sn, scn, Sfn_unlim)))
                else:
                    if stored:
                        Slope = F(slope[k])                                             # :1087
                    else:
                        Slope = ((eR - eL) * Igrad) * mask                              # :1089
                    Sfn_unlim = -(KHlen) * Slope                                        # :1092
                haL_, haR_ = F(h_avail[k]), F(h_avail[k], True)
                if use_EOS:                                                             # :1141-1149
                    le = uhtot <= 0.0
                    counts["uhtot_le0"] += int(le.sum()); counts["uhtot_gt0"] += int((~le).sum())
                    Sfn_safe = np.where(le, uhtot * (1.0 - F(h_frac[k])), uhtot * (1.0 - F(h_frac[k], True)))
                    Sfn_est = (GV.Z_to_H * Sfn_unlim + ratio * Sfn_safe) / (1.0 + ratio)
                else:
                    Sfn_est = GV.Z_to_H * Sfn_unlim                                     # :1151
                rL, rR = F(rsum[k]), F(rsum[k], True)
                lo = _max(Sfn_est, -rL)                                                 # :1156
                counts["rsum_clip_lo"] += int((-rL > Sfn_est).sum())
                counts["rsum_clip_hi"] += int((rR < lo).sum())
                Sfn_in_H = _min(lo, rR)
                t = _dmin((Sfn_in_H - uhtot), haL_)                                     # :1160-1161: second argument on a tie
                counts["havail_clip_hi"] += int((haL_ < (Sfn_in_H - uhtot)).sum())
                counts["havail_clip_lo"] += int((-haR_ > t).sum())
                D = _dmax(t, -haR_)                                                     # (MAX(+0.0, -0.0) is -0.0 in uhGM)
                uhtot = uhtot + D                                                       # :1190
                F(D3[k])[...] = D
            F(D3[0])[...] = -uhtot                                                      # :1534-1535

        uhD, vhD = hD
        for dir, tr, GM in ((0, uhtr, uhGM), (1, vhtr, vhGM)):                          # :600-609
            (r0, r1), (c0, c1_), _ = _faces(d, dir)
            sl = (slice(None), slice(r0, r1), slice(c0, c1_))
            tr[sl] = tr[sl] + hD[dir][sl] * dt
            if GM is not None:
                GM[sl] = hD[dir][sl]
        sl = d.sl(0, d.ni - 1, 0, d.nj - 1)
        j0, j1, i0, i1 = sl[0].start, sl[0].stop, sl[1].start, sl[1].stop
        div = ((uhD[:, j0:j1, i0:i1] - uhD[:, j0:j1, i0 - 1:i1 - 1]) + (vhD[:, j0:j1, i0:i1] - vhD[:, j0 - 1:j1 - 1, i0:i1]))
        hn = h[:, j0:j1, i0:i1] - dt * M[G["IareaT"]][sl] * div                         # :611-613
        fl = hn < GV.Angstrom_H
        counts["angstrom_floor"] += int(fl.sum())
        h[:, j0:j1, i0:i1] = np.where(fl, GV.Angstrom_H, hn)
    if diag is not None:
        diag.update(uhD=uhD, vhD=vhD, h_avail=h_avail)
    return counts


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_thickness_diffuse_cpu.py and tests/test_thickness_diffuse_gpu.py

def inputs(d, M, GV, seed=5, uniform_patch=False, thin_top=False):
    """tests/setvisc_ref.inputs as they are (h with a band of Angstrom-thin bottom layers, T, S, p_surf) plus uhtr, vhtr, a
    khth2d field and stored slopes; with `uniform_patch` T and S are uniform in a block of columns (mag_grad2 == 0); with
    `thin_top` the two top layers of a band of rows are Angstrom thin (no mass is available above their interfaces: the
    h_avail_rsum clips of :1156 fire at a few layers, which otherwise takes 75)."""
    from mom6_amd import synth
    from tests import setvisc_ref
    b = setvisc_ref.inputs(d, M, GV, seed=seed)
    out = dict(h=b["h"], T=b["T"], S=b["S"], p_surf=b["p_surf"])
    out["uhtr"] = np.ascontiguousarray(1.0e6 * synth.smooth_field(d, seed + 400, nk=d.nk, ox=1.0, oy=0.5))
    out["vhtr"] = np.ascontiguousarray(1.0e6 * synth.smooth_field(d, seed + 401, nk=d.nk, ox=0.5, oy=1.0))
    out["khth2d"] = np.ascontiguousarray(600.0 * (1.0 + 0.5 * synth.smooth_field(d, seed + 402, ox=0.5, oy=0.5)))
    out["slope_x"] = np.ascontiguousarray(2.0e-3 * synth.smooth_field(d, seed + 403, nk=d.nk + 1, ox=1.0, oy=0.5))
    out["slope_y"] = np.ascontiguousarray(2.0e-3 * synth.smooth_field(d, seed + 404, nk=d.nk + 1, ox=0.5, oy=1.0))
    if thin_top and d.nk > 3:
        jl = np.arange(d.shape2()[0]) - d.joff + d.j_glob0
        band = ((jl >= 3) & (jl <= 6))[:, None] & np.ones(d.pitch, bool)[None, :]
        h = out["h"].copy()
        for k in (0, 1):
            h[k] = np.where(band, GV.Angstrom_H, h[k])
        out["h"] = np.ascontiguousarray(h)
    if uniform_patch:
        il = np.arange(d.pitch) - d.ioff + d.i_glob0
        jl = np.arange(d.shape2()[0]) - d.joff + d.j_glob0
        patch = ((jl >= 8) & (jl <= 14))[:, None] & ((il >= 20) & (il <= 30))[None, :]
        out["T"] = np.ascontiguousarray(np.where(patch[None], 8.0, out["T"]))
        out["S"] = np.ascontiguousarray(np.where(patch[None], 35.0, out["S"]))
    return out


# case -> (params members, EOS form, None or "form" (each of the eight), given p_surf, stored slopes, given uhGM/vhGM, dt, input options)
CASES = {
    "noeos": (dict(), None, False, False, False, 900.0, {}),
    "eos": (dict(), "form", False, False, False, 900.0, {}),
    "psurf": (dict(), abi.WRIGHT, True, False, False, 900.0, {}),
    "slopes_eos": (dict(), abi.WRIGHT, False, True, False, 900.0, {}),
    "slopes_noeos": (dict(), None, False, True, False, 900.0, {}),
    "khth2d": (dict(Khth=0.0, read_khth=1), abi.WRIGHT, False, False, False, 900.0, {}),
    "kmax": (dict(Khth=600.0, Khth_Max=300.0, Khth_Min=50.0), abi.WRIGHT, False, False, False, 900.0, {}),
    "kmin": (dict(Khth=10.0, Khth_Min=200.0), None, False, False, False, 900.0, {}),
    "large": (dict(Khth=1.0e7), abi.WRIGHT, False, False, False, 3600.0, {}),
    "large_noeos": (dict(Khth=1.0e7), None, False, False, False, 3600.0, {}),
    "kd0": (dict(kappa_smooth=0.0), abi.WRIGHT, False, False, False, 900.0, dict(uniform_patch=True)),
    "gm": (dict(), abi.WRIGHT, False, False, True, 900.0, {}),
    "thin_top": (dict(Khth=1.0e7), abi.WRIGHT, False, False, False, 3600.0, dict(thin_top=True)),
}


def case(name, form=None):
    mods, eos_form, give_ps, stored, give_gm, dt, opts = CASES[name]
    P = abi.thickness_diffuse_params_default()
    for k, val in mods.items():
        setattr(P, k, val)
    if eos_form == "form":
        eos_form = form
    eos = abi.eos_params_default(eos_form) if eos_form is not None else None
    return P, eos, give_ps, stored, give_gm, dt, opts


def run(d, M, GV, P, inp, dt, eos=None, give_ps=False, stored=False, give_gm=False, fill=np.nan, orc=None, diag=None):
    """The restatement on copies of the inputs; uhGM, vhGM start as `fill`.  Returns (outputs, counts)."""
    out = dict(h=inp["h"].copy(), uhtr=inp["uhtr"].copy(), vhtr=inp["vhtr"].copy())
    gm = dict(uhGM=np.full(d.shape3(), fill), vhGM=np.full(d.shape3(), fill)) if give_gm else {}
    counts = thickness_diffuse(d, M, GV, P, out["h"], out["uhtr"], out["vhtr"], dt, T=inp["T"], S=inp["S"],
                               p_surf=inp["p_surf"] if give_ps else None, eos=eos, khth2d=inp["khth2d"] if P.read_khth else None,
                               slope_x=inp["slope_x"] if stored else None, slope_y=inp["slope_y"] if stored else None, orc=orc,
                               diag=diag, **gm)
    out.update(gm)
    return out, counts
