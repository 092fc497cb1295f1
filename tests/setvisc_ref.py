"""The checker of mom6x_set_viscous_BBL: a numpy restatement of the non-channel, Boussinesq path of set_viscous_BBL
(src/parameterizations/vertical/MOM_set_viscosity.F90:135-1115), vectorised over the faces of one direction, with a loop over k
and masks for the lanes still in each walk.  Arrays are in the pitched tile layout of include/mom6x.h ([k, j + joff, i + ioff]).

The arithmetic is the reference's, operation for operation (x**2 written as x*x; no operation is reordered), so that the device
result can be held to it bit for bit.  The density derivatives come from the oracle's EOS (oracle/orc.py eos_density_derivs, the
restatement pinned to the reference's EOS_unit_tests), one face at a time.  `counts` records how often each branch fired, so that
a test can show the branches it claims to cover were reached."""
import numpy as np

from mom6_amd import abi
from tests.ref_common import _faces

G = abi.G
BRANCHES = ("vanished_skip", "frac_used", "layer1_eos", "layer1_rlay", "thick_min", "correct_bounds", "RiNo_cap", "body_force",
            "no_weight")


def _min(a, b):
    """Fortran MIN(a, b) of two reals, b on a tie: dmin on the device (set_visc.hip), not the _min of tests/ref_common.py."""
    return np.where(a < b, a, b)


def set_viscous_BBL(d, M, GV, P, u, v, h, T=None, S=None, p_surf=None, eos=None, tideamp=None, Rlay=None, Kv_bbl_u=None,
                    Kv_bbl_v=None, bbl_thick_u=None, bbl_thick_v=None, Ray_u=None, Ray_v=None, counts=None, orc=None):
    """Fills the given output arrays in place, as mom6x_set_viscous_BBL does; returns the branch counts."""
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    if not P.bottomdraglaw:                                      # :323
        return counts
    assert not P.channel_drag and P.nkml == 0 and not P.open_bcs and not P.ice_shelf and not P.SpV_avg
    use_EOS = eos is not None and bool(P.BBL_use_EOS)           # :340
    if use_EOS and orc is None:
        from oracle import orc
    nz = d.nk
    h_neglect, dz_neglect = GV.H_subroundoff, GV.dZ_subroundoff
    Rho0x400_G = 400.0 * (GV.H_to_RZ / ((P.L_to_Z * P.L_to_Z) * GV.g_Earth))   # :331, MOM_verticalGrid.F90:178
    cdrag_sqrt = np.sqrt(P.cdrag)                               # :343
    cdrag_sqrt_H = cdrag_sqrt * P.L_to_H                        # :344
    cdrag_L_to_H = P.cdrag * P.L_to_H                           # :346
    BBL_thick_max = P.Rad_Earth * P.L_to_Z                      # :348
    HRg = GV.H_to_RZ * GV.g_Earth
    if Ray_u is not None:                                       # :442-443
        Ray_u[...] = 0.0
        Ray_v[...] = 0.0
    Mq = M[G["CoriolisBu"]]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for dir in (0, 1):                                      # m = 1, 2 (:450)
            (r0, r1), (c0, c1), (oj, oi) = _faces(d, dir)

            def F(a, dj=0, di=0):
                return a[..., r0 + dj:r1 + dj, c0 + di:c1 + di]

            vel, oth = (u, v) if dir == 0 else (v, u)
            do_i = F(M[G["mask2dCv" if dir else "mask2dCu"]]) > 0.0    # :453-464
            mO = M[G["mask2dCu" if dir else "mask2dCv"]]

            def at_vel(k):                                      # :470-479 / :494-503, dz = H_to_Z*h (:352)
                hL, hR = F(h[k]), F(h[k], oj, oi)
                dzL, dzR = GV.H_to_Z * hL, GV.H_to_Z * hR
                up = F(vel[k]) * (hR - hL) >= 0
                h_at = np.where(up, 2.0 * hL * hR / (hL + hR + h_neglect), 0.5 * (hL + hR))
                dz_at = np.where(up, 2.0 * dzL * dzR / (dzL + dzR + dz_neglect), 0.5 * (dzL + dzR))
                return h_at, dz_at

            def TS_vel(k):                                      # :485-487
                return 0.5 * (F(T[k]) + F(T[k], oj, oi)), 0.5 * (F(S[k]) + F(S[k], oj, oi))

            def other_at_face(k):                               # set_v_at_u :1819-1860 / set_u_at_v :1863-1906
                hk, ok = h[k], oth[k]
                if dir == 0:
                    w0m = (F(hk, -1, 0) + F(hk)) * F(mO, -1, 0)
                    w1m = (F(hk, -1, 1) + F(hk, 0, 1)) * F(mO, -1, 1)
                    w00 = (F(hk) + F(hk, 1, 0)) * F(mO)
                    w10 = (F(hk, 0, 1) + F(hk, 1, 1)) * F(mO, 0, 1)
                    tot = (w0m + w10) + (w1m + w00)
                    num = ((w00 * F(ok)) + (w1m * F(ok, -1, 1))) + ((w10 * F(ok, 0, 1)) + (w0m * F(ok, -1, 0)))
                else:
                    wm0 = (F(hk, 0, -1) + F(hk)) * F(mO, 0, -1)
                    w00 = (F(hk) + F(hk, 0, 1)) * F(mO)
                    wm1 = (F(hk, 1, -1) + F(hk, 1, 0)) * F(mO, 1, -1)
                    w01 = (F(hk, 1, 0) + F(hk, 1, 1)) * F(mO, 1, 0)
                    tot = (wm0 + w01) + (w00 + wm1)
                    num = ((w00 * F(ok)) + (wm1 * F(ok, 1, -1))) + ((wm0 * F(ok, 0, -1)) + (w01 * F(ok, 1, 0)))
                return np.where(tot > 0.0, num / tot, 0.0)

            # u2_bg (:609-621)
            if P.BBL_use_tidal_bg:
                mT = M[G["mask2dT"]]
                tL, tR = F(tideamp), F(tideamp, oj, oi)
                u2_bg = 0.5 * (F(mT) * (tL * tL) + F(mT, oj, oi) * (tR * tR))
            else:
                u2_bg = np.full(do_i.shape, P.drag_bg_vel * P.drag_bg_vel)

            # the near-bottom walk over at most Hbbl (:623-700)
            z = np.zeros(do_i.shape)
            umag_avg, h_bbl_drag, dz_bbl_drag, T_EOS, S_EOS = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
            if use_EOS or P.body_force_drag or not P.linear_drag:
                htot_vel, hwtot, hutot, dztot_vel, dzwtot, Thtot, Shtot = (z.copy() for _ in range(7))
                act = do_i.copy()
                for k in range(nz - 1, -1, -1):
                    act &= ~(htot_vel >= P.Hbbl)                # exit
                    h_at, dz_at = at_vel(k)
                    hweight = _min(P.Hbbl - htot_vel, h_at)
                    skip = act & (hweight < 1.5 * GV.Angstrom_H + h_neglect)   # cycle
                    counts["vanished_skip"] += int(skip.sum())
                    go = act & ~skip
                    dzweight = _min(P.dz_bbl - dztot_vel, dz_at)
                    htot_vel = np.where(go, htot_vel + h_at, htot_vel)
                    hwtot = np.where(go, hwtot + hweight, hwtot)
                    dztot_vel = np.where(go, dztot_vel + dz_at, dztot_vel)
                    dzwtot = np.where(go, dzwtot + dzweight, dzwtot)
                    g2 = go & (hweight >= 0.0)
                    if not P.linear_drag:
                        w = F(vel[k]); a = other_at_face(k)
                        hutot = np.where(g2, hutot + hweight * np.sqrt(w * w + a * a + u2_bg), hutot)
                    if use_EOS:
                        Tv, Sv = TS_vel(k)
                        Thtot = np.where(g2, Thtot + hweight * Tv, Thtot)
                        Shtot = np.where(g2, Shtot + hweight * Sv, Shtot)
                I_hwtot = np.where(hwtot > 0.0, 1.0 / hwtot, 0.0)
                nw = hwtot <= 0.0
                counts["no_weight"] += int((nw & do_i).sum())
                if P.linear_drag:
                    ustar = np.full(do_i.shape, cdrag_sqrt_H * P.drag_bg_vel)
                else:
                    ustar = np.where(nw, cdrag_sqrt_H * P.drag_bg_vel, cdrag_sqrt_H * hutot / hwtot)
                umag_avg = hutot * I_hwtot
                h_bbl_drag = hwtot
                dz_bbl_drag = dzwtot
                if use_EOS:
                    T_EOS = np.where(hwtot > 0.0, Thtot / hwtot, 0.0)
                    S_EOS = np.where(hwtot > 0.0, Shtot / hwtot, 0.0)
            else:
                ustar = np.full(do_i.shape, cdrag_sqrt_H * P.drag_bg_vel)

            # pressure at the bottom, k = 1..nz (:701-711)
            if use_EOS:
                press = 0.5 * (F(p_surf) + F(p_surf, oj, oi)) if p_surf is not None else z.copy()
                for k in range(nz):
                    press = press + HRg * (0.5 * (F(h[k]) + F(h[k], oj, oi)))
                dR_dT, dR_dS = z.copy(), z.copy()
                for jj, ii in zip(*np.nonzero(do_i)):
                    dR_dT[jj, ii], dR_dS[jj, ii] = orc.eos_density_derivs(eos, float(T_EOS[jj, ii]), float(S_EOS[jj, ii]),
                                                                          float(press[jj, ii]))

            # the stratification-limited thickness (:720-840)
            ustarsq = Rho0x400_G * (ustar * ustar)
            htot, dztot = z.copy(), z.copy()
            act = do_i.copy()
            if use_EOS:
                Thtot, Shtot, oldfn = z.copy(), z.copy(), z.copy()
                for k in range(nz - 1, 0, -1):
                    h_at, dz_at = at_vel(k)
                    run = act & ~(h_at <= 0.0)                  # cycle
                    Tk, Sk = TS_vel(k)
                    oldfn = np.where(run, dR_dT * (Thtot - Tk * htot) + dR_dS * (Shtot - Sk * htot), oldfn)
                    ex = run & (oldfn >= ustarsq)               # exit
                    act &= ~ex; run &= ~ex
                    Tm, Sm = TS_vel(k - 1)
                    Dfn = (dR_dT * (Tk - Tm) + dR_dS * (Sk - Sm)) * (h_at + htot)
                    whole = (oldfn + Dfn) <= ustarsq
                    frac_used = np.sqrt((ustarsq - oldfn) / (Dfn))
                    counts["frac_used"] += int((run & ~whole).sum())
                    Dh = np.where(whole, h_at, h_at * frac_used)
                    Ddz = np.where(whole, dz_at, dz_at * frac_used)
                    htot = np.where(run, htot + Dh, htot)
                    dztot = np.where(run, dztot + Ddz, dztot)
                    Thtot = np.where(run, Thtot + Tk * Dh, Thtot)
                    Shtot = np.where(run, Shtot + Sk * Dh, Shtot)
                h_at, dz_at = at_vel(0)
                T1, S1 = TS_vel(0)
                l1 = do_i & (oldfn < ustarsq) & (h_at > 0.0)
                l1 &= dR_dT * (Thtot - T1 * htot) + dR_dS * (Shtot - S1 * htot) < ustarsq
                counts["layer1_eos"] += int(l1.sum())
                htot = np.where(l1, htot + h_at, htot)
                dztot = np.where(l1, dztot + dz_at, dztot)
            else:                                               # GV%Rlay, nkml = 0 so K2 = 2 (:350)
                Rhtot = z.copy()
                for k in range(nz - 1, 0, -1):
                    h_at, dz_at = at_vel(k)
                    oldfn = Rhtot - Rlay[k] * htot
                    Dfn = (Rlay[k] - Rlay[k - 1]) * (h_at + htot)
                    run = do_i & ~(oldfn >= ustarsq)            # cycle
                    whole = (oldfn + Dfn) <= ustarsq
                    frac_used = np.sqrt((ustarsq - oldfn) / (Dfn))
                    counts["frac_used"] += int((run & ~whole).sum())
                    Dh = np.where(whole, h_at, h_at * frac_used)
                    Ddz = np.where(whole, dz_at, dz_at * frac_used)
                    htot = np.where(run, htot + Dh, htot)
                    dztot = np.where(run, dztot + Ddz, dztot)
                    Rhtot = np.where(run, Rhtot + Rlay[k] * Dh, Rhtot)
                h_at, dz_at = at_vel(0)
                l1 = do_i & (Rhtot - Rlay[0] * htot < ustarsq)
                counts["layer1_rlay"] += int(l1.sum())
                htot = np.where(l1, htot + h_at, htot)
                dztot = np.where(l1, dztot + dz_at, dztot)

            # Killworth and Edwards (1999) eq. 2.20 (:842-876)
            C2f = (F(Mq, 0, -1) + F(Mq)) if dir else (F(Mq, -1, 0) + F(Mq))
            ustH = ustar
            root = np.sqrt(0.25 * (ustH * ustH) + (htot * C2f) * (htot * C2f))
            floor1 = dztot * ustH <= (P.BBL_thick_min + dz_neglect) * (0.5 * ustH + root)
            t1 = np.where(floor1, P.BBL_thick_min, (dztot * ustH) / (0.5 * ustH + root))
            t2 = dztot / (0.5 + np.sqrt(0.25 + htot * htot * C2f * C2f / (ustar * ustar)))
            floor2 = t2 < P.BBL_thick_min
            t2 = np.where(floor2, P.BBL_thick_min, t2)
            form1 = P.cdrag * u2_bg <= 0.0
            bbl_thick = np.where(form1, t1, t2)
            counts["thick_min"] += int((do_i & np.where(form1, floor1, floor2)).sum())
            if P.RiNo_mix:
                cap = bbl_thick > 0.5 * P.dz_bbl
                counts["RiNo_cap"] += int((do_i & cap).sum())
                bbl_thick = np.where(cap, 0.5 * P.dz_bbl, bbl_thick)
            if P.body_force_drag:
                bbl_thick = dz_bbl_drag

            # viscosity (:1019-1047)
            if P.correct_BBL_bounds:
                cb = cdrag_sqrt * ustar * bbl_thick <= P.Kv_BBL_min
                counts["correct_bounds"] += int((do_i & cb).sum())
                big = (cdrag_sqrt * ustar) * BBL_thick_max > P.Kv_BBL_min
                bbl_thick = np.where(cb, np.where(big, P.Kv_BBL_min / (cdrag_sqrt * ustar), BBL_thick_max), bbl_thick)
                kv_bbl = np.where(cb, P.Kv_BBL_min, (cdrag_sqrt * ustar) * bbl_thick)
            else:
                kv_bbl = (cdrag_sqrt * ustar) * bbl_thick

            # DRAG_AS_BODY_FORCE (:1049-1070)
            if P.body_force_drag:
                Ray = Ray_u if dir == 0 else Ray_v
                bf = do_i & (h_bbl_drag > 0.0)
                counts["body_force"] += int(bf.sum())
                h_sum = z.copy()
                I_hw = np.where(bf, 1.0 / h_bbl_drag, 0.0)
                act = bf.copy()
                for k in range(nz - 1, -1, -1):
                    h_at, _ = at_vel(k)
                    h_bbl_fr = _min(h_bbl_drag - h_sum, h_at) * I_hw
                    Rk = F(Ray[k])
                    Rk[act] = (Rk + (cdrag_L_to_H * umag_avg) * h_bbl_fr)[act]
                    h_sum = np.where(act, h_sum + h_at, h_sum)
                    act &= ~(h_sum >= h_bbl_drag)
                kv_bbl = np.where(bf, P.Kv_BBL_min, kv_bbl)
            kv_bbl = np.where(P.Kv_BBL_min > kv_bbl, P.Kv_BBL_min, kv_bbl)

            bt, kv = (bbl_thick_u, Kv_bbl_u) if dir == 0 else (bbl_thick_v, Kv_bbl_v)
            F(bt)[do_i] = bbl_thick[do_i]
            if kv is not None:
                F(kv)[do_i] = kv_bbl[do_i]
    return counts


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_set_visc_cpu.py and tests/test_set_visc_gpu.py

def inputs(d, M, GV, seed=5, strat=1.0, vanish=True, u_max=0.3):
    """u, v, h, T, S (a stratification scaled by `strat`), p_surf and tideamp on a tile; with `vanish` the two bottom layers of a
    band of rows are Angstrom thin (vanished layers in the near-bottom walk).  The band is laid in global coordinates, like every
    other field here, so that a tile of any layout sees its part of the one-tile state."""
    from mom6_amd import synth
    h, u, v = synth.make_state(d, M, seed=20250808 + seed, u_max=u_max, h_pert=0.01)
    T = np.zeros_like(h); S = np.zeros_like(h)
    for k in range(d.nk):
        T[k] = 10.0 + strat * (10.0 - 15.0 * k / max(d.nk - 1, 1) + 0.8 * synth.smooth_field(d, seed + k, ox=0.5, oy=0.5))
        S[k] = 34.5 + strat * (1.0 * k / max(d.nk - 1, 1) - 0.5 + 0.2 * synth.smooth_field(d, seed + 100 + k, ox=0.5, oy=0.5))
    if vanish and d.nk > 2:
        ig = np.arange(d.pitch) - d.ioff + d.i_glob0
        jg = np.arange(d.shape2()[0]) - d.joff + d.j_glob0
        band = ((jg >= d.nj_glob // 3) & (jg <= d.nj_glob // 2))[:, None] & ((ig >= -1) & (ig <= d.ni_glob))[None, :]
        for k in (d.nk - 2, d.nk - 1):
            h[k] = np.where(band, GV.Angstrom_H, h[k])
    p_surf = 1.0e4 * (1.0 + 0.2 * synth.smooth_field(d, seed + 300, ox=0.5, oy=0.5))
    tideamp = 0.03 * (1.0 + 0.5 * synth.smooth_field(d, seed + 301, ox=0.5, oy=0.5))
    return dict(u=u, v=v, h=h, T=np.ascontiguousarray(T), S=np.ascontiguousarray(S), p_surf=np.ascontiguousarray(p_surf),
                tideamp=np.ascontiguousarray(tideamp))


# switch set -> (set_visc_params members, EOS form or None, given p_surf, given Ray_u/v, input options)
SWITCHES = {
    "eos": (dict(drag_bg_vel=0.05), "form", False, False, {}),
    "rlay": (dict(drag_bg_vel=0.3), None, False, False, {}),
    "linear": (dict(linear_drag=1, drag_bg_vel=0.1), None, False, False, {}),
    "bounds": (dict(correct_BBL_bounds=1, Kv_BBL_min=1.0e-2, drag_bg_vel=0.02), abi.WRIGHT, False, False, {}),
    "tidal": (dict(BBL_use_tidal_bg=1, drag_bg_vel=1.0e30), abi.WRIGHT, False, False, {}),
    "body": (dict(body_force_drag=1, drag_bg_vel=0.05), abi.WRIGHT, False, True, {}),
    "rino": (dict(RiNo_mix=1, drag_bg_vel=5.0), None, False, False, {}),
    "psurf": (dict(drag_bg_vel=0.05), abi.WRIGHT, True, False, {}),
    "bg0": (dict(drag_bg_vel=0.0, BBL_thick_min=8.0), abi.WRIGHT, False, False, {}),
    "weak": (dict(drag_bg_vel=0.1), abi.WRIGHT, False, False, dict(strat=1.0e-4)),
}


def switch_case(name, form=None, Kv=1.0e-4, HBBL=10.0):
    mods, eos_form, give_ps, give_ray, opts = SWITCHES[name]
    P = abi.set_visc_params_default(HBBL=HBBL, Kv=Kv)
    for k, val in mods.items():
        setattr(P, k, val)
    if eos_form == "form":
        eos_form = form
    eos = abi.eos_params_default(eos_form) if eos_form is not None else None
    return P, eos, give_ps, give_ray, opts


def run(d, M, GV, P, inp, eos=None, Rlay=None, give_ps=False, give_ray=False, fill=np.nan, orc=None):
    """The restatement on numpy inputs; outputs start as `fill`.  Returns (outputs, counts)."""
    out = dict(Kv_bbl_u=np.full(d.shape2(), fill), Kv_bbl_v=np.full(d.shape2(), fill), bbl_thick_u=np.full(d.shape2(), fill),
               bbl_thick_v=np.full(d.shape2(), fill))
    if give_ray:
        out["Ray_u"] = np.full(d.shape3(), fill); out["Ray_v"] = np.full(d.shape3(), fill)
    counts = set_viscous_BBL(d, M, GV, P, inp["u"], inp["v"], inp["h"], T=inp["T"], S=inp["S"],
                             p_surf=inp["p_surf"] if give_ps else None, eos=eos, tideamp=inp["tideamp"], Rlay=Rlay, orc=orc, **out)
    return out, counts
