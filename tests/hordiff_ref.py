"""The checker of mom6x_tracer_hordiff: a numpy restatement of tracer_hordiff (src/tracer/MOM_tracer_hor_diff.F90:119-699) on its
along-layer path (:541-612) -- the face diffusivities and khdt_x, khdt_y (:237-357, all three branches), the iteration count
(:371-390), the zeroing and accumulation of df_x, df_y (:392-402, :581-588), the iteration (:544-612) with conc_underflow --
written from the Fortran operation for operation and vectorised over the faces of one direction and over the layers (which do not
interact).  Arrays are in the pitched tile layout of include/mom6x.h ([k, j + joff, i + ioff]).  MAX and MIN return their first
argument on a tie.  `counts` records how often each branch fired.

The Fortran module cannot be built stand-alone (it needs the tracer registry, VarMix, MEKE and the domain types), so
tests/test_tracer_hor_diff_cpu.py first holds this module to facts that do not come from it."""
import math

import numpy as np

from mom6_amd import abi
from tests.ref_common import _faces, _max, _min

G = abi.G
EPSILON = 2.0 ** -52
BRANCHES = ("itts_1", "itts_ge3_check", "itts_from_max", "clamp_x_on", "clamp_x_off", "clamp_y_on", "clamp_y_off", "kh_max", "kh_min",
            "pass_floor", "pass_slope", "meke_nonzero", "eady_nonzero", "closed_face_wet", "vanished_next_thick", "underflow_flushed",
            "underflow_kept")
PLANES = ("L2u", "SN_u", "L2v", "SN_v", "Res_fn_h", "Rd_dx_h", "MEKE_Kh")


def group_pass(d, a):
    """The group pass of an h-point field on ONE tile (full halo): the wrap of a re-entrant direction, x first, then y over the
    wrapped columns (which fills the corners); nothing on a closed boundary."""
    w, ni, nj, io, jo = d.halo, d.ni, d.nj, d.ioff, d.joff
    if d.reentrant_x:
        a[..., jo:jo + nj, io - w:io] = a[..., jo:jo + nj, io + ni - w:io + ni]
        a[..., jo:jo + nj, io + ni:io + ni + w] = a[..., jo:jo + nj, io:io + w]
    if d.reentrant_y:
        c0, c1 = (io - w, io + ni + w) if d.reentrant_x else (io, io + ni)
        a[..., jo - w:jo, c0:c1] = a[..., jo + nj - w:jo + nj, c0:c1]
        a[..., jo + nj:jo + nj + w, c0:c1] = a[..., jo:jo + w, c0:c1]


def num_itts_of(max_CFL):
    """:382 / :386"""
    return max(1, int(math.ceil(max_CFL - 4.0 * EPSILON)))


def refused(P, planes):
    """The field a switched-on term lacks (what the call names in its error), or None."""
    vm = bool(P.use_variable_mixing)
    need = []
    if vm and P.KhTr_Slope_Cff > 0.0:
        need += ["L2u", "SN_u", "L2v", "SN_v"]
    if vm and P.use_MEKE_Kh:
        need += ["MEKE_Kh"]
    if P.Resoln_scaled_KhTr:
        need += ["Res_fn_h"]
    if vm and P.KhTr_passivity_coeff > 0.0:
        need += ["Rd_dx_h"]
    for n in need:
        if planes.get(n) is None:
            return n
    return None


def khdt_faces(d, M, P, dt, planes, counts=None):
    """khdt_x on the u faces and khdt_y on the v faces (:237-357) as arrays over the face ranges of _faces."""
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    out = []
    use_VarMix = bool(P.use_variable_mixing)
    Resoln_scaled = bool(P.Resoln_scaled_KhTr)
    use_Eady = use_VarMix and P.KhTr_Slope_Cff > 0.0
    for dir in (0, 1):
        (r0, r1), (c0, c1), (oj, oi) = _faces(d, dir)

        def F(a, right=False):
            dj, di = (oj, oi) if right else (0, 0)
            return a[..., r0 + dj:r1 + dj, c0 + di:c1 + di]

        ln = F(M[G["dx_Cv" if dir else "dy_Cu"]]) * F(M[G["IdyCv" if dir else "IdxCu"]])
        if use_VarMix:                                                           # :238-281
            Kh_loc = np.full(ln.shape, P.KhTr)
            if use_Eady:
                e = P.KhTr_Slope_Cff * F(planes["L2v" if dir else "L2u"]) * F(planes["SN_v" if dir else "SN_u"])
                counts["eady_nonzero"] += int((e != 0.0).sum())
                Kh_loc = Kh_loc + e
            if P.use_MEKE_Kh:
                m = P.MEKE_KhTr_fac * np.sqrt(F(planes["MEKE_Kh"]) * F(planes["MEKE_Kh"], True))
                counts["meke_nonzero"] += int((m != 0.0).sum())
                Kh_loc = Kh_loc + m
            if P.KhTr_max > 0.0:
                counts["kh_max"] += int((P.KhTr_max < Kh_loc).sum())
                Kh_loc = _min(Kh_loc, P.KhTr_max)
            if Resoln_scaled:
                Kh_loc = Kh_loc * 0.5 * (F(planes["Res_fn_h"]) + F(planes["Res_fn_h"], True))
            counts["kh_min"] += int((P.KhTr_min > Kh_loc).sum())
            Kh = _max(Kh_loc, P.KhTr_min)
            if P.KhTr_passivity_coeff > 0.0:
                Rd_dx = 0.5 * (F(planes["Rd_dx_h"]) + F(planes["Rd_dx_h"], True))
                sl = P.KhTr_passivity_coeff * Rd_dx
                counts["pass_slope"] += int((sl > P.KhTr_passivity_min).sum())
                counts["pass_floor"] += int((~(sl > P.KhTr_passivity_min)).sum())
                Kh_loc = Kh * _max(P.KhTr_passivity_min, sl)
                if P.KhTr_max > 0.0:
                    counts["kh_max"] += int((P.KhTr_max < Kh_loc).sum())
                    Kh_loc = _min(Kh_loc, P.KhTr_max)
                counts["kh_min"] += int((P.KhTr_min > Kh_loc).sum())
                Kh = _max(Kh_loc, P.KhTr_min)
            kh = dt * (Kh * ln)
        elif Resoln_scaled:                                                      # :282-294
            Res_fn = 0.5 * (F(planes["Res_fn_h"]) + F(planes["Res_fn_h"], True))
            kh = dt * (P.KhTr * ln) * Res_fn
        else:
            kh = dt * (P.KhTr * ln)                                              # :305, :317
        if P.max_diff_CFL > 0.0:                                                 # :322-357
            aT = M[G["areaT"]]
            khdt_max = 0.125 * P.max_diff_CFL * _min(F(aT), F(aT, True))
            on = kh > khdt_max
            counts["clamp_y_on" if dir else "clamp_x_on"] += int(on.sum())
            counts["clamp_y_off" if dir else "clamp_x_off"] += int((~on).sum())
            kh = _min(kh, khdt_max)
        out.append(np.ascontiguousarray(kh))
    return out


def cell_cfl(d, M, khx, khy):
    """CFL(i,j) on the computational domain (:375-376) from the face arrays of khdt_faces."""
    IaT = M[G["IareaT"]][d.sl(0, d.ni - 1, 0, d.nj - 1)]
    return 2.0 * ((khx[:, :-1] + khx[:, 1:]) + (khy[:-1, :] + khy[1:, :])) * IaT


def tracer_hordiff(d, M, GV, P, h, dt, tracers, planes=None, conc_underflow=None, df_x=None, df_y=None, khdt_x=None, khdt_y=None,
                   CFL=None, counts=None, max_across=None, pass_fn=None, record=None):
    """Updates the tracers (and df_x, df_y, khdt_x, khdt_y, CFL where given) in place, as mom6x_tracer_hordiff does; returns
    num_itts (0 after the early return of :199).  max_across: max_across_PEs; pass_fn: the group pass of one field (default: the
    one-tile wrap).  `record`, a dict, receives max_CFL."""
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    planes = planes or {}
    ntr = len(tracers)
    if ntr == 0 or (P.KhTr <= 0.0 and not P.use_variable_mixing):               # :199
        return 0
    assert all(getattr(P, n) == 0 for n in abi.TRACER_HOR_DIFF_MUST_BE_0) and refused(P, planes) is None
    if pass_fn is None:
        pass_fn = lambda a: group_pass(d, a)                                     # noqa: E731
    Idt = 1.0 / dt
    h_neglect = GV.H_subroundoff
    io, jo, ni, nj = d.ioff, d.joff, d.ni, d.nj
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        khx, khy = khdt_faces(d, M, P, dt, planes, counts)
        if khdt_x is not None:
            khdt_x[jo:jo + nj, io - 1:io + ni] = khx
        if khdt_y is not None:
            khdt_y[jo - 1:jo + nj, io:io + ni] = khy
        if P.check_diffusive_CFL:                                                # :371-384
            cfl = cell_cfl(d, M, khx, khy)
            max_CFL = 0.0
            big = cfl[cfl > 0.0]
            if big.size:
                max_CFL = float(big.max())
            if max_across is not None:
                max_CFL = max_across(max_CFL)
            if record is not None:
                record["max_CFL"] = max_CFL
            num_itts = num_itts_of(max_CFL)
            counts["itts_ge3_check"] += int(num_itts >= 3)
            if CFL is not None:
                CFL[jo:jo + nj, io:io + ni] = cfl
        elif P.max_diff_CFL > 0.0:
            num_itts = num_itts_of(P.max_diff_CFL)
            counts["itts_from_max"] += 1
        else:
            num_itts = 1
        counts["itts_1"] += int(num_itts == 1)
        I_numitts = 1.0 / float(num_itts)
        for f, dir in ((df_x, 0), (df_y, 1)):                                    # :392-402
            (r0, r1), (c0, c1), _ = _faces(d, dir)
            for a in (f or []):
                if a is not None:
                    a[:, r0:r1, c0:c1] = 0.0

        wet = M[G["mask2dT"]] > 0.0
        counts["closed_face_wet"] += int(((M[G["dy_Cu"]][jo:jo + nj, io - 1:io + ni] == 0.0) &
                                          (wet[jo:jo + nj, io - 1:io + ni] | wet[jo:jo + nj, io:io + ni + 1])).sum())
        hxl, hxr = h[:, jo:jo + nj, io - 1:io + ni], h[:, jo:jo + nj, io:io + ni + 1]
        hyl, hyr = h[:, jo - 1:jo + nj, io:io + ni], h[:, jo:jo + nj + 1, io:io + ni]
        hC = h[:, jo:jo + nj, io:io + ni]
        thin, thick = 2.0 * GV.Angstrom_H, 1.0e6 * GV.Angstrom_H
        for a, b in ((hxl, hxr), (hyl, hyr)):
            counts["vanished_next_thick"] += int((((a <= thin) & (b > thick)) | ((b <= thin) & (a > thick))).sum())
        scale = I_numitts
        for itt in range(num_itts):
            for T in tracers:                                                    # do_group_pass :545
                pass_fn(T)
            Coef_x = ((scale * khx) * 2.0 * (hxl * hxr)) / (hxl + hxr + h_neglect)    # :564
            Coef_y = ((scale * khy) * 2.0 * (hyl * hyr)) / (hyl + hyr + h_neglect)    # :558
            Ihdxdy = M[G["IareaT"]][jo:jo + nj, io:io + ni] / (hC + h_neglect)        # :569
            for m, T in enumerate(tracers):
                fx = Coef_x * (T[:, jo:jo + nj, io - 1:io + ni] - T[:, jo:jo + nj, io:io + ni + 1])
                fy = Coef_y * (T[:, jo - 1:jo + nj, io:io + ni] - T[:, jo:jo + nj + 1, io:io + ni])
                dTr = Ihdxdy * ((fx[:, :, :-1] - fx[:, :, 1:]) + (fy[:, :-1, :] - fy[:, 1:, :]))   # :575-579
                if df_x is not None and df_x[m] is not None:                     # :581-584
                    df_x[m][:, jo:jo + nj, io - 1:io + ni] = df_x[m][:, jo:jo + nj, io - 1:io + ni] + fx * Idt
                if df_y is not None and df_y[m] is not None:                     # :585-588
                    df_y[m][:, jo - 1:jo + nj, io:io + ni] = df_y[m][:, jo - 1:jo + nj, io:io + ni] + fy * Idt
                T[:, jo:jo + nj, io:io + ni] = T[:, jo:jo + nj, io:io + ni] + dTr      # :598
            for m, T in enumerate(tracers):                                      # :605-610
                uf = conc_underflow[m] if conc_underflow is not None else 0.0
                if uf > 0.0:
                    c = T[:, jo:jo + nj, io:io + ni]
                    fl = np.abs(c) < uf
                    counts["underflow_flushed"] += int((fl & (c != 0.0)).sum())
                    counts["underflow_kept"] += int((~fl).sum())
                    c[fl] = 0.0
    return num_itts


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_tracer_hor_diff_cpu.py and tests/test_tracer_hor_diff_gpu.py

def inputs(d, M, GV, ntr=2, seed=5):
    """h, T, S of tests/setvisc_ref.inputs (Angstrom on land) with the two bottom layers Angstrom thin in a band of rows -- global
    rows, so that a tile of any layout sees its part of the one-tile state --, dyes that span twelve decades, and the 2-D planes of
    VarMix and MEKE."""
    from mom6_amd import synth
    from tests import setvisc_ref
    b = setvisc_ref.inputs(d, M, GV, seed=seed, vanish=False)
    if d.nk > 2:
        jg = np.arange(d.nrows) - d.joff + d.j_glob0
        band = ((jg >= d.nj_glob // 3) & (jg <= d.nj_glob // 2))[:, None]
        for k in (d.nk - 2, d.nk - 1):
            b["h"][k] = np.where(band, GV.Angstrom_H, b["h"][k])
    tr = [b["T"], b["S"]][:ntr]
    for m in range(2, ntr):
        tr.append(np.ascontiguousarray(10.0 ** (-6.0 * (1.0 + synth.smooth_field(d, seed + 500 + m, nk=d.nk, ox=0.5, oy=0.5)))))

    def sm(n, ox, oy):
        return synth.smooth_field(d, seed + 600 + n, ox=ox, oy=oy)
    planes = dict(L2u=1.0e9 * (1.0 + 0.5 * sm(0, 1.0, 0.5)), SN_u=1.0e-6 * (1.0 + sm(1, 1.0, 0.5)) ** 2,
                  L2v=1.0e9 * (1.0 + 0.5 * sm(2, 0.5, 1.0)), SN_v=1.0e-6 * (1.0 + sm(3, 0.5, 1.0)) ** 2,
                  Res_fn_h=np.clip(0.6 + 0.4 * sm(4, 0.5, 0.5), 0.0, 1.0), Rd_dx_h=0.25 * (1.0 + 0.9 * np.clip(sm(5, 0.5, 0.5), -1.0, 1.0)),
                  MEKE_Kh=2000.0 * (1.0 + 0.9 * np.clip(sm(6, 0.5, 0.5), -1.0, 1.0)))
    return dict(h=b["h"], tracers=tr, planes={n: np.ascontiguousarray(a) for n, a in planes.items()})


VARMIX = dict(use_variable_mixing=1, KhTr=500.0, KhTr_Slope_Cff=1.0, use_MEKE_Kh=1, MEKE_KhTr_fac=1.0, KhTr_max=4000.0, KhTr_min=1500.0,
              Resoln_scaled_KhTr=1, KhTr_passivity_coeff=3.0, KhTr_passivity_min=0.5)
# case -> (params members, dt, what is chosen from the grid, the tracers' conc_underflow or None, df_x / df_y given, khdt_x / khdt_y / CFL given)
#   cfl=c:      KHTR such that the largest cell CFL is c (KHTR enters khdt linearly without variable mixing)
#   clamp_x=c:  KHTR such that khdt_x reaches its limit 0.125*c*min(areaT) at the median u face, with MAX_TR_DIFFUSION_CFL = c
#   clamp="mid": MAX_TR_DIFFUSION_CFL between the medians over the open u and the open v faces of khdt / (0.125*min(areaT))
#   cfl_dt=c:   dt such that the largest cell CFL is c (dt enters khdt linearly)
CASES = {
    "const": (dict(KhTr=1000.0), 3600.0, {}, None, False, False),
    "const_df": (dict(KhTr=1000.0), 3600.0, {}, None, True, True),
    "check3": (dict(check_diffusive_CFL=1), 3600.0, dict(cfl=3.0), None, True, True),
    "check1": (dict(KhTr=1000.0, check_diffusive_CFL=1), 3600.0, {}, None, False, True),
    "maxcfl": (dict(max_diff_CFL=2.5), 3600.0, dict(clamp_x=2.5), None, True, True),
    "varmix": (VARMIX, 86400.0, dict(clamp="mid"), None, False, True),
    "varmix_check": (dict(VARMIX, check_diffusive_CFL=1), 86400.0, dict(cfl_dt=3.5), None, True, True),
    "resoln": (dict(KhTr=2000.0, Resoln_scaled_KhTr=1, KhTr_min=1.0e9), 3600.0, {}, None, False, True),
    "underflow": (dict(KhTr=1000.0), 3600.0, {}, 1.0e-6, False, False),
}


def case(name, d, M, planes):
    """The parameters of a case on the grid (d, M) -- a tile of a layout takes the ones of the whole grid -- and its other settings."""
    mods, dt, pick, uf, give_df, give_out = CASES[name]
    P = abi.tracer_hor_diff_params_default()
    for k, val in mods.items():
        setattr(P, k, val)

    def unlimited(P1, dt1):
        Q = abi.TracerHorDiffParams.from_buffer_copy(P1)
        Q.max_diff_CFL = -1.0
        return khdt_faces(d, M, Q, dt1, planes)
    aT = M[G["areaT"]]
    io, jo, ni, nj = d.ioff, d.joff, d.ni, d.nj
    lim_x = 0.125 * np.minimum(aT[jo:jo + nj, io - 1:io + ni], aT[jo:jo + nj, io:io + ni + 1])
    lim_y = 0.125 * np.minimum(aT[jo - 1:jo + nj, io:io + ni], aT[jo:jo + nj + 1, io:io + ni])
    if "cfl" in pick:
        P.KhTr = 1.0
        P.KhTr = pick["cfl"] / float(cell_cfl(d, M, *unlimited(P, dt)).max())
    if "clamp_x" in pick:
        P.KhTr = 1.0
        r = unlimited(P, dt)[0] / lim_x
        P.KhTr = pick["clamp_x"] * 1.0 / float(np.median(r[r > 0.0]))
    if "clamp" in pick:
        khx, khy = unlimited(P, dt)
        rx, ry = khx / lim_x, khy / lim_y
        P.max_diff_CFL = float(np.sqrt(np.median(rx[rx > 0.0]) * np.median(ry[ry > 0.0])))
    if "cfl_dt" in pick:
        dt = dt * pick["cfl_dt"] / float(cell_cfl(d, M, *unlimited(P, dt)).max())
    return P, dt, uf, give_df, give_out


def df_given(m, dir):
    """Which tracers of a case with flux diagnostics have df_x (dir 0) / df_y (1): entries of the lists may be absent."""
    return (m % 2 == 0) if dir == 0 else (m % 3 != 2)


def run(d, M, GV, P, inp, dt, uf=None, give_df=False, give_out=False, fill=np.nan, counts=None, **kw):
    """The restatement on copies of the inputs; df_x, df_y, khdt_x, khdt_y and CFL start as `fill`.  Returns (outputs, num_itts,
    counts); outputs: tracers, df_x, df_y (lists) and khdt_x, khdt_y, CFL."""
    ntr = len(inp["tracers"])
    out = dict(tracers=[t.copy() for t in inp["tracers"]], df_x=None, df_y=None, khdt_x=None, khdt_y=None, CFL=None)
    if give_df:
        out["df_x"] = [np.full(d.shape3(), fill) if df_given(m, 0) else None for m in range(ntr)]
        out["df_y"] = [np.full(d.shape3(), fill) if df_given(m, 1) else None for m in range(ntr)]
    if give_out:
        out.update(khdt_x=np.full(d.shape2(), fill), khdt_y=np.full(d.shape2(), fill), CFL=np.full(d.shape2(), fill))
    if counts is None:
        counts = dict.fromkeys(BRANCHES, 0)
    n = tracer_hordiff(d, M, GV, P, inp["h"], dt, out["tracers"], planes=inp["planes"], conc_underflow=[uf] * ntr if uf else None,
                       df_x=out["df_x"], df_y=out["df_y"], khdt_x=out["khdt_x"], khdt_y=out["khdt_y"], CFL=out["CFL"], counts=counts, **kw)
    return out, n, counts
