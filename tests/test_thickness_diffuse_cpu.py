"""thickness_diffuse's restatement (tests/thickdiff_ref.py) held to facts that do not come from it: closed forms, the exact zero
column sum of the fluxes, the bounds of the limiters, conservation, the quarter turn, unit scaling, a tile cut and the branches
its case list reaches; and the exports and ABI size of the device routine.  The device is held to the restatement in
tests/test_thickness_diffuse_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import thickdiff_ref as R
from tests.test_oracle_invariants_cpu import Turn

G = abi.G
GRIDS = {"benchmark_small": lambda nk: H.benchmark_small(nk=nk)[1:],
         "island_basin": lambda nk: H.island_basin(nk=nk)[1:],
         "partial_faces": lambda nk: (lambda d, M: (d, H.partial_faces(d, M)))(*H.benchmark_small(nk=nk)[1:])}


def _bits(a, b, name, signed_zero_ok=False):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    ne = a.view(np.int64) != b.view(np.int64)
    if signed_zero_ok:
        ne &= ~((a == 0.0) & (b == 0.0))
    n = int(ne.sum())
    assert n == 0, f"{name}: {n} of {a.size} words differ"


def test_exports_and_struct_size():
    lib = abi.load_library()
    assert hasattr(lib, "mom6x_thickness_diffuse_init") and hasattr(lib, "mom6x_thickness_diffuse")
    assert lib.mom6x_struct_size(19) == C.sizeof(abi.ThicknessDiffuseParams)


def _flat(nk):
    """benchmark_small with a flat bottom at 4000 m and open water everywhere it was open."""
    d, M = H.benchmark_small(nk=nk)[1:]
    M = M.copy()
    M[G["bathyT"]] = 4000.0
    return d, M


def test_level_interfaces_give_no_flux():
    d, M = _flat(6)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    inp["h"] = np.full(d.shape3(), 4000.0 / d.nk)
    P = abi.thickness_diffuse_params_default()
    diag = {}
    out, _ = R.run(d, M, GV, P, inp, 900.0, diag=diag)
    assert (diag["uhD"] == 0.0).all() and (diag["vhD"] == 0.0).all()
    for n in ("h", "uhtr", "vhtr"):
        _bits(out[n], inp[n], n)


def test_two_layers_one_tilted_interface_closed_form():
    """No EOS, no limiter: uhD(I,j,2) = Z_to_H*(-(KH*dy_Cu)*(((e(i+1,2)-e(i,2))*IdxCu)*mask2dCu)) (:1089-1092, :1151-1160) with
    KH = min(KH_u_CFL, max(KHTH_MIN, KHTH)), uhD(I,j,1) its negative (:1534); the same at the v faces."""
    d, M = _flat(2)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    ii = (np.arange(d.pitch) - d.ioff)[None, :] * np.ones(d.shape2())
    jj = (np.arange(d.shape2()[0]) - d.joff)[:, None] * np.ones(d.shape2())
    h = np.empty(d.shape3())
    h[1] = 2000.0 + 0.5 * ii + 0.25 * jj
    h[0] = 4000.0 - h[1]
    inp["h"] = h
    dt = 900.0
    P = abi.thickness_diffuse_params_default(KHTH=100.0)
    P.Khth_Min = 20.0
    diag = {}
    R.run(d, M, GV, P, inp, dt, diag=diag)
    e2 = -(M[G["bathyT"]] + 0.0) + h[1] * GV.H_to_Z
    for s, far, Idx, Idy, Ig, ln, mk in (("u", (0, 1), "IdxCu", "IdyCu", "IdxCu", "dy_Cu", "mask2dCu"),
                                         ("v", (1, 0), "IdxCv", "IdyCv", "IdyCv", "dx_Cv", "mask2dCv")):
        sl = H.interior(d, s)
        sr = (slice(sl[0].start + far[0], sl[0].stop + far[0]), slice(sl[1].start + far[1], sl[1].stop + far[1]))
        KH_CFL = (0.25 * P.max_Khth_CFL) / (dt * ((M[G[Idx]][sl] * M[G[Idx]][sl]) + (M[G[Idy]][sl] * M[G[Idy]][sl])))
        KH = np.minimum(KH_CFL, max(P.Khth_Min, P.Khth))
        want = GV.Z_to_H * (-(KH * M[G[ln]][sl]) * (((e2[sr] - e2[sl]) * M[G[Ig]][sl]) * M[G[mk]][sl]))
        got = diag[s + "hD"]
        assert (KH == 100.0).all() and (want != 0.0).sum() > 100
        _bits(got[1][sl], want, s + "hD(2)", signed_zero_ok=True)
        _bits(got[0][sl], -got[1][sl], s + "hD(1)", signed_zero_ok=True)   # (a closed face: uhtot = 0.0 + -0.0 = +0.0)


def _case_run(d, M, GV, name, form=abi.WRIGHT, orc=None, diag=None, inp=None):
    P, eos, ps, stored, gm, dt, opts = R.case(name, form=form)
    if inp is None:
        inp = R.inputs(d, M, GV, **opts)
    out, counts = R.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored, give_gm=gm, orc=orc, diag=diag)
    return inp, out, counts, dt


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("nk", [8, 75])
@pytest.mark.parametrize("name", ["eos", "noeos"])
def test_exact_properties(grid, nk, name, orc):
    d, M = GRIDS[grid](nk)
    GV = abi.vgrid_default()
    diag = {}
    inp, out, counts, dt = _case_run(d, M, GV, name, orc=orc, diag=diag)
    ha = diag["h_avail"]
    for s, far, ln in (("u", (0, 1), "dy_Cu"), ("v", (1, 0), "dx_Cv")):
        sl = H.interior(d, s)
        sr = (slice(sl[0].start + far[0], sl[0].stop + far[0]), slice(sl[1].start + far[1], sl[1].stop + far[1]))
        D = diag[s + "hD"][(slice(None),) + sl]
        assert np.isfinite(D).all()
        tot = np.zeros(D.shape[1:])
        for k in range(nk - 1, 0, -1):          # k = nz..2 in that order, then layer 1: exactly zero
            tot = tot + D[k]
        assert ((tot + D[0]) == 0.0).all()
        hL, hR = ha[(slice(None),) + sl], ha[(slice(None),) + sr]
        assert (D[1:] <= hL[1:]).all() and (D[1:] >= -hR[1:]).all()       # :1160; layer 1 takes -uhtot unclipped
        closed = M[G[ln]][sl] == 0.0
        assert closed.any() and (D[:, closed] == 0.0).all()
        assert (closed | ~(M[G["mask2dC" + s]][sl] > 0) == closed).all()  # every masked face is a closed one
    sh = H.interior(d, "h")
    assert (out["h"][(slice(None),) + sh] >= GV.Angstrom_H).all() and np.isfinite(out["h"]).all()
    # the halo of h, and every point of uhtr / vhtr outside the face ranges, are left as they were
    keep = np.ones(d.shape2(), bool); keep[sh] = False
    _bits(out["h"][:, keep], inp["h"][:, keep], "h outside the domain")
    for s in "uv":
        keep = np.ones(d.shape2(), bool); keep[H.interior(d, s)] = False
        _bits(out[s + "htr"][:, keep], inp[s + "htr"][:, keep], s + "htr outside the faces")
    # volume: the fluxes cancel pairwise, the domain's edge faces are closed, so sum(areaT*h) changes by rounding only: each new
    # h carries at most 8 roundings of relative size 2**-53 on terms bounded by the donor's h (a face drains at most a quarter of a
    # cell), hence the bound 32 * 2**-53 * sum(areaT*h).  Only meaningful when the Angstrom floor never acted.
    if counts["angstrom_floor"] == 0:
        A = M[G["areaT"]][sh]
        v0 = math.fsum((A[None] * inp["h"][(slice(None),) + sh]).ravel().tolist())
        v1 = math.fsum((A[None] * out["h"][(slice(None),) + sh]).ravel().tolist())
        assert not np.array_equal(out["h"], inp["h"])
        assert abs(v1 - v0) <= 32 * 2.0 ** -53 * v0, (v0, v1)
    print(f"{grid}/{nk}/{name}: angstrom_floor taken {counts['angstrom_floor']} times")


def test_volume_is_conserved_where_the_floor_is_idle(orc):
    """The case of test_exact_properties' volume check must exist: KHTH = 600, dt = 900 on benchmark_small never takes the floor."""
    d, M = GRIDS["benchmark_small"](8)
    _, _, counts, _ = _case_run(d, M, abi.vgrid_default(), "noeos")
    assert counts["angstrom_floor"] == 0


def _turned(d, M, inp):
    T = Turn(d)
    ir = dict(h=T.h(inp["h"]), T=T.h(inp["T"]), S=T.h(inp["S"]), p_surf=T.h(inp["p_surf"]), khth2d=T.h(inp["khth2d"]),
              uhtr=T.v_to_u(inp["vhtr"]), vhtr=T.u_to_v(inp["uhtr"]), slope_x=T.v_to_u(inp["slope_y"]),
              slope_y=T.u_to_v(inp["slope_x"]))
    return T, T.metrics(M), ir


@pytest.mark.parametrize("name", ["eos", "noeos", "slopes_eos", "khth2d", "gm", "large"])
def test_quarter_turn(name, orc):
    """Cell (i, j) -> (nj-1-j, i), u' = -v, v' = u: the u-face results of the turned problem are the v-face results of the
    original.  h, uhtr, vhtr bit for bit; uhGM, vhGM bit for bit except that -0.0 == +0.0 is allowed here (and only here)."""
    d, M = H.island_basin(nk=6)[1:]
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    T, Mr, ir = _turned(d, M, inp)
    da, db = {}, {}
    _, a, _, _ = _case_run(d, M, GV, name, orc=orc, diag=da, inp=inp)
    _, b, _, _ = _case_run(T.dr, Mr, GV, name, orc=orc, diag=db, inp=ir)
    slu, slv, slh = H.interior(T.dr, "u"), H.interior(T.dr, "v"), H.interior(T.dr, "h")
    k = (slice(None),)
    _bits(b["h"][k + slh], T.h(a["h"])[k + slh], name + ": h")
    _bits(b["uhtr"][k + slu], T.v_to_u(a["vhtr"])[k + slu], name + ": uhtr'")
    _bits(b["vhtr"][k + slv], T.u_to_v(a["uhtr"])[k + slv], name + ": vhtr'")
    _bits(db["uhD"][k + slu], T.v_to_u(da["vhD"])[k + slu], name + ": uhD'", signed_zero_ok=True)
    _bits(db["vhD"][k + slv], T.u_to_v(da["uhD"])[k + slv], name + ": vhD'", signed_zero_ok=True)
    assert np.abs(da["uhD"]).max() > 0


def scaled(d, M, GV, P, inp, dt, dim, p=11):
    """The problem in units scaled by 2**p in one of T, L, H, Z, R (MOM_unit_scaling.F90): metrics, GV, the params' unit factors,
    the inputs and dt together; and the factors that unscale the outputs."""
    sc = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0)
    sc[dim] = 2.0 ** p
    T_, L, Hs, Z, Rr = sc["T"], sc["L"], sc["H"], sc["Z"], sc["R"]
    M2 = M.copy()
    for n in abi.METRICS:
        if n.startswith(("dx", "dy")): M2[G[n]] = M[G[n]] * L
        elif n.startswith(("Idx", "Idy")): M2[G[n]] = M[G[n]] / L
        elif n.startswith("area"): M2[G[n]] = M[G[n]] * L * L
        elif n.startswith("Iarea"): M2[G[n]] = M[G[n]] / (L * L)
    M2[G["bathyT"]] = M[G["bathyT"]] * Z
    M2[G["CoriolisBu"]] = M[G["CoriolisBu"]] / T_
    GV2 = abi.vgrid_default()
    GV2.g_Earth = GV.g_Earth * L * L / (Z * T_ * T_); GV2.Rho0 = GV.Rho0 * Rr
    GV2.Angstrom_H = GV.Angstrom_H * Hs; GV2.H_subroundoff = GV.H_subroundoff * Hs; GV2.dZ_subroundoff = GV.dZ_subroundoff * Z
    GV2.H_to_Z = GV.H_to_Z * Z / Hs; GV2.Z_to_H = GV.Z_to_H * Hs / Z
    GV2.H_to_RZ = GV.H_to_RZ * Rr * Z / Hs; GV2.RZ_to_H = GV.RZ_to_H * Hs / (Rr * Z)
    P2 = abi.ThicknessDiffuseParams.from_buffer_copy(P)
    kh = L * L / T_
    P2.Khth = P.Khth * kh; P2.Khth_Min = P.Khth_Min * kh; P2.Khth_Max = P.Khth_Max * kh
    P2.slope_max = P.slope_max * Z / L; P2.kappa_smooth = P.kappa_smooth * Hs * Z / T_
    P2.Z_to_L = P.Z_to_L * L / Z; P2.Z_to_H_fill = P.Z_to_H_fill * Hs / Z
    tr = L * L * Hs
    in2 = dict(h=inp["h"] * Hs, T=inp["T"], S=inp["S"], p_surf=inp["p_surf"] * (Rr * L * L / (T_ * T_)), khth2d=inp["khth2d"] * kh,
               uhtr=inp["uhtr"] * tr, vhtr=inp["vhtr"] * tr, slope_x=inp["slope_x"] * (Z / L), slope_y=inp["slope_y"] * (Z / L))
    unscale = dict(h=1.0 / Hs, uhtr=1.0 / tr, vhtr=1.0 / tr, uhGM=T_ / tr, vhGM=T_ / tr)
    return M2, GV2, P2, in2, dt * T_, unscale


# the EOS takes pressure, temperature and salinity in fixed units (mom6x_eos_params carries no rescaling), so a case that
# evaluates it is scaled in H and Z only, as in tests/test_set_visc_cpu.py
SCALE_CASES = (("noeos", "TLHZR"), ("slopes_noeos", "TLHZR"), ("kmin", "TLHZR"), ("large_noeos", "TLHZR"), ("slopes_eos", "TLHZR"),
               ("gm", "HZ"), ("kd0", "HZ"), ("khth2d", "HZ"))


@pytest.mark.parametrize("name,dims", SCALE_CASES)
def test_unit_scaling_by_2_to_the_11(name, dims, orc):
    d, M = H.benchmark_small(nk=6)[1:]
    GV = abi.vgrid_default()
    P, eos, ps, stored, gm, dt, opts = R.case(name, form=abi.WRIGHT)
    inp = R.inputs(d, M, GV, **opts)
    ref, _ = R.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored, give_gm=True, fill=0.0, orc=orc)
    for dim in dims:
        M2, GV2, P2, in2, dt2, un = scaled(d, M, GV, P, inp, dt, dim)
        got, _ = R.run(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, stored=stored, give_gm=True, fill=0.0, orc=orc)
        for n in ref:
            _bits(got[n] * un[n], ref[n], f"{name}.{dim}:{n}")


def cut(one, d, dt_, s):
    """The part of a one-tile array that a tile's points of stagger `s` cover (a cut in x, in y or in both), and the tile's own
    slices."""
    slt = H.interior(dt_, s)
    i0, j0 = dt_.i_glob0 - dt_.ioff + d.ioff, dt_.j_glob0 - dt_.joff + d.joff
    slg = (slice(slt[0].start + j0, slt[0].stop + j0), slice(slt[1].start + i0, slt[1].stop + i0))
    return slt, slg


# both tiles of the 2 x 1 layout and the four of the 2 x 2 one: the only cut with open water in a halo corner next to a coast
CUT_TILES = [((2, 1), (0, 0)), ((2, 1), (1, 0)), ((2, 2), (0, 0)), ((2, 2), (1, 0)), ((2, 2), (0, 1)), ((2, 2), (1, 1))]


@pytest.mark.parametrize("name", ["eos", "noeos", "gm"])
def test_tile_cut_2x1(name, orc):
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=8)[1:]
    _, one, _, _ = _case_run(d, M, GV, name, orc=orc)
    for layout, pe in CUT_TILES:
        dt_, Mt = H.benchmark_small(nk=8, layout=layout, pe=pe)[1:]
        _, tile, _, _ = _case_run(dt_, Mt, GV, name, orc=orc)
        for n in one:
            s = {"h": "h", "uhtr": "u", "vhtr": "v", "uhGM": "u", "vhGM": "v"}[n]
            slt, slg = cut(one, d, dt_, s)
            _bits(tile[n][:, slt[0], slt[1]], one[n][:, slg[0], slg[1]], f"tile {layout} {pe} {name}:{n}")


REQUIRED = ("bottom_zero_pos", "bottom_zero_neg", "bottom_scale_pos", "bottom_scale_neg", "mag_grad2_zero", "rsum_clip_lo",
            "rsum_clip_hi", "havail_clip_hi", "havail_clip_lo", "uhtot_le0", "uhtot_gt0", "hfrac_zero", "KH_cfl", "KH_max",
            "kap_zero")


def test_the_case_list_reaches_every_branch(orc):
    """Counted over the case list (one EOS form is enough for the walk's branches) on benchmark_small and island_basin at 8 and 75
    layers; the h_avail_rsum clips need the 75-layer EOS case with KHTH = 1e7, dt = 3600.  The Angstrom floor (:613) is a rounding
    guard: its count is reported, not asserted."""
    GV = abi.vgrid_default()
    tot = dict.fromkeys(R.BRANCHES, 0)
    for grid in ("benchmark_small", "island_basin"):
        for nk in (8, 75):
            d, M = GRIDS[grid](nk)
            for name in R.CASES:
                _, _, counts, _ = _case_run(d, M, GV, name, orc=orc)
                for k, v in counts.items():
                    tot[k] += v
    print("branch counts:", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)
