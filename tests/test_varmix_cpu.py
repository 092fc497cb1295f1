"""calc_slope_functions' restatement (tests/varmix_ref.py) held to facts that do not come from it: closed forms, the bound of the
slopes, the one-interface limit of the Eady depth scale, the quarter turn, the v faces' weight**2, unit scaling, a tile cut and the
branches its case list reaches; and the exports and ABI size of the device routine.  The device is held to the restatement in
tests/test_varmix_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import varmix_ref as R
from tests.test_oracle_invariants_cpu import Turn
from tests.test_thickness_diffuse_cpu import GRIDS, _bits, _flat, scaled

G = abi.G


def test_exports_and_struct_size():
    lib = abi.load_library()
    assert hasattr(lib, "mom6x_varmix_init") and hasattr(lib, "mom6x_calc_slope_functions")
    assert lib.mom6x_struct_size(21) == C.sizeof(abi.VarMixParams)
    assert lib.mom6x_abi_version() == 6
    p = abi.varmix_params_default()
    assert (p.kappa_smooth, p.VarMix_Ktop, p.h_min_N2, p.Visbeck_S_max, p.Eady_GR_D_scale, p.cropping_distance) == (
        1.0e-6, 2, 1.0, 0.0, 0.0, 0.0)
    assert all(getattr(p, n) == 0 for n in abi.VARMIX_MUST_BE_0)


def _case_run(d, M, GV, name, form=abi.WRIGHT, orc=None, inp=None, fill=np.nan, mods=None):
    P, eos, ps, dg, dt, opts = R.case(name, GV, form=form, nk=d.nk)
    for k, v in (mods or {}).items():
        setattr(P, k, v)
    if inp is None:
        inp = R.inputs(d, M, GV, **opts)
    out, counts = R.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, give_diag=dg, orc=orc, fill=fill)
    return P, inp, out, counts


@pytest.mark.parametrize("name", ["eady_diag", "visbeck_diag", "eady_noeos", "visbeck_noeos", "just_e", "just_e_full"])
def test_level_interfaces_give_no_slope(name, orc):
    """Level interfaces over a flat bottom with T, S that vary with depth only: every slope is zero and SN = 0 in all three
    branches, with and without an EOS."""
    d, M = _flat(6)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    one = np.ones(d.shape2())
    inp["h"] = np.full(d.shape3(), 4000.0 / d.nk)
    inp["T"] = np.stack([(20.0 - 3.0 * k) * one for k in range(d.nk)])
    inp["S"] = np.stack([(34.0 + 0.2 * k) * one for k in range(d.nk)])
    inp["p_surf"] = 1.0e4 * one
    P, _, out, _ = _case_run(d, M, GV, name, orc=orc, inp=inp)
    for s in ("SN_u", "SN_v"):
        assert (out[s][np.isfinite(out[s])] == 0.0).all() and np.isfinite(out[s][H.interior(d, s[-1])]).all()
    if P.use_stored_slopes:
        for s, rng in (("slope_x", (-2, d.ni, -1, d.nj)), ("slope_y", (-1, d.ni, -2, d.nj))):
            a = R._A(d, out[s], rng)[1:d.nk]
            assert (a == 0.0).all()
            assert np.isnan(out[s][0]).all() and np.isnan(out[s][d.nk]).all()


def test_two_layers_one_tilted_interface_closed_form():
    """No EOS, two layers: slope_x(I,j,2) = (e(i+1,2)-e(i,2))*IdxCu (MOM_isopycnal_slopes.F90:397) and the same at the v faces;
    branch 3's SN_u = mask2dCu*sqrt((H_geom*S2)*(g_prime(2)/max(Hdn,Hup,h_min_N2)) / max(bathyT(i),bathyT(i+1))) (:1201-1242) with
    the slopes of the one interface."""
    d, M = _flat(2)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    ii = (np.arange(d.pitch) - d.ioff)[None, :] * np.ones(d.shape2())
    jj = (np.arange(d.shape2()[0]) - d.joff)[:, None] * np.ones(d.shape2())
    h = np.empty(d.shape3())
    h[1] = 2000.0 + 0.5 * ii + 0.25 * jj
    h[0] = 4000.0 - h[1]
    inp["h"] = h
    e2 = -(M[G["bathyT"]] + 0.0) + h[1] * GV.H_to_Z
    _, _, out, _ = _case_run(d, M, GV, "visbeck_noeos", inp=inp)
    for s, rng, far, Ig in (("slope_x", (-2, d.ni, -1, d.nj), (1, 0), "IdxCu"), ("slope_y", (-1, d.ni, -2, d.nj), (0, 1), "IdyCv")):
        want = (R._A(d, e2, rng, *far) - R._A(d, e2, rng)) * R._A(d, M[G[Ig]], rng)
        assert (want != 0.0).sum() > 100
        _bits(R._A(d, out[s][1], rng), want, s)
    Rlay, gp = abi.layer_densities(2, Rho0=GV.Rho0, g_Earth=GV.g_Earth)
    P, _, out, counts = _case_run(d, M, GV, "just_e", inp=inp)
    assert counts["H_cutoff_mask"] == 0
    Ex = (np.roll(e2, -1, axis=1) - e2) * M[G["IdxCu"]]
    Ey = (np.roll(e2, -1, axis=0) - e2) * M[G["IdyCv"]]
    sl = H.interior(d, "u")
    sq = lambda a: a * a
    sh = lambda a, di, dj: np.roll(np.roll(a, -di, axis=1), -dj, axis=0)
    S2 = sq(Ex) + 0.25 * ((sq(Ey) + sq(sh(Ey, 1, -1))) + (sq(sh(Ey, 1, 0)) + sq(sh(Ey, 0, -1))))
    Hh = 2. * h[1] * h[0] / (h[1] + h[0] + GV.H_subroundoff)
    Hdn, Hup = Hh, sh(Hh, 1, 0)
    bT = M[G["bathyT"]]
    want = M[G["mask2dCu"]] * np.sqrt((np.sqrt(Hdn * Hup) * S2) * (gp[1] / np.maximum(np.maximum(Hdn, Hup), P.h_min_N2))
                                      / np.maximum(bT, sh(bT, 1, 0)))
    assert (want[sl] > 0.0).sum() > 100
    _bits(out["SN_u"][sl], want[sl], "SN_u")


@pytest.mark.parametrize("name", ["eady", "visbeck", "visbeck_neg"])
def test_slopes_are_bounded_by_one(name, orc):
    d, M = GRIDS["island_basin"](8)
    _, _, out, _ = _case_run(d, M, abi.vgrid_default(), name, orc=orc)
    for s in ("slope_x", "slope_y"):
        a = out[s][np.isfinite(out[s])]
        assert a.size > 1000 and (np.abs(a) <= 1.0).all() and np.abs(a).max() > 0.0


def test_eady_depth_scale_above_the_first_interface(orc):
    """EADY_GROWTH_RATE_D_SCALE = 1 m, less than dzu(K=2), without cropping: interface 2 takes the weight D_scale/dzu and fills the
    depth scale, so the un-combined SN_u (rows jsc-1 and jec+1 keep it) is the one-interface value
    mask*((w*dzSxN(2))/(dz_neglect + w*dzu(2))).  The bound: sum_dz after interface 2 is 1 m up to the two roundings of w and
    w*dzu (2**-52 relative), so an interface K below sees dz = max(0, D_scale - sum_dz) <= 2**-52 m, a weight <= 2**-52/dzu(K), and adds
    at most 2**-52*dzSxN(K)/dzu(K) to vint_SN; the final division by sum_dz moves the result by another 2**-52 relative at most."""
    d, M = H.benchmark_small(nk=8, layout=(1, 2), pe=(0, 1))[1:]       # the northern tile: its row jsc-1 is open water
    GV = abi.vgrid_default()
    _, _, out, _ = _case_run(d, M, GV, "eady_diag", orc=orc, mods=dict(Eady_GR_D_scale=1.0, cropping_distance=-1.0))
    dzn = GV.dZ_subroundoff
    rng = (-1, d.ni - 1, -1, -1)
    dz2, sn2 = R._A(d, out["dzu"][1], rng), R._A(d, out["dzSxN"][1], rng)
    sel = dz2 > 1.0
    w = (1.0 - dzn) / (dz2 + dzn)                                       # dnew = min(dz_neglect + dzu, D_scale) = D_scale
    want = R._A(d, M[G["mask2dCu"]], rng) * ((w * sn2) / (dzn + w * dz2))
    got = R._A(d, out["SN_u"], rng)
    below = sum(R._A(d, out["dzSxN"][k], rng) / (R._A(d, out["dzu"][k], rng) + dzn) for k in range(2, d.nk))
    tol = 2.0 ** -52 * below + 2.0 ** -51 * np.abs(want)
    assert (want[sel] > 0).sum() > 10 and (np.abs(got - want) <= tol)[sel].all()


def test_v_faces_accumulate_weight_squared(orc):
    """calc_Eady_growth_rate_2D sums weight*dzSxN at the u faces but weight**2*dzSyN at the v faces (:1028 against :1071).  The v
    points outside isc..iec keep the un-combined value: recomputed here from the posted dzv, dzSyN with weight**2 it must match
    bit for bit, and with weight it must not (so that a `fix` of the asymmetry fails here)."""
    d, M = H.benchmark_small(nk=8, layout=(2, 1), pe=(0, 0))[1:]       # the western tile: its column iec+1 is open water
    GV = abi.vgrid_default()
    P, inp, out, _ = _case_run(d, M, GV, "eady_diag", orc=orc)
    e = R.find_eta(d, M, inp["h"], P.H_to_Z)
    dzn = GV.dZ_subroundoff
    r_crp = 1. / max(dzn, P.cropping_distance)
    differs = False
    for i in (-1, d.ni):
        rng = (i, i, -1, d.nj - 1)
        A = lambda a, dj=0: R._A(d, a, rng, 0, dj)
        res = {}
        for power in (1, 2):
            vint, sum_dz = np.zeros(A(e[0]).shape), np.full(A(e[0]).shape, dzn)
            for k in range(1, d.nk):
                dzk = A(out["dzv"][k])
                dz = np.maximum(0., np.minimum(sum_dz + dzk, P.Eady_GR_D_scale) - sum_dz)
                w = dz / (dzk + dzn)
                w = w * np.minimum(np.maximum(0., (np.minimum(A(e[0]), A(e[0], 1)) - np.maximum(A(e[k]), A(e[k], 1))) * r_crp), 1.)
                w = w * np.minimum(np.maximum(0., (np.minimum(A(e[k]), A(e[k], 1)) - np.maximum(A(e[d.nk]), A(e[d.nk], 1))) * r_crp), 1.)
                vint = vint + (w * w if power == 2 else w) * A(out["dzSyN"][k])
                sum_dz = sum_dz + w * dzk
            res[power] = A(M[G["mask2dCv"]]) * (vint / sum_dz)
        _bits(A(out["SN_v"]), res[2], f"SN_v at i = {i}")
        differs |= bool((res[1] != res[2]).any())
    assert differs


def _turn_inputs(T, inp):
    return dict(h=T.h(inp["h"]), T=T.h(inp["T"]), S=T.h(inp["S"]), p_surf=T.h(inp["p_surf"]))


@pytest.mark.parametrize("name", ["visbeck", "visbeck_diag", "visbeck_noeos", "just_e", "just_e_full"])
def test_quarter_turn(name, orc):
    """Cell (i, j) -> (nj-1-j, i): the u-face results of the turned problem are the v-face results of the original, slope_x' =
    -slope_y, bit for bit, in the branches with stored slopes alone and with neither switch.  The simpler Eady growth rate is
    left out on purpose: its v faces sum weight**2 (test_v_faces_accumulate_weight_squared)."""
    d, M = H.island_basin(nk=6)[1:]
    GV = abi.vgrid_default()
    T = Turn(d)
    Mr = T.metrics(M)
    _, inp, a, _ = _case_run(d, M, GV, name, orc=orc, fill=0.0)
    _, _, b, _ = _case_run(T.dr, Mr, GV, name, orc=orc, inp=_turn_inputs(T, inp), fill=0.0)
    slu, slv = H.interior(T.dr, "u"), H.interior(T.dr, "v")
    k = (slice(1, d.nk),)
    _bits(b["SN_u"][slu], T.v_to_u(a["SN_v"], sign=1.0)[slu], name + ": SN_u'")
    _bits(b["SN_v"][slv], T.u_to_v(a["SN_u"])[slv], name + ": SN_v'")
    assert np.abs(a["SN_u"]).max() > 0
    if "slope_x" in a:
        _bits(b["slope_x"][k + slu], T.v_to_u(a["slope_y"])[k + slu], name + ": slope_x'", signed_zero_ok=True)
        _bits(b["slope_y"][k + slv], T.u_to_v(a["slope_x"])[k + slv], name + ": slope_y'", signed_zero_ok=True)
    if "N2_u" in a:
        _bits(b["N2_u"][k + slu], T.v_to_u(a["N2_v"], sign=1.0)[k + slu], name + ": N2_u'")
        _bits(b["S2_u"][slu], T.v_to_u(a["S2_v"], sign=1.0)[slu], name + ": S2_u'")
        _bits(b["S2_v"][slv], T.u_to_v(a["S2_u"])[slv], name + ": S2_v'")


def scaled_varmix(d, M, GV, P, inp, dt, dim, p=11):
    """The problem in units scaled by 2**p in one of T, L, H, Z, R: the metrics, GV and dt from thickness_diffuse's scaled(), the
    VarMix members, GV%Rlay and GV%g_prime here; and the factors that unscale the outputs."""
    sc = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0)
    sc[dim] = 2.0 ** p
    T_, L, Hs, Z, Rr = sc["T"], sc["L"], sc["H"], sc["Z"], sc["R"]
    dummy = dict(h=inp["h"], T=inp["T"], S=inp["S"], p_surf=inp["p_surf"])
    dummy.update({n: np.zeros(1) for n in ("khth2d", "uhtr", "vhtr", "slope_x", "slope_y")})
    M2, GV2, _, in2, dt2, _ = scaled(d, M, GV, abi.thickness_diffuse_params_default(), dummy, dt, dim, p)
    P2 = abi.VarMixParams.from_buffer_copy(P)
    P2.kappa_smooth = P.kappa_smooth * Hs * Z / T_; P2.Visbeck_S_max = P.Visbeck_S_max * Z / L
    P2.Eady_GR_D_scale = P.Eady_GR_D_scale * Z; P2.cropping_distance = P.cropping_distance * Z
    P2.h_min_N2 = P.h_min_N2 * Hs; P2.max_depth = P.max_depth * Z; P2.Angstrom_Z = P.Angstrom_Z * Z
    P2.H_to_Z = GV2.H_to_Z; P2.H_to_RZ = GV2.H_to_RZ; P2.g_Earth = GV2.g_Earth; P2.Rho0 = GV2.Rho0
    P2.Z_to_L = P.Z_to_L * L / Z; P2.Z_to_H_fill = P.Z_to_H_fill * Hs / Z
    Rlay, gp = abi.layer_densities(d.nk, Rho0=GV.Rho0, g_Earth=GV.g_Earth)
    un = dict(SN_u=T_, SN_v=T_, slope_x=L / Z, slope_y=L / Z, N2_u=(Z * T_ / L) ** 2, N2_v=(Z * T_ / L) ** 2, dzu=1 / Z, dzv=1 / Z,
              dzSxN=T_ / Z, dzSyN=T_ / Z, S2_u=(L / Z) ** 2, S2_v=(L / Z) ** 2)
    return M2, GV2, P2, {n: in2[n] for n in ("h", "T", "S", "p_surf")}, dt2, Rlay * Rr, gp * (L * L / (Z * T_ * T_)), un


# the EOS takes pressure, temperature and salinity in fixed units, so a case that evaluates it is scaled in H and Z only
SCALE_CASES = (("just_e", "TLHZR"), ("just_e_full", "TLHZR"), ("eady_noeos", "TLHZR"), ("visbeck_noeos", "TLHZR"),
               ("eady_diag", "HZ"), ("visbeck_diag", "HZ"))


@pytest.mark.parametrize("name,dims", SCALE_CASES)
def test_unit_scaling_by_2_to_the_11(name, dims, orc):
    d, M = H.benchmark_small(nk=6)[1:]
    GV = abi.vgrid_default()
    P, eos, ps, dg, dt, opts = R.case(name, GV, form=abi.WRIGHT, nk=d.nk)
    inp = R.inputs(d, M, GV, **opts)
    ref, _ = R.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, give_diag=dg, orc=orc, fill=0.0)
    for dim in dims:
        M2, GV2, P2, in2, dt2, Rlay2, gp2, un = scaled_varmix(d, M, GV, P, inp, dt, dim)
        got, _ = R.run(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, give_diag=dg, orc=orc, fill=0.0, Rlay=Rlay2, g_prime=gp2)
        for n in ref:
            _bits(got[n] * un[n], ref[n], f"{name}.{dim}:{n}")


STAG = dict(SN_u="u", SN_v="v", slope_x="u", slope_y="v", N2_u="u", N2_v="v", dzu="u", dzv="v", dzSxN="u", dzSyN="v", S2_u="u",
            S2_v="v")


def cut2(d, dt_, s):
    """The part of a one-tile array that a tile's own points of stagger `s` cover (a cut in x, in y or in both), and the tile's own
    slices."""
    slt = H.interior(dt_, s)
    i0, j0 = dt_.i_glob0 - dt_.ioff + d.ioff, dt_.j_glob0 - dt_.joff + d.joff
    slg = (slice(slt[0].start + j0, slt[0].stop + j0), slice(slt[1].start + i0, slt[1].stop + i0))
    return slt, slg


# (2, 2): the only cut with open water in a halo corner next to a coast (the four-face averages read those corners)
TILES = [((2, 1), (0, 0)), ((2, 1), (1, 0)), ((1, 2), (0, 0)), ((1, 2), (0, 1)),
         ((2, 2), (0, 0)), ((2, 2), (1, 0)), ((2, 2), (0, 1)), ((2, 2), (1, 1))]


@pytest.mark.parametrize("name", ["eady_diag", "visbeck_diag", "just_e"])
def test_tile_cuts(name, orc):
    """Each tile of a 2 x 1, of a 1 x 2 and of a 2 x 2 layout, on its cut of the inputs (halos two wide and more), gives its own
    faces of the one-tile result.  The y cut puts open water on a tile's rows jsc-1 and jec+1 (the grids have a rim of land
    there), the 2 x 2 cut also in the halo corner that points to the middle of the basin."""
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=8)[1:]
    _, _, one, _ = _case_run(d, M, GV, name, orc=orc)
    for layout, pe in TILES:
        dt_, Mt = H.benchmark_small(nk=8, layout=layout, pe=pe)[1:]
        _, _, tile, _ = _case_run(dt_, Mt, GV, name, orc=orc)
        for n in one:
            slt, slg = cut2(d, dt_, STAG[n])
            _bits(tile[n][..., slt[0], slt[1]], one[n][..., slg[0], slg[1]], f"tile {layout} {pe} {name}:{n}")
        if layout == (1, 2) and pe == (0, 1):
            assert (tile["SN_v"][dt_.joff - 1, dt_.ioff:dt_.ioff + dt_.ni] > 0.0).sum() > 10      # row J = jsc-1 is open water


REQUIRED = ("mag_grad2_zero", "N2_clipped", "S2max_applied", "S2max_idle", "Dscale_full", "Dscale_partial", "Dscale_zero",
            "crop_top_0", "crop_top_mid", "crop_top_1", "crop_bot_0", "crop_bot_mid", "crop_bot_1", "H_cutoff_mask", "bathy_cutoff",
            "denom_bathy", "denom_dztot")


def test_the_case_list_reaches_every_branch(orc):
    """Counted over the case list (one EOS form is enough for the walks' branches) on benchmark_small and island_basin at 8 and 75
    layers.  H_u <= 0 in calc_Visbeck_coeffs_old (:890) cannot be reached with h >= Angstrom_H (H_geom is a product of square roots
    of positive thicknesses): its count, and that of the clipped radicand of dzSxN, are reported, not asserted."""
    GV = abi.vgrid_default()
    tot = dict.fromkeys(R.BRANCHES, 0)
    for grid in ("benchmark_small", "island_basin"):
        for nk in (8, 75):
            d, M = GRIDS[grid](nk)
            for name, form in R.case_list(forms=(abi.WRIGHT,)):
                _, _, _, counts = _case_run(d, M, GV, name, form=form, orc=orc)
                for k, v in counts.items():
                    tot[k] += v
    print("branch counts:", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)
