"""set_viscous_BBL's restatement (tests/setvisc_ref.py) on its own: closed forms, its quarter-turn symmetry and its unit scaling,
and the ABI size of mom6x_set_visc_params.  The device is held to the restatement in tests/test_set_visc_gpu.py."""
import ctypes as C

import numpy as np

from mom6_amd import abi
from tests import helpers as H
from tests import setvisc_ref as R
from tests.test_oracle_invariants_cpu import Turn

G = abi.G


def _grid(nk=6, fn=H.benchmark_small):
    gg, d, M = fn(nk=nk)
    return d, M


def _u_faces(d, M):
    return H.interior(d, "u"), M[G["mask2dCu"]][H.interior(d, "u")] > 0


def test_struct_size_matches_the_library():
    assert abi.load_library().mom6x_struct_size(18) == C.sizeof(abi.SetViscParams)


def test_one_layer_column_closed_form():
    """nk = 1, at rest, DRAG_BG_VEL > 0: u* = sqrt(cdrag)*drag_bg_vel, the BBL is the whole (one-layer) column limited by rotation,
    bbl_thick = D / (1/2 + sqrt(1/4 + (D*2f/u*)**2)) (KW99 eq. 2.20 without stratification), Kv = sqrt(cdrag)*u*bbl_thick."""
    d, M = _grid(nk=1)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV, vanish=False, u_max=0.0)
    P = abi.set_visc_params_default(HBBL=1.0e4, Kv=0.0)
    P.drag_bg_vel = 0.05
    out, counts = R.run(d, M, GV, P, inp, Rlay=np.array([1035.0]))
    sl, m = _u_faces(d, M)
    h = inp["h"][0]
    hu = h[sl]; hR = h[sl[0], slice(sl[1].start + 1, sl[1].stop + 1)]
    D = 2.0 * hu * hR / (hu + hR + GV.H_subroundoff)
    q = M[G["CoriolisBu"]]
    C2f = q[slice(sl[0].start - 1, sl[0].stop - 1), sl[1]] + q[sl]
    ustar = np.sqrt(P.cdrag) * P.drag_bg_vel
    want = D / (0.5 + np.sqrt(0.25 + (D * C2f / ustar) ** 2))
    got = out["bbl_thick_u"][sl]
    assert m.sum() > 50 and counts["layer1_rlay"] > 0
    np.testing.assert_allclose(got[m], want[m], rtol=1e-13)
    np.testing.assert_allclose(out["Kv_bbl_u"][sl][m], np.sqrt(P.cdrag) * ustar * want[m], rtol=1e-13)


def test_resting_unstratified_column_is_all_boundary_layer():
    """EOS path, u = v = 0, uniform T and S: no stratification stops the walk, so the BBL height before the rotation limit is
    the whole column (layer 1 included)."""
    d, M = _grid(nk=6)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV, vanish=False, u_max=0.0)
    inp["T"][:] = 8.0; inp["S"][:] = 35.0
    inp["h"][:] = np.where(M[G["mask2dT"]][None] > 0, 500.0, 1e-10)
    P = abi.set_visc_params_default(HBBL=10.0, Kv=0.0)
    P.drag_bg_vel = 0.05
    out, counts = R.run(d, M, GV, P, inp, eos=abi.eos_params_default(abi.WRIGHT))
    sl, m = _u_faces(d, M)
    m &= M[G["mask2dT"]][sl] > 0
    D = 6 * 500.0
    q = M[G["CoriolisBu"]]
    C2f = q[slice(sl[0].start - 1, sl[0].stop - 1), sl[1]] + q[sl]
    ustar = np.sqrt(P.cdrag) * P.drag_bg_vel
    want = D / (0.5 + np.sqrt(0.25 + (D * C2f / ustar) ** 2))
    assert counts["layer1_eos"] > 0 and counts["frac_used"] == 0
    np.testing.assert_allclose(out["bbl_thick_u"][sl][m], want[m], rtol=1e-12)


def test_linear_drag_has_a_constant_ustar():
    """LINEAR_DRAG without EOS or body force: u* = sqrt(cdrag)*DRAG_BG_VEL everywhere, so Kv/bbl_thick = cdrag*DRAG_BG_VEL."""
    d, M = _grid(nk=6)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    Rlay, _ = abi.layer_densities(d.nk)
    P, eos, _, _, _ = R.switch_case("linear", Kv=0.0)
    out, _ = R.run(d, M, GV, P, inp, Rlay=Rlay)
    for s in "uv":
        sl = H.interior(d, s)
        m = M[G["mask2dC" + s]][sl] > 0
        ratio = out["Kv_bbl_" + s][sl][m] / out["bbl_thick_" + s][sl][m]
        np.testing.assert_allclose(ratio, np.sqrt(P.cdrag) * (np.sqrt(P.cdrag) * P.drag_bg_vel), rtol=1e-14)


def _turned(d, M, inp):
    T = Turn(d)
    Mr = T.metrics(M)
    ir = dict(u=T.v_to_u(inp["v"]), v=T.u_to_v(inp["u"]), h=T.h(inp["h"]), T=T.h(inp["T"]), S=T.h(inp["S"]),
              p_surf=T.h(inp["p_surf"]), tideamp=T.h(inp["tideamp"]))
    return T, Mr, ir


def _bits(a, b, name):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    n = int((a.view(np.int64) != b.view(np.int64)).sum())
    assert n == 0, f"{name}: {n} words differ"


def test_quarter_turn_symmetry_of_the_restatement():
    """Cell (i, j) -> (nj-1-j, i), u' = -v, v' = u: the u-face outputs of the turned grid are the v-face outputs of the original
    bit for bit, in the EOS, the Rlay and the body-force paths."""
    d, M = _grid(nk=6, fn=H.island_basin)
    GV = abi.vgrid_default()
    Rlay, _ = abi.layer_densities(d.nk)
    inp = R.inputs(d, M, GV)
    T, Mr, ir = _turned(d, M, inp)
    for name in ("eos", "rlay", "body", "tidal"):
        P, eos, ps, ray, _ = R.switch_case(name, form=abi.WRIGHT)
        a, _ = R.run(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray, fill=0.0)
        b, _ = R.run(T.dr, Mr, GV, P, ir, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray, fill=0.0)
        slu = H.interior(T.dr, "u")
        for n in ("bbl_thick", "Kv_bbl"):
            _bits(b[n + "_u"][slu], T.v_to_u(a[n + "_v"], sign=1.0)[slu], f"{name}:{n}")
            _bits(b[n + "_v"][H.interior(T.dr, "v")], T.u_to_v(a[n + "_u"])[H.interior(T.dr, "v")], f"{name}:{n} (v')")
        if ray:
            _bits(b["Ray_u"][(slice(None),) + slu], T.v_to_u(a["Ray_v"], sign=1.0)[(slice(None),) + slu], f"{name}:Ray")


def scaled(d, M, GV, P, inp, dim, p=11):
    """The problem in units scaled by 2**p in one of T, L, H, Z, R (MOM_unit_scaling.F90), and the factors that unscale the outputs."""
    s = 2.0 ** p
    sc = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0)
    sc[dim] = s
    T_, L, Hs, Z, Rr = sc["T"], sc["L"], sc["H"], sc["Z"], sc["R"]
    M2 = M.copy()
    M2[G["CoriolisBu"]] = M[G["CoriolisBu"]] / T_
    M2[G["bathyT"]] = M[G["bathyT"]] * Z
    GV2 = abi.vgrid_default()
    GV2.g_Earth = GV.g_Earth * L * L / (Z * T_ * T_); GV2.Rho0 = GV.Rho0 * Rr
    GV2.Angstrom_H = GV.Angstrom_H * Hs; GV2.H_subroundoff = GV.H_subroundoff * Hs; GV2.dZ_subroundoff = GV.dZ_subroundoff * Z
    GV2.H_to_Z = GV.H_to_Z * Z / Hs; GV2.Z_to_H = GV.Z_to_H * Hs / Z
    GV2.H_to_RZ = GV.H_to_RZ * Rr * Z / Hs; GV2.RZ_to_H = GV.RZ_to_H * Hs / (Rr * Z)
    P2 = abi.SetViscParams.from_buffer_copy(P)
    P2.drag_bg_vel = P.drag_bg_vel * L / T_ if P.drag_bg_vel < 1e29 else P.drag_bg_vel
    P2.Hbbl = P.Hbbl * Hs; P2.dz_bbl = P.dz_bbl * Z; P2.BBL_thick_min = P.BBL_thick_min * Z
    P2.Kv_BBL_min = P.Kv_BBL_min * Hs * Z / T_; P2.Rad_Earth = P.Rad_Earth * L
    P2.L_to_Z = P.L_to_Z * Z / L; P2.L_to_H = P.L_to_H * Hs / L
    in2 = dict(u=inp["u"] * (L / T_), v=inp["v"] * (L / T_), h=inp["h"] * Hs, T=inp["T"], S=inp["S"],
               p_surf=inp["p_surf"] * (Rr * L * L / (T_ * T_)), tideamp=inp["tideamp"] * (L / T_))
    unscale = dict(bbl_thick=1.0 / Z, Kv_bbl=T_ / (Hs * Z), Ray=T_ / Hs)
    return M2, GV2, P2, in2, unscale, Rr


SCALE_CASES = (("rlay", "TLHZR"), ("body", "HZ"), ("bounds", "HZ"), ("tidal", "HZ"))


def test_unit_scaling_by_2_to_the_11():
    """Every output scales by its exact power of 2 when one of the units is scaled by 2**11.  The EOS paths are scaled in H and Z
    only: the EOS itself takes pressure, temperature and salinity in fixed units (no rescaling in mom6x_eos_params)."""
    d, M = _grid(nk=6)
    GV = abi.vgrid_default()
    Rlay, _ = abi.layer_densities(d.nk)
    inp = R.inputs(d, M, GV)
    for name, dims in SCALE_CASES:
        P, eos, ps, ray, _ = R.switch_case(name, form=abi.WRIGHT)
        ref, _ = R.run(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray, fill=0.0)
        for dim in dims:
            M2, GV2, P2, in2, un, Rr = scaled(d, M, GV, P, inp, dim)
            got, _ = R.run(d, M2, GV2, P2, in2, eos=eos, Rlay=Rlay * Rr, give_ps=ps, give_ray=ray, fill=0.0)
            for n in ref:
                _bits(got[n] * un[n.rsplit("_", 1)[0]], ref[n], f"{name}.{dim}:{n}")


def test_tile_cuts():
    """Each tile of a 2 x 1 and of a 2 x 2 layout, on its cut of the inputs (one halo point is read), gives its own faces of the
    one-tile result.  The 2 x 2 cut puts open water in the halo corner that set_v_at_u and set_u_at_v read (v(i+1, J-1) of a u
    face), which on the closed grids is land."""
    from tests.test_thickness_diffuse_cpu import CUT_TILES, cut
    GV = abi.vgrid_default()
    d, M = _grid(nk=8)
    Rlay, _ = abi.layer_densities(d.nk)
    inp = R.inputs(d, M, GV)
    for name in ("eos", "body", "tidal", "rlay"):
        P, eos, ps, ray, _ = R.switch_case(name, form=abi.WRIGHT)
        one, _ = R.run(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)
        for layout, pe in CUT_TILES:
            dt, Mt = H.benchmark_small(nk=8, layout=layout, pe=pe)[1:]
            tile, _ = R.run(dt, Mt, GV, P, R.inputs(dt, Mt, GV), eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)
            for n in one:
                slt, slg = cut(None, d, dt, n[-1])
                _bits(tile[n][..., slt[0], slt[1]], one[n][..., slg[0], slg[1]], f"tile {layout} {pe} {name}:{n}")
            if layout == (2, 2):      # the corner that points to the middle of the basin is open water
                ci, cj = (dt.ni if pe[0] == 0 else -1), (dt.nj if pe[1] == 0 else -1)
                assert Mt[G["mask2dT"]][dt.joff + cj, dt.ioff + ci] > 0
