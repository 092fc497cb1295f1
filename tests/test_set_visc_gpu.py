"""mom6x_set_viscous_BBL on the device (mom6_amd/csrc/set_visc.hip) against the restatement tests/setvisc_ref.py, bit for bit:
every switch set and EOS form on coasts, narrowed faces and vanished bottom layers; the faces it must leave alone; the headline
grid's quarter turn, unit scaling and bounds; and 2 x 1 and 2 x 2 tile cuts of the same problem."""
import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import setvisc_ref as R
from tests.test_thickness_diffuse_cpu import CUT_TILES, cut

pytestmark = pytest.mark.gpu
G = abi.G
FORMS = (abi.LINEAR, abi.WRIGHT, abi.WRIGHT_FULL, abi.WRIGHT_REDUCED, abi.UNESCO, abi.ROQUET_RHO, abi.JACKETT06, abi.ROQUET_SPV)


def _device(d, M, GV, P, inp, eos=None, Rlay=None, give_ps=False, give_ray=False, fill=np.nan, dy=None):
    """One mom6x_set_viscous_BBL call on inputs that live on the host; outputs start as `fill`.  In a context of its own, or in
    the caller's `dy`, which is then left open."""
    import torch
    from mom6_amd.dycore import Dycore
    own = dy is None
    if own:
        dy = Dycore(d, M, GV)
    try:
        if Rlay is not None:
            dy.PressureForce_init(abi.pgf_params_default(GV.Rho0), Rlay, np.full(d.nk, GV.g_Earth))
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        dy.set_visc_init(P, eos, t["tideamp"])
        out = dict(Kv_bbl_u=dy.to_dev(np.full(d.shape2(), fill)), Kv_bbl_v=dy.to_dev(np.full(d.shape2(), fill)),
                   bbl_thick_u=dy.to_dev(np.full(d.shape2(), fill)), bbl_thick_v=dy.to_dev(np.full(d.shape2(), fill)))
        if give_ray:
            out["Ray_u"] = dy.to_dev(np.full(d.shape3(), fill)); out["Ray_v"] = dy.to_dev(np.full(d.shape3(), fill))
        torch.cuda.synchronize()
        dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], p_surf=t["p_surf"] if give_ps else None, **out)
        dy.sync()
        return {n: a.cpu().numpy() for n, a in out.items()}
    finally:
        if own:
            dy.close()


def _bits(a, b, name):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    ne = a.view(np.int64) != b.view(np.int64)
    n = int(ne.sum())
    if n:
        raise AssertionError(f"{name}: {n} of {a.size} words differ; max|diff| {np.nanmax(np.abs(a - b)[ne]):.3e}")


GRIDS = {"benchmark_small": lambda nk: H.benchmark_small(nk=nk)[1:],
         "island_basin": lambda nk: H.island_basin(nk=nk)[1:],
         "partial_faces": lambda nk: (lambda d, M: (d, H.partial_faces(d, M)))(*H.benchmark_small(nk=nk)[1:])}
CASES = [(s, None) for s in R.SWITCHES if s != "eos"] + [("eos", f) for f in FORMS]


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("nk", [8, 75])
def test_parity_with_the_restatement(grid, nk, orc):
    """Every switch set (and BBL_USE_EOS with each of the eight EOS forms) bit for bit, the whole output arrays included: faces
    that are masked or outside :450-460 keep the NaN they started with, and Ray_u/v are zero except where body-force drag adds."""
    d, M = GRIDS[grid](nk)
    GV = abi.vgrid_default()
    Rlay, _ = abi.layer_densities(nk)
    base = R.inputs(d, M, GV)
    tot = dict.fromkeys(R.BRANCHES, 0)
    for name, form in CASES:
        P, eos, ps, ray, opts = R.switch_case(name, form=form)
        inp = R.inputs(d, M, GV, **opts) if opts else base
        want, counts = R.run(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray, orc=orc)
        got = _device(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)
        for n in want:
            _bits(got[n], want[n], f"{grid}/{nk}/{name}/{form}:{n}")
        for s in "uv":
            sl = H.interior(d, s)
            m = M[G["mask2dC" + s]][sl] > 0
            assert np.isfinite(got["bbl_thick_" + s][sl][m]).all()
            untouched = np.ones(d.shape2(), bool)
            untouched[sl] = ~m
            assert np.isnan(got["bbl_thick_" + s][untouched]).all() and np.isnan(got["Kv_bbl_" + s][untouched]).all()
        if ray:
            for s in "uv":
                sl = H.interior(d, s)
                face = np.zeros(d.shape2(), bool)
                face[sl] = M[G["mask2dC" + s]][sl] > 0
                Ray = got["Ray_" + s]
                assert np.isfinite(Ray).all() and (Ray[:, face] != 0).any() and (Ray[:, ~face] == 0).all()
        for k, v in counts.items():
            tot[k] += v
    for k in ("vanished_skip", "frac_used", "layer1_eos", "layer1_rlay", "thick_min", "correct_bounds", "body_force", "RiNo_cap"):
        assert tot[k] > 0, (k, tot)


def test_parity_at_360x180x75_wright(orc):
    gg, d, M = H.benchmark_360()
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    for name in ("eos", "body"):
        P, eos, ps, ray, _ = R.switch_case(name, form=abi.WRIGHT)
        want, counts = R.run(d, M, GV, P, inp, eos=eos, give_ps=ps, give_ray=ray, orc=orc)
        got = _device(d, M, GV, P, inp, eos=eos, give_ps=ps, give_ray=ray)
        for n in want:
            _bits(got[n], want[n], f"360/{name}:{n}")
        assert counts["frac_used"] > 0 and counts["vanished_skip"] > 0


def test_off_and_refused_settings():
    """BOTTOMDRAGLAW = False writes nothing; CHANNEL_DRAG, a bulk mixed layer, open boundaries, ice shelves and SpV_avg are
    refused at set_visc_init; body-force drag without Ray_u/v is refused at the call."""
    import torch
    from mom6_amd.dycore import Dycore
    gg, d, M = H.benchmark_small(nk=8)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        for member in ("channel_drag", "nkml", "open_bcs", "ice_shelf", "SpV_avg"):
            P = abi.set_visc_params_default()
            setattr(P, member, 1)
            with pytest.raises(Exception):
                dy.set_visc_init(P, abi.eos_params_default())
        P = abi.set_visc_params_default(); P.bottomdraglaw = 0
        dy.set_visc_init(P, abi.eos_params_default())
        out = [dy.to_dev(np.full(d.shape2(), np.nan)) for _ in range(4)]
        torch.cuda.synchronize()
        dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], Kv_bbl_u=out[0], Kv_bbl_v=out[1], bbl_thick_u=out[2],
                           bbl_thick_v=out[3])
        dy.sync()
        assert all(bool(torch.isnan(a).all()) for a in out)
        P = abi.set_visc_params_default(); P.body_force_drag = 1
        dy.set_visc_init(P, abi.eos_params_default())
        with pytest.raises(Exception):
            dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], Kv_bbl_u=out[0], Kv_bbl_v=out[1], bbl_thick_u=out[2],
                               bbl_thick_v=out[3])
    finally:
        dy.close()


def test_tile_cut_2x1():
    """Each tile of a 2 x 1 and of a 2 x 2 layout, called on its cut of the inputs (halos included), gives its part of the one-tile
    result, the west and south edge faces (I = isc-1, J = jsc-1) included.  The 2 x 2 cut is the one with open water in a halo
    corner next to a coast: v(i+1, J-1) of a u face, u(I-1, j+1) of a v face."""
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=8)[1:]
    inp = R.inputs(d, M, GV)
    for name in ("eos", "body", "tidal", "rlay"):
        P, eos, ps, ray, _ = R.switch_case(name, form=abi.WRIGHT)
        Rlay, _ = abi.layer_densities(d.nk)
        one = _device(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)
        for layout, pe in CUT_TILES:
            gg, dt, Mt = H.benchmark_small(nk=8, layout=layout, pe=pe)
            it = R.inputs(dt, Mt, GV)
            for s in "uv":
                slt, slg = cut(None, d, dt, s)
                _bits(it["u" if s == "u" else "v"][:, slt[0], slt[1]], inp[s][:, slg[0], slg[1]], f"input {s}")
            tile = _device(dt, Mt, GV, P, it, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)
            for n in one:
                slt, slg = cut(None, d, dt, n[-1])
                _bits(tile[n][..., slt[0], slt[1]], one[n][..., slg[0], slg[1]], f"tile {layout} {pe} {name}:{n}")


# -- the headline grid, device only ----------------------------------------------------------------------------------------------

def _headline_state(d, Md, seed=5):
    import torch
    from mom6_amd import synth_dev
    dev = Md.device
    h, u, v = synth_dev.make_state(d, Md, u_max=0.3, h_pert=0.01)
    kk = torch.arange(d.nk, dtype=torch.float64, device=dev)[:, None, None] / max(d.nk - 1, 1)
    T = (10.0 + (10.0 - 15.0 * kk) + 0.8 * synth_dev.smooth_field(d, dev, seed, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    S = (34.5 + (kk - 0.5) + 0.2 * synth_dev.smooth_field(d, dev, seed + 100, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    tideamp = (0.03 * (1.0 + 0.5 * synth_dev.smooth_field(d, dev, seed + 301, ox=0.5, oy=0.5))).contiguous()
    return dict(u=u, v=v, h=h, T=T, S=S, tideamp=tideamp)


def _dev_call(d, M, GV, P, t, eos, Rlay=None):
    import torch
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        if Rlay is not None:
            dy.PressureForce_init(abi.pgf_params_default(GV.Rho0), Rlay, np.full(d.nk, GV.g_Earth))
        dy.set_visc_init(P, eos, t["tideamp"])
        out = {n: torch.zeros(d.shape2(), dtype=torch.float64, device=t["h"].device) for n in ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")}
        torch.cuda.synchronize()
        dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], **out)
        dy.sync()
        return out
    finally:
        dy.close()


def test_headline_turn_scaling_and_bounds():
    """1440 x 1080 x 75, WRIGHT: the quarter turn maps the v-face outputs onto the u-face outputs of the turned grid bit for bit;
    scaling H or Z (and, in the Rlay path, T, L or R) by 2**11 scales every output by its exact power; bbl_thick >= BBL_THICK_MIN,
    Kv >= KV_BBL_MIN, all finite."""
    import torch
    from tests.test_invariants_gpu import TTurn, _basin
    from tests.test_set_visc_cpu import scaled
    dev = torch.device("cuda", 0)
    d, M = _basin("full")
    Md = torch.as_tensor(M, device=dev)
    GV = abi.vgrid_default()
    t = _headline_state(d, Md)
    P, eos, _, _, _ = R.switch_case("bg0", form=abi.WRIGHT)
    P.BBL_thick_min = 2.0
    ref = _dev_call(d, M, GV, P, t, eos)
    for s in "uv":
        sl = H.interior(d, s)
        m = Md[G["mask2dC" + s]][sl] > 0
        bt, kv = ref["bbl_thick_" + s][sl][m], ref["Kv_bbl_" + s][sl][m]
        assert bool(torch.isfinite(bt).all()) and bool(torch.isfinite(kv).all())
        assert bool((bt >= P.BBL_thick_min).all()) and bool((kv >= P.Kv_BBL_min).all())
    # quarter turn
    T = TTurn(d)
    Mr = T.metrics(M)
    tr = dict(u=T.v_to_u(t["v"]), v=T.u_to_v(t["u"]), h=T.h(t["h"]), T=T.h(t["T"]), S=T.h(t["S"]), tideamp=T.h(t["tideamp"]))
    rot = _dev_call(T.dr, Mr, GV, P, tr, eos)
    del tr
    slu, slv = H.interior(T.dr, "u"), H.interior(T.dr, "v")
    for n in ("bbl_thick", "Kv_bbl"):
        a = T.v_to_u(ref[n + "_v"], sign=1.0)[slu]; b = rot[n + "_u"][slu]
        assert bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all()), n + " (turn, u')"
        a = T.u_to_v(ref[n + "_u"])[slv]; b = rot[n + "_v"][slv]
        assert bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all()), n + " (turn, v')"
    del rot
    # unit scaling
    Rlay, _ = abi.layer_densities(d.nk)
    for name, eos_s, dims, base in (("bg0", eos, "HZ", ref), ("rlay", None, "TLHZR", None)):
        Pn, _, _, _, _ = R.switch_case(name, form=abi.WRIGHT)
        if name == "bg0":
            Pn.BBL_thick_min = 2.0
        else:
            base = _dev_call(d, M, GV, Pn, t, None, Rlay=Rlay)
        for dim in dims:
            tn = {k: a for k, a in t.items()}
            M2, GV2, P2, _, un, Rr = scaled(d, M, GV, Pn, {k: np.zeros(1) for k in ("u", "v", "h", "T", "S", "p_surf", "tideamp")}, dim)
            sc = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0); sc[dim] = 2.0 ** 11
            vel = sc["L"] / sc["T"]
            tn = dict(u=t["u"] * vel, v=t["v"] * vel, h=t["h"] * sc["H"], T=t["T"], S=t["S"], tideamp=t["tideamp"] * vel)
            got = _dev_call(d, M2, GV2, P2, tn, eos_s, Rlay=None if eos_s is not None else Rlay * Rr)
            del tn
            for n in got:
                a = got[n] * un[n.rsplit("_", 1)[0]]
                assert bool((a.view(torch.int64) == base[n].view(torch.int64)).all()), f"{name}.{dim}:{n}"


def test_coupling_over_steps(orc, sums):
    """Four dynamics steps of benchmark_small (WRIGHT in the pressure force and in the BBL, BOTTOMDRAGLAW, vertvisc_coef inside
    the step), set_viscous_BBL before each: mom6x_set_viscous_BBL on the device, the restatement feeding the oracle's step
    (OrcModel.set_vertvisc reads the same four arrays, updated in place).  u, v, h, uh, vh bit for bit in each arithmetic of the
    mass-flux kernels (the `sums` fixture), the four BBL fields too; Kv_bbl_u must change between steps."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import cases
    cfg = H.benchmark_small()
    gg, d, M = cfg
    inp = cases.rk2_inputs(cfg)
    GV, Rlay, gp, dt = inp["GV"], inp["Rlay"], inp["gp"], inp["dt"]
    bt_mod = dict(strong_drag=1)   # (the default drag path goes through btstep's pow: not bit-exact, tests/test_rk2_gpu.py)
    T, S = cases.thermo_state(d, M)
    eos = abi.eos_params_default(abi.WRIGHT)
    vv = abi.vertvisc_params_default()
    sv = abi.set_visc_params_default(HBBL=vv.Hbbl, Kv=vv.Kv)
    sv.drag_bg_vel = 0.05
    names = ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")
    nsteps = 4

    # ---------------- oracle: the restatement before each orc step
    cont, bt, cor, pgf, rk2 = cases.rk2_params(d, GV, bt_mod)
    m = orc.OrcModel(d, M, GV, cont, bt, cor, pgf, rk2, Rlay, gp, 0)
    m.set_tv(T, S, eos)
    ovis = {n: np.zeros(d.shape2()) for n in names}
    m.set_vertvisc(vv, *(ovis[n] for n in names), None, None, None)
    so = dict(u=inp["u"].copy(), v=inp["v"].copy(), h=inp["h"].copy(), uh=np.zeros_like(inp["h"]), vh=np.zeros_like(inp["h"]),
              uhtr=np.zeros_like(inp["h"]), vhtr=np.zeros_like(inp["h"]), eta_av=np.zeros(d.shape2()))
    R.set_viscous_BBL(d, M, GV, sv, so["u"], so["v"], so["h"], T=T, S=S, eos=eos, orc=orc, **ovis)
    m.initialize(so["u"], so["v"], so["h"], so["uh"], so["vh"], dt)
    ohist = []
    for n in range(nsteps):
        R.set_viscous_BBL(d, M, GV, sv, so["u"], so["v"], so["h"], T=T, S=S, eos=eos, orc=orc, **ovis)
        ohist.append({k: a.copy() for k, a in ovis.items()})
        m.step(so["u"], so["v"], so["h"], so["uh"], so["vh"], so["uhtr"], so["vhtr"], so["eta_av"], inp["taux"], inp["tauy"], dt,
               inp["coefs"], calc_dtbt=(n == 0))

    # ---------------- device: mom6x_set_viscous_BBL before each step
    cont2, bt2, cor2, pgf2, rk22 = cases.rk2_params(d, GV, bt_mod)
    dyc = Dycore(d, M, GV, 0)
    try:
        dyc.continuity_init(cont2); dyc.barotropic_init(bt2); dyc.CoriolisAdv_init(cor2); dyc.PressureForce_init(pgf2, Rlay, gp)
        dyc.initialize_dyn_split_RK2(rk22)
        Td, Sd = dyc.to_dev(T), dyc.to_dev(S)
        dyc.PressureForce_set_tv(Td, Sd, eos)
        dyc.vertvisc_init(vv)
        dvis = {n: dyc.zeros2() for n in names}
        dyc.vertvisc_set_visc(*(dvis[n] for n in names))
        dyc.set_visc_init(sv, eos)
        sg = dict(u=dyc.to_dev(inp["u"]), v=dyc.to_dev(inp["v"]), h=dyc.to_dev(inp["h"]), uh=dyc.zeros3(), vh=dyc.zeros3(),
                  uhtr=dyc.zeros3(), vhtr=dyc.zeros3(), eta_av=dyc.zeros2())
        txd, tyd = dyc.to_dev(inp["taux"]), dyc.to_dev(inp["tauy"])
        torch.cuda.synchronize()
        dyc.set_viscous_BBL(sg["u"], sg["v"], sg["h"], T=Td, S=Sd, **dvis)
        dyc.dyn_split_RK2_new_run(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], dt)
        for n in range(nsteps):
            dyc.set_viscous_BBL(sg["u"], sg["v"], sg["h"], T=Td, S=Sd, **dvis)
            dyc.sync()
            for k in names:
                H.assert_bitwise(dvis[k].cpu().numpy(), ohist[n][k], f"step {n}: {k}", H.interior(d, k[-1]))
            dyc.step_MOM_dyn_split_RK2(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], sg["uhtr"], sg["vhtr"], sg["eta_av"], txd, tyd,
                                       dt, calc_dtbt=(n == 0))
        dyc.sync()
        for n, st in (("u", "u"), ("v", "v"), ("h", "h"), ("uh", "u"), ("vh", "v")):
            H.assert_bitwise(sg[n].cpu().numpy(), so[n], f"{sums}: {n}", H.interior(d, st))
    finally:
        dyc.close()
    sl = H.interior(d, "u")
    assert not np.array_equal(ohist[0]["Kv_bbl_u"][sl], ohist[-1]["Kv_bbl_u"][sl]), "Kv_bbl_u did not change between steps"
    assert np.abs(so["u"]).max() > 0
