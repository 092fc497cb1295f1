"""mom6x_set_BBL_TKE and mom6x_set_diffusivity on the device (mom6_amd/csrc/set_diffusivity.hip) against the restatement
tests/setdiff_ref.py, bit for bit and on whole arrays with no tolerated signed zero.  Every output starts as NaN, so the points the
reference leaves alone are checked too, and the arrays the reference fills as a whole (Kd_int, Kd_lay, Kd_extra_T, Kd_extra_S,
Kv_slow, Kv_shear) must carry their fill in the halo.  Every exp-free case on a bowl and on a basin with an island at 2, 3, 4 and
8 layers, one OM4-like case at 75; the sites of exp, sin, log and tanh held to the project's bound for its transcendental sites;
-0 planted; launch edges; 2 x 2 tiles as host threads with the exchange counter; inputs only read and no state between calls;
refusals and error paths; the chain from mom6x_set_viscous_BBL to mom6x_triDiagTS_Eulerian on device pointers."""
import functools
import json
import os
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import setdiff_ref as R
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
INPUT_ONLY = ("u", "v", "h", "T", "S", "p_surf", "tv_p_surf", "Kd_shear", "ustar_tidal", "BBL_tidal_dis", "Ray_u", "Ray_v") + R.VISC
FILLED = ("Kd_int", "Kd_lay", "Kd_extra_T", "Kd_extra_S", "Kv_slow", "Kv_shear")
CONFIGS = (("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 8), ("island_basin", 4))


def _grid(grid, nk, layout=(1, 1), pe=(0, 0)):
    gg, d, M = getattr(H, grid)(nk=nk, layout=layout, pe=pe)
    return d, M, R.geoLatT(d, gg)


def _device(d, M, GV, P, eos, opt, inp, lat, fill=np.nan, ncalls=1, layout=None, pe=None, uid=None):
    """One mom6x_set_diffusivity_init, then `ncalls` times mom6x_set_BBL_TKE and mom6x_set_diffusivity on device arrays, the
    second reading the planes of the first; every output starts as `fill` (before the first call only).  Returns the outputs, the
    module's Kd_sfc plane and the exchanges made."""
    import torch
    from mom6_amd import parallel
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        if layout is not None:
            parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
        t = {n: dy.to_dev(inp[n]) for n in INPUT_ONLY}
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, P, opt, fill).items()}
        dy.set_diffusivity_init(P, eos, None if eos is not None else abi.layer_densities(d.nk)[0], lat if opt["lat"] else None)
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        for _ in range(ncalls):
            dy.set_BBL_TKE(t["u"], t["v"], t["h"], *[t[n] for n in R.VISC], *[out[n] for n in R.BBL_OUT])
            dy.set_diffusivity(t["h"], opt["dt"], out["Kd_int"], u=t["u"], v=t["v"], T=t["T"], S=t["S"], ustar_BBL=out["ustar_BBL"],
                               BBL_meanKE_loss=out["BBL_meanKE_loss"], **{n: t[n] for n in opt["given"]},
                               **{n: out[n] for n in opt["out"]})
        nex = dy.comm_exchange_count()
        dy.sync()
        for n in t:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        got = {n: a.cpu().numpy() for n, a in out.items()}
        return got, dy.set_diffusivity_field("Kd_sfc").cpu().numpy().copy(), nex
    finally:
        dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name):
    """The restatement's result of an exp-free case on a grid, computed once and shared by the tests below (read only)."""
    d, M0, lat = _grid(grid, nk)
    GV = abi.vgrid_default()
    P, eos, opt = R.case(name, GV)
    M = R.metrics(M0, opt["f0"])
    inp = R.inputs(d, M, GV, **opt["inp"])
    want, counts = R.run(d, M, GV, P, eos, opt, inp, lat=lat)
    return d, M, lat, GV, P, eos, opt, inp, want, counts


def _check(d, P, opt, got, want, tag):
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], f"{tag}: {n}")
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    for n in FILLED:                                            # the fills of :369-374, :452-453 reach the halo
        if n in got and not (n == "Kv_shear" and P.use_Kd_shear):
            fill = {"Kd_int": P.Kd, "Kd_lay": P.Kd, "Kv_slow": P.Kv}.get(n, 0.0)
            assert (got[n][:, halo] == fill).all(), (tag, n)
    for n in ("N2_3d", "Kd_bkgnd", "Kv_bkgnd", "KT_extra", "KS_extra", "Kd_BBL") + R.BBL_OUT:   # diagnostics and planes: NaN outside
        if n in got:
            assert np.isnan(got[n][..., halo]).all(), (tag, n)
            lev = slice(1, d.nk) if n == "Kd_BBL" else slice(None)
            if n != "Kd_BBL" or (P.bottomdraglaw and P.BBL_effic > 0.0):
                assert np.isfinite(got[n][..., ~halo][lev] if got[n].ndim == 3 else got[n][~halo]).all(), (tag, n)
    assert np.isfinite(got["Kd_int"]).all()


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_parity_with_the_restatement(grid, nk):
    """Every exp-free case, whole arrays bit for bit; set_BBL_TKE's planes come from the device's own call, also where it takes
    the early return."""
    for name in R.CASES_EXP_FREE:
        d, M, lat, GV, P, eos, opt, inp, want, _ = _want(grid, nk, name)
        got, _, nex = _device(d, M, GV, P, eos, opt, inp, lat)
        _check(d, P, opt, got, want, f"{grid}/{nk}/{name}")
        assert nex == 0


def test_the_branches_of_the_cpu_list_are_reached_by_what_ran():
    """The restatement's counters over the cases and grids of test_parity_with_the_restatement against the list of
    tests/test_set_diffusivity_cpu.py, less the arms that only a case with an exp reaches."""
    from tests.test_set_diffusivity_cpu import REQUIRED, ONLY_WITH_EXP
    tot = dict.fromkeys(R.BRANCHES, 0)
    for grid, nk in CONFIGS:
        for name in R.CASES_EXP_FREE:
            for k, v in _want(grid, nk, name)[-1].items():
                tot[k] += v
    print("branch counts", tot)
    assert tot["exp"] == 0
    for k in REQUIRED:
        if k not in ONLY_WITH_EXP:
            assert tot[k] > 0, (k, tot)


def test_om4_case_at_75_layers():
    """EOS WRIGHT, the law of the wall, the floors and double diffusion's salt-finger arm at the headline's layer count."""
    d, M, lat, GV, P, eos, opt, inp, want, counts = _want("benchmark_small", 75, "om4")
    assert counts["salt_finger"] > 0 and counts["lotw_limited"] > 0 and counts["floor_int_fired"] > 0 and counts["exp"] == 0
    got, _, _ = _device(d, M, GV, P, eos, opt, inp, lat)
    _check(d, P, opt, got, want, "benchmark_small/75/om4")


def test_exp_sites_are_held_to_a_tolerance():
    """exp in the law of the wall's decay with f /= 0 and in the diffusive-convection arm, sin and log in the Henyey plane, tanh
    in the tanh-of-latitude plane: the device's functions and numpy's may differ in the last bit, so every field is held to 1e-12
    of its range (the bound of tests/test_barotropic_gpu.py and of test_MEKE_gpu.py::test_pow_cases_are_held_to_a_tolerance).
    With the library's own Kd_sfc plane handed to the restatement, the Henyey and tanh cases are bit for bit.  The largest
    differences are recorded in profiles/set_diffusivity_exp.json (MOM6X_RECORD_SET_DIFFUSIVITY_EXP names the file)."""
    GV = abi.vgrid_default()
    worst = {}
    for name in R.CASES_EXP:
        P, eos, opt = R.case(name, GV)
        d, M0, lat = _grid("benchmark_small", 8)
        M = R.metrics(M0, opt["f0"])
        inp = R.inputs(d, M, GV, **opt["inp"])
        want, counts = R.run(d, M, GV, P, eos, opt, inp, lat=lat)
        got, Kd_sfc, _ = _device(d, M, GV, P, eos, opt, inp, lat)
        if opt["lat"]:
            got["Kd_sfc"], want["Kd_sfc"] = Kd_sfc, R.Kd_sfc_plane(d, P, lat)
            assert np.ptp(want["Kd_sfc"][H.interior(d, "h")]) > 0.1 * P.Kd
            fed, _ = R.run(d, M, GV, P, eos, opt, inp, Kd_sfc=Kd_sfc)
            for n in fed:
                _bits(got[n], fed[n], f"{name} with the library's Kd_sfc: {n}")
        else:
            assert counts["exp"] > 0
        assert set(got) == set(want)
        for n in want:
            ok = np.isfinite(want[n])
            assert np.array_equal(np.isfinite(got[n]), ok), (name, n)
            rng = want[n][ok].max() - want[n][ok].min()
            if rng > 0.0:
                worst[f"{name}:{n}"] = float(np.abs(got[n][ok] - want[n][ok]).max() / rng)
            else:
                _bits(got[n], want[n], f"{name}: {n}")
    print("exp sites: largest difference / range:", worst)
    if os.environ.get("MOM6X_RECORD_SET_DIFFUSIVITY_EXP"):
        json.dump(dict(case="benchmark_small x 8, tests/setdiff_ref.py CASES_EXP", largest_difference_over_range=worst, bound=1.0e-12),
                  open(os.environ["MOM6X_RECORD_SET_DIFFUSIVITY_EXP"], "w"), indent=1)
    for n, v in worst.items():
        assert v <= 1.0e-12, (n, v)


def test_set_BBL_TKE_with_negative_zero_planted():
    """-0 over a block of u (uhtot = 0 + hvel*(-0) stays +0, u2_bbl = 0) and in bbl_thick_u, where cdrag_sqrt*(-0) > 0 is false and
    the face gives neither ustar nor u2_bbl (the inputs carry that patch already); the early return is in every case of
    test_parity_with_the_restatement that has no bottom-drag mixing."""
    d, M, lat, GV, P, eos, opt, inp, _, _ = _want("island_basin", 4, "lotw")
    inp = {n: a.copy() for n, a in inp.items()}
    inp["u"][(slice(None),) + d.sl(8, 16, 4, 12)] = -0.0
    inp["bbl_thick_u"][d.sl(24, 28, 18, 22)] = -0.0
    assert np.signbit(inp["bbl_thick_u"]).any()
    want, _ = R.run(d, M, GV, P, eos, opt, inp, lat=lat)
    got, _, _ = _device(d, M, GV, P, eos, opt, inp, lat)
    for n in want:
        _bits(got[n], want[n], "planted: " + n)
    z = got["BBL_meanKE_loss"][H.interior(d, "h")]
    assert (z == 0.0).any() and (z > 0.0).any()
    Pz, _, optz = R.case("no_drag", GV)
    gotz, _, _ = _device(d, M, GV, Pz, abi.eos_params_default(abi.LINEAR), optz, inp, lat)
    for n in R.BBL_OUT:
        assert (gotz[n][H.interior(d, "h")] == 0.0).all() and not np.signbit(gotz[n][H.interior(d, "h")]).any(), n


def test_reentrant_tile_one_lane_wider_and_one_row_taller_than_a_work_group():
    """A land-free doubly re-entrant tile of the work-group's width and one more, its height and one more, two layers: the last
    lane and the last row are blocks of their own, and k > 2 is never true."""
    from tests.test_dyn_edges_cpu import torus
    bx, by, _ = abi.lane_launch_shape()
    GV = abi.vgrid_default()
    d, M0 = torus(bx + 1, by + 1, nk=2)[1:]
    lat = R.geoLatT(d)
    for name in ("om4", "lotw_ray", "shear", "ramp"):
        P, eos, opt = R.case(name, GV)
        M = R.metrics(M0, opt["f0"])
        inp = R.inputs(d, M, GV, **opt["inp"])
        want, counts = R.run(d, M, GV, P, eos, opt, inp, lat=lat)
        assert counts["n2_nk2"] == d.ni * d.nj
        got, _, _ = _device(d, M, GV, P, eos, opt, inp, lat)
        _check(d, P, opt, got, want, "torus/" + name)


def test_two_by_two_tiles_as_host_threads_exchange_nothing():
    """The four tiles of a 2 x 2 layout as host threads on one GPU (tests/transport), each on its cut of the inputs, equal the
    one-tile run on their own points; neither call exchanges anything."""
    from mom6_amd import parallel
    lib = abi.load_library()
    layout = (2, 2)
    for name in ("om4", "lotw_ray"):
        d, M, lat, GV, P, eos, opt, inp, _, _ = _want("benchmark_small", 8, name)
        one, _, _ = _device(d, M, GV, P, eos, opt, inp, lat)
        H.use_threads_transport(lib)
        try:
            uid = parallel.unique_id(lib)
            out, errors = {}, []

            def tile(pe):
                try:
                    dt_, Mt0, latt = _grid("benchmark_small", 8, layout=layout, pe=pe)
                    Mt = R.metrics(Mt0, opt["f0"])
                    tin = R.inputs(dt_, Mt, GV, **opt["inp"])
                    out[pe] = (dt_,) + _device(dt_, Mt, GV, P, eos, opt, tin, latt, layout=layout, pe=pe, uid=uid)
                except Exception:                                       # noqa: BLE001 -- reported by the main thread
                    import traceback
                    errors.append((pe, traceback.format_exc()))
            pes = [(px, py) for py in range(layout[1]) for px in range(layout[0])]
            threads = [threading.Thread(target=tile, args=(pe,)) for pe in pes]
            for th in threads:
                th.start()
            for th in threads:
                th.join(timeout=120)
        finally:
            H.use_threads_transport(lib, on=False)
        assert not errors, errors[0][1]
        assert len(out) == len(pes)
        for pe in pes:
            dt_, got, _, nex = out[pe]
            assert nex == 0, (name, pe, nex)
            own = H.interior(dt_, "h")
            part = d.sl(dt_.i_glob0, dt_.i_glob0 + dt_.ni - 1, dt_.j_glob0, dt_.j_glob0 + dt_.nj - 1)
            for n in one:
                _bits(np.ascontiguousarray(got[n][(Ellipsis,) + own]), np.ascontiguousarray(one[n][(Ellipsis,) + part]),
                      f"{name} tile {pe}: {n}")


def test_two_consecutive_calls_give_the_same_bits():
    """The work arrays carry no state: a second pair of calls on the same arrays leaves every bit where the first put it
    (the inputs are compared after the calls in every test of this file)."""
    for name in ("om4", "shear"):
        d, M, lat, GV, P, eos, opt, inp, want, _ = _want("island_basin", 4, name)
        got, _, _ = _device(d, M, GV, P, eos, opt, inp, lat, ncalls=2)
        for n in want:
            _bits(got[n], want[n], f"second call/{name}: {n}")


def test_refused_settings_and_error_paths():
    """Each `must be 0` member and bottom-drag mixing without the law of the wall are refused at init with a message naming the
    setting; the law of the wall without KD_MAX, DOUBLE_DIFFUSION without an EOS or without both Kd_extra arrays, a latitude
    function without geoLatT and a call before init are errors; the outputs stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M, lat = _grid("benchmark_small", 4)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    eos = abi.eos_params_default(abi.WRIGHT)
    dflt = abi.set_diffusivity_params_default
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(inp[n]) for n in ("u", "v", "h", "T", "S") + R.VISC}
        Kd_int = dy.to_dev(np.full(d.shape3(d.nk + 1), np.nan))
        Kd_lay = dy.to_dev(np.full(d.shape3(), np.nan))
        KeT = dy.to_dev(np.full(d.shape3(d.nk + 1), np.nan))
        planes = [dy.to_dev(np.full(d.shape2(), np.nan)) for _ in range(2)]
        torch.cuda.synchronize()
        with pytest.raises(Exception, match="initialized"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"])
        with pytest.raises(Exception, match="initialized"):
            dy.set_BBL_TKE(t["u"], t["v"], t["h"], *[t[n] for n in R.VISC], *planes)
        words = dict(ML_radiation="ML_RADIATION", use_tidal_mixing="INT_TIDE_DISSIPATION", use_int_tides="INTERNAL_TIDES",
                     use_CVMix_ddiff="USE_CVMIX_DDIFF", Bryan_Lewis_diffusivity="BRYAN_LEWIS_DIFFUSIVITY",
                     horiz_varying_background="HORIZ_VARYING_BACKGROUND", user_change_diff="USER_CHANGE_DIFFUSIVITY",
                     nkml="bulk mixed layer", SpV_avg="SpV_avg", open_bcs="open boundary")
        assert set(words) == set(abi.SET_DIFFUSIVITY_MUST_BE_0)
        for member, word in words.items():
            with pytest.raises(Exception, match="error 3.*" + word):
                dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, **{member: 1}), eos)
        with pytest.raises(Exception, match="error 3.*USE_LOTW_BBL_DIFFUSIVITY"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, BBL_effic=0.2), eos)
        with pytest.raises(Exception, match="KD_MAX"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, BBL_effic=0.2, use_LOTW_BBL_diffusivity=1), eos)
        with pytest.raises(Exception, match="DOUBLE_DIFFUSION"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, double_diffusion=1), None, abi.layer_densities(d.nk)[0])
        with pytest.raises(Exception, match="geoLatT"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, Henyey_IGW_background=1), eos)
        with pytest.raises(Exception, match="geoLatT"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, Kd_tanh_lat_fn=1), eos)
        with pytest.raises(Exception, match="Rlay"):
            dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5), None)
        with pytest.raises(Exception, match="initialized"):       # a refused init leaves no module behind
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"])
        dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, double_diffusion=1), eos)
        with pytest.raises(Exception, match="Kd_extra_T and Kd_extra_S"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"], Kd_lay=Kd_lay)
        with pytest.raises(Exception, match="Kd_extra_T and Kd_extra_S"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"], Kd_extra_T=KeT)
        with pytest.raises(Exception, match="tv%T"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, Kd_extra_T=KeT, Kd_extra_S=KeT)
        dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, use_Kd_shear=1), eos)
        with pytest.raises(Exception, match="Kd_shear"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"])
        dy.set_diffusivity_init(dflt(GV, Kd=1.0e-5, BBL_effic=0.2, use_LOTW_BBL_diffusivity=1, Kd_max=1.0e-2), eos)
        with pytest.raises(Exception, match="ustar_BBL"):
            dy.set_diffusivity(t["h"], 3600.0, Kd_int, T=t["T"], S=t["S"])
        with pytest.raises(Exception, match="bbl_thick"):
            dy.set_BBL_TKE(t["u"], t["v"], t["h"], None, None, None, None, *planes)
        dy.sync()
        for a in (Kd_int, Kd_lay, KeT, *planes):
            assert torch.isnan(a).all()
    finally:
        dy.close()


def test_chain_from_set_viscous_BBL_to_triDiagTS_Eulerian(orc):
    """benchmark_small x 8, WRIGHT: mom6x_set_viscous_BBL -> mom6x_set_BBL_TKE -> mom6x_set_diffusivity -> ent =
    dt*Kd_int/(0.5*(dz(k-1) + dz(k)) + dz_neglect) with torch ops on the context's stream -> mom6x_triDiagTS_Eulerian, all on
    device pointers with no host copy in between; against tests/setvisc_ref.py, tests/setdiff_ref.py, the same ent in numpy and
    the oracle's solve, bit for bit."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import setvisc_ref
    d, M0, lat = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    P, eos, opt = R.case("om4", GV)
    M = R.metrics(M0, opt["f0"])
    sv_in = setvisc_ref.inputs(d, M, GV)
    inp = dict(R.inputs(d, M, GV, **opt["inp"]), u=sv_in["u"], v=sv_in["v"])
    Psv = setvisc_ref.switch_case("eos", form=abi.WRIGHT)[0]
    dt = opt["dt"]
    nz = d.nk
    # the restatements in sequence
    visc = {n: np.full(d.shape2(), np.nan) for n in R.VISC}
    setvisc_ref.set_viscous_BBL(d, M, GV, Psv, inp["u"], inp["v"], inp["h"], T=inp["T"], S=inp["S"], eos=eos, orc=orc, **visc)
    want, _ = R.run(d, M, GV, P, eos, opt, dict(inp, **visc), lat=lat, orc=orc)

    def ent_of(Kd_int, h, xp):
        ent = xp.zeros_like(Kd_int)
        dz = GV.H_to_Z * h
        ent[1:nz] = dt * Kd_int[1:nz] / (0.5 * (dz[:nz - 1] + dz[1:nz]) + GV.dZ_subroundoff)
        return ent
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    ent_w = np.where(own, ent_of(want["Kd_int"], inp["h"], np), 0.0)
    Tw, Sw = inp["T"].copy(), inp["S"].copy()
    orc.triDiagTS_Eulerian(d, inp["h"], np.ascontiguousarray(ent_w), Tw, GV.H_subroundoff)
    orc.triDiagTS_Eulerian(d, inp["h"], np.ascontiguousarray(ent_w), Sw, GV.H_subroundoff)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(inp[n]) for n in ("u", "v", "h", "T", "S")}
        for n in R.VISC:
            t[n] = dy.to_dev(np.full(d.shape2(), np.nan))
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, P, opt).items()}
        own_d = dy.to_dev(own.astype(np.float64)) > 0.5
        dy.set_visc_init(Psv, eos)
        dy.set_diffusivity_init(P, eos)
        torch.cuda.synchronize()
        dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], **{n: t[n] for n in R.VISC})
        dy.set_BBL_TKE(t["u"], t["v"], t["h"], *[t[n] for n in R.VISC], *[out[n] for n in R.BBL_OUT])
        dy.set_diffusivity(t["h"], dt, out["Kd_int"], T=t["T"], S=t["S"], ustar_BBL=out["ustar_BBL"],
                           BBL_meanKE_loss=out["BBL_meanKE_loss"], **{n: out[n] for n in opt["out"]})
        with torch.cuda.stream(dy.torch_stream()):
            ent = torch.where(own_d, ent_of(out["Kd_int"], t["h"], torch), torch.zeros_like(out["Kd_int"])).contiguous()
        dy.triDiagTS_Eulerian(t["h"], ent, t["T"], t["S"])
        dy.sync()
        for n in R.VISC:
            _bits(t[n].cpu().numpy(), visc[n], "chain: " + n)
        for n in want:
            _bits(out[n].cpu().numpy(), want[n], "chain: " + n)
        _bits(ent.cpu().numpy(), ent_w, "chain: ent")
        sl = H.interior(d, "h")
        H.assert_bitwise(t["T"].cpu().numpy(), Tw, "chain: T", sl)
        H.assert_bitwise(t["S"].cpu().numpy(), Sw, "chain: S", sl)
        assert not np.array_equal(Tw[(slice(None),) + sl], inp["T"][(slice(None),) + sl])
    finally:
        dy.close()
