"""mom6x_applyBoundaryFluxesInOut on the device (mom6_amd/csrc/diabatic_aux.hip) against the restatement tests/bflux_ref.py, bit
for bit and on whole arrays with no tolerated signed zero.  Every output starts as NaN and the halos of h, T and S are NaN, so the
points the reference leaves alone are checked too; cTKE and SkinBuoyFlux, which the reference fills as a whole, must carry 0 in the
halo.  Every exp-free case on a bowl at 1, 2, 3 and 8 layers and on a basin with an island at 4, one OM4-like case at 75; the exp
cases held to the project's bound for its transcendental sites; launch edges; -0 planted; land columns; inputs only read; two
calls in a row; 2 x 2 tiles as host threads with the exchange counter; the status counts; refusals and error paths; the chain
from mom6x_set_diffusivity to mom6x_triDiagTS_Eulerian on device pointers."""
import functools
import json
import os
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import bflux_ref as R
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 8), ("island_basin", 4))


def _grid(grid, nk, layout=(1, 1), pe=(0, 0)):
    return getattr(H, grid)(nk=nk, layout=layout, pe=pe)[1:]


def _nan_halo(d, inp):
    """The inputs with NaN in the halos of h, T and S: nothing outside the computational domain may be read or written."""
    inp = dict(inp)
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    for n in ("h", "T", "S"):
        inp[n] = np.where(own[None], inp[n], np.nan)
    return inp


def _device(d, M, GV, P, eos, opt, inp, fill=np.nan, ncalls=1, layout=None, pe=None, uid=None, forcing=True):
    """One mom6x_diabatic_aux_init, then `ncalls` times mom6x_applyBoundaryFluxesInOut on the same device arrays; every output
    starts as `fill`.  Returns the state as tests/bflux_ref.py run() does, the status counts and the exchanges made; the inputs
    are compared with what was uploaded."""
    import torch
    from mom6_amd import parallel
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        if layout is not None:
            parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
        st = {n: dy.to_dev(inp[n]) for n in ("h", "T", "S")}
        ro = {n: dy.to_dev(inp[n]) for n in ("opacity_band", "sw_pen_band", "tv_p_surf") if inp[n] is not None}
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, opt, fill).items()}
        fh = R.flux_planes(d, opt, inp, fill, forcing)
        f = {n: dy.to_dev(a) for n, a in fh.items()} if fh is not None else None
        dy.diabatic_aux_init(P, eos)
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        for _ in range(ncalls):
            dy.applyBoundaryFluxesInOut(opt["dt"], f, st["h"], st["T"], st["S"], nsw=opt["nsw"], opacity_band=ro.get("opacity_band"),
                                        sw_pen_band=ro.get("sw_pen_band"), tv_p_surf=ro["tv_p_surf"] if opt["p_surf"] else None,
                                        aggregate_FW_forcing=opt["agg"], evap_CFL_limit=opt["cfl"],
                                        minimum_forcing_depth=opt["depth"], **out)
        nex = dy.comm_exchange_count()
        status = dy.diabatic_aux_status()
        assert dy.diabatic_aux_status() == (0, 0, 0)            # the counts are since the last status call
        for n in ro:
            _bits(ro[n].cpu().numpy(), inp[n], n + " is only read")
        if f is not None:
            for n in fh:
                if n not in opt["fout"]:
                    _bits(f[n].cpu().numpy(), fh[n], "fluxes%" + n + " is only read")
        got = {n: a.cpu().numpy() for n, a in st.items()}
        got.update({n: a.cpu().numpy() for n, a in out.items()})
        if f is not None:
            got.update({"fluxes." + n: f[n].cpu().numpy() for n in opt["fout"]})
        return got, status, nex
    finally:
        dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, ncalls=1):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    d, M = _grid(grid, nk)
    GV = abi.vgrid_default()
    P, eos, opt = R.case(name, GV)
    inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
    want, status, counts = R.run(d, M, GV, P, eos, opt, inp, ncalls=ncalls)
    return d, M, GV, P, eos, opt, inp, want, status, counts


def _check(d, opt, got, want, tag):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for n in want:
        _bits(got[n], want[n], f"{tag}: {n}")
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    for n in ("h", "T", "S", "dSV_dT", "dSV_dS", "createdH", "penSW_diag", "penSWflux_diag", "nonpenSW_diag"):
        if n in got:
            assert np.isnan(got[n][..., halo]).all(), (tag, n)
            assert np.isfinite(got[n][..., ~halo]).all(), (tag, n)
    for n in ("cTKE", "SkinBuoyFlux"):                          # the fills of :808-809 reach the halo
        if n in got:
            assert (got[n][..., halo] == 0.0).all() and not np.signbit(got[n][..., halo]).any(), (tag, n)
            assert np.isfinite(got[n]).all(), (tag, n)
    for n in got:
        if n.startswith("fluxes.") and n != "fluxes.TempxPmE":
            assert np.isnan(got[n][halo]).all() and np.isfinite(got[n][~halo]).all(), (tag, n)


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_parity_with_the_restatement(grid, nk):
    """Every exp-free case, whole arrays bit for bit, and the three counts.  At nk = 1 steps A, B, C and the redistribution from
    the bottom all act on one layer."""
    for name in R.CASES_EXP_FREE:
        d, M, GV, P, eos, opt, inp, want, status, counts = _want(grid, nk, name)
        assert counts["exp"] == 0, (name, counts["exp"])
        got, st, nex = _device(d, M, GV, P, eos, opt, inp)
        _check(d, opt, got, want, f"{grid}/{nk}/{name}")
        assert st == status, (name, st, status)
        assert nex == 0


def test_the_branches_of_the_cpu_list_are_reached_by_what_ran():
    """The restatement's counters over the cases and grids of test_parity_with_the_restatement against the list of
    tests/test_diabatic_aux_cpu.py, less the arms that only a case with an exp reaches."""
    from tests.test_diabatic_aux_cpu import REQUIRED, ONLY_WITH_EXP
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
    """EOS WRIGHT, three bands, the energetics, SkinBuoyFlux and every diagnostic at the headline's layer count, exp-free."""
    d, M, GV, P, eos, opt, inp, want, status, counts = _want("benchmark_small", 75, "wright_3")
    assert counts["exp"] == 0 and counts["tke_large_od"] > 0 and counts["bottom_all"] > 0 and counts["a_energetics"] > 0
    got, st, _ = _device(d, M, GV, P, eos, opt, inp)
    _check(d, opt, got, want, "benchmark_small/75/wright_3")
    assert st == status


def test_exp_sites_are_held_to_a_tolerance():
    """Realistic opacities (0.05 .. 3 m-1): the device's exp and numpy's may differ in the last bit, so every field is held to
    1e-12 of its range (the bound of tests/test_barotropic_gpu.py, test_MEKE_gpu.py and test_set_diffusivity_gpu.py for a
    transcendental site).  The largest differences are recorded in profiles/diabatic_aux_exp.json
    (MOM6X_RECORD_DIABATIC_AUX_EXP names the file)."""
    worst = {}
    for name in R.CASES_EXP:
        d, M, GV, P, eos, opt, inp, want, status, counts = _want("benchmark_small", 8, name)
        assert counts["exp"] > 0
        got, st, _ = _device(d, M, GV, P, eos, opt, inp)
        assert st == status and set(got) == set(want)
        for n in want:
            ok = np.isfinite(want[n])
            assert np.array_equal(np.isfinite(got[n]), ok), (name, n)
            rng = want[n][ok].max() - want[n][ok].min()
            if rng > 0.0:
                worst[f"{name}:{n}"] = float(np.abs(got[n][ok] - want[n][ok]).max() / rng)
            else:
                _bits(got[n], want[n], f"{name}: {n}")
    print("exp sites: largest difference / range:", worst)
    if os.environ.get("MOM6X_RECORD_DIABATIC_AUX_EXP"):
        json.dump(dict(case="benchmark_small x 8, tests/bflux_ref.py CASES_EXP", largest_difference_over_range=worst, bound=1.0e-12),
                  open(os.environ["MOM6X_RECORD_DIABATIC_AUX_EXP"], "w"), indent=1)
    for n, v in worst.items():
        assert v <= 1.0e-12, (n, v)


def _edge_shapes():
    bx, by, _ = abi.lane_launch_shape()
    return [(bx, by), (bx + 1, by + 1), (2 * bx + 1, by), (1, by + 1)]


@pytest.mark.parametrize("ni,nj", _edge_shapes())
def test_launch_extents(ni, nj):
    """Land-free doubly re-entrant tiles whose extents are a whole number of work-groups and one more (a last work-group with one
    live lane, a last row of its own) and a tile one cell wide, three layers."""
    d, M = H.torus(nk=3, ni=ni, nj=nj)[1:]
    GV = abi.vgrid_default()
    for name in ("wright_3", "wright_full_4", "no_eos_old"):
        P, eos, opt = R.case(name, GV)
        inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
        want, status, _ = R.run(d, M, GV, P, eos, opt, inp)
        got, st, _ = _device(d, M, GV, P, eos, opt, inp)
        _check(d, opt, got, want, f"torus {ni}x{nj}/{name}")
        assert st == status


def test_upward_sweep_in_one_lane_of_a_wavefront_and_in_none():
    """Opaque water everywhere: no lane has shortwave left at the bottom and every wavefront skips the upward loop.  Then one
    column of clear water: exactly one lane of one wavefront takes it."""
    d, M = H.torus(nk=4, ni=40, nj=6)[1:]
    GV = abi.vgrid_default()
    P, eos, opt = R.case("linear_e", GV)
    assert opt["opacity"] == "huge"
    base = _nan_halo(d, R.case_inputs(d, M, GV, opt, thin=False, dry=False, ground=False))
    for clear, n_up in ((None, 0), ((17, 3), 1)):
        inp = dict(base, opacity_band=base["opacity_band"].copy())
        if clear:
            inp["opacity_band"][(Ellipsis,) + d.sl(clear[0], clear[0], clear[1], clear[1])] = 0.0
        want, status, counts = R.run(d, M, GV, P, eos, opt, inp)
        assert counts["bottom_all"] + counts["bottom_limited"] == n_up and counts["tchg_full"] == n_up * d.nk
        got, st, _ = _device(d, M, GV, P, eos, opt, inp)
        _check(d, opt, got, want, f"upward sweep in {n_up} lanes")


def test_negative_zero_planted():
    """-0 over blocks of evap, sw_pen_band and T: no zero of opposite sign anywhere (the comparisons are on bit patterns)."""
    d, M, GV, P, eos, opt, inp, _, _, _ = _want("island_basin", 4, "wright_3")
    inp = dict(inp, T=inp["T"].copy(), sw_pen_band=inp["sw_pen_band"].copy(), fluxes=dict(inp["fluxes"]))
    inp["fluxes"]["evap"] = inp["fluxes"]["evap"].copy()
    inp["fluxes"]["evap"][d.sl(4, 12, 4, 10)] = -0.0
    inp["sw_pen_band"][(slice(None),) + d.sl(8, 16, 6, 14)] = -0.0
    inp["T"][(slice(None),) + d.sl(10, 20, 8, 16)] = -0.0
    for n in ("lprec", "fprec", "vprec", "lrunoff", "frunoff", "lrunoff_glc", "frunoff_glc", "seaice_melt"):
        inp["fluxes"][n] = inp["fluxes"][n].copy()
        inp["fluxes"][n][d.sl(4, 8, 4, 8)] = 0.0                  # with them netMassInOut is +0 or -0 there
    want, status, _ = R.run(d, M, GV, P, eos, opt, inp)
    assert any(np.signbit(a[np.isfinite(a) & (a == 0.0)]).any() for a in want.values())
    got, st, _ = _device(d, M, GV, P, eos, opt, inp)
    _check(d, opt, got, want, "planted")
    assert st == status


def test_land_columns_get_the_shortwave_step_only():
    """Fluxes and shortwave over land with IGNORE_FLUXES_OVER_LAND: a land column keeps h and S, gets no netMassIn | netMassOut
    and no step A or B, but its T takes absorbRemainingSW's heating and its derivatives are formed, as in the reference."""
    d, M, GV, P, eos, opt, inp, _, _, _ = _want("island_basin", 4, "land")
    inp = dict(inp, opacity_band=np.full_like(inp["opacity_band"], 1.0e16))   # opaque even to what step B leaves of a 1e-10 m layer
    want, status, counts = R.run(d, M, GV, P, eos, opt, inp)
    assert counts["land_flux"] > 0 and status[2] == 0 and counts["exp"] == 0
    got, st, _ = _device(d, M, GV, P, eos, opt, inp)
    _check(d, opt, got, want, "land")
    assert st == status
    land = np.zeros(d.shape2(), bool)
    land[H.interior(d, "h")] = True
    land &= ~(M[G["mask2dT"]] > 0.0)
    assert land.any()
    _bits(got["h"][:, land], inp["h"][:, land], "h over land")
    _bits(got["S"][:, land], inp["S"][:, land], "S over land")
    assert (got["T"][:, land] != inp["T"][:, land]).any()
    assert np.isfinite(got["dSV_dT"][:, land]).all()


def test_without_fluxes_only_the_fills_and_the_derivatives_are_made():
    """fluxes = NULL (.not.associated(fluxes%sw)): with energetics the derivatives and the fills, h, T, S untouched (:814, :900)."""
    d, M, GV, P, eos, opt, inp, _, _, _ = _want("benchmark_small", 3, "wright_3")
    want, status, _ = R.run(d, M, GV, P, eos, opt, inp, forcing=False)
    got, st, _ = _device(d, M, GV, P, eos, opt, inp, forcing=False)
    for n in want:
        _bits(got[n], want[n], "no fluxes: " + n)
    for n in ("h", "T", "S"):
        _bits(got[n], inp[n], "no fluxes: " + n + " untouched")
    assert (got["cTKE"] == 0.0).all() and (got["SkinBuoyFlux"] == 0.0).all() and np.isnan(got["createdH"]).all()
    assert st == status == (0, 0, 0)


def test_two_calls_in_a_row_equal_two_calls_of_the_restatement():
    """No state lives between calls; tv%TempxPmE accumulates over both (the caller zeroes it), heat_content_massin | massout are
    set anew by each."""
    for name in ("wright_3", "wright_full_4"):
        d, M, GV, P, eos, opt, inp, want, status, _ = _want("island_basin", 4, name, 2)
        one = _want("island_basin", 4, name)[7]
        assert not np.array_equal(want["fluxes.TempxPmE"], one["fluxes.TempxPmE"])
        got, st, _ = _device(d, M, GV, P, eos, opt, inp, ncalls=2)
        _check(d, opt, got, want, "two calls/" + name)
        assert st == status


def test_two_by_two_tiles_as_host_threads_exchange_nothing():
    """The four tiles of a 2 x 2 layout as host threads on one GPU (tests/transport), each on its cut of the inputs, equal the
    one-tile run on their own points; the call exchanges nothing."""
    from mom6_amd import parallel
    lib = abi.load_library()
    layout = (2, 2)
    name = "wright_3"
    d, M, GV, P, eos, opt, inp, want, _, _ = _want("benchmark_small", 8, name)
    H.use_threads_transport(lib)
    try:
        uid = parallel.unique_id(lib)
        out, errors = {}, []

        def tile(pe):
            try:
                dt_, Mt = _grid("benchmark_small", 8, layout=layout, pe=pe)
                tin = R.case_inputs(dt_, Mt, GV, opt)
                out[pe] = (dt_,) + _device(dt_, Mt, GV, P, eos, opt, tin, layout=layout, pe=pe, uid=uid)
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
        assert nex == 0, (pe, nex)
        own = H.interior(dt_, "h")
        part = d.sl(dt_.i_glob0, dt_.i_glob0 + dt_.ni - 1, dt_.j_glob0, dt_.j_glob0 + dt_.nj - 1)
        for n in want:
            _bits(np.ascontiguousarray(got[n][(Ellipsis,) + own]), np.ascontiguousarray(want[n][(Ellipsis,) + part]), f"tile {pe}: {n}")


def test_status_counts_groundings_and_fluxes_over_land():
    """Ordinary inputs that the reference answers with a warning or a message: the patch that evaporates more than its columns
    hold grounds in as many columns as the restatement says and fills createdH; fluxes over land are counted without
    IGNORE_FLUXES_OVER_LAND and not with it."""
    d, M = _grid("island_basin", 4)
    GV = abi.vgrid_default()
    P, eos, opt = R.case("split", GV)
    for ground in (False, True):
        inp = _nan_halo(d, R.case_inputs(d, M, GV, opt, ground=ground, dry=False))
        want, status, _ = R.run(d, M, GV, P, eos, opt, inp)
        got, st, _ = _device(d, M, GV, P, eos, opt, inp)
        _check(d, opt, got, want, f"ground={ground}")
        assert st == status and status[1] == 0
        k = int((want["createdH"][H.interior(d, "h")] != 0.0).sum())
        assert status[0] == k and (k > 0) == ground
    for ignore in (0, 1):
        P, eos, opt = R.case("land", GV)
        P.ignore_fluxes_over_land = ignore
        inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
        want, status, counts = R.run(d, M, GV, P, eos, opt, inp)
        got, st, _ = _device(d, M, GV, P, eos, opt, inp)
        _check(d, opt, got, want, f"ignore={ignore}")
        assert st == status and status[2] == (0 if ignore else counts["land_flux"]) and counts["land_flux"] > 0


def test_refused_settings_and_error_paths():
    """Each `must be 0` member is refused at init, more than four bands and the energetics under UNESCO, ROQUET_RHO or JACKETT_06
    at the call, each with a message naming the setting; a missing plane, missing optics arrays, energetics or SkinBuoyFlux
    without an equation of state, the heat-content switches without their planes and a call before init are errors; the arrays
    of the energetics stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = _grid("benchmark_small", 4)
    GV = abi.vgrid_default()
    P0, _, opt = R.case("wright_3", GV)
    inp = R.case_inputs(d, M, GV, dict(opt, nsw=4))
    dflt = abi.diabatic_aux_params_default
    eos = abi.eos_params_default(abi.WRIGHT)
    dy = Dycore(d, M, GV)
    try:
        st = {n: dy.to_dev(inp[n]) for n in ("h", "T", "S")}
        op, pen = dy.to_dev(inp["opacity_band"]), dy.to_dev(inp["sw_pen_band"])
        f = {n: dy.to_dev(inp["fluxes"][n]) for n in R.FLUX_REQUIRED}
        e3 = [dy.to_dev(np.full(d.shape3(), np.nan)) for _ in range(3)]
        skin = dy.to_dev(np.full(d.shape2(), np.nan))
        ener = dict(cTKE=e3[0], dSV_dT=e3[1], dSV_dS=e3[2])
        torch.cuda.synchronize()
        call = lambda fl=f, nsw=0, **kw: dy.applyBoundaryFluxesInOut(3600.0, fl, st["h"], st["T"], st["S"], nsw=nsw, **kw)
        with pytest.raises(Exception, match="initialized"):
            call()
        with pytest.raises(Exception, match="initialized"):
            dy.diabatic_aux_status()
        words = dict(do_brine_plume="DO_BRINE_PLUME", enthalpy_from_coupler="heat_content_evap", SpV_avg="SpV_avg", nkml="bulk mixed layer")
        assert set(words) == set(abi.DIABATIC_AUX_MUST_BE_0)
        for member, word in words.items():
            with pytest.raises(Exception, match="error 3.*" + word):
                dy.diabatic_aux_init(dflt(GV, **{member: 1}), eos)
        with pytest.raises(Exception, match="initialized"):       # a refused init leaves no module behind
            call()
        dy.diabatic_aux_init(dflt(GV), None)
        with pytest.raises(Exception, match="error 1.*cTKE.*equation of state"):
            call(**ener)
        with pytest.raises(Exception, match="error 1.*SkinBuoyFlux.*equation of state"):
            call(SkinBuoyFlux=skin)
        for form, word in ((abi.UNESCO, "UNESCO"), (abi.ROQUET_RHO, "ROQUET_RHO"), (abi.JACKETT06, "JACKETT_06")):
            dy.diabatic_aux_init(dflt(GV), abi.eos_params_default(form))
            with pytest.raises(Exception, match="error 3.*" + word):
                call(**ener)
            call(SkinBuoyFlux=skin)                                # without energetics every form is accepted
        dy.diabatic_aux_init(dflt(GV), eos)
        with pytest.raises(Exception, match="error 3.*more than 4 bands"):
            call(nsw=5, opacity_band=op, sw_pen_band=pen)
        with pytest.raises(Exception, match="error 1.*opacity_band"):
            call(nsw=2, sw_pen_band=pen)
        with pytest.raises(Exception, match="error 1.*opacity_band"):
            call(nsw=2, opacity_band=op)
        for n, word in (("lw", "lw"), ("evap", "evaporation"), ("fprec", "precipitation"), ("frunoff_glc", "frunoff_glc"),
                        ("seaice_melt", "seaice_melt")):
            with pytest.raises(Exception, match="error 1.*" + word):
                call(fl={m: a for m, a in f.items() if m != n})
        with pytest.raises(Exception, match="error 1.*penSW_diag"):
            call(penSWflux_diag=dy.to_dev(np.full(d.shape3(d.nk + 1), np.nan)))
        dy.diabatic_aux_init(dflt(GV, use_river_heat_content=1), eos)
        with pytest.raises(Exception, match="error 1.*USE_RIVER_HEAT_CONTENT"):
            call()
        dy.diabatic_aux_init(dflt(GV, use_calving_heat_content=1), eos)
        with pytest.raises(Exception, match="error 1.*USE_CALVING_HEAT_CONTENT"):
            call()
        dy.sync()
        for a in e3:
            assert torch.isnan(a).all()
    finally:
        dy.close()


def test_chain_from_set_diffusivity_to_triDiagTS_Eulerian(orc):
    """benchmark_small x 8, WRIGHT: mom6x_set_diffusivity -> mom6x_applyBoundaryFluxesInOut -> ent = dt*Kd_int/(0.5*(dz(k-1) +
    dz(k)) + dz_neglect) from the NEW thicknesses with torch ops on the context's stream -> mom6x_triDiagTS_Eulerian, all on device
    pointers with no host copy in between; against tests/setdiff_ref.py, tests/bflux_ref.py, the same ent in numpy and the
    oracle's solve, bit for bit."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import setdiff_ref
    d, M = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    Psd, eos, osd = setdiff_ref.case("dd_sf", GV)
    Pda, _, opt = R.case("wright_3", GV)
    inp = R.case_inputs(d, M, GV, opt, thin=False, dry=False, ground=False)
    sd_in = dict(setdiff_ref.inputs(d, M, GV, **osd["inp"]), h=inp["h"], T=inp["T"], S=inp["S"])
    dt = opt["dt"]
    nz = d.nk
    Kd_sfc = setdiff_ref.Kd_sfc_plane(d, Psd)
    sd_want, _ = setdiff_ref.run(d, M, GV, Psd, eos, osd, sd_in, Kd_sfc=Kd_sfc, orc=orc)
    want, status, _ = R.run(d, M, GV, Pda, eos, opt, inp, orc=orc)

    def ent_of(Kd_int, h, xp):
        ent = xp.zeros_like(Kd_int)
        dz = GV.H_to_Z * h
        ent[1:nz] = dt * Kd_int[1:nz] / (0.5 * (dz[:nz - 1] + dz[1:nz]) + GV.dZ_subroundoff)
        return ent
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    ent_w = np.where(own, ent_of(sd_want["Kd_int"], want["h"], np), 0.0)
    Tw, Sw = want["T"].copy(), want["S"].copy()
    orc.triDiagTS_Eulerian(d, want["h"], np.ascontiguousarray(ent_w), Tw, GV.H_subroundoff)
    orc.triDiagTS_Eulerian(d, want["h"], np.ascontiguousarray(ent_w), Sw, GV.H_subroundoff)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(sd_in[n]) for n in ("u", "v", "h", "T", "S") + tuple(osd["given"])}
        sd_out = {n: dy.to_dev(a) for n, a in setdiff_ref.outputs(d, Psd, osd).items()}
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, opt).items()}
        fh = R.flux_planes(d, opt, inp)
        f = {n: dy.to_dev(a) for n, a in fh.items()}
        op, pen = dy.to_dev(inp["opacity_band"]), dy.to_dev(inp["sw_pen_band"])
        own_d = dy.to_dev(own.astype(np.float64)) > 0.5
        dy.set_diffusivity_init(Psd, eos)
        dy.diabatic_aux_init(Pda, eos)
        torch.cuda.synchronize()
        dy.set_diffusivity(t["h"], osd["dt"], sd_out["Kd_int"], T=t["T"], S=t["S"], **{n: t[n] for n in osd["given"]},
                           **{n: sd_out[n] for n in osd["out"]})
        dy.applyBoundaryFluxesInOut(dt, f, t["h"], t["T"], t["S"], nsw=opt["nsw"], opacity_band=op, sw_pen_band=pen,
                                    aggregate_FW_forcing=opt["agg"], evap_CFL_limit=opt["cfl"], minimum_forcing_depth=opt["depth"],
                                    **out)
        with torch.cuda.stream(dy.torch_stream()):
            ent = torch.where(own_d, ent_of(sd_out["Kd_int"], t["h"], torch), torch.zeros_like(sd_out["Kd_int"])).contiguous()
        dy.triDiagTS_Eulerian(t["h"], ent, t["T"], t["S"])
        dy.sync()
        assert dy.diabatic_aux_status() == status
        _bits(sd_out["Kd_int"].cpu().numpy(), sd_want["Kd_int"], "chain: Kd_int")
        for n in out:
            _bits(out[n].cpu().numpy(), want[n], "chain: " + n)
        _bits(t["h"].cpu().numpy(), want["h"], "chain: h")
        _bits(ent.cpu().numpy(), ent_w, "chain: ent")
        sl = H.interior(d, "h")
        H.assert_bitwise(t["T"].cpu().numpy(), Tw, "chain: T", sl)
        H.assert_bitwise(t["S"].cpu().numpy(), Sw, "chain: S", sl)
        assert not np.array_equal(Tw[(slice(None),) + sl], want["T"][(slice(None),) + sl])
    finally:
        dy.close()
