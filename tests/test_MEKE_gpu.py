"""mom6x_step_forward_MEKE on the device (mom6_amd/csrc/MEKE.hip) against the restatement tests/meke_ref.py, bit for bit and on whole
arrays with no tolerated signed zero (Ku, Au, Le and every diagnostic start as NaN, so the points the reference leaves alone are
checked too): every pow-free case on coasts, narrowed faces, vanished layers and an equator; layer counts; -0 planted in hu, hv and
MEKE; consecutive calls of which the first runs MEKE_equilibrium, also split across a fresh context; 2 x 1, 1 x 2 and 2 x 2 tile layouts as host threads
with the exchange counter; a re-entrant tile one lane wider than a work-group; refused settings and error paths; the chain from
mom6x_set_viscous_BBL and mom6x_calc_slope_functions to mom6x_tracer_hordiff on device pointers.  The cases with MEKE_Cb, MEKE_Ct > 0
evaluate two pows and are held to the project's bound for its other pow sites (tests/test_barotropic_gpu.py)."""
import functools
import json
import os
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import meke_ref as R
from tests.test_MEKE_cpu import GRIDS, cut_from_one_tile
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
INPUT_ONLY = ("h", "hu", "hv", "SN_u", "SN_v", "Rd_dx_h") + R.VISC + R.SOURCES


def _call(dy, t, st, dt, given, dg):
    kw = {n: t[n] for n in given if n in INPUT_ONLY}
    kw.update({n: st[n] for n in ("Kh", "Ku", "Au", "Le") if n in st})
    dy.step_forward_MEKE(st["MEKE"], t["h"], t["SN_u"], t["SN_v"], dt, **kw, **dg)


def _device(d, M, GV, P, inp, dt, dF, given, give_diag, fill=np.nan, ncalls=1, dy=None, st0=None, initialized=None, layout=None,
            pe=None, uid=None):
    """One mom6x_MEKE_init and `ncalls` mom6x_step_forward_MEKE calls on inputs that live on the host; Ku, Au, Le and every
    diagnostic start as `fill`.  Returns the state and the diagnostics of the last call, and the exchanges each call made.  In a
    context of its own, or in the caller's `dy`, which is then left open."""
    import torch
    from mom6_amd import parallel
    from mom6_amd.dycore import Dycore
    own = dy is None
    if own:
        dy = Dycore(d, M, GV)
    try:
        if layout is not None:
            parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
        t = {n: dy.to_dev(a) for n, a in inp.items() if n in INPUT_ONLY}
        st = {n: dy.to_dev(a) for n, a in (st0 if st0 is not None else R.state(d, inp, given, fill)).items()}
        dg = {n: dy.to_dev(a) for n, a in R.outputs(d, give_diag, fill).items()}
        dy.MEKE_init(P, dF[0], dF[1])
        if initialized is not None:
            dy.MEKE_set_initialized(initialized)
        torch.cuda.synchronize()
        nex = []
        for _ in range(ncalls):
            dy.comm_exchange_count(reset=True)
            _call(dy, t, st, dt, given, dg)
            nex.append(dy.comm_exchange_count())
        dy.sync()
        for n in t:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        out = {n: a.cpu().numpy() for n, a in st.items()}
        out.update({n: a.cpu().numpy() for n, a in dg.items()})
        return out, nex
    finally:
        if own:
            dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, ncalls=1):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    d, M, dF = GRIDS[grid](nk)
    GV = abi.vgrid_default()
    P, given, dg, dt = R.case(name, GV)
    inp = R.inputs(d, M, GV)
    counts = dict.fromkeys(R.BRANCHES, 0)
    st, cs, want, npass = None, None, None, 0
    for _ in range(ncalls):
        if want is not None:
            st = {n: want[n] for n in R.STATE if n in want}
        else:
            cs = dict(initialize=not P.cold_start)
        want, _c, npass = R.run(d, M, GV, P, inp, dt, dF, given=given, give_diag=dg, counts=counts, st=st, cs=cs)
    return d, M, dF, GV, P, given, dg, dt, inp, want, counts, npass


def _both(grid, nk, name, tot=None):
    d, M, dF, GV, P, given, dg, dt, inp, want, counts, _ = _want(grid, nk, name)
    got, _ = _device(d, M, GV, P, inp, dt, dF, given, dg)
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], f"{grid}/{nk}/{name}:{n}")
    if tot is not None:
        for k, v in counts.items():
            tot[k] += v
    return d, inp, got


@pytest.mark.parametrize("grid", list(GRIDS))
def test_parity_with_the_restatement(grid):
    """Every pow-free case at 8 and 75 layers, whole arrays bit for bit: MEKE outside the computational domain keeps its (finite)
    halo, Ku, Au, Le and every diagnostic outside the reference's ranges keep their NaN.  The branches of the CPU test are counted
    again over what ran here."""
    from tests.test_MEKE_cpu import REQUIRED
    tot = dict.fromkeys(R.BRANCHES, 0)
    for nk in (8, 75):
        for name in R.CASES_POW_FREE:
            d, inp, got = _both(grid, nk, name, tot=tot)
            dom = np.zeros(d.shape2(), bool)
            dom[H.interior(d, "h")] = True
            assert np.isfinite(got["MEKE"]).all() and not np.array_equal(got["MEKE"], inp["MEKE"])
            for n in ("Ku", "Au", "Le", "src", "Ue", "gamma_b", "LmixScale"):
                if n in got:
                    assert np.isfinite(got[n][dom]).all() and np.isnan(got[n][~dom]).all(), (name, n)
            for s in "uv":
                if "Kh_" + s in got and R.CASES[name][0].get("MEKE_Kh", -1.0) >= 0.:
                    face = np.zeros(d.shape2(), bool)
                    face[H.interior(d, s)] = True
                    assert np.isfinite(got["Kh_" + s][face]).all() and np.isnan(got["Kh_" + s][~face]).all(), (name, s)
    print(f"{grid}: branch counts {tot}")
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)
    assert tot["Kh_lim_Kh_absent"] == 0


@pytest.mark.parametrize("nk", [1, 2, 3, 76, 77, 120])
def test_layer_counts(nk):
    """The three column sums are loops over the layer count given at run time, k = 1..nz in order: one path for any nk, the counts
    around the on-chip solvers' bound (76) and beyond included."""
    for name in ("adv", "adv_bug", "gm_alt"):
        _both("benchmark_small", nk, name)


def test_negative_zero_planted_and_nan_at_untouched_points():
    """-0 in hu, hv and MEKE over a block of columns, land included: baroHu = 0. + (-0*H_to_RZ) is +0 while the bug arm's single
    product keeps -0 (neither sign advects), and (-0 + sdt*src)*mask decides the zero MEKE leaves on land.  Points that are
    neither read nor written hold NaN before and after: h beyond its first halo point, hu and hv outside their faces, SN and the
    visc planes outside their faces."""
    for name in ("adv", "adv_bug"):
        d, M, dF, GV, P, given, dg, dt, inp, _, _, _ = _want("island_basin", 8, name)
        inp = {n: a.copy() for n, a in inp.items()}
        blk = d.sl(10, 20, 6, 16)
        for n in ("hu", "hv"):
            inp[n][(slice(None),) + blk] = -0.0
        inp["MEKE"][blk] = -0.0
        read = np.zeros(d.shape2(), bool)
        read[H.interior(d, "h", extra=1)] = True
        inp["h"][:, ~read] = np.nan
        for s in "uv":
            face = np.zeros(d.shape2(), bool)
            face[H.interior(d, s)] = True
            for n in ("h" + s, "SN_" + s, "Kv_bbl_" + s, "bbl_thick_" + s):
                inp[n][..., ~face] = np.nan
        want, _, _ = R.run(d, M, GV, P, inp, dt, dF, given=given, give_diag=True)
        got, _ = _device(d, M, GV, P, inp, dt, dF, given, True)
        for n in want:
            _bits(got[n], want[n], f"planted/{name}: {n}")
        z = got["MEKE"][blk]
        assert (z == 0.0).any() and (z != 0.0).any() and np.isfinite(got["MEKE"]).all()


@pytest.mark.parametrize("name", ["equil_visc", "equil", "equil_alt"])
def test_three_calls_of_a_new_run_and_a_restart_in_a_fresh_context(name):
    """Three consecutive calls, the first of them with MEKE_equilibrium (no MEKE_COLD_START), carry MEKE, Kh and -- in "equil_visc",
    which allocates all four planes of pass_Kh -- Ku, Au and Le, each rewritten with its halo at every call; and the module's
    restart property: one call, the whole state copied to a fresh context with mom6x_MEKE_set_initialized, two more calls."""
    d, M, dF, GV, P, given, dg, dt, inp, want, _, _ = _want("benchmark_small", 8, name, ncalls=3)
    three, _ = _device(d, M, GV, P, inp, dt, dF, given, False, ncalls=3)
    for n in want:
        _bits(three[n], want[n], f"three calls/{name}: {n}")
    one, _ = _device(d, M, GV, P, inp, dt, dF, given, False, ncalls=1)
    _bits(one["MEKE"], _want("benchmark_small", 8, name)[9]["MEKE"], f"one call/{name}: MEKE")
    assert not np.array_equal(one["MEKE"], three["MEKE"])
    if name == "equil_visc":
        assert set(one) == set(R.STATE)
        for n in ("Ku", "Au"):
            assert np.isfinite(one[n][H.interior(d, "h")]).all() and not np.array_equal(one[n], three[n], equal_nan=True), n
    again, _ = _device(d, M, GV, P, inp, dt, dF, given, False, ncalls=2, st0=one, initialized=True)
    for n in want:
        _bits(again[n], three[n], f"1 + 2 calls/{name}: {n}")


def _expected_exchanges(P, given):
    kh_flux = P.MEKE_Kh >= 0. or P.KhMEKE_Fac > 0. or P.MEKE_advection_factor > 0.
    return int(kh_flux or P.MEKE_K4 >= 0.) + 1 + int(any(n in given for n in ("Kh", "Ku", "Au", "Le")))


@pytest.mark.parametrize("layout", [(2, 1), (1, 2), (2, 2)])
def test_tile_layouts_as_host_threads(layout):
    """The tiles of a layout as host threads on one GPU (tests/transport), each on its cut of the inputs: every plane of every tile,
    halos included, equals the one-tile result of the device wherever the tile's array lies over the one-tile array, and the
    exchange counter reads 1, 2 or 3 per call as the case's switches predict."""
    from mom6_amd import parallel
    lib = abi.load_library()
    GV = abi.vgrid_default()
    for name in ("kh_k4", "k4", "gm", "one_pass"):          # 3, 2, 2 and 1 exchanges
        d, M, dF, _, P, given, dg, dt, inp, _, _, npass = _want("benchmark_small", 8, name)
        one, _ = _device(d, M, GV, P, inp, dt, dF, given, dg)
        assert npass == _expected_exchanges(P, given)
        H.use_threads_transport(lib)
        try:
            uid = parallel.unique_id(lib)
            out, errors = {}, []

            def tile(pe):
                try:
                    dt_, Mt, dFt = GRIDS["benchmark_small"](8, layout=layout, pe=pe)
                    tin = R.inputs(dt_, Mt, GV)
                    out[pe] = (dt_,) + _device(dt_, Mt, GV, P, tin, dt, dFt, given, dg, layout=layout, pe=pe, uid=uid)
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
            dt_, got, nex = out[pe]
            assert nex == [_expected_exchanges(P, given)], (name, pe, nex)
            for n in one:
                mine, part = cut_from_one_tile(d, dt_, n, got[n], one[n])
                _bits(mine, part, f"{name} {layout} tile {pe}: {n}")


def test_reentrant_tile_one_lane_wider_than_a_work_group():
    """A land-free doubly re-entrant tile whose width is the work-group's and one more, with the biharmonic on: the internal
    passes wrap MEKE (two points are read) and Kh around, and the five-point stencils cross the edge of a work-group."""
    from tests.test_dyn_edges_cpu import torus
    bx, by, _ = abi.lane_launch_shape()
    GV = abi.vgrid_default()
    d, M0 = torus(bx + 1, by + 1, nk=4)[1:]
    M, dFx, dFy = R.metrics(d, M0)
    for name in ("kh_k4", "adv", "visc"):
        P, given, dg, dt = R.case(name, GV)
        inp = R.inputs(d, M, GV)
        want, _, _ = R.run(d, M, GV, P, inp, dt, (dFx, dFy), given=given, give_diag=dg)
        got, _ = _device(d, M, GV, P, inp, dt, (dFx, dFy), given, dg)
        for n in want:
            _bits(got[n], want[n], f"torus/{name}: {n}")
        assert np.isfinite(got["Kh"]).all() if "Kh" in got else True


def test_pow_cases_are_held_to_a_tolerance():
    """The defaults MEKE_CB = 25 and MEKE_CT = 50 bring x**0.8 and x**0.25 (:1284, :1289): the device's pow and libm's may differ in
    the last bit, as at btstep's one site, so MEKE, Kh and Ku are held to 1e-12 of each field's range (the bound of
    tests/test_barotropic_gpu.py).  The largest differences seen are recorded in profiles/MEKE_pow.json.  A first call that runs MEKE_equilibrium with the pows
    is exercised for finiteness only: the root find stops at a bracket of 1e-12 m2 s-2, which dominates any such bound."""
    d, M, dF, GV, P, given, dg, dt, inp, want, counts, _ = _want("benchmark_small", 8, "pow")
    assert counts["pow"] > 0
    got, _ = _device(d, M, GV, P, inp, dt, dF, given, dg)
    assert set(got) == set(want)
    worst = {}
    for n in ("MEKE", "Kh", "Ku"):
        ok = np.isfinite(want[n])
        assert np.array_equal(np.isfinite(got[n]), ok)
        rng = want[n][ok].max() - want[n][ok].min()
        worst[n] = float(np.abs(got[n][ok] - want[n][ok]).max() / rng)
    print("pow: largest difference / range:", worst)
    if os.environ.get("MOM6X_RECORD_MEKE_POW"):                                 # a file name: how profiles/MEKE_pow.json was made
        json.dump(dict(case="benchmark_small x 8, tests/meke_ref.py case 'pow'", largest_difference_over_range=worst, bound=1.0e-12),
                  open(os.environ["MOM6X_RECORD_MEKE_POW"], "w"), indent=1)
    for n, v in worst.items():
        assert v <= 1.0e-12, (n, v)
    d, M, dF, GV, P, given, dg, dt, inp, want, _, _ = _want("benchmark_small", 8, "pow_equil")
    got, _ = _device(d, M, GV, P, inp, dt, dF, given, dg)
    for n in got:
        assert np.array_equal(np.isfinite(got[n]), np.isfinite(want[n])), n


def test_refused_settings_and_error_paths():
    """Each `must be 0` member raises at init with a message naming the setting; a call before init, a missing plane (named), the
    Coriolis gradients without MEKE_OLD_LSCALE are errors.  (The halo check of mom6x_MEKE_init cannot be reached from a context,
    whose own halo is at least three: tests/test_MEKE_cpu.py looks for it.)"""
    import torch
    from mom6_amd.dycore import Dycore
    d, M, dF = GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        args = (t["MEKE"], t["h"], t["SN_u"], t["SN_v"], 3600.0)
        with pytest.raises(Exception, match="initialized"):
            dy.step_forward_MEKE(*args)
        with pytest.raises(Exception, match="initialized"):
            dy.MEKE_set_initialized(True)
        words = dict(eke_source_file="EKE_SOURCE = file", eke_source_dbclient="dbclient", use_Kh_diff="USE_KH_IN_MEKE",
                     non_Boussinesq="Boussinesq", open_bcs="open boundary", debug="DEBUG")
        assert set(words) == set(abi.MEKE_MUST_BE_0)
        for member, word in words.items():
            with pytest.raises(Exception, match=word):
                dy.MEKE_init(abi.MEKE_params_default(GV, **{member: 1}), *dF)
        with pytest.raises(Exception, match="dF_dx"):
            dy.MEKE_init(abi.MEKE_params_default(GV))
        torch.cuda.synchronize()
        dy.MEKE_init(abi.MEKE_params_default(GV, use_old_lscale=1))             # no Coriolis gradients needed
        with pytest.raises(Exception, match="MEKE%Kh"):
            dy.step_forward_MEKE(*args)
        dy.MEKE_init(abi.MEKE_params_default(GV, MEKE_FrCoeff=0.5), *dF)
        with pytest.raises(Exception, match="mom_src"):
            dy.step_forward_MEKE(*args, Kh=t["Kh"])
        dy.MEKE_init(abi.MEKE_params_default(GV, viscosity_coeff_Ku=1.0), *dF)
        with pytest.raises(Exception, match="MEKE%Ku"):
            dy.step_forward_MEKE(*args, Kh=t["Kh"])
        dy.MEKE_init(abi.MEKE_params_default(GV, viscosity_coeff_Au=1.0), *dF)
        with pytest.raises(Exception, match="MEKE%Au"):
            dy.step_forward_MEKE(*args, Kh=t["Kh"])
        dy.MEKE_init(abi.MEKE_params_default(GV, MEKE_advection_factor=1.0), *dF)
        with pytest.raises(Exception, match="hu and hv"):
            dy.step_forward_MEKE(*args, Kh=t["Kh"])
        dy.sync()
    finally:
        dy.close()


def test_chain_from_set_viscous_BBL_to_tracer_hordiff(orc):
    """benchmark_small x 8, WRIGHT: mom6x_set_viscous_BBL, mom6x_calc_slope_functions, mom6x_step_forward_MEKE and
    mom6x_tracer_hordiff with MEKE_KHTR_FAC on the same device arrays, nothing passing through the host in between; against
    tests/setvisc_ref.py, tests/varmix_ref.py, tests/meke_ref.py and tests/hordiff_ref.py in sequence, bit for bit."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import hordiff_ref, setvisc_ref, varmix_ref
    d, M, dF = GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    eos = abi.eos_params_default(abi.WRIGHT)
    sv_in = setvisc_ref.inputs(d, M, GV)
    inp = dict(R.inputs(d, M, GV), h=sv_in["h"])
    Psv = setvisc_ref.switch_case("eos", form=abi.WRIGHT)[0]
    Pvm = abi.varmix_params_default(GV, max_depth=4000.0)
    Rlay, gp = abi.layer_densities(d.nk)
    P, given, _, dt = R.case("visc", GV)
    Pthd = abi.tracer_hor_diff_params_default(KHTR=50.0, use_variable_mixing=1, use_MEKE_Kh=1, MEKE_KhTr_fac=0.5)
    # the restatements in sequence
    visc = {n: np.full(d.shape2(), np.nan) for n in R.VISC}
    setvisc_ref.set_viscous_BBL(d, M, GV, Psv, sv_in["u"], sv_in["v"], sv_in["h"], T=sv_in["T"], S=sv_in["S"], eos=eos, orc=orc, **visc)
    SN = dict(SN_u=np.zeros(d.shape2()), SN_v=np.zeros(d.shape2()))
    varmix_ref.calc_slope_functions(d, M, GV, Pvm, sv_in["h"], dt, SN["SN_u"], SN["SN_v"], T=sv_in["T"], S=sv_in["S"], eos=eos, Rlay=Rlay,
                                    g_prime=gp, orc=orc)
    win = dict(inp, **visc, **SN)
    want, _, _ = R.run(d, M, GV, P, win, dt, dF, given=given)
    tr = [sv_in["T"].copy(), sv_in["S"].copy()]
    hordiff_ref.tracer_hordiff(d, M, GV, Pthd, sv_in["h"], dt, tr, planes=dict(MEKE_Kh=want["Kh"]))
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in dict(inp, u=sv_in["u"], v=sv_in["v"], T=sv_in["T"], S=sv_in["S"]).items()}
        for n in R.VISC:
            t[n] = dy.to_dev(np.full(d.shape2(), np.nan))
        t["SN_u"], t["SN_v"] = dy.zeros2(), dy.zeros2()
        st = {n: dy.to_dev(a) for n, a in R.state(d, inp, given).items()}
        trd = [dy.to_dev(sv_in["T"]), dy.to_dev(sv_in["S"])]
        dy.set_visc_init(Psv, eos)
        dy.varmix_init(Pvm, eos, Rlay, gp)
        dy.MEKE_init(P, *dF)
        dy.tracer_hor_diff_init(Pthd)
        torch.cuda.synchronize()
        dy.set_viscous_BBL(t["u"], t["v"], t["h"], T=t["T"], S=t["S"], **{n: t[n] for n in R.VISC})
        dy.calc_slope_functions(t["h"], dt, t["SN_u"], t["SN_v"], T=t["T"], S=t["S"])
        _call(dy, t, st, dt, given, {})
        dy.tracer_hordiff(t["h"], dt, trd, MEKE_Kh=st["Kh"])
        dy.sync()
        for n in R.VISC:
            _bits(t[n].cpu().numpy(), visc[n], "chain: " + n)
        for n in SN:
            _bits(t[n].cpu().numpy(), SN[n], "chain: " + n)
        for n in st:
            _bits(st[n].cpu().numpy(), want[n], "chain: " + n)
        for m, n in enumerate("TS"):
            _bits(trd[m].cpu().numpy(), tr[m], "chain: " + n)
        assert not np.array_equal(tr[0], sv_in["T"])
    finally:
        dy.close()
