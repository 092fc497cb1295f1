"""mom6x_energetic_PBL, mom6x_energetic_PBL_get_MLD and mom6x_ePBL_augment_Kd on the device (mom6_amd/csrc/energetic_PBL.hip)
against the restatement tests/epbl_ref.py.  Every output starts as NaN and the halos of every input are NaN.  The cases of
CASES_EXACT, which call no exp, log or pow, are compared bit for bit on whole arrays (Kd_int, ML_depth, every diagnostic, OBL_its)
at 1, 2, 3, 4 and 8 layers on a bowl, 4 on a basin with an island and one case at 75; the cases of CASES_LIBM on the columns whose
trace does not depend on the last bits of those functions (tests/test_energetic_PBL_cpu.py has the screen)."""
import functools
import json
import os
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import epbl_ref as R
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 4), ("benchmark_small", 8),
           ("island_basin", 4))
IN3 = ("h", "u", "v", "T", "S", "dSV_dT", "dSV_dS", "TKE_forced")
IN2 = ("ustar", "buoy_flux")


def _grid(grid, nk, layout=(1, 1), pe=(0, 0)):
    return getattr(H, grid)(nk=nk, layout=layout, pe=pe)[1:]


def _nan_halo(d, inp):
    """NaN in the halos of every input: nothing outside the computational domain may be read (u and v keep the one face to the
    west and south that find_uv_at_h reads)."""
    inp = dict(inp)
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    ownu = np.zeros(d.shape2(), bool); ownu[H.interior(d, "u")] = True
    ownv = np.zeros(d.shape2(), bool); ownv[H.interior(d, "v")] = True
    for n in IN3 + IN2:
        m = ownu if n == "u" else ownv if n == "v" else own
        inp[n] = np.where(m, inp[n], np.nan)
    return inp


def _device(d, M, GV, P, opt, inp, fill=np.nan, ncalls=None, layout=None, pe=None, uid=None):
    """One mom6x_energetic_PBL_init, then `ncalls` calls on the same device arrays.  Returns the outputs by name and the exchanges
    made; the inputs are compared with what was uploaded."""
    import torch
    from mom6_amd import parallel
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        if layout is not None:
            parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
        mke = P.MKE_to_TKE_effic > 0.0
        t = {n: dy.to_dev(inp[n]) for n in IN3 + IN2 if mke or n not in ("u", "v")}
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, opt, fill).items()}
        dy.energetic_PBL_init(P)
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        for _ in range(ncalls or opt["ncalls"]):
            dy.energetic_PBL(t["h"], t["T"], t["S"], t["dSV_dT"], t["dSV_dS"], t["TKE_forced"], t["ustar"], t["buoy_flux"], opt["dt"],
                             u=t.get("u"), v=t.get("v"), **out)
        dy.sync()
        nex = dy.comm_exchange_count()
        for n in t:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        return {n: a.cpu().numpy() for n, a in out.items()}, nex
    finally:
        dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    d, M = _grid(grid, nk)
    GV = abi.vgrid_default()
    P, opt = R.case(name, GV)
    inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
    m = R.Libm()
    want, counts = R.run(d, M, GV, P, opt, inp, math=m)
    return d, M, GV, P, opt, inp, want, counts, dict(m.counts)


def _check(d, got, want, tag):
    assert set(got) == set(want), (sorted(got), sorted(want))
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    for n in want:
        _bits(got[n], want[n], f"{tag}: {n}")
        assert np.isnan(got[n][..., halo]).all(), (tag, n)
        assert np.isfinite(got[n][..., ~halo]).all(), (tag, n)


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_exact_cases_bit_for_bit(grid, nk):
    """Every case without a libm call, whole arrays.  nk = 1 has no interior interface, nk = 2 only the K == 2 arms, nk = 3 is the
    first with k-2 terms.  The case `guess` makes two calls in a row, the second starting from the first's ML_depth."""
    for name in R.CASES_EXACT:
        d, M, GV, P, opt, inp, want, counts, libm = _want(grid, nk, name)
        assert libm == dict(exp=0, log=0, pow=0), (name, libm)
        got, nex = _device(d, M, GV, P, opt, inp)
        _check(d, got, want, f"{grid}/{nk}/{name}")
        assert nex == 0


def test_the_arms_of_the_cpu_list_are_reached_by_what_ran():
    from tests.test_energetic_PBL_cpu import REQUIRED, ONLY_LIBM
    tot = dict.fromkeys(R.BRANCHES, 0)
    for grid, nk in CONFIGS:
        for name in R.CASES_EXACT:
            for k, v in _want(grid, nk, name)[7].items():
                tot[k] += v
    print("branch counts", tot)
    for k in REQUIRED:
        if k not in ONLY_LIBM:
            assert tot[k] > 0, (k, tot)


def test_one_case_at_75_layers():
    d, M, GV, P, opt, inp, want, counts, libm = _want("benchmark_small", 75, "croot_new")
    assert libm == dict(exp=0, log=0, pow=0) and counts["newton"] > 0 and counts["unstable_max_le0"] > 0
    got, _ = _device(d, M, GV, P, opt, inp)
    _check(d, got, want, "benchmark_small/75/croot_new")


def _edge_shapes():
    bx, by, _ = abi.lane_launch_shape()
    return [(bx, by), (bx + 1, by + 1), (2 * bx + 1, by), (1, by + 1)]


@pytest.mark.parametrize("ni,nj", _edge_shapes())
def test_launch_extents(ni, nj):
    """Land-free doubly re-entrant tiles whose extents are a whole number of work-groups and one more, and a tile one cell wide."""
    d, M = H.torus(nk=3, ni=ni, nj=nj)[1:]
    GV = abi.vgrid_default()
    for name in ("croot_new", "rh18_orig"):
        P, opt = R.case(name, GV)
        inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
        want, _ = R.run(d, M, GV, P, opt, inp)
        got, _ = _device(d, M, GV, P, opt, inp)
        _check(d, got, want, f"torus {ni}x{nj}/{name}")


def test_one_lane_iterates_to_the_limit_while_its_wavefront_converges_at_once():
    """A row of one wavefront on an f-plane: every column a copy of one that converges in its first iteration, then lane 17 a copy
    of one that reaches max_MLD_its; and the row with no such lane."""
    bx, by, _ = abi.lane_launch_shape()
    d, M = H.torus(nk=3, ni=bx, nj=by)[1:]
    GV = abi.vgrid_default()
    P, opt = R.case("rh18_orig", GV)
    base = R.case_inputs(d, M, GV, opt)
    w0, _ = R.run(d, M, GV, P, opt, base)
    its = w0["OBL_its"][H.interior(d, "h")]
    slow = np.argwhere(its == P.max_MLD_its); fast = np.argwhere(its == 1)
    assert len(slow) and len(fast), np.bincount(its.astype(int).ravel())
    (js, is_), (jf, if_) = slow[0], fast[0]
    for lanes, n_slow in ((False, 0), (True, 1)):
        inp = {}
        for n in IN3 + IN2:
            a = base[n].copy()
            col = a[..., d.joff + jf, d.ioff + if_]
            a[..., :, :] = col[..., None, None] if a.ndim == 3 else col
            if lanes:
                a[..., d.joff + 1, d.ioff + 17] = base[n][..., d.joff + js, d.ioff + is_]
            inp[n] = a
        inp = _nan_halo(d, inp)
        want, _ = R.run(d, M, GV, P, opt, inp)
        wi = want["OBL_its"][H.interior(d, "h")]
        assert (wi == P.max_MLD_its).sum() == n_slow and (wi == 1).sum() == wi.size - n_slow
        got, _ = _device(d, M, GV, P, opt, inp)
        _check(d, got, want, f"{n_slow} slow lanes")


def test_land_columns_are_zero():
    d, M, GV, P, opt, inp, want, _, _ = _want("island_basin", 4, "croot_new")
    got, _ = _device(d, M, GV, P, opt, inp)
    land = np.zeros(d.shape2(), bool)
    land[H.interior(d, "h")] = True
    land &= ~(M[G["mask2dT"]] > 0.0)
    assert land.any()
    for n in got:
        z = got[n][..., land]
        assert (z == 0.0).all() and not np.signbit(z).any(), n


def test_two_calls_with_a_stored_first_guess():
    """MLD_iteration_guess: the second call starts from the first's ML_depth and differs from a single call."""
    d, M, GV, P, opt, inp, want, counts, _ = _want("island_basin", 4, "guess")
    assert opt["ncalls"] == 2 and counts["first_guess_stored"] > 0
    one, _ = R.run(d, M, GV, P, opt, inp, ncalls=1)
    assert not np.array_equal(one["OBL_its"], want["OBL_its"], equal_nan=True)
    got, _ = _device(d, M, GV, P, opt, inp)
    _check(d, got, want, "guess x 2")


def test_two_by_two_tiles_as_host_threads_exchange_nothing():
    from mom6_amd import parallel
    lib = abi.load_library()
    layout = (2, 2)
    d, M, GV, P, opt, inp, want, _, _ = _want("benchmark_small", 8, "croot_new")
    H.use_threads_transport(lib)
    try:
        uid = parallel.unique_id(lib)
        out, errors = {}, []

        def tile(pe):
            try:
                dt_, Mt = _grid("benchmark_small", 8, layout=layout, pe=pe)
                tin = R.case_inputs(dt_, Mt, GV, opt)
                out[pe] = (dt_,) + _device(dt_, Mt, GV, P, opt, tin, layout=layout, pe=pe, uid=uid)
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
        assert nex == 0, (pe, nex)
        own = H.interior(dt_, "h")
        part = d.sl(dt_.i_glob0, dt_.i_glob0 + dt_.ni - 1, dt_.j_glob0, dt_.j_glob0 + dt_.nj - 1)
        for n in want:
            _bits(np.ascontiguousarray(got[n][(Ellipsis,) + own]), np.ascontiguousarray(want[n][(Ellipsis,) + part]), f"tile {pe}: {n}")


@pytest.mark.parametrize("additive", (True, False))
def test_augment_Kd_and_get_MLD(additive):
    """The driver's loop, both arms, levels 2..nk, with -0 planted in Kd_ePBL - Kd_shear; h_ML and get_MLD are scaled copies."""
    from mom6_amd import synth
    from mom6_amd.dycore import Dycore
    d, M = _grid("island_basin", 4)
    GV = abi.vgrid_default()
    f = lambda n, nk: np.ascontiguousarray(1.0e-3 * (1.5 + synth.smooth_field(d, 70 + n, nk=nk, ox=0.5, oy=0.5)))
    a = dict(Kd_ePBL=f(0, d.nk + 1), Kd_shear=f(1, d.nk + 1), Kv_shear=f(2, d.nk + 1), Kd_heat=f(3, d.nk + 1), Kd_salt=f(4, d.nk + 1),
             MLD=np.ascontiguousarray(50.0 * (1.5 + synth.smooth_field(d, 80, ox=0.5, oy=0.5))))
    a["Kd_ePBL"][2][d.sl(3, 9, 3, 9)] = 0.0
    a["Kd_shear"][2][d.sl(3, 9, 3, 9)] = 0.0
    a["Kd_shear"][2][d.sl(3, 5, 3, 9)] = -0.0
    a["Kd_shear"][1][d.sl(10, 20, 3, 9)] = a["Kd_ePBL"][1][d.sl(10, 20, 3, 9)]
    own = np.zeros(d.shape2(), bool); own[H.interior(d, "h")] = True
    a = {n: np.where(own, x, np.nan) for n, x in a.items()}
    want = {n: a[n].copy() for n in ("Kv_shear", "Kd_heat", "Kd_salt")}
    want["h_ML"] = np.full(d.shape2(), np.nan); want["MLD2"] = np.full(d.shape2(), np.nan)
    R.augment_Kd(d, GV, a["Kd_ePBL"], a["Kd_shear"], want["Kv_shear"], want["Kd_heat"], want["Kd_salt"], additive, 0.7, a["MLD"], want["h_ML"])
    R.get_MLD(d, a["MLD"], want["MLD2"], 3.0)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(x) for n, x in a.items()}
        t["h_ML"] = dy.to_dev(np.full(d.shape2(), np.nan)); t["MLD2"] = dy.to_dev(np.full(d.shape2(), np.nan))
        dy.energetic_PBL_init(abi.energetic_PBL_params_default(GV))
        dy.ePBL_augment_Kd(t["Kd_ePBL"], t["Kv_shear"], t["Kd_heat"], t["Kd_salt"], Kd_shear=None if additive else t["Kd_shear"],
                           ePBL_is_additive=additive, ePBL_Prandtl=0.7, MLD=t["MLD"], h_ML=t["h_ML"])
        dy.energetic_PBL_get_MLD(t["MLD"], t["MLD2"], 3.0)
        dy.sync()
        for n in want:
            _bits(t[n].cpu().numpy(), want[n], f"augment additive={additive}: {n}")
        for n in ("Kd_ePBL", "Kd_shear", "MLD"):
            _bits(t[n].cpu().numpy(), a[n], n + " is only read")
        for n in ("Kv_shear", "Kd_heat", "Kd_salt"):               # levels 1 and nk + 1 stay
            _bits(t[n].cpu().numpy()[0], a[n][0], n + " level 1"); _bits(t[n].cpu().numpy()[d.nk], a[n][d.nk], n + " bottom")
    finally:
        dy.close()


def test_refused_settings_and_error_paths():
    """Each `must be 0` member is refused at init with a message naming the setting, so is TKE_diagnostics with MKE conversion;
    a missing array, MKE conversion without u and v, no equation of state, a diag_TKE_* plane without TKE_diagnostics and a call
    before init are errors; the outputs stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = _grid("benchmark_small", 4)
    GV = abi.vgrid_default()
    P0, opt = R.case("croot_orig", GV)
    inp = R.case_inputs(d, M, GV, opt)
    dflt = abi.energetic_PBL_params_default
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(inp[n]) for n in IN3 + IN2}
        Kd = dy.to_dev(np.full(d.shape3(d.nk + 1), np.nan)); MLD = dy.to_dev(np.full(d.shape2(), np.nan))
        pl = dy.to_dev(np.full(d.shape2(), np.nan))
        torch.cuda.synchronize()

        def call(skip=None, u=None, v=None, Kd_=Kd, **kw):
            a = {n: (None if n == skip else t[n]) for n in ("h", "T", "S", "dSV_dT", "dSV_dS", "TKE_forced", "ustar", "buoy_flux")}
            dy.energetic_PBL(a["h"], a["T"], a["S"], a["dSV_dT"], a["dSV_dS"], a["TKE_forced"], a["ustar"], a["buoy_flux"], 3600.0, Kd_, MLD,
                             u=u, v=v, **kw)
        with pytest.raises(Exception, match="initialized"):
            call()
        with pytest.raises(Exception, match="initialized"):
            dy.energetic_PBL_get_MLD(MLD, pl)
        words = dict(ePBL_BBL_effic="EPBL_BBL_EFFIC", ePBL_tidal_effic="EPBL_BBL_TIDAL_EFFIC", ePBL_BBL_use_mstar="EPBL_BBL_USE_MSTAR",
                     use_LT="Langmuir", eqdisc="EPBL_EQD_DIFFUSIVITY_SHAPE", eqdisc_v0="EPBL_EQD_DIFFUSIVITY_VELOCITY",
                     eqdisc_v0h="EPBL_EQD_DIFFUSIVITY_VELOCITY_H", direct_calc="DIRECT_EPBL_MIXING_CALC", options_diff="EPBL_OPTIONS_DIFF",
                     pert_epbl="stochastic", ustar_shelf="ustar_shelf", tau_mag="tau_mag", SpV_avg="SpV_avg")
        assert set(words) == set(abi.ENERGETIC_PBL_MUST_BE_0)
        for member, word in words.items():
            with pytest.raises(Exception, match="error 3.*" + word):
                dy.energetic_PBL_init(dflt(GV, **{member: 1}))
        with pytest.raises(Exception, match="error 3.*TKE_diagnostics together with MKE_TO_TKE_EFFIC"):
            dy.energetic_PBL_init(dflt(GV, TKE_diagnostics=1, MKE_to_TKE_effic=0.1))
        with pytest.raises(Exception, match="error 1.*EPBL_MSTAR_SCHEME"):
            dy.energetic_PBL_init(dflt(GV, mstar_scheme=1))
        with pytest.raises(Exception, match="initialized"):       # a refused init leaves no module behind
            call()
        dy.energetic_PBL_init(dflt(GV))
        call()
        with pytest.raises(Exception, match="error 3.*Langmuir"):
            dy.energetic_PBL_init(dflt(GV, use_LT=1))
        with pytest.raises(Exception, match="initialized"):       # nor does a refused init after a good one
            call()
        Kd.fill_(float("nan")); MLD.fill_(float("nan")); torch.cuda.synchronize()
        dy.energetic_PBL_init(dflt(GV, has_eos=0))
        with pytest.raises(Exception, match="error 1.*equation of state"):
            call()
        dy.energetic_PBL_init(dflt(GV, MKE_to_TKE_effic=0.1))
        with pytest.raises(Exception, match="error 1.*needs u and v"):
            call()
        with pytest.raises(Exception, match="error 1.*needs u and v"):
            call(u=t["u"])
        dy.energetic_PBL_init(dflt(GV))
        with pytest.raises(Exception, match="error 1.*friction velocity"):
            call(skip="ustar")
        for n in ("h", "T", "dSV_dS", "TKE_forced", "buoy_flux"):
            with pytest.raises(Exception, match="error 1.*null h"):
                call(skip=n)
        with pytest.raises(Exception, match="error 1.*Kd_int"):
            call(Kd_=None)
        with pytest.raises(Exception, match="error 1.*TKE_diagnostics"):
            call(diag_TKE_wind=pl)
        with pytest.raises(Exception, match="error 1.*go together"):
            dy.ePBL_augment_Kd(Kd, Kd, Kd, Kd, MLD=MLD)
        with pytest.raises(Exception, match="error 1.*Kd_shear"):
            dy.ePBL_augment_Kd(Kd, Kd, Kd, Kd, ePBL_is_additive=False)
        dy.sync()
        assert torch.isnan(Kd).all() and torch.isnan(MLD).all() and torch.isnan(pl).all()
    finally:
        dy.close()


def test_libm_cases_on_the_steady_columns():
    """The cases with exp, log or pow: a last-bit difference between the device's functions and libm's can flip a branch or an
    iteration count, so the columns whose trace changes under +-2 ulp on every result (tests/test_energetic_PBL_cpu.py screen())
    are left out and counted -- at most 5 % of the wet columns -- and the steady ones are held, per field, to four times the
    largest difference over range among the five CPU runs, and not less than 1e-12 of range.  The CPU spreads and the device's
    largest differences go to the file MOM6X_RECORD_EPBL_LIBM names (profiles/ePBL_libm.json).  The case mke_shear runs at 4
    layers too: among its steady columns are solves that take a false-position step (:1794) and one that ends at 20 steps
    (:1799), so both arms of the bracketed solve are compared on the device.  (Its spreads are large: a column that ends at
    max_MLD_its returns the depth of an iteration that has not converged, which moves by 4e-4 of range under +-2 ulp.)"""
    from tests.test_energetic_PBL_cpu import screen, solve_arms, CAP, LIBM_RUNS
    rec = {}
    fp = mx = 0
    for name, nk in LIBM_RUNS:
        d, M, GV, P, opt, inp, want, steady, spread, traces = screen("benchmark_small", nk, name, nan_halo=_nan_halo)
        a, b = solve_arms(traces, steady)
        fp += a; mx += b
        name = f"{name}/{nk}"
        wet = M[G["mask2dT"]][H.interior(d, "h")] > 0.0
        left = int((wet & ~steady).sum())
        assert left <= CAP * wet.sum(), (name, left, int(wet.sum()))
        got, _ = _device(d, M, GV, P, opt, inp)
        assert set(got) == set(want)
        keep = np.zeros(d.shape2(), bool)
        keep[H.interior(d, "h")] = steady | ~wet
        rec[name] = dict(left_out=left, wet=int(wet.sum()), cpu_spread={}, device={}, bound={})
        for n in want:
            w, g = want[n][..., keep], got[n][..., keep]
            assert np.isfinite(g).all(), (name, n)
            rng = float(w.max() - w.min())
            diff = float(np.abs(g - w).max())
            bound = max(4.0 * spread[n], 1.0e-12)
            rec[name]["cpu_spread"][n] = spread[n]; rec[name]["device"][n] = diff / rng if rng > 0.0 else diff
            rec[name]["bound"][n] = bound
        print(name, json.dumps(rec[name]))
    assert fp > 0 and mx > 0, (fp, mx)     # both arms of the bracketed solve ran in columns that were compared
    if os.environ.get("MOM6X_RECORD_EPBL_LIBM"):
        json.dump(dict(case="benchmark_small, tests/test_energetic_PBL_cpu.py LIBM_RUNS (case/layers)", cap=CAP,
                       steady_columns_with_a_false_position_step=fp, steady_columns_with_a_solve_of_20_steps=mx, cases=rec), open(os.environ["MOM6X_RECORD_EPBL_LIBM"], "w"),
                  indent=1)
    for name, r in rec.items():
        for n, v in r["device"].items():
            assert v <= r["bound"][n], (name, n, v, r["bound"][n])


def test_chain_from_set_diffusivity_through_energetic_PBL_to_triDiagTS_Eulerian(orc):
    """benchmark_small x 8, WRIGHT: mom6x_set_diffusivity -> mom6x_applyBoundaryFluxesInOut -> mom6x_energetic_PBL on the cTKE,
    dSV_dT, dSV_dS and SkinBuoyFlux it wrote -> mom6x_ePBL_augment_Kd on Kd_heat = Kd_salt = Kd_int -> ent from Kd_heat and the
    new thicknesses with torch ops on the context's stream -> mom6x_triDiagTS_Eulerian, all on device pointers with no host copy
    in between; against the same chain of restatements and the oracle's solve, bit for bit."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import setdiff_ref, bflux_ref
    d, M = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    Psd, eos, osd = setdiff_ref.case("dd_sf", GV)
    Pda, _, oda = bflux_ref.case("wright_3", GV)
    Pe, oe = R.case("croot_new", GV)
    binp = bflux_ref.case_inputs(d, M, GV, oda, thin=False, dry=False, ground=False)
    einp = R.case_inputs(d, M, GV, oe)
    sd_in = dict(setdiff_ref.inputs(d, M, GV, **osd["inp"]), h=binp["h"], T=binp["T"], S=binp["S"])
    dt = oda["dt"]
    nz = d.nk
    Kd_sfc = setdiff_ref.Kd_sfc_plane(d, Psd)
    sd_want, _ = setdiff_ref.run(d, M, GV, Psd, eos, osd, sd_in, Kd_sfc=Kd_sfc, orc=orc)
    bw, status, _ = bflux_ref.run(d, M, GV, Pda, eos, oda, binp, orc=orc)
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    ew = R.outputs(d, oe)
    m = R.Libm()
    R.energetic_PBL(d, M, GV, Pe, bw["h"], None, None, bw["T"], bw["S"], bw["dSV_dT"], bw["dSV_dS"], bw["cTKE"], einp["ustar"],
                    bw["SkinBuoyFlux"], dt, math=m, **ew)
    assert m.counts == dict(exp=0, log=0, pow=0)
    Kv0 = np.where(own, 1.0e-4, np.nan) * np.ones(d.shape3(nz + 1))
    Kv_w = Kv0.copy()
    Kh_w, Ks_w = sd_want["Kd_int"].copy(), sd_want["Kd_int"].copy()
    hML_w = np.full(d.shape2(), np.nan)
    R.augment_Kd(d, GV, ew["Kd_int"], None, Kv_w, Kh_w, Ks_w, True, 1.0, ew["ML_depth"], hML_w)
    assert not np.array_equal(Kh_w[1:nz][:, own], sd_want["Kd_int"][1:nz][:, own])

    def ent_of(Kd_int, h, xp):
        ent = xp.zeros_like(Kd_int)
        dz = GV.H_to_Z * h
        ent[1:nz] = dt * Kd_int[1:nz] / (0.5 * (dz[:nz - 1] + dz[1:nz]) + GV.dZ_subroundoff)
        return ent
    ent_w = np.where(own, ent_of(Kh_w, bw["h"], np), 0.0)
    Tw, Sw = bw["T"].copy(), bw["S"].copy()
    orc.triDiagTS_Eulerian(d, bw["h"], np.ascontiguousarray(ent_w), Tw, GV.H_subroundoff)
    orc.triDiagTS_Eulerian(d, bw["h"], np.ascontiguousarray(ent_w), Sw, GV.H_subroundoff)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(sd_in[n]) for n in ("u", "v", "h", "T", "S") + tuple(osd["given"])}
        sd_out = {n: dy.to_dev(a) for n, a in setdiff_ref.outputs(d, Psd, osd).items()}
        bout = {n: dy.to_dev(a) for n, a in bflux_ref.outputs(d, oda).items()}
        eout = {n: dy.to_dev(a) for n, a in R.outputs(d, oe).items()}
        f = {n: dy.to_dev(a) for n, a in bflux_ref.flux_planes(d, oda, binp).items()}
        op, pen = dy.to_dev(binp["opacity_band"]), dy.to_dev(binp["sw_pen_band"])
        ustar = dy.to_dev(einp["ustar"])
        Kv = dy.to_dev(Kv0); hML = dy.to_dev(np.full(d.shape2(), np.nan))
        own_d = dy.to_dev(own.astype(np.float64)) > 0.5
        dy.set_diffusivity_init(Psd, eos)
        dy.diabatic_aux_init(Pda, eos)
        dy.energetic_PBL_init(Pe)
        torch.cuda.synchronize()
        dy.set_diffusivity(t["h"], osd["dt"], sd_out["Kd_int"], T=t["T"], S=t["S"], **{n: t[n] for n in osd["given"]},
                           **{n: sd_out[n] for n in osd["out"]})
        dy.applyBoundaryFluxesInOut(dt, f, t["h"], t["T"], t["S"], nsw=oda["nsw"], opacity_band=op, sw_pen_band=pen,
                                    aggregate_FW_forcing=oda["agg"], evap_CFL_limit=oda["cfl"], minimum_forcing_depth=oda["depth"],
                                    **bout)
        dy.energetic_PBL(t["h"], t["T"], t["S"], bout["dSV_dT"], bout["dSV_dS"], bout["cTKE"], ustar, bout["SkinBuoyFlux"], dt, **eout)
        with torch.cuda.stream(dy.torch_stream()):
            Kh = sd_out["Kd_int"].clone(); Ks = sd_out["Kd_int"].clone()
        dy.ePBL_augment_Kd(eout["Kd_int"], Kv, Kh, Ks, ePBL_is_additive=True, ePBL_Prandtl=1.0, MLD=eout["ML_depth"], h_ML=hML)
        with torch.cuda.stream(dy.torch_stream()):
            ent = torch.where(own_d, ent_of(Kh, t["h"], torch), torch.zeros_like(Kh)).contiguous()
        dy.triDiagTS_Eulerian(t["h"], ent, t["T"], t["S"])
        dy.sync()
        for n in eout:
            _bits(eout[n].cpu().numpy(), ew[n], "chain: " + n)
        _bits(Kh.cpu().numpy(), Kh_w, "chain: Kd_heat"); _bits(Ks.cpu().numpy(), Ks_w, "chain: Kd_salt")
        _bits(Kv.cpu().numpy(), Kv_w, "chain: Kv_shear"); _bits(hML.cpu().numpy(), hML_w, "chain: h_ML")
        _bits(ent.cpu().numpy(), ent_w, "chain: ent")
        sl = H.interior(d, "h")
        H.assert_bitwise(t["T"].cpu().numpy(), Tw, "chain: T", sl)
        H.assert_bitwise(t["S"].cpu().numpy(), Sw, "chain: S", sl)
    finally:
        dy.close()
