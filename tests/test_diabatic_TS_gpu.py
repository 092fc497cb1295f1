"""mom6x_make_frazil, mom6x_adjust_salt and mom6x_geothermal_in_place on the device (mom6_amd/csrc/diabatic_TS.hip) against the
restatement tests/frazil_ref.py, bit for bit and on whole arrays with no tolerated signed zero.  Every output and every point
outside the range of a call starts as NaN, and h, T and S are NaN beyond the requested halo, so what the reference leaves alone is
checked too; the arrays geothermal_in_place fills as a whole must carry 0 in the halo.  Every case of the table on a bowl at 1, 2,
3 and 8 layers and on a basin with an island at 4, a polar case at 75; halo widths 0, 1 and the context's; the switches of
make_frazil; the nullable outputs of geothermal_in_place and its BFlx_geothermal under every equation of state; launch edges;
wavefronts with one busy lane and with one idle lane; land; -0 planted; inputs only read; two calls in a row; 2 x 2 tiles as host
threads with the exchange counter; refusals and error paths; the chain from make_frazil to make_frazil on device pointers."""
import functools
import itertools
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import frazil_ref as R

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 8), ("island_basin", 4))
ROUTINES = ("frazil", "salt", "geo")


def _orc():
    """The oracle, built (test infrastructure only): what the session's `orc` fixture returns, for the cached restatements."""
    from oracle import orc
    orc.build()
    return orc


def _bits(a, b, name):
    H.assert_bitwise(a, b, name)                                  # bit patterns over the whole array; NaN words must be the same words


def _grid(grid, nk, layout=(1, 1), pe=(0, 0)):
    return getattr(H, grid)(nk=nk, layout=layout, pe=pe)[1:]


def _prep(d, inp, halo):
    """NaN in h, T, S, frazil and internal_heat beyond the computational domain widened by halo, in salt_deficit beyond the
    computational domain: nothing out there may be read or written."""
    inp = R.nan_beyond(d, inp, halo)
    wide = np.zeros(d.shape2(), bool)
    wide[d.sl(-halo, d.ni - 1 + halo, -halo, d.nj - 1 + halo)] = True
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    inp["frazil"] = np.where(wide, inp["frazil"], np.nan)
    inp["internal_heat"] = np.where(wide, inp["internal_heat"], np.nan)
    inp["salt_deficit"] = np.where(own, inp["salt_deficit"], np.nan)
    return inp


class _Dy:
    """A Dycore for the length of a `with`."""
    def __init__(self, d, M, GV, layout=None, pe=None, uid=None):
        from mom6_amd import parallel
        from mom6_amd.dycore import Dycore
        self.dy = Dycore(d, M, GV)
        if layout is not None:
            parallel.attach_comm(self.dy, layout, pe, None, unique_id=uid)

    def __enter__(self):
        return self.dy

    def __exit__(self, *a):
        self.dy.close()


def _device(dy, d, opt, Pf, Pg, inp, halo=0, ncalls=1, routines=ROUTINES):
    """The three routines on the device as tests/frazil_ref.py run() runs them: each on its own upload of the inputs, every
    output of geothermal_in_place starting as NaN.  h, S, p_surf and the host plane of geo_heat are compared with what was
    uploaded.  Returns {routine: {array: result}} and the exchanges made."""
    import torch
    eos = abi.eos_params_default(opt["eos"]) if opt["eos"] is not None else None
    res = {}
    ro = {n: dy.to_dev(inp[n]) for n in ("h", "S", "p_surf")}
    geo_host = inp["geo_heat"].copy()
    torch.cuda.synchronize()
    dy.comm_exchange_count(reset=True)
    if "frazil" in routines:
        T, fr = dy.to_dev(inp["T"]), dy.to_dev(inp["frazil"])
        torch.cuda.synchronize()
        dy.make_frazil_init(Pf)
        for _ in range(ncalls):
            dy.make_frazil(ro["h"], T, ro["S"], fr, ro["p_surf"] if opt["p_surf"] else None, halo)
        dy.sync()
        res["frazil"] = dict(T=T.cpu().numpy(), frazil=fr.cpu().numpy())
    if "salt" in routines:
        S, sd = dy.to_dev(inp["S"]), dy.to_dev(inp["salt_deficit"])
        torch.cuda.synchronize()
        for _ in range(ncalls):
            dy.adjust_salt(ro["h"], S, sd, opt["S_min"])
        dy.sync()
        res["salt"] = dict(S=S.cpu().numpy(), salt_deficit=sd.cpu().numpy())
    if "geo" in routines:
        T = dy.to_dev(inp["T"])
        out = {n: dy.to_dev(a) for n, a in R.geo_outputs(d, opt, inp=inp).items()}
        torch.cuda.synchronize()
        dy.geothermal_init(Pg, geo_host, eos)
        for _ in range(ncalls):
            dy.geothermal_in_place(ro["h"], T, ro["S"], opt["dt"], halo=halo, **out)
        dy.sync()
        res["geo"] = dict({n: a.cpu().numpy() for n, a in out.items()}, T=T.cpu().numpy())
    nex = dy.comm_exchange_count()
    for n in ro:
        _bits(ro[n].cpu().numpy(), inp[n], n + " is only read")
    _bits(geo_host, inp["geo_heat"], "geo_heat is only read")
    return res, nex


def _check(d, got, want, halo, tag):
    wide = np.zeros(d.shape2(), bool)
    wide[d.sl(-halo, d.ni - 1 + halo, -halo, d.nj - 1 + halo)] = True
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    assert set(got) == set(want)
    for r in want:
        assert set(got[r]) == set(want[r]), (r, sorted(got[r]), sorted(want[r]))
        for n in want[r]:
            _bits(got[r][n], want[r][n], f"{tag}: {r}.{n}")
            a = got[r][n]
            if n in ("BFlx_geothermal", "dTdt_diag", "heat_tend_diag"):          # the fills of :434, :436 reach the halo
                assert np.isfinite(a).all(), (tag, n)
                assert (a[..., ~wide] == 0.0).all() and not np.signbit(a[..., ~wide]).any(), (tag, n)
            else:
                rng = own if n == "salt_deficit" else wide
                assert np.isnan(a[..., ~rng]).all() and np.isfinite(a[..., rng]).all(), (tag, r, n)


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, halo=0, ncalls=1, neg_zero=False):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    orc = _orc()
    d, M = _grid(grid, nk)
    GV = abi.vgrid_default()
    Pf, Pg, opt = R.case(name, GV)
    inp = _prep(d, R.inputs(d, M, GV, neg_zero=neg_zero, **opt["inp"]), halo)
    want, counts = R.run(d, M, GV, opt, Pf, Pg, inp, halo=halo, orc=orc, ncalls=ncalls)
    return d, M, GV, Pf, Pg, opt, inp, want, counts


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_parity_with_the_restatement(grid, nk):
    """Every case of the table, whole arrays bit for bit.  At nk = 1 the reclaim arm and the walk act on the same layer."""
    d, M = _grid(grid, nk)
    with _Dy(d, M, abi.vgrid_default()) as dy:
        for name in R.CASES:
            d, M, GV, Pf, Pg, opt, inp, want, counts = _want(grid, nk, name)
            got, nex = _device(dy, d, opt, Pf, Pg, inp)
            _check(d, got, want, 0, f"{grid}/{nk}/{name}")
            assert nex == 0


def test_the_branches_of_the_cpu_list_are_reached_by_what_ran():
    from tests.test_diabatic_TS_cpu import REQUIRED
    tot = R.new_counts()
    for grid, nk in CONFIGS:
        for name in R.CASES:
            for k, v in _want(grid, nk, name)[-1].items():
                tot[k] += v
    for halo in (1, 4):
        for k, v in _want("island_basin", 4, "linear_p", halo)[-1].items():
            tot[k] += v
    print("branch counts", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)


def test_polar_case_at_75_layers():
    """The headline's layer count: polar rows below freezing throughout, pressure-dependent freezing, heat spread over many
    layers, every output of geothermal_in_place, EOS WRIGHT."""
    d, M, GV, Pf, Pg, opt, inp, want, counts = _want("benchmark_small", 75, "linear_p", 4)
    assert counts["fz_thick_freeze"] > 0 and counts["fz_gate_closed"] > 0 and counts["geo_several_layers"] > 0
    with _Dy(d, M, GV) as dy:
        got, _ = _device(dy, d, opt, Pf, Pg, inp, halo=4)
    _check(d, got, want, 4, "benchmark_small/75/linear_p")


@pytest.mark.parametrize("halo", [0, 1, 4])
def test_halo_widths(halo):
    """make_frazil and geothermal_in_place on the computational domain widened by 0, 1 and the context's 4 points, on the basin with
    an island (the halo beyond its closed edges is land) and on the re-entrant torus (wet halos)."""
    for grid, nk, names in (("island_basin", 4, ("linear_p", "teos_poly_p", "millero_p")), ("torus", 3, ("linear_p", "scaled"))):
        for name in names:
            d, M, GV, Pf, Pg, opt, inp, want, _ = _want(grid, nk, name, halo)
            with _Dy(d, M, GV) as dy:
                got, nex = _device(dy, d, opt, Pf, Pg, inp, halo=halo)
            _check(d, got, want, halo, f"{grid}/{name}/halo {halo}")
            assert nex == 0


def test_frazil_switches():
    """The three freezing-point forms x PRESSURE_DEPENDENT_FRAZIL x p_surf given or not x RECLAIM_FRAZIL."""
    d, M = _grid("island_basin", 4)
    GV = abi.vgrid_default()
    inp = _prep(d, R.inputs(d, M, GV), 1)
    with _Dy(d, M, GV) as dy:
        for form, pdf, ps, reclaim in itertools.product((abi.TFREEZE_LINEAR, abi.TFREEZE_MILLERO, abi.TFREEZE_TEOSPOLY), (0, 1),
                                                        (False, True), (0, 1)):
            Pf = abi.frazil_params_default(form_of_TFreeze=form, pressure_dependent_frazil=pdf, reclaim_frazil=reclaim, dTFr_dp=-7.6e-8)
            opt = dict(R.case("linear", GV)[2], p_surf=ps)
            T, fr = inp["T"].copy(), inp["frazil"].copy()
            R.make_frazil(d, M, GV, Pf, inp["h"], T, inp["S"], fr, inp["p_surf"] if ps else None, 1)
            got, _ = _device(dy, d, opt, Pf, None, inp, halo=1, routines=("frazil",))
            _check(d, got, dict(frazil=dict(T=T, frazil=fr)), 1, f"form {form} pdf {pdf} p_surf {ps} reclaim {reclaim}")


def test_geothermal_outputs_in_every_combination():
    """Each of the sixteen sets of nullable outputs, at 3 layers with halo 1; the arrays filled as a whole carry 0 in the halo."""
    orc = _orc()
    d, M = _grid("benchmark_small", 3)
    GV = abi.vgrid_default()
    _, Pg, base = R.case("linear_p", GV)
    inp = _prep(d, R.inputs(d, M, GV), 1)
    eos = abi.eos_params_default(base["eos"])
    with _Dy(d, M, GV) as dy:
        for m in range(16):
            opt = dict(base, out=tuple(n for b, n in enumerate(R._GEO_ALL) if m >> b & 1))
            T = inp["T"].copy()
            out = R.geo_outputs(d, opt, inp=inp)
            R.geothermal_in_place(d, M, GV, Pg, inp["geo_heat"], inp["h"], T, inp["S"], opt["dt"], halo=1, eos=eos, orc=orc, **out)
            got, _ = _device(dy, d, opt, None, Pg, inp, halo=1, routines=("geo",))
            _check(d, got, dict(geo=dict(out, T=T)), 1, f"outputs {opt['out']}")


@pytest.mark.parametrize("form", [abi.LINEAR, abi.WRIGHT, abi.WRIGHT_FULL, abi.WRIGHT_REDUCED, abi.UNESCO, abi.ROQUET_RHO, abi.JACKETT06,
                                  abi.ROQUET_SPV])
def test_BFlx_geothermal_under_every_equation_of_state(form):
    """The bottom layer's density derivative of each form against the oracle's, at 3 layers with halo 2: in the columns of the i
    halo the reference's EOS domain leaves the derivative 0."""
    orc = _orc()
    d, M = _grid("torus", 3)
    GV = abi.vgrid_default()
    _, Pg, base = R.case("linear_p", GV)
    opt = dict(base, eos=form, out=("BFlx_geothermal",))
    inp = _prep(d, R.inputs(d, M, GV), 2)
    T = inp["T"].copy()
    out = R.geo_outputs(d, opt, inp=inp)
    R.geothermal_in_place(d, M, GV, Pg, inp["geo_heat"], inp["h"], T, inp["S"], opt["dt"], halo=2, eos=abi.eos_params_default(form),
                          orc=orc, **out)
    assert (out["BFlx_geothermal"][H.interior(d, "h")] != 0.0).any()
    with _Dy(d, M, GV) as dy:
        got, _ = _device(dy, d, opt, None, Pg, inp, halo=2, routines=("geo",))
    _check(d, got, dict(geo=dict(out, T=T)), 2, f"EOS form {form}")


def _edge_shapes():
    bx, by, i0 = abi.lane_launch_shape()
    at0, at4 = bx, bx + i0 - 4                                    # halo 0: lanes from i = 0; halo 4: from i_first up to ni + 3
    return [(at0 - 1, by - 1, 0), (at0, by, 0), (at0 + 1, by + 1, 0), (1, by + 1, 0),
            (at4 - 1, by - 1, 4), (at4, by, 4), (at4 + 1, by + 1, 4), (2 * bx + i0 - 3, by + 1, 4)]


@pytest.mark.parametrize("ni,nj,halo", _edge_shapes())
def test_launch_extents(ni, nj, halo):
    """Land-free doubly re-entrant tiles whose launch extents sit one point under, at and one point over a whole number of
    work-groups, with and without the halo, three layers."""
    d, M = H.torus(nk=3, ni=ni, nj=nj)[1:]
    GV = abi.vgrid_default()
    orc = _orc()
    with _Dy(d, M, GV) as dy:
        for name in ("linear_p", "teos_poly"):
            Pf, Pg, opt = R.case(name, GV)
            inp = _prep(d, R.inputs(d, M, GV), halo)
            want, _ = R.run(d, M, GV, opt, Pf, Pg, inp, halo=halo, orc=orc)
            got, _ = _device(dy, d, opt, Pf, Pg, inp, halo=halo)
            _check(d, got, want, halo, f"torus {ni}x{nj} halo {halo}/{name}")


def _flat(d, M, T, S, geo):
    GV = abi.vgrid_default()
    f2 = lambda v: np.full(d.shape2(), float(v))
    h = np.full(d.shape3(), 50.0)
    return dict(h=h, T=np.full(d.shape3(), float(T)), S=np.full(d.shape3(), float(S)), frazil=f2(0.0), salt_deficit=f2(0.0),
                internal_heat=f2(1.0), p_surf=f2(0.0), geo_heat=M[G["mask2dT"]] * geo)


def test_wavefronts_with_one_busy_lane_and_with_one_idle_lane():
    """8 layers on a torus one wavefront wide.  One cold column among warm ones: one lane of its wavefront walks the freezing
    arm, the others read T only; and the reverse.  One column whose salt deficit reaches the surface among idle ones.  One heated
    column in a row of unheated ones."""
    d, M = H.torus(nk=8, ni=64, nj=4)[1:]
    GV = abi.vgrid_default()
    Pf, Pg, opt = R.case("linear", GV)
    opt = dict(opt, S_min=30.0, out=("internal_heat", "dTdt_diag"))
    Pg.geothermal_thick = 120.0
    col = (slice(None),) + d.sl(17, 17, 2, 2)
    with _Dy(d, M, GV) as dy:
        for T0, T1, S0, S1, n_busy in ((5.0, -3.0, 35.0, 1.0, 1), (-3.0, 5.0, 1.0, 35.0, d.ni * d.nj - 1)):
            inp = _flat(d, M, T0, S0, 0.0)
            inp["T"][col] = T1; inp["S"][col] = S1
            inp["geo_heat"][d.sl(17, 17, 2, 2)] = 0.1
            inp = _prep(d, inp, 0)
            want, counts = R.run(d, M, GV, opt, Pf, Pg, inp)
            assert counts["fz_reaches_surface"] == n_busy and counts["salt_reaches_surface"] == n_busy, counts
            assert counts["fz_gate_closed"] == (d.ni * d.nj - n_busy) * d.nk and counts["salt_gate_closed"] == (d.ni * d.nj - n_busy) * d.nk
            assert counts["geo_row_skipped"] == d.nj - 1 and counts["geo_unheated_column"] == d.ni - 1 and counts["geo_several_layers"] == 1
            got, _ = _device(dy, d, opt, Pf, Pg, inp)
            _check(d, got, want, 0, f"{n_busy} busy lanes")


def test_land_columns():
    """Land columns of the basin, some with frazil > 0: the reclaim arm has no land mask (it divides by the land column's hc as the
    reference does), the walks leave land alone, and frazil = frazil + fraz_col runs there too."""
    d, M, GV, Pf, Pg, opt, inp, want, counts = _want("island_basin", 4, "linear_p", 1)
    wide = np.zeros(d.shape2(), bool)
    wide[d.sl(-1, d.ni, -1, d.nj)] = True
    land = wide & ~(M[G["mask2dT"]] > 0.0)
    assert (inp["frazil"][land] > 0.0).any() and counts["fz_land_column"] > 0
    with _Dy(d, M, GV) as dy:
        got, _ = _device(dy, d, opt, Pf, Pg, inp, halo=1)
    _check(d, got, want, 1, "land")
    _bits(got["frazil"]["T"][1:, land], inp["T"][1:, land], "T below the surface over land")
    _bits(got["geo"]["T"][:, land], inp["T"][:, land], "geothermal T over land")
    assert (got["frazil"]["T"][0][land] != inp["T"][0][land]).any()      # the reclaim arm ran over land


def test_negative_zero_planted():
    """-0 over blocks of frazil, salt_deficit and T: T = -0 is not below 0, and the sums turn a stored -0 into +0."""
    for name in ("linear", "millero_p"):
        d, M, GV, Pf, Pg, opt, inp, want, _ = _want("island_basin", 4, name, 1, 1, True)
        assert np.signbit(inp["frazil"][np.isfinite(inp["frazil"]) & (inp["frazil"] == 0.0)]).any()
        fr = want["frazil"]["frazil"]
        assert not np.signbit(fr[np.isfinite(fr) & (fr == 0.0)]).any()
        with _Dy(d, M, GV) as dy:
            got, _ = _device(dy, d, opt, Pf, Pg, inp, halo=1)
        _check(d, got, want, 1, "planted/" + name)


def test_two_calls_in_a_row_equal_two_calls_of_the_restatement():
    for name in ("linear_p", "millero"):
        d, M, GV, Pf, Pg, opt, inp, want, _ = _want("island_basin", 4, name, 1, 2)
        one = _want("island_basin", 4, name, 1)[7]
        assert not np.array_equal(want["geo"]["T"], one["geo"]["T"], equal_nan=True)
        with _Dy(d, M, GV) as dy:
            got, _ = _device(dy, d, opt, Pf, Pg, inp, halo=1, ncalls=2)
        _check(d, got, want, 1, "two calls/" + name)


def test_two_by_two_tiles_as_host_threads_exchange_nothing():
    """The four tiles of a 2 x 2 layout as host threads on one GPU (tests/transport), each on its cut of the inputs, equal the
    one-tile run on their own points; the calls exchange nothing."""
    from mom6_amd import parallel
    lib = abi.load_library()
    layout = (2, 2)
    d, M, GV, Pf, Pg, opt, inp, want, _ = _want("benchmark_small", 8, "linear_p")
    H.use_threads_transport(lib)
    try:
        uid = parallel.unique_id(lib)
        out, errors = {}, []

        def tile(pe):
            try:
                dt_, Mt = _grid("benchmark_small", 8, layout=layout, pe=pe)
                tin = _prep(dt_, R.inputs(dt_, Mt, GV), 0)
                with _Dy(dt_, Mt, GV, layout=layout, pe=pe, uid=uid) as dy:
                    out[pe] = (dt_,) + _device(dy, dt_, opt, Pf, Pg, tin)
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
        for r in want:
            for n in want[r]:
                _bits(np.ascontiguousarray(got[r][n][(Ellipsis,) + own]), np.ascontiguousarray(want[r][n][(Ellipsis,) + part]),
                      f"tile {pe}: {r}.{n}")


def test_refused_settings_and_error_paths():
    """TFREEZE_FORM = TEOS10 and use_conT_absS are refused by name; an unknown form, a call before init, a null array, a halo
    outside 0 .. the context's, dt <= 0 and BFlx_geothermal without an equation of state or S are errors; nothing is written."""
    import torch
    d, M = _grid("benchmark_small", 3)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    with _Dy(d, M, GV) as dy:
        t = {n: dy.to_dev(inp[n]) for n in ("h", "T", "S", "frazil", "salt_deficit")}
        nan2, nan3 = dy.to_dev(np.full(d.shape2(), np.nan)), dy.to_dev(np.full(d.shape3(), np.nan))
        torch.cuda.synchronize()
        fz = lambda **kw: dy.make_frazil(kw.get("h", t["h"]), kw.get("T", t["T"]), kw.get("S", t["S"]), kw.get("frazil", t["frazil"]),
                                         None, kw.get("halo", 0))
        geo = lambda dt=3600.0, halo=0, h=t["h"], T=t["T"], S=t["S"], **kw: dy.geothermal_in_place(h, T, S, dt, halo=halo, **kw)
        with pytest.raises(Exception, match="error 1.*initialized"):
            fz()
        with pytest.raises(Exception, match="error 1.*initialized"):
            geo()
        with pytest.raises(Exception, match="error 3.*TEOS10"):
            dy.make_frazil_init(abi.frazil_params_default(form_of_TFreeze=abi.TFREEZE_TEOS10))
        with pytest.raises(Exception, match="error 3.*use_conT_absS"):
            dy.make_frazil_init(abi.frazil_params_default(use_conT_absS=1))
        for form in (0, 5):
            with pytest.raises(Exception, match="error 1.*form_of_TFreeze"):
                dy.make_frazil_init(abi.frazil_params_default(form_of_TFreeze=form))
        with pytest.raises(Exception, match="error 1.*C_p"):
            dy.make_frazil_init(abi.frazil_params_default(C_p=0.0))
        with pytest.raises(Exception, match="error 1.*initialized"):       # a refused init leaves no module behind
            fz()
        dy.make_frazil_init(abi.frazil_params_default())
        for halo in (-1, d.halo + 1):
            with pytest.raises(Exception, match="error 1.*halo"):
                fz(halo=halo)
        for n in ("h", "T", "S", "frazil"):
            with pytest.raises(Exception, match="error 1.*null"):
                fz(**{n: None})
        for a, b, c in ((None, t["S"], t["salt_deficit"]), (t["h"], None, t["salt_deficit"]), (t["h"], t["S"], None)):
            with pytest.raises(Exception, match="error 1.*adjust_salt"):
                dy.adjust_salt(a, b, c, 0.01)
        with pytest.raises(Exception, match="error 1.*null"):
            dy.lib.mom6x_geothermal_init(dy.ctx, None, None, None) and abi.check(dy.lib, 1)
        with pytest.raises(Exception, match="error 1.*C_p"):
            dy.geothermal_init(abi.geothermal_params_default(GV, C_p=-1.0), inp["geo_heat"])
        eos = abi.eos_params_default(abi.WRIGHT)
        eos.form = 99
        with pytest.raises(Exception, match="error 1.*EQN_OF_STATE"):
            dy.geothermal_init(abi.geothermal_params_default(GV), inp["geo_heat"], eos)
        with pytest.raises(Exception, match="error 1.*initialized"):
            geo()
        dy.geothermal_init(abi.geothermal_params_default(GV), inp["geo_heat"], None)
        with pytest.raises(Exception, match="error 1.*BFlx_geothermal.*equation of state"):
            geo(BFlx_geothermal=nan2)
        for dt in (0.0, -1.0):
            with pytest.raises(Exception, match="error 1.*dt"):
                geo(dt=dt)
        for halo in (-1, d.halo + 1):
            with pytest.raises(Exception, match="error 1.*halo"):
                geo(halo=halo, dTdt_diag=nan3)
        with pytest.raises(Exception, match="error 1.*null"):
            geo(h=None)
        with pytest.raises(Exception, match="error 1.*null"):
            geo(T=None)
        dy.geothermal_init(abi.geothermal_params_default(GV), inp["geo_heat"], abi.eos_params_default(abi.WRIGHT))
        with pytest.raises(Exception, match="error 1.*BFlx_geothermal.*tv%S"):
            geo(S=None, BFlx_geothermal=nan2)
        geo(S=None)                                                 # without BFlx_geothermal S is not needed
        dy.sync()
        assert torch.isnan(nan2).all() and torch.isnan(nan3).all()
        for n in ("h", "S", "frazil", "salt_deficit"):
            _bits(t[n].cpu().numpy(), inp[n], n + " untouched")


def test_chain_from_make_frazil_to_make_frazil(orc):
    """benchmark_small x 8: make_frazil -> geothermal_in_place -> applyBoundaryFluxesInOut -> adjust_salt -> triDiagTS_Eulerian ->
    make_frazil on device pointers with no host copy in between, against the same chain of tests/frazil_ref.py, tests/bflux_ref.py
    and the oracle's solve, bit for bit.  The state is cold and fresh enough for the last three stages each to change something."""
    import torch
    from tests import bflux_ref as B
    d, M = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    Pf, Pg, opt = R.case("linear_p", GV)
    S_min = 34.5
    Pda, _, bopt = B.case("plain", GV)
    binp = B.case_inputs(d, M, GV, bopt, thin=False, dry=False, ground=False)
    inp = R.inputs(d, M, GV)
    inp["h"] = binp["h"]
    dt = bopt["dt"]
    nz = d.nk
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    ent = np.zeros(d.shape3(nz + 1))
    ent[1:nz] = np.where(own, 2.0, 0.0)
    # the restatements
    c1, c2, c3 = R.new_counts(), R.new_counts(), R.new_counts()
    T, S, fr = inp["T"].copy(), inp["S"].copy(), inp["frazil"].copy()
    sd, ih = inp["salt_deficit"].copy(), inp["internal_heat"].copy()
    R.make_frazil(d, M, GV, Pf, inp["h"], T, S, fr, inp["p_surf"], 0, c1)
    R.geothermal_in_place(d, M, GV, Pg, inp["geo_heat"], inp["h"], T, S, dt, internal_heat=ih, counts=c1)
    st, status, _ = B.run(d, M, GV, Pda, None, bopt, dict(binp, T=T, S=S), orc=orc)
    h, T, S = st["h"], st["T"], st["S"]
    S_in = S.copy()
    R.adjust_salt(d, M, GV, h, S, sd, S_min, c2)
    assert c2["salt_deficit"] > 0 and c2["salt_reaches_surface"] > 0
    T_in = T.copy()
    orc.triDiagTS_Eulerian(d, h, np.ascontiguousarray(ent), T, GV.H_subroundoff)
    orc.triDiagTS_Eulerian(d, h, np.ascontiguousarray(ent), S, GV.H_subroundoff)
    sl = (slice(None),) + H.interior(d, "h")
    assert not np.array_equal(T[sl], T_in[sl])
    T[:, ~own] = T_in[:, ~own]; S[:, ~own] = S_in[:, ~own]          # the solve's halo is not compared
    T_solved = T.copy()
    R.make_frazil(d, M, GV, Pf, h, T, S, fr, inp["p_surf"], 0, c3)
    assert c3["fz_thick_freeze"] + c3["fz_thin_cold"] > 0 and not np.array_equal(T[sl], T_solved[sl])
    with _Dy(d, M, GV) as dy:
        t = {n: dy.to_dev(a) for n, a in dict(inp, h=binp["h"]).items() if n != "geo_heat"}
        fh = B.flux_planes(d, bopt, binp)
        f = {n: dy.to_dev(a) for n, a in fh.items()}
        ent_d = dy.to_dev(ent)
        dy.make_frazil_init(Pf)
        dy.geothermal_init(Pg, inp["geo_heat"], None)
        dy.diabatic_aux_init(Pda, None)
        torch.cuda.synchronize()
        dy.make_frazil(t["h"], t["T"], t["S"], t["frazil"], t["p_surf"], 0)
        dy.geothermal_in_place(t["h"], t["T"], t["S"], dt, internal_heat=t["internal_heat"])
        dy.applyBoundaryFluxesInOut(dt, f, t["h"], t["T"], t["S"], nsw=0, aggregate_FW_forcing=bopt["agg"], evap_CFL_limit=bopt["cfl"],
                                    minimum_forcing_depth=bopt["depth"])
        dy.adjust_salt(t["h"], t["S"], t["salt_deficit"], S_min)
        dy.triDiagTS_Eulerian(t["h"], ent_d, t["T"], t["S"])
        dy.make_frazil(t["h"], t["T"], t["S"], t["frazil"], t["p_surf"], 0)
        dy.sync()
        assert dy.diabatic_aux_status() == status
        own_sl = H.interior(d, "h")
        for n, w in (("h", h), ("T", T), ("S", S), ("frazil", fr), ("salt_deficit", sd), ("internal_heat", ih)):
            H.assert_bitwise(t[n].cpu().numpy(), w, "chain: " + n, own_sl)
