"""mom6x_tracer_hordiff on the device (mom6_amd/csrc/tracer_hor_diff.hip) against the restatement tests/hordiff_ref.py, bit for
bit and on whole arrays: every case of the list on closed, island, channel and doubly re-entrant grids with 1, 2, 8 and 9 tracers;
a grid around the edges of the kernel's tile; layer counts; 360 x 180 x 75; refused and off settings; 2 x 1, 1 x 2 and 2 x 2
layouts with real exchanges and an all-reduce that matters; four coupled dynamics steps with tracer advection in the order of
step_MOM; and the headline grid's fixed point, quarter turn and unit scaling."""
import threading

import numpy as np
import pytest

from mom6_amd import abi, parallel
from tests import helpers as H
from tests import hordiff_ref as R
from tests.test_tracer_hor_diff_cpu import GRIDS, REQUIRED, compare_cut, scaled

pytestmark = pytest.mark.gpu
G = abi.G


def _bits(a, b, name):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    ne = a.view(np.int64) != b.view(np.int64)
    n = int(ne.sum())
    if n:
        with np.errstate(invalid="ignore"):
            raise AssertionError(f"{name}: {n} of {a.size} words differ; max|diff| {np.nanmax(np.abs(a - b)[ne]):.3e}")


def _call(dy, d, P, inp, dt, uf=None, give_df=False, give_out=False, fill=np.nan):
    """One init and one mom6x_tracer_hordiff call on inputs that live on the host, through an existing context; the outputs as
    tests/hordiff_ref.run returns them, and num_itts."""
    import torch
    ntr = len(inp["tracers"])
    h = dy.to_dev(inp["h"])
    tr = [dy.to_dev(t) for t in inp["tracers"]]
    pl = {n: dy.to_dev(a) for n, a in inp["planes"].items()}
    full3 = lambda: dy.to_dev(np.full(d.shape3(), fill))   # noqa: E731
    full2 = lambda: dy.to_dev(np.full(d.shape2(), fill))   # noqa: E731
    dfx = [full3() if R.df_given(m, 0) else None for m in range(ntr)] if give_df else None
    dfy = [full3() if R.df_given(m, 1) else None for m in range(ntr)] if give_df else None
    o2 = dict(khdt_x=full2(), khdt_y=full2(), CFL=full2()) if give_out else {}
    dy.tracer_hor_diff_init(P)
    torch.cuda.synchronize()
    n = dy.tracer_hordiff(h, dt, tr, conc_underflow=[uf] * ntr if uf else None, df_x=dfx, df_y=dfy, **pl, **o2)
    dy.sync()
    cpu = lambda a: a.cpu().numpy() if a is not None else None   # noqa: E731
    out = dict(tracers=[cpu(t) for t in tr], df_x=[cpu(a) for a in dfx] if dfx else None, df_y=[cpu(a) for a in dfy] if dfy else None,
               khdt_x=cpu(o2.get("khdt_x")), khdt_y=cpu(o2.get("khdt_y")), CFL=cpu(o2.get("CFL")))
    _bits(h.cpu().numpy(), inp["h"], "h is only read")
    return out, n


def _same(want, got, name):
    for n, a in want.items():
        if a is None:
            assert got[n] is None
            continue
        for m, (x, y) in enumerate(zip(a, got[n]) if isinstance(a, list) else [(a, got[n])]):
            if x is None:
                assert y is None
            else:
                _bits(y, x, f"{name}: {n}[{m}]")


def _both(dy, d, M, GV, name, ntr, counts=None):
    inp = R.inputs(d, M, GV, ntr=ntr)
    P, dt, uf, give_df, give_out = R.case(name, d, M, inp["planes"])
    want, nw, _ = R.run(d, M, GV, P, inp, dt, uf=uf, give_df=give_df, give_out=give_out, counts=counts)
    got, ng = _call(dy, d, P, inp, dt, uf=uf, give_df=give_df, give_out=give_out)
    assert ng == nw, (name, ng, nw)
    _same(want, got, f"{name}/ntr={ntr}")
    return inp, want, got, nw


@pytest.mark.parametrize("grid", list(GRIDS))
def test_parity_with_the_restatement(grid):
    """Every case of the list at 4 and 75 layers with 1, 2, 8 and 9 tracers in turn (the eight-at-a-time seam), whole arrays bit for
    bit: the halos of the tracers hold what the group pass inside the call put there (the wrap of channel and torus), the words of
    df_x, df_y, khdt_x, khdt_y and CFL outside their ranges keep the NaN they started with.  The branches of the CPU test are
    counted again over what ran here (a torus has no closed face, a channel no closed u face)."""
    from mom6_amd.dycore import Dycore
    GV = abi.vgrid_default()
    tot = dict.fromkeys(R.BRANCHES, 0)
    seen = set()
    for nk, ntrs in ((4, (1, 2, 8, 9)), (75, (9, 8, 2, 1))):
        d, M = GRIDS[grid](nk)
        dy = Dycore(d, M, GV)
        try:
            for ci, name in enumerate(R.CASES):
                ntr = ntrs[(ci + (1 if name == "underflow" else 0)) % 4]
                inp, want, got, n = _both(dy, d, M, GV, name, ntr, tot)
                seen.add(ntr)
                assert not np.array_equal(got["tracers"][0], inp["tracers"][0]) and all(np.isfinite(t).all() for t in got["tracers"])
                if got["df_x"] is not None:
                    face = np.zeros(d.shape2(), bool); face[H.interior(d, "u")] = True
                    assert np.isfinite(got["df_x"][0][:, face]).all() and np.isnan(got["df_x"][0][:, ~face]).all()
        finally:
            dy.close()
    assert seen == {1, 2, 8, 9}
    print(f"{grid}: branch counts {tot}")
    for k in REQUIRED:
        if not (grid in ("torus", "channel") and k == "closed_face_wet"):   # (dy_Cu = 0: a channel's walls are rows, with closed v faces only)
            assert tot[k] > 0, (k, tot)


def test_tile_edges():
    """ni one more and nj one less than a multiple of the kernel's tile extents (its own constants), more than one tile both ways,
    three layers: the last tile of a row has one column, the last segment lacks a row.  Three iterations re-make the saved edges."""
    from mom6_amd.dycore import Dycore
    lib = abi.load_library()
    import ctypes as C
    tx, ty, mt = C.c_int(0), C.c_int(0), C.c_int(0)
    abi.check(lib, lib.mom6x_tracer_hordiff_tile(C.byref(tx), C.byref(ty), C.byref(mt)))
    ni, nj = tx.value + 1, 2 * ty.value - 1
    d, M = H.benchmark_small(nk=3, ni=ni, nj=nj)[1:]
    GV = abi.vgrid_default()
    dy = Dycore(d, M, GV)
    try:
        assert dy.tracer_hordiff_tile() == (tx.value, ty.value, mt.value)
        for name, ntr in (("check3", 2), ("const_df", 3), ("maxcfl", 9)):
            _, _, _, n = _both(dy, d, M, GV, name, ntr)
            assert n == (1 if name == "const_df" else 3)
    finally:
        dy.close()


@pytest.mark.parametrize("nk", [1, 2, 76, 77, 120])
def test_layer_counts(nk):
    """One path, the layer count is a run-time value (a grid dimension of the launch); the counts straddle the other modules'
    on-chip bounds."""
    from mom6_amd.dycore import Dycore
    d, M = H.benchmark_small(nk=nk)[1:]
    GV = abi.vgrid_default()
    dy = Dycore(d, M, GV)
    try:
        for name in ("const_df", "check3"):
            _both(dy, d, M, GV, name, 2)
    finally:
        dy.close()


@pytest.mark.parametrize("name,itts", [("const_df", 1), ("check3", 3)])
def test_parity_at_360x180x75(name, itts):
    from mom6_amd.dycore import Dycore
    d, M = H.benchmark_360()[1:]
    GV = abi.vgrid_default()
    dy = Dycore(d, M, GV)
    try:
        _, _, _, n = _both(dy, d, M, GV, name, 2)
        assert n == itts
    finally:
        dy.close()


def test_off_and_refused_settings():
    """Each `must be 0` member raises at init with a message naming the setting; a switched-on term without its plane raises at
    the call, naming the field; KHTR = 0 without variable mixing, and an empty registry, write nothing."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = H.benchmark_small(nk=4)[1:]
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV, ntr=2)
    dy = Dycore(d, M, GV)
    try:
        words = dict(use_neutral_diffusion="USE_NEUTRAL_DIFFUSION", use_hor_bnd_diffusion="USE_HORIZONTAL_BOUNDARY_DIFFUSION",
                     Diffuse_ML_interior="DIFFUSE_ML_TO_INTERIOR", offline="read_khdt_x", open_bcs="open boundary")
        assert set(words) == set(abi.TRACER_HOR_DIFF_MUST_BE_0)
        for member, word in words.items():
            P = abi.tracer_hor_diff_params_default(KHTR=1000.0)
            setattr(P, member, 1)
            with pytest.raises(abi.Mom6xError, match=word):
                dy.tracer_hor_diff_init(P)
        h = dy.to_dev(inp["h"])
        tr = [dy.to_dev(t) for t in inp["tracers"]]
        pl = {n: dy.to_dev(a) for n, a in inp["planes"].items()}
        P = abi.tracer_hor_diff_params_default()
        for k, v in R.VARMIX.items():
            setattr(P, k, v)
        dy.tracer_hor_diff_init(P)
        for field in R.PLANES:
            args = dict(pl); args[field] = None
            assert R.refused(P, args) == field
            with pytest.raises(abi.Mom6xError, match=field):
                dy.tracer_hordiff(h, 3600.0, tr, **args)
        P = abi.tracer_hor_diff_params_default(KHTR=1000.0, Resoln_scaled_KhTr=1)
        dy.tracer_hor_diff_init(P)
        with pytest.raises(abi.Mom6xError, match="Res_fn_h"):
            dy.tracer_hordiff(h, 3600.0, tr)
        dy.sync()
        for P, reg in ((abi.tracer_hor_diff_params_default(KHTR=0.0), tr), (abi.tracer_hor_diff_params_default(KHTR=1000.0), [])):
            dy.tracer_hor_diff_init(P)
            df = [dy.to_dev(np.full(d.shape3(), np.nan)) for _ in range(4)]
            torch.cuda.synchronize()
            n = dy.tracer_hordiff(h, 3600.0, reg, df_x=df[:len(reg)], df_y=df[2:2 + len(reg)])
            dy.sync()
            assert n == 0 and all(bool(torch.isnan(a).all()) for a in df)
            for m, t in enumerate(tr):
                _bits(t.cpu().numpy(), inp["tracers"][m], f"off: tracer {m}")
    finally:
        dy.close()


# -- layouts with real exchanges ---------------------------------------------------------------------------------------------

LAYOUT_NK, LAYOUT_NTR, LAYOUT_CASE = 3, 2, "varmix_check"


def _tile_itts(layout):
    """num_itts of the restatement on each tile's cut ALONE (no max_across_PEs), with the parameters of the whole grid."""
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=LAYOUT_NK)[1:]
    pf = R.case(LAYOUT_CASE, d, M, R.inputs(d, M, GV, ntr=1)["planes"])
    # the case's dt puts the largest cell CFL of the whole grid at 3.5; at 3.3 the largest CFL of the west half and of the north
    # half (0.885 and 0.845 of it on this grid) lie below 3, so that those tiles alone would take three iterations, not four
    pf = (pf[0], pf[1] * (3.3 / 3.5)) + pf[2:]
    alone = {}
    for py in range(layout[1]):
        for px in range(layout[0]):
            dt_, Mt = H.benchmark_small(nk=LAYOUT_NK, layout=layout, pe=(px, py))[1:]
            alone[(px, py)] = R.run(dt_, Mt, GV, pf[0], R.inputs(dt_, Mt, GV, ntr=1), pf[1])[1]
    return pf, alone


def _run_tile(layout, pe, uid, pf, out, errors):
    try:
        from mom6_amd.dycore import Dycore
        GV = abi.vgrid_default()
        d, M = H.benchmark_small(nk=LAYOUT_NK, layout=layout, pe=pe)[1:]
        P, dt, uf, give_df, give_out = pf
        dy = Dycore(d, M, GV)
        try:
            if layout != (1, 1):
                parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
            out[pe] = _call(dy, d, P, R.inputs(d, M, GV, ntr=LAYOUT_NTR), dt, uf=uf, give_df=give_df, give_out=give_out) + (d,)
        finally:
            dy.close()
    except Exception:                                                 # noqa: BLE001 -- reported by the main thread
        import traceback
        errors.append((pe, traceback.format_exc()))


@pytest.mark.parametrize("layout", [(2, 1), (1, 2), (2, 2)])
def test_layouts_with_exchanges(layout):
    """The tiles of a layout as host threads on one GPU, with CHECK_DIFFUSIVE_CFL and at least three iterations: the group pass of
    every iteration is a real exchange, and the iteration count needs max_across_PEs -- the restatement, run on each tile's cut
    alone, gives different counts for at least two tiles.  Each tile must equal its part of the one-tile result bit for bit."""
    lib = abi.load_library()
    pf, alone = _tile_itts(layout)
    assert len(set(alone.values())) >= 2, alone
    errors, ref, out = [], {}, {}
    _run_tile((1, 1), (0, 0), None, pf, ref, errors)
    assert not errors, errors[0][1]
    one, n_one, d1 = ref[(0, 0)]
    assert n_one >= 3 and n_one == max(alone.values())
    H.use_threads_transport(lib)
    try:
        uid = parallel.unique_id(lib)
        pes = [(px, py) for py in range(layout[1]) for px in range(layout[0])]
        threads = [threading.Thread(target=_run_tile, args=(layout, pe, uid, pf, out, errors)) for pe in pes]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
    finally:
        H.use_threads_transport(lib, on=False)
    assert not errors, errors[0][1]
    assert len(out) == len(pes)
    for pe in pes:
        tile, n, dt_ = out[pe]
        assert n == n_one, (pe, n, n_one)
        compare_cut(one, tile, d1, dt_, f"{layout} tile {pe}", bits=_bits)


# -- coupling ------------------------------------------------------------------------------------------------------------------

def test_coupling_over_steps(orc, sums):
    """Four dynamics steps of benchmark_small in the order of step_MOM: after steps 2 and 4 advect_tracer of T, S with the
    accumulated transports, then tracer_hordiff with 2*dt (MOM.F90:1481-1526); the oracle and the restatement on the host side.
    T, S bit for bit in each arithmetic of the mass-flux kernels, and T must differ from a run without the call."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import cases
    cfg = H.benchmark_small()
    gg, d, M = cfg
    inp = cases.rk2_inputs(cfg)
    GV, Rlay, gp, dt = inp["GV"], inp["Rlay"], inp["gp"], inp["dt"]
    bt_mod = dict(strong_drag=1)   # (the default drag path goes through btstep's pow: not bit-exact, tests/test_rk2_gpu.py)
    T0, S0 = cases.thermo_state(d, M)
    P = abi.tracer_hor_diff_params_default(KHTR=2000.0, check_diffusive_CFL=1)
    nsteps = 4

    def oracle(diffuse):
        cont, bt, cor, pgf, rk2 = cases.rk2_params(d, GV, bt_mod)
        m = orc.OrcModel(d, M, GV, cont, bt, cor, pgf, rk2, Rlay, gp, 0)
        so = dict(u=inp["u"].copy(), v=inp["v"].copy(), h=inp["h"].copy(), uh=np.zeros_like(inp["h"]), vh=np.zeros_like(inp["h"]),
                  uhtr=np.zeros_like(inp["h"]), vhtr=np.zeros_like(inp["h"]), eta_av=np.zeros(d.shape2()), T=T0.copy(), S=S0.copy())
        m.initialize(so["u"], so["v"], so["h"], so["uh"], so["vh"], dt)
        hist = []
        for n in range(nsteps):
            m.step(so["u"], so["v"], so["h"], so["uh"], so["vh"], so["uhtr"], so["vhtr"], so["eta_av"], inp["taux"], inp["tauy"], dt,
                   inp["coefs"], calc_dtbt=(n == 0))
            if n % 2 == 1:
                orc.advect_tracer(d, M, GV, 0, dt, 2, so["h"], so["uhtr"], so["vhtr"], 2 * dt, [so["T"], so["S"]])
                so["uhtr"][:] = 0.0; so["vhtr"][:] = 0.0
                if diffuse:
                    R.tracer_hordiff(d, M, GV, P, so["h"], 2 * dt, [so["T"], so["S"]])
                hist.append((so["T"].copy(), so["S"].copy()))
        return so, hist

    so, hist = oracle(True)
    plain, _ = oracle(False)
    sl = (slice(None),) + H.interior(d, "h")
    assert not np.array_equal(so["T"][sl], plain["T"][sl])

    cont2, bt2, cor2, pgf2, rk22 = cases.rk2_params(d, GV, bt_mod)
    dyc = Dycore(d, M, GV, 0)
    try:
        dyc.continuity_init(cont2); dyc.barotropic_init(bt2); dyc.CoriolisAdv_init(cor2); dyc.PressureForce_init(pgf2, Rlay, gp)
        dyc.initialize_dyn_split_RK2(rk22)
        sg = {n: dyc.to_dev(a) for n, a in (("u", inp["u"]), ("v", inp["v"]), ("h", inp["h"]), ("T", T0), ("S", S0))}
        sg.update(uh=dyc.zeros3(), vh=dyc.zeros3(), uhtr=dyc.zeros3(), vhtr=dyc.zeros3(), eta_av=dyc.zeros2())
        dyc.vertvisc_set_coef(*[dyc.to_dev(x) if x is not None else None for x in inp["coefs"][0]])
        dyc.tracer_advect_init(dt, 2)
        dyc.tracer_hor_diff_init(P)
        txd, tyd = dyc.to_dev(inp["taux"]), dyc.to_dev(inp["tauy"])
        torch.cuda.synchronize()
        dyc.dyn_split_RK2_new_run(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], dt)
        for n in range(nsteps):
            dyc.step_MOM_dyn_split_RK2(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], sg["uhtr"], sg["vhtr"], sg["eta_av"], txd, tyd,
                                       dt, calc_dtbt=(n == 0))
            if n % 2 == 1:
                dyc.advect_tracer(sg["h"], sg["uhtr"], sg["vhtr"], 2 * dt, [sg["T"], sg["S"]])
                dyc.sync()
                sg["uhtr"].zero_(); sg["vhtr"].zero_()
                torch.cuda.synchronize()
                dyc.tracer_hordiff(sg["h"], 2 * dt, [sg["T"], sg["S"]])
                dyc.sync()
                for k, want in zip("TS", hist[n // 2]):
                    H.assert_bitwise(sg[k].cpu().numpy(), want, f"{sums}: step {n}: {k}", H.interior(d, "h"))
    finally:
        dyc.close()


# -- the headline grid, device only ----------------------------------------------------------------------------------------------

def _dev_call(d, M, GV, P, h, tracers, dt):
    """On copies of the tracers (device tensors); returns the tracers, df_x and df_y of the first one, khdt_x, khdt_y."""
    import torch
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        dy.tracer_hor_diff_init(P)
        tr = [t.clone() for t in tracers]
        dfx, dfy = torch.zeros_like(h), torch.zeros_like(h)
        kx, ky = torch.zeros_like(h[0]), torch.zeros_like(h[0])
        torch.cuda.synchronize()
        n = dy.tracer_hordiff(h, dt, tr, df_x=[dfx] + [None] * (len(tr) - 1), df_y=[dfy] + [None] * (len(tr) - 1), khdt_x=kx, khdt_y=ky)
        dy.sync()
        return dict(tracers=tr, df_x=dfx, df_y=dfy, khdt_x=kx, khdt_y=ky), n
    finally:
        dy.close()


def test_headline_fixed_point_turn_and_scaling():
    """1440 x 1080 x 75 with T, S and a uniform third tracer, KHTR = 1000, MAX_TR_DIFFUSION_CFL = 2 (two iterations): all values
    finite; the uniform tracer unchanged bit for bit; the quarter turn bit for bit (fluxes up to the sign of a zero); scaling L, T
    or H by 2**11 scales every output by its exact power."""
    import torch
    from tests.test_invariants_gpu import TTurn, _basin
    from tests.test_set_visc_gpu import _headline_state
    dev = torch.device("cuda", 0)
    d, M = _basin("full")
    Md = torch.as_tensor(M, device=dev)
    GV = abi.vgrid_default()
    t = _headline_state(d, Md)
    h = t["h"]
    tracers = [t["T"], t["S"], torch.full_like(t["T"], 34.7)]
    del t
    dt = 7200.0
    P = abi.tracer_hor_diff_params_default(KHTR=1000.0, max_diff_CFL=2.0)
    ref, n = _dev_call(d, M, GV, P, h, tracers, dt)
    assert n == 2
    k = (slice(None),)
    slh, slu, slv = H.interior(d, "h"), H.interior(d, "u"), H.interior(d, "v")
    assert all(bool(torch.isfinite(a).all()) for a in ref["tracers"] + [ref["df_x"], ref["df_y"], ref["khdt_x"], ref["khdt_y"]])
    assert not bool(torch.equal(ref["tracers"][0][k + slh], tracers[0][k + slh])) and float(ref["df_x"].abs().max()) > 0

    def same(a, b, name, zeros=False):
        ne = a.contiguous().view(torch.int64) != b.contiguous().view(torch.int64)
        if zeros:
            ne &= ~((a == 0.0) & (b == 0.0))
        assert not bool(ne.any()), name

    same(ref["tracers"][2], tracers[2], "the uniform tracer")
    # quarter turn
    T = TTurn(d)
    Mr = T.metrics(M)
    rot, nr = _dev_call(T.dr, Mr, GV, P, T.h(h), [T.h(a) for a in tracers], dt)
    assert nr == n
    rlh, rlu, rlv = H.interior(T.dr, "h"), H.interior(T.dr, "u"), H.interior(T.dr, "v")
    for m in range(3):
        same(rot["tracers"][m][k + rlh], T.h(ref["tracers"][m])[k + rlh], f"turn: tracer {m}")
    same(rot["df_x"][k + rlu], T.v_to_u(ref["df_y"])[k + rlu], "turn: df_x'", zeros=True)
    same(rot["df_y"][k + rlv], T.u_to_v(ref["df_x"])[k + rlv], "turn: df_y'", zeros=True)
    same(rot["khdt_x"][rlu], T.v_to_u(ref["khdt_y"], sign=1.0)[rlu], "turn: khdt_x'")
    same(rot["khdt_y"][rlv], T.u_to_v(ref["khdt_x"])[rlv], "turn: khdt_y'")
    del rot
    # unit scaling
    dummy = dict(h=np.zeros(1), tracers=[], planes={n: np.zeros(1) for n in R.PLANES})
    for dim in "LTH":
        M2, GV2, P2, _, dt2, un = scaled(d, M, GV, P, dummy, dt, dim)
        got, n2 = _dev_call(d, M2, GV2, P2, h * (2.0 ** 11 if dim == "H" else 1.0), tracers, dt2)
        assert n2 == n
        for m in range(3):
            same(got["tracers"][m][k + slh], ref["tracers"][m][k + slh], f"scale {dim}: tracer {m}")
        same((got["df_x"] * un["df_x"])[k + slu], ref["df_x"][k + slu], f"scale {dim}: df_x")
        same((got["df_y"] * un["df_y"])[k + slv], ref["df_y"][k + slv], f"scale {dim}: df_y")
        same((got["khdt_x"] * un["khdt_x"])[slu], ref["khdt_x"][slu], f"scale {dim}: khdt_x")
        same((got["khdt_y"] * un["khdt_y"])[slv], ref["khdt_y"][slv], f"scale {dim}: khdt_y")
        del got
