"""mom6x_neutral_diffusion_calc_coeffs, mom6x_neutral_diffusion and mom6x_tracer_hordiff_neutral on the device
(mom6_amd/csrc/neutral_diffusion.hip, tracer_hor_diff.hip) against the restatement tests/ndiff_ref.py, whole arrays bit for bit:
the ten coefficient arrays on their face ranges, every tracer, tendency, trans_x_2d and trans_y_2d.  The arithmetic is + - * / and
compares, plus the density derivatives that eos_dev.h reproduces bit for bit; there is no tolerance class and no site needed one.
Every input has NaN in every halo point beyond the first and every output starts as NaN: afterwards the outputs' halos are still
NaN, their interiors finite, the inputs (Coef_x and Coef_y, which hold NaN on every plane but the first, among them) are what was
uploaded, and neither call has made an exchange.  tests/test_neutral_diffusion_cpu.py screens the restatement without a GPU."""
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import hordiff_ref
from tests import ndiff_ref as R
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = R.CONFIGS
IN = ("h", "T", "S", "p_surf")
DIAG = ("tendency", "trans_x_2d", "trans_y_2d")


def _ibits(a, b, name):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    n = int((a != b).sum())
    assert n == 0, f"{name}: {n} of {a.size} words differ"


def _device(d, M, GV, P, opt, inp, fill=np.nan, ncoeffs=1, ndiff=1, dy=None, init=True, info=None):
    """One mom6x_neutral_diffusion_init, `ncoeffs` calc_coeffs calls and `ndiff` neutral_diffusion calls, each on fresh copies of
    the tracers.  Returns the outputs as ndiff_ref.run names them (the coefficients cut to nothing: whole arrays, compared on
    their face ranges) and the exchanges made; the inputs are compared with what was uploaded."""
    import torch
    from mom6_amd.dycore import Dycore
    own = dy is None
    dy = dy or Dycore(d, M, GV)
    try:
        ntr = len(inp["tracers"])
        t = {n: dy.to_dev(inp[n]) for n in IN if n in inp}
        Cx, Cy = R.coef_planes(d, M)
        cx, cy = dy.to_dev(Cx), dy.to_dev(Cy)
        if init:
            dy.neutral_diffusion_init(P, R.case_eos(opt))
        if info is not None:
            info["work_bytes"] = dy.neutral_diffusion_work_bytes()
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        for _ in range(ncoeffs):
            dy.neutral_diffusion_calc_coeffs(t["h"], t["T"], t["S"], t.get("p_surf"))
        out = None
        for _ in range(ndiff):
            prev = out
            tr = [dy.to_dev(x) for x in inp["tracers"]]
            o = {n: [dy.to_dev(np.full(d.shape3() if n == "tendency" else d.shape2(), fill)) for _ in range(ntr)] for n in DIAG}
            torch.cuda.synchronize()
            dy.neutral_diffusion(t["h"], cx, cy, R.DT, tr, conc_underflow=R.case_uf(opt, ntr), **o)
            dy.sync()
            out = dict(tracers=[x.cpu().numpy() for x in tr], **{n: [x.cpu().numpy() for x in o[n]] for n in DIAG})
            if prev is not None:
                for n in out:
                    for m in range(ntr):
                        _bits(out[n][m], prev[n][m], f"a second neutral_diffusion call: {n}[{m}]")
        dy.sync()
        nex = dy.comm_exchange_count()
        assert dy.neutral_diffusion_status() == (0, 0, 0, 0)
        for dir, p in ((0, "u"), (1, "v")):
            for n, a in dy.neutral_diffusion_coeffs(dir).items():
                out[p + n] = a.cpu().numpy()
        for n in t:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        _bits(cx.cpu().numpy(), Cx, "Coef_x is only read"); _bits(cy.cpu().numpy(), Cy, "Coef_y is only read")
        return out, nex
    finally:
        if own:
            dy.close()


def _check(d, got, want, tag):
    slu, slv, slh = H.interior(d, "u"), H.interior(d, "v"), H.interior(d, "h")
    k = (slice(None),)
    for p, sl in (("u", slu), ("v", slv)):
        for n in ("PoL", "PoR", "hEff"):
            _bits(got[p + n][k + sl], want[p + n][k + sl], f"{tag}: {p}{n}")
        for n in ("KoL", "KoR"):
            _ibits(got[p + n][k + sl], want[p + n][k + sl], f"{tag}: {p}{n}")
    ring = np.ones(d.shape2(), bool); ring[H.interior(d, "h", extra=1)] = False
    for n, sl in (("tracers", slh), ("tendency", slh), ("trans_x_2d", slu), ("trans_y_2d", slv)):
        assert len(got[n]) == len(want[n])
        for m, (a, b) in enumerate(zip(got[n], want[n])):
            _bits(a, b, f"{tag}: {n}[{m}]")
            inside = np.zeros(d.shape2(), bool); inside[sl] = True
            assert np.isfinite(a[..., inside]).all(), (tag, n, m)
            assert np.isnan(a[..., ring if n == "tracers" else ~inside]).all(), (tag, n, m)


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_every_case_bit_for_bit(grid, nk):
    """Whole arrays.  nk = 1 has one layer and no interior interface, nk = 2 the first interior one with both index clamps of
    interface_scalar active, nk = 4 the first interface with neither km2 nor kp1 clamped."""
    for name in R.CASES:
        d, M, GV, P, opt, inp, want, counts = R.want(grid, nk, name)
        got, nex = _device(d, M, GV, P, opt, inp)
        _check(d, got, want, f"{grid}/{nk}/{name}")
        assert nex == 0


def test_the_arms_of_the_cpu_list_are_reached_by_what_ran():
    from tests.test_neutral_diffusion_cpu import REQUIRED, total_counts
    tot = total_counts()
    print("arm counts", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)


def test_the_slope_case_at_75_layers():
    d, M, GV, P, opt, inp, want, counts = R.want("benchmark_small", 75, "slope", ni=20, nj=12)
    assert counts["left_interp"] > 0 and counts["right_interp"] > 0 and counts["flux_down"] > 0 and counts["unclamped"] > 0
    got, nex = _device(d, M, GV, P, opt, inp)
    _check(d, got, want, "benchmark_small 20 x 12/75/slope")
    assert nex == 0


def _edge_shapes():
    lib = abi.load_library()
    import ctypes as C
    bx, by, i0 = C.c_int(0), C.c_int(0), C.c_int(0)
    abi.check(lib, lib.mom6x_neutral_diffusion_tile(C.byref(bx), C.byref(by), C.byref(i0)))
    return bx.value, by.value, i0.value


# (grid, layers, the grid's shape from the kernels' block extents (bx, by) and the i of their first lane (i0 = -IAL), the case).
# k_ndiff_update starts at i = 0, j = 0: its extents are ni and nj, and the first three tori sit on its edges.  The column kernels
# (k_ndiff_interface, k_ndiff_edges) run i = i0 .. ni and j = -1 .. nj, extents ni + 1 - i0 and nj + 2; the face kernels
# (k_ndiff_positions, k_ndiff_flux) i = i0 .. ni - 1 and j = -1 .. nj - 1, extents ni - i0 and nj + 1.  The four tori torus_i0_*
# have ni = bx + i0 - 2 .. bx + i0 + 1 and nj = 2 by - 3 .. 2 by: the column kernels' extents are one less than, equal to and one
# more than a whole number of blocks at the first three of them, the face kernels' at the last three.
LAUNCH_EDGES = {
    "torus_less": ("torus", 3, lambda bx, by, i0: dict(ni=bx - 1, nj=by - 1), "slope"),
    "torus_equal": ("torus", 3, lambda bx, by, i0: dict(ni=bx, nj=by), "new_order"),
    "torus_more": ("torus", 3, lambda bx, by, i0: dict(ni=bx + 1, nj=by + 1), "slope"),
    "torus_i0_a": ("torus", 3, lambda bx, by, i0: dict(ni=bx + i0 - 2, nj=2 * by - 3), "slope"),
    "torus_i0_b": ("torus", 3, lambda bx, by, i0: dict(ni=bx + i0 - 1, nj=2 * by - 2), "new_order"),
    "torus_i0_c": ("torus", 3, lambda bx, by, i0: dict(ni=bx + i0, nj=2 * by - 1), "slope"),
    "torus_i0_d": ("torus", 3, lambda bx, by, i0: dict(ni=bx + i0 + 1, nj=2 * by), "new_order"),
    "bowl_7x5": ("benchmark_small", 3, lambda bx, by, i0: dict(ni=7, nj=5), "slope"),        # fewer columns than a wavefront
}


@pytest.mark.parametrize("poison", ("0", "1"))
@pytest.mark.parametrize("edge", sorted(LAUNCH_EDGES))
def test_launch_shape_edges(monkeypatch, edge, poison):
    """Land-free tori whose ni and nj are one less than, equal to and one more than the block extents of the module's
    kernels (its own constants), tori that put the same three positions where the kernels that start at i = i_first and j = -1
    round up to another block, and 7 x 5 x 3, on a workspace that starts as zeros and as NaN: every word a call reads of the
    module's arrays it has written before."""
    from mom6_amd.dycore import Dycore
    bx, by, i0 = _edge_shapes()
    grid, nk, shape, name = LAUNCH_EDGES[edge]
    kw = shape(bx, by, i0)
    d, M, GV, P, opt, inp, want, counts = R.want(grid, nk, name, **kw)
    assert (d.ni, d.nj) == (kw["ni"], kw["nj"]) and counts["left_interp"] > 0 and counts["flux_down"] > 0
    if grid == "torus":
        assert counts["dry_face"] == 0 and counts["land_cell"] == 0
    else:
        assert (d.ni + 2) * (d.nj + 2) < 64
    monkeypatch.setenv("MOM6X_POISON_WORK", poison)
    dy = Dycore(d, M, GV)
    try:
        assert dy.neutral_diffusion_tile() == (bx, by, i0)
        info = {}
        got, nex = _device(d, M, GV, P, opt, inp, dy=dy, info=info)
        ns = 2 * nk + 2
        planes8 = 5 * (nk + 1) + 2 * (2 * ns + 2 * (ns - 1)) + (4 * nk + 1) + 2 * (nk + 1)
        assert info["work_bytes"] == d.slab * (8 * planes8 + 2 * 2 * 2 * ns), info
        assert nex == 0
        _check(d, got, want, f"{edge}, poison {poison}")
    finally:
        dy.close()


@pytest.mark.parametrize("ntr", (1, 2, 9))
def test_tracer_counts(ntr):
    d, M, GV, P, opt, inp, want, _ = R.want("island_basin", 4, "underflow", ntr=ntr)
    got, nex = _device(d, M, GV, P, opt, inp)
    assert len(got["tracers"]) == ntr and nex == 0
    _check(d, got, want, f"ntr = {ntr}")


def test_two_calls_in_a_row_are_one():
    """Two calc_coeffs calls give the bits of one; so do two neutral_diffusion calls on fresh copies of the tracers (compared
    inside _device), in both orders of the additions."""
    for name in ("massless", "new_order"):
        d, M, GV, P, opt, inp, want, _ = R.want("island_basin", 4, name)
        got, nex = _device(d, M, GV, P, opt, inp, ncoeffs=2, ndiff=2)
        _check(d, got, want, name + " x 2")
        assert nex == 0


# -- tracer_hordiff_neutral ----------------------------------------------------------------------------------------------------

def _hordiff_case(d, M, itts, recalc):
    """(tracer_hor_diff params, neutral diffusion params, dt): KHTR such that CHECK_DIFFUSIVE_CFL finds `itts` iterations (the
    largest cell CFL is itts - 0.5)."""
    Pthd = abi.tracer_hor_diff_params_default(KHTR=1.0, check_diffusive_CFL=1 if itts > 1 else 0)
    if itts > 1:
        khx, khy = hordiff_ref.khdt_faces(d, M, Pthd, R.DT, {})
        Pthd.KhTr = (itts - 0.5) / float(hordiff_ref.cell_cfl(d, M, khx, khy).max())
    else:
        Pthd.KhTr = R.KHTR
    return Pthd, abi.neutral_diffusion_params_default(recalc_neutral_surf=int(recalc)), R.DT


def _registry(inp):
    """T and S inside the registry, as in the reference, with the three tracers behind them."""
    return [inp["T"], inp["S"]] + list(inp["tracers"])


def _hordiff_want(d, M, GV, Pthd, Pnd, eos, inp, dt, uf, **kw):
    tr = [x.copy() for x in _registry(inp)]
    ntr = len(tr)
    out = dict(tracers=tr, tendency=[np.full(d.shape3(), np.nan) if m != 1 else None for m in range(ntr)],
               trans_x_2d=[np.full(d.shape2(), np.nan) if m != 2 else None for m in range(ntr)],
               trans_y_2d=[np.full(d.shape2(), np.nan) for m in range(ntr)])
    rec = {}
    n = R.tracer_hordiff_neutral(d, M, GV, Pthd, Pnd, eos, inp["h"], dt, tr, tr[0], tr[1], inp.get("p_surf"), conc_underflow=uf,
                                 tendency=out["tendency"], trans_x_2d=out["trans_x_2d"], trans_y_2d=out["trans_y_2d"], record=rec, **kw)
    for p in "uv":
        for c in ("PoL", "PoR", "KoL", "KoR", "hEff"):
            out[p + c] = getattr(rec["CS"], p + c)
    return out, n, rec


def _hordiff_device(dy, d, Pthd, Pnd, eos, inp, dt, uf):
    import torch
    tr = [dy.to_dev(x) for x in _registry(inp)]
    ntr = len(tr)
    h = dy.to_dev(inp["h"])
    ps = dy.to_dev(inp["p_surf"]) if "p_surf" in inp else None
    nan3 = lambda: dy.to_dev(np.full(d.shape3(), np.nan))   # noqa: E731
    nan2 = lambda: dy.to_dev(np.full(d.shape2(), np.nan))   # noqa: E731
    o = dict(tendency=[nan3() if m != 1 else None for m in range(ntr)], trans_x_2d=[nan2() if m != 2 else None for m in range(ntr)],
             trans_y_2d=[nan2() for m in range(ntr)])
    dy.tracer_hor_diff_init(Pthd)
    dy.neutral_diffusion_init(Pnd, eos)
    torch.cuda.synchronize()
    dy.comm_exchange_count(reset=True)
    n = dy.tracer_hordiff_neutral(h, dt, tr, tr[0], tr[1], p_surf=ps, conc_underflow=uf, **o)
    dy.sync()
    nex = dy.comm_exchange_count()
    assert dy.neutral_diffusion_status() == (0, 0, 0, 0)
    cpu = lambda a: a.cpu().numpy() if a is not None else None   # noqa: E731
    out = dict(tracers=[cpu(x) for x in tr], **{k: [cpu(x) for x in v] for k, v in o.items()})
    for dir, p in ((0, "u"), (1, "v")):
        for c, a in dy.neutral_diffusion_coeffs(dir).items():
            out[p + c] = a.cpu().numpy()
    _bits(h.cpu().numpy(), inp["h"], "h is only read")
    return out, n, nex


def _hordiff_same(d, got, want, tag, interior_only=False):
    slu, slv, slh = H.interior(d, "u"), H.interior(d, "v"), H.interior(d, "h")
    k = (slice(None),)
    for p, sl in (("u", slu), ("v", slv)):
        for c in ("PoL", "PoR", "hEff"):
            _bits(got[p + c][k + sl], want[p + c][k + sl], f"{tag}: {p}{c}")
        for c in ("KoL", "KoR"):
            _ibits(got[p + c][k + sl], want[p + c][k + sl], f"{tag}: {p}{c}")
    for n, sl in (("tracers", slh), ("tendency", slh), ("trans_x_2d", slu), ("trans_y_2d", slv)):
        for m, (a, b) in enumerate(zip(got[n], want[n])):
            if b is None:
                assert a is None
            elif n == "tracers" and not interior_only:
                _bits(a, b, f"{tag}: {n}[{m}]")
            else:
                _bits(a[..., sl[0], sl[1]], b[..., sl[0], sl[1]], f"{tag}: {n}[{m}]")


@pytest.mark.parametrize("itts,recalc", [(1, 0), (3, 0), (3, 1)])
def test_tracer_hordiff_neutral(itts, recalc):
    """The neutral branch :479-539 with T and S inside the registry, on a closed basin with an island and on a torus (whose group
    pass moves data): one iteration, and three through CHECK_DIFFUSIVE_CFL with RECALC_NEUTRAL_SURF off and on."""
    from mom6_amd.dycore import Dycore
    GV = abi.vgrid_default()
    for grid, kw in (("island_basin", dict(nk=4)), ("torus", dict(nk=3, ni=24, nj=16))):
        d, M = getattr(H, grid)(**kw)[1:]
        P, opt = R.case("psurf")
        inp = R.case_inputs(d, M, GV, opt)
        eos = R.case_eos(opt)
        Pthd, Pnd, dt = _hordiff_case(d, M, itts, recalc)
        uf = [0.0, 0.0, 0.0, 1.9, 0.0]
        want, nw, rec = _hordiff_want(d, M, GV, Pthd, Pnd, eos, inp, dt, uf)
        assert nw == itts and rec["passes"] == itts and rec["calc_coeffs"] == (itts if recalc else 1)
        dy = Dycore(d, M, GV)
        try:
            got, ng, nex = _hordiff_device(dy, d, Pthd, Pnd, eos, inp, dt, uf)
        finally:
            dy.close()
        assert ng == nw
        _hordiff_same(d, got, want, f"{grid}: {itts} iterations, recalc {recalc}")
        assert not np.array_equal(got["tracers"][0], _registry(inp)[0])


def _run_tile(layout, pe, uid, args, out, errors):
    try:
        from mom6_amd import parallel
        from mom6_amd.dycore import Dycore
        GV = abi.vgrid_default()
        d1, inp1, Pthd, Pnd, eos, dt, uf = args
        d, M = H.benchmark_small(nk=3, layout=layout, pe=pe)[1:]
        inp = {n: ([R.cut(d1, d, x) for x in a] if isinstance(a, list) else R.cut(d1, d, a)) for n, a in inp1.items()}
        dy = Dycore(d, M, GV)
        try:
            if layout != (1, 1):
                parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
            out[pe] = _hordiff_device(dy, d, Pthd, Pnd, eos, inp, dt, uf) + (d,)
        finally:
            dy.close()
    except Exception:                                                 # noqa: BLE001 -- reported by the main thread
        import traceback
        errors.append((pe, traceback.format_exc()))


@pytest.mark.parametrize("layout", [(2, 1), (1, 2), (2, 2)])
def test_layouts_with_exchanges(layout):
    """The tiles of a layout as host threads on one GPU, three iterations with RECALC_NEUTRAL_SURF: every tile's interior equals
    its part of the one-tile result bit for bit, and every tile has made exactly num_itts group passes."""
    from mom6_amd import parallel
    lib = abi.load_library()
    GV = abi.vgrid_default()
    d1, M1 = H.benchmark_small(nk=3)[1:]
    P, opt = R.case("slope")
    inp1 = R.case_inputs(d1, M1, GV, opt)
    eos = R.case_eos(opt)
    Pthd, Pnd, dt = _hordiff_case(d1, M1, 3, 1)
    args = (d1, inp1, Pthd, Pnd, eos, dt, None)
    errors, ref, out = [], {}, {}
    _run_tile((1, 1), (0, 0), None, args, ref, errors)
    assert not errors, errors[0][1]
    one, n_one, _, _ = ref[(0, 0)]
    assert n_one == 3
    H.use_threads_transport(lib)
    try:
        uid = parallel.unique_id(lib)
        pes = [(px, py) for py in range(layout[1]) for px in range(layout[0])]
        threads = [threading.Thread(target=_run_tile, args=(layout, pe, uid, args, out, errors)) for pe in pes]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
    finally:
        H.use_threads_transport(lib, on=False)
    assert not errors, errors[0][1]
    assert len(out) == len(pes)
    for pe in pes:
        tile, n, nex, dt_ = out[pe]
        assert n == n_one and nex == n_one, (pe, n, nex)
        own = H.interior(dt_, "h")
        part = d1.sl(dt_.i_glob0, dt_.i_glob0 + dt_.ni - 1, dt_.j_glob0, dt_.j_glob0 + dt_.nj - 1)
        for name in ("tracers", "tendency"):
            for m, (a, b) in enumerate(zip(tile[name], one[name])):
                if b is not None:
                    _bits(a[..., own[0], own[1]], b[..., part[0], part[1]], f"{layout} tile {pe}: {name}[{m}]")


# -- refusals and the neighbour module -----------------------------------------------------------------------------------------

def test_refused_settings_and_error_paths():
    """Each refused setting is named; a refused init leaves no module behind, also after a good one; calls before init, and
    neutral_diffusion before the first calc_coeffs, fail with a message; the outputs stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = H.benchmark_small(nk=4)[1:]
    GV = abi.vgrid_default()
    P, opt = R.case("slope")
    eos = R.case_eos(opt)
    inp = R.case_inputs(d, M, GV, opt)
    dflt = abi.neutral_diffusion_params_default
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(inp[n]) for n in ("h", "T", "S")}
        tr = [dy.to_dev(x) for x in inp["tracers"]]
        cx, cy = (dy.to_dev(a) for a in R.coef_planes(d, M))
        torch.cuda.synchronize()
        with pytest.raises(abi.Mom6xError, match="error 1.*neutral_diffusion_init must be called first"):
            dy.neutral_diffusion_calc_coeffs(t["h"], t["T"], t["S"])
        with pytest.raises(abi.Mom6xError, match="error 1.*neutral_diffusion_init must be called first"):
            dy.neutral_diffusion(t["h"], cx, cy, R.DT, tr)
        words = dict(interior_only="NDIFF_INTERIOR_ONLY", tapering="NDIFF_TAPERING", KhTh_use_vert_struct="KHTR_USE_EBT_STRUCT",
                     use_unmasked_transport_bug="NDIFF_USE_UNMASKED_TRANSPORT_BUG")
        assert set(words) == set(abi.NEUTRAL_DIFFUSION_MUST_BE_0)
        bad = [(dflt(**{m: 1}), eos, w) for m, w in words.items()] + [(dflt(continuous_reconstruction=0), eos, "NDIFF_CONTINUOUS"),
                                                                       (dflt(), None, "equation of state")]
        for Pb, e, word in bad:
            assert R.refused(Pb, GV, e) == word
            with pytest.raises(abi.Mom6xError, match="error 3.*" + word):
                dy.neutral_diffusion_init(Pb, e)
            assert dy.neutral_diffusion_work_bytes() == 0
        dy.neutral_diffusion_init(P, eos)
        assert dy.neutral_diffusion_work_bytes() > 0
        with pytest.raises(abi.Mom6xError, match="error 1.*calc_coeffs must be called first"):
            dy.neutral_diffusion(t["h"], cx, cy, R.DT, tr)
        with pytest.raises(abi.Mom6xError, match="error 1.*tracer_hor_diff_init must be called"):
            dy.tracer_hordiff_neutral(t["h"], R.DT, tr, t["T"], t["S"])
        dy.neutral_diffusion_calc_coeffs(t["h"], t["T"], t["S"])
        with pytest.raises(abi.Mom6xError, match="error 1.*dt must be positive"):
            dy.neutral_diffusion(t["h"], cx, cy, 0.0, tr)
        with pytest.raises(abi.Mom6xError, match="error 1.*null h, T or S"):
            dy.neutral_diffusion_calc_coeffs(t["h"], None, t["S"])
        with pytest.raises(abi.Mom6xError, match="error 3.*NDIFF_TAPERING"):   # a refused init after a good one
            dy.neutral_diffusion_init(dflt(tapering=1), eos)
        assert dy.neutral_diffusion_work_bytes() == 0
        with pytest.raises(abi.Mom6xError, match="error 1.*neutral_diffusion_init must be called first"):
            dy.neutral_diffusion(t["h"], cx, cy, R.DT, tr)
        dy.tracer_hor_diff_init(abi.tracer_hor_diff_params_default(KHTR=1000.0))
        with pytest.raises(abi.Mom6xError, match="error 1.*neutral_diffusion_init must be called first"):
            dy.tracer_hordiff_neutral(t["h"], R.DT, tr, t["T"], t["S"])
        with pytest.raises(abi.Mom6xError, match="USE_NEUTRAL_DIFFUSION"):     # the along-layer init goes on refusing the flag
            dy.tracer_hor_diff_init(abi.tracer_hor_diff_params_default(KHTR=1000.0, use_neutral_diffusion=1))
        dy.sync()
        for m, x in enumerate(tr):
            _bits(x.cpu().numpy(), inp["tracers"][m], f"tracer {m} is as it was")
    finally:
        dy.close()
    # A non-Boussinesq context: mom6x_ctx_create refuses it by name, so there is no context on which neutral_diffusion_init's own
    # refusal of it could run (the restatement's refused() has the case); no module exists, and the library reports no bytes.
    GVn = abi.vgrid_default(); GVn.Boussinesq = 0
    assert R.refused(P, GVn, eos) == "non-Boussinesq"
    with pytest.raises(Exception, match="error 3.*BOUSSINESQ"):
        Dycore(d, M, GVn)
    assert abi.load_library().mom6x_neutral_diffusion_work_bytes(None) == 0


def test_tracer_hordiff_is_what_it_was_beside_the_module():
    """mom6x_tracer_hordiff before and after a neutral_diffusion_init (and a neutral call) on the same context: the same bits."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = H.island_basin(nk=4)[1:]
    GV = abi.vgrid_default()
    P, opt = R.case("slope")
    inp = R.case_inputs(d, M, GV, opt)
    Pthd = abi.tracer_hor_diff_params_default(KHTR=2000.0, max_diff_CFL=2.0)
    dy = Dycore(d, M, GV)
    try:
        h = dy.to_dev(inp["h"])
        dy.tracer_hor_diff_init(Pthd)

        def along():
            tr = [dy.to_dev(x) for x in _registry(inp)]
            df = [dy.to_dev(np.full(d.shape3(), np.nan)) for _ in range(2)]
            torch.cuda.synchronize()
            n = dy.tracer_hordiff(h, R.DT, tr, df_x=[df[0]] + [None] * 4, df_y=[df[1]] + [None] * 4)
            dy.sync()
            return n, [x.cpu().numpy() for x in tr + df]
        n0, before = along()
        dy.neutral_diffusion_init(P, R.case_eos(opt))
        tr = [dy.to_dev(x) for x in _registry(inp)]
        torch.cuda.synchronize()
        assert dy.tracer_hordiff_neutral(h, R.DT, tr, tr[0], tr[1]) == n0 == 2
        dy.sync()
        n1, after = along()
        assert n1 == n0
        for m, (a, b) in enumerate(zip(after, before)):
            _bits(a, b, f"tracer_hordiff after neutral_diffusion_init: array {m}")
    finally:
        dy.close()
