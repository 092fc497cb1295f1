"""mom6x_kappa_shear_init and mom6x_Calculate_kappa_shear on the device (mom6_amd/csrc/kappa_shear.hip) against the restatement
tests/kappa_shear_ref.py, whole arrays bit for bit: the arithmetic is + - * / and sqrt, there is no tolerance class.  Every output
starts as NaN and the halo of every input is NaN (u and v keep the one face to the west and south); afterwards the outputs' halos
are still NaN, their interiors finite, and the inputs are what was uploaded.  Every case of the table at 1, 2, 3, 4 and 8 layers on
a bowl and at 4 on a basin with an island, the case `shear` at 75; slots of the workspace reused on a poisoned workspace, evenly
and at the launch-shape edges (lanes of one wavefront that walk unequal numbers of columns, a work_columns that is no multiple of
64, a column count that is none, fewer columns than a wavefront, 75 layers with reuse); two calls; the chain into
mom6x_set_diffusivity; two tiles; the refusals.  The restatement is held to the reference's own compiled MOM_kappa_shear.F90 by
tests/test_ref_parity_cpu.py, and the device to its recorded results by tests/test_ref_parity_gpu.py;
tests/test_kappa_shear_cpu.py screens the restatement without it."""
import functools
import threading

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import kappa_shear_ref as R
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 4), ("benchmark_small", 8),
           ("island_basin", 4))
IN3 = ("u", "v", "h", "T", "S")
IN2 = ("p_surf",)


def _grid(grid, nk, layout=(1, 1), pe=(0, 0), **kw):
    return getattr(H, grid)(nk=nk, layout=layout, pe=pe, **kw)[1:]


def _nan_halo(d, inp):
    """NaN in the halos of every input: nothing outside the computational domain may be read (u and v keep the one face to the
    west and south that find_uv_at_h reads)."""
    inp = dict(inp)
    own = np.zeros(d.shape2(), bool); own[H.interior(d, "h")] = True
    ownu = np.zeros(d.shape2(), bool); ownu[H.interior(d, "u")] = True
    ownv = np.zeros(d.shape2(), bool); ownv[H.interior(d, "v")] = True
    for n in IN3 + IN2:
        if n in inp:
            m = ownu if n == "u" else ownv if n == "v" else own
            inp[n] = np.where(m, inp[n], np.nan)
    return inp


def _device(d, M, GV, P, opt, inp, fill=np.nan, ncalls=1, layout=None, pe=None, uid=None, work_columns=None, info=None):
    """One mom6x_kappa_shear_init, then `ncalls` calls on the same device arrays.  Returns the outputs by name and the exchanges
    made; the inputs are compared with what was uploaded.  info: a dict that gets work_bytes, what kappa_shear_work_bytes reports."""
    import torch
    from mom6_amd import parallel
    from mom6_amd.dycore import Dycore
    dy = Dycore(d, M, GV)
    try:
        if layout is not None:
            parallel.attach_comm(dy, layout, pe, None, unique_id=uid)
        layered = opt["eos"] is None
        t = {n: dy.to_dev(inp[n]) for n in IN3 + IN2 if n in inp and not (layered and n in ("T", "S"))}
        out = {n: dy.to_dev(a) for n, a in R.outputs(d, opt, fill).items()}
        if work_columns is not None:
            P2 = abi.KappaShearParams.from_buffer_copy(P); P2.work_columns = work_columns
        else:
            P2 = P
        dy.kappa_shear_init(P2, R.case_eos(opt), inp["Rlay"] if layered else None)
        if info is not None:
            info["work_bytes"] = dy.kappa_shear_work_bytes()
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        for _ in range(ncalls):
            dy.Calculate_kappa_shear(t["u"], t["v"], t["h"], opt["dt"], out["kappa_io"], out["tke_io"], out["kv_io"], T=t.get("T"),
                                     S=t.get("S"), p_surf=t.get("p_surf"), zero_mix=opt["zero_mix"],
                                     **{n: out[n] for n in opt["diag"]})
        dy.sync()
        nex = dy.comm_exchange_count()
        for n in t:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        return {n: a.cpu().numpy() for n, a in out.items()}, nex
    finally:
        dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, **kw):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    d, M = _grid(grid, nk, **kw)
    GV = abi.vgrid_default()
    P, opt = R.case(name, GV)
    inp = _nan_halo(d, R.case_inputs(d, M, GV, opt))
    want, counts = R.run(d, M, GV, P, opt, inp)
    return d, M, GV, P, opt, inp, want, counts


def _check(d, got, want, tag):
    assert set(got) == set(want), (sorted(got), sorted(want))
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    for n in want:
        _bits(got[n], want[n], f"{tag}: {n}")
        assert np.isnan(got[n][..., halo]).all(), (tag, n)
        assert np.isfinite(got[n][..., ~halo]).all(), (tag, n)


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_every_case_bit_for_bit(grid, nk):
    """Whole arrays.  nk = 1 has no interior interface and nzc = 1, nk = 2 is the first with one, nk = 3 the first that enters the
    h_Int loop :1097."""
    for name in R.CASES:
        d, M, GV, P, opt, inp, want, counts = _want(grid, nk, name)
        got, nex = _device(d, M, GV, P, opt, inp)
        _check(d, got, want, f"{grid}/{nk}/{name}")
        assert nex == 0


def test_the_arms_of_the_cpu_list_are_reached_by_what_ran():
    from tests.test_kappa_shear_cpu import REQUIRED
    tot = R.new_counts()
    for grid, nk in CONFIGS:
        for name in R.CASES:
            for k, v in _want(grid, nk, name)[7].items():
                tot[k] += v
    print("branch counts", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)


def test_the_shear_case_at_75_layers():
    d, M, GV, P, opt, inp, want, counts = _want("benchmark_small", 75, "shear", ni=20, nj=12)
    assert counts["pred_corr"] > 0 and counts["two_iterations"] > 0 and counts["merged"] > 0
    got, _ = _device(d, M, GV, P, opt, inp)
    _check(d, got, want, "benchmark_small 20 x 12/75/shear")


def test_a_slot_is_reused_without_a_trace_of_its_previous_column(monkeypatch):
    """960 columns through one wavefront's worth of slots (15 columns a slot) give the bits of the default, one slot a column; and
    again on a workspace that starts as NaN: a slot's previous column does not leak into the next."""
    for name in ("shear", "nkml2"):
        d, M, GV, P, opt, inp, want, counts = _want("benchmark_small", 8, name)
        assert d.ni * d.nj == 960 and counts["merged"] > 0 and counts["pred_corr"] > 0
        for poison in ("0", "1"):
            monkeypatch.setenv("MOM6X_POISON_WORK", poison)
            got, _ = _device(d, M, GV, P, opt, inp, work_columns=64)
            _check(d, got, want, f"{name}: 64 slots, poison {poison}")
    monkeypatch.setenv("MOM6X_POISON_WORK", "1")
    d, M, GV, P, opt, inp, want, _ = _want("benchmark_small", 8, "shear")
    got, _ = _device(d, M, GV, P, opt, inp)
    _check(d, got, want, "shear: the default slots, poisoned")


def _edge_torus():
    from tests import ref_param as RP
    ni, nj = RP.edge_torus_shape()
    return dict(ni=ni, nj=nj)


# (grid, layers, keyword arguments of the grid, work_columns, the slots that makes, (columns, whole passes, busy lanes of the last pass))
LAUNCH_EDGES = {
    # 1008 columns through 64 slots: lanes 0..47 walk 16 columns and lanes 48..63 walk 15, so the last sixteen lanes of the only
    # wavefront have left the grid-stride loop while the others are still iterating
    "island_64": ("island_basin", 4, {}, 64, 64, (1008, 15, 48)),
    # work_columns = 65 rounds up to 128 slots (two wavefronts): 112 lanes walk 8 columns, the last 16 of the second wavefront 7
    "island_65": ("island_basin", 4, {}, 65, 128, (1008, 7, 112)),
    # the edge torus is (bx + 1) x (by + 1) = 65 x 5: 325 columns, no multiple of 64, rows of bx + 1; after five whole passes the
    # last pass has five busy lanes (the shape gives no pass with a single busy lane) beside 59 that are done
    "torus_64": ("torus", 3, _edge_torus, 64, 64, (325, 5, 5)),
    # fewer columns than a wavefront: 35 columns in the default slots, which round up to 64: one wavefront, 29 lanes never busy
    "bowl_7x5": ("benchmark_small", 4, dict(ni=7, nj=5), None, 64, (35, 0, 35)),
    # 75 layers with reuse: 240 columns through 64 slots, 48 lanes walk 4 and 16 walk 3, at the deepest K stride of the workspace
    "bowl_75": ("benchmark_small", 75, dict(ni=20, nj=12), 64, 64, (240, 3, 48)),
}


@pytest.mark.parametrize("poison", ("0", "1"))
@pytest.mark.parametrize("edge", sorted(LAUNCH_EDGES))
def test_launch_shape_edges(monkeypatch, edge, poison):
    """The case `shear` at the launch shapes of LAUNCH_EDGES, on a workspace that starts as zeros and as NaN, whole arrays bit for
    bit against the restatement (held to the compiled reference by tests/test_ref_parity_cpu.py) and, where a result of the
    reference is recorded for the grid (island basin x 4, torus x 3), against that too.  The shape a name stands for is asserted
    from the grid, the workspace reports the rounded slot count, and the restatement has mixing columns on the grid."""
    from tests import ref_param as RP
    grid, nk, kw, wc, slots, (ncol, whole, last) = LAUNCH_EDGES[edge]
    kw = kw() if callable(kw) else kw
    d, M, GV, P, opt, inp, want, counts = _want(grid, nk, "shear", **kw)
    assert d.ni * d.nj == ncol == whole * slots + last and 0 < last < slots, (d.ni, d.nj)
    assert (slots + 63) // 64 * 64 == slots and (wc is None or (wc + 63) // 64 * 64 == slots)
    assert counts["pred_corr"] > 0 and counts["two_iterations"] > 0, counts
    monkeypatch.setenv("MOM6X_POISON_WORK", poison)
    info = {}
    got, nex = _device(d, M, GV, P, opt, inp, work_columns=wc, info=info)
    assert info["work_bytes"] == 51 * (nk + 1) * slots * 8, (info, slots)
    assert nex == 0
    _check(d, got, want, f"{edge}, poison {poison}")
    cfg = ("kshear", "shear", grid, dict(kw, nk=nk))
    if cfg in RP.golden_configs():
        gold = RP.load_golden(*cfg, M, RP.golden_setup(*cfg)[5])
        for n, b in gold.items():
            _bits(np.ascontiguousarray(got[n][(Ellipsis,) + RP.dom(d)]), b, f"{edge}, poison {poison}: {n} against the recorded reference")


def test_two_calls_in_a_row_are_one():
    for name in ("shear", "layered"):
        d, M, GV, P, opt, inp, want, _ = _want("island_basin", 4, name)
        got, nex = _device(d, M, GV, P, opt, inp, ncalls=2)
        _check(d, got, want, name + " x 2")
        assert nex == 0


def test_chain_into_set_diffusivity():
    """mom6x_Calculate_kappa_shear, then mom6x_set_BBL_TKE and mom6x_set_diffusivity with use_Kd_shear on the same device pointers,
    against tests/setdiff_ref.py fed the restatement's Kd_shear; visc%Kv_shear passes through set_diffusivity untouched."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import setdiff_ref
    d, M, GV, P, opt, inp, want, counts = _want("benchmark_small", 8, "shear")
    Psd, eos, osd = setdiff_ref.case("shear", GV)
    assert Psd.use_Kd_shear and "Kd_shear" in osd["given"]
    sdi = dict(setdiff_ref.inputs(d, M, GV, **osd["inp"]), u=inp["u"], v=inp["v"], h=inp["h"], T=inp["T"], S=inp["S"],
               p_surf=inp["p_surf"], Kd_shear=want["kappa_io"])
    sd_want, _ = setdiff_ref.run(d, M, GV, Psd, eos, osd, sdi)
    base, _ = setdiff_ref.run(d, M, GV, Psd, eos, osd, dict(sdi, Kd_shear=np.zeros_like(want["kappa_io"])))
    own = np.zeros(d.shape2(), bool); own[H.interior(d, "h")] = True
    assert not np.array_equal(base["Kd_int"][:, own], sd_want["Kd_int"][:, own])
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(sdi[n]) for n in ("u", "v", "h", "T", "S", "p_surf") + tuple(setdiff_ref.VISC)}
        ks = {n: dy.to_dev(a) for n, a in R.outputs(d, opt).items()}
        sd = {n: dy.to_dev(a) for n, a in setdiff_ref.outputs(d, Psd, osd).items()}
        dy.kappa_shear_init(P, R.case_eos(opt))
        dy.set_diffusivity_init(Psd, eos)
        torch.cuda.synchronize()
        dy.comm_exchange_count(reset=True)
        dy.Calculate_kappa_shear(t["u"], t["v"], t["h"], opt["dt"], ks["kappa_io"], ks["tke_io"], ks["kv_io"], T=t["T"], S=t["S"],
                                 p_surf=t["p_surf"], zero_mix=opt["zero_mix"], **{n: ks[n] for n in opt["diag"]})
        dy.set_BBL_TKE(t["u"], t["v"], t["h"], *[t[n] for n in setdiff_ref.VISC], *[sd[n] for n in setdiff_ref.BBL_OUT])
        given = dict(Kd_shear=ks["kappa_io"], p_surf=t["p_surf"])
        outs = {n: (ks["kv_io"] if n == "Kv_shear" else sd[n]) for n in osd["out"]}
        dy.set_diffusivity(t["h"], osd["dt"], sd["Kd_int"], u=t["u"], v=t["v"], T=t["T"], S=t["S"], ustar_BBL=sd["ustar_BBL"],
                           BBL_meanKE_loss=sd["BBL_meanKE_loss"], **{n: given[n] for n in osd["given"]}, **outs)
        dy.sync()
        assert dy.comm_exchange_count() == 0
        for n in want:
            _bits(ks[n].cpu().numpy(), want[n], "chain: " + n)
        for n in sd_want:
            if n != "Kv_shear":
                _bits(sd[n].cpu().numpy(), sd_want[n], "chain: set_diffusivity " + n)
    finally:
        dy.close()


def test_two_by_one_tiles_as_host_threads_exchange_nothing():
    from mom6_amd import parallel
    lib = abi.load_library()
    layout = (2, 1)
    d, M, GV, P, opt, inp, want, _ = _want("benchmark_small", 8, "shear")
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


def test_refused_settings_and_error_paths():
    """VERTEX_SHEAR and a non-Boussinesq context are refused by name; a refused or invalid init leaves no module behind, also after
    a good one; the invalid values of init and of a call are errors; the outputs stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = _grid("benchmark_small", 4)
    GV = abi.vgrid_default()
    P, opt = R.case("shear", GV)
    eos = R.case_eos(opt)
    inp = R.case_inputs(d, M, GV, opt)
    dflt = abi.kappa_shear_params_default
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(inp[n]) for n in IN3 + IN2}
        o = [dy.to_dev(np.full(d.shape3(d.nk + 1), np.nan)) for _ in range(3)]
        torch.cuda.synchronize()

        def call(dt=3600.0, skip=(), out=o, **kw):
            a = {n: (None if n in skip else t[n]) for n in IN3}
            dy.Calculate_kappa_shear(a["u"], a["v"], a["h"], dt, out[0], out[1], out[2], T=a["T"], S=a["S"], **kw)
        with pytest.raises(Exception, match="initialized"):
            call()
        assert set(abi.KAPPA_SHEAR_MUST_BE_0) == {"KS_at_vertex"}
        with pytest.raises(Exception, match="error 3.*VERTEX_SHEAR"):
            dy.kappa_shear_init(dflt(GV, KS_at_vertex=1), eos)
        for bad, word in ((dict(max_KS_it=0), "MAX_KAPPA_SHEAR_IT"), (dict(max_RiNo_it=0), "MAX_RINO_IT"), (dict(RiNo_crit=0.0), "RINO_CRIT"),
                          (dict(kappa_src_max_chg=1.0), "KAPPA_SHEAR_MAX_KAP_SRC_CHG"), (dict(work_columns=-1), "work_columns")):
            with pytest.raises(Exception, match="error 1.*" + word):
                dy.kappa_shear_init(dflt(GV, **bad), eos)
        with pytest.raises(Exception, match="initialized"):       # a refused init leaves no module behind
            call()
        dy.kappa_shear_init(P, eos)
        assert dy.kappa_shear_work_bytes() == 51 * (d.nk + 1) * 960 * 8
        call()
        with pytest.raises(Exception, match="error 3.*VERTEX_SHEAR"):
            dy.kappa_shear_init(dflt(GV, KS_at_vertex=1), eos)
        with pytest.raises(Exception, match="initialized"):       # nor does a refused init after a good one
            call()
        assert dy.kappa_shear_work_bytes() == 0
        for x in o:
            x.fill_(float("nan"))
        torch.cuda.synchronize()
        dy.kappa_shear_init(P, eos)
        with pytest.raises(Exception, match="error 1.*dt must be positive"):
            call(dt=0.0)
        with pytest.raises(Exception, match="error 1.*together"):
            call(skip=("S",))
        with pytest.raises(Exception, match="error 1.*Rlay"):
            call(skip=("T", "S"))
        for n in ("u", "v", "h"):
            with pytest.raises(Exception, match="error 1.*null u, v or h"):
                call(skip=(n,))
        with pytest.raises(Exception, match="error 1.*kappa_io"):
            call(out=[o[0], None, o[2]])
        dy.kappa_shear_init(P, None, inp["Rlay"])
        with pytest.raises(Exception, match="error 1.*equation of state"):
            call()
        dy.sync()
        assert all(torch.isnan(x).all() for x in o)
    finally:
        dy.close()
    GVn = abi.vgrid_default(); GVn.Boussinesq = 0
    with pytest.raises(Exception, match="error 3.*BOUSSINESQ"):     # no such context exists for kappa_shear_init to refuse
        Dycore(d, M, GVn)
