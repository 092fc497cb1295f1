"""mom6x_opacity_init and mom6x_set_pen_shortwave on the device (mom6_amd/csrc/opacity.hip) against the restatement
tests/opacity_ref.py.  Every output starts as NaN, so the halo the call must keep is checked too, and every input is compared with
what was uploaded.  The exact class of the case table (chlorophyll of 0 and 1, the chlorophyll-free schemes) bit for bit on whole
arrays with no tolerated signed zero, on a bowl at 1, 2 and 3 layers and a basin with an island at 4; the transcendental class
(smooth chlorophyll, and opac_diag everywhere) to 1e-12 of each field's range; launch edges; -0 planted; negative chlorophyll
counted; two calls in a row; refusals and error codes; the chain into mom6x_applyBoundaryFluxesInOut on the same pointers."""
import functools
import json
import os

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import opacity_ref as R
from tests import bflux_ref as B

pytestmark = pytest.mark.gpu
G = abi.G
CONFIGS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("island_basin", 4))
BOUND = 1.0e-12   # the project's bound for a transcendental site, as a fraction of the field's range


def _bits(a, b, name):
    H.assert_bitwise(a, b, name)                                  # bit patterns over the whole array; NaN words must be the same words


def _grid(grid, nk):
    return getattr(H, grid)(nk=nk)[1:]


class _Dy:
    """A Dycore for the length of a `with`."""
    def __init__(self, d, M, GV):
        from mom6_amd.dycore import Dycore
        self.dy = Dycore(d, M, GV)

    def __enter__(self):
        return self.dy

    def __exit__(self, *a):
        self.dy.close()


def _device(dy, d, P, opt, inp, ncalls=1, init=True):
    """mom6x_opacity_init, then `ncalls` times mom6x_set_pen_shortwave on outputs that start as NaN.  Returns the outputs as
    tests/opacity_ref.py run() does and the count of mom6x_opacity_status; the inputs are compared with what was uploaded."""
    import torch
    kw = R.call_args(opt, inp)
    scale = kw.pop("opacity_scale")
    ro = {n: dy.to_dev(a) for n, a in kw.items()}
    out = {n: dy.to_dev(a) for n, a in R.outputs(d, P, opt).items()}
    torch.cuda.synchronize()
    if init:
        dy.opacity_init(P)
    for _ in range(ncalls):
        dy.set_pen_shortwave(out["opacity_band"], out["sw_pen_band"], opacity_scale=scale, **ro,
                             **{n: a for n, a in out.items() if n in R._DIAG})
    neg = dy.opacity_status()
    assert dy.opacity_status() == 0                               # the count is since the last status call
    for n in ro:
        _bits(ro[n].cpu().numpy(), kw[n], n + " is only read")
    return {n: a.cpu().numpy() for n, a in out.items()}, neg


def _ratio(got, want, name):
    """The largest difference over the field's range (over its magnitude for a field that is one constant and so has no range);
    the finite points must be the same points."""
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), name
    rng = want[ok].max() - want[ok].min()
    if rng == 0.0:
        rng = np.abs(want[ok]).max()
    if rng == 0.0:
        _bits(got, want, name)
        return 0.0
    return float(np.abs(got[ok] - want[ok]).max() / rng)


def _check(d, got, want, tag, exact=True, worst=None):
    """Exact: every output but opac_diag bit for bit.  opac_diag, and everything of a transcendental case, to BOUND of range.
    The halo is still NaN and the computational domain finite."""
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    assert set(got) == set(want), (sorted(got), sorted(want))
    for n in want:
        if exact and n not in R.OUT_TRANSCENDENTAL:
            _bits(got[n], want[n], f"{tag}: {n}")
        else:
            r = _ratio(got[n], want[n], f"{tag}: {n}")
            if worst is not None:
                worst[f"{tag}:{n}"] = r
            assert r <= BOUND, (tag, n, r)
        assert np.isnan(got[n][..., ~own]).all() and np.isfinite(got[n][..., own]).all(), (tag, n)


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, ncalls=1):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    d, M = _grid(grid, nk)
    GV = abi.vgrid_default()
    P, opt = R.case(name)
    inp = R.case_inputs(d, M, opt)
    want, neg, counts = R.run(d, M, GV, P, opt, inp, ncalls=ncalls)
    return d, M, GV, P, opt, inp, want, neg, counts


@pytest.mark.parametrize("grid,nk", CONFIGS)
def test_exact_class_bit_for_bit(grid, nk):
    """Every case of the exact class, whole arrays.  At nk = 1, 2, 3 the walk over chl_3d runs with fewer layers than it loads
    ahead; at 4 with exactly as many."""
    d, M = _grid(grid, nk)
    with _Dy(d, M, abi.vgrid_default()) as dy:
        for name in R.CASES_EXACT:
            d, M, GV, P, opt, inp, want, neg, counts = _want(grid, nk, name)
            got, n = _device(dy, d, P, opt, inp)
            _check(d, got, want, f"{grid}/{nk}/{name}")
            assert n == neg == 0, name


def test_more_layers_than_the_walk_loads_ahead():
    """chl_3d at 9 layers: two full groups of the walk's look-ahead and one layer over."""
    for name in ("manizza_3", "morel_1", "ohlmann_1"):
        d, M, GV, P, opt, inp, want, neg, _ = _want("island_basin", 9, name)
        assert opt["chl"] == "3d"
        with _Dy(d, M, GV) as dy:
            got, n = _device(dy, d, P, opt, inp)
        _check(d, got, want, f"island_basin/9/{name}")


def test_transcendental_class_within_the_bound():
    """Smooth chlorophyll of 0.01 .. 20 mg m-3: the device's pow, log10 and tanh against numpy's, every field to 1e-12 of its
    range (the bound of tests/test_diabatic_aux_gpu.py, test_MEKE_gpu.py and test_set_diffusivity_gpu.py for a transcendental
    site).  The Ohlmann lookups are away from the half-integers (checked on the CPU), so both sides pick the same entry.  The
    largest ratios are recorded in profiles/set_opacity_transcendental.json (MOM6X_RECORD_SET_OPACITY names the file)."""
    worst = {}
    d, M = _grid("benchmark_small", 8)
    with _Dy(d, M, abi.vgrid_default()) as dy:
        for name in R.CASES_TRANSCENDENTAL:
            d, M, GV, P, opt, inp, want, neg, counts = _want("benchmark_small", 8, name)
            assert counts["ohlmann_near_half"] == 0
            got, n = _device(dy, d, P, opt, inp)
            for f in want:
                worst[f"{name}:{f}"] = _ratio(got[f], want[f], f"{name}: {f}")
            assert n == 0
    print("transcendental sites: largest difference / range:", worst)
    if os.environ.get("MOM6X_RECORD_SET_OPACITY"):
        json.dump(dict(case="benchmark_small x 8, tests/opacity_ref.py CASES_TRANSCENDENTAL", largest_difference_over_range=worst,
                       bound=BOUND), open(os.environ["MOM6X_RECORD_SET_OPACITY"], "w"), indent=1)
    for n, v in worst.items():
        assert v <= BOUND, (n, v)


def _edge_shapes():
    bx, by, _ = abi.lane_launch_shape()
    return [(bx, by), (bx + 1, by + 1), (2 * bx + 1, by), (1, by + 1)]


@pytest.mark.parametrize("ni,nj", _edge_shapes())
def test_launch_extents(ni, nj):
    """Land-free doubly re-entrant tiles whose extents are a whole number of work-groups and one more (a last work-group with one
    live lane, a last row of its own) and a tile one cell wide, three layers."""
    d, M = H.torus(nk=3, ni=ni, nj=nj)[1:]
    GV = abi.vgrid_default()
    with _Dy(d, M, GV) as dy:
        for name in ("manizza_7", "manizza_3", "morel_3", "ohlmann_1", "double_0", "single_0"):
            P, opt = R.case(name)
            inp = R.case_inputs(d, M, opt)
            want, neg, _ = R.run(d, M, GV, P, opt, inp)
            got, n = _device(dy, d, P, opt, inp)
            _check(d, got, want, f"torus {ni}x{nj}/{name}")
            assert n == 0


def test_negative_zero_planted():
    """-0 over blocks of sw and of the four band planes: no zero of opposite sign anywhere (the comparisons are on bit patterns)."""
    d, M = _grid("island_basin", 4)
    GV = abi.vgrid_default()
    seen = False
    with _Dy(d, M, GV) as dy:
        for name in ("manizza_7", "manizza_1", "manizza_folded", "morel_1", "morel_2", "ohlmann_0", "ohlmann_1", "double_0", "single_0"):
            P, opt = R.case(name)
            inp = R.case_inputs(d, M, opt)
            for m, n in enumerate(R.SW_NAMES):
                inp[n][d.sl(4 + 2 * m, 14 + 2 * m, 3 + m, 12 + m)] = -0.0
            want, neg, _ = R.run(d, M, GV, P, opt, inp)
            seen = seen or any(np.signbit(a[np.isfinite(a) & (a == 0.0)]).any() for a in want.values())
            got, n = _device(dy, d, P, opt, inp)
            _check(d, got, want, f"planted/{name}")
    assert seen


def _points(d, M):
    """Three wet points and one land point of the computational domain, as (j, i) indices into a plane."""
    own = np.zeros(d.shape2(), bool)
    own[H.interior(d, "h")] = True
    wet = M[G["mask2dT"]] > 0.0
    w, l = np.argwhere(own & wet), np.argwhere(own & ~wet)
    return [tuple(w[3]), tuple(w[len(w) // 2]), tuple(w[-2])], tuple(l[len(l) // 2])


def test_negative_chl_2d_is_counted_and_the_other_columns_are_untouched():
    """Three wet points and one land point with negative chl_2d: the status count is 3 and then 0 (inside _device), and every
    other column carries the bits of the run without them."""
    d, M, GV, P, opt, inp, want, _, _ = _want("island_basin", 4, "manizza_2")
    assert opt["chl"] == "2d"
    wetp, landp = _points(d, M)
    bad = dict(inp, chl_2d=inp["chl_2d"].copy())
    keep = np.ones(d.shape2(), bool)
    for p in wetp + [landp]:
        bad["chl_2d"][p] = -0.25
        keep[p] = False
    assert R.run(d, M, GV, P, opt, bad)[1] == 3
    with _Dy(d, M, GV) as dy:
        got, n = _device(dy, d, P, opt, bad)
    assert n == 3
    for f in want:
        _bits(got[f][..., keep], want[f][..., keep], f)
    assert np.isfinite(got["sw_pen_band"][:, ~keep]).all()            # MANIZZA_05's fluxes do not depend on the chlorophyll


def test_negative_chl_3d_is_counted_by_cell():
    d, M, GV, P, opt, inp, want, _, _ = _want("island_basin", 4, "manizza_3")
    assert opt["chl"] == "3d"
    wetp, landp = _points(d, M)
    bad = dict(inp, chl_3d=inp["chl_3d"].copy())
    keep = np.ones(d.shape2(), bool)
    for p, ks in zip(wetp + [landp], ((0, 1, 2, 3), (2,), (0, 3), (0, 1, 2, 3))):
        for k in ks:
            bad["chl_3d"][(k,) + p] = -0.25
        keep[p] = False
    assert R.run(d, M, GV, P, opt, bad)[1] == 7
    with _Dy(d, M, GV) as dy:
        got, n = _device(dy, d, P, opt, bad)
    assert n == 7
    for f in want:
        _bits(got[f][..., keep], want[f][..., keep], f)


def test_two_calls_in_a_row_give_the_bits_of_one():
    for name in ("manizza_0", "manizza_folded", "ohlmann_3", "double_1"):
        d, M, GV, P, opt, inp, want, _, _ = _want("island_basin", 4, name)
        with _Dy(d, M, GV) as dy:
            got, n = _device(dy, d, P, opt, inp, ncalls=2)
        _check(d, got, want, f"twice/{name}")


def test_no_bands_does_nothing():
    d, M = _grid("benchmark_small", 2)
    P, opt = R.case("manizza_0")
    P.nbands = 0
    inp = R.case_inputs(d, M, opt)
    with _Dy(d, M, abi.vgrid_default()) as dy:
        got, n = _device(dy, d, P, opt, inp)
    assert n == 0 and all(np.isnan(a).all() for a in got.values())


def test_refusals_and_error_codes():
    """A call before init; nbands 5 (unsupported, by name); OHLMANN_03 with 3 bands and the other band-count rules; both
    chlorophyll pointers; a scheme / chlorophyll mismatch either way; OHLMANN_03 without shortwave; a non-Boussinesq context.
    The outputs stay as they were."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = _grid("benchmark_small", 2)
    GV = abi.vgrid_default()
    dflt = abi.opacity_params_default
    inp = R.inputs(d, M)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        op, pen = dy.to_dev(np.full((4,) + d.shape3(), np.nan)), dy.to_dev(np.full((4,) + d.shape2(), np.nan))
        torch.cuda.synchronize()
        call = lambda **kw: dy.set_pen_shortwave(op, pen, **kw)
        with pytest.raises(Exception, match="error 1.*initialized"):
            call(sw=t["sw"], chl_2d=t["chl_2d"])
        with pytest.raises(Exception, match="error 1.*initialized"):
            dy.opacity_status()
        with pytest.raises(Exception, match="error 3.*more than 4 bands"):
            dy.opacity_init(dflt(nbands=5))
        with pytest.raises(Exception, match="error 1.*OHLMANN_03.*nbands==2"):
            dy.opacity_init(dflt(opacity_scheme=R.OHLMANN, nbands=3))
        with pytest.raises(Exception, match="error 1.*double_exp"):
            dy.opacity_init(dflt(opacity_scheme=R.DOUBLE_EXP, nbands=1))
        with pytest.raises(Exception, match="error 1.*single_exp"):
            dy.opacity_init(dflt(opacity_scheme=R.SINGLE_EXP, nbands=2))
        with pytest.raises(Exception, match="error 1.*not valid"):
            dy.opacity_init(dflt(opacity_scheme=0))
        with pytest.raises(Exception, match="error 1.*negative"):
            dy.opacity_init(dflt(nbands=-1))
        with pytest.raises(Exception, match="error 1.*initialized"):       # a refused init leaves no module behind
            call(sw=t["sw"], chl_2d=t["chl_2d"])
        dy.opacity_init(dflt(nbands=3))
        with pytest.raises(Exception, match="error 1.*both"):
            call(sw=t["sw"], chl_2d=t["chl_2d"], chl_3d=t["chl_3d"])
        with pytest.raises(Exception, match="error 1.*needs chl_2d or chl_3d"):
            call(sw=t["sw"])
        with pytest.raises(Exception, match="error 1.*opacity_band"):
            dy.set_pen_shortwave(None, pen, sw=t["sw"], chl_2d=t["chl_2d"])
        dy.opacity_init(dflt(opacity_scheme=R.DOUBLE_EXP, nbands=2, pen_sw_scale=10.0))
        with pytest.raises(Exception, match="error 1.*takes no chlorophyll"):
            call(sw=t["sw"], chl_2d=t["chl_2d"])
        dy.opacity_init(dflt(opacity_scheme=R.OHLMANN, nbands=2))
        with pytest.raises(Exception, match="error 1.*No shortwave input"):
            call(chl_2d=t["chl_2d"])
        with pytest.raises(Exception, match="error 1.*No shortwave input"):
            call(chl_2d=t["chl_2d"], sw_vis_dir=t["sw_vis_dir"], sw_vis_dif=t["sw_vis_dif"], sw_nir_dir=t["sw_nir_dir"])
        with pytest.raises(Exception, match="error 1.*No shortwave input"):   # the visible pair without the near-infrared one
            call(chl_2d=t["chl_2d"], sw=t["sw"], sw_vis_dir=t["sw_vis_dir"], sw_vis_dif=t["sw_vis_dif"])
        assert dy.opacity_status() == 0
        dy.sync()
        assert torch.isnan(op).all() and torch.isnan(pen).all()
    finally:
        dy.close()
    GV2 = abi.vgrid_default()
    GV2.Boussinesq = 0
    with pytest.raises(Exception, match="error 3.*BOUSSINESQ"):       # no such context exists for opacity_init to refuse
        Dycore(d, M, GV2)


def _chain(d, M, GV, Pa, eos, bopt, binp, Po, oopt, chl_2d):
    """opacity_ref feeding bflux_ref, and the device doing the same on device pointers: mom6x_set_pen_shortwave writes into two
    buffers that go unchanged, the same pointers, into mom6x_applyBoundaryFluxesInOut.  The buffers start as zeros.  Returns
    (want, got, the restatement's counts)."""
    import torch
    nsw = Po.nbands
    sw = binp["fluxes"]["sw"]
    opb, pen = np.zeros((nsw,) + d.shape3()), np.zeros((nsw,) + d.shape2())
    kw = dict(sw=sw, opacity_scale=GV.H_to_Z)
    if chl_2d is not None:
        kw["chl_2d"] = chl_2d
    R.set_pen_shortwave(d, M, R.init(Po, GV), opb, pen, **kw)
    binp = dict(binp, opacity_band=opb, sw_pen_band=pen)
    want, status, counts = B.run(d, M, GV, Pa, eos, bopt, binp)
    with _Dy(d, M, GV) as dy:
        st = {n: dy.to_dev(binp[n]) for n in ("h", "T", "S")}
        out = {n: dy.to_dev(a) for n, a in B.outputs(d, bopt).items()}
        fh = B.flux_planes(d, bopt, binp)
        f = {n: dy.to_dev(a) for n, a in fh.items()}
        o_dev, p_dev = dy.to_dev(np.zeros_like(opb)), dy.to_dev(np.zeros_like(pen))
        c_dev = dy.to_dev(chl_2d) if chl_2d is not None else None
        tsurf = dy.to_dev(binp["tv_p_surf"])
        torch.cuda.synchronize()
        dy.opacity_init(Po)
        dy.diabatic_aux_init(Pa, eos)
        dy.set_pen_shortwave(o_dev, p_dev, sw=f["sw"], chl_2d=c_dev, opacity_scale=GV.H_to_Z)
        dy.applyBoundaryFluxesInOut(bopt["dt"], f, st["h"], st["T"], st["S"], nsw=nsw, opacity_band=o_dev, sw_pen_band=p_dev,
                                    tv_p_surf=tsurf if bopt["p_surf"] else None, aggregate_FW_forcing=bopt["agg"],
                                    evap_CFL_limit=bopt["cfl"], minimum_forcing_depth=bopt["depth"], **out)
        assert dy.opacity_status() == 0 and dy.diabatic_aux_status() == status
        got = {n: a.cpu().numpy() for n, a in st.items()}
        got.update({n: a.cpu().numpy() for n, a in out.items()})
        got.update({"fluxes." + n: f[n].cpu().numpy() for n in bopt["fout"]})
        got["opacity_band"], got["sw_pen_band"] = o_dev.cpu().numpy(), p_dev.cpu().numpy()
    want = dict(want, opacity_band=opb, sw_pen_band=pen)
    return want, got, counts


def test_chain_double_exp_into_applyBoundaryFluxesInOut_bit_for_bit():
    """DOUBLE_EXP with e-folding scales of 1e-9 m: every layer's optical depth is 0 or beyond 750, the restatement of
    applyBoundaryFluxesInOut evaluates no exp that could differ, and the chain is bit for bit."""
    d, M = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    Pa, eos, bopt = B.case("linear_e", GV)
    bopt = dict(bopt, nsw=2)
    binp = B.case_inputs(d, M, GV, bopt, thin=False, dry=False)
    Po = abi.opacity_params_default(opacity_scheme=R.DOUBLE_EXP, nbands=2, pen_sw_scale=1.0e-9, pen_sw_scale_2nd=2.0e-9, sw_1st_exp_ratio=0.58)
    want, got, counts = _chain(d, M, GV, Pa, eos, bopt, binp, Po, None, None)
    assert counts["exp"] == 0
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], "chain DOUBLE_EXP: " + n)


def test_chain_manizza_into_applyBoundaryFluxesInOut_within_the_bound():
    """MANIZZA_05 with three bands and smooth chlorophyll: every field of the chain to 1e-12 of its range."""
    d, M = _grid("benchmark_small", 8)
    GV = abi.vgrid_default()
    Pa, eos, bopt = B.case("real_3", GV)
    binp = B.case_inputs(d, M, GV, bopt)
    Po = abi.opacity_params_default(nbands=3)
    chl = R.inputs(d, M, chl="smooth")["chl_2d"]
    want, got, counts = _chain(d, M, GV, Pa, eos, bopt, binp, Po, None, chl)
    assert counts["exp"] > 0
    assert set(got) == set(want)
    worst = {n: _ratio(got[n], want[n], "chain MANIZZA_05: " + n) for n in want}
    print("chain MANIZZA_05: largest difference / range:", worst)
    for n, v in worst.items():
        assert v <= BOUND, (n, v)
