"""mom6x_mixedlayer_restrat on the device (mom6_amd/csrc/mixed_layer_restrat.hip) against the restatement tests/mle_ref.py, bit for
bit and on whole arrays with no tolerated signed zero (every diagnostic starts as NaN, so the points the reference leaves alone are
checked too): every case with MLE_TAIL_DH = 0 on coasts, narrowed faces, vanished layers and an equator; every EOS form; layer
counts; a -0 planted in uhtr; consecutive calls that carry the filtered planes, also into a fresh context; 2 x 1, 1 x 2 and 2 x 2
tile cuts; the device's mu; refused settings and error paths; the chain from mom6x_thickness_diffuse on device pointers.  The one case
with MLE_TAIL_DH > 0 evaluates a pow and is held to the project's bound for its other pow site (tests/test_barotropic_gpu.py)."""
import functools

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import mle_ref as R
from tests.test_mixed_layer_restrat_cpu import GRIDS, MU_ARGS, REQUIRED, STAG, TILES, cut2
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
G = abi.G
INPUT_ONLY = ("T", "S", "ustar", "h_MLD", "Rd_dx_h", "mle_fl")


def _call(dy, t, P, dt, given, dg):
    dy.mixedlayer_restrat(t["h"], t["uhtr"], t["vhtr"], t["T"], t["S"], t["ustar"], dt, MLD_filtered=t["MLD_filtered"],
                          MLD_filtered_slow=t["MLD_filtered_slow"], **{n: t[n] for n in given}, **dg)


def _device(d, M, GV, P, inp, dt, eos, given, give_diag, fill=np.nan, ncalls=1, dy=None):
    """One mom6x_mixedlayer_restrat_init and `ncalls` mom6x_mixedlayer_restrat calls on inputs that live on the host; every
    diagnostic starts as `fill`.  Returns the state and the diagnostics of the last call.  In a context of its own, or in the
    caller's `dy`, which is then left open."""
    import torch
    from mom6_amd.dycore import Dycore
    own = dy is None
    if own:
        dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        dg = {n: dy.to_dev(a) for n, a in R.outputs(d, give_diag, fill).items()}
        dy.mixedlayer_restrat_init(P, eos)
        torch.cuda.synchronize()
        for _ in range(ncalls):
            _call(dy, t, P, dt, given, dg)
        dy.sync()
        for n in INPUT_ONLY:
            _bits(t[n].cpu().numpy(), inp[n], n + " is only read")
        out = {n: t[n].cpu().numpy() for n in R.STATE}
        out.update({n: a.cpu().numpy() for n, a in dg.items()})
        return out
    finally:
        if own:
            dy.close()


@functools.lru_cache(maxsize=None)
def _want(grid, nk, name, form, ncalls=1):
    """The restatement's result of a case on a grid, computed once and shared by the tests below (read only)."""
    from oracle import orc
    orc.build()
    d, M = GRIDS[grid](nk)
    GV = abi.vgrid_default()
    P, given, dg, dt = R.case(name, GV)
    eos = abi.eos_params_default(form)
    inp = R.inputs(d, M, GV)
    counts = dict.fromkeys(R.BRANCHES, 0)
    want = None
    for _ in range(ncalls):
        state = {n: want[n] for n in R.STATE} if want is not None else None
        want, _c = R.run(d, M, GV, P, inp, dt, eos, given=given, give_diag=dg, orc=orc, counts=counts, state=state)
    return d, M, GV, P, eos, given, dg, dt, inp, want, counts


def _both(grid, nk, name, form=abi.WRIGHT, tot=None):
    d, M, GV, P, eos, given, dg, dt, inp, want, counts = _want(grid, nk, name, form)
    got = _device(d, M, GV, P, inp, dt, eos, given, dg)
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], f"{grid}/{nk}/{name}/{form}:{n}")
    if tot is not None:
        for k, v in counts.items():
            tot[k] += v
    return d, inp, got


@pytest.mark.parametrize("grid", list(GRIDS))
def test_parity_with_the_restatement(grid):
    """Every case with MLE_TAIL_DH = 0 under WRIGHT at 8 and 75 layers, and the other seven EOS forms on the case that detects its
    mixed layer, whole arrays bit for bit: h outside the computational domain, uhtr | vhtr outside their faces and every diagnostic
    outside the reference's ranges keep what they held (NaN for the diagnostics).  The branches of the CPU test are counted again
    over what ran here."""
    tot = dict.fromkeys(R.BRANCHES, 0)
    for nk in (8, 75):
        for name in R.CASES_TAIL0:
            d, inp, got = _both(grid, nk, name, tot=tot)
            assert not np.array_equal(got["h"], inp["h"]) and np.isfinite(got["h"]).all()
            if "uhml" in got:
                for s in "uv":
                    face = np.zeros(d.shape2(), bool)
                    face[H.interior(d, s)] = True
                    assert np.isfinite(got[s + "hml"][:, face]).all() and np.isnan(got[s + "hml"][:, ~face]).all()
                    assert np.isfinite(got[s + "Dml"][face]).all() and np.isnan(got[s + "timescale"][~face]).all()
    for form in R.FORMS:
        if form != abi.WRIGHT:
            _both(grid, 8, "detect", form=form)
    print(f"{grid}: branch counts {tot}")
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)


@pytest.mark.parametrize("nk", [1, 2, 3, 76, 77, 120])
def test_layer_counts(nk):
    """Every walk is a loop over the layer count given at run time: one path for any nk, the counts around the on-chip solvers'
    bound (76) and beyond included; detect_mld's k = 2..nz loop does not run at all with one layer."""
    for name in ("detect", "both_filters", "front_plane"):
        _both("benchmark_small", nk, name)


def _planted():
    """The case "both_filters" with -0 planted in uhtr and vhtr over a block of whole columns (below the mixed layers and above
    them, at open faces and at land) and NaN at every point the routine must not touch: the halo of h beyond its first point, uhtr
    and vhtr outside their faces."""
    d, M, GV, P, eos, given, dg, dt, inp, _, _ = _want("benchmark_small", 8, "both_filters", abi.WRIGHT)
    inp = {n: a.copy() for n, a in inp.items()}
    blk = (slice(None),) + d.sl(-1, 14, 0, 11)
    inp["uhtr"][blk] = -0.0
    inp["vhtr"][blk] = -0.0
    read = np.zeros(d.shape2(), bool)
    read[H.interior(d, "h", extra=1)] = True
    inp["h"][:, ~read] = np.nan
    for s in "uv":
        face = np.zeros(d.shape2(), bool)
        face[H.interior(d, s)] = True
        inp[s + "htr"][:, ~face] = np.nan
    return d, M, GV, P, eos, given, dg, dt, inp, read


def test_negative_zero_in_uhtr_and_nan_at_untouched_points(orc):
    """uhtr = -0 stays -0 at a face whose uDml + uDml_slow is zero (:531: uhtr is not touched) and where both fluxes are negative
    (uhml = -0 below the mixed layers), and becomes +0 where +0*dt is added; all three happen in the planted block.  Points the
    routine must not read or write hold NaN before and after."""
    d, M, GV, P, eos, given, dg, dt, inp, read = _planted()
    want, _ = R.run(d, M, GV, P, inp, dt, eos, given=given, give_diag=dg, orc=orc)
    got = _device(d, M, GV, P, inp, dt, eos, given, dg)
    for n in want:
        _bits(got[n], want[n], "planted: " + n)
    blk = (slice(None),) + d.sl(-1, 14, 0, 11)
    z = got["uhtr"][blk]
    assert ((z == 0.0) & np.signbit(z)).any() and ((z == 0.0) & ~np.signbit(z)).any() and (z != 0.0).any()
    assert np.isnan(got["h"][:, ~read]).all() and np.isfinite(got["h"][(slice(None),) + H.interior(d, "h")]).all()


def test_three_calls_carry_the_filtered_planes():
    d, M, GV, P, eos, given, dg, dt, inp, want, _ = _want("island_basin", 8, "both_filters", abi.WRIGHT, ncalls=3)
    got = _device(d, M, GV, P, inp, dt, eos, given, False, ncalls=3)
    for n in R.STATE:
        _bits(got[n], want[n], "three calls: " + n)
    one = _want("island_basin", 8, "both_filters", abi.WRIGHT)[9]
    assert not np.array_equal(one["MLD_filtered"], want["MLD_filtered"])


def test_filtered_planes_restart_a_fresh_context():
    """Two calls, the state and the two filtered planes (the restart fields) copied to a fresh context, and two more calls equal
    four calls in one context: the context keeps nothing between calls."""
    d, M, GV, P, eos, given, dg, dt, inp, _, _ = _want("benchmark_small", 8, "both_filters", abi.WRIGHT)
    four = _device(d, M, GV, P, inp, dt, eos, given, False, ncalls=4)
    two = _device(d, M, GV, P, inp, dt, eos, given, False, ncalls=2)
    again = _device(d, M, GV, P, dict(inp, **{n: two[n] for n in R.STATE}), dt, eos, given, False, ncalls=2)
    for n in R.STATE:
        _bits(again[n], four[n], "2 + 2 calls: " + n)
    want = _want("benchmark_small", 8, "both_filters", abi.WRIGHT, ncalls=4)[9]
    for n in R.STATE:
        _bits(four[n], want[n], "four calls: " + n)


@functools.lru_cache(maxsize=None)
def _one_tile_device(name):
    d, M, GV, P, eos, given, dg, dt, inp, _, _ = _want("benchmark_small", 8, name, abi.WRIGHT)
    return _device(d, M, GV, P, inp, dt, eos, given, dg)


@pytest.mark.parametrize("layout,pe", TILES)
def test_tile_cuts(layout, pe, orc):
    """Each tile of a 2 x 1, of a 1 x 2 and of a 2 x 2 layout, called on its cut of the inputs with the filtered planes cut from the one-tile
    state: whole arrays bit for bit against the restatement on the same tile, and its own points equal to the one-tile result of
    the device, the filtered planes and the h-point diagnostics one point into the halo."""
    name = "both_filters"
    GV = abi.vgrid_default()
    d, M, _, P, eos, given, dg, dt, inp, _, _ = _want("benchmark_small", 8, name, abi.WRIGHT)
    one = _one_tile_device(name)
    dt_, Mt = GRIDS["benchmark_small"](8, layout=layout, pe=pe)
    tin = R.inputs(dt_, Mt, GV)
    for n in ("MLD_filtered", "MLD_filtered_slow"):
        slt, slg = cut2(d, dt_, "h", extra=1)
        tin[n] = np.full(dt_.shape2(), np.nan)
        tin[n][slt] = inp[n][slg]
    want, _ = R.run(dt_, Mt, GV, P, tin, dt, eos, given=given, give_diag=dg, orc=orc)
    tile = _device(dt_, Mt, GV, P, tin, dt, eos, given, dg)
    for n in want:
        _bits(tile[n], want[n], f"tile {layout} {pe}:{n} against the restatement")
        slt, slg = cut2(d, dt_, STAG.get(n, "h"), extra=0 if n in STAG else 1)
        _bits(tile[n][..., slt[0], slt[1]], one[n][..., slg[0], slg[1]], f"tile {layout} {pe}:{n} against one tile")


def test_mu_at_the_reference_arguments():
    """The ten values of mixedlayer_restrat_unit_tests (:2023-2042) from the device's mu, exactly or within epsilon as the reference
    states them."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = GRIDS["benchmark_small"](2)
    dy = Dycore(d, M, abi.vgrid_default())
    try:
        sig = dy.to_dev(np.array([a[0] for a in MU_ARGS]))
        dh = dy.to_dev(np.array([a[1] for a in MU_ARGS]))
        out = dy.to_dev(np.full(len(MU_ARGS), np.nan))
        torch.cuda.synchronize()
        dy.mixedlayer_restrat_mu(sig, dh, out)
        dy.sync()
        got = out.cpu().numpy()
    finally:
        dy.close()
    for (s, h_, true, tol), g in zip(MU_ARGS, got):
        assert abs(g - true) <= tol, (s, h_, g, true)
    tail0 = np.array([a[1] == 0.0 for a in MU_ARGS])
    _bits(got[tail0], np.array([float(R.mu(a[0], a[1])) for a in MU_ARGS])[tail0], "mu with MLE_TAIL_DH = 0")


def test_off_and_refused_settings():
    """Each `must be 0` member raises at init with a message naming the setting, as do a missing equation of state and a missing
    source of the mixed-layer depth (the reference's own fatal errors); at the call a missing h_MLD, Rd_dx_h or filtered plane is
    an error that names the field; with both coefficients zero no transport is made and h, uhtr, vhtr keep their bits."""
    import torch
    from mom6_amd.dycore import Dycore
    d, M = GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    inp = R.inputs(d, M, GV)
    eos = abi.eos_params_default()
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        words = dict(use_Bodner="BODNER", nkml="bulk mixed layer", use_Stanley_ML="STANLEY", non_Boussinesq="Boussinesq",
                     open_bcs="open boundary", debug="DEBUG")
        assert set(words) == set(abi.MIXEDLAYER_RESTRAT_MUST_BE_0)
        for member, word in words.items():
            with pytest.raises(Exception, match=word):
                dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, **{member: 1}), eos)
        with pytest.raises(Exception, match="equation of state"):
            dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV), None)
        with pytest.raises(Exception, match="No MLD to use"):
            dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, MLE_density_diff=0.0), eos)
        with pytest.raises(Exception, match="initialized"):
            dy.mixedlayer_restrat(t["h"], t["uhtr"], t["vhtr"], t["T"], t["S"], t["ustar"], 3600.0)
        args = (t["h"], t["uhtr"], t["vhtr"], t["T"], t["S"], t["ustar"], 3600.0)
        torch.cuda.synchronize()
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, **R.PBL), eos)
        with pytest.raises(Exception, match="h_MLD"):
            dy.mixedlayer_restrat(*args)
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, front_length=500.0), eos)
        with pytest.raises(Exception, match="Rd_dx_h"):
            dy.mixedlayer_restrat(*args)
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV), eos)
        with pytest.raises(Exception, match="Rd_dx_h"):
            dy.mixedlayer_restrat(*args, mle_fl=t["mle_fl"])
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, MLE_MLD_decay_time=86400.0), eos)
        with pytest.raises(Exception, match="MLD_filtered"):
            dy.mixedlayer_restrat(*args)
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, MLE_MLD_decay_time2=86400.0), eos)
        with pytest.raises(Exception, match="MLD_filtered_slow"):
            dy.mixedlayer_restrat(*args, MLD_filtered=t["MLD_filtered"])
        dy.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV), eos)      # both coefficients 0 (the defaults)
        dy.mixedlayer_restrat(*args)
        dy.sync()
        for n in ("h", "uhtr", "vhtr"):
            _bits(t[n].cpu().numpy(), inp[n], "coefficients 0: " + n)
    finally:
        dy.close()


def test_chain_from_thickness_diffuse(orc):
    """benchmark_small x 8, WRIGHT: mom6x_thickness_diffuse and mom6x_mixedlayer_restrat on the same device arrays h, uhtr, vhtr, one
    after the other as step_MOM_dynamics calls them (MOM.F90:1388, :1422), nothing passing through the host in between; against
    tests/thickdiff_ref.py followed by tests/mle_ref.py, bit for bit."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests import thickdiff_ref
    d, M = GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    eos = abi.eos_params_default(abi.WRIGHT)
    inp = R.inputs(d, M, GV)
    P, given, _, dt = R.case("both_filters", GV)
    Ptd = abi.thickness_diffuse_params_default()
    w = {n: inp[n].copy() for n in R.STATE}
    thickdiff_ref.thickness_diffuse(d, M, GV, Ptd, w["h"], w["uhtr"], w["vhtr"], dt, T=inp["T"], S=inp["S"], eos=eos, orc=orc)
    mid = w["h"].copy()
    want, _ = R.run(d, M, GV, P, inp, dt, eos, given=given, orc=orc, state=w)
    assert not np.array_equal(mid, inp["h"]) and not np.array_equal(want["h"], mid)
    dy = Dycore(d, M, GV)
    try:
        t = {n: dy.to_dev(a) for n, a in inp.items()}
        dy.thickness_diffuse_init(Ptd, eos)
        dy.mixedlayer_restrat_init(P, eos)
        torch.cuda.synchronize()
        dy.thickness_diffuse(t["h"], t["uhtr"], t["vhtr"], dt, T=t["T"], S=t["S"])
        _call(dy, t, P, dt, given, {})
        dy.sync()
        for n in R.STATE:
            _bits(t[n].cpu().numpy(), want[n], "chain: " + n)
    finally:
        dy.close()


def test_tail_uses_a_pow_and_is_held_to_a_tolerance():
    """MLE_TAIL_DH = 0.5: mu raises to the power 2 through pow (:744), the device's and libm's may differ in the last bit, as at
    btstep's one site: h, uhtr, vhtr, uhml, vhml within 1e-12 of each field's range (the bound of tests/test_barotropic_gpu.py).
    Largest differences seen, relative to the range, on benchmark_small x 8: see profiles/mixedlayer_restrat_pow.json."""
    d, M, GV, P, eos, given, dg, dt, inp, want, _ = _want("benchmark_small", 8, "tail", abi.WRIGHT)
    got = _device(d, M, GV, P, inp, dt, eos, given, dg)
    assert set(got) == set(want)
    worst = {}
    for n in ("h", "uhtr", "vhtr", "uhml", "vhml"):
        ok = np.isfinite(want[n])
        assert np.array_equal(np.isfinite(got[n]), ok)
        rng = want[n][ok].max() - want[n][ok].min()
        worst[n] = float(np.abs(got[n][ok] - want[n][ok]).max() / rng)
    print("tail: largest difference / range:", worst)
    for n, v in worst.items():
        assert v <= 1.0e-12, (n, v)
