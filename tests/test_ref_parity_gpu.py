"""mom6x_set_pen_shortwave, mom6x_energetic_PBL, mom6x_Calculate_kappa_shear, mom6x_neutral_diffusion_calc_coeffs with
mom6x_neutral_diffusion, mom6x_calc_slope_functions and mom6x_thickness_diffuse on the device against what the reference's own
compiled MOM_opacity.F90, MOM_energetic_PBL.F90, MOM_kappa_shear.F90, MOM_neutral_diffusion.F90, MOM_lateral_mixing_coeffs.F90 and
MOM_thickness_diffuse.F90 gave on the same seeded inputs:
the recorded results tests/golden/ref_opacity_*.npz, ref_epbl_*.npz, ref_kshear_*.npz, ref_ndiff_*.npz, ref_varmix_*.npz and
ref_thickdiff_*.npz
(scripts/record_ref_parity.py wrote them from oracle/_ref/libref_param.so; tests/test_ref_parity_cpu.py holds the restatements
and the live library to the same files).  Nothing here needs the compiled reference.

Exactly the recorded cases: manizza_3, morel_1 and ohlmann_1 on a basin with an island at 4 layers; croot_new and rh18_orig_tl (rh18_orig at a transition scale the reference's init accepts) on a
bowl at 3 and 8 layers; each of the five on a land-free torus one cell larger than a work-group in each direction.  Bit for bit on
the computational domain; opac_diag, a tanh, to the project's bound of 1e-12 of its range.  Every output starts as NaN and its halo
must still be NaN.  mstar_sfc and ustar_diag are compared at wet points, where the reference defines them; OBL_its reaches no
diagnostic of the reference and is not recorded.

Kind kshear: shear, bugs, nkml2, layered, newton and tie on the basin with an island at 4 layers, shear and nkml2 on the bowl at 8, shear
on the bowl at 2, shear and layered on the torus at 3.  The device is fed u and v (its own find_uv_at_h runs; the compiled routine
was handed the restatement's u_h, v_h) with NaN halos; kappa_io, tke_io, kv_io and the four 3-D diagnostics bit for bit, there is
no tolerance class; no halo exchange happens.  KS_its reaches no diagnostic of the reference and is not recorded.

Kind ndiff: every case of ndiff_ref.CASES on the basin with an island at 4 layers, slope on the bowl at 1 and at 2, slope and massless on
the bowl at 8, slope and new_order on the torus at 3, fed through _device of tests/test_neutral_diffusion_gpu.py (one init, one
calc_coeffs and one neutral_diffusion call) with that file's NaN-beyond-the-first-halo inputs.  Every tracer and its content tendency
on the computational domain, trans_x_2d and trans_y_2d on their face ranges, bit for bit: there is no tolerance class.  Every
diagnostic starts as NaN and is still NaN outside its range, the tracers keep the NaN of their outer halos; no exchange happens and
the status is (0, 0, 0, 0).  The coefficient arrays are private to the compiled module and are not recorded; the neutral branch of
tracer_hordiff and the discontinuous reconstruction are outside what was compiled.

Kinds varmix and thickdiff (ref_param.GOLDEN_VARMIX, GOLDEN_THICKDIFF): mom6x_calc_slope_functions and mom6x_thickness_diffuse against
the reference's own MOM_lateral_mixing_coeffs.F90 (with MOM_isopycnal_slopes.F90 and MOM_interface_heights.F90) and
MOM_thickness_diffuse.F90: every case on the basin with an island at 4 layers (khth2d excepted, whose plane the reference reads from
a file), eady and eos once per equation of state there; eady, visbeck, just_e and eos, noeos on the bowl at 1, 2 and 8 layers (at
one layer their layered twins: the reference's vert_fill_TS reads layer 2); eady_diag, visbeck_diag and eos, slopes_noeos on the
torus at 3; and the chain, one calc_slope_functions whose slopes one thickness_diffuse reads, on the bowl at 8.  Fed through
_device of tests/test_varmix_gpu.py and tests/test_thickness_diffuse_gpu.py with inputs that are NaN beyond what the reference
reads (ref_param.nan_beyond) and outputs that start as NaN: every output bit for bit on the range the reference writes
(ref_param.varmix_ranges, thickdiff_ranges) and NaN, or for h, uhtr and vhtr the input's bits, outside it; no halo exchange; status
0 (every call is checked).  There is no tolerance class.  tests/test_ref_parity_cpu.py asserts that these configurations by
themselves reach every arm of REQUIRED of tests/test_varmix_cpu.py and tests/test_thickness_diffuse_cpu.py."""
import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import opacity_ref
from tests import ref_param as RP

pytestmark = pytest.mark.gpu
G = abi.G
BOUND = 1.0e-12


def _ids():
    return [RP.golden_name(*c) for c in RP.golden_configs()]


def _compare(tag, kind, d, M, gold, got):
    dm = RP.dom(d)
    wet = (M[G["mask2dT"]] > 0.0)[dm]
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    names = set(got) - set(RP.EPBL_NOT_EXPOSED) - set(RP.KSHEAR_NOT_EXPOSED)
    if kind == "kshear":                 # (a file that would pass the size limit leaves out diagnostics)
        assert set(RP.KSHEAR_CORE) <= set(gold) <= names, (sorted(gold), sorted(got))
    else:
        assert set(gold) == names, (sorted(gold), sorted(got))
    for n, a in got.items():
        assert np.isnan(a[..., halo]).all() and np.isfinite(a[..., ~halo]).all(), (tag, n)
    for n, b in gold.items():
        a = np.ascontiguousarray(got[n][(Ellipsis,) + dm])
        if n in RP.EPBL_WET_ONLY:
            a, b = a[..., wet], b[..., wet]
        if n in opacity_ref.OUT_TRANSCENDENTAL:
            rng = float(b.max() - b.min()) or float(np.abs(b).max())
            r = float(np.abs(a - b).max() / rng)
            print(tag, n, "largest difference / range", r)
            assert r <= BOUND, (tag, n, r)
        else:
            H.assert_bitwise(a, np.ascontiguousarray(b), f"{tag}: {n}")


def _ndiff(tag, d, M, GV, P, opt, inp, gold):
    """The four outputs bit for bit on the ranges of test_neutral_diffusion_gpu._check; NaN outside them (the tracers: beyond the
    first halo, where the inputs hold NaN); no exchange; status (0, 0, 0, 0) (asserted inside _device)."""
    from tests.test_neutral_diffusion_gpu import _device
    got, nex = _device(d, M, GV, P, opt, inp)
    assert nex == 0
    assert set(RP.NDIFF_CORE) <= set(gold) <= set(RP.NDIFF_OUT), sorted(gold)
    rng = RP.ndiff_ranges(d)
    ring = np.ones(d.shape2(), bool); ring[H.interior(d, "h", extra=1)] = False
    for n in RP.NDIFF_OUT:
        inside = np.zeros(d.shape2(), bool); inside[rng[n]] = True
        for m, a in enumerate(got[n]):
            assert np.isfinite(a[..., inside]).all(), (tag, n, m)
            assert np.isnan(a[..., ring if n == "tracers" else ~inside]).all(), (tag, n, m)
    for n, recorded in gold.items():
        assert len(recorded) == len(got[n]) == len(inp["tracers"]), (tag, n)
        for m, (a, b) in enumerate(zip(got[n], recorded)):
            H.assert_bitwise(np.ascontiguousarray(a[(Ellipsis,) + rng[n]]), np.ascontiguousarray(b), f"{tag}: {n}[{m}]")


def _recorded(kind, name, gold, exposed):
    """CORE <= recorded <= exposed: a file that would pass the size limit leaves out diagnostics, never a core array."""
    core = set(RP.VARMIX_CORE if kind == "varmix" else RP.THICKDIFF_CORE) & set(exposed)
    assert core <= set(gold) <= set(exposed), (sorted(gold), sorted(exposed))


def _lateral(tag, kind, name, d, M, GV, P, opt, inp, gold):
    from mom6_amd.dycore import Dycore
    from tests import test_thickness_diffuse_gpu as TG, test_varmix_gpu as VG
    dy = Dycore(d, M, GV)
    try:
        dy.comm_exchange_count(reset=True)
        if kind == "varmix":
            got = VG._device(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"], give_diag=True, dy=dy)
            rng = RP.varmix_ranges(d, P)
        elif opt["chain"] is None:
            got = TG._device(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"], stored=opt["stored"], give_gm=True,
                             dy=dy)
            rng = {n: (slice(None),) + s for n, s in RP.thickdiff_ranges(d).items()}
        else:
            import torch
            Pv = opt["chain"]
            t = {n: dy.to_dev(inp[n]) for n in ("h", "uhtr", "vhtr", "T", "S")}
            g = {n: dy.to_dev(np.full(d.shape2() if n.startswith("SN") else d.shape3(d.nk + 1), np.nan)) for n in RP.VARMIX_MEMBERS}
            dy.varmix_init(Pv, opt["eos"], *abi.layer_densities(d.nk, Rho0=GV.Rho0, g_Earth=GV.g_Earth))
            dy.thickness_diffuse_init(P, opt["eos"])
            torch.cuda.synchronize()
            dy.calc_slope_functions(t["h"], opt["dt"], g["SN_u"], g["SN_v"], T=t["T"], S=t["S"], slope_x=g["slope_x"], slope_y=g["slope_y"])
            dy.thickness_diffuse(t["h"], t["uhtr"], t["vhtr"], opt["dt"], T=t["T"], S=t["S"], slope_x=g["slope_x"], slope_y=g["slope_y"])
            dy.sync()
            got = {n: a.cpu().numpy() for n, a in dict(g, h=t["h"], uhtr=t["uhtr"], vhtr=t["vhtr"]).items()}
            rng = dict({n: (slice(None),) + RP.thickdiff_ranges(d)[n] for n in RP.THICKDIFF_CORE},
                       **{n: RP.varmix_ranges(d, Pv)[n] for n in RP.VARMIX_MEMBERS})
        assert dy.comm_exchange_count() == 0
    finally:
        dy.close()
    _recorded(kind, name, gold, [n for n in got if n in rng])
    for n, a in got.items():
        inside = np.zeros(a.shape, bool)
        if n in rng:
            inside[rng[n]] = True
        assert np.isfinite(a[inside]).all(), (tag, n)
        if n in RP.THICKDIFF_CORE:           # changed in place: outside the range the input's bits, NaN included
            H.assert_bitwise(a[~inside], inp[n][~inside], f"{tag}: {n} outside its range")
        else:
            assert np.isnan(a[~inside]).all(), (tag, n)
    for n, b in gold.items():
        H.assert_bitwise(np.ascontiguousarray(got[n][rng[n]]), np.ascontiguousarray(b), f"{tag}: {n}")


@pytest.mark.parametrize("kind,name,grid,kw", RP.golden_configs(), ids=_ids())
def test_device_against_the_recorded_reference(kind, name, grid, kw):
    d, M, GV, P, opt, inp = RP.golden_setup(kind, name, grid, kw)
    gold = RP.load_golden(kind, name, grid, kw, M, inp)           # (the stored SHA-256 of every input is checked here)
    tag = RP.golden_name(kind, name, grid, kw)
    if kind == "opacity":
        from tests.test_opacity_gpu import _Dy, _device
        with _Dy(d, M, GV) as dy:
            got, neg = _device(dy, d, P, opt, inp)
        assert neg == 0
    elif kind == "ndiff":
        _ndiff(tag, d, M, GV, P, opt, inp, gold)
        return
    elif kind in ("varmix", "thickdiff"):
        _lateral(tag, kind, name, d, M, GV, P, opt, inp, gold)
        return
    elif kind == "kshear":
        from tests.test_kappa_shear_gpu import _device, _nan_halo
        got, nex = _device(d, M, GV, P, opt, _nan_halo(d, inp))
        assert nex == 0
    else:
        from tests.test_energetic_PBL_gpu import _device, _nan_halo
        got, nex = _device(d, M, GV, P, opt, _nan_halo(d, inp))
        assert nex == 0
    _compare(tag, kind, d, M, gold, got)
