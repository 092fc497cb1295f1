"""The python restatements under tests/ held to the reference's own compiled code (oracle/_ref/libref_param.so: MOM_EOS_Wright*.F90,
MOM_EOS_linear.F90, MOM_intrinsic_functions.F90, MOM_opacity.F90, MOM_energetic_PBL.F90, MOM_kappa_shear.F90,
MOM_neutral_diffusion.F90, MOM_isopycnal_slopes.F90, MOM_lateral_mixing_coeffs.F90 and MOM_thickness_diffuse.F90 with MOM_EOS.F90
and MOM_interface_heights.F90, built where they lie against interface stand-ins, see oracle/Makefile and tests/ref_param.py).  The restatements were written from the same reading of the Fortran as the
kernels they check, so a misread line sits in both; these tests are what involves the reference's code itself.

Classes.  EXACT: whole arrays bit for bit on the computational domain.  TOLERANCE: the sites whose value goes through an
intrinsic that two builds may round differently (tanh in opac_diag, pow and log10 of smooth chlorophyll, exp, log and pow of the
libm cases of ePBL), held to the project's bound of 1e-12 of each field's range.  No site had to move from the first class to
the second (see CHANGELOG.md).  MOM_kappa_shear has no second class: its arithmetic is + - * / and sqrt, and every word is EXACT.
Nor has MOM_neutral_diffusion: + - * / and compares around Wright's and the linear equation of state.  Of it the compiled module
hands out the tracers, their content tendencies and the two transports; its coefficient arrays (PoL, PoR, KoL, KoR, hEff) are
private and are held through those and through two probing tracers.  Outside the comparison stay the neutral branch of
tracer_hordiff (MOM_tracer_hor_diff.F90 is not compiled), the coefficient arrays themselves and the discontinuous reconstruction.

Without oracle/_ref every test that runs a door skips; the comparison of the restatements with the recorded results
(tests/golden/ref_opacity_*.npz, ref_epbl_*.npz, ref_kshear_*.npz, ref_ndiff_*.npz) never skips."""
import functools
import json
import os

import numpy as np
import pytest

from mom6_amd import abi
from tests import bflux_ref as B
from tests import epbl_ref as E
from tests import helpers as H
from tests import kappa_shear_ref as K
from tests import ndiff_ref as N
from tests import opacity_ref as R
from tests import ref_param as RP
from tests import thickdiff_ref as TD
from tests import varmix_ref as V
from tests.test_kappa_shear_cpu import CONFIGS as KSHEAR_GRIDS, REQUIRED as KSHEAR_REQUIRED, RESCALE_SETS, _DIM_OUT, rescaled
from tests.test_thickness_diffuse_cpu import GRIDS as LAT_GRIDS, REQUIRED as TD_REQUIRED, SCALE_CASES as TD_SCALE_CASES, scaled as td_scaled
from tests.test_varmix_cpu import REQUIRED as V_REQUIRED, SCALE_CASES as V_SCALE_CASES, scaled_varmix

G = abi.G
BOUND = 1.0e-12      # the project's bound for a transcendental site (BOUND of tests/test_opacity_gpu.py), as a fraction of the range
WORST = {}           # tolerance-class field -> the largest difference over range seen (profiles/ref_parity_libm.json)


def _need_lib():
    if RP.lib() is None:
        pytest.skip("oracle/_ref/libref_param.so is not built (needs the reference's sources and amdflang: make -C oracle ref)")


def _ratio(got, want, name):
    """The largest difference over the field's range (over its magnitude for a constant field)."""
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), name
    if want.size == 0:
        return 0.0
    rng = float(want.max() - want.min()) or float(np.abs(want).max())
    if rng == 0.0:
        H.assert_bitwise(got, want, name)
        return 0.0
    return float(np.abs(got - want).max() / rng)


def _held(got, want, name, exact):
    if exact:
        H.assert_bitwise(got, want, name)
    else:
        r = _ratio(got, want, name)
        WORST[name] = max(WORST.get(name, 0.0), r)
        assert r <= BOUND, (name, r)


# ------------------------------------------------------------------------------------------------------------------------------
# Wright, linear and the intrinsic functions

def _points(n=4000):
    """Over and beyond the fits' range, as test_unesco_and_roquet_against_the_compiled_reference: negative salinity, p = 0."""
    rng = np.random.default_rng(11)
    T = rng.uniform(-3.0, 42.0, n); S = rng.uniform(-1.0, 42.0, n); p = rng.uniform(0.0, 1.2e8, n)
    S[:50] = 0.0; p[50:100] = 0.0; T[100:120] = 0.0
    return T, S, p


@pytest.mark.parametrize("name", ["WRIGHT", "WRIGHT_FULL", "WRIGHT_REDUCED", "LINEAR"])
def test_wright_and_linear_against_the_compiled_reference(orc, name):
    """orc.eos_density, orc.eos_density_anomaly and orc.eos_density_derivs equal density_elem, density_anomaly_elem and
    calculate_density_derivs_elem of the reference's own file, and bflux_ref.specvol_derivs (with its hand-copied coefficient
    tables) equals calculate_specvol_derivs_elem, bit for bit at 4000 random points."""
    _need_lib()
    T, S, p = _points()
    n = T.size
    e = abi.eos_params_default(getattr(abi, name))
    if name == "LINEAR":
        e.dRho_dp = 4.5e-7
    for rho_ref in (0.0, 1035.0):
        ref = RP.eos_points(e, T, S, p, rho_ref)
        mine = np.array([orc.eos_density(e, T[i], S[i], p[i]) for i in range(n)])
        mine_a = np.array([orc.eos_density_anomaly(e, T[i], S[i], p[i], rho_ref) for i in range(n)])
        mine_d = np.array([orc.eos_density_derivs(e, T[i], S[i], p[i]) for i in range(n)])
        H.assert_bitwise(mine, ref["rho"], name + " density")
        H.assert_bitwise(mine_a, ref["rho_anom"], name + " density anomaly")
        H.assert_bitwise(mine_d[:, 0], ref["drho_dT"], name + " drho_dT"); H.assert_bitwise(mine_d[:, 1], ref["drho_dS"], name + " drho_dS")
        dSV_dT, dSV_dS = B.specvol_derivs(e, T, S, p)
        H.assert_bitwise(np.asarray(dSV_dT), ref["dSV_dT"], name + " dSV_dT"); H.assert_bitwise(np.asarray(dSV_dS), ref["dSV_dS"], name + " dSV_dS")
    assert ref["rho"].min() > 900.0 and ref["rho"].max() < 1120.0
    # the door's other outputs against each other: spec_vol_elem is the inverse of density_elem to rounding
    assert np.abs(ref["spv"] * ref["rho"] - 1.0).max() < 8 * np.finfo(float).eps


def _cuberoot_points():
    rng = np.random.default_rng(5)
    x = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.1e-308, 3e-310, 1.0, -1.0, 8.0, -27.0, 0.125, 1e-300, 1e300, -1e300,
         1.7976931348623157e308]
    x += list(10.0 ** rng.uniform(-300.0, 300.0, 3000) * rng.choice([-1.0, 1.0], 3000))
    x += list(rng.uniform(5e-324, 2.2e-308, 200))                 # subnormals
    x += list(np.ldexp(rng.uniform(0.5, 1.0, 600), rng.integers(-6, 7, 600)))   # every exponent modulo 3 near one
    return np.array(x)


def test_cuberoot_against_the_compiled_reference():
    """epbl_ref.cuberoot equals cuberoot of MOM_intrinsic_functions.F90 bit for bit: 0, -0, subnormals, 1e-300 .. 1e300, negatives."""
    _need_lib()
    x = _cuberoot_points()
    ref = RP.cuberoot(x)
    mine = np.array([E.cuberoot(float(v)) for v in x])
    H.assert_bitwise(mine, ref, "cuberoot")
    assert np.signbit(ref[1]) and ref[1] == 0.0 and not np.signbit(ref[0])
    c = RP.invcosh(np.array([1.0, 2.0, 1.0e8]))                     # the door into invcosh answers
    assert c[0] == 0.0 and abs(c[1] - np.arccosh(2.0)) < 1e-15 and abs(c[2] - np.arccosh(1.0e8)) < 1e-13


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_opacity

OPACITY_GRIDS = (("benchmark_small", 3), ("island_basin", 4))


def _compare_opacity(tag, d, want, got, exact):
    dm = (Ellipsis,) + RP.dom(d)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for n in want:
        _held(got[n][dm], want[n][dm], f"{tag}: {n}", exact and n not in R.OUT_TRANSCENDENTAL)


@pytest.mark.parametrize("grid,nk", OPACITY_GRIDS)
def test_opacity_exact_class_against_the_compiled_reference(grid, nk):
    """Every case of opacity_ref.CASES_EXACT: opacity_band, sw_pen_band, SW_pen and SW_vis_pen of opacity_init + set_opacity, whole
    arrays bit for bit; opac_diag (a tanh) to 1e-12 of its range."""
    _need_lib()
    d, M = getattr(H, grid)(nk=nk)[1:]
    GV = abi.vgrid_default()
    for name in R.CASES_EXACT:
        P, opt = R.case(name)
        inp = R.case_inputs(d, M, opt)
        want, neg, _ = R.run(d, M, GV, P, opt, inp)
        got, fatal = RP.opacity(d, M, GV, P, opt, inp)
        assert fatal == 0 and neg == 0, (name, fatal)
        _compare_opacity(f"{grid}/{nk}/{name}", d, want, got, True)


@pytest.mark.parametrize("grid,nk", OPACITY_GRIDS)
def test_opacity_transcendental_class_against_the_compiled_reference(grid, nk):
    """Smooth chlorophyll: numpy's pow, log10 and tanh against the Fortran runtime's, every field to 1e-12 of its range."""
    _need_lib()
    d, M = getattr(H, grid)(nk=nk)[1:]
    GV = abi.vgrid_default()
    for name in R.CASES_TRANSCENDENTAL:
        P, opt = R.case(name)
        inp = R.case_inputs(d, M, opt)
        want, neg, counts = R.run(d, M, GV, P, opt, inp)
        assert counts["ohlmann_near_half"] == 0
        got, fatal = RP.opacity(d, M, GV, P, opt, inp)
        assert fatal == 0
        _compare_opacity(f"{grid}/{nk}/{name}", d, want, got, False)


@pytest.mark.parametrize("grid,nk", OPACITY_GRIDS)
def test_opacity_with_Z_rescaled_against_the_compiled_reference(grid, nk):
    """The exact class with the Z unit rescaled by 2**-11 (Z_RESCALE_POWER through the reference's own unit_scaling_init; the
    members of the restatement's parameters in the rescaled unit, as tests/test_opacity_cpu.py::test_Z_rescaled_is_exact)."""
    _need_lib()
    s = 2.0 ** -11
    d, M = getattr(H, grid)(nk=nk)[1:]
    for name in R.CASES_EXACT:
        _, opt = R.case(name)
        Q = abi.opacity_params_default(**dict(R.CASES[name][0]))
        Q.pen_sw_scale *= s; Q.pen_sw_scale_2nd *= s; Q.opacity_land_value /= s; Q.Z_to_m = 1.0 / s; Q.m_to_Z = s
        for n in range(6):
            Q.manizza_coef[n] /= s; Q.morel_coef[n] *= s
        GV2 = abi.vgrid_default()
        GV2.H_to_Z = s; GV2.Z_to_H = 1.0 / s; GV2.dZ_subroundoff *= s
        inp = R.case_inputs(d, M, opt)
        want, _, _ = R.run(d, M, GV2, Q, opt, inp)
        got, fatal = RP.opacity(d, M, GV2, Q, opt, inp)
        assert fatal == 0, name
        _compare_opacity(f"{grid}/{nk}/{name} Z x 2**-11", d, want, got, True)


def test_opacity_init_refusals_are_the_references():
    """The band-count rules of opacity_init (:1151-1160) are FATAL in the reference where the restatement raises."""
    _need_lib()
    d, M = H.benchmark_small(nk=2)[1:]
    GV = abi.vgrid_default()
    for sch, nb in ((R.DOUBLE_EXP, 1), (R.DOUBLE_EXP, 3), (R.SINGLE_EXP, 2), (R.OHLMANN, 3), (R.OHLMANN, 1)):
        P = abi.opacity_params_default(opacity_scheme=sch, nbands=nb)
        with pytest.raises(ValueError):
            R.init(P, GV)
        opt = dict(given=(), chl=None, scale=1.0, diag=())
        got, fatal = RP.opacity(d, M, GV, P, opt, {})
        assert fatal >= 1 and got is None, (sch, nb)


@pytest.mark.parametrize("case,answer_date", [("linear_e", 99991231), ("wright_3", 99991231), ("linear_e", 20181231), ("wright_3", 20181231)])
def test_absorbRemainingSW_against_the_compiled_reference(case, answer_date):
    """bflux_ref.absorbRemainingSW row by row against absorbRemainingSW of MOM_opacity.F90 (:600-867), with the thicknesses and
    opacities of two cases of tests/bflux_ref.py in which no exp is reached (the opacity is 0 or 1e6 m-1), the TKE sink included,
    under both optics answer dates: T, Pen_SW_bnd and TKE bit for bit."""
    _need_lib()
    d, M = H.benchmark_small(nk=4)[1:]
    GV = abi.vgrid_default()
    P0, eos, opt = B.case(case, GV)
    inp = B.case_inputs(d, M, GV, opt)
    P = abi.diabatic_aux_params_default(GV, optics_answer_date=answer_date)
    nsw, dt = opt["nsw"], opt["dt"]
    dm = RP.dom(d)
    h = np.ascontiguousarray(inp["h"][(slice(None),) + dm])
    op = np.ascontiguousarray(inp["opacity_band"][(slice(None), slice(None)) + dm])
    Pen0 = np.maximum(inp["sw_pen_band"][(slice(None),) + dm], 0.0) * (dt / (GV.Rho0 * P.C_p))        # [C H]
    T0 = np.ascontiguousarray(inp["T"][(slice(None),) + dm])
    dSV = np.full(h.shape, 2.0e-4 / 1035.0) * (1.0 + 0.1 * np.cos(np.arange(h.shape[2]))[None, None, :])
    H_limit = float(max(GV.Angstrom_H, GV.H_subroundoff))
    counts = dict.fromkeys(B.BRANCHES, 0)
    T, Pen, TKE = T0.copy(), Pen0.copy(), np.zeros(h.shape)
    with np.errstate(all="ignore"):
        B.absorbRemainingSW(GV, P, h, op, nsw, dt, H_limit, T, Pen, TKE=TKE, dSV_dT=dSV, counts=counts)
    assert counts["exp"] == 0, counts
    assert np.abs(T - T0).max() > 0.0 and np.abs(TKE).max() > 0.0
    for j in range(h.shape[1]):
        Tj, Pj, Kj = T0[:, j].copy(), np.ascontiguousarray(Pen0[:, j]), np.zeros(h[:, j].shape)
        fatal = RP.absorbRemainingSW(GV, P, np.ascontiguousarray(h[:, j]), np.ascontiguousarray(op[:, :, j]), nsw, dt, H_limit, Tj, Pj,
                                     TKE=Kj, dSV_dT=np.ascontiguousarray(dSV[:, j]))
        assert fatal == 0
        H.assert_bitwise(T[:, j], Tj, f"{case} row {j}: T"); H.assert_bitwise(Pen[:, j], Pj, f"{case} row {j}: Pen_SW_bnd")
        H.assert_bitwise(TKE[:, j], Kj, f"{case} row {j}: TKE")


def test_sumSWoverBands_door_answers():
    """The door into sumSWoverBands (:873): the flux at the surface is the sum of the bands, it does not grow with depth, and with
    an opacity of 1e6 m-1 nothing is left below the first thick layer.  (The project has no restatement to hold to it.)"""
    _need_lib()
    GV = abi.vgrid_default()
    P = abi.diabatic_aux_params_default(GV)
    nk, ni, nsw = 4, 7, 2
    h = np.full((nk, ni), 10.0); h[0, ::2] = 1.0e-3
    op = np.full((nsw, nk, ni), 1.0e6); op[:, 0, ::2] = 0.0
    pen = np.stack([np.linspace(1.0e-3, 2.0e-3, ni), np.linspace(3.0e-3, 1.0e-3, ni)])
    net, fatal = RP.sumSWoverBands(GV, P, h, h.copy(), op, nsw, 3600.0, float(max(GV.Angstrom_H, GV.H_subroundoff)), pen)
    assert fatal == 0
    H.assert_bitwise(net[0], pen[0] + pen[1], "netPen at the surface")
    assert (np.diff(net, axis=0) <= 0.0).all() and (net[2:] == 0.0).all()
    H.assert_bitwise(net[1, ::2], net[0, ::2], "no absorption at zero opacity")


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_energetic_PBL

EPBL_GRIDS = (("benchmark_small", 1), ("benchmark_small", 2), ("benchmark_small", 3), ("benchmark_small", 8), ("island_basin", 4))


def _compare_epbl(tag, d, M, want, got, exact, keep=None):
    """Every output epbl_ref.outputs names but those the reference exposes through no diagnostic (OBL_its), on the computational
    domain (`keep`: on those of its columns); mstar_sfc and ustar_diag at wet points, where the reference sets them."""
    dm = RP.dom(d)
    wet = (M[G["mask2dT"]] > 0.0)[dm]
    assert set(got) == set(want) - set(RP.EPBL_NOT_EXPOSED), (sorted(got), sorted(want))
    for n in got:
        a, b = got[n][(Ellipsis,) + dm], want[n][(Ellipsis,) + dm]
        sel = np.ones(wet.shape, bool) if keep is None else keep.copy()
        if n in RP.EPBL_WET_ONLY:
            sel &= wet
        _held(a[..., sel], b[..., sel], f"{tag}: {n}", exact)


@pytest.mark.parametrize("grid,nk", EPBL_GRIDS)
def test_epbl_exact_class_against_the_compiled_reference(grid, nk):
    """Every case of epbl_ref.CASES_EXACT (the two-call case `guess` among them): Kd_int, the mixed-layer depth of
    energetic_PBL_get_MLD and every diagnostic the case names, bit for bit."""
    _need_lib()
    d, M = getattr(H, grid)(nk=nk)[1:]
    GV = abi.vgrid_default()
    ran = 0
    for name in E.CASES_EXACT:
        P, opt = E.case(name, GV)
        inp = E.case_inputs(d, M, GV, opt)
        m = E.Libm()
        want, _ = E.run(d, M, GV, P, opt, inp, math=m)
        assert m.counts == dict(exp=0, log=0, pow=0), name
        got, fatal = RP.energetic_PBL(d, M, GV, P, opt, inp)
        if E.reference_refuses(P):          # rh18_orig, translay1: the reference's init stops; their twins rh18_orig_tl, translay_hi run
            assert fatal > 0 and got is None, name
            continue
        assert fatal == 0, name
        _compare_epbl(f"{grid}/{nk}/{name}", d, M, want, got, True)
        ran += 1
    assert ran == len(E.CASES_EXACT) - 2 and {"rh18_orig_tl", "translay_hi"} <= set(E.CASES_EXACT)


def test_epbl_libm_class_against_the_compiled_reference():
    """The cases with exp, log or pow, on the columns the screen of tests/test_energetic_PBL_cpu.py keeps (those whose trace does
    not change when every libm result moves by 2 ulp), to 1e-12 of each field's range.  The cap on what the screen leaves out is
    asserted first, from the restatement alone."""
    from tests.test_energetic_PBL_cpu import CAP, LIBM_RUNS, screen
    assert CAP == 0.05
    kept = {}
    for name, nk in LIBM_RUNS:
        d, M, GV, P, opt, inp, want, steady, spread, _ = screen("benchmark_small", nk, name)
        wet = M[G["mask2dT"]][H.interior(d, "h")] > 0.0
        assert int((wet & ~steady).sum()) <= CAP * wet.sum(), name
        kept[(name, nk)] = (d, M, GV, P, opt, inp, want, steady | ~wet)
    _need_lib()
    for (name, nk), (d, M, GV, P, opt, inp, want, keep) in kept.items():
        got, fatal = RP.energetic_PBL(d, M, GV, P, opt, inp)
        assert fatal == 0, name
        _compare_epbl(f"benchmark_small/{nk}/{name}", d, M, want, got, False, keep=keep)


def test_epbl_init_refusal_is_the_references():
    """EPBL_TRANSITION_SCALE of 0 or 1 with USE_MLD_ITERATION is FATAL in energetic_PBL_init (:3969-3972), which the device and
    the restatement take (include/mom6x.h says so): epbl_ref.reference_refuses names exactly what the compiled reference stops
    on, and of the case table only rh18_orig and translay1 are such."""
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=2)[1:]
    _, opt = E.case("croot_orig", GV)
    inp = E.case_inputs(d, M, GV, opt)
    for v, it, bad in ((0.0, 1, True), (1.0, 1, True), (-0.5, 1, True), (0.0, 0, False), (1.0, 0, False), (0.5, 1, False)):
        P = abi.energetic_PBL_params_default(GV, TKE_decay=0.0, answer_date=20240101, transLay_scale=v, Use_MLD_iteration=it)
        assert E.reference_refuses(P) == bad, (v, it)
        if RP.lib() is not None:
            got, fatal = RP.energetic_PBL(d, M, GV, P, opt, inp)
            assert (fatal > 0) == bad, (v, it, fatal)
    assert {n for n in E.CASES if E.reference_refuses(E.case(n, GV)[0])} == {"rh18_orig", "translay1"}


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_kappa_shear

KSHEAR_RUNS = tuple((grid, nk, ()) for grid, nk in KSHEAR_GRIDS) + (("benchmark_small", 75, (("ni", 20), ("nj", 12))),)
KSHEAR_QUIET = ("quiet",)            # the one case whose inputs do not shear: no column of it mixes, by design
KSHEAR_OUT = RP.KSHEAR_CORE + K.DIAG_3D


def _kshear_cases(nk):
    return tuple(K.CASES) if nk != 75 else ("shear",)


@functools.lru_cache(maxsize=None)
def _kshear(grid, nk, kw, name):
    """A case on a grid with every diagnostic asked for, and the restatement's result and counters: computed once (read only)."""
    d, M = getattr(H, grid)(nk=nk, **dict(kw))[1:]
    GV = abi.vgrid_default()
    P, opt = K.case(name, GV)
    opt = dict(opt, diag=K.DIAG_3D + K.DIAG_2D)
    inp = K.case_inputs(d, M, GV, opt)
    want, counts = K.run(d, M, GV, P, opt, inp)
    return d, M, GV, P, opt, inp, want, counts


def _compare_kshear(tag, d, want, got):
    """kappa_io, tke_io, kv_io and the four 3-D diagnostics on the computational domain, bit for bit.  Not held here: KS_its,
    which reaches no diagnostic of the reference (like OBL_its of ePBL) and stays compared with the restatement only."""
    dm = (Ellipsis,) + RP.dom(d)
    assert set(got) == set(want) - set(RP.KSHEAR_NOT_EXPOSED) == set(KSHEAR_OUT), (sorted(got), sorted(want))
    for n in KSHEAR_OUT:
        H.assert_bitwise(np.ascontiguousarray(got[n][dm]), np.ascontiguousarray(want[n][dm]), f"{tag}: {n}")


@pytest.mark.parametrize("grid,nk,kw", KSHEAR_RUNS, ids=lambda v: "x".join(str(b) for _, b in v) if isinstance(v, tuple) else str(v))
def test_kappa_shear_against_the_compiled_reference(grid, nk, kw):
    """tests/kappa_shear_ref.py against Calculate_kappa_shear of the reference's own MOM_kappa_shear.F90, set up by its own
    kappa_shear_init, EOS_init (MOM_EOS.F90: the unit conversion around the array call and the `scale` product, :781-829, are the
    reference's text) and unit_scaling_init: every case of the table on the bowl at 1, 2, 3, 4 and 8 layers and on the island basin
    at 4, and `shear` at 20 x 12 x 75.  kappa_io, tke_io, kv_io, N2_shear_in, S2_shear_in, N2_shear_mean and S2_shear_mean, whole
    arrays on the computational domain, bit for bit; zero FATALs.

    Outside the comparison: find_uv_at_h (MOM_diabatic_aux.F90:546-611, twenty lines): its module imports extractFluxes1d,
    MOM_interpolate and the tracer flow control, out of reach of interface-only stand-ins, so the compiled routine is handed the
    u_h, v_h that kappa_shear_ref.find_uv_at_h makes; those lines stay held only by tests/test_kappa_shear_cpu.py (rescaling, the
    inserted massless layers) and by the device comparison.  KS_its reaches no diagnostic of the reference.

    A comparison of columns that do not mix proves little: with an interior interface (more layers than the nkml that are
    merged into one), every case whose inputs shear has columns
    in the predictor-corrector (`quiet` is the one that is meant not to), and `shear` keeps the floors of
    tests/test_kappa_shear_cpu.py: a quarter of the wet columns mix, a tenth take two or more outer iterations."""
    for name in _kshear_cases(nk):
        d, M, GV, P, opt, inp, want, counts = _kshear(grid, nk, kw, name)
        if nk > P.nkml:               # an interior interface is left after the first nkml layers are merged into one (:261)
            assert (counts["pred_corr"] > 0) == (name not in KSHEAR_QUIET), (grid, nk, name, counts["pred_corr"])
        if name == "tie" and nk >= 2:   # the tie of N2 = MAX(0.0, -0.0) (:1492-1502) is reached: the reference answers -0.0
            z = want["N2_init"][(Ellipsis,) + RP.dom(d)]
            assert (np.signbit(z) & (z == 0.0)).any(), (grid, nk)
        if name == "shear" and nk >= 2:
            own = np.zeros(d.shape2(), bool); own[H.interior(d, "h")] = True
            wet = own & (M[G["mask2dT"]] > 0.0)
            mixed = (want["kappa_io"][:, wet] > 0.0).any(axis=0)
            two = want["KS_its"][wet] >= 2.0
            assert 4 * mixed.sum() >= wet.sum() and 10 * two.sum() >= wet.sum(), (grid, nk, int(mixed.sum()), int(two.sum()), int(wet.sum()))
    _need_lib()
    for name in _kshear_cases(nk):
        d, M, GV, P, opt, inp, want, counts = _kshear(grid, nk, kw, name)
        got, fatal = RP.Calculate_kappa_shear(d, M, GV, P, opt, inp)
        assert fatal == 0, (grid, nk, name, fatal)
        _compare_kshear(f"{grid}/{nk}/{name}", d, want, got)


def test_kappa_shear_compared_set_reaches_every_required_arm():
    """Over everything test_kappa_shear_against_the_compiled_reference compares, every arm of tests/test_kappa_shear_cpu.REQUIRED is
    reached, from the restatement's counters alone (newton_pivot_K, :1853, stays unreached: no input that reaches it is known)."""
    tot = K.new_counts()
    for grid, nk, kw in KSHEAR_RUNS:
        for name in _kshear_cases(nk):
            for k, v in _kshear(grid, nk, kw, name)[7].items():
                tot[k] += v
    for k in KSHEAR_REQUIRED:
        assert tot[k] > 0, (k, tot)
    print("newton_pivot_K over the compared set:", tot["newton_pivot_K"])


@pytest.mark.parametrize("name", ("layered", "shear"))
def test_kappa_shear_rescaled_through_the_references_unit_scaling_init(name):
    """Z, L, T, H and R rescaled by 2**11 one at a time and all at once with unequal powers (the sets of
    tests/test_kappa_shear_cpu.py), set in the door: the *_RESCALE_POWERs go through the reference's own unit_scaling_init, the
    parameters through the `scale=` of its kappa_shear_init, the equation of state through the factors its EOS_init takes from US.
    The unscaled outputs are the unscaled run's bits, and the rescaled restatement equals the rescaled reference: the restatement's
    placement of the US% and GV% factors is held to the compiled init and not to itself."""
    _need_lib()
    d, M, GV, P, opt, inp, want, counts = _kshear("island_basin", 4, (), name)
    assert counts["pred_corr"] > 0
    base, fatal = RP.Calculate_kappa_shear(d, M, GV, P, opt, inp)
    assert fatal == 0
    _compare_kshear(f"{name} unscaled", d, want, base)
    dm = (Ellipsis,) + RP.dom(d)
    for sc in RESCALE_SETS:
        M2, GV2, P2, opt2, inp2, f = rescaled(name, sc, M, GV, P, opt, inp)
        got, fatal = RP.Calculate_kappa_shear(d, M2, GV2, P2, opt2, inp2)
        assert fatal == 0, (name, sc)
        mine, _ = K.run(d, M2, GV2, P2, opt2, inp2)
        _compare_kshear(f"{name} rescaled by Z, L, T, H, R = {sc}", d, mine, got)
        for n in KSHEAR_OUT:
            H.assert_bitwise(np.ascontiguousarray(got[n][dm] / f(_DIM_OUT[n])), np.ascontiguousarray(base[n][dm]),
                             f"{name}: {n} of the reference, rescaled by {sc} and unscaled")


def test_kappa_shear_init_refusals_against_the_references():
    """kappa_shear_ref.init_check (the twin of what mom6x_kappa_shear_init rejects as invalid) against the compiled
    kappa_shear_init: the reference has no FATAL of its own and accepts every value the device rejects (include/mom6x.h lists the
    difference); what both take, both take; an equation of state the reference does not know is FATAL in its EOS_init."""
    GV = abi.vgrid_default()
    dflt = abi.kappa_shear_params_default
    d, M = H.benchmark_small(nk=2)[1:]
    _, opt = K.case("shear", GV)
    inp = K.case_inputs(d, M, GV, opt)
    init_only = dict(opt, dt=0.0)
    rejected = (dict(max_KS_it=0), dict(max_RiNo_it=0), dict(RiNo_crit=0.0), dict(RiNo_crit=-0.25), dict(kappa_src_max_chg=1.0),
                dict(nkml=0), dict(lambda_=0.0))
    accepted = (dict(), dict(nkml=2), dict(kappa_src_max_chg=5.0), dict(RiNo_crit=0.3), dict(max_KS_it=1, max_RiNo_it=1))
    for mods, bad in [(m, True) for m in rejected] + [(m, False) for m in accepted]:
        P = dflt(GV, **mods)
        if bad:
            with pytest.raises(ValueError):
                K.init_check(P, GV)
        else:
            K.init_check(P, GV)
        if RP.lib() is not None:
            got, fatal = RP.Calculate_kappa_shear(d, M, GV, P, init_only, inp)
            assert fatal == 0, (mods, fatal)          # accepted, or rejected by the device alone: never the other way round
    _need_lib()
    got, fatal = RP.Calculate_kappa_shear(d, M, GV, dflt(GV), init_only, inp, table_extra=[("EQN_OF_STATE", "NO_SUCH_EOS")])
    assert fatal >= 1 and got is None


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_neutral_diffusion

NDIFF_RUNS = tuple((grid, nk, (), tuple(N.CASES)) for grid, nk in N.CONFIGS) + (
    ("benchmark_small", 75, (("ni", 20), ("nj", 12)), ("slope",)),
    ("torus", 3, tuple(zip(("ni", "nj"), RP.edge_torus_shape())), ("slope", "new_order")))
NDIFF_PROBED = ("slope", "ties", "massless")
# What the compiled neutral_diffusion_init does with each setting that mom6x_neutral_diffusion_init refuses (include/mom6x.h):
# setting -> (members of the parameters, FATALs of the reference's own, calls of stood-in procedures, in words)
NDIFF_REFUSALS = {
    "NDIFF_CONTINUOUS": (dict(continuous_reconstruction=0), 0, 2,
                         "accepts: no FATAL and no WARNING; goes on into initialize_remapping and extract_member_remapping_CS (:248-251)"),
    "NDIFF_INTERIOR_ONLY": (dict(interior_only=1), 1, 2,
                            "accepts the setting; asks the diabatic driver for KPP and ePBL (:294-295) and is FATAL where neither is there (:297)"),
    "NDIFF_TAPERING": (dict(tapering=1), 0, 0, "ignores it: NDIFF_TAPERING is read only under NDIFF_INTERIOR_ONLY (:195-200)"),
    "KHTR_USE_EBT_STRUCT": (dict(KhTh_use_vert_struct=1), 0, 0, "accepts: no FATAL and no WARNING (Coef_h is allocated, :306-308)"),
    "NDIFF_USE_UNMASKED_TRANSPORT_BUG": (dict(use_unmasked_transport_bug=1), 0, 0, "accepts: no FATAL and no WARNING"),
}


def _compare_ndiff(tag, d, want, got, names=RP.NDIFF_OUT):
    """The tracers and tendencies on the computational domain, trans_x_2d and trans_y_2d on their face ranges (the ranges of
    tests/test_neutral_diffusion_gpu.py's _check), bit for bit.  Not held here: the ten coefficient arrays of
    RP.NDIFF_NOT_EXPOSED, which the compiled module keeps private."""
    rng = RP.ndiff_ranges(d)
    assert set(got) == set(RP.NDIFF_OUT) and set(RP.NDIFF_NOT_EXPOSED) == set(N.COEFFS) <= set(want), (sorted(got), sorted(want))
    for n in names:
        assert len(got[n]) == len(want[n]), (tag, n)
        for m, (a, b) in enumerate(zip(got[n], want[n])):
            sl = (Ellipsis,) + rng[n]
            assert np.isfinite(b[sl]).all(), (tag, n, m)
            H.assert_bitwise(np.ascontiguousarray(a[sl]), np.ascontiguousarray(b[sl]), f"{tag}: {n}[{m}]")


def _ndiff_tag(grid, nk, kw, name):
    return "/".join([grid] + [str(v) for _, v in kw] + [str(nk), name])


@functools.lru_cache(maxsize=None)
def _ndiff_probed(name):
    """A case on the island basin at 4 layers with a registry of T, S, the case's three tracers and two probes, and the
    restatement's result and counters: computed once (read only)."""
    d, M, GV, P, opt, inp = N.want("island_basin", 4, name)[:6]
    nk = d.nk
    rng = np.random.default_rng(23)
    noise = 0.25 * rng.uniform(-1.0, 1.0, d.shape2())                       # the seeded column noise: below half a unit
    index = np.stack([np.full(d.shape2(), k + 1.0) + noise for k in range(nk)])
    zmid = np.cumsum(inp["h"], axis=0) - 0.5 * inp["h"]                       # (NaN where h is: beyond the first halo)
    pmid = (GV.g_Earth * GV.H_to_RZ) * zmid
    linear = (2.0 + rng.uniform(-1.0, 1.0, d.shape2())) + (1.0e-6 * (1.0 + rng.uniform(0.0, 1.0, d.shape2()))) * pmid
    keep = np.isfinite(inp["h"][0])
    inp = dict(inp, tracers=[inp["T"].copy(), inp["S"].copy()] + [t.copy() for t in inp["tracers"]] +
               [np.where(keep, index, np.nan), np.where(keep, linear, np.nan)])
    want, counts = N.run(d, M, GV, P, opt, inp)
    return d, M, GV, P, opt, inp, want, counts


def _ndiff_two_rounds():
    """(d, M, GV, P, opt, first inputs, second inputs, the restatement's outputs after the second round, its counters): `slope`
    on the island basin at 4 layers, then calc_coeffs from the thicknesses, T, S of `massless` and neutral_diffusion once more on
    the tracers the first round left."""
    d, M, GV, P, opt, inp, one, _ = N.want("island_basin", 4, "slope")
    inp2 = N.want("island_basin", 4, "massless")[5]
    counts = N.new_counts()
    CS = N.calc_coeffs(d, M, GV, P, N.case_eos(opt), inp2["h"], inp2["T"], inp2["S"], None, counts=counts)
    out = dict(tracers=[t.copy() for t in one["tracers"]], tendency=[np.full(d.shape3(), np.nan) for _ in range(3)],
               trans_x_2d=[np.full(d.shape2(), np.nan) for _ in range(3)], trans_y_2d=[np.full(d.shape2(), np.nan) for _ in range(3)])
    Cx, Cy = N.coef_planes(d, M)
    N.neutral_diffusion(d, M, GV, P, CS, inp2["h"], Cx, Cy, N.DT, out["tracers"], None, out["tendency"], out["trans_x_2d"],
                        out["trans_y_2d"], counts)
    out.update({n: getattr(CS, n) for n in N.COEFFS})
    return d, M, GV, P, opt, inp, inp2, out, counts


def _ndiff_hordiff_rounds():
    """Two iterations of the restatement's neutral branch of tracer_hordiff with RECALC_NEUTRAL_SURF on the bowl at 3 layers, T
    and S outside the registry and no group pass (one closed tile has nothing to exchange): what it hands calc_coeffs and
    neutral_diffusion in its two iterations is what the door's two rounds are handed.  Returns (d, M, GV, P, opt, inp, Coef_x and
    Coef_y, dt of an iteration, the restatement's outputs, its counters)."""
    from tests import hordiff_ref
    d, M, GV, P, opt, inp = N.want("benchmark_small", 3, "slope")[:6]
    Pthd = abi.tracer_hor_diff_params_default(KHTR=1.0, check_diffusive_CFL=1)
    khx, khy = hordiff_ref.khdt_faces(d, M, Pthd, N.DT, {})
    Pthd.KhTr = 1.5 / float(hordiff_ref.cell_cfl(d, M, khx, khy).max())
    P2 = abi.NeutralDiffusionParams.from_buffer_copy(P); P2.recalc_neutral_surf = 1
    out = dict(tracers=[t.copy() for t in inp["tracers"]], tendency=[np.full(d.shape3(), np.nan) for _ in range(3)],
               trans_x_2d=[np.full(d.shape2(), np.nan) for _ in range(3)], trans_y_2d=[np.full(d.shape2(), np.nan) for _ in range(3)])
    counts = N.new_counts()
    rec = {}
    n = N.tracer_hordiff_neutral(d, M, GV, Pthd, P2, N.case_eos(opt), inp["h"], N.DT, out["tracers"], inp["T"], inp["S"],
                                 tendency=out["tendency"], trans_x_2d=out["trans_x_2d"], trans_y_2d=out["trans_y_2d"], counts=counts,
                                 pass_fn=lambda a: None, record=rec)
    assert n == 2 and rec["calc_coeffs"] == 2 and counts["recalc"] == 1 and counts["itt_gt1"] == 1
    khx, khy = hordiff_ref.khdt_faces(d, M, Pthd, N.DT, {})
    io, jo, ni, nj = d.ioff, d.joff, d.ni, d.nj
    Cx = np.full(d.shape3(d.nk + 1), np.nan); Cy = np.full(d.shape3(d.nk + 1), np.nan)
    Cx[0, jo:jo + nj, io - 1:io + ni] = 0.5 * khx; Cy[0, jo - 1:jo + nj, io:io + ni] = 0.5 * khy
    out.update({c: getattr(rec["CS"], c) for c in N.COEFFS})
    return d, M, GV, P2, opt, inp, (Cx, Cy), 0.5 * N.DT, out, counts


@pytest.mark.parametrize("grid,nk,kw,cases", NDIFF_RUNS, ids=[_ndiff_tag(g, n, kw, "") for g, n, kw, _ in NDIFF_RUNS])
def test_neutral_diffusion_against_the_compiled_reference(grid, nk, kw, cases):
    """tests/ndiff_ref.py against neutral_diffusion_calc_coeffs and neutral_diffusion of the reference's own
    MOM_neutral_diffusion.F90, set up by its own neutral_diffusion_init, EOS_init (the array form of calculate_density_derivs with
    its unit conversions, MOM_EOS.F90:781-829, is the reference's text) and unit_scaling_init: every case of ndiff_ref.CASES on the
    bowl at 1, 2, 3, 4 and 8 layers and on the island basin at 4, `slope` at 20 x 12 x 75, `slope` and `new_order` on the land-free
    torus one cell larger than a work-group, from the NaN-beyond-the-first-halo inputs of ndiff_ref.want.  Every tracer and its
    content tendency on the computational domain and both transports on their face ranges, bit for bit; zero FATALs.  All words
    are of the EXACT class: the path is + - * / and compares with Wright's and the linear equation of state, and no site of it goes
    through an intrinsic that two builds may round differently (x**2 at :1209 is x * x).

    Outside the comparison: PoL, PoR, KoL, KoR and hEff themselves (private components of neutral_diffusion_CS; id_uhEff_2d and
    id_vhEff_2d are registered nowhere), held through what they produce and by the probing registry below; the neutral branch of
    tracer_hordiff (MOM_tracer_hor_diff.F90 is not compiled); the discontinuous reconstruction (MOM_remapping is stood in for)."""
    _need_lib()
    for name in cases:
        d, M, GV, P, opt, inp, want, counts = N.want(grid, nk, name, **dict(kw))
        got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp)
        assert fatal == 0, (grid, nk, name, fatal)
        _compare_ndiff(_ndiff_tag(grid, nk, kw, name), d, want, got)


@pytest.mark.parametrize("name", NDIFF_PROBED)
def test_neutral_diffusion_with_a_probing_registry(name):
    """`slope`, `ties` and `massless` once more on the island basin at 4 layers with a registry of seven: T, S, the case's three
    tracers and two probes.  The probes stand in for the coefficient arrays the compiled reference hides: one equals its layer's
    index plus a seeded noise per column of less than half a unit, so that a KoL or KoR taken one interface off moves its flux
    by a whole unit; the other is linear in pressure within each column, so that its interface values and sublayer means follow
    PoL and PoR.  Both must move for the comparison to mean anything, which is asserted from the restatement first."""
    d, M, GV, P, opt, inp, want, counts = _ndiff_probed(name)
    assert len(inp["tracers"]) == 7 and counts["flux_down"] > 0
    own = (slice(None),) + H.interior(d, "h")
    for m in (5, 6):
        assert (want["tendency"][m][own] != 0.0).sum() > 0.1 * want["tendency"][m][own].size, (name, m)
    _need_lib()
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp)
    assert fatal == 0
    _compare_ndiff(f"{name} with probes", d, want, got)


@pytest.mark.parametrize("name", ("slope", "refp", "refp_wright"))
def test_neutral_diffusion_rescaled_through_the_references_unit_scaling_init(name):
    """`slope`, and `refp` and `refp_wright` (the reference pressure under the linear and under Wright's equation of state) with
    a surface pressure, with Z, L, T, H, R, C and S rescaled by 2**11 one at a time and all at once
    with unequal powers (the sets of tests/test_neutral_diffusion_cpu.py).  The *_RESCALE_POWERs go through the reference's own
    unit_scaling_init, NDIFF_REF_PRES through the `scale=` of its neutral_diffusion_init and the equation of state through the
    factors its EOS_init takes from US; the vertical grid's members (GV is a stand-in: MOM_verticalGrid.F90 is not compiled) are
    the rescaled grid's.  After unscaling, every word is the unscaled door's, and the rescaled restatement equals the rescaled
    reference: where the restatement puts its unit factors is held to the compiled module and not to itself."""
    _need_lib()
    from tests.test_neutral_diffusion_cpu import RESCALE_SETS, _DIM_OUT, rescaled
    d, M, GV, P, opt, inp = N.want("island_basin", 4, name)[:6]
    if name.startswith("refp"):
        opt = dict(opt, p_surf=True)
        inp = N.nan_halo(d, N.case_inputs(d, M, GV, opt))
        assert "p_surf" in inp and P.ref_pres > 0.0
    want, _ = N.run(d, M, GV, P, opt, inp)
    base, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp)
    assert fatal == 0
    _compare_ndiff(f"{name} unscaled", d, want, base)
    rng = RP.ndiff_ranges(d)
    for sc in RESCALE_SETS:
        M2, GV2, P2, inp2, coef, dt2, f = rescaled(sc, d, M, GV, P, inp)
        powers = {u: -RP._power_of_two(s, u) for u, s in zip("ZLTHRCS", sc) if u != "H"}      # US%x_to_m = 1 / sc: the power is -11
        got, fatal = RP.neutral_diffusion(d, M2, GV2, P2, opt, inp2, powers=powers, dt=dt2, coef=coef)
        assert fatal == 0, (name, sc)
        mine, _ = N.run(d, M2, GV2, P2, opt, inp2, dt=dt2, coef=coef)
        _compare_ndiff(f"{name} rescaled by Z, L, T, H, R, C, S = {sc}", d, mine, got)
        for n in RP.NDIFF_OUT:
            for m, (a, b) in enumerate(zip(got[n], base[n])):
                sl = (Ellipsis,) + rng[n]
                H.assert_bitwise(np.ascontiguousarray(a[sl] / f(_DIM_OUT.get(n, (0,) * 7))), np.ascontiguousarray(b[sl]),
                                 f"{name}: {n}[{m}] of the reference, rescaled by {sc} and unscaled")


def test_neutral_diffusion_second_round_on_one_control_structure():
    """calc_coeffs and neutral_diffusion twice on ONE neutral_diffusion_CS of the reference.  First `slope`, then coefficients
    from the thicknesses, T and S of `massless` (layers of zero thickness where `slope` had none): a position, an index or an
    effective thickness left over from the first round would show in the second round's tracers and transports.  Then the two
    iterations the restatement's tracer_hordiff_neutral makes under RECALC_NEUTRAL_SURF (calc_coeffs again, neutral_diffusion
    with half the coefficients and half the time step): its loop is not compared (MOM_tracer_hor_diff.F90 is not compiled), what
    it calls twice is."""
    d, M, GV, P, opt, inp, inp2, want, _ = _ndiff_two_rounds()
    hd = _ndiff_hordiff_rounds()
    _need_lib()
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp, ncalls=2, inp2=inp2)
    assert fatal == 0
    _compare_ndiff("slope, then massless on the same control structure", d, want, got)
    d, M, GV, P, opt, inp, coef, dt, want, _ = hd
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp, ncalls=2, coef=coef, dt=dt)
    assert fatal == 0
    _compare_ndiff("two iterations of tracer_hordiff_neutral", d, want, got)


def test_neutral_diffusion_init_refusals_against_the_references():
    """Every setting mom6x_neutral_diffusion_init refuses (ndiff_ref.refused names it) against the compiled
    neutral_diffusion_init: NDIFF_REFUSALS records what the reference does.  It has no FATAL and no WARNING for any of them: it
    accepts the discontinuous reconstruction, the vertical structure and the unmasked-transport bug, ignores NDIFF_TAPERING
    without NDIFF_INTERIOR_ONLY, and under NDIFF_INTERIOR_ONLY is FATAL only where the diabatic driver has neither KPP nor ePBL.
    The refusals are the device's alone (include/mom6x.h lists the difference).  Calls of stood-in procedures (MOM_remapping,
    MOM_diabatic_driver) are counted apart from the reference's own FATALs.  An unknown EQN_OF_STATE is FATAL in its EOS_init."""
    GV = abi.vgrid_default()
    eos = abi.eos_params_default()
    assert N.refused(abi.neutral_diffusion_params_default(), GV, eos) is None
    for word, (mods, own, standins, _) in NDIFF_REFUSALS.items():
        assert N.refused(abi.neutral_diffusion_params_default(**mods), GV, eos) == word
    assert set(sum((tuple(m) for m, _, _, _ in NDIFF_REFUSALS.values()), ())) == {"continuous_reconstruction"} | set(abi.NEUTRAL_DIFFUSION_MUST_BE_0)
    _need_lib()
    d, M, GV, P, opt, inp = N.want("benchmark_small", 2, "slope")[:6]
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp, dt=0.0)
    assert fatal == 0 and got == {} and RP.standin_never_count() == 0
    for word, (mods, own, standins, _) in NDIFF_REFUSALS.items():
        got, fatal = RP.neutral_diffusion(d, M, GV, abi.neutral_diffusion_params_default(**mods), opt, inp, dt=0.0)
        never = RP.standin_never_count()
        assert (fatal - never, never) == (own, standins), (word, fatal, never)
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp, dt=0.0, table_extra=[("EQN_OF_STATE", "NO_SUCH_EOS")])
    assert fatal >= 1 and got is None and RP.standin_never_count() == 0
    got, fatal = RP.neutral_diffusion(d, M, GV, P, opt, inp, dt=0.0, table_extra=[("USE_NEUTRAL_DIFFUSION", False)])
    assert fatal == 1 and got is None             # (the door counts an init that answers "not used")


def test_neutral_diffusion_compared_set_reaches_every_required_arm():
    """Over everything the door tests above compare -- NDIFF_RUNS, the probing registry, the second rounds -- every arm of
    tests/test_neutral_diffusion_cpu.REQUIRED is reached, from the restatement's counters alone; `recalc` and `itt_gt1` by the two
    iterations whose calls the second-round test compares."""
    from tests.test_neutral_diffusion_cpu import NOT_REACHED, REQUIRED
    tot = N.new_counts()
    runs = [N.want(grid, nk, name, **dict(kw))[7] for grid, nk, kw, cases in NDIFF_RUNS for name in cases]
    runs += [_ndiff_probed(name)[7] for name in NDIFF_PROBED] + [_ndiff_two_rounds()[8], _ndiff_hordiff_rounds()[9]]
    for counts in runs:
        for k, v in counts.items():
            tot[k] += v
    assert set(REQUIRED) | set(NOT_REACHED) == set(N.ARMS) and len(REQUIRED) == len(N.ARMS) - 4
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)


# ------------------------------------------------------------------------------------------------------------------------------
# MOM_lateral_mixing_coeffs (with MOM_isopycnal_slopes and MOM_interface_heights) and MOM_thickness_diffuse

NARROW = (("ni", 20), ("nj", 12))        # a narrowed bowl
# every grid and layer count of tests/test_varmix_cpu.py, test_varmix_gpu.py and test_thickness_diffuse_gpu.py below 360 x 180:
# (grid, nk, grid keywords, which cases): "all" is every entry of the case list, the eight equations of state included; "layers"
# the cases of those files' test_layer_counts
LATERAL_RUNS = tuple((grid, nk, (), "all") for grid in LAT_GRIDS for nk in (8, 75)) + (("benchmark_small", 6, (), "all"),) + tuple(
    ("benchmark_small", nk, (), "layers") for nk in (1, 2, 3, 4, 52, 53, 76, 77, 120)) + tuple(
    ("benchmark_small", nk, NARROW, "layers") for nk in (1, 2, 3, 75)) + (("island_basin", 4, (), "all"),)
VARMIX_OUT = RP.VARMIX_MEMBERS + tuple(RP.VARMIX_DIAG_NAMES)


def _lat_id(v):
    return "x".join(str(b) for _, b in v) if isinstance(v, tuple) else str(v)


def _lat_grid(grid, nk, kw):
    return H.benchmark_small(nk=nk, **dict(kw))[1:] if kw else LAT_GRIDS[grid](nk)


def _varmix_cases(nk, which):
    if which == "all":
        return tuple(V.case_list())
    names = ("eady", "visbeck", "eady_noeos", "visbeck_noeos", "just_e") if nk > 1 else ("eady_noeos", "visbeck_noeos", "just_e")
    return tuple((n, abi.WRIGHT if V.CASES[n][1] == "form" else None) for n in names + (("just_e_full",) if nk > 2 else ()))


def _thick_cases(nk, which):
    if which == "all":
        return tuple((n, f) for n, c in TD.CASES.items() if n not in RP.THICKDIFF_LEFT_OUT
                     for f in (V.FORMS if c[1] == "form" else (None,)))
    return (("noeos", None), ("eos", abi.WRIGHT), ("large", None)) if nk > 1 else (("noeos", None),)


@functools.lru_cache(maxsize=None)
def _varmix(grid, nk, kw, name, form):
    """A case on a grid with every diagnostic asked for, and the restatement's result and counters: computed once (read only)."""
    from oracle import orc
    orc.build()
    d, M = _lat_grid(grid, nk, kw)
    GV = abi.vgrid_default()
    P, eos, ps, dg, dt, opts = V.case(name, GV, form=form, nk=nk)
    if name == "just_e_full" and nk > 2:
        P.VarMix_Ktop = max(P.VarMix_Ktop, 3)
    inp = V.inputs(d, M, GV, **opts)
    want, counts = V.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, give_diag=True, orc=orc)
    return d, M, GV, P, eos, ps, dt, inp, want, counts


@functools.lru_cache(maxsize=None)
def _thick(grid, nk, kw, name, form):
    from oracle import orc
    orc.build()
    d, M = _lat_grid(grid, nk, kw)
    GV = abi.vgrid_default()
    P, eos, ps, stored, gm, dt, opts = TD.case(name, form=form or abi.WRIGHT)
    inp = TD.inputs(d, M, GV, **opts)
    want, counts = TD.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored, give_gm=True, orc=orc)
    return d, M, GV, P, eos, ps, stored, dt, inp, want, counts


def _written(d, P, want, tag):
    """The restatement started every output as NaN: what it wrote is exactly the reference's ranges (RP.varmix_ranges)."""
    rng = RP.varmix_ranges(d, P)
    for n, a in want.items():
        r = np.zeros(a.shape, bool)
        if n in rng:
            r[rng[n]] = True
        assert np.array_equal(~np.isnan(a), r), f"{tag}: {n} is not written on its range"
    return rng


def _compare_varmix(tag, d, P, want, got, names=VARMIX_OUT):
    """SN_u, SN_v, slope_x, slope_y (members of VarMix_CS) and N2_u, N2_v, S2_u, S2_v, dzu, dzv, dzSxN, dzSyN (what the module posts),
    each on the range the reference writes, bit for bit; the reference hands out everything the restatement makes."""
    rng = _written(d, P, want, tag)
    assert set(rng) <= set(got), (tag, sorted(rng), sorted(got))
    for n in names:
        if n in rng:
            H.assert_bitwise(np.ascontiguousarray(got[n][rng[n]]), np.ascontiguousarray(want[n][rng[n]]), f"{tag}: {n}")


def _compare_thick(tag, d, want, got, names=RP.THICKDIFF_OUT):
    """h, uhtr, vhtr, CDp%uhGM, CDp%vhGM and the posted uhGM, vhGM diagnostics on their ranges, bit for bit."""
    rng = RP.thickdiff_ranges(d)
    for n in names:
        s = (Ellipsis,) + rng[n]
        H.assert_bitwise(np.ascontiguousarray(got[n][s]), np.ascontiguousarray(want[n][s]), f"{tag}: {n}")
        if n + "_diag" in got:
            H.assert_bitwise(np.ascontiguousarray(got[n + "_diag"][s]), np.ascontiguousarray(want[n][s]), f"{tag}: posted {n}")
    assert "uhGM_diag" in got and "vhGM_diag" in got, tag


@pytest.mark.parametrize("grid,nk,kw,which", LATERAL_RUNS, ids=_lat_id)
def test_calc_slope_functions_against_the_compiled_reference(grid, nk, kw, which):
    """tests/varmix_ref.py against calc_slope_functions of the reference's own MOM_lateral_mixing_coeffs.F90 with
    calc_isoneutral_slopes and vert_fill_TS of MOM_isopycnal_slopes.F90, find_eta of MOM_interface_heights.F90 and the array forms
    of calculate_density_derivs of MOM_EOS.F90, set up by the reference's unit_scaling_init, EOS_init and VarMix_init: every entry
    of the case list, the eight equations of state included, on the bowl, the island basin and the partially blocked faces at 8 and
    75 layers and on the bowl at 6, and the layer-count cases on the bowl at 1, 2, 3, 4, 52, 53, 76, 77 and 120 layers and on a
    narrowed bowl at 1, 2, 3 and 75.  Every output on the range the reference writes, bit for bit; zero FATALs and no call of a
    stand-in that must never run.  There is no tolerance class: + - * / and sqrt only."""
    for name, form in _varmix_cases(nk, which):
        d, M, GV, P, eos, ps, dt, inp, want, counts = _varmix(grid, nk, kw, name, form)
        rng = _written(d, P, want, f"{grid}/{nk}/{name}")
        if name == "eady_tie" and nk >= 2 and not kw:
            # the tie of the radicand of dzSxN (MOM_isopycnal_slopes.F90:418) is reached: MAX(0.0, -0.0), the reference answers -0.0
            z = want["dzSxN"][rng["dzSxN"]][1:-1]
            assert (np.signbit(z) & (z == 0.0)).any(), (grid, nk)
    _need_lib()
    for name, form in _varmix_cases(nk, which):
        d, M, GV, P, eos, ps, dt, inp, want, counts = _varmix(grid, nk, kw, name, form)
        got, fatal = RP.calc_slope_functions(d, M, GV, P, inp, dt, eos=eos, give_ps=ps)
        assert fatal == 0 and RP.standin_never_count() == 0, (grid, nk, name, form, fatal)
        _compare_varmix(f"{grid}/{nk}/{name}/{form}", d, P, want, got)


@pytest.mark.parametrize("grid,nk,kw,which", LATERAL_RUNS, ids=_lat_id)
def test_thickness_diffuse_against_the_compiled_reference(grid, nk, kw, which):
    """tests/thickdiff_ref.py against thickness_diffuse and thickness_diffuse_full of the reference's own MOM_thickness_diffuse.F90,
    set up by its thickness_diffuse_init and by VarMix_init, through which the stored slopes go: every case but khth2d (whose
    plane the reference reads from a file into a private member), eos once per equation of state, on the grids and layer counts of
    test_calc_slope_functions_against_the_compiled_reference.  h, uhtr, vhtr, CDp%uhGM, CDp%vhGM and the posted uhGM, vhGM on their
    ranges, bit for bit."""
    _need_lib()
    for name, form in _thick_cases(nk, which):
        d, M, GV, P, eos, ps, stored, dt, inp, want, counts = _thick(grid, nk, kw, name, form)
        got, fatal = RP.thickness_diffuse(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored)
        assert fatal == 0 and RP.standin_never_count() == 0, (grid, nk, name, form, fatal)
        _compare_thick(f"{grid}/{nk}/{name}/{form}", d, want, got)
        if name == "noeos" and grid != "partial_faces":
            # the tie of the uhD limiter (:1160-1161) is reached: MAX(+0.0, -0.0), and the reference answers -0.0
            z = want["uhGM"][(slice(1, None),) + RP.thickdiff_ranges(d)["uhGM"]]
            assert nk == 1 or (np.signbit(z) & (z == 0.0)).any(), (grid, nk)


@pytest.mark.parametrize("L_scale", [3.0e4, -0.25])
def test_L2_planes_against_the_compiled_VarMix_init(L_scale):
    """CS%L2u, CS%L2v of VarMix_init (:1759-1772) at the two signs of VISBECK_L_SCALE of test_L2_planes_of_the_init_call, on the
    partially blocked faces and with L rescaled (L_to_m = 2), whole planes bit for bit."""
    _need_lib()
    d, M = LAT_GRIDS["partial_faces"](8)
    GV = abi.vgrid_default()
    M2, GV2, _, _, _, _ = td_scaled(d, M, GV, abi.thickness_diffuse_params_default(), {n: np.zeros(1) for n in (
        "h", "T", "S", "p_surf", "khth2d", "uhtr", "vhtr", "slope_x", "slope_y")}, 900.0, "L", p=-1)
    P = abi.varmix_params_default(GV2, Visbeck_L_scale=L_scale, L_to_m=2.0, Z_to_L=0.5)
    want = V.varmix_L2(d, M2, P)
    assert (want[0] != 0.0).any() and (L_scale > 0 or (want[0] == 0.0).any())
    inp = V.inputs(d, M2, GV2)
    got, fatal = RP.calc_slope_functions(d, M2, GV2, P, inp, 0.0, sc=dict(L=0.5))
    assert fatal == 0 and RP.standin_never_count() == 0
    for w, n in zip(want, ("L2u", "L2v")):
        H.assert_bitwise(got[n], w, n)


def _chain(kind):
    """The chain of test_chain_into_thickness_diffuse_and_tracer_hordiff (kind visbeck) and its twin through
    calc_Eady_growth_rate_2D: the two restatements, the first's slopes handed to the second."""
    from oracle import orc
    orc.build()
    d, M = LAT_GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    eos = abi.eos_params_default(abi.WRIGHT)
    inp = TD.inputs(d, M, GV)
    Pv, Ptd = RP.chain_params(GV)
    if kind == "eady":
        Pv = abi.varmix_params_default(GV, **V.EADY)
    w = dict(SN_u=np.full(d.shape2(), np.nan), SN_v=np.full(d.shape2(), np.nan), slope_x=np.zeros(d.shape3(d.nk + 1)),
             slope_y=np.zeros(d.shape3(d.nk + 1)))
    Rlay, gp = abi.layer_densities(d.nk)
    rounds = []
    h, uhtr, vhtr = inp["h"].copy(), inp["uhtr"].copy(), inp["vhtr"].copy()
    for r in range(2):
        V.calc_slope_functions(d, M, GV, Pv, h, RP.CHAIN_DT, w["SN_u"], w["SN_v"], T=inp["T"], S=inp["S"], eos=eos, Rlay=Rlay,
                               g_prime=gp, slope_x=w["slope_x"], slope_y=w["slope_y"], orc=orc)
        TD.thickness_diffuse(d, M, GV, Ptd, h, uhtr, vhtr, RP.CHAIN_DT, T=inp["T"], S=inp["S"], eos=eos, slope_x=w["slope_x"],
                             slope_y=w["slope_y"], orc=orc)
        rounds.append(dict({n: a.copy() for n, a in w.items()}, h=h.copy(), uhtr=uhtr.copy(), vhtr=vhtr.copy()))
    return d, M, GV, Pv, Ptd, eos, inp, rounds


@pytest.mark.parametrize("kind", ["visbeck", "eady"])
def test_chain_of_the_two_on_one_VarMix_CS(kind):
    """The reference's real path: one calc_slope_functions whose stored slopes one thickness_diffuse reads from the same VarMix_CS
    (benchmark_small x 8, WRIGHT, dt = 3600), against the two restatements chained the same way; and two such rounds on the same
    control structures, the second from the first's h.  h, uhtr, vhtr, the slopes and SN_u, SN_v of the last round, bit for bit."""
    _need_lib()
    d, M, GV, Pv, Ptd, eos, inp, rounds = _chain(kind)
    rng = dict(RP.varmix_ranges(d, Pv), **{n: RP.thickdiff_ranges(d)[n] for n in RP.THICKDIFF_CORE})
    assert not np.array_equal(rounds[0]["h"], rounds[1]["h"]) and not np.array_equal(rounds[0]["slope_x"][1:-1], rounds[1]["slope_x"][1:-1])
    for ncalls in (1, 2):
        got, fatal = RP.thickness_diffuse(d, M, GV, Ptd, inp, RP.CHAIN_DT, eos=eos, chain=Pv, ncalls=ncalls)
        assert fatal == 0 and RP.standin_never_count() == 0
        for n in RP.CHAIN_OUT:
            s = rng[n] if n in RP.VARMIX_MEMBERS else (Ellipsis,) + rng[n]
            H.assert_bitwise(np.ascontiguousarray(got[n][s]), np.ascontiguousarray(rounds[ncalls - 1][n][s]), f"chain {kind} x {ncalls}: {n}")


def test_second_call_on_the_same_control_structures():
    """State carried in a control structure would show in a second call: calc_slope_functions twice on one VarMix_CS, the second
    on another h, gives what a fresh one gives on that h; thickness_diffuse twice on one thickness_diffuse_CS gives the restatement
    applied twice."""
    _need_lib()
    from oracle import orc
    for name in ("eady_diag", "visbeck_diag", "just_e"):
        d, M, GV, P, eos, ps, dt, inp, want, counts = _varmix("island_basin", 4, (), name, None)
        inp2 = dict(inp, h=np.ascontiguousarray(inp["h"][:, ::-1, :] * 1.03125))
        want2, _ = V.run(d, M, GV, P, inp2, dt, eos=eos, give_ps=ps, give_diag=True, orc=orc)
        got, fatal = RP.calc_slope_functions(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, ncalls=2, inp2=inp2)
        assert fatal == 0 and RP.standin_never_count() == 0
        assert not np.array_equal(want2["SN_u"], want["SN_u"], equal_nan=True)
        _compare_varmix(f"{name}, second call", d, P, want2, got)
    for name in ("eos", "slopes_noeos", "gm"):
        d, M, GV, P, eos, ps, stored, dt, inp, want, counts = _thick("island_basin", 4, (), name, abi.WRIGHT)
        want2, _ = TD.run(d, M, GV, P, dict(inp, **{n: want[n] for n in RP.THICKDIFF_CORE}), dt, eos=eos, give_ps=ps, stored=stored,
                          give_gm=True, orc=orc)
        got, fatal = RP.thickness_diffuse(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored, ncalls=2)
        assert fatal == 0 and RP.standin_never_count() == 0
        assert not np.array_equal(want2["h"], want["h"])
        _compare_thick(f"{name}, second call", d, want2, got)


@pytest.mark.parametrize("name,dims", V_SCALE_CASES)
def test_calc_slope_functions_rescaled_through_the_references_unit_scaling_init(name, dims):
    """The cases and dimensions of tests/test_varmix_cpu.SCALE_CASES, each of T, L, H, Z, R rescaled by 2**11: the *_RESCALE_POWERs
    go through the reference's own unit_scaling_init, the parameters through the `scale=` of its VarMix_init, H through GV.  The
    rescaled restatement equals the rescaled reference, and the reference unscaled is the unscaled run, bit for bit."""
    _need_lib()
    from oracle import orc
    d, M, GV, P, eos, ps, dt, inp, want, counts = _varmix("benchmark_small", 6, (), name, abi.WRIGHT if V.CASES[name][1] == "form" else None)
    base, fatal = RP.calc_slope_functions(d, M, GV, P, inp, dt, eos=eos, give_ps=ps)
    assert fatal == 0
    _compare_varmix(f"{name} unscaled", d, P, want, base)
    rng = RP.varmix_ranges(d, P)
    for dim in dims:
        M2, GV2, P2, in2, dt2, Rlay2, gp2, un = scaled_varmix(d, M, GV, P, inp, dt, dim)
        P2.L_to_m = 1.0 / (2.0 ** 11 if dim == "L" else 1.0)       # (scaled_varmix leaves it: only VarMix_init's L2 planes read it)
        mine, _ = V.run(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, give_diag=True, orc=orc, Rlay=Rlay2, g_prime=gp2)
        got, fatal = RP.calc_slope_functions(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, sc={dim: 2.0 ** 11}, Rlay=Rlay2, g_prime=gp2)
        assert fatal == 0 and RP.standin_never_count() == 0, (name, dim)
        _compare_varmix(f"{name} rescaled in {dim}", d, P2, mine, got)
        for n in rng:
            H.assert_bitwise(np.ascontiguousarray(got[n][rng[n]] * un[n]), np.ascontiguousarray(base[n][rng[n]]),
                             f"{name}: {n} of the reference, rescaled in {dim} and unscaled")


@pytest.mark.parametrize("name,dims", [c for c in TD_SCALE_CASES if c[0] not in RP.THICKDIFF_LEFT_OUT])
def test_thickness_diffuse_rescaled_through_the_references_unit_scaling_init(name, dims):
    """Likewise the cases of tests/test_thickness_diffuse_cpu.SCALE_CASES (khth2d is outside the comparison)."""
    _need_lib()
    from oracle import orc
    d, M, GV, P, eos, ps, stored, dt, inp, want, counts = _thick("benchmark_small", 6, (), name, abi.WRIGHT)
    base, fatal = RP.thickness_diffuse(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored)
    assert fatal == 0
    _compare_thick(f"{name} unscaled", d, want, base)
    rng = RP.thickdiff_ranges(d)
    for dim in dims:
        M2, GV2, P2, in2, dt2, un = td_scaled(d, M, GV, P, inp, dt, dim)
        mine, _ = TD.run(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, stored=stored, give_gm=True, orc=orc)
        got, fatal = RP.thickness_diffuse(d, M2, GV2, P2, in2, dt2, eos=eos, give_ps=ps, stored=stored, sc={dim: 2.0 ** 11})
        assert fatal == 0 and RP.standin_never_count() == 0, (name, dim)
        _compare_thick(f"{name} rescaled in {dim}", d, mine, got)
        for n in RP.THICKDIFF_OUT:
            s = (Ellipsis,) + rng[n]
            H.assert_bitwise(np.ascontiguousarray(got[n][s] * un[n]), np.ascontiguousarray(base[n][s]),
                             f"{name}: {n} of the reference, rescaled in {dim} and unscaled")


def _lateral_counts(configs=None):
    """The restatements' branch counts over the live compared set (configs None) or over the recorded set."""
    tv, tt = dict.fromkeys(V.BRANCHES, 0), dict.fromkeys(TD.BRANCHES, 0)
    if configs is None:
        runs_v = [_varmix(g, nk, kw, n, f)[9] for g, nk, kw, w in LATERAL_RUNS for n, f in _varmix_cases(nk, w)]
        runs_t = [_thick(g, nk, kw, n, f)[10] for g, nk, kw, w in LATERAL_RUNS for n, f in _thick_cases(nk, w)]
    else:
        from oracle import orc
        orc.build()
        runs_v, runs_t = [], []
        for kind, name, grid, kw in configs:
            if kind not in ("varmix", "thickdiff"):
                continue
            d, M, GV, P, opt, inp = RP.golden_setup(kind, name, grid, kw)
            (runs_v if kind == "varmix" else runs_t).append(_restatement(kind, d, M, GV, P, opt, inp, counts=True))
    for tot, runs in ((tv, runs_v), (tt, runs_t)):
        for c in runs:
            for k, v in c.items():
                tot[k] += v
    return tv, tt


def test_lateral_compared_set_reaches_every_required_arm():
    """Over everything the two door tests above compare, every arm of REQUIRED of tests/test_varmix_cpu.py and of
    tests/test_thickness_diffuse_cpu.py is reached, from the restatements' counters alone."""
    tv, tt = _lateral_counts()
    for k in V_REQUIRED:
        assert tv[k] > 0, (k, tv)
    for k in TD_REQUIRED:
        assert tt[k] > 0, (k, tt)


def test_lateral_recorded_set_reaches_every_required_arm():
    """The recorded configurations (what the device is held to on the GPU) reach every one of those arms by themselves, KH_max and
    the rest of the diffusivity clips included, so the GPU test's coverage is a checked fact.  Never skips."""
    tv, tt = _lateral_counts(RP.golden_configs())
    print("recorded set:", tv, tt)
    for k in V_REQUIRED:
        assert tv[k] > 0, (k, tv)
    for k in TD_REQUIRED:
        assert tt[k] > 0, (k, tt)


# what the reference's inits do with each `must be 0` member that a parameter file can set: (FATALs of the reference's own, calls
# of a stand-in that must never run).  include/mom6x.h states the result.
LATERAL_REFUSALS = {
    ("thickdiff", "use_FGNV_streamfn"): (0, 1),      # accepted; VarMix_init then wants wave speeds (wave_speed_init, :2003)
    ("thickdiff", "use_stanley_gm"): (1, 0),         # FATAL without STANLEY_COEFF >= 0 (:2334) ...
    ("thickdiff", "use_stanley_gm+coeff"): (0, 0),   # ... accepted with it
    ("thickdiff", "detangle_interfaces"): (0, 0), ("thickdiff", "Kh_eta_bg"): (0, 0), ("thickdiff", "Kh_eta_vel"): (0, 0),
    ("thickdiff", "use_GME"): (0, 0),
    ("thickdiff", "use_MEKE"): (0, 1),               # accepted; VarMix_init then wants Rd/dx and with it wave speeds (:1602, :1955)
    ("thickdiff", "read_khth+Khth"): (1, 2),         # FATAL: KHTH > 0 with READ_KHTH (:2218); the read and its pass_var leave the compiled files
    ("varmix", "use_stanley_iso"): (1, 0),           # FATAL without STANLEY_COEFF >= 0 (:1621) ...
    ("varmix", "use_stanley_iso+coeff"): (0, 0),     # ... accepted with it
    ("varmix", "debug"): (0, 0),
    ("varmix", "simpler_without_stored"): (1, 0),    # FATAL (:1722): the device refuses it too
}


def test_lateral_init_refusals_against_the_references():
    """Which members of abi.THICKNESS_DIFFUSE_MUST_BE_0 and abi.VARMIX_MUST_BE_0 the reference's own inits stop on: only the two
    Stanley switches without a coefficient (and KHTH > 0 with READ_KHTH, USE_SIMPLER_EADY_GROWTH_RATE without USE_STORED_SLOPES,
    which the device refuses as well).  Everything else the device refuses the reference accepts.  The members that no parameter
    sets (RP.THICKDIFF_NOT_PARAMS, RP.VARMIX_NOT_PARAMS: VarMix%use_variable_mixing, which VarMix_init sets TRUE by default, the OBC
    pointer, GV%Boussinesq, GV%nkml, the GMwork diagnostic, STOCH) cannot be asked of an init."""
    assert {k[1].split("+")[0] for k in LATERAL_REFUSALS if k[0] == "thickdiff"} | set(RP.THICKDIFF_NOT_PARAMS) >= set(abi.THICKNESS_DIFFUSE_MUST_BE_0)
    assert {k[1].split("+")[0] for k in LATERAL_REFUSALS if k[0] == "varmix"} | set(RP.VARMIX_NOT_PARAMS) >= set(abi.VARMIX_MUST_BE_0)
    _need_lib()
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=2)[1:]
    inp = TD.inputs(d, M, GV)
    for (kind, what), (own, never) in LATERAL_REFUSALS.items():
        member, _, extra = what.partition("+")
        tab = [("STANLEY_COEFF", 1.0)] if extra == "coeff" else []
        if kind == "thickdiff":
            P = abi.thickness_diffuse_params_default()
            if what == "read_khth+Khth":
                tab = [("READ_KHTH", True)]
            else:
                tab.append((RP.THICKDIFF_PARAM_NAMES[member][0], 1.0 if member.startswith("Kh_eta") else True))
            got, fatal = RP.thickness_diffuse(d, M, GV, P, inp, 0.0, table_extra=tab)
        else:
            P = abi.varmix_params_default(GV)
            if member == "simpler_without_stored":
                tab = [("USE_SIMPLER_EADY_GROWTH_RATE", True)]
            else:
                tab.append((RP.VARMIX_PARAM_NAMES[member][0], True))
            got, fatal = RP.calc_slope_functions(d, M, GV, P, inp, 0.0, table_extra=tab)
        n = RP.standin_never_count()
        assert (fatal - n, n) == (own, never), (kind, what, fatal, n)


def test_zz_record_the_tolerance_class():
    """profiles/ref_parity_libm.json: the largest difference over range of every tolerance-class field seen by the tests above
    (MOM6X_RECORD_REF_PARITY names the file).  Runs last in the file; without the library there is nothing to record."""
    _need_lib()
    print("tolerance class: largest difference / range:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})
    for k, v in WORST.items():
        assert v <= BOUND, (k, v)
    if os.environ.get("MOM6X_RECORD_REF_PARITY"):
        by_field = {}
        for k, v in WORST.items():
            case, field = k.rsplit(": ", 1)
            f = ("opacity " if "smooth_" in case or field == "opac_diag" else "ePBL ") + field
            by_field[f] = max(by_field.get(f, 0.0), v)
        json.dump(dict(reference="oracle/_ref/libref_param.so: MOM_opacity.F90 and MOM_energetic_PBL.F90 compiled with amdflang -O2 "
                                 "-ffp-contract=off, against numpy and python's math",
                       bound=BOUND, largest_difference_over_range=by_field, by_case={k: v for k, v in sorted(WORST.items()) if v > 0.0}),
                  open(os.environ["MOM6X_RECORD_REF_PARITY"], "w"), indent=1)


# ------------------------------------------------------------------------------------------------------------------------------
# recorded results

def _restatement(kind, d, M, GV, P, opt, inp, counts=False):
    if kind in ("varmix", "thickdiff"):
        return _lateral_restatement(kind, d, M, GV, P, opt, inp, counts)
    if kind == "kshear":
        return K.run(d, M, GV, P, opt, inp)[0]
    if kind == "ndiff":
        return {n: a for n, a in N.run(d, M, GV, P, opt, inp)[0].items() if n in RP.NDIFF_OUT}
    if kind == "opacity":
        return R.run(d, M, GV, P, opt, inp)[0]
    return E.run(d, M, GV, P, opt, inp)[0]


def _lateral_restatement(kind, d, M, GV, P, opt, inp, counts=False):
    """The restatement on a recorded varmix or thickdiff configuration (NaN inputs beyond what the reference reads), every output
    cut to its range as the recorder cuts the door's; or its branch counts."""
    from oracle import orc
    orc.build()
    if kind == "varmix":
        want, c = V.run(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"], give_diag=True, orc=orc)
        rng = _written(d, P, want, "recorded")
        return c if counts else {n: np.ascontiguousarray(want[n][rng[n]]) for n in rng}
    rng = RP.thickdiff_ranges(d)
    if opt["chain"] is None:
        want, c = TD.run(d, M, GV, P, inp, opt["dt"], eos=opt["eos"], give_ps=opt["give_ps"], stored=opt["stored"], give_gm=True, orc=orc)
        return c if counts else {n: np.ascontiguousarray(want[n][(Ellipsis,) + rng[n]]) for n in RP.THICKDIFF_OUT}
    Pv = opt["chain"]
    w = dict(SN_u=np.full(d.shape2(), np.nan), SN_v=np.full(d.shape2(), np.nan), slope_x=np.full(d.shape3(d.nk + 1), np.nan),
             slope_y=np.full(d.shape3(d.nk + 1), np.nan))
    Rlay, gp = abi.layer_densities(d.nk)
    io = {n: inp[n].copy() for n in RP.THICKDIFF_CORE}
    V.calc_slope_functions(d, M, GV, Pv, io["h"], opt["dt"], w["SN_u"], w["SN_v"], T=inp["T"], S=inp["S"], eos=opt["eos"], Rlay=Rlay,
                           g_prime=gp, slope_x=w["slope_x"], slope_y=w["slope_y"], orc=orc)
    c = TD.thickness_diffuse(d, M, GV, P, io["h"], io["uhtr"], io["vhtr"], opt["dt"], T=inp["T"], S=inp["S"], eos=opt["eos"],
                             slope_x=w["slope_x"], slope_y=w["slope_y"], orc=orc)
    rv = RP.varmix_ranges(d, Pv)
    out = {n: np.ascontiguousarray(io[n][(Ellipsis,) + rng[n]]) for n in RP.THICKDIFF_CORE}
    out.update({n: np.ascontiguousarray(w[n][rv[n]]) for n in RP.VARMIX_MEMBERS})
    return c if counts else out


def _lateral_golden_names(kind, name, gold, out):
    """CORE <= recorded <= exposed, and what is left out is the head of the kind's drop order."""
    core = set(RP.VARMIX_CORE if kind == "varmix" else RP.THICKDIFF_CORE) & set(out)
    order = [n for n in (RP.CHAIN_DROP_ORDER if name == "chain" else RP.VARMIX_DROP_ORDER if kind == "varmix" else RP.THICKDIFF_DROP_ORDER)
             if n in out]
    left_out = sorted(set(out) - set(gold))
    assert core <= set(gold) <= set(out) and left_out == sorted(order[:len(left_out)]), (sorted(gold), sorted(out))


def _against_golden(tag, kind, d, M, gold, out):
    """`out` (whole arrays) against the recorded computational domain, in the classes of the live comparisons."""
    if kind in ("varmix", "thickdiff"):      # both sides are cut to the ranges the reference writes; finite there, bit for bit
        _lateral_golden_names(kind, tag.split("_")[2], gold, out)
        for n in gold:
            assert np.isfinite(out[n]).all(), (tag, n)
            H.assert_bitwise(out[n], np.ascontiguousarray(gold[n]), f"{tag}: {n}")
        return
    if kind == "ndiff":                  # lists of arrays, each on its own range; a file over the size limit leaves out diagnostics
        left_out = sorted(set(out) - set(gold))
        assert set(RP.NDIFF_CORE) <= set(gold) <= set(out) == set(RP.NDIFF_OUT), sorted(gold)
        assert left_out == sorted(RP.NDIFF_DROP_ORDER[:len(left_out)]), sorted(gold)
        for n in gold:
            assert len(gold[n]) == len(out[n]), (tag, n)
            for m, (a, b) in enumerate(zip(out[n], gold[n])):
                H.assert_bitwise(np.ascontiguousarray(a[(Ellipsis,) + RP.ndiff_ranges(d)[n]]), np.ascontiguousarray(b), f"{tag}: {n}[{m}]")
        return
    dm = RP.dom(d)
    wet = (M[G["mask2dT"]] > 0.0)[dm]
    names = set(out) - set(RP.EPBL_NOT_EXPOSED) - set(RP.KSHEAR_NOT_EXPOSED)
    if kind == "kshear":                 # a file that would pass the size limit leaves out diagnostics, the last named first
        left_out = sorted(names - set(gold))
        assert set(RP.KSHEAR_CORE) <= set(gold) <= names and left_out == sorted(RP.KSHEAR_DROP_ORDER[:len(left_out)]), sorted(gold)
    else:
        assert set(gold) == names, (sorted(gold), sorted(names))
    for n in gold:
        a, b = out[n][(Ellipsis,) + dm], gold[n]
        if n in RP.EPBL_WET_ONLY:
            a, b = a[..., wet], b[..., wet]
        _held(np.ascontiguousarray(a), np.ascontiguousarray(b), f"{tag}: {n}", n not in R.OUT_TRANSCENDENTAL)


def test_restatements_against_the_recorded_reference():
    """Never skips: the restatements on the recorded configurations against tests/golden/ref_*.npz, whose inputs are regenerated
    from the seeded case_inputs and checked against the stored SHA-256."""
    for kind, name, grid, kw in RP.golden_configs():
        d, M, GV, P, opt, inp = RP.golden_setup(kind, name, grid, kw)
        gold = RP.load_golden(kind, name, grid, kw, M, inp)
        _against_golden(RP.golden_name(kind, name, grid, kw), kind, d, M, gold, _restatement(kind, d, M, GV, P, opt, inp))


def test_recorded_reference_is_what_the_library_gives():
    """The doors again on the recorded configurations: bit for bit what tests/golden holds (scripts/record_ref_parity.py)."""
    _need_lib()
    for kind, name, grid, kw in RP.golden_configs():
        d, M, GV, P, opt, inp = RP.golden_setup(kind, name, grid, kw)
        gold = RP.load_golden(kind, name, grid, kw, M, inp)
        got, fatal = RP.DOORS[kind](d, M, GV, P, opt, inp)
        assert fatal == 0
        if kind in ("ndiff", "varmix", "thickdiff"):
            _against_golden(RP.golden_name(kind, name, grid, kw), kind, d, M, gold, got)
            continue
        dm = (Ellipsis,) + RP.dom(d)
        assert set(got) == set(gold) if kind != "kshear" else set(gold) <= set(got)
        for n in gold:
            if n in RP.EPBL_WET_ONLY:
                wet = (M[G["mask2dT"]] > 0.0)[RP.dom(d)]
                H.assert_bitwise(got[n][dm][wet], gold[n][wet], f"{name}: {n}")
            else:
                H.assert_bitwise(got[n][dm], gold[n], f"{name}: {n}")
    largest = max(os.path.getsize(os.path.join(RP.GOLDEN, f)) for f in os.listdir(RP.GOLDEN) if f.startswith("ref_"))
    assert largest <= 248 * 1024, largest
