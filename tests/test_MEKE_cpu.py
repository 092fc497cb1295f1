"""step_forward_MEKE's restatement (tests/meke_ref.py) held to facts that do not come from it: the closed forms of the two
equilibria, the sign change of the residual across the root find's bracket, the bits of pure damping, the conservation of
sum(areaT*mass*MEKE) by the fluxes, the maximum principle of the limited Laplacian diffusion, the grid-scale mixing length, the
quarter turn, unit scaling, tile cuts and the branches its case list reaches; and the exports and ABI size of the device routine.
The device is held to the restatement in tests/test_MEKE_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import meke_ref as R
from tests.test_thickness_diffuse_cpu import _bits, _flat
from tests.test_varmix_cpu import TILES

G = abi.G
EPS = float(np.finfo(np.float64).eps)


def _grid(name, part=None):
    def make(nk, layout=(1, 1), pe=(0, 0)):
        d, M = getattr(H, name)(nk=nk, layout=layout, pe=pe)[1:]
        if part is not None:
            M = part(d, M)
        M, dF_dx, dF_dy = R.metrics(d, M)
        return d, M, (dF_dx, dF_dy)
    return make


# the grids of tests/test_mixed_layer_restrat_cpu.py, each with an equator and with G%dF_dx, G%dF_dy
GRIDS = {"benchmark_small": _grid("benchmark_small"), "island_basin": _grid("island_basin"),
         "partial_faces": _grid("benchmark_small", H.partial_faces)}


def cut_from_one_tile(d, dt_, name, tile, one):
    """A tile's part of a plane and the same points of the one-tile plane: MEKE, Kh, Ku, Au, Le with the tile's whole halo, as the
    group passes leave it, wherever that lies over the one-tile array's own halo; a diagnostic at the tile's own points or faces."""
    e = dt_.halo if name in R.STATE else 0
    rs, cs = H.interior(dt_, R.DIAG_STAG.get(name, "h"), extra=e)
    dj, di = dt_.j_glob0 - dt_.joff + d.joff, dt_.i_glob0 - dt_.ioff + d.ioff
    r0, r1 = max(rs.start, d.joff - d.halo - dj), min(rs.stop, d.joff + d.nj + d.halo - dj)
    c0, c1 = max(cs.start, d.ioff - d.halo - di), min(cs.stop, d.ioff + d.ni + d.halo - di)
    return tile[..., r0:r1, c0:c1], one[..., r0 + dj:r1 + dj, c0 + di:c1 + di]


def _case_run(grid, nk, name, mods=None, inp_mods=None, give_diag=None, fill=np.nan, given=None):
    d, M, dF = GRIDS[grid](nk) if isinstance(grid, str) else grid
    GV = abi.vgrid_default()
    P, gv, dg, dt = R.case(name, GV)
    for k, v in (mods or {}).items():
        setattr(P, k, v)
    inp = R.inputs(d, M, GV)
    inp.update(inp_mods(d, M, inp) if inp_mods else {})
    out, counts, npass = R.run(d, M, GV, P, inp, dt, dF, given=gv if given is None else given,
                               give_diag=dg if give_diag is None else give_diag, fill=fill)
    return d, M, GV, P, inp, out, counts, dt


def test_exports_struct_size_and_defaults():
    lib = abi.load_library()
    for n in ("mom6x_MEKE_init", "mom6x_MEKE_set_initialized", "mom6x_step_forward_MEKE"):
        assert hasattr(lib, n), n
    assert lib.mom6x_struct_size(23) == C.sizeof(abi.MEKEParams)
    assert lib.mom6x_struct_size(24) == -1
    assert lib.mom6x_abi_version() == 6
    p = abi.MEKE_params_default()
    assert (p.MEKE_damping, p.MEKE_Cd_scale, p.MEKE_Cb, p.MEKE_min_gamma, p.MEKE_Ct) == (0.0, 0.0, 25.0, 1.0e-4, 50.0)    # :1400-1418
    assert (p.MEKE_GMcoeff, p.MEKE_FrCoeff, p.MEKE_bhFrCoeff, p.MEKE_GMECoeff) == (-1.0, -1.0, -1.0, -1.0)
    assert (p.MEKE_GEOMETRIC, p.MEKE_GEOMETRIC_alpha, p.MEKE_equilibrium_alt, p.MEKE_equilibrium_restoring) == (0, 0.05, 0, 0)
    assert p.MEKE_restoring_rate == 1.0 / 1.0e6
    assert (p.MEKE_BGsrc, p.MEKE_Kh, p.MEKE_K4, p.MEKE_dtScale, p.MEKE_positive, p.MEKE_KhCoeff, p.MEKE_Uscale) == (0.0, -1.0, -1.0, 1.0, 0,
                                                                                                                  1.0, 0.0)
    assert (p.GM_src_alt, p.MEKE_min_depth_tot, p.visc_drag, p.KhMEKE_Fac) == (0, 1.0, 1, 0.0)
    assert (p.use_old_lscale, p.use_min_lscale, p.lscale_maxval, p.Rd_as_max_scale) == (0, 0, 1.0e7, 0)
    assert (p.viscosity_coeff_Ku, p.viscosity_coeff_Au, p.Lfixed, p.fixed_total_depth) == (0.0, 0.0, 0.0, 1)
    assert (p.aDeform, p.aRhines, p.aEady, p.aFrict, p.aGrid) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert (p.MEKE_advection_factor, p.MEKE_advection_bug, p.MEKE_topographic_beta, p.cdrag, p.cold_start) == (0.0, 0, 0.0, 0.003, 0)
    assert (p.T_to_s, p.L_to_m, p.m_s_to_L_T) == (1.0, 1.0, 1.0)
    assert abi.MEKE_MUST_BE_0 == ("eke_source_file", "eke_source_dbclient", "use_Kh_diff", "non_Boussinesq", "open_bcs", "debug")
    assert all(getattr(p, n) == 0 for n in abi.MEKE_MUST_BE_0)
    assert [f for f, _ in abi.MEKEParams._fields_][-6:] == list(abi.MEKE_MUST_BE_0)


def test_the_halo_requirement_of_K4_is_in_the_library():
    """mom6x_MEKE_init asks for a context halo of two with MEKE_K4 >= 0 and of one otherwise.  mom6x_ctx_create itself asks for three
    (continuity_PPM), so today no context can fall short and the check cannot be made to fire; it stands for a context with a
    smaller halo, and this only sees that it was compiled in."""
    txt = open(abi.LIB_PATH, "rb").read()
    assert b"MEKE_K4 >= 0 (the biharmonic of MEKE) needs a halo of two" in txt


def _SN_of(d, inp):
    s = H.interior(d, "h")
    r, c = s
    west = (r, slice(c.start - 1, c.stop - 1))
    south = (slice(r.start - 1, r.stop - 1), c)
    return np.minimum(np.minimum(inp["SN_u"][s], inp["SN_u"][west]), np.minimum(inp["SN_v"][s], inp["SN_v"][south]))


@pytest.mark.parametrize("grid", ["benchmark_small", "island_basin"])
def test_equilibrium_alt_is_its_closed_form(grid):
    """MEKE_EQUILIBRIUM_ALT: the first call starts from (alpha*SN*depth)**2/cd2 (:1037) exactly -- checked with every source,
    every damping and the fluxes off (MEKE_Cd_scale = 0, no visc_drag, so the step leaves MEKE alone)."""
    mods = dict(MEKE_Cd_scale=0.0, visc_drag=0, MEKE_KhCoeff=0.0)
    d, M, GV, P, inp, out, counts, dt = _case_run(grid, 8, "equil_alt", mods=mods, given=())
    s = H.interior(d, "h")
    depth = (M[G["bathyT"]][s] + 0.0) * GV.Z_to_H
    t = (P.MEKE_GEOMETRIC_alpha * _SN_of(d, inp)) * depth
    want = (t * t) / (P.cdrag * P.cdrag)
    assert counts["equil_alt"] == want.size and want.max() > 0
    _bits(out["MEKE"][s], want * M[G["mask2dT"]][s], "MEKE of the alternative equilibrium")


def _closed_form_setup(grid):
    d, M, dF = GRIDS[grid](8)
    GV = abi.vgrid_default()
    P = abi.MEKE_params_default(GV, MEKE_Cb=0.0, MEKE_Ct=0.0, MEKE_Cd_scale=1.0, use_old_lscale=1, MEKE_damping=0.0, MEKE_Uscale=0.0,
                                visc_drag=0, fixed_total_depth=0)
    inp = R.inputs(d, M, GV)
    return d, M, dF, GV, P, inp


@pytest.mark.parametrize("grid", ["benchmark_small", "island_basin"])
def test_general_equilibrium_against_its_closed_form(grid):
    """With MEKE_Cb = MEKE_Ct = 0, MEKE_Cd_scale = 1, MEKE_OLD_LSCALE, MEKE_damping = 0, MEKE_Uscale = 0 and no visc_drag:
    gamma_b**2 = gamma_t**2 = 1 and L = sqrt(areaT), so resid(E) = KhCoeff*sqrt(2E)*L*SN**2 - c*sqrt(cd2*2E)*E with
    c = H_to_RZ*I_mass = 1/D (D the column's thickness), whose positive root is E* = KhCoeff*L*SN**2/(c*cdrag) =
    KhCoeff*L*SN**2*D/cdrag.  The root find returns a point of a bracket no wider than 1e-12 m2 s-2 (:1027, :1108) on whose ends
    the COMPUTED residual has opposite signs.  The computed source carries at most 4 roundings (sqrt, *L, SN*SN, the product) and
    the computed damping 4 (cdrag*cdrag and cd2*2E under the square root, the square root, c*, *E; 2*E and the factors 1 are
    exact), so the computed sign is the true one whenever |E - E*| > 8*eps*E*; E* as formed here has 4 roundings of its own.  Hence
    |E - E*| <= 1e-12 + 16*eps*E*.

    Where that holds.  The loop of :1108-1134 stops on EKEerr = min(EKE - EKEmin, EKEmax - EKE), the distance of the newest point
    from the nearer end of the bracket.  With the bisection that is half the width and the bound follows.  With the secant it is
    the length of one step of a regula falsi: the residual is concave, the secant's point falls left of the root and only EKEmin
    moves, so the root lies beyond the last point by that step times r/(1 - r), r the contraction of the iteration.  For this
    residual, with x = E/E* and b = EKEmax/E*, g(x) = sqrt(x)*(1 - x), g'(1) = -1 and r = 1 + g'(1)*(b - 1)/g(b) = 1 - 1/sqrt(b),
    r/(1 - r) = sqrt(b) - 1.  When the secant is switched on inside the bisection (:1125: two left points in a row, L1 < L2, with a
    falling residual) the right end is 2*L2 - L1 < 2*E*, so b < 2 and the root is within 0.42 of the step: the bound holds.  It is
    switched on in the bracket search (:1092) only at a second widening, which leaves b anywhere up to 10 and the root up to 2.2
    steps away: there the routine does not keep to its own tolerance (seen: 2.1e-12 m2 s-2 with Eady growth rates of 4e-6 s-1, which
    put E* at 1-100 m2 s-2).  The condition, then, is that no column widens its bracket twice, E* <= 0.1 m2 s-2, ten times the
    reference's own first guess; tests/meke_ref.inputs keeps SN_u, SN_v at oceanic 0.8e-7 .. 7.2e-7 s-1, which gives
    E* = L*SN**2*D/cdrag <= 1e5*(7.2e-7)**2*4000/0.003 = 0.07 m2 s-2, and the condition is asserted below, column by column."""
    d, M, dF, GV, P, inp = _closed_form_setup(grid)
    s = H.interior(d, "h")
    counts = dict.fromkeys(R.BRANCHES, 0)
    mass = np.zeros(d.shape2())
    for k in range(d.nk):
        mass = mass + M[G["mask2dT"]] * (GV.H_to_RZ * inp["h"][k])
    SN, area = _SN_of(d, inp), M[G["areaT"]][s]
    checked, beyond, worst = 0, 0, 0.0
    for j in range(SN.shape[0]):
        for i in range(SN.shape[1]):
            m = mass[s][j, i]
            Im = 1.0 / m if m > 0.0 else 0.0
            w0 = counts["bracket_widened"]
            E, _ = R.equilibrium_column(P, GV, float(area[j, i]), 0.0, float(m * GV.RZ_to_H), 0.0, float(SN[j, i]), Im, 0.0, counts)
            assert counts["bracket_widened"] - w0 <= 1, "the condition of the bound: no second widening of the bracket"
            if Im * SN[j, i] > 0.0:
                star = P.MEKE_KhCoeff * math.sqrt(area[j, i]) * SN[j, i] * SN[j, i] / ((GV.H_to_RZ * Im) * P.cdrag)
                worst = max(worst, abs(E - star) - 16 * EPS * star)
                beyond += abs(E - star) > 1.0e-12 + 16 * EPS * star
                checked += 1
            else:
                assert E == 0.0
    print(f"{grid}: {checked} columns, {beyond} beyond the bound, largest |E - E*| less the rounding term {worst}")
    assert checked > 300 and counts["secant_used"] > 0 and (grid != "benchmark_small" or counts["bracket_widened"] > 100)
    assert beyond == 0, (beyond, worst)


@pytest.mark.parametrize("name", ["equil", "equil_old", "pow_equil"])
def test_the_residual_changes_sign_across_the_bracket(name):
    """For every column of the general cases: the residual -- written out here from :1077-1081 with the length-scale factors of the
    last bracket call, which the bisection keeps using (:1117-1121) -- is >= 0 at E - tol and <= 0 at E + tol, tol = 1e-12 m2 s-2.

    As test_general_equilibrium_against_its_closed_form derives, the loop stops on the length of the secant's last step, and that
    bounds the distance to the root when the secant was switched on inside the bisection (the right end of the bracket is then
    within twice the root), not when the bracket search switched it on at a second or later widening (:1092) and the bisection kept
    it.  (With length scales that depend on E the bisection drops such a secant at its first step: ResMin comes from the search's
    own factors, :1122.)  The condition -- no column ends in a secant kept from the search, "secant_kept_from_search" of
    tests/meke_ref.py -- is asserted, and the inputs (SN of oceanic size) meet it."""
    d, M, dF = GRIDS["benchmark_small"](8)
    GV = abi.vgrid_default()
    P, given, _, dt = R.case(name, GV)
    inp = R.inputs(d, M, GV)
    counts = dict.fromkeys(R.BRANCHES, 0)
    s = H.interior(d, "h")
    visc = {n: inp[n] for n in R.VISC} if all(n in given for n in R.VISC) else None
    drv = R.drag_rate_visc(d, M, P, visc, counts)
    depth = (M[G["bathyT"]][s] + 0.0) * GV.Z_to_H
    mass = np.zeros(d.shape2())
    for k in range(d.nk):
        mass = mass + M[G["mask2dT"]] * (GV.H_to_RZ * inp["h"][k])
    Im = np.where(mass[s] > 0, 1.0 / np.where(mass[s] > 0, mass[s], 1.0), 0.0)
    dt_full = np.full(d.shape2(), np.nan); dt_full[H.interior(d, "h", extra=1)] = ((M[G["bathyT"]] + 0.0) * GV.Z_to_H)[H.interior(d, "h", extra=1)]
    beta = np.zeros(depth.shape) if P.use_old_lscale else R._beta(d, M, GV, P, dt_full, dF[0], dF[1], counts)
    SN, area, Rd = _SN_of(d, inp), M[G["areaT"]][s], inp["Rd_dx_h"][s]
    tol, checked, missed = 1.0e-12, 0, 0

    def resid(E, b, t, L, sn, im, dv):
        Kh = P.MEKE_KhCoeff * math.sqrt(2.0 * t * E) * L
        drag = (GV.H_to_RZ * im) * math.sqrt(dv * dv + P.cdrag ** 2 * (2.0 * b * E + P.MEKE_Uscale ** 2))
        return Kh * sn * sn - (P.MEKE_damping + drag * b) * E
    for j in range(SN.shape[0]):
        for i in range(SN.shape[1]):
            a = (float(area[j, i]), float(beta[j, i]), float(depth[j, i]), float(Rd[j, i]), float(SN[j, i]), float(Im[j, i]), float(drv[j, i]))
            E, fac = R.equilibrium_column(P, GV, *a, counts)
            assert counts["secant_kept_from_search"] == 0, "the condition of the check: no secant kept from the bracket search"
            if fac is None:
                assert E == 0.0
                continue
            lo, hi = resid(max(E - tol, 0.0), *fac, a[4], a[5], a[6]), resid(E + tol, *fac, a[4], a[5], a[6])
            missed += not (lo >= 0.0 >= hi)
            checked += 1
    print(f"{name}: {checked} columns, {missed} without a sign change across [E - tol, E + tol]")
    assert checked > 300 and counts["secant_used"] > 0
    assert missed == 0, (missed, checked)


@pytest.mark.parametrize("split", [False, True])
def test_pure_damping_of_a_uniform_state(split):
    """MEKE uniform, only MEKE_damping and MEKE_BGsrc: with MEKE_Kh < 0 and MEKE_K4 < 0 damp_step = 1 and the step is the single
    division (M + sdt*src)/(1 + sdt*d); with MEKE_Kh = 0 (no diffusion of a uniform field, but the Strang split) it is the bits
    of ((M + sdt*src)/(1 + .5*sdt*d))/(1 + .5*sdt*d)."""
    d, M = _flat(4)
    M, dFx, dFy = R.metrics(d, M)
    GV = abi.vgrid_default()
    P = abi.MEKE_params_default(GV, MEKE_Cb=0.0, MEKE_Ct=0.0, visc_drag=0, MEKE_damping=3.0e-6, MEKE_BGsrc=2.0e-9, cold_start=1,
                                MEKE_KhCoeff=0.0, aGrid=1.0, MEKE_dtScale=1.5, MEKE_Kh=0.0 if split else -1.0)
    inp = R.inputs(d, M, GV)
    inp["h"] = np.full(d.shape3(), 4000.0 / d.nk)
    M0 = 0.0123
    inp["MEKE"] = M0 * M[G["mask2dT"]]
    dt = 3600.0
    out, _, _ = R.run(d, M, GV, P, inp, dt, (dFx, dFy))
    sdt = dt * 1.5
    if split:
        want = ((M0 + sdt * 2.0e-9) / (1. + (sdt * 0.5) * 3.0e-6)) / (1. + (sdt * 0.5) * 3.0e-6)
    else:
        want = (M0 + sdt * 2.0e-9) / (1. + (sdt * 1.) * 3.0e-6)
    s = H.interior(d, "h")
    wet = M[G["mask2dT"]][s] > 0
    assert wet.sum() > 500
    got = out["MEKE"][s]
    if split:      # the diffusive flux of a uniform field is (+-)0 between wet cells; next to land MEKE differs and diffuses
        inner = wet.copy()
        for ax, sh in ((0, 1), (0, -1), (1, 1), (1, -1)):
            inner &= np.roll(wet, sh, axis=ax)
        inner[0, :] = inner[-1, :] = False; inner[:, 0] = inner[:, -1] = False
        wet = inner
        assert wet.sum() > 400
    _bits(got[wet], np.full(int(wet.sum()), want), "damped MEKE")


def _mass(d, M, GV, h):
    mass = np.zeros(d.shape2())
    for k in range(d.nk):
        mass = mass + M[G["mask2dT"]] * (GV.H_to_RZ * h[k])
    return mass


@pytest.mark.parametrize("grid", ["benchmark_small", "island_basin"])
@pytest.mark.parametrize("name", ["kh_k4", "adv", "k4"])
def test_fluxes_conserve_the_mass_weighted_sum(grid, name):
    """No sources and no damping (MEKE_BGsrc = 0, MEKE_damping = 0, MEKE_Cd_scale = MEKE_Cb = 0, no visc_drag, no source plane):
    MEKE changes by sdt*IareaT*I_mass times the divergence of fluxes that vanish at land faces (their mass factor or transport is
    zero there), so sum(areaT*mass*MEKE) over the wet cells is conserved up to rounding: each cell's update has 4 differences and
    sums, 2 products and one addition per flux kind, all on terms bounded by sum_faces |flux|*sdt; a generous count is 16 roundings
    of that per cell and flux kind."""
    mods = dict(MEKE_BGsrc=0.0, MEKE_damping=0.0, MEKE_Cd_scale=0.0, visc_drag=0, MEKE_GMcoeff=-1.0, MEKE_positive=0)
    given = tuple(n for n in R.CASES[name][1] if n not in R.SOURCES + R.VISC)

    def positive(d, M, inp):
        return dict(MEKE=np.abs(inp["MEKE"]) + 1.0e-3 * M[G["mask2dT"]])
    d, M, GV, P, inp, out, counts, dt = _case_run(grid, 8, name, mods=mods, given=given, inp_mods=positive, give_diag=False)
    s = H.interior(d, "h")
    w = (M[G["areaT"]] * _mass(d, M, GV, inp["h"]))[s]
    before, after = (w * inp["MEKE"][s]).sum(), (w * out["MEKE"][s]).sum()
    assert not np.array_equal(out["MEKE"][s], inp["MEKE"][s])
    moved = (w * np.abs(out["MEKE"][s] - inp["MEKE"][s])).sum()
    assert abs(after - before) <= 64 * EPS * (before + moved) and moved > 1.0e-6 * before, (before, after, moved)


@pytest.mark.parametrize("grid", ["benchmark_small", "island_basin", "partial_faces"])
def test_laplacian_diffusion_obeys_the_maximum_principle(grid):
    """Laplacian diffusion alone (no source, no damping): Kh_u*Inv_Kh_max <= 1/4 after the limiter (:693-695), and Inv_Kh_max =
    2*sdt*(dy_Cu*IdxCu)*max(IareaT) with the harmonic mass 2*m1*m2/(m1+m2) <= 2*m(i,j) bounds each face's weight
    sdt*IareaT*I_mass*Kh*(dy_Cu*IdxCu)*mass_harm by 1/4, so the new value is a convex combination of the five-point neighbourhood:
    within its min and max up to one rounding of each of the ~10 terms.  Kh_u, Kh_v <= 0.25/Inv_Kh_max; a uniform field on
    non-uniform mass keeps its bits."""
    mods = dict(MEKE_damping=0.0, MEKE_Cd_scale=0.0, visc_drag=0, KhMEKE_Fac=1.0, MEKE_Kh=1000.0, MEKE_KhCoeff=0.0)
    d, M, GV, P, inp, out, counts, dt = _case_run(grid, 8, "kh", mods=mods, given=("Kh",), give_diag=True)
    assert counts["Kh_lim_Kh_present"] > 0
    s = H.interior(d, "h")
    r, c = s
    nb = [inp["MEKE"][s]] + [inp["MEKE"][(slice(r.start + dj, r.stop + dj), slice(c.start + di, c.stop + di))]
                              for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0))]
    # a closed face carries no flux: its neighbour does not bound the value, the cell itself does
    lo, hi = np.min(nb, axis=0), np.max(nb, axis=0)
    wet = M[G["mask2dT"]][s] > 0
    tol = 16 * EPS * np.max(np.abs(nb), axis=0)
    new = out["MEKE"][s]
    assert (new[wet] >= (lo - tol)[wet]).all() and (new[wet] <= (hi + tol)[wet]).all()
    sdt = dt * P.MEKE_dtScale
    for st, ln, Il, far in (("u", "dy_Cu", "IdxCu", (0, 1)), ("v", "dx_Cv", "IdyCv", (1, 0))):
        f = H.interior(d, st)
        fr = (slice(f[0].start + far[0], f[0].stop + far[0]), slice(f[1].start + far[1], f[1].stop + far[1]))
        Inv = 2.0 * sdt * ((M[G[ln]][f] * M[G[Il]][f]) * np.maximum(M[G["IareaT"]][f], M[G["IareaT"]][fr]))
        with np.errstate(divide="ignore"):
            assert (out["Kh_" + st][f] * Inv <= 0.25 * (1 + 2 * EPS)).all()
    uni = dict(MEKE=0.0371 * np.ones(d.shape2()))
    d, M, GV, P, inp, out, _, _ = _case_run(grid, 8, "kh", mods=mods, given=("Kh",), inp_mods=lambda *_: uni)
    wetfull = M[G["mask2dT"]] > 0
    interior = np.zeros(d.shape2(), bool); interior[s] = True
    _bits(out["MEKE"][interior & wetfull], inp["MEKE"][interior & wetfull], "a uniform field")


@pytest.mark.parametrize("min_lscale", [1, 0])
def test_the_grid_scale_mixing_length_and_MEKE_positive(min_lscale):
    """With MEKE_ALPHA_GRID alone LmixScale is aGrid*sqrt(areaT): exactly in the MEKE_MIN_LSCALE form (a MIN with the ceiling
    1e7 m), within one ulp in the harmonic form (1/(1/x): two roundings).  MEKE_POSITIVE leaves no negative value."""
    mods = dict(use_min_lscale=min_lscale, aGrid=0.75, MEKE_positive=1)
    d, M, GV, P, inp, out, counts, _ = _case_run("island_basin", 8, "gm", mods=mods, give_diag=True)
    s = H.interior(d, "h")
    want = 0.75 * np.sqrt(M[G["areaT"]][s])
    got = out["LmixScale"][s]
    if min_lscale:
        _bits(got, want, "LmixScale")
    else:
        assert (np.abs(got - want) <= np.spacing(want)).all()
    assert (inp["MEKE"][s] < 0).any() and (out["MEKE"][s] >= 0).all() and counts["positive_clip"] > 0
    assert not np.signbit(out["MEKE"][s]).any()


def _turned(T, inp, dF):
    """The inputs on the grid turned by a quarter: cell (i, j) -> (nj-1-j, i), so x' runs along -y and y' along x."""
    out = {n: T.h(inp[n]) for n in ("h", "MEKE", "Kh", "Rd_dx_h") + R.SOURCES}
    out["hu"], out["hv"] = T.v_to_u(inp["hv"]), T.u_to_v(inp["hu"])
    for a in ("SN_", "Kv_bbl_", "bbl_thick_"):
        out[a + "u"], out[a + "v"] = T.v_to_u(inp[a + "v"], sign=1.0), T.u_to_v(inp[a + "u"])
    return out, (T.h(-dF[1]), T.h(dF[0]))


@pytest.mark.parametrize("name", ["kh_k4", "adv", "topo_beta", "visc", "equil"])
def test_quarter_turn(name):
    """Cell (i, j) -> (nj-1-j, i): every h-point result of the turned problem is the turned result, bit for bit, and Kh_u | Kh_v
    of the turned problem are Kh_v | Kh_u of the original.  Every sum the routine forms over a cell's four faces or four vertices
    pairs opposite faces or diagonal vertices, a turn swaps the pairs, and addition is commutative; a flux changes sign with its
    direction, which is exact."""
    from tests.test_oracle_invariants_cpu import Turn
    d, M, dF = GRIDS["island_basin"](6)
    GV = abi.vgrid_default()
    P, given, _, dt = R.case(name, GV)
    inp = R.inputs(d, M, GV)
    a, _, _ = R.run(d, M, GV, P, inp, dt, dF, given=given, give_diag=True, fill=0.0)
    T = Turn(d)
    tin, tdF = _turned(T, inp, dF)
    b, _, _ = R.run(T.dr, T.metrics(M), GV, P, tin, dt, tdF, given=given, give_diag=True, fill=0.0)
    slh, slu, slv = H.interior(T.dr, "h"), H.interior(T.dr, "u"), H.interior(T.dr, "v")
    assert not np.array_equal(a["MEKE"], inp["MEKE"])
    for n in a:
        if n in ("Kh_u", "Kh_v"):
            continue
        _bits(b[n][slh], T.h(a[n])[slh], f"{name}: {n}'")
    _bits(b["Kh_u"][slu], T.v_to_u(a["Kh_v"], sign=1.0)[slu], name + ": Kh_u'")
    _bits(b["Kh_v"][slv], T.u_to_v(a["Kh_u"])[slv], name + ": Kh_v'")


def scaled_MEKE(d, M, GV, P, inp, dF, dt, dim, p=11):
    """The problem in units scaled by 2**p in one of T, L, H, Z, R: the metrics, GV and dt from thickness_diffuse's scaled(), the
    module's members, inputs and Coriolis gradients here; and the factors that unscale the outputs."""
    from tests.test_thickness_diffuse_cpu import scaled
    sc = dict(T=1.0, L=1.0, H=1.0, Z=1.0, R=1.0)
    sc[dim] = 2.0 ** p
    T_, L, Hs, Z, Rr = sc["T"], sc["L"], sc["H"], sc["Z"], sc["R"]
    zero = np.zeros(1)
    dummy = dict(h=inp["h"], T=zero, S=zero, p_surf=zero, khth2d=zero, uhtr=zero, vhtr=zero, slope_x=zero, slope_y=zero)
    M2, GV2, _, _, dt2, _ = scaled(d, M, GV, abi.thickness_diffuse_params_default(), dummy, dt, dim, p)
    P2 = abi.MEKEParams.from_buffer_copy(P)
    for n, f in (("MEKE_damping", 1 / T_), ("MEKE_restoring_rate", 1 / T_), ("MEKE_BGsrc", L * L / T_ ** 3), ("MEKE_Kh", L * L / T_),
                 ("MEKE_K4", L ** 4 / T_), ("MEKE_Uscale", L / T_), ("MEKE_min_depth_tot", Hs), ("lscale_maxval", L), ("Lfixed", L),
                 ("cdrag", Hs / L), ("T_to_s", 1 / T_), ("L_to_m", 1 / L), ("m_s_to_L_T", L / T_)):
        setattr(P2, n, getattr(P, n) * f)
    src = Rr * Z * L * L / T_ ** 3
    fac = dict(h=Hs, hu=Hs * L * L, hv=Hs * L * L, SN_u=1 / T_, SN_v=1 / T_, Kv_bbl_u=Hs * Z / T_, Kv_bbl_v=Hs * Z / T_, bbl_thick_u=Z,
               bbl_thick_v=Z, MEKE=L * L / T_ ** 2, Kh=L * L / T_, Rd_dx_h=1.0, GM_src=src, mom_src=src, mom_src_bh=src, GME_snk=src)
    in2 = {n: inp[n] * fac[n] for n in inp}
    dF2 = (dF[0] / (T_ * L), dF[1] / (T_ * L))
    e, kh, rate = T_ ** 2 / (L * L), T_ / (L * L), T_ ** 3 / (L * L)
    un = dict(MEKE=e, Kh=kh, Ku=kh, Au=T_ / L ** 4, Le=1 / L, src=rate, src_adv=rate, src_mom_K4=rate, src_btm_drag=rate, src_GM=rate,
              src_mom_lp=rate, src_mom_bh=rate, decay=T_, Kh_u=kh, Kh_v=kh, LmixScale=1 / L, LRhines=1 / L, LEady=1 / L, Ue=T_ / L,
              Ub=T_ / L, Ut=T_ / L, gamma_b=1.0, gamma_t=1.0)
    return M2, GV2, P2, in2, dF2, dt2, un


@pytest.mark.parametrize("name", ["kh_k4", "adv", "mom_bh", "topo_beta", "visc", "min_lscale", "gm_alt", "restoring", "equil", "equil_alt"])
def test_unit_scaling_by_2_to_the_11(name):
    """Every dimension of MOM_unit_scaling.F90 in turn, T, L, H, Z, R scaled by 2**11: the unscaled results keep their bits (the
    square roots are of even powers of the factor; the bracket, the tolerance and the floors of the root find and of the length
    scales carry US%m_s_to_L_T, US%T_to_s, US%L_to_m)."""
    d, M, dF = GRIDS["benchmark_small"](6)
    GV = abi.vgrid_default()
    P, given, _, dt = R.case(name, GV)
    inp = R.inputs(d, M, GV)
    ref, _, _ = R.run(d, M, GV, P, inp, dt, dF, given=given, give_diag=True, fill=0.0)
    for dim in "TLHZR":
        M2, GV2, P2, in2, dF2, dt2, un = scaled_MEKE(d, M, GV, P, inp, dF, dt, dim)
        got, _, _ = R.run(d, M2, GV2, P2, in2, dt2, dF2, given=given, give_diag=True, fill=0.0)
        for n in ref:
            _bits(got[n] * un[n], ref[n], f"{name}.{dim}:{n}")


@pytest.mark.parametrize("name", ["kh_k4", "adv", "visc", "topo_beta"])
def test_tile_cuts(name):
    """The tiles of a 2 x 1, of a 1 x 2 and of a 2 x 2 layout in lockstep, each on its cut of the inputs and with the restatement's
    halo fill between them: every plane of every tile, halos included, equals the one-tile result where it lies over it."""
    GV = abi.vgrid_default()
    d, M, dF = GRIDS["benchmark_small"](8)
    P, given, dg, dt = R.case(name, GV)
    one, _, npass1 = R.run(d, M, GV, P, R.inputs(d, M, GV), dt, dF, given=given, give_diag=dg)
    for layout in ((2, 1), (1, 2), (2, 2)):
        pes = [pe for lay, pe in TILES if lay == layout]
        assert len(pes) == layout[0] * layout[1]
        tiles = []
        for pe in pes:
            dt_, Mt, dFt = GRIDS["benchmark_small"](8, layout=layout, pe=pe)
            tiles.append((dt_, Mt, dFt, R.inputs(dt_, Mt, GV)))
        res = R.run_tiles(tiles, GV, P, dt, given, dg)
        for (dt_, _, _, _), (out, npass) in zip(tiles, res):
            assert npass == npass1
            for n in one:
                mine, part = cut_from_one_tile(d, dt_, n, out[n], one[n])
                _bits(mine, part, f"tile {layout} at {dt_.i_glob0},{dt_.j_glob0} {name}:{n}")


REQUIRED = tuple(b for b in R.BRANCHES if b not in ("Kh_lim_Kh_absent", "secant_kept_from_search", "pow"))


def test_the_case_list_reaches_every_branch():
    """Counted over the pow-free case list on benchmark_small and island_basin at 8 layers: each source plane, the alternative GM
    form, the restoring, the biharmonic and the Laplacian fluxes with their limiters firing and not, KhMEKE_Fac, advection by
    transports of either sign and zero, the bug arm, visc_drag on and off, both depth forms, MEKE_POSITIVE, a negative MEKE that is
    not damped, every form of the mixing length and each term of the harmonic one, topographic beta, Kh, Ku, Au, Le, both
    equilibria, and in the root find the secant used, the secant dropped and the bracket widened.
    The condition of the one departure from the reference: in the arm without MEKE%Kh (max(0, MEKE_Kh) limited per face here,
    carried from face to face there) the limiter must not fire.  It fires when MEKE_Kh*2*sdt*(dy_Cu*IdxCu)*max(IareaT) > 1/4,
    i.e. MEKE_Kh > dx**2/(8*sdt) ~ 8e4 m2 s-1 on the finer of these grids (50 km, 3600 s); the cases of that arm use 1000 m2 s-1
    or less, and the count is 0 in every one of them.  With MEKE%Kh given (3e6 m2 s-1 in a patch, KhMEKE_Fac = 1) it fires."""
    tot = dict.fromkeys(R.BRANCHES, 0)
    for grid in ("benchmark_small", "island_basin"):
        for name in R.CASES_POW_FREE:
            *_, counts, _ = _case_run(grid, 8, name)
            assert counts["Kh_lim_Kh_absent"] == 0, name
            for k, v in counts.items():
                tot[k] += v
    print("branch counts:", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)
    assert tot["Kh_lim_Kh_present"] > 0 and tot["pow"] == 0
    *_, counts, _ = _case_run("benchmark_small", 8, "pow")
    assert counts["pow"] > 0
