"""What pins tests/ndiff_ref.py, the checker of mom6x_neutral_diffusion_calc_coeffs, mom6x_neutral_diffusion and
mom6x_tracer_hordiff_neutral, without a GPU.  The restatement and the kernels come from one reading of MOM_neutral_diffusion.F90.
That reading is held to the Fortran itself elsewhere: tests/test_ref_parity_cpu.py compares the restatement bit for bit with the
reference's own compiled module (oracle/_ref/libref_param.so, where it is built) and with results recorded from it
(tests/golden/ref_ndiff_*.npz, always), through the tracers, tendencies and transports; the coefficient arrays, which the compiled
module keeps private, the neutral branch of tracer_hordiff (MOM_tracer_hor_diff.F90 is not compiled) and the discontinuous
reconstruction stay outside that comparison.  The checks here need no compiled reference and stand on something else: the reference's
dimensional test (Z, L, T, H, R, C and S each rescaled by 2**11 leave the unscaled bits), the transposed grid with the
rotationally symmetric order of additions, a uniform tracer, the tracer content, invariants of the positions, the arms the case
table reaches on the grids of the GPU tests, two floors on how much of the `slope` case really slopes and diffuses, and the struct
and the init rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import ndiff_ref as R
from tests.test_oracle_invariants_cpu import SWAP

G = abi.G
EPS = 2.0 ** -52
# The arms the case table must reach on the grids the GPU tests use.  Of ARMS, left out:
#   ave_dx0            ppm_ave with dx == 0 (:1206): a sublayer of no extent in one column has hL or hR = 0, so its hEff is the
#                      harmonic mean 0 and neutral_surface_flux skips it (:2428) before it gets to ppm_ave
#   interp_equal_drho  :1589 dRhoPos - dRhoNeg == 0: the callers come with dRhoTop < dRhoBot (:1465, :1508), and the difference of two
#                      unequal doubles is not zero
#   bl_clamp_K, bl_clamp_P  the clamp :1541-1554 with bl_kl = bl_kr = 1, bl_zl = bl_zr = 0 (:543) is the identity: the test below
#                      holds the two counters to zero
NOT_REACHED = ("ave_dx0", "interp_equal_drho", "bl_clamp_K", "bl_clamp_P")
REQUIRED = tuple(a for a in R.ARMS if a not in NOT_REACHED)


def _bits(a, b, name):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if a.dtype == np.float64:
        ne = a.view(np.int64) != b.view(np.int64)
    else:
        ne = a != b
    assert not ne.any(), f"{name}: {int(ne.sum())} of {a.size} words differ"


def _hordiff_counts():
    """Three iterations of the neutral branch of tracer_hordiff with RECALC_NEUTRAL_SURF, for the two arms only it has."""
    from tests import hordiff_ref
    GV = abi.vgrid_default()
    d, M = H.benchmark_small(nk=3)[1:]
    P, opt = R.case("slope")
    inp = R.case_inputs(d, M, GV, opt)
    Pthd = abi.tracer_hor_diff_params_default(KHTR=1.0, check_diffusive_CFL=1)
    khx, khy = hordiff_ref.khdt_faces(d, M, Pthd, R.DT, {})
    Pthd.KhTr = 2.5 / float(hordiff_ref.cell_cfl(d, M, khx, khy).max())
    counts = R.new_counts()
    tr = [inp["T"].copy(), inp["S"].copy()]
    rec = {}
    n = R.tracer_hordiff_neutral(d, M, GV, Pthd, abi.neutral_diffusion_params_default(recalc_neutral_surf=1), R.case_eos(opt), inp["h"],
                                 R.DT, tr, tr[0], tr[1], counts=counts, record=rec)
    assert n == 3 and rec["passes"] == 3 and rec["calc_coeffs"] == 3
    return counts


def total_counts():
    tot = R.new_counts()
    for grid, nk in R.CONFIGS:
        for name in R.CASES:
            for k, v in R.want(grid, nk, name)[7].items():
                tot[k] += v
    for k, v in _hordiff_counts().items():
        tot[k] += v
    return tot


def test_exports_struct_and_defaults_agree_with_the_header():
    lib = abi.load_library()
    for name in ("mom6x_neutral_diffusion_init", "mom6x_neutral_diffusion_work_bytes", "mom6x_neutral_diffusion_calc_coeffs",
                 "mom6x_neutral_diffusion", "mom6x_neutral_diffusion_coeffs", "mom6x_neutral_diffusion_status",
                 "mom6x_neutral_diffusion_tile", "mom6x_tracer_hordiff_neutral"):
        assert hasattr(lib, name), name
    assert lib.mom6x_struct_size(36) == C.sizeof(abi.NeutralDiffusionParams)
    assert lib.mom6x_struct_size(37) == -1 and lib.mom6x_abi_version() == 6
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mom6x.h")).read()
    body = re.search(r"typedef struct mom6x_neutral_diffusion_params \{(.*?)\} mom6x_neutral_diffusion_params;", hdr, re.S).group(1)
    members = re.findall(r"^\s*(int|double)\s+(\w+);", body, re.M)
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in members] == list(abi.NeutralDiffusionParams._fields_)
    assert [n for _, n in members][:8] == ["continuous_reconstruction", "ref_pres", "interior_only", "tapering", "KhTh_use_vert_struct",
                                          "use_unmasked_transport_bug", "ndiff_answer_date", "recalc_neutral_surf"]
    P = abi.neutral_diffusion_params_default()
    assert (P.continuous_reconstruction, P.ref_pres, P.ndiff_answer_date, P.recalc_neutral_surf) == (1, -1.0, 20240101, 0)
    assert (P.RL2_T2_to_Pa, P.C_to_degC, P.S_to_ppt, P.kg_m3_to_R) == (1.0, 1.0, 1.0, 1.0)
    assert abi.NEUTRAL_DIFFUSION_MUST_BE_0 == ("interior_only", "tapering", "KhTh_use_vert_struct", "use_unmasked_transport_bug")
    assert all(getattr(P, n) == 0 for n in abi.NEUTRAL_DIFFUSION_MUST_BE_0)
    bx, by, i0 = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.mom6x_neutral_diffusion_tile(C.byref(bx), C.byref(by), C.byref(i0)) == 0
    assert (bx.value, by.value, i0.value) == abi.lane_launch_shape(lib)


def test_refusals_decided_on_the_host():
    GV = abi.vgrid_default()
    dflt = abi.neutral_diffusion_params_default
    eos = abi.eos_params_default()
    assert R.refused(dflt(), GV, eos) is None and R.refused(dflt(ref_pres=2.0e7, ndiff_answer_date=20240401, recalc_neutral_surf=1), GV, eos) is None
    assert R.refused(dflt(continuous_reconstruction=0), GV, eos) == "NDIFF_CONTINUOUS"
    for member, word in (("interior_only", "NDIFF_INTERIOR_ONLY"), ("tapering", "NDIFF_TAPERING"), ("KhTh_use_vert_struct", "KHTR_USE_EBT_STRUCT"),
                         ("use_unmasked_transport_bug", "NDIFF_USE_UNMASKED_TRANSPORT_BUG")):
        assert R.refused(dflt(**{member: 1}), GV, eos) == word
    GVn = abi.vgrid_default(); GVn.Boussinesq = 0
    assert R.refused(dflt(), GVn, eos) == "non-Boussinesq"
    assert R.refused(dflt(), GV, None) == "equation of state"
    lib = abi.load_library()
    P = dflt()
    assert lib.mom6x_neutral_diffusion_init(None, C.byref(P), C.byref(eos)) == 1                         # MOM6X_EINVAL
    assert b"null argument" in lib.mom6x_last_error()
    assert lib.mom6x_neutral_diffusion_calc_coeffs(None, None, None, None, None) == 1
    assert b"neutral_diffusion_init must be called first" in lib.mom6x_last_error()
    assert lib.mom6x_neutral_diffusion(None, None, None, None, C.c_double(1.0), None, None, 0, None, None, None) == 1
    assert lib.mom6x_neutral_diffusion_work_bytes(None) == 0


# powers of (Z, L, T, H, R, C, S)
_PRES = (0, 2, -2, 0, 1, 0, 0)
_DIM_GV = dict(g_Earth=(-1, 2, -2, 0, 0, 0, 0), Rho0=(0, 0, 0, 0, 1, 0, 0), Angstrom_H=(0, 0, 0, 1, 0, 0, 0), H_subroundoff=(0, 0, 0, 1, 0, 0, 0),
               dZ_subroundoff=(1, 0, 0, 0, 0, 0, 0), H_to_Z=(1, 0, 0, -1, 0, 0, 0), Z_to_H=(-1, 0, 0, 1, 0, 0, 0), H_to_RZ=(1, 0, 0, -1, 1, 0, 0),
               RZ_to_H=(-1, 0, 0, 1, -1, 0, 0))
_DIM_P = dict(ref_pres=_PRES, RL2_T2_to_Pa=(0, -2, 2, 0, -1, 0, 0), kg_m3_to_R=(0, 0, 0, 0, 1, 0, 0), C_to_degC=(0, 0, 0, 0, 0, -1, 0),
              S_to_ppt=(0, 0, 0, 0, 0, 0, -1))
_DIM_IN = dict(h=(0, 0, 0, 1, 0, 0, 0), T=(0, 0, 0, 0, 0, 1, 0), S=(0, 0, 0, 0, 0, 0, 1), p_surf=_PRES)
_DIM_OUT = dict(hEff=(0, 0, 0, 1, 0, 0, 0), tendency=(0, 0, -1, 1, 0, 0, 0), trans_x_2d=(0, 2, -1, 1, 0, 0, 0), trans_y_2d=(0, 2, -1, 1, 0, 0, 0))
RESCALE_SETS = [tuple(2.0 ** 11 if n == m else 1.0 for n in range(7)) for m in range(7)] + \
               [(2.0 ** 11, 2.0 ** 5, 2.0 ** -7, 2.0 ** 9, 2.0 ** 3, 2.0 ** -4, 2.0 ** 6)]


def rescaled(sc, d, M, GV, P, inp):
    """A case with Z, L, T, H, R, C and S rescaled by the factors `sc`: (metrics, vertical grid, parameters, inputs, Coef_x and
    Coef_y, dt, f), f giving the factor of a unit from its seven powers (tests/test_ref_parity_cpu.py rescales the compiled
    reference the same way)."""
    f = lambda pw: float(np.prod([s ** p for s, p in zip(sc, pw)]))                    # noqa: E731
    L, T_ = sc[1], sc[2]
    GV2 = abi.vgrid_default()
    for n, pw in _DIM_GV.items():
        setattr(GV2, n, getattr(GV, n) * f(pw))
    P2 = abi.NeutralDiffusionParams.from_buffer_copy(P)
    for n, pw in _DIM_P.items():
        setattr(P2, n, getattr(P, n) * f(pw))
    M2 = M.copy()
    for n in abi.METRICS:
        if n.startswith(("dx", "dy")): M2[G[n]] = M[G[n]] * L
        elif n.startswith(("Idx", "Idy")): M2[G[n]] = M[G[n]] / L
        elif n.startswith("area"): M2[G[n]] = M[G[n]] * L * L
        elif n.startswith("Iarea"): M2[G[n]] = M[G[n]] / (L * L)
    inp2 = {n: (a * f(_DIM_IN[n]) if n in _DIM_IN else a) for n, a in inp.items()}
    coef = tuple(a * (L * L) for a in R.coef_planes(d, M))
    return M2, GV2, P2, inp2, coef, R.DT * T_, f


@pytest.mark.parametrize("name", ("slope", "refp", "psurf", "massless"))
def test_dimensional_rescaling(name):
    """The reference's test.dim: Z, L, T, H, R, C and S rescaled by 2**11, one at a time and all at once with unequal powers.
    The vertical grid, the metrics, the parameters (the reference pressure and the unit factors of the equation of state with them)
    and the inputs are scaled in, the outputs are unscaled, and every bit of Po, Ko, hEff, the tracers and the diagnostics is the
    unscaled run's.  A unit factor in the wrong place (pa_to_H :382, the pressure handed to the equation of state, Idt) breaks it."""
    d, M, GV, P, opt, inp, want, _ = R.want("island_basin", 4, name)
    for sc in RESCALE_SETS:
        M2, GV2, P2, inp2, coef, dt2, f = rescaled(sc, d, M, GV, P, inp)
        got, _ = R.run(d, M2, GV2, P2, opt, inp2, dt=dt2, coef=coef)
        for n in R.COEFFS:
            a = got[n] / f(_DIM_OUT["hEff"]) if n.endswith("hEff") else got[n]
            _bits(a, want[n], f"{name}: {n} rescaled by Z, L, T, H, R, C, S = {sc}")
        for n in ("tracers", "tendency", "trans_x_2d", "trans_y_2d"):
            for m, (a, b) in enumerate(zip(got[n], want[n])):
                _bits(a / f(_DIM_OUT.get(n, (0,) * 7)), b, f"{name}: {n}[{m}] rescaled by {sc}")


class Transpose:
    """(i, j) -> (j, i) of a tile: whole pitched arrays, halos included; a u face becomes the v face of the same indices."""

    def __init__(self, d):
        self.d = d
        self.dr = abi.dims_init(d.nj, d.ni, d.nk, d.halo)
        w = d.halo
        self.i = np.arange(-w - 1, d.ni + w); self.j = np.arange(-w - 1, d.nj + w)

    def __call__(self, a):
        d, dr = self.d, self.dr
        out = np.zeros(a.shape[:-2] + dr.shape2(), dtype=a.dtype)
        out[..., (self.i + dr.joff)[:, None], (self.j + dr.ioff)[None, :]] = np.swapaxes(
            a[..., (self.j + d.joff)[:, None], (self.i + d.ioff)[None, :]], -1, -2)
        return np.ascontiguousarray(out)

    def metrics(self, M):
        Mr = np.zeros((abi.G_COUNT,) + self.dr.shape2())
        for n in abi.METRICS:
            Mr[G[SWAP.get(n, n)]] = self(M[G[n]])
        return np.ascontiguousarray(Mr)


@pytest.mark.parametrize("kind", ("slope", "ties", "massless"))
def test_the_transposed_grid_gives_the_transposed_bits(kind):
    """With ndiff_answer_date = 20240401 the update is (N + S) + (E + W), which a transposition of the index space turns into
    (E + W) + (N + S): every bit of the coefficients (u and v trade places), the tracers and the diagnostics is the transposed
    one.  A restatement that mixes up an index, a staggering, left and right or the order of a sum fails it.  The earlier order,
    which adds E, W, N, S surface by surface, is not symmetric, and the test shows that it would have noticed."""
    GV = abi.vgrid_default()
    d, M = H.island_basin(nk=4)[1:]
    opt = dict(R.case("slope")[1], kind=kind)
    inp = R.case_inputs(d, M, GV, opt)
    T = Transpose(d)
    Mr = T.metrics(M)
    inpr = {n: ([T(x) for x in a] if isinstance(a, list) else T(a)) for n, a in inp.items()}
    slu, slv, slh = H.interior(T.dr, "u"), H.interior(T.dr, "v"), H.interior(T.dr, "h")
    k = (slice(None),)
    differs = {}
    for date in (20240401, 20240101):
        P = abi.neutral_diffusion_params_default(ndiff_answer_date=date)
        one, _ = R.run(d, M, GV, P, opt, inp)
        two, _ = R.run(T.dr, Mr, GV, P, opt, inpr)
        for c in ("PoL", "PoR", "KoL", "KoR", "hEff"):
            _bits(two["u" + c][k + slu], T(one["v" + c])[k + slu], f"{kind}: u{c}' is v{c} transposed")
            _bits(two["v" + c][k + slv], T(one["u" + c])[k + slv], f"{kind}: v{c}' is u{c} transposed")
        same = True
        for m in range(3):
            pairs = [(two["tracers"][m][k + slh], T(one["tracers"][m])[k + slh], "tracer"),
                     (two["tendency"][m][k + slh], T(one["tendency"][m])[k + slh], "tendency"),
                     (two["trans_x_2d"][m][slu], T(one["trans_y_2d"][m])[slu], "trans_x_2d'"),
                     (two["trans_y_2d"][m][slv], T(one["trans_x_2d"][m])[slv], "trans_y_2d'")]
            for a, b, n in pairs:
                if date > 20240330:
                    _bits(a, b, f"{kind}: {n} {m} transposed")
                else:
                    same = same and np.array_equal(a, b)
        differs[date] = not same
    assert differs[20240101] or kind != "slope", "the surface-by-surface order came out symmetric: the test would not see an order"


def test_a_uniform_tracer_keeps_every_bit():
    for grid, nk in R.CONFIGS:
        for name in R.CASES:
            d, M, GV, P, opt, inp, out, _ = R.want(grid, nk, name)
            _bits(out["tracers"][2], inp["tracers"][2], f"{grid}/{nk}/{name}: the uniform tracer")
            own = H.interior(d, "h")
            assert not out["tendency"][2][(slice(None),) + own].any(), (grid, nk, name)
            if nk > 1:
                assert not np.array_equal(out["tracers"][0], inp["tracers"][0]), (grid, nk, name)


@pytest.mark.parametrize("name", ("slope", "massless", "new_order", "ties"))
def test_the_tracer_content_is_kept(name):
    """The sum over the cells of t * (h + H_subroundoff) * areaT changes by no more than the rounding of its own summation:
    (number of terms) x eps x the sum of the terms' magnitudes.  The cases have no underflow."""
    for grid, nk in R.CONFIGS:
        d, M, GV, P, opt, inp, out, _ = R.want(grid, nk, name)
        assert opt["uf"] is None
        own = (slice(None),) + H.interior(d, "h")
        w = ((inp["h"] + GV.H_subroundoff) * M[G["areaT"]])[own] * (M[G["mask2dT"]][own[1:]] > 0.0)
        for m in (0, 1):
            before = inp["tracers"][m][own] * w
            after = out["tracers"][m][own] * w
            bound = before.size * EPS * float(np.abs(before).sum())
            change = abs(float(after.sum()) - float(before.sum()))
            print(f"{grid}/{nk}/{name} tracer {m}: content changes by {change:.3e}, bound {bound:.3e}")
            assert change <= bound, (grid, nk, name, m, change, bound)


def test_invariants_of_the_positions():
    """Ko + Po does not decrease down the surfaces in either column; 0 <= Po <= 1; 1 <= Ko <= nk; hEff >= 0; dry faces hold 0 and
    1; on `flat` every Po is exactly 0 or 1; and the boundary-layer clamp :1541-1554 never changes a value."""
    for grid, nk in R.CONFIGS:
        for name in R.CASES:
            d, M, GV, P, opt, inp, out, counts = R.want(grid, nk, name)
            assert counts["bl_clamp_K"] == 0 and counts["bl_clamp_P"] == 0
            for p in "uv":
                sl = (slice(None),) + H.interior(d, p)
                wet = M[G["mask2dC" + p]][sl[1:]] > 0.0
                for side in "LR":
                    Po, Ko = out[p + "Po" + side][sl], out[p + "Ko" + side][sl].astype(np.int64)
                    assert (Po >= 0.0).all() and (Po <= 1.0).all() and (Ko >= 1).all() and (Ko <= nk).all(), (grid, nk, name, p, side)
                    pos = Ko + Po
                    assert (pos[1:] >= pos[:-1]).all() and (Ko[1:] >= Ko[:-1]).all(), (grid, nk, name, p, side)
                    assert (Po[:, ~wet] == 0.0).all() and (Ko[:, ~wet] == 1).all()
                    if name == "flat":
                        assert ((Po == 0.0) | (Po == 1.0)).all(), (grid, nk, p, side)
                hEff = out[p + "hEff"][sl]
                assert (hEff >= 0.0).all() and (hEff[:, ~wet] == 0.0).all() and np.isfinite(hEff).all()
                if nk > 1:
                    assert (hEff[:, wet] > 0.0).any()


def test_the_case_list_reaches_every_required_arm():
    tot = total_counts()
    print("arm counts:", tot)
    for k in REQUIRED:
        assert tot[k] > 0, (k, tot)
    for k in NOT_REACHED:
        assert tot[k] == 0, (k, "is reached after all: move it to REQUIRED")


def test_the_slope_case_slopes_and_diffuses():
    """Conditions on the inputs, on every grid of the GPU tests with more than one layer (one layer has Tint(1) = Tint(2): it is
    unstratified, and every position is 0 or 1) and at 75 layers: at least a quarter of the wet faces have a surface with
    0 < Po < 1, and at least a tenth of the sublayers with hEff > 0 carry a flux of the smooth tracer."""
    for grid, nk, kw in [(g, n, {}) for g, n in R.CONFIGS if n > 1] + [("benchmark_small", 75, dict(ni=20, nj=12))]:
        d, M, GV, P, opt, inp, out, _ = R.want(grid, nk, "slope", **kw)
        nwet = nfrac = nsub = nflux = 0
        for dir, p in ((0, "u"), (1, "v")):
            sl = (slice(None),) + H.interior(d, p)
            wet = M[G["mask2dC" + p]][sl[1:]] > 0.0
            frac = np.zeros(wet.shape, bool)
            for side in "LR":
                Po = out[p + "Po" + side][sl]
                frac |= ((Po > 0.0) & (Po < 1.0)).any(axis=0)
            nwet += int(wet.sum()); nfrac += int((frac & wet).sum())
            thick = out[p + "hEff"][sl] > 0.0
            nsub += int(thick.sum()); nflux += int((thick & (out["Flx"][0][dir][sl] != 0.0)).sum())
        print(f"{grid}/{nk}: {nfrac / nwet:.2f} of the wet faces have a fractional position, {nflux / nsub:.2f} of the sublayers a flux")
        assert nfrac >= 0.25 * nwet and nflux >= 0.1 * nsub, (grid, nk, nfrac, nwet, nflux, nsub)


def test_a_tile_s_cut_gives_its_part():
    """Each tile of a layout, called on its cut of the inputs (one halo point included) with the whole grid's parameters, gives
    its part of the one-tile answer."""
    GV = abi.vgrid_default()
    d, M, _, P, opt, _, one, _ = R.want("benchmark_small", 3, "slope")
    whole = R.case_inputs(d, M, GV, opt)
    for layout in ((2, 1), (1, 2)):
        for px in range(layout[0]):
            for py in range(layout[1]):
                dt_, Mt = H.benchmark_small(nk=3, layout=layout, pe=(px, py))[1:]
                inp = R.nan_halo(dt_, {n: ([R.cut(d, dt_, x) for x in a] if isinstance(a, list) else R.cut(d, dt_, a)) for n, a in whole.items()})
                tile, _ = R.run(dt_, Mt, GV, P, opt, inp)
                own = H.interior(dt_, "h")
                part = d.sl(dt_.i_glob0, dt_.i_glob0 + dt_.ni - 1, dt_.j_glob0, dt_.j_glob0 + dt_.nj - 1)
                for m in range(3):
                    _bits(tile["tracers"][m][:, own[0], own[1]], one["tracers"][m][:, part[0], part[1]], f"{layout} tile {(px, py)}: tracer {m}")
