"""The grids of tests/test_dyn_edges_gpu.py and the reasons for them, checked without a GPU.

The kernels of the dynamics go wrong at the edges of their tiles and launches, and only open water shows it:

  tiles     k_corad_lds and k_corad_fused advance by mom6x_tile_steps(0) = (30, 14) points over the ni + 1 by nj + 1 points
            (-1..ni-1, -1..nj-1), k_hv_fused by mom6x_tile_steps(1) = (28, 20) over the same points; both pad gx * gy * gz tiles
            to a multiple of 8, renumber them across the XCDs and let the work-groups at or past the count return.  A tile count
            that is one short, or an `out` predicate that stops one point early, changes nothing on a grid whose ni + 1 and
            nj + 1 are neither a whole number of steps nor one more -- and none of the module tests' grids is.
            advect_tracer's x passes own mom6x_tile_steps(2) = 240 cells per tile, its y passes 128 rows per segment.
  lanes     every other kernel of the split RK2 step, of PressureForce, vertvisc and of hor_visc's four-kernel chain gives a point
            of a plane a lane in work-groups of 64 x 4 (mom6x_lane_launch_shape): LAUNCHES below is the table of their extents.
  water     on a closed basin the last open face lies inside the tile and the corner cells of the halo are land: a launch that is
            one lane short, or a kernel that fetches a wrong corner word, multiplies what it got wrong by a zero mask.  Every
            shape here is a doubly re-entrant grid without land (H.torus).

What reads the corner cells (isc-1 | iec+1, jsc-1 | jec+1) of u, v and h (test_the_corner_cells_of_the_halo): CAu, CAv, diffu and
diffv at the tile's own faces on the torus, and on none of double_gyre, benchmark_small, channel and island_basin.  PFu and PFv
(layered, and under WRIGHT with the PLM reconstruction) keep every bit on the torus too: a pressure force reads the cells on either
side of its face and no corner.  Two RK2 steps from a state whose corner cells are scaled (test_the_corner_cells_and_the_RK2_state)
differ from the unscaled run in every bit-compared field, u, v, h, uh and vh, at the tile's own points on the torus -- the step takes
the halo of its inputs as given and the new-run initialisation and the predictor read it through CorAdCalc and
horizontal_viscosity -- and in none of them on double_gyre."""
import numpy as np
import pytest

from mom6_amd import abi
from tests import cases
from tests import helpers as H
from tests.test_dyn_gpu import CORAD_MODS, CorAdCalc_inputs, PressureForce_eos_inputs, visc_inputs
from tests.test_horvisc_gpu import FLAGS, horizontal_viscosity_inputs, hv_params
from tests.test_lateral_edges_cpu import CORNER_FACTOR, EDGE_SHAPES, SHAPE
from tests.test_tracer_gpu import ADVECT_CASES, advect_tracer_inputs

G = abi.G
HALO = 4
STEPS_CORAD, STEPS_HOR_VISC, STEPS_TRACER = (abi.tile_steps(w) for w in (abi.TILE_CORAD, abi.TILE_HOR_VISC, abi.TILE_TRACER_ADVECT))


def torus(ni, nj, nk=4):
    return H.torus(nk=nk, ni=ni, nj=nj, halo=HALO)


# ---- tiles ----------------------------------------------------------------------------------------------------------------------
def tile_shapes(sx, sy):
    """ni + 1 and nj + 1 a whole number of steps and one more, over one and over two tiles; the last two cross the smallest extent
    along one axis with the largest along the other."""
    return [(sx - 1, sy - 1), (sx, sy), (2 * sx - 1, 2 * sy - 1), (2 * sx, 2 * sy), (sx - 1, 2 * sy), (2 * sx, sy - 1)]


def tile_counts(ni, nj, sx, sy):
    """gx, gy of coriolis_adv.hip CorAdCalc_bc and hor_visc.hip mom6x_horizontal_viscosity."""
    return (ni + 1 + sx - 1) // sx, (nj + 1 + sy - 1) // sy


CORAD_TILE_SHAPES = tile_shapes(*STEPS_CORAD)
HV_TILE_SHAPES = tile_shapes(*STEPS_HOR_VISC)
CORAD_TWO_CHUNKS = STEPS_CORAD + (50,)      # kc = 25 (nk % 25 == 0): two chunks of layers, gz = 2
HV_TWO_CHUNKS = STEPS_HOR_VISC + (100,)     # beyond 80 layers kc = 25: four chunks


def test_todays_steps_and_tile_shapes():
    lib = abi.load_library()
    assert hasattr(lib, "mom6x_tile_steps") and lib.mom6x_tile_steps(0, None, None) == 0
    assert lib.mom6x_tile_steps(3, None, None) != 0 and lib.mom6x_tile_steps(-1, None, None) != 0
    assert (STEPS_CORAD, STEPS_HOR_VISC, STEPS_TRACER) == ((30, 14), (28, 20), (240, 128))
    assert CORAD_TILE_SHAPES[:4] == [(29, 13), (30, 14), (59, 27), (60, 28)] and CORAD_TILE_SHAPES[4:] == [(29, 28), (60, 13)]
    assert HV_TILE_SHAPES[:4] == [(27, 19), (28, 20), (55, 39), (56, 40)] and HV_TILE_SHAPES[4:] == [(27, 40), (56, 19)]


@pytest.mark.parametrize("shapes,steps", [(CORAD_TILE_SHAPES, STEPS_CORAD), (HV_TILE_SHAPES, STEPS_HOR_VISC)], ids=["CorAdCalc", "hor_visc"])
def test_tile_shapes_sit_on_the_tiles_edges(shapes, steps):
    """The points a tiled kernel covers, ni + 1 along i and nj + 1 along j, are a whole number of steps and one more, for one step
    and for two; the set has fewer than 8 tiles (the padded work-groups leave), a count that is no multiple of 8, and more
    than 8."""
    sx, sy = steps
    for n, s, ext in ((0, sx, [ni + 1 for ni, _ in shapes]), (1, sy, [nj + 1 for _, nj in shapes])):
        assert sorted(set(ext)) == [s, s + 1, 2 * s, 2 * s + 1], (n, ext)
    for ni, nj in shapes:
        gx, gy = tile_counts(ni, nj, sx, sy)
        assert gx == (1 if ni + 1 <= sx else 2 if ni + 1 <= 2 * sx else 3) and gy == (1 if nj + 1 <= sy else 2 if nj + 1 <= 2 * sy else 3)
    counts = [gx * gy for gx, gy in (tile_counts(ni, nj, sx, sy) for ni, nj in shapes)]
    assert counts == [1, 4, 4, 9, 3, 3]
    assert any(c < 8 for c in counts) and any(c % 8 for c in counts) and any(c > 8 for c in counts)
    # the grids of the module tests: neither a whole number of steps nor one more, for the kernel that ran on them
    older = [(44, 40), (32, 24), (40, 24)] if steps == STEPS_CORAD else [(36, 28), (40, 24), (32, 24)]
    for ni, nj in older:
        assert (ni + 1) % sx > 1 and (nj + 1) % sy > 1, (ni, nj)


# ---- lanes ----------------------------------------------------------------------------------------------------------------------
# The launches in 64 x 4 work-groups of an x-first split RK2 step with its callees (dyn_split_RK2.hip, barotropic.hip,
# pressure_force.hip, vert_friction.hip, continuity.hip) and of hor_visc.hip's four-kernel chain: (file, kernel, family, lanes
# along i beyond ni, rows beyond nj).  Family "nxa": grid3(nxa(ni + a, -b), ...): the first lane sits at i_first = -16 and the
# extent is ni + a - b - i_first; "plain": grid3(ni + a, ...), the first lane at the first point.  Not in the table, because their
# extents move from sub-step to sub-step with the wide halo of btstep (isv..iev, between ni and ni + 2 * halo + 1): k_btcl,
# k_find_Cor, k_bt_clip, k_face_areas_eta, k_bt_pred, k_bt_vel, k_bt_eta; the column kernels in work-groups of 64 x 1
# (k_vertvisc_cols, k_vertvisc_coef_cols: the extents along i of the table, no rounding along j); the mass-flux kernels, whose
# 16-face strips STRIPS below is about.  A y-first step (first_direction = 1) adds k_convergence<1> on nxa(ni + 6, -3).
LAUNCHES = [
    ("dyn_split_RK2.hip", "k_eta", "plain", 0, 0),
    ("dyn_split_RK2.hip", "k_h_av (whole halo)", "nxa", HALO, 2 * HALO),          # nxa(ni + 2 * halo, -halo)
    ("dyn_split_RK2.hip", "k_bc_accel", "nxa", 0, 1),                             # nxa(ni + 1, -1)
    ("dyn_split_RK2.hip", "k_vel_update", "nxa", 0, 1),
    ("dyn_split_RK2.hip", "k_h_av (two points)", "nxa", 2, 4),                    # nxa(ni + 4, -2)
    ("dyn_split_RK2.hip", "k_h_av (one point)", "nxa", 1, 2),                     # nxa(ni + 2, -1)
    ("dyn_split_RK2.hip", "k_uhtr", "nxa", 2, 5),                                 # nxa(ni + 5, -3)
    ("barotropic.hip", "k_btcalc<0>, k_bt_col<0>", "nxa", 0, 0),
    ("barotropic.hip", "k_btcalc<1>, k_bt_col<1>", "plain", 0, 1),
    ("barotropic.hip", "k_layer_accel", "nxa", 0, 1),
    ("barotropic.hip", "k_bt_init_static, k_btcont_copy, k_uhbt0, k_cor_ref_eta_src", "plain", 1, 1),
    ("barotropic.hip", "k_bt_mass_source, k_set_dtbt, k_bt_post", "plain", 0, 0),
    ("barotropic.hip", "k_face_areas_as_fits", "plain", 3, 3),
    ("barotropic.hip", "k_bt_copy_in", "plain", 2 * HALO + 1, 2 * HALO + 1),
    ("pressure_force.hip", "k_pgf_e, k_pgf_main, k_pgf_main_eos", "nxa", 1, 2),   # nxa(ni + 2, -1)
    ("vert_friction.hip", "k_vertvisc<0>, k_vertvisc_coef<0>, k_vertvisc_remnant<0>", "nxa", 0, 0),
    ("vert_friction.hip", "k_vertvisc<1>, k_vertvisc_coef<1>, k_vertvisc_remnant<1>", "plain", 0, 1),
    ("continuity.hip", "k_convergence<0> (rows js - 3 .. je + 3)", "plain", 0, 6),
    ("continuity.hip", "k_convergence<1>", "plain", 0, 0),
    ("hor_visc.hip", "k_hv_strain", "nxa", 2, 4),                                 # nxa(ni + 4, -2)
    ("hor_visc.hip", "k_hv_del2, k_hv_leith", "nxa", 1, 3),                       # nxa(ni + 3, -2)
    ("hor_visc.hip", "k_hv_vort", "nxa", 2, 5),                                   # nxa(ni + 5, -3)
    ("hor_visc.hip", "k_hv_stress", "nxa", 1, 2),                                 # nxa(ni + 2, -1)
    ("hor_visc.hip", "k_hv_accel", "nxa", 0, 1),                                  # nxa(ni + 1, -1)
]


def lane_extent(ni, family, extra, i_first):
    return ni + extra - (i_first if family == "nxa" else 0)


def lane_shapes(bx, by, i_first):
    """EDGE_SHAPES of tests/test_lateral_edges_cpu.py (the "nxa" extents ni + {0, 1, 2} - i_first) and, for every extent of the
    table that they leave without a remainder of 0 or of 1 modulo bx, the ni that puts it on one work-group and on one lane more;
    nj = by + 1 .. 2 * by in turn: four consecutive nj give every remainder modulo by whatever a launch adds to the rows."""
    extents = sorted({(f, x) for _, _, f, x, _ in LAUNCHES})
    have = [ni for ni, _ in EDGE_SHAPES]
    more = set()
    for family, extra in extents:
        for r in (0, 1):
            if not any(lane_extent(ni, family, extra, i_first) % bx == r for ni in have + sorted(more)):
                more.add(bx + r - extra + (i_first if family == "nxa" else 0))
    return list(EDGE_SHAPES) + [(ni, by + 1 + t % by) for t, ni in enumerate(sorted(more))]


LANE_SHAPES = lane_shapes(*SHAPE)
NF = 16    # the faces along i of a strip of the mass-flux kernels (continuity_wave.hip MOM6X_MFW_NF, continuity_lds.hip NF)


def zonal_strip_faces(ni, ioff):
    """The faces a zonal mass-flux launch spreads over its strips: a0 = is - 1 .. a1 = ie (continuity.hip run_direction<0>) from
    the strip base pib = a0 rounded down to a cache line of the pitched rows (continuity_wave.hip:1074, continuity_lds.hip:792);
    gx = (a1 - pib + NF) / NF strips (continuity_wave.hip:1013, continuity_lds.hip:723)."""
    a0, a1 = -1, ni - 1
    pib = a0 - (a0 + ioff) % NF
    return a1 - pib + 1


def test_todays_lane_shapes_and_their_coverage():
    bx, by, i_first = SHAPE
    assert LANE_SHAPES == EDGE_SHAPES + [(44, 5), (45, 6), (55, 7), (56, 8), (61, 5), (62, 6), (63, 7), (64, 8), (65, 5)]
    assert {x for _, _, f, x, _ in LAUNCHES if f == "nxa"} == {0, 1, 2, HALO}
    assert {x for _, _, f, x, _ in LAUNCHES if f == "plain"} == {0, 1, 3, 2 * HALO + 1}
    assert all(55 <= ni <= 65 for ni, _ in LANE_SHAPES[len(EDGE_SHAPES) + 2:])        # the additions for the plain family
    for _, kernel, family, x, y in LAUNCHES:
        ext = [lane_extent(ni, family, x, i_first) for ni, _ in LANE_SHAPES]
        rows = [nj + y for _, nj in LANE_SHAPES]
        for r in (0, 1):
            assert any(e % bx == r for e in ext), (kernel, "lanes", r)
            assert any(e % by == r for e in rows), (kernel, "rows", r)
    # none of the additions is redundant: each is the only shape with a remainder of 0 or 1 for some extent
    for ni, _ in LANE_SHAPES[len(EDGE_SHAPES):]:
        others = [n for n, _ in LANE_SHAPES if n != ni]
        assert any(lane_extent(ni, f, x, i_first) % bx in (0, 1) and
                   not any(lane_extent(n, f, x, i_first) % bx == lane_extent(ni, f, x, i_first) % bx for n in others)
                   for _, _, f, x, _ in LAUNCHES), ni


def test_the_mass_flux_strips():
    """The zonal face range (ni + 16 faces from the strip base) is a whole number of 16-face strips at ni = 48, 64 and 112 and one
    face more at ni = 49, 65 and 113: LANE_SHAPES has them, no grid needs adding."""
    whole, one_more = [], []
    for ni, nj in LANE_SHAPES:
        d = torus(ni, nj)[1]
        assert d.ioff % NF == 0
        n = zonal_strip_faces(ni, d.ioff)
        assert n == ni + 16
        (whole if n % NF == 0 else one_more if n % NF == 1 else []).append(ni)
    assert whole == [48, 112, 64] and one_more == [49, 113, 65]


# ---- advect_tracer's tiles and segments -------------------------------------------------------------------------------------------
def advect_stencil(schemes):
    """tracer_advect.hip advect_stencil (USE_HUYNH_STENCIL_BUG = False): 3 with a PPM or PPM:H3 tracer, else 2."""
    return 3 if any(s in (1, 2) for s in schemes) else 2


def first_pass_extent(n, stencil):
    """The cells along the direction of the first pass of an iteration: after a halo update the work range is widened by
    (halo / stencil) stencils and the pass gives one back (mom6x_advect_tracer: isv..iev of advect_tiled)."""
    return n + 2 * (HALO // stencil - 1) * stencil


def x_tiles(ext):
    return (ext - 1 + STEPS_TRACER[0]) // STEPS_TRACER[0]       # ntile = (i1 - i0 + TX) / TX


def y_segments(ext):
    return (ext - 1 + STEPS_TRACER[1]) // STEPS_TRACER[1]       # nseg = (j1 - j0 + SEGY) / SEGY


# the scheme sets of test_advect_tracer with a three-point stencil (every pass then covers the tile's own cells: ni along i, nj along j)
ADVECT_X_CASES = [c for c in ADVECT_CASES if c[1] == 0 and advect_stencil(c[0]) == 3]
ADVECT_Y_CASES = [c for c in ADVECT_CASES if c[1] == 1 and advect_stencil(c[0]) == 3]
TRACER_X_SHAPES = [(STEPS_TRACER[0], 9), (STEPS_TRACER[0] + 1, 9)]
TRACER_Y_SHAPES = [(9, STEPS_TRACER[1]), (9, STEPS_TRACER[1] + 1)]


def test_tracer_tiles_and_segments():
    assert len(ADVECT_X_CASES) == 2 and len(ADVECT_Y_CASES) == 2
    assert TRACER_X_SHAPES == [(240, 9), (241, 9)] and TRACER_Y_SHAPES == [(9, 128), (9, 129)]
    assert [x_tiles(first_pass_extent(ni, 3)) for ni, _ in TRACER_X_SHAPES] == [1, 2]
    assert [first_pass_extent(ni, 3) - STEPS_TRACER[0] for ni, _ in TRACER_X_SHAPES] == [0, 1]      # one tile and one more column
    assert [y_segments(first_pass_extent(nj, 3)) for _, nj in TRACER_Y_SHAPES] == [1, 2]
    assert [first_pass_extent(nj, 3) - STEPS_TRACER[1] for _, nj in TRACER_Y_SHAPES] == [0, 1]      # one segment and one more row
    # the grids test_advect_tracer has: 600 x 300 (three tiles, three segments), everything else within one; with a two-point
    # stencil the first pass of "wide" covers 604 and 304
    for n, s in ((600, 3), (300, 3), (604, 2), (304, 2), (44, 2), (40, 2), (96, 3)):
        assert first_pass_extent(n, s) % STEPS_TRACER[0] > 1 and first_pass_extent(n, s) % STEPS_TRACER[1] > 1


# ---- open water -----------------------------------------------------------------------------------------------------------------
ALL_SHAPES = sorted(set(LANE_SHAPES + CORAD_TILE_SHAPES + HV_TILE_SHAPES + TRACER_X_SHAPES + TRACER_Y_SHAPES + [(96, 40)]))


@pytest.mark.parametrize("ni,nj", ALL_SHAPES)
def test_the_last_faces_and_the_corner_cells_are_open_water(ni, nj):
    gg, d, M = torus(ni, nj, nk=2)
    assert (d.ni, d.nj, d.halo) == (ni, nj, HALO) and d.pitch >= d.ioff + ni + d.halo
    assert (M[G["mask2dCu"]][d.sl(ni - 1, ni - 1, 0, nj - 1)] == 1.0).all()      # the u faces of column I = iec
    assert (M[G["mask2dCv"]][d.sl(0, ni - 1, nj - 1, nj - 1)] == 1.0).all()      # the v faces of row J = jec
    for i in (-1, ni):
        for j in (-1, nj):
            assert M[G["mask2dT"]][d.joff + j, d.ioff + i] == 1.0


# ---- the cases of the GPU file ----------------------------------------------------------------------------------------------------
CORAD_EDGE_MODS = [dict(),                                                                            # k_corad_lds
                   dict(bound_Coriolis=1, Coriolis_En_Dis=1, KE_Scheme=abi.KE_GUDONOV),               # k_corad_fused
                   dict(Coriolis_Scheme=abi.ARAKAWA_HSU90),
                   dict(Coriolis_Scheme=abi.ARAKAWA_LAMB81, rough=1),                                 # k_corad_q + k_corad_acc
                   dict(Coriolis_Scheme=abi.ROBUST_ENSTRO, rough=1)]
CORAD_LANE_MODS = CORAD_EDGE_MODS[3:]
HV_EDGE_FLAGS = ["om4_class", "smagorinsky", "smagorinsky_bound_coriolis", "leith_kh_ah_modified"]
HV_LANE_FLAGS = HV_EDGE_FLAGS[3:]
PGF_EOS_CASES = [("WRIGHT", dict()), ("WRIGHT", dict(Recon_Scheme=1, MassWghtInterp=3)), ("WRIGHT", dict(Recon_Scheme=2, MassWghtInterp=3)),
                 ("UNESCO", dict(EOS_quadrature=1))]
RK2_SHAPES = LANE_SHAPES + CORAD_TILE_SHAPES + HV_TILE_SHAPES
RK2_EXTRA_SHAPES = [LANE_SHAPES[0], CORAD_TILE_SHAPES[3]]         # also without the remnant in the solve, and with an equation of state


def corad_kernel(mods, legacy=False):
    """The kernel CorAdCalc_bc launches for an option set (the first one of the two-kernel form)."""
    scheme = mods.get("Coriolis_Scheme", abi.SADOURNY75_ENERGY)
    if legacy or scheme in (abi.ARAKAWA_LAMB81, abi.AL_BLEND, abi.ROBUST_ENSTRO):
        return "k_corad_q"
    lean = scheme == abi.SADOURNY75_ENERGY and not mods.get("bound_Coriolis") and not mods.get("Coriolis_En_Dis")
    return "k_corad_lds" if lean else "k_corad_fused"


def hor_visc_kernel(flags, legacy=False):
    """The last kernel mom6x_horizontal_viscosity launches for an entry of FLAGS."""
    P = FLAGS[flags]
    return "k_hv_accel" if legacy or P.get("Leith_Kh") or P.get("Leith_Ah") else "k_hv_fused"


def rk2_hor_visc(cfg):
    """The OM4-class switches of horizontal_viscosity with the step's dt."""
    return hv_params(FLAGS["om4_class"], dt=cases.rk2_inputs(cfg, False, False)["dt"])


def oracle_rk2(orc, cfg, nsteps=2, rk2_mod=None, eos_form=None, recon=0):
    """The oracle's side of test_rk2_gpu.run(orc, cfg, nsteps, bt_mod=dict(strong_drag=1), dev_vv=dict(), hv=rk2_hor_visc(cfg), ...):
    (inputs, final state, OrcModel)."""
    gg, d, M = cfg
    inp = cases.rk2_inputs(cfg, False, False)
    tv = None
    if eos_form is not None:
        tv = cases.thermo_state(d, M) + (abi.eos_params_default(eos_form),)
        tv[2].Recon_Scheme = recon
    vv = (abi.vertvisc_params_default(),) + tuple(visc_inputs(d, M, with_shear=True)) + (inp["coefs"][0][4], inp["coefs"][0][5])
    so, m = cases.oracle_rk2(orc, cfg, inp, nsteps, dict(strong_drag=1), rk2_mod, None, 0, tv=tv, vv=vv, hv=rk2_hor_visc(cfg))
    return inp, so, m


def _last_column_is_felt(d, CAu):
    return np.abs(CAu[(slice(None),) + d.sl(d.ni - 1, d.ni - 1, 0, d.nj - 1)]).max() > 0.0


@pytest.mark.parametrize("ni,nj", sorted(set(CORAD_TILE_SHAPES + LANE_SHAPES)) + [(96, 40)])
def test_the_oracle_runs_the_CorAdCalc_cases(orc, ni, nj):
    mods = CORAD_MODS if (ni, nj) == (96, 40) else CORAD_EDGE_MODS if (ni, nj) in CORAD_TILE_SHAPES else CORAD_LANE_MODS
    shapes = [(ni, nj, 3 if (ni, nj) == (96, 40) else 4)] + ([CORAD_TWO_CHUNKS] if (ni, nj) == STEPS_CORAD else [])
    for a, b, nk in shapes:
        cfg = torus(a, b, nk)
        for m in mods:
            CAu, CAv = CorAdCalc_inputs(orc, cfg, m)[3:]
            assert np.isfinite(CAu).all() and np.isfinite(CAv).all() and _last_column_is_felt(cfg[1], CAu), (a, b, nk, m)
            if (ni, nj) == (96, 40):      # and with cell areas that differ from cell to cell: another answer
                CAu2 = CorAdCalc_inputs(orc, (cfg[0], cfg[1], H.uneven_cell_areas(cfg[1], cfg[2])), m)[3]
                assert np.isfinite(CAu2).all() and _differ(_own(cfg[1], CAu, "u"), _own(cfg[1], CAu2, "u")), m


@pytest.mark.parametrize("ni,nj", sorted(set(HV_TILE_SHAPES + LANE_SHAPES)) + [(96, 40)])
def test_the_oracle_runs_the_hor_visc_cases(orc, ni, nj):
    flags = sorted(FLAGS) if (ni, nj) == (96, 40) else HV_EDGE_FLAGS if (ni, nj) in HV_TILE_SHAPES else HV_LANE_FLAGS
    shapes = [(ni, nj, 4)] + ([HV_TWO_CHUNKS] if (ni, nj) == STEPS_HOR_VISC else [])
    for a, b, nk in shapes:
        cfg = torus(a, b, nk)
        for f in flags:
            du, dv = horizontal_viscosity_inputs(orc, cfg, f)[3:]
            assert np.isfinite(du).all() and np.isfinite(dv).all() and _last_column_is_felt(cfg[1], du), (a, b, nk, f)


@pytest.mark.parametrize("ni,nj", LANE_SHAPES)
def test_the_oracle_runs_the_PressureForce_cases(orc, ni, nj):
    cfg = torus(ni, nj); gg, d, M = cfg
    for form, mods in PGF_EOS_CASES:
        GV, CS, eos, Rlay, gp, h, T, S = PressureForce_eos_inputs(orc, cfg, form, mods)
        o = dict(PFu=np.zeros_like(h), PFv=np.zeros_like(h), pbce=np.zeros_like(h), eta=np.zeros(d.shape2()))
        orc.PressureForce(d, M, GV, CS, Rlay, gp, h, o["PFu"], o["PFv"], o["pbce"], o["eta"], T=T, S=S, eos=eos)
        assert all(np.isfinite(a).all() for a in o.values()) and _last_column_is_felt(d, o["PFu"]), (form, mods)
    o = dict(PFu=np.zeros_like(h), PFv=np.zeros_like(h))
    orc.PressureForce(d, M, GV, CS, Rlay, gp, h, o["PFu"], o["PFv"])
    assert all(np.isfinite(a).all() for a in o.values()) and _last_column_is_felt(d, o["PFu"])


@pytest.mark.parametrize("ni,nj", RK2_SHAPES)
def test_the_oracle_runs_the_RK2_cases(orc, sums, ni, nj):
    """Two steps stay finite, move, keep the volume, and CAu is felt at the u faces of column I = iec."""
    cfg = torus(ni, nj); gg, d, M = cfg
    runs = [dict()] + ([dict(rk2_mod=dict(visc_rem_dt_bug=0)), dict(eos_form=abi.WRIGHT, recon=1)] if (ni, nj) in RK2_EXTRA_SHAPES else [])
    for kw in runs:
        inp, so, m = oracle_rk2(orc, cfg, **kw)
        assert all(np.isfinite(so[k]).all() for k in so) and 1e-3 < np.abs(so["u"]).max() < 1.0, kw
        assert _last_column_is_felt(d, m["CAu"]) and _last_column_is_felt(d, m["diffu"]), kw
        sl = H.interior(d, "h"); A = M[G["areaT"]][sl]
        assert abs((so["h"][(Ellipsis,) + sl] * A).sum() / (inp["h"][(Ellipsis,) + sl] * A).sum() - 1.0) < 1e-13, kw


@pytest.mark.parametrize("ni,nj", [(96, 40)] + TRACER_X_SHAPES + TRACER_Y_SHAPES)
def test_the_oracle_runs_the_advect_tracer_cases(orc, ni, nj):
    cfg = torus(ni, nj, nk=2); gg, d, M = cfg
    todo = ADVECT_CASES if (ni, nj) == (96, 40) else ADVECT_X_CASES if (ni, nj) in TRACER_X_SHAPES else ADVECT_Y_CASES
    for schemes, first, post in todo:
        GV, dt_dyn, dt, h_end, uhtr, vhtr, trs = advect_tracer_inputs(orc, cfg, schemes, post)
        tro = [t.copy() for t in trs]
        it = orc.advect_tracer(d, M, GV, first, dt_dyn, 0, h_end, uhtr, vhtr, dt, tro, schemes)
        assert it >= 1 and all(np.isfinite(t).all() for t in tro)
        sl = (Ellipsis,) + H.interior(d, "h")
        assert all(np.abs(a - b)[sl].max() > 1e-6 for a, b in zip(tro, trs)), (schemes, first, post)
        if post > 1.0:
            assert it >= 3, (schemes, first, post, it)      # the limiter asks for more passes, as on test_advect_tracer's grids


# ---- the corner cells of the halo -------------------------------------------------------------------------------------------------
def scale_corners(d, a):
    """A copy with the words of the four corner cells of the halo's first ring multiplied by CORNER_FACTOR, in every layer."""
    a = a.copy()
    for i in (-1, d.ni):
        for j in (-1, d.nj):
            a[..., d.joff + j, d.ioff + i] *= CORNER_FACTOR
    return a


def _differ(a, b):
    return not np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _own(d, a, stagger):
    return a[(Ellipsis,) + H.interior(d, stagger)]


def corner_experiment(orc, cfg):
    """Which of CAu, CAv, diffu, diffv, PFu, PFv (layered, and under WRIGHT with PLM reconstruction) change at the tile's own faces
    when the corner cells of u, v and h are scaled: {name: bool}."""
    gg, d, M = cfg
    out = {}
    GV, CS, (u, v, h, uh, vh), CAu, CAv = CorAdCalc_inputs(orc, cfg, dict())
    CAu2, CAv2 = np.zeros_like(h), np.zeros_like(h)
    orc.CorAdCalc(d, M, GV, CS, scale_corners(d, u), scale_corners(d, v), scale_corners(d, h), uh, vh, CAu2, CAv2)
    out["CAu"] = _differ(_own(d, CAu, "u"), _own(d, CAu2, "u")); out["CAv"] = _differ(_own(d, CAv, "v"), _own(d, CAv2, "v"))
    GV, P, (u, v, h), du, dv = horizontal_viscosity_inputs(orc, cfg, "om4_class")
    du2, dv2 = np.zeros_like(u), np.zeros_like(v)
    orc.horizontal_viscosity(d, M, GV, P, orc.hor_visc_init(d, M, P), scale_corners(d, u), scale_corners(d, v), scale_corners(d, h), du2, dv2)
    out["diffu"] = _differ(_own(d, du, "u"), _own(d, du2, "u")); out["diffv"] = _differ(_own(d, dv, "v"), _own(d, dv2, "v"))
    GV, CS, eos, Rlay, gp, h, T, S = PressureForce_eos_inputs(orc, cfg, "WRIGHT", dict(Recon_Scheme=1))
    for tag, kw in (("", dict()), ("_eos", dict(T=T, S=S, eos=eos))):
        r = []
        for hh in (h, scale_corners(d, h)):
            o = dict(PFu=np.zeros_like(h), PFv=np.zeros_like(h), pbce=np.zeros_like(h), eta=np.zeros(d.shape2()))
            orc.PressureForce(d, M, GV, CS, Rlay, gp, hh, o["PFu"], o["PFv"], o["pbce"], o["eta"], **kw)
            r.append(o)
        out["PFu" + tag] = _differ(_own(d, r[0]["PFu"], "u"), _own(d, r[1]["PFu"], "u"))
        out["PFv" + tag] = _differ(_own(d, r[0]["PFv"], "v"), _own(d, r[1]["PFv"], "v"))
    return out


def test_the_corner_cells_of_the_halo(orc):
    """CAu, CAv, diffu and diffv read the corner cells at the tile's own faces on the torus and on none of the closed grids and the
    channel, where a zero mask multiplies what they read.  PFu and PFv never do (printed, and held here as found)."""
    got = corner_experiment(orc, H.torus(nk=4))
    print("torus:", got)
    assert all(got[n] for n in ("CAu", "CAv", "diffu", "diffv")), got
    assert not any(got[n] for n in ("PFu", "PFv", "PFu_eos", "PFv_eos")), got
    for grid in ("double_gyre", "benchmark_small", "channel", "island_basin"):
        got = corner_experiment(orc, getattr(H, grid)(nk=4))
        print(grid + ":", got)
        assert not any(got.values()), (grid, got)


def test_the_corner_cells_and_the_RK2_state(orc):
    """Two RK2 steps from a state whose corner cells of u, v and h are scaled: what changes in the state at the tile's own points
    (printed; held as found: everything on the torus, nothing on the closed basin)."""
    for grid in ("torus", "double_gyre"):
        cfg = getattr(H, grid)(nk=3); gg, d, M = cfg
        inp = cases.rk2_inputs(cfg, False, False)
        inp2 = dict(inp, u=scale_corners(d, inp["u"]), v=scale_corners(d, inp["v"]), h=scale_corners(d, inp["h"]))
        so = [cases.oracle_rk2(orc, cfg, x, 2, dict(strong_drag=1), hv=rk2_hor_visc(cfg))[0] for x in (inp, inp2)]
        got = {n: _differ(_own(d, so[0][n], st), _own(d, so[1][n], st)) for n, st in (("u", "u"), ("v", "v"), ("h", "h"), ("uh", "u"), ("vh", "v"))}
        print(grid + ":", got)
        assert got == RK2_CORNER_FINDING[grid], (grid, got)


RK2_CORNER_FINDING = {"torus": dict(u=True, v=True, h=True, uh=True, vh=True),
                      "double_gyre": dict(u=False, v=False, h=False, uh=False, vh=False)}
