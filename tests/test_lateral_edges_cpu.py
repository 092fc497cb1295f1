"""The grids of tests/test_lateral_edges_gpu.py and the reasons for them, checked without a GPU.

set_viscous_BBL, thickness_diffuse, calc_slope_functions and mixedlayer_restrat give each cell or face of a plane one lane, in
work-groups of bx x by lanes whose first lane sits at i = i_first (mom6x_lane_launch_shape: 64, 4, -16), and launch
ni + {0, 1, 2} - i_first lanes along i and nj + {1, 2, 3, 4} rows.  An extent that is one lane or one row short is invisible as
long as it rounds up to the same number of work-groups, and a last lane that only ever sees land hides what it reads.  EDGE_SHAPES
are doubly re-entrant grids without land (H.torus) whose extents are exact multiples of the work-group and one more, in x over one
and over two work-groups: open water up to the last lane and in every corner of the halo.

Which outputs read a corner of the halo (cells (isc-1 | iec+1, jsc-1 | jec+1) of h, T, S, u, v), from the restatements on
H.torus(nk=4), every case of the lists below:
  set_viscous_BBL      Kv_bbl_u | v, bbl_thick_u | v and, with body-force drag, Ray_u | v at the tile's own faces (set_v_at_u,
                       set_u_at_v: v(i+1, J-1) of a u face);
  calc_slope_functions SN_u, SN_v (and S2_u, S2_v) at the tile's own faces in all three branches (the four-face averages); the
                       slopes, N2 and dz planes on their widened ranges only;
  thickness_diffuse    nothing: h, uhtr, vhtr, uhGM and vhGM keep every bit;
  mixedlayer_restrat   nothing at the tile's own points; only the planes posted one point into the halo, at the corner cell
                       itself: Rml_av_fast, MLD_fast, MLD_slow and the two filtered planes.
On H.benchmark_small, as on every closed grid, the corners are land and no output at the tile's own points depends on them."""
import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import mle_ref, setvisc_ref, thickdiff_ref, varmix_ref
from tests.test_mixed_layer_restrat_cpu import STAG as MLE_STAG
from tests.test_varmix_cpu import STAG as VARMIX_STAG

G = abi.G
X_EXTRA = (0, 1, 2)        # the launches' extents along i are ni + X_EXTRA - i_first lanes ...
Y_EXTRA = (1, 2, 3, 4)     # ... and nj + Y_EXTRA rows


def edge_shapes(bx, by, i_first):
    """(ni, nj): ni = m*bx + i_first - 2 .. m*bx + i_first + 1 for m = 1, 2, nj = by + 1 .. 2*by, upwards for m = 1 and downwards
    for m = 2."""
    n = max(4, by)
    out = []
    for m in (1, 2):
        for t in range(n):
            out.append((m * bx + i_first - 2 + t % 4, by + 1 + t % by if m == 1 else 2 * by - t % by))
    return out


SHAPE = abi.lane_launch_shape()
EDGE_SHAPES = edge_shapes(*SHAPE)


def edge_grid(ni, nj, nk=4):
    return H.torus(nk=nk, ni=ni, nj=nj)[1:]


def test_the_accessor_and_todays_shapes():
    lib = abi.load_library()
    assert hasattr(lib, "mom6x_lane_launch_shape")
    assert lib.mom6x_lane_launch_shape(None, None, None) == 0
    assert SHAPE == (64, 4, -16)
    assert EDGE_SHAPES == [(46, 5), (47, 6), (48, 7), (49, 8), (110, 8), (111, 7), (112, 6), (113, 5)]


def test_every_extent_is_an_exact_multiple_and_one_more():
    """Along i, each of the three extents is a multiple of bx and a multiple plus one, both within two work-groups and beyond
    them; each of the four row counts is a multiple of by and a multiple plus one."""
    bx, by, i_first = SHAPE
    for x in X_EXTRA:
        ext = [ni + x - i_first for ni, _ in EDGE_SHAPES]
        for r in (0, 1):
            assert any(e % bx == r and e <= bx + 1 for e in ext), (x, r, ext)
            assert any(e % bx == r and e > bx + 1 for e in ext), (x, r, ext)
    for y in Y_EXTRA:
        rows = [nj + y for _, nj in EDGE_SHAPES]
        for r in (0, 1):
            assert any(e % by == r for e in rows), (y, r, rows)
        assert all(e > by for e in rows)


def test_none_of_the_older_grids_sits_on_an_edge():
    """What the module tests ran before: no extent along i a multiple of bx or one more, every row count off the multiples of by
    (nj + 4 is one whenever nj is, and then nj + 1 .. nj + 3 are not)."""
    bx, by, i_first = SHAPE
    for ni in (20, 36, 40, 360, 1440):
        assert all((ni + x - i_first) % bx > 1 for x in X_EXTRA), ni
    for nj in (12, 24, 28, 180, 1080):
        assert nj % by == 0


@pytest.mark.parametrize("ni,nj", EDGE_SHAPES)
def test_the_last_column_and_row_are_open_water(ni, nj):
    d, M = edge_grid(ni, nj)
    assert (d.ni, d.nj) == (ni, nj) and d.pitch >= d.ioff + ni + d.halo
    assert (M[G["mask2dCu"]][d.sl(ni - 1, ni - 1, 0, nj - 1)] == 1.0).all()      # the u faces of column I = iec
    assert (M[G["mask2dCv"]][d.sl(0, ni - 1, nj - 1, nj - 1)] == 1.0).all()      # the v faces of row J = jec
    for i in (-1, ni):
        for j in (-1, nj):
            assert M[G["mask2dT"]][d.joff + j, d.ioff + i] == 1.0
    b, Mb = H.benchmark_small(nk=4, ni=ni, nj=nj)[1:]
    assert not Mb[G["mask2dCu"]][b.sl(ni - 1, ni - 1, 0, nj - 1)].any()            # a bowl of the same size: all of them closed
    assert not Mb[G["mask2dCv"]][b.sl(0, ni - 1, nj - 1, nj - 1)].any()


@pytest.mark.parametrize("ni,nj", EDGE_SHAPES)
def test_the_restatements_run_on_every_shape(ni, nj, orc):
    """The cases of tests/test_lateral_edges_gpu.py: at the tile's own points every output is finite, or NaN throughout where the
    case's branch does not write it (S2_u | v outside the Visbeck branch); the module's results proper are finite."""
    main = dict(set_visc=("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v"), thickness_diffuse=("h", "uhtr", "vhtr"),
                varmix=("SN_u", "SN_v"), mle=("h", "uhtr", "vhtr"))
    d, M = edge_grid(ni, nj)
    GV = abi.vgrid_default()
    for module in MODULES:
        for name in EDGE_CASES[module]:
            want = restatement(module, name, d, M, GV, orc)[1]
            for n, a in want.items():
                st = STAGGER[module](n)
                sl = (Ellipsis,) + H.interior(d, st)
                if module == "varmix" and a.ndim == 3:
                    sl = (slice(1, d.nk),) + H.interior(d, st)
                assert np.isfinite(a[sl]).all() or (n not in main[module] and np.isnan(a[sl]).all()), (module, name, n)


# ---- the cases of the GPU tests, and one way to run a module's restatement on them ----------------------------------------------
MODULES = ("set_visc", "thickness_diffuse", "varmix", "mle")
EDGE_CASES = {"set_visc": ("eos", "rlay", "body", "psurf"), "thickness_diffuse": ("eos", "noeos", "gm", "khth2d"),
              "varmix": ("eady_diag", "visbeck_diag", "just_e"), "mle": ("detect", "both_filters", "front_plane")}
STAGGER = {"set_visc": lambda n: n[-1],
           "thickness_diffuse": lambda n: dict(h="h", uhtr="u", vhtr="v", uhGM="u", vhGM="v")[n],
           "varmix": lambda n: VARMIX_STAG[n], "mle": lambda n: MLE_STAG.get(n, "h")}


def module_metrics(module, d, M):
    """mixedlayer_restrat's grids carry an equator (tests/mle_ref.metrics)."""
    return mle_ref.metrics(d, M) if module == "mle" else M


def restatement(module, name, d, M, GV, orc, scale_inputs=None, every_diag=False):
    """(the arguments of the module's _device helper, the restatement's outputs) of a case under WRIGHT.  `scale_inputs` maps the
    inputs before the run (the corner experiment)."""
    M = module_metrics(module, d, M)
    ident = scale_inputs or (lambda inp: inp)
    if module == "set_visc":
        P, eos, ps, ray, opts = setvisc_ref.switch_case(name, form=abi.WRIGHT)
        Rlay, _ = abi.layer_densities(d.nk)
        inp = ident(setvisc_ref.inputs(d, M, GV, **opts))
        want, _ = setvisc_ref.run(d, M, GV, P, inp, eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray, orc=orc)
        return ((d, M, GV, P, inp), dict(eos=eos, Rlay=Rlay, give_ps=ps, give_ray=ray)), want
    if module == "thickness_diffuse":
        P, eos, ps, stored, gm, dt, opts = thickdiff_ref.case(name, form=abi.WRIGHT)
        inp = ident(thickdiff_ref.inputs(d, M, GV, **opts))
        want, _ = thickdiff_ref.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, stored=stored, give_gm=gm, orc=orc)
        return ((d, M, GV, P, inp, dt), dict(eos=eos, give_ps=ps, stored=stored, give_gm=gm)), want
    if module == "varmix":
        P, eos, ps, dg, dt, opts = varmix_ref.case(name, GV, form=abi.WRIGHT, nk=d.nk)
        inp = ident(varmix_ref.inputs(d, M, GV, **opts))
        want, _ = varmix_ref.run(d, M, GV, P, inp, dt, eos=eos, give_ps=ps, give_diag=dg, orc=orc)
        return ((d, M, GV, P, inp, dt), dict(eos=eos, give_ps=ps, give_diag=dg)), want
    P, given, dg, dt = mle_ref.case(name, GV)
    eos = abi.eos_params_default(abi.WRIGHT)
    inp = ident(mle_ref.inputs(d, M, GV))
    dg = dg or every_diag
    want, _ = mle_ref.run(d, M, GV, P, inp, dt, eos, given=given, give_diag=dg, orc=orc)
    return ((d, M, GV, P, inp, dt, eos, given, dg), {}), want


# ---- the corners of the halo ----------------------------------------------------------------------------------------------------
CORNER_FACTOR = 1.25


def scale_corners(d, names):
    """Multiply the words of the four corner cells of the halo's first ring, (isc-1 | iec+1, jsc-1 | jec+1), by CORNER_FACTOR in
    every layer of the named inputs."""
    def f(inp):
        out = dict(inp)
        for n in names:
            a = inp[n].copy()
            for i in (-1, d.ni):
                for j in (-1, d.nj):
                    a[..., d.joff + j, d.ioff + i] *= CORNER_FACTOR
            out[n] = a
        return out
    return f


def zero_corners(d, a):
    a = a.copy()
    for i in (-1, d.ni):
        for j in (-1, d.nj):
            a[..., d.joff + j, d.ioff + i] = 0.0
    return a


def _differ(a, b):
    return not np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _corner_runs(module, name, grid, orc, names):
    d, M = getattr(H, grid)(nk=4)[1:]
    GV = abi.vgrid_default()
    a = restatement(module, name, d, M, GV, orc, every_diag=True)[1]
    b = restatement(module, name, d, M, GV, orc, scale_inputs=scale_corners(d, names), every_diag=True)[1]
    return d, a, b


def _own(module, d, n, a):
    return a[(Ellipsis,) + H.interior(d, STAGGER[module](n))]


CORNER_READERS = [("set_visc", "eos", ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")),
                  ("set_visc", "rlay", ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")),
                  ("set_visc", "psurf", ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")),
                  ("set_visc", "body", ("Ray_u", "Ray_v")),
                  ("varmix", "eady_diag", ("SN_u", "SN_v")),
                  ("varmix", "visbeck_diag", ("SN_u", "SN_v", "S2_u", "S2_v")),
                  ("varmix", "just_e", ("SN_u", "SN_v"))]


@pytest.mark.parametrize("module,name,outputs", CORNER_READERS)
def test_own_faces_read_the_corners_of_the_halo(module, name, outputs, orc):
    """With the corner cells of h, T, S (and u, v) scaled, these outputs change at the tile's own faces on the torus, in both
    directions; on benchmark_small no output changes there at all -- which is why a kernel that fetched a wrong corner word passed
    on the closed grids."""
    names = ("h", "T", "S", "u", "v") if module == "set_visc" else ("h", "T", "S")
    d, a, b = _corner_runs(module, name, "torus", orc, names)
    for n in outputs:
        assert _differ(_own(module, d, n, a[n]), _own(module, d, n, b[n])), n
    if module == "varmix" and "slope_x" in a:          # the slopes and N2 only on their widened ranges
        for n in ("slope_x", "slope_y", "N2_u", "N2_v"):
            assert _differ(a[n], b[n]) and not _differ(_own(module, d, n, a[n]), _own(module, d, n, b[n])), n
    d, a, b = _corner_runs(module, name, "benchmark_small", orc, names)
    for n in a:
        assert not _differ(_own(module, d, n, a[n]), _own(module, d, n, b[n])), n


@pytest.mark.parametrize("module,name", [("thickness_diffuse", n) for n in ("eos", "noeos", "gm", "khth2d", "slopes_eos")] +
                         [("mle", n) for n in ("detect", "both_filters", "front_plane", "pbl")])
def test_what_does_not_read_the_corners(module, name, orc):
    """thickness_diffuse: no bit of any output (but the scaled words of h themselves) depends on the corner cells, torus or not.
    mixedlayer_restrat: nothing at the tile's own points; the h-point planes that are posted one point into the halo change, at
    the corner cells alone."""
    for grid in ("torus", "benchmark_small"):
        d, a, b = _corner_runs(module, name, grid, orc, ("h", "T", "S"))
        for n in a:
            assert not _differ(_own(module, d, n, a[n]), _own(module, d, n, b[n])), (grid, n)
            assert not _differ(zero_corners(d, a[n]), zero_corners(d, b[n])), (grid, n, "beyond the corner cells")
        if module == "mle":
            assert _differ(a["Rml_av_fast"], b["Rml_av_fast"]), grid
