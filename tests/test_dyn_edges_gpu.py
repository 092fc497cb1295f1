"""CorAdCalc, horizontal_viscosity, PressureForce, the split RK2 step and advect_tracer on the device against the oracle where their
kernels go wrong and the module tests' closed basins cannot show it: doubly re-entrant grids without land (H.torus) whose extents
sit on the edges of the tiles (mom6x_tile_steps) and of the 64 x 4 work-groups (mom6x_lane_launch_shape).  The shapes, the table of
launches they come from and the reasons are in tests/test_dyn_edges_cpu.py, which guards them without a GPU.

Bit for bit at the tile's own points against the oracle on the same host arrays, the sign of a zero included.  The outputs of the
single-module calls start as NaN, and beyond the points their launch reaches (cover_* below, from the launch lines) every word
must still be NaN.  The bodies are those of the module tests (CorAdCalc_case, horizontal_viscosity_case, PressureForce_case,
PressureForce_eos_case, advect_tracer_case, test_rk2_gpu.run)."""
import os
import subprocess
import sys

import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import test_rk2_gpu as rk2_gpu
from tests.test_dyn_edges_cpu import (ADVECT_X_CASES, ADVECT_Y_CASES, CORAD_EDGE_MODS, CORAD_LANE_MODS, CORAD_TILE_SHAPES, CORAD_TWO_CHUNKS,
                                      HV_EDGE_FLAGS, HV_LANE_FLAGS, HV_TILE_SHAPES, HV_TWO_CHUNKS, LANE_SHAPES, PGF_EOS_CASES,
                                      RK2_EXTRA_SHAPES, RK2_SHAPES, TRACER_X_SHAPES, TRACER_Y_SHAPES, corad_kernel, hor_visc_kernel,
                                      rk2_hor_visc, torus)
from tests.test_dyn_gpu import CORAD_MODS, CorAdCalc_case, PressureForce_case, PressureForce_eos_case
from tests.test_horvisc_gpu import FLAGS, horizontal_viscosity_case
from tests.test_tracer_gpu import ADVECT_CASES, advect_tracer_case

pytestmark = pytest.mark.gpu
# the two-kernel form of CorAdCalc and the four-kernel chain of hor_visc for every case (read once per process: the last test
# of this file runs the CorAdCalc and hor_visc tests again in a process that has them set)
LEGACY_CORAD = os.environ.get("MOM6X_CORAD") == "legacy"
LEGACY_HORVISC = os.environ.get("MOM6X_HORVISC") == "legacy"


def cover_faces(d):
    """CAu | CAv and diffu | diffv: k_corad_acc and k_hv_accel are launched over gridk | grid3(nxa(ni + 1, -1), nj + 1, ...), the
    points (-1..ni-1, -1..nj-1), and k_corad_lds, k_corad_fused and k_hv_fused write where `out` | `out_u`, `out_v` hold, within
    the same points."""
    return d.sl(-1, d.ni - 1, -1, d.nj - 1)


def cover_pgf(d):
    """PFu, PFv, pbce and eta: k_pgf_main and k_pgf_main_eos are launched over grid3(nxa(ni + 2, -1), nj + 2, 1), the points
    (-1..ni, -1..nj)."""
    return d.sl(-1, d.ni, -1, d.nj)


def _ids(m):
    return "-".join(f"{k}={v}" for k, v in m.items()) or "default"


def _corad(orc, cfg, mods):
    rep = CorAdCalc_case(orc, cfg, mods, cover=cover_faces(cfg[1]))
    ran = {k for k in rep if k in ("k_corad_lds", "k_corad_fused", "k_corad_q")}
    assert ran == {corad_kernel(mods, LEGACY_CORAD)} and rep[ran.pop()][0] == 1, (mods, sorted(rep))


def _hor_visc(orc, cfg, flags):
    rep = horizontal_viscosity_case(orc, cfg, flags, cover=cover_faces(cfg[1]))
    ran = {k for k in rep if k in ("k_hv_fused", "k_hv_accel")}
    assert ran == {hor_visc_kernel(flags, LEGACY_HORVISC)} and rep[ran.pop()][0] == 1, (flags, sorted(rep))
    assert ("k_hv_leith" in rep) == ("leith" in flags)


# ---- CorAdCalc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("areas", ["even", "uneven"])
@pytest.mark.parametrize("mods", CORAD_MODS, ids=_ids)
def test_CorAdCalc_on_the_torus(orc, mods, areas):
    """Every option set of test_CorAdCalc on 96 x 40 x 3 points of open water: 4 x 3 tiles of k_corad_lds | k_corad_fused, two
    work-groups along i of k_corad_q and k_corad_acc, wet corner cells in the halo.  Once more with cell areas that differ from
    cell to cell (H.uneven_cell_areas): on the torus as it is every cell has the same area, and Area_q would come out right from
    the area of any neighbour."""
    gg, d, M = H.torus()
    _corad(orc, (gg, d, H.uneven_cell_areas(d, M) if areas == "uneven" else M), mods)


@pytest.mark.parametrize("ni,nj,nk", [s + (4,) for s in CORAD_TILE_SHAPES] + [CORAD_TWO_CHUNKS])
def test_CorAdCalc_tile_edges(orc, ni, nj, nk):
    """ni + 1 and nj + 1 a whole number of tile steps and one more: a tile count that is one short leaves the last column or row
    NaN, one that is one too many (or a work-group past the count that does not leave) writes beyond cover_faces.  50 layers on one
    step by one: two chunks of layers."""
    for mods in CORAD_EDGE_MODS:
        _corad(orc, torus(ni, nj, nk), mods)


@pytest.mark.parametrize("ni,nj", LANE_SHAPES)
def test_CorAdCalc_lane_edges(orc, ni, nj):
    """The two-kernel form on the launch extents of k_corad_q (nxa(ni + 3, -2) by nj + 3) and k_corad_acc (nxa(ni + 1, -1) by
    nj + 1)."""
    for mods in CORAD_LANE_MODS:
        _corad(orc, torus(ni, nj), mods)


# ---- horizontal_viscosity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_horizontal_viscosity_on_the_torus(orc, flags):
    """Every entry of FLAGS on 96 x 40 x 4 points of open water."""
    _hor_visc(orc, H.torus(nk=4), flags)


@pytest.mark.parametrize("ni,nj,nk", [s + (4,) for s in HV_TILE_SHAPES] + [HV_TWO_CHUNKS])
def test_horizontal_viscosity_tile_edges(orc, ni, nj, nk):
    """The OM4 and the generic instantiation of k_hv_fused (and the four-kernel chain) with ni + 1 and nj + 1 a whole number of tile
    steps and one more; 100 layers on one step by one: chunks of 25 layers."""
    for flags in HV_EDGE_FLAGS:
        _hor_visc(orc, torus(ni, nj, nk), flags)


@pytest.mark.parametrize("ni,nj", LANE_SHAPES)
def test_horizontal_viscosity_lane_edges(orc, ni, nj):
    """The four-kernel chain with Leith on the launch extents of k_hv_strain, k_hv_del2, k_hv_vort, k_hv_leith, k_hv_stress and
    k_hv_accel."""
    for flags in HV_LANE_FLAGS:
        _hor_visc(orc, torus(ni, nj), flags)


def test_the_legacy_switches():
    """MOM6X_CORAD=legacy and MOM6X_HORVISC=legacy are read once per process: the CorAdCalc and hor_visc tests above again in a
    process that has them set, where every case must have run k_corad_q + k_corad_acc | the four-kernel chain."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                        "test_CorAdCalc or test_horizontal_viscosity"], env=dict(os.environ, MOM6X_CORAD="legacy", MOM6X_HORVISC="legacy"),
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- PressureForce --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni,nj", LANE_SHAPES)
def test_PressureForce_lane_edges(orc, ni, nj):
    """The layered path (k_pgf_main) and k_pgf_main_eos -- WRIGHT with the analytic integrals, with the PLM and the PPM
    reconstruction and MassWghtInterp = 3, UNESCO with EOS_QUADRATURE -- on four layers."""
    cfg = torus(ni, nj)
    PressureForce_case(orc, cfg, 1, cover=cover_pgf(cfg[1]))
    for form, mods in PGF_EOS_CASES:
        PressureForce_eos_case(orc, cfg, form, mods, cover=cover_pgf(cfg[1]))


# ---- the split RK2 step ---------------------------------------------------------------------------------------------------------
def _rk2(orc, cfg, **kw):
    rk2_gpu.run(orc, cfg, nsteps=2, bt_mod=dict(strong_drag=1), dev_vv=dict(), hv=rk2_hor_visc(cfg), **kw)


@pytest.mark.parametrize("ni,nj", RK2_SHAPES)
def test_rk2_steps(orc, sums, ni, nj):
    """Two steps with vertvisc_coef and OM4-class horizontal_viscosity inside the step, four layers, under each order of the
    mass-flux sums: every prognostic and restart field bit for bit, the volume kept (test_rk2_gpu.run)."""
    _rk2(orc, torus(ni, nj))


@pytest.mark.parametrize("ni,nj", RK2_EXTRA_SHAPES)
def test_rk2_steps_without_the_remnant_in_the_solve(orc, sums, ni, nj):
    _rk2(orc, torus(ni, nj), rk2_mod=dict(visc_rem_dt_bug=0))


@pytest.mark.parametrize("ni,nj", RK2_EXTRA_SHAPES)
def test_rk2_steps_with_an_equation_of_state(orc, sums, ni, nj):
    _rk2(orc, torus(ni, nj), eos_form=abi.WRIGHT, recon=1)


# ---- advect_tracer --------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["tiled", "legacy"])
def tracer_path(request, monkeypatch):
    """As in tests/test_tracer_gpu.py: one kernel per direction and pass, and the face + cell kernel pairs."""
    monkeypatch.setenv("MOM6X_TRACER", request.param)
    return request.param


@pytest.mark.parametrize("schemes,first,post", ADVECT_CASES)
def test_advect_tracer_on_the_torus(orc, tracer_path, schemes, first, post):
    advect_tracer_case(orc, H.torus(nk=2), schemes, first, post)


@pytest.mark.parametrize("ni,nj", TRACER_X_SHAPES + TRACER_Y_SHAPES)
def test_advect_tracer_tile_edges(orc, tracer_path, ni, nj):
    """The first pass of an x-first call over one tile of cells and over one cell more, of a y-first call over one segment of rows
    and over one row more; the tiled path ran that many tiles | segments in every pass."""
    cfg = torus(ni, nj, nk=2)
    for schemes, first, post in (ADVECT_X_CASES if (ni, nj) in TRACER_X_SHAPES else ADVECT_Y_CASES):
        rep = advect_tracer_case(orc, cfg, schemes, first, post)
        assert ("k_ta_x_tile" in rep) == (tracer_path == "tiled") and ("k_ta_face<0>" in rep) == (tracer_path == "legacy"), sorted(rep)
