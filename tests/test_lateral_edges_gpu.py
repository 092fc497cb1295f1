"""set_viscous_BBL, thickness_diffuse, calc_slope_functions and mixedlayer_restrat on the device against their restatements where a
one-lane-per-face kernel goes wrong and the module tests' closed basins cannot show it: the eight doubly re-entrant grids of
tests/test_lateral_edges_cpu.py (EDGE_SHAPES: every launch extent an exact multiple of the work-group and one more, along i over
one and over two work-groups, open water up to the last lane and in every corner of the halo), and H.torus (96 x 40) and H.channel
(32 x 24) with every case of each module's list.  Whole arrays, bit for bit, every output and diagnostic starting as NaN; no
tolerance anywhere."""
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import mle_ref, setvisc_ref, thickdiff_ref, varmix_ref
from tests import test_mixed_layer_restrat_gpu as mle_gpu
from tests import test_set_visc_gpu as setvisc_gpu
from tests import test_thickness_diffuse_gpu as thickdiff_gpu
from tests import test_varmix_gpu as varmix_gpu
from tests.test_lateral_edges_cpu import EDGE_CASES, EDGE_SHAPES, MODULES, edge_grid, module_metrics, restatement
from tests.test_thickness_diffuse_gpu import _bits

pytestmark = pytest.mark.gpu
DEVICE = {"set_visc": setvisc_gpu._device, "thickness_diffuse": thickdiff_gpu._device, "varmix": varmix_gpu._device,
          "mle": mle_gpu._device}
# every case of each module's own list; mixedlayer_restrat without "tail", whose pow has its tolerance test in the module's file
ALL_CASES = {"set_visc": tuple(setvisc_ref.SWITCHES), "thickness_diffuse": tuple(thickdiff_ref.CASES),
             "varmix": tuple(varmix_ref.CASES), "mle": mle_ref.CASES_TAIL0}
GRIDS = {"torus": lambda: H.torus(nk=8)[1:], "channel": lambda: H.channel(nk=8)[1:]}


def _run_cases(module, names, d, M, label, every_diag):
    """The cases one after the other in one context, each against the restatement on the same inputs."""
    from mom6_amd.dycore import Dycore
    from oracle import orc
    orc.build()
    GV = abi.vgrid_default()
    dy = Dycore(d, module_metrics(module, d, M), GV)
    try:
        assert dy.lane_launch_shape() == abi.lane_launch_shape()
        for name in names:
            (args, kw), want = restatement(module, name, d, M, GV, orc, every_diag=every_diag)
            got = DEVICE[module](*args, dy=dy, **kw)
            assert set(got) == set(want)
            for n in want:
                _bits(got[n], want[n], f"{label}/{module}/{name}:{n}")
    finally:
        dy.close()


@pytest.mark.parametrize("ni,nj", EDGE_SHAPES)
@pytest.mark.parametrize("module", MODULES)
def test_launch_extents(module, ni, nj):
    """Four layers on a torus of ni x nj cells.  An extent that is one lane or one row short leaves the last column or row of a
    work array or of an output unwritten: NaN, or the fill of the work space, where the restatement has a number -- at an open
    face, so that nothing masks it.  mixedlayer_restrat is given every diagnostic pointer."""
    d, M = edge_grid(ni, nj)
    _run_cases(module, EDGE_CASES[module], d, M, f"{ni}x{nj}", every_diag=True)


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("module", MODULES)
def test_reentrant_grids(module, grid):
    """Eight layers, every case of the module's list under WRIGHT.  The torus: two work-groups along i and open water in the
    corners of the halo, which the four-face averages of calc_slope_functions and set_v_at_u | set_u_at_v read; the channel: walls
    that are whole rows.  The branch counts of the module tests are not asked for here: a torus has no coast."""
    d, M = GRIDS[grid]()
    _run_cases(module, ALL_CASES[module], d, M, grid, every_diag=False)
