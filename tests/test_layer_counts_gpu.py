"""Both sides of every layer-count dispatch edge, against the oracle.

The kernels that keep a whole column on chip unroll it at compile time (mom6x_dev.h COLS_NK_DISPATCH): an instantiation for
exactly 75 layers, then BOUNDS of 52, 66 and 76 slots with a uniform test `k < nk` on the layer index; deeper columns walk
through HBM.  k_hv_fused holds the whole column up to 80 layers and works in 25- or 15-layer chunks above that (hor_visc.hip).
The mass-flux kernels carry at most 128 layers; deeper, continuity runs the thread-per-column kernels in the REFERENCE order.
An off-by-one in a `k < nk` guard, a wrong LDS size for a bound or a ragged last chunk shows at exactly these edges, so every
case here sits on one side of one: the tracer solves, the z* regrid with the remap after it and horizontal_viscosity, each bit
for bit against the oracle (zeros of opposite sign not tolerated), and each case shows from the profile labels which
instantiation -- or which walk -- actually ran.  (The whole split-RK2 step at 52 / 53 / 66 / 67 / 77 layers and the mass flux at
32 / 33 / 64 / 65 / 80 / 81 / 128 / 130 are in the lists of tests/test_rk2_gpu.py and tests/test_continuity_gpu.py.)

Grids of 70 x 10 and 40 x 12 columns: rows that are not a multiple of the 64-lane work-group."""
import ctypes as C

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests.test_continuity_gpu import _run_case
from tests.test_horvisc_gpu import horizontal_viscosity_case
from tests.test_remap_gpu import regrid_zstar_remap_case
from tests.test_tracer_gpu import tridiagonal_case, vertdiff_sinking_case

pytestmark = pytest.mark.gpu

COLS_NK_BOUND = 76
MOM6X_EUNSUPPORTED = 3   # include/mom6x.h


def cols_label(nk, pair=False):
    """The template argument COLS_NK_DISPATCH picks for nk (the TS pair has no exact-75 instantiation), as the profile labels
    spell it; None: the walk."""
    if nk > COLS_NK_BOUND:
        return None
    if nk == 75 and not pair:
        return "75"
    return "-52" if nk <= 52 else "-66" if nk <= 66 else "-COLS_NK_BOUND"


@pytest.mark.parametrize("nk", [52, 53, 66, 67, 74, 76, 77, 90])
def test_tridiagonal_solvers_across_the_column_bounds(orc, nk):
    """triDiagTS (T and S paired, and single), triDiagTS_Eulerian, tracer_vertdiff and tracer_vertdiff_Eulerian: the body of
    tests/test_tracer_gpu.py::test_tridiagonal_solvers.  Five launches of one k_tridiag_cols instantiation (the pair's bound, the
    four single-field solves' instantiation), or five of the walk k_tridiag above 76 layers."""
    rep = tridiagonal_case(orc, H.benchmark_small(nk=nk, ni=70, nj=10))
    cols = {k: n for k, (n, _) in rep.items() if k.startswith("k_tridiag")}
    single, pair = cols_label(nk), cols_label(nk, pair=True)
    if single is None:
        assert cols == {"k_tridiag": 5}, cols
    elif single == pair:
        assert cols == {f"k_tridiag_cols<{single}>": 5}, cols
    else:
        assert cols == {f"k_tridiag_cols<{pair}>": 1, f"k_tridiag_cols<{single}>": 4}, cols


@pytest.mark.parametrize("nk", [52, 53, 66, 67, 74, 76, 77, 90])
def test_tracer_vertdiff_with_sinking_across_the_column_bounds(orc, nk):
    """tracer_vertdiff (+ _Eulerian) with sink_rate and a bottom reservoir: the body of
    tests/test_tracer_gpu.py::test_tracer_vertdiff_with_sinking at the same layer counts."""
    vertdiff_sinking_case(orc, H.benchmark_small(nk=nk, ni=70, nj=10), True)


@pytest.mark.parametrize("nk", [52, 53, 66, 67, 76, 77, 90])
@pytest.mark.parametrize("mods", [dict(), dict(old_grid_weight=0.4, depth_of_time_filter_shallow=200., depth_of_time_filter_deep=900.)],
                         ids=["plain", "time_filter"])
def test_ALE_regrid_zstar_then_remap_across_the_column_bounds(orc, nk, mods):
    """ALE_regrid for z*, then the remapping of two tracers and the velocities onto the new grid: the body of
    tests/test_remap_gpu.py::test_ALE_regrid_zstar_then_remap.  k_regrid_zstar_cols with the bound COLS_NK_DISPATCH picks,
    or the walk k_regrid_zstar above 76 layers."""
    rep = regrid_zstar_remap_case(orc, H.benchmark_small(nk=nk, ni=70, nj=12), mods)
    ran = {k: n for k, (n, _) in rep.items() if k.startswith("k_regrid_zstar")}
    lab = cols_label(nk)
    assert ran == ({"k_regrid_zstar": 1} if lab is None else {f"k_regrid_zstar_cols<{lab}>": 1}), ran


@pytest.mark.parametrize("nk", [75, 80, 81, 90, 95, 100])
@pytest.mark.parametrize("flags", ["default_biharmonic", "om4_class", "both_better_bounds"])
def test_horizontal_viscosity_across_the_column_chunks(orc, nk, flags):
    """horizontal_viscosity (the body of tests/test_horvisc_gpu.py::test_horizontal_viscosity): k_hv_fused holds the whole column
    up to 80 layers (75, 80), above that 25-layer chunks when they divide the column (100) and 15-layer chunks otherwise -- ragged
    (81: 5 x 15 + 6, 95: 6 x 15 + 5) or exact (90).  Default flags, the OM4-class instantiation (Laplacian + Smagorinsky
    biharmonic) and Laplacian + biharmonic with both better bounds; one launch of k_hv_fused, not the four-kernel chain."""
    gg, d, M = H.benchmark_small(nk=nk, ni=40, nj=12)
    rep = horizontal_viscosity_case(orc, (gg, d, H.partial_faces(d, M)), flags)
    assert rep.get("k_hv_fused", (0, 0))[0] == 1 and "k_hv_strain" not in rep, sorted(rep)


@pytest.mark.parametrize("order", [abi.SUM_TREE16, abi.SUM_TREE16_FMA], ids=["tree", "fma"])
def test_tree_orders_are_refused_beyond_128_layers(order):
    """The wave-owned kernel carries at most 128 layers (8 slots x 16 lanes): continuity_init refuses the tree orders at 130 with
    MOM6X_EUNSUPPORTED, and accepts them at 128."""
    from mom6_amd.dycore import Dycore
    for nk, want in ((130, MOM6X_EUNSUPPORTED), (128, 0)):
        gg, d, M = H.benchmark_small(nk=nk, ni=40, nj=12)
        GV = abi.vgrid_default()
        dyc = Dycore(d, M, GV)
        CS = abi.continuity_params_default(nk, GV.Angstrom_H)
        CS.sum_order = order
        assert dyc.lib.mom6x_continuity_init(dyc.ctx, C.byref(CS)) == want, nk
        dyc.close()


@pytest.mark.parametrize("mode", ["full", "adjust"])
def test_default_order_beyond_128_layers_is_the_reference_order(orc, mode, monkeypatch):
    """Without MOM6X_SUMS and MOM6X_MASSFLUX, 130 layers: the default order is REFERENCE, the thread-per-column kernels run (not
    the wave-owned or LDS kernels), bit for bit against the REFERENCE-order oracle."""
    monkeypatch.delenv("MOM6X_SUMS", raising=False)
    monkeypatch.delenv("MOM6X_MASSFLUX", raising=False)
    assert abi.default_sum_order(130) == abi.SUM_REFERENCE and abi.continuity_params_default(130).sum_order == abi.SUM_REFERENCE
    ran = {}
    _run_case(orc, H.benchmark_small(nk=130, ni=40, nj=12), 1, mode, thin=0.1, launches=ran)
    assert ran.get("k_mass_flux<DIR>", (0, 0))[0] >= 2, sorted(ran)
    assert not any(k.startswith(("k_mass_flux_wave", "k_mass_flux_lds")) for k in ran), sorted(ran)
