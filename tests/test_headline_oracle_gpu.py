"""The headline grid against the oracle: one whole split-RK2 step at 1440 x 1080 x 75 with every callee on the device
(vertvisc_coef, horizontal_viscosity, btstep), built from bench.py's own recipe -- bench.global_grid, bench.hor_visc_params and
the parameters and seeded fields of bench.build_model -- with the oracle given exactly the device's initial arrays.

Faults that only a large grid shows are invisible on the small cases of the other files: grid-stride and work-group-count
arithmetic, 32-bit overflow of pitched 3-D offsets (about 1.2e8 cells per field here), the XCD-ordered tile walks.
tests/test_configs_gpu.py checks this grid through size-independent properties; this file holds it to the oracle:
  - MOM6X_SUMS=exact with BT_STRONG_DRAG: bit for bit against the REFERENCE-order oracle,
  - the default order (TREE16_FMA) with BT_STRONG_DRAG: bit for bit against the oracle's restatement of the same arithmetic,
  - the benchmark's exact configuration (default order, btstep's default drag path with its pow): within 1e-12 of range of the
    REFERENCE-order oracle after the step (recorded by test_sum_order_gpu._report as "headline_1440x1080x75").
One oracle step is about 13 s on 16 host threads and its model holds some 30 GB: each case frees it before the next, and an
allocation that fails FAILS the test (a skip would hide that this grid went unchecked)."""
import gc

import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests.test_rk2_gpu import STAG
from tests.test_sum_order_gpu import _budgets, _drift, _fields, _report

pytestmark = pytest.mark.gpu
G = abi.G

NI, NJ, NK, DT = 1440, 1080, 75, 900.0
HEADLINE_BOUND = 1.0e-12   # of max |field|, after the step


@pytest.fixture(scope="module")
def headline_inputs(orc):
    """The grid and the initial host arrays of bench.build_model / bench.cpu_baseline (synth, not synth_dev: the oracle must get
    exactly the device's inputs, so both sides start from these)."""
    import os
    import bench
    from mom6_amd import synth
    orc.set_threads(orc.usable_cores())
    try:
        gg = bench.global_grid(NI, NJ)
        d, M = gg.tile(NK, 4, (1, 1), (0, 0))
        h, u, v = synth.make_state(d, M, u_max=float(os.environ.get("MOM6X_BENCH_UMAX", "0.5")), h_pert=0.01)
        kbu = np.ascontiguousarray(2.0e-3 * (1.0 + 0.5 * synth.smooth_field(d, 91, ox=1.0, oy=0.5)) * M[G["mask2dCu"]])
        kbv = np.ascontiguousarray(2.0e-3 * (1.0 + 0.5 * synth.smooth_field(d, 92, ox=0.5, oy=1.0)) * M[G["mask2dCv"]])
        taux = np.ascontiguousarray(0.1 * synth.smooth_field(d, 41, ox=1.0, oy=0.5) * M[G["mask2dCu"]])
    except MemoryError as e:
        pytest.fail(f"host memory: the headline grid's initial state could not be allocated ({e!r})")
    return dict(d=d, M=M, h=h, u=u, v=v, kbu=kbu, kbv=kbv, bbl=np.full(d.shape2(), 10.0), taux=taux, tauy=np.zeros(d.shape2()))


def _headline_pair(orc, X, dev_order, orc_order, strong_drag):
    """An oracle model and a device model of bench.build_model's configuration from the same initial arrays, each stepped once."""
    import bench
    import torch
    from mom6_amd.dycore import Dycore
    d, M = X["d"], X["M"]
    GV = abi.vgrid_default()
    Rlay, gp = abi.layer_densities(NK, GV.Rho0, GV.g_Earth)

    def params(order):
        cont = abi.continuity_params_default(NK, GV.Angstrom_H)
        cont.sum_order = order
        bt = abi.barotropic_params_default(20.0)
        bt.strong_drag = strong_drag
        return (cont, bt, abi.coriolis_params_default(), abi.pgf_params_default(GV.Rho0), abi.rk2_params_default(),
                abi.vertvisc_params_default(Kv=1.0e-4, Hmix=20.0, Hbbl=10.0), bench.hor_visc_params(abi, DT))

    try:
        # ---- oracle
        cont, bt, cor, pgf, rk2, vv, hv = params(orc_order)
        m = orc.OrcModel(d, M, GV, cont, bt, cor, pgf, rk2, Rlay, gp, 0)
        m.set_vertvisc(vv, X["kbu"], X["kbv"], X["bbl"], X["bbl"].copy())
        m.set_hor_visc(hv)
        so = dict(u=X["u"].copy(), v=X["v"].copy(), h=X["h"].copy(), uh=np.zeros_like(X["h"]), vh=np.zeros_like(X["h"]),
                  uhtr=np.zeros_like(X["h"]), vhtr=np.zeros_like(X["h"]), eta_av=np.zeros(d.shape2()))
        m.initialize(so["u"], so["v"], so["h"], so["uh"], so["vh"], DT)
        m.step(so["u"], so["v"], so["h"], so["uh"], so["vh"], so["uhtr"], so["vhtr"], so["eta_av"], X["taux"], X["tauy"], DT,
               (None,) * 6, calc_dtbt=True)
    except MemoryError as e:
        pytest.fail(f"host memory: the oracle model of the headline grid could not be allocated ({e!r})")
    # ---- device
    cont2, bt2, cor2, pgf2, rk22, vv2, hv2 = params(dev_order)
    dyc = Dycore(d, M, GV, 0)
    dyc.continuity_init(cont2); dyc.barotropic_init(bt2); dyc.CoriolisAdv_init(cor2); dyc.PressureForce_init(pgf2, Rlay, gp)
    dyc.initialize_dyn_split_RK2(rk22)
    dyc.vertvisc_init(vv2)
    keep = [dyc.to_dev(a) for a in (X["kbu"], X["kbv"], X["bbl"], X["bbl"])]
    dyc.vertvisc_set_visc(*keep)
    dyc.hor_visc_init(hv2)
    sg = dict(u=dyc.to_dev(X["u"]), v=dyc.to_dev(X["v"]), h=dyc.to_dev(X["h"]), uh=dyc.zeros3(), vh=dyc.zeros3(),
              uhtr=dyc.zeros3(), vhtr=dyc.zeros3(), eta_av=dyc.zeros2())
    tx, ty = dyc.to_dev(X["taux"]), dyc.to_dev(X["tauy"])
    torch.cuda.synchronize()
    dyc.dyn_split_RK2_new_run(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], DT)
    dyc.step_MOM_dyn_split_RK2(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], sg["uhtr"], sg["vhtr"], sg["eta_av"], tx, ty, DT,
                               calc_dtbt=True)
    dyc.sync()
    assert np.isfinite(so["u"]).all() and np.abs(so["u"]).max() > 1e-3
    return dict(d=d, M=M, dt=DT, inp=dict(h=X["h"]), cont=cont2, m=m, so=so, dyc=dyc, sg=sg, keep=(keep, tx, ty))


def _free(p):
    import torch
    p["dyc"].close()
    p.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _bitwise(p):
    for n, a, b in _fields(p):
        H.assert_bitwise(a, b, n, H.interior(p["d"], STAG[n]), signed_zero_ok=False)


def test_headline_reference_order_is_bit_identical(orc, headline_inputs, monkeypatch):
    """MOM6X_SUMS=exact, BT_STRONG_DRAG: every prognostic and restart field equals the REFERENCE-order oracle in every bit."""
    monkeypatch.setenv("MOM6X_SUMS", "exact")
    order = abi.default_sum_order(NK)
    assert order == abi.SUM_REFERENCE
    p = _headline_pair(orc, headline_inputs, order, abi.SUM_REFERENCE, strong_drag=1)
    try:
        _bitwise(p)
        _budgets(p)
    finally:
        _free(p)


def test_headline_default_order_is_bit_identical_to_its_restatement(orc, headline_inputs, monkeypatch):
    """The default order (TREE16_FMA), BT_STRONG_DRAG: every field equals the oracle's restatement of the same arithmetic."""
    monkeypatch.delenv("MOM6X_SUMS", raising=False)
    order = abi.default_sum_order(NK)
    assert order == abi.SUM_TREE16_FMA
    p = _headline_pair(orc, headline_inputs, order, order, strong_drag=1)
    try:
        _bitwise(p)
        _budgets(p)
    finally:
        _free(p)


def test_headline_benchmark_configuration_within_bound_of_the_reference_order(orc, headline_inputs, monkeypatch):
    """The benchmark's exact configuration -- the default order on btstep's default drag path (bt_rem = av_rem**(1/nstep), the
    device's pow) -- against the REFERENCE-order oracle with libm's pow: every field within 1e-12 of its range after the step."""
    monkeypatch.delenv("MOM6X_SUMS", raising=False)
    order = abi.default_sum_order(NK)
    assert order == abi.SUM_TREE16_FMA
    p = _headline_pair(orc, headline_inputs, order, abi.SUM_REFERENCE, strong_drag=0)
    try:
        rows = [_drift(p)]
        eta_err = _budgets(p)
        _report("headline_1440x1080x75", rows, dict(sum_k_uh_minus_uhbt_as_eta_change=eta_err, tol_eta=p["cont"].tol_eta),
                bound=HEADLINE_BOUND)
        bad = {n: v for n, v in rows[-1].items() if v > HEADLINE_BOUND}
        assert not bad, bad
    finally:
        _free(p)
