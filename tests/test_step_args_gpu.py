"""What the RK2 step hands its callees -- the deferrals of btstep / btcalc, the time average and the skipped convergence of its
continuity calls, the widths of its group passes -- are arguments of those calls and nothing a later caller can inherit:
a step that fails half-way leaves the public entry points whole, and the step's own group passes stay as narrow as the reference's."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from mom6_amd import abi, parallel, synth
from tests import cases, helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = abi.G
NK = 8


def _step_context(cfg, inp):
    """A context with everything the step needs and vertvisc_coef on the device (vertvisc_init): the step's btstep calls then
    leave their layer accelerations to the consumer."""
    from mom6_amd.dycore import Dycore
    from tests.test_dyn_gpu import visc_inputs
    gg, d, M = cfg
    cont, bt, cor, pgf, rk2 = cases.rk2_params(d, inp["GV"], dict(strong_drag=1))
    dyc = Dycore(d, M, inp["GV"], 0)
    dyc.continuity_init(cont); dyc.barotropic_init(bt); dyc.CoriolisAdv_init(cor); dyc.PressureForce_init(pgf, inp["Rlay"], inp["gp"])
    dyc.initialize_dyn_split_RK2(rk2)
    vis = list(visc_inputs(d, M)) + [inp["coefs"][0][4], inp["coefs"][0][5]]
    dyc.vertvisc_init(abi.vertvisc_params_default())
    dyc.vertvisc_set_visc(*[dyc.to_dev(a) if a is not None else None for a in vis])
    return dyc


def _public_inputs(cfg, inp):
    """Seeded operands of btcalc(h, h_u, h_v), btstep and continuity_PPM; the BT_cont_type is what a continuity call of a
    context of its own makes of them."""
    from mom6_amd.dycore import BTContDev
    gg, d, M = cfg
    mu, mv = M[G["mask2dCu"]] > 0, M[G["mask2dCv"]] > 0
    h, u, v, dt = inp["h"], inp["u"], inp["v"], inp["dt"]
    I = dict(h=h, u=u, v=v, taux=inp["taux"], tauy=inp["tauy"], ucor=0.9 * u, vcor=0.9 * v)
    I["vr_u"] = np.clip(0.8 + 0.3 * synth.smooth_field(d, 11, nk=d.nk, ox=1.0, oy=0.5), 0, 1) * mu
    I["vr_v"] = np.clip(0.8 + 0.3 * synth.smooth_field(d, 12, nk=d.nk, ox=0.5, oy=1.0), 0, 1) * mv
    I["eta"] = (h.sum(0) - M[G["bathyT"]]) * M[G["mask2dT"]]
    I["eta_PF"] = I["eta"] * (1.0 + 0.01 * synth.smooth_field(d, 43, ox=0.5, oy=0.5))
    pbce = np.zeros_like(h)
    pbce[0] = 9.8
    for k in range(1, d.nk):
        pbce[k] = pbce[k - 1] + 0.02 * (1.0 + 0.1 * synth.smooth_field(d, 30 + k, ox=0.5, oy=0.5))
    I["pbce"] = pbce
    I["bcu"] = 1e-6 * synth.smooth_field(d, 21, nk=d.nk, ox=1, oy=.5) * mu
    I["bcv"] = 1e-6 * synth.smooth_field(d, 22, nk=d.nk, ox=.5, oy=1) * mv
    I = {k: np.ascontiguousarray(a) for k, a in I.items()}
    dyc = _step_context(cfg, inp)
    T = {k: dyc.to_dev(I[k]) for k in ("u", "v", "h", "vr_u", "vr_v")}
    btd = BTContDev(dyc)
    hp, uh, vh = dyc.zeros3(), dyc.zeros3(), dyc.zeros3()
    dyc.continuity_PPM(T["u"], T["v"], T["h"], hp, uh, vh, dt, visc_rem_u=T["vr_u"], visc_rem_v=T["vr_v"], BT_cont=btd)
    dyc.sync()
    I["bt"] = {n: btd[n].cpu().numpy() for n in abi.BTCont._names}
    I["uh0"], I["vh0"] = uh.cpu().numpy(), vh.cpu().numpy()
    dyc.close()
    return I


def _public_calls(dyc, I, dt, dtbt):
    """btcalc, [bt_mass_source,] btstep and continuity_PPM through the public entry points, every output array NaN beforehand."""
    import torch
    from mom6_amd.dycore import BTContDev
    T = {k: dyc.to_dev(a) for k, a in I.items() if k != "bt"}
    btd = BTContDev(dyc)
    for n in abi.BTCont._names:
        btd[n].copy_(torch.from_numpy(I["bt"][n]))
    nan3 = lambda: dyc.zeros3().fill_(float("nan")); nan2 = lambda: dyc.zeros2().fill_(float("nan"))   # noqa: E731
    o = dict(alu=nan3(), alv=nan3(), eta_out=nan2(), uhbtav=nan2(), vhbtav=nan2(), h=nan3(), uh=nan3(), vh=nan3())
    torch.cuda.synchronize()
    dyc.barotropic_dtbt(dtbt)
    dyc.btcalc(T["h"], btd["h_u"], btd["h_v"])
    dyc.bt_mass_source(T["h"], T["eta"], True)          # (CS%eta_cor, which btstep reads, as these operands give it)
    dyc.btstep(T["u"], T["v"], T["eta"], dt, T["bcu"], T["bcv"], T["taux"], T["tauy"], T["pbce"], T["eta_PF"], T["ucor"], T["vcor"],
               o["alu"], o["alv"], o["eta_out"], o["uhbtav"], o["vhbtav"], T["vr_u"], T["vr_v"], btd,
               uh0=T["uh0"], vh0=T["vh0"], u_uh0=T["u"], v_vh0=T["v"])
    dyc.continuity_PPM(T["u"], T["v"], T["h"], o["h"], o["uh"], o["vh"], dt, visc_rem_u=T["vr_u"], visc_rem_v=T["vr_v"])
    dyc.sync()
    return {k: a.cpu().numpy() for k, a in o.items()}


def test_a_failed_step_leaves_the_public_entry_points_whole():
    """One good step, then one whose horizontal_viscosity callback fails: the predictor's btstep has left its layer accelerations
    to their consumer and the corrector's btcalc its fractions to the next btstep.  btcalc, btstep and continuity_PPM called
    afterwards from outside give, bit for bit, what they give in a context that never stepped."""
    import torch
    cfg = H.benchmark_small(nk=NK)
    d = cfg[1]
    inp = cases.rk2_inputs(cfg, False, False)
    dt = inp["dt"]
    I = _public_inputs(cfg, inp)
    dyc = _step_context(cfg, inp)
    sg = dict(u=dyc.to_dev(inp["u"]), v=dyc.to_dev(inp["v"]), h=dyc.to_dev(inp["h"]), uh=dyc.zeros3(), vh=dyc.zeros3(),
              uhtr=dyc.zeros3(), vhtr=dyc.zeros3(), eta_av=dyc.zeros2())
    txd, tyd = dyc.to_dev(inp["taux"]), dyc.to_dev(inp["tauy"])
    torch.cuda.synchronize()
    dyc.dyn_split_RK2_new_run(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], dt)
    args = [sg[n] for n in ("u", "v", "h", "uh", "vh", "uhtr", "vhtr", "eta_av")] + [txd, tyd, dt]
    dyc.step_MOM_dyn_split_RK2(*args, calc_dtbt=True)
    dyc.sync()
    dtbt = dyc.barotropic_dtbt()
    with pytest.raises(abi.Mom6xError, match="horizontal_viscosity callback failed"):
        dyc.step_MOM_dyn_split_RK2(*args, horizontal_viscosity=lambda *a: 1)
    after = _public_calls(dyc, I, dt, dtbt)
    dyc.close()
    fresh = _step_context(cfg, inp)
    want = _public_calls(fresh, I, dt, dtbt)
    fresh.close()
    for k in ("alu", "alv", "eta_out", "uhbtav", "vhbtav", "h", "uh", "vh"):
        H.assert_bitwise(after[k], want[k], f"after a failed step: {k}")
    for k, st in (("alu", "u"), ("alv", "v"), ("h", "h"), ("uh", "u"), ("vh", "v"), ("eta_out", "h")):
        assert np.isfinite(after[k][(Ellipsis,) + tuple(H.interior(d, st))]).all(), k


# ---- the widths of the step's group passes
def _tile_step_counts(layout, pe, uid, out, errors):
    """One step of one tile of the 2 x 1 channel: (packed exchanges, bytes sent) of that step."""
    try:
        import torch
        from mom6_amd.dycore import Dycore
        gg, d1, M1 = H.channel(nk=NK)
        inp = cases.rk2_inputs((gg, d1, M1), False, False)
        d, M = gg.tile(NK, 4, layout, pe)

        def cut(a):
            rows = np.arange(d.nrows) - d.joff + d.j_glob0
            cols = np.mod(np.arange(d.pitch) - d.ioff + d.i_glob0, d1.ni)
            src_r = np.clip(rows + d1.joff, 0, d1.nrows - 1); src_c = np.clip(cols + d1.ioff, 0, d1.pitch - 1)
            return np.ascontiguousarray(a[..., src_r[:, None], src_c[None, :]])
        dt = inp["dt"]
        cont, bt, cor, pgf, rk2 = cases.rk2_params(d, inp["GV"], dict(strong_drag=1))
        dyc = Dycore(d, M, inp["GV"], 0)
        parallel.attach_comm(dyc, layout, pe, None, unique_id=uid)
        dyc.continuity_init(cont); dyc.barotropic_init(bt); dyc.CoriolisAdv_init(cor); dyc.PressureForce_init(pgf, inp["Rlay"], inp["gp"])
        dyc.initialize_dyn_split_RK2(rk2)
        dyc.vertvisc_set_coef(*[dyc.to_dev(cut(a)) if a is not None else None for a in inp["coefs"][0]])
        sg = dict(u=dyc.to_dev(cut(inp["u"])), v=dyc.to_dev(cut(inp["v"])), h=dyc.to_dev(cut(inp["h"])), uh=dyc.zeros3(), vh=dyc.zeros3(),
                  uhtr=dyc.zeros3(), vhtr=dyc.zeros3(), eta_av=dyc.zeros2())
        txd, tyd = dyc.to_dev(cut(inp["taux"])), dyc.to_dev(cut(inp["tauy"]))
        torch.cuda.synchronize()
        dyc.dyn_split_RK2_new_run(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], dt)
        dyc.comm_exchange_count(reset=True); dyc.comm_exchange_bytes(reset=True)
        dyc.step_MOM_dyn_split_RK2(sg["u"], sg["v"], sg["h"], sg["uh"], sg["vh"], sg["uhtr"], sg["vhtr"], sg["eta_av"], txd, tyd, dt,
                                   calc_dtbt=True)
        dyc.sync()
        out[pe] = (dyc.comm_exchange_count(), dyc.comm_exchange_bytes())
        dyc.close()
    except Exception:                                                 # noqa: BLE001 -- reported by the main thread
        import traceback
        errors.append((pe, traceback.format_exc()))


def step_counts():
    """[[exchanges, bytes] of tile (0, 0), ... of tile (1, 0)] for one step of the 2 x 1 channel, tiles as host threads."""
    from mom6_amd.abi import load_library
    H.use_threads_transport(load_library())
    try:
        layout, pes = (2, 1), [(0, 0), (1, 0)]
        uid = parallel.unique_id(load_library())
        out, errors = {}, []
        threads = [threading.Thread(target=_tile_step_counts, args=(layout, pe, uid, out, errors)) for pe in pes]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not errors, errors[0][1]
        return [list(out[pe]) for pe in pes]
    finally:
        H.use_threads_transport(load_library(), on=False)


# [exchanges, bytes] per tile of the step above, as this test printed them on the commit before the step's widths became arguments
# of the passes (one MI355X, both tiles as host threads; under MOM6X_PASS_WIDTHS=full the same step sends 397056 bytes per tile).
# Integers that follow from the grid, the layer count and the widths alone.
NARROW_COUNTS = [[17, 306304], [17, 306304]]


def test_the_steps_group_passes_stay_narrow():
    """The step sends the reference's own 2-3 rows of its 3-D fields (create_group_pass(..., halo=), RK2.F90:476-495), not
    NIHALO = 4: as many exchanges as with MOM6X_PASS_WIDTHS=full, strictly fewer bytes, and exactly the recorded numbers."""
    narrow = step_counts()
    r = subprocess.run([sys.executable, "-m", "tests.test_step_args_gpu"], env=dict(os.environ, MOM6X_PASS_WIDTHS="full"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    full = json.loads(r.stdout.strip().splitlines()[-1])
    print("step_counts narrow", narrow, "full", full)
    for t in range(2):
        assert narrow[t][0] == full[t][0] and narrow[t][0] > 0, (narrow, full)
        assert narrow[t][1] < full[t][1], (narrow, full)
    assert narrow == NARROW_COUNTS, (narrow, NARROW_COUNTS)


if __name__ == "__main__":
    print(json.dumps(step_counts()))
