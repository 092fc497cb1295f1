"""The life of a context and of the modules' states it owns: an entry called before its module's init is refused with the reference's
message; the setters that may come before their init do; an init repeated on a live context leaves what a fresh context would have;
the RK2 step hands vertvisc its thicknesses under DIRECT_STRESS without leaving them behind for the public vertvisc; and contexts that
are created, filled with every module's arrays and destroyed give their device memory back."""
import numpy as np
import pytest

from mom6_amd import abi, synth
from tests import cases, helpers as H

pytestmark = pytest.mark.gpu
G = abi.G
NK = 8
EINVAL = 1   # MOM6X_EINVAL (include/mom6x.h)


def _cfg():
    return H.benchmark_small(nk=NK)   # 40 x 24 x 8


def _bits(a, b, name):
    """Whole arrays, bit patterns: a NaN an output started with counts as a value like any other."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    n = int((a.view(np.int64) != b.view(np.int64)).sum())
    assert n == 0, f"{name}: {n} of {a.size} words differ"


def _nan3(dyc, nk=None):
    # (the fill on the context's stream, like the zeros before it: on torch's own stream nothing orders the two, and the first
    # work of a fresh context's stream can start late enough for its zeros to land on top of the NaNs)
    import torch
    with torch.cuda.stream(dyc.torch_stream()):
        return dyc.zeros3(nk).fill_(float("nan"))


def _nan2(dyc):
    import torch
    with torch.cuda.stream(dyc.torch_stream()):
        return dyc.zeros2().fill_(float("nan"))


# ---- 1. use before init
# entry -> (the call on a fresh context; z3 / z2: a 3-D array / a plane of zeros, the message mom6x_last_error() holds afterwards).
# The messages are the ones this test printed on the commit before the modules' states left the context.
def _btstep(y, z3, z2):
    y.btstep(z3, z3, z2, 600.0, z3, z3, z2, z2, z3, z2, z3, z3, z3, z3, z2, z2, z2, z3, z3, None)


USE_BEFORE_INIT = {
    "continuity_PPM": (lambda y, z3, z2: y.continuity_PPM(z3, z3, z3, z3, z3, z3, 600.0),
                       "MOM_continuity_PPM: Module must be initialized before it is used."),
    "btcalc": (lambda y, z3, z2: y.btcalc(z3), "btcalc: Module MOM_barotropic must be initialized before it is used."),
    "btstep": (_btstep, "btstep: Module MOM_barotropic must be initialized before it is used."),
    "set_dtbt": (lambda y, z3, z2: y.set_dtbt(z3), "set_dtbt: Module MOM_barotropic must be initialized before it is used."),
    "CorAdCalc": (lambda y, z3, z2: y.CorAdCalc(z3, z3, z3, z3, z3, z3, z3),
                  "MOM_CoriolisAdv: Module must be initialized before it is used."),
    "PressureForce": (lambda y, z3, z2: y.PressureForce(z3, z3, z3, z3, z2),
                      "MOM_PressureForce_FV_Bouss: Module must be initialized before it is used."),
    "vertvisc_coef": (lambda y, z3, z2: y.vertvisc_coef(z3, z3, z3, 600.0),
                      "MOM_vert_friction(coef): Module must be initialized before it is used."),
    "horizontal_viscosity": (lambda y, z3, z2: y.horizontal_viscosity(z3, z3, z3, z3, z3),
                             "MOM_hor_visc: Module must be initialized before it is used."),
    "set_viscous_BBL": (lambda y, z3, z2: y.set_viscous_BBL(z3, z3, z3, bbl_thick_u=z2, bbl_thick_v=z2),
                        "MOM_set_viscosity(BBL): Module must be initialized before it is used."),
    "thickness_diffuse": (lambda y, z3, z2: y.thickness_diffuse(z3, z3, z3, 600.0),
                          "MOM_thickness_diffuse: Module must be initialized before it is used."),
    "tracer_hordiff": (lambda y, z3, z2: y.tracer_hordiff(z3, 600.0, [z3]),
                       "MOM_tracer_hor_diff: tracer_hor_diff_init must be called before tracer_hordiff."),
    "calc_slope_functions": (lambda y, z3, z2: y.calc_slope_functions(z3, 600.0, z2, z2),
                             "MOM_lateral_mixing_coeffs.F90, calc_slope_functions: Module must be initialized before it is used."),
    "mixedlayer_restrat": (lambda y, z3, z2: y.mixedlayer_restrat(z3, z3, z3, z3, z3, z2, 600.0),
                           "mixedlayer_restrat: Module must be initialized before it is used."),
    "advect_tracer": (lambda y, z3, z2: y.advect_tracer(z3, z3, z3, 600.0, [z3]),
                      "MOM_tracer_advect: tracer_advect_init must be called before advect_tracer."),
    "write_energy": (lambda y, z3, z2: y.write_energy(z3, z3, z3), "write_energy: Module must be initialized before it is used."),
    "step_dyn_split_RK2": (lambda y, z3, z2: y.step_MOM_dyn_split_RK2(z3, z3, z3, z3, z3, z3, z3, z2, z2, z2, 600.0),
                           "step_MOM_dyn_split_RK2: initialize_dyn_split_RK2 must be called first"),
}


@pytest.mark.parametrize("entry", list(USE_BEFORE_INIT))
def test_use_before_init_is_refused_with_the_references_message(entry):
    from mom6_amd.dycore import Dycore
    gg, d, M = _cfg()
    call, text = USE_BEFORE_INIT[entry]
    dyc = Dycore(d, M, abi.vgrid_default())
    try:
        with pytest.raises(abi.Mom6xError) as e:
            call(dyc, dyc.zeros3(), dyc.zeros2())
        print(entry, "->", str(e.value))
        assert str(e.value) == f"mom6x error {EINVAL}: {text}"
        assert dyc.lib.mom6x_last_error().decode() == text
        dyc.sync()
    finally:
        dyc.close()


# ---- 2. setters before init
HMIX = 900.0   # HMIX_STRESS: the wind stress goes into the topmost 900 m, several layers of the 4000 m bowl


def _pgf_and_vertvisc(setters_first):
    """PressureForce with a linear EOS and vertvisc_coef + vertvisc under DIRECT_STRESS; the setters before or after the inits."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests.test_dyn_gpu import visc_inputs
    gg, d, M = _cfg()
    GV = abi.vgrid_default()
    Rlay, gp = abi.layer_densities(d.nk)
    h, u, v = synth.make_state(d, M)
    T, S = cases.thermo_state(d, M)
    taux = np.ascontiguousarray(0.1 * synth.smooth_field(d, 41, ox=1.0, oy=0.5) * M[G["mask2dCu"]])
    tauy = np.ascontiguousarray(0.05 * synth.smooth_field(d, 42, ox=0.5, oy=1.0) * M[G["mask2dCv"]])
    dyc = Dycore(d, M, GV)
    try:
        hd, Td, Sd = dyc.to_dev(h), dyc.to_dev(T), dyc.to_dev(S)
        vis = [dyc.to_dev(a) if a is not None else None for a in visc_inputs(d, M)]

        def setters():
            dyc.PressureForce_set_tv(Td, Sd, abi.eos_params_default(abi.LINEAR))
            dyc.vertvisc_set_visc(*vis)
            dyc.vertvisc_set_direct_stress(HMIX, hd)

        def inits():
            dyc.PressureForce_init(abi.pgf_params_default(GV.Rho0), Rlay, gp)
            dyc.vertvisc_init(abi.vertvisc_params_default())

        for f in ((setters, inits) if setters_first else (inits, setters)):
            f()
        o = dict(PFu=_nan3(dyc), PFv=_nan3(dyc), pbce=_nan3(dyc), eta=_nan2(dyc), u=dyc.to_dev(u), v=dyc.to_dev(v),
                 taux_bot=_nan2(dyc), tauy_bot=_nan2(dyc))
        tx, ty = dyc.to_dev(taux), dyc.to_dev(tauy)
        torch.cuda.synchronize()
        dyc.PressureForce(hd, o["PFu"], o["PFv"], o["pbce"], o["eta"])
        dyc.vertvisc_coef(o["u"], o["v"], hd, 600.0)
        dyc.vertvisc(o["u"], o["v"], tx, ty, 600.0, o["taux_bot"], o["tauy_bot"])
        dyc.sync()
        o["a_u"] = dyc.vertvisc_field("a_u")
        return {n: a.cpu().numpy() for n, a in o.items()}, u
    finally:
        dyc.close()


def test_setters_may_come_before_their_inits():
    want, u0 = _pgf_and_vertvisc(False)
    got, _ = _pgf_and_vertvisc(True)
    for n in want:
        _bits(got[n], want[n], n)
    sl = (Ellipsis,) + tuple(H.interior(_cfg()[1], "u"))
    assert np.isfinite(want["PFu"][sl]).all() and np.abs(want["PFu"][sl]).max() > 0
    assert np.isfinite(want["u"][sl]).all() and not np.array_equal(want["u"][sl], u0[sl])


# ---- 3. re-initialisation
def _fresh(d, M, GV):
    from mom6_amd.dycore import Dycore
    return Dycore(d, M, GV)


def _twice(device, first, last):
    """`device(dy=...)` runs an init and a call in the context it is given: `first` then `last` in one context against `last` in
    a fresh one, whole arrays bit for bit."""
    gg, d, M = _cfg()
    GV = abi.vgrid_default()
    dy = _fresh(d, M, GV)
    try:
        device(d, M, GV, dy, *first)
        got = device(d, M, GV, dy, *last)
    finally:
        dy.close()
    dy = _fresh(d, M, GV)
    try:
        want = device(d, M, GV, dy, *last)
    finally:
        dy.close()
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], n)
    return want


def test_reinit_thickness_diffuse_regrows_its_work_arrays():
    """Without an equation of state (3 work arrays), then with the Wright one (7)."""
    from tests import thickdiff_ref as R
    from tests.test_thickness_diffuse_gpu import _device

    def device(d, M, GV, dy, name):
        P, eos, ps, stored, gm, dt, opts = R.case(name, form=abi.WRIGHT)
        return _device(d, M, GV, P, R.inputs(d, M, GV, **opts), dt, eos=eos, give_ps=ps, stored=stored, give_gm=gm, dy=dy)
    want = _twice(device, ("noeos",), ("gm",))
    assert np.isfinite(want["h"]).all() and np.isnan(want["uhGM"]).any() and np.isfinite(want["uhGM"]).any()


def test_reinit_tracer_hor_diff():
    from tests import hordiff_ref as R
    from tests.test_tracer_hor_diff_gpu import _call

    def device(d, M, GV, dy, name):
        inp = R.inputs(d, M, GV, ntr=2)
        P, dt, uf, give_df, give_out = R.case(name, d, M, inp["planes"])
        out, n = _call(dy, d, P, inp, dt, uf=uf, give_df=give_df, give_out=give_out)
        flat = {f"tracer{m}": t for m, t in enumerate(out["tracers"])}
        flat.update({f"{k}{m}": a for k in ("df_x", "df_y") for m, a in enumerate(out[k] or []) if a is not None})
        flat.update({k: out[k] for k in ("khdt_x", "khdt_y", "CFL") if out[k] is not None})
        flat["num_itts"] = np.array([float(n)])
        return flat
    want = _twice(device, ("const",), ("check3",))
    assert want["num_itts"][0] > 1 and "khdt_x" in want and "df_x0" in want


def test_reinit_varmix():
    from tests import varmix_ref as R
    from tests.test_varmix_gpu import _device

    def device(d, M, GV, dy, name):
        P, eos, ps, dg, dt, opts = R.case(name, GV, form=abi.WRIGHT, nk=d.nk)
        return _device(d, M, GV, P, R.inputs(d, M, GV, **opts), dt, eos=eos, give_ps=ps, give_diag=dg, dy=dy)
    want = _twice(device, ("just_e",), ("visbeck_diag",))     # (work arrays of nk + 1, then of 7 nk + 3 planes)
    assert np.isfinite(want["SN_u"]).any()


def test_reinit_mixedlayer_restrat():
    from tests import mle_ref as R
    from tests.test_mixed_layer_restrat_gpu import _device

    def device(d, M, GV, dy, name):
        P, given, dg, dt = R.case(name, GV)
        return _device(d, M, GV, P, R.inputs(d, M, GV), dt, abi.eos_params_default(abi.WRIGHT), given, dg, dy=dy)
    want = _twice(device, ("detect",), ("both_filters",))
    assert np.isfinite(want["h"]).all()


def _continuity(dyc, cont, inp):
    import torch
    o = dict(h=_nan3(dyc), uh=_nan3(dyc), vh=_nan3(dyc))
    T = {k: dyc.to_dev(inp[k]) for k in ("u", "v", "h", "vr_u", "vr_v")}
    dyc.continuity_init(cont)
    torch.cuda.synchronize()
    dyc.continuity_PPM(T["u"], T["v"], T["h"], o["h"], o["uh"], o["vh"], inp["dt"], visc_rem_u=T["vr_u"], visc_rem_v=T["vr_v"])
    dyc.sync()
    return {k: a.cpu().numpy() for k, a in o.items()}


def test_reinit_continuity_ppm_then_upwind():
    cfg = _cfg()
    gg, d, M = cfg
    inp = cases.continuity_inputs(cfg)
    ppm = abi.continuity_params_default(d.nk, inp["GV"].Angstrom_H)
    upwind = abi.continuity_params_default(d.nk, inp["GV"].Angstrom_H)
    upwind.upwind_1st = 1
    dyc = _fresh(d, M, inp["GV"])
    try:
        first = _continuity(dyc, ppm, inp)
        got = _continuity(dyc, upwind, inp)
    finally:
        dyc.close()
    dyc = _fresh(d, M, inp["GV"])
    try:
        want = _continuity(dyc, upwind, inp)
    finally:
        dyc.close()
    for n in want:
        _bits(got[n], want[n], n)
    sl = (Ellipsis,) + tuple(H.interior(d, "u"))
    assert np.isfinite(want["uh"][sl]).all() and not np.array_equal(first["uh"][sl], want["uh"][sl])   # (the scheme matters)


def test_reinit_barotropic_keeps_its_state():
    """barotropic_init again on a live context, with other parameters and then with the first ones: btcalc, bt_mass_source, btstep
    and continuity_PPM through the public entries give what they give in a context initialised once, and so do the static fields."""
    from tests.test_step_args_gpu import _public_calls, _public_inputs, _step_context
    cfg = _cfg()
    gg, d, M = cfg
    inp = cases.rk2_inputs(cfg, False, False)
    I = _public_inputs(cfg, inp)
    STATIC = ("IDatu", "IDatv", "q_D", "D_u_Cor", "D_v_Cor", "ubtav", "vbtav")

    def calls(dyc):
        out = _public_calls(dyc, I, inp["dt"], 30.0)
        out.update({n: dyc.barotropic_field(n).cpu().numpy() for n in STATIC})
        return out
    cont, bt, cor, pgf, rk2 = cases.rk2_params(d, inp["GV"], dict(strong_drag=1))
    other = cases.rk2_params(d, inp["GV"], dict(strong_drag=0, bebt=0.3, BT_Coriolis_scale=0.5))[1]
    dyc = _step_context(cfg, inp)
    try:
        dyc.barotropic_init(other)
        mid = calls(dyc)
        dyc.barotropic_init(bt)
        got = calls(dyc)
    finally:
        dyc.close()
    dyc = _step_context(cfg, inp)
    try:
        want = calls(dyc)
    finally:
        dyc.close()
    assert set(got) == set(want)
    for n in want:
        _bits(got[n], want[n], n)
    sl = (Ellipsis,) + tuple(H.interior(d, "h"))
    assert np.isfinite(want["eta_out"][sl]).all() and not np.array_equal(mid["eta_out"][sl], want["eta_out"][sl])   # (the parameters matter)


# ---- 4. DIRECT_STRESS through a step
def test_direct_stress_through_a_step_and_a_public_vertvisc_after_it(orc):
    """Two steps of the case with DIRECT_STRESS (HMIX_STRESS = 20 m) and vertvisc_coef on the device, the eight prognostic arrays
    bit for bit the oracle's (tests/test_rk2_gpu.run asserts that); then vertvisc through its public entry in the context that has
    stepped and in one that has not: the same bits -- the step's thicknesses are an argument of its own calls."""
    import torch
    from mom6_amd.dycore import Dycore
    from tests.test_rk2_gpu import run
    from tests.test_dyn_gpu import visc_inputs
    c = H.island_basin()
    gg, d, M = c
    inp = cases.rk2_inputs(c, False, False)
    P = abi.hor_visc_params_default(1200.0)
    P.Smagorinsky_Ah = 1; P.Smag_bi_const = 0.03
    P.dt = inp["dt"]
    h2 = np.ascontiguousarray(inp["h"] * (1.0 + 0.05 * synth.smooth_field(d, 77, nk=d.nk, ox=0.5, oy=0.5)))   # the host's own DIRECT_STRESS thicknesses
    dt = 600.0

    def public(dyc, out):
        a = dict(u=dyc.to_dev(inp["u"]), v=dyc.to_dev(inp["v"]), tbu=_nan2(dyc), tbv=_nan2(dyc))
        tx, ty, hd = dyc.to_dev(inp["taux"]), dyc.to_dev(inp["tauy"]), dyc.to_dev(h2)
        dyc.vertvisc_set_direct_stress(20.0, hd)
        torch.cuda.synchronize()
        dyc.vertvisc_coef(a["u"], a["v"], hd, dt)
        dyc.vertvisc(a["u"], a["v"], tx, ty, dt, a["tbu"], a["tbv"])
        dyc.sync()
        out.update({n: t.cpu().numpy() for n, t in a.items()})

    got = {}
    run(orc, c, nsteps=2, bt_mod=dict(strong_drag=1, bebt=0.2), rk2_mod=dict(be=0.7), cor_mod=dict(Coriolis_En_Dis=1, bound_Coriolis=1),
        eos_form=abi.LINEAR, dev_vv=dict(Kvml_invZ2=0.01), hv=P, Hmix_stress=20.0,
        hook=lambda dyc, when: public(dyc, got) if when == "after" else None)
    want = {}
    vv = abi.vertvisc_params_default()
    vv.Kvml_invZ2 = 0.01
    dyc = Dycore(d, M, inp["GV"])
    try:
        dyc.vertvisc_init(vv)
        dyc.vertvisc_set_visc(*[dyc.to_dev(a) if a is not None else None
                                for a in list(visc_inputs(d, M)) + [inp["coefs"][0][4], inp["coefs"][0][5]]])
        public(dyc, want)
    finally:
        dyc.close()
    assert set(got) == set(want) == {"u", "v", "tbu", "tbv"}
    for n in want:
        _bits(got[n], want[n], n)
    sl = (Ellipsis,) + tuple(H.interior(d, "u"))
    assert np.isfinite(want["u"][sl]).all() and not np.array_equal(want["u"][sl], inp["u"][sl])


# ---- 5. create and destroy
def _fill_and_close(d, M, GV, st):
    """A context with every module's arrays allocated, closed again."""
    import torch
    from mom6_amd.dycore import Dycore
    dyc = Dycore(d, M, GV)
    eos = abi.eos_params_default(abi.WRIGHT)
    Rlay, gp = abi.layer_densities(d.nk)
    cont, bt, cor, pgf, rk2 = cases.rk2_params(d, GV)
    dyc.continuity_init(cont); dyc.barotropic_init(bt); dyc.CoriolisAdv_init(cor); dyc.PressureForce_init(pgf, Rlay, gp)
    dyc.initialize_dyn_split_RK2(rk2)
    dyc.vertvisc_init(abi.vertvisc_params_default())
    dyc.hor_visc_init(abi.hor_visc_params_default(900.0))
    dyc.set_visc_init(abi.set_visc_params_default(), eos)
    dyc.thickness_diffuse_init(abi.thickness_diffuse_params_default(), eos)
    dyc.tracer_hor_diff_init(abi.tracer_hor_diff_params_default(KHTR=1000.0))
    dyc.varmix_init(abi.varmix_params_default(GV, use_stored_slopes=1, calculate_Eady_growth_rate=1), eos, Rlay, gp)
    dyc.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV), eos)
    dyc.tracer_advect_init(900.0, 2)
    dyc.sum_output_init(abi.sum_output_params_default(900.0), gp)
    t = {n: dyc.to_dev(a) for n, a in st.items()}
    hn, dz = dyc.zeros3(), dyc.zeros3(d.nk + 1)
    torch.cuda.synchronize()
    CS = abi.remapping_params_default(abi.REMAP_PPM_H4, GV.H_subroundoff, om4_remap_via_sub_cells=1)
    dyc.ALE_remap_velocities(CS, t["hu_o"], t["hv_o"], t["hu_n"], t["hv_n"], t["u"], t["v"], conserve_ke=True)   # (allocates the source column)
    dyc.ALE_regrid_rho(abi.regrid_rho_params_default(), eos, st_target(d), t["h"], t["T"], t["S"], hn, dz)       # (allocates the host vectors' copy)
    dyc.sync()
    dyc.close()


def st_target(d):
    return np.linspace(1020.0, 1040.0, d.nk + 1)


def test_create_and_destroy_give_the_memory_back():
    """Twenty contexts on the grid of scripts/leak_check.py, each with every init call and the two lazily allocating ALE entries.
    Device memory in use after the fourth and after the twentieth differs by less than half of what one 3-D array lost per cycle
    would add (16 cycles x nk x slab x 8 bytes / 2): a condition, not a measurement."""
    import torch
    gg, d, M = H.channel(nk=20, ni=256, nj=128)
    GV = abi.vgrid_default()
    h, u, v = synth.make_state(d, M)
    T, S = cases.thermo_state(d, M)
    tot = h.sum(0)
    w = np.linspace(1.0, 3.0, d.nk)[:, None, None] * np.ones_like(h)
    st = dict(h=h, u=u, v=v, T=T, S=S, hu_o=h, hv_o=h, hu_n=np.ascontiguousarray(w / w.sum(0) * tot), hv_n=np.ascontiguousarray(w / w.sum(0) * tot))

    def used():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info()
        return total - free
    base = None
    for it in range(20):
        _fill_and_close(d, M, GV, st)
        if it == 3:
            base = used()
    growth = used() - base
    bound = 16 * d.nk * d.slab * 8 // 2
    print(f"device memory in use after 4 cycles {base} B, growth over the next 16: {growth} B (bound {bound} B)")
    assert growth < bound
