"""Time the kernels of mom6x_step_forward_MEKE on the headline grid (bench.py's build_model: 1440 x 1080 x 75) with the context's
per-launch events (mom6x_prof_*), in a setting that runs all three column sums (MEKE_ADVECTION_FACTOR = 1) with both diffusions,
and compare k_meke_cols -- the call's only 3-D traffic: h, hu, hv read once each -- with the box's copy rate (bench.box_calibration)
and with a device copy of three 3-D arrays' worth of bytes timed in the same run.  Prints one JSON line.

    python scripts/dev/time_MEKE.py [--reps 20] [--out profiles/meke_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    dev = dyc.device
    GV = dyc.GV
    h = st["h"]
    sf = lambda seed, **kw: synth_dev.smooth_field(d, dev, seed, **kw)                   # noqa: E731
    s = dyc.torch_stream()
    with torch.cuda.stream(s):
        hu = (1.0e10 * sf(600, nk=d.nk, ox=1.0, oy=0.5)).contiguous()
        hv = (1.0e10 * sf(601, nk=d.nk, ox=0.5, oy=1.0)).contiguous()
        SN_u = (4.0e-6 * (1.0 + 0.8 * sf(602, ox=1.0, oy=0.5))).contiguous()
        SN_v = (4.0e-6 * (1.0 + 0.8 * sf(603, ox=0.5, oy=1.0))).contiguous()
        MEKE = (1.0e-2 * (1.0 + 0.9 * sf(608, ox=0.5, oy=0.5))).contiguous()
        Kh = (500.0 * (1.0 + 0.5 * sf(609, ox=0.5, oy=0.5))).contiguous()
        Ku = torch.zeros_like(Kh)
        Rd = (1.2 + 1.1 * sf(610, ox=0.5, oy=0.5)).contiguous()
        GM = (-2.0e-3 * (1.0 + 0.9 * sf(611, ox=0.5, oy=0.5))).contiguous()
    zero = np.zeros(d.shape2())
    P = abi.MEKE_params_default(GV, cold_start=1, MEKE_GMcoeff=1.0, viscosity_coeff_Ku=1.0, aRhines=0.15, aEady=0.15, MEKE_Kh=500.0,
                                MEKE_K4=1.0e12, MEKE_advection_factor=1.0, visc_drag=0)
    dyc.MEKE_init(P, zero, zero)
    calib = bench.box_calibration(dyc.device)

    def call():
        dyc.step_forward_MEKE(MEKE, h, SN_u, SN_v, args.dt, hu=hu, hv=hv, Rd_dx_h=Rd, GM_src=GM, Kh=Kh, Ku=Ku)

    torch.cuda.synchronize()
    for _ in range(3):
        call()
    dyc.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record(s)
    for n in range(a.reps):
        call()
        ev[n + 1].record(s)
    dyc.sync(); ev[-1].synchronize()
    call_ms = statistics.median(ev[n].elapsed_time(ev[n + 1]) for n in range(a.reps))
    dycore.prof_enable(dyc, True)
    per = {}
    for _ in range(a.reps):
        dycore.prof_reset(dyc)
        call()
        dyc.sync()
        for k, (cnt, tot) in dycore.prof_report(dyc).items():
            if k.startswith("k_meke") and cnt > 0 and tot > 0.0:
                per.setdefault(k, []).append(tot / cnt)
    dycore.prof_enable(dyc, False)
    kern = {k: round(statistics.median(v), 4) for k, v in per.items()}
    # the three arrays as the kernel reads them: a copy moves each byte twice, so a copy of 1.5 arrays moves the kernel's bytes
    nbytes = 3 * 8 * d.nk * d.ni * d.nj
    src = torch.ones(nbytes // 16, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(); dst.copy_(src); c1.record(); c1.synchronize()
        t.append(c0.elapsed_time(c1))
    copy_ms = statistics.median(t)
    cols = kern["k_meke_cols"]
    line = dict(routine="mom6x_step_forward_MEKE", grid=[args.ni, args.nj, args.nk], reps=a.reps, call_ms=round(call_ms, 4), kernels_ms=kern,
                k_meke_cols=dict(ms=cols, GB_read=round(nbytes / 1e9, 3), GBps=round(nbytes / 1e9 / (cols / 1e3), 1),
                                 frac_of_box_copy_rate=round(nbytes / 1e9 / (cols / 1e3) / calib["copy_GBps"], 4),
                                 copy_of_the_same_bytes_ms=round(copy_ms, 4), times_that_copy=round(cols / copy_ms, 3)),
                box_calibration=calib, MEKE_finite=bool(torch.isfinite(MEKE[d.sl(0, d.ni - 1, 0, d.nj - 1)]).all()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
