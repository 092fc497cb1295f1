"""Time mom6x_calc_slope_functions on the headline grid (bench.py's build_model: 1440 x 1080 x 75; a stratified T, S; WRIGHT) in
each of its three branches and, in the same run, the round trip a host-side calc_slope_functions needs at the least: h, T, S to
the host and slope_x, slope_y, SN_u, SN_v back.  Prints one JSON line: per branch the call's ms (device events around repeated
calls), the ms of each kernel (the context's own per-launch events, in a pass of its own after the timed one), the bytes each
kernel must move counted from the shapes, and the fraction of this box's measured stream rate (bench.box_calibration's copy) that
this gives; then the round trip's ms.

    python scripts/dev/time_calc_slope_functions.py [--reps 10] [--out profiles/calc_slope_functions_time.json]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# words per cell-layer through HBM, each array counted once per kernel that touches it (the two cells of a face share lines, a
# direction of the face pass re-reads what the other read):
#   k_vm_cols: h three times (e bottom-up, pres top-down, the solve), T, S in; e, pres, T_f, S_f, c1 out; T_f, S_f, c1 back in and
#              T_f, S_f out again for the back-substitution (15); without an EOS h in, e out (2)
#   k_vm_faces, per direction: h, e, pres, T_f, S_f in, the slope out (6), N2 out where it is kept (+1)
#   k_vm_visbeck, per direction: h, its own slope, the other direction's slope, N2 in (4)
#   k_vm_just_e, per direction: h, e in (2)
WORDS = {"k_vm_cols": 15, "k_vm_cols(no EOS)": 2, "k_vm_faces<2,1>": 12, "k_vm_faces<2,2>": 14, "k_vm_visbeck": 8, "k_vm_just_e": 4,
         "k_vm_eady_combine": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    # a stratified T, S on the benchmark's h (the state of the headline tests): 20..5 degC and 34..35 ppt top to bottom plus a smooth field
    dev = dyc.device
    kk = torch.arange(d.nk, dtype=torch.float64, device=dev)[:, None, None] / max(d.nk - 1, 1)
    T = (10.0 + (10.0 - 15.0 * kk) + 0.8 * synth_dev.smooth_field(d, dev, 5, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    S = (34.5 + (kk - 0.5) + 0.2 * synth_dev.smooth_field(d, dev, 105, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    h = st["h"]
    GV = dyc.GV
    Rlay, gp = abi.layer_densities(d.nk, Rho0=GV.Rho0, g_Earth=GV.g_Earth)
    eos = abi.eos_params_default(abi.WRIGHT)
    SN_u, SN_v = dyc.zeros2(), dyc.zeros2()
    slope_x, slope_y = dyc.zeros3(d.nk + 1), dyc.zeros3(d.nk + 1)
    s = dyc.torch_stream()
    cl = d.nk * d.ni * d.nj
    calib = bench.box_calibration(dyc.device)
    branches = {"simpler_Eady": (dict(use_stored_slopes=1, use_simpler_Eady_growth_rate=1), eos),
                "stored_slopes": (dict(use_stored_slopes=1), eos),
                "just_e": (dict(), None)}
    out = {}
    for name, (mods, e) in branches.items():
        dyc.varmix_init(abi.varmix_params_default(GV, **mods), e, Rlay, gp)
        kw = dict(T=T, S=S, slope_x=slope_x, slope_y=slope_y) if e is not None else {}
        torch.cuda.synchronize()
        for _ in range(3):
            dyc.calc_slope_functions(h, args.dt, SN_u, SN_v, **kw)
        dyc.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(a.reps):
            dyc.calc_slope_functions(h, args.dt, SN_u, SN_v, **kw)
        e1.record(s)
        dyc.sync(); e1.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        dycore.prof_enable(dyc, True); dycore.prof_reset(dyc)
        for _ in range(a.reps):
            dyc.calc_slope_functions(h, args.dt, SN_u, SN_v, **kw)
        dyc.sync()
        kern = {}
        for k, (cnt, tot) in dycore.prof_report(dyc).items():
            if not k.startswith("k_vm") or cnt == 0 or tot <= 0.0:   # (the report keeps the names of the branches before at count 0)
                continue
            w = WORDS.get("k_vm_cols(no EOS)" if (k == "k_vm_cols" and e is None) else k)
            kms = tot / max(cnt, 1)
            kern[k] = dict(ms=round(kms, 4), words_per_cell_layer=w, GB=round(8 * w * cl / 1e9, 3) if w is not None else None,
                           frac_of_copy_rate=round(8 * w * cl / 1e9 / (kms / 1e3) / calib["copy_GBps"], 4) if w else None)
        dycore.prof_enable(dyc, False)
        out[name] = dict(ms=round(ms, 4), kernels=kern, SN_finite=bool(torch.isfinite(SN_u[d.sl(0, d.ni - 1, 0, d.nj - 1)]).all()))
    # the host path's least traffic: h, T, S down to pinned host memory; slope_x, slope_y, SN_u, SN_v back up
    down, up = (h, T, S), (slope_x, slope_y, SN_u, SN_v)
    hd = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in down]
    hu = [torch.zeros(x.shape, dtype=x.dtype, pin_memory=True) for x in up]

    def round_trip():
        for hst, x in zip(hd, down):
            hst.copy_(x, non_blocking=True)
        for hst, x in zip(hu, up):
            x.copy_(hst, non_blocking=True)

    round_trip()
    torch.cuda.synchronize()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    round_trip()
    c1.record(); c1.synchronize()
    line = dict(routine="mom6x_calc_slope_functions (WRIGHT)", grid=[args.ni, args.nj, args.nk], reps=a.reps, branches=out,
                box_calibration=calib, round_trip_ms=round(c0.elapsed_time(c1), 3),
                round_trip_GB=round(sum(x.numel() for x in down + up) * 8 / 1e9, 3))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
