"""Time mom6x_set_pen_shortwave on the headline grid (bench.py's build_model: 1440 x 1080 x 75) with the context's per-launch
events (mom6x_prof_*): MANIZZA_05 with three bands and chl_2d (OM4's setting), the same with chl_3d, and DOUBLE_EXP.  Chlorophyll
is smooth, 0.03 .. 3 mg m-3; the shortwave is fluxes%sw alone.  Beside each call, in the same process, a device fill and a
device copy of the bytes the call must move: 8*nbands*nk*columns written, plus 8*nk*columns read with chl_3d (the planes are
nk times smaller and are left out).  Registers and occupancy come from mom6_amd/lib/kernel_resources.json.  Prints one JSON line.

    python scripts/dev/time_set_opacity.py [--reps 10] [--out profiles/set_opacity_kernels.json]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    from mom6_amd import build as mbuild
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    dev, GV = dyc.device, dyc.GV
    s = dyc.torch_stream()
    nk = d.nk
    sf = lambda n: synth_dev.smooth_field(d, dev, 900 + n, ox=0.5, oy=0.5)
    with torch.cuda.stream(s):
        sw = (150.0 * (1.0 + 0.9 * sf(1))).contiguous()
        chl_2d = torch.exp(2.302585092994046 * (-0.5 + 1.0 * sf(2))).contiguous()
        zf = (torch.arange(nk, dtype=torch.float64, device=dev) / (nk - 1))[:, None, None]
        chl_3d = (chl_2d[None] * (1.0 - 0.5 * zf)).contiguous()
        opacity_band = torch.full((3,) + d.shape3(), float("nan"), dtype=torch.float64, device=dev)
        sw_pen_band = torch.full((3,) + d.shape2(), float("nan"), dtype=torch.float64, device=dev)
    dyc.sync()
    calib = bench.box_calibration(dyc.device)
    cells, cols = nk * d.ni * d.nj, d.ni * d.nj
    manizza = abi.opacity_params_default(nbands=3)
    double = abi.opacity_params_default(opacity_scheme=abi.OPACITY_DOUBLE_EXP, nbands=2, pen_sw_scale=15.0, pen_sw_scale_2nd=0.35,
                                        sw_1st_exp_ratio=0.58)
    H_to_Z = GV.H_to_Z
    cases = dict(
        MANIZZA_05_chl_2d=(manizza, lambda: dyc.set_pen_shortwave(opacity_band, sw_pen_band, sw=sw, chl_2d=chl_2d, opacity_scale=H_to_Z),
                           8 * 3 * cells, 0),
        MANIZZA_05_chl_3d=(manizza, lambda: dyc.set_pen_shortwave(opacity_band, sw_pen_band, sw=sw, chl_3d=chl_3d, opacity_scale=H_to_Z),
                           8 * 3 * cells, 8 * cells),
        DOUBLE_EXP=(double, lambda: dyc.set_pen_shortwave(opacity_band, sw_pen_band, sw=sw, opacity_scale=H_to_Z), 8 * 2 * cells, 0))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(); fn(); c1.record(); c1.synchronize()
            t.append(c0.elapsed_time(c1))
        return statistics.median(t)

    def fill_ms(nbytes):
        dst = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        return timed(lambda: dst.fill_(1.0))

    def copy_ms(nbytes):
        src = torch.ones(max(nbytes // 16, 1), dtype=torch.float64, device=dev)   # a copy moves each byte twice: half the bytes as the source
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))

    res_json = json.load(open(os.path.join(os.path.dirname(mbuild.LIB), "kernel_resources.json")))["opacity.hip"]
    out = {}
    for name, (P, call, written, read) in cases.items():
        dyc.opacity_init(P)
        for _ in range(2):
            call()
        dyc.sync()
        dycore.prof_enable(dyc, True)
        per, seen = [], {}
        for _ in range(a.reps):
            dyc.sync()
            dycore.prof_reset(dyc)
            call()
            dyc.sync()
            tot_ms = 0.0
            for k, (cnt, tot) in dycore.prof_report(dyc).items():
                if k.startswith("k_opacity_cols") and cnt > 0 and tot > 0.0:
                    tot_ms += tot; seen[k] = seen.get(k, 0) + cnt
            per.append(tot_ms)
        dycore.prof_enable(dyc, False)
        if not seen:
            raise SystemExit("time_set_opacity: the context's per-launch events recorded no launch of k_opacity_cols")
        assert dyc.opacity_status() == 0
        ms, fms, cms = statistics.median(per), fill_ms(written + read), copy_ms(written + read)
        out[name] = dict(kernels=sorted(seen), launches_per_call=sum(seen.values()) // a.reps, ms=round(ms, 4),
                         GBps=round((written + read) / 1e9 / (ms * 1e-3), 1),
                         yardstick=dict(GB_written=round(written / 1e9, 4), GB_read=round(read / 1e9, 4), fill_ms=round(fms, 4),
                                        copy_ms=round(cms, 4), kernel_over_that_fill=round(ms / fms, 2),
                                        kernel_over_that_copy=round(ms / cms, 2),
                                        ms_at_box_copy_rate=round((written + read) / 1e9 / calib["copy_GBps"] * 1e3, 4)))
    own = (Ellipsis,) + d.sl(0, d.ni - 1, 0, d.nj - 1)
    line = dict(cases=out, grid=[args.ni, args.nj, args.nk], reps=a.reps,
                setting="sw alone, opacity_scale = GV%H_to_Z, no diagnostics; chlorophyll 0.03 .. 3 mg m-3",
                what_must_move="8*nbands*nk*columns written; with chl_3d 8*nk*columns read",
                registers={k: v for k, v in res_json.items()}, box_calibration=calib,
                outputs_finite=bool(torch.isfinite(opacity_band[:2][own]).all() and torch.isfinite(sw_pen_band[:2][own]).all()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
