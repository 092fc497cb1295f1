"""Time mom6x_make_frazil, mom6x_adjust_salt and mom6x_geothermal_in_place on the headline grid (bench.py's build_model:
1440 x 1080 x 75) with the context's per-launch events (mom6x_prof_*) on an OM4-like state: the rows of the southern and northern
sixth of the grid below freezing throughout, the rest warm; salinity above MIN_SALINITY everywhere; a geothermal flux of 0.05 ..
0.15 W m-2 with GEOTHERMAL_THICKNESS = 0.1 m, which the bottom layer takes.  T is restored before every repetition.  Beside each
call, in the same process, a device copy of the bytes the call must move: one word per cell-layer read for make_frazil (T) and
for adjust_salt (S) in the warm case; for geothermal_in_place the layers heated (h read, T read and written, per column geo_heat,
mask2dT and internal_heat read and written), plus the column of h, the bottom T and S and the plane written when BFlx_geothermal is
asked for.  Registers and occupancy come from mom6_amd/lib/kernel_resources.json.  Prints one JSON line.

    python scripts/dev/time_diabatic_TS.py [--reps 10] [--out profiles/diabatic_TS_kernels.json]
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
    import numpy as np
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    from mom6_amd import build as mbuild
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    dev, GV = dyc.device, dyc.GV
    h = st["h"]
    s = dyc.torch_stream()
    nk = d.nk
    sf = lambda n: synth_dev.smooth_field(d, dev, 700 + n, ox=0.5, oy=0.5)
    mask = keep[4][abi.G["mask2dT"]]
    mask_h = mask.cpu().numpy() if hasattr(mask, "cpu") else np.asarray(mask)
    with torch.cuda.stream(s):
        zf = (torch.arange(nk, dtype=torch.float64, device=dev) / (nk - 1))[:, None, None]
        pT, pS = sf(10)[None], sf(11)[None]
        rows = torch.arange(d.shape2()[0], dtype=torch.float64, device=dev)[None, :, None] - d.joff
        polar = (rows < d.nj / 6.0) | (rows >= d.nj * 5.0 / 6.0)
        T0 = torch.where(polar, -2.4 + 0.2 * pT + 0.0 * zf, 20.0 - 15.0 * zf ** 0.5 + 0.8 * pT * (1.0 - 0.5 * zf)).contiguous()
        T = T0.clone()
        S = (34.5 + 1.0 * zf + 0.2 * pS).contiguous()
        zero2 = lambda: torch.zeros(d.shape2(), dtype=torch.float64, device=dev)
        frazil, deficit, iheat, bflx = zero2(), zero2(), zero2(), zero2()
        geo_d = (0.1 * (1.0 + 0.5 * sf(25))).contiguous()
    dyc.sync()
    geo_heat = mask_h * geo_d.cpu().numpy()
    dyc.make_frazil_init(abi.frazil_params_default())
    dyc.geothermal_init(abi.geothermal_params_default(GV), geo_heat, abi.eos_params_default(abi.WRIGHT))
    calib = bench.box_calibration(dyc.device)
    calls = dict(
        make_frazil=(lambda: dyc.make_frazil(h, T, S, frazil), ("k_frazil_cols",)),
        adjust_salt=(lambda: dyc.adjust_salt(h, S, deficit, 0.01), ("k_salt_cols",)),
        geothermal_in_place=(lambda: dyc.geothermal_in_place(h, T, S, args.dt, internal_heat=iheat), ("k_geo_cols",)),
        geothermal_in_place_BFlx=(lambda: dyc.geothermal_in_place(h, T, S, args.dt, internal_heat=iheat, BFlx_geothermal=bflx),
                                  ("k_geo_cols", "k_geo_fill")))
    cells, cols = nk * d.ni * d.nj, d.ni * d.nj
    must = dict(make_frazil=8 * cells, adjust_salt=8 * cells, geothermal_in_place=8 * 7 * cols,
                geothermal_in_place_BFlx=8 * (7 + nk + 3) * cols)

    def restore():
        with torch.cuda.stream(s):
            T.copy_(T0)

    def copy_ms(nbytes):
        src = torch.ones(max(nbytes // 16, 1), dtype=torch.float64, device=dev)   # a copy moves each byte twice: half the bytes as the source
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(); dst.copy_(src); c1.record(); c1.synchronize()
            t.append(c0.elapsed_time(c1))
        return statistics.median(t)

    torch.cuda.synchronize()
    res_json = json.load(open(os.path.join(os.path.dirname(mbuild.LIB), "kernel_resources.json")))["diabatic_TS.hip"]
    out = {}
    for name, (call, kernels) in calls.items():
        for _ in range(2):
            restore(); call()
        dyc.sync()
        dycore.prof_enable(dyc, True)
        per, seen = [], {}
        for _ in range(a.reps):
            restore()
            dyc.sync()
            dycore.prof_reset(dyc)
            call()
            dyc.sync()
            tot_ms = 0.0
            for k, (cnt, tot) in dycore.prof_report(dyc).items():
                if k.startswith(kernels) and cnt > 0 and tot > 0.0:
                    tot_ms += tot; seen[k] = seen.get(k, 0) + cnt
            per.append(tot_ms)
        dycore.prof_enable(dyc, False)
        if not seen:
            raise SystemExit(f"time_diabatic_TS: the context's per-launch events recorded no launch of {kernels}")
        ms, cms = statistics.median(per), copy_ms(must[name])
        out[name] = dict(kernels=sorted(seen), ms=round(ms, 4),
                         yardstick=dict(GB=round(must[name] / 1e9, 4), copy_ms=round(cms, 4),
                                        ms_at_box_copy_rate=round(must[name] / 1e9 / calib["copy_GBps"] * 1e3, 4),
                                        kernel_over_that_copy=round(ms / cms, 2)))
    dyc.sync()
    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    line = dict(routines=out, grid=[args.ni, args.nj, args.nk], reps=a.reps,
                setting="TFREEZE_FORM = LINEAR, RECLAIM_FRAZIL, no pressure dependence; MIN_SALINITY = 0.01; GEOTHERMAL_THICKNESS = 0.1 m, "
                        "EQN_OF_STATE = WRIGHT for BFlx_geothermal; a third of the rows below freezing",
                what_must_move="make_frazil, adjust_salt: 1 word per cell-layer read (the warm case); geothermal_in_place: 7 words per "
                               "column (one layer heated), with BFlx_geothermal nk + 3 more",
                registers={k: v for k, v in res_json.items()}, box_calibration=calib,
                frazil_columns=int((frazil[own] > 0.0).sum()), outputs_finite=bool(torch.isfinite(T[(slice(None),) + own]).all()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
