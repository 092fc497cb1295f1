"""Time mom6x_mixedlayer_restrat on the headline grid (bench.py's build_model: 1440 x 1080 x 75; a stratified T, S with fronts;
WRIGHT) in two settings -- the boundary-layer scheme's MLD with both running means and a frontal length (OM4's), and detect_mld --
and, in the same run, (a) a device copy of the call's algorithmic bytes on this box and (b) the round trip a host-side
mixedlayer_restrat needs at the least: h, uhtr, vhtr, T, S to the host and h, uhtr, vhtr back (the host's own compute counted as
zero).  Prints one JSON line: per setting the median ms of `--reps` calls (a pair of device events around each), the median ms of
each kernel (the context's own per-launch events, in passes of their own after the timed ones), the bytes each kernel moves
counted from the shapes, and how the call compares with (a) and (b).

    python scripts/dev/time_mixedlayer_restrat.py [--reps 20] [--out profiles/mixedlayer_restrat_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# words per cell-layer through HBM, each array counted once per kernel that touches it, over the whole column (the walks of
# k_mle_cols and the limiter walks of k_mle_faces stop at the base of the mixed layer and move less than this):
#   k_mle_cols: h, T, S in (3); with detect_mld the same three once more over the whole column (6)
#   k_mle_faces, per direction: h in, uhtr in and out, uhml out (4)
#   k_mle_cells: h in and out, uhml, vhml in (4)
WORDS = {"k_mle_cols": 3, "k_mle_cols(detect)": 6, "k_mle_faces": 8, "k_mle_cells": 4}
# what any implementation of the call must move: h, uhtr, vhtr in and out (6); T, S only down to the mixed-layer base (not counted)
ALGORITHMIC_WORDS = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    dev = dyc.device
    kk = torch.arange(d.nk, dtype=torch.float64, device=dev)[:, None, None] / max(d.nk - 1, 1)
    T = (10.0 + (10.0 - 15.0 * kk) + 0.8 * synth_dev.smooth_field(d, dev, 5, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    S = (34.5 + (kk - 0.5) + 0.2 * synth_dev.smooth_field(d, dev, 105, nk=d.nk, ox=0.5, oy=0.5)).contiguous()
    T[: d.nk // 8] += 2.0 * synth_dev.smooth_field(d, dev, 505, ox=0.5, oy=0.5)           # fronts in the upper ocean
    h0 = st["h"]
    GV = dyc.GV
    eos = abi.eos_params_default(abi.WRIGHT)
    sf = lambda seed: synth_dev.smooth_field(d, dev, seed, ox=0.5, oy=0.5)              # noqa: E731  (a 2-D plane)
    ustar = (0.012 * (1.0 + 0.8 * sf(501))).abs().contiguous()
    h_MLD = (90.0 + 70.0 * sf(502)).contiguous()                                         # 20 .. 160 m
    Rd = (1.2 + 1.1 * sf(503)).contiguous()
    s = dyc.torch_stream()
    cl = d.nk * d.ni * d.nj
    calib = bench.box_calibration(dyc.device)
    OM4 = dict(MLE_use_PBL_MLD=1, MLE_density_diff=0.0, ml_restrat_coef=1.0, ml_restrat_coef2=0.5, front_length=500.0,
               MLE_MLD_decay_time=345600.0, MLE_MLD_decay_time2=2.592e6)
    settings = {"pbl_mld_two_filters_front_length": (OM4, dict(h_MLD=h_MLD, Rd_dx_h=Rd)),
                "detect_mld": (dict(ml_restrat_coef=0.0625), {})}
    out = {}
    for name, (mods, planes) in settings.items():
        dyc.mixedlayer_restrat_init(abi.mixedlayer_restrat_params_default(GV, **mods), eos)
        with torch.cuda.stream(s):
            h, uhtr, vhtr = h0.clone(), torch.zeros_like(h0), torch.zeros_like(h0)
            F1, F2 = (0.8 * h_MLD).contiguous(), (1.5 * h_MLD).contiguous()
        kw = dict(planes, MLD_filtered=F1, MLD_filtered_slow=F2)

        def call():
            dyc.mixedlayer_restrat(h, uhtr, vhtr, T, S, ustar, args.dt, **kw)

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
        ms = statistics.median(ev[n].elapsed_time(ev[n + 1]) for n in range(a.reps))
        dycore.prof_enable(dyc, True)
        per = {}
        for _ in range(a.reps):
            dycore.prof_reset(dyc)
            call()
            dyc.sync()
            for k, (cnt, tot) in dycore.prof_report(dyc).items():
                if k.startswith("k_mle") and cnt > 0 and tot > 0.0:
                    per.setdefault(k, []).append(tot / cnt)
        dycore.prof_enable(dyc, False)
        kern = {}
        for k, v in per.items():
            base = k.split("<")[0]
            w = WORDS["k_mle_cols(detect)" if (base == "k_mle_cols" and "detect" in name) else base]
            kms = statistics.median(v)
            kern[k] = dict(ms=round(kms, 4), words_per_cell_layer=w, GB=round(8 * w * cl / 1e9, 3),
                           frac_of_copy_rate=round(8 * w * cl / 1e9 / (kms / 1e3) / calib["copy_GBps"], 4))
        out[name] = dict(ms=round(ms, 4), kernels=kern, moved_GB=round(8 * sum(v["words_per_cell_layer"] for v in kern.values()) * cl / 1e9, 3),
                         h_finite=bool(torch.isfinite(h[(slice(None),) + d.sl(0, d.ni - 1, 0, d.nj - 1)]).all()),
                         h_changed=bool((h != h0).any()))
    # (a) a device copy of the algorithmic bytes: 3 arrays in, 3 arrays out is a copy of three 3-D arrays
    src = torch.ones((ALGORITHMIC_WORDS // 2,) + tuple(h0.shape), dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(); dst.copy_(src); c1.record(); c1.synchronize()
        t.append(c0.elapsed_time(c1))
    copy_ms = statistics.median(t)
    del src, dst
    # (b) the host path's least traffic: h, uhtr, vhtr, T, S down to pinned host memory; h, uhtr, vhtr back up
    z = torch.zeros_like(h0)
    down, up = (h0, z, z, T, S), (h0, z, z)
    hd = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in down]
    hu = [torch.zeros(x.shape, dtype=x.dtype, pin_memory=True) for x in up]
    tgt = [torch.empty_like(h0) for _ in up]

    def round_trip():
        for hst, x in zip(hd, down):
            hst.copy_(x, non_blocking=True)
        for hst, x in zip(hu, tgt):
            x.copy_(hst, non_blocking=True)

    round_trip()
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(); round_trip(); c1.record(); c1.synchronize()
        t.append(c0.elapsed_time(c1))
    rt_ms = statistics.median(t)
    for v in out.values():
        v["times_the_copy"] = round(v["ms"] / copy_ms, 3)
        v["round_trip_over_call"] = round(rt_ms / v["ms"], 2)
    line = dict(routine="mom6x_mixedlayer_restrat (WRIGHT)", grid=[args.ni, args.nj, args.nk], reps=a.reps, settings=out,
                box_calibration=calib, algorithmic_GB=round(8 * ALGORITHMIC_WORDS * h0.numel() / 1e9, 3),
                copy_of_algorithmic_bytes_ms=round(copy_ms, 4), round_trip_ms=round(rt_ms, 3),
                round_trip_GB=round(sum(x.numel() for x in down + up) * 8 / 1e9, 3),
                faster_than_the_round_trip=all(v["ms"] < rt_ms for v in out.values()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
