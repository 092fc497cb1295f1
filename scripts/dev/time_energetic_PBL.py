"""Time mom6x_energetic_PBL on the headline grid (bench.py's build_model: 1440 x 1080 x 75) with the context's per-launch events
(mom6x_prof_*) on an OM4-like case: EPBL_MSTAR_SCHEME = OM4, the default TKE_DECAY = 2.5, the mixed-layer-depth iteration with its
defaults, Kd_int, ML_depth and OBL_its as outputs.  Beside it, in the same run, a device copy of the bytes ONE pass over the inputs
and outputs must move (h, T, S, dSV_dT, dSV_dS, TKE_forced read; Kd_int written).  The kernel walks the column once per iteration
of the mixed-layer depth, and a wavefront leaves the iteration with its slowest lane, so the ratio to that copy is above 1; the
distribution of OBL_its says by how much.  Registers and occupancy come from mom6_amd/lib/kernel_resources.json.  Prints one JSON
line.

    python scripts/dev/time_energetic_PBL.py [--reps 10] [--out profiles/ePBL_kernels.json]
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
    ap.add_argument("--diag", action="store_true", help="TKE_diagnostics with the seven diag_TKE_* planes: k_epbl_cols<., true, false> and k_epbl_diag_out")
    a = ap.parse_args()
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
    sf = lambda n: synth_dev.smooth_field(d, dev, 900 + n, ox=0.5, oy=0.5)
    with torch.cuda.stream(s):
        zf = (torch.arange(nk, dtype=torch.float64, device=dev) / (nk - 1))[:, None, None]
        pT, pS = sf(10)[None], sf(11)[None]
        T = (20.0 - 15.0 * zf ** 0.5 + 0.8 * pT * (1.0 - 0.5 * zf)).contiguous()
        S = (34.5 + 1.0 * zf + 0.2 * pS).contiguous()
        aT = ((2.0e-4 / 1035.0) * (1.0 + 0.3 * pT) * (1.0 - 0.3 * zf)).contiguous()
        aS = (-(7.6e-4 / 1035.0) * (1.0 + 0.1 * pS) * (1.0 + 0.0 * zf)).contiguous()
        TKE = (-0.02 * torch.exp(-8.0 * zf) * (1.0 + 0.5 * pT)).contiguous()
        TKE[0] = 0.5 * sf(40)
        ustar = (0.011 + 0.009 * sf(50)).contiguous()
        bflux = (2.0e-7 * sf(51)).contiguous()
        nan3 = lambda lev: torch.full(d.shape3(lev), float("nan"), dtype=torch.float64, device=dev)
        nan2 = lambda: torch.full(d.shape2(), float("nan"), dtype=torch.float64, device=dev)
        Kd, MLD, its = nan3(nk + 1), nan2(), nan2()
        dg = {n: nan2() for n in dyc.ENERGETIC_PBL_OUT if n.startswith("diag_TKE_")} if a.diag else {}
    P = abi.energetic_PBL_params_default(GV, mstar_scheme=abi.EPBL_MSTAR_OM4, C_Ek=0.17, mstar_cap=10.0, TKE_diagnostics=int(a.diag))
    dyc.energetic_PBL_init(P)
    calib = bench.box_calibration(dyc.device)

    def call():
        dyc.energetic_PBL(h, T, S, aT, aS, TKE, ustar, bflux, args.dt, Kd, MLD, OBL_its=its, **dg)

    torch.cuda.synchronize()
    for _ in range(2):
        call()
    dyc.sync()
    dycore.prof_enable(dyc, True)
    per, per_out, name = [], [], None
    for _ in range(a.reps):
        dycore.prof_reset(dyc)
        call()
        dyc.sync()
        for k, (cnt, tot) in dycore.prof_report(dyc).items():
            if k.startswith("k_epbl_cols") and cnt > 0 and tot > 0.0:
                per.append(tot / cnt); name = k
            if k.startswith("k_epbl_diag_out") and cnt > 0 and tot > 0.0:
                per_out.append(tot / cnt)
    dycore.prof_enable(dyc, False)
    if name is None:
        raise SystemExit("time_energetic_PBL: the context's per-launch events recorded no k_epbl_cols launch")
    ms = statistics.median(per)
    A = 8 * nk * d.ni * d.nj
    must = 6 * A + 8 * (nk + 1) * d.ni * d.nj

    src = torch.ones(max(must // 16, 1), dtype=torch.float64, device=dev)   # a copy moves each byte twice: half the bytes as the source
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t = []
    for _ in range(a.reps):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(); dst.copy_(src); c1.record(); c1.synchronize()
        t.append(c0.elapsed_time(c1))
    copy_ms = statistics.median(t)

    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    wet = keep[4][abi.G["mask2dT"]][own] > 0.0
    n_its = its[own][wet].to(torch.int64)
    hist = torch.bincount(n_its, minlength=P.max_MLD_its + 1).tolist()
    # what a wavefront pays: the largest count among the 64 lanes of each row segment
    it2 = its[own].clone(); it2[~wet] = 0.0
    pad = (-it2.shape[1]) % 64
    wave = torch.nn.functional.pad(it2, (0, pad)).reshape(it2.shape[0], -1, 64).max(dim=2).values
    r = json.load(open(os.path.join(os.path.dirname(mbuild.LIB), "kernel_resources.json")))["energetic_PBL.hip"]
    res = next(v for k, v in r.items() if ("k_epbl_colsILb1ELb1ELb0E" if a.diag else "k_epbl_colsILb1ELb0ELb0E") in k)
    line = dict(routine="mom6x_energetic_PBL", grid=[args.ni, args.nj, args.nk], reps=a.reps, kernel=name,
                setting="EPBL_MSTAR_SCHEME = OM4, TKE_DECAY = 2.5, USE_MLD_ITERATION with the defaults, orig_PE_calc, CUBE_ROOT_TKE; Kd_int, ML_depth, OBL_its" + (", TKE_diagnostics with the seven diag_TKE_* planes" if a.diag else ""),
                ms=round(ms, 3), k_epbl_diag_out_ms=round(statistics.median(per_out), 4) if per_out else None,
                yardstick=dict(what="a device copy of the bytes one pass must move: h, T, S, dSV_dT, dSV_dS, TKE_forced read; Kd_int written",
                               GB=round(must / 1e9, 3), copy_ms=round(copy_ms, 4), ms_at_box_copy_rate=round(must / 1e9 / calib["copy_GBps"] * 1e3, 4),
                               kernel_over_that_copy=round(ms / copy_ms, 2)),
                OBL_its=dict(histogram=hist, mean=round(float(n_its.double().mean()), 3), mean_of_wavefront_max=round(float(wave.mean()), 3)),
                registers=res, box_calibration=calib,
                outputs_finite=bool(torch.isfinite(Kd[(slice(None),) + own]).all() and torch.isfinite(MLD[own]).all()),
                Kd_max=float(Kd[(slice(None),) + own].max()), MLD_mean=float(MLD[own][wet].mean()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
