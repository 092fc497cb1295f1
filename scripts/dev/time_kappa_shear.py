"""Time mom6x_Calculate_kappa_shear on the headline grid (bench.py's build_model: 1440 x 1080 x 75) with the context's per-launch
events (mom6x_prof_*): the `shear` setting of tests/kappa_shear_ref.py (layers of about 10 m, a tanh shear layer across the middle
of the column in a band of 45 % of the rows whose bulk Ri is 0.1 to 0.3, WRIGHT, zero_mix, kappa_0 = 1.5e-5) and a quiescent one
(the same with a fortieth of the velocities: no interface below Ri_crit).  Beside each call, in the same process, a device copy of
the bytes the call must move: u, v, h, T, S of nk levels read and kappa_io, tke_io, kv_io of nk + 1 levels written.  Registers and
occupancy come from mom6_amd/lib/kernel_resources.json; the workspace bytes from the library.  Prints one JSON line.

    python scripts/dev/time_kappa_shear.py [--reps 5] [--work-columns 0] [--out profiles/kappa_shear_kernels.json]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--work-columns", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    from mom6_amd import build as mbuild
    G = abi.G
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    Md = keep[4]
    dev, GV = dyc.device, dyc.GV
    s = dyc.torch_stream()
    nk = d.nk
    sf = lambda n, **kw: synth_dev.smooth_field(d, dev, 700 + n, ox=0.5, oy=0.5, **kw)   # noqa: E731
    with torch.cuda.stream(s):
        wet = Md[G["mask2dT"]] > 0
        kk = torch.arange(nk, dtype=torch.float64, device=dev)[:, None, None]
        h = torch.where(wet[None], 10.0 * (1.0 + 0.3 * sf(0, nk=5)[torch.arange(nk, device=dev) % 5]), torch.zeros((), dtype=torch.float64, device=dev)).contiguous()
        rows = torch.arange(d.shape2()[0], device=dev) - d.joff
        j0 = int(0.25 * d.nj); j1 = j0 + int(round(0.45 * d.nj))
        band = torch.where((rows >= j0) & (rows < j1), 1.0, 0.05).to(torch.float64)[:, None]
        prof = torch.tanh((kk - 0.5 * (nk - 1)) / 1.5)
        profv = torch.tanh((kk - 0.5 * (nk - 1) + 0.5) / 1.5)
        u1 = ((0.8 * (0.6 + 0.8 * sf(20)) * band)[None] * prof * Md[G["mask2dCu"]][None]).contiguous()
        v1 = ((-0.24 * (0.6 + 0.8 * sf(21)) * band)[None] * profv * Md[G["mask2dCv"]][None]).contiguous()
        T = (25.0 - 0.3 * kk + 0.2 * sf(10)[None]).contiguous()   # 25 .. 3 degC: stable down to the bottom layer
        S = (34.5 + 0.02 * kk + 0.05 * sf(11)[None]).contiguous()
        p_surf = (1.0e4 * (1.0 + 0.5 * sf(40))).contiguous()
        out = [torch.full(d.shape3(nk + 1), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
        its = torch.full(d.shape2(), float("nan"), dtype=torch.float64, device=dev)
    dyc.sync()
    calib = bench.box_calibration(dyc.device)
    cols = d.ni * d.nj
    nbytes = 8 * cols * (5 * nk + 3 * (nk + 1))
    P = abi.kappa_shear_params_default(GV, kappa_0=1.5e-5, work_columns=a.work_columns)
    dyc.kappa_shear_init(P, abi.eos_params_default(abi.WRIGHT))
    work_bytes = dyc.kappa_shear_work_bytes()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(); fn(); c1.record(); c1.synchronize()
            t.append(c0.elapsed_time(c1))
        return statistics.median(t)

    def copy_ms(nb):
        src = torch.ones(max(nb // 16, 1), dtype=torch.float64, device=dev)   # a copy moves each byte twice: half the bytes as the source
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))

    res_json = json.load(open(os.path.join(os.path.dirname(mbuild.LIB), "kernel_resources.json")))["kappa_shear.hip"]
    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    res = {}
    for name, scale in (("shear", 1.0), ("quiescent", 0.025)):
        with torch.cuda.stream(s):
            u = (scale * u1).contiguous(); v = (scale * v1).contiguous()
        call = lambda: dyc.Calculate_kappa_shear(u, v, h, 3600.0, out[0], out[1], out[2], T=T, S=S, p_surf=p_surf, zero_mix=True,   # noqa: E731
                                                 KS_its=its)
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
                if k.startswith("k_kappa_shear") and cnt > 0 and tot > 0.0:
                    tot_ms += tot; seen[k] = seen.get(k, 0) + cnt
            per.append(tot_ms)
        dycore.prof_enable(dyc, False)
        if not seen:
            raise SystemExit("time_kappa_shear: the context's per-launch events recorded no launch of k_kappa_shear")
        ms, cms = statistics.median(per), copy_ms(nbytes)
        w = wet[own]
        it = its[own][w]
        mixing = (out[0][(Ellipsis,) + own] > 0).any(dim=0)[w]
        res[name] = dict(kernels=sorted(seen), launches_per_call=sum(seen.values()) // a.reps, ms=round(ms, 3),
                         GBps_of_what_must_move=round(nbytes / 1e9 / (ms * 1e-3), 1), copy_ms=round(cms, 3),
                         kernel_over_that_copy=round(ms / cms, 2), ms_at_box_copy_rate=round(nbytes / 1e9 / calib["copy_GBps"] * 1e3, 3),
                         wet_columns=int(w.sum()), columns_with_kappa_gt_0=int(mixing.sum()), KS_its_mean=round(float(it.mean()), 3),
                         KS_its_max=int(it.max()), outputs_finite=bool(all(torch.isfinite(o[(Ellipsis,) + own]).all() for o in out)))
    line = dict(cases=res, grid=[args.ni, args.nj, args.nk], reps=a.reps, dt=3600.0,
                setting="WRIGHT, zero_mix, p_surf, kappa_0 = 1.5e-5, KS_its the only diagnostic",
                what_must_move="8*columns*(5*nk + 3*(nk + 1)) bytes: u, v, h, T, S read, kappa_io, tke_io, kv_io written",
                GB_that_must_move=round(nbytes / 1e9, 3), work_columns=work_bytes // (51 * (nk + 1) * 8), workspace_bytes=work_bytes,
                registers={k: v for k, v in res_json.items()}, box_calibration=calib)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
