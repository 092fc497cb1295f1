"""Time mom6x_neutral_diffusion_calc_coeffs and mom6x_neutral_diffusion on the headline grid (bench.py's build_model: 1440 x 1080 x
75) with the context's per-launch events (mom6x_prof_*): layers of about 60 m, T falling by 14 degC and S rising by 1 from top to
bottom with horizontal variations of half that (isopycnals cross the layers), WRIGHT, the local interface pressure, KHTR = 1000 m2
s-1 over an hour; neutral_diffusion with 2 and with 8 tracers, in both orders of its additions.  Beside each call, in the same
process, a device copy of the bytes the call must move:
  calc_coeffs        h, T, S read; Pint, Tint, Sint, dRdT, dRdS and the ten coefficient arrays written
  neutral_diffusion  h and the ten coefficient arrays read once, every tracer read and written
Registers and occupancy come from mom6_amd/lib/kernel_resources.json; the resident bytes from the library.  Prints one JSON line.

    python scripts/dev/time_neutral_diffusion.py [--reps 5] [--out profiles/neutral_diffusion_kernels.json]
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
    ap.add_argument("--ni", type=int, default=1440)
    ap.add_argument("--nj", type=int, default=1080)
    ap.add_argument("--nk", type=int, default=75)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, dycore, synth_dev
    from mom6_amd import build as mbuild
    G = abi.G
    args = types.SimpleNamespace(ni=a.ni, nj=a.nj, nk=a.nk, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    Md = keep[4]
    dev, GV = dyc.device, dyc.GV
    s = dyc.torch_stream()
    nk = d.nk
    ns = 2 * nk + 2
    sf = lambda n, **kw: synth_dev.smooth_field(d, dev, 800 + n, ox=0.5, oy=0.5, **kw)   # noqa: E731
    DT, KHTR = 3600.0, 1000.0
    with torch.cuda.stream(s):
        wet = Md[G["mask2dT"]] > 0
        zf = ((torch.arange(nk, dtype=torch.float64, device=dev) + 0.5) / nk)[:, None, None]
        h = torch.where(wet[None], 60.0 * (1.0 + 0.3 * sf(0, nk=5)[torch.arange(nk, device=dev) % 5]),
                        torch.full((), GV.Angstrom_H, dtype=torch.float64, device=dev)).contiguous()
        T = (22.0 - 14.0 * zf + 7.0 * sf(10)[None] + 0.3 * sf(12, nk=3)[torch.arange(nk, device=dev) % 3]).contiguous()
        S = (34.0 + 1.0 * zf + 0.4 * sf(11)[None]).contiguous()
        tracers = [(1.0 + 0.5 * zf + (0.4 + 0.05 * m) * sf(20 + m)[None]).contiguous() for m in range(8)]
        Coef_x = torch.zeros(d.shape3(nk + 1), dtype=torch.float64, device=dev)
        Coef_y = torch.zeros(d.shape3(nk + 1), dtype=torch.float64, device=dev)
        Coef_x[0] = DT * (KHTR * (Md[G["dy_Cu"]] * Md[G["IdxCu"]]))
        Coef_y[0] = DT * (KHTR * (Md[G["dx_Cv"]] * Md[G["IdyCv"]]))
    dyc.sync()
    calib = bench.box_calibration(dyc.device)
    cols = d.ni * d.nj
    coef_bytes = cols * 2 * (8 * 2 * ns + 2 * 2 * ns + 8 * (ns - 1))
    must = dict(calc_coeffs=cols * 8 * (3 * nk + 5 * (nk + 1)) + coef_bytes)
    for ntr in (2, 8):
        must[f"neutral_diffusion_{ntr}"] = cols * 8 * nk * (1 + 2 * ntr) + coef_bytes

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

    def profiled(call):
        call()
        dyc.sync()
        dycore.prof_enable(dyc, True)
        per, kernels = [], {}
        for _ in range(a.reps):
            dyc.sync()
            dycore.prof_reset(dyc)
            call()
            dyc.sync()
            tot_ms, each = 0.0, {}
            for k, (cnt, tot) in dycore.prof_report(dyc).items():
                if k.startswith("k_ndiff") and cnt > 0 and tot > 0.0:
                    tot_ms += tot; each[k] = (cnt, tot)
            per.append(tot_ms)
            for k, (cnt, tot) in each.items():
                kernels.setdefault(k, []).append((cnt, tot))
        dycore.prof_enable(dyc, False)
        if not kernels:
            raise SystemExit("time_neutral_diffusion: the context's per-launch events recorded no launch of k_ndiff_*")
        return statistics.median(per), {k: dict(launches=v[0][0], ms=round(statistics.median(t for _, t in v), 3)) for k, v in kernels.items()}

    res_json = json.load(open(os.path.join(os.path.dirname(mbuild.LIB), "kernel_resources.json")))["neutral_diffusion.hip"]
    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    res = {}

    def record(name, ms, kernels, nbytes, **more):
        cms = copy_ms(nbytes)
        res[name] = dict(kernels=kernels, ms=round(ms, 3), GB_that_must_move=round(nbytes / 1e9, 3),
                         GBps_of_what_must_move=round(nbytes / 1e9 / (ms * 1e-3), 1), copy_ms=round(cms, 3),
                         kernel_over_that_copy=round(ms / cms, 2), ms_at_box_copy_rate=round(nbytes / 1e9 / calib["copy_GBps"] * 1e3, 3), **more)

    work = {}
    for date in (20240101, 20240401):
        dyc.neutral_diffusion_init(abi.neutral_diffusion_params_default(ndiff_answer_date=date), abi.eos_params_default(abi.WRIGHT))
        work["resident_bytes"] = dyc.neutral_diffusion_work_bytes()
        ms, kernels = profiled(lambda: dyc.neutral_diffusion_calc_coeffs(h, T, S))
        if date == 20240101:
            cu = dyc.neutral_diffusion_coeffs(0)
            Po = cu["PoL"][(Ellipsis,) + d.sl(-1, d.ni - 1, 0, d.nj - 1)]
            wet_u = Md[G["mask2dCu"]][d.sl(-1, d.ni - 1, 0, d.nj - 1)] > 0
            frac = ((Po > 0) & (Po < 1)).any(dim=0)
            record("calc_coeffs", ms, kernels, must["calc_coeffs"], wet_u_faces=int(wet_u.sum()),
                   wet_u_faces_with_a_fractional_position=int((frac & wet_u).sum()))
        for ntr in (2, 8):
            trs = [t.clone() for t in tracers[:ntr]]
            dyc.sync()
            ms, kernels = profiled(lambda: dyc.neutral_diffusion(h, Coef_x, Coef_y, DT, trs))
            record(f"neutral_diffusion_{ntr}_tracers_answer_date_{date}", ms, kernels, must[f"neutral_diffusion_{ntr}"],
                   tracers_finite=bool(all(torch.isfinite(t[(Ellipsis,) + own]).all() for t in trs)))
        assert dyc.neutral_diffusion_status() == (0, 0, 0, 0)
    line = dict(cases=res, grid=[a.ni, a.nj, a.nk], reps=a.reps, dt=DT,
                setting="WRIGHT, NDIFF_REF_PRES = -1, no p_surf, KHTR = 1000, no diagnostics; every neutral_diffusion call works on the tracers the call before left",
                what_must_move=dict(calc_coeffs="h, T, S read; five interface arrays and the ten coefficient arrays written",
                                    neutral_diffusion="h and the ten coefficient arrays read once; every tracer read and written"),
                registers={k: v for k, v in res_json.items()}, box_calibration=calib, **work)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
