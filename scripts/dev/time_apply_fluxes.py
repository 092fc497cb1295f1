"""Time the kernels of mom6x_applyBoundaryFluxesInOut on the headline grid (bench.py's build_model: 1440 x 1080 x 75) with the
context's per-launch events (mom6x_prof_*): EOS WRIGHT, three bands of penetrating shortwave with realistic opacities, the
energetics (cTKE, dSV_dT, dSV_dS) and SkinBuoyFlux.  For the column kernel: the time, the bytes by the accounting of DESIGN.md
section 4 (bytes_moved below), that rate against the box's copy rate (bench.box_calibration), and the yardstick -- a device copy,
timed in the same run, of the bytes the call MUST move (h, T, S and the opacities read once; h, T, S, cTKE, dSV_dT, dSV_dS written
once) -- next to a copy of what the kernel does move (the htot pre-sum reads h a second time).  Prints one JSON line.

    python scripts/dev/time_apply_fluxes.py [--reps 20] [--out profiles/diabatic_aux_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def bytes_moved(d, nsw):
    """Bytes in units of one 3-D array over the computational domain (A) or one whole array (W: slab x levels).  k_da_cols, per
    column and level: the pre-sum reads h = 1; the walk reads h, T, S and at most nsw opacities (a band that is used up is not
    read further down) and writes h, T, S, cTKE, dSV_dT, dSV_dS = 9 + nsw; the upward loop only where shortwave reached the bottom;
    about forty planes.  k_da_fill writes the halos of cTKE (nk levels) and of SkinBuoyFlux.  What the call must move: the same
    without the second read of h."""
    A = 8 * d.nk * d.ni * d.nj
    plane = 8 * d.ni * d.nj
    W = 8 * d.slab
    return dict(k_da_cols=(10 + nsw) * A + 40 * plane, k_da_fill=(W - plane) * (d.nk + 1)), (9 + nsw) * A


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
    dev, GV = dyc.device, dyc.GV
    h = st["h"]
    s = dyc.torch_stream()
    nk, nsw = d.nk, 3
    sf = lambda n: synth_dev.smooth_field(d, dev, 800 + n, ox=0.5, oy=0.5)
    with torch.cuda.stream(s):
        zf = (torch.arange(nk, dtype=torch.float64, device=dev) / (nk - 1))[:, None, None]
        pT, pS = sf(10)[None], sf(11)[None]
        T = (20.0 - 15.0 * zf + 0.8 * pT * (1.0 - 0.5 * zf)).contiguous()
        S = (34.5 + 1.0 * zf + 0.2 * pS).contiguous()
        wet = keep[4][abi.G["mask2dT"]]
        fl = dict(sw=150.0 * (1.0 + sf(30)), lw=-60.0 * (1.0 + 0.3 * sf(31)), latent=-90.0 * (1.0 + 0.8 * sf(32)), sens=15.0 * sf(33),
                  evap=1.0e-4 * (sf(34) - 0.3), lprec=8.0e-5 * (sf(35) + 0.2), fprec=1.0e-5 * sf(36).abs(), vprec=2.0e-5 * sf(37),
                  lrunoff=3.0e-5 * sf(38).clamp(min=0.0), frunoff=1.0e-5 * sf(39).clamp(min=0.0),
                  lrunoff_glc=4.0e-6 * sf(40).clamp(min=0.0), frunoff_glc=2.0e-6 * sf(41).clamp(min=0.0),
                  seaice_melt=3.0e-5 * sf(42), salt_flux=1.0e-6 * sf(45))
        fl = {n: (v * wet).contiguous() for n, v in fl.items()}
        pen = torch.stack([fl["sw"] * (0.25 / (n + 1)) for n in range(nsw)]).contiguous()
        opac = torch.stack([(op * (1.0 + 0.1 * pT)).expand(nk, -1, -1) for op in (0.05, 0.3, 3.0)]).contiguous()
        out = {n: torch.full(d.shape3(), float("nan"), dtype=torch.float64, device=dev) for n in ("cTKE", "dSV_dT", "dSV_dS")}
        out["SkinBuoyFlux"] = torch.full(d.shape2(), float("nan"), dtype=torch.float64, device=dev)
        for n in ("netMassIn", "netMassOut"):
            fl[n] = torch.full(d.shape2(), float("nan"), dtype=torch.float64, device=dev)
    dyc.diabatic_aux_init(abi.diabatic_aux_params_default(GV, ignore_fluxes_over_land=1), abi.eos_params_default(abi.WRIGHT))
    calib = bench.box_calibration(dyc.device)

    def call():
        dyc.applyBoundaryFluxesInOut(args.dt, fl, h, T, S, nsw=nsw, opacity_band=opac, sw_pen_band=pen, aggregate_FW_forcing=True,
                                     evap_CFL_limit=0.8, minimum_forcing_depth=0.001, **out)

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
            if k.startswith("k_da_") and cnt > 0 and tot > 0.0:
                per.setdefault(k.split("<")[0], []).append(tot / cnt)
    dycore.prof_enable(dyc, False)
    kern_ms = {k: statistics.median(v) for k, v in per.items()}
    moved, must = bytes_moved(d, nsw)

    def copy_ms(nbytes):                                        # a copy moves each byte twice: half the bytes as the source
        src = torch.ones(max(nbytes // 16, 1), dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(); dst.copy_(src); c1.record(); c1.synchronize()
            t.append(c0.elapsed_time(c1))
        return statistics.median(t)

    kernels = {}
    for k, ms in kern_ms.items():
        if k not in moved:
            continue
        nb = moved[k]
        cp = copy_ms(nb)
        kernels[k] = dict(ms=round(ms, 4), GB_moved=round(nb / 1e9, 3), GBps=round(nb / 1e9 / (ms / 1e3), 1),
                          frac_of_box_copy_rate=round(nb / 1e9 / (ms / 1e3) / calib["copy_GBps"], 4),
                          copy_of_the_same_bytes_ms=round(cp, 4), times_that_copy=round(ms / cp, 3))
    must_ms = copy_ms(must)
    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    status = dyc.diabatic_aux_status()
    cT = out["cTKE"][(slice(None),) + own]
    line = dict(routine="mom6x_applyBoundaryFluxesInOut", grid=[args.ni, args.nj, args.nk], reps=a.reps,
                setting="EOS WRIGHT, 3 bands (0.05, 0.3, 3 m-1), energetics (cTKE, dSV_dT, dSV_dS), SkinBuoyFlux, netMassIn, netMassOut",
                call_ms=round(call_ms, 4), kernels=kernels,
                yardstick=dict(what="a device copy of the bytes the call must move: h, T, S and 3 opacities read; h, T, S, cTKE, dSV_dT, dSV_dS written",
                               GB=round(must / 1e9, 3), copy_ms=round(must_ms, 4), ms_at_box_copy_rate=round(must / 1e9 / calib["copy_GBps"] * 1e3, 4),
                               k_da_cols_over_that_copy=round(kern_ms.get("k_da_cols", float("nan")) / must_ms, 3),
                               second_read_of_h_GB=round((moved["k_da_cols"] - must) / 1e9, 3)),
                box_calibration=calib, status_after_all_calls=status, outputs_finite=bool(torch.isfinite(cT).all() and torch.isfinite(T[(slice(None),) + own]).all()),
                cTKE_min=float(cT.min()), cTKE_max=float(cT.max()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
