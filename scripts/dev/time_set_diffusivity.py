"""Time the kernels of mom6x_set_BBL_TKE and mom6x_set_diffusivity on the headline grid (bench.py's build_model: 1440 x 1080 x 75)
with the context's per-launch events (mom6x_prof_*), with an equation of state (WRIGHT), the law of the wall, the dissipation
floors and double diffusion on and Kd_int, Kd_lay, Kd_extra_T, Kd_extra_S as outputs.  For each kernel: the time, the bytes it moves
by the accounting of DESIGN.md section 4 (bytes_moved below), that rate against the box's copy rate (bench.box_calibration) and
against a device copy of the same number of bytes timed in the same run; and the floor of an on-chip column variant, which would read
h, T, S once and write the four outputs once.  Prints one JSON line.

    python scripts/dev/time_set_diffusivity.py [--reps 20] [--out profiles/set_diffusivity_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def bytes_moved(d):
    """Bytes per kernel, in units of one 3-D array over the computational domain (A) or one whole array (W: slab x levels).
    k_sd_cols, per column and level: sweep 1 (vert_fill_TS) reads h, T, S, writes T_f, S_f, c1, then reads those three and writes
    T_f, S_f = 11; sweep 2 reads h, T_f, S_f, writes dRho_int, N2_int, N2_lay, Kd_lay_2d, Kd_extra_T, Kd_extra_S = 9; sweep 3 touches
    the two deepest levels only; sweep 4 reads Kd_lay_2d, N2_int, N2_lay, h and writes Kd_int, Kd_lay = 6.  k_sd_fill writes the halos
    of Kd_int, Kd_extra_T, Kd_extra_S (nk + 1 levels) and Kd_lay (nk), and the two outer interfaces of Kd_extra_T, Kd_extra_S on the
    computational domain.  k_set_BBL_TKE with a boundary layer thinner than the
    bottom layer: one level of h, u, v, the four planes of set_viscous_BBL, five metric planes, three planes written."""
    A = 8 * d.nk * d.ni * d.nj
    plane = 8 * d.ni * d.nj
    W = 8 * d.slab
    return dict(k_sd_cols=26 * A, k_sd_fill=(W - plane) * (3 * (d.nk + 1) + d.nk) + 4 * plane, k_set_BBL_TKE=(3 + 4 + 5 + 3) * plane), 7 * A


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
    h, u, v = st["h"], st["u"], st["v"]
    Kv_bbl_u, Kv_bbl_v, bbl_u, bbl_v = keep[:4]
    s = dyc.torch_stream()
    nk = d.nk
    with torch.cuda.stream(s):
        zf = (torch.arange(nk, dtype=torch.float64, device=dev) / (nk - 1))[:, None, None]
        pT = synth_dev.smooth_field(d, dev, 710, ox=0.5, oy=0.5)[None]
        pS = synth_dev.smooth_field(d, dev, 711, ox=0.5, oy=0.5)[None]
        T = (20.0 - 15.0 * zf + 0.8 * pT * (1.0 - 0.5 * zf)).contiguous()
        # salt falls with depth in the northern half (salt fingers) and rises in the southern
        north = (torch.arange(d.shape2()[0], device=dev) - d.joff >= d.nj // 2)[None, :, None]
        S = torch.where(north, 36.0 - 2.2 * zf + 0.2 * pS, 34.5 + 1.0 * zf + 0.2 * pS).contiguous()
        out = {n: torch.full(d.shape3(nk if n == "Kd_lay" else nk + 1), float("nan"), dtype=torch.float64, device=dev)
               for n in ("Kd_int", "Kd_lay", "Kd_extra_T", "Kd_extra_S")}
        planes = [torch.full(d.shape2(), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    P = abi.set_diffusivity_params_default(GV, Kd=1.5e-5, double_diffusion=1, BBL_effic=0.2, use_LOTW_BBL_diffusivity=1, Kd_max=1.0e-2,
                                           dissip_min=1.0e-9, dissip_N0=1.0e-8, dissip_N1=2.0e-5, dissip_Kd_min=2.0e-6)
    dyc.set_diffusivity_init(P, abi.eos_params_default(abi.WRIGHT))
    calib = bench.box_calibration(dyc.device)

    def call():
        dyc.set_BBL_TKE(u, v, h, Kv_bbl_u, Kv_bbl_v, bbl_u, bbl_v, *planes)
        dyc.set_diffusivity(h, args.dt, out["Kd_int"], T=T, S=S, ustar_BBL=planes[0], BBL_meanKE_loss=planes[1],
                            **{n: out[n] for n in ("Kd_lay", "Kd_extra_T", "Kd_extra_S")})

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
            if (k.startswith("k_sd") or k.startswith("k_set_BBL_TKE")) and cnt > 0 and tot > 0.0:
                per.setdefault(k.split("<")[0], []).append(tot / cnt)
    dycore.prof_enable(dyc, False)
    kern_ms = {k: statistics.median(v) for k, v in per.items()}
    moved, on_chip = bytes_moved(d)

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
    own = d.sl(0, d.ni - 1, 0, d.nj - 1)
    Kd = out["Kd_int"][(slice(None),) + own]
    line = dict(routine="mom6x_set_BBL_TKE + mom6x_set_diffusivity", grid=[args.ni, args.nj, args.nk], reps=a.reps,
                setting="EOS WRIGHT, USE_LOTW_BBL_DIFFUSIVITY, dissipation floors, DOUBLE_DIFFUSION; Kd_int, Kd_lay, Kd_extra_T, Kd_extra_S",
                call_ms=round(call_ms, 4), kernels=kernels,
                on_chip_variant_floor=dict(GB_moved=round(on_chip / 1e9, 3), what="h, T, S read once; Kd_int, Kd_lay, Kd_extra_T, Kd_extra_S written once",
                                           ms_at_box_copy_rate=round(on_chip / 1e9 / calib["copy_GBps"] * 1e3, 4),
                                           copy_of_the_same_bytes_ms=round(copy_ms(on_chip), 4)),
                box_calibration=calib, Kd_int_finite=bool(torch.isfinite(Kd).all()), Kd_int_max=float(Kd.max()),
                salt_finger_interfaces=int((out["Kd_extra_S"][(slice(None),) + own] > 0).sum()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
