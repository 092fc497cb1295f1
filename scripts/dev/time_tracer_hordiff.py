"""Time mom6x_tracer_hordiff on the headline state (bench.py's build_model and make_thermo: 1440 x 1080 x 75, KHTR = 1000) with
2 and 8 tracers, each with one iteration and with three (MAX_TR_DIFFUSION_CFL = 3, no CFL check: no synchronisation), as the
median of --reps calls, each between two device events.  In the same process: a device copy that moves exactly the algorithmic
bytes of the call, (8 + 16 ntr) B per cell-layer and iteration (h read; every tracer read and written: ntr whole arrays and half
an array copied, since a copy reads and writes each of its bytes), and the round trip the call replaces (h and the tracers to pinned
host memory, the tracers back).  Prints one JSON line per case.

    python scripts/dev/time_tracer_hordiff.py [--reps 20] [--out profiles/tracer_hordiff_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, stream, reps, torch):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi, synth_dev
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    thermo, _report = bench.make_thermo(args, dyc, d, st, 4)
    cells = dict(zip(thermo.__code__.co_freevars, (c.cell_contents for c in thermo.__closure__)))
    h = st["h"]
    reg = [cells["T"].clone(), cells["S"].clone()]
    for m in range(6):
        reg.append((1.0 + synth_dev.smooth_field(d, h.device, 700 + m, nk=d.nk, ox=0.5, oy=0.5)).contiguous())
    dst = [torch.empty_like(x) for x in reg]
    half = h.numel() // 2
    s = dyc.torch_stream()
    cl = d.nk * d.ni * d.nj
    lines = []
    for ntr in (2, 8):
        tr = reg[:ntr]
        for itts in (1, 3):
            P = abi.tracer_hor_diff_params_default(KHTR=1000.0, max_diff_CFL=3.0 if itts == 3 else -1.0)
            dyc.tracer_hor_diff_init(P)
            torch.cuda.synchronize()
            for _ in range(3):
                n = dyc.tracer_hordiff(h, 3600.0, tr)
            dyc.sync()
            assert n == itts
            ms = timed(lambda: dyc.tracer_hordiff(h, 3600.0, tr), s, a.reps, torch)

            def copy():
                with torch.cuda.stream(s):
                    for _ in range(itts):
                        for x, y in zip(tr, dst):
                            y.copy_(x)
                        dst[-1].view(-1)[:half].copy_(h.view(-1)[:half])
            copy(); dyc.sync()
            copy_ms = timed(copy, s, a.reps, torch)
            down = [h] + tr
            host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in down]

            def round_trip():
                with torch.cuda.stream(s):
                    for hst, x in zip(host, down):
                        hst.copy_(x, non_blocking=True)
                    for hst, x in zip(host[1:], tr):
                        x.copy_(hst, non_blocking=True)
            round_trip(); dyc.sync()
            trip_ms = timed(round_trip, s, max(3, a.reps // 4), torch)
            del host
            alg = (8 + 16 * ntr) * cl * itts
            line = dict(routine=f"mom6x_tracer_hordiff (KHTR = 1000): {itts} x (k_thd_save_x + k_thd_save_y + k_thd_tile) + k_thd_khdt",
                        grid=[args.ni, args.nj, args.nk], ntr=ntr, num_itts=itts, reps=a.reps, ms=round(ms, 4),
                        algorithmic_GB=round(alg / 1e9, 3), frac_of_hbm_peak=round(alg / 1e9 / (ms / 1e3) / bench.HBM_PEAK_GBS, 4),
                        equal_bytes_copy_ms=round(copy_ms, 4), call_over_copy=round(ms / copy_ms, 3),
                        round_trip_ms=round(trip_ms, 3), round_trip_over_call=round(trip_ms / ms, 1),
                        finite=all(bool(torch.isfinite(x).all()) for x in tr))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
