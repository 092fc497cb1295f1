"""Time mom6x_thickness_diffuse on the headline state (bench.py's build_model and make_thermo: 1440 x 1080 x 75, WRIGHT, KHTH = 600)
and, in the same run, the round trip a host-side thickness_diffuse needs at the least: h, T, S to the host and h, uhtr, vhtr
back.  Prints one JSON line: the call's ms (device events), the algorithmic bytes from the shapes (8 words per cell-layer with an
EOS: h, T, S read, uhtr, vhtr read and written, h written), the bytes the three kernels actually move through HBM counted the same
way, the fractions of the HBM roof, and the round trip's ms.

    python scripts/dev/time_thickness_diffuse.py [--reps 20] [--out profiles/thickness_diffuse_time.json]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# words per cell-layer through HBM, each array counted once per kernel that touches it (the two cells of a face share lines):
# k_td_cols reads h, T, S, writes h_avail_rsum, h_frac, pres, T_f, S_f, c1 and re-reads T_f, S_f, c1 to write T_f, S_f again (14);
# k_td_faces reads h, T_f, S_f, pres, h_avail_rsum, h_frac once per direction (12), reads and writes uhtr | vhtr and writes
# uhD | vhD (6); k_td_update reads uhD, vhD, h and writes h (4)
WORDS_MOVED = 14 + 18 + 4
WORDS_FLOOR = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from mom6_amd import abi
    args = types.SimpleNamespace(ni=1440, nj=1080, nk=75, dt=900.0, tracers=2, bthalo=0)
    dyc, d, st, taux, tauy, keep = bench.build_model(args, (1, 1), (0, 0), 0)
    thermo, _report = bench.make_thermo(args, dyc, d, st, 4)
    cells = dict(zip(thermo.__code__.co_freevars, (c.cell_contents for c in thermo.__closure__)))
    T, S = cells["T"], cells["S"]
    h, uhtr, vhtr = st["h"].clone(), st["uhtr"].clone(), st["vhtr"].clone()
    dyc.thickness_diffuse_init(abi.thickness_diffuse_params_default(KHTH=600.0), abi.eos_params_default(abi.WRIGHT))
    torch.cuda.synchronize()
    s = dyc.torch_stream()
    for _ in range(3):
        dyc.thickness_diffuse(h, uhtr, vhtr, args.dt, T=T, S=S)
    dyc.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.reps):
        dyc.thickness_diffuse(h, uhtr, vhtr, args.dt, T=T, S=S)
    e1.record(s)
    dyc.sync(); e1.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    # the host path's least traffic: h, T, S down to pinned host memory, h, uhtr, vhtr back up
    down, up = (h, T, S), (h, uhtr, vhtr)
    host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in down]

    def round_trip():
        for hst, x in zip(host, down):
            hst.copy_(x, non_blocking=True)
        for hst, x in zip(host, up):
            x.copy_(hst, non_blocking=True)

    hsave = [x.clone() for x in up]
    round_trip()
    torch.cuda.synchronize()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    round_trip()
    c1.record(); c1.synchronize()
    trip_ms = c0.elapsed_time(c1)
    for x, y in zip(up, hsave):
        x.copy_(y)
    cl = d.nk * d.ni * d.nj
    b_floor, b_moved = 8 * WORDS_FLOOR * cl, 8 * WORDS_MOVED * cl
    line = dict(routine="mom6x_thickness_diffuse (WRIGHT, KHTH = 600): k_td_cols + k_td_faces<2,1> + k_td_update",
                grid=[args.ni, args.nj, args.nk], ms=round(ms, 4), reps=a.reps,
                floor_words_per_cell_layer=WORDS_FLOOR, floor_GB=round(b_floor / 1e9, 3),
                frac_of_hbm_peak_floor=round(b_floor / 1e9 / (ms / 1e3) / bench.HBM_PEAK_GBS, 4),
                moved_words_per_cell_layer=WORDS_MOVED, moved_GB=round(b_moved / 1e9, 3),
                frac_of_hbm_peak_moved=round(b_moved / 1e9 / (ms / 1e3) / bench.HBM_PEAK_GBS, 4),
                round_trip_ms=round(trip_ms, 3), round_trip_GB=round(6 * h.numel() * 8 / 1e9, 3),
                h_finite=bool(torch.isfinite(h).all()))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
