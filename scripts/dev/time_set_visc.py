"""Time mom6x_set_viscous_BBL on the headline state (bench.py's build_model and make_thermo: 1440 x 1080 x 75, WRIGHT) and, in the
same run, the device-to-host copy of u, v and h that a host-side set_viscous_BBL needs at the least.  Prints one JSON line: the
kernel's ms, its algorithmic bytes (from the shapes and the layers the walks actually visited, counted on the device from the
outputs' inputs) and the fraction of the HBM roof, and the D2H copy's ms.

    python scripts/dev/time_set_visc.py [--reps 20] [--out profiles/set_visc_time.json]
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def walk_layers(h, u, v, M, d, Hbbl, Angstrom_H, h_neglect):
    """The layers the near-bottom walk of each unmasked face reads (bottom-up until Hbbl of non-vanished fluid, as in
    set_visc.hip), summed over the faces of both directions.  Uses the arithmetic mean thickness: a count, not a result."""
    import torch
    from mom6_amd import abi
    G = abi.G
    tot = 0
    for dirn, (vel, mname, dj, di) in enumerate(((u, "mask2dCu", 0, 1), (v, "mask2dCv", 1, 0))):
        j0, j1 = (d.joff, d.joff + d.nj) if dirn == 0 else (d.joff - 1, d.joff + d.nj)
        i0, i1 = (d.ioff - 1, d.ioff + d.ni) if dirn == 0 else (d.ioff, d.ioff + d.ni)
        hv = 0.5 * (h[:, j0:j1, i0:i1] + h[:, j0 + dj:j1 + dj, i0 + di:i1 + di])
        m = M[G[mname]][j0:j1, i0:i1] > 0
        ok = (hv >= 1.5 * Angstrom_H + h_neglect).flip(0)
        above = torch.cumsum(torch.where(ok, hv.flip(0), torch.zeros_like(hv)), 0) - torch.where(ok, hv.flip(0), torch.zeros_like(hv))
        visited = (above < Hbbl)                                   # the walk reads layer k unless Hbbl was reached below it
        tot += int((visited & m[None]).sum().item())
    return tot


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
    u, v, h = st["u"], st["v"], st["h"]
    P = abi.set_visc_params_default(HBBL=10.0, Kv=1.0e-4)
    P.drag_bg_vel = 0.05
    dyc.set_visc_init(P, abi.eos_params_default(abi.WRIGHT))
    out = {n: dyc.zeros2() for n in ("Kv_bbl_u", "Kv_bbl_v", "bbl_thick_u", "bbl_thick_v")}
    torch.cuda.synchronize()
    s = dyc.torch_stream()
    for _ in range(3):
        dyc.set_viscous_BBL(u, v, h, T=T, S=S, **out)
    dyc.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(a.reps):
        dyc.set_viscous_BBL(u, v, h, T=T, S=S, **out)
    e1.record(s)
    dyc.sync(); e1.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    # the host path's least traffic: u, v, h down to pinned host memory
    host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (u, v, h)]
    for hst, x in zip(host, (u, v, h)):
        hst.copy_(x, non_blocking=True)
    torch.cuda.synchronize()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    for hst, x in zip(host, (u, v, h)):
        hst.copy_(x, non_blocking=True)
    c1.record(); c1.synchronize()
    d2h_ms = c0.elapsed_time(c1)
    # algorithmic bytes: the pressure sum reads h over the whole column, once per cell from HBM (the faces share their cells); the
    # near-bottom walk adds, per visited face-layer, its own velocity and T and S (one word each per face: the neighbouring face
    # reads the other cell); the 2-D planes (2 masks, Coriolis, tideamp unused) and the 4 outputs add 8 words per face.
    nface = int((keep[4][abi.G["mask2dCu"]] > 0).sum().item() + (keep[4][abi.G["mask2dCv"]] > 0).sum().item())
    GV = dyc.GV
    nvis = walk_layers(h, u, v, keep[4], d, P.Hbbl, GV.Angstrom_H, GV.H_subroundoff)
    b_h = 8 * d.nk * d.ni * d.nj
    b_alg = b_h + 8 * 3 * nvis + 8 * 8 * nface
    line = dict(kernel="k_set_viscous_BBL<2> (WRIGHT)", grid=[args.ni, args.nj, args.nk], ms=round(ms, 4), reps=a.reps,
                faces=nface, walk_layers_visited=nvis, algorithmic_GB=round(b_alg / 1e9, 3), h_once_GB=round(b_h / 1e9, 3),
                GBps=round(b_alg / 1e9 / (ms / 1e3), 1), frac_of_hbm_peak=round(b_alg / 1e9 / (ms / 1e3) / bench.HBM_PEAK_GBS, 4),
                d2h_uvh_ms=round(d2h_ms, 3), d2h_uvh_GB=round(sum(x.numel() for x in (u, v, h)) * 8 / 1e9, 3))
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    dyc.close()


if __name__ == "__main__":
    main()
