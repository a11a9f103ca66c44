"""What a molecular line cube costs on the device: one mcgpu_line_map call (method 2, --npix x --npix pixels, one inclination,
two transitions of the synthetic rotor, Keplerian rotation) on ref4.1 in 2D, ref4.1 in 3D and a Voronoi model of the ref4.1
disk, with 41 and 101 channels.  Next to each, mcgpu_tau_maps (optical depth only) for the same pixels: the bare walk, one
ray per LANE, so the ratio shows what the profile and one ray per WAVE cost.  Figures are device-event times, --reps calls
after one warm-up call: min, median, max.  n_capped must be 0.

The kinetic temperature is analytic here, 200 K (r / AU)^-0.5 with a floor of 10 K, and v_turb = 100 m/s: the tool times the ray
tracer, not a temperature step.  The longest walk and the mean n_vpoints come from the restatement (tests/line_walk.py over the
CPU oracle) on a --sample x --sample image of the same map.

    python tools/line_bench.py [--models ref41,ref41_3d,voronoi] [--sites 100000] [--npix 512] [--reps 3] [--sample 24]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mcfost_amd.engine import Engine          # noqa: E402
from mcfost_amd.host import model as M        # noqa: E402
from mcfost_amd.host import molecule as MOL   # noqa: E402


def build(name, sites, incl):
    kw = dict(RT_imin=incl, RT_imax=incl, RT_n_incl=1)
    if name == "ref41":
        return M.build_model(M.DiskConfig(**kw))
    if name == "ref41_3d":
        return M.build_model(M.DiskConfig(name="ref4.1_3D", nz=50, n_az=72, l3D=True, **kw))
    from mcfost_amd.host import voronoi as V
    return M.build_voronoi_model(M.DiskConfig(**kw), sites, seed=1, tessellator=V.device_tessellator(0), platonic=True)


def tables(m, n_speed):
    g = m.grid
    n = m.n_cells
    voro = g.get("grid_type", 1) == 3
    if voro:
        xyz = np.asarray(g["v_xyz_dp"], np.float64).reshape(-1, 3)[:n]
        x, y = xyz[:, 0], xyz[:, 1]
    else:
        r, phi = np.asarray(g["r_grid"], np.float64)[:n], np.asarray(g["phi_grid"], np.float64)[:n]
        x, y = r * np.cos(phi), r * np.sin(phi)
    rc = np.maximum(np.hypot(x, y), 1e-3)
    T = np.maximum(200.0 * rc ** -0.5, 10.0).astype(np.float32)
    vk = np.sqrt(6.67408e-11 * 1.98855e30 / (rc * MOL.AU_TO_M))
    if voro:
        vel = dict(vxyz=np.stack([-y / rc * vk, x / rc * vk, np.zeros(n)], 1).reshape(-1))
    else:
        vel = dict(vfield_mode=1, vfield=vk.astype(np.float32), lkeplerian=True, linfall=False)
    gas = np.asarray(m.rho_dust, np.float64)[:n] * 100.0 / (2.3 * MOL.MH) * 1.0e6
    ts = MOL.tab_speed_rt(-6000.0, 6000.0, n_speed)
    return MOL.line_tables(m, MOL.linear_rotor(), T, gas, np.full(n, 1.0e-4, np.float32), (2, 3), ts, v_turb=100.0, velocity=vel)


def walk_stats(m, mol, map_size, sample):
    """(longest walk, mean n_vpoints) of a sample x sample image of the same map, from the restatement."""
    import line_walk as W
    from oracle import Oracle
    o = Oracle(m, 1000)
    rays = W.ray_starts(m, 2, sample, sample, map_size)
    paths = W.walk_paths(o, m, rays)
    small = dict(mol, tab_speed=np.zeros(1))
    h = W.cube_from_paths(m, small, rays, paths)["hist"]
    return int(paths["n_steps"].max()), float((h * np.arange(h.size)).sum() / max(1, h.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ref41,ref41_3d,voronoi")
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--npix", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--incl", type=float, default=60.0)
    ap.add_argument("--channels", default="41,101")
    args = ap.parse_args()
    out = {"npix": args.npix, "reps": args.reps, "incl": args.incl, "models": {}}
    for name in args.models.split(","):
        t0 = time.perf_counter()
        m = build(name, args.sites, args.incl)
        t_build = time.perf_counter() - t0
        m.midplane_snap = 0   # the library's default (bench.py)
        size = 2.2 * float(m.cfg.rout)
        lam = int(np.argmin(np.abs(np.asarray(m.lam) - 1300.0))) + 1
        e = Engine(m, 1e6)
        tau_ms = []
        for i in range(args.reps + 1):
            t = e.tau_maps(lam, args.npix, args.npix, size, surface=False)[2]
            if i:
                tau_ms.append(t)
        row = {"n_cells": int(m.n_cells), "rays": args.npix * args.npix, "tau_maps_median_ms": float(np.median(tau_ms)),
               "model_build_s": t_build, "channels": {}}
        mol = None
        for ns in (int(c) for c in args.channels.split(",")):
            mol = tables(m, ns)
            ms, capped, peak = [], 0, 0.0
            for i in range(args.reps + 1):
                spec, cont, capped, t = e.line_map(mol, npix_x=args.npix, npix_y=args.npix, map_size=size)
                peak = float(spec.max())
                del spec, cont
                if i:
                    ms.append(t)
            row["channels"][ns] = {"min_ms": float(min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(max(ms)),
                                   "n_capped": int(capped), "peak": peak,
                                   "ratio_to_tau_maps": float(np.median(ms) / np.median(tau_ms))}
            print("%-9s %8d cells  %3d channels  %9.3f ms  [%9.3f, %9.3f]   tau_maps %8.3f ms   ratio %7.1f   n_capped %d"
                  % (name, row["n_cells"], ns, np.median(ms), min(ms), max(ms), np.median(tau_ms),
                     np.median(ms) / np.median(tau_ms), capped), flush=True)
        e.close()
        if args.sample:
            row["longest_walk"], row["mean_n_vpoints"] = walk_stats(m, mol, size, args.sample)
            print("%-9s longest walk %d crossings, mean n_vpoints %.1f (a %d x %d sample of the map; model built in %.1f s)"
                  % (name, row["longest_walk"], row["mean_n_vpoints"], args.sample, args.sample, t_build), flush=True)
        out["models"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
