"""What compute_column costs on the device: one mcgpu_compute_column call (type 2, the dust optical depth from every cell
towards the star, +z, -z and +r: 4 n_cells rays in one launch) on ref4.1 in 2D, ref4.1 in 3D and the bench's Voronoi model
(the ref4.1 disk as --sites Voronoi sites, tessellated by the product's kernel).  The figure is the device-event time the
call returns, --reps calls after one warm-up call: min, median, max.  n_capped must be 0.

    python tools/column_bench.py [--models ref41,ref41_3d,voronoi] [--sites 1000000] [--reps 5] [--type 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcfost_amd.engine import Engine          # noqa: E402
from mcfost_amd.host import model as M        # noqa: E402


def build(name, sites):
    if name == "ref41":
        return M.build_model(M.ref41())
    if name == "ref41_3d":
        return M.build_model(M.ref41_3d())
    from mcfost_amd.host import voronoi as V
    return M.build_voronoi_model(M.ref41(), sites, seed=1, tessellator=V.device_tessellator(0), platonic=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ref41,ref41_3d,voronoi")
    ap.add_argument("--sites", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--type", type=int, default=2, choices=[1, 2, 3])
    args = ap.parse_args()
    out = {"type": args.type, "reps": args.reps, "models": {}}
    for name in args.models.split(","):
        t0 = time.perf_counter()
        m = build(name, args.sites)
        t_build = time.perf_counter() - t0
        m.midplane_snap = 0   # the library's default (bench.py)
        lam = int(np.argmin(np.abs(np.asarray(m.lam) - 1.0))) + 1
        rng = np.random.default_rng(1)
        gas = 1.0e12 * np.exp(rng.normal(size=m.n_cells)) if args.type != 2 else None
        ab = np.full(m.n_cells, 1.0e-4, np.float32) if args.type == 3 else None
        e = Engine(m, 1e6)
        ms, capped, col = [], 0, None
        for i in range(args.reps + 1):
            col, capped, t = e.compute_column(args.type, lam=lam, gas_density=gas, abundance=ab)
            if i:
                ms.append(t)
        tau_mid, tau_ang = e.integ_tau(lam, 45.0)
        e.close()
        row = {"n_cells": int(m.n_cells), "rays": 4 * int(m.n_cells), "lambda": lam, "min_ms": float(min(ms)),
               "median_ms": float(np.median(ms)), "max_ms": float(max(ms)), "n_capped": int(capped),
               "max_column": float(col.max()), "tau_midplane": float(tau_mid), "tau_45deg": float(tau_ang),
               "model_build_s": t_build}
        out["models"][name] = row
        print("%-9s %8d cells  %8d rays  %8.3f ms  [%8.3f, %8.3f]  %6.1f Mrays/s  n_capped %d  (model built in %.1f s)"
              % (name, row["n_cells"], row["rays"], row["median_ms"], row["min_ms"], row["max_ms"],
                 row["rays"] / row["median_ms"] * 1e-3, capped, t_build), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
