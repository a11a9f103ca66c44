"""What the SED step's mean radiation field costs: BASELINE config 2's SED step (ref4.1, ten inclinations, default-real
xI_scatt) at one star-dominated and one disk-dominated wavelength, with option "radiation_field_sed" off and on, the row
of xJ_abs in HBM ("xj_where" = 1) or in the workgroup's LDS (= 2), and what the automatic rule (= 0) takes.

With the option on the commit passes deposit xI_scatt with atomics, so the option-off figure is given twice: as a context
runs by default ("xi_log" = 1: the deposit log where it pays) and with atomics ("xi_log" = 0), which isolates the extra
deposit.  Every figure: the median of --reps runs of mcgpu_run_mono's kernel time after one warm-up run, and the spread.

    python tools/xj_bench.py [--lambdas 5,35] [--n2 2000] [--reps 3] [--observers 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcfost_amd.engine import Engine, McgpuError   # noqa: E402
from mcfost_amd.host import model as M        # noqa: E402

# name, radiation_field_sed, xj_where, xi_log, block_threads (0: the launcher's choice)
VARIANTS = (("off, default (xi_log 1)", 0, 0, 1, 0), ("off, atomics (xi_log 0)", 0, 0, 0, 0), ("on, HBM (xj_where 1)", 1, 1, 0, 0),
            ("on, LDS (xj_where 2)", 1, 2, 0, 0), ("on, LDS, 256 threads", 1, 2, 0, 256), ("on, HBM, 256 threads", 1, 1, 0, 256),
            ("on, LDS, 128 threads", 1, 2, 0, 128), ("on, automatic (xj_where 0)", 1, 0, 0, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lambdas", default="5,35")
    ap.add_argument("--n2", type=int, default=2000, help="packets in the stop bin per stream")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--observers", type=int, default=10)
    args = ap.parse_args()
    cfg = M.ref41()
    cfg.RT_n_incl = args.observers
    m = M.build_model(cfg)
    e = Engine(m, 5e6)
    T = e.temp_finale(e.run_thermal(5_000_000, seed=3)["E_abs"])
    e.close()
    out = {"n_cells": int(m.n_cells), "observers": args.observers, "n2": args.n2, "reps": args.reps, "wavelengths": {}}
    for lam in [int(x) for x in args.lambdas.split(",")]:
        rows = {}
        for name, bits, where, xi_log, bt in VARIANTS:
            e = Engine(m, 5e6)
            e.set_xI_precision(4)
            e.set_option("xi_log", xi_log)
            if bits:
                e.set_option("radiation_field_sed", bits)
                e.set_option("xj_where", where)
            td = e.repartition_energie(lam, T, fetch=False)
            ms, r = [], None
            try:
                for i in range(args.reps + 1):
                    r = e.run_mono(lam, args.n2, seed=100, n_chunks=m.cfg.n_photons_loop, fetch_xI=False, device_tables=td,
                                   block_threads=bt)
                    if i:
                        ms.append(r["kernel_ms"])
            except McgpuError as err:   # ("xj_where" = 2 where the row does not fit)
                print("lambda %2d  %-28s refused: %s" % (lam, name, str(err).split(": ", 1)[-1]), flush=True)
                rows[name] = {"refused": str(err)}
                e.close()
                continue
            rows[name] = {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
                          "packets": int(r["counters"]["packets"]), "crossings": int(r["counters"]["crossings"]),
                          "xj_lds": e.get_info("xj_lds") if bits else None,
                          "frac_E_stars": float(td["frac_E_stars"])}
            e.close()
            print("lambda %2d (%.3g um, frac_E_stars %.3f)  %-28s median %8.2f ms  [%8.2f, %8.2f]  %d packets, %.1f crossings each%s"
                  % (lam, m.lam[lam - 1], td["frac_E_stars"], name, rows[name]["median_ms"], rows[name]["min_ms"], rows[name]["max_ms"],
                     rows[name]["packets"], rows[name]["crossings"] / max(rows[name]["packets"], 1),
                     "" if not bits else ("  row in LDS" if rows[name]["xj_lds"] else "  row in HBM")), flush=True)
        out["wavelengths"][lam] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
