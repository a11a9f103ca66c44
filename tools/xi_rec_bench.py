#!/usr/bin/env python3
"""A/B of the SED commit pass's deposit paths on ref4.1 as ref4.1.para runs it (3 inclinations, no Stokes tracking in the
deposits, N_type_flux = 5): option "xi_log" = 0 (default-real atomics in the packed layout) against 3 (16-byte records in
the binned log, mc_xirec.hip.h) on the same build, alternating, at the three wavelengths the earlier A/Bs used (0.3, 1 and
60 um).  Every stream runs to a fixed packet count (n_phot_lim), so a call is one commit pass and nothing is scouted.
Reports per run the pass's time on the stream, packets and records per second, the folds' time and the overflow and drain
counts, then per wavelength the median and the spread of each option.  Not the benchmark (bench.py is).
Usage: python tools/xi_rec_bench.py [--packets-per-stream 100000] [--runs 5] [--log-mb 0] [--buckets 0] [--fold-kb 0]"""
import argparse, dataclasses, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mcfost_amd.engine import Engine
from mcfost_amd.host import model as M

ap = argparse.ArgumentParser()
ap.add_argument("--packets-per-stream", type=int, default=100000, help="x 128 streams per wavelength")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--wavelengths", default="0.3,1,60", help="in um: the nearest of the model's")
ap.add_argument("--log-mb", type=int, default=0)
ap.add_argument("--buckets", type=int, default=0)
ap.add_argument("--fold-kb", type=int, default=0)
a = ap.parse_args()

cfg = dataclasses.replace(M.ref41(), RT_n_incl=3, lsepar_pola=False)
m = M.build_model(cfg)
e = Engine(m, 5e6)
T = e.temp_finale(e.run_thermal(5_000_000, seed=3)["E_abs"])
M.repartition_energie(m, T)
e.close()
# (a context per option: leaving "xi_log" = 3 frees the record log, and its allocation is not part of a pass)
engines = {}
for opt in (0, 3):
    e = engines[opt] = Engine(m, 5e6)
    e.set_rt1()
    e.set_xI_precision(4)
    for name, value in (("xi_log", opt), ("xi_rec_log_mb", a.log_mb), ("xi_rec_buckets", a.buckets), ("xi_rec_fold_kb", a.fold_kb)):
        e.set_option(name, value)
INFO = ("records", "chunks", "folded", "drained", "overflow_blocks", "buckets", "split", "fold_ms", "log_bytes")


def one(lam, opt, seed):
    e = engines[opt]
    t = time.perf_counter()
    r = e.run_mono(lam, 10 ** 12, n_phot_lim=float(a.packets_per_stream), seed=seed, fetch_xI=False)
    wall = time.perf_counter() - t
    c = r["counters"]
    out = dict(lam=lam, wl_um=float(m.lam[lam - 1]), xi_log=opt, packets=c["packets"], crossings=c["crossings"], stream_ms=r["kernel_ms"],
               wall_s=wall, packets_per_s=c["packets"] / (1e-3 * r["kernel_ms"]))
    if opt == 3:
        out.update({k: e.get_info("xi_rec_" + k) for k in INFO})
        out["records_per_s"] = out["records"] / (1e-3 * r["kernel_ms"])
        out["fold_share"] = out["fold_ms"] / r["kernel_ms"]
        out["fold_bytes_read"] = 16.0 * out["folded"] * out["split"]
    return out


for wl in [float(x) for x in a.wavelengths.split(",")]:
    lam = int(np.argmin(np.abs(np.log(np.asarray(m.lam) / wl)))) + 1
    for opt in (0, 3):
        one(lam, opt, 1)          # (module load, the log's allocation)
    ms = {0: [], 3: []}
    for k in range(a.runs):
        for opt in (0, 3):
            r = one(lam, opt, 2)
            ms[opt].append(r["stream_ms"])
            print(json.dumps(r))
    med = {o: float(np.median(v)) for o, v in ms.items()}
    print(json.dumps(dict(summary=True, lam=lam, wl_um=float(m.lam[lam - 1]), runs=a.runs,
                          atomics_ms=dict(median=med[0], min=min(ms[0]), max=max(ms[0])),
                          record_log_ms=dict(median=med[3], min=min(ms[3]), max=max(ms[3])),
                          record_log_over_atomics=med[3] / med[0])))
for e in engines.values():
    e.close()
