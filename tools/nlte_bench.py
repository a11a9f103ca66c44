"""Cost of the grains out of LTE, measured: ref4.1 2D with 16 non-LTE grains (lonly_nLTE, live) against the same model as
LTE through the same single-role kernel with the xJ_abs accumulator on (option radiation_field = 2).

    python tools/nlte_bench.py [--packets 1e7] [--repeat 3] [--grains 16]

Prints one JSON line: packets/s of both (best of --repeat launches after one warm-up, device events around the kernel),
absorptions served per wave visit of the non-LTE launch, and the registers / scratch / LDS of the non-LTE kernel as the
library's code object states them.  Needs an MI355X; there is no fallback.

The alternative form of the event, one lane per event instead of the whole wave, is a tuning build:
    python __graft_entry__.py variant nlte_one_lane -DMCGPU_NLTE_ONE_LANE
    MCGPU_LIB=mcfost_amd/csrc/variants/nlte_one_lane.so python tools/nlte_bench.py"""
import argparse
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mcfost_amd import engine as eng          # noqa: E402
from mcfost_amd.host import model as M        # noqa: E402


def kernel_resources(lib, pattern):
    """{symbol: (vgprs, sgprs, scratch bytes / lane, static LDS bytes)} of the gfx950 kernels whose name matches"""
    data, out, pos = open(lib, "rb").read(), {}, 0
    readelf = shutil.which("llvm-readelf") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        raise SystemExit("nlte_bench: llvm-readelf not found (PATH, ROCM_PATH): the kernels' registers cannot be read")
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", pos)
        if i < 0:
            return out
        pos, o = i + 1, i + 32
        for _ in range(struct.unpack_from("<Q", data, i + 24)[0]):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if "gfx950" not in triple or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[i + off:i + off + size])
                f.flush()
                txt = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True).stdout
            for blk in txt.split(".agpr_count:")[1:]:
                sym = re.search(r"\.symbol:\s+(\S+)", blk).group(1)
                if re.search(pattern, sym):
                    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                    out[sym] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))


def best_rate(e, n, repeat, seed0):
    e.run_thermal(min(n, 1000000), seed=seed0)           # warm-up: code object, buffers
    ms = [e.run_thermal(n, seed=seed0 + 1 + r)["kernel_ms"] for r in range(repeat)]
    return n / (min(ms) * 1e-3), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=float, default=1e7)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--grains", type=int, default=16)
    a = ap.parse_args()
    n = int(a.packets)
    m = M.build_model(M.ref41())
    grains = M.synthetic_grains(m, a.grains)
    _, dens = M.settled_grain_density(m, grains, xi=0.0, per_cell=False, n_classes=1)
    nl = M.init_nlte(m, grains, dens, (1, a.grains))
    lte = eng.Engine(m, n)
    lte.set_option("radiation_field", 2)                 # the single-role kernel, xJ_abs on
    r_lte, ms_lte = best_rate(lte, n, a.repeat, 100)
    lte.close()
    e = eng.Engine(m, n)
    e.set_nlte(nl)
    e.set_J0(nl["J0"])
    e.set_option("nlte_stats", 1)
    r_nl, ms_nl = best_rate(e, n, a.repeat, 100)
    events, visits = e.get_info("nlte_events"), e.get_info("nlte_visits")
    e.close()
    res = kernel_resources(eng.LIB_PATH, r"k_thermal_nlteILb0E")      # the 2D instantiations
    print(json.dumps(dict(model="ref41 2D", packets=n, grains=a.grains, lte_xJ_packets_per_s=r_lte, nlte_packets_per_s=r_nl,
                          ratio=r_nl / r_lte, lte_ms=ms_lte, nlte_ms=ms_nl, events_per_wave_visit=events / max(visits, 1.0),
                          events_per_packet=events / n,
                          kernels={k: dict(vgprs=v[0], sgprs=v[1], scratch=v[2], lds_static=v[3]) for k, v in res.items()})))


if __name__ == "__main__":
    main()
