"""The record log of the SED commit pass (option "xi_log" = 3, mcfost_amd/csrc/mc_xirec.hip.h) on the CPU: the one
placement function puts every value of a record where xi32_offset puts the flux type that deposit reaches, the path
applies exactly where a crossing adds at most three default reals, and the fold -- compiled for one emulated lane -- sums a
log laid out as the transport kernel lays it out (blocks in per-workgroup parts of per-bucket regions)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mcfost_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "emu", "emu_xirec.cpp")
    so = os.path.join(HERE, "emu", "libemu_xirec.so")
    deps = [src, os.path.join(CSRC, "mc_xirec.hip.h"), os.path.join(CSRC, "mc_xi32.hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    l = C.CDLL(so)
    for f in ("values", "applies", "slots", "binf"):
        getattr(l, "xirec_probe_" + f).argtypes = [C.c_int] * 3
    l.xirec_probe_offset.argtypes = [C.c_int] * 5
    l.xirec_probe_xi32_offset.argtypes = [C.c_int] * 5
    l.emu_fold_xirec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                 C.c_int, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    return l


@pytest.fixture(scope="module")
def stage_lib():
    """the staging protocol (mc_binned.hip.h) instantiated for the 16-byte record, one emulated lane"""
    src = os.path.join(HERE, "emu", "emu_xirec_stage.cpp")
    so = os.path.join(HERE, "emu", "libemu_xirec_stage.so")
    deps = [src, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, h) for h in
            ("mc_xirec.hip.h", "mc_xi32.hip.h", "mc_binned.hip.h", "mc_device.hip.h", "mc_mono.hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", so, src])
    l = C.CDLL(so)
    l.emu_xirec_stage_and_fold.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong,
                                           C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    return l


def test_placement_and_where_the_path_applies(lib):
    from mcfost_amd.engine import xi32_layout
    covered = set()
    for nRT in range(1, 13):
        for pola in (False, True):
            for contrib in (False, True):
                nS = 4 if pola else 1
                V = lib.xirec_probe_values(nRT, pola, contrib)
                lay = xi32_layout(nRT, pola, contrib)
                # V as the issue defines it: nRT (nA + 1) with contributions (nA = n_Stokes - 1), nRT n_Stokes without
                assert V == nRT * nS == lay["record_values"]
                assert bool(lib.xirec_probe_applies(nRT, pola, contrib)) == (V <= 3) == lay["record_log"], (nRT, pola, contrib)
                if V > 3:
                    continue
                covered.add((nRT, contrib))
                assert lib.xirec_probe_slots(nRT, pola, contrib) == (2 * nRT if contrib else nRT)
                places = set()
                for star in (True, False):
                    for q in range(V):    # (no Stokes tracking here: value q is observer q's flux)
                        # the flux type that deposit reaches: I, or with contributions the packet's origin (n_Stokes + 2 / + 4, 1-based)
                        t = (nS + 1 if star else nS + 3) if contrib else 0
                        o = lib.xirec_probe_offset(nRT, pola, contrib, star, q)
                        assert o == lib.xirec_probe_xi32_offset(nRT, pola, contrib, q, t) and 0 <= o < lay["binf"]
                        places.add(o)
                assert len(places) == (2 * nRT if contrib else nRT)
    assert covered == {(n, c) for n in (1, 2, 3) for c in (False, True)}
    for nRT, pola, contrib in ((1, True, True), (4, False, True), (10, True, True)):
        assert xi32_layout(nRT, pola, contrib)["record_log"] is False
        assert not lib.xirec_probe_applies(nRT, pola, contrib)


@pytest.mark.parametrize("shift,n_buckets", [(13, 4), (12, 5)])
def test_fold_of_a_log_in_regions(lib, shift, n_buckets):
    """2e5 random records over 18 000 sub-bins as full blocks of 64 in the parts (3 workgroups, uneven) of the buckets'
    regions, one part cut at its cap; split = 3.  (18 000 sub-bins in power-of-two buckets are 3 buckets of 8192 or 5 of
    4096: the four-bucket layout has an empty fourth region, the five-bucket one none.)  Every accumulator is a
    default-real sum of <= ~30 positive terms: rtol 1e-5 against float64 sums."""
    rng = np.random.default_rng(11)
    n_sub, n_rec, n_parts, nRT, contrib = 18000, 200000, 3, 3, True
    binf = lib.xirec_probe_binf(nRT, False, contrib)
    sub = rng.integers(0, n_sub, n_rec).astype(np.uint32)
    star = rng.random(n_rec) < 0.4
    val = rng.uniform(0.1, 1.0, (n_rec, 3)).astype(np.float32)
    part = rng.choice(n_parts, n_rec, p=(0.6, 0.3, 0.1))
    bucket = sub >> shift
    assert bucket.max() < n_buckets
    rec_t = np.dtype([("key", "<u4"), ("v", "<f4", (3,))])
    assert rec_t.itemsize == 16
    count = np.zeros((n_buckets, n_parts), np.uint32)
    for b in range(n_buckets):
        for p in range(n_parts):
            count[b, p] = np.count_nonzero((bucket == b) & (part == p)) // 64     # (the rest stays in the staging: drained)
    cap = count.max(axis=1).astype(np.uint32)
    cap[1] = np.sort(count[1])[-2]                      # bucket 1: its largest part is cut at the cap
    assert count[1].max() > cap[1] > 0
    off = np.concatenate(([0], np.cumsum(cap.astype(np.uint64) * n_parts)[:-1])).astype(np.uint32)
    total_blocks = int((cap.astype(np.uint64) * n_parts).sum())
    log = np.zeros(total_blocks * 64, rec_t)
    log["key"] = 0x7FFFFFFF                              # (what a region holds behind its blocks must never be read)
    log["v"] = 1e30
    x0 = rng.uniform(0.0, 1.0, (n_sub, binf)).astype(np.float32)
    want = x0.astype(np.float64)
    n_in = 0
    for b in range(n_buckets):
        for p in range(n_parts):
            idx = np.flatnonzero((bucket == b) & (part == p))
            n_blk = min(int(count[b, p]), int(cap[b]))         # records beyond the cap are not in the log
            idx = idx[:n_blk * 64]
            at = (int(off[b]) + int(cap[b]) * p) * 64
            log["key"][at:at + idx.size] = sub[idx] | (star[idx].astype(np.uint32) << 31)
            log["v"][at:at + idx.size] = val[idx]
            n_in += idx.size
            for q in range(nRT):
                o = np.where(star[idx], lib.xirec_probe_offset(nRT, 0, contrib, 1, q), lib.xirec_probe_offset(nRT, 0, contrib, 0, q))
                np.add.at(want, (sub[idx], o), val[idx, q].astype(np.float64))
    slice_sub = ((1 << shift) + 2) // 3
    split = ((1 << shift) + slice_sub - 1) // slice_sub
    assert split == 3
    x = x0.copy()
    stats = np.zeros(4, np.uint64)
    count_before = count.copy()
    rc = lib.emu_fold_xirec(log.ctypes.data, count.ctypes.data, off.ctypes.data, cap.ctypes.data, n_buckets, shift, n_parts,
                            x.ctypes.data, nRT, int(contrib), n_sub, slice_sub, split, stats.ctypes.data)
    assert rc == 0
    assert int(stats[2]) == n_in and n_in < n_rec and np.array_equal(count, count_before)
    assert np.allclose(x.astype(np.float64), want, rtol=1e-5, atol=0.0)
    assert np.count_nonzero(want != x0) > 0.9 * n_sub


@pytest.mark.parametrize("nRT,contrib", [(3, True), (2, False), (1, True)])
def test_staging_of_records_one_lane(lib, stage_lib, nRT, contrib):
    """The transport side's road for a record, by one emulated lane: bin_deposit / bin_settle / bin_drain instantiated for
    the 16-byte record (no key arrays), regions planned by k_plan_uniform for 3 workgroups that make 60 / 30 / 10 % of the
    records -- the first one's parts overflow --, then the fold.  Every record arrives exactly once, by exactly one of the
    three ways, whichever it takes."""
    rng = np.random.default_rng(5)
    n_sub, n, n_parts, shift, n_buckets = 18000, 60000, 3, 12, 5
    binf = lib.xirec_probe_binf(nRT, False, contrib)
    sub = rng.integers(0, n_sub, n).astype(np.uint32)
    star = rng.random(n) < 0.4
    val = np.zeros((n, 3), np.float32)
    val[:, :nRT] = rng.uniform(0.1, 1.0, (n, nRT))
    part = rng.choice(n_parts, n, p=(0.6, 0.3, 0.1)).astype(np.int32)
    keys = (sub | (star.astype(np.uint32) << 31)).astype(np.uint32)
    total_blocks = n_buckets * n_parts * 64          # 64 blocks per part: ~128 wanted by workgroup 0, ~64 by 1, ~21 by 2
    slice_sub = ((1 << shift) + 2) // 3
    x = np.zeros((n_sub, binf), np.float32)
    stats = np.zeros(4, np.uint64)
    rc = stage_lib.emu_xirec_stage_and_fold(n, keys.ctypes.data, val.ctypes.data, part.ctypes.data, n_parts, n_buckets, shift,
                                            total_blocks, x.ctypes.data, nRT, int(contrib), n_sub, slice_sub, 3, stats.ctypes.data)
    assert rc == 0
    over, drained, folded, made = (int(v) for v in stats)
    assert made == n == folded + drained + 64 * over
    assert over > 0 and folded > 0 and 0 < drained <= 63 * n_buckets * n_parts
    want = np.zeros((n_sub, binf))
    for q in range(nRT):
        o = np.where(star, lib.xirec_probe_offset(nRT, 0, contrib, 1, q), lib.xirec_probe_offset(nRT, 0, contrib, 0, q))
        np.add.at(want, (sub, o), val[:, q].astype(np.float64))
    assert np.allclose(x.astype(np.float64), want, rtol=1e-5, atol=0.0)
