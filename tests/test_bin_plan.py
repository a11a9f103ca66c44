"""The region plans of the deposit logs (k_plan_uniform / k_plan_bins, mcfost_amd/csrc/mc_binned.hip.h) on the CPU, one
emulated lane: whatever the last launch counted, however the next launch's workgroup count and size differ from the
last one's and however small or large the log is, the regions lie in order, do not overlap, end inside the log, every
bucket gets room where the log has more than is wanted, and the counts are cleared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mcfost_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "emu", "emu_plan.cpp")
    so = os.path.join(HERE, "emu", "libemu_plan.so")
    deps = [src, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, h) for h in ("mc_binned.hip.h", "mc_device.hip.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    l = C.CDLL(so)
    l.emu_plan_uniform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_ulonglong, C.c_int]
    l.emu_plan_uniform.restype = None
    l.emu_plan_bins.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_double, C.c_int, C.c_void_p]
    l.emu_plan_bins.restype = None
    return l


def check_regions(off, cap, n_parts, total_blocks, what):
    """the properties a launch relies on: its workgroup `p` writes the blocks [off[b] + cap[b] p, ... + cap[b]) of bucket b"""
    off, cap = off.astype(np.uint64), cap.astype(np.uint64)
    end = off + cap * np.uint64(n_parts)
    assert np.all(np.diff(off.astype(np.int64)) >= 0), what
    assert np.all(end[:-1] <= off[1:]), what
    assert int(end[-1]) <= total_blocks, what


def random_total(rng, typical):
    """a log from nothing to the largest one (block indices are 32-bit), and sizes around what the case wants"""
    kind = rng.integers(0, 6)
    if kind == 0:
        return int(rng.integers(0, 64))
    if kind == 1:
        return 2 ** 32 - 1 - int(rng.integers(0, 3))
    if kind == 2:
        return int(rng.integers(0, 2 ** 32))
    return int(min(2 ** 32 - 1, typical * rng.uniform(0.05, 4.0)))


def test_uniform_plan(lib):
    rng = np.random.default_rng(3)
    for case in range(300):
        nb, n_parts = int(rng.integers(1, 97)), int(rng.integers(1, 301))
        total = random_total(rng, nb * n_parts * 10)
        off, cap = np.full(nb, 0xDEADBEEF, np.uint32), np.full(nb, 0xDEADBEEF, np.uint32)
        lib.emu_plan_uniform(off.ctypes.data, cap.ctypes.data, nb, total, n_parts)
        what = (case, nb, n_parts, total)
        check_regions(off, cap, n_parts, total, what)
        assert np.all(cap == total // nb // n_parts), what          # the log split evenly, whole blocks per workgroup
        assert np.array_equal(off.astype(np.uint64), np.arange(nb, dtype=np.uint64) * np.uint64((total // nb // n_parts) * n_parts)), what


def test_plan_from_the_last_launch_counts(lib):
    rng = np.random.default_rng(4)
    n_roomy = n_cut = 0
    for case in range(500):
        nb, n_parts, n_next = int(rng.integers(1, 97)), int(rng.integers(1, 301)), int(rng.integers(1, 301))
        growth = float(10.0 ** rng.uniform(-2.0, 2.0))
        scale = (0, 3, 200, 10 ** 5, 2 ** 32 - 1)[int(rng.integers(0, 5))]
        count = rng.integers(0, scale + 1, (nb, n_parts)).astype(np.uint32)
        count[rng.random(nb) < 0.3] = 0                                  # buckets the last launch never used
        n = count.astype(np.uint64).sum(axis=1).astype(np.float64)
        wants = n * growth * 1.5 + 8.0 * n_next                           # (the plan's own rule)
        total = random_total(rng, float(wants.sum()))
        off, cap = np.full(nb, 0xDEADBEEF, np.uint32), np.full(nb, 0xDEADBEEF, np.uint32)
        want = np.zeros(nb)
        lib.emu_plan_bins(count.ctypes.data, nb, n_parts, off.ctypes.data, cap.ctypes.data, total, growth, n_next, want.ctypes.data)
        what = (case, nb, n_parts, n_next, growth, scale, total)
        check_regions(off, cap, n_next, total, what)
        assert not count.any(), what                                      # cleared for the next launch
        # (two roundings here, one or two in the plan, whichever way its compiler contracts the multiply-add)
        assert np.allclose(want, wants, rtol=1e-15, atol=0.0), what
        wanted = 0.0
        for w in want:                                                    # (summed in the plan's order)
            wanted += w
        if total > wanted:
            n_roomy += 1
            assert np.all(cap > 0), what
            # nothing is cut: every workgroup gets its share of what is wanted, the floor of 8 blocks included
            assert np.array_equal(cap.astype(np.uint64), np.floor(want).astype(np.uint64) // np.uint64(n_next)), what
            assert np.all(cap >= 8), what
        else:
            n_cut += 1
    assert n_roomy > 100 and n_cut > 100
