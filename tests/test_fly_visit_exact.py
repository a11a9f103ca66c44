"""Bit-exactness of the flying loop's crossing under the flight predicate, on the CPU.

tests/emu/emu_fly_visit.cpp walks packets, crossing by crossing, through fly_visit_step_2d (the flying waves' crossing,
with the part of roles_body that keeps the per-visit counters) and through
fly_step_2d<..., WAVE = false>, its specification.  After every crossing they must agree, bit for bit, in x, y, z, u, v,
w, ri, zj, ic, kf, st, pk_cross (VAR: also kab), in the cell and value of the deposit, in c_cross, c_kill, c_dark and
finished, and -- while the packet is still in flight -- in extr (fly_step_2d also subtracts from the extr of a packet
that does not fly; nothing reads that value).
Inputs: the states of tests/test_fly_step_exact.py (golden walks, random states, the hole, the midplane from zj = 1, above
the top layer, a star's cell on the way, a stop inside a cell) and packets put ON a wall so that each of the three
rounding-level fix-ups (s1 == 0, t < 0, z1 == 0 -> grid_prec) applies, and the test asserts that each of them did."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import Oracle
from oracle.binding import _p
from test_fly_step_exact import _model, _states

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_visit.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_visit.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished", "kab", "deposit"]
VARIANTS = {"plain": 0, "mrw": 1, "var": 2}


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _on_wall(name, rng):
    """Packets on a wall, on the side that only rounding reaches (the indices are set, not looked up): (states, ri, zj)."""
    from helpers import load_golden
    g = load_golden(name)
    r_lim = np.asarray(g["grid_r_lim"], float)
    zmax = np.asarray(g["grid_zmax"], float)
    n_rad, nz = len(zmax), int(round(len(g["grid_z_lim"]) / len(zmax))) - 2
    k = 60
    s, fri, fzj = [], [], []
    # s1 == 0: a hair outside the outer wall of cell ri, moving along the tangent (x u + y v = 0 exactly)
    ri = rng.integers(1, n_rad + 1, k)
    th = rng.uniform(0.1, np.pi - 0.1, k)
    z = rng.uniform(0.05, 0.9, k) * zmax[ri - 1]
    s.append(np.column_stack([r_lim[ri] * (1 + 4e-14), np.zeros(k), z, np.zeros(k), np.sin(th), np.cos(th)]))
    fri.append(ri)
    fzj.append(np.minimum((z / (zmax[ri - 1] / nz)).astype(int) + 1, nz))
    # t < 0: a hair below the lower wall of layer zj, moving down
    ri = rng.integers(1, n_rad + 1, k)
    zj = rng.integers(2, nz + 1, k)
    r = rng.uniform(0.3, 0.7, k) * (r_lim[ri] - r_lim[ri - 1]) + r_lim[ri - 1]
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[:, 2] = -np.abs(d[:, 2]) - 1e-3
    d /= np.linalg.norm(d, axis=1)[:, None]
    s.append(np.column_stack([r, np.zeros(k), (zj - 1) * (zmax[ri - 1] / nz) * (1 - 1e-13), d]))
    fri.append(ri)
    fzj.append(zj)
    # z1 == 0: in the midplane, moving in it
    ri = rng.integers(1, n_rad + 1, k)
    r = rng.uniform(0.3, 0.7, k) * (r_lim[ri] - r_lim[ri - 1]) + r_lim[ri - 1]
    ph = rng.uniform(0, 2 * np.pi, k)
    s.append(np.column_stack([r, np.zeros(k), np.zeros(k), np.cos(ph), np.sin(ph), np.zeros(k)]))
    fri.append(np.full(k, -1))
    fzj.append(np.full(k, -1))
    return np.vstack(s), np.concatenate(fri).astype(np.int32), np.concatenate(fzj).astype(np.int32)


@pytest.mark.parametrize("name,variant", [("pascucci", "plain"), ("ref41", "plain"), ("small2d", "plain"),
                                          ("small2d", "mrw"), ("ref41", "var")])
@pytest.mark.parametrize("dark_every", [0, 7])
def test_visit_form_is_bit_exact(emu, name, variant, dark_every):
    m = _model(name)
    orc = Oracle(m, 1000)
    rng = np.random.default_rng(12345 + dark_every)
    st, extr, star = _states(m, name, rng)
    n0 = st.shape[0]
    ws, wri, wzj = _on_wall(name, rng)
    nw = ws.shape[0]
    st = np.ascontiguousarray(np.vstack([st, ws]))
    extr = np.concatenate([extr, np.full(nw, 1e30)])
    star = np.concatenate([star, np.full(nw, -1, np.int32)]).astype(np.int32)
    fri = np.concatenate([np.full(n0, -1, np.int32), wri]).astype(np.int32)
    fzj = np.concatenate([np.full(n0, -1, np.int32), wzj]).astype(np.int32)
    n = st.shape[0]
    steps, where = (np.zeros(n, np.int32) for _ in range(2))
    fixes = np.zeros((n, 3), np.int32)
    E = [np.zeros(m.n_cells + 1) for _ in range(2)]
    rc = emu.emu_fly_visit_compare(C.byref(orc.cm), dark_every, VARIANTS[variant], n, _p(st, C.c_double), _p(extr, C.c_double),
                                   _p(star, C.c_int), _p(fri, C.c_int), _p(fzj, C.c_int), 100000, _p(steps, C.c_int),
                                   _p(where, C.c_int), _p(fixes, C.c_int), *[_p(e, C.c_double) for e in E])
    assert rc == 0, rc
    assert steps.sum() > 5 * n  # (the walks test many crossings, not only the first)
    bad = {FIELDS[f]: int((where == f).sum()) for f in np.unique(where) if f}
    assert not bad, bad
    assert np.array_equal(E[0].view(np.int64), E[1].view(np.int64))
    assert E[0].sum() > 0
    # each fix-up applied: at the first crossing of the packets made for it ...
    k = nw // 3
    for i, what in enumerate(("s1 == 0", "t < 0", "z1 == 0")):
        assert fixes[n0 + i * k: n0 + (i + 1) * k, i].sum() >= k // 2, (what, fixes[n0:].sum(axis=0))
    # ... and how often on every other walk (for the record: they stay selects of the common path)
    print("fix-ups on %d crossings of golden, random and edge states: %s" % (steps[:n0].sum(), fixes[:n0].sum(axis=0)))
