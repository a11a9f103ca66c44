"""Bit-exactness of the 2D crossing with the padded cell key, on the CPU.

tests/emu/emu_fly_pad.cpp walks packets, crossing by crossing, through fly_visit_step_2d<..., PAD = true> (the flying
waves' crossing, with the part of roles_body that keeps the per-visit counters), fly_step_2d<..., PAD = true> (the serving
waves') and fly_step_2d<..., PAD = false>, the specification.  After every crossing all three must agree, bit for bit, in
x, y, z, u, v, w, ri, zj, kf, st, pk_cross, in c_cross, c_kill, c_dark and finished, in the value of the deposit and --
while the packet is in flight -- in extr.  The padded key must be ri + (n_rad + 2) zj, the same in both padded forms, and
name the slot of the specification's cell, or a halo slot exactly where the specification says "no cell".
Inputs: the states of tests/test_fly_step_exact.py (golden walks, random states, the hole, the midplane from zj = 1, above
the top layer, a star's cell on the way, a stop inside a cell) and the packets ON a wall of tests/test_fly_visit_exact.py;
plain and with the walk's bit in the crossing counter, with and without dark cells.

And the pieces that go with the key: the padded copy of the opacities, the folds' way back from a padded slot to the
cell (grids whose slot count is no multiple of the waves of a workgroup), and sqrt_nonneg's zero case."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import Oracle
from oracle.binding import _p
from test_fly_step_exact import _model, _states
from test_fly_visit_exact import _on_wall

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_pad.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_pad.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished", "deposit", "key"]
AGAINST = {0: "", 1: " (serving form)", 2: " (specification)"}
VARIANTS = {"plain": 0, "mrw": 1}
_DELTAS = {}   # (name, variant, dark_every) -> (smallest, largest) positive discriminant of the walks


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    lib = C.CDLL(LIB)
    lib.emu_pad_layout.restype = None
    lib.emu_sqrt_zero_case.restype = None
    return lib


def _walk(emu, name, variant, dark_every):
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
    n_rad, nz = int(m.grid["n_rad"]), int(m.grid["nz"])
    n_pad = (n_rad + 2) * (nz + 2)
    EA, EB, EC = np.zeros(n_pad), np.zeros(n_pad), np.zeros(m.n_cells + 1)
    info = np.zeros(2, np.int32)
    delta = np.zeros(2)
    rc = emu.emu_fly_pad_compare(C.byref(orc.cm), dark_every, VARIANTS[variant], n, _p(st, C.c_double), _p(extr, C.c_double),
                                 _p(star, C.c_int), _p(fri, C.c_int), _p(fzj, C.c_int), 100000, _p(steps, C.c_int),
                                 _p(where, C.c_int), _p(EA, C.c_double), _p(EB, C.c_double), _p(EC, C.c_double),
                                 _p(info, C.c_int), _p(delta, C.c_double))
    assert rc == 0, rc
    _DELTAS[(name, variant, dark_every)] = (float(delta[0]), float(delta[1]))
    return m, n, steps, where, EA, EB, EC, info


@pytest.mark.parametrize("name,variant", [("pascucci", "plain"), ("ref41", "plain"), ("small2d", "plain"), ("small2d", "mrw")])
@pytest.mark.parametrize("dark_every", [0, 7])
def test_padded_forms_are_bit_exact(emu, name, variant, dark_every):
    m, n, steps, where, EA, EB, EC, info = _walk(emu, name, variant, dark_every)
    assert steps.sum() > 5 * n  # (the walks test many crossings, not only the first)
    bad = {FIELDS[f % 32] + AGAINST[f // 32]: int((where == f).sum()) for f in np.unique(where) if f}
    assert not bad, bad
    # the two padded grids are the same, and their real slots hold the specification's grid
    assert np.array_equal(EA.view(np.int64), EB.view(np.int64))
    n_rad, nz = int(m.grid["n_rad"]), int(m.grid["nz"])
    pad = EA.reshape(nz + 2, n_rad + 2)
    assert np.array_equal(pad[1:nz + 1, 1:n_rad + 1].ravel().view(np.int64), EC[:m.n_cells].view(np.int64))
    assert EC[:m.n_cells].sum() > 0 and EC[m.n_cells] == 0.0
    # the virtual cells were crossed, and what was deposited there lies in the halo
    assert info[0] > 0
    halo = pad.copy()
    halo[1:nz + 1, 1:n_rad + 1] = 0.0
    assert halo.sum() > 0
    assert (info[1] > 0) == (dark_every > 0), info


@pytest.mark.parametrize("n_rad,nz", [(13, 5), (20, 10), (100, 70), (1, 1)])
def test_padded_table_and_the_way_back(emu, n_rad, nz):
    rng = np.random.default_rng(n_rad * 1000 + nz)
    plain = rng.uniform(1.0, 2.0, n_rad * nz)
    n_pad = (n_rad + 2) * (nz + 2)
    padded = np.full(n_pad, -1.0)
    cell = np.full(n_pad, -7, np.int32)
    emu.emu_pad_layout(n_rad, nz, _p(plain, C.c_double), _p(padded, C.c_double), _p(cell, C.c_int))
    # the padded table against the plain one for every (ri, zj), halo included (cell (ri, zj) is entry ri - 1 + n_rad (zj - 1))
    want = np.zeros((nz + 2, n_rad + 2))
    want[1:nz + 1, 1:n_rad + 1] = plain.reshape(nz, n_rad)
    assert np.array_equal(padded.reshape(nz + 2, n_rad + 2), want)
    want_cell = np.full((nz + 2, n_rad + 2), -1, np.int32)
    want_cell[1:nz + 1, 1:n_rad + 1] = np.arange(n_rad * nz, dtype=np.int32).reshape(nz, n_rad)
    assert np.array_equal(cell.reshape(nz + 2, n_rad + 2), want_cell)
    # the folds: every real slot is folded exactly once per round of slices and no halo slot ever, whatever the number of
    # waves (row counts that are no multiple of it included), and the real slots arrive at their cells
    E_pad = rng.uniform(1.0, 2.0, n_pad)
    for n_waves in (1, 3, 7, 16):
        E_out = np.zeros(n_rad * nz)
        visits = np.zeros(n_pad, np.int32)
        folded = emu.emu_pad_fold(n_rad, nz, n_waves, _p(E_pad, C.c_double), _p(E_out, C.c_double), _p(visits, C.c_int))
        assert folded == n_rad * nz
        assert np.array_equal(visits, (want_cell.ravel() >= 0).astype(np.int32))
        assert np.array_equal(E_out, E_pad.reshape(nz + 2, n_rad + 2)[1:nz + 1, 1:n_rad + 1].ravel())


def test_sqrt_zero_case(emu):
    """sqrt_nonneg's zero case as one maximum against the select it replaces: the same bits on 0, on the smallest and the
    largest discriminant of the golden walks and on random positive values."""
    if not _DELTAS:
        for name in ("pascucci", "ref41", "small2d"):
            _walk(emu, name, "plain", 0)
    ends = [d for pair in _DELTAS.values() for d in pair]
    assert min(ends) > 0.0 and max(ends) < 1e300
    rng = np.random.default_rng(7)
    x = np.concatenate([[0.0, -0.0], ends, [min(ends), max(ends)], 10.0 ** rng.uniform(-20, 20, 100000)])
    a, b = np.zeros_like(x), np.zeros_like(x)
    emu.emu_sqrt_zero_case(len(x), _p(x, C.c_double), _p(a, C.c_double), _p(b, C.c_double))
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert a[0] == 0.0 and not np.signbit(a[0]) and not np.signbit(b[1])
    assert np.all(np.abs(a[2:] - np.sqrt(x[2:])) <= 2e-16 * np.sqrt(x[2:]))
