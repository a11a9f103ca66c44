"""Bit-exactness of the 2D crossing's flying-loop form, on the CPU.

tests/emu/emu_fly_step.cpp walks packets, crossing by crossing, through fly_step_2d<..., WAVE = true> (the flying waves'
form, with its caller's per-visit bookkeeping), fly_step_2d<..., WAVE = false> (serving waves, tail kernel, host tail)
and roles_cross<false, ...> (the retained exact path through cross_cell_lean), and reports the first field in which
they part.  The first two must agree in every field and deposit, bit for bit.  The third must agree in every
direction, state, index and counter, crossing by crossing, and it goes on from the flying form's point and extr after
each crossing: the wall point, the length and extr differ from it in their last bits (fly_step_2d forms x and y as one
multiply-add where cross_cell_lean rounds the product first), a difference HEAD's fly_step_2d already had on the same
walks -- the expected mapping.  roles_cross leaves a finished packet's indices as they were and keeps no cell index:
those are not compared.
Inputs: the reference's golden walks, random states on the Pascucci and ref4.1 grids, constructed edge states (the
hole, the midplane from zj = 1, above the top layer, a star's cell on the way, a stop inside a cell), with and
without dark cells."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mcfost_amd.host import model as M
from oracle import Oracle
from oracle.binding import _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_step.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_step.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished"]


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _model(name):
    from helpers import CONFIGS
    m = M.build_model(CONFIGS[name](M))
    return m


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def _states(m, name, rng):
    """(positions + directions, extr, star_key) of golden, random and constructed packets."""
    from helpers import load_golden
    g = load_golden(name)
    wk = g["walk"]
    r_lim = np.asarray(g["grid_r_lim"], float)
    zmax = np.asarray(g["grid_zmax"], float)
    n_rad, nz = len(zmax), int(round(len(g["grid_z_lim"]) / len(zmax))) - 2
    s = [wk[:, :6]]
    # random: anywhere in the disk (and a little beyond), uniform directions
    n = 3000
    r = rng.uniform(0.0, 1.05, n) ** 2 * r_lim[-1]
    ph = rng.uniform(0, 2 * np.pi, n)
    zm = np.interp(r, 0.5 * (r_lim[1:] + r_lim[:-1]), zmax)
    z = rng.uniform(-1.1, 1.1, n) * zm
    s.append(np.column_stack([r * np.cos(ph), r * np.sin(ph), z, _unit(rng, n)]))
    # constructed: in the hole; at the midplane heading for it from zj = 1; above the top layer; tiny |z|
    k = 400
    rh = rng.uniform(0.0, 0.99, k) * r_lim[0]
    s.append(np.column_stack([rh, np.zeros(k), rng.uniform(-1, 1, k) * zmax[0], _unit(rng, k)]))
    rr = rng.uniform(r_lim[0], r_lim[-1], k)
    zz = 1e-3 * np.interp(rr, 0.5 * (r_lim[1:] + r_lim[:-1]), zmax) / nz
    dd = _unit(rng, k)
    dd[:, 2] = -np.abs(dd[:, 2]) * np.sign(zz)
    s.append(np.column_stack([rr, np.zeros(k), zz, dd]))
    s.append(np.column_stack([rr, np.zeros(k), 1.2 * np.interp(rr, 0.5 * (r_lim[1:] + r_lim[:-1]), zmax), _unit(rng, k)]))
    s.append(np.column_stack([rr, np.zeros(k), np.full(k, 1e-14), _unit(rng, k)]))
    st = np.ascontiguousarray(np.vstack(s))
    n_all = st.shape[0]
    extr = rng.exponential(1.0, n_all)
    extr[: n_all // 3] = 1e30  # (a third never stops: long walks, out of the grid)
    star = np.full(n_all, -1, np.int32)
    pick = rng.random(n_all) < 0.3  # a star's cell somewhere on the way
    ri = rng.integers(0, n_rad + 1, n_all)
    zj = rng.integers(1, nz + 1, n_all)
    star[pick] = (ri + (n_rad + 2) * (zj + nz + 1))[pick]
    return st, extr, star


@pytest.mark.parametrize("name", ["pascucci", "ref41", "small2d"])
@pytest.mark.parametrize("dark_every", [0, 7])
def test_flying_form_is_bit_exact(emu, name, dark_every):
    m = _model(name)
    orc = Oracle(m, 1000)
    rng = np.random.default_rng(12345 + dark_every)
    st, extr, star = _states(m, name, rng)
    n = st.shape[0]
    steps, ab, ac = (np.zeros(n, np.int32) for _ in range(3))
    E = [np.zeros(m.n_cells + 1) for _ in range(3)]
    rc = emu.emu_fly_compare(C.byref(orc.cm), dark_every, n, _p(st, C.c_double), _p(extr, C.c_double),
                             _p(star, C.c_int), 100000, _p(steps, C.c_int), _p(ab, C.c_int), _p(ac, C.c_int),
                             *[_p(e, C.c_double) for e in E])
    assert rc == 0, rc
    assert steps.sum() > 5 * n  # (the walks test many crossings, not only the first)
    bad_ab = {FIELDS[f]: int((ab == f).sum()) for f in np.unique(ab) if f}
    bad_ac = {FIELDS[f]: int((ac == f).sum()) for f in np.unique(ac) if f}
    assert not bad_ab, bad_ab
    assert not bad_ac, bad_ac
    assert np.array_equal(E[0].view(np.int64), E[1].view(np.int64))
