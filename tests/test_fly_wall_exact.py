"""Bit-exactness of the wall records of the padded 2D role kernels (WallRec, mc_roles.hip.h), on the CPU.

The flying waves' crossing no longer forms the vertical wall ahead: the wall travels with the flight, loaded with the
kappa_factor of the cell from one 32-byte record per padded cell.  tests/emu/emu_fly_wall.cpp checks both halves:

  * the table, as the library's builders make it, entry for entry against section 2 of fly_step_2d evaluated at every padded
    (ri, zj) a crossing can reach -- the hole, the outside column and the row above the disk included -- in both directions
    and on both sides of the midplane, bit for bit; every entry of the table, the unreachable row zj = 0 too, is finite, the
    factors are the padded kappa_factor, and the records start on a 32-byte boundary;
  * the crossings: packets walked through fly_visit_step_2d<..., PAD, WALL> and through fly_step_2d<..., PAD = false>, the
    specification, side by side.  After every crossing they agree, bit for bit, in x, y, z, u, v, w, ri, zj, kf, st,
    pk_cross, in c_cross, c_kill, c_dark and finished, in the value of the deposit and -- while the packet flies -- in extr;
    the key is the padding of the specification's index; and before every crossing the wall the flight carries is its cell's
    record for the direction that crossing finds.
Inputs: the states of tests/test_fly_step_exact.py (golden, random, edge) and the packets ON a wall of
tests/test_fly_visit_exact.py, so that each of the three fix-ups fires, and states made for the corners of section 2:
through the midplane from zj = 1, up out of layer nz and on in the row nz + 1, in the hole, w = 0 and dz == 0, and flights
that start at z = -0.0 and z = +0.0.  Plain, with the walk's bit in the crossing counter, with and without dark cells (the
kernels use the form where there is no dark zone; the form itself is exact with the mirror too)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import Oracle
from oracle.binding import _p
from test_fly_step_exact import _model, _states, _unit
from test_fly_visit_exact import _on_wall

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_wall.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_wall.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished", "deposit", "key", "carried wall"]
VARIANTS = {"plain": 0, "mrw": 1}
CORNERS = ["through the midplane", "up out of layer nz", "in the row nz + 1", "in the hole", "dz == 0", "w == 0",
           "z0 = -0.0", "z0 = +0.0"]


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _grid(n_rad, nz):
    """Columns of a flared disk: zmax grows outwards, the cell height is zmax / nz as the library requires."""
    if (n_rad, nz) == (100, 70):
        from mcfost_amd.host import model as M
        m = M.build_model(M.pascucci())
        zmax = np.asarray(m.grid["zmax"], np.float64)
        z_lim = np.asarray(m.grid["z_lim"], np.float64).ravel()
        assert len(zmax) == n_rad and int(m.grid["nz"]) == nz
        return z_lim[n_rad:2 * n_rad].copy(), zmax.copy()   # (z_lim(i, 2): what mcgpu_set_grid_cyl takes as the cell height)
    rng = np.random.default_rng(100 * n_rad + nz)
    zmax = np.cumsum(rng.uniform(0.5, 3.0, n_rad))
    return zmax / nz, zmax


@pytest.mark.parametrize("n_rad,nz", [(20, 10), (13, 5), (100, 70)])
def test_wall_table(emu, n_rad, nz):
    ch, zmax = _grid(n_rad, nz)
    rng = np.random.default_rng(n_rad + nz)
    kf = rng.uniform(1.0, 2.0, n_rad * nz)
    n_pad = (n_rad + 2) * (nz + 2)
    rec = np.full((n_pad, 4), np.nan)
    spec, used = np.zeros((n_pad, 4)), np.zeros((n_pad, 4))
    rc = emu.emu_wall_table(n_rad, nz, _p(ch, C.c_double), _p(zmax, C.c_double), _p(kf, C.c_double), _p(rec, C.c_double),
                            _p(spec, C.c_double), _p(used, C.c_double))
    assert rc == 0
    assert np.all(np.isfinite(rec))
    # what a crossing gets from the record is the specification's wall, in both directions and on both sides of the midplane
    assert np.array_equal(used.view(np.int64), spec.view(np.int64))
    r = rec.reshape(nz + 2, n_rad + 2, 4)
    s = spec.reshape(nz + 2, n_rad + 2, 4)
    assert np.array_equal(r[1:, :, 0].view(np.int64), s[1:, :, 0].view(np.int64))   # z_dn: away = false, z0 > 0
    assert np.array_equal(r[1:, :, 2].view(np.int64), s[1:, :, 2].view(np.int64))   # z_up: away = true, z0 > 0
    # the corners: the mirror's sign in the row zj = 1 and nowhere else, 1e10 above the disk, the hole and the outside column
    # as the columns next to them
    assert np.all(r[1, :, 0] < 0.0) and np.all(r[2:, :, 0] > 0.0) and np.all(r[1:, :, 2] > 0.0)
    assert np.all(r[nz + 1, :, 2] == 1.0e10) and np.all(r[1:nz + 1, :, 2] < 1.0e10)
    assert np.array_equal(r[:, 0, [0, 2]], r[:, 1, [0, 2]]) and np.array_equal(r[:, n_rad + 1, [0, 2]], r[:, n_rad, [0, 2]])
    assert np.all(r[0] == 0.0)
    # the factors: the padded kappa_factor in both halves of a record, 0 in the halo
    want = np.zeros((nz + 2, n_rad + 2))
    want[1:nz + 1, 1:n_rad + 1] = kf.reshape(nz, n_rad)
    assert np.array_equal(r[:, :, 1], want) and np.array_equal(r[:, :, 3], want)


def _corners(name, rng):
    """States for the corners of section 2: (states, ri, zj); ri / zj = -1: looked up."""
    from helpers import load_golden
    g = load_golden(name)
    r_lim = np.asarray(g["grid_r_lim"], float)
    zmax = np.asarray(g["grid_zmax"], float)
    n_rad, nz = len(zmax), int(round(len(g["grid_z_lim"]) / len(zmax))) - 2
    k = 80
    mid = 0.5 * (r_lim[1:] + r_lim[:-1])
    s = []

    def radii():
        return rng.uniform(r_lim[0], r_lim[-1], k)

    # through the midplane from zj = 1: steeply down (up on the mirror side), so that the vertical wall is the nearest
    for sign in (1.0, -1.0):
        rr = radii()
        d = _unit(rng, k)
        d[:, 2] = -sign * (np.abs(d[:, 2]) + 2.0)
        d /= np.linalg.norm(d, axis=1)[:, None]
        s.append(np.column_stack([rr, np.zeros(k), sign * rng.uniform(0.05, 0.9, k) * np.interp(rr, mid, zmax) / nz, d]))
    # up out of layer nz, then on in the row nz + 1
    for sign in (1.0, -1.0):
        rr = radii()
        d = _unit(rng, k)
        d[:, 2] = sign * (np.abs(d[:, 2]) + 2.0)
        d /= np.linalg.norm(d, axis=1)[:, None]
        s.append(np.column_stack([rr, np.zeros(k), sign * (1.0 - rng.uniform(0.05, 0.9, k) / nz) * np.interp(rr, mid, zmax), d]))
    # in the row nz + 1, coming down again / flying along
    rr = radii()
    s.append(np.column_stack([rr, np.zeros(k), rng.choice([-1.0, 1.0], k) * 1.05 * np.interp(rr, mid, zmax), _unit(rng, k)]))
    # in the hole, at every height
    rh = rng.uniform(0.0, 0.99, k) * r_lim[0]
    ph = rng.uniform(0, 2 * np.pi, k)
    s.append(np.column_stack([rh * np.cos(ph), rh * np.sin(ph), rng.uniform(-1.2, 1.2, k) * zmax[0], _unit(rng, k)]))
    # w = 0: no vertical wall ahead, at any height
    rr = radii()
    ph = rng.uniform(0, 2 * np.pi, k)
    s.append(np.column_stack([rr, np.zeros(k), rng.uniform(-1.1, 1.1, k) * np.interp(rr, mid, zmax), np.cos(ph), np.sin(ph),
                              np.zeros(k)]))
    # flights that start at z = -0.0 and at z = +0.0, in every direction (dz == 0 at the first crossing)
    for zero in (-0.0, 0.0):
        s.append(np.column_stack([radii(), np.zeros(k), np.full(k, zero), _unit(rng, k)]))
    st = np.vstack(s)
    return st, np.full(st.shape[0], -1, np.int32), np.full(st.shape[0], -1, np.int32)


@pytest.mark.parametrize("name,variant", [("pascucci", "plain"), ("ref41", "plain"), ("small2d", "plain"), ("small2d", "mrw")])
@pytest.mark.parametrize("dark_every", [0, 7])
def test_wall_form_is_bit_exact(emu, name, variant, dark_every):
    m = _model(name)
    orc = Oracle(m, 1000)
    rng = np.random.default_rng(12345 + dark_every)
    st, extr, star = _states(m, name, rng)
    n0 = st.shape[0]
    ws, wri, wzj = _on_wall(name, rng)
    nw = ws.shape[0]
    cs, cri, czj = _corners(name, rng)
    nc = cs.shape[0]
    st = np.ascontiguousarray(np.vstack([st, ws, cs]))
    cextr = rng.exponential(1.0, nc)
    cextr[::2] = 1e30
    extr = np.concatenate([extr, np.full(nw, 1e30), cextr])
    star = np.concatenate([star, np.full(nw + nc, -1, np.int32)]).astype(np.int32)
    fri = np.concatenate([np.full(n0, -1, np.int32), wri, cri]).astype(np.int32)
    fzj = np.concatenate([np.full(n0, -1, np.int32), wzj, czj]).astype(np.int32)
    n = st.shape[0]
    steps, where = (np.zeros(n, np.int32) for _ in range(2))
    fixes = np.zeros((n, 3), np.int32)
    n_rad, nz = int(m.grid["n_rad"]), int(m.grid["nz"])
    n_pad = (n_rad + 2) * (nz + 2)
    EA, EC = np.zeros(n_pad), np.zeros(m.n_cells + 1)
    info = np.zeros(9, np.int32)
    rc = emu.emu_fly_wall_compare(C.byref(orc.cm), dark_every, VARIANTS[variant], n, _p(st, C.c_double), _p(extr, C.c_double),
                                  _p(star, C.c_int), _p(fri, C.c_int), _p(fzj, C.c_int), 100000, _p(steps, C.c_int),
                                  _p(where, C.c_int), _p(fixes, C.c_int), _p(EA, C.c_double), _p(EC, C.c_double),
                                  _p(info, C.c_int))
    assert rc == 0, rc
    assert steps.sum() > 5 * n  # (the walks test many crossings, not only the first)
    bad = {FIELDS[f]: int((where == f).sum()) for f in np.unique(where) if f}
    assert not bad, bad
    # the real slots of the padded grid hold the specification's grid
    pad = EA.reshape(nz + 2, n_rad + 2)
    assert np.array_equal(pad[1:nz + 1, 1:n_rad + 1].ravel().view(np.int64), EC[:m.n_cells].view(np.int64))
    assert EC[:m.n_cells].sum() > 0 and EC[m.n_cells] == 0.0
    # each fix-up fired at the first crossing of the packets made for it
    k = nw // 3
    for i, what in enumerate(("s1 == 0", "t < 0", "z1 == 0")):
        assert fixes[n0 + i * k: n0 + (i + 1) * k, i].sum() >= k // 2, (what, fixes[n0:n0 + nw].sum(axis=0))
    # every corner of section 2 was crossed
    print("corners:", dict(zip(CORNERS, info[:8].tolist())), "mirrored:", int(info[8]))
    for what, count in zip(CORNERS, info[:8]):
        assert count >= 40, (what, int(count))
    assert (info[8] > 0) == (dark_every > 0), info
