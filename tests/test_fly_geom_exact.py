"""Bit-exactness of the padded crossing's bookkeeping (fly_geom_2d<WALL = true>, mc_roles.hip.h), on the CPU.

The flying waves' crossing of the padded kernels without a dark zone forms three pieces of bookkeeping with fewer
instructions than the specification: the wall's side of the midplane (pad_wall_side: z0's sign bit goes into the wall, no
compare and select), the layer behind a vertical wall (fly_layer_step: a closed form, no delta_zj) and the row's address
(fly_row: a 24-bit multiply-add; the emulation indexes the table).  tests/emu/emu_fly_geom.cpp holds each against the
specification:

  * the crossings: packets walked through fly_visit_step_2d<..., PAD, WALL> and through fly_step_2d<..., PAD = false>, the
    specification, side by side.  After every crossing they agree, bit for bit, in x, y, z, u, v, w, ri, zj, kf, st,
    pk_cross, in c_cross, c_kill, c_dark and finished, in the value of the deposit and -- while the packet flies -- in extr;
    the key is the padding of the specification's index, and before every crossing the wall the flight carries is its cell's
    record for the direction that crossing finds.  Inputs: the states of tests/test_fly_step_exact.py (golden, random,
    edge), the packets ON a wall of tests/test_fly_visit_exact.py, so that each of the three fix-ups fires, and the corners
    of tests/test_fly_wall_exact.py (through the midplane, out of layer nz, in the row nz + 1, in the hole, dz == 0, w == 0,
    z0 = +-0.0), on the 20 x 10, 13 x 5 and 100 x 70 grids, plain and with the walk's bit in the crossing counter;
  * the layer step, exhaustively: for nz in {1, 2, 5, 10, 70}, every zj0 = 1 .. nz + 1 and both values of `away`, the closed
    form is zj0 + delta_zj of the specification (nz = 1: both clamps meet);
  * the wall time: the time to the vertical wall and the fix-up bit behind section 2's two overrides, with pad_wall_side's
    wall and with the specification's select, bit for bit -- z0 = +-0.0, +-denormal, +-1 ulp around the wall, ON the wall
    (where a sign applied behind the subtraction would turn the specification's +0.0 into -0.0), random; the wall positive,
    stored negative (row 1) and 1e10; inv_w of both signs and HUGE_DP; in and out of the hole."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mcfost_amd.host import model as M
from oracle import Oracle
from oracle.binding import _p
from test_fly_step_exact import _model, _states
from test_fly_visit_exact import _on_wall
from test_fly_wall_exact import _corners

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_geom.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_geom.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished", "deposit", "key", "carried wall"]
VARIANTS = {"plain": 0, "mrw": 1}
CORNERS = ["through the midplane", "up out of layer nz", "in the row nz + 1", "in the hole", "dz == 0", "w == 0",
           "z0 = -0.0", "z0 = +0.0"]
HUGE_DP = 1.79769313486231570815e+308


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _build(name):
    """The model of a grid; the 13 x 5 grid has no golden file: its states are drawn on the model's own grid."""
    if name != "small13x5":
        return _model(name), None
    m = M.build_model(M.small(n_rad=13, nz=5))
    g = {"walk": np.zeros((0, 6)), "grid_r_lim": np.asarray(m.grid["r_lim"], float),
         "grid_zmax": np.asarray(m.grid["zmax"], float), "grid_z_lim": np.asarray(m.grid["z_lim"], float).ravel()}
    assert len(g["grid_zmax"]) == 13 and len(g["grid_z_lim"]) == 13 * 7
    return m, g


@pytest.mark.parametrize("name,variant", [("small2d", "plain"), ("small2d", "mrw"), ("small13x5", "plain"),
                                          ("small13x5", "mrw"), ("pascucci", "plain"), ("pascucci", "mrw")])
def test_padded_bookkeeping_is_bit_exact(emu, monkeypatch, name, variant):
    m, grid = _build(name)
    if grid is not None:
        import helpers
        monkeypatch.setattr(helpers, "load_golden", lambda _name: grid)
    n_rad, nz = int(m.grid["n_rad"]), int(m.grid["nz"])
    assert (n_rad, nz) == {"small2d": (20, 10), "small13x5": (13, 5), "pascucci": (100, 70)}[name]
    orc = Oracle(m, 1000)
    rng = np.random.default_rng(4242)
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
    n_pad = (n_rad + 2) * (nz + 2)
    EA, EC = np.zeros(n_pad), np.zeros(m.n_cells + 1)
    info = np.zeros(8, np.int32)
    rc = emu.emu_fly_geom_compare(C.byref(orc.cm), VARIANTS[variant], n, _p(st, C.c_double), _p(extr, C.c_double),
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
    print("corners:", dict(zip(CORNERS, info.tolist())))
    for what, count in zip(CORNERS, info):
        assert count >= 40, (what, int(count))


@pytest.mark.parametrize("nz", [1, 2, 5, 10, 70])
def test_layer_step_is_the_specifications(emu, nz):
    got, want = (np.full(2 * (nz + 1), -99, np.int32) for _ in range(2))
    emu.emu_layer_step(nz, _p(got, C.c_int), _p(want, C.c_int))
    assert np.array_equal(got, want), (got.reshape(-1, 2), want.reshape(-1, 2))
    w = want.reshape(nz + 1, 2)   # [zj0 - 1, away]
    assert w[0, 0] == 2 and w[nz, 1] == nz + 1 and w.min() >= 1 and w.max() == nz + 1


def _wall_cases(rng):
    ulp = lambda x, k: (np.float64(x).view(np.int64) + k).view(np.float64)
    z0s, zws = [], []
    for zw in (0.37, 12.5, 1.0e10, -0.37, -12.5, 3.0e-300):   # (positive, 1e10, stored negative: row 1)
        a = abs(zw)
        z0 = [0.0, -0.0, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4, a, -a, ulp(a, 1), ulp(a, -1), -ulp(a, 1), -ulp(a, -1)]
        z0 += list(rng.uniform(-2.0, 2.0, 60) * a) + list(rng.uniform(-1.0, 1.0, 20) * 1e-12 * a)
        z0s += z0
        zws += [zw] * len(z0)
    z0, zw = np.array(z0s), np.array(zws)
    rows = []
    for inv_w in (1.7, -1.7, 1.0e3, -1.0e3, HUGE_DP, -HUGE_DP):
        # (w with inv_w's sign, as flight_constants forms the pair; w = 0 below HUGE_DP's threshold as well)
        for w in ((1.0 / inv_w if abs(inv_w) < 1e300 else np.copysign(1e-320, inv_w)), np.copysign(0.0, inv_w)):
            for hole in (0, 1):
                rows.append(np.column_stack([z0, zw, np.full_like(z0, w), np.full_like(z0, inv_w), np.full_like(z0, hole)]))
    return np.vstack(rows)


def test_wall_time_is_the_specifications(emu):
    c = _wall_cases(np.random.default_rng(7))
    n = c.shape[0]
    z0, zw, w, inv_w = (np.ascontiguousarray(c[:, i]) for i in range(4))
    hole = np.ascontiguousarray(c[:, 4].astype(np.int32))
    t_new, t_spec = np.zeros(n), np.zeros(n)
    f_new, f_spec = (np.full(n, -1, np.int32) for _ in range(2))
    emu.emu_wall_time(n, _p(z0, C.c_double), _p(zw, C.c_double), _p(w, C.c_double), _p(inv_w, C.c_double), _p(hole, C.c_int),
                      _p(t_new, C.c_double), _p(f_new, C.c_int), _p(t_spec, C.c_double), _p(f_spec, C.c_int))
    diff = np.nonzero(t_new.view(np.int64) != t_spec.view(np.int64))[0]
    assert diff.size == 0, [(z0[i], zw[i], w[i], inv_w[i], hole[i], t_new[i], t_spec[i]) for i in diff[:5]]
    assert np.array_equal(f_new, f_spec)
    # the cases reach every outcome: a wall ahead, the t < 0 fix-up, both overrides, a packet ON the wall (t = +-0.0)
    out = (hole == 0) & (w * z0 != 0.0)
    assert (f_spec == 2).sum() > 100 and (t_spec == 1.0e10).sum() > 100 and ((t_spec > 0) & (t_spec < 1e10) & out).sum() > 100
    assert ((t_spec == 0.0) & out).sum() >= 8
