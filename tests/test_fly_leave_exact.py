"""Bit-exactness of the flying waves' crossing with the leave test at the commit (fly_visit_step_2d<..., PAD, WALL, LATE>
and fly_leave_2d, mc_roles.hip.h), on the CPU.

The padded kernels without a dark zone no longer test in front of every crossing whether the flight has left the grid or
reached its star's cell: the test sits behind the commit of the one crossing that can make it true, guarded by a necessary
condition on the cell entered, and runs once per visit for every flight a wave picks up.  tests/emu/emu_fly_leave.cpp holds
this against the specification, fly_step_2d<..., PAD = false>:

  * whole flights, walked visit by visit as the flying branch of roles_body runs them (visits of 1, 4 and any number of
    crossings: the pick-up test in front of every crossing, of some, of the first alone).  After every crossing the two
    agree, bit for bit, in x, y, z, u, v, w, ri, zj, kf, st, pk_cross, in c_cross, c_kill, c_dark and finished, in the value
    of the deposit and -- while the packet flies -- in extr; the key is the padding of the specification's index, the wall
    the flight carries is its cell's record, and no crossing starts in a cell that the test would have ended the flight
    in.  Where the new form has set a leaving state behind its commit, the comparison is made after the one extra call in
    which the specification finds that out, and that call must have changed nothing but st.
    Inputs: the states of tests/test_fly_step_exact.py (golden, random, edge), the packets ON a wall of
    tests/test_fly_visit_exact.py, the corners of tests/test_fly_wall_exact.py, and the leave cases below, on the 20 x 10,
    13 x 5 and 100 x 70 grids, plain and with the walk's bit in the crossing counter.  The test asserts that each occurred:
      - the last crossing, into column n_rad + 1;
      - the row nz + 1 entered in a column whose zmax is below zmaxmax, with |z1| below zmaxmax (stays), equal to it
        (stays), 1 ulp above it (leaves) and further above (leaves): flights along z = const (w = 0) whose row index is set
        to nz, so that the pick-up passes and the crossing itself commits the row nz + 1, and flights that rise through
        zmaxmax on their way out;
      - the star's cell as the next cell, and as the cell a flight starts in;
      - a flight picked up already outside (beyond Rmax, above zmaxmax);
      - a flight that crosses the hole (in from column 1, out again);
  * zj of the end point from ONE conversion, and the fraction as fract_nonneg: qd at integers, +-1 ulp around them, from
    2^31 and 2^52 on, NaN -- the same zj and the same bits of the fraction as with the floor in front, and for every qd
    that is a number the zj of fly_step_2d's minimum on the doubles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mcfost_amd.host import model as M
from oracle import Oracle
from oracle.binding import _p
from test_fly_step_exact import _model, _states, _unit
from test_fly_visit_exact import _on_wall
from test_fly_wall_exact import _corners

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_fly_leave.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_leave.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "emu", "emu_kernel.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
FIELDS = ["none", "x", "y", "z", "u", "v", "w", "ri", "zj", "ic", "kf", "extr", "st", "pk_cross", "c_cross", "c_kill",
          "c_dark", "finished", "deposit", "key", "carried wall", "the specification's extra call", "crossing from an untested cell"]
VARIANTS = {"plain": 0, "mrw": 1}
INFO = ["into column n_rad + 1", "row nz + 1 below zmaxmax: stays", "row nz + 1 at zmaxmax: stays",
        "row nz + 1, 1 ulp above zmaxmax: leaves", "row nz + 1 above zmaxmax: leaves", "star's cell next", "star's cell at the start",
        "picked up outside", "into the hole", "out of the hole", "guard alone", "visits"]
GRIDS = {"small2d": (20, 10), "small13x5": (13, 5), "pascucci": (100, 70)}


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _build(name):
    """The model of a grid; the 13 x 5 grid has no golden file: its states are drawn on the model's own grid."""
    if name != "small13x5":
        from helpers import load_golden
        return _model(name), load_golden(name), False
    m = M.build_model(M.small(n_rad=13, nz=5))
    g = {"walk": np.zeros((0, 6)), "grid_r_lim": np.asarray(m.grid["r_lim"], float),
         "grid_zmax": np.asarray(m.grid["zmax"], float), "grid_z_lim": np.asarray(m.grid["z_lim"], float).ravel()}
    assert len(g["grid_zmax"]) == 13 and len(g["grid_z_lim"]) == 13 * 7
    return m, g, True


def _leave_cases(g, rng):
    """(states, ri, zj, star): ri / zj = -1: looked up; star -1: none, -2: the start cell, -3: the first crossing's next cell."""
    r_lim = np.asarray(g["grid_r_lim"], float)
    zmax = np.asarray(g["grid_zmax"], float)
    n_rad, nz = len(zmax), int(round(len(g["grid_z_lim"]) / len(zmax))) - 2
    zmm = zmax.max()
    mid = 0.5 * (r_lim[1:] + r_lim[:-1])
    ulp = lambda x, k: (np.float64(x).view(np.int64) + k).view(np.float64)
    k = 48
    s, fri, fzj, star = [], [], [], []

    def add(st, ri=-1, zj=-1, sk=-1):
        s.append(st)
        n = st.shape[0]
        fri.append(np.full(n, -1) if np.isscalar(ri) else ri)
        fzj.append(np.full(n, zj) if np.isscalar(zj) else zj)
        star.append(np.full(n, sk))

    def horizontal(n):
        ph = rng.uniform(0, 2 * np.pi, n)
        return np.column_stack([np.cos(ph), np.sin(ph), np.zeros(n)])

    low = np.nonzero(zmax < zmm * (1 - 1e-6))[0]   # columns whose zmax is below zmaxmax
    assert low.size > 0, "every column reaches zmaxmax"
    # the row nz + 1 committed by the crossing itself: along z = const at zmaxmax - 1 ulp, zmaxmax, zmaxmax + 1 ulp, both sides
    # of the midplane, from a cell whose row index is set to nz (a radial move recomputes it: nz + 1)
    for z in (ulp(zmm, -1), zmm, ulp(zmm, 1)):
        col = rng.choice(low, k)
        rr = rng.uniform(0.2, 0.8, k) * (r_lim[col + 1] - r_lim[col]) + r_lim[col]
        ph = rng.uniform(0, 2 * np.pi, k)
        sg = rng.choice([-1.0, 1.0], k)
        add(np.column_stack([rr * np.cos(ph), rr * np.sin(ph), sg * z, horizontal(k)]), zj=nz)
    # rising through zmaxmax in the row nz + 1, on the way out (and some that come down again first)
    col = rng.choice(low, k)
    rr = rng.uniform(0.2, 0.8, k) * (r_lim[col + 1] - r_lim[col]) + r_lim[col]
    d = _unit(rng, k)
    d[:, 2] = np.abs(d[:, 2]) * 0.05 + 1e-3
    d /= np.linalg.norm(d, axis=1)[:, None]
    sg = rng.choice([-1.0, 1.0], k)
    d[:, 2] *= sg
    add(np.column_stack([rr, np.zeros(k), sg * zmm * (1 - rng.uniform(1e-9, 1e-3, k)), d]))
    # the last crossing into column n_rad + 1: outward from the last columns
    rr = rng.uniform(r_lim[-3], r_lim[-1], k)
    zz = rng.uniform(-0.9, 0.9, k) * np.interp(rr, mid, zmax)
    d = _unit(rng, k) * np.array([1.0, 0.1, 0.1])
    d[:, 0] = np.abs(d[:, 0]) + 1.0
    d /= np.linalg.norm(d, axis=1)[:, None]
    add(np.column_stack([rr, np.zeros(k), zz, d]))
    # the star's cell as the cell a flight starts in, and as the cell its first crossing enters
    for sk in (-2, -3):
        rr = rng.uniform(r_lim[0], r_lim[-1], k)
        add(np.column_stack([rr, np.zeros(k), rng.uniform(-0.95, 0.95, k) * np.interp(rr, mid, zmax), _unit(rng, k)]), sk=sk)
    # picked up already outside: beyond the outer edge, above zmaxmax
    rr = r_lim[-1] * rng.uniform(1.001, 1.5, k)
    add(np.column_stack([rr, np.zeros(k), rng.uniform(-1, 1, k) * zmm, _unit(rng, k)]))
    rr = rng.uniform(r_lim[0], r_lim[-1], k)
    add(np.column_stack([rr, np.zeros(k), rng.choice([-1.0, 1.0], k) * zmm * rng.uniform(1.0001, 2.0, k), _unit(rng, k)]))
    # across the hole: from the first column, aimed inside the inner edge
    rr = rng.uniform(1.0, 1.0, k) * (r_lim[0] + 0.5 * (r_lim[1] - r_lim[0]))
    aim = rng.uniform(-0.8, 0.8, k) * r_lim[0]   # impact parameter
    th = np.arcsin(aim / rr)
    wz = rng.uniform(-0.02, 0.02, k)
    d = np.column_stack([-np.cos(th), np.sin(th), wz])
    d /= np.linalg.norm(d, axis=1)[:, None]
    add(np.column_stack([rr, np.zeros(k), rng.uniform(-0.3, 0.3, k) * zmax[0], d]))
    st = np.vstack(s)
    return (st, np.concatenate(fri).astype(np.int32), np.concatenate(fzj).astype(np.int32), np.concatenate(star).astype(np.int32))


@pytest.mark.parametrize("name,variant", [("small2d", "plain"), ("small2d", "mrw"), ("small13x5", "plain"),
                                          ("small13x5", "mrw"), ("pascucci", "plain"), ("pascucci", "mrw")])
def test_leave_at_the_commit_is_bit_exact(emu, monkeypatch, name, variant):
    m, grid, own = _build(name)
    if own:
        import helpers
        monkeypatch.setattr(helpers, "load_golden", lambda _name: grid)
    n_rad, nz = int(m.grid["n_rad"]), int(m.grid["nz"])
    assert (n_rad, nz) == GRIDS[name]
    orc = Oracle(m, 1000)
    rng = np.random.default_rng(2718)
    st, extr, star = _states(m, name, rng)
    n0 = st.shape[0]
    ws, wri, wzj = _on_wall(name, rng)
    cs, cri, czj = _corners(name, rng)
    ls, lri, lzj, lstar = _leave_cases(grid, rng)
    nw, nc, nl = ws.shape[0], cs.shape[0], ls.shape[0]
    st = np.ascontiguousarray(np.vstack([st, ws, cs, ls]))
    cextr = rng.exponential(1.0, nc)
    cextr[::2] = 1e30
    extr = np.concatenate([extr, np.full(nw, 1e30), cextr, np.full(nl, 1e30)])
    star = np.concatenate([star, np.full(nw + nc, -1, np.int32), lstar]).astype(np.int32)
    fri = np.concatenate([np.full(n0, -1, np.int32), wri, cri, lri]).astype(np.int32)
    fzj = np.concatenate([np.full(n0, -1, np.int32), wzj, czj, lzj]).astype(np.int32)
    n = st.shape[0]
    # visits of 1 crossing (the pick-up test in front of each), of 4, and as long as the flight
    visit = np.array([1, 4, 100000], np.int32)[np.arange(n) % 3]
    visit[n - nl:] = np.array([100000, 4, 100000, 1], np.int32)[np.arange(nl) % 4]
    steps, where = (np.zeros(n, np.int32) for _ in range(2))
    n_pad = (n_rad + 2) * (nz + 2)
    EA, EC = np.zeros(n_pad), np.zeros(m.n_cells + 1)
    info = np.zeros(len(INFO), np.int32)
    rc = emu.emu_fly_leave_compare(C.byref(orc.cm), VARIANTS[variant], n, _p(st, C.c_double), _p(extr, C.c_double),
                                   _p(star, C.c_int), _p(fri, C.c_int), _p(fzj, C.c_int), _p(visit, C.c_int), 100000,
                                   _p(steps, C.c_int), _p(where, C.c_int), _p(EA, C.c_double), _p(EC, C.c_double),
                                   _p(info, C.c_int))
    assert rc == 0, rc
    assert steps.sum() > 5 * n  # (the walks test many crossings, not only the first)
    bad = {FIELDS[f]: int((where == f).sum()) for f in np.unique(where) if f}
    assert not bad, (bad, np.nonzero(where)[0][:10])
    # the real slots of the padded grid hold the specification's grid
    pad = EA.reshape(nz + 2, n_rad + 2)
    assert np.array_equal(pad[1:nz + 1, 1:n_rad + 1].ravel().view(np.int64), EC[:m.n_cells].view(np.int64))
    assert EC[:m.n_cells].sum() > 0 and EC[m.n_cells] == 0.0
    # every leave case occurred
    print("cases:", dict(zip(INFO, info.tolist())))
    # (the guard alone is counted, not required: in a consistent state |z| > zmaxmax is the row nz + 1 already)
    for what, count in zip(INFO, info):
        assert count >= 8 or what == "guard alone", (what, int(count))


@pytest.mark.parametrize("nz", [1, 5, 10, 70])
def test_zj_of_the_end_point_from_one_conversion(emu, nz):
    rng = np.random.default_rng(99)
    ulp = lambda x, k: (np.asarray(x, np.float64).view(np.int64) + k).view(np.float64)
    ints = np.concatenate([np.arange(0.0, 80.0), 2.0 ** np.arange(7, 31), [2.0 ** 31 - 2, 2.0 ** 31 - 1, 2.0 ** 31, 2.0 ** 31 + 1,
                           2.0 ** 32, 2.0 ** 40, 2.0 ** 51, 2.0 ** 52 - 1, 2.0 ** 52, 2.0 ** 52 + 1, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64,
                           1e30, 1e300, np.finfo(float).max]])
    pos = ints[ints > 0]
    qd = np.concatenate([ints, ulp(ints, 1), ulp(pos, -1), [0.5, ulp(0.5, 1), ulp(0.5, -1), 5e-324, 2.2e-308, 2.0 ** 52 - 0.5,
                         2.0 ** 31 - 0.5, 2.0 ** 31 - 1.5], rng.uniform(0, nz + 3, 2000), 2.0 ** rng.uniform(-30, 70, 2000),
                         [np.nan, np.copysign(np.nan, -1.0)]])
    qd = np.ascontiguousarray(qd[~np.isinf(qd)])   # (the largest double + 1 ulp; |z1| rzn is finite)
    n = qd.size
    zj_new, zj_spec, zj_step = (np.full(n, -99, np.int32) for _ in range(3))
    fr_new, fr_spec = np.zeros(n), np.zeros(n)
    emu.emu_zj_end(n, nz, _p(qd, C.c_double), _p(zj_new, C.c_int), _p(fr_new, C.c_double), _p(zj_spec, C.c_int),
                   _p(fr_spec, C.c_double), _p(zj_step, C.c_int))
    assert np.array_equal(zj_new, zj_spec)
    assert np.array_equal(fr_new.view(np.int64), fr_spec.view(np.int64))
    num = ~np.isnan(qd)
    assert np.array_equal(zj_new[num], zj_step[num]) and (zj_new[~num] == 1).all()
    assert zj_new.min() == 1 and zj_new.max() == nz + 1
    # the fraction: exact, in [0, 1), +0.0 at every integer and from 2^52 on, a NaN for a NaN
    assert (fr_new[num] >= 0).all() and (fr_new[num] < 1).all() and np.isnan(fr_new[~num]).all()
    whole = num & (qd == np.floor(qd))
    assert whole.sum() > 150 and (fr_new[whole].view(np.int64) == 0).all() and whole[num & (qd >= 2.0 ** 52)].all()
    assert np.array_equal(fr_new[num] + np.floor(qd[num]), qd[num])
