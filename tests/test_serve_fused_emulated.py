"""The fused serving round of the padded 2D role kernels (mc_roles.hip.h, FUSED) on one emulated lane.

A serving lane bins its exited packet directly behind the SRV pop, keeps the record and emits the next packet into it in
the same round; a packet that leaves the grid later in the round (an emission that misses the grid, an exit within the first
crossings, a flight flown in place that leaves) stays the lane's record and is binned at the top of its next serving round.
tests/emu/emu_serve_fused.cpp compiles that round into the plain instantiations (the ones the emulation runs; the library
builds it into the padded ones) and counts the records that were reused, the exits that were held over a round boundary
and the held exits that a hand-over wrote out.  Which round bins or emits a packet must not matter: packet for packet the
oracle's counters, n_sent, SED counts and absorbed energy -- on the 20 x 10 and 13 x 5 grids, with a dark zone, with the
walk, with a star above the disk whose emissions partly miss the grid, through the kernel that hands its last packets
over, and with a packet count that is no multiple of the id batch, so that the last round's lanes may not emit."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mcfost_amd.host import model as M
from oracle import Oracle
from oracle.binding import _p
from test_kernel_emulation import N_COUNTERS, _Opts

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_serve_fused.cpp")
LIB = os.path.join(HERE, "emu", "libemu_serve_fused.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC] + [os.path.join(HERE, "emu", f) for f in ("emu_kernel.cpp", "emu_conv.h")] + \
       [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
N = 3001   # (no multiple of the id batch: the last batch is short, and lanes that binned an exit find no id)


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _run(emu, orc, prior, roles, tail=0):
    m = orc.model
    E = np.zeros(m.n_cells)
    sed = np.zeros((9, m.cfg.N_phi, m.cfg.N_thet, m.n_lambda))
    ns = np.zeros(m.n_lambda)
    cnt = np.zeros(N_COUNTERS, np.uint64)
    stats = np.zeros(3, np.uint64)
    o = _Opts(7, 0, N, 1, 1, 0, 1.0)
    rc = emu.emu_run_roles_fused(C.byref(orc.cm), C.byref(o), _p(prior, C.c_double), *roles, tail, _p(E, C.c_double),
                                 _p(sed, C.c_double), _p(ns, C.c_double), _p(cnt, C.c_uint64), _p(stats, C.c_uint64))
    assert rc == 0, rc
    return dict(E_abs=E, sed=sed, n_sent=ns, counters=[int(c) for c in cnt], reused=int(stats[0]), held=int(stats[1]),
                handed=int(stats[2]))


def _model(name):
    if name == "small13x5":
        return M.build_model(M.small(n_rad=13, nz=5))
    if name == "small2d_star_above":   # (the star outside the grid: part of its emissions miss the disk -- exits made by the emission)
        cfg = M.small(lsepar_pola=False)
        cfg.star_xyz = (0.0, 0.0, 400.0)
        return M.build_model(cfg)
    m = M.build_model(M.small())
    if name == "small2d_dark":   # (as test_emulated_role_schedule)
        m = copy.copy(m)
        dz = np.zeros(m.n_cells, np.uint8)
        kf = m.kappa_factor.copy()
        kf[::m.cfg.n_rad] = 0.0
        dz[np.argsort(kf)[-40:]] = 1
        m.l_dark_zone = dz
    if name == "small2d_mrw":
        M.init_mrw(m)
    return m


# n_srv_pref, k_short, fly_iters, emit_qmax: the one wave serves and flies long flights in place (first two: every flight
# that leaves does so in the server's hands, a held exit), with a FLY ring that stops the emission at once (emit_qmax 0:
# lanes that binned an exit may not emit); or it prefers to fly and serves only what it owns (its exits come off the SRV ring)
ROLES = ((1, 2, 3, 128), (1, 1, 64, 0), (0, 2, 3, 128))


@pytest.mark.parametrize("tail", [0, 40])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_dark", "small2d_mrw", "small2d_star_above"])
def test_emulated_fused_serving_round_runs_the_same_packets(emu, name, tail):
    m = _model(name)
    orc = Oracle(m, N)
    prior = orc.run_thermal(2000, seed=1)["E_abs"]
    b = orc.run_thermal(N, seed=7, frozen=True, E_prior=prior, n_threads=4)
    reused = held = handed = 0
    for roles in ROLES:
        a = _run(emu, orc, prior, roles, tail)
        print(name, tail, roles, "reused", a["reused"], "held", a["held"], "handed over", a["handed"])
        assert a["counters"] == list(b["counters"].values()), roles
        assert np.array_equal(a["n_sent"], b["n_sent"]) and np.array_equal(a["sed"][4], b["sed"][4])
        assert np.allclose(a["E_abs"], b["E_abs"], rtol=1e-9, atol=1e-11 * b["E_abs"].max())
        reused += a["reused"]; held += a["held"]; handed += a["handed"]
        if roles[0] == 1:   # (the serving wave: nearly every packet ends in its hands and the next one takes its record)
            assert a["reused"] > N // 2 and a["held"] > N // 2, (roles, a["reused"], a["held"])
    assert reused > N and held > N


def test_emulated_hand_over_meets_a_held_exit(emu):
    """Over the settings and thresholds below, at least one hand-over finds the serving lane with an exit it has not yet
    binned: the record goes out with its state and the tail kernel bins it -- the totals are still the oracle's."""
    m = _model("small2d")
    orc = Oracle(m, N)
    prior = orc.run_thermal(2000, seed=1)["E_abs"]
    b = orc.run_thermal(N, seed=7, frozen=True, E_prior=prior, n_threads=4)
    handed = 0
    for tail in (1, 2, 3, 5, 8, 13, 21, 40):
        a = _run(emu, orc, prior, (1, 2, 3, 128), tail)
        assert a["counters"] == list(b["counters"].values()), tail
        assert np.array_equal(a["n_sent"], b["n_sent"]) and np.array_equal(a["sed"][4], b["sed"][4])
        assert np.allclose(a["E_abs"], b["E_abs"], rtol=1e-9, atol=1e-11 * b["E_abs"].max())
        handed += a["handed"]
    print("held exits handed over:", handed)
    assert handed > 0
