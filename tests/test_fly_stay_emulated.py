"""Lean re-entry of the flying waves (mc_roles.hip.h, RunArgs::fly_stay) on one emulated lane.

tests/emu/emu_fly_stay.cpp compiles the 2D role kernels for the host with lean re-entries built into the plain
instantiations (the ones the emulation runs; the library builds them into the padded ones) and runs them with
fly_stay = 1 (a full scheduling round at every visit of the rings), 2, 16 and a large value.  The one wave prefers to fly
(n_srv_pref = 0), so it is the wave that re-enters -- the harness counts the lean rounds, and there must be many.  Which
round runs a packet must not matter: the same packets, counter for counter, as with full rounds and as the oracle's; with
a dark zone, with the walk, and through the kernel that hands its last packets over, where the one wave that decides the
hand-over is itself lean (its full rounds then keep one residue of 16: it must still see the work run out)."""
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
SRC = os.path.join(HERE, "emu", "emu_fly_stay.cpp")
LIB = os.path.join(HERE, "emu", "libemu_fly_stay.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC] + [os.path.join(HERE, "emu", f) for f in ("emu_kernel.cpp", "emu_conv.h")] + \
       [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
LARGE = 1 << 20
N = 3000


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def _run(emu, orc, prior, stay, roles, tail=0):
    m = orc.model
    E = np.zeros(m.n_cells)
    sed = np.zeros((9, m.cfg.N_phi, m.cfg.N_thet, m.n_lambda))
    ns = np.zeros(m.n_lambda)
    cnt = np.zeros(N_COUNTERS, np.uint64)
    lean = C.c_uint64(0)
    o = _Opts(7, 0, N, 1, 1, 0, 1.0)
    rc = emu.emu_run_roles_stay(C.byref(orc.cm), C.byref(o), _p(prior, C.c_double), stay, *roles, tail, _p(E, C.c_double),
                                _p(sed, C.c_double), _p(ns, C.c_double), _p(cnt, C.c_uint64), C.byref(lean))
    assert rc == 0, rc
    return dict(E_abs=E, sed=sed, n_sent=ns, counters=[int(c) for c in cnt], lean_rounds=int(lean.value))


def _model(name):
    if name == "small13x5":
        return M.build_model(M.small(n_rad=13, nz=5))
    if name == "small2d_hg":
        return M.build_model(M.small(aniso_method=2, lsepar_pola=False))
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


@pytest.mark.parametrize("tail", [0, 40])
@pytest.mark.parametrize("name", ["small2d", "small13x5", "small2d_hg", "small2d_dark", "small2d_mrw"])
def test_emulated_lean_reentry_runs_the_same_packets(emu, name, tail):
    m = _model(name)
    orc = Oracle(m, N)
    prior = orc.run_thermal(2000, seed=1)["E_abs"]
    b = orc.run_thermal(N, seed=7, frozen=True, E_prior=prior, n_threads=4)
    for roles in ((0, 2, 3, 128), (0, 1, 64, 4)):   # (n_srv_pref = 0: the settings of test_emulated_role_schedule in which the wave prefers to fly)
        full = _run(emu, orc, prior, 1, roles, tail)
        assert full["lean_rounds"] == 0
        assert full["counters"] == list(b["counters"].values())
        assert np.array_equal(full["n_sent"], b["n_sent"]) and np.array_equal(full["sed"][4], b["sed"][4])
        assert np.allclose(full["E_abs"], b["E_abs"], rtol=1e-9, atol=1e-11 * b["E_abs"].max())
        for stay in (2, 16, LARGE):
            lean = _run(emu, orc, prior, stay, roles, tail)
            print(name, tail, roles, stay, "lean rounds", lean["lean_rounds"])
            assert lean["lean_rounds"] > N // 10, (roles, stay, lean["lean_rounds"])
            assert lean["counters"] == full["counters"], (roles, stay)
            assert np.array_equal(lean["n_sent"], full["n_sent"]) and np.array_equal(lean["sed"][4], full["sed"][4])
            # (the rounds run the packets in another order: the sums' last digits, by the tolerance of the emulation tests)
            assert np.allclose(lean["E_abs"], full["E_abs"], rtol=1e-9, atol=1e-11 * full["E_abs"].max())
