"""The mean radiation field of the SED step (save_radiation_field's step-2 branch, radiation_field.f90:57-61) on one
emulated lane: tests/emu/emu_mono_xj.cpp runs the product's commit kernels that keep xJ_abs / xN_abs (k_mono_xj,
k_mono_sph_xj, k_mono_voro_xj) on the HBM path.

The identity that pins the new deposit to the oracle, which needs no change for it: without Stokes tracking
calc_xI_scatt deposits l * Stokes(1) * tab_s11_pos(it) under the very condition of xJ_abs (dust_ray_tracing.f90:509-516),
and tab_s11_pos is only the deposit's phase function (the scattering angle is drawn from prob_s11_pos).  With
tab_s11_pos = 1 (exactly representable) the oracle's sum over the sub-bins of xI_scatt(phik, psup, 1, iRT, icell) IS
xJ_abs(icell, lambda), for every observer iRT -- and the sum over the sub-bins removes the midplane psup ambiguity that
helpers.xI_close has to excuse.  Method 2: sum over (theta_I, phi_I) of I_spec(1, ..., icell) + I_spec_star(icell)
(radiation_field.f90:92-119).

Tolerance: that of tests/test_gpu_parity.py::_mono_parity for the same two computations without Stokes tracking,
rtol = 1e-6 with atol = 1e-8 x the largest value; no cell is exempt.  The oracle's sums for two observers could differ only
in their order of summation: measured here on the five models below at 8 streams x 6 packets the difference is exactly 0
(with tab_s11_pos = 1 every observer adds the same numbers in the same order; printed by the test), and the emulated
lane's xJ_abs lies within 7e-14 of the largest value (3D; 2e-16 to 1.3e-15 on the others) of those sums."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import sed_model
from mcfost_amd.host import model as M
from oracle import Oracle
from oracle.binding import _MonoOpts, _p
from test_kernel_emulation import N_COUNTERS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_mono_xj.cpp")
LIB = os.path.join(HERE, "emu", "libemu_mono_xj.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC] + [os.path.join(HERE, "emu", f) for f in ("emu_kernel.cpp", "emu_conv.h", "cross_cell_literal.h")] + \
       [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
RTOL, ATOL_REL = 1e-6, 1e-8    # (_mono_parity)
N_CHUNKS = 8


@pytest.fixture(scope="module")
def emu():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast"] + fma + ["-o", LIB, SRC])
    return C.CDLL(LIB)


def field_model(name):
    """The models of the issue, without Stokes tracking and with tab_s11_pos = 1 (set before any engine or oracle is built)."""
    if name == "3d":
        m = sed_model(M.small(n_rad=10, nz=5, n_az=6, l3D=True, lsepar_pola=False), n_thermal=30000)
    elif name == "sph":
        m = sed_model(M.small(grid_type=2, lsepar_pola=False), n_thermal=30000)
    elif name == "voronoi":
        m = sed_model(M.small(lsepar_pola=False), voronoi_sites=300, n_thermal=30000)
    else:
        m = sed_model(M.small(lsepar_pola=False), n_thermal=30000)
    if name == "dark":   # (the dark zone of test_kernel_emulation: the densest cells, never the first radial cell)
        m = copy.copy(m)
        dz = np.zeros(m.n_cells, np.uint8)
        kf = m.kappa_factor.copy()
        kf[::m.cfg.n_rad] = 0.0
        dz[np.argsort(kf)[-40:]] = 1
        m.l_dark_zone = dz
    m.tab_s11_pos = np.ones_like(m.tab_s11_pos)
    return m


def oracle_xJ(b, rt2=False):
    """xJ_abs(icell) of the wavelength from the oracle's run by the identity above: per observer [nRT, n_cells] (method 1)
    or [1, n_cells] (method 2)."""
    if rt2:
        return (b["I_spec"][..., 0].sum(axis=(1, 2)) + b["I_spec_star"])[None, :]
    return b["xI_scatt"][:, :, 0].sum(axis=(2, 3)).T


def emu_xj(emu, orc, lam, n2, seed, rt=1, rt2=(0, 0), want_xN=True, n_chunks=N_CHUNKS):
    m = orc.model
    o = _MonoOpts(seed, lam, lam, n_chunks, 0, float(n2), 1e9, int(m.capt_sup), int(rt), 1, int(rt2[0]), int(rt2[1]), None, None)
    xJ = np.zeros(m.n_cells)
    xN = np.zeros(m.n_cells, np.uint32)
    sed = np.zeros((9, m.cfg.N_phi, m.cfg.N_thet, m.n_lambda))
    ns = np.zeros(m.n_lambda)
    per = np.zeros(n_chunks, np.uint64)
    cnt = np.zeros(N_COUNTERS, np.uint64)
    rc = emu.emu_run_mono_xj(C.byref(orc.cm), C.byref(o), _p(xJ, C.c_double), _p(xN, C.c_uint32) if want_xN else None,
                             _p(sed, C.c_double), _p(ns, C.c_double), _p(per, C.c_uint64), _p(cnt, C.c_uint64))
    assert rc == 0, rc
    return dict(xJ=xJ, xN=xN, n_sent_chunk=per, counters=[int(c) for c in cnt])


def assert_field(xJ, ref):
    """device xJ_abs [n_cells] against the oracle's sums [n_obs, n_cells]: every observer's, every cell"""
    scale = np.abs(ref).max()
    assert scale > 0
    spread = np.abs(ref - ref[0]).max() / scale
    print("oracle: largest difference between two observers' sums / largest value = %.2e" % spread)
    assert spread < 1e-3 * ATOL_REL
    for q in range(ref.shape[0]):
        err = np.abs(xJ - ref[q])
        print("observer %d: max |device - oracle| / largest value = %.2e" % (q, err.max() / scale))
        assert np.allclose(xJ, ref[q], rtol=RTOL, atol=ATOL_REL * scale), q


@pytest.mark.parametrize("name,lam", [("2d", 4), ("3d", 4), ("sph", 4), ("voronoi", 9), ("dark", 4)])
def test_emulated_xJ_is_the_oracles_sum_over_the_sub_bins(emu, name, lam):
    m = field_model(name)
    orc = Oracle(m, 1e5)
    a = emu_xj(emu, orc, lam, 6, 40 + lam)
    b = orc.run_mono(lam, 6, seed=40 + lam, n_chunks=N_CHUNKS, n_phot_lim=1e9, rt1=True, n_threads=4)
    assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == list(b["counters"].values())
    if name == "dark":
        assert a["counters"][7] > 0   # (packets were mirrored)
    assert_field(a["xJ"], oracle_xJ(b))
    # xN_abs: one count per deposit -- positive exactly where xJ_abs is, and no more counts than crossings
    assert np.array_equal(a["xN"] > 0, a["xJ"] > 0)
    assert 0 < int(a["xN"].sum()) <= a["counters"][1]
    # without ray-tracing deposits the run still has its radiation field: the same packets in the same order on one lane
    c = emu_xj(emu, orc, lam, 6, 40 + lam, rt=0)
    assert np.array_equal(c["xJ"], a["xJ"]) and np.array_equal(c["xN"], a["xN"])
    # ... and the counts are optional
    d = emu_xj(emu, orc, lam, 6, 40 + lam, want_xN=False)
    assert np.array_equal(d["xJ"], a["xJ"]) and not d["xN"].any()


def test_emulated_xJ_method2(emu):
    m = field_model("2d")
    orc = Oracle(m, 1e5)
    a = emu_xj(emu, orc, 4, 6, 51, rt=2, rt2=(15, 15))
    b = orc.run_mono(4, 6, seed=51, n_chunks=N_CHUNKS, n_phot_lim=1e9, rt2=(15, 15), n_threads=4)
    assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == list(b["counters"].values())
    ref = oracle_xJ(b, rt2=True)
    scale = ref.max()
    assert scale > 0
    print("max |device - oracle| / largest value = %.2e" % (np.abs(a["xJ"] - ref[0]).max() / scale))
    assert np.allclose(a["xJ"], ref[0], rtol=RTOL, atol=ATOL_REL * scale)
    assert np.array_equal(a["xN"] > 0, a["xJ"] > 0)
    c = emu_xj(emu, orc, 4, 6, 51, rt=1)   # the deposit does not care which ray-tracing method rides along
    assert np.array_equal(c["xJ"], a["xJ"]) and np.array_equal(c["xN"], a["xN"])
