"""The host branches of the packet loop's own math (mc_device.hip.h under MCGPU_LANE_EMULATION, which the host tail runs)
against the extended-precision references of tests/device_math_cases.py -- the same arguments and bounds as the device's
sequences get in tests/test_device_math_gpu.py, so that a failure there points at the device's instructions and not at
the formula.

tests/emu/emu_math.cpp compiles mc_math_probe.hip.h's dispatch for one emulated lane: the written-out cast and |a - b| + 1,
sincos(PI * x), the division in az_sector_certain, az_sector, cdapres_pi, rotation, stokes_rotation, stokes_apply, hg_draw,
and sqrt_nonneg's Newton sequence from a seed of 1 / sqrt(x) rounded to 26 bits (the device takes v_rsq_f64's).
sqrt_fast_nonneg, log_pos and tau_of_draw are libm on the host: there is nothing of the project's to probe."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_math_cases as cases
from mcfost_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_math.cpp")
LIB = os.path.join(HERE, "emu", "libemu_math.so")
CSRC = os.path.join(os.path.dirname(HERE), "mcfost_amd", "csrc")
DEPS = [SRC] + [os.path.join(HERE, "emu", f) for f in ("emu_kernel.cpp", "emu_conv.h", "cross_cell_literal.h")] + \
       [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]

# C of hg's bound C eps (1 + q^2 (1 + 2 / D)) / (2 |g|): numpy's unfused float64 evaluation of the formula misses the
# extended reference by at most 1.9263 units on the inputs of device_math_cases.hg_inputs -> the smallest power of two
# that passes is 2, times four (test_hg_constant_is_derived recomputes it)
HG_C = 8.0


@pytest.fixture(scope="module")
def probe():
    if (not os.path.exists(LIB)) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        # the host tail's flags (__graft_entry__.HOST_CXX_FLAGS): multiply-adds contracted as hipcc contracts them
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast", "-mfma", "-o", LIB, SRC])
    lib = C.CDLL(LIB)

    def run(kind, *rows):
        code, n_in, n_out = Engine.MATH_KINDS[kind]
        assert len(rows) == n_in
        ins = np.ascontiguousarray(np.broadcast_arrays(*[np.asarray(r, np.float64) for r in rows]), dtype=np.float64)
        ins = ins.reshape(n_in, -1)
        out = np.empty((n_out, ins.shape[1]), np.float64)
        dp = C.POINTER(C.c_double)
        rc = lib.emu_probe_math(C.c_int(code), C.c_uint64(ins.shape[1]), ins.ctypes.data_as(dp), C.c_int(n_in),
                                out.ctypes.data_as(dp), C.c_int(n_out))
        assert rc == 0, (kind, rc)
        return out
    run.lib = lib
    return run


def test_extended_precision_is_there():
    cases.require_extended()


def test_hg_constant_is_derived():
    C_, worst = cases.hg_constant()
    print("hg: numpy float64 / unit", worst, "-> C", C_)
    assert C_ == HG_C


def test_kinds_without_a_host_form_and_wrong_rows_are_refused(probe):
    x, o = np.ones(4), np.empty(8)
    dp = C.POINTER(C.c_double)
    call = lambda code, n_in, n_out: probe.lib.emu_probe_math(C.c_int(code), C.c_uint64(4), x.ctypes.data_as(dp), C.c_int(n_in),
                                                              o.ctypes.data_as(dp), C.c_int(n_out))
    for kind in ("sqrt_fast_nonneg", "log_pos", "tau_of_draw"):
        assert call(Engine.MATH_KINDS[kind][0], 1, 1) == 3
    assert call(99, 1, 1) == 3 and call(-1, 1, 1) == 3
    assert call(Engine.MATH_KINDS["sqrt_nonneg"][0], 2, 1) == 3 and call(Engine.MATH_KINDS["sqrt_nonneg"][0], 1, 1) == 0


def test_sqrt_nonneg_newton_sequence_from_a_26_bit_seed(probe):
    cases.check_sqrt_nonneg(probe)


def test_f64_to_i32_sat_written_out(probe):
    cases.check_f64_to_i32_sat(probe)


def test_sad_plus1_u32_written_out(probe):
    cases.check_sad_plus1_u32(probe)


@pytest.mark.parametrize("which", list(cases.SINCOS_RANGES))
def test_sincos_pi_through_the_product(probe, which):
    """sincos of the product PI * x against pi eps + 2 eps = 5.71e-16.  Measured on both ranges: |s - sin| <= 3.50e-16,
    |c - cos| <= 3.16e-16.  This test found the plain product wanting for x = 2 rand (6.91e-16 and 6.43e-16: for x in [1, 2)
    the product lies in [pi, 2 pi) and rounds twice as coarsely); the host branch now subtracts the period first."""
    cases.check_sincos_pi(probe, which)


def test_az_sector_with_the_division(probe):
    cases.check_az_sector(probe)


def test_cdapres_pi(probe):
    cases.check_cdapres_pi(probe)


def test_rotation_against_the_literal_form(probe):
    cases.check_rotation(probe)


def test_stokes_rotation_against_the_literal_route(probe):
    cases.check_stokes_rotation(probe)


def test_stokes_apply_against_the_matrix_statement(probe):
    cases.check_stokes_apply(probe)


def test_hg_draw(probe):
    cases.check_hg(probe, HG_C)
