"""The packet loop's own math on the device (mcgpu_probe_math: mc_math_probe.hip.h calls the functions of mc_device.hip.h,
one item per thread) against the extended-precision references of tests/device_math_cases.py: the Newton sequences behind
v_rsq_f64, log_pos and the optical depth of every draw, the two named instructions, sincospi over every azimuth the loop
forms, the default-real arctangent behind az_sector, cdapres_pi, the transcendental-free rotation and Stokes rotation,
and the Henyey-Greenstein draw.  tests/test_device_math_emulated.py holds the host branches against the same references.
Each test is one or two launches."""
import numpy as np
import pytest

import device_math_cases as cases
from mcfost_amd.engine import Engine
from test_device_math_emulated import HG_C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    e = Engine.bare(device=0)
    yield e.probe_math
    e.close()


def test_unknown_kind_and_wrong_rows_are_refused(probe):
    e = probe.__self__
    import ctypes as C
    x, o = np.ones(4), np.empty(8)
    dp = C.POINTER(C.c_double)
    call = lambda code, n_in, n_out: e.lib.mcgpu_probe_math(e.ctx, C.c_int(code), C.c_uint64(4), x.ctypes.data_as(dp), C.c_int(n_in),
                                                            o.ctypes.data_as(dp), C.c_int(n_out))
    assert call(99, 1, 1) == 3 and call(-1, 1, 1) == 3          # MCGPU_ERR_ARG
    assert call(Engine.MATH_KINDS["sincos_pi"][0], 1, 1) == 3 and call(Engine.MATH_KINDS["sincos_pi"][0], 2, 2) == 3
    assert call(Engine.MATH_KINDS["sqrt_nonneg"][0], 1, 1) == 0 and o[0] == 1.0


def test_sqrt_nonneg_is_correctly_rounded(probe):
    cases.check_sqrt_nonneg(probe)


def test_sqrt_fast_nonneg_within_a_few_ulp(probe):
    cases.check_sqrt_fast_nonneg(probe)


def test_log_pos(probe):
    cases.check_log_pos(probe)


def test_tau_of_every_draw(probe):
    cases.check_tau_of_draw(probe)


def test_f64_to_i32_sat(probe):
    cases.check_f64_to_i32_sat(probe)


def test_sad_plus1_u32(probe):
    cases.check_sad_plus1_u32(probe)


@pytest.mark.parametrize("which", list(cases.SINCOS_RANGES))
def test_sincos_pi_of_every_azimuth(probe, which):
    cases.check_sincos_pi(probe, which)


def test_sincos_pi_exact_values(probe):
    cases.check_sincos_pi_exact_values(probe)


def test_az_sector(probe):
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
    cases.check_hg(probe, HG_C)      # (C and the value that gave it: test_device_math_emulated.py)
