// emu_math.cpp -- TEST INFRASTRUCTURE: the kinds of mcgpu_probe_math (mcfost_amd/csrc/mc_math_probe.hip.h) on one emulated
// lane (the shim of emu_kernel.cpp): the MCGPU_LANE_EMULATION branches of f64_to_i32_sat, sad_plus1_u32, sincos_pi and
// az_sector_certain, az_sector, cdapres_pi, rotation, stokes_rotation, stokes_apply and hg_draw as the host tail runs
// them, and sqrt_nonneg's Newton sequence from a 26-bit seed.  Built only by tests/test_device_math_emulated.py.
#include "emu_kernel.cpp"
#include "../../mcfost_amd/csrc/mc_math_probe.hip.h"

// as mcgpu_probe_math: 0, or 3 (MCGPU_ERR_ARG) for an unknown kind (sqrt_fast_nonneg, log_pos and tau_of_draw are libm here) or a wrong
// row count
extern "C" int emu_probe_math(int kind, uint64_t n, const double* in, int n_in, double* out, int n_out) {
  int want_in = 0, want_out = 0;
  if (!mcgpu::math_probe_rows(kind, want_in, want_out) || n_in != want_in || n_out != want_out) return 3;
  for (uint64_t i = 0; i < n; ++i) mcgpu::math_probe_item(kind, (size_t)i, (size_t)n, in, out);
  return 0;
}
