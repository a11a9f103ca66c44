// mc_math_probe.hip.h -- the packet loop's own math on chosen arguments (mcgpu_probe_math, include/mcgpu.h;
// tests/test_device_math_gpu.py).  The packet loop replaces library routines and the reference's literal formulas with
// shorter forms (mc_device.hip.h: sqrt_nonneg, log_pos, az_sector_certain, rotation, stokes_rotation, hg_draw ...); this
// probe calls those very functions, one item per thread, so that a test can hold the device's instruction sequences
// against an extended-precision reference.  tests/emu/emu_math.cpp compiles math_probe_item for one emulated lane: the
// host branches of the same functions, which the host tail runs.
#pragma once
#include "mc_device.hip.h"

namespace mcgpu {

enum MathProbeKind {
  MP_SQRT_NONNEG = 0,      // in: x                                      out: sqrt_nonneg(x)
  MP_SQRT_FAST_NONNEG,     // in: x                                      out: sqrt_fast_nonneg(x)
  MP_LOG_POS,              // in: x                                      out: log_pos(x)
  MP_TAU_OF_DRAW,          // in: rand (default real)                    out: tau_of_draw(rand)
  MP_F64_TO_I32_SAT,       // in: x                                      out: f64_to_i32_sat(x)
  MP_SAD_PLUS1_U32,        // in: a, b (unsigned 32-bit)                 out: sad_plus1_u32(a, b)
  MP_SINCOS_PI,            // in: x                                      out: s, c
  MP_AZ_SECTOR_CERTAIN,    // in: x, y, n_az                             out: k, certain (0 / 1)
  MP_AZ_SECTOR,            // in: x, y, n_az                             out: az_sector(.., false), az_sector(.., true)
  MP_CDAPRES_PI,           // in: cospsi, phi / pi, u0, v0, w0           out: u1, v1, w1
  MP_ROTATION,             // in: xinit, yinit, zinit, u1, v1, w1        out: xfin, yfin, zfin
  MP_STOKES_ROTATION,      // in: u0, v0, w0, u1, v1, w1                 out: cos omega, sin omega
  MP_STOKES_APPLY,         // in: S[4], cw, sw, M12, M22, M33, M34, M44, M11   out: S[4]
  MP_HG,                   // in: g, rand (default reals), nang          out: itheta, cospsi (hg_draw), hg_cosine
  MP_N_KINDS
};

// rows of n doubles a kind reads and writes; false for a kind this build does not have (the emulated lane has libm in
// place of sqrt_fast_nonneg, log_pos and so of tau_of_draw: nothing of the device's to probe)
inline bool math_probe_rows(int kind, int& n_in, int& n_out) {
  switch (kind) {
    case MP_SQRT_NONNEG: n_in = 1; n_out = 1; return true;
#ifndef MCGPU_LANE_EMULATION
    case MP_SQRT_FAST_NONNEG: case MP_LOG_POS: case MP_TAU_OF_DRAW: n_in = 1; n_out = 1; return true;
#endif
    case MP_F64_TO_I32_SAT: n_in = 1; n_out = 1; return true;
    case MP_SAD_PLUS1_U32: n_in = 2; n_out = 1; return true;
    case MP_SINCOS_PI: n_in = 1; n_out = 2; return true;
    case MP_AZ_SECTOR_CERTAIN: case MP_AZ_SECTOR: n_in = 3; n_out = 2; return true;
    case MP_CDAPRES_PI: n_in = 5; n_out = 3; return true;
    case MP_ROTATION: n_in = 6; n_out = 3; return true;
    case MP_STOKES_ROTATION: n_in = 6; n_out = 2; return true;
    case MP_STOKES_APPLY: n_in = 12; n_out = 4; return true;
    case MP_HG: n_in = 3; n_out = 3; return true;
    default: return false;
  }
}

// item i of n: row r of `in` / `out` is in[r * n + i].  Integers and default reals travel as doubles (exact).
__device__ inline void math_probe_item(int kind, size_t i, size_t n, const double* in, double* out) {
#define MP_IN(r) in[(size_t)(r) * n + i]
#define MP_OUT(r) out[(size_t)(r) * n + i]
  switch (kind) {
    case MP_SQRT_NONNEG: {
#ifdef MCGPU_LANE_EMULATION
      // the Newton sequence itself from a seed as good as the device's instruction gives (26 bits of 1 / sqrt(x))
      const double x = MP_IN(0);
      double y = 1.0 / std::sqrt(x);
      if (y <= HUGE_DP) {
        long long b = __double_as_longlong(y);
        b = (b + (1ll << 25)) & ~((1ll << 26) - 1ll);
        y = __longlong_as_double(b);
      }
      MP_OUT(0) = sqrt_nonneg_from_seed(x, y);
#else
      MP_OUT(0) = sqrt_nonneg(MP_IN(0));
#endif
    } break;
#ifndef MCGPU_LANE_EMULATION
    case MP_SQRT_FAST_NONNEG: MP_OUT(0) = sqrt_fast_nonneg(MP_IN(0)); break;
    case MP_LOG_POS: MP_OUT(0) = log_pos(MP_IN(0)); break;
    case MP_TAU_OF_DRAW: MP_OUT(0) = tau_of_draw((float)MP_IN(0)); break;
#endif
    case MP_F64_TO_I32_SAT: MP_OUT(0) = (double)f64_to_i32_sat(MP_IN(0)); break;
    case MP_SAD_PLUS1_U32: MP_OUT(0) = (double)sad_plus1_u32((unsigned int)MP_IN(0), (unsigned int)MP_IN(1)); break;
    case MP_SINCOS_PI: {
      double s, c;
      sincos_pi(MP_IN(0), &s, &c);
      MP_OUT(0) = s; MP_OUT(1) = c;
    } break;
    case MP_AZ_SECTOR_CERTAIN: {
      int k = 0;
      const bool certain = az_sector_certain(MP_IN(0), MP_IN(1), (int)MP_IN(2), k);
      MP_OUT(0) = (double)k; MP_OUT(1) = certain ? 1.0 : 0.0;
    } break;
    case MP_AZ_SECTOR: {
      MP_OUT(0) = (double)az_sector(MP_IN(0), MP_IN(1), (int)MP_IN(2), false);
      MP_OUT(1) = (double)az_sector(MP_IN(0), MP_IN(1), (int)MP_IN(2), true);
    } break;
    case MP_CDAPRES_PI: {
      double u1, v1, w1;
      cdapres_pi(MP_IN(0), MP_IN(1), MP_IN(2), MP_IN(3), MP_IN(4), u1, v1, w1);
      MP_OUT(0) = u1; MP_OUT(1) = v1; MP_OUT(2) = w1;
    } break;
    case MP_ROTATION: {
      double xf, yf, zf;
      rotation(MP_IN(0), MP_IN(1), MP_IN(2), MP_IN(3), MP_IN(4), MP_IN(5), xf, yf, zf);
      MP_OUT(0) = xf; MP_OUT(1) = yf; MP_OUT(2) = zf;
    } break;
    case MP_STOKES_ROTATION: {
      double cw, sw;
      stokes_rotation(MP_IN(0), MP_IN(1), MP_IN(2), MP_IN(3), MP_IN(4), MP_IN(5), cw, sw);
      MP_OUT(0) = cw; MP_OUT(1) = sw;
    } break;
    case MP_STOKES_APPLY: {
      double S[4] = {MP_IN(0), MP_IN(1), MP_IN(2), MP_IN(3)};
      stokes_apply(S, MP_IN(4), MP_IN(5), MP_IN(6), MP_IN(7), MP_IN(8), MP_IN(9), MP_IN(10), MP_IN(11));
      MP_OUT(0) = S[0]; MP_OUT(1) = S[1]; MP_OUT(2) = S[2]; MP_OUT(3) = S[3];
    } break;
    case MP_HG: {
      int itheta = 0;
      double cospsi = 0.0;
      hg_draw((float)MP_IN(0), (float)MP_IN(1), (int)MP_IN(2), itheta, cospsi);
      MP_OUT(0) = (double)itheta; MP_OUT(1) = cospsi; MP_OUT(2) = hg_cosine((float)MP_IN(0), (float)MP_IN(1));
    } break;
    default: break;
  }
#undef MP_IN
#undef MP_OUT
}

#ifndef MCGPU_LANE_EMULATION
// one thread per item, 256 threads per block
static __global__ void __launch_bounds__(256) k_probe_math(int kind, size_t n, const double* __restrict__ in,
                                                           double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) math_probe_item(kind, i, n, in, out);
}
#endif

}  // namespace mcgpu
