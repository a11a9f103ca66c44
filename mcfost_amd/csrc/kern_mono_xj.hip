// Translation unit of the SED commit pass that also keeps the mean radiation field, xJ_abs / xN_abs of the SED step
// (option "radiation_field_sed"): k_mono_xj, k_mono_sph_xj (mc_mono.hip.h), k_mono_voro_xj (mc_mono_voronoi.hip.h).
// Only what can be launched: commit passes with atomic deposits (no scout pass, no log, no records).  See mc_kernels.h.
#include <hip/hip_runtime.h>

#include "mc_device.hip.h"
#include "mc_voronoi.hip.h"
#include "mc_mono.hip.h"
#include "mc_mono_voronoi.hip.h"
#include "mc_kernels.h"

namespace mcgpu {

const void* kpick_mono_xj(bool l3d, bool pola, bool dark, bool f32) {
  return bsel(l3d, [&](auto L3D) { return bsel(pola, [&](auto POLA) { return bsel(dark, [&](auto DARK) {
    return bsel(f32, [&](auto F32) -> const void* {
      return (const void*)k_mono_xj<MCGPU_BV(L3D), MCGPU_BV(POLA), MCGPU_BV(DARK), MCGPU_BV(F32)>;
    }); }); }); });
}

const void* kpick_mono_sph_xj(bool l3d, bool pola, bool f32) {
  return bsel(l3d, [&](auto L3D) { return bsel(pola, [&](auto POLA) { return bsel(f32, [&](auto F32) -> const void* {
    return (const void*)k_mono_sph_xj<MCGPU_BV(L3D), MCGPU_BV(POLA), MCGPU_BV(F32)>;
  }); }); });
}

const void* kpick_mono_voro_xj(bool pola, bool f32) {
  return bsel(pola, [&](auto POLA) { return bsel(f32, [&](auto F32) -> const void* {
    return (const void*)k_mono_voro_xj<MCGPU_BV(POLA), MCGPU_BV(F32)>;
  }); });
}

}  // namespace mcgpu
