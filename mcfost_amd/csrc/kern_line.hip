// Translation unit of the molecular line ray tracer (mc_line.hip.h): k_line_map, k_line_map_voro (emission_line_map,
// mol_transfer.f90:484-847; integ_ray_mol, optical_depth.f90:419-599) and k_line_sum1 (method 1's sum).  See mc_kernels.h.
#include <hip/hip_runtime.h>

#include "mc_line.hip.h"
#include "mc_kernels.h"

namespace mcgpu {

const void* kpick_line_map(bool voro, bool l3d) {
  if (voro) return (const void*)k_line_map_voro;
  return bsel(l3d, [&](auto L3D) -> const void* { return (const void*)k_line_map<MCGPU_BV(L3D)>; });
}

const void* kpick_line_sum1() { return (const void*)k_line_sum1; }

}  // namespace mcgpu
