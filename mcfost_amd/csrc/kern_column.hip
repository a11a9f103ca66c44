// Translation unit of the column densities and optical depths to every cell (mc_column.hip.h): k_compute_column,
// k_compute_column_voro (compute_column, optical_depth.f90:328-415) and k_integ_tau, k_integ_tau_voro (integ_tau, :186-244).
// See mc_kernels.h.
#include <hip/hip_runtime.h>

#include "mc_column.hip.h"
#include "mc_kernels.h"

namespace mcgpu {

const void* kpick_compute_column(bool voro, bool l3d) {
  if (voro) return (const void*)k_compute_column_voro;
  return bsel(l3d, [&](auto L3D) -> const void* { return (const void*)k_compute_column<MCGPU_BV(L3D)>; });
}

const void* kpick_integ_tau(bool voro, bool l3d) {
  if (voro) return (const void*)k_integ_tau_voro;
  return bsel(l3d, [&](auto L3D) -> const void* { return (const void*)k_integ_tau<MCGPU_BV(L3D)>; });
}

}  // namespace mcgpu
