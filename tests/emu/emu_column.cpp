// emu_column.cpp -- TEST INFRASTRUCTURE: the column kernels (mcfost_amd/csrc/mc_column.hip.h: k_compute_column,
// k_compute_column_voro, k_integ_tau, k_integ_tau_voro) on one emulated lane (the shim of emu_kernel.cpp), so that the whole
// walk runs on the CPU before it runs on a device.  Built only by tests/test_column.py.
#include "emu_kernel.cpp"
#include "../../mcfost_amd/csrc/mc_column.hip.h"

// column [4 n_cells] (direction-major, = column(n_cells, 4) column-major); r_grid / z_grid / phi_grid: null on a Voronoi grid.
// cap_used (may be null) receives column_cap of the grid.
extern "C" int emu_compute_column(const oracle_model* m, int type, int lambda, const double* r_grid, const double* z_grid,
                                  const double* phi_grid, const double* gas_density, const float* abundance, float* column,
                                  unsigned long long* n_capped, int* cap_used) {
  Conv cv(m);
  const DevModel& M = cv.M;
  if (lds_bytes(M, true) > sizeof(lds_raw)) return 31;
  ColumnArgs A;
  memset(&A, 0, sizeof(A));
  A.type = type; A.lambda = type == 2 ? lambda : 1;
  A.cap = column_cap(M.n_rad, M.nz, M.n_az, M.n_cells, cv.voro);
  if (cap_used) *cap_used = A.cap;
  const float mu_mH = (float)((double)2.3f * (1.007825032231 * (1.0 / 6.022140857e23)));   // (mcgpu_compute_column)
  const double AU_to_m = 149597870700.0, m_to_cm2 = 1.0e2 * 1.0e2;
  A.CD_units = type == 1 ? AU_to_m * (double)mu_mH / m_to_cm2 : AU_to_m / m_to_cm2;
  A.r_grid = r_grid; A.z_grid = z_grid; A.phi_grid = phi_grid; A.gas_density = gas_density; A.abundance = abundance;
  A.column = column;
  unsigned long long capped = 0ull;
  A.n_capped = &capped;
  gridDim.x = 1; blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  if (cv.voro) k_compute_column_voro(M, A, cv.G);
  else if (m->l3D) k_compute_column<true>(M, A);
  else k_compute_column<false>(M, A);
  if (n_capped) *n_capped = capped;
  return 0;
}

extern "C" int emu_integ_tau(const oracle_model* m, int lambda, float angle_deg, float* tau_midplane, float* tau_angle) {
  Conv cv(m);
  const DevModel& M = cv.M;
  if (lds_bytes(M, true) > sizeof(lds_raw)) return 31;
  float out[2] = {0.0f, 0.0f};
  gridDim.x = 1; blockDim.x = 1; blockIdx.x = 0;   // (a stride of 1: lane 0 stages every table entry, lane 1 all but the first again)
  for (unsigned lane = 0; lane < 2; ++lane) {   // the kernel's two lanes, one after the other
    threadIdx.x = lane;
    if (cv.voro) k_integ_tau_voro(M, cv.G, lambda, angle_deg, out);
    else if (m->l3D) k_integ_tau<true>(M, lambda, angle_deg, out);
    else k_integ_tau<false>(M, lambda, angle_deg, out);
  }
  threadIdx.x = 0; blockDim.x = 1;
  *tau_midplane = out[0]; *tau_angle = out[1];
  return 0;
}
