// The arguments of the column kernels (mc_column.hip.h) and the cap on a ray's crossings: plain host / device declarations,
// shared by the unit of the kernels (kern_column.hip) and the unit of the launchers (mcgpu.hip), which needs no kernel of
// the family.
#pragma once

namespace mcgpu {

struct ColumnArgs {
  int type, lambda;              // 1, 2, 3; 1-based wavelength (type 2)
  int cap;                       // column_cap
  double CD_units;               // (:343-347), formed by the host
  const double* r_grid;          // centres of the cells (null on a Voronoi grid: the FP64 sites of the grid)
  const double* z_grid;
  const double* phi_grid;
  const double* gas_density;     // real(dp) gas_density(n_cells) (density.f90:27)
  const float* abundance;        // real tab_abundance(n_cells) (molecular_emission.f90:64)
  float* column;                 // column(n_cells, 4)
  unsigned long long* n_capped;
};

inline int column_cap(int n_rad, int nz, int n_az, int n_cells, bool voro) {
  if (voro) {
    int c = 1;
    while ((long long)c * c * c < (long long)n_cells) ++c;
    return 64 * c + 1024;
  }
  return 8 * (n_rad + 2 * nz + n_az) + 64;
}

}  // namespace mcgpu
