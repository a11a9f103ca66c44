// Column densities and optical depths from every cell: compute_column (optical_depth.f90:328-415) and integ_tau (:186-244).
//   k_compute_column<L3D>    cylindrical and spherical grids (the grid's operators picked at run time, as optical_length_tot
//   k_compute_column_voro    does); Voronoi grids.  One ray per lane, 4 n_cells rays in one launch: ray t goes from the centre
//                            of cell t % n_cells in direction t / n_cells + 1 -- the cell index runs fastest, so a wave holds
//                            64 neighbouring cells of one row that go the same way and whose trip counts fall off together.
//                            A ray starts INSIDE its cell (next_cell = icell, previous_cell = 0: no index_cell, no
//                            move_to_grid) and sums l_contrib * factor over the real cells up to the edge of the grid:
//                              type 1  CD_units * gas_density(icell0)                          (column_density.fits.gz)
//                              type 2  kappa(p_icell, lambda) * kappa_factor(icell0)           (optical_depth_to_cell.fits.gz)
//                              type 3  CD_units * gas_density(icell0) * tab_abundance(icell0)  (a molecule's column density)
//                            in double, stored as a default real.  No star test, no dark-zone mirror, no random walk, no
//                            deposits: the reference has none here, and l_dark_zone does not change the result.
//   k_integ_tau<L3D> / _voro integ_tau's two rays from the origin, optical_length_tot / _voro as they stand: lane 0 along +x,
//                            lane 1 along (sqrt(1 - w0^2), 0, w0), w0 = cos(angle pi / 180).
// Departure from the reference (lvariable_dust): compute_column sets p_icell = icell0 BEFORE icell0 = next_cell (:386-388), so
// it reads the opacity row of the PREVIOUS cell and row 0 for the first one -- a defect (optical_length_tot, :283-287, points
// at the current cell).  These kernels take the class of the current cell.
// Cells without a direction: a centre on the axis (direction 4) or at the origin (direction 1) is a division by zero in the
// reference; 0 is written there.
//
// A bounded walk.  The 1e8 guard of optical_length_tot is replaced by a cap derived from the grid (column_cap):
//   cylindrical / spherical   8 (n_rad + 2 nz + n_az) + 64.  A straight line meets each of the n_rad + 1 cylinders or spheres
//                             at most twice and each of the n_az azimuthal half-planes at most once; on a spherical grid each
//                             of the 2 nz + 1 cones at most twice; on a cylindrical grid the layer walls z_lim(i, j) are
//                             horizontal inside a radial cell, z is monotonic along the ray, and the relative height
//                             z / zmax(r) along a line through a flared disk turns a few times at the most, so the layer walls
//                             add a few times 2 nz + 2.  That is below 4 (n_rad + 2 nz + n_az); the factor 8 leaves as much
//                             again for zero-length steps at corners (the line through the origin of direction 1 meets the
//                             axis, where every azimuthal wall passes).
//   Voronoi                   64 ceil(n_cells^(1/3)) + 1024.  The cells are convex (a cut cell's void is crossed in the same
//                             step), so a line visits a cell once; a box diagonal of a uniform tessellation crosses about
//                             2.5 n_cells^(1/3) cells, and the sites of a disk crowd towards the midplane and the star by
//                             factors that the 64 covers (tests/test_column.py prints the longest walk of its grids).
// A ray that reaches the cap stops, keeps what it has summed, and adds one to n_capped: a pathological ray costs a bounded
// number of crossings instead of holding the device.
#pragma once
#include "mc_column_args.h"
#include "mc_raytrace.hip.h"
#include "mc_voronoi.hip.h"

namespace mcgpu {

// the direction of ray `dir` from (x1, y1, z1) (:368-379), the reference's order of operations; false: no direction
// (nd_mul / nd_add: products and sums that no build fuses -- the device's, the one-lane emulation's)
__device__ inline bool column_direction(int dir, double x1, double y1, double z1, double& u, double& v, double& w) {
  if (dir == 1) {
    const double n2 = nd_add(nd_add(nd_mul(x1, x1), nd_mul(y1, y1)), nd_mul(z1, z1));
    if (!(n2 > 0.0)) return false;
    const double norm = 1.0 / sqrt(n2);
    u = -x1 * norm; v = -y1 * norm; w = -z1 * norm;
  } else if (dir == 2) {
    u = 0.0; v = 0.0; w = 1.0;
  } else if (dir == 3) {
    u = 0.0; v = 0.0; w = -1.0;
  } else {
    const double n2 = nd_add(nd_mul(x1, x1), nd_mul(y1, y1));
    if (!(n2 > 0.0)) return false;
    const double norm = 1.0 / sqrt(n2);
    u = x1 * norm; v = y1 * norm; w = 0.0;
  }
  return true;
}

// factor of cell ic (0-based) without the opacity of type 2
__device__ inline double column_gas_factor(const ColumnArgs& A, int ic) {
  const double f = nd_mul(A.CD_units, A.gas_density[ic]);
  return A.type == 3 ? nd_mul(f, (double)A.abundance[ic]) : f;
}

template <bool L3D>
__device__ inline float column_ray(const Lds& T, const DevModel& M, const ColumnArgs& A, int icell, int dir) {
  const int n_rad = M.n_rad, nz = M.nz;
  const bool sph = M.grid_sph != 0;
  int q = icell - 1;  // inverse of the closed-form mapping
  int ri = q % n_rad + 1, zj, k = 1;
  q /= n_rad;
  if (L3D) {
    const int jj = q % (2 * nz);
    k = q / (2 * nz) + 1;
    zj = jj < nz ? jj - nz : jj - nz + 1;
  } else {
    zj = q + 1;
  }
  double sp, cp;
  sincos(A.phi_grid[icell - 1], &sp, &cp);
  double x = A.r_grid[icell - 1] * cp, y = A.r_grid[icell - 1] * sp, z = A.z_grid[icell - 1];
  double u, v, w;
  if (!column_direction(dir, x, y, z, u, v, w)) return 0.0f;
  const double a = u * u + v * v;
  const double inv_a = (a > TINY_REAL) ? 1.0 / a : HUGE_REAL;
  const double inv_w = (fabs(w) > TINY_REAL) ? 1.0 / w : copysign(HUGE_DP, w);
  double sum = 0.0;
  bool capped = true;
  for (int it = 0; it < A.cap; ++it) {
    const int azj = zj < 0 ? -zj : zj;
    if ((ri == n_rad + 1) || (!sph && (azj == nz + 1) && (fabs(z) > M.zmaxmax))) { capped = false; break; }  // test_exit_grid
    double x1, y1, z1, l;
    int ri1, zj1, k1;
    if (sph) cross_cell_sph<L3D>(T, M, x, y, z, u, v, w, ri, zj, k, x1, y1, z1, ri1, zj1, k1, l);
    else MCGPU_CROSS<L3D>(T, M, x, y, z, u, v, w, inv_a, inv_w, ri, zj, k, x1, y1, z1, ri1, zj1, k1, l);
    if (is_real_cell<L3D>(n_rad, nz, ri, zj)) {
      const int ic = cell_index<L3D>(n_rad, nz, ri, zj, k);
      double factor;
      if (A.type == 2) {
        const double kap = M.n_classes ? M.v_kappa[(size_t)M.cell_class[ic] * M.n_lambda + (A.lambda - 1)] : T.kappa[A.lambda - 1];
        factor = nd_mul(kap, M.kappa_factor[ic]);
      } else {
        factor = column_gas_factor(A, ic);
      }
      sum = nd_add(sum, nd_mul(l, factor));  // unfused, the reference's order
    }
    x = x1; y = y1; z = z1;
    ri = ri1; zj = zj1; k = k1;
  }
  if (capped) atomicAdd(A.n_capped, 1ull);
  return (float)sum;  // column is a default real
}

__device__ inline float column_ray_voro(const Lds& T, const DevModel& M, const VoroGrid& G, const ColumnArgs& A, int icell, int dir) {
  double x = G.xyz_dp[3 * (size_t)(icell - 1)], y = G.xyz_dp[3 * (size_t)(icell - 1) + 1], z = G.xyz_dp[3 * (size_t)(icell - 1) + 2];
  double u, v, w;
  if (!column_direction(dir, x, y, z, u, v, w)) return 0.0f;
  int next = icell, cur = 0, prev = 0;
  double sum = 0.0;
  bool capped = true;
  for (int it = 0; it < A.cap; ++it) {
    prev = cur;
    cur = next;
    if (cur <= 0 || cur > G.n_cells) { capped = false; break; }  // test_exit_grid (icell < 0: a wall of the box)
    const VoroCell C = G.cell[cur - 1];
    double x1, y1, z1, l, l_contrib, l_void;
    voro_cross_cell(G, M, C, x, y, z, u, v, w, cur, prev, x1, y1, z1, next, l, l_contrib, l_void);
    if (cur <= M.n_cells) {
      double factor;
      if (A.type == 2) {
        const double kap = M.n_classes ? M.v_kappa[(size_t)M.cell_class[cur - 1] * M.n_lambda + (A.lambda - 1)] : T.kappa[A.lambda - 1];
        factor = nd_mul(kap, C.kf);
      } else {
        factor = column_gas_factor(A, cur - 1);
      }
      sum = nd_add(sum, nd_mul(l_contrib, factor));
    }
    x = x1; y = y1; z = z1;
  }
  if (capped) atomicAdd(A.n_capped, 1ull);
  return (float)sum;
}

template <bool L3D>
__global__ void __launch_bounds__(256) k_compute_column(const DevModel M, const ColumnArgs A) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);  // geometry, kappa: the table set of k_tau_maps
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const long n_rays = 4L * M.n_cells;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_rays; t += (long)gridDim.x * blockDim.x) {
    const int d0 = (int)(t / M.n_cells), ic = (int)(t - (long)d0 * M.n_cells);
    A.column[t] = column_ray<L3D>(T, M, A, ic + 1, d0 + 1);
  }
}

__global__ void __launch_bounds__(256) k_compute_column_voro(const DevModel M, const ColumnArgs A, const VoroGrid G) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const long n_rays = 4L * M.n_cells;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_rays; t += (long)gridDim.x * blockDim.x) {
    const int d0 = (int)(t / M.n_cells), ic = (int)(t - (long)d0 * M.n_cells);
    A.column[t] = column_ray_voro(T, M, G, A, ic + 1, d0 + 1);
  }
}

// integ_tau's second direction (:225-227): angle is a default real, the rest double
__device__ inline void integ_tau_direction(int lane, float angle_deg, double& u, double& v, double& w) {
  if (lane == 0) { u = 1.0; v = 0.0; w = 0.0; return; }
  w = cos((double)angle_deg * PI / 180.0);
  u = sqrt(nd_add(1.0, -nd_mul(w, w)));
  v = 0.0;
}

// out[0] = the midplane ray, out[1] = the ray at angle_deg from the axis
template <bool L3D>
__global__ void __launch_bounds__(64) k_integ_tau(const DevModel M, int lambda, float angle_deg, float* out) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane < 2) {
    double u, v, w;
    integ_tau_direction(lane, angle_deg, u, v, w);
    out[lane] = optical_length_tot<L3D>(T, M, lambda, 0.0, 0.0, 0.0, u, v, w);
  }
}

__global__ void __launch_bounds__(64) k_integ_tau_voro(const DevModel M, const VoroGrid G, int lambda, float angle_deg, float* out) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane < 2) {
    double u, v, w;
    integ_tau_direction(lane, angle_deg, u, v, w);
    out[lane] = optical_length_tot_voro(T, M, G, lambda, 0.0, 0.0, 0.0, u, v, w);
  }
}

}  // namespace mcgpu
