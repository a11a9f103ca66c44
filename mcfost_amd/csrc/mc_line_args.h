// The arguments of the line ray tracer's kernels (mc_line.hip.h) and the sizes of a wave's share of the LDS: plain host /
// device declarations, shared by the unit of the kernels (kern_line.hip) and the unit of the launchers (mcgpu.hip), which
// needs no kernel of the family.
#pragma once
#include <stddef.h>

namespace mcgpu {

constexpr int LINE_N_VPOINTS_MAX = 200;   // n_vpoints_max (optical_depth.f90:873)
constexpr int LINE_N_RAD_RT = 100, LINE_N_PHI_RT = 36;   // method 1 (mol_transfer.f90:502)
constexpr int LINE_MAX_CHANNELS = 1024;   // the cap on n_speed * nTrans (MCGPU_LINE_MAX_CHANNELS, include/mcgpu.h)

struct LineArgs {
  // observers and the image plane (the fields rt_image_plane reads are those of RtArgs, filled by the launcher)
  int method;                    // 1: log-sampled spectrum, 2: pixels
  int npix_x, npix_y, npix_x_max;
  int nRT;
  double map_size, taille_pix;   // AU; (map_size / zoom) / max(npix_x, npix_y) (mol_transfer.f90:636)
  double l_far;                  // 10 Rmax
  double Rmin, Rmax;
  double cst_phi;                // method 1: pi / 36 (l_sym_ima) or 2 pi / 36
  double inv_dist;               // 1 / (distance * pc_to_AU)
  // the molecule
  int n_speed, nTrans;
  const double* tab_speed;       // [n_speed] m/s
  const double* transfreq;       // [nTrans]
  const double* kappa_mol;       // kappa_mol_o_freq(n_cells, nTrans)
  const double* emis_mol;        // emissivite_mol_o_freq(n_cells, nTrans)
  const double* emis_dust;       // emissivite_dust(n_cells, nTrans)
  const double* kabs_LTE;        // kappa_abs_LTE(p_n_cells, nTrans)
  int p_n_cells;
  const double* norme_m1;        // norme_phiProf_m1(n_cells)
  const double* sigma2_m1;       // sigma2_phiProf_m1(n_cells)
  const float* dv_line;          // dv_line(n_cells), default real
  // the velocity field
  int vfield_mode;               // 1: analytic, 2: vfield3d (Voronoi grids: vxyz)
  int lkeplerian, linfall, vfield_coord;
  float chi_infall;
  const float* vfield;           // vfield(n_cells) or vfield3d(n_cells, 3)
  const double* vxyz;            // vxyz(3, n_cells)
  int lonly_top, lonly_bottom;
  int cap;                       // column_cap (mc_column_args.h)
  // outputs
  float* spectrum;               // (npix_x, npix_y, n_speed, nTrans, nRT) or null
  float* continu;                // (npix_x, npix_y, nTrans, nRT) or null
  double* rays;                  // method 1: [nRT * 3600][nTrans][n_speed + 1], the continuum in place n_speed
  unsigned long long* n_capped;
};

// doubles of LDS that one wave of the line kernels owns: the projected velocities of a step and, per transition and
// channel (the continuum is channel n_speed), tau and I0
constexpr size_t line_wave_doubles(int n_speed, int nTrans) {
  return (size_t)LINE_N_VPOINTS_MAX + 2 * (size_t)(n_speed + 1) * (size_t)nTrans;
}

}  // namespace mcgpu
