// Molecular line channel maps: emission_line_map (mol_transfer.f90:484-687) with intensite_pixel_mol (:691-847), integ_ray_mol
// (optical_depth.f90:419-599), local_line_profile (:863-927), phiProf (molecular_emission.f90:183-207) and v_proj (:675-775).
//   k_line_map<L3D>   cylindrical and spherical grids (the grid's operators picked at run time, as k_tau_maps does);
//   k_line_map_voro   Voronoi grids (previous_cell = 0 at every step, one velocity point per cell).
//   k_line_sum1       method 1: the 3600 rays of an observer summed from their buffer in the reference's loop order.
// One WAVE per ray, the lanes are the velocity channels:
//   - the ray (pixel centre, move_to_grid backwards from 10 Rmax, intersect_stars, the crossings, test_exit_grid) is computed
//     by every lane with the same operands: wave-uniform, no divergence, the walk of k_tau_maps;
//   - per step, v_proj at the two ends gives n_vpoints; the inner points are computed one per lane, strided by WAVE_LANES,
//     and shared through the wave's LDS (vel[200]);
//   - channel iv = lane, lane + WAVE_LANES, ... <= n_speed forms its own profile (n_vpoints exp), and per transition
//     opacity, dtau, Snu, I0 and tau (two more exp), in double, in the reference's order of operations (nd_mul / nd_add:
//     products and sums that no build fuses).  Channel n_speed is the CONTINUUM: the same code with a profile of exactly 0
//     gives kappa_cont, dtau_c, Snu_c, I0c and tau_c of (:524-551) without a second code path, so a channel whose profile
//     underflows to 0 equals the continuum bit for bit;
//   - tau and I0 of every (channel, transition) live in the wave's LDS, [transition][channel]: a lane reads and writes only
//     its own channels (no synchronisation, consecutive lanes on consecutive banks), and the same source runs with
//     WAVE_LANES = 1 on the emulated lane.  A wave owns 200 + 2 (n_speed + 1) nTrans doubles (line_wave_doubles).
// No atomics in the sums; n_capped is the only atomic.
// Departures from the reference: include/mcgpu.h (mcgpu_line_map).
#pragma once
#include "mc_column_args.h"
#include "mc_line_args.h"
#include "mc_raytrace.hip.h"
#include "mc_voronoi.hip.h"

namespace mcgpu {

// the order between one lane's writes of vel[] and the other lanes' reads: a wave executes its LDS instructions in order
__device__ __forceinline__ void line_wave_sync() {
#ifndef MCGPU_LANE_EMULATION
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
#endif
}

// v_proj (molecular_emission.f90:675-775) of cell ic (0-based) at (x, y, z) along (u, v, w)
template <bool L3D, bool VORO>
__device__ inline double line_v_proj(const LineArgs& A, int n_cells, int ic, double x, double y, double z, double u, double v,
                                     double w) {
  if (VORO) {
    const double* p = A.vxyz + 3 * (size_t)ic;
    return nd_add(nd_add(nd_mul(p[0], u), nd_mul(p[1], v)), nd_mul(p[2], w));
  }
  double vx, vy, vz;
  if (A.vfield_mode == 2) {
    const double a1 = (double)A.vfield[ic], a2 = (double)A.vfield[ic + (size_t)n_cells], a3 = (double)A.vfield[ic + 2 * (size_t)n_cells];
    if (A.vfield_coord == 1) {
      vx = a1; vy = a2; vz = a3;
    } else if (A.vfield_coord == 2) {
      const double phi = atan2(y, x);
      double sp, cp;
      sincos(phi, &sp, &cp);
      vx = nd_add(nd_mul(cp, a1), -nd_mul(sp, a2));
      vy = nd_add(nd_mul(sp, a1), nd_mul(cp, a2));
      vz = (!L3D && z < 0.0) ? -a3 : a3;
    } else {
      const double v_theta = (!L3D && z < 0.0) ? -a3 : a3;
      const double rcyl2 = nd_add(nd_mul(x, x), nd_mul(y, y));
      const double r2 = nd_add(rcyl2, nd_mul(z, z));
      const double rcyl = sqrt(rcyl2), r = sqrt(r2);
      const double cos_theta = rcyl / r, sin_theta = z / r;
      const double cos_phi = x / rcyl, sin_phi = y / rcyl;
      vz = nd_add(nd_mul(-v_theta, cos_theta), nd_mul(a1, sin_theta));
      const double v_rcyl = nd_add(nd_mul(v_theta, sin_theta), nd_mul(a1, cos_theta));
      vx = nd_add(nd_mul(v_rcyl, cos_phi), -nd_mul(a2, sin_phi));
      vy = nd_add(nd_mul(v_rcyl, sin_phi), nd_mul(a2, cos_phi));
    }
    return nd_add(nd_add(nd_mul(vx, u), nd_mul(vy, v)), nd_mul(vz, w));
  }
  const double velocity = (double)A.vfield[ic];
  if (A.lkeplerian) {
    double r = sqrt(nd_add(nd_mul(x, x), nd_mul(y, y)));
    if (!(r > TINY_DP)) return 0.0;
    double norm = 1.0 / r;
    vx = nd_mul(nd_mul(-y, norm), velocity);
    vy = nd_mul(nd_mul(x, norm), velocity);
    if (!A.linfall) return nd_add(nd_mul(vx, u), nd_mul(vy, v));
    r = sqrt(nd_add(nd_add(nd_mul(x, x), nd_mul(y, y)), nd_mul(z, z)));
    norm = 1.0 / r;
    const double chi = (double)A.chi_infall;
    vx = nd_add(vx, -nd_mul(nd_mul(nd_mul(chi, x), norm), velocity));
    vy = nd_add(vy, -nd_mul(nd_mul(nd_mul(chi, y), norm), velocity));
    vz = nd_add(0.0, -nd_mul(nd_mul(nd_mul(chi, z), norm), velocity));
    return nd_add(nd_add(nd_mul(vx, u), nd_mul(vy, v)), nd_mul(vz, w));
  }
  // linfall alone (the launcher refuses a field that is neither)
  const double r = sqrt(nd_add(nd_add(nd_mul(x, x), nd_mul(y, y)), nd_mul(z, z)));
  if (!(r > TINY_DP)) return 0.0;
  const double norm = 1.0 / r;
  vx = nd_mul(nd_mul(x, norm), velocity);
  vy = nd_mul(nd_mul(y, norm), velocity);
  vz = nd_mul(nd_mul(z, norm), velocity);
  return nd_add(nd_add(nd_mul(vx, u), nd_mul(vy, v)), nd_mul(vz, w));
}

// n_vpoints (optical_depth.f90:889-893): dv a default real, the quotient in single precision, nint half away from zero
__device__ inline int line_n_vpoints(double v0, double v1, float dv_line) {
  const float dv = (float)fabs(nd_add(v1, -v0));
  const float q = nf_mul(dv / dv_line, 20.0f);
  if (!(q < (float)LINE_N_VPOINTS_MAX)) return LINE_N_VPOINTS_MAX;   // (also a quotient that is no number)
  const int n = (int)roundf(q);
  return n < 2 ? 2 : n;
}

// One cell of integ_ray_mol (:505-552) for the channels of this lane.  The step goes from (x0, y0, z0) over l_void_before,
// then l_contrib inside cell ic (0-based); kf = kappa_factor(icell); W = the wave's LDS.
template <bool L3D, bool VORO>
__device__ inline void line_cell(const DevModel& M, const LineArgs& A, double* W, int lane, int ic, double kf, double x0, double y0,
                                 double z0, double x1, double y1, double z1, double u, double v, double w, double l_void,
                                 double l_contrib) {
  double* vel = W;
  double* tau = W + LINE_N_VPOINTS_MAX;
  const int nch = A.n_speed + 1;
  double* I0 = tau + (size_t)nch * A.nTrans;
  const int n_cells = M.n_cells;
  const double v0 = line_v_proj<L3D, VORO>(A, n_cells, ic, x0, y0, z0, u, v, w);
  int n_vp = 1;
  line_wave_sync();   // (the reads of the step before are done)
  if (VORO) {
    if (lane == 0) vel[0] = v0;
  } else {
    const double v1 = line_v_proj<L3D, VORO>(A, n_cells, ic, x1, y1, z1, u, v, w);
    n_vp = line_n_vpoints(v0, v1, A.dv_line[ic]);
    for (int ivp = 2 + lane; ivp <= n_vp - 1; ivp += WAVE_LANES) {
      const double d = nd_add(l_void, nd_mul((double)ivp / (double)n_vp, l_contrib));
      vel[ivp - 1] = line_v_proj<L3D, VORO>(A, n_cells, ic, nd_add(x0, nd_mul(d, u)), nd_add(y0, nd_mul(d, v)),
                                            nd_add(z0, nd_mul(d, w)), u, v, w);
    }
    if (lane == 0) { vel[0] = v0; vel[n_vp - 1] = v1; }
  }
  line_wave_sync();
  double ft = 1.0;                                   // facteur_tau (:517-519)
  if (A.lonly_top && z0 < 0.0) ft = 0.0;
  if (A.lonly_bottom && z0 > 0.0) ft = 0.0;
  const double norme = A.norme_m1[ic], s2 = A.sigma2_m1[ic];
  const int icl = A.p_n_cells > 1 ? M.cell_class[ic] : 0;
  for (int iv = lane; iv < nch; iv += WAVE_LANES) {
    double P = 0.0;
    if (iv < A.n_speed) {
      const double ts = A.tab_speed[iv];
      for (int p = 0; p < n_vp; ++p) {
        const double t = nd_add(ts, -vel[p]);
        P = nd_add(P, nd_mul(norme, exp(-nd_mul(s2, nd_mul(t, t)))));
      }
      P = P / (double)n_vp;
    }
    for (int it = 0; it < A.nTrans; ++it) {
      const size_t row = (size_t)ic + (size_t)n_cells * it;
      const double kappa_cont = nd_mul(A.kabs_LTE[icl + (size_t)A.p_n_cells * it], kf);
      const double opacity = nd_add(nd_mul(nd_mul(A.kappa_mol[row], P), ft), kappa_cont);
      const double dtau = nd_mul(l_contrib, opacity);
      const double Snu = nd_add(nd_mul(nd_mul(A.emis_mol[row], P), ft), A.emis_dust[row]) / nd_add(opacity, 1.0e-300);
      const int s = it * nch + iv;
      const double t0 = tau[s];
      I0[s] = nd_add(I0[s], nd_mul(nd_mul(exp(-t0), nd_add(1.0, -exp(-dtau))), Snu));
      tau[s] = nd_add(t0, dtau);
    }
  }
}

// the start of ray `ray` of the launch: observer q, the point on the image plane, the pixel's size and its place
__device__ inline void line_ray_start(const RtArgs& R, const LineArgs& A, long ray, int& q, double pc[3], double uvw[3],
                                      double& pixelsize, long& ipix) {
  double xpi[3], ypi[3];
  if (A.method == 2) {
    const long per_dir = (long)A.npix_x_max * A.npix_y;
    q = (int)(ray / per_dir);
    const long rem = ray - (long)q * per_dir;
    const int j = (int)(rem / A.npix_x_max) + 1, i = (int)(rem - (long)(j - 1) * A.npix_x_max) + 1;
    rt_image_plane(R, q, uvw, xpi, ypi);
    for (int c = 0; c < 3; ++c) {
      const double dx = nd_mul(xpi[c], A.taille_pix), dy = nd_mul(ypi[c], A.taille_pix);
      const double Icorner = nd_add(nd_mul(uvw[c], A.l_far), -nd_mul(nd_mul(0.5, A.map_size), nd_add(xpi[c], ypi[c])));   // (:572)
      const double corner = nd_add(nd_add(Icorner, nd_mul((double)(i - 1), dx)), nd_mul((double)(j - 1), dy));          // (:663)
      pc[c] = nd_add(nd_add(corner, nd_mul(0.5, dx)), nd_mul(0.5, dy));                                                 // (:762-764)
    }
    pixelsize = A.taille_pix;
    ipix = (i - 1) + (long)A.npix_x * (j - 1);
  } else {
    const int per_dir = LINE_N_RAD_RT * LINE_N_PHI_RT;
    q = (int)(ray / per_dir);
    const int rem = (int)(ray - (long)q * per_dir);
    const int ri_RT = rem / LINE_N_PHI_RT + 1, phi_RT = rem - (ri_RT - 1) * LINE_N_PHI_RT + 1;
    rt_image_plane(R, q, uvw, xpi, ypi);
    const double rmin_RT = nd_mul(fmax(nd_mul(uvw[2], 0.9), 0.05), A.Rmin), rmax_RT = nd_mul(2.0, A.Rmax);   // (:589-590)
    const double fact_r = exp(nd_mul(1.0 / ((double)LINE_N_RAD_RT - 1.0), log(rmax_RT / rmin_RT)));
    double r = rmin_RT;
    for (int k = 2; k <= ri_RT; ++k) r = nd_mul(r, fact_r);
    const double fact_A = sqrt(nd_mul(PI, nd_add(fact_r, -1.0 / fact_r)) / (double)LINE_N_PHI_RT);
    pixelsize = nd_mul(fact_A, r);
    const double phi = nd_mul(A.cst_phi, (double)phi_RT - 0.5);
    double sp, cp;
    sincos(phi, &sp, &cp);
    for (int c = 0; c < 3; ++c)
      pc[c] = nd_add(nd_add(nd_mul(uvw[c], A.l_far), nd_mul(nd_mul(r, sp), xpi[c])), nd_mul(nd_mul(r, cp), ypi[c]));     // (:625)
    ipix = 0;
  }
}

// the ray's result: I0 * (pixelsize / (distance pc_to_AU))^2 * transfreq (:824-833)
__device__ inline void line_store(const LineArgs& A, const double* W, int lane, long ray, int q, double pixelsize, long ipix) {
  const int nch = A.n_speed + 1;
  const double* I0 = W + LINE_N_VPOINTS_MAX + (size_t)nch * A.nTrans;
  const double sr = nd_mul(pixelsize, A.inv_dist);
  const double sr2 = nd_mul(sr, sr);
  const size_t npix = (size_t)A.npix_x * A.npix_y;
  for (int iv = lane; iv < nch; iv += WAVE_LANES) {
    for (int it = 0; it < A.nTrans; ++it) {
      const double val = nd_mul(nd_mul(I0[it * nch + iv], sr2), A.transfreq[it]);
      if (A.method != 2) {
        A.rays[((size_t)ray * A.nTrans + it) * nch + iv] = val;
      } else if (iv < A.n_speed) {
        if (A.spectrum) A.spectrum[ipix + npix * ((size_t)iv + (size_t)A.n_speed * (it + (size_t)A.nTrans * q))] = (float)val;
      } else if (A.continu) {
        A.continu[ipix + npix * (it + (size_t)A.nTrans * q)] = (float)val;
      }
    }
  }
}

__device__ inline void line_clear(const LineArgs& A, double* W, int lane) {
  const int n = 2 * (A.n_speed + 1) * A.nTrans;
  for (int s = lane; s < n; s += WAVE_LANES) W[LINE_N_VPOINTS_MAX + s] = 0.0;
}

// where the wave's share of the LDS begins (behind the tables of lds_carve, on a multiple of 8 bytes)
__device__ inline double* line_wave_lds(double* lds_raw, const DevModel& M, const LineArgs& A, int wave) {
  return lds_raw + (lds_bytes(M, true) + 7) / 8 + (size_t)wave * line_wave_doubles(A.n_speed, A.nTrans);
}

template <bool L3D>
__global__ void __launch_bounds__(256) k_line_map(const DevModel M, const RtArgs R, const LineArgs A) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const int n_rad = M.n_rad, nz = M.nz;
  const bool sph = M.grid_sph != 0;
  const int lane = threadIdx.x % WAVE_LANES, wave = threadIdx.x / WAVE_LANES, waves = blockDim.x / WAVE_LANES;
  double* W = line_wave_lds(lds_raw, M, A, wave);
  const long n_rays = A.method == 2 ? (long)A.nRT * A.npix_x_max * A.npix_y : (long)A.nRT * LINE_N_RAD_RT * LINE_N_PHI_RT;
  for (long ray = (long)blockIdx.x * waves + wave; ray < n_rays; ray += (long)gridDim.x * waves) {
    int q;
    long ipix;
    double pc[3], uvw[3], pixelsize;
    line_ray_start(R, A, ray, q, pc, uvw, pixelsize, ipix);
    const double u = -uvw[0], v = -uvw[1], w = -uvw[2];  // reverse propagation
    double x = pc[0], y = pc[1], z = pc[2];
    line_clear(A, W, lane);
    int ri, zj, k;
    const bool hit = sph ? move_to_grid_sph<L3D>(T, M, x, y, z, u, v, w, ri, zj, k) : move_to_grid<L3D>(T, M, x, y, z, u, v, w, ri, zj, k);
    if (hit) {
      const double a = u * u + v * v;
      const double inv_a = (a > TINY_REAL) ? 1.0 / a : HUGE_REAL;
      const double inv_w = (fabs(w) > TINY_REAL) ? 1.0 / w : copysign(HUGE_DP, w);
      const int i_star = intersect_stars(M, x, y, z, u, v, w);
      int star_key = -1;
      if (i_star > 0) {
        const int* sc = &M.star_cell[4 * (i_star - 1)];
        star_key = sc[0] + (n_rad + 2) * ((sc[1] + nz + 1) + (2 * nz + 3) * (sc[2] - 1));
      }
      bool capped = true;
      for (int it = 0; it < A.cap; ++it) {
        const int azj = zj < 0 ? -zj : zj;
        if ((ri == n_rad + 1) || (!sph && (azj == nz + 1) && (fabs(z) > M.zmaxmax))) { capped = false; break; }  // test_exit_grid
        if (star_key >= 0 && (ri + (n_rad + 2) * ((zj + nz + 1) + (2 * nz + 3) * (k - 1))) == star_key) { capped = false; break; }
        double x1, y1, z1, l;
        int ri1, zj1, k1;
        if (sph) cross_cell_sph<L3D>(T, M, x, y, z, u, v, w, ri, zj, k, x1, y1, z1, ri1, zj1, k1, l);
        else MCGPU_CROSS<L3D>(T, M, x, y, z, u, v, w, inv_a, inv_w, ri, zj, k, x1, y1, z1, ri1, zj1, k1, l);
        if (is_real_cell<L3D>(n_rad, nz, ri, zj)) {
          const int ic = cell_index<L3D>(n_rad, nz, ri, zj, k);
          line_cell<L3D, false>(M, A, W, lane, ic, M.kappa_factor[ic], x, y, z, x1, y1, z1, u, v, w, 0.0, l);
        }
        x = x1; y = y1; z = z1;
        ri = ri1; zj = zj1; k = k1;
      }
      if (capped && lane == 0) atomicAdd(A.n_capped, 1ull);
    }
    line_store(A, W, lane, ray, q, pixelsize, ipix);
  }
}

__global__ void __launch_bounds__(256) k_line_map_voro(const DevModel M, const RtArgs R, const LineArgs A, const VoroGrid G) {
  extern __shared__ double lds_raw[];
  const Lds T = lds_carve(lds_raw, M, true);
  lds_stage_mono(T, M, 1);
  __syncthreads();
  const int lane = threadIdx.x % WAVE_LANES, wave = threadIdx.x / WAVE_LANES, waves = blockDim.x / WAVE_LANES;
  double* W = line_wave_lds(lds_raw, M, A, wave);
  const long n_rays = A.method == 2 ? (long)A.nRT * A.npix_x_max * A.npix_y : (long)A.nRT * LINE_N_RAD_RT * LINE_N_PHI_RT;
  for (long ray = (long)blockIdx.x * waves + wave; ray < n_rays; ray += (long)gridDim.x * waves) {
    int q;
    long ipix;
    double pc[3], uvw[3], pixelsize;
    line_ray_start(R, A, ray, q, pc, uvw, pixelsize, ipix);
    const double u = -uvw[0], v = -uvw[1], w = -uvw[2];
    double x = pc[0], y = pc[1], z = pc[2];
    line_clear(A, W, lane);
    int icell = 0;
    if (voro_move_to_grid(G, x, y, z, u, v, w, icell)) {
      const int i_star = intersect_stars(M, x, y, z, u, v, w);
      const int star_icell = (i_star > 0) ? M.star_cell[4 * (i_star - 1)] : 0;
      bool capped = true;
      for (int it = 0; it < A.cap; ++it) {
        if (icell < 0) { capped = false; break; }                                    // test_exit_grid
        if (star_icell > 0 && icell == star_icell) { capped = false; break; }
        const VoroCell C = G.cell[icell - 1];
        double x1, y1, z1, l, l_contrib, l_void;
        int next;
        voro_cross_cell(G, M, C, x, y, z, u, v, w, icell, 0, x1, y1, z1, next, l, l_contrib, l_void);  // (previous_cell = 0, :502)
        if (icell <= M.n_cells)
          line_cell<true, true>(M, A, W, lane, icell - 1, C.kf, x, y, z, x1, y1, z1, u, v, w, l_void, l_contrib);
        x = x1; y = y1; z = z1;
        icell = next;
      }
      if (capped && lane == 0) atomicAdd(A.n_capped, 1ull);
    }
    line_store(A, W, lane, ray, q, pixelsize, ipix);
  }
}

// method 1 (:837-839): spectrum(1, 1, iv, it, q) = the rays' values added one after the other in the reference's loop
// order (radius outer, azimuth inner) to a DEFAULT REAL, as `spectrum = spectrum + IP` does; one thread per value
static __global__ void __launch_bounds__(256) k_line_sum1(const LineArgs A) {
  const int nch = A.n_speed + 1, per_dir = LINE_N_RAD_RT * LINE_N_PHI_RT;
  const long n = (long)A.nRT * A.nTrans * nch;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int iv = (int)(t % nch), it = (int)((t / nch) % A.nTrans), q = (int)(t / ((long)nch * A.nTrans));
  float s = 0.0f;
  for (int r = 0; r < per_dir; ++r) s = (float)nd_add((double)s, A.rays[(((size_t)q * per_dir + r) * A.nTrans + it) * nch + iv]);
  if (iv < A.n_speed) { if (A.spectrum) A.spectrum[(size_t)iv + (size_t)A.n_speed * (it + (size_t)A.nTrans * q)] = s; }
  else if (A.continu) A.continu[it + (size_t)A.nTrans * q] = s;
}

}  // namespace mcgpu
