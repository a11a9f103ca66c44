// emu_line.cpp -- TEST INFRASTRUCTURE: the line ray tracer's kernels (mcfost_amd/csrc/mc_line.hip.h: k_line_map,
// k_line_map_voro, k_line_sum1) on one emulated lane (the shim of emu_kernel.cpp: WAVE_LANES = 1, so the one lane takes every
// velocity point and every channel in turn), so that the whole walk runs on the CPU before it runs on a device.  Built only by
// tests/test_line_map.py.
#include "emu_kernel.cpp"
#include "../../include/mcgpu.h"
#include "../../mcfost_amd/csrc/mc_line.hip.h"

// The arguments as mcgpu_line_map forms them (mcfost_amd/csrc/mcgpu.hip).  spectrum / continu in the C-ABI's layouts, zeroed
// here; cap_used (may be null) receives column_cap of the grid.
extern "C" int emu_line_map(const oracle_model* m, double ang_disque, double Rmax, const float* tab_RT_az, const mcgpu_line_opts* lo,
                            float* spectrum, float* continu, unsigned long long* n_capped, int* cap_used) {
  Conv cv(m);
  const DevModel& M = cv.M;
  const int nRT = m->RT_n_incl * m->RT_n_az, ns = lo->n_speed, nT = lo->nTrans;
  if ((lds_bytes(M, true) + 7) / 8 * 8 + line_wave_doubles(ns, nT) * sizeof(double) > sizeof(lds_raw)) return 31;
  if ((long long)ns * nT > MCGPU_LINE_MAX_CHANNELS) return MCGPU_ERR_ARG;
  RtArgs R;
  memset(&R, 0, sizeof(R));
  R.RT_n_incl = m->RT_n_incl; R.nRT = nRT; R.ang_disque = ang_disque;
  R.rt_u = m->tab_u_rt; R.rt_v = m->tab_v_rt; R.rt_w = m->tab_w_rt; R.rt_az = tab_RT_az;
  const int npx = lo->method == 2 ? lo->npix_x : 1, npy = lo->method == 2 ? lo->npix_y : 1;
  LineArgs A;
  memset(&A, 0, sizeof(A));
  A.method = lo->method; A.nRT = nRT;
  A.npix_x = npx; A.npix_y = npy;
  A.npix_x_max = (lo->method == 2 && lo->l_sym_ima) ? npx / 2 + npx % 2 : npx;
  A.map_size = lo->map_size;
  A.taille_pix = lo->method == 2 ? (lo->map_size / lo->zoom) / (double)(npx > npy ? npx : npy) : 0.0;
  A.l_far = 10.0 * Rmax;
  A.Rmin = lo->Rmin; A.Rmax = Rmax;
  A.cst_phi = (lo->l_sym_ima ? M_PI : 2.0 * M_PI) / (double)LINE_N_PHI_RT;
  A.inv_dist = 1.0 / (lo->distance_pc * (648000.0 / M_PI));
  A.n_speed = ns; A.nTrans = nT;
  A.tab_speed = lo->tab_speed; A.transfreq = lo->transfreq; A.kappa_mol = lo->kappa_mol_o_freq;
  A.emis_mol = lo->emissivite_mol_o_freq; A.emis_dust = lo->emissivite_dust; A.kabs_LTE = lo->kappa_abs_LTE;
  A.p_n_cells = M.n_classes ? M.n_classes : 1;
  A.norme_m1 = lo->norme_phiProf_m1; A.sigma2_m1 = lo->sigma2_phiProf_m1; A.dv_line = lo->dv_line;
  A.vfield_mode = lo->vfield_mode; A.lkeplerian = lo->lkeplerian; A.linfall = lo->linfall; A.vfield_coord = lo->vfield_coord;
  A.chi_infall = lo->chi_infall; A.vfield = lo->vfield; A.vxyz = lo->vxyz;
  A.lonly_top = lo->lonly_top; A.lonly_bottom = lo->lonly_bottom;
  A.cap = column_cap(M.n_rad, M.nz, M.n_az, M.n_cells, cv.voro);
  if (cap_used) *cap_used = A.cap;
  const size_t n_cont = (size_t)npx * npy * nT * nRT;
  if (spectrum) memset(spectrum, 0, sizeof(float) * n_cont * ns);
  if (continu) memset(continu, 0, sizeof(float) * n_cont);
  A.spectrum = spectrum; A.continu = continu;
  unsigned long long capped = 0ull;
  A.n_capped = &capped;
  std::vector<double> rays;
  if (lo->method == 1) {
    rays.resize((size_t)nRT * LINE_N_RAD_RT * LINE_N_PHI_RT * nT * (ns + 1));
    A.rays = rays.data();
  }
  gridDim.x = 1; blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  if (cv.voro) k_line_map_voro(M, R, A, cv.G);
  else if (m->l3D) k_line_map<true>(M, R, A);
  else k_line_map<false>(M, R, A);
  if (lo->method == 1) {
    const long n_val = (long)nRT * nT * (ns + 1);
    for (long t = 0; t < n_val; ++t) { blockIdx.x = (unsigned)t; k_line_sum1(A); }
    blockIdx.x = 0;
  }
  if (n_capped) *n_capped = capped;
  return 0;
}
