// emu_mono_xj.cpp -- TEST INFRASTRUCTURE: the SED commit pass that also keeps the mean radiation field (k_mono_xj,
// k_mono_sph_xj, k_mono_voro_xj: mono_body's XJ, mc_mono.hip.h "The mean radiation field") on one emulated lane (the shim
// of emu_kernel.cpp).  The scout passes run the plain kernels, as mcgpu_run_mono's do; the commit pass deposits
// xJ_abs / xN_abs of the wavelength into the caller's rows next to xI_scatt (rt1 = 1), I_spec (rt1 = 2) or nothing
// (rt1 = 0).  The emulation takes the HBM path: one lane has no LDS atomics to speak of.  Built only by
// tests/test_sed_radiation_field_emulated.py.
#include "emu_kernel.cpp"

// xJ, xN: [n_cells] rows of the wavelength (added to); xN may be null.  o->rt1: 0, 1 or 2 (then o->n_theta_I, o->n_phi_I).
extern "C" int emu_run_mono_xj(const oracle_model* m, const oracle_mono_opts* o, double* xJ, unsigned int* xN, double* sed,
                               double* n_sent, uint64_t* n_sent_chunk, uint64_t* counters) {
  Conv cv(m);
  const DevModel& M = cv.M;
  const VoroGrid& G = cv.G;
  const bool voro = cv.voro;
  const bool rt1 = o->rt1 == 1, rt2 = o->rt1 == 2;
  if (rt2 && (m->l3D || voro)) return 31;

  const size_t nsed = (size_t)9 * m->n_lambda * m->N_thet * m->N_phi;
  const int nRT = m->RT_n_incl * m->RT_n_az;
  memset(sed, 0, sizeof(double) * nsed);
  memset(n_sent, 0, sizeof(double) * m->n_lambda);
  const bool pola = m->lsepar_pola && m->aniso_method == 1, dark = M.dark != nullptr, l3d = m->l3D != 0;
  const Xi32Lay xi_lay = xi32_layout(nRT ? nRT : 1, pola, m->lsepar_contrib != 0);
  std::vector<double> xI_dev(rt1 ? (size_t)m->n_cells * m->n_theta_rt * m->n_az_rt * nRT * XI_LINE : 1, 0.0);
  std::vector<double> I_spec(rt2 ? (size_t)m->n_cells * o->n_phi_I * o->n_theta_I * XI_LINE : 1, 0.0), I_star(m->n_cells, 0.0);
  unsigned long long cnt[24];
  memset(cnt, 0, sizeof(cnt));
  int err = 0;
  MonoArgs A;
  memset(&A, 0, sizeof(A));
  A.seed = o->seed; A.lambda = o->lambda; A.p_lambda = o->p_lambda; A.capt_sup = o->capt_sup; A.rt1 = rt1 ? 1 : 0;
  A.frac_E_stars = m->frac_E_stars[o->lambda - 1]; A.frac_E_disk = m->frac_E_disk[o->lambda - 1];
  A.prob_E_cell = m->prob_E_cell ? m->prob_E_cell + (size_t)(m->n_cells + 1) * (o->lambda - 1) : nullptr;
  A.n_chunks = o->n_chunks; A.first_chunk = o->first_chunk;
  A.RT_n_incl = m->RT_n_incl > 0 ? m->RT_n_incl : 1; A.nRT = rt1 ? nRT : 0;
  A.rt_u = m->tab_u_rt; A.rt_v = m->tab_v_rt; A.rt_w = m->tab_w_rt;
  A.n_az_rt = m->n_az_rt; A.n_theta_rt = m->n_theta_rt; A.N_type_flux = m->N_type_flux; A.contrib = m->lsepar_contrib;
  A.s11 = m->tab_s11_pos ? m->tab_s11_pos + (size_t)(m->nang_scatt + 1) * (o->p_lambda - 1) : nullptr;
  A.xI = xI_dev.data(); A.xI_f32 = 0; A.xi = xi_lay;
  if (rt2) {   // (mcgpu_set_rt2's N_type_flux)
    A.rt2 = 1; A.n_theta_I = o->n_theta_I; A.n_phi_I = o->n_phi_I; A.I_spec = I_spec.data(); A.I_spec_star = I_star.data();
    A.N_type_flux = (pola ? 4 : 1) + (m->lsepar_contrib ? 4 : 0);
  }
  A.sed = sed; A.n_sent = n_sent; A.counters = cnt; A.next_item = cnt + 8; A.err = &err;
  A.inner_iters = 8; A.min_active = 0;
#define SCOUT_RUN() do {                                                                                           \
    if (voro) { if (pola) k_mono_voro<true, true>(M, A, G); else k_mono_voro<false, true>(M, A, G); }              \
    else if (M.grid_sph) {                                                                                         \
      if (l3d) { if (pola) k_mono_sph<true, true, true>(M, A); else k_mono_sph<true, false, true>(M, A); }          \
      else { if (pola) k_mono_sph<false, true, true>(M, A); else k_mono_sph<false, false, true>(M, A); }            \
    } else if (l3d) {                                                                                              \
      if (pola) { if (dark) k_mono<true, true, true, true>(M, A); else k_mono<true, true, false, true>(M, A); }    \
      else { if (dark) k_mono<true, false, true, true>(M, A); else k_mono<true, false, false, true>(M, A); }       \
    } else {                                                                                                       \
      if (pola) { if (dark) k_mono<false, true, true, true>(M, A); else k_mono<false, true, false, true>(M, A); }  \
      else { if (dark) k_mono<false, false, true, true>(M, A); else k_mono<false, false, false, true>(M, A); }     \
    } } while (0)
#define COMMIT_RUN() do {                                                                                                      \
    if (voro) { if (pola) k_mono_voro_xj<true, false>(M, A, G); else k_mono_voro_xj<false, false>(M, A, G); }                  \
    else if (M.grid_sph) {                                                                                                     \
      if (l3d) { if (pola) k_mono_sph_xj<true, true, false>(M, A); else k_mono_sph_xj<true, false, false>(M, A); }              \
      else { if (pola) k_mono_sph_xj<false, true, false>(M, A); else k_mono_sph_xj<false, false, false>(M, A); }                \
    } else if (l3d) {                                                                                                          \
      if (pola) { if (dark) k_mono_xj<true, true, true, false>(M, A); else k_mono_xj<true, true, false, false>(M, A); }        \
      else { if (dark) k_mono_xj<true, false, true, false>(M, A); else k_mono_xj<true, false, false, false>(M, A); }           \
    } else {                                                                                                                   \
      if (pola) { if (dark) k_mono_xj<false, true, true, false>(M, A); else k_mono_xj<false, true, false, false>(M, A); }      \
      else { if (dark) k_mono_xj<false, false, true, false>(M, A); else k_mono_xj<false, false, false, false>(M, A); }         \
    } } while (0)
  const int nc = o->n_chunks;
  const unsigned long long lim = (unsigned long long)std::ceil(o->n_phot_lim);
  std::vector<unsigned long long> need(nc, (unsigned long long)o->n_photons2), sent(nc, 0ull), base(nc + 1, 0ull);
  std::vector<int> active;
  if (o->n_photons2 > 0 && lim > 0) for (int c = 0; c < nc; ++c) active.push_back(c);
  while (!active.empty()) {
    const int na = (int)active.size();
    const unsigned long long batch = 64;
    std::vector<unsigned char> hits((size_t)na * batch, 0);
    A.active = active.data(); A.seq0 = sent.data(); A.batch = batch; A.hits = hits.data(); A.n_items = (size_t)na * batch;
    cnt[8] = 0;
    SCOUT_RUN();
    if (err) return err;
    std::vector<int> still;
    for (int a = 0; a < na; ++a) {  // what k_mono_scan does with one wave per stream
      const int c = active[a];
      unsigned long long usable = batch;
      if (sent[c] + batch >= lim) usable = lim > sent[c] ? lim - sent[c] : 0;
      unsigned long long s = 0;
      bool fin = false;
      for (; s < usable; ++s)
        if (hits[(size_t)a * batch + s] && --need[c] == 0) { ++s; fin = true; break; }
      if (!fin && usable < batch) { s = usable; fin = true; }
      sent[c] += fin ? s : batch;
      if (!fin) still.push_back(c);
    }
    active.swap(still);
  }
  for (int c = 0; c < nc; ++c) { base[c + 1] = base[c] + sent[c]; n_sent_chunk[c] = sent[c]; }
  A.item_base = base.data(); A.n_items = base[nc]; A.active = nullptr; A.seq0 = nullptr; A.hits = nullptr; A.batch = 0;
  A.xJ = xJ; A.xN = xN; A.xj_lds = 0;   // (the scout passes above never saw them)
  cnt[8] = 0;
  if (A.n_items) COMMIT_RUN();
#undef SCOUT_RUN
#undef COMMIT_RUN
  for (int q = 0; q < 8; ++q) counters[q] = cnt[q];
  return err;
}
