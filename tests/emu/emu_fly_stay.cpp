// emu_fly_stay.cpp -- TEST INFRASTRUCTURE: the 2D role kernels (mc_roles.hip.h) on one emulated lane (the shim of
// emu_kernel.cpp) with RunArgs::fly_stay given: the flying waves' lean re-entry against a full round at every visit.  The
// emulation runs the plain instantiations, which the library builds without lean re-entries; MCGPU_LEAN_PLAIN compiles
// them in here, so that the schedule's logic -- the control word, the stay's count, the fold clock, the hand-over seen from
// a lean round -- runs on the host.  Built only by tests/test_fly_stay_emulated.py.
#define MCGPU_LEAN_PLAIN 1
static unsigned long long g_lean_rounds = 0ull;   // visits of the rings that skipped the full round
#define MCGPU_LEAN_TEST_HOOK(taken) do { if (taken) ++g_lean_rounds; } while (0)
#include "emu_kernel.cpp"

// As emu_run_thermal's role schedule (MCGPU_EMU_ROLES): n_srv_pref, k_short, fly_iters, emit_qmax; 2D, LDS deposits, one
// dust class.  n_srv_pref = 0: the one wave prefers to fly, so it is the wave that re-enters.  tail_thr > 0: the kernel that
// hands its last packets over (k_thermal_roles_tail), finished by k_tail.
extern "C" int emu_run_roles_stay(const oracle_model* m, const oracle_opts* o, const double* E_prior, int fly_stay, int nsp,
                                  int ks, int fi, int eq, int tail_thr, double* E_abs, double* sed, double* n_sent,
                                  uint64_t* counters, uint64_t* lean_rounds) {
  g_lean_rounds = 0ull;
  Conv cv(m);
  const DevModel& M = cv.M;
  if (cv.voro || M.grid_sph || M.n_classes || m->l3D) return 31;
  const int n_rec = RQ_MIN_REC;
  if (lds_bytes(M) + sizeof(double) * m->n_cells + rq_lds_bytes(true, n_rec) + 64 > sizeof(lds_raw)) return 31;
  memset(E_abs, 0, sizeof(double) * m->n_cells);
  memset(sed, 0, sizeof(double) * (size_t)9 * m->n_lambda * m->N_thet * m->N_phi);
  memset(n_sent, 0, sizeof(double) * m->n_lambda);
  unsigned long long cnt[24];
  memset(cnt, 0, sizeof(cnt));
  int err = 0;
  RunArgs A;
  memset(&A, 0, sizeof(A));
  A.seed = o->seed; A.first_packet = o->first_packet; A.n_packets = o->n_packets;
  A.qscale = o->n_replicas >= 1.0 ? o->n_replicas : 1.0;
  A.frozen = o->frozen; A.E_prior = E_prior; A.E_abs = E_abs; A.sed = sed; A.n_sent = n_sent;
  A.counters = cnt; A.next_packet = cnt + 12; A.err = &err;
  A.inner_iters = 8; A.flags = 0; A.flush_every = 4; A.min_active = 0;
  A.fly_stay = fly_stay;
  const bool pola = m->lsepar_pola && m->aniso_method == 1, dark = M.dark != nullptr, mrw = M.mrw != 0;
  if (tail_thr > 0) {
    const size_t carry_cap = (size_t)n_rec + 1 + PK_BATCH;
    std::vector<Rec<true>> carry(carry_cap);
    unsigned int carry_n = 0u;
    RunArgs Ar = A;
    Ar.carry_out = carry.data(); Ar.carry_out_n = &carry_n; Ar.carry_cap = (unsigned int)carry_cap;
    Ar.tail_threshold = tail_thr;
#define RUNT(b, c, mm) do { k_thermal_roles_tail<b, c, true, mm>(M, Ar, n_rec, nsp, ks, fi, 65, eq); \
                            if (!err) { const int rct = emu_tail_rounds(A, carry, carry_n, [&](const RunArgs& Ax, const void* recs, unsigned int* np, unsigned int* nx) { \
                              k_tail<false, b, c, mm>(M, Ax, recs, np, nx); }, &err); if (rct) return rct; } } while (0)
    if (mrw) { if (pola) { if (dark) RUNT(true, true, true); else RUNT(true, false, true); } else { if (dark) RUNT(false, true, true); else RUNT(false, false, true); } }
    else { if (pola) { if (dark) RUNT(true, true, false); else RUNT(true, false, false); } else { if (dark) RUNT(false, true, false); else RUNT(false, false, false); } }
#undef RUNT
  } else {
#define RUNR(b, c, mm) k_thermal_roles<false, b, c, true, mm>(M, A, n_rec, nsp, ks, fi, 65, eq)
    if (mrw) { if (pola) { if (dark) RUNR(true, true, true); else RUNR(true, false, true); } else { if (dark) RUNR(false, true, true); else RUNR(false, false, true); } }
    else { if (pola) { if (dark) RUNR(true, true, false); else RUNR(true, false, false); } else { if (dark) RUNR(false, true, false); else RUNR(false, false, false); } }
#undef RUNR
  }
  for (int q = 0; q < ORACLE_N_COUNTERS; ++q) counters[q] = cnt[q];
  *lean_rounds = g_lean_rounds;
  return err;
}
