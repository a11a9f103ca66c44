// emu_serve_fused.cpp -- TEST INFRASTRUCTURE: the 2D role kernels (mc_roles.hip.h) on one emulated lane (the shim of
// emu_kernel.cpp) with the fused serving round compiled in: a serving lane bins its exited packet directly behind the
// SRV pop, keeps the record and emits the next packet into it in the same round (roles_body, FUSED).  The emulation runs
// the plain instantiations, which the library builds with the former order of the phases; MCGPU_SERVE_FUSED_PLAIN
// compiles the fused round into them here, so that its logic -- the record reused without a ring operation, the exit held
// over a round boundary, the record of a lane that may not emit, the hand-over of a held exit, the end of the launch --
// runs on the host.  Built only by tests/test_serve_fused_emulated.py.
#define MCGPU_SERVE_FUSED_PLAIN 1
static unsigned long long g_reused = 0ull;       // emissions into the record whose packet the lane had just binned
static unsigned long long g_held = 0ull;         // exits binned at the top of a round that the lane held since its last round
static unsigned long long g_handed = 0ull;       // held exits that a hand-over wrote out
#define MCGPU_SERVE_FUSED_TEST_HOOK(reused, held) do { if (reused) ++g_reused; if (held) ++g_held; } while (0)
#define MCGPU_SERVE_FUSED_HAND_HOOK(handed) do { if (handed) ++g_handed; } while (0)
#include "emu_kernel.cpp"

// As emu_run_thermal's role schedule (MCGPU_EMU_ROLES): n_srv_pref, k_short, fly_iters, emit_qmax; 2D, LDS deposits, one
// dust class.  n_srv_pref = 1: the one wave serves (and flies long flights in place), 0: it prefers to fly and serves what
// it owns.  tail_thr > 0: the kernel that hands its last packets over (k_thermal_roles_tail), finished by k_tail.
// stats: { records reused, exits held over a round boundary, held exits handed over }
extern "C" int emu_run_roles_fused(const oracle_model* m, const oracle_opts* o, const double* E_prior, int nsp, int ks, int fi,
                                   int eq, int tail_thr, double* E_abs, double* sed, double* n_sent, uint64_t* counters,
                                   uint64_t* stats) {
  g_reused = g_held = g_handed = 0ull;
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
  A.fly_stay = 1;
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
#undef RUNR
#define RUNR(b, c, mm) k_thermal_roles<false, b, c, true, mm>(M, A, n_rec, nsp, ks, fi, 65, eq)
    if (mrw) { if (pola) { if (dark) RUNR(true, true, true); else RUNR(true, false, true); } else { if (dark) RUNR(false, true, true); else RUNR(false, false, true); } }
    else { if (pola) { if (dark) RUNR(true, true, false); else RUNR(true, false, false); } else { if (dark) RUNR(false, true, false); else RUNR(false, false, false); } }
#undef RUNR
  }
  for (int q = 0; q < ORACLE_N_COUNTERS; ++q) counters[q] = cnt[q];
  stats[0] = g_reused; stats[1] = g_held; stats[2] = g_handed;
  return err;
}
