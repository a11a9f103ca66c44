// emu_fly_step.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) that walks packets through the
// 2D crossing three ways in lockstep and reports where they part:
//   A  fly_step_2d<..., WAVE = true>   the flying waves' form (per-visit bookkeeping; the caller's part emulated below)
//   B  fly_step_2d<..., WAVE = false>  the form of the serving waves, the tail kernel and the host tail
//   C  roles_cross<false, ...>         the retained exact path through cross_cell_lean
// Built only by tests/test_fly_step_exact.py.
#include "emu_kernel.cpp"

namespace {
struct Walker {
  Flight F;
  unsigned int c_cross = 0, c_kill = 0, c_dark = 0;
  int fin = 0;
};
}  // namespace

// Field codes of the first difference (A against B, then A against C)
enum { D_NONE = 0, D_X = 1, D_Y, D_Z, D_U, D_V, D_W, D_RI, D_ZJ, D_IC, D_KF, D_EXTR, D_ST, D_PK, D_CROSS, D_KILL, D_DARK, D_FIN };

template <bool DARK>
static int walk_one(const Lds& T, const DevModel& M, const RunArgs& A, const double* s, double extr, int star_key, int kmax,
                    double* EA, double* EB, double* EC, int* steps, int* where_ab, int* where_ac) {
  Walker a, b, c;
  Walker* ws[3] = {&a, &b, &c};
  for (Walker* w : ws) {
    flight_clear(w->F);
    Flight& F = w->F;
    F.x = s[0]; F.y = s[1]; F.z = s[2]; F.u = s[3]; F.v = s[4]; F.w = s[5];
    F.extr = extr; F.S0 = 1.0; F.star_key = star_key; F.st = S_FLIGHT; F.pk_cross = 0u;
    index_cell<false>(T, M, F.x, F.y, F.z, F.ri, F.zj, F.k);
    flight_constants<false, false>(T, M, F, 1 + (int)(M.n_lambda / 2));
  }
  *where_ab = *where_ac = D_NONE;
  int k = 0;
  for (; k < kmax && (a.F.st == S_FLIGHT || b.F.st == S_FLIGHT || c.F.st == S_FLIGHT); ++k) {
    // A: the flying loop's call and its per-visit part (roles_body): the wave's crossings, the star's cell
    const bool any_star = __ballot(a.F.st == S_FLIGHT && a.F.star_key >= 0) != 0ull;
    const bool flew = a.F.st == S_FLIGHT;
    unsigned int cw = 0;
    a.fin += fly_step_2d<DARK, true, false, false, false, true>(T, M, A, EA, a.F, cw, a.c_kill, a.c_dark, nullptr, nullptr, any_star);
    a.c_cross += cw;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    b.fin += fly_step_2d<DARK, true>(T, M, A, EB, b.F, b.c_cross, b.c_kill, b.c_dark);
    if (c.F.st == S_FLIGHT) {
      int dep_ic = -1;
      double dep_v = 0.0;
      c.fin += roles_cross<false, DARK, true>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark, dep_ic, dep_v);
    }
    auto same = [](double p, double q) { return __double_as_longlong(p) == __double_as_longlong(q); };
    bool full_cmp = true;
    // (full: bit for bit.  Against C only the direction, the state, the indices and the counters: the wall point, the
    // length and with them extr differ from C in their last bits -- fly_step_2d forms x and y as one multiply-add where
    // cross_cell_lean rounds the product first, as HEAD's fly_step_2d already did -- so C goes on from A's point and
    // extr after every crossing: each crossing is compared from the same input)
    auto close = [&](double p, double q, const Flight&) { return !full_cmp || same(p, q); };
    auto diff = [&](const Walker& p, const Walker& q, bool full) -> int {
      full_cmp = full;
      if (!close(p.F.x, q.F.x, p.F)) return D_X;
      if (!close(p.F.y, q.F.y, p.F)) return D_Y;
      if (!close(p.F.z, q.F.z, p.F)) return D_Z;
      if (!same(p.F.u, q.F.u)) return D_U;
      if (!same(p.F.v, q.F.v)) return D_V;
      if (!same(p.F.w, q.F.w)) return D_W;
      if (p.F.st != q.F.st) return D_ST;
      // (C, roles_cross, leaves a finished packet's indices, extr and kf as they were and keeps no cell index)
      if (!full && p.F.st != S_FLIGHT) return D_NONE;
      if (p.F.ri != q.F.ri) return D_RI;
      if (p.F.zj != q.F.zj) return D_ZJ;
      if (full && !same(p.F.kf, q.F.kf)) return D_KF;
      if (full && !same(p.F.extr, q.F.extr)) return D_EXTR;
      if (p.F.pk_cross != q.F.pk_cross) return D_PK;
      if (p.c_cross != q.c_cross) return D_CROSS;
      if (p.c_kill != q.c_kill) return D_KILL;
      if (p.c_dark != q.c_dark) return D_DARK;
      if (p.fin != q.fin) return D_FIN;
      if (full && p.F.ic != q.F.ic) return D_IC;
      return D_NONE;
    };
    if (*where_ab == D_NONE) *where_ab = diff(a, b, true);
    if (*where_ac == D_NONE) *where_ac = diff(a, c, false);
    if (*where_ab != D_NONE || *where_ac != D_NONE) { ++k; break; }
    c.F.x = a.F.x; c.F.y = a.F.y; c.F.z = a.F.z; c.F.extr = a.F.extr;
  }
  *steps = k;
  return 0;
}

// n packets, s: n x 6 (x, y, z, u, v, w), extr and star_key per packet; dark_every > 0: every dark_every-th cell is dark.
// Per packet: crossings walked, the field of the first A/B difference and of the first A/C difference (0: none).
// EA, EB, EC: the three paths' deposits (n_cells each), summed over all packets in the same order.
extern "C" int emu_fly_compare(const oracle_model* m, int dark_every, int n, const double* s, const double* extr,
                               const int* star_key, int kmax, int* steps, int* where_ab, int* where_ac,
                               double* EA, double* EB, double* EC) {
  Conv cv(m);
  if (cv.voro || m->l3D || cv.M.grid_sph || lds_bytes(cv.M) > sizeof(lds_raw)) return 31;
  DevModel M = cv.M;
  std::vector<unsigned char> dark(M.n_cells + 1, 0);
  if (dark_every > 0) {
    for (int i = 0; i < M.n_cells; i += dark_every) dark[i] = 1;
    M.dark = dark.data();
  }
  const Lds T = lds_carve(lds_raw, M);
  lds_stage(T, M);
  int err = 0;
  RunArgs A;
  memset(&A, 0, sizeof(A));
  A.err = &err;
  for (int i = 0; i < n; ++i) {
    if (dark_every > 0) walk_one<true>(T, M, A, s + 6 * i, extr[i], star_key[i], kmax, EA, EB, EC, steps + i, where_ab + i, where_ac + i);
    else walk_one<false>(T, M, A, s + 6 * i, extr[i], star_key[i], kmax, EA, EB, EC, steps + i, where_ab + i, where_ac + i);
  }
  return err;
}
