// emu_fly_visit.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) that walks packets through the
// 2D crossing two ways in lockstep and reports where they part:
//   A  fly_visit_step_2d<...>          the flying waves' crossing under the flight predicate (the caller's part of
//                                       roles_body -- the per-visit bookkeeping -- emulated below, one crossing per visit)
//   B  fly_step_2d<..., WAVE = false>  its specification: the form of the serving waves, the tail kernel and the host tail
// Built only by tests/test_fly_visit_exact.py.
#include "emu_kernel.cpp"

namespace {
struct Walker {
  Flight F;
  unsigned int c_cross = 0, c_kill = 0, c_dark = 0;
  int fin = 0;
};
}  // namespace

// Field codes of the first difference
enum { D_NONE = 0, D_X = 1, D_Y, D_Z, D_U, D_V, D_W, D_RI, D_ZJ, D_IC, D_KF, D_EXTR, D_ST, D_PK, D_CROSS, D_KILL, D_DARK, D_FIN,
       D_KAB, D_DEP };

// force_ri / force_zj >= 0: the packet's indices are set instead of looked up (a packet put ON a wall, on the side that
// only rounding reaches).  fixes[3]: crossings at which the fix-up of s1 == 0, t < 0, z1 == 0 applied.
template <bool DARK, bool MRW, bool VAR>
static void walk_one(const Lds& T, const DevModel& M, const RunArgs& A, const double* s, double extr, int star_key, int force_ri,
                     int force_zj, int kmax, double* EA, double* EB, int* steps, int* where, int* fixes) {
  Walker a, b;
  Walker* ws[2] = {&a, &b};
  for (Walker* w : ws) {
    flight_clear(w->F);
    Flight& F = w->F;
    F.x = s[0]; F.y = s[1]; F.z = s[2]; F.u = s[3]; F.v = s[4]; F.w = s[5];
    F.extr = extr; F.S0 = 1.0; F.star_key = star_key; F.st = S_FLIGHT; F.pk_cross = 0u;
    index_cell<false>(T, M, F.x, F.y, F.z, F.ri, F.zj, F.k);
    if (force_ri >= 0) F.ri = force_ri;
    if (force_zj >= 0) F.zj = force_zj;
    flight_constants<false, VAR>(T, M, F, 1 + (int)(M.n_lambda / 2));
  }
  auto same = [](double p, double q) { return __double_as_longlong(p) == __double_as_longlong(q); };
  *where = D_NONE;
  int k = 0;
  for (; k < kmax && (a.F.st == S_FLIGHT || b.F.st == S_FLIGHT); ++k) {
    const int ic = a.F.ic;  // (the cell of this crossing's deposit; n_cells: none -- the arrays have that entry)
    if (a.F.st == S_FLIGHT) {  // which fix-ups apply at this crossing
      double l, z1;
      int ri1, zj1;
      const bool will_cross = !((a.F.ri == M.n_rad + 1) || (a.F.zj == M.nz + 1 && fabs(a.F.z) > M.zmaxmax));
      if (will_cross) {
        const int fix = fly_geom_2d(T, M, a.F, l, z1, ri1, zj1);
        for (int i = 0; i < 3; ++i) fixes[i] += (fix >> i) & 1;
      }
    }
    // A: the flying loop's call and its per-visit part (roles_body)
    const bool flew = a.F.st == S_FLIGHT;
    a.c_cross -= a.F.pk_cross & 0x7FFFFFFFu;
    fly_visit_step_2d<DARK, true, MRW, VAR>(T, M, A, EA, a.F, a.c_dark);
    a.c_cross += a.F.pk_cross & 0x7FFFFFFFu;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    if ((MRW ? (a.F.pk_cross & 0x7FFFFFFFu) : a.F.pk_cross) > 200000000u && a.F.st == S_FLIGHT) { *A.err = 13; a.F.st = S_EMIT; a.fin += 1; }
    // B
    b.fin += fly_step_2d<DARK, true, MRW, false, VAR, false>(T, M, A, EB, b.F, b.c_cross, b.c_kill, b.c_dark);
    const Flight &p = a.F, &q = b.F;
    int d = D_NONE;
    if (!same(p.x, q.x)) d = D_X;
    else if (!same(p.y, q.y)) d = D_Y;
    else if (!same(p.z, q.z)) d = D_Z;
    else if (!same(p.u, q.u)) d = D_U;
    else if (!same(p.v, q.v)) d = D_V;
    else if (!same(p.w, q.w)) d = D_W;
    else if (p.st != q.st) d = D_ST;
    else if (p.ri != q.ri) d = D_RI;
    else if (p.zj != q.zj) d = D_ZJ;
    else if (p.ic != q.ic) d = D_IC;
    else if (!same(p.kf, q.kf)) d = D_KF;
    else if (VAR && !same(p.kab, q.kab)) d = D_KAB;
    // (the old form also subtracts from the extr of a packet that does not fly; nothing reads that value)
    else if (p.st == S_FLIGHT && !same(p.extr, q.extr)) d = D_EXTR;
    else if (p.pk_cross != q.pk_cross) d = D_PK;
    else if (a.c_cross != b.c_cross) d = D_CROSS;
    else if (a.c_kill != b.c_kill) d = D_KILL;
    else if (a.c_dark != b.c_dark) d = D_DARK;
    else if (a.fin != b.fin) d = D_FIN;
    else if (!same(EA[ic], EB[ic])) d = D_DEP;
    if (d != D_NONE) { *where = d; ++k; break; }
  }
  *steps = k;
}

// n packets, s: n x 6 (x, y, z, u, v, w); extr, star_key, force_ri, force_zj per packet; dark_every > 0: every
// dark_every-th cell is dark; variant 0: plain, 1: MRW (bit 31 of the crossing counter), 2: VAR (per-cell opacities: a
// table made here from the model's, varied from cell to cell).
// Per packet: crossings walked, the field of the first difference (0: none), the fix-ups that applied (n x 3).
// EA, EB: the two paths' deposits (n_cells + 1 each), summed over all packets in the same order.
extern "C" int emu_fly_visit_compare(const oracle_model* m, int dark_every, int variant, int n, const double* s, const double* extr,
                                     const int* star_key, const int* force_ri, const int* force_zj, int kmax, int* steps,
                                     int* where, int* fixes, double* EA, double* EB) {
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
  std::vector<double2> kk((size_t)(M.n_cells + 1) * M.n_lambda, double2{0.0, 0.0});
  if (variant == 2) {
    for (int ic = 0; ic < M.n_cells; ++ic)
      for (int l = 0; l < M.n_lambda; ++l)
        kk[(size_t)ic * M.n_lambda + l] = double2{T.kappa[l] * M.kappa_factor[ic] * (1.0 + 0.125 * (ic % 5)), T.kabs[l] * (1.0 + 0.0625 * (ic % 3))};
    M.v_kk = kk.data();
  }
  int err = 0;
  RunArgs A;
  memset(&A, 0, sizeof(A));
  A.err = &err;
  for (int i = 0; i < n; ++i) {
    const double* si = s + 6 * i;
#define WALK(D, W, V) walk_one<D, W, V>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], kmax, EA, EB, steps + i, where + i, fixes + 3 * i)
    if (dark_every > 0) { if (variant == 1) WALK(true, true, false); else if (variant == 2) WALK(true, false, true); else WALK(true, false, false); }
    else { if (variant == 1) WALK(false, true, false); else if (variant == 2) WALK(false, false, true); else WALK(false, false, false); }
#undef WALK
  }
  return err;
}
