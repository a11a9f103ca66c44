// emu_fly_leave.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) for the flying waves' crossing
// with the leave test at the commit (fly_visit_step_2d<..., PAD, WALL, LATE = true> and fly_leave_2d, mc_roles.hip.h):
//   * whole flights walked, visit by visit as the flying branch of roles_body runs them -- the pick-up test once per visit,
//     then up to `visit_len` crossings -- through
//       A  fly_visit_step_2d<..., PAD = true, WALL = true, LATE = true>   the flying waves' crossing
//       C  fly_step_2d<..., PAD = false>                                  the specification
//     side by side, compared after every crossing; where A has set a leaving state behind its commit, C gets the one
//     extra call in which it finds that out, and that call must change nothing but its st (and the extr nobody reads);
//   * zj of the end point from one conversion and the fraction as fract_nonneg, against the floor written out.
// Built only by tests/test_fly_leave_exact.py.
#include "emu_kernel.cpp"

namespace {
struct Walker {
  Flight F;
  unsigned int c_cross = 0, c_kill = 0, c_dark = 0;
  int fin = 0;
};
bool same(double p, double q) { return __double_as_longlong(p) == __double_as_longlong(q); }

// the tables as the library lays them out for model M: plain factors, padded factors, wall records, in one array
std::vector<double> device_table(const DevModel& M, const double* kappa_factor, const double* ch, const double* zmax) {
  const int np = pad_cells_2d(M.n_rad, M.nz);
  const size_t at = pad_wall_offset(M.n_cells, M.n_rad, M.nz);
  std::vector<double> kf(at + 4 * (size_t)np, 0.0);
  memcpy(kf.data(), kappa_factor, sizeof(double) * M.n_cells);
  double* const padded = kf.data() + M.n_cells + 1;
  pad_table_2d(M.n_rad, M.nz, kappa_factor, padded);
  std::vector<WallRec> rec((size_t)np, WallRec{0.0, 0.0, 0.0, 0.0});
  pad_walls_2d(M.n_rad, M.nz, ch, zmax, rec.data());
  pad_wall_factors_2d(M.n_rad, M.nz, padded, rec.data());
  memcpy(kf.data() + at, rec.data(), sizeof(WallRec) * np);
  return kf;
}
}  // namespace

// Field codes of the first difference
enum { D_NONE = 0, D_X = 1, D_Y, D_Z, D_U, D_V, D_W, D_RI, D_ZJ, D_IC, D_KF, D_EXTR, D_ST, D_PK, D_CROSS, D_KILL, D_DARK, D_FIN,
       D_DEP, D_KEY, D_WALL, D_EXTRA_CALL, D_UNTESTED };
// What happened, counted over all packets
enum { I_OUT_COLUMN = 0,   // a crossing committed the column n_rad + 1, and the flight left there, in the loop
       I_TOP_BELOW,        // a crossing committed the row nz + 1 of a column with zmax < zmaxmax, |z| < zmaxmax: stays
       I_TOP_EQUAL,        // ... |z| == zmaxmax: stays
       I_TOP_ULP,          // ... |z| 1 ulp above zmaxmax: leaves, in the loop
       I_TOP_ABOVE,        // ... |z| further above: leaves, in the loop
       I_STAR_NEXT,        // a crossing committed the star's cell: killed, in the loop
       I_STAR_START,       // a flight picked up in the star's cell: killed at pick-up
       I_PICKED_OUTSIDE,   // a flight picked up outside the grid: left at pick-up
       I_HOLE_IN,          // a crossing from column 1 into the hole
       I_HOLE_OUT,         // a crossing out of the hole
       I_GUARD_ONLY,       // the necessary condition held and the full test did not (the flight went on)
       I_VISITS,           // visits walked
       I_COUNT };

// open: inside a visit, whose bookkeeping (roles_body: crossings, a packet killed) is counted as it would stand if the visit
// ended here; flew: the lane was in flight when the visit began
static int first_difference(const DevModel& M, const Walker& a, const Walker& c, bool open, bool flew, const double* EA,
                            const double* EC, int K, int ic) {
  const Flight &p = a.F, &r = c.F;
  const unsigned int a_cross = a.c_cross + (open ? (p.pk_cross & 0x7FFFFFFFu) : 0u);
  const unsigned int a_kill = a.c_kill + ((open && flew && p.st == S_EMIT) ? 1u : 0u);
  const int a_fin = a.fin + ((open && flew && p.st == S_EMIT) ? 1 : 0);
  if (!same(p.x, r.x)) return D_X;
  if (!same(p.y, r.y)) return D_Y;
  if (!same(p.z, r.z)) return D_Z;
  if (!same(p.u, r.u)) return D_U;
  if (!same(p.v, r.v)) return D_V;
  if (!same(p.w, r.w)) return D_W;
  if (p.st != r.st) return D_ST;
  if (p.ri != r.ri) return D_RI;
  if (p.zj != r.zj) return D_ZJ;
  // the padded key is the padding of the specification's index, and names a halo slot exactly where that says "no cell"
  if (pad_cell_of_key(M.n_rad, M.nz, p.ic) != (r.ic < M.n_cells ? r.ic : -1)) return D_IC;
  if (p.ic != pad_key_2d(M.n_rad, p.ri, p.zj)) return D_KEY;
  if (!same(p.kf, r.kf)) return D_KF;
  // (fly_step_2d also subtracts from the extr of a packet that does not fly; nothing reads that value)
  if (p.st == S_FLIGHT && !same(p.extr, r.extr)) return D_EXTR;
  if (p.pk_cross != r.pk_cross) return D_PK;
  if (a_cross != c.c_cross) return D_CROSS;
  if (a_kill != c.c_kill) return D_KILL;
  if (a.c_dark != c.c_dark) return D_DARK;
  if (a_fin != c.fin) return D_FIN;
  if (K >= 0 && ic < M.n_cells && !same(EA[K], EC[ic])) return D_DEP;
  return D_NONE;
}

// the specification's one call on a flight that has left: nothing but st may change (and extr, which nobody reads again)
static bool only_st_changed(const Flight& b, const Flight& r) {
  return same(b.x, r.x) && same(b.y, r.y) && same(b.z, r.z) && same(b.u, r.u) && same(b.v, r.v) && same(b.w, r.w) &&
         b.ri == r.ri && b.zj == r.zj && b.ic == r.ic && same(b.kf, r.kf) && b.pk_cross == r.pk_cross && b.star_key == r.star_key;
}

// star_key >= -1: as given (plain encoding); -2: the cell the flight starts in; -3: the cell its first crossing enters
template <bool MRW>
static void walk_one(const Lds& T, const DevModel& M, const RunArgs& A, const double* s, double extr, int star_key, int force_ri,
                     int force_zj, int visit_len, int kmax, double* EA, double* EC, int* steps, int* where, int* info) {
  Walker a, c;
  const int bias = pad_star_bias(M.n_rad, M.nz);
  const int lambda = 1 + (int)(M.n_lambda / 2);
  const WallRec* wall = pad_wall_records(M);
  for (int q = 0; q < 2; ++q) {
    Flight& F = q == 0 ? a.F : c.F;
    flight_clear(F);
    F.x = s[0]; F.y = s[1]; F.z = s[2]; F.u = s[3]; F.v = s[4]; F.w = s[5];
    F.extr = extr; F.S0 = 1.0; F.st = S_FLIGHT; F.pk_cross = 0u;
    index_cell<false>(T, M, F.x, F.y, F.z, F.ri, F.zj, F.k);
    if (force_ri >= 0) F.ri = force_ri;
    if (force_zj >= 0) F.zj = force_zj;
    if (q == 0) flight_constants<false, false, false, true, true>(T, M, F, lambda);
    else flight_constants<false, false>(T, M, F, lambda);
  }
  if (star_key == -2) star_key = a.F.ri + (M.n_rad + 2) * (a.F.zj + M.nz + 1);
  if (star_key == -3) {
    double l, z1;
    int ri1, zj1;
    fly_geom_2d<true>(T, M, a.F, l, z1, ri1, zj1);
    star_key = ri1 + (M.n_rad + 2) * (zj1 + M.nz + 1);
  }
  a.F.star_key = star_key - bias;  // (as roles_body has a padded flight's key inside its loops)
  c.F.star_key = star_key;
  const double zmm_ulp = __longlong_as_double(__double_as_longlong(M.zmaxmax) + 1);
  *where = D_NONE;
  int k = 0;
  while (k < kmax && *where == D_NONE && (a.F.st == S_FLIGHT || c.F.st == S_FLIGHT)) {
    // ---- one visit of a flying wave (roles_body) ----
    info[I_VISITS] += 1;
    const bool flew = a.F.st == S_FLIGHT;
    a.c_cross -= a.F.pk_cross & 0x7FFFFFFFu;
    if (flew) fly_leave_2d(M, a.F);   // the pick-up test
    if (!flew || a.F.st != S_FLIGHT) {
      // left at pick-up (or A does not fly and C does: a difference): the specification finds out in one call
      if (flew) info[a.F.st == S_EMIT ? I_STAR_START : I_PICKED_OUTSIDE] += 1;
      const Flight before = c.F;
      c.fin += fly_step_2d<false, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
      ++k;
      if (!only_st_changed(before, c.F)) *where = D_EXTRA_CALL;
      else *where = first_difference(M, a, c, true, flew, EA, EC, -1, 0);
    }
    for (int it = 0; it < visit_len && k < kmax && *where == D_NONE && a.F.st == S_FLIGHT; ++it, ++k) {
      const int K = a.F.ic, ic = c.F.ic;  // the slot / cell of this crossing's deposit
      const int ri0 = a.F.ri, zj0 = a.F.zj;   // (the cell this crossing starts in)
      // a crossing starts in a tested cell, always
      if ((ri0 == M.n_rad + 1) || (zj0 == M.nz + 1 && fabs(a.F.z) > M.zmaxmax) || a.F.ic == a.F.star_key) { *where = D_UNTESTED; break; }
      // the wall the flight carries is its cell's record for this crossing's direction
      const bool away = a.F.w * a.F.z > 0.0;
      if (!same(a.F.zw, away ? wall[K].z_up : wall[K].z_dn)) { *where = D_WALL; break; }
      fly_visit_step_2d<false, true, MRW, false, true, true, true>(T, M, A, EA, a.F, a.c_dark, nullptr, nullptr, wall);
      c.fin += fly_step_2d<false, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
      const bool moved = a.F.st != S_INTERACT;   // (no dark zone: a crossing either stops the flight or enters the next cell)
      const bool left = a.F.st == S_EXITED || a.F.st == S_EMIT;
      if (left) {
        const Flight before = c.F;
        c.fin += fly_step_2d<false, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
        if (!only_st_changed(before, c.F)) { *where = D_EXTRA_CALL; break; }
      }
      if (moved) {
        const int ri1 = a.F.ri, zj1 = a.F.zj;
        const double az = fabs(a.F.z);
        if (ri1 == M.n_rad + 1 && a.F.st == S_EXITED) info[I_OUT_COLUMN] += 1;
        if (ri1 >= 1 && ri1 <= M.n_rad && zj1 == M.nz + 1 && M.zmax[ri1 - 1] < M.zmaxmax) {
          if (az < M.zmaxmax && a.F.st == S_FLIGHT) info[I_TOP_BELOW] += 1;
          if (az == M.zmaxmax && a.F.st == S_FLIGHT) info[I_TOP_EQUAL] += 1;
          if (az == zmm_ulp && a.F.st == S_EXITED) info[I_TOP_ULP] += 1;
          if (az > zmm_ulp && a.F.st == S_EXITED) info[I_TOP_ABOVE] += 1;
        }
        if (a.F.st == S_EMIT) info[I_STAR_NEXT] += 1;
        if (ri0 == 1 && ri1 == 0) info[I_HOLE_IN] += 1;
        if (ri0 == 0 && ri1 == 1) info[I_HOLE_OUT] += 1;
        if (!left && ((ri1 > M.n_rad) || (az > M.zmaxmax) || (a.F.ic == a.F.star_key))) info[I_GUARD_ONLY] += 1;
      }
      *where = first_difference(M, a, c, true, flew, EA, EC, K, ic);
    }
    // ---- the visit's bookkeeping ----
    a.c_cross += a.F.pk_cross & 0x7FFFFFFFu;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    if ((MRW ? (a.F.pk_cross & 0x7FFFFFFFu) : a.F.pk_cross) > 200000000u && a.F.st == S_FLIGHT) { *A.err = 13; a.F.st = S_EMIT; a.fin += 1; }
    if (*where == D_NONE) *where = first_difference(M, a, c, false, false, EA, EC, -1, 0);
  }
  *steps = k;
}

// n packets, s: n x 6 (x, y, z, u, v, w); extr, star_key (plain encoding; -2 / -3: see walk_one), force_ri, force_zj and the
// visit's length per packet; variant 0: plain, 1: MRW (the walk's bit in the crossing counter).
// Per packet: calls of the specification walked, the code of the first difference (0: none).  EA: the padded form's
// deposits (pad_cells_2d slots), EC: the specification's (n_cells + 1), summed over all packets in the same order.
// info[I_COUNT]: what happened (see the enum).
extern "C" int emu_fly_leave_compare(const oracle_model* m, int variant, int n, const double* s, const double* extr,
                                     const int* star_key, const int* force_ri, const int* force_zj, const int* visit_len, int kmax,
                                     int* steps, int* where, double* EA, double* EC, int* info) {
  Conv cv(m);
  if (cv.voro || m->l3D || cv.M.grid_sph || lds_bytes(cv.M) > sizeof(lds_raw)) return 31;
  DevModel M = cv.M;
  const std::vector<double> kf = device_table(M, m->kappa_factor, M.ch, M.zmax);
  M.kappa_factor = kf.data();
  M.dark = nullptr;
  const Lds T = lds_carve(lds_raw, M);
  lds_stage(T, M);
  int err = 0;
  RunArgs A;
  memset(&A, 0, sizeof(A));
  A.err = &err;
  for (int i = 0; i < I_COUNT; ++i) info[i] = 0;
  for (int i = 0; i < n; ++i) {
    const double* si = s + 6 * i;
    if (variant == 1) walk_one<true>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], visit_len[i], kmax, EA, EC, steps + i, where + i, info);
    else walk_one<false>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], visit_len[i], kmax, EA, EC, steps + i, where + i, info);
  }
  return err;
}

// zj of the end point of a radial move, for n values of qd = |z1| rzn (>= 0, or a NaN):
//   zj_new / fr_new     fly_geom_2d<WALL = true>: one conversion, the fraction as fract_nonneg
//   zj_spec / fr_spec   fly_geom_2d<WALL = false>: the floor, then the conversion; qd - floor(qd)
//   zj_step             fly_step_2d: the minimum taken on the doubles (undefined for a NaN: -1 here)
extern "C" void emu_zj_end(int n, int nz, const double* qd, int* zj_new, double* fr_new, int* zj_spec, double* fr_spec, int* zj_step) {
  for (int i = 0; i < n; ++i) {
    const double q = qd[i];
    const int fn = f64_to_i32_sat(q);
    zj_new[i] = (fn < nz ? fn : nz) + 1;
    fr_new[i] = fract_nonneg(q);
    const double fl = floor(q);
    const int fs = f64_to_i32_sat(fl);
    zj_spec[i] = (fs < nz ? fs : nz) + 1;
    fr_spec[i] = q - fl;
    zj_step[i] = q == q ? (int)fmin(fl, (double)nz) + 1 : -1;
  }
}
