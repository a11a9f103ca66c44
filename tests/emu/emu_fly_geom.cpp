// emu_fly_geom.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) for the bookkeeping of the
// padded crossing, fly_geom_2d<WALL = true> (mc_roles.hip.h: pad_wall_side, fly_layer_step, fly_row):
//   * packets walked, crossing by crossing, through
//       A  fly_visit_step_2d<..., PAD = true, WALL = true>   the flying waves' crossing
//       C  fly_step_2d<..., PAD = false>                     the specification
//     with the caller's per-visit bookkeeping of roles_body emulated for A, one crossing per visit;
//   * the layer behind a vertical wall, fly_layer_step, against zj0 + delta_zj written out from fly_step_2d;
//   * the time to the vertical wall with pad_wall_side's wall against the specification's select, through the rest of
//     section 2 (the two overrides, the fix-up bit) written out from fly_geom_2d.
// Built only by tests/test_fly_geom_exact.py.
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
       D_DEP, D_KEY, D_WALL };

template <bool MRW>
static void walk_one(const Lds& T, const DevModel& M, const RunArgs& A, const double* s, double extr, int star_key, int force_ri,
                     int force_zj, int kmax, double* EA, double* EC, int* steps, int* where, int* fixes, int* info) {
  Walker a, c;
  const int bias = pad_star_bias(M.n_rad, M.nz);
  const int lambda = 1 + (int)(M.n_lambda / 2);
  for (int q = 0; q < 2; ++q) {
    Flight& F = q == 0 ? a.F : c.F;
    flight_clear(F);
    F.x = s[0]; F.y = s[1]; F.z = s[2]; F.u = s[3]; F.v = s[4]; F.w = s[5];
    F.extr = extr; F.S0 = 1.0; F.st = S_FLIGHT; F.pk_cross = 0u;
    F.star_key = q == 0 ? star_key - bias : star_key;  // (as roles_body has a padded flight's key inside its loops)
    index_cell<false>(T, M, F.x, F.y, F.z, F.ri, F.zj, F.k);
    if (force_ri >= 0) F.ri = force_ri;
    if (force_zj >= 0) F.zj = force_zj;
    if (q == 0) flight_constants<false, false, false, true, true>(T, M, F, lambda);
    else flight_constants<false, false>(T, M, F, lambda);
  }
  const WallRec* wall = pad_wall_records(M);
  *where = D_NONE;
  int k = 0;
  for (; k < kmax && (a.F.st == S_FLIGHT || c.F.st == S_FLIGHT); ++k) {
    const int K = a.F.ic, ic = c.F.ic;  // the slot / cell of this crossing's deposit
    const bool flew = a.F.st == S_FLIGHT;
    const bool leaves = (a.F.ri == M.n_rad + 1) || (a.F.zj == M.nz + 1 && fabs(a.F.z) > M.zmaxmax) || a.F.ic == a.F.star_key;
    if (flew && !leaves) {
      // which fix-ups this crossing takes, and which corners of section 2 it visits
      double l, z1;
      int ri1, zj1;
      const int fx = fly_geom_2d<true>(T, M, a.F, l, z1, ri1, zj1);
      fixes[0] += fx & 1; fixes[1] += (fx >> 1) & 1; fixes[2] += (fx >> 2) & 1;
      const double dz = a.F.w * a.F.z;
      const bool away = dz > 0.0;
      info[0] += (a.F.zj == 1 && !away && a.F.ri >= 1) ? 1 : 0;          // through the midplane
      info[1] += (a.F.zj == M.nz && away && a.F.ri >= 1) ? 1 : 0;        // up out of the top layer
      info[2] += (a.F.zj == M.nz + 1) ? 1 : 0;                           // in the row above the disk
      info[3] += (a.F.ri == 0) ? 1 : 0;                                  // in the hole
      info[4] += (dz == 0.0) ? 1 : 0;                                    // no vertical wall ahead
      info[5] += (a.F.w == 0.0) ? 1 : 0;
      info[6] += (a.F.z == 0.0 && std::signbit(a.F.z)) ? 1 : 0;          // z0 = -0.0
      info[7] += (a.F.z == 0.0 && !std::signbit(a.F.z)) ? 1 : 0;         // z0 = +0.0
      // the wall the flight carries is its cell's record for this crossing's direction
      const double want = away ? wall[K].z_up : wall[K].z_dn;
      if (!same(a.F.zw, want)) { *where = D_WALL; ++k; break; }
    }
    a.c_cross -= a.F.pk_cross & 0x7FFFFFFFu;
    fly_visit_step_2d<false, true, MRW, false, true, true>(T, M, A, EA, a.F, a.c_dark, nullptr, nullptr, wall);
    a.c_cross += a.F.pk_cross & 0x7FFFFFFFu;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    if ((MRW ? (a.F.pk_cross & 0x7FFFFFFFu) : a.F.pk_cross) > 200000000u && a.F.st == S_FLIGHT) { *A.err = 13; a.F.st = S_EMIT; a.fin += 1; }
    c.fin += fly_step_2d<false, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
    int d = D_NONE;
    const Flight &p = a.F, &r = c.F;
    if (!same(p.x, r.x)) d = D_X;
    else if (!same(p.y, r.y)) d = D_Y;
    else if (!same(p.z, r.z)) d = D_Z;
    else if (!same(p.u, r.u)) d = D_U;
    else if (!same(p.v, r.v)) d = D_V;
    else if (!same(p.w, r.w)) d = D_W;
    else if (p.st != r.st) d = D_ST;
    else if (p.ri != r.ri) d = D_RI;
    else if (p.zj != r.zj) d = D_ZJ;
    // the padded key is the padding of the specification's index, and names a halo slot exactly where that says "no cell"
    else if (pad_cell_of_key(M.n_rad, M.nz, p.ic) != (r.ic < M.n_cells ? r.ic : -1)) d = D_IC;
    else if (p.ic != pad_key_2d(M.n_rad, p.ri, p.zj)) d = D_KEY;
    else if (!same(p.kf, r.kf)) d = D_KF;
    // (fly_step_2d also subtracts from the extr of a packet that does not fly; nothing reads that value)
    else if (p.st == S_FLIGHT && !same(p.extr, r.extr)) d = D_EXTR;
    else if (p.pk_cross != r.pk_cross) d = D_PK;
    else if (a.c_cross != c.c_cross) d = D_CROSS;
    else if (a.c_kill != c.c_kill) d = D_KILL;
    else if (a.c_dark != c.c_dark) d = D_DARK;
    else if (a.fin != c.fin) d = D_FIN;
    else if (ic < M.n_cells && !same(EA[K], EC[ic])) d = D_DEP;
    if (d != D_NONE) { *where = d; ++k; break; }
  }
  *steps = k;
}

// n packets, s: n x 6 (x, y, z, u, v, w); extr, star_key (plain encoding), force_ri, force_zj per packet; variant 0: plain,
// 1: MRW (the walk's bit in the crossing counter).
// Per packet: crossings walked, the code of the first difference (0: none), the fix-ups its crossings took (s1 == 0, t < 0,
// z1 == 0).  EA: the padded form's deposits (pad_cells_2d slots), EC: the specification's (n_cells + 1), summed over all
// packets in the same order.  info[0..7]: crossings through the midplane, up out of layer nz, in the row nz + 1, in the hole,
// with dz == 0, with w == 0, from z0 = -0.0, from z0 = +0.0.
extern "C" int emu_fly_geom_compare(const oracle_model* m, int variant, int n, const double* s, const double* extr,
                                    const int* star_key, const int* force_ri, const int* force_zj, int kmax, int* steps,
                                    int* where, int* fixes, double* EA, double* EC, int* info) {
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
  for (int i = 0; i < 8; ++i) info[i] = 0;
  for (int i = 0; i < n; ++i) {
    const double* si = s + 6 * i;
    if (variant == 1) walk_one<true>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], kmax, EA, EC, steps + i, where + i, fixes + 3 * i, info);
    else walk_one<false>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], kmax, EA, EC, steps + i, where + i, fixes + 3 * i, info);
  }
  return err;
}

// The layer behind a vertical wall for zj0 = 1 .. nz + 1 and both values of `away`: got[2 (zj0 - 1) + away] from
// fly_layer_step, want[...] = zj0 + delta_zj with fly_step_2d's delta_zj.
extern "C" void emu_layer_step(int nz, int* got, int* want) {
  for (int zj0 = 1; zj0 <= nz + 1; ++zj0)
    for (int a = 0; a < 2; ++a) {
      const bool away = a == 1;
      const bool top = (zj0 == nz + 1);
      const int delta_zj = away ? (top ? 0 : 1) : ((zj0 == 1) ? 1 : -1);
      want[2 * (zj0 - 1) + a] = zj0 + delta_zj;
      got[2 * (zj0 - 1) + a] = fly_layer_step(nz, zj0, away);
    }
}

// Section 2 behind the wall, from fly_geom_2d: the time to the wall zl, the two overrides, the fix-up bit.
static double wall_time(double zl, double z0, double w, double inv_w, bool hole, int* fix) {
  const double dz = w * z0;
  double t = (zl - z0) * inv_w;
  *fix = ((t < 0.0) && !((dz == 0.0) || hole)) ? 2 : 0;
  t = (t < 0.0) ? GRID_PREC : t;
  t = ((dz == 0.0) || hole) ? 1.0e10 : t;
  return t;
}
// n cases (z0, zw, w, inv_w, hole): the time and the fix-up bit with pad_wall_side's wall (t_new, fix_new) and with the
// specification's zl = (z0 < 0.0) ? -zw : zw (t_spec, fix_spec).
extern "C" void emu_wall_time(int n, const double* z0, const double* zw, const double* w, const double* inv_w, const int* hole,
                              double* t_new, int* fix_new, double* t_spec, int* fix_spec) {
  for (int i = 0; i < n; ++i) {
    t_new[i] = wall_time(pad_wall_side(zw[i], z0[i]), z0[i], w[i], inv_w[i], hole[i] != 0, fix_new + i);
    t_spec[i] = wall_time((z0[i] < 0.0) ? -zw[i] : zw[i], z0[i], w[i], inv_w[i], hole[i] != 0, fix_spec + i);
  }
}
