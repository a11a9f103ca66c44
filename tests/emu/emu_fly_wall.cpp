// emu_fly_wall.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) for the wall records of the
// padded 2D role kernels (WallRec, mc_roles.hip.h):
//   * the table the library's builders make (pad_walls_2d, pad_wall_factors_2d) against section 2 of the crossing, written
//     out here from fly_step_2d, for every padded cell, both directions and both sides of the midplane;
//   * packets walked, crossing by crossing, through
//       A  fly_visit_step_2d<..., PAD = true, WALL = true>   the flying waves' crossing: the wall travels with the flight
//       C  fly_step_2d<..., PAD = false>                     the specification: plain cell index, the wall formed anew
//     with the caller's per-visit bookkeeping of roles_body emulated for A, one crossing per visit.
// Built only by tests/test_fly_wall_exact.py.
#include "emu_kernel.cpp"

namespace {
struct Walker {
  Flight F;
  unsigned int c_cross = 0, c_kill = 0, c_dark = 0;
  int fin = 0;
};
bool same(double p, double q) { return __double_as_longlong(p) == __double_as_longlong(q); }

// the wall records as the library lays them out for model M (mcgpu_set_grid_cyl: the walls, upload_cell_opacities: the
// factors, behind the plain and the padded factors in one array)
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

// section 2 of fly_step_2d up to zl, expression for expression (R0: the row of ri0)
double spec_wall(const RowT& R0, int nz, int zj0, bool away, double z0) {
  const bool top = (zj0 == nz + 1);
  const bool flip = !away && (zj0 == 1);
  const int jm = away ? zj0 : (zj0 == 1 ? 1 : zj0 - 1);
  const bool below = jm < nz;
  double zmag = (double)(below ? jm : 1) * *(below ? &R0.ch : &R0.zmax);
  zmag = __builtin_fma(zmag, __longlong_as_double(away ? 0x3D06800000000000ll : (long long)0xBD06800000000000ull), zmag);
  zmag = (away && top) ? 1.0e10 : zmag;
  const bool neg = (z0 < 0.0) != flip;
  return __longlong_as_double(__double_as_longlong(zmag) | (neg ? (long long)0x8000000000000000ull : 0ll));
}
}  // namespace

// Field codes of the first difference
enum { D_NONE = 0, D_X = 1, D_Y, D_Z, D_U, D_V, D_W, D_RI, D_ZJ, D_IC, D_KF, D_EXTR, D_ST, D_PK, D_CROSS, D_KILL, D_DARK, D_FIN,
       D_DEP, D_KEY, D_WALL };

// The table for a grid of n_rad columns (ch, zmax) and nz layers with the factors kf (n_rad * nz).
// rec: the pad_cells_2d records as built (4 doubles each); spec: per padded cell the specification's zl for
// (away = false, z0 > 0), (away = false, z0 < 0), (away = true, z0 > 0), (away = true, z0 < 0), formed from the rows the
// kernel stages in LDS (lds_stage); used: what the record gives a crossing in those four cases, by the rule of
// fly_geom_2d<WALL = true>.  Rows zj = 0 of spec / used are left 0: no cell of a 2D grid.
extern "C" int emu_wall_table(int n_rad, int nz, const double* ch, const double* zmax, const double* kf, double* rec,
                              double* spec, double* used) {
  DevModel M;
  memset(&M, 0, sizeof(M));
  M.n_rad = n_rad; M.nz = nz; M.n_az = 1; M.n_cells = n_rad * nz;
  const std::vector<double> tab = device_table(M, kf, ch, zmax);
  const size_t at = pad_wall_offset(M.n_cells, n_rad, nz);
  if (at % 4 != 0 || at < (size_t)M.n_cells + 1 + pad_cells_2d(n_rad, nz)) return 1;
  memcpy(rec, tab.data() + at, sizeof(WallRec) * pad_cells_2d(n_rad, nz));
  const WallRec* R = reinterpret_cast<const WallRec*>(rec);
  for (int zj = 1; zj <= nz + 1; ++zj)
    for (int ri = 0; ri <= n_rad + 1; ++ri) {
      // (the row of ri as lds_stage fills it)
      const int rin = ri == 0 ? 0 : (ri - 1 < n_rad ? ri - 1 : n_rad - 1);
      RowT R0;
      memset(&R0, 0, sizeof(R0));
      R0.ch = ch[rin]; R0.zmax = zmax[rin];
      const int K = pad_key_2d(n_rad, ri, zj);
      for (int c = 0; c < 4; ++c) {
        const bool away = c >= 2;
        const double z0 = (c & 1) ? -0.25 * ch[rin] : 0.25 * ch[rin];
        spec[4 * K + c] = spec_wall(R0, nz, zj, away, z0);
        const double zw = away ? R[K].z_up : R[K].z_dn;
        used[4 * K + c] = (z0 < 0.0) ? -zw : zw;
      }
    }
  return 0;
}

template <bool DARK, bool MRW>
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
  const unsigned char* dark_pad = DARK ? pad_dark(M) : nullptr;
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
    fly_visit_step_2d<DARK, true, MRW, false, true, true>(T, M, A, EA, a.F, a.c_dark, nullptr, dark_pad, wall);
    a.c_cross += a.F.pk_cross & 0x7FFFFFFFu;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    if ((MRW ? (a.F.pk_cross & 0x7FFFFFFFu) : a.F.pk_cross) > 200000000u && a.F.st == S_FLIGHT) { *A.err = 13; a.F.st = S_EMIT; a.fin += 1; }
    c.fin += fly_step_2d<DARK, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
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
  info[8] += (int)a.c_dark;
}

// n packets, s: n x 6 (x, y, z, u, v, w); extr, star_key (plain encoding), force_ri, force_zj per packet; dark_every > 0:
// every dark_every-th cell is dark; variant 0: plain, 1: MRW.
// Per packet: crossings walked, the code of the first difference (0: none), the fix-ups its crossings took (s1 == 0, t < 0,
// z1 == 0).  EA: the wall form's deposits (pad_cells_2d slots), EC: the specification's (n_cells + 1), summed over all
// packets in the same order.  info[0..7]: crossings through the midplane, up out of layer nz, in the row nz + 1, in the hole,
// with dz == 0, with w == 0, from z0 = -0.0, from z0 = +0.0; info[8]: packets mirrored at a dark cell.
extern "C" int emu_fly_wall_compare(const oracle_model* m, int dark_every, int variant, int n, const double* s, const double* extr,
                                    const int* star_key, const int* force_ri, const int* force_zj, int kmax, int* steps,
                                    int* where, int* fixes, double* EA, double* EC, int* info) {
  Conv cv(m);
  if (cv.voro || m->l3D || cv.M.grid_sph || lds_bytes(cv.M) > sizeof(lds_raw)) return 31;
  DevModel M = cv.M;
  const int np = pad_cells_2d(M.n_rad, M.nz);
  const std::vector<double> kf = device_table(M, m->kappa_factor, M.ch, M.zmax);
  M.kappa_factor = kf.data();
  std::vector<unsigned char> dark((size_t)M.n_cells + np, 0);
  if (dark_every > 0) {
    for (int i = 0; i < M.n_cells; i += dark_every) dark[i] = 1;
    std::vector<unsigned char> plain(dark.begin(), dark.begin() + M.n_cells);
    pad_table_2d(M.n_rad, M.nz, plain.data(), dark.data() + M.n_cells);
    M.dark = dark.data();
  } else M.dark = nullptr;
  const Lds T = lds_carve(lds_raw, M);
  lds_stage(T, M);
  int err = 0;
  RunArgs A;
  memset(&A, 0, sizeof(A));
  A.err = &err;
  for (int i = 0; i < 9; ++i) info[i] = 0;
  for (int i = 0; i < n; ++i) {
    const double* si = s + 6 * i;
#define WALK(D, W) walk_one<D, W>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], kmax, EA, EC, steps + i, where + i, fixes + 3 * i, info)
    if (dark_every > 0) { if (variant == 1) WALK(true, true); else WALK(true, false); }
    else { if (variant == 1) WALK(false, true); else WALK(false, false); }
#undef WALK
  }
  return err;
}
