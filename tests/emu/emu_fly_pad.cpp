// emu_fly_pad.cpp -- TEST INFRASTRUCTURE: one emulated lane (the shim of emu_kernel.cpp) that walks packets through the 2D
// crossing three ways in lockstep and reports where they part:
//   A  fly_visit_step_2d<..., PAD = true>  the flying waves' crossing with the padded cell key (the caller's per-visit
//                                          bookkeeping of roles_body emulated below, one crossing per visit)
//   B  fly_step_2d<..., PAD = true>        the serving waves' crossing with the padded cell key
//   C  fly_step_2d<..., PAD = false>       the specification: plain cell index, "no cell" = n_cells
// and the small pieces that go with the padded key: the padded tables, the folds' way back to the plain index and the
// square root's zero case.  Built only by tests/test_fly_pad_exact.py.
#include "emu_kernel.cpp"

namespace {
struct Walker {
  Flight F;
  unsigned int c_cross = 0, c_kill = 0, c_dark = 0;
  int fin = 0;
};
double g_delta_min = 1e300, g_delta_max = 0.0;  // the positive discriminants the walks took the square root of
}  // namespace

// Field codes of the first difference (B against A: + 32, C against A: + 64)
enum { D_NONE = 0, D_X = 1, D_Y, D_Z, D_U, D_V, D_W, D_RI, D_ZJ, D_IC, D_KF, D_EXTR, D_ST, D_PK, D_CROSS, D_KILL, D_DARK, D_FIN,
       D_DEP, D_KEY };

// the discriminant fly_geom_2d takes the root of (its section 1, expression for expression)
static double radial_delta(const Lds& T, const Flight& p) {
  const RowT& R0 = T.row[p.ri];
  const bool hole = (p.ri == 0);
  const double r_2 = p.x * p.x + p.y * p.y;
  const double dot = p.x * p.u + p.y * p.v;
  const double b = dot * p.inv_a;
  const double c_in = (r_2 - R0.rl_in) * p.inv_a;
  const double c_out = (r_2 - R0.rl_out) * p.inv_a;
  const double bb = b * b;
  const double d_in = bb - c_in;
  const double d_out = fmax(bb - c_out, 0.0);
  const bool use_in = hole || ((dot < 0.0) && !(d_in < 0.0));
  return use_in ? d_in : d_out;
}

template <bool DARK, bool MRW>
static void walk_one(const Lds& T, const DevModel& M, const RunArgs& A, const double* s, double extr, int star_key, int force_ri,
                     int force_zj, int kmax, double* EA, double* EB, double* EC, int* steps, int* where, int* info) {
  Walker a, b, c;
  Walker* ws[3] = {&a, &b, &c};
  const int bias = pad_star_bias(M.n_rad, M.nz);
  const int lambda = 1 + (int)(M.n_lambda / 2);
  for (int q = 0; q < 3; ++q) {
    Flight& F = ws[q]->F;
    flight_clear(F);
    F.x = s[0]; F.y = s[1]; F.z = s[2]; F.u = s[3]; F.v = s[4]; F.w = s[5];
    F.extr = extr; F.S0 = 1.0; F.st = S_FLIGHT; F.pk_cross = 0u;
    F.star_key = q < 2 ? star_key - bias : star_key;  // (as roles_body has a padded flight's key inside its loops)
    index_cell<false>(T, M, F.x, F.y, F.z, F.ri, F.zj, F.k);
    if (force_ri >= 0) F.ri = force_ri;
    if (force_zj >= 0) F.zj = force_zj;
    if (q < 2) flight_constants<false, false, false, true>(T, M, F, lambda);
    else flight_constants<false, false>(T, M, F, lambda);
  }
  auto same = [](double p, double q) { return __double_as_longlong(p) == __double_as_longlong(q); };
  const double* kf_pad = pad_kappa_factor(M);
  const unsigned char* dark_pad = DARK ? pad_dark(M) : nullptr;
  *where = D_NONE;
  int k = 0;
  for (; k < kmax && (a.F.st == S_FLIGHT || b.F.st == S_FLIGHT || c.F.st == S_FLIGHT); ++k) {
    const int K = a.F.ic, ic = c.F.ic;  // the slot / cell of this crossing's deposit
    if (a.F.st == S_FLIGHT && !((a.F.ri == M.n_rad + 1) || (a.F.zj == M.nz + 1 && fabs(a.F.z) > M.zmaxmax))) {
      const double d = radial_delta(T, a.F);
      if (d > 0.0) { g_delta_min = d < g_delta_min ? d : g_delta_min; g_delta_max = d > g_delta_max ? d : g_delta_max; }
    }
    // A: the flying loop's call and its per-visit part (roles_body)
    const bool flew = a.F.st == S_FLIGHT;
    a.c_cross -= a.F.pk_cross & 0x7FFFFFFFu;
    fly_visit_step_2d<DARK, true, MRW, false, true>(T, M, A, EA, a.F, a.c_dark, kf_pad, dark_pad);
    a.c_cross += a.F.pk_cross & 0x7FFFFFFFu;
    if (flew && a.F.st == S_EMIT) { a.c_kill++; a.fin += 1; }
    if ((MRW ? (a.F.pk_cross & 0x7FFFFFFFu) : a.F.pk_cross) > 200000000u && a.F.st == S_FLIGHT) { *A.err = 13; a.F.st = S_EMIT; a.fin += 1; }
    // B, C
    b.fin += fly_step_2d<DARK, true, MRW, false, false, false, true>(T, M, A, EB, b.F, b.c_cross, b.c_kill, b.c_dark);
    c.fin += fly_step_2d<DARK, true, MRW, false, false, false, false>(T, M, A, EC, c.F, c.c_cross, c.c_kill, c.c_dark);
    int d = D_NONE;
    for (int q = 1; q < 3 && d == D_NONE; ++q) {
      const Walker& o = *ws[q];
      const Flight &p = a.F, &r = o.F;
      if (!same(p.x, r.x)) d = D_X;
      else if (!same(p.y, r.y)) d = D_Y;
      else if (!same(p.z, r.z)) d = D_Z;
      else if (!same(p.u, r.u)) d = D_U;
      else if (!same(p.v, r.v)) d = D_V;
      else if (!same(p.w, r.w)) d = D_W;
      else if (p.st != r.st) d = D_ST;
      else if (p.ri != r.ri) d = D_RI;
      else if (p.zj != r.zj) d = D_ZJ;
      else if (q == 1 && p.ic != r.ic) d = D_IC;
      // the padded key is the padding of the specification's index, and names a halo slot exactly where that says "no cell"
      else if (q == 2 && pad_cell_of_key(M.n_rad, M.nz, p.ic) != (r.ic < M.n_cells ? r.ic : -1)) d = D_IC;
      else if (!same(p.kf, r.kf)) d = D_KF;
      // (fly_step_2d also subtracts from the extr of a packet that does not fly; nothing reads that value)
      else if (p.st == S_FLIGHT && !same(p.extr, r.extr)) d = D_EXTR;
      else if (p.pk_cross != r.pk_cross) d = D_PK;
      else if (a.c_cross != o.c_cross) d = D_CROSS;
      else if (a.c_kill != o.c_kill) d = D_KILL;
      else if (a.c_dark != o.c_dark) d = D_DARK;
      else if (a.fin != o.fin) d = D_FIN;
      if (d != D_NONE) d += 32 * q;
    }
    if (d == D_NONE && a.F.ic != pad_key_2d(M.n_rad, a.F.ri, a.F.zj)) d = D_KEY;
    if (d == D_NONE && !same(EA[K], EB[K])) d = D_DEP + 32;
    if (d == D_NONE && ic < M.n_cells && !same(EA[K], EC[ic])) d = D_DEP + 64;
    if (ic >= M.n_cells && flew) info[0] += 1;  // crossings of virtual cells: their deposits went to halo slots
    if (d != D_NONE) { *where = d; ++k; break; }
  }
  *steps = k;
  info[1] += (int)a.c_dark;
}

// n packets, s: n x 6 (x, y, z, u, v, w); extr, star_key (plain encoding), force_ri, force_zj per packet; dark_every > 0:
// every dark_every-th cell is dark; variant 0: plain, 1: MRW.
// Per packet: crossings walked, the code of the first difference (0: none).  EA, EB: the padded paths' deposits
// (pad_cells_2d slots), EC: the specification's (n_cells + 1), summed over all packets in the same order.
// info[0]: crossings of virtual cells, info[1]: packets mirrored at a dark cell; delta[0..1]: the smallest and the largest
// positive discriminant of the radial wall met on the way.
extern "C" int emu_fly_pad_compare(const oracle_model* m, int dark_every, int variant, int n, const double* s, const double* extr,
                                   const int* star_key, const int* force_ri, const int* force_zj, int kmax, int* steps,
                                   int* where, double* EA, double* EB, double* EC, int* info, double* delta) {
  Conv cv(m);
  if (cv.voro || m->l3D || cv.M.grid_sph || lds_bytes(cv.M) > sizeof(lds_raw)) return 31;
  DevModel M = cv.M;
  const int np = pad_cells_2d(M.n_rad, M.nz);
  // the tables as mcgpu_set_opacity lays them out: the plain entries, then the padded copy
  std::vector<double> kf((size_t)M.n_cells + 1 + np, 0.0);
  memcpy(kf.data(), m->kappa_factor, sizeof(double) * M.n_cells);
  pad_table_2d(M.n_rad, M.nz, m->kappa_factor, kf.data() + M.n_cells + 1);
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
  g_delta_min = 1e300; g_delta_max = 0.0;
  info[0] = info[1] = 0;
  for (int i = 0; i < n; ++i) {
    const double* si = s + 6 * i;
#define WALK(D, W) walk_one<D, W>(T, M, A, si, extr[i], star_key[i], force_ri[i], force_zj[i], kmax, EA, EB, EC, steps + i, where + i, info)
    if (dark_every > 0) { if (variant == 1) WALK(true, true); else WALK(true, false); }
    else { if (variant == 1) WALK(false, true); else WALK(false, false); }
#undef WALK
  }
  delta[0] = g_delta_min; delta[1] = g_delta_max;
  return err;
}

// The padded copy of a table of n_rad x nz values (padded: pad_cells_2d values) and, per padded key, the plain index of
// its cell (-1: halo) -- what mcgpu_set_opacity and the folds of roles_body use.
extern "C" void emu_pad_layout(int n_rad, int nz, const double* plain, double* padded, int* cell_of_key) {
  pad_table_2d(n_rad, nz, plain, padded);
  for (int K = 0; K < pad_cells_2d(n_rad, nz); ++K) cell_of_key[K] = pad_cell_of_key(n_rad, nz, K);
}

// The folds of roles_body on a padded private grid E_pad (pad_fold_rows): every slice of n_waves, 64 lanes each, once round,
// added to E_out (n_rad * nz values) at the plain index; visits[K] counts how often slot K was folded.  Returns the number
// of slots folded.
extern "C" int emu_pad_fold(int n_rad, int nz, int n_waves, const double* E_pad, double* E_out, int* visits) {
  int folded = 0;
  for (int slice = 0; slice < n_waves; ++slice)
    for (int lane = 0; lane < 64; ++lane)
      pad_fold_rows(n_rad, nz, n_waves, slice, lane, [&](int K, int ic) {
        visits[K] += 1;
        E_out[ic] += E_pad[K];
        ++folded;
      });
  return folded;
}

// sqrt_nonneg's Newton sequence (mc_device.hip.h) from a seed y ~ 1 / sqrt(x) -- the host has no v_rsq_f64; any seed of
// a few good bits runs the same sequence, and x = 0 gives the same infinite seed -- with the old zero case (a select) and
// the new one (a maximum).
extern "C" void emu_sqrt_zero_case(int n, const double* x, double* with_select, double* with_max) {
  for (int i = 0; i < n; ++i) {
    double y = 1.0 / std::sqrt(x[i]);   // (cut to about 24 bits, as the instruction gives)
    y = __longlong_as_double(__double_as_longlong(y) & ~0xFFFFFFFll);
    // the old form, written out: the sequence with a select for x = 0 ...
    double g = x[i] * y;
    double h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x[i]);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x[i]);
    g = __builtin_fma(d, h, g);
    with_select[i] = (x[i] == 0.0) ? 0.0 : g;
    // ... and the shipped one: the device's own function, from the same seed
    with_max[i] = mcgpu::sqrt_nonneg_from_seed(x[i], y);
  }
}
