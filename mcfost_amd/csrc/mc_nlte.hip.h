// mc_nlte.hip.h -- the grains in radiative equilibrium but out of LTE (lRE_nLTE, methode_chauffage = 2): one temperature
// per grain size and cell instead of one per cell.
//
//   im_reemission_NLTE  (thermal_emission.f90:775-866)  nlte_event()       one absorption + re-emission by such a grain
//   Temp_finale_nLTE    (thermal_emission.f90:932-1014) nlte_final_temp()  the grain's temperature at the end of the step
//   init_reemission's lRE_nLTE block (:552-582)         nlte_init_row()    log_E_em_1grain(k, T), kdB_dT_1grain_nLTE_CDF(:, k, T)
//
// The event is written ONCE, for a whole wave: the reference forms
//     J_abs = sum_lambda C_abs_norm(k, lambda) * (xJ_abs(icell, lambda) + J0(icell, lambda))
// at every absorption -- a dot product over the whole wavelength grid against a live accumulator.  A wave serves the event
// of one of its lanes together: lane j sums lambda = j, j + 64, ... (a cell's wavelengths are contiguous, so the wave reads
// ceil(8 n_lambda / 64) lines), the 64 partial sums are added in a fixed tree, and the grain bisection, the temperature
// search and the wavelength bisection run on wave-uniform values.  The order of the sum does not depend on which lanes
// asked, so an event's result depends on its inputs alone.  The launch (thermal_body<..., NLTE = true>, mc_device.hip.h),
// the probe, the final-temperature kernel (kern_nlte.hip) and the one-lane CPU build of the tests (one emulated lane plays
// the 64 lanes in turn, same tree) all call the functions below.
//
// The reference's ratchet xT_ech_1grain (the search for T_int starts where the last event of the grain and cell ended) is
// replaced by a bisection of log_E_em_1grain(k, :): the same answer wherever that row does not decrease with T, which the
// setters check (the in-flight J_abs of a cell only grows).
#pragma once
#ifndef MCGPU_LANE_EMULATION
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace mcgpu {

constexpr double NLTE_TINY_DP = 2.22507385850720138309e-308;   // tiny_dp

// What a non-LTE launch reads besides DevModel / RunArgs (a kernel argument of its own: the structures every other kernel
// takes stay as they are).  Device layouts, as mcgpu_set_nlte lays them out (0-based C indices):
struct NlteArgs {
  int n_grains;            // grain_RE_nLTE_end - grain_RE_nLTE_start + 1; grains are numbered 1 .. n_grains here
  int n_lambda, n_T, n_cells;
  int ldJ;                 // doubles per cell of J0 / xJ: n_lambda rounded up to whole 64-byte lines
  const float* Cabs;       // [n_grains][n_lambda]      C_abs_norm(k, lambda) (default real)
  const double* kcdf;      // [n_lambda][n_grains + 1]  kabs_nLTE_CDF(0:n, lambda) of the single dust class
  const double* proba;     // [n_lambda][n_cells]       Proba_abs_RE_LTE(icell, lambda); null: lonly_nLTE
  const double* lE;        // [n_grains][n_T]           log_E_em_1grain(k, T)
  const double* cdf;       // [n_grains][n_T][n_lambda] kdB_dT_1grain_nLTE_CDF(lambda, k, T)
  const float* tab_Temp;   // [n_T]
  const double* J0;        // [n_cells][ldJ] or null (zeros)
  double* xJ;              // [n_cells][ldJ] the launch's xJ_abs accumulator (a cell's wavelengths contiguous)
  const double* dens;      // [n_cells][n_grains] dust_density_o_n_grains(k, icell) n_grains(k), or null (present everywhere)
  double L_packet_th;
  unsigned long long* stats;  // [0] events served, [1] wave visits that served at least one (null: not counted)
};

struct NlteEvent {
  int k;         // the absorbing grain, 1 .. n_grains
  int T_int;     // 2 .. n_T
  double Temp;
  int lambda;    // the new wavelength, 1 .. n_lambda
};

inline int nlte_ldJ(int n_lambda) { return (n_lambda + 7) / 8 * 8; }

#ifdef MCGPU_LANE_EMULATION
static inline int nlte_readlane(int v, int) { return v; }
static inline float nlte_readlane_f(float v, int) { return v; }
static inline double nlte_uniform(double v) { return v; }
static inline double nlte_fma(double a, double b, double c) { return ::fma(a, b, c); }
#else
// the value of lane `src` (wave-uniform, from a ballot) as a scalar
__device__ __forceinline__ int nlte_readlane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float nlte_readlane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
// a value every lane holds alike, as a scalar: what follows branches and addresses tables without divergence
__device__ __forceinline__ double nlte_uniform(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)b);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)((unsigned long long)b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double nlte_fma(double a, double b, double c) { return fma(a, b, c); }
#endif

// lane j's part of the sum: lambda = j + 1, j + 65, ... in increasing order.  live: the accumulator of the running launch,
// scaled like the live E_abs of the LTE branch (partial * nb_proc, thermal_emission.f90:670) and read the way that branch
// reads it -- relaxed agent-scope loads: the lines are written by atomics from every XCD and a plain cached load may keep
// returning an old copy; frozen: J0 alone.
__device__ inline double nlte_partial(const NlteArgs& N, const float* C, const double* J0, const double* xJ, bool live,
                                      double qscale, int j) {
  double p = 0.0;
  for (int l = j; l < N.n_lambda; l += 64) {
    double J = J0 ? J0[l] : 0.0;
    if (live) J = nlte_fma(__hip_atomic_load(&xJ[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), qscale, J);
    p = nlte_fma((double)C[l], J, p);
  }
  return p;
}

// J_abs of grain k (1-based) in cell ic (0-based): 64 partial sums, then the tree ((0+32)+(16+48))+... of a butterfly.
// Every lane of the wave calls it with the same arguments and receives the same bits.
__device__ inline double nlte_J_abs(const NlteArgs& N, int k, int ic, bool live, double qscale, int lane) {
  const float* C = N.Cabs + (size_t)(k - 1) * N.n_lambda;
  const double* J0 = N.J0 ? N.J0 + (size_t)ic * N.ldJ : nullptr;
  const double* xJ = N.xJ + (size_t)ic * N.ldJ;
#ifdef MCGPU_LANE_EMULATION
  (void)lane;
  double s[64];
  for (int j = 0; j < 64; ++j) s[j] = nlte_partial(N, C, J0, xJ, live, qscale, j);
  for (int off = 32; off > 0; off >>= 1)
    for (int j = 0; j < off; ++j) s[j] = s[j] + s[j + off];   // (lane j of the butterfly: s[j] + s[j ^ off])
  return s[0];
#else
  double p = nlte_partial(N, C, J0, xJ, live, qscale, lane);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) p = p + __shfl_xor(p, off);
  return nlte_uniform(p);
#endif
}

// The same sum by ONE lane, lambda = 1 .. n_lambda in order: the alternative to the wave-served event, kept for measuring
// it (-DMCGPU_NLTE_ONE_LANE tuning builds, tools/nlte_bench.py); the order of the sum, hence its last bits, differ.
__device__ inline double nlte_J_abs_lane(const NlteArgs& N, int k, int ic, bool live, double qscale) {
  const float* C = N.Cabs + (size_t)(k - 1) * N.n_lambda;
  const double* J0 = N.J0 ? N.J0 + (size_t)ic * N.ldJ : nullptr;
  const double* xJ = N.xJ + (size_t)ic * N.ldJ;
  double p = 0.0;
  for (int l = 0; l < N.n_lambda; ++l) {
    double J = J0 ? J0[l] : 0.0;
    if (live) J = nlte_fma(__hip_atomic_load(&xJ[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), qscale, J);
    p = nlte_fma((double)C[l], J, p);
  }
  return p;
}

// the sampled temperature just above log_E_abs in the grain's row (1-based, 2 .. n_T): what the reference's ratchet
// (:823-828) ends on when the row does not decrease
__device__ inline int nlte_T_int(const double* lE_k, int n_T, double log_E_abs) {
  int lo = 2, hi = n_T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lE_k[mid - 1] < log_E_abs) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Temp between the two sampled temperatures (:833-838)
__device__ inline double nlte_interp_temp(const NlteArgs& N, const double* lE_k, int T_int, double log_E_abs, double& Temp1,
                                          double& Temp2) {
  Temp2 = (double)N.tab_Temp[T_int - 1];
  Temp1 = (double)N.tab_Temp[T_int - 2];
  const double frac = (log_E_abs - lE_k[T_int - 2]) / (lE_k[T_int - 1] - lE_k[T_int - 2]);
  return exp(log(Temp2) * frac + log(Temp1) * (1.0 - frac));
}

// im_reemission_NLTE: every argument wave-uniform (WAVE = false: one lane's own event); ic 0-based, lambda0 1-based
template <bool WAVE = true>
__device__ inline NlteEvent nlte_event(const NlteArgs& N, double volume, int ic, int lambda0, float rand1, float rand2,
                                       bool live, double qscale, int lane) {
  NlteEvent e;
  // the grain that absorbs (:798-810; kmin starts on the first grain, as there)
  {
    const double* c = N.kcdf + (size_t)(lambda0 - 1) * (N.n_grains + 1);
    int kmin = 1, kmax = N.n_grains, k = (kmin + kmax) / 2;
    while ((kmax - kmin) > 1) {
      if (c[k] < (double)rand1) kmin = k; else kmax = k;
      k = (kmin + kmax) / 2;
    }
    e.k = kmax;
  }
  const double J_abs = WAVE ? nlte_J_abs(N, e.k, ic, live, qscale, lane) : nlte_J_abs_lane(N, e.k, ic, live, qscale);
  const double log_E_abs = log(J_abs * N.L_packet_th / volume);   // :820
  const double* lE_k = N.lE + (size_t)(e.k - 1) * N.n_T;
  e.T_int = nlte_T_int(lE_k, N.n_T, log_E_abs);
  double Temp1, Temp2;
  e.Temp = nlte_interp_temp(N, lE_k, e.T_int, log_E_abs, Temp1, Temp2);
  // the wavelength: bisection in the CDF interpolated between the two temperatures (:843-861)
  const double frac_T2 = (e.Temp - Temp1) / (Temp2 - Temp1);
  const double frac_T1 = 1.0 - frac_T2;
  const double* cdf1 = N.cdf + ((size_t)(e.k - 1) * N.n_T + (size_t)(e.T_int - 2)) * N.n_lambda;
  const double* cdf2 = cdf1 + N.n_lambda;
  int l1 = 0, l2 = N.n_lambda, l = (l1 + l2) / 2;
  while ((l2 - l1) > 1) {
    const double proba = frac_T1 * cdf1[l - 1] + frac_T2 * cdf2[l - 1];
    if ((double)rand2 > proba) l1 = l; else l2 = l;
    l = (l1 + l2) / 2;
  }
  e.lambda = l + 1;
  return e;
}

// Temp_finale_nLTE for one (grain, cell) (:961-1006), every argument wave-uniform; from the accumulator as it is
// (xJ_abs + J0, no scaling: the step is over)
__device__ inline float nlte_final_temp(const NlteArgs& N, double volume, int k, int ic, float T_min, int lane) {
  if (N.dens && !(N.dens[(size_t)ic * N.n_grains + (k - 1)] > NLTE_TINY_DP)) return 0.0f;
  const double J_absorbe = nlte_J_abs(N, k, ic, true, 1.0, lane) * N.L_packet_th / volume;
  if (J_absorbe < NLTE_TINY_DP) return T_min;
  const double log_E_abs = log(J_absorbe);
  const double* lE_k = N.lE + (size_t)(k - 1) * N.n_T;
  if (log_E_abs < lE_k[0]) return T_min;
  const int T_int = nlte_T_int(lE_k, N.n_T, log_E_abs);
  double Temp1, Temp2;
  return (float)nlte_interp_temp(N, lE_k, T_int, log_E_abs, Temp1, Temp2);
}

// init_reemission, the lRE_nLTE block for one (grain, T) (:552-582): the sums run in the reference's order over lambda.
// No tab_Temp(1) floor and no density, unlike the LTE table; the CDF starts at the SECOND wavelength (integ3(1) = 0).
// C: the grain's C_abs_norm row; row: the CDF's n_lambda values; returns log_E_em_1grain(k, T).
__device__ inline double nlte_init_row(double Temp, int n_lambda, const double* tab_lambda, const double* tab_delta_lambda,
                                       const float* C, double* row) {
  const float thermal_const = (float)(299792458.0 * 6.626070040e-34 / 1.38064852e-23);  // constants.f90:24
  const double cst_E = 2.0 * 6.626070040e-34 * (299792458.0 * 299792458.0) * (4.0 * 3.141592653589793238462643383279502884197);
  const double cst = (double)thermal_const / Temp;
  double integ = 0.0, integ3 = 0.0;
  for (int l = 0; l < n_lambda; ++l) {
    const double wl = tab_lambda[l] * (double)1.e-6f;  // default-real literals (:439-440)
    const double delta_wl = tab_delta_lambda[l] * (double)1.e-6f;
    const double cst_wl = cst / wl;
    double B = 0.0, dB_dT = 0.0;
    if (cst_wl < 500.0) {
      const double coeff_exp = exp(cst_wl);
      const double wl2 = wl * wl, wl5 = (wl2 * wl2) * wl;
      B = 1.0 / (wl5 * (coeff_exp - 1.0)) * delta_wl;
      dB_dT = B * cst_wl * coeff_exp / (coeff_exp - 1.0);
    }
    integ = integ + (double)C[l] * B;
    if (l > 0) integ3 = integ3 + (double)C[l] * dB_dT;
    row[l] = integ3;
  }
  const double tot = row[n_lambda - 1];
  const bool ok = tot > NLTE_TINY_DP;   // (the table stays 0 otherwise)
  for (int l = 0; l < n_lambda; ++l) row[l] = ok ? row[l] / tot : 0.0;
  return (integ > NLTE_TINY_DP) ? log(integ * cst_E) : -1000.0;
}

}  // namespace mcgpu
