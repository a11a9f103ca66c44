// emu_nlte.cpp -- TEST INFRASTRUCTURE: the device header of the grains out of LTE (mcfost_amd/csrc/mc_nlte.hip.h)
// compiled for the host: one emulated lane plays the 64 lanes of a wave in turn and adds their partial sums in the wave's
// own tree, so an event is computed here bit for bit as a wave computes it (up to libm's exp / log).  Built only by
// tests/test_nlte.py; nothing in mcfost_amd/ references it.
#define MCGPU_LANE_EMULATION 1
#include <math.h>
#include <stdint.h>

#define __device__
#define __host__
#define __forceinline__ inline
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))

#include "../../mcfost_amd/csrc/mc_nlte.hip.h"

using namespace mcgpu;

extern "C" {

// tables in the DEVICE layouts of NlteArgs (the caller transposes as mcgpu_set_nlte does)
int emu_nlte_events(int n_grains, int n_lambda, int n_T, int n_cells, const float* Cabs, const double* kcdf, const double* lE,
                    const double* cdf, const float* tab_Temp, const double* J0, const double* volume, double L_packet_th,
                    int n, const int* icell, const int* lambda0, const float* rand1, const float* rand2, int* k_out,
                    int* T_int_out, double* Temp_out, int* lambda_out) {
  NlteArgs N{};
  N.n_grains = n_grains; N.n_lambda = n_lambda; N.n_T = n_T; N.n_cells = n_cells; N.ldJ = nlte_ldJ(n_lambda);
  N.Cabs = Cabs; N.kcdf = kcdf; N.lE = lE; N.cdf = cdf; N.tab_Temp = tab_Temp; N.J0 = J0; N.L_packet_th = L_packet_th;
  for (int i = 0; i < n; ++i) {
    if (icell[i] < 1 || icell[i] > n_cells || lambda0[i] < 1 || lambda0[i] > n_lambda) return 1;
    const int ic = icell[i] - 1;
    const NlteEvent e = nlte_event(N, volume[ic], ic, lambda0[i], rand1[i], rand2[i], false, 1.0, 0);
    k_out[i] = e.k; T_int_out[i] = e.T_int; Temp_out[i] = e.Temp; lambda_out[i] = e.lambda;
  }
  return 0;
}

// Temp_finale_nLTE from xJ + J0, both [n_cells][ldJ]; dens [n_cells][n_grains] or null; out [n_cells][n_grains]
int emu_nlte_temp_finale(int n_grains, int n_lambda, int n_T, int n_cells, const float* Cabs, const double* lE,
                         const float* tab_Temp, const double* J0, double* xJ, const double* dens, const double* volume,
                         double L_packet_th, float T_min, float* Tdust_1grain) {
  NlteArgs N{};
  N.n_grains = n_grains; N.n_lambda = n_lambda; N.n_T = n_T; N.n_cells = n_cells; N.ldJ = nlte_ldJ(n_lambda);
  N.Cabs = Cabs; N.lE = lE; N.tab_Temp = tab_Temp; N.J0 = J0; N.xJ = xJ; N.dens = dens; N.L_packet_th = L_packet_th;
  for (int ic = 0; ic < n_cells; ++ic)
    for (int k = 1; k <= n_grains; ++k) Tdust_1grain[(size_t)ic * n_grains + (k - 1)] = nlte_final_temp(N, volume[ic], k, ic, T_min, 0);
  return 0;
}

}  // extern "C"
