// Translation unit of the grains out of LTE (mc_nlte.hip.h): k_thermal_nlte, the non-LTE instantiation of the single-role
// packet kernel (thermal_body<..., NLTE = true>, mc_device.hip.h), and the small kernels around it -- the probe of one
// re-emission event, Temp_finale_nLTE, the per-grain re-emission tables and the lRE_nLTE term of repartition_energie.
// See mc_kernels.h.
#include <hip/hip_runtime.h>

#include "mc_device.hip.h"
#include "mc_kernels.h"

namespace mcgpu {

template <bool L3D, bool POLA, bool DARK, bool LDSE>
__global__ void __launch_bounds__(LDSE ? MCGPU_LDS_BLOCK : 256) k_thermal_nlte(const DevModel M, const RunArgs A, const NlteArgs N) {
  extern __shared__ double lds_raw[];
  thermal_body<L3D, POLA, DARK, LDSE, false, false, false, true>(M, A, lds_raw, &N);
}

// one re-emission event per wave, evaluated on J0 (frozen), as the launch serves it
static __global__ void __launch_bounds__(256) k_probe_reemission_nlte(const NlteArgs N, const double* volume, int n, const int* icell,
                                                                      const int* lambda0, const float* rand1, const float* rand2,
                                                                      int* k_out, int* T_int_out, double* Temp_out, int* lambda_out) {
  const int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;   // (wave-uniform)
  const int ic = icell[i] - 1;
  const NlteEvent e = nlte_event(N, volume[ic], ic, lambda0[i], rand1[i], rand2[i], false, 1.0, lane);
  if (lane == 0) { k_out[i] = e.k; T_int_out[i] = e.T_int; Temp_out[i] = e.Temp; lambda_out[i] = e.lambda; }
}

// Temp_finale_nLTE: one cell per wave, its grains one after the other; Tdust_1grain(k, icell)
static __global__ void __launch_bounds__(256) k_temp_finale_nlte(const NlteArgs N, const double* volume, float T_min, float* Tdust_1grain) {
  const int ic = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (ic >= N.n_cells) return;   // (wave-uniform)
  for (int k = 1; k <= N.n_grains; ++k) {
    const float Temp = nlte_final_temp(N, volume[ic], k, ic, T_min, lane);
    if (lane == 0) Tdust_1grain[(size_t)ic * N.n_grains + (k - 1)] = Temp;
  }
}

// the per-grain re-emission tables: one thread per (grain, T), the wavelength sums in the reference's order
static __global__ void k_init_reemission_nlte(int n_grains, int n_T, int n_lambda, const float* tab_Temp, const double* tab_lambda,
                                              const double* tab_delta_lambda, const float* Cabs, double* lE, double* cdf) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_grains * n_T) return;
  const int k = idx / n_T, t = idx - k * n_T;
  lE[(size_t)k * n_T + t] = nlte_init_row((double)tab_Temp[t], n_lambda, tab_lambda, tab_delta_lambda, Cabs + (size_t)k * n_lambda,
                                          cdf + ((size_t)k * n_T + t) * n_lambda);
}

// repartition_energie, the lRE_nLTE term (thermal_emission.f90:1832-1850): E_cell(icell) += the grains' emission at the
// wavelength; Tdust_1grain [n_cells][n_grains], dens [n_cells][n_grains] = dust_density_o_n_grains(k, icell) n_grains(k)
static __global__ void k_repart_nlte(int n_cells, int n_grains, const float* Cabs_l, int ldC, double wl, const float* Tdust_1grain,
                                     const double* dens, const double* volume, const unsigned char* dark, double* E_cell, double* E_corr) {
  const int ic = blockIdx.x * blockDim.x + threadIdx.x;
  if (ic >= n_cells) return;
  const float thermal_const = (float)(299792458.0 * 6.626070040e-34 / 1.38064852e-23);
  const double cst_wl_max = 88.72283905206835 - (double)1.0e-4f;   // log(huge_real) - 1.0e-4 (:1802)
  double E_emise = 0.0;
  if (!(dark && dark[ic])) {
    for (int k = 0; k < n_grains; ++k) {
      const float Temp = Tdust_1grain[(size_t)ic * n_grains + k];
      if (Temp > FLT_TINY) {
        const double cst_wl = (double)thermal_const / ((double)Temp * wl);
        if (cst_wl < cst_wl_max) {
          const double wl2 = wl * wl, wl5 = (wl2 * wl2) * wl;
          E_emise = E_emise + 4.0 * (double)Cabs_l[(size_t)k * ldC] * dens[(size_t)ic * n_grains + k] * volume[ic] / (wl5 * (exp(cst_wl) - 1.0));
        }
      }
    }
  }
  E_cell[ic] = E_cell[ic] + E_emise;
  E_corr[ic] = E_corr[ic] + E_emise;   // (weight_proba_emission is 1 wherever the call is accepted)
}

const void* kpick_thermal_nlte(bool lds, bool l3d, bool pola, bool dark) {
  return bsel(lds, [&](auto LDSE) { return bsel(l3d, [&](auto L3D) { return bsel(pola, [&](auto POLA) {
    return bsel(dark, [&](auto DARK) -> const void* {
      return (const void*)k_thermal_nlte<MCGPU_BV(L3D), MCGPU_BV(POLA), MCGPU_BV(DARK), MCGPU_BV(LDSE)>;
    }); }); }); });
}
const void* kpick_probe_reemission_nlte() { return (const void*)k_probe_reemission_nlte; }
const void* kpick_temp_finale_nlte() { return (const void*)k_temp_finale_nlte; }
const void* kpick_init_reemission_nlte() { return (const void*)k_init_reemission_nlte; }
const void* kpick_repart_nlte() { return (const void*)k_repart_nlte; }

}  // namespace mcgpu
