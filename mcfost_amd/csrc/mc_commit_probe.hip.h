// Unit probe of the SED commit pass's atomic deposit staging (mcgpu_probe_xi_commit, mcgpu.hip;
// tests/test_xi_commit_exact.py): the wave functions of mc_mono.hip.h that exist only for whole waves on the GPU --
// wave_deposit_records, deposit_rt1_wave_f32, deposit_rt1_wave_row, rt1_store_weights / row_put, angles_scatt_rt1_wave --
// run by whole workgroups on deposits the caller chooses, so that a test can put every lane of eight waves into one
// sub-bin, leave a wave one depositing lane or none, keep a lane's results across rounds in which its neighbours start
// new flights, and compare the array with integer-valued inputs bit for bit.
//
// Round r of the launch: global thread g handles item r * T + g (T = threads of the launch), every lane in converged flow
// as mono_body calls the functions.  The kernel carves its own LDS (xi_commit_probe_lds): the per-lane results in the form
// the path under test reads, the per-wave tiles, the Mueller columns, the observers' rotation constants.
#pragma once
#include "mc_mono.hip.h"

namespace mcgpu {

struct XiCommitProbe {
  int mode;      // 0: deposits, 1: angles_scatt_rt1 (the per-lane results are copied out after every round)
  int path;      // mode 0: 0 deposit_rt1_wave (FP64 records), 1 deposit_rt1_wave_f32 with the flight's weights,
                 //         2 deposit_rt1_wave_row, 3 deposit_rt1_wave_f32 with dust classes (weights per crossing)
  int n_rounds;
  int by_wave;   // mode 1: angles_scatt_rt1_wave (1) or the per-lane angles_scatt_rt1 (0)
  int with_mu;   // mode 1: the deposit weights are computed (w_mu) instead of the angles
  // per item
  const int* where;      // [n][4] icell (0: no deposit), psup, phik, flags: bit 0 flag_star, bit 1 a new flight starts
  const float* l;        // [n] path length
  const float* weights;  // paths 1, 2: [n][nRT][4 with Stokes tracking, else 1], read where a new flight starts
  const int* itheta;     // paths 0, 3: [n][nRT]
  const double* cosw;    // paths 0, 3 with Stokes tracking: [n][nRT]
  const double* sinw;
  const double* S;       // paths 0, 3 and mode 1: [n][4]
  const double* dir;     // mode 1: [n][3]
  const float* mu;       // [6][nang + 1] the Mueller columns of p_lambda
  // mode 1: the per-lane results after every round
  float* dump_row;       // [n][rowf]
  int* dump_itheta;      // [n][nRT]
  double* dump_cosw;     // [n][nRT] (the 8 bytes of the slot, whatever they hold)
  double* dump_sinw;
};

struct XiCommitProbeLds {
  size_t tile, tile_addr, cosw, sinw, rot, row, itheta, tile_mask, mu, bytes;
};
__host__ __device__ inline XiCommitProbeLds xi_commit_probe_lds(int nang, int nRT, int threads, bool pola, int rowf) {
  XiCommitProbeLds L;
  size_t b = 0;
  L.tile = b; b += (size_t)threads * XI_LINE * sizeof(double);
  L.tile_addr = b; b += (size_t)threads * sizeof(unsigned long long);
  L.cosw = b; b += (rowf > 0 || !pola) ? 0 : (size_t)nRT * threads * sizeof(double);
  L.sinw = b; b += (rowf > 0 || !pola) ? 0 : (size_t)nRT * threads * sizeof(double);
  L.rot = b; b += (size_t)3 * nRT * sizeof(double);
  b = (b + 15) / 16 * 16;
  L.row = b; b += (size_t)(rowf > 0 ? rowf : 0) * threads * sizeof(float);
  L.itheta = b; b += rowf > 0 ? 0 : (size_t)nRT * threads * sizeof(int);
  L.tile_mask = b; b += (size_t)threads * sizeof(unsigned int);
  L.mu = b; b += (size_t)6 * (nang + 1) * sizeof(float);
  L.bytes = (b + 15) / 16 * 16;
  return L;
}

template <bool POLA>
__global__ void __launch_bounds__(512) k_probe_xi_commit(const DevModel M, const MonoArgs A, const XiCommitProbe P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xi_commit_probe_raw[];
  const int tid = (int)threadIdx.x, nth = (int)blockDim.x, na1 = M.nang + 1, nRT = A.nRT;
  const XiCommitProbeLds C = xi_commit_probe_lds(M.nang, nRT, nth, POLA, A.rowf);
  unsigned char* const base = xi_commit_probe_raw;
  RtScratch R;
  R.cosw = reinterpret_cast<double*>(base + C.cosw);
  R.sinw = reinterpret_cast<double*>(base + C.sinw);
  R.itheta = reinterpret_cast<int*>(base + C.itheta);
  double* const rot = reinterpret_cast<double*>(base + C.rot);
  R.rot = rot;
  float* const row = A.rowf > 0 ? reinterpret_cast<float*>(base + C.row) : nullptr;
  float* const mu = reinterpret_cast<float*>(base + C.mu);
  double* const tile = reinterpret_cast<double*>(base + C.tile) + (size_t)(tid >> 6) * 64 * XI_LINE;   // this wave's
  unsigned long long* const tile_addr = reinterpret_cast<unsigned long long*>(base + C.tile_addr) + (size_t)(tid >> 6) * 64;
  unsigned int* const tile_mask = reinterpret_cast<unsigned int*>(base + C.tile_mask) + (size_t)(tid >> 6) * 64;
  // (mono_lds_setup: the row's padding is zero for the whole launch; here every per-lane result starts from zero)
  if (row) for (size_t i = tid; i < (size_t)A.rowf * nth; i += nth) row[i] = 0.0f;
  else {
    for (size_t i = tid; i < (size_t)nRT * nth; i += nth) R.itheta[i] = 0;
    if (POLA) for (size_t i = tid; i < (size_t)nRT * nth; i += nth) { R.cosw[i] = 0.0; R.sinw[i] = 0.0; }
  }
  for (int i = tid; i < 6 * na1; i += nth) mu[i] = P.mu[i];
  if (P.mode == 1) for (int q = tid; q < nRT; q += nth) rt1_observer_rot(A, q, rot + 3 * q);
  __syncthreads();

  const unsigned long long T = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nv = POLA ? 4 : 1;
  double S[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < P.n_rounds; ++r) {
    const unsigned long long i = (unsigned long long)r * T + g;
    const int4 wh = reinterpret_cast<const int4*>(P.where)[i];
    const bool star = (wh.w & 1) != 0, fresh = (wh.w & 2) != 0;
    if (P.mode == 1) {
      const double u = P.dir[3 * i], v = P.dir[3 * i + 1], w = P.dir[3 * i + 2];
      const double Sn[4] = {P.S[4 * i], P.S[4 * i + 1], P.S[4 * i + 2], P.S[4 * i + 3]};
      const float* const w_mu = P.with_mu ? mu : nullptr;
      if (P.by_wave) angles_scatt_rt1_wave<POLA>(M, A, R, fresh, u, v, w, w_mu, Sn, tile, row, star);
      else if (fresh) angles_scatt_rt1<POLA>(M, A, R, u, v, w, w_mu, Sn, nullptr, row, star);
      if (row) {
        for (int p = 0; p < A.rowf; ++p) P.dump_row[i * A.rowf + p] = row[(((size_t)(p >> 2) * nth + tid) << 2) + (p & 3)];
      } else {
        for (int q = 0; q < nRT; ++q) {
          P.dump_itheta[i * nRT + q] = R.itheta[q * nth + tid];
          if (POLA) { P.dump_cosw[i * nRT + q] = R.cosw[q * nth + tid]; P.dump_sinw[i * nRT + q] = R.sinw[q * nth + tid]; }
        }
      }
      continue;
    }
    if (fresh) {   // the lane's per-lane results are rewritten; otherwise those of its previous flight still serve
      if (P.path == 0 || P.path == 3) {
        for (int q = 0; q < nRT; ++q) {
          R.itheta[q * nth + tid] = P.itheta[i * nRT + q];
          if (POLA) { R.cosw[q * nth + tid] = P.cosw[i * nRT + q]; R.sinw[q * nth + tid] = P.sinw[i * nRT + q]; }
        }
        S[0] = P.S[4 * i]; S[1] = P.S[4 * i + 1]; S[2] = P.S[4 * i + 2]; S[3] = P.S[4 * i + 3];
      } else {
        for (int q = 0; q < nRT; ++q) {
          const float* f = P.weights + (i * nRT + q) * nv;
          rt1_store_weights<POLA, Rt1WeightsGiven>(A, R, q, tid, nullptr, row, star, (double)f[0], POLA ? (double)f[1] : 0.0,
                                                   POLA ? (double)f[2] : 0.0, POLA ? (double)f[3] : 0.0, 0.0, 0.0);
        }
      }
    }
    RtDeposit D;
    D.on = wh.x != 0; D.icell = D.on ? wh.x : 1; D.psup = D.on ? wh.y : 1; D.phik = D.on ? wh.z : 1; D.l = D.on ? (double)P.l[i] : 0.0;
    if (__ballot(D.on) != 0ull) {   // (mono_body)
      if (P.path == 0) deposit_rt1_wave<POLA>(M, A, R, mu, D, S, star, tile, tile_addr, tile_mask);
      else if (P.path == 2) deposit_rt1_wave_row(A, row, D, star, tile, tile_addr);
      else deposit_rt1_wave_f32<POLA>(M, A, R, mu, D, S, star, tile, tile_addr, tile_mask);
    }
  }
}

}  // namespace mcgpu
