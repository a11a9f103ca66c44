// emu_xi_commit.cpp -- TEST INFRASTRUCTURE: the value-by-value forms of deposit_rt1_wave (mcfost_amd/csrc/mc_mono.hip.h
// under MCGPU_LANE_EMULATION: the FP64 records and the packed default-real layout) on deposits the caller chooses, one
// emulated lane after the other.  tests/test_xi_commit_reference.py holds the int64 reference of
// tests/xi_commit_cases.py against it, so that a mismatch of the wave functions on the GPU
// (tests/test_xi_commit_exact.py) points at their staging.  Built only by that test; nothing in mcfost_amd/ references it.
#include "emu_kernel.cpp"

// deposit i: where[i] = (icell, psup, phik, flag_star), path length l[i], the flight's per-lane results itheta, cosw,
// sinw [i][nRT] and Stokes vector S[i][4].  mu [6][nang + 1]; with n_classes the class tables vtab
// [6][n_classes][n_lambda][nang + 1] and cell_class [n_cells] instead.  xI += the deposits: double [sub-bin][nRT][8], or
// (f32) float [sub-bin][binf].
extern "C" int emu_xi_commit(int n, const int* where, const double* l, const int* itheta, const double* cosw, const double* sinw,
                             const double* S, const float* mu, int nang, int nRT, int pola, int contrib, int f32, int n_cells,
                             int n_theta_rt, int n_az_rt, int n_classes, int n_lambda, int p_lambda, const int* cell_class,
                             const float* vtab, void* xI) {
  DevModel M;
  memset(&M, 0, sizeof(M));
  MonoArgs A;
  memset(&A, 0, sizeof(A));
  M.nang = nang; M.n_cells = n_cells;
  if (n_classes) {
    const size_t nt = (size_t)n_classes * n_lambda * (nang + 1);
    M.n_classes = n_classes; M.n_lambda = n_lambda; M.cell_class = cell_class;
    M.v_s11 = vtab; M.v_s12 = vtab + nt; M.v_s22 = vtab + 2 * nt; M.v_s33 = vtab + 3 * nt; M.v_s34 = vtab + 4 * nt; M.v_s44 = vtab + 5 * nt;
  }
  A.nRT = nRT; A.RT_n_incl = nRT; A.contrib = contrib; A.N_type_flux = (pola ? 4 : 1) + (contrib ? 4 : 0);
  A.n_theta_rt = n_theta_rt; A.n_az_rt = n_az_rt; A.p_lambda = n_classes ? p_lambda : 1; A.rt1 = 1;
  A.xI = reinterpret_cast<double*>(xI); A.xI_f32 = f32; A.xi = xi32_layout(nRT, pola != 0, contrib != 0);
  blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  std::vector<int> it(nRT);
  std::vector<double> cw(nRT), sw(nRT);
  RtScratch R;
  R.itheta = it.data(); R.cosw = cw.data(); R.sinw = sw.data(); R.rot = nullptr;
  for (int i = 0; i < n; ++i) {
    const int* w = where + 4 * (size_t)i;
    if (w[0] < 1 || w[0] > n_cells || w[1] < 1 || w[1] > n_theta_rt || w[2] < 1 || w[2] > n_az_rt) return 1;
    for (int q = 0; q < nRT; ++q) {
      it[q] = itheta[(size_t)i * nRT + q]; cw[q] = cosw[(size_t)i * nRT + q]; sw[q] = sinw[(size_t)i * nRT + q];
      if (it[q] < 0 || it[q] > nang) return 2;
    }
    RtDeposit D;
    D.on = true; D.icell = w[0]; D.psup = w[1]; D.phik = w[2]; D.l = l[i];
    if (pola) deposit_rt1_wave<true>(M, A, R, mu, D, S + 4 * (size_t)i, w[3] != 0, nullptr, nullptr, nullptr);
    else deposit_rt1_wave<false>(M, A, R, mu, D, S + 4 * (size_t)i, w[3] != 0, nullptr, nullptr, nullptr);
  }
  return 0;
}
