// emu_xirec_stage.cpp -- TEST INFRASTRUCTURE: the staging protocol of mcfost_amd/csrc/mc_binned.hip.h instantiated for the
// SED commit pass's 16-byte record (mc_xirec.hip.h) and run by one emulated lane: every workgroup deposits its records
// through bin_deposit / bin_settle / bin_drain into regions planned by k_plan_uniform, k_fold_xirec sums the log.
// Built only by tests/test_xi_record_fold.py; nothing in mcfost_amd/ references it.
#define MCGPU_XIREC_EMULATE_STAGING 1
#include "emu_kernel.cpp"

// keys [n] (sub-bin | flag_star << 31), vals [n][3], part [n] (the workgroup that makes the record); xI [n_sub][binf] +=
// everything; stats[0..3] as XiRecLog names them (stats[3]: the records deposited).  1: a size does not fit the emulation.
extern "C" int emu_xirec_stage_and_fold(int n, const unsigned int* keys, const float* vals, const int* part, int n_parts, int n_buckets,
                                        int shift, unsigned long long total_blocks, float* xI, int nRT, int contrib, unsigned int n_sub,
                                        int slice_sub, int split, unsigned long long* stats) {
  const Xi32Lay xi = xi32_layout(nRT, false, contrib != 0);
  if ((size_t)slice_sub * xirec_slots(xi, nRT) > sizeof(xirec_fold_slice) / sizeof(float)) return 1;
  std::vector<XiRec> log((size_t)total_blocks * XIREC_H);
  std::vector<unsigned int> count((size_t)n_buckets * n_parts, 0u), off(n_buckets), cap(n_buckets);
  gridDim.x = 1; blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  k_plan_uniform(off.data(), cap.data(), n_buckets, total_blocks, n_parts);
  XiRecLog L{};
  L.vals = log.data(); L.count = count.data(); L.off = off.data(); L.cap = cap.data(); L.stats = stats;
  L.n_buckets = n_buckets; L.shift = shift; L.n_parts = n_parts;
  const XiRecSink K = {xI, xi, nRT, n_sub};
  std::vector<double> lds((bin_lds_bytes_of<XiRec>(n_buckets) + 31) / 8);
  char* base = reinterpret_cast<char*>(lds.data());
  base += (16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15;
  for (int p = 0; p < n_parts; ++p) {
    blockIdx.x = (unsigned int)p;
    const BinStageT<XiRec> S = bin_carve_of<XiRec>(base, n_buckets);
    bin_init(S, n_buckets);
    BinLane P;
    bin_lane_init(P);
    for (int i = 0; i < n; ++i) {
      if (part[i] != p) continue;
      XiRec r;
      r.key = keys[i]; r.v[0] = vals[3 * i]; r.v[1] = vals[3 * i + 1]; r.v[2] = vals[3 * i + 2];
      bin_deposit<XiRec>(S, L, K, 0, P, true, (int)(keys[i] & 0x7FFFFFFFu), r);
      stats[3]++;
    }
    bin_settle(S, L, K, 0, P);
    bin_drain(S, L, K);
  }
  for (int b = 0; b < n_buckets * split; ++b) { blockIdx.x = (unsigned int)b; k_fold_xirec(L, xI, xi, nRT, n_sub, slice_sub, split); }
  blockIdx.x = 0;
  return 0;
}
