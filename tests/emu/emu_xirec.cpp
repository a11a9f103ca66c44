// emu_xirec.cpp -- TEST INFRASTRUCTURE: the record log of the SED commit pass (mcfost_amd/csrc/mc_xirec.hip.h) compiled for
// the host: the placement function next to xi32_offset, and k_fold_xirec run workgroup by workgroup by one emulated lane.
// Built only by tests/test_xi_record_fold.py; nothing in mcfost_amd/ references it.
#define MCGPU_LANE_EMULATION 1
#include <stddef.h>
#include <stdint.h>

#define __device__
#define __host__
#define __global__
#define __launch_bounds__(...)
struct emu_dim3 { unsigned int x, y, z; };
static emu_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1};
static inline void __syncthreads() {}
static inline float atomicAdd(float* p, float v) { float o = *p; *p += v; return o; }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { unsigned long long o = *p; *p += v; return o; }

#include "../../mcfost_amd/csrc/mc_xirec.hip.h"

using namespace mcgpu;

extern "C" {

int xirec_probe_values(int nRT, int pola, int contrib) { return xirec_values(nRT, pola != 0, contrib != 0); }
int xirec_probe_applies(int nRT, int pola, int contrib) { return xirec_applies(nRT, pola != 0, contrib != 0) ? 1 : 0; }
int xirec_probe_slots(int nRT, int pola, int contrib) { return xirec_slots(xi32_layout(nRT, pola != 0, contrib != 0), nRT); }
int xirec_probe_binf(int nRT, int pola, int contrib) { return xi32_layout(nRT, pola != 0, contrib != 0).binf; }
// place of value q of a stellar / thermal record; and of flux type `type` (0-based) of observer q (xi32_offset)
int xirec_probe_offset(int nRT, int pola, int contrib, int flag_star, int q) {
  return xirec_offset(xi32_layout(nRT, pola != 0, contrib != 0), nRT, flag_star != 0, q);
}
int xirec_probe_xi32_offset(int nRT, int pola, int contrib, int q, int type) {
  return xi32_offset(xi32_layout(nRT, pola != 0, contrib != 0), q, type, pola ? 4 : 1);
}

// k_fold_xirec over the whole grid: recs [blocks][64] of 16 bytes, count [n_buckets][n_parts], off / cap [n_buckets];
// xI [n_sub][binf] += the log; stats[2] += the records summed.  Returns 1 where a slice exceeds the emulated LDS.
int emu_fold_xirec(void* recs, unsigned int* count, const unsigned int* off, const unsigned int* cap, int n_buckets, int shift,
                   int n_parts, float* xI, int nRT, int contrib, unsigned int n_sub, int slice_sub, int split,
                   unsigned long long* stats) {
  const Xi32Lay xi = xi32_layout(nRT, false, contrib != 0);
  if ((size_t)slice_sub * xirec_slots(xi, nRT) > sizeof(xirec_fold_slice) / sizeof(float)) return 1;
  XiRecLog L{};
  L.vals = reinterpret_cast<XiRec*>(recs); L.count = count; L.off = off; L.cap = cap; L.stats = stats;
  L.n_buckets = n_buckets; L.shift = shift; L.n_parts = n_parts;
  blockDim.x = 1; threadIdx.x = 0;
  for (int b = 0; b < n_buckets * split; ++b) { blockIdx.x = (unsigned int)b; k_fold_xirec(L, xI, xi, nRT, n_sub, slice_sub, split); }
  blockIdx.x = 0;
  return 0;
}
}
