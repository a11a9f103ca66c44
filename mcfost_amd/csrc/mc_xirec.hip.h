// The SED commit pass's deposits as 16-byte RECORDS in a binned log (option "xi_log" = 3): the path for runs with few
// observers, where a crossing's deposit is at most three default reals of one origin (calc_xI_scatt,
// dust_ray_tracing.f90:480-529: xI_scatt += l * Stokes(1) * s11(it_q) for every observer q).
//
// The sorted log (mc_xilog.hip.h) names a FLIGHT in its record and gathers that flight's weight row in the fold; with
// short flights the gather and the sort cost more than the atomics they replace.  Here the record IS the deposit:
//   XiRec = {key = sub-bin index | flag_star << 31, v[q] = l * w[q]}     (w: the flight's deposit weights, kept by the lane)
// and it takes the thermal step's road (mc_binned.hip.h, instantiated for this value type): staged per address-range
// bucket in LDS (bucket = sub-bin >> shift, two half-buffers of 64 records = 2 KB per bucket), written by the wave that
// completes a half as one contiguous 1 KB block of the workgroup's own part of the bucket's region, and summed by the
// bucket's owners in LDS (k_fold_xirec).  No sort, no row gather, no per-crossing atomics.
//
// Where it applies: V <= 3 values per deposit -- V = nRT * n_Stokes default reals of one crossing in the packed layout
// (with lsepar_contrib a packet reaches nRT * (nA + 1) values, nA = n_Stokes - 1: the same number) --, i.e. one to three
// observers without Stokes tracking, with or without contributions.
#pragma once
#include "mc_xi32.hip.h"
// (the lane emulation has no default-real commit pass: it compiles the placement and the fold, and -- where a test asks
// for it, tests/emu/emu_xirec_stage.cpp -- the staging's instantiation for this record with one emulated lane)
#if !defined(MCGPU_LANE_EMULATION) || defined(MCGPU_XIREC_EMULATE_STAGING)
#define MCGPU_XIREC_STAGING 1
#include "mc_binned.hip.h"
#endif

namespace mcgpu {

constexpr int XIREC_MAX_V = 3;
constexpr int XIREC_H = 64;   // records per block (= BIN_H, mc_binned.hip.h)
#ifdef MCGPU_LANE_EMULATION
constexpr int XIREC_WAVE = 1;
#else
constexpr int XIREC_WAVE = 64;
#endif

struct alignas(16) XiRec {
  unsigned int key;        // ((icell-1) n_theta_rt + psup-1) n_az_rt + phik-1, bit 31: flag_star
  float v[XIREC_MAX_V];    // value q of the deposit (q >= V: 0)
};

// default reals one packet's crossing adds to a sub-bin in the packed layout
__host__ __device__ inline int xirec_values(int nRT, bool pola, bool contrib) {
  const Xi32Lay L = xi32_layout(nRT, pola, contrib);
  return contrib ? nRT * (L.nA + 1) : nRT * L.nA;
}
__host__ __device__ inline bool xirec_applies(int nRT, bool pola, bool contrib) { return xirec_values(nRT, pola, contrib) <= XIREC_MAX_V; }

// THE placement: where value q of a stellar / thermal record goes inside its sub-bin (the fold's write-out, the overflow
// path and the end-of-launch drain all ask here).  With V <= 3 there is no Stokes tracking: value q is observer q's flux,
// which goes to the place of I -- or, where I is not stored (lsepar_contrib), to the place of the packet's origin.
__host__ __device__ inline int xirec_offset(const Xi32Lay& L, int nRT, bool flag_star, int q) {
  (void)nRT;
  if (L.oS < 0) return q * L.sA;
  return flag_star ? L.oS + q * L.sS : L.oT + q * L.sT;
}
// the fold's accumulators per sub-bin: both origins where contributions are kept, [star x nRT | thermal x nRT]
__host__ __device__ inline int xirec_slots(const Xi32Lay& L, int nRT) { return L.oS < 0 ? nRT : 2 * nRT; }

// HBM side of the log (the fields mc_binned.hip.h's staging reads are named as BinLog names them)
struct XiRecLog {
  XiRec* vals;                 // [blocks][64]
  unsigned int* keys;          // (none: the record carries its key)
  unsigned int* count;         // [n_buckets][n_parts] blocks workgroup `part` wanted to write in the last launch
  const unsigned int* off;     // [n_buckets] first block of the bucket's region
  const unsigned int* cap;     // [n_buckets] blocks of ONE workgroup's part of the region (n_parts of them in a row)
  unsigned long long* stats;   // [0] blocks that overflowed their part, [1] records added at the end of a launch,
                               // [2] records the fold summed, [3] records the transport kernel made
  int n_buckets, shift;        // bucket = sub-bin >> shift
  int n_parts;                 // workgroups of the transport kernel
};

// Fold.  Workgroup (bucket b = blockIdx.x / split, s = blockIdx.x % split) owns the sub-bins
// [(b << shift) + s * slice_sub, ... + slice_sub) of the bucket: it reads ALL blocks of the bucket's region, sums the
// records of its own sub-bins into xirec_slots default reals per sub-bin in LDS (ds_add_f32) and skips the others, then
// adds the non-zero accumulators to xI_scatt once.  The region is read `split` times: 16 bytes x split per record.
#ifdef MCGPU_LANE_EMULATION
float xirec_fold_slice[1 << 16];
#endif
static __global__ void __launch_bounds__(1024) k_fold_xirec(const XiRecLog L, float* xI, const Xi32Lay xi, int nRT, unsigned int n_sub,
                                                            int slice_sub, int split) {
#ifdef MCGPU_LANE_EMULATION
  float* const slice = xirec_fold_slice;
#else
  extern __shared__ float xirec_slice_lds[];
  float* const slice = xirec_slice_lds;
#endif
  const int b = blockIdx.x / split, s = blockIdx.x % split;
  const int slots = xirec_slots(xi, nRT);
  const unsigned int b_end = ((unsigned int)b + 1u) << L.shift;
  const unsigned int lo = ((unsigned int)b << L.shift) + (unsigned int)s * (unsigned int)slice_sub;
  unsigned int hi = lo + (unsigned int)slice_sub;
  if (hi > b_end) hi = b_end;
  if (hi > n_sub) hi = n_sub;
  if (lo >= hi) return;
  const int n_acc = (int)(hi - lo) * slots;
  for (int i = threadIdx.x; i < n_acc; i += blockDim.x) slice[i] = 0.0f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_waves = blockDim.x >= 64 ? (int)(blockDim.x >> 6) : 1;
  const unsigned int cap = L.cap[b];
  const size_t first = (size_t)L.off[b];
  const int thermal_at = xi.oS < 0 ? 0 : nRT;
  unsigned long long mine = 0ull;
  for (int part = 0; part < L.n_parts; ++part) {
    const unsigned int cnt = L.count[(size_t)b * L.n_parts + part];
    const unsigned int n_blk = cnt < cap ? cnt : cap;
    const size_t p0 = first + (size_t)cap * part;
    for (unsigned int blk = (unsigned int)wave; blk < n_blk; blk += (unsigned int)n_waves) {
      for (int l = lane; l < XIREC_H; l += XIREC_WAVE) {
        const XiRec r = L.vals[(p0 + blk) * XIREC_H + l];
        const unsigned int sub = r.key & 0x7FFFFFFFu;
        if (sub < lo || sub >= hi) continue;
        float* acc = slice + (size_t)(sub - lo) * slots + ((r.key >> 31) ? 0 : thermal_at);
        atomicAdd(acc, r.v[0]);
        if (nRT > 1) atomicAdd(acc + 1, r.v[1]);
        if (nRT > 2) atomicAdd(acc + 2, r.v[2]);
        ++mine;
      }
    }
  }
  if (mine) atomicAdd(&L.stats[2], mine);
  __syncthreads();
  for (int i = threadIdx.x; i < n_acc; i += blockDim.x) {
    const float a = slice[i];
    if (a == 0.0f) continue;
    const int sb = i / slots, sl = i - sb * slots;
    const bool star = xi.oS < 0 || sl < nRT;
    const int q = sl < nRT ? sl : sl - nRT;
    atomicAdd(xI + (size_t)(lo + (unsigned int)sb) * xi.binf + xirec_offset(xi, nRT, star, q), a);
  }
}

#ifdef MCGPU_XIREC_STAGING
static_assert(XIREC_H == BIN_H && XIREC_WAVE == BIN_WAVE, "the log's blocks are the staging's half-buffers");
template <> struct BinKeyed<XiRec> { static constexpr bool value = true; };

// Where a record goes that the log does not take -- a block whose part of the log is full, what is left in the
// half-buffers at the end of a launch, the spin's safety valve (mc_binned.hip.h): xI_scatt, with default-real atomics.
struct XiRecSink {
  float* xI;
  Xi32Lay xi;
  int nRT;
  unsigned int n_sub;   // sub-bins of xI_scatt: a key beyond them is dropped, never written
};
__device__ inline void bin_sink_add(const XiRecSink& K, unsigned int, const XiRec& r) {
  if ((r.key & 0x7FFFFFFFu) >= K.n_sub) return;   // (never: a logic error must not write outside the array)
  float* const bin = K.xI + (size_t)(r.key & 0x7FFFFFFFu) * K.xi.binf;
  const bool star = (r.key >> 31) != 0u;
  atomicAdd(bin + xirec_offset(K.xi, K.nRT, star, 0), r.v[0]);
  if (K.nRT > 1) atomicAdd(bin + xirec_offset(K.xi, K.nRT, star, 1), r.v[1]);
  if (K.nRT > 2) atomicAdd(bin + xirec_offset(K.xi, K.nRT, star, 2), r.v[2]);
}
#endif

}  // namespace mcgpu
