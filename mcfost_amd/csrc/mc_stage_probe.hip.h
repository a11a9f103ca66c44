// Unit probe of the deposit logs' staging (mcgpu_probe_bin_stage, mcgpu.hip): the LDS protocol of mc_binned.hip.h run by
// whole workgroups on records the caller chooses, for both of its value types --
//   V = double, log BinLog,   sink double*     the thermal step's (cell, FP64) records, folded by k_fold_bins
//   V = XiRec,  log XiRecLog, sink XiRecSink   the SED commit pass's 16-byte records, folded by k_fold_xirec
// -- so that a test can put every lane of eight waves into one bucket, leave a wave one active lane, starve the log or
// end a launch on a half-full half-buffer, and compare the sums with integer-valued inputs bit for bit.  The kernel calls
// the library's own bin_carve_of / bin_init / bin_lane_init / bin_deposit / bin_settle / bin_drain under the contract
// mono_body keeps: every lane calls bin_deposit in converged flow, bin_settle follows the loop, then __syncthreads(),
// then bin_drain.
#pragma once
#include "mc_binned.hip.h"
#include "mc_xirec.hip.h"

namespace mcgpu {

constexpr unsigned int STAGE_PROBE_NONE = 0xFFFFFFFFu;   // the key of "no record": the lane is inactive in that round

// record i as the caller gave it: the value of a (cell, double) record, or the 16-byte record with its key
__device__ inline double stage_probe_record(const double* vals, unsigned long long i, unsigned int, double*) { return vals[i]; }
__device__ inline XiRec stage_probe_record(const float* vals, unsigned long long i, unsigned int key, XiRec*) {
  XiRec r;
  r.key = key; r.v[0] = vals[3 * i]; r.v[1] = vals[3 * i + 1]; r.v[2] = vals[3 * i + 2];
  return r;
}

// what a region of the log holds before the first launch: never read, whatever the counts say
__device__ inline void stage_probe_stale(const BinLog& L, size_t i) { L.keys[i] = 0x7FFFFFFFu; L.vals[i] = 1e30; }
__device__ inline void stage_probe_stale(const XiRecLog& L, size_t i) {
  XiRec r;
  r.key = 0x7FFFFFFFu; r.v[0] = r.v[1] = r.v[2] = 1e30f;
  L.vals[i] = r;
}
template <typename LOG>
__global__ void __launch_bounds__(256) k_probe_stage_fill(const LOG L, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) stage_probe_stale(L, i);
}

// Round r of the launch: global thread g handles record first + r * T + g (T = threads of the launch).  stats[3] += the
// records made (as mono_body counts them).
template <typename V, typename LOG, typename SINK, typename IN>
__global__ void __launch_bounds__(768) k_probe_bin_stage(const LOG L, const SINK E, const unsigned int* __restrict__ keys,
                                                        const IN* __restrict__ vals, unsigned long long first, int n_rounds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stage_probe_lds[];
  const BinStageT<V> S = bin_carve_of<V>(stage_probe_lds, L.n_buckets);
  bin_init(S, L.n_buckets);
  __syncthreads();
  BinLane P;
  bin_lane_init(P);
  const int lane = threadIdx.x & 63;
  const unsigned long long T = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long made = 0ull;
  for (int r = 0; r < n_rounds; ++r) {
    const unsigned long long i = first + (unsigned long long)r * T + g;
    const unsigned int key = keys[i];
    const bool active = key != STAGE_PROBE_NONE;
    const V v = stage_probe_record(vals, i, key, (V*)nullptr);
    if (active) made++;
    bin_deposit<V>(S, L, E, lane, P, active, (int)(key & 0x7FFFFFFFu), v);
  }
  bin_settle(S, L, E, lane, P);
  __syncthreads();
  bin_drain(S, L, E);
  for (int off = 32; off > 0; off >>= 1) made += __shfl_down(made, off);
  if (lane == 0 && made) atomicAdd(&L.stats[3], made);
}

}  // namespace mcgpu
