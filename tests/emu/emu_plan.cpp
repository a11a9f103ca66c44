// emu_plan.cpp -- TEST INFRASTRUCTURE: the region plans of the deposit logs (k_plan_uniform / k_plan_bins,
// mcfost_amd/csrc/mc_binned.hip.h) run by one emulated lane on counts the test chooses.
// Built only by tests/test_bin_plan.py; nothing in mcfost_amd/ references it.
#include "emu_kernel.cpp"

extern "C" void emu_plan_uniform(unsigned int* off, unsigned int* cap, int n_buckets, unsigned long long total_blocks, int n_parts) {
  gridDim.x = 1; blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  k_plan_uniform(off, cap, n_buckets, total_blocks, n_parts);
}

// count [n_buckets][n_parts] (in: the last launch's block counts; out: cleared), want [n_buckets] (out: the plan's scratch)
extern "C" void emu_plan_bins(unsigned int* count, int n_buckets, int n_parts, unsigned int* off, unsigned int* cap,
                              unsigned long long total_blocks, double growth, int n_parts_next, double* want) {
  gridDim.x = 1; blockDim.x = 1; threadIdx.x = 0; blockIdx.x = 0;
  BinLog L{};
  L.count = count; L.n_buckets = n_buckets; L.n_parts = n_parts;
  k_plan_bins(L, off, cap, total_blocks, growth, n_parts_next, want);
}
