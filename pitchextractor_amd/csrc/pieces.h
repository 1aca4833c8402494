// What the kernels that cut a row into pieces share (noise.hip, stimuli.hip; rir_synth.hip's decay kernel takes the
// reductions alone).
// The piece geometry: a workgroup of kThreads owns kPiece consecutive samples of one row, counted from the row's own
// first sample, a thread kRun consecutive ones of them.  The reductions and the scan of one double per thread over
// that workgroup, in a fixed order.  The mix at a signal-to-noise ratio that stands on these is snr_mix.h.
#pragma once
#include <math.h>
#include "dsp.h"

namespace pe {

constexpr int kThreads = 256;
constexpr int kRun = 8;                          // consecutive samples of one thread
constexpr int kPiece = kRun * kThreads;          // scan / reduction piece S = 2048 samples

// One double per thread over a workgroup of kThreads in a fixed order (the sum and the max: a tree; the scan:
// Hillis-Steele); every thread gets the result.  s_sum: kThreads doubles.  The barrier behind the last read lets a
// loop call these back to back, and the caller use s_sum afterwards, without a barrier of its own; a caller that
// has touched s_sum itself meets a barrier before the call (rir_decay_kernel does).
template <class Op>
__device__ __forceinline__ double block_tree_d(double v, double* s_sum, int tid, Op op) {
#pragma clang fp contract(off)
  s_sum[tid] = v;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if (tid < st) s_sum[tid] = op(s_sum[tid], s_sum[tid + st]);
    __syncthreads();
  }
  const double out = s_sum[0];
  __syncthreads();
  return out;
}

__device__ __forceinline__ double block_sum_d(double v, double* s_sum, int tid) {
  return block_tree_d(v, s_sum, tid, [](double a, double b) { return a + b; });
}

__device__ __forceinline__ double block_max_d(double v, double* s_sum, int tid) {
  return block_tree_d(v, s_sum, tid, [](double a, double b) { return fmax(a, b); });
}

// returns the sum of the threads before `tid`, and the sum of all in `total`
__device__ __forceinline__ double block_scan(double v, double* s_sum, int tid, double& total) {
#pragma clang fp contract(off)
  s_sum[tid] = v;
  __syncthreads();
  for (int st = 1; st < kThreads; st <<= 1) {
    const double add = tid >= st ? s_sum[tid - st] : 0.0;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  const double before = tid > 0 ? s_sum[tid - 1] : 0.0;
  total = s_sum[kThreads - 1];
  __syncthreads();
  return before;
}

}  // namespace pe
