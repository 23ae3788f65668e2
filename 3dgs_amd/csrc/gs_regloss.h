// gs_regloss.h -- what the image-space regularisers share (gs_loss.hip: distortion, depth prior; gs_normal.hip: the normal
// map's two losses): a gradient is rounded to float once and stored or added (put_grad), the loss is summed in double, per
// block into `partial` (block_partial) and by reg_loss_finish_kernel in a fixed order -- the same bits in every run.
#pragma once
#include <algorithm>

#include "gs_common.h"

namespace gs {

constexpr int kRegBlocks = 256;  // blocks of a grid-stride regulariser = doubles of its SCR_DEPTH_LOSS scratch

// blocks of 256 threads for n pixels
static inline int reg_blocks(long long n) { return (int)std::min<long long>(kRegBlocks, (n + 255) / 256); }

#ifdef __HIPCC__
// the sum over a 256-thread block (tid = the thread's linear index) of v -> partial[block]
__device__ __forceinline__ void block_partial_at(double v, double *__restrict__ partial, int tid, int block) {
  __shared__ double s_wave[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63) == 0) s_wave[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) partial[block] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

__device__ __forceinline__ void block_partial(double v, double *__restrict__ partial) {
  block_partial_at(v, partial, (int)threadIdx.x, (int)blockIdx.x);
}

template <bool kAdd>
__device__ __forceinline__ void put_grad(float *__restrict__ g, long long i, double v) {
  if (!g) return;
  if constexpr (kAdd) g[i] += (float)v;
  else g[i] = (float)v;
}

// one wave: the blocks' partial sums in a fixed order, x scale, as the one float of the loss
static __global__ __launch_bounds__(64) void reg_loss_finish_kernel(const double *__restrict__ partial, int n, double scale,
                                                                    float *__restrict__ loss_out) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) v += partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (threadIdx.x == 0) *loss_out = (float)(scale * v);
}
#endif

}  // namespace gs
