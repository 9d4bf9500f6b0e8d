// Reductions over one workgroup of 256 threads (4 waves of 64), shared by track.hip, capture.hip,
// live.hip, gallery.hip, evaluate.hip, embed_misc.hip and rollcall.hip.
//
// The contract of every block_* function here, for all 256 threads of the block calling it:
//   - a barrier comes before the write of `red` (4 elements of LDS), so LDS written before the
//     call is visible after it, and `red` may be reused by the next call;
//   - every thread returns the same value;
//   - the value is a fixed function of the 256 inputs: a shuffle tree inside each wave
//     (offsets 32, 16, ..., 1), then the four wave partials r0..r3 in the order each function
//     states.  The kernels' bit-reproducibility rests on these orders: do not unify them.
// The block_* functions write the wave tree out rather than call wave_sum: with the call inlined
// the compiler schedules the wave-index shift on the other side of the barrier, and the kernels'
// instruction streams were to stay as they were when these functions moved here.
// (align.hip's block_sum_i64 puts its barrier after the write, which is another contract, and
// embed_misc.hip's block_sum_1024 is a 16-wave block.)
#pragma once
#include <hip/hip_runtime.h>

namespace frhip {

// Sum over the 64 lanes of a wave, in every lane.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sum of int or float: (r0 + r1) + (r2 + r3).
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  static_assert(sizeof(T) == 4, "int or float; doubles take block_sum_double's order");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Maximum of int.
__device__ __forceinline__ int block_max(int v, int* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

// Maximum of unsigned 64-bit keys (rollcall.hip: a score's ordered image over a face index).
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
  return a > b ? a : b;
}

// Sum of double, the wave partials in sequence: ((r0 + r1) + r2) + r3.
__device__ __forceinline__ double block_sum_double(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace frhip
