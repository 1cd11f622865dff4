// block_scan.h — the workgroup prefix sum of the stream compactions
// (reg2aln.hip: the CIGAR jobs; samtext.hip: the SAM text's offsets).
// Internal; included by the .hip translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bwagpu {

// exclusive prefix of v over the workgroup's 256 threads; *total = the workgroup's sum
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* total) {
  __shared__ T wsum[4];
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  T incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  __syncthreads();  // wsum of an earlier call has been read
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  T before = 0, all = 0;
  for (int x = 0; x < 4; ++x) {
    before += x < w ? wsum[x] : 0;
    all += wsum[x];
  }
  *total = all;
  return before + incl - v;
}

}  // namespace bwagpu
