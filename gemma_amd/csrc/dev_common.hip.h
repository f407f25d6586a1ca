// Device helpers shared by the kernels of more than one unit.
#pragma once

#include <hip/hip_runtime.h>

namespace gemma_hip {

// the sum of v over the 64 lanes of a wavefront, in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

} // namespace gemma_hip
