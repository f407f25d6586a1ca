// What the host side of i8gemm_dense16.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in i8gemm_dense16.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "i8gemm.h"

namespace gemma_hip {

template <bool RAW>
__global__ __launch_bounds__(512, 2) void i8gemm_dense16_kernel_t(I8PackArgs g);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define I8GEMM_DENSE16_INSTANCES(T) \
  T void i8gemm_dense16_kernel_t<true>(I8PackArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
I8GEMM_DENSE16_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip
