// What the host side of i8gemm_sparse2_r16.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in i8gemm_sparse2_r16.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "i8gemm_sparse2.h"

// LDS stages of the K pipeline (S2_STAGE = 32 KiB each): LDS-DMA runs S2_R16_NST - 1 K-tiles ahead.  4 = rounds 3-5; 5 fills the
// CU's 160 KiB exactly: 128 instead of 96 KiB of operands in flight per CU.  Round 6: the loop's data side is bound by
// (bytes in flight) / (latency of an L2 miss served across the fabric) -- profiles/r06_power_table.txt: with the dense matrix
// instructions compiled out the same loop still takes 29 ms for its 382 GB of LDS-DMA = 53 GB/s per CU = 96 KiB per ~1.8 us.
#ifndef S2_R16_NST
#define S2_R16_NST 4
#endif

namespace gemma_hip {

constexpr int S2_R16_LDS = S2_R16_NST * S2_STAGE; // dynamic LDS of a launch
static_assert(S2_R16_LDS >= 16 * 512 * 16, "the epilogue parks 16 x 16 bytes per lane of the mask accumulators in the launch's LDS");

__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_kernel(Sparse2Args g);

__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_g_kernel(Sparse2Args g);

__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_ep_kernel(Sparse2Args g);

__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_ep_g_kernel(Sparse2Args g);

} // namespace gemma_hip
