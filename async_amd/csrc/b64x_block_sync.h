// The block barrier of the line-wrapped encode and the strict decode
// (b64x_wrap_body.h, b64x_strict_body.h and the translation units that include
// them): one definition for a unit that includes both.
#ifndef ASYNC_AMD_B64X_BLOCK_SYNC_H
#define ASYNC_AMD_B64X_BLOCK_SYNC_H

#include <hip/hip_runtime.h>

namespace {

// __syncthreads() with every LDS access of this wave done first (the form of
// b64x_kernels.hip: the hardware barrier does not wait for LDS writes).
__device__ __forceinline__ void block_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

}  // namespace

#endif  // ASYNC_AMD_B64X_BLOCK_SYNC_H
