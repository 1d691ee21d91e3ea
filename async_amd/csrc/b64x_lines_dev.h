// What the device side of the line-wrapped encode and the strict decode
// shares (b64x_wrap_body.h, b64x_strict_body.h and the translation units that
// include them): the plan header's structs under their short names, the
// vector types of the wide loads and stores, the block barrier and the
// launch status.  One definition each for a unit that includes both bodies.
#ifndef ASYNC_AMD_B64X_LINES_DEV_H
#define ASYNC_AMD_B64X_LINES_DEV_H

#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x_lines_plan.h"

#define DEV __device__ __forceinline__
#define HD __host__ __device__ __forceinline__

namespace {

using lines_plan::Alpha;
using lines_plan::StrictArgs;
using lines_plan::WrapArgs;

// dword vectors at dword (not 8- or 16-byte) alignment
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));

// __syncthreads() with every LDS access of this wave done first (the form of
// b64x_kernels.hip: the hardware barrier does not wait for LDS writes).
DEV void block_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// The last launch (or runtime call) as the ABI's status.
inline int hip_status()
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    return -EIO;
}

}  // namespace

#endif  // ASYNC_AMD_B64X_LINES_DEV_H
