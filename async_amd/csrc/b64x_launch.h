// b64x_launch.h -- internal: what the host-only sessions unit
// (b64x_sessions.cpp) calls in the kernel unit (b64x_kernels.hip), where
// all of it is defined next to the kernels it launches.  Host functions with
// hidden visibility: none of them is part of the library's ABI.  Every one
// returns the ABI's status (0 or a negative errno) unless it says otherwise.
#ifndef ASYNC_AMD_B64X_LAUNCH_H
#define ASYNC_AMD_B64X_LAUNCH_H

#include <hip/hip_runtime_api.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"

namespace b64x_launch __attribute__((visibility("hidden"))) {

static inline int hip_err(hipError_t e)
{
    if (e == hipSuccess) return 0;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    return -EIO;
}

// Sequence numbers of decode calls and batches: nonzero, process-wide.
uint32_t next_seq();

// b64x_decode_dev, plus an optional host mirror of the result record that
// the kernels write themselves (sessions; see write_result).
int decode_dev_impl(const void *d_in, uint64_t nchars, void *d_out, b64x_dec_result *d_res,
                    b64x_dec_result *h_res, const b64x_alphabet *abc, unsigned flags,
                    void *d_workspace, void *stream, uint32_t seq);

// A lane's batch decode of njobs jobs at src + d_in_off[j] into
// h_out + d_out_off[j]: the batch kernels (each job's alphabet count in
// d_vcount[j]), then k_batch_finish, which writes the records h_res[j] with
// `seq`.  Both skip the jobs of `big` characters or more and the chained
// ones (d_flags[j] & B64X_LANE_CHAINED).
int lane_batch_decode(const uint8_t *src, const uint64_t *d_in_off, const uint64_t *d_out_off,
                      const uint8_t *d_flags, uint32_t njobs, uint64_t big, uint8_t *h_out,
                      uint64_t *d_vcount, b64x_dec_result *h_res, const b64x_alphabet *abc,
                      hipStream_t stream, uint32_t seq);

// k_spell_head: a chained job's head from its predecessor's record.
int spell_head(uint8_t *d_head, const b64x_dec_result *h_prev, b64x_dec_result *h_log,
               const b64x_alphabet *abc, hipStream_t stream);

// k_stamp: v into *h_stamp, behind everything queued on the stream.
int stamp(uint64_t *h_stamp, uint64_t v, hipStream_t stream);

// k_gather_host: `total` (> 0) bytes of a batch with lent segments into d_in.
int gather_host(uint8_t *d_in, const uint8_t *h_in, uint64_t total, const b64x_seg *d_seg,
                uint32_t nseg, hipStream_t stream);

}  // namespace b64x_launch

#endif  // ASYNC_AMD_B64X_LAUNCH_H
