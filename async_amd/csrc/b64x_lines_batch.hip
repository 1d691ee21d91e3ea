// Ragged batches of the line-wrapped encode and the strict decode for gfx950
// (include/b64x.h, b64x_encode_lines_batch / b64x_decode_strict_batch): nbuf
// buffers of unequal lengths addressed by device-resident offsets, each
// wrapped or strictly decoded on its own.  A translation unit and a code
// object of its own, linked after b64x_kernels.o, b64x_wrap.o and
// b64x_strict.o; the per-lane bodies are those of the one-buffer kernels
// (b64x_wrap_body.h, b64x_strict_body.h), one copy.
//
// Layout ("k_encode_lines_batch / k_decode_strict_batch").  The
// work unit is a wave.  A persistent grid of 256-lane blocks is sized from
// nbuf and the device; wave g of G walks buffers g, g + G, ...  For each
// buffer the wave
//   1. reads the buffer's two offsets (scalar loads) and runs the prologue of
//      b64x_lines_plan.h on them, wave-uniform: length -> E, W, full lines,
//      the short last line, the hot count, off_e1 / off_e2, the LENGTH
//      verdict.  Lengths exist on the device only: the grid and every kernel
//      argument depend on nbuf, abc and fmt alone, so a captured call can be
//      replayed on other lengths;
//   2. walks the hot part in passes of 64 lanes (1,024 bytes of text out, or
//      1,024 characters in).  The pass's (line, column) is carried in scalar
//      registers from pass to pass -- additions, no division -- and a lane's
//      is one 32-bit multiply-high from there, as in the one-buffer kernels;
// A buffer that is not dword aligned on both sides, or any buffer of a call
// whose reciprocal is not exact (or L < 16), has no hot part: the wave takes
// the whole of it bytewise, 16 bytes or characters per lane.  That is a
// wave-uniform decision.
//   3. The tails of the aligned buffers (the last groups, the pads, a short
//      last line and its separator: at most four 16-byte elements) are not
//      walked buffer by buffer -- three lanes of a wave in a loop of dependent
//      loads, which cost more than the hot part of a 1 KiB buffer -- but
//      dense: a second pass takes the wave's buffers 16 at a time, a lane to
//      each of a buffer's four tail elements, the lane working out its
//      buffer's plan itself (the same prologue, per lane).  No hot wave
//      diverges into the bytewise code.
//
// Strict decode: a wave owns its buffers alone, so the lowest offence key of
// each lives in a record of the wave's own in LDS (16 of them: the buffers of
// one dense pass).  The bodies lower it with the same atomicMin as in the
// one-buffer kernels (an LDS atomic here, and none at all for good text);
// after the dense pass lanes 0..15 turn the keys into the finished records
// and write them whole.  No memset node, no global atomic, no record kernel.
//
// One wave walks one buffer: a buffer of hundreds of MiB is exact (64-bit
// positions throughout) but runs at one wave's rate; it belongs on the
// one-buffer calls.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "b64x.h"
#include "b64x_strict_body.h"
#include "b64x_wrap_body.h"

namespace {

using lines_plan::Call;
using lines_plan::kPassLanes;

constexpr uint32_t kBatchTH = 256;                      // kWrapTH == kStrictTH: the tables' builders
constexpr uint32_t kBatchWaves = kBatchTH / kPassLanes;  // work units per block
constexpr uint32_t kBlocksPerCU = 8;
// The dense tail pass: a lane to each of the first kTailPieces tail elements
// of kTailBufs buffers.
constexpr uint32_t kTailPieces = 4;
constexpr uint32_t kTailBufs = kPassLanes / kTailPieces;

static_assert(kBatchTH == kWrapTH && kBatchTH == kStrictTH, "the table builders' block size");

// Keep the compiler from moving LDS accesses across this point.  Within one
// wave the LDS executes DS instructions in issue order, so program order is
// all that the hand-off of the wave's record between its lanes needs.
DEV void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's index in the block, as the scalar it is.
DEV uint32_t wave_in_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x / kPassLanes); }

// ---------------------------------------------------------------- encode --

// The hot blocks of one buffer, a pass of 64 at a time.  (kt, ct): line and
// column of the pass's first byte.
template <typename IDX>
DEV void encode_hot(const uint8_t *tab, const uint4 *low16, const uint4 *sep16,
                    const uint8_t *rin, uint8_t *rout, uint32_t lane, const WrapArgs &w,
                    const Call &c)
{
    uint64_t kt = 0;
    uint32_t ct = 0;
    for (uint64_t j0 = 0; j0 < w.hot_blocks; j0 += kPassLanes) {
        const uint64_t j = j0 + lane;
        if (j < w.hot_blocks) {
            const uint32_t rel = ct + 16 * lane;
            const uint32_t dk = __umulhi(rel, c.magic);
            wrap_block<IDX>(tab, low16, sep16, rin, rout + 16 * j, (IDX) kt + dk,
                            rel - dk * c.P, w);
        }
        kt += c.step_k;
        ct += c.step_c;
        if (ct >= c.P) {
            ct -= c.P;
            kt++;
        }
    }
}

// One buffer's WrapArgs from its plan (what the bodies read of it).
DEV WrapArgs wrap_args(uint64_t len, const lines_plan::WrapPlan &p, const Call &c)
{
    WrapArgs w = {};
    w.len = len;
    w.E = p.E;
    w.W = p.W;
    w.full_lines = p.full_lines;
    w.hot_blocks = p.hot_blocks;
    w.L = c.L;
    w.P = c.P;
    w.s = c.s;
    w.sep = c.sep;
    w.last_len = p.last_len;
    return w;
}

__global__ __launch_bounds__(kBatchTH) void k_encode_lines_batch(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t nbuf,
    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, Call c, Alpha a)
{
    __shared__ uint8_t tab[64];
    __shared__ __attribute__((aligned(16))) uint8_t low16b[kLowRows * 16];
    __shared__ __attribute__((aligned(16))) uint8_t sep16b[kSepRows * 16];
    build_enc_table(tab, a);
    build_splice_tables(low16b, sep16b, c.sep, c.s);
    block_sync();
    const uint4 *low16 = (const uint4 *) low16b;
    const uint4 *sep16 = (const uint4 *) sep16b;
    const uint32_t lane = threadIdx.x % kPassLanes;
    const uint64_t waves = (uint64_t) gridDim.x * kBatchWaves;
    const uint64_t first = (uint64_t) blockIdx.x * kBatchWaves + wave_in_block();
    // Wave-uniform walk: the hot blocks of the aligned buffers; the others
    // bytewise as a whole.  The first kTailPieces tail pieces of an aligned
    // buffer are left to the dense pass below.
    for (uint64_t b = first; b < nbuf; b += waves) {
        const uint64_t beg = in_off[b], len = in_off[b + 1] - beg;
        if (len == 0) continue;
        const uint8_t *rin = in + beg;
        uint8_t *rout = out + out_off[b];
        const bool fast = c.fast && ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) == 0;
        const lines_plan::WrapPlan p = lines_plan::wrap_plan(len, c, fast);
        const WrapArgs w = wrap_args(len, p, c);
        if (p.hot_blocks) {
            if (p.W >> 32)
                encode_hot<uint64_t>(tab, low16, sep16, rin, rout, lane, w, c);
            else
                encode_hot<uint32_t>(tab, low16, sep16, rin, rout, lane, w, c);
        }
        for (uint64_t q0 = 16 * (p.hot_blocks + (fast ? kTailPieces : 0) + lane); q0 < p.W;
             q0 += 16 * kPassLanes) {
            const uint64_t left = p.W - q0;
            wrap_bytes(tab, rin, rout, q0, left >= 16 ? 16u : (uint32_t) left, w, a);
        }
    }
    // The tails of the aligned buffers, dense: the wave's buffers again, 16 to
    // a pass, a lane to each of a buffer's first kTailPieces tail pieces (an
    // aligned buffer has no more: at most 28 characters, three separators and
    // 15 bytes of a cut block), the lane working its buffer's plan out itself.
    for (uint64_t b0 = first; b0 < nbuf; b0 += waves * kTailBufs) {
        const uint64_t b = b0 + (lane / kTailPieces) * waves;
        if (b >= nbuf) continue;
        const uint64_t beg = in_off[b], len = in_off[b + 1] - beg;
        const uint8_t *rin = in + beg;
        uint8_t *rout = out + out_off[b];
        if (len == 0 || !c.fast || ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) != 0) continue;
        const lines_plan::WrapPlan p = lines_plan::wrap_plan(len, c, true);
        const uint64_t q0 = 16 * (p.hot_blocks + lane % kTailPieces);
        if (q0 >= p.W) continue;
        const uint64_t left = p.W - q0;
        wrap_bytes(tab, rin, rout, q0, left >= 16 ? 16u : (uint32_t) left, wrap_args(len, p, c), a);
    }
}

// ---------------------------------------------------------------- decode --

// The record of a text no encoder writes at this length, or of the empty text.
DEV void write_record(b64x_strict_result *dst, uint64_t out_len, uint64_t err_pos, uint32_t err)
{
    b64x_strict_result r;
    r.out_len = out_len;
    r.err_pos = err_pos;
    r.err = err;
    r.reserved = 0;
    *dst = r;
}

DEV StrictArgs strict_args(uint64_t W, const lines_plan::StrictPlan &p, const Call &c,
                           const Alpha &a)
{
    StrictArgs w = {};
    w.E = p.E;
    w.W = W;
    w.off_e1 = p.off_e1;
    w.off_e2 = p.off_e2;
    w.L = c.L;
    w.P = c.P;
    w.s = c.s;
    w.sep = c.sep;
    w.sep_mask = c.sep_mask;
    w.trailing = c.trailing;
    w.a = a;
    return w;
}

// A wave takes its buffers 16 at a time.  Each of the 16 has a record of the
// wave's own in LDS (err_pos: the lowest offence key; reserved: 1 = the final
// record is written already).  First the wave-uniform walk: the hot lanes of
// each aligned buffer, the whole of the others bytewise.  Then the tails of
// the aligned buffers, dense: a lane to each of a buffer's first kTailPieces
// tail lanes (it has no more: the characters from E - 4 - 15 on and what two
// windows can cost), the lane working its buffer's plan out itself.  Then
// lanes 0..15 turn the keys into records.
template <bool WRAP>
__global__ __launch_bounds__(kBatchTH) void k_decode_strict_batch(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t nbuf,
    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, b64x_strict_result *res,
    Call c, Alpha a)
{
    __shared__ uint8_t tab[256];
    __shared__ b64x_strict_result recs[kBatchWaves][kTailBufs];
    build_dec_table(tab, a);
    block_sync();
    const uint32_t lane = threadIdx.x % kPassLanes;
    const uint32_t wv = wave_in_block();
    const uint64_t waves = (uint64_t) gridDim.x * kBatchWaves;
    for (uint64_t b0 = (uint64_t) blockIdx.x * kBatchWaves + wv; b0 < nbuf;
         b0 += waves * kTailBufs) {
        for (uint32_t i = 0; i < kTailBufs; i++) {
            const uint64_t b = b0 + i * waves;
            if (b >= nbuf) break;
            b64x_strict_result *rec = &recs[wv][i];
            const uint64_t beg = in_off[b], W = in_off[b + 1] - beg;
            const uint8_t *rin = in + beg;
            uint8_t *rout = out + out_off[b];
            const bool fast = c.fast && ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) == 0;
            const lines_plan::StrictPlan p = lines_plan::strict_plan(W, c, fast);
            const bool done = W == 0 || p.length_error;
            if (lane == 0) {
                rec->out_len = 0;
                rec->err_pos = kNoKey;
                rec->reserved = done ? 1 : 0;
                if (done)
                    write_record(res + b, 0, W,
                                 p.length_error ? B64X_STRICT_LENGTH : B64X_STRICT_OK);
            }
            wave_lds_order();
            if (done) continue;
            const StrictArgs w = strict_args(W, p, c, a);
            // (kt, ct): line and column of the pass's first character
            uint64_t kt = 0;
            uint32_t ct = 0;
            for (uint64_t j0 = 0; j0 < p.hot_lanes; j0 += kPassLanes) {
                const uint64_t j = j0 + lane;
                if (j < p.hot_lanes) {
                    if (WRAP) {
                        const uint32_t rel = ct + kLaneChars * lane;
                        const uint32_t dk = mul_hi32(rel, c.magic);
                        const uint32_t col = rel - dk * c.L;
                        strict_lane<true>(tab, rin, rout + 12 * j, &rec->err_pos,
                                          (kt + dk) * c.P + col, col, w);
                    } else {
                        strict_lane<false>(tab, rin, rout + 12 * j, &rec->err_pos,
                                           kLaneChars * j, 0, w);
                    }
                }
                if (WRAP) {
                    kt += c.step_k;
                    ct += c.step_c;
                    if (ct >= c.L) {
                        ct -= c.L;
                        kt++;
                    }
                }
            }
            const uint64_t lanes = p.hot_lanes + p.tail_lanes;
            for (uint64_t jl = p.hot_lanes + (fast ? kTailPieces : 0) + lane; jl < lanes;
                 jl += kPassLanes)
                strict_bytes(tab, rin, rout, rec, jl, w);
        }
        wave_lds_order();
        {
            const uint32_t i = lane / kTailPieces;
            const uint64_t b = b0 + i * waves;
            if (b < nbuf && c.fast) {
                const uint64_t beg = in_off[b], W = in_off[b + 1] - beg;
                const uint8_t *rin = in + beg;
                uint8_t *rout = out + out_off[b];
                if (W != 0 && ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) == 0) {
                    const lines_plan::StrictPlan p = lines_plan::strict_plan(W, c, true);
                    if (!p.length_error && lane % kTailPieces < p.tail_lanes)
                        strict_bytes(tab, rin, rout, &recs[wv][i],
                                     p.hot_lanes + lane % kTailPieces, strict_args(W, p, c, a));
                }
            }
        }
        wave_lds_order();
        if (lane < kTailBufs) {
            const uint64_t b = b0 + lane * waves;
            if (b < nbuf) {
                b64x_strict_result r = recs[wv][lane];
                if (!r.reserved) {
                    finish_record(&r);
                    res[b] = r;
                }
            }
        }
        wave_lds_order();
    }
}

// ---------------------------------------------------------------- host --

// A persistent grid: a wave per buffer up to what the device holds at once.
int batch_grid(uint32_t nbuf, uint32_t *grid)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0) {
        const int rc = hip_status();
        return rc ? rc : -ENODEV;
    }
    const uint64_t want = ((uint64_t) nbuf + kBatchWaves - 1) / kBatchWaves;
    const uint64_t cap = (uint64_t) cus * kBlocksPerCU;
    *grid = (uint32_t) (want < cap ? want : cap);
    return 0;
}

}  // namespace

extern "C" {

int b64x_encode_lines_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                            void *d_out, const uint64_t *d_out_off,
                            const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_off) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (!lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t grid = 0;
    if ((rc = batch_grid(nbuf, &grid)) != 0) return rc;
    hipLaunchKernelGGL(k_encode_lines_batch, dim3(grid), dim3(kBatchTH), 0, (hipStream_t) stream,
                       (const uint8_t *) d_in, d_in_off, nbuf, (uint8_t *) d_out, d_out_off,
                       lines_plan::make_call(fmt, a, false), a);
    return hip_status();
}

int b64x_decode_strict_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                             void *d_out, const uint64_t *d_out_off, b64x_strict_result *d_res,
                             const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_off || !d_res || (((uintptr_t) d_res) & 7))
        return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (fmt && !lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t grid = 0;
    if ((rc = batch_grid(nbuf, &grid)) != 0) return rc;
    const Call c = lines_plan::make_call(fmt, a, true);
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    if (fmt)
        hipLaunchKernelGGL((k_decode_strict_batch<true>), dim3(grid), dim3(kBatchTH), 0,
                           (hipStream_t) stream, in, d_in_off, nbuf, out, d_out_off, d_res, c, a);
    else
        hipLaunchKernelGGL((k_decode_strict_batch<false>), dim3(grid), dim3(kBatchTH), 0,
                           (hipStream_t) stream, in, d_in_off, nbuf, out, d_out_off, d_res, c, a);
    return hip_status();
}

}  // extern "C"
