// The walk that the one-pass units of the strict decode that skips line
// breaks share (b64x_skip_rows.hip: k_skip_decode_rows; b64x_skip_pieces.hip:
// k_skip_decode_pieces): the pass's sizes, the 256-entry table with a byte's
// sextet and class, the order of a wave's own LDS accesses, a chunk's entries,
// the last three kept bytes of a pass and the packing of four sextets.  One
// copy, as b64x_skip_body.h.  Layout: DESIGN.md §5, "k_skip_decode_rows".
#ifndef ASYNC_AMD_B64X_SKIP_WALK_H
#define ASYNC_AMD_B64X_SKIP_WALK_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "b64x_skip_body.h"

namespace {

constexpr uint32_t kLanes = lines_plan::kPassLanes;
constexpr uint32_t kPass = lines_plan::kPassUnits;   // bytes per pass (a chunk per lane)
constexpr uint32_t kUnit = 16;                       // sextets a lane decodes at once (12 bytes)
constexpr uint32_t kSextets = kPass + kUnit;         // a pass's sextets behind a carry of < kUnit

// A byte's table entry: its sextet in the low byte (data characters only),
// its class as a packed count -- 16 entries sum without a carry between the
// fields: the sextets' sum stays below bit 10, each count is at most 16 -- and
// a flag in the sign bit for the 64.
constexpr uint32_t kCntShift = 10, kPadShift = 15, kStrangerShift = 20;
constexpr uint32_t kCntKept = 1u << kCntShift;          // bits 10..14: not a skipped byte
constexpr uint32_t kCntPadc = 1u << kPadShift;          // bits 15..19: the pad character (with pad)
constexpr uint32_t kCntStranger = 1u << kStrangerShift;  // bits 20..24: kept, outside the 64, no pad
constexpr uint32_t kIsData = 1u << 31;                  // one of the 64

static_assert(kSkipTH == 256 && kChunk == kUnit && kSextets % 16 == 0 && 16 * 63 < kCntKept,
              "the pass's layout");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3a1 __attribute__((ext_vector_type(3), aligned(1)));  // at any address

DEV void build_row_table(uint32_t *tab, const Alpha &a, const SkipSet &k)
{
    const uint32_t b = threadIdx.x;  // kSkipTH == 256
    uint32_t e = 0;
    if (!in_skip(b, k)) {
        const uint32_t t = classify(b, a);
        e = kCntKept | (t < 64 ? t | kIsData : t == 0xC0u ? kCntPadc : kCntStranger);
    }
    tab[b] = e;
}

// Keep the compiler from moving LDS accesses across this point.  Within one
// wave the LDS executes DS instructions in issue order, so program order is
// all that the hand-off of sextets between the wave's lanes needs.
DEV void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The entries of a lane's chunk; what the chunk holds beyond the row's edge
// counts as skipped.
DEV void classify_chunk(const uint32_t *tab, const Chunk &ch, uint32_t (&t)[kChunk])
{
#pragma unroll
    for (uint32_t i = 0; i < kChunk; i++) t[i] = tab[chunk_byte(ch, i)];
    if (ch.valid != 0xFFFFu) {
#pragma unroll
        for (uint32_t i = 0; i < kChunk; i++) t[i] = ((ch.valid >> i) & 1u) ? t[i] : 0u;
    }
}

// The last three kept bytes of the text so far and their offsets, the last
// one first: the wave's, the same in every lane.
struct Tail {
    uint32_t b0, b1, b2;
    uint64_t o0, o1, o2;
};

// The (up to) three last kept bytes of a pass, a chunk to a lane, go in front
// of the older ones.  off0: the row offset of lane 0's byte 0.  The ballot of
// the lanes that still hold a kept byte names the highest one.
DEV void tail_of_pass(const uint32_t *tab, const Chunk &ch, uint64_t off0, uint32_t lane, Tail *tl)
{
    uint32_t left = 0;
#pragma unroll
    for (uint32_t i = 0; i < kChunk; i++) left |= ((tab[chunk_byte(ch, i)] >> kCntShift) & 1u) << i;
    left &= ch.valid;
#pragma unroll
    for (uint32_t found = 0; found < 3; found++) {
        const uint64_t holders = __ballot(left != 0);
        if (holders == 0) break;
        const uint32_t top = 63u - (uint32_t) __clzll((long long) holders);
        const uint32_t mt = (uint32_t) __shfl((int) left, (int) top);
        const uint32_t j = 31u - (uint32_t) __clz((int) mt);
        const uint32_t word = j < 4 ? ch.w[0] : j < 8 ? ch.w[1] : j < 12 ? ch.w[2] : ch.w[3];
        const uint32_t byte = ((uint32_t) __shfl((int) word, (int) top) >> (8 * (j & 3))) & 0xFFu;
        const uint64_t off = off0 + kChunk * top + j;
        // into place `found`; what stood there and behind it is older
        if (found == 0) {
            tl->b2 = tl->b1, tl->o2 = tl->o1;
            tl->b1 = tl->b0, tl->o1 = tl->o0;
            tl->b0 = byte, tl->o0 = off;
        } else if (found == 1) {
            tl->b2 = tl->b1, tl->o2 = tl->o1;
            tl->b1 = byte, tl->o1 = off;
        } else {
            tl->b2 = byte, tl->o2 = off;
        }
        if (lane == top) left &= ~(1u << j);
    }
}

// 4 sextets (one to a byte, the first in the lowest) -> 24 bits.
DEV uint32_t pack_group(uint32_t w)
{
    return ((w & 0x3Fu) << 18) | ((w & 0x3F00u) << 4) | ((w >> 10) & 0xFC0u) | (w >> 24);
}

}  // namespace

#endif  // ASYNC_AMD_B64X_SKIP_WALK_H
