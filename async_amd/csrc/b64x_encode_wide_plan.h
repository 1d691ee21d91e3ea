// The plan of the ragged encode that balances a batch over its bytes
// (b64x_encode_wide.hip, b64x_encode_batch_wide): the grid, a wave's share of
// the arena, and which 16-byte output blocks of a buffer a span of its bytes
// owns.  Plain integer arithmetic, no HIP: the same text compiles as host C++
// with no include path but this directory
// (tests/csrc/encode_wide_plan_check.cpp), which is how lengths past 2^32 and
// totals up to 2^64 - 1 are checked without a GPU.
//
// Shares.  The buffers lie end to end in one arena of
// total = in_off[nbuf] - in_off[0] bytes.  The grid has Wv = 4 blocks waves;
// wave w takes the arena bytes [w S, (w + 1) S) below total, with
//     S = max(kShareMin, 48 ceil(total / (48 Wv)))
// so that S Wv >= total whatever the host's hint was: no wave loops over
// spans, and the hint sizes the grid and nothing else,
//     blocks = clamp(ceil(total_hint / (4 kShareMin)), 1, 8 CUs)
// with total_hint == 0 ("unknown") filling the device.
//
// Ownership.  A buffer of len bytes has B 16-byte output blocks
// (ceil(W / 16) wrapped, ceil(E / 16) plain).  For a byte position x of it
//     cut(x) = 0                                        x == 0
//              B                                        x >= len
//              min(B, ceil(char_off(4 ceil(x / 3)) / 16))  else
// and a span [a, z) of the buffer owns blocks [cut(a), cut(z)).  cut is
// monotone and neighbouring spans share their boundary, so every block has
// exactly one owner, whatever the lengths and wherever the spans fall.
//
// Hot blocks.  Wrapped: those of lines_plan::wrap_plan.  Plain: block j reads
// the 12 bytes from 12 j as dwords and is hot while 12 j + 16 <= len; the rest
// (at most two blocks) and every block of a buffer that is not dword aligned
// on both sides are written bytewise.
#ifndef ASYNC_AMD_B64X_ENCODE_WIDE_PLAN_H
#define ASYNC_AMD_B64X_ENCODE_WIDE_PLAN_H

#include <stdint.h>

#include "b64x_lines_plan.h"

namespace enc_wide_plan {

constexpr uint32_t kBlockLanes = 256;                       // lanes per block
constexpr uint32_t kBlockWaves = kBlockLanes / lines_plan::kPassLanes;
constexpr uint32_t kBlocksPerCU = 8;                        // the grid's bound
constexpr uint64_t kShareMin = 12288;                       // T: input bytes a wave takes at least
constexpr uint64_t kShareUnit = 48;                         // shares are multiples of four lanes' input
constexpr uint32_t kEmptyRun = 8;                           // empty buffers walked before a search

// Blocks of a call: of total_hint and the device alone.
static inline uint32_t grid_blocks(uint64_t total_hint, uint32_t cus)
{
    const uint64_t cap = (uint64_t) (cus ? cus : 1) * kBlocksPerCU;
    if (total_hint == 0) return (uint32_t) cap;
    const uint64_t per = kBlockWaves * kShareMin;
    const uint64_t want = total_hint / per + (total_hint % per ? 1 : 0);
    return (uint32_t) (want < 1 ? 1 : want > cap ? cap : want);
}

// S: the arena bytes of one wave.  48 q <= 2^64 / waves + 48: no overflow
// from four waves on.
LP_HD uint64_t share(uint64_t total, uint32_t waves)
{
    const uint64_t d = kShareUnit * waves;
    const uint64_t q = lines_plan::div32(total, (uint32_t) d);
    const uint64_t s = kShareUnit * (q + (q * d != total ? 1 : 0));
    return s < kShareMin ? kShareMin : s;
}

// s w, or 2^64 - 1 where that does not fit (w < 2^32).
LP_HD uint64_t mul_sat(uint64_t s, uint32_t w)
{
    const uint64_t lo = (s & 0xFFFFFFFFull) * w, hi = (s >> 32) * w;
    if (hi >> 32) return ~0ull;
    const uint64_t r = (hi << 32) + lo;
    return r < lo ? ~0ull : r;
}

// Wave w's span [*lo, *hi) of the arena; false: it owns nothing.  A product
// past 2^64 - 1 lies past every total.
LP_HD bool span(uint64_t total, uint64_t s, uint32_t w, uint64_t *lo, uint64_t *hi)
{
    *lo = mul_sat(s, w);
    if (*lo >= total) return false;
    *hi = total - *lo > s ? *lo + s : total;
    return true;
}

LP_HD uint64_t blocks_of(uint64_t text) { return text / 16 + (text % 16 ? 1 : 0); }

// The first block that the bytes from x on own (c.s == 0: plain text).
LP_HD uint64_t cut(uint64_t x, uint64_t len, uint64_t B, const lines_plan::Call &c)
{
    if (x == 0) return 0;
    if (x >= len) return B;
    const uint64_t g = x / 3 + (x % 3 ? 1 : 0);  // x < len: 4 g is at most E + 3
    const uint64_t b = blocks_of(lines_plan::char_off(4 * g, c));
    return b < B ? b : B;
}

// The plain form's buffer: E characters, blocks [0, hot_blocks) by dwords.
struct PlainPlan {
    uint64_t E;
    uint64_t hot_blocks;
};

LP_HD PlainPlan plain_plan(uint64_t n, bool pad, bool fast)
{
    PlainPlan p;
    p.E = lines_plan::encoded_len(n, pad);
    p.hot_blocks = fast && n >= 16 ? (n - 16) / 12 + 1 : 0;
    return p;
}

}  // namespace enc_wide_plan

#endif  // ASYNC_AMD_B64X_ENCODE_WIDE_PLAN_H
