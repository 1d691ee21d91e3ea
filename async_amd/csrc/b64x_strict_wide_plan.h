// The plan of the ragged strict decode that balances a batch over its bytes
// (b64x_strict_wide.hip, b64x_decode_strict_batch_wide): the grid, a wave's
// share of the arena of text, and which 16-character lanes of a text a span of
// its bytes owns.  Plain integer arithmetic, no HIP: the same text compiles as
// host C++ with no include path but this directory
// (tests/csrc/strict_wide_plan_check.cpp), which is how lengths past 2^32 and
// totals up to 2^64 - 1 are checked without a GPU.
//
// Shares.  The texts lie end to end in one arena of
// total = in_off[nbuf] - in_off[0] bytes.  The grid has Wv = 4 blocks waves;
// wave w takes the arena bytes [w S, (w + 1) S) below total, with
//     S = max(kShareMin, 16 ceil(total / (16 Wv)))
// so that S Wv >= total whatever the host's hint was: no wave loops over
// spans, and the hint sizes the grid and nothing else,
//     blocks = clamp(ceil(total_hint / (4 kShareMin)), 1, 8 CUs)
// with total_hint == 0 ("unknown") filling the device.  The saturating
// product and the span are those of the encode's plan, one copy.
//
// Ownership.  A text of W bytes that has an E has lanes = hot_lanes +
// tail_lanes = ceil(E / 16) lanes of 16 characters (12 output bytes), as
// lines_plan::strict_plan counts them.  For a position x of the text, with
// (k, r) = divmod(x, P),
//     chars_below(x) = k L + min(r, L)            (plain text: x)
// is the number of characters that stand below x, and
//     cut(x) = 0                                        x == 0
//              lanes                                    x >= W
//              min(lanes, ceil(chars_below(x) / 16))    else
// A span [a, z) of the text owns lanes [cut(a), cut(z)): lane j belongs to the
// span that holds the text offset of character 16 j.  cut is monotone and
// neighbouring spans share their boundary, so every lane has exactly one
// owner, wherever the boundaries fall: in mid-group, inside a separator, on a
// text's first or last byte.  A text with a LENGTH verdict has no lanes.
#ifndef ASYNC_AMD_B64X_STRICT_WIDE_PLAN_H
#define ASYNC_AMD_B64X_STRICT_WIDE_PLAN_H

#include <stdint.h>

#include "b64x_encode_wide_plan.h"
#include "b64x_lines_plan.h"

namespace strict_wide_plan {

using enc_wide_plan::mul_sat;
using enc_wide_plan::span;

constexpr uint32_t kBlockLanes = 256;                       // lanes per block
constexpr uint32_t kBlockWaves = kBlockLanes / lines_plan::kPassLanes;
constexpr uint32_t kBlocksPerCU = 8;                        // the grid's bound
constexpr uint64_t kShareMin = 16384;                       // T: text bytes a wave takes at least (16 passes)
constexpr uint64_t kShareUnit = 16;                         // shares are multiples of a lane's characters
constexpr uint32_t kEmptyRun = 8;                           // empty texts walked before a search

// Blocks of a call: of total_hint and the device alone.
static inline uint32_t grid_blocks(uint64_t total_hint, uint32_t cus)
{
    const uint64_t cap = (uint64_t) (cus ? cus : 1) * kBlocksPerCU;
    if (total_hint == 0) return (uint32_t) cap;
    const uint64_t per = kBlockWaves * kShareMin;
    const uint64_t want = total_hint / per + (total_hint % per ? 1 : 0);
    return (uint32_t) (want < 1 ? 1 : want > cap ? cap : want);
}

// S: the arena bytes of one wave.  16 q <= 2^64 / waves + 16: no overflow
// from two waves on.
LP_HD uint64_t share(uint64_t total, uint32_t waves)
{
    const uint64_t d = kShareUnit * waves;
    const uint64_t q = lines_plan::div32(total, (uint32_t) d);
    const uint64_t s = kShareUnit * (q + (q * d != total ? 1 : 0));
    return s < kShareMin ? kShareMin : s;
}

// The characters that stand below position x of a text (c.s == 0: plain).
LP_HD uint64_t chars_below(uint64_t x, const lines_plan::Call &c)
{
    if (!c.s) return x;
    const uint64_t k = lines_plan::div32(x, c.P), r = x - k * c.P;
    return k * c.L + (r < c.L ? r : c.L);
}

// The first lane that the bytes from x on own, of a text of W bytes and
// `lanes` lanes.
LP_HD uint64_t cut(uint64_t x, uint64_t W, uint64_t lanes, const lines_plan::Call &c)
{
    if (x == 0) return 0;
    if (x >= W) return lanes;
    const uint64_t n = chars_below(x, c);
    const uint64_t j = n / 16 + (n % 16 ? 1 : 0);
    return j < lanes ? j : lanes;
}

}  // namespace strict_wide_plan

#endif  // ASYNC_AMD_B64X_STRICT_WIDE_PLAN_H
