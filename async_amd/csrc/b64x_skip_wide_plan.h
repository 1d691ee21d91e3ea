// The launch plan of the strict skip decode of one large piece
// (b64x_skip_wide.hip): the tile size as a function of the piece's length, the
// tile count, the workspace size and the grid.  Plain integer arithmetic, no
// HIP: the same text compiles as host C++ with no include path at all
// (tests/csrc/skip_wide_plan_check.cpp), which is how lengths past 2^32 and at
// the top of the 64-bit range are checked without a GPU.
//
// The tile rule.  A piece of len bytes at address lo is cut into tiles of T
// bytes of address span from the 16-byte floor of lo, so its span is
// len + (lo mod 16) <= len + 15.  T depends on len alone:
//     T(len) = max(4,096, ceil(ceil((len + 15) / 16,384) / 1,024) * 1,024)
// a multiple of the pass (1,024 bytes), 4,096 up to 64 MiB - 15 and from there
// the smallest multiple of the pass that keeps the tile count at or below
// 16,384.  The workspace holds a head of 64 bytes and a record of 64 bytes for
// each of the ceil((len + 15) / T) tiles the worst alignment gives.
#ifndef ASYNC_AMD_B64X_SKIP_WIDE_PLAN_H
#define ASYNC_AMD_B64X_SKIP_WIDE_PLAN_H

#include <stdint.h>

namespace skip_wide_plan {

constexpr uint64_t kPassBytes = 1024;    // a wave's pass (b64x_skip_walk.h)
constexpr uint64_t kTileMin = 4096;      // T of every piece below 64 MiB
constexpr uint64_t kMaxTiles = 16384;    // tiles of one piece, at most
constexpr uint64_t kHeadBytes = 64;      // the workspace head
constexpr uint64_t kRecordBytes = 64;    // a tile's record
constexpr uint64_t kWavesPerBlock = 4;
constexpr uint64_t kBlocksPerCU = 8;

static inline uint64_t div_up(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// len + 15, or the largest value where that does not fit.
static inline uint64_t widest_span(uint64_t len) { return len > UINT64_MAX - 15 ? UINT64_MAX : len + 15; }

static inline uint64_t tile_bytes(uint64_t len)
{
    const uint64_t per = div_up(widest_span(len), kMaxTiles);  // < 2^50
    const uint64_t t = div_up(per, kPassBytes) * kPassBytes;
    return t < kTileMin ? kTileMin : t;
}

// Tiles of a piece whose first byte stands `head` (0..15) bytes behind a
// 16-byte boundary.  An empty piece has one, empty, tile: its wave emits what
// the state carried.
static inline uint64_t tile_count(uint64_t len, uint32_t head)
{
    if (len == 0) return 1;
    const uint64_t span = len > UINT64_MAX - head ? UINT64_MAX : len + head;
    return div_up(span, tile_bytes(len));
}

static inline uint64_t workspace_bytes(uint64_t len)
{
    return kHeadBytes + kRecordBytes * div_up(widest_span(len), tile_bytes(len));
}

// A wave per tile, the waves striding over the tiles.
static inline uint32_t grid_blocks(uint64_t tiles, uint32_t cus)
{
    const uint64_t want = div_up(tiles, kWavesPerBlock), cap = (uint64_t) cus * kBlocksPerCU;
    return (uint32_t) (want < cap ? want : cap);
}

}  // namespace skip_wide_plan

#endif  // ASYNC_AMD_B64X_SKIP_WIDE_PLAN_H
