// The launch plan of the strict skip decode of many pieces of any size
// (b64x_skip_pieces_wide.hip): the tile size, the bound on the tiles of a
// call, the workspace layout and size and the grids, all as functions of the
// host bound on the call's text (total_cap), the number of pieces and the CU
// count -- never of a piece's length, which only the device sees.  Plain
// integer arithmetic, no HIP: the same text compiles as host C++ with no
// include path but this directory (tests/csrc/skip_pieces_wide_plan_check.cpp).
//
// The tile rule.  T = skip_wide_plan::tile_bytes(total_cap): 4,096 below
// 64 MiB, from there the multiple of 1,024 that keeps total_cap / T at or below
// 16,384.  Piece i (len_i bytes, its first byte head_i = 0..15 bytes behind a
// 16-byte boundary) is cut into tiles of T bytes of address span from that
// boundary, as the one-piece call cuts its piece:
//     tiles_i = len_i ? ceil((len_i + head_i) / T) : 1     <= 16,384
// and, because (len_i + 15) / T + 1 > tiles_i and 15 / T < 1,
//     sum tiles_i <= ceil(total_cap / T) + 2 npieces = tile_bound.
//
// The workspace, every part at a multiple of 64 bytes:
//     ctl      64 bytes: the call's tiles (0 with BOUND), the BOUND flag, the
//              text's bytes, the number of pieces of more than kWaveTiles tiles
//     heads    64 bytes per piece
//     records  64 bytes per tile of tile_bound
//     map      8 bytes per tile of tile_bound: piece | tile in piece << 32
//     big      4 bytes per piece that can have more than kWaveTiles tiles
#ifndef ASYNC_AMD_B64X_SKIP_PIECES_WIDE_PLAN_H
#define ASYNC_AMD_B64X_SKIP_PIECES_WIDE_PLAN_H

#include <stdint.h>

#include "b64x_skip_wide_plan.h"

namespace skip_pw_plan {

using skip_wide_plan::div_up;

constexpr uint64_t kCtlBytes = 64;
constexpr uint64_t kHeadBytes = 64;     // a piece's head
constexpr uint64_t kRecordBytes = skip_wide_plan::kRecordBytes;
constexpr uint64_t kMapBytes = 8;       // a tile's map entry
constexpr uint64_t kWaveTiles = 64;     // the scan: a wave up to here, a workgroup above
constexpr uint64_t kPrepLanes = 1024;   // prep's one workgroup

static inline uint64_t tile_bytes(uint64_t total_cap) { return skip_wide_plan::tile_bytes(total_cap); }

// log2 T where T is a power of two, else 0 (T >= 4,096: 0 is free).
static inline uint32_t tile_shift(uint64_t total_cap)
{
    const uint64_t t = tile_bytes(total_cap);
    if (t & (t - 1)) return 0;
    uint32_t s = 0;
    while ((t >> s) != 1) s++;
    return s;
}

// Tiles of a piece, as the device counts them.
static inline uint64_t piece_tiles(uint64_t len, uint32_t head, uint64_t tile)
{
    if (len == 0) return 1;
    const uint64_t span = len > UINT64_MAX - head ? UINT64_MAX : len + head;
    return div_up(span, tile);
}

// No call within total_cap has more tiles: < 2^15 + 2^33.
static inline uint64_t tile_bound(uint64_t total_cap, uint32_t npieces)
{
    return div_up(total_cap, tile_bytes(total_cap)) + 2 * (uint64_t) npieces;
}

// Pieces of more than kWaveTiles tiles, at the most.
static inline uint64_t big_bound(uint64_t total_cap, uint32_t npieces)
{
    const uint64_t by_tiles = tile_bound(total_cap, npieces) / (kWaveTiles + 1);
    return by_tiles < npieces ? by_tiles : npieces;
}

struct Layout {
    uint64_t heads, records, map, big, bytes;  // offsets in the workspace, and its size
};

// The largest value: 2^38 + 2^39 + 2^36 + 2^34 and small change.
static inline Layout layout(uint64_t total_cap, uint32_t npieces)
{
    const uint64_t bound = tile_bound(total_cap, npieces);
    Layout l;
    l.heads = kCtlBytes;
    l.records = l.heads + kHeadBytes * (uint64_t) npieces;
    l.map = l.records + kRecordBytes * bound;
    l.big = l.map + div_up(kMapBytes * bound, 64) * 64;
    l.bytes = l.big + div_up(4 * big_bound(total_cap, npieces), 64) * 64;
    return l;
}

static inline uint64_t workspace_bytes(uint64_t total_cap, uint32_t npieces)
{
    return layout(total_cap, npieces).bytes;
}

// Count and decode: a wave per tile, the waves striding over the tiles the
// call turns out to have.
static inline uint32_t tile_grid(uint64_t total_cap, uint32_t npieces, uint32_t cus)
{
    return skip_wide_plan::grid_blocks(tile_bound(total_cap, npieces), cus);
}

// Scan: a workgroup per large piece, a wave per small one.
static inline uint32_t scan_grid(uint32_t npieces, uint32_t cus)
{
    const uint64_t cap = (uint64_t) cus * skip_wide_plan::kBlocksPerCU;
    return (uint32_t) (npieces < cap ? npieces : cap);
}

}  // namespace skip_pw_plan

#endif  // ASYNC_AMD_B64X_SKIP_PIECES_WIDE_PLAN_H
