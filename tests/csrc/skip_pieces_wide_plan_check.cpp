// The launch plan of the strict skip decode of many pieces of any size
// (async_amd/csrc/b64x_skip_pieces_wide_plan.h) as a host program with its own
// main: built by tests/test_decode_strict_skip_pieces_wide.py with the host
// compiler under ASan + UBSan, no include path but the header's directory.
//
// Queries, one per line, on standard input: <total_cap> <npieces> <cus>.  One
// line per query:
//   tile_bytes tile_shift tile_bound big_bound heads records map big bytes
//   tile_grid scan_grid
// Then, with the argument "brute": random sets of lengths and heads 0..15 --
// all-empty and all-one-byte sets among them -- whose tiles, counted piece by
// piece as the device counts them, must stay within tile_bound of the sets'
// own total (the tightest bound a caller can give) and of looser ones, for a
// small and a large T.  Prints the number of sets, or the first set that
// breaks the bound and exits 1.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "b64x_skip_pieces_wide_plan.h"

namespace plan = skip_pw_plan;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int brute()
{
    uint64_t sets = 0;
    for (uint32_t round = 0; round < 20000; round++) {
        const uint32_t n = 1 + (uint32_t) (rnd() % (round % 50 == 0 ? 3000 : 40));
        const uint32_t kind = round % 8;  // 0: all empty, 1: all one byte, else mixed
        std::vector<uint64_t> len(n);
        std::vector<uint32_t> head(n);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t r = rnd();
            uint64_t l;
            if (kind == 0) l = 0;
            else if (kind == 1) l = 1;
            else if (kind == 2) l = r % 3;                          // around the empty piece
            else if (kind == 3) l = 4096 * (r % 4 + 1) + (r >> 8) % 33 - 16;  // around tile edges
            else if (kind == 4) l = (r % 8 == 0) ? (r >> 8) % (100u << 20) : (r >> 8) % 100;
            else l = (r >> 8) % (1u << (r % 24));
            len[i] = l;
            head[i] = (uint32_t) (rnd() % 16);
            total += l;
        }
        // the tightest bound, looser ones, and one that makes T large
        const uint64_t caps[] = {total, total + 1, total + 4095, total + (rnd() % (1u << 20)),
                                 total + (1ull << 30), total + (1ull << 40)};
        for (const uint64_t cap : caps) {
            const uint64_t tile = plan::tile_bytes(cap);
            uint64_t tiles = 0, big = 0;
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t t = plan::piece_tiles(len[i], head[i], tile);
                if (t > skip_wide_plan::kMaxTiles) {
                    printf("piece of %" PRIu64 " bytes at head %u: %" PRIu64 " tiles of %" PRIu64 "\n",
                           len[i], head[i], t, tile);
                    return 1;
                }
                tiles += t;
                big += t > plan::kWaveTiles;
            }
            if (tiles > plan::tile_bound(cap, n) || big > plan::big_bound(cap, n)) {
                printf("set of %u pieces, %" PRIu64 " bytes, bound %" PRIu64 ": %" PRIu64
                       " tiles > %" PRIu64 ", or %" PRIu64 " large pieces > %" PRIu64 "\n",
                       n, total, cap, tiles, plan::tile_bound(cap, n), big, plan::big_bound(cap, n));
                return 1;
            }
            sets++;
        }
    }
    printf("%" PRIu64 "\n", sets);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "brute") == 0) return brute();
    uint64_t cap;
    uint32_t npieces, cus;
    while (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &cap, &npieces, &cus) == 3) {
        const plan::Layout l = plan::layout(cap, npieces);
        printf("%" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
               " %" PRIu64 " %u %u\n",
               plan::tile_bytes(cap), plan::tile_shift(cap), plan::tile_bound(cap, npieces),
               plan::big_bound(cap, npieces), l.heads, l.records, l.map, l.big, l.bytes,
               plan::tile_grid(cap, npieces, cus), plan::scan_grid(npieces, cus));
    }
    return 0;
}
