// The launch plan of the one-large-piece strict skip decode
// (async_amd/csrc/b64x_skip_wide_plan.h) as a host program with its own main:
// built by tests/test_decode_strict_skip_wide.py with the host compiler under
// ASan + UBSan, no include path but the header's directory.
//
// Queries, one per line, on standard input: <len> <head> <cus>, head being
// the low four bits of the piece's address.  One line per query:
//   tile_bytes tile_count workspace_bytes grid_blocks
#include <inttypes.h>
#include <stdio.h>

#include "b64x_skip_wide_plan.h"

int main()
{
    uint64_t len;
    unsigned head, cus;
    while (scanf("%" SCNu64 " %u %u", &len, &head, &cus) == 3) {
        const uint64_t tiles = skip_wide_plan::tile_count(len, head);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", skip_wide_plan::tile_bytes(len), tiles,
               skip_wide_plan::workspace_bytes(len), skip_wide_plan::grid_blocks(tiles, cus));
    }
    return 0;
}
