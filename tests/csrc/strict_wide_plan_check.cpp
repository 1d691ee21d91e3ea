// Host build of the plan of the ragged strict decode balanced over bytes
// (async_amd/csrc/b64x_strict_wide_plan.h), for checking its arithmetic
// without a GPU: tests/test_decode_strict_batch_wide.py compiles this file
// with the host compiler and -fsanitize=address,undefined, runs it as a child
// process and compares every number with a model written in Python.
//
// Queries, one per line, on standard input:
//   K                                    the constants: T unit block_waves blocks_per_cu empty_run
//   G <total_hint> <cus>                 the grid: blocks
//   S <total> <waves>                    the share: S, and 1 if S waves >= total (128-bit)
//   N <total> <waves> <w>                wave w's span: owns lo hi
//   U <L> <s> <trailing> <pad> <aligned> <W> <x>...
//                                        a text of W bytes (L 0: plain):
//                                        length_error E hot_lanes tail_lanes cut(x)...
// `aligned`: the text is dword aligned on both sides (the hot path also needs
// the call's `fast`).  A text with a LENGTH verdict has no lanes: every cut is
// 0.  One line of numbers is printed per query.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "b64x_strict_wide_plan.h"

static const int kMaxValues = 4096;

static int answer(char kind, const uint64_t *v, int nv)
{
    static const uint8_t sep[4] = {'\r', '\n', '\n', '\r'};  // the plan never looks at the bytes
    if (kind == 'K' && nv == 0) {
        printf("%" PRIu64 " %" PRIu64 " %u %u %u\n", strict_wide_plan::kShareMin,
               strict_wide_plan::kShareUnit, strict_wide_plan::kBlockWaves,
               strict_wide_plan::kBlocksPerCU, strict_wide_plan::kEmptyRun);
        return 0;
    }
    if (kind == 'G' && nv == 2) {
        printf("%u\n", strict_wide_plan::grid_blocks(v[0], (uint32_t) v[1]));
        return 0;
    }
    if (kind == 'S' && nv == 2) {
        const uint64_t s = strict_wide_plan::share(v[0], (uint32_t) v[1]);
        const unsigned __int128 cover = (unsigned __int128) s * v[1];
        printf("%" PRIu64 " %d\n", s, cover >= v[0] ? 1 : 0);
        return 0;
    }
    if (kind == 'N' && nv == 3) {
        const uint64_t s = strict_wide_plan::share(v[0], (uint32_t) v[1]);
        uint64_t lo = 0, hi = 0;
        const bool owns = strict_wide_plan::span(v[0], s, (uint32_t) v[2], &lo, &hi);
        printf("%d %" PRIu64 " %" PRIu64 "\n", owns ? 1 : 0, owns ? lo : 0, owns ? hi : 0);
        return 0;
    }
    if (kind == 'U' && nv >= 6) {
        const lines_plan::Call c = lines_plan::make_call(
            (uint32_t) v[0], (uint32_t) v[1], sep, v[2] != 0, v[3] != 0, true);
        const bool fast = c.fast && v[4] != 0;
        const uint64_t W = v[5];
        const lines_plan::StrictPlan p = lines_plan::strict_plan(W, c, fast);
        const uint64_t lanes = p.length_error ? 0 : p.hot_lanes + p.tail_lanes;
        printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64, p.length_error, p.E, p.hot_lanes,
               p.tail_lanes);
        for (int i = 6; i < nv; i++)
            printf(" %" PRIu64, strict_wide_plan::cut(v[i], W, lanes, c));
        printf("\n");
        return 0;
    }
    return -1;
}

static int parse(char *line, uint64_t *v)
{
    char *tok = strtok(line, " \t\r\n");
    if (!tok) return 0;  // an empty line
    const char kind = tok[0];
    int nv = 0;
    while ((tok = strtok(NULL, " \t\r\n")) != NULL) {
        if (nv == kMaxValues) return -1;
        v[nv++] = strtoull(tok, NULL, 10);
    }
    return answer(kind, v, nv);
}

int main()
{
    char *line = NULL;
    size_t cap = 0;
    uint64_t *v = (uint64_t *) malloc(sizeof(uint64_t) * kMaxValues);
    if (!v) return 2;
    int rc = 0;
    while (rc == 0 && getline(&line, &cap, stdin) >= 0)
        if (parse(line, v)) {
            fprintf(stderr, "bad query\n");
            rc = 2;
        }
    free(line);
    free(v);
    return rc;
}
