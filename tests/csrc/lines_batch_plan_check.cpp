// Host build of the per-buffer prologue of the ragged line-wrapped encode and
// strict decode kernels (async_amd/csrc/b64x_lines_plan.h), for checking its
// arithmetic without a GPU: tests/test_lines_batch.py compiles this file with
// the host compiler and -fsanitize=address,undefined, runs it as a child
// process and compares every field with formulas written in Python.
//
// Queries, one per line, on standard input (or one query as the arguments):
//   C <L> <s> <decode>                       the call: fast magic step_k step_c
//   E <L> <s> <trailing> <pad> <aligned> <n> encode of n bytes:
//                                            E W full_lines last_len hot_blocks tail_pieces
//   D <L> <s> <trailing> <pad> <aligned> <W> strict decode of W bytes of text (L 0: plain):
//                                            E length_error hot_lanes tail_lanes off_e1 off_e2
// `aligned`: the buffer is dword aligned on both sides (the hot path also
// needs the call's `fast`).  One line of numbers is printed per query.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "b64x_lines_plan.h"

static int answer(char kind, const uint64_t *v, int nv)
{
    static const uint8_t sep[4] = {'\r', '\n', '\n', '\r'};  // the plan never looks at the bytes
    if (kind == 'C' && nv == 3) {
        const lines_plan::Call c =
            lines_plan::make_call((uint32_t) v[0], (uint32_t) v[1], sep, true, true, v[2] != 0);
        printf("%u %u %u %u\n", c.fast, c.magic, c.step_k, c.step_c);
        return 0;
    }
    if ((kind == 'E' || kind == 'D') && nv == 6) {
        const bool decode = kind == 'D';
        const lines_plan::Call c = lines_plan::make_call(
            (uint32_t) v[0], (uint32_t) v[1], sep, v[2] != 0, v[3] != 0, decode);
        const bool fast = c.fast && v[4] != 0;
        if (decode) {
            const lines_plan::StrictPlan p = lines_plan::strict_plan(v[5], c, fast);
            printf("%" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.E,
                   p.length_error, p.hot_lanes, p.tail_lanes, p.off_e1, p.off_e2);
        } else {
            if (c.L == 0) return -1;
            const lines_plan::WrapPlan p = lines_plan::wrap_plan(v[5], c, fast);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 "\n", p.E, p.W,
                   p.full_lines, p.last_len, p.hot_blocks, p.tail_pieces);
        }
        return 0;
    }
    return -1;
}

static int parse(char *line)
{
    char *tok = strtok(line, " \t\r\n");
    if (!tok) return 0;  // an empty line
    const char kind = tok[0];
    uint64_t v[6];
    int nv = 0;
    while ((tok = strtok(NULL, " \t\r\n")) != NULL) {
        if (nv == 6) return -1;
        v[nv++] = strtoull(tok, NULL, 10);
    }
    return answer(kind, v, nv);
}

int main(int argc, char **argv)
{
    char line[256];
    if (argc > 1) {
        size_t used = 0;
        for (int i = 1; i < argc; i++) {
            const int n = snprintf(line + used, sizeof line - used, "%s ", argv[i]);
            if (n < 0 || (size_t) n >= sizeof line - used) return 2;
            used += (size_t) n;
        }
        return parse(line) ? 2 : 0;
    }
    while (fgets(line, sizeof line, stdin))
        if (parse(line)) {
            fprintf(stderr, "bad query\n");
            return 2;
        }
    return 0;
}
