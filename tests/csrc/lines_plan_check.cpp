// Host build of the launch plans of the one-buffer and strided line-wrapped
// encode and strict decode (plan_wrap_one, plan_wrap_rows, plan_strict of
// async_amd/csrc/b64x_lines_plan.h), for checking them without a GPU:
// tests/test_lines_plan.py compiles this file with the host compiler and
// -fsanitize=address,undefined, runs it as a child process and checks what it
// prints.  (The per-buffer plans of the ragged kernels: lines_batch_plan_check.cpp.)
//
// Queries, one per line, on standard input (or one query as the arguments),
// <in> and <out> being the low four bits of the two addresses:
//   W <L> <s> <trailing> <pad> <in> <out> <n>          plan_wrap_one
//   R <L> <s> <trailing> <pad> <in> <out> <nbuf> <in_stride> <out_stride> <len>
//                                                      plan_wrap_rows
//       kind grid, then WrapArgs: len E W full_lines in_stride out_stride hot_blocks
//       hot_slots tail_blocks tail_slots m64 m64_hb hot_tiles L P s sep last_len magic_p
//       magic_hb hot_blocks32
//   S <L> <s> <trailing> <pad> <in> <out> <nbuf> <in_stride> <out_stride> <W>
//                                                      plan_strict (L 0: plain)
//       kind grid length_error, then StrictArgs: E W in_stride out_stride off_e1 off_e2
//       hot_lanes hot_slots tail_lanes tail_slots m64 m64_hl hot_tiles L P s sep sep_mask
//       magic_l magic_hl hot_lanes32 trailing
// kind: 0 bytewise, 1 hot.  One line of numbers is printed per query.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "b64x_lines_plan.h"

static void print_row(const uint64_t *f, size_t n)
{
    for (size_t i = 0; i < n; i++) printf("%" PRIu64 "%c", f[i], i + 1 < n ? ' ' : '\n');
}

static int print_wrap(const lines_plan::WrapLaunch &p)
{
    const lines_plan::WrapArgs &w = p.w;
    const uint64_t f[] = {(uint64_t) p.kind, p.grid, w.len, w.E, w.W, w.full_lines, w.in_stride,
                          w.out_stride, w.hot_blocks, w.hot_slots, w.tail_blocks, w.tail_slots,
                          w.m64, w.m64_hb, w.hot_tiles, w.L, w.P, w.s, w.sep, w.last_len,
                          w.magic_p, w.magic_hb, w.hot_blocks32};
    print_row(f, sizeof f / sizeof f[0]);
    return 0;
}

static int answer(char kind, const uint64_t *v, int nv)
{
    static const uint8_t sep[4] = {'\r', '\n', '\n', '\r'};  // the plan never looks at the bytes
    if ((kind == 'W' && nv == 7 && v[0]) || (kind == 'R' && nv == 10 && v[0])) {
        const lines_plan::Call c = lines_plan::make_call((uint32_t) v[0], (uint32_t) v[1], sep,
                                                         v[2] != 0, v[3] != 0, false);
        const uint32_t in = (uint32_t) v[4], out = (uint32_t) v[5];
        return print_wrap(kind == 'W' ? lines_plan::plan_wrap_one(v[6], c, in, out)
                                      : lines_plan::plan_wrap_rows(v[9], (uint32_t) v[6], c, in,
                                                                   out, v[7], v[8]));
    }
    if (kind == 'S' && nv == 10) {
        const lines_plan::Alpha a = {'+', '/', '=', v[3] != 0 ? 1u : 0u};
        const lines_plan::Call c = lines_plan::make_call((uint32_t) v[0], (uint32_t) v[1], sep,
                                                         v[2] != 0, v[3] != 0, true);
        const lines_plan::StrictLaunch p = lines_plan::plan_strict(
            v[9], (uint32_t) v[6], c, a, (uint32_t) v[4], (uint32_t) v[5], v[7], v[8]);
        const lines_plan::StrictArgs &w = p.w;
        const uint64_t f[] = {(uint64_t) p.kind, p.grid, p.length_error, w.E, w.W, w.in_stride,
                              w.out_stride, w.off_e1, w.off_e2, w.hot_lanes, w.hot_slots,
                              w.tail_lanes, w.tail_slots, w.m64, w.m64_hl, w.hot_tiles, w.L, w.P,
                              w.s, w.sep, w.sep_mask, w.magic_l, w.magic_hl, w.hot_lanes32,
                              w.trailing};
        print_row(f, sizeof f / sizeof f[0]);
        return 0;
    }
    return -1;
}

static int parse(char *line)
{
    char *tok = strtok(line, " \t\r\n");
    if (!tok) return 0;  // an empty line
    const char kind = tok[0];
    uint64_t v[10];
    int nv = 0;
    while ((tok = strtok(NULL, " \t\r\n")) != NULL) {
        if (nv == 10) return -1;
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
