// The arithmetic of the line format, stated once for the line-wrapped encode
// and the strict decode in all their forms (b64x_wrap.hip, b64x_strict.hip,
// b64x_lines_batch.hip): how many characters and bytes a text has, where
// character e stands, which 16-byte blocks or 16-character lanes are hot, and
// where the reciprocals that replace the divisions are exact.
//
//   - the kernels' argument structs (Alpha, WrapArgs, StrictArgs, Call) and
//     the argument checks that need no device (fmt_ok, alpha_ok);
//   - the per-buffer plans (wrap_plan, strict_plan): on the device the
//     wave-uniform prologue a wave of the ragged kernels runs once per buffer;
//   - the host's launch plans of the one-buffer and strided calls
//     (plan_wrap_one, plan_wrap_rows, plan_strict), built on the former.
//
// No HIP header is needed: plain integers in, plain integers out.  The same
// text compiles as host C++ (tests/csrc/lines_batch_plan_check.cpp and
// lines_plan_check.cpp, with no include path but this directory), which is
// how lengths past 2^32, grids past 2^31 and the reciprocals' edges are
// checked without a GPU.
#ifndef ASYNC_AMD_B64X_LINES_PLAN_H
#define ASYNC_AMD_B64X_LINES_PLAN_H

#include <stdint.h>
#include <string.h>

#include "../../include/b64x.h"  // plain C; by its place, so that this header needs no -I

#if defined(__HIPCC__)
#define LP_HD __host__ __device__ __forceinline__
#else
#define LP_HD static inline
#endif

namespace lines_plan {

// The one-buffer and strided kernels run blocks of 256 lanes, each lane a
// 16-byte output block (encode) or 16 characters (decode): a hot tile covers
// 4,096 bytes or characters.
constexpr uint32_t kBlockLanes = 256;
// The ragged kernels' work unit is a wave: 64 such lanes, so a pass covers
// 1,024 bytes or characters.
constexpr uint32_t kPassLanes = 64;
constexpr uint32_t kPassUnits = kPassLanes * 16;
// A lane's position is its tile's (or pass's) column plus its own offset: the
// 32-bit reciprocal must be exact below divisor + a tile.
constexpr uint32_t kRecipSpan = kBlockLanes * 16;

// ------------------------------------------------------ kernel arguments --
// Plain integers; they travel as kernel arguments (capture-safe, nothing on
// the device to set up), so fields, order and types are part of the kernels.

struct Alpha {
    uint32_t p62, p63, padc, pad;
};

// One call of the line-wrapped encode (one buffer or rows).
struct WrapArgs {
    uint64_t len;         // input bytes per row
    uint64_t E;           // characters per row
    uint64_t W;           // wrapped bytes per row
    uint64_t full_lines;  // E / L
    uint64_t in_stride, out_stride;
    uint64_t hot_blocks;  // per row: blocks [0, hot_blocks) take the hot path
    uint64_t hot_slots;   // hot_blocks * hot rows
    uint64_t tail_blocks; // per row: 16-byte pieces of [16 hot_blocks, W)
    uint64_t tail_slots;  // tail_blocks * hot rows
    uint64_t m64;         // floor(2^64 / P) + 1
    uint64_t m64_hb;      // floor(2^64 / hot_blocks) + 1  (rows)
    uint32_t hot_tiles;   // grid blocks that run the hot path
    uint32_t L, P, s;     // line length, pitch L + s, separator length
    uint32_t sep;         // the separator, little-endian, unused bytes zero
    uint32_t last_len;    // E mod L
    uint32_t magic_p;     // ceil(2^32 / P)
    uint32_t magic_hb;    // ceil(2^32 / hot_blocks)  (rows)
    uint32_t hot_blocks32;
};

// One call of the strict decode (one buffer or rows).
struct StrictArgs {
    uint64_t E;           // characters per row
    uint64_t W;           // text bytes per row
    uint64_t in_stride, out_stride;
    uint64_t off_e1, off_e2;  // row offsets of characters E - 1 and E - 2
    uint64_t hot_lanes;   // per row: lanes [0, hot_lanes) take the hot path
    uint64_t hot_slots;   // hot_lanes * rows
    uint64_t tail_lanes;  // per row: the lanes of characters [16 hot_lanes, E)
    uint64_t tail_slots;  // tail_lanes * rows
    uint64_t m64;         // floor(2^64 / L) + 1
    uint64_t m64_hl;      // floor(2^64 / hot_lanes) + 1  (rows)
    uint32_t hot_tiles;   // grid blocks that run the hot path
    uint32_t L, P, s;     // line length, pitch L + s, separator length (plain: 0)
    uint32_t sep;         // the separator, little-endian, unused bytes zero
    uint32_t sep_mask;    // 0xFF for each of its s bytes
    uint32_t magic_l;     // ceil(2^32 / L)
    uint32_t magic_hl;    // ceil(2^32 / hot_lanes)  (rows)
    uint32_t hot_lanes32;
    uint32_t trailing;
    Alpha a;
};

// What depends on the alphabet and the format alone.  Nothing in it depends
// on a length.
struct Call {
    uint32_t L, P, s;     // line length, pitch L + s, separator length (plain: 0)
    uint32_t sep;         // the separator, little-endian, unused bytes zero
    uint32_t sep_mask;    // 0xFF for each of its s bytes
    uint32_t trailing;
    uint32_t pad;
    uint32_t magic;       // ceil(2^32 / d), d = P (encode) or L (decode)
    uint32_t fast;        // L >= 16 and magic exact below d + kRecipSpan; else all bytewise
    uint32_t step_k, step_c;  // kPassUnits = step_k d + step_c
};

static_assert(sizeof(Alpha) == 16 && sizeof(WrapArgs) == 136 && sizeof(StrictArgs) == 152 &&
                  sizeof(Call) == 44,
              "kernel arguments: the layout is fixed");

// ------------------------------------------------------- argument checks --

inline Alpha make_alpha(const b64x_alphabet *abc)
{
    Alpha a;
    const char p62 = abc ? abc->pos62 : (char) -1;
    const char p63 = abc ? abc->pos63 : (char) -1;
    const char pc = abc ? abc->padchar : (char) -1;
    a.p62 = (uint8_t) (p62 == (char) -1 ? '+' : p62);
    a.p63 = (uint8_t) (p63 == (char) -1 ? '/' : p63);
    a.padc = (uint8_t) (pc == (char) -1 ? '=' : pc);
    a.pad = abc ? (abc->pad ? 1 : 0) : 1;
    return a;
}

inline bool is_alnum(uint32_t c) { return c - 'A' < 26u || c - 'a' < 26u || c - '0' < 10u; }

// The decoder needs what the encoder takes for granted: 64 distinct
// characters and a pad character that is none of them.
inline bool alpha_ok(const Alpha &a)
{
    if (a.p62 == a.p63 || is_alnum(a.p62) || is_alnum(a.p63)) return false;
    return !(a.pad && (is_alnum(a.padc) || a.padc == a.p62 || a.padc == a.p63));
}

// The format's rules, in the order include/b64x.h states them.
inline bool fmt_ok(const b64x_lines *f, const Alpha &a)
{
    if (!f) return false;
    if (f->line_len == 0 || f->line_len % 4 != 0) return false;
    if (f->sep_len < 1 || f->sep_len > 4) return false;
    if (f->flags & ~B64X_LINES_TRAILING) return false;
    if ((uint64_t) f->line_len + f->sep_len > 0xFFFFFFFFull) return false;
    for (uint32_t i = 0; i < f->sep_len; i++) {
        const uint32_t c = f->sep[i];
        if (is_alnum(c) || c == a.p62 || c == a.p63) return false;
    }
    return true;
}

// ----------------------------------------------------------- reciprocals --

// *magic = ceil(2^32 / d); true if its multiply-high is x / d for every
// x < bound.
LP_HD bool recip32(uint64_t d, uint64_t bound, uint32_t *magic)
{
    *magic = (uint32_t) ((0xFFFFFFFFull + d) / d);
    const uint64_t err = (uint64_t) *magic * d - (1ull << 32);  // < d
    return bound < (1ull << 32) && bound * err < (1ull << 32);
}

// *m64 = floor(2^64 / d) + 1; true if its multiply-high is x / d for every
// x <= max:  x (m64 d - 2^64) < 2^64.
LP_HD bool recip64(uint64_t d, uint64_t max, uint64_t *m64)
{
    *m64 = ~0ull / d + 1;
    return max <= ~0ull / d;
}

// The 32-bit reciprocal serves line lengths from 16 (a 16-byte block then
// holds at most one separator) and, on the encode, pitches up to 2^24
// (P > L: not a pitch that wrapped round 32 bits, which fmt_ok refuses but
// b64x_encoded_lines_len still measures).
LP_HD bool divisor_ok(uint32_t L, uint32_t P, bool decode)
{
    return L >= 16 && (decode || (P > L && P <= (1u << 24)));
}

// A divisor d (the pitch or the line length) as reciprocals, if they are
// exact for the call: the 32-bit one below `bound`, the 64-bit one up to
// `max64` (set only where the 32-bit one is exact).
LP_HD bool set_reciprocals(uint32_t d, uint64_t bound, uint64_t max64, uint32_t *magic,
                           uint64_t *m64)
{
    return recip32(d, bound, magic) && recip64(d, max64, m64);
}

// ---------------------------------------------------------------- format --

// decode: the divisor is the line length (positions are characters); encode:
// the pitch (positions are bytes of text).  L == 0: plain text (decode only).
LP_HD Call make_call(uint32_t L, uint32_t s, const uint8_t *sep, bool trailing, bool pad,
                     bool decode)
{
    Call c;
    c.L = L;
    c.s = L ? s : 0;
    c.P = L + c.s;
    c.sep = c.sep_mask = 0;
    for (uint32_t i = 0; i < c.s; i++) {
        c.sep |= (uint32_t) sep[i] << (8 * i);
        c.sep_mask |= 0xFFu << (8 * i);
    }
    c.trailing = trailing ? 1 : 0;
    c.pad = pad ? 1 : 0;
    c.magic = c.step_k = c.step_c = 0;
    c.fast = L == 0 ? 1 : 0;
    const uint32_t d = decode ? c.L : c.P;
    if (divisor_ok(L, c.P, decode))
        c.fast = recip32(d, (uint64_t) d + kRecipSpan, &c.magic) ? 1 : 0;
    if (d) {
        c.step_k = kPassUnits / d;
        c.step_c = kPassUnits % d;
    }
    return c;
}

// f == NULL: plain text (decode only).
inline Call make_call(const b64x_lines *f, const Alpha &a, bool decode)
{
    if (!f) return make_call(0, 0, nullptr, false, a.pad != 0, decode);
    return make_call(f->line_len, f->sep_len, f->sep, (f->flags & B64X_LINES_TRAILING) != 0,
                     a.pad != 0, decode);
}

// The same for a kernel that works in tiles: the 32-bit bound is the call's
// own, d + kRecipSpan, which make_call has checked already.
inline bool tile_reciprocals(const Call &c, bool decode, uint64_t max64, uint32_t *magic,
                             uint64_t *m64)
{
    if (!divisor_ok(c.L, c.P, decode)) return false;
    *magic = c.magic;
    return c.fast && recip64(decode ? c.L : c.P, max64, m64);
}

// 32-bit division where the value allows it.
LP_HD uint64_t div32(uint64_t x, uint32_t d)
{
    return (x >> 32) ? x / d : (uint64_t) ((uint32_t) x / d);
}

LP_HD uint64_t encoded_len(uint64_t n, bool pad)
{
    const uint64_t g = n / 3, r = n - 3 * g;
    return 4 * g + (r ? (pad ? 4 : r + 1) : 0);
}

// Offset in the text of character e.
LP_HD uint64_t char_off(uint64_t e, const Call &c)
{
    if (!c.s) return e;
    const uint64_t k = div32(e, c.L);
    return k * c.P + (e - k * c.L);
}

// ---------------------------------------------------------------- encode --

struct WrapPlan {
    uint64_t E;            // characters
    uint64_t W;            // bytes of wrapped text
    uint64_t full_lines;   // E / L
    uint64_t hot_blocks;   // 16-byte blocks [0, hot_blocks) take the hot path
    uint64_t tail_pieces;  // 16-byte pieces of [16 hot_blocks, W), bytewise
    uint32_t last_len;     // E mod L
};

// `fast`: the call's reciprocals are exact and this buffer is dword aligned on
// both sides.  Hot are the blocks wholly below the first character whose
// group does not have 20 readable bytes behind its first byte (nothing
// outside the buffer is read).
LP_HD WrapPlan wrap_plan(uint64_t n, const Call &c, bool fast)
{
    WrapPlan p;
    p.E = encoded_len(n, c.pad != 0);
    p.full_lines = div32(p.E, c.L);
    p.last_len = (uint32_t) (p.E - p.full_lines * c.L);
    const uint64_t lines = p.full_lines + (p.last_len ? 1 : 0);
    p.W = p.E ? p.E + (uint64_t) c.s * (lines - (c.trailing ? 0 : 1)) : 0;
    p.hot_blocks = 0;
    if (fast && n >= 17) p.hot_blocks = char_off((n - 17) / 3 * 4, c) / 16;
    p.tail_pieces = (p.W - 16 * p.hot_blocks + 15) / 16;
    return p;
}

// ---------------------------------------------------------------- decode --

struct StrictPlan {
    uint64_t E;             // characters (no E: those of the whole lines)
    uint64_t hot_lanes;     // lanes [0, hot_lanes) of 16 characters take the hot path
    uint64_t tail_lanes;    // the lanes of characters [16 hot_lanes, E), bytewise
    uint64_t off_e1, off_e2;  // offsets of characters E - 1 and E - 2 (E >= 2)
    uint32_t length_error;  // no encoder output has this length: {LENGTH, W}
};

// Steps 1 and 2 of the scalar procedure of b64x.h for a text of W bytes, and
// the hot/tail split: hot lanes lie below character E - 4 with their load
// window (24 bytes from the dword at or below the lane's first byte; plain:
// its 16 bytes) inside the text.
LP_HD StrictPlan strict_plan(uint64_t W, const Call &c, bool fast)
{
    StrictPlan p;
    p.E = W;
    p.hot_lanes = p.tail_lanes = p.off_e1 = p.off_e2 = 0;
    p.length_error = 0;
    if (W == 0) return p;
    bool has_e = true;
    uint64_t k1 = 0;  // the line of character E - 1
    if (c.s) {
        const uint64_t m = c.trailing ? W : W + c.s;
        if (m < W) {  // W + s wrapped round: no text is that long
            p.E = 0;
            has_e = false;
        } else {
            const uint64_t k = div32(m, c.P), r = m - k * c.P;
            const uint64_t rem = r > c.s ? r - c.s : 0;  // < L: the short last line
            const uint64_t lines = k + (rem ? 1 : 0);    // ceil(E / L)
            p.E = k * c.L + rem;
            if (r != 0 && r <= c.s) has_e = false;
            // the encoder's length for E characters gives W back
            if (p.E == 0 || p.E + (uint64_t) c.s * (lines - (c.trailing ? 0 : 1)) != W)
                has_e = false;
            k1 = lines ? lines - 1 : 0;
        }
    }
    if (has_e && (c.pad ? (p.E & 3) != 0 : (p.E & 3) == 1)) has_e = false;
    if (!has_e) {
        p.length_error = 1;
        return p;
    }
    if (p.E >= 2) {
        if (c.s) {
            const uint64_t c1 = p.E - 1 - k1 * c.L;  // the column of character E - 1
            p.off_e1 = k1 * c.P + c1;
            p.off_e2 = p.off_e1 - 1 - (c1 ? 0 : c.s);
        } else {
            p.off_e1 = p.E - 1;
            p.off_e2 = p.E - 2;
        }
    }
    uint64_t n = 0;
    if (fast && p.E >= 4 + 16) {
        n = (p.E - 4) / 16;
        const uint64_t win = c.s ? 24 : 16;
        while (n > 0 && (char_off((n - 1) * 16, c) & ~(uint64_t) 3) + win > W) n--;
    }
    p.hot_lanes = n;
    p.tail_lanes = (p.E + 15) / 16 - n;
    return p;
}

// ---------------------------------------------------------- launch plans --
// How the host runs a one-buffer or strided call.  kHot: the grid is
// hot_tiles blocks of hot blocks or lanes, then the blocks of the tail
// slots.  kAny: the bytewise kernel for the whole text, grid-stride.  The
// alignment facts come in as the low four bits of the two addresses.

enum Kind { kAny, kHot };

inline uint64_t blocks_of(uint64_t slots) { return (slots + kBlockLanes - 1) / kBlockLanes; }

// The bytewise kernels walk every row's 16-byte or 16-character slots.
inline uint32_t any_grid(uint64_t per_row, uint32_t nbuf)
{
    const uint64_t grid = blocks_of(per_row * nbuf);
    return grid > (1u << 20) ? 1u << 20 : (uint32_t) grid;
}

struct WrapLaunch {
    Kind kind;
    uint32_t grid;
    WrapArgs w;
};

inline WrapLaunch wrap_any(uint64_t len, const WrapPlan &p, const Call &c, uint64_t in_stride,
                           uint64_t out_stride)
{
    WrapLaunch r;
    r.kind = kAny;
    r.grid = 0;
    memset(&r.w, 0, sizeof r.w);
    r.w.len = len;
    r.w.E = p.E;
    r.w.W = p.W;
    r.w.full_lines = p.full_lines;
    r.w.last_len = p.last_len;
    r.w.in_stride = in_stride;
    r.w.out_stride = out_stride;
    r.w.L = c.L;
    r.w.P = c.P;
    r.w.s = c.s;
    r.w.sep = c.sep;
    return r;
}

// One buffer of n bytes.  Hot from a dword-aligned input and a 16-byte
// aligned output: the blocks of wrap_plan.
inline WrapLaunch plan_wrap_one(uint64_t n, const Call &c, uint32_t in_low4, uint32_t out_low4)
{
    const WrapPlan p = wrap_plan(n, c, true);
    WrapLaunch r = wrap_any(n, p, c, 0, 0);
    WrapArgs &w = r.w;
    const bool aligned = (in_low4 & 3) == 0 && (out_low4 & 15) == 0;
    if (aligned && n >= 17 && tile_reciprocals(c, false, w.W, &w.magic_p, &w.m64)) {
        w.hot_blocks = p.hot_blocks;
        w.tail_blocks = w.tail_slots = p.tail_pieces;
        const uint64_t tiles = blocks_of(w.hot_blocks);
        const uint64_t grid = tiles + blocks_of(w.tail_slots);
        if (w.hot_blocks > 0 && grid < (1ull << 31)) {
            w.hot_slots = w.hot_blocks;
            w.hot_tiles = (uint32_t) tiles;
            r.kind = kHot;
            r.grid = (uint32_t) grid;
            return r;
        }
    }
    r.grid = any_grid((w.W + 15) / 16, 1);
    return r;
}

// nbuf > 1 rows of len bytes.  kHot covers rows [0, nbuf - 1) only: a row is
// hot up to the first character of an incomplete group, and such a window may
// read into the next row, so the last row goes alone, as one buffer
// (plan_wrap_one).  Positions inside a row are 32-bit; the (row, block) of a
// slot comes from the reciprocals of hot_blocks.  kAny covers all nbuf rows.
inline WrapLaunch plan_wrap_rows(uint64_t len, uint32_t nbuf, const Call &c, uint32_t in_low4,
                                 uint32_t out_low4, uint64_t in_stride, uint64_t out_stride)
{
    WrapLaunch r = wrap_any(len, wrap_plan(len, c, false), c, in_stride, out_stride);
    WrapArgs &w = r.w;
    const uint32_t hot_rows = nbuf - 1;
    const bool aligned = ((in_low4 | out_low4 | in_stride | out_stride) & 3) == 0;
    if (aligned && len >= 20 && w.W < (1u << 28) && divisor_ok(c.L, c.P, false) &&
        set_reciprocals(c.P, w.W, w.W, &w.magic_p, &w.m64)) {
        const uint64_t e_c = len / 3 * 4;  // characters of complete groups
        const uint64_t hot_end = (e_c == w.E && w.last_len == 0) ? w.W : char_off(e_c, c);
        w.hot_blocks = hot_end / 16;
        w.hot_slots = w.hot_blocks * hot_rows;
        w.tail_blocks = (w.W - 16 * w.hot_blocks + 15) / 16;
        w.tail_slots = w.tail_blocks * hot_rows;
        const uint64_t tiles = blocks_of(w.hot_slots);
        const uint64_t grid = tiles + blocks_of(w.tail_slots);
        if (w.hot_blocks > 1 && grid < (1ull << 31)) {
            w.hot_blocks32 = (uint32_t) w.hot_blocks;
            // exact: the lane's slot below hot_blocks + a block, the tile's below hot_slots
            const bool ok32 = recip32(w.hot_blocks, w.hot_blocks + kBlockLanes, &w.magic_hb);
            const bool ok64 = recip64(w.hot_blocks, w.hot_slots, &w.m64_hb);
            if (ok32 && ok64) {
                w.hot_tiles = (uint32_t) tiles;
                r.kind = kHot;
                r.grid = (uint32_t) grid;
                return r;
            }
        }
    }
    r.grid = any_grid((w.W + 15) / 16, nbuf);
    return r;
}

struct StrictLaunch {
    Kind kind;
    uint32_t grid;
    uint32_t length_error;  // no kernel reads the text: every record is {LENGTH, W}
    StrictArgs w;
};

// nbuf rows of W bytes of text (nbuf == 1: one buffer of any length; rows:
// 32-bit positions inside a row, the strides dword aligned too).
inline StrictLaunch plan_strict(uint64_t W, uint32_t nbuf, const Call &c, const Alpha &a,
                                uint32_t in_low4, uint32_t out_low4, uint64_t in_stride,
                                uint64_t out_stride)
{
    const bool aligned = ((in_low4 | out_low4) & 3) == 0 &&
                         (nbuf == 1 || ((in_stride | out_stride) & 3) == 0);
    const StrictPlan p = strict_plan(W, c, aligned);
    StrictLaunch r;
    r.kind = kAny;
    r.grid = 0;
    r.length_error = p.length_error;
    StrictArgs &w = r.w;
    memset(&w, 0, sizeof w);
    w.E = p.E;
    w.W = W;
    w.in_stride = in_stride;
    w.out_stride = out_stride;
    w.off_e1 = p.off_e1;
    w.off_e2 = p.off_e2;
    w.L = c.L;
    w.P = c.P;
    w.s = c.s;
    w.sep = c.sep;
    w.sep_mask = c.sep_mask;
    w.trailing = c.trailing;
    w.a = a;
    const uint64_t hot = p.hot_lanes, per_row = p.hot_lanes + p.tail_lanes;
    if (nbuf == 1 && hot > 0 && (!c.s || tile_reciprocals(c, true, w.E, &w.magic_l, &w.m64))) {
        w.hot_lanes = w.hot_slots = hot;
        w.tail_lanes = w.tail_slots = per_row - hot;
        const uint64_t tiles = blocks_of(hot);
        const uint64_t grid = tiles + blocks_of(w.tail_slots);
        if (grid < (1ull << 31)) {
            w.hot_tiles = (uint32_t) tiles;
            r.kind = kHot;
            r.grid = (uint32_t) grid;
            return r;
        }
    }
    if (nbuf > 1 && hot > 1 && W < (1u << 28) &&
        (!c.s || (divisor_ok(c.L, c.P, true) &&
                  set_reciprocals(c.L, w.E, w.E, &w.magic_l, &w.m64)))) {
        w.hot_lanes = hot;
        w.hot_slots = hot * nbuf;
        w.tail_lanes = per_row - hot;
        w.tail_slots = w.tail_lanes * nbuf;
        w.hot_lanes32 = (uint32_t) hot;
        // exact: the lane's slot below hot + a block, the tile's below hot_slots
        const bool ok32 = recip32(hot, hot + kBlockLanes, &w.magic_hl);
        const bool ok64 = recip64(hot, w.hot_slots, &w.m64_hl);
        const uint64_t tiles = blocks_of(w.hot_slots);
        const uint64_t grid = tiles + blocks_of(w.tail_slots);
        if (ok32 && ok64 && grid < (1ull << 31)) {
            w.hot_tiles = (uint32_t) tiles;
            r.kind = kHot;
            r.grid = (uint32_t) grid;
            return r;
        }
    }
    w.hot_lanes = w.hot_slots = w.tail_lanes = w.tail_slots = 0;
    w.hot_tiles = 0;
    r.grid = any_grid(per_row, nbuf);
    return r;
}

}  // namespace lines_plan

#endif  // ASYNC_AMD_B64X_LINES_PLAN_H
