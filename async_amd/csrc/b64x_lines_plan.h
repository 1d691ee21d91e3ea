// Per-buffer arithmetic of the ragged line-wrapped encode and strict decode
// (b64x_lines_batch.hip): what the strided kernels get from the host in
// WrapArgs / StrictArgs, worked out from one buffer's length.  On the device
// it is the wave-uniform prologue a wave runs once per buffer; the same text
// compiles as host C++ (tests/csrc/lines_batch_plan_check.cpp), which is how
// lengths past 2^32 and the reciprocals' edges are checked without a GPU.
//
// No HIP header is needed: plain integers in, plain integers out.
#ifndef ASYNC_AMD_B64X_LINES_PLAN_H
#define ASYNC_AMD_B64X_LINES_PLAN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LP_HD __host__ __device__ __forceinline__
#else
#define LP_HD static inline
#endif

namespace lines_plan {

// The work unit is a wave: 64 lanes, each a 16-byte output block (encode) or
// 16 characters (decode), so a pass covers 1,024 bytes or characters.
constexpr uint32_t kPassLanes = 64;
constexpr uint32_t kPassUnits = kPassLanes * 16;
// The reciprocal must be exact below divisor + kRecipSpan (the bound of the
// one-buffer kernels' set_reciprocals(); a pass needs divisor + 1,024).
constexpr uint32_t kRecipSpan = 4096;

// What depends on the alphabet and the format alone; travels as a kernel
// argument.  Nothing in it depends on a length.
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
    if (L >= 16 && (decode || c.P <= (1u << 24))) {
        c.magic = (uint32_t) ((0xFFFFFFFFull + d) / d);
        const uint64_t err = (uint64_t) c.magic * d - (1ull << 32);  // < d
        const uint64_t max32 = (uint64_t) d + kRecipSpan;
        c.fast = max32 < (1ull << 32) && max32 * err < (1ull << 32) ? 1 : 0;
    }
    if (d) {
        c.step_k = kPassUnits / d;
        c.step_c = kPassUnits % d;
    }
    return c;
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
// group does not have 20 readable bytes behind its first byte (the rule of
// b64x_encode_lines_dev: nothing outside the buffer is read).
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

}  // namespace lines_plan

#endif  // ASYNC_AMD_B64X_LINES_PLAN_H
