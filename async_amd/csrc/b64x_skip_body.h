// What the units of the strict decode that skips line breaks share
// (b64x_skip.hip: b64x_decode_strict_skip_dev / _batch; b64x_skip_rows.hip:
// b64x_decode_strict_skip_strided): the skip set and its host-side rules, a
// byte's class, the 16-byte chunks at 16-byte aligned addresses with their
// bounds-checked load, a wave's totals and their fold, and the verdict
// arithmetic (steps 2 to 6 of the procedure of b64x.h) from those totals and
// the last three kept bytes.  One copy, as b64x_wrap_body.h and
// b64x_strict_body.h.  Layout: DESIGN.md §5, "k_skip_check" and
// "k_skip_decode_rows".
//
// Why the first pad character decides PAD.  Let c be the number of pad
// characters among the kept bytes u[0..E) and npad (0..2) the pads u ends in,
// D = E - npad.  u[D..E) are pad characters by the definition of npad, so
// exactly c - npad pad characters stand at kept positions below D: there is a
// PAD offence iff c > npad.  If there is one, the first pad character of the
// text stands below D too -- were it at or above D, every pad character would
// be, and c would equal npad.  So the PAD offence at the lowest offset is the
// first pad character, exactly when c > npad, and a pass needs to keep
// nothing about pads but c and that one offset.
#ifndef ASYNC_AMD_B64X_SKIP_BODY_H
#define ASYNC_AMD_B64X_SKIP_BODY_H

#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_strict_body.h"

namespace {

constexpr uint32_t kSkipTH = lines_plan::kBlockLanes;        // lanes per block (the table's builders)
constexpr uint32_t kSkipWaves = kSkipTH / lines_plan::kPassLanes;
constexpr uint32_t kChunk = 16;                              // bytes per lane
constexpr uint32_t kSkipBlocksPerCU = 8;
constexpr uint64_t kNone = ~0ull;

// A byte's class as a packed count: 16 of them sum without a carry between
// the fields (each at most 16).
constexpr uint32_t kKept = 1u;          // bits 0..4: not a skipped byte
constexpr uint32_t kPadc = 1u << 5;     // bits 5..9: the pad character (with pad)
constexpr uint32_t kStranger = 1u << 10;  // bits 10..14: kept, outside the 64, not the pad character

struct SkipSet {
    uint64_t bytes;  // byte i in bits [8 i, 8 i + 8)
    uint32_t n;
};

// What a block, a wave or a lane knows of its part of the text.
struct Slot {
    uint64_t E;           // kept bytes
    uint64_t c;           // pad characters among them
    uint64_t first_char;  // lowest offset of a stranger (kNone: none)
    uint64_t first_pad;   // lowest offset of a pad character (kNone: none)
};

static_assert(sizeof(Slot) == 32, "a slot of the workspace head");

typedef uint32_t u32x4a16 __attribute__((ext_vector_type(4), aligned(16)));

HD bool in_skip(uint32_t b, const SkipSet &k)
{
    bool hit = false;
    for (uint32_t i = 0; i < k.n; i++) hit |= ((uint32_t) (k.bytes >> (8 * i)) & 0xFFu) == b;
    return hit;
}

HD uint32_t skip_class(uint32_t b, const Alpha &a, const SkipSet &k)
{
    if (in_skip(b, k)) return 0;
    const uint32_t t = classify(b, a);
    return t < 64 ? kKept : t == 0xC0u ? kKept | kPadc : kKept | kStranger;
}

DEV void build_class_table(uint16_t *tab, const Alpha &a, const SkipSet &k)
{
    tab[threadIdx.x] = (uint16_t) skip_class(threadIdx.x, a, k);  // kSkipTH == 256
}

// ---------------------------------------------------------------- chunks --

// The 16 bytes at the 16-byte aligned address A, as far as they lie in the
// text [lo, hi): bit i of `valid` says that byte i does.  A chunk inside the
// text is one 16-byte load.  One that reaches outside is taken a dword at a
// time as far as whole dwords lie inside the text -- all of it where the text
// starts and ends at 4-byte aligned addresses -- and bytewise for the rest; the
// bytes outside are never loaded.  The loads name the global address space: an
// address that went through an integer would otherwise be loaded from as a
// flat one, and a flat load in flight counts as an LDS access too, so a wait
// for a table lookup would also wait for a chunk loaded ahead.
struct Chunk {
    uint32_t w[4];
    uint32_t valid;
};

#define B64X_GLOBAL __attribute__((address_space(1)))

DEV Chunk load_chunk(uintptr_t A, uintptr_t lo, uintptr_t hi)
{
    Chunk ch;
    if (A >= lo && A + kChunk <= hi) {
        const u32x4a16 v = __builtin_nontemporal_load((const B64X_GLOBAL u32x4a16 *) A);
        ch.w[0] = v.x;
        ch.w[1] = v.y;
        ch.w[2] = v.z;
        ch.w[3] = v.w;
        ch.valid = 0xFFFFu;
        return ch;
    }
    ch.valid = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
        const uintptr_t p = A + 4 * d;
        ch.w[d] = 0;
        if (p >= lo && p + 4 <= hi) {
            ch.w[d] = *(const B64X_GLOBAL uint32_t *) p;
            ch.valid |= 0xFu << (4 * d);
        } else if (p + 4 > lo && p < hi) {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                if (p + i >= lo && p + i < hi) {
                    ch.w[d] |= (uint32_t) *(const B64X_GLOBAL uint8_t *) (p + i) << (8 * i);
                    ch.valid |= 1u << (4 * d + i);
                }
            }
        }
    }
    return ch;
}

DEV uint32_t chunk_byte(const Chunk &ch, uint32_t i) { return (ch.w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// The chunks of a text: from the 16-byte aligned address at or below its
// first byte to the one that holds its last.
DEV uint64_t chunk_count(uintptr_t lo, uint64_t n)
{
    return n ? ((lo + n + kChunk - 1) >> 4) - (lo >> 4) : 0;
}

// Every lane of the wave leaves with the wave's totals.
DEV Slot wave_fold(Slot s)
{
#pragma unroll
    for (uint32_t d = 1; d < lines_plan::kPassLanes; d <<= 1) {
        s.E += __shfl_xor((unsigned long long) s.E, d);
        s.c += __shfl_xor((unsigned long long) s.c, d);
        const uint64_t fc = __shfl_xor((unsigned long long) s.first_char, d);
        const uint64_t fp = __shfl_xor((unsigned long long) s.first_pad, d);
        if (fc < s.first_char) s.first_char = fc;
        if (fp < s.first_pad) s.first_pad = fp;
    }
    return s;
}

// ---------------------------------------------------------- the verdict --

// The last (up to) three kept bytes of a text, the last one first, with
// their offsets.
struct Last3 {
    uint32_t byte[3];
    uint64_t off[3];
};

// Steps 2 to 6 of the procedure of b64x.h from a text's totals and its last
// min(E, 3) kept bytes.
HD b64x_strict_result skip_verdict(uint64_t n, const Slot &s, const Last3 &l, const Alpha &a)
{
    b64x_strict_result r;
    r.out_len = 0;
    r.err_pos = 0;
    r.err = B64X_STRICT_OK;
    r.reserved = 0;
    if (s.E == 0) return r;
    uint32_t npad = 0;
    if (a.pad && l.byte[0] == a.padc) npad = (s.E >= 2 && l.byte[1] == a.padc) ? 2 : 1;
    const uint64_t D = s.E - npad;
    const bool pad_offence = s.c > npad;  // then first_pad is it (the header's note)
    if (pad_offence && s.first_pad < s.first_char) {
        r.err = B64X_STRICT_PAD;
        r.err_pos = s.first_pad;
    } else if (s.first_char != kNone) {
        r.err = B64X_STRICT_CHAR;
        r.err_pos = s.first_char;
    } else if (a.pad ? (s.E & 3) != 0 : (s.E & 3) == 1) {
        r.err = B64X_STRICT_LENGTH;
        r.err_pos = n;
    } else {
        const uint32_t r4 = (uint32_t) D & 3u;
        // u[D - 1] is the kept byte npad places from the end, one of the 64.
        // Read as values first: a choice between the lvalues l.byte[i] is a
        // choice between addresses, which would need `l` to stand in memory.
        const uint32_t y0 = l.byte[0], y1 = l.byte[1], y2 = l.byte[2];
        const uint64_t f0 = l.off[0], f1 = l.off[1], f2 = l.off[2];
        const uint32_t b = npad == 0 ? y0 : npad == 1 ? y1 : y2;
        const uint64_t off = npad == 0 ? f0 : npad == 1 ? f1 : f2;
        if (D > 0 && r4 >= 2 && (classify(b, a) & (r4 == 2 ? 15u : 3u))) {
            r.err = B64X_STRICT_BITS;
            r.err_pos = off;
        } else {
            r.out_len = decoded_len(D);
        }
    }
    return r;
}

// ---------------------------------------------------------------- host --

// NULL: CR and LF.  The set's rules, in the order b64x.h states them.
inline bool make_skip(const b64x_skip *skip, const Alpha &a, SkipSet *k)
{
    static const b64x_skip crlf = {2, {'\r', '\n', 0, 0, 0, 0, 0, 0}};
    if (!skip) skip = &crlf;
    if (skip->n > 8) return false;
    k->bytes = 0;
    k->n = skip->n;
    for (uint32_t i = 0; i < skip->n; i++) {
        const uint32_t t = classify(skip->bytes[i], a);
        if (t < 64 || t == 0xC0u) return false;  // one of the 64, or the pad character (with pad)
        k->bytes |= (uint64_t) skip->bytes[i] << (8 * i);
    }
    return true;
}

inline int device_cus(uint32_t *cus)
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0) {
        const int rc = hip_status();
        return rc ? rc : -ENODEV;
    }
    *cus = (uint32_t) n;
    return 0;
}

inline uint64_t at_most(uint64_t want, uint64_t cap) { return want < cap ? want : cap; }

}  // namespace

#endif  // ASYNC_AMD_B64X_SKIP_BODY_H
