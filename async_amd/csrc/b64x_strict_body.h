// The per-lane bodies of the strict decode, shared by b64x_strict.hip
// (b64x_decode_strict_dev / _strided) and b64x_lines_batch.hip
// (b64x_decode_strict_batch): strict_lane() decodes and checks 16 characters
// of a row's hot part, strict_bytes() up to 16 characters of its tail as the
// scalar procedure of b64x.h states it.  The structs they take are those of
// b64x_lines_plan.h.  Layout: b64x_strict.hip's header and DESIGN.md §5,
// "k_decode_strict".
#ifndef ASYNC_AMD_B64X_STRICT_BODY_H
#define ASYNC_AMD_B64X_STRICT_BODY_H

#include <string.h>

#include "b64x.h"
#include "b64x_lines_dev.h"

namespace {

constexpr uint32_t kStrictTH = lines_plan::kBlockLanes;  // lanes per block
constexpr uint32_t kLaneChars = 16;                  // characters per lane (12 bytes out)
constexpr uint32_t kTileChars = kStrictTH * kLaneChars;
constexpr uint64_t kNoKey = ~0ull;

// ------------------------------------------------------------ primitives --

HD uint32_t align_byte(uint32_t hi, uint32_t lo, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
    return (uint32_t) ((((uint64_t) hi << 32) | lo) >> (8 * (n & 3)));
#endif
}

// v_perm_b32: byte i of the result is byte sel[i] of {S0:S1} (0-3 = s1, 4-7 = s0).
HD uint32_t perm_bytes(uint32_t s0, uint32_t s1, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(s0, s1, sel);
#else
    const uint64_t src = ((uint64_t) s0 << 32) | s1;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r |= (uint32_t) ((src >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return r;
#endif
}

HD uint32_t mul_hi32(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t) (((uint64_t) a * b) >> 32);
#endif
}

HD uint64_t mul_hi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t) (((unsigned __int128) a * b) >> 64);
#endif
}

// Lower the row's key (the record's err_pos field, all ones before the call).
HD void key_min(uint64_t *key, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin((unsigned long long *) key, (unsigned long long) v);
#else
    if (v < *key) *key = v;
#endif
}

// 12 bytes at a dword-aligned address: one non-temporal dwordx3 store.
HD void store12(uint8_t *dst, uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    u32x3a4 o;
    o.x = a;
    o.y = b;
    o.z = c;
    __builtin_nontemporal_store(o, (u32x3a4 *) dst);
#else
    const uint32_t o[3] = {a, b, c};
    memcpy(dst, o, 12);
#endif
}

HD uint64_t make_key(uint64_t off, uint32_t kind) { return (off << 3) | kind; }

// byte -> sextet; 0x80: not one of the 64; 0xC0: the pad character (with pad)
HD uint32_t classify(uint32_t b, const Alpha &a)
{
    if (b - 'A' < 26u) return b - 'A';
    if (b - 'a' < 26u) return b - 'a' + 26;
    if (b - '0' < 10u) return b - '0' + 52;
    if (b == a.p62) return 62;
    if (b == a.p63) return 63;
    return a.pad && b == a.padc ? 0xC0u : 0x80u;
}

// D: the row's data characters, E less the 0..2 pad characters it ends in
// (both characters loaded at once: their offsets come with the call).
HD uint64_t data_chars(const uint8_t *rin, const StrictArgs &w)
{
    if (!w.a.pad || w.E < 2) return w.E;
    const uint32_t c1 = rin[w.off_e1], c2 = rin[w.off_e2];
    if (c1 != w.a.padc) return w.E;
    return c2 == w.a.padc ? w.E - 2 : w.E - 1;
}

HD uint64_t decoded_len(uint64_t D)
{
    const uint32_t r4 = (uint32_t) D & 3u;
    return D / 4 * 3 + (r4 ? r4 - 1 : 0);
}

// ------------------------------------------------------------ bytewise --

// A lane's bytes of text in registers: 10 dwords from the dword-aligned
// address at or below the lane's first byte (3 bytes of slack, 16 characters
// and up to 5 separators of 4 bytes).  Whole dwords are loaded where they lie
// inside the row, single bytes at its edges: nothing outside the row is read,
// and a lane costs a handful of memory requests instead of one per byte.
constexpr uint32_t kSpanDwords = 10;

HD void load_span(uint32_t (&d)[kSpanDwords], const uint8_t *rin, uint64_t off0, uint64_t end,
                  uint64_t W, uint32_t *al)
{
    const uint8_t *p0 = rin + off0;
    *al = (uint32_t) ((uintptr_t) p0 & 3);
    const uint8_t *ab = p0 - *al;
#pragma unroll
    for (uint32_t q = 0; q < kSpanDwords; q++) {
        const uint8_t *lo = ab + 4 * q;
        uint32_t v = 0;
        if (lo < rin + end) {
            if (lo >= rin && lo + 4 <= rin + W) {
                v = *(const uint32_t *) lo;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 4; i++)
                    if (lo + i >= p0 && lo + i < rin + end) v |= (uint32_t) lo[i] << (8 * i);
            }
        }
        d[q] = v;
    }
}

HD uint32_t span_byte(const uint32_t (&d)[kSpanDwords], uint32_t p)
{
    const uint32_t i = p >> 2;
    uint32_t v = d[0];
#pragma unroll
    for (uint32_t q = 1; q < kSpanDwords; q++) v = i == q ? d[q] : v;
    return (v >> (8 * (p & 3))) & 0xFFu;
}

// Characters [16 jl, min(16 jl + 16, E)) of a row, one at a time, as the
// scalar procedure of b64x.h states it: each character's class, the unused
// bits of character D - 1, the separator after a line's last character and
// after character E - 1 (with trailing).  Whole groups give 3 bytes, the
// row's last group 1 or 2; gathered in registers and stored as whole dwords
// where the destination is dword aligned, the rest bytewise.  No alignment
// assumed.  The lane that owns character E - 1 leaves the row's out_len in
// its record.
HD void strict_bytes(const uint8_t *tab, const uint8_t *rin, uint8_t *rout,
                     b64x_strict_result *rec, uint64_t jl, const StrictArgs &w)
{
    const uint64_t D = data_chars(rin, w);
    const uint64_t ea = jl * kLaneChars;
    const uint32_t cnt = w.E - ea < kLaneChars ? (uint32_t) (w.E - ea) : kLaneChars;
    // 32-bit division where the row allows it
    const uint64_t k0 = !w.s ? 0 : (w.E >> 32) ? ea / w.L : (uint32_t) ea / w.L;
    const uint32_t c0 = w.s ? (uint32_t) (ea - k0 * w.L) : 0;
    const uint64_t off0 = w.s ? k0 * w.P + c0 : ea;
    // the lane's text: its characters, the separators between and behind them
    const uint32_t wraps = w.s ? (c0 + cnt - 1) / w.L : 0;
    uint64_t end = off0 + cnt + wraps * w.s + w.s;
    if (end > w.W) end = w.W;
    uint32_t d[kSpanDwords], al;
    load_span(d, rin, off0, end, w.W, &al);
    uint64_t off = off0, best = kNoKey, olo = 0;
    uint32_t c = c0, v = 0, n = 0, ohi = 0, nout = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < cnt; i++) {
        const uint64_t e = ea + i;
        if (e < D) {
            const uint32_t t = tab[span_byte(d, (uint32_t) (off - off0) + al)];
            const uint32_t r = (uint32_t) D & 3u;
            uint64_t cand = kNoKey;
            if (t & 0x80u)
                cand = make_key(off, (t & 0x40u) ? B64X_STRICT_PAD : B64X_STRICT_CHAR);
            else if (e == D - 1 && r >= 2 && (t & (r == 2 ? 15u : 3u)))
                cand = make_key(off, B64X_STRICT_BITS);
            if (cand < best) best = cand;
            v = (v << 6) | (t & 63u);
            n++;
        }
        off++;
        c++;
        const bool last = e == w.E - 1;
        if (w.s && (last ? w.trailing != 0 : c == w.L)) {
            uint32_t got = 0;
            for (uint32_t q = 0; q < w.s; q++)
                got |= span_byte(d, (uint32_t) (off - off0) + al + q) << (8 * q);
            const uint32_t diff = got ^ w.sep;
            if (diff) {  // the separator's first wrong byte
                uint32_t q = 0;
                while (((diff >> (8 * q)) & 0xFFu) == 0) q++;
                const uint64_t cand = make_key(off + q, B64X_STRICT_SEP);
                if (cand < best) best = cand;
            }
        }
        if (w.s && c == w.L) {
            c = 0;
            off += w.s;
        }
        if ((e & 3) == 3 || last) {
            // 3, 2 or 1 bytes of this group behind the lane's earlier ones
            const uint32_t nb = n == 4 ? 3 : n == 3 ? 2 : n == 2 ? 1 : 0;
            const uint32_t g = n == 4 ? v : n == 3 ? v << 6 : v << 12;  // 24 bits, left-aligned
            for (uint32_t q = 0; q < nb; q++) {
                const uint32_t byte = (g >> (16 - 8 * q)) & 0xFFu;
                if (nout < 8) olo |= (uint64_t) byte << (8 * nout);
                else ohi |= byte << (8 * (nout - 8));
                nout++;
            }
            v = 0;
            n = 0;
        }
    }
    uint8_t *dst = rout + jl * 12;
    const uint32_t nd = (((uintptr_t) dst) & 3) == 0 ? nout >> 2 : 0;
    if (nd > 0) ((uint32_t *) dst)[0] = (uint32_t) olo;
    if (nd > 1) ((uint32_t *) dst)[1] = (uint32_t) (olo >> 32);
    if (nd > 2) ((uint32_t *) dst)[2] = ohi;
#pragma unroll 1
    for (uint32_t i = 4 * nd; i < nout; i++)
        dst[i] = (uint8_t) (i < 8 ? olo >> (8 * i) : (uint64_t) ohi >> (8 * (i - 8)));
    if (ea + cnt == w.E) rec->out_len = decoded_len(D);
    if (best != kNoKey) key_min(&rec->err_pos, best);
}

// ----------------------------------------------------------------- hot --

// 4 characters (little-endian dword) -> 24 bits; the OR of the lookups to *acc.
HD uint32_t dec_group(const uint8_t *tab, uint32_t cw, uint32_t *acc)
{
    const uint32_t t0 = tab[cw & 0xFFu];
    const uint32_t t1 = tab[(cw >> 8) & 0xFFu];
    const uint32_t t2 = tab[(cw >> 16) & 0xFFu];
    const uint32_t t3 = tab[cw >> 24];
    *acc |= t0 | t1 | t2 | t3;
    return (t0 << 18) | (t1 << 12) | (t2 << 6) | t3;
}

// One hot lane: the 16 characters from row offset p0 (line column c), all of
// them data characters below D - 1, with the lane's window inside the row.
template <bool WRAP>
HD void strict_lane(const uint8_t *tab, const uint8_t *rin, uint8_t *dst, uint64_t *key,
                    uint64_t p0, uint32_t c, const StrictArgs &w)
{
    uint32_t C[4];
    uint32_t jS = 64;      // lane byte of the separator (none: beyond the lane)
    uint32_t sepbad = 0;
    if (WRAP) {
        const uint8_t *wp = rin + (p0 & ~(uint64_t) 3);
        const uint32_t al = (uint32_t) p0 & 3u;
        const u32x4a4 w0 = __builtin_nontemporal_load((const u32x4a4 *) wp);
        const u32x2a4 w1 = __builtin_nontemporal_load((const u32x2a4 *) (wp + 16));
        // the 20 bytes from p0 on
        const uint32_t x0 = align_byte(w0.y, w0.x, al);
        const uint32_t x1 = align_byte(w0.z, w0.y, al);
        const uint32_t x2 = align_byte(w0.w, w0.z, al);
        const uint32_t x3 = align_byte(w1.x, w0.w, al);
        const uint32_t x4 = align_byte(w1.y, w1.x, al);
        jS = w.L - c;                     // a multiple of 4, >= 4
        const uint32_t gs = jS >> 2;      // groups before the separator
        // group g after the separator: the bytes s further on
        const uint32_t sh = w.s & 3u;
        const uint32_t y0 = sh ? align_byte(x1, x0, sh) : x1;
        const uint32_t y1 = sh ? align_byte(x2, x1, sh) : x2;
        const uint32_t y2 = sh ? align_byte(x3, x2, sh) : x3;
        const uint32_t y3 = sh ? align_byte(x4, x3, sh) : x4;
        C[0] = x0;                        // gs >= 1
        C[1] = 1 < gs ? x1 : y1;
        C[2] = 2 < gs ? x2 : y2;
        C[3] = 3 < gs ? x3 : y3;
        (void) y0;
        if (gs <= 4) {
            const uint32_t sd = gs == 1 ? x1 : gs == 2 ? x2 : gs == 3 ? x3 : x4;
            sepbad = (sd ^ w.sep) & w.sep_mask;
        }
    } else {
        const u32x4a4 w0 = __builtin_nontemporal_load((const u32x4a4 *) (rin + p0));
        C[0] = w0.x;
        C[1] = w0.y;
        C[2] = w0.z;
        C[3] = w0.w;
    }
    uint32_t acc = 0;
    const uint32_t v0 = dec_group(tab, C[0], &acc);
    const uint32_t v1 = dec_group(tab, C[1], &acc);
    const uint32_t v2 = dec_group(tab, C[2], &acc);
    const uint32_t v3 = dec_group(tab, C[3], &acc);
    // 12 bytes: v0's bits 23..16, 15..8, 7..0, then v1's, ...
    store12(dst, perm_bytes(v1, v0, 0x06000102u), perm_bytes(v2, v1, 0x05060001u),
            perm_bytes(v3, v2, 0x04050600u));
    if (((acc & 0x80u) | sepbad) == 0) return;
    // Something is wrong in this lane's bytes: the first bad character (the
    // lowest offset among the characters) against the first bad separator byte.
    uint64_t best = kNoKey;
    bool found = false;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        const uint32_t t = tab[(C[i >> 2] >> (8 * (i & 3))) & 0xFFu];
        if (!found && (t & 0x80u)) {
            found = true;
            best = make_key(p0 + i + (i >= jS ? w.s : 0u),
                            (t & 0x40u) ? B64X_STRICT_PAD : B64X_STRICT_CHAR);
        }
    }
    if (WRAP && sepbad) {
        uint32_t q = 0;
        while (((sepbad >> (8 * q)) & 0xFFu) == 0) q++;
        const uint64_t cand = make_key(p0 + jS + q, B64X_STRICT_SEP);
        if (cand < best) best = cand;
    }
    key_min(key, best);
}

// One row's record from its key; out_len is there already (strict_bytes).
HD void finish_record(b64x_strict_result *r)
{
    const uint64_t key = r->err_pos;
    if (key != kNoKey) {
        r->out_len = 0;
        r->err_pos = key >> 3;
        r->err = (uint32_t) key & 7u;
    } else {
        r->err_pos = 0;
        r->err = B64X_STRICT_OK;
    }
    r->reserved = 0;
}

DEV void build_dec_table(uint8_t *tab, const Alpha &a)
{
    tab[threadIdx.x] = (uint8_t) classify(threadIdx.x, a);  // kStrictTH == 256
}

}  // namespace

#endif  // ASYNC_AMD_B64X_STRICT_BODY_H
