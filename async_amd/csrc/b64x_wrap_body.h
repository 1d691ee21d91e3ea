// The per-lane bodies of the line-wrapped encode, shared by b64x_wrap.hip
// (b64x_encode_lines_dev / _strided) and b64x_lines_batch.hip
// (b64x_encode_lines_batch): wrap_block() writes one 16-byte output block of a
// row's hot part, wrap_bytes() up to 16 bytes of its tail.  The structs they
// take are those of b64x_lines_plan.h.  Layout: b64x_wrap.hip's header and
// DESIGN.md §5, "k_encode_lines".
#ifndef ASYNC_AMD_B64X_WRAP_BODY_H
#define ASYNC_AMD_B64X_WRAP_BODY_H

#include "b64x_lines_dev.h"

namespace {

constexpr uint32_t kWrapTH = lines_plan::kBlockLanes;  // lanes per block: one 16-byte block each
constexpr uint32_t kWrapTile = kWrapTH * 16;            // output bytes per hot tile

// src/base64encoder.c:26-27 (62-char map) + :49-59 (62 -> pos62, 63 -> pos63)
DEV uint32_t enc_char(uint32_t v, const Alpha &a)
{
    return v < 26 ? 'A' + v
         : v < 52 ? 'a' + (v - 26)
         : v < 62 ? '0' + (v - 52)
         : v == 62 ? a.p62 : a.p63;
}

DEV void build_enc_table(uint8_t *tab, const Alpha &a)
{
    if (threadIdx.x < 64) tab[threadIdx.x] = (uint8_t) enc_char(threadIdx.x, a);
}

// 3 bytes (big-endian in bits 23..0) -> 4 characters, little-endian dword.
DEV uint32_t enc_group(const uint8_t *tab, uint32_t g)
{
    uint32_t c0 = tab[g >> 18];
    uint32_t c1 = tab[(g >> 12) & 63];
    uint32_t c2 = tab[(g >> 6) & 63];
    uint32_t c3 = tab[g & 63];
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// The hot path's splice tables, built once per block in LDS:
//   low16[x], x = 0..16: a 16-byte mask with the low x bytes set
//   sep16[x + 3], x = -3..16: the separator at bytes [x, x + s) of a 16-byte
//                 block, what falls outside dropped, zero elsewhere
constexpr uint32_t kLowRows = 17, kSepRows = 20;

DEV void build_splice_tables(uint8_t *low16, uint8_t *sep16, uint32_t sep, uint32_t s)
{
    for (uint32_t i = threadIdx.x; i < kLowRows * 16; i += kWrapTH)
        low16[i] = (i & 15) < (i >> 4) ? 0xFF : 0;
    for (uint32_t i = threadIdx.x; i < kSepRows * 16; i += kWrapTH) {
        const int32_t o = (int32_t) (i & 15) - ((int32_t) (i >> 4) - 3);
        sep16[i] = o >= 0 && o < (int32_t) s ? (uint8_t) (sep >> (8 * o)) : 0;
    }
}

// ------------------------------------------------------------ bytewise --

// Bytes [q0, q0 + cnt) of a row's wrapped text (cnt <= 16, q0 + cnt <= W),
// one at a time: a character is the sextet of its 3-byte group (loaded when
// the walk enters it; the missing bytes of the last group zero, finalize(),
// src/base64encoder.c:61-99) or the pad character past the group's real
// characters.  Gathered in registers and stored as whole dwords where the
// destination is dword aligned, the rest bytewise.
DEV void wrap_bytes(const uint8_t *tab, const uint8_t *in, uint8_t *out, uint64_t q0,
                    uint32_t cnt, const WrapArgs &w, const Alpha &a)
{
    uint64_t k = q0 / w.P;
    uint32_t c = (uint32_t) (q0 - k * w.P);
    uint64_t lo = 0, hi = 0;   // bytes 0..7, 8..15
    uint64_t cur = ~0ull;      // first byte of the group in g
    uint32_t g = 0, real = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t chars = k < w.full_lines ? w.L : w.last_len;
        uint32_t v;
        if (c < chars) {
            const uint64_t e = k * w.L + c;
            const uint64_t bi = (e >> 2) * 3;
            if (bi != cur) {
                const uint64_t rem = w.len - bi;  // >= 1
                g = (uint32_t) in[bi] << 16;
                if (rem > 1) g |= (uint32_t) in[bi + 1] << 8;
                if (rem > 2) g |= in[bi + 2];
                real = rem >= 3 ? 4u : (uint32_t) rem + 1;
                cur = bi;
            }
            const uint32_t ci = (uint32_t) e & 3u;
            v = ci < real ? tab[(g >> (18 - 6 * ci)) & 63] : a.padc;
        } else {
            v = (w.sep >> (8 * ((c - chars) & 3))) & 0xFFu;
        }
        if (i < 8) lo |= (uint64_t) v << (8 * i);
        else hi |= (uint64_t) v << (8 * (i - 8));
        if (++c == w.P) {
            c = 0;
            k++;
        }
    }
    uint8_t *dst = out + q0;
    const uint32_t nd = (((uintptr_t) dst) & 3) == 0 ? cnt >> 2 : 0;
    if (nd > 0) ((uint32_t *) dst)[0] = (uint32_t) lo;
    if (nd > 1) ((uint32_t *) dst)[1] = (uint32_t) (lo >> 32);
    if (nd > 2) ((uint32_t *) dst)[2] = (uint32_t) hi;
    if (nd > 3) ((uint32_t *) dst)[3] = (uint32_t) (hi >> 32);
#pragma unroll 1
    for (uint32_t i = 4 * nd; i < cnt; i++)
        dst[i] = (uint8_t) ((i < 8 ? lo : hi) >> (8 * (i & 7)));
}

// ----------------------------------------------------------------- hot --

// One hot block: 16 bytes at row offset 16 j, whose line is k and column c0.
// IDX is uint32_t when every position of the call fits in 32 bits.
template <typename IDX>
DEV void wrap_block(const uint8_t *tab, const uint4 *low16, const uint4 *sep16,
                    const uint8_t *rin, uint8_t *dst, IDX k, uint32_t c0, const WrapArgs &w)
{
    const int32_t jS = (int32_t) w.L - (int32_t) c0;  // block byte of the separator
    const bool pre = jS > 0;                          // the block starts with characters
    const IDX v = k * (IDX) w.L + c0;
    // the block's first character: v, or the next line's first, (k + 1) L = v + jS
    const IDX eF = pre ? v : v - (IDX) (uint32_t) (-jS);
    const uint32_t r = pre ? (c0 & 3u) : 0u;          // eF mod 4 (L is a multiple of 4)
    const int32_t d_post = pre ? (int32_t) r - (int32_t) w.s : -jS - (int32_t) w.s;
    const IDX bo = (eF >> 2) * 3;                     // first byte of eF's group
    const uint8_t *wp = rin + (bo & ~(IDX) 3);
    const uint32_t al = (uint32_t) bo & 3u;
    const u32x4a4 w0 = __builtin_nontemporal_load((const u32x4a4 *) wp);
    const uint32_t w4 = __builtin_nontemporal_load((const uint32_t *) (wp + 16));
    // the 15 bytes of groups 0..4 from byte 0 of x
    const uint32_t x = __builtin_amdgcn_alignbyte(w0.y, w0.x, al);
    const uint32_t y = __builtin_amdgcn_alignbyte(w0.z, w0.y, al);
    const uint32_t z = __builtin_amdgcn_alignbyte(w0.w, w0.z, al);
    const uint32_t u = __builtin_amdgcn_alignbyte(w4, w0.w, al);
    // v_perm_b32 selectors: byte i of the result picks byte sel[i] of
    // {S0:S1} (0-3 = S1, 4-7 = S0, 0x0c = zero).
    uint32_t C[5];
    C[0] = enc_group(tab, __builtin_amdgcn_perm(0u, x, 0x0c000102u));  // in0 in1 in2
    C[1] = enc_group(tab, __builtin_amdgcn_perm(y, x, 0x0c030405u));   // in3 in4 in5
    C[2] = enc_group(tab, __builtin_amdgcn_perm(z, y, 0x0c020304u));   // in6 in7 in8
    C[3] = enc_group(tab, __builtin_amdgcn_perm(0u, z, 0x0c010203u));  // in9 in10 in11
    C[4] = enc_group(tab, __builtin_amdgcn_perm(0u, u, 0x0c000102u));  // in12 in13 in14
    // Block byte j is C[j + r] before the separator and C[j + d_post] after
    // it (d_post in -4..2; a byte after the separator never reaches below
    // C[0]): two byte-funnels of C, merged under byte masks.
    const bool back = d_post < 0;
    const uint32_t bp = (uint32_t) d_post & 3u;
    // byte masks and the separator in place, from the block's LDS tables
    const int32_t je = jS + (int32_t) w.s;
    const uint4 mp4 = low16[jS < 0 ? 0 : jS > 16 ? 16 : jS];      // bytes before the separator
    const uint4 ms4 = low16[je < 0 ? 0 : je > 16 ? 16 : je];      // ... and the separator's
    const uint4 sp4 = sep16[jS > 16 ? 19 : jS + 3];               // jS >= -3
    const uint32_t m_pre[4] = {mp4.x, mp4.y, mp4.z, mp4.w};
    const uint32_t m_sep[4] = {ms4.x, ms4.y, ms4.z, ms4.w};
    const uint32_t sp[4] = {sp4.x, sp4.y, sp4.z, sp4.w};
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t before = __builtin_amdgcn_alignbyte(C[d + 1], C[d], r);
        const uint32_t hi = back ? C[d] : C[d + 1];
        const uint32_t lo = back ? (d > 0 ? C[d > 0 ? d - 1 : 0] : 0u) : C[d];
        const uint32_t after = __builtin_amdgcn_alignbyte(hi, lo, bp);
        o[d] = (before & m_pre[d]) | sp[d] | (after & ~m_sep[d]);
    }
    __builtin_nontemporal_store(u32x4a4{o[0], o[1], o[2], o[3]}, (u32x4a4 *) dst);
}

}  // namespace

#endif  // ASYNC_AMD_B64X_WRAP_BODY_H
