// Strict skip decode of texts that arrive in pieces (include/b64x.h,
// b64x_decode_strict_skip_pieces): many streams in one launch, each with a
// state of 128 bytes in device memory and one piece of its text, read once by
// the wave that owns it.  A translation unit and a code object of its own,
// linked after b64x_skip_rows.o; no kernel of the other units is touched.
//
// Layout ("k_skip_decode_pieces").  The walk is that of
// k_skip_decode_rows (b64x_skip_walk.h): wave g of G takes pieces g, g + G,
// ..., a chunk of 16 bytes at an aligned address to a lane, passes of 1,024
// bytes with the next one loaded ahead, the 256-entry table behind the unit's
// only block barrier, compaction into the wave's own LDS, 12-byte stores per
// 16 sextets.  What a piece adds to a row:
//   before  the wave loads its state: the totals of the text so far, its last
//           three kept bytes with their offsets and the 0..3 sextets the
//           pieces before left over, which go to the front of the sextet
//           buffer as a pass's carry does.  Every offset is an offset in the
//           text: the row's, plus the bytes the state has taken.
//   after   a piece that is not the last emits the whole groups of the carry
//           bytewise, keeps the 0..3 sextets behind them and stores the
//           state; its verdict has the steps of the procedure that can only
//           become more true as the text grows (PAD and CHAR).  The last
//           piece emits the partial group too, takes the whole verdict and
//           zeroes the state.
//   error   a state that holds a report gives it again at once: no more than
//           the piece's first pass is loaded, nothing of it is looked at, and
//           nothing is written but the record (and, for the last piece, the
//           zeroed state).
// The state's words (all zero: the start of a text):
//   0  bytes taken, |T|            5..7  offsets of the last three kept bytes,
//   1  E, kept bytes                     the last one first
//   2  c, pad characters           8     those bytes (bits 0..23), the count of
//   3  first stranger, offset + 1        sextets left over (24..25), the
//   4  first pad character, + 1          sextets (32..55)
//   9  the report's kind (0: none), 10 its offset; 11..15 zero.
//
// No workspace, no atomic, no dependency between waves: the states of one
// call are distinct, so a state is read and written by one wave only.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_skip_walk.h"

namespace {

static_assert(sizeof(b64x_skip_state) == B64X_SKIP_STATE_BYTES, "the state of b64x.h");

// A value that is the same in every lane, as one.
DEV uint32_t uniform(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
DEV uint64_t uniform(uint64_t v)
{
    return ((uint64_t) uniform((uint32_t) (v >> 32)) << 32) | uniform((uint32_t) v);
}

// Steps 2 and 3 of the procedure of b64x.h on the text so far: the offences
// that more text cannot take back.  npad can only hide pad characters that
// the text ends in; a pad character below a data character stays an offence.
DEV b64x_strict_result verdict_so_far(const Slot &s, const Last3 &l, const Alpha &a)
{
    b64x_strict_result r;
    r.out_len = 0;
    r.err_pos = 0;
    r.err = B64X_STRICT_OK;
    r.reserved = 0;
    uint32_t npad = 0;
    if (a.pad && s.E >= 1 && l.byte[0] == a.padc) npad = (s.E >= 2 && l.byte[1] == a.padc) ? 2 : 1;
    if (s.c > npad && s.first_pad < s.first_char) {
        r.err = B64X_STRICT_PAD;
        r.err_pos = s.first_pad;
    } else if (s.first_char != kNone) {
        r.err = B64X_STRICT_CHAR;
        r.err_pos = s.first_char;
    }
    return r;
}

// Wave g of G takes pieces g, g + G, ...
template <bool DECODE>
__global__ __launch_bounds__(kSkipTH) void k_skip_decode_pieces(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t npieces,
    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, b64x_skip_state *state,
    const uint32_t *__restrict__ sid, const uint8_t *__restrict__ flags,
    b64x_strict_result *__restrict__ res, Alpha a, SkipSet k)
{
    __shared__ uint32_t tab[256];
    // a wave's sextets, and behind them a byte per lane for what is no sextet
    __shared__ __attribute__((aligned(16))) uint8_t sextets[DECODE ? kSkipWaves : 1][kSextets + kLanes];
    build_row_table(tab, a, k);
    block_sync();
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    uint8_t *const sx = sextets[DECODE ? wv : 0];
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    uint64_t b = (uint64_t) blockIdx.x * kSkipWaves + wv;
    // A piece's edges are loaded a piece ahead, and its first chunks before its
    // state is looked at: a row's address is arithmetic, a piece's is not.
    uint64_t beg = 0, end = 0;
    if (b < npieces) beg = in_off[b], end = in_off[b + 1];
    for (; b < npieces; b += waves) {
        const uint64_t len = end - beg;
        const uint8_t *rin = in + beg;
        const uintptr_t lo = (uintptr_t) rin, hi = lo + len;
        const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
        const uint64_t chunks = chunk_count(lo, len);
        Chunk next = {};
        if (lane < chunks) next = load_chunk(A0 + kChunk * lane, lo, hi);
        if (b + waves < npieces) beg = in_off[b + waves], end = in_off[b + waves + 1];
        const bool final = flags && (uniform((uint32_t) flags[b]) & B64X_PIECE_FINAL);
        uint64_t *const st = state[sid ? (uint64_t) uniform(sid[b]) : b].w;
        // a text that was refused: the same record, and the piece is not looked at
        const uint32_t kind = uniform((uint32_t) st[9]);
        if (kind != B64X_STRICT_OK) {
            b64x_strict_result r;
            r.out_len = 0;
            r.err_pos = st[10];
            r.err = kind;
            r.reserved = 0;
            if (lane == 0) res[b] = r;
            if (final && lane < 16) st[lane] = 0;
            continue;
        }
        const uint64_t pos = uniform(st[0]);  // the text offset of the piece's byte 0
        const uint64_t E0 = uniform(st[1]);
        const uint64_t fc = uniform(st[3]), fp = uniform(st[4]);
        const uint64_t w8 = uniform(st[8]);
        // pad characters and the first offences: the wave's, the same in every lane
        Slot s = {0, uniform(st[2]), fc ? fc - 1 : kNone, fp ? fp - 1 : kNone};
        const uint64_t c0 = s.c;
        Tail tl = {(uint32_t) w8 & 0xFFu, (uint32_t) (w8 >> 8) & 0xFFu, (uint32_t) (w8 >> 16) & 0xFFu,
                   uniform(st[5]), uniform(st[6]), uniform(st[7])};
        const uint32_t cin = (uint32_t) (w8 >> 24) & 3u;  // sextets the pieces before left over
        uint8_t *rout = DECODE ? out + out_off[b] : nullptr;
        const uint64_t base0 = pos + (uint64_t) (A0 - lo);  // the text offset of chunk 0's byte 0 (wraps)
        uint64_t kept_here = 0;  // this lane's kept bytes; summed behind the last pass
        // The last pass with kept bytes in three lanes or more: its last three
        // kept bytes are the text's so far, and are looked for only when no
        // later pass takes its place.
        Chunk pend = {};
        uint64_t pend_q0 = 0;
        bool pending = false;
        uint32_t carry = cin;  // sextets at the front of sx, < kUnit
        uint64_t units = 0;    // units stored so far
        if (DECODE) {
            if (lane < cin) sx[lane] = (uint8_t) (w8 >> (32 + 8 * (lane & 3u))) & 0x3Fu;
            wave_lds_order();
        }
        for (uint64_t q0 = 0; q0 < chunks; q0 += kLanes) {
            const Chunk ch = next;
            // the next pass's chunk is on its way while this one is worked on
            const uint64_t qn = q0 + kLanes + lane;
            next = Chunk{};
            if (qn < chunks) next = load_chunk(A0 + kChunk * qn, lo, hi);
            uint32_t t[kChunk];
            classify_chunk(tab, ch, t);
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t i = 0; i < kChunk; i++) sum += t[i];
            const uint32_t nkept = (sum >> kCntShift) & 31u, npadc = (sum >> kPadShift) & 31u,
                           nstranger = (sum >> kStrangerShift) & 31u;
            kept_here += nkept;
            // pad characters and strangers are few: the lanes that hold some, one by one
            for (uint64_t rest = __ballot((npadc | nstranger) != 0); rest; rest &= rest - 1) {
                const uint32_t l = (uint32_t) __builtin_ctzll(rest);
                uint32_t pm = 0, sm = 0;
#pragma unroll
                for (uint32_t i = 0; i < kChunk; i++) {
                    const uint32_t ti = (uint32_t) __builtin_amdgcn_readlane((int) t[i], (int) l);
                    pm |= ((ti >> kPadShift) & 1u) << i;
                    sm |= ((ti >> kStrangerShift) & 1u) << i;
                }
                const uint64_t off = base0 + kChunk * (q0 + l);
                s.c += (uint32_t) __popc(pm);
                if (pm && s.first_pad == kNone) s.first_pad = off + (uint32_t) __builtin_ctz(pm);
                if (sm && s.first_char == kNone) s.first_char = off + (uint32_t) __builtin_ctz(sm);
            }
            if (__popcll(__ballot(nkept != 0)) >= 3) {
                pend = ch;
                pend_q0 = q0;
                pending = true;
            } else {
                if (pending) tail_of_pass(tab, pend, base0 + kChunk * pend_q0, lane, &tl);
                pending = false;
                tail_of_pass(tab, ch, base0 + kChunk * q0, lane, &tl);
            }
            if (!DECODE) continue;
            // place: this lane's data characters behind those of the lanes below
            const uint32_t mine = nkept - npadc - nstranger;
            uint32_t incl = mine;
#pragma unroll
            for (uint32_t d = 1; d < kLanes; d <<= 1) {
                const uint32_t up = (uint32_t) __shfl_up((int) incl, d);
                if (lane >= d) incl += up;
            }
            const uint32_t total = carry + (uint32_t) __shfl((int) incl, (int) (kLanes - 1));
            // compact: a sextet to its place, anything else to the lane's spare byte
            uint32_t at = carry + incl - mine;
            const uint32_t spare = kSextets + lane;
#pragma unroll
            for (uint32_t i = 0; i < kChunk; i++) {
                const bool is_data = (int32_t) t[i] < 0;
                sx[is_data ? at : spare] = (uint8_t) t[i];
                at += is_data;
            }
            wave_lds_order();
            // decode: a unit to a lane, at most 64 of them (total < 1,024 + 16)
            const uint32_t whole = total / kUnit;
            carry = total % kUnit;
            if (lane < whole) {
                const u32x4 v = *(const u32x4 *) (sx + kUnit * lane);
                const uint32_t v0 = pack_group(v.x), v1 = pack_group(v.y), v2 = pack_group(v.z),
                               v3 = pack_group(v.w);
                const uint32_t o0 = perm_bytes(v1, v0, 0x06000102u), o1 = perm_bytes(v2, v1, 0x05060001u),
                               o2 = perm_bytes(v3, v2, 0x04050600u);
                // 12 bytes at any alignment, as one store (global accesses need none)
                u32x3a1 o;
                o.x = o0;
                o.y = o1;
                o.z = o2;
                __builtin_nontemporal_store(o, (u32x3a1 *) (rout + 12 * (units + lane)));
            }
            units += whole;
            // carry: what stands behind the last whole unit moves to the front
            const uint32_t left = lane < carry ? sx[kUnit * whole + lane] : 0u;
            wave_lds_order();
            if (lane < carry) sx[lane] = (uint8_t) left;
            wave_lds_order();
        }
        uint64_t w8n = 0;  // the sextets a piece that is not the last leaves over
        if (DECODE) {
            // the carry's whole groups and, for the last piece, the text's partial one:
            // byte i of them comes from two neighbouring sextets; at most 11 bytes
            const uint32_t nbytes = final ? (uint32_t) decoded_len(carry) : carry / 4 * 3;
            if (lane < nbytes) {
                const uint32_t g = lane / 3, r = lane % 3;
                const uint32_t x = sx[4 * g + r], y = sx[4 * g + r + 1];
                const uint32_t byte = r == 0 ? (x << 2) | (y >> 4) : r == 1 ? (x << 4) | (y >> 2) : (x << 6) | y;
                rout[12 * units + lane] = (uint8_t) byte;
            }
            const uint32_t g4 = carry & ~3u, keep = carry & 3u;
            const uint32_t mine = lane < keep ? sx[g4 + lane] : 0u;
            w8n = ((uint64_t) uniform((uint32_t) __shfl((int) mine, 0))) << 32 |
                  ((uint64_t) uniform((uint32_t) __shfl((int) mine, 1))) << 40 |
                  ((uint64_t) uniform((uint32_t) __shfl((int) mine, 2))) << 48;
            wave_lds_order();  // the next piece's sextets come after these reads
        }
        if (pending) tail_of_pass(tab, pend, base0 + kChunk * pend_q0, lane, &tl);
#pragma unroll
        for (uint32_t d = 1; d < kLanes; d <<= 1)
            kept_here += __shfl_xor((unsigned long long) kept_here, d);
        s.E = E0 + kept_here;
        // Without an offence every kept byte is a data character or a pad
        // character, so this is the carry and the piece's data characters: in
        // a decoding call 16 units + carry.
        const uint64_t kd = cin + kept_here - (s.c - c0);
        const Last3 last = {{tl.b0, tl.b1, tl.b2}, {tl.o0, tl.o1, tl.o2}};
        b64x_strict_result r;
        if (final) {
            r = skip_verdict(pos + len, s, last, a);
            if (r.err == B64X_STRICT_OK) r.out_len = decoded_len(kd);  // what this piece wrote
            if (lane < 16) st[lane] = 0;
        } else {
            r = verdict_so_far(s, last, a);
            if (r.err == B64X_STRICT_OK) r.out_len = kd / 4 * 3;
            if (lane == 0) {
                st[0] = pos + len;
                st[1] = s.E;
                st[2] = s.c;
                st[3] = s.first_char + 1;  // kNone: 0
                st[4] = s.first_pad + 1;
                st[5] = tl.o0;
                st[6] = tl.o1;
                st[7] = tl.o2;
                st[8] = tl.b0 | (tl.b1 << 8) | (tl.b2 << 16) | ((uint32_t) (kd & 3u) << 24) | w8n;
                st[9] = r.err;
                st[10] = r.err_pos;
            }
        }
        if (lane == 0) res[b] = r;
    }
}

}  // namespace

extern "C" {

uint64_t b64x_skip_piece_cap(uint64_t len) { return b64x_decoded_cap(len + 3); }

int b64x_decode_strict_skip_pieces(const void *d_in, const uint64_t *d_in_off, uint32_t npieces,
                                   void *d_out, const uint64_t *d_out_off, b64x_skip_state *d_state,
                                   const uint32_t *d_sid, const uint8_t *d_flags,
                                   b64x_strict_result *d_res, const b64x_alphabet *abc,
                                   const b64x_skip *skip, void *stream)
{
    if (npieces == 0) return 0;
    if (!d_in || !d_in_off || !d_state || !d_res) return -EINVAL;
    if ((((uintptr_t) d_res) & 7) || (((uintptr_t) d_state) & 7)) return -EINVAL;
    if (d_out && !d_out_off) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    SkipSet k;
    if (!make_skip(skip, a, &k)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t cus = 0;
    if ((rc = device_cus(&cus)) != 0) return rc;
    const uint64_t want = ((uint64_t) npieces + kSkipWaves - 1) / kSkipWaves;
    const uint32_t grid = (uint32_t) at_most(want, (uint64_t) cus * kSkipBlocksPerCU);
    const hipStream_t st = (hipStream_t) stream;
    if (d_out)
        hipLaunchKernelGGL(k_skip_decode_pieces<true>, dim3(grid), dim3(kSkipTH), 0, st,
                           (const uint8_t *) d_in, d_in_off, npieces, (uint8_t *) d_out, d_out_off,
                           d_state, d_sid, d_flags, d_res, a, k);
    else
        hipLaunchKernelGGL(k_skip_decode_pieces<false>, dim3(grid), dim3(kSkipTH), 0, st,
                           (const uint8_t *) d_in, d_in_off, npieces, (uint8_t *) nullptr,
                           (const uint64_t *) nullptr, d_state, d_sid, d_flags, d_res, a, k);
    return hip_status();
}

}  // extern "C"
