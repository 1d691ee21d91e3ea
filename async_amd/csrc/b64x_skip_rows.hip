// Strict decode of uniform rows that skips a small set of bytes, in one pass
// (include/b64x.h, b64x_decode_strict_skip_strided): the text of a row is read
// once, by the wave that owns the row, which compacts the kept characters and
// decodes them itself.  A translation unit and a code object of its own,
// linked after b64x_skip.o; no kernel of the other units is touched.
//
// Layout ("k_skip_decode_rows").  Wave g of G takes rows g,
// g + G, ...  A row is cut into 16-byte chunks at 16-byte aligned *addresses*
// (b64x_skip_body.h), a chunk to a lane, so the wave walks forward in passes
// of 1,024 bytes; the first and the last chunk go through the bounds-checked
// load.  A pass:
//   classify  a 256-entry LDS table gives each byte its sextet and its class as
//             a packed count (kept / pad character / stranger), so a lane sums
//             its 16 entries; the few lanes that hold a pad character or a
//             stranger are looked at one by one, wave-uniformly, for c and the
//             lowest offset of each.
//   place     the inclusive prefix sum of the lanes' data-character counts
//             across the wave (shuffles), less the lane's own count, on top of
//             the sextets carried over: the index of the lane's first sextet.
//   compact   each lane puts its sextets at those indices into the wave's own
//             LDS buffer (1,024 + the carry); a byte that is no sextet goes to
//             a spare byte of the lane's, so that no store is conditional.
//   decode    behind wave_lds_order() -- program order is all a wave needs
//             for its own LDS -- lane u reads unit u (16 sextets, one 16-byte
//             LDS read), packs it to 12 bytes and stores them with one
//             12-byte store, whatever the row's alignment: global accesses
//             need none on gfx950, and a dword-aligned row gets dword-aligned
//             stores.
//   carry     the 0..15 sextets behind the last whole unit move to the front
//             of the buffer.  Units, not groups of 4, so that every store of
//             an aligned row stays dword aligned from pass to pass.
// The wave also carries the last three kept bytes with their offsets (the
// verdict's npad, D and u[D - 1]), so nothing is walked backwards: a pass
// with kept bytes in three lanes or more is held back in registers and looked
// through only if no later pass takes its place.  After the
// last pass the carry gives 0..11 bytes, stored bytewise, and lane 0 writes
// the record whole.  Bytes are written before the verdict is known; the count
// of data characters never exceeds the row's length, so they stay inside the
// row's capacity whatever the row holds.
//
// No workspace, no atomic, no dependency between waves: the kernel's only
// block barrier stands behind the table.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_skip_walk.h"

namespace {

// Wave g of G takes rows g, g + G, ...
template <bool DECODE>
__global__ __launch_bounds__(kSkipTH) void k_skip_decode_rows(
    const uint8_t *__restrict__ in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
    uint8_t *__restrict__ out, uint64_t out_stride, b64x_strict_result *__restrict__ res, Alpha a,
    SkipSet k)
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
    for (uint64_t b = (uint64_t) blockIdx.x * kSkipWaves + wv; b < nbuf; b += waves) {
        const uint8_t *rin = in + b * in_stride;
        uint8_t *rout = DECODE ? out + b * out_stride : nullptr;
        const uintptr_t lo = (uintptr_t) rin, hi = lo + len;
        const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
        const uint64_t base0 = (uint64_t) (A0 - lo);  // the row offset of chunk 0's byte 0 (wraps)
        const uint64_t chunks = chunk_count(lo, len);
        uint64_t kept_here = 0;  // this lane's kept bytes; summed behind the last pass
        // pad characters and the first offences: the wave's, the same in every lane
        Slot s = {0, 0, kNone, kNone};
        Tail tl = {0, 0, 0, 0, 0, 0};
        // The last pass with kept bytes in three lanes or more: its last three
        // kept bytes are the text's so far, and are looked for only when no
        // later pass takes its place.
        Chunk pend = {};
        uint64_t pend_q0 = 0;
        bool pending = false;
        uint32_t carry = 0;  // sextets at the front of sx, < kUnit
        uint64_t units = 0;  // units stored so far
        Chunk next = {};
        if (lane < chunks) next = load_chunk(A0 + kChunk * lane, lo, hi);
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
        if (DECODE) {
            // the carry's whole groups and the row's last, partial one: byte i of them
            // comes from two neighbouring sextets; decoded_len(carry) <= 11 bytes
            const uint32_t nbytes = (uint32_t) decoded_len(carry);
            if (lane < nbytes) {
                const uint32_t g = lane / 3, r = lane % 3;
                const uint32_t x = sx[4 * g + r], y = sx[4 * g + r + 1];
                const uint32_t byte = r == 0 ? (x << 2) | (y >> 4) : r == 1 ? (x << 4) | (y >> 2) : (x << 6) | y;
                rout[12 * units + lane] = (uint8_t) byte;
            }
            wave_lds_order();  // the next row's sextets come after these reads
        }
        if (pending) tail_of_pass(tab, pend, base0 + kChunk * pend_q0, lane, &tl);
#pragma unroll
        for (uint32_t d = 1; d < kLanes; d <<= 1)
            kept_here += __shfl_xor((unsigned long long) kept_here, d);
        s.E = kept_here;
        const Last3 last = {{tl.b0, tl.b1, tl.b2}, {tl.o0, tl.o1, tl.o2}};
        const b64x_strict_result r = skip_verdict(len, s, last, a);
        if (lane == 0) res[b] = r;
    }
}

}  // namespace

extern "C" {

int b64x_decode_strict_skip_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                                    void *d_out, uint64_t out_stride, b64x_strict_result *d_res,
                                    const b64x_alphabet *abc, const b64x_skip *skip, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_res || (((uintptr_t) d_res) & 7)) return -EINVAL;
    if (in_stride < len) return -EINVAL;
    if (d_out && out_stride < b64x_decoded_cap(len)) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    SkipSet k;
    if (!make_skip(skip, a, &k)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t cus = 0;
    if ((rc = device_cus(&cus)) != 0) return rc;
    const uint64_t want = ((uint64_t) nbuf + kSkipWaves - 1) / kSkipWaves;
    const uint32_t grid = (uint32_t) at_most(want, (uint64_t) cus * kSkipBlocksPerCU);
    const hipStream_t st = (hipStream_t) stream;
    if (d_out)
        hipLaunchKernelGGL(k_skip_decode_rows<true>, dim3(grid), dim3(kSkipTH), 0, st,
                           (const uint8_t *) d_in, in_stride, len, nbuf, (uint8_t *) d_out, out_stride,
                           d_res, a, k);
    else
        hipLaunchKernelGGL(k_skip_decode_rows<false>, dim3(grid), dim3(kSkipTH), 0, st,
                           (const uint8_t *) d_in, in_stride, len, nbuf, (uint8_t *) nullptr,
                           (uint64_t) 0, d_res, a, k);
    return hip_status();
}

}  // extern "C"
