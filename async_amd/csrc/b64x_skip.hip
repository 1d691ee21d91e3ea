// Strict decode that skips a small set of bytes (CR and LF by default)
// wherever they stand, for gfx950 (include/b64x.h, b64x_decode_strict_skip_*):
// the verdict of the strict decoder on the text with those bytes taken out,
// with the kind and the offset (in the text as given) of the first offence.
// A translation unit and a code object of its own, linked after
// b64x_lines_batch.o; no kernel of the other units is touched.
//
// Layout ("k_skip_check").  The bytes of an accepted text are,
// by definition, what the lenient decoder writes for it, so the decoding call
// enqueues b64x_decode_dev / b64x_decode_batch on the caller's workspace and
// this unit adds the verdict only: a read-only pass that classifies every
// byte, and a finish step.
//
//   k_skip_check        one buffer.  The text is cut into 16-byte chunks at
//       16-byte aligned *addresses*; a lane takes a chunk with one 16-byte
//       load, a 256-lane block a tile of 4,096 bytes, the grid (CUs x 8
//       blocks at most) strides over the tiles.  The first and the last chunk
//       may reach outside the text: those are taken in whole dwords where
//       they lie inside it and bytewise for the rest, the bytes outside
//       never loaded.  A 256-entry LDS table gives each byte its
//       class as a packed count (kept / pad character / outside the 64), so a
//       lane sums its 16 lookups and looks closer only where a pad character
//       or a stranger showed.  Each lane keeps E (kept bytes), c (pad
//       characters among them), the lowest offset of a stranger and the lowest
//       offset of a pad character; the block folds them (wave shuffles, then
//       one LDS atomic each per wave) and the last wave to arrive leaves the
//       four values in the block's own slot of the workspace head.  No memset
//       node, no global atomic.
//   k_skip_finish       one wave.  Sums the slots, walks backwards from the
//       end of the text in steps of 1,024 bytes until it holds the last three
//       kept bytes and their offsets, and writes the record whole.
//   k_skip_check_batch  ragged batch, a wave per buffer (waves stride over
//       the buffers, offsets read with scalar loads): the same chunks in
//       passes of 1,024 bytes, sums and minima in the wave's registers, the
//       same backward walk, the record written whole.  No atomic at all.
//
// The skip set, the class table, the chunks, a wave's totals and the verdict
// arithmetic are b64x_skip_body.h's, shared with b64x_skip_rows.hip.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "b64x.h"
#include "b64x_skip_body.h"

namespace {

constexpr uint32_t kWalkStep = lines_plan::kPassUnits;       // bytes per backward step (one wave)
constexpr uint32_t kSkipMaxGrid = 2048;                      // slots in the workspace head

// The workspace head: a b64x_dec_result for the lenient decoder, then a slot
// per block of the largest grid.  A multiple of 256, so that the lenient
// decoder's workspace behind it is aligned as the caller's is.
constexpr uint64_t kHeadRes = 64;
constexpr uint64_t kHeadBytes = (kHeadRes + kSkipMaxGrid * sizeof(Slot) + 255) & ~255ull;

static_assert(sizeof(b64x_dec_result) <= kHeadRes, "the head's layout");

// One chunk into a lane's slot; off0: the text offset of the chunk's byte 0
// (wraps below zero for a first chunk that starts before the text, and the
// sum with a valid byte's index is its offset again).  A lane meets its
// chunks in ascending order, but the minimum is taken anyway.
DEV void scan_chunk(const uint16_t *tab, const Chunk &ch, uint64_t off0, Slot *s)
{
    uint32_t sum = 0;
    if (ch.valid == 0xFFFFu) {
#pragma unroll
        for (uint32_t i = 0; i < kChunk; i++) sum += tab[chunk_byte(ch, i)];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kChunk; i++)
            sum += ((ch.valid >> i) & 1u) ? tab[chunk_byte(ch, i)] : 0u;
    }
    s->E += sum & 31u;
    s->c += (sum >> 5) & 31u;
    if ((sum >> 5) == 0) return;
    // a pad character or a stranger among these 16: the lowest of each
    uint64_t fc = kNone, fp = kNone;
#pragma unroll
    for (uint32_t q = 0; q < kChunk; q++) {
        const uint32_t i = kChunk - 1 - q;
        const uint32_t t = ((ch.valid >> i) & 1u) ? tab[chunk_byte(ch, i)] : 0u;
        if (t & kStranger) fc = off0 + i;
        if (t & kPadc) fp = off0 + i;
    }
    if (fc < s->first_char) s->first_char = fc;
    if (fp < s->first_pad) s->first_pad = fp;
}

// ---------------------------------------------------------- the verdict --

// The last `want` (<= 3, <= E) kept bytes of the text, the last one first,
// with their offsets.  The wave walks backwards from the 16-byte boundary at
// or above the end in steps of kWalkStep bytes, a chunk to a lane; within a
// step the ballot of the lanes that still hold a kept byte names the highest
// one.  A text that ends in a long run of skipped bytes is walked at this one
// wave's rate.
DEV Last3 last_kept(uintptr_t lo, uintptr_t hi, uint32_t lane, uint32_t want, const SkipSet &k)
{
    Last3 r = {};
    uint32_t found = 0;
    uintptr_t end = (hi + kChunk - 1) & ~(uintptr_t) (kChunk - 1);
    while (found < want && end > lo) {
        const uintptr_t base = end - kWalkStep;
        const Chunk ch = load_chunk(base + kChunk * lane, lo, hi);
        uint32_t m = 0;
#pragma unroll
        for (uint32_t i = 0; i < kChunk; i++)
            if (((ch.valid >> i) & 1u) && !in_skip(chunk_byte(ch, i), k)) m |= 1u << i;
        while (found < want) {
            const uint64_t holders = __ballot(m != 0);
            if (holders == 0) break;
            const uint32_t top = 63u - (uint32_t) __clzll((long long) holders);
            const uint32_t mt = (uint32_t) __shfl((int) m, (int) top);
            const uint32_t j = 31u - (uint32_t) __clz((int) mt);
            const uint32_t word = j < 4 ? ch.w[0] : j < 8 ? ch.w[1] : j < 12 ? ch.w[2] : ch.w[3];
            const uint32_t b = ((uint32_t) __shfl((int) word, (int) top) >> (8 * (j & 3))) & 0xFFu;
            const uint64_t off = (uint64_t) (base + kChunk * top + j - lo);
#pragma unroll
            for (uint32_t q = 0; q < 3; q++)
                if (q == found) {
                    r.byte[q] = b;
                    r.off[q] = off;
                }
            found++;
            if (lane == top) m &= ~(1u << j);
        }
        end = base;
    }
    return r;
}

// Steps 2 to 6 of the procedure of b64x.h from the text's totals; every lane
// of the wave takes part and holds the same record at the end.
DEV b64x_strict_result wave_verdict(const uint8_t *in, uint64_t n, const Slot &s, uint32_t lane,
                                    const Alpha &a, const SkipSet &k)
{
    if (s.E == 0) return skip_verdict(n, s, Last3{}, a);
    return skip_verdict(
        n, s, last_kept((uintptr_t) in, (uintptr_t) in + n, lane, s.E < 3 ? (uint32_t) s.E : 3u, k), a);
}

// ------------------------------------------------------------- kernels --

// One buffer: every byte's class, the block's totals into its slot.
__global__ __launch_bounds__(kSkipTH) void k_skip_check(const uint8_t *__restrict__ in, uint64_t n,
                                                        Slot *__restrict__ slots, Alpha a,
                                                        SkipSet k)
{
    __shared__ uint16_t tab[256];
    __shared__ unsigned long long tot[4];  // E, c, first_char, first_pad of the block
    __shared__ uint32_t arrived;
    build_class_table(tab, a, k);
    if (threadIdx.x == 0) {
        tot[0] = tot[1] = 0;
        tot[2] = tot[3] = kNone;
        arrived = 0;
    }
    block_sync();
    const uintptr_t lo = (uintptr_t) in, hi = lo + n;
    const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
    const uint64_t chunks = chunk_count(lo, n);
    const uint64_t tiles = (chunks + kSkipTH - 1) / kSkipTH;
    Slot s = {0, 0, kNone, kNone};
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t q = t * kSkipTH + threadIdx.x;
        if (q < chunks) {
            const uintptr_t A = A0 + kChunk * q;
            scan_chunk(tab, load_chunk(A, lo, hi), (uint64_t) (A - lo), &s);
        }
    }
    s = wave_fold(s);
    // The block's totals: each wave adds its own with LDS atomics, then counts
    // itself in.  The counter is a release sequence: the wave that draws the
    // last ticket sees what the others added before they drew theirs.
    if (threadIdx.x % lines_plan::kPassLanes == 0) {
        __hip_atomic_fetch_add(&tot[0], (unsigned long long) s.E, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&tot[1], (unsigned long long) s.c, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_min(&tot[2], (unsigned long long) s.first_char, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_min(&tot[3], (unsigned long long) s.first_pad, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t ticket = __hip_atomic_fetch_add(&arrived, 1u, __ATOMIC_ACQ_REL,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        if (ticket == kSkipWaves - 1) {
            Slot b;
            b.E = __hip_atomic_load(&tot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            b.c = __hip_atomic_load(&tot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            b.first_char = __hip_atomic_load(&tot[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            b.first_pad = __hip_atomic_load(&tot[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            slots[blockIdx.x] = b;
        }
    }
}

// One wave: the slots' totals, the backward walk, the record.
__global__ __launch_bounds__(lines_plan::kPassLanes) void k_skip_finish(
    const uint8_t *__restrict__ in, uint64_t n, const Slot *__restrict__ slots, uint32_t nslots,
    b64x_strict_result *res, Alpha a, SkipSet k)
{
    const uint32_t lane = threadIdx.x;
    Slot s = {0, 0, kNone, kNone};
    for (uint32_t i = lane; i < nslots; i += lines_plan::kPassLanes) {
        const Slot b = slots[i];
        s.E += b.E;
        s.c += b.c;
        if (b.first_char < s.first_char) s.first_char = b.first_char;
        if (b.first_pad < s.first_pad) s.first_pad = b.first_pad;
    }
    s = wave_fold(s);
    const b64x_strict_result r = wave_verdict(in, n, s, lane, a, k);
    if (lane == 0) *res = r;
}

// Ragged batch: wave g of G takes buffers g, g + G, ...
__global__ __launch_bounds__(kSkipTH) void k_skip_check_batch(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t nbuf,
    b64x_strict_result *res, Alpha a, SkipSet k)
{
    __shared__ uint16_t tab[256];
    build_class_table(tab, a, k);
    block_sync();
    const uint32_t lane = threadIdx.x % lines_plan::kPassLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / lines_plan::kPassLanes);
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    for (uint64_t b = (uint64_t) blockIdx.x * kSkipWaves + wv; b < nbuf; b += waves) {
        const uint64_t beg = in_off[b], n = in_off[b + 1] - beg;
        const uint8_t *rin = in + beg;
        const uintptr_t lo = (uintptr_t) rin, hi = lo + n;
        const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
        const uint64_t chunks = chunk_count(lo, n);
        Slot s = {0, 0, kNone, kNone};
        // passes of kWalkStep bytes: a chunk to a lane
        for (uint64_t q = lane; q < chunks; q += lines_plan::kPassLanes) {
            const uintptr_t A = A0 + kChunk * q;
            scan_chunk(tab, load_chunk(A, lo, hi), (uint64_t) (A - lo), &s);
        }
        s = wave_fold(s);
        const b64x_strict_result r = wave_verdict(rin, n, s, lane, a, k);
        if (lane == 0) res[b] = r;
    }
}

}  // namespace

extern "C" {

uint64_t b64x_strict_skip_workspace_size(uint64_t nchars, bool validate_only)
{
    return kHeadBytes + (validate_only ? 0 : b64x_decode_workspace_size(nchars));
}

int b64x_decode_strict_skip_dev(const void *d_in, uint64_t nchars, void *d_out,
                                b64x_strict_result *d_res, const b64x_alphabet *abc,
                                const b64x_skip *skip, void *d_workspace, void *stream)
{
    if (!d_in || !d_res || !d_workspace) return -EINVAL;
    if ((((uintptr_t) d_res) | ((uintptr_t) d_workspace)) & 7) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    SkipSet k;
    if (!make_skip(skip, a, &k)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t cus = 0;
    if ((rc = device_cus(&cus)) != 0) return rc;
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *ws = (uint8_t *) d_workspace;
    Slot *slots = (Slot *) (ws + kHeadRes);
    const hipStream_t st = (hipStream_t) stream;
    // at most one chunk more than the length holds: the first may start before the text
    const uint64_t tiles = (nchars / kChunk + 2 + kSkipTH - 1) / kSkipTH;
    const uint32_t grid =
        (uint32_t) at_most(tiles, at_most((uint64_t) cus * kSkipBlocksPerCU, kSkipMaxGrid));
    hipLaunchKernelGGL(k_skip_check, dim3(grid), dim3(kSkipTH), 0, st, in, nchars, slots, a, k);
    if ((rc = hip_status()) != 0) return rc;
    hipLaunchKernelGGL(k_skip_finish, dim3(1), dim3(lines_plan::kPassLanes), 0, st, in, nchars,
                       (const Slot *) slots, grid, d_res, a, k);
    if ((rc = hip_status()) != 0) return rc;
    if (!d_out) return 0;
    // the bytes: the lenient decoder, on the rest of the caller's workspace
    return b64x_decode_dev(d_in, nchars, d_out, (b64x_dec_result *) ws, abc, 0, ws + kHeadBytes,
                           stream);
}

int b64x_decode_strict_skip_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                                  void *d_out, const uint64_t *d_out_off,
                                  b64x_strict_result *d_res, const b64x_alphabet *abc,
                                  const b64x_skip *skip, void *d_workspace, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_in_off || !d_res || (((uintptr_t) d_res) & 7)) return -EINVAL;
    if (d_out && (!d_out_off || !d_workspace || (((uintptr_t) d_workspace) & 7))) return -EINVAL;
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
    hipLaunchKernelGGL(k_skip_check_batch, dim3(grid), dim3(kSkipTH), 0, (hipStream_t) stream,
                       (const uint8_t *) d_in, d_in_off, nbuf, d_res, a, k);
    if ((rc = hip_status()) != 0) return rc;
    if (!d_out) return 0;
    return b64x_decode_batch(d_in, d_in_off, nbuf, d_out, d_out_off, (uint64_t *) d_workspace, abc,
                             stream);
}

}  // extern "C"
