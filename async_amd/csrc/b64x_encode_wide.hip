// The ragged encode, plain and line-wrapped, balanced over the batch's bytes
// and not over its buffers (include/b64x.h, b64x_encode_batch_wide): nbuf
// buffers of any lengths addressed by device-resident offsets, an 8 MiB buffer
// among 4 KiB ones spread over the device like the rest.  A translation unit
// and a code object of its own, linked after the other eight satellites; the
// wrapped form's per-lane bodies are those of the one-buffer kernels
// (b64x_wrap_body.h), one copy, the plain form's a small one of this unit.
//
// Layout ("k_encode_wide"; the arithmetic is
// b64x_encode_wide_plan.h).  in_off is monotone, so the buffers lie end to end
// in one arena.  Every wave reads its size, total = in_off[nbuf] - in_off[0],
// and takes an equal span of it; the grid comes from the host's hint and the
// device, the share from the total on the device, so the hint cannot make the
// result wrong and a captured call replays on other offsets.  For its span a
// wave
//   1. finds the first buffer that ends after the span's start: one binary
//      search over in_off with scalar loads;
//   2. walks forward while buffers start before the span's end (a run of
//      empty buffers costs a second search, not a load each).  Per buffer it
//      runs the prologue of b64x_lines_plan.h (or plain_plan) and turns the
//      part of the buffer inside the span into a range of 16-byte output
//      blocks, [cut(a), cut(z)): every block has exactly one owner;
//   3. writes the owned blocks below hot_blocks in passes of 64 lanes (dword
//      loads, v_perm, table lookups; the wrapped pass's line and column come
//      from one division at the range's first block and additions from
//      there), the others bytewise.  Whether a buffer is dword aligned on
//      both sides decides that for the whole of it, wave-uniform.
// No workspace, no atomic, one launch.  A block whose waves own nothing
// leaves before it builds its tables.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_encode_wide_plan.h"
#include "b64x_wrap_body.h"

namespace {

using lines_plan::Call;
using lines_plan::kPassLanes;

constexpr uint32_t kWideTH = enc_wide_plan::kBlockLanes;
constexpr uint32_t kWideWaves = enc_wide_plan::kBlockWaves;

static_assert(kWideTH == kWrapTH, "the table builders' block size");

// The wave's index in the block, as the scalar it is.
DEV uint32_t wave_in_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x / kPassLanes); }

// The first buffer that ends after arena position pos; nbuf if none does.
DEV uint64_t first_ending_after(const uint64_t *in_off, uint32_t nbuf, uint64_t pos)
{
    uint64_t lo = 0, hi = nbuf;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (in_off[mid + 1] > pos)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// --------------------------------------------------------------- wrapped --

// One buffer's WrapArgs from its plan (what the bodies read of it).
DEV WrapArgs wrap_args(uint64_t len, const lines_plan::WrapPlan &p, const Call &c)
{
    WrapArgs w = {};
    w.len = len;
    w.E = p.E;
    w.W = p.W;
    w.full_lines = p.full_lines;
    w.hot_blocks = p.hot_blocks;
    w.L = c.L;
    w.P = c.P;
    w.s = c.s;
    w.sep = c.sep;
    w.last_len = p.last_len;
    return w;
}

// Hot blocks [j0, j1) of one buffer, a pass of 64 at a time.  (kt, ct): line
// and column of the pass's first byte, divided out once.
template <typename IDX>
DEV void wrap_hot(const uint8_t *tab, const uint4 *low16, const uint4 *sep16, const uint8_t *rin,
                  uint8_t *rout, uint32_t lane, uint64_t j0, uint64_t j1, const WrapArgs &w,
                  const Call &c)
{
    uint64_t kt = lines_plan::div32(16 * j0, c.P);
    uint32_t ct = (uint32_t) (16 * j0 - kt * c.P);
    for (uint64_t jp = j0; jp < j1; jp += kPassLanes) {
        const uint64_t j = jp + lane;
        if (j < j1) {
            const uint32_t rel = ct + 16 * lane;
            const uint32_t dk = __umulhi(rel, c.magic);
            wrap_block<IDX>(tab, low16, sep16, rin, rout + 16 * j, (IDX) kt + dk,
                            rel - dk * c.P, w);
        }
        kt += c.step_k;
        ct += c.step_c;
        if (ct >= c.P) {
            ct -= c.P;
            kt++;
        }
    }
}

// Blocks [j0, j1) of a wrapped buffer.
DEV void wrap_range(const uint8_t *tab, const uint4 *low16, const uint4 *sep16,
                    const uint8_t *rin, uint8_t *rout, uint32_t lane, uint64_t j0, uint64_t j1,
                    const WrapArgs &w, const Call &c, const Alpha &a)
{
    const uint64_t h1 = j1 < w.hot_blocks ? j1 : w.hot_blocks;
    if (j0 < h1) {
        if (w.W >> 32)
            wrap_hot<uint64_t>(tab, low16, sep16, rin, rout, lane, j0, h1, w, c);
        else
            wrap_hot<uint32_t>(tab, low16, sep16, rin, rout, lane, j0, h1, w, c);
    }
    for (uint64_t j = (j0 > w.hot_blocks ? j0 : w.hot_blocks) + lane; j < j1; j += kPassLanes) {
        const uint64_t left = w.W - 16 * j;
        wrap_bytes(tab, rin, rout, 16 * j, left >= 16 ? 16u : (uint32_t) left, w, a);
    }
}

// ----------------------------------------------------------------- plain --

// 12 input bytes in dwords x, y, z -> 16 characters.
DEV u32x4a4 plain_quad(const uint8_t *tab, uint32_t x, uint32_t y, uint32_t z)
{
    // v_perm_b32 selectors: byte i of the result picks byte sel[i] of
    // {S0:S1} (0-3 = S1, 4-7 = S0, 0x0c = zero).
    u32x4a4 o;
    o.x = enc_group(tab, __builtin_amdgcn_perm(0u, x, 0x0c000102u));  // in0 in1 in2
    o.y = enc_group(tab, __builtin_amdgcn_perm(y, x, 0x0c030405u));   // in3 in4 in5
    o.z = enc_group(tab, __builtin_amdgcn_perm(z, y, 0x0c020304u));   // in6 in7 in8
    o.w = enc_group(tab, __builtin_amdgcn_perm(0u, z, 0x0c010203u));  // in9 in10 in11
    return o;
}

// Characters [16 j, 16 j + cnt) of a plain text (cnt <= 16), group by group:
// the missing bytes of the last group zero, the pad character past its real
// characters (finalize(), src/base64encoder.c:61-99).  Stored as wrap_bytes
// stores: whole dwords where the destination is dword aligned.
DEV void plain_bytes(const uint8_t *tab, const uint8_t *in, uint8_t *out, uint64_t j, uint32_t cnt,
                     uint64_t len, const Alpha &a)
{
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint64_t bi = 12 * j + 3 * q;
        if (4 * q >= cnt) continue;  // then bi >= len too
        const uint64_t rem = len - bi;  // >= 1
        uint32_t g = (uint32_t) in[bi] << 16;
        if (rem > 1) g |= (uint32_t) in[bi + 1] << 8;
        if (rem > 2) g |= in[bi + 2];
        uint32_t ch = enc_group(tab, g);
        if (rem < 3) {
            const uint32_t keep = rem == 1 ? 0xFFFFu : 0xFFFFFFu;
            ch = (ch & keep) | ((a.padc * 0x01010101u) & ~keep);
        }
        o[q] = ch;
    }
    uint8_t *dst = out + 16 * j;
    const uint32_t nd = (((uintptr_t) dst) & 3) == 0 ? cnt >> 2 : 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
        if (q < nd) ((uint32_t *) dst)[q] = o[q];
#pragma unroll 1
    for (uint32_t i = 4 * nd; i < cnt; i++) dst[i] = (uint8_t) (o[i >> 2] >> (8 * (i & 3)));
}

// Blocks [j0, j1) of a plain buffer of len bytes and E characters.
DEV void plain_range(const uint8_t *tab, const uint8_t *rin, uint8_t *rout, uint32_t lane,
                     uint64_t j0, uint64_t j1, uint64_t len, const enc_wide_plan::PlainPlan &p,
                     const Alpha &a)
{
    const uint64_t h1 = j1 < p.hot_blocks ? j1 : p.hot_blocks;
    for (uint64_t j = j0 + lane; j < h1; j += kPassLanes) {
        const u32x3a4 v = __builtin_nontemporal_load((const u32x3a4 *) (rin + 12 * j));
        __builtin_nontemporal_store(plain_quad(tab, v.x, v.y, v.z), (u32x4a4 *) (rout + 16 * j));
    }
    for (uint64_t j = (j0 > p.hot_blocks ? j0 : p.hot_blocks) + lane; j < j1; j += kPassLanes) {
        const uint64_t left = p.E - 16 * j;
        plain_bytes(tab, rin, rout, j, left >= 16 ? 16u : (uint32_t) left, len, a);
    }
}

// ---------------------------------------------------------------- kernel --

template <bool WRAP>
__global__ __launch_bounds__(kWideTH) void k_encode_wide(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t nbuf,
    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, Call c, Alpha a)
{
    __shared__ uint8_t tab[64];
    __shared__ __attribute__((aligned(16))) uint8_t low16b[kLowRows * 16];
    __shared__ __attribute__((aligned(16))) uint8_t sep16b[kSepRows * 16];
    const uint64_t base = in_off[0], total = in_off[nbuf] - base;
    const uint64_t S = enc_wide_plan::share(total, gridDim.x * kWideWaves);
    // the block's first wave owns nothing: nor do the others
    if (enc_wide_plan::mul_sat(S, blockIdx.x * kWideWaves) >= total) return;
    build_enc_table(tab, a);
    if (WRAP) build_splice_tables(low16b, sep16b, c.sep, c.s);
    block_sync();
    const uint4 *low16 = (const uint4 *) low16b;
    const uint4 *sep16 = (const uint4 *) sep16b;
    const uint32_t lane = threadIdx.x % kPassLanes;
    uint64_t lo, hi;
    if (!enc_wide_plan::span(total, S, blockIdx.x * kWideWaves + wave_in_block(), &lo, &hi)) return;
    const uint64_t A = base + lo, Z = base + hi;  // the span, as offsets of `in`
    uint32_t empties = 0;
    for (uint64_t b = first_ending_after(in_off, nbuf, A); b < nbuf; b++) {
        const uint64_t beg = in_off[b];
        if (beg >= Z) break;
        const uint64_t end = in_off[b + 1], len = end - beg;
        if (len == 0) {
            // a long run of empty buffers: search for its end
            if (++empties == enc_wide_plan::kEmptyRun) {
                empties = 0;
                b = first_ending_after(in_off, nbuf, beg) - 1;
            }
            continue;
        }
        empties = 0;
        const uint64_t x0 = A > beg ? A - beg : 0, x1 = Z < end ? Z - beg : len;
        const uint8_t *rin = in + beg;
        uint8_t *rout = out + out_off[b];
        const bool fast = c.fast && ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) == 0;
        if (WRAP) {
            const lines_plan::WrapPlan p = lines_plan::wrap_plan(len, c, fast);
            const uint64_t B = enc_wide_plan::blocks_of(p.W);
            const uint64_t j0 = enc_wide_plan::cut(x0, len, B, c);
            const uint64_t j1 = enc_wide_plan::cut(x1, len, B, c);
            if (j0 < j1)
                wrap_range(tab, low16, sep16, rin, rout, lane, j0, j1, wrap_args(len, p, c), c, a);
        } else {
            const enc_wide_plan::PlainPlan p = enc_wide_plan::plain_plan(len, c.pad != 0, fast);
            const uint64_t B = enc_wide_plan::blocks_of(p.E);
            const uint64_t j0 = enc_wide_plan::cut(x0, len, B, c);
            const uint64_t j1 = enc_wide_plan::cut(x1, len, B, c);
            if (j0 < j1) plain_range(tab, rin, rout, lane, j0, j1, len, p, a);
        }
    }
}

// ------------------------------------------------------------------ host --

int wide_grid(uint64_t total_hint, uint32_t *grid)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0) {
        const int rc = hip_status();
        return rc ? rc : -ENODEV;
    }
    *grid = enc_wide_plan::grid_blocks(total_hint, (uint32_t) cus);
    return 0;
}

}  // namespace

extern "C" {

int b64x_encode_batch_wide(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                           uint64_t total_hint, void *d_out, const uint64_t *d_out_off,
                           const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_off) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (fmt && !lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t grid = 0;
    if ((rc = wide_grid(total_hint, &grid)) != 0) return rc;
    const Call c = lines_plan::make_call(fmt, a, false);
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    if (fmt)
        hipLaunchKernelGGL((k_encode_wide<true>), dim3(grid), dim3(kWideTH), 0,
                           (hipStream_t) stream, in, d_in_off, nbuf, out, d_out_off, c, a);
    else
        hipLaunchKernelGGL((k_encode_wide<false>), dim3(grid), dim3(kWideTH), 0,
                           (hipStream_t) stream, in, d_in_off, nbuf, out, d_out_off, c, a);
    return hip_status();
}

}  // extern "C"
