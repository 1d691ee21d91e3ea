// The ragged strict decode, plain and line-wrapped, balanced over the batch's
// bytes and not over its texts (include/b64x.h, b64x_decode_strict_batch_wide):
// nbuf texts of any lengths addressed by device-resident offsets, an 8 MiB
// text among 4 KiB ones spread over the device like the rest.  A translation
// unit and a code object of its own, linked after b64x_encode_wide.o; the
// per-lane bodies are those of the one-buffer kernels (b64x_strict_body.h),
// one copy.
//
// Layout ("k_decode_strict_wide"; the arithmetic is
// b64x_strict_wide_plan.h).  in_off is monotone, so the texts lie end to end
// in one arena.  Every wave reads its size, total = in_off[nbuf] - in_off[0],
// and takes an equal span of it; the grid comes from the host's hint and the
// device, the share from the total on the device, so the hint cannot make the
// result wrong and a captured call replays on other offsets.  Canonical text
// is the easy decode: where every character and separator stands follows from
// a text's length and the format alone, so there is no count pass, no scan
// and no workspace.  For its span a wave
//   1. finds the first text that ends after the span's start: one binary
//      search over in_off with scalar loads;
//   2. walks forward while texts start before the span's end (a run of empty
//      texts costs a second search, not a load each).  Per text it runs the
//      prologue of b64x_lines_plan.h (strict_plan) and turns the part of the
//      text inside the span into a range of 16-character lanes,
//      [cut(a), cut(z)): lane j belongs to the span that holds character
//      16 j, so every lane has exactly one owner.  A text with a LENGTH
//      verdict has no lanes and nothing of it is read;
//   3. decodes the owned lanes below hot_lanes in passes of 64 (the first
//      pass's line and column come from one division at the range's first
//      lane, the next ones' from additions, a lane's from one multiply-high),
//      the others bytewise, a lane to each.  Whether a text is dword aligned
//      on both sides decides that for the whole of it, wave-uniform.
// A lane checks its characters and the separator that follows any of them, the
// owner of character E - 1 the trailing one: every byte of every text is
// checked exactly once.
//
// The record.  A text may be shared by many waves, so its lowest offence key
// lives in the record itself, as in the one-buffer call: k_strict_wide_clear
// (one thread per text) fills the records with ones (the empty key), a lane
// that finds an offence lowers the key with one 64-bit atomicMin (good text
// performs none), the owner of character E - 1 leaves out_len, and
// k_strict_wide_record (one thread per text) gives every record its final
// form -- the LENGTH and empty ones too, from the length alone.  Three graph
// nodes whatever the sizes, all three kernels: the one-buffer call's memset
// node is a kernel here because a captured memset node left other bytes than
// ones in the records from the second replay of a graph on (the first replay
// and every direct call were right), and this call is made to be replayed.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_strict_body.h"
#include "b64x_strict_wide_plan.h"

namespace {

using lines_plan::Call;
using lines_plan::kPassLanes;

constexpr uint32_t kWideTH = strict_wide_plan::kBlockLanes;
constexpr uint32_t kWideWaves = strict_wide_plan::kBlockWaves;

static_assert(kWideTH == kStrictTH, "the table builder's block size");

// The wave's index in the block, as the scalar it is.
DEV uint32_t wave_in_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x / kPassLanes); }

// The first text that ends after arena position pos; nbuf if none does.
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

// One text's StrictArgs from its plan (what the bodies read of it).
DEV StrictArgs strict_args(uint64_t W, const lines_plan::StrictPlan &p, const Call &c,
                           const Alpha &a)
{
    StrictArgs w = {};
    w.E = p.E;
    w.W = W;
    w.off_e1 = p.off_e1;
    w.off_e2 = p.off_e2;
    w.L = c.L;
    w.P = c.P;
    w.s = c.s;
    w.sep = c.sep;
    w.sep_mask = c.sep_mask;
    w.trailing = c.trailing;
    w.a = a;
    return w;
}

// Hot lanes [j0, j1) of one text, a pass of 64 at a time.  (kt, ct): line and
// column of the pass's first character, divided out once.  IDX: the type a
// text offset fits.
template <bool WRAP, typename IDX>
DEV void strict_hot(const uint8_t *tab, const uint8_t *rin, uint8_t *rout, uint64_t *key,
                    uint32_t lane, uint64_t j0, uint64_t j1, const StrictArgs &w, const Call &c)
{
    uint64_t kt = 0;
    uint32_t ct = 0;
    if (WRAP) {
        kt = lines_plan::div32(kLaneChars * j0, c.L);
        ct = (uint32_t) (kLaneChars * j0 - kt * c.L);
    }
    for (uint64_t jp = j0; jp < j1; jp += kPassLanes) {
        const uint64_t j = jp + lane;
        if (j < j1) {
            if (WRAP) {
                const uint32_t rel = ct + kLaneChars * lane;
                const uint32_t dk = mul_hi32(rel, c.magic);
                const uint32_t col = rel - dk * c.L;
                const IDX p0 = ((IDX) kt + dk) * c.P + col;
                strict_lane<true>(tab, rin, rout + 12 * j, key, p0, col, w);
            } else {
                strict_lane<false>(tab, rin, rout + 12 * j, key, kLaneChars * j, 0, w);
            }
        }
        if (WRAP) {
            kt += c.step_k;
            ct += c.step_c;
            if (ct >= c.L) {
                ct -= c.L;
                kt++;
            }
        }
    }
}

// Lanes [j0, j1) of a text whose plan is p.
template <bool WRAP>
DEV void strict_range(const uint8_t *tab, const uint8_t *rin, uint8_t *rout,
                      b64x_strict_result *rec, uint32_t lane, uint64_t j0, uint64_t j1,
                      const lines_plan::StrictPlan &p, const StrictArgs &w, const Call &c)
{
    const uint64_t h1 = j1 < p.hot_lanes ? j1 : p.hot_lanes;
    if (j0 < h1) {
        if (w.W >> 32)
            strict_hot<WRAP, uint64_t>(tab, rin, rout, &rec->err_pos, lane, j0, h1, w, c);
        else
            strict_hot<WRAP, uint32_t>(tab, rin, rout, &rec->err_pos, lane, j0, h1, w, c);
    }
    for (uint64_t j = (j0 > p.hot_lanes ? j0 : p.hot_lanes) + lane; j < j1; j += kPassLanes)
        strict_bytes(tab, rin, rout, rec, j, w);
}

// ---------------------------------------------------------------- kernels --

template <bool WRAP>
__global__ __launch_bounds__(kWideTH) void k_decode_strict_wide(
    const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off, uint32_t nbuf,
    uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off, b64x_strict_result *res,
    Call c, Alpha a)
{
    __shared__ uint8_t tab[256];
    const uint64_t base = in_off[0], total = in_off[nbuf] - base;
    const uint64_t S = strict_wide_plan::share(total, gridDim.x * kWideWaves);
    // the block's first wave owns nothing: nor do the others
    if (strict_wide_plan::mul_sat(S, blockIdx.x * kWideWaves) >= total) return;
    build_dec_table(tab, a);
    block_sync();
    const uint32_t lane = threadIdx.x % kPassLanes;
    uint64_t lo, hi;
    if (!strict_wide_plan::span(total, S, blockIdx.x * kWideWaves + wave_in_block(), &lo, &hi))
        return;
    const uint64_t A = base + lo, Z = base + hi;  // the span, as offsets of `in`
    uint32_t empties = 0;
    for (uint64_t b = first_ending_after(in_off, nbuf, A); b < nbuf; b++) {
        const uint64_t beg = in_off[b];
        if (beg >= Z) break;
        const uint64_t end = in_off[b + 1], W = end - beg;
        if (W == 0) {
            // a long run of empty texts: search for its end
            if (++empties == strict_wide_plan::kEmptyRun) {
                empties = 0;
                b = first_ending_after(in_off, nbuf, beg) - 1;
            }
            continue;
        }
        empties = 0;
        const uint8_t *rin = in + beg;
        uint8_t *rout = out + out_off[b];
        const bool fast = c.fast && ((((uintptr_t) rin) | ((uintptr_t) rout)) & 3) == 0;
        const lines_plan::StrictPlan p = lines_plan::strict_plan(W, c, fast);
        if (p.length_error) continue;  // the record kernel's; nothing of it is read
        const uint64_t x0 = A > beg ? A - beg : 0, x1 = Z < end ? Z - beg : W;
        const uint64_t lanes = p.hot_lanes + p.tail_lanes;
        const uint64_t j0 = strict_wide_plan::cut(x0, W, lanes, c);
        const uint64_t j1 = strict_wide_plan::cut(x1, W, lanes, c);
        if (j0 < j1)
            strict_range<WRAP>(tab, rin, rout, res + b, lane, j0, j1, p, strict_args(W, p, c, a),
                               c);
    }
}

// The empty key (all ones) in every record, one thread per text.
__global__ __launch_bounds__(kWideTH) void k_strict_wide_clear(b64x_strict_result *res,
                                                               uint32_t nbuf)
{
    const uint64_t b = (uint64_t) blockIdx.x * kWideTH + threadIdx.x;
    if (b >= nbuf) return;
    b64x_strict_result f;
    f.out_len = kNoKey;
    f.err_pos = kNoKey;
    f.err = ~0u;
    f.reserved = ~0u;
    res[b] = f;
}

// The records' final form, one thread per text: the key the decode left
// becomes {out_len, err_pos, err}; an empty text and a length no encoder
// writes get theirs from the length alone.
__global__ __launch_bounds__(kWideTH) void k_strict_wide_record(
    const uint64_t *__restrict__ in_off, uint32_t nbuf, b64x_strict_result *res, Call c)
{
    const uint64_t b = (uint64_t) blockIdx.x * kWideTH + threadIdx.x;
    if (b >= nbuf) return;
    const uint64_t W = in_off[b + 1] - in_off[b];
    const lines_plan::StrictPlan p = lines_plan::strict_plan(W, c, false);
    if (W == 0 || p.length_error) {
        b64x_strict_result f;
        f.out_len = 0;
        f.err_pos = W;
        f.err = p.length_error ? B64X_STRICT_LENGTH : B64X_STRICT_OK;
        f.reserved = 0;
        res[b] = f;
        return;
    }
    finish_record(&res[b]);
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
    *grid = strict_wide_plan::grid_blocks(total_hint, (uint32_t) cus);
    return 0;
}

}  // namespace

extern "C" {

int b64x_decode_strict_batch_wide(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                                  uint64_t total_hint, void *d_out, const uint64_t *d_out_off,
                                  b64x_strict_result *d_res, const b64x_alphabet *abc,
                                  const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_off || !d_res || (((uintptr_t) d_res) & 7))
        return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (fmt && !lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t grid = 0;
    if ((rc = wide_grid(total_hint, &grid)) != 0) return rc;
    const Call c = lines_plan::make_call(fmt, a, true);
    const hipStream_t st = (hipStream_t) stream;
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    const uint32_t rgrid = (uint32_t) (((uint64_t) nbuf + kWideTH - 1) / kWideTH);
    // the empty key in every record, then the decode lowers it
    hipLaunchKernelGGL(k_strict_wide_clear, dim3(rgrid), dim3(kWideTH), 0, st, d_res, nbuf);
    if ((rc = hip_status()) != 0) return rc;
    if (fmt)
        hipLaunchKernelGGL((k_decode_strict_wide<true>), dim3(grid), dim3(kWideTH), 0, st, in,
                           d_in_off, nbuf, out, d_out_off, d_res, c, a);
    else
        hipLaunchKernelGGL((k_decode_strict_wide<false>), dim3(grid), dim3(kWideTH), 0, st, in,
                           d_in_off, nbuf, out, d_out_off, d_res, c, a);
    if ((rc = hip_status()) != 0) return rc;
    hipLaunchKernelGGL(k_strict_wide_record, dim3(rgrid), dim3(kWideTH), 0, st, d_in_off, nbuf,
                       d_res, c);
    return hip_status();
}

}  // extern "C"
