// Line-wrapped base64 encode for gfx950 (MIME 76/CRLF, PEM 64/LF): the text
// b64x_encode_dev() writes, cut into lines of L characters with a separator
// of s bytes after each (include/b64x.h, b64x_encode_lines_*).  A translation
// unit and a code object of its own, linked after b64x_kernels.o: the kernels
// of b64x_kernels.hip are not touched by it.
//
// Layout ("k_encode_lines").  The kernel is indexed by the
// *output*: a lane owns one 16-byte block of a row's text and writes it with
// one non-temporal dwordx4 store.  Writes are 1.37x the reads, so the stores
// are the ones kept whole; the loads are a dword-aligned 20-byte window that
// is funnel-shifted to the block's first 3-byte group.
//
//   block at row offset p:  line k = p / (L+s), column c0 = p mod (L+s)
//   (a wave-scalar (line, column) of the tile plus a 32-bit multiply-high per
//   lane; no 64-bit division per lane).  With L >= 16 a block holds at most
//   one separator, at block bytes [jS, jS+s), jS = L - c0:
//       bytes before it are characters  v + j        (v = k L + c0)
//       bytes after it are characters   v + j - s
//   both runs come from the same 5 groups (20 characters C[0..20) from the
//   group of the block's first character on); the block is two byte-funnels
//   of C merged under byte masks, with the separator in between (the masks
//   and the separator in place are 16-byte rows of two small LDS tables).
//
// L is a multiple of 4, so a line starts on a 3-byte group and a block never
// needs bits of a group outside its 5.  The "hot" blocks are those that lie
// wholly in the part of a row whose characters come from complete groups
// with 20 readable bytes behind their first group; the rest of the row (the
// last blocks: partial group, padding, a short last line and its separator)
// is written bytewise by extra blocks at the end of the same grid, dense, so
// that no hot wave diverges into the bytewise code.  Where there is no hot
// part, k_encode_lines_any takes the whole text with the same bytewise code.
//
// Which of the two runs, its grid and its WrapArgs are the host's launch plan
// (plan_wrap_one, plan_wrap_rows of b64x_lines_plan.h, plain host C++ that is
// tested without a GPU); what is here is validate, plan, launch.  The
// per-lane bodies (wrap_block, wrap_bytes) are in b64x_wrap_body.h, shared
// with the ragged form (b64x_lines_batch.hip).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include <type_traits>

#include "b64x.h"
#include "b64x_wrap_body.h"

namespace {

// Any layout, any alignment, any line length: a lane takes 16-byte pieces of
// a row's text (row-relative, no alignment assumed) bytewise, grid-stride.
__global__ __launch_bounds__(kWrapTH) void k_encode_lines_any(
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t nbuf, WrapArgs w,
    Alpha a)
{
    __shared__ uint8_t tab[64];
    build_enc_table(tab, a);
    block_sync();
    const uint64_t per_row = (w.W + 15) / 16;
    const uint64_t slots = per_row * nbuf;
    const uint64_t step = (uint64_t) gridDim.x * kWrapTH;
    for (uint64_t t = (uint64_t) blockIdx.x * kWrapTH + threadIdx.x; t < slots; t += step) {
        const uint64_t b = nbuf == 1 ? 0 : t / per_row;
        const uint64_t q0 = (t - b * per_row) * 16;
        const uint64_t left = w.W - q0;
        wrap_bytes(tab, in + b * w.in_stride, out + b * w.out_stride, q0,
                   left >= 16 ? 16u : (uint32_t) left, w, a);
    }
}

// Grid: hot_tiles blocks of hot blocks, then the blocks of the tail slots.
// ROWS: a batch of rows (32-bit positions inside a row); else one buffer,
// BIG when its positions need 64 bits.
template <bool ROWS, bool BIG>
__global__ __launch_bounds__(kWrapTH) void k_encode_lines(
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, WrapArgs w, Alpha a)
{
    typedef typename std::conditional<BIG, uint64_t, uint32_t>::type IDX;
    __shared__ uint8_t tab[64];
    __shared__ __attribute__((aligned(16))) uint8_t low16b[kLowRows * 16];
    __shared__ __attribute__((aligned(16))) uint8_t sep16b[kSepRows * 16];
    build_enc_table(tab, a);
    build_splice_tables(low16b, sep16b, w.sep, w.s);
    block_sync();
    const uint4 *low16 = (const uint4 *) low16b;
    const uint4 *sep16 = (const uint4 *) sep16b;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < w.hot_tiles) {
        if (ROWS) {
            // the tile's first slot gives its (row, block) once (scalar); a
            // lane's is a 32-bit multiply-high from there, as for the line
            const uint64_t t0 = (uint64_t) blockIdx.x * kWrapTH;
            if (t0 + tid >= w.hot_slots) return;
            const uint64_t b0 = __umul64hi(t0, w.m64_hb);
            const uint32_t rel = (uint32_t) (t0 - b0 * w.hot_blocks) + tid;
            const uint32_t db = __umulhi(rel, w.magic_hb);
            const uint64_t b = b0 + db;
            const uint32_t p = 16 * (rel - db * w.hot_blocks32);
            const uint32_t k = __umulhi(p, w.magic_p);
            wrap_block<uint32_t>(tab, low16, sep16, in + b * w.in_stride,
                                 out + b * w.out_stride + p, k, p - k * w.P, w);
        } else {
            const IDX j = (IDX) blockIdx.x * kWrapTH + tid;
            if (j >= (IDX) w.hot_blocks) return;
            // the tile's (line, column), wave-scalar; the lane's from there
            const uint64_t pt = (uint64_t) blockIdx.x * kWrapTile;
            const uint64_t kt = __umul64hi(pt, w.m64);
            const uint32_t rel = (uint32_t) (pt - kt * w.P) + 16 * tid;
            const uint32_t dk = __umulhi(rel, w.magic_p);
            wrap_block<IDX>(tab, low16, sep16, in, out + 16 * (uint64_t) j, (IDX) kt + dk,
                            rel - dk * w.P, w);
        }
        return;
    }
    const uint64_t t = (uint64_t) (blockIdx.x - w.hot_tiles) * kWrapTH + tid;
    if (t >= w.tail_slots) return;
    const uint64_t b = ROWS ? t / w.tail_blocks : 0;
    const uint64_t q0 = 16 * (w.hot_blocks + (t - b * w.tail_blocks));
    const uint64_t left = w.W - q0;
    wrap_bytes(tab, in + b * w.in_stride, out + b * w.out_stride, q0,
               left >= 16 ? 16u : (uint32_t) left, w, a);
}

// ---------------------------------------------------------------- host --

using lines_plan::WrapLaunch;

uint32_t low4(const void *p) { return (uint32_t) ((uintptr_t) p & 15); }

// kAny: all nbuf rows; kHot: the rows the plan covers (one buffer, or all but
// the last row).
int launch(const void *d_in, void *d_out, uint32_t nbuf, const WrapLaunch &p, const Alpha &a,
           void *stream)
{
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    const dim3 g(p.grid), b(kWrapTH);
    const hipStream_t st = (hipStream_t) stream;
    if (p.kind == lines_plan::kAny)
        hipLaunchKernelGGL(k_encode_lines_any, g, b, 0, st, in, out, nbuf, p.w, a);
    else if (nbuf > 1)
        hipLaunchKernelGGL((k_encode_lines<true, false>), g, b, 0, st, in, out, p.w, a);
    else if (p.w.W < (1ull << 32))
        hipLaunchKernelGGL((k_encode_lines<false, false>), g, b, 0, st, in, out, p.w, a);
    else
        hipLaunchKernelGGL((k_encode_lines<false, true>), g, b, 0, st, in, out, p.w, a);
    return hip_status();
}

int launch_one(const void *d_in, uint64_t n, void *d_out, const Alpha &a,
               const lines_plan::Call &c, void *stream)
{
    return launch(d_in, d_out, 1, lines_plan::plan_wrap_one(n, c, low4(d_in), low4(d_out)), a,
                  stream);
}

}  // namespace

extern "C" {

uint64_t b64x_encoded_lines_len(uint64_t n, bool pad, const b64x_lines *fmt)
{
    if (!fmt || fmt->line_len == 0 || fmt->sep_len > 4) return 0;
    const lines_plan::Call c = lines_plan::make_call(
        fmt->line_len, fmt->sep_len, fmt->sep, (fmt->flags & B64X_LINES_TRAILING) != 0, pad, false);
    return lines_plan::wrap_plan(n, c, false).W;
}

int b64x_encode_lines_dev(const void *d_in, uint64_t n, void *d_out,
                          const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (n == 0) return 0;
    if (!d_in || !d_out) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (!lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    const int rc = b64x_device_check();
    if (rc) return rc;
    return launch_one(d_in, n, d_out, a, lines_plan::make_call(fmt, a, false), stream);
}

int b64x_encode_lines_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                              void *d_out, uint64_t out_stride,
                              const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0 || len == 0) return 0;
    if (!d_in || !d_out) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (!lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    const lines_plan::Call c = lines_plan::make_call(fmt, a, false);
    const WrapLaunch p =
        nbuf == 1 ? lines_plan::plan_wrap_one(len, c, low4(d_in), low4(d_out))
                  : lines_plan::plan_wrap_rows(len, nbuf, c, low4(d_in), low4(d_out), in_stride,
                                               out_stride);
    if (in_stride < len || out_stride < p.w.W) return -EINVAL;
    const int rc = b64x_device_check();
    if (rc) return rc;
    const int rc2 = launch(d_in, d_out, nbuf, p, a, stream);
    if (rc2 || nbuf == 1 || p.kind == lines_plan::kAny) return rc2;
    // the rows' hot kernel leaves the last row out: it goes as one buffer
    const uint64_t last = nbuf - 1;
    return launch_one((const uint8_t *) d_in + last * in_stride, len,
                      (uint8_t *) d_out + last * out_stride, a, c, stream);
}

}  // extern "C"
