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
// that no hot wave diverges into the bytewise code.  Buffers that are not
// dword aligned, L < 16, or a line pitch the 32-bit reciprocal is not exact
// for take k_encode_lines_any: the same bytewise code for the whole text.
//
// The per-lane bodies (wrap_block, wrap_bytes) and the structs they take are
// in b64x_wrap_body.h, shared with the ragged form (b64x_lines_batch.hip).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "b64x.h"
#include "b64x_wrap_body.h"

namespace {

// Any layout, any alignment, any line length: a lane takes 16-byte pieces of
// a row's text (row-relative, no alignment assumed) bytewise, grid-stride.
__global__ __launch_bounds__(kWrapTH) void k_encode_lines_any(
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t nbuf, WrapArgs w,
    EncAlpha a)
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
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, WrapArgs w, EncAlpha a)
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

EncAlpha enc_alpha(const b64x_alphabet *abc)
{
    EncAlpha a;
    const char p62 = abc ? abc->pos62 : (char) -1;
    const char p63 = abc ? abc->pos63 : (char) -1;
    const char pc = abc ? abc->padchar : (char) -1;
    a.p62 = (uint8_t) (p62 == (char) -1 ? '+' : p62);
    a.p63 = (uint8_t) (p63 == (char) -1 ? '/' : p63);
    a.padc = (uint8_t) (pc == (char) -1 ? '=' : pc);
    a.pad = abc ? (abc->pad ? 1 : 0) : 1;
    return a;
}

bool fmt_ok(const b64x_lines *f, const EncAlpha &a)
{
    if (!f) return false;
    if (f->line_len == 0 || f->line_len % 4 != 0) return false;
    if (f->sep_len < 1 || f->sep_len > 4) return false;
    if (f->flags & ~B64X_LINES_TRAILING) return false;
    if ((uint64_t) f->line_len + f->sep_len > 0xFFFFFFFFull) return false;
    for (uint32_t i = 0; i < f->sep_len; i++) {
        const uint32_t c = f->sep[i];
        if (c - 'A' < 26u || c - 'a' < 26u || c - '0' < 10u || c == a.p62 || c == a.p63)
            return false;
    }
    return true;
}

uint64_t wrapped_len(uint64_t E, const b64x_lines *f)
{
    if (E == 0) return 0;
    const uint64_t lines = (E + f->line_len - 1) / f->line_len;
    return E + (uint64_t) f->sep_len * (lines - ((f->flags & B64X_LINES_TRAILING) ? 0 : 1));
}

int hip_status()
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    return -EIO;
}

// Row offset of character e (e < E, or e == E inside a short last line).
uint64_t char_offset(uint64_t e, uint32_t L, uint32_t P) { return e / L * P + e % L; }

WrapArgs base_args(uint64_t len, const EncAlpha &a, const b64x_lines *f, uint64_t in_stride,
                   uint64_t out_stride)
{
    WrapArgs w;
    memset(&w, 0, sizeof w);
    w.len = len;
    w.E = b64x_encoded_len(len, a.pad);
    w.W = wrapped_len(w.E, f);
    w.L = f->line_len;
    w.s = f->sep_len;
    w.P = w.L + w.s;
    w.full_lines = w.E / w.L;
    w.last_len = (uint32_t) (w.E % w.L);
    for (uint32_t i = 0; i < w.s; i++) w.sep |= (uint32_t) f->sep[i] << (8 * i);
    w.in_stride = in_stride;
    w.out_stride = out_stride;
    return w;
}

// The line pitch's reciprocals, if they are exact for this call: the 32-bit
// one for every value below `max32`, the 64-bit one for every row offset.
bool set_reciprocals(WrapArgs &w, uint64_t max32)
{
    if (w.L < 16 || w.P > (1u << 24)) return false;
    w.magic_p = (uint32_t) ((0xFFFFFFFFull + w.P) / w.P);
    const uint64_t err = (uint64_t) w.magic_p * w.P - (1ull << 32);  // < P
    if (max32 >= (1ull << 32) || max32 * err >= (1ull << 32)) return false;
    w.m64 = ~0ull / w.P + 1;
    return w.W <= ~0ull / w.P;  // offset * (m64 P - 2^64) < 2^64
}

int launch_any(const void *d_in, void *d_out, uint32_t nbuf, const WrapArgs &w,
               const EncAlpha &a, void *stream)
{
    const uint64_t slots = (w.W + 15) / 16 * nbuf;
    uint64_t grid = (slots + kWrapTH - 1) / kWrapTH;
    if (grid > (1u << 20)) grid = 1u << 20;
    hipLaunchKernelGGL(k_encode_lines_any, dim3((uint32_t) grid), dim3(kWrapTH), 0,
                       (hipStream_t) stream, (const uint8_t *) d_in, (uint8_t *) d_out, nbuf, w, a);
    return hip_status();
}

// One buffer.
int launch_one(const void *d_in, uint64_t n, void *d_out, const EncAlpha &a,
               const b64x_lines *f, void *stream)
{
    WrapArgs w = base_args(n, a, f, 0, 0);
    const bool aligned = (((uintptr_t) d_in) & 3) == 0 && (((uintptr_t) d_out) & 15) == 0;
    if (aligned && n >= 17 && set_reciprocals(w, (uint64_t) w.P + kWrapTile)) {
        // hot: the blocks wholly below the first character whose group does
        // not have 20 readable bytes behind its first byte
        const uint64_t e_hot = (n - 17) / 3 * 4;
        w.hot_blocks = char_offset(e_hot, w.L, w.P) / 16;
        const uint64_t tiles = (w.hot_blocks + kWrapTH - 1) / kWrapTH;
        w.tail_blocks = w.tail_slots = (w.W - 16 * w.hot_blocks + 15) / 16;
        const uint64_t grid = tiles + (w.tail_slots + kWrapTH - 1) / kWrapTH;
        if (w.hot_blocks > 0 && grid < (1ull << 31)) {
            w.hot_slots = w.hot_blocks;
            w.hot_tiles = (uint32_t) tiles;
            if (w.W < (1ull << 32))
                hipLaunchKernelGGL((k_encode_lines<false, false>), dim3((uint32_t) grid),
                                   dim3(kWrapTH), 0, (hipStream_t) stream,
                                   (const uint8_t *) d_in, (uint8_t *) d_out, w, a);
            else
                hipLaunchKernelGGL((k_encode_lines<false, true>), dim3((uint32_t) grid),
                                   dim3(kWrapTH), 0, (hipStream_t) stream,
                                   (const uint8_t *) d_in, (uint8_t *) d_out, w, a);
            return hip_status();
        }
    }
    return launch_any(d_in, d_out, 1, w, a, stream);
}

}  // namespace

extern "C" {

uint64_t b64x_encoded_lines_len(uint64_t n, bool pad, const b64x_lines *fmt)
{
    if (!fmt || fmt->line_len == 0 || fmt->sep_len > 4) return 0;
    return wrapped_len(b64x_encoded_len(n, pad), fmt);
}

int b64x_encode_lines_dev(const void *d_in, uint64_t n, void *d_out,
                          const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (n == 0) return 0;
    if (!d_in || !d_out) return -EINVAL;
    const EncAlpha a = enc_alpha(abc);
    if (!fmt_ok(fmt, a)) return -EINVAL;
    const int rc = b64x_device_check();
    if (rc) return rc;
    return launch_one(d_in, n, d_out, a, fmt, stream);
}

int b64x_encode_lines_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                              void *d_out, uint64_t out_stride,
                              const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    if (nbuf == 0 || len == 0) return 0;
    if (!d_in || !d_out) return -EINVAL;
    const EncAlpha a = enc_alpha(abc);
    if (!fmt_ok(fmt, a)) return -EINVAL;
    WrapArgs w = base_args(len, a, fmt, in_stride, out_stride);
    if (in_stride < len || out_stride < w.W) return -EINVAL;
    const int rc = b64x_device_check();
    if (rc) return rc;
    if (nbuf == 1) return launch_one(d_in, len, d_out, a, fmt, stream);
    // Rows at dword-aligned addresses: every row but the last takes the hot
    // path up to the first character of an incomplete group (a window may
    // read into the next row, so the last row goes alone, as one buffer).
    const uint32_t hot_rows = nbuf - 1;
    const bool aligned =
        ((((uintptr_t) d_in) | ((uintptr_t) d_out) | in_stride | out_stride) & 3) == 0;
    if (aligned && len >= 20 && w.W < (1u << 28) && set_reciprocals(w, w.W)) {
        const uint64_t e_c = len / 3 * 4;  // characters of complete groups
        const uint64_t hot_end = (e_c == w.E && w.last_len == 0) ? w.W : char_offset(e_c, w.L, w.P);
        w.hot_blocks = hot_end / 16;
        w.hot_slots = w.hot_blocks * hot_rows;
        w.tail_blocks = (w.W - 16 * w.hot_blocks + 15) / 16;
        w.tail_slots = w.tail_blocks * hot_rows;
        const uint64_t tiles = (w.hot_slots + kWrapTH - 1) / kWrapTH;
        const uint64_t grid = tiles + (w.tail_slots + kWrapTH - 1) / kWrapTH;
        if (w.hot_blocks > 1 && grid < (1ull << 31)) {
            w.hot_blocks32 = (uint32_t) w.hot_blocks;
            w.magic_hb = (uint32_t) ((0xFFFFFFFFull + w.hot_blocks) / w.hot_blocks);
            w.m64_hb = ~0ull / w.hot_blocks + 1;
            const uint64_t err = (uint64_t) w.magic_hb * w.hot_blocks - (1ull << 32);
            // exact: the lane's slot below hot_blocks + kWrapTH, the tile's below hot_slots
            if ((w.hot_blocks + kWrapTH) * err < (1ull << 32) &&
                w.hot_slots <= ~0ull / w.hot_blocks) {
                w.hot_tiles = (uint32_t) tiles;
                hipLaunchKernelGGL((k_encode_lines<true, false>), dim3((uint32_t) grid),
                                   dim3(kWrapTH), 0, (hipStream_t) stream,
                                   (const uint8_t *) d_in, (uint8_t *) d_out, w, a);
                const int rc2 = hip_status();
                if (rc2) return rc2;
                return launch_one((const uint8_t *) d_in + (uint64_t) hot_rows * in_stride, len,
                                  (uint8_t *) d_out + (uint64_t) hot_rows * out_stride, a, fmt,
                                  stream);
            }
        }
    }
    return launch_any(d_in, d_out, nbuf, w, a, stream);
}

}  // extern "C"
