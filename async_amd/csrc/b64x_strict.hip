// Strict base64 decode for gfx950: accepts exactly the texts b64x_encode_dev()
// and b64x_encode_lines_*() write under the same alphabet and line format,
// decodes them, and otherwise reports the kind and offset of the first
// offence (include/b64x.h, b64x_decode_strict_*).  A translation unit and a
// code object of its own, linked after b64x_kernels.o and b64x_wrap.o: the
// kernels of those files are not touched by it.
//
// Layout ("k_decode_strict").  The kernel is indexed by the
// *output*: a lane owns 16 characters of a row (characters [16 j, 16 j + 16))
// and writes their 12 bytes with one non-temporal dwordx3 store.
//
//   character e stands at row offset (e / L) P + e mod L  (P = L + s; plain
//   text: e).  L is a multiple of 4 and 16 j is one of 16, so a lane's column
//   c is a multiple of 4, a 4-character group never straddles a line, and with
//   L >= 16 the lane's run crosses at most one separator, which starts at a
//   dword boundary of the run: lane byte jS = L - c.  The lane loads a
//   dword-aligned 24-byte window (one 16-byte and one 8-byte load), funnels
//   it to the run's first byte, and takes group g from the window's dword g
//   (before the separator) or from the bytes s further on (after it).
//
// Who checks which byte: a lane checks its 16 characters and the separator
// that follows any of them (so the lane that owns the last character of a
// line checks that line's separator, the owner of character E - 1 the
// trailing one).  Every byte of the text is checked by exactly one lane.  A
// 256-entry LDS table maps a byte to its sextet, 0x80 set for "not one of the
// 64" and 0xC0 for the pad character; a lane ORs its 16 lookups and XORs the
// separator dword against the separator in place, and only a lane that found
// something works out which byte it was and does one 64-bit atomicMin of
// (offset << 3 | kind) on the record's err_pos field (all ones = no offence:
// good text performs no atomics).  The lowest key is the first offence.
//
// The "hot" lanes are those whose 16 characters lie below character E - 4
// and whose window lies inside the text; the rest of a row (the last group
// and its pads, the unused-bits check, a short last line, the trailing
// separator) is decoded bytewise, following the scalar procedure of b64x.h
// literally, by extra blocks at the end of the same grid.  Where there is no
// hot part, k_decode_strict_any takes the whole text with the same bytewise
// code.
//
// Which of the two runs, its grid and its StrictArgs are the host's launch
// plan (plan_strict of b64x_lines_plan.h, plain host C++ that is tested
// without a GPU); what is here is validate, plan, launch.
//
// The record: a memset node fills it with ones (the empty key), the decode
// kernel lowers the key and the lane that owns character E - 1 (which counts
// the pads anyway) leaves out_len, and k_strict_record (one thread per row)
// turns the key into {out_len, err_pos, err}.  No host round trip, no
// workspace, no state.
//
// The per-lane bodies (strict_lane, strict_bytes) are in b64x_strict_body.h,
// shared with the ragged form (b64x_lines_batch.hip), which keeps its records
// in LDS instead.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_strict_body.h"

namespace {

HD uint64_t *row_key(b64x_strict_result *res, uint64_t b) { return &res[b].err_pos; }

// A hot tile's lane `tid` (ROWS: a batch of rows, 32-bit positions inside a
// row; else one buffer of any length).
template <bool ROWS, bool WRAP>
HD void hot_body(uint32_t bid, uint32_t tid, const uint8_t *tab, const uint8_t *in, uint8_t *out,
                 b64x_strict_result *res, const StrictArgs &w)
{
    if (ROWS) {
        // the tile's first slot gives its (row, lane) once (scalar); a lane's
        // is a 32-bit multiply-high from there, as its line is
        const uint64_t t0 = (uint64_t) bid * kStrictTH;
        if (t0 + tid >= w.hot_slots) return;
        const uint64_t b0 = mul_hi64(t0, w.m64_hl);
        const uint32_t rel = (uint32_t) (t0 - b0 * w.hot_lanes) + tid;
        const uint32_t db = mul_hi32(rel, w.magic_hl);
        const uint64_t b = b0 + db;
        const uint32_t j = rel - db * w.hot_lanes32;
        const uint32_t e0 = j * kLaneChars;
        uint32_t k = 0, c = 0;
        if (WRAP) {
            k = mul_hi32(e0, w.magic_l);
            c = e0 - k * w.L;
        }
        strict_lane<WRAP>(tab, in + b * w.in_stride, out + b * w.out_stride + 12 * (uint64_t) j,
                          row_key(res, b), WRAP ? (uint64_t) k * w.P + c : e0, c, w);
    } else {
        const uint64_t j = (uint64_t) bid * kStrictTH + tid;
        if (j >= w.hot_lanes) return;
        uint64_t p0 = j * kLaneChars;
        uint32_t c = 0;
        if (WRAP) {
            // the tile's (line, column), wave-scalar; the lane's from there
            const uint64_t et = (uint64_t) bid * kTileChars;
            const uint64_t kt = mul_hi64(et, w.m64);
            const uint32_t rel = (uint32_t) (et - kt * w.L) + kLaneChars * tid;
            const uint32_t dk = mul_hi32(rel, w.magic_l);
            c = rel - dk * w.L;
            p0 = (kt + dk) * w.P + c;
        }
        strict_lane<WRAP>(tab, in, out + 12 * j, row_key(res, 0), p0, c, w);
    }
}

template <bool ROWS>
HD void tail_body(uint32_t bid, uint32_t tid, const uint8_t *tab, const uint8_t *in, uint8_t *out,
                  b64x_strict_result *res, const StrictArgs &w)
{
    const uint64_t t = (uint64_t) (bid - w.hot_tiles) * kStrictTH + tid;
    if (t >= w.tail_slots) return;
    const uint64_t b = !ROWS ? 0
                       : w.tail_lanes == 1 ? t
                       : (w.tail_slots >> 32) ? t / w.tail_lanes
                                              : (uint32_t) t / (uint32_t) w.tail_lanes;
    strict_bytes(tab, in + b * w.in_stride, out + b * w.out_stride, res + b,
                 w.hot_lanes + (t - b * w.tail_lanes), w);
}

// ------------------------------------------------------------- kernels --

// Grid: hot_tiles blocks of hot lanes, then the blocks of the tail slots.
template <bool ROWS, bool WRAP>
__global__ __launch_bounds__(kStrictTH) void k_decode_strict(
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, b64x_strict_result *res,
    StrictArgs w)
{
    __shared__ uint8_t tab[256];
    build_dec_table(tab, w.a);
    block_sync();
    if (blockIdx.x < w.hot_tiles)
        hot_body<ROWS, WRAP>(blockIdx.x, threadIdx.x, tab, in, out, res, w);
    else
        tail_body<ROWS>(blockIdx.x, threadIdx.x, tab, in, out, res, w);
}

// Any layout, any alignment, any line length: every lane bytewise, grid-stride.
__global__ __launch_bounds__(kStrictTH) void k_decode_strict_any(
    const uint8_t *__restrict__ in, uint8_t *__restrict__ out, b64x_strict_result *res,
    uint32_t nbuf, StrictArgs w)
{
    __shared__ uint8_t tab[256];
    build_dec_table(tab, w.a);
    block_sync();
    const uint64_t per_row = (w.E + kLaneChars - 1) / kLaneChars;
    const uint64_t slots = per_row * nbuf;
    const uint64_t step = (uint64_t) gridDim.x * kStrictTH;
    for (uint64_t t = (uint64_t) blockIdx.x * kStrictTH + threadIdx.x; t < slots; t += step) {
        const uint64_t b = nbuf == 1 ? 0 : t / per_row;
        strict_bytes(tab, in + b * w.in_stride, out + b * w.out_stride, res + b,
                     t - b * per_row, w);
    }
}

// The records' final form, one thread per row.  length_error: no encoder
// output has this length ({LENGTH, nchars}; nothing was decoded).
__global__ __launch_bounds__(kStrictTH) void k_strict_record(
    b64x_strict_result *res, uint32_t nbuf, uint32_t length_error, uint64_t nchars)
{
    const uint64_t b = (uint64_t) blockIdx.x * kStrictTH + threadIdx.x;
    if (b >= nbuf) return;
    if (length_error) {
        b64x_strict_result f;
        f.out_len = 0;
        f.err_pos = nchars;
        f.err = B64X_STRICT_LENGTH;
        f.reserved = 0;
        res[b] = f;
        return;
    }
    finish_record(&res[b]);
}

// ---------------------------------------------------------------- host --

using lines_plan::StrictLaunch;

uint32_t low4(const void *p) { return (uint32_t) ((uintptr_t) p & 15); }

int launch(const void *d_in, void *d_out, b64x_strict_result *d_res, uint32_t nbuf,
           const StrictLaunch &p, hipStream_t st)
{
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    const dim3 g(p.grid), b(kStrictTH);
    const bool rows = nbuf > 1;
    if (p.kind == lines_plan::kAny)
        hipLaunchKernelGGL(k_decode_strict_any, g, b, 0, st, in, out, d_res, nbuf, p.w);
    else if (!rows && p.w.s)
        hipLaunchKernelGGL((k_decode_strict<false, true>), g, b, 0, st, in, out, d_res, p.w);
    else if (!rows)
        hipLaunchKernelGGL((k_decode_strict<false, false>), g, b, 0, st, in, out, d_res, p.w);
    else if (p.w.s)
        hipLaunchKernelGGL((k_decode_strict<true, true>), g, b, 0, st, in, out, d_res, p.w);
    else
        hipLaunchKernelGGL((k_decode_strict<true, false>), g, b, 0, st, in, out, d_res, p.w);
    return hip_status();
}

// Both entry points: nbuf rows of nchars bytes.
int decode_strict(const void *d_in, uint64_t in_stride, uint64_t nchars, uint32_t nbuf,
                  void *d_out, uint64_t out_stride, b64x_strict_result *d_res,
                  const b64x_alphabet *abc, const b64x_lines *fmt, bool strided, void *stream)
{
    if (!d_in || !d_out || !d_res || (((uintptr_t) d_res) & 7)) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    if (fmt && !lines_plan::fmt_ok(fmt, a)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    const StrictLaunch p =
        lines_plan::plan_strict(nchars, nbuf, lines_plan::make_call(fmt, a, true), a, low4(d_in),
                                low4(d_out), in_stride, out_stride);
    if (strided && (in_stride < nchars || out_stride < (p.w.E + 3) / 4 * 3)) return -EINVAL;
    if (nbuf == 0) return 0;
    const int rc = b64x_device_check();
    if (rc) return rc;
    const hipStream_t st = (hipStream_t) stream;
    const uint64_t res_bytes = (uint64_t) nbuf * sizeof(b64x_strict_result);
    if (nchars == 0) {  // the empty text: {0, 0, OK}
        if (hipMemsetAsync(d_res, 0, res_bytes, st) != hipSuccess) return hip_status();
        return 0;
    }
    if (!p.length_error) {
        // the empty key in every record, then the decode lowers it
        if (hipMemsetAsync(d_res, 0xFF, res_bytes, st) != hipSuccess) return hip_status();
        const int rc2 = launch(d_in, d_out, d_res, nbuf, p, st);
        if (rc2) return rc2;
    }
    const uint32_t rgrid = (nbuf + kStrictTH - 1) / kStrictTH;
    hipLaunchKernelGGL(k_strict_record, dim3(rgrid), dim3(kStrictTH), 0, st, d_res, nbuf,
                       p.length_error, nchars);
    return hip_status();
}

}  // namespace

extern "C" {

uint64_t b64x_strict_decoded_cap(uint64_t nchars, const b64x_lines *fmt)
{
    // a pitch past 32 bits, which no call accepts, has no Call: 0 as well (b64x.h)
    if (fmt && (fmt->line_len == 0 || fmt->sep_len < 1 || fmt->sep_len > 4 ||
                (uint64_t) fmt->line_len + fmt->sep_len > 0xFFFFFFFFull))
        return 0;
    const lines_plan::Call c = lines_plan::make_call(fmt, lines_plan::make_alpha(nullptr), true);
    return (lines_plan::strict_plan(nchars, c, false).E + 3) / 4 * 3;
}

int b64x_decode_strict_dev(const void *d_in, uint64_t nchars, void *d_out,
                           b64x_strict_result *d_res, const b64x_alphabet *abc,
                           const b64x_lines *fmt, void *stream)
{
    return decode_strict(d_in, 0, nchars, 1, d_out, 0, d_res, abc, fmt, false, stream);
}

int b64x_decode_strict_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                               void *d_out, uint64_t out_stride, b64x_strict_result *d_res,
                               const b64x_alphabet *abc, const b64x_lines *fmt, void *stream)
{
    return decode_strict(d_in, in_stride, len, nbuf, d_out, out_stride, d_res, abc, fmt, true,
                         stream);
}

}  // extern "C"
