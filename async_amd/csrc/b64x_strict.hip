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
// literally, by extra blocks at the end of the same grid.  Buffers or strides
// that are not dword aligned, L < 16, or a line length the 32-bit reciprocal
// is not exact for take k_decode_strict_any: the same bytewise code for the
// whole text.
//
// The record: a memset node fills it with ones (the empty key), the decode
// kernel lowers the key and the lane that owns character E - 1 (which counts
// the pads anyway) leaves out_len, and k_strict_record (one thread per row)
// turns the key into {out_len, err_pos, err}.  No host round trip, no
// workspace, no state.
//
// The per-lane bodies (strict_lane, strict_bytes) and the structs they take
// are in b64x_strict_body.h, shared with the ragged form
// (b64x_lines_batch.hip), which keeps its records in LDS instead.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>

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

// Step 1 of the contract without the pad rules: the characters E a text of
// nchars bytes holds.  false: no E exists (*E is then the characters of its
// whole lines).
bool text_chars(uint64_t nchars, const b64x_lines *f, uint64_t *E)
{
    *E = nchars;
    if (!f || nchars == 0) return true;
    const uint64_t L = f->line_len, s = f->sep_len, P = L + s;
    const bool trailing = (f->flags & B64X_LINES_TRAILING) != 0;
    const uint64_t m = trailing ? nchars : nchars + s;
    if (m < nchars) {  // nchars + s wrapped round: no text is that long
        *E = 0;
        return false;
    }
    const uint64_t k = m / P, r = m % P;
    *E = k * L + (r > s ? r - s : 0);
    if (r != 0 && r <= s) return false;
    // the encoder's length for E characters gives nchars back
    const uint64_t lines = (*E + L - 1) / L;
    return *E + s * (lines - (trailing ? 0 : 1)) == nchars;
}

int hip_status()
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    return -EIO;
}

StrictArgs base_args(uint64_t nchars, uint64_t E, const DecAlpha &a, const b64x_lines *f,
                     uint64_t in_stride, uint64_t out_stride)
{
    StrictArgs w;
    memset(&w, 0, sizeof w);
    w.E = E;
    w.W = nchars;
    w.in_stride = in_stride;
    w.out_stride = out_stride;
    w.a = a;
    if (f) {
        w.L = f->line_len;
        w.s = f->sep_len;
        w.P = w.L + w.s;
        w.trailing = (f->flags & B64X_LINES_TRAILING) ? 1 : 0;
        for (uint32_t i = 0; i < w.s; i++) {
            w.sep |= (uint32_t) f->sep[i] << (8 * i);
            w.sep_mask |= 0xFFu << (8 * i);
        }
    }
    if (E >= 2) {
        w.off_e1 = char_offset(E - 1, w);
        w.off_e2 = char_offset(E - 2, w);
    }
    return w;
}

// The line length's reciprocals, if they are exact for this call: the 32-bit
// one for every value below `max32`, the 64-bit one for every character index.
bool set_reciprocals(StrictArgs &w, uint64_t max32)
{
    if (w.L < kLaneChars) return false;
    w.magic_l = (uint32_t) ((0xFFFFFFFFull + w.L) / w.L);
    const uint64_t err = (uint64_t) w.magic_l * w.L - (1ull << 32);  // < L
    if (max32 >= (1ull << 32) || max32 * err >= (1ull << 32)) return false;
    w.m64 = ~0ull / w.L + 1;
    return w.E <= ~0ull / w.L;  // index * (m64 L - 2^64) < 2^64
}

// Lanes [0, n) of a row are hot: their characters lie below E - 4 (the last
// group, with the pads and the unused bits, is the tail's) and their windows
// inside the text.
uint64_t count_hot_lanes(const StrictArgs &w)
{
    if (w.E < 4 + kLaneChars) return 0;
    uint64_t n = (w.E - 4) / kLaneChars;
    const uint64_t win = w.s ? 24 : 16;
    while (n > 0 && (char_offset((n - 1) * kLaneChars, w) & ~(uint64_t) 3) + win > w.W) n--;
    return n;
}

enum PlanKind { kPlanAny, kPlanOne, kPlanRows };

struct Plan {
    PlanKind kind;
    uint32_t grid;
    StrictArgs w;
};

// How a call of `nbuf` rows runs (w: base_args).
Plan make_plan(const void *d_in, const void *d_out, uint32_t nbuf, StrictArgs w)
{
    Plan p;
    const uint64_t per_row = (w.E + kLaneChars - 1) / kLaneChars;
    const bool aligned = ((((uintptr_t) d_in) | ((uintptr_t) d_out)) & 3) == 0 &&
                         (nbuf == 1 || ((w.in_stride | w.out_stride) & 3) == 0);
    const uint64_t hot = aligned ? count_hot_lanes(w) : 0;
    if (nbuf == 1 && hot > 0 && (!w.s || set_reciprocals(w, (uint64_t) w.L + kTileChars))) {
        w.hot_lanes = w.hot_slots = hot;
        w.tail_lanes = w.tail_slots = per_row - hot;
        const uint64_t tiles = (hot + kStrictTH - 1) / kStrictTH;
        const uint64_t grid = tiles + (w.tail_slots + kStrictTH - 1) / kStrictTH;
        if (grid < (1ull << 31)) {
            w.hot_tiles = (uint32_t) tiles;
            p.kind = kPlanOne;
            p.grid = (uint32_t) grid;
            p.w = w;
            return p;
        }
    }
    if (nbuf > 1 && hot > 1 && w.W < (1u << 28) && (!w.s || set_reciprocals(w, w.E))) {
        w.hot_lanes = hot;
        w.hot_slots = hot * nbuf;
        w.tail_lanes = per_row - hot;
        w.tail_slots = w.tail_lanes * nbuf;
        w.hot_lanes32 = (uint32_t) hot;
        w.magic_hl = (uint32_t) ((0xFFFFFFFFull + hot) / hot);
        w.m64_hl = ~0ull / hot + 1;
        const uint64_t err = (uint64_t) w.magic_hl * hot - (1ull << 32);
        const uint64_t tiles = (w.hot_slots + kStrictTH - 1) / kStrictTH;
        const uint64_t grid = tiles + (w.tail_slots + kStrictTH - 1) / kStrictTH;
        // exact: the lane's slot below hot + kStrictTH, the tile's below hot_slots
        if ((hot + kStrictTH) * err < (1ull << 32) && w.hot_slots <= ~0ull / hot &&
            grid < (1ull << 31)) {
            w.hot_tiles = (uint32_t) tiles;
            p.kind = kPlanRows;
            p.grid = (uint32_t) grid;
            p.w = w;
            return p;
        }
    }
    w.hot_lanes = w.hot_slots = w.tail_lanes = w.tail_slots = 0;
    w.hot_tiles = 0;
    uint64_t grid = (per_row * nbuf + kStrictTH - 1) / kStrictTH;
    if (grid > (1u << 20)) grid = 1u << 20;
    p.kind = kPlanAny;
    p.grid = (uint32_t) grid;
    p.w = w;
    return p;
}

int launch(const void *d_in, void *d_out, b64x_strict_result *d_res, uint32_t nbuf,
           const Plan &p, hipStream_t st)
{
    const uint8_t *in = (const uint8_t *) d_in;
    uint8_t *out = (uint8_t *) d_out;
    const dim3 g(p.grid), b(kStrictTH);
    if (p.kind == kPlanAny)
        hipLaunchKernelGGL(k_decode_strict_any, g, b, 0, st, in, out, d_res, nbuf, p.w);
    else if (p.kind == kPlanOne && p.w.s)
        hipLaunchKernelGGL((k_decode_strict<false, true>), g, b, 0, st, in, out, d_res, p.w);
    else if (p.kind == kPlanOne)
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
    const DecAlpha a = dec_alpha(abc);
    if (fmt && !fmt_ok(fmt, a)) return -EINVAL;
    if (!alpha_ok(a)) return -EINVAL;
    uint64_t E;
    bool has_e = text_chars(nchars, fmt, &E);
    if (strided && (in_stride < nchars || out_stride < (E + 3) / 4 * 3)) return -EINVAL;
    if (nbuf == 0) return 0;
    const int rc = b64x_device_check();
    if (rc) return rc;
    const hipStream_t st = (hipStream_t) stream;
    const uint64_t res_bytes = (uint64_t) nbuf * sizeof(b64x_strict_result);
    if (nchars == 0) {  // the empty text: {0, 0, OK}
        if (hipMemsetAsync(d_res, 0, res_bytes, st) != hipSuccess) return hip_status();
        return 0;
    }
    if (has_e && (a.pad ? E % 4 != 0 : E % 4 == 1)) has_e = false;
    const StrictArgs w = base_args(nchars, E, a, fmt, in_stride, out_stride);
    const uint32_t rgrid = (nbuf + kStrictTH - 1) / kStrictTH;
    if (has_e) {
        // the empty key in every record, then the decode lowers it
        if (hipMemsetAsync(d_res, 0xFF, res_bytes, st) != hipSuccess) return hip_status();
        const Plan p = make_plan(d_in, d_out, nbuf, w);
        const int rc2 = launch(d_in, d_out, d_res, nbuf, p, st);
        if (rc2) return rc2;
    }
    hipLaunchKernelGGL(k_strict_record, dim3(rgrid), dim3(kStrictTH), 0, st, d_res, nbuf,
                       has_e ? 0u : 1u, nchars);
    return hip_status();
}

}  // namespace

extern "C" {

uint64_t b64x_strict_decoded_cap(uint64_t nchars, const b64x_lines *fmt)
{
    if (fmt && (fmt->line_len == 0 || fmt->sep_len < 1 || fmt->sep_len > 4)) return 0;
    uint64_t E;
    text_chars(nchars, fmt, &E);
    return (E + 3) / 4 * 3;
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
