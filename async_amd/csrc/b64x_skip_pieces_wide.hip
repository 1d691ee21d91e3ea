// Strict skip decode of many pieces of any size in one call (include/b64x.h,
// b64x_decode_strict_skip_pieces_wide): what b64x_decode_strict_skip_pieces
// does, piece for piece on the same 128-byte states, with a wave per tile of
// every piece instead of a wave per piece, and with every length read on the
// device.  A translation unit and a code object of its own, linked after
// b64x_skip_wide.o; no kernel of the other units is touched.
//
// Layout ("k_skip_pw_*").  T is b64x_skip_pieces_wide_plan.h's
// function of the host bound on the call's text; every piece is cut into tiles
// of T bytes of address span from the 16-byte floor of its own address, an
// empty piece has one empty tile.  Four launches in stream order (three
// without an output), every grid fixed by the bound, the number of pieces and
// the CU count; no hand-off inside a launch, no spin, no global atomic.
//   k_skip_pw_prep    one workgroup of 1,024 lanes, a wave to a run of
//       consecutive pieces, 64 pieces to a step, eight steps' offsets loaded
//       at once.  First pass: the run's tiles and its pieces of more than 64
//       tiles; the sixteen runs meet at the kernel's barrier.  A text longer
//       than the bound, a piece longer than it or more tiles than the bound
//       allows set the BOUND flag, and nothing else is written.  Second pass:
//       a piece's head (its edges, its first tile, its tile count), the map
//       entries of its tiles (piece | tile in piece << 32; a piece of more
//       than four tiles is filled by the whole wave) and the list of the
//       pieces the scan gives a workgroup.
//   k_skip_pw_count   k_skip_wide_count's body, a wave per tile of the map.
//       A tile's record is that unit's; its offsets are offsets in the piece.
//   k_skip_pw_scan    per piece, over its own records: a workgroup for each
//       piece of the list (k_skip_wide_scan's body), then a wave for each
//       piece of at most 64 tiles, a record to a lane.  Either leaves S_t and
//       the front sextets in the records, the verdict in the record, the new
//       state, and in the piece's head whether the decode pass has anything
//       to do and whether the piece is final.  With BOUND: the records
//       {0, the text's bytes, BOUND} and nothing else.
//   k_skip_pw_decode  k_skip_wide_decode's body, a wave per tile of the map:
//       it reads its record, its piece's head and the output offset, nothing
//       of the state.
// The workspace needs no preparation: prep writes ctl, the heads, the map and
// the list before anything reads them, count writes every record the scan
// reads, the scan the words the decode pass reads.
//
// TileRec, Carry / join, data_tail_of_pass and last_kept are
// b64x_skip_wide.hip's and verdict_so_far b64x_skip_pieces.hip's, kept here as
// copies: those units' code objects stay as they are.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_skip_walk.h"
#include "b64x_skip_pieces_wide_plan.h"

namespace {

namespace plan = skip_pw_plan;

static_assert(sizeof(b64x_skip_state) == B64X_SKIP_STATE_BYTES, "the state of b64x.h");
static_assert(skip_wide_plan::kPassBytes == kPass && skip_wide_plan::kWavesPerBlock == kSkipWaves &&
                  skip_wide_plan::kBlocksPerCU == kSkipBlocksPerCU &&
                  skip_wide_plan::kTileMin % kPass == 0 && plan::kWaveTiles == kLanes,
              "the plan's sizes");

constexpr uint32_t kScanTH = kSkipTH;  // the scan's workgroup
constexpr uint32_t kScanWaves = kScanTH / kLanes;
constexpr uint32_t kScanBatch = 4;     // records a lane has in flight
constexpr uint32_t kPrepTH = (uint32_t) plan::kPrepLanes;
constexpr uint32_t kPrepWaves = kPrepTH / kLanes;
constexpr uint32_t kPrepBatch = 8;     // steps whose offsets are loaded at once
constexpr uint32_t kFillAlone = 4;     // a lane fills the map of a piece of up to so many tiles

struct TileRec {
    uint64_t kept, pads, first_char, first_pad, d, tail, S, cs;
};
static_assert(sizeof(TileRec) == plan::kRecordBytes, "a tile's record");

// A piece's head: flags is the scan's (bit 0: the decode pass has nothing to
// do, bit 1: the piece is final), the rest prep's.
struct Head {
    uint64_t flags, beg, len, first, nt, spare[3];
};
static_assert(sizeof(Head) == plan::kHeadBytes, "a piece's head");

constexpr uint64_t kHeadIdle = 1, kHeadFinal = 2;

// ctl's words.
constexpr uint32_t kCtlTiles = 0, kCtlBound = 1, kCtlText = 2, kCtlBig = 3;

// A value that is the same in every lane, as one.
DEV uint32_t uniform(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
DEV uint64_t uniform(uint64_t v)
{
    return ((uint64_t) uniform((uint32_t) (v >> 32)) << 32) | uniform((uint32_t) v);
}

DEV uint64_t lane_value(uint64_t v, uint32_t l)
{
    return ((uint64_t) (uint32_t) __shfl((int) (v >> 32), (int) l) << 32) |
           (uint32_t) __shfl((int) (uint32_t) v, (int) l);
}

// Data characters and the last min(3, d) of their sextets, the last one in
// bits 0..5; the fields above them are zero.
struct Carry {
    uint64_t d;
    uint32_t v;
};

constexpr uint32_t kCarryMask = 0x3FFFFu;

// a, then b.
DEV Carry join(const Carry &a, const Carry &b)
{
    const uint32_t n = b.d < 3 ? (uint32_t) b.d : 3u;
    Carry r;
    r.d = a.d + b.d;
    r.v = (n == 3 ? 0u : (a.v << (6 * n)) & kCarryMask) | b.v;
    return r;
}

// The last r (0..3) sextets of v as they stand at the front of a sextet
// buffer and in word 8 of the state: a byte each, the oldest lowest.
DEV uint32_t front_sextets(uint32_t v, uint32_t r)
{
    uint32_t cs = 0;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
        if (i < r) cs |= ((v >> (6 * (r - 1 - i))) & 0x3Fu) << (8 * i);
    return cs;
}

// The last (up to) three data sextets of a pass, a chunk to a lane, behind
// those of the passes before.
DEV void data_tail_of_pass(const uint32_t *tab, const Chunk &ch, uint32_t lane, uint32_t *tail)
{
    uint32_t left = 0;
#pragma unroll
    for (uint32_t i = 0; i < kChunk; i++) left |= (tab[chunk_byte(ch, i)] >> 31) << i;
    left &= ch.valid;
    uint32_t v = 0, n = 0;
#pragma unroll
    for (uint32_t found = 0; found < 3; found++) {
        const uint64_t holders = __ballot(left != 0);
        if (holders == 0) break;
        const uint32_t top = 63u - (uint32_t) __clzll((long long) holders);
        const uint32_t mt = (uint32_t) __shfl((int) left, (int) top);
        const uint32_t j = 31u - (uint32_t) __clz((int) mt);
        const uint32_t word = j < 4 ? ch.w[0] : j < 8 ? ch.w[1] : j < 12 ? ch.w[2] : ch.w[3];
        const uint32_t byte = ((uint32_t) __shfl((int) word, (int) top) >> (8 * (j & 3))) & 0xFFu;
        v |= (tab[byte] & 0x3Fu) << (6 * found);
        n++;
        if (lane == top) left &= ~(1u << j);
    }
    *tail = (n == 3 ? 0u : (*tail << (6 * n)) & kCarryMask) | v;
}

// Steps 2 and 3 of the procedure of b64x.h on the text so far: the offences
// that more text cannot take back (b64x_skip_pieces.hip's, a copy).
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

// The last `want` (<= 3, <= the piece's kept bytes) kept bytes of the piece,
// the last one first, with their offsets in it (b64x_skip.hip's, a copy): the
// wave walks backwards from the 16-byte boundary at or above the end in steps
// of a pass, a chunk to a lane.
DEV Last3 last_kept(uintptr_t lo, uintptr_t hi, uint32_t lane, uint32_t want, const SkipSet &k)
{
    Last3 r = {};
    uint32_t found = 0;
    uintptr_t end = (hi + kChunk - 1) & ~(uintptr_t) (kChunk - 1);
    while (found < want && end > lo) {
        const uintptr_t base = end - kPass;
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

// The chunks of tile t of a piece: its first one, and how many.
struct TileSpan {
    uint64_t first, n;
};

DEV TileSpan tile_span(uint64_t t, uint64_t tile_chunks, uint64_t chunks)
{
    TileSpan s;
    s.first = t * tile_chunks;
    s.n = s.first < chunks ? (chunks - s.first < tile_chunks ? chunks - s.first : tile_chunks) : 0;
    return s;
}

// Tiles of a piece of len bytes whose first byte stands head bytes behind a
// 16-byte boundary (plan::piece_tiles; len + head does not wrap: len is at
// most the bound, and a longer one has set BOUND before this counts).
DEV uint64_t tiles_of(uint64_t len, uint32_t head, uint64_t tile, uint32_t shift)
{
    if (len == 0) return 1;
    const uint64_t span = len > UINT64_MAX - head ? UINT64_MAX : len + head;
    if (shift) return (span >> shift) + ((span & (tile - 1)) != 0);
    return span / tile + (span % tile != 0);
}

// What a state holds of the text so far.
struct StateIn {
    uint64_t pos, E0, c0, fc, fp, p0, p1, p2, w8;
};

DEV StateIn load_state(const uint64_t *st)
{
    StateIn s;
    s.pos = uniform(st[0]);  // the text offset of the piece's byte 0
    s.E0 = uniform(st[1]);
    s.c0 = uniform(st[2]);
    s.fc = uniform(st[3]);
    s.fp = uniform(st[4]);
    s.p0 = uniform(st[5]);
    s.p1 = uniform(st[6]);
    s.p2 = uniform(st[7]);
    s.w8 = uniform(st[8]);
    return s;
}

// The sextets the pieces before left over.
DEV Carry carry_of(const StateIn &s)
{
    const uint32_t cin = (uint32_t) (s.w8 >> 24) & 3u;
    Carry pre = {cin, 0};
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
        if (i < cin) pre.v = (pre.v << 6) | ((uint32_t) (s.w8 >> (32 + 8 * i)) & 0x3Fu);
    return pre;
}

// A state that holds a report: the same record, and nothing else.  One wave.
DEV void repeat_report(uint64_t *st, uint32_t kind, bool final, uint32_t lane, Head *head,
                       b64x_strict_result *res)
{
    b64x_strict_result r;
    r.out_len = 0;
    r.err_pos = st[10];
    r.err = kind;
    r.reserved = 0;
    if (lane == 0) {
        *res = r;
        head->flags = kHeadIdle | (final ? kHeadFinal : 0);
    }
    if (final && lane < 16) st[lane] = 0;
}

// One wave, behind the scan of a piece's records: the piece's totals `tot`
// and the carry with every tile `all` give the verdict, the record, the new
// state and the head's flags (k_skip_wide_scan's last part).
DEV void finish_piece(uint64_t *st, const StateIn &in, const Slot &tot, const Carry &all,
                      uintptr_t lo, uint64_t len, bool final, uint32_t decode, uint32_t lane,
                      Head *head, b64x_strict_result *res, const Alpha &a, const SkipSet &k)
{
    const uint64_t pos = in.pos;
    // the text so far: the state's totals and the piece's
    Slot T;
    T.E = in.E0 + tot.E;
    T.c = in.c0 + tot.c;
    T.first_char = in.fc ? in.fc - 1 : tot.first_char != kNone ? pos + tot.first_char : kNone;
    T.first_pad = in.fp ? in.fp - 1 : tot.first_pad != kNone ? pos + tot.first_pad : kNone;
    // its last three kept bytes: the piece's, then the state's own
    const uint32_t want = tot.E < 3 ? (uint32_t) tot.E : 3u;
    Last3 f = {};
    if (want) f = last_kept(lo, lo + len, lane, want, k);
    const uint32_t ob0 = (uint32_t) in.w8 & 0xFFu, ob1 = (uint32_t) (in.w8 >> 8) & 0xFFu,
                   ob2 = (uint32_t) (in.w8 >> 16) & 0xFFu;
    const uint32_t f0 = f.byte[0], f1 = f.byte[1], f2 = f.byte[2];
    const uint64_t g0 = pos + f.off[0], g1 = pos + f.off[1], g2 = pos + f.off[2];
    Last3 last;
    last.byte[0] = want >= 1 ? f0 : ob0;
    last.off[0] = want >= 1 ? g0 : in.p0;
    last.byte[1] = want >= 2 ? f1 : want == 1 ? ob0 : ob1;
    last.off[1] = want >= 2 ? g1 : want == 1 ? in.p0 : in.p1;
    last.byte[2] = want == 3 ? f2 : want == 2 ? ob0 : want == 1 ? ob1 : ob2;
    last.off[2] = want == 3 ? g2 : want == 2 ? in.p0 : want == 1 ? in.p1 : in.p2;
    // Without an offence every kept byte is a data character or a pad
    // character, so this is what the piece has to decode, carry included.
    const uint64_t kd = all.d;
    b64x_strict_result r;
    if (final) {
        r = skip_verdict(pos + len, T, last, a);
        if (r.err == B64X_STRICT_OK) r.out_len = decoded_len(kd);  // what this piece writes
        if (lane < 16) st[lane] = 0;
    } else {
        r = verdict_so_far(T, last, a);
        if (r.err == B64X_STRICT_OK) r.out_len = kd / 4 * 3;
        if (lane == 0) {
            const uint64_t left = decode ? front_sextets(all.v, (uint32_t) kd & 3u) : 0u;
            st[0] = pos + len;
            st[1] = T.E;
            st[2] = T.c;
            st[3] = T.first_char + 1;  // kNone: 0
            st[4] = T.first_pad + 1;
            st[5] = last.off[0];
            st[6] = last.off[1];
            st[7] = last.off[2];
            st[8] = last.byte[0] | (last.byte[1] << 8) | (last.byte[2] << 16) |
                    ((uint32_t) (kd & 3u) << 24) | (left << 32);
            st[9] = r.err;
            st[10] = r.err_pos;
        }
    }
    if (lane == 0) {
        *res = r;
        // with an offence the decode pass writes nothing
        head->flags = (r.err != B64X_STRICT_OK ? kHeadIdle : 0) | (final ? kHeadFinal : 0);
    }
}

// ------------------------------------------------------------- kernels --

// One workgroup: every piece's tiles, their prefix, the map and the list.
__global__ __launch_bounds__(kPrepTH) void k_skip_pw_prep(
    const uint8_t *in, const uint64_t *__restrict__ in_off, uint32_t npieces, uint64_t total_cap,
    uint64_t tile, uint32_t shift, uint64_t bound, uint64_t *__restrict__ ctl,
    Head *__restrict__ heads, uint64_t *__restrict__ map, uint32_t *__restrict__ big)
{
    __shared__ uint64_t wtiles[kPrepWaves];
    __shared__ uint32_t wbig[kPrepWaves], wbad[kPrepWaves];
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const uint64_t text = uniform(in_off[npieces]) - uniform(in_off[0]);
    // this wave's run of pieces: whole steps
    const uint64_t run = (((uint64_t) npieces + kPrepWaves - 1) / kPrepWaves + kLanes - 1) / kLanes * kLanes;
    const uint64_t p0 = wv * run < npieces ? wv * run : npieces;
    const uint64_t p1 = p0 + run < npieces ? p0 + run : npieces;
    uint64_t my_tiles = 0;
    uint32_t my_big = 0, my_bad = 0;
    for (uint64_t i0 = p0; i0 < p1; i0 += kLanes * kPrepBatch) {
        uint64_t b[kPrepBatch], e[kPrepBatch];
#pragma unroll
        for (uint32_t j = 0; j < kPrepBatch; j++) {
            const uint64_t i = i0 + kLanes * j + lane;
            b[j] = e[j] = 0;
            if (i < p1) b[j] = in_off[i], e[j] = in_off[i + 1];
        }
#pragma unroll
        for (uint32_t j = 0; j < kPrepBatch; j++) {
            const uint64_t i = i0 + kLanes * j + lane;
            if (i >= p1) continue;
            const uint64_t len = e[j] - b[j];
            if (len > total_cap) {
                my_bad = 1;
                continue;
            }
            const uint64_t nt = tiles_of(len, (uint32_t) ((uintptr_t) in + b[j]) & (kChunk - 1), tile, shift);
            my_tiles += nt;
            my_big += nt > plan::kWaveTiles;
        }
    }
#pragma unroll
    for (uint32_t d = 1; d < kLanes; d <<= 1) {
        my_tiles += __shfl_xor((unsigned long long) my_tiles, d);
        my_big += (uint32_t) __shfl_xor((int) my_big, d);
        my_bad |= (uint32_t) __shfl_xor((int) my_bad, d);
    }
    if (lane == 0) wtiles[wv] = my_tiles, wbig[wv] = my_big, wbad[wv] = my_bad;
    block_sync();
    uint64_t tiles_before = 0, tiles_all = 0;
    uint32_t big_before = 0, big_all = 0, bad = text > total_cap;
#pragma nounroll
    for (uint32_t w = 0; w < kPrepWaves; w++) {
        if (w < wv) tiles_before += wtiles[w], big_before += wbig[w];
        tiles_all += wtiles[w];
        big_all += wbig[w];
        bad |= wbad[w];
    }
    bad |= tiles_all > bound;
    if (threadIdx.x == 0) {
        ctl[kCtlTiles] = bad ? 0 : tiles_all;
        ctl[kCtlBound] = bad;
        ctl[kCtlText] = text;
        ctl[kCtlBig] = bad ? 0 : big_all;
    }
    if (bad) return;  // nothing of the call is looked at
    // Every entry written below lies under tiles_all <= bound, every list
    // entry under big_all <= bound / 65.
    for (uint64_t i0 = p0; i0 < p1; i0 += kLanes * kPrepBatch) {
        uint64_t b[kPrepBatch], e[kPrepBatch];
#pragma unroll
        for (uint32_t j = 0; j < kPrepBatch; j++) {
            const uint64_t i = i0 + kLanes * j + lane;
            b[j] = e[j] = 0;
            if (i < p1) b[j] = in_off[i], e[j] = in_off[i + 1];
        }
#pragma unroll
        for (uint32_t j = 0; j < kPrepBatch; j++) {  // unrolled: b and e stay in registers
            const uint64_t i = i0 + kLanes * j + lane;
            if (i0 + kLanes * j >= p1) continue;  // the same in every lane
            const bool mine = i < p1;
            const uint64_t len = e[j] - b[j];
            const uint32_t nt = mine ? (uint32_t) tiles_of(len, (uint32_t) ((uintptr_t) in + b[j]) & (kChunk - 1),
                                                            tile, shift) : 0u;  // <= 16,384
            // the step's exclusive prefix: 64 x 16,384 fits 32 bits
            uint32_t incl = nt;
#pragma unroll
            for (uint32_t d = 1; d < kLanes; d <<= 1) {
                const uint32_t up = (uint32_t) __shfl_up((int) incl, d);
                if (lane >= d) incl += up;
            }
            const uint64_t first = tiles_before + (incl - nt);
            const uint64_t bigs = __ballot(nt > plan::kWaveTiles);
            if (mine) {
                Head h = {0, b[j], len, first, nt, {0, 0, 0}};
                heads[i] = h;
                if (nt <= kFillAlone)
                    for (uint32_t t = 0; t < nt; t++) map[first + t] = i | ((uint64_t) t << 32);
                if (nt > plan::kWaveTiles)
                    big[big_before + (uint32_t) __popcll(bigs & ((1ull << lane) - 1))] = (uint32_t) i;
            }
            // the map of a longer piece: the wave's lanes side by side
            for (uint64_t rest = __ballot(nt > kFillAlone); rest; rest &= rest - 1) {
                const uint32_t l = (uint32_t) __builtin_ctzll(rest);
                const uint64_t f = lane_value(first, l), piece = i0 + kLanes * j + l;
                const uint32_t n = (uint32_t) __shfl((int) nt, (int) l);
                for (uint32_t t = lane; t < n; t += kLanes) map[f + t] = piece | ((uint64_t) t << 32);
            }
            tiles_before += (uint32_t) __shfl((int) incl, (int) (kLanes - 1));
            big_before += (uint32_t) __popcll(bigs);
        }
    }
}

// What a wave knows of the tile it takes next, loaded a tile ahead.
struct TileOf {
    uint64_t piece, tin, beg, len;
};

// Wave g of G takes tiles g, g + G, ... of the map: a tile's totals into its record.
__global__ __launch_bounds__(kSkipTH) void k_skip_pw_count(
    const uint8_t *__restrict__ in, uint64_t tile_chunks, const uint64_t *__restrict__ ctl,
    const Head *__restrict__ heads, const uint64_t *__restrict__ map,
    const b64x_skip_state *__restrict__ state, const uint32_t *__restrict__ sid,
    TileRec *__restrict__ recs, Alpha a, SkipSet k)
{
    __shared__ uint32_t tab[256];
    const uint64_t ntiles = uniform(ctl[kCtlTiles]);  // with BOUND: none
    build_row_table(tab, a, k);
    block_sync();
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    uint64_t t = (uint64_t) blockIdx.x * kSkipWaves + wv;
    // a tile's place is loaded a tile ahead, its piece's edges behind that
    uint64_t m = 0, m_next = 0;
    if (t < ntiles) m = uniform(map[t]);
    if (t + waves < ntiles) m_next = uniform(map[t + waves]);
    for (; t < ntiles; t += waves) {
        const uint64_t piece = m & 0xFFFFFFFFu, tin = m >> 32;
        const uint64_t beg = uniform(heads[piece].beg), len = uniform(heads[piece].len);
        const uint64_t sx = sid ? (uint64_t) uniform(sid[piece]) : piece;
        m = m_next;
        if (t + 2 * waves < ntiles) m_next = uniform(map[t + 2 * waves]);
        const uintptr_t lo = (uintptr_t) in + beg, hi = lo + len;
        const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
        const uint64_t chunks = chunk_count(lo, len);
        const TileSpan ts = tile_span(tin, tile_chunks, chunks);
        const uintptr_t At = A0 + kChunk * ts.first;
        const uint64_t base0 = (uint64_t) (At - lo);  // the piece offset of the tile's byte 0 (wraps)
        Chunk next = {};
        if (lane < ts.n) next = load_chunk(At + kChunk * lane, lo, hi);
        // a text that was refused: the piece is not looked at
        if (uniform((uint32_t) state[sx].w[9]) != B64X_STRICT_OK) continue;
        Slot s = {0, 0, kNone, kNone};  // c and the first offences: the wave's, the same in every lane
        uint64_t kept_here = 0, data_here = 0;  // this lane's; summed behind the last pass
        // The last pass with data characters in three lanes or more: its last
        // three are the tile's so far, and are looked for only when no later
        // pass takes its place.
        Chunk pend = {};
        bool pending = false;
        uint32_t tail = 0;
        for (uint64_t q0 = 0; q0 < ts.n; q0 += kLanes) {
            const Chunk ch = next;
            // the next pass's chunk is on its way while this one is worked on
            const uint64_t qn = q0 + kLanes + lane;
            next = Chunk{};
            if (qn < ts.n) next = load_chunk(At + kChunk * qn, lo, hi);
            uint32_t t16[kChunk];
            classify_chunk(tab, ch, t16);
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t i = 0; i < kChunk; i++) sum += t16[i];
            const uint32_t nkept = (sum >> kCntShift) & 31u, npadc = (sum >> kPadShift) & 31u,
                           nstranger = (sum >> kStrangerShift) & 31u;
            const uint32_t mine = nkept - npadc - nstranger;
            kept_here += nkept;
            data_here += mine;
            // pad characters and strangers are few: the lanes that hold some, one by one
            for (uint64_t rest = __ballot((npadc | nstranger) != 0); rest; rest &= rest - 1) {
                const uint32_t l = (uint32_t) __builtin_ctzll(rest);
                uint32_t pm = 0, sm = 0;
#pragma unroll
                for (uint32_t i = 0; i < kChunk; i++) {
                    const uint32_t ti = (uint32_t) __builtin_amdgcn_readlane((int) t16[i], (int) l);
                    pm |= ((ti >> kPadShift) & 1u) << i;
                    sm |= ((ti >> kStrangerShift) & 1u) << i;
                }
                const uint64_t off = base0 + kChunk * (q0 + l);
                s.c += (uint32_t) __popc(pm);
                if (pm && s.first_pad == kNone) s.first_pad = off + (uint32_t) __builtin_ctz(pm);
                if (sm && s.first_char == kNone) s.first_char = off + (uint32_t) __builtin_ctz(sm);
            }
            if (__popcll(__ballot(mine != 0)) >= 3) {
                pend = ch;
                pending = true;
            } else {
                if (pending) data_tail_of_pass(tab, pend, lane, &tail);
                pending = false;
                data_tail_of_pass(tab, ch, lane, &tail);
            }
        }
        if (pending) data_tail_of_pass(tab, pend, lane, &tail);
#pragma unroll
        for (uint32_t d = 1; d < kLanes; d <<= 1) {
            kept_here += __shfl_xor((unsigned long long) kept_here, d);
            data_here += __shfl_xor((unsigned long long) data_here, d);
        }
        // eight words, a lane each
        const uint64_t w = lane == 0 ? kept_here : lane == 1 ? s.c : lane == 2 ? s.first_char
                         : lane == 3 ? s.first_pad : lane == 4 ? data_here : lane == 5 ? tail : 0;
        if (lane < 8) ((uint64_t *) &recs[t])[lane] = w;
    }
}

// The records of one piece by one workgroup (k_skip_wide_scan's body): a lane
// folds a strip of consecutive records, a wave scans its lanes, the waves
// meet at the barrier, wave 0 finishes the piece.  wtot: this round's.
DEV void scan_by_block(uint64_t (*wtot)[6], const uint8_t *in, Head *head, uint64_t *st, bool final,
                       uint32_t decode, TileRec *all_recs, b64x_strict_result *res, const Alpha &a,
                       const SkipSet &k)
{
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const uint64_t ntiles = uniform(head->nt);
    TileRec *const recs = all_recs + uniform(head->first);
    const StateIn sin = load_state(st);
    Carry pre = carry_of(sin);
    // a strip of consecutive records to a lane
    const uint64_t per = (ntiles + kScanTH - 1) / kScanTH;
    const uint64_t beg = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles;
    const uint64_t end = beg + per < ntiles ? beg + per : ntiles;
    Slot s = {0, 0, kNone, kNone};
    Carry inc = {0, 0};
    for (uint64_t t = beg; t < end; t += kScanBatch) {
        // the loads of a batch first: they do not wait for one another
        TileRec r[kScanBatch];
#pragma unroll
        for (uint32_t i = 0; i < kScanBatch; i++) {
            r[i] = TileRec{0, 0, kNone, kNone, 0, 0, 0, 0};
            if (t + i < end) {
                const TileRec &g = recs[t + i];
                r[i].kept = g.kept;
                r[i].pads = g.pads;
                r[i].first_char = g.first_char;
                r[i].first_pad = g.first_pad;
                r[i].d = g.d;
                r[i].tail = g.tail;
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < kScanBatch; i++) {
            s.E += r[i].kept;
            s.c += r[i].pads;
            if (r[i].first_char < s.first_char) s.first_char = r[i].first_char;
            if (r[i].first_pad < s.first_pad) s.first_pad = r[i].first_pad;
            inc = join(inc, Carry{r[i].d, (uint32_t) r[i].tail});  // d == 0 changes nothing
        }
    }
    // the wave's inclusive scan of its strips, and its totals
#pragma unroll
    for (uint32_t d = 1; d < kLanes; d <<= 1) {
        Carry up;
        up.d = __shfl_up((unsigned long long) inc.d, d);
        up.v = (uint32_t) __shfl_up((int) inc.v, d);
        if (lane >= d) inc = join(up, inc);
    }
    s = wave_fold(s);
    if (lane == kLanes - 1) {
        wtot[wv][0] = inc.d;
        wtot[wv][1] = inc.v;
        wtot[wv][2] = s.E;
        wtot[wv][3] = s.c;
        wtot[wv][4] = s.first_char;
        wtot[wv][5] = s.first_pad;
    }
    block_sync();
    Carry all = pre;  // the carry and every tile
    Slot tot = {0, 0, kNone, kNone};
#pragma nounroll
    for (uint32_t w = 0; w < kScanWaves; w++) {
        const Carry cw = {wtot[w][0], (uint32_t) wtot[w][1]};
        if (w < wv) pre = join(pre, cw);
        all = join(all, cw);
        tot.E += wtot[w][2];
        tot.c += wtot[w][3];
        if (wtot[w][4] < tot.first_char) tot.first_char = wtot[w][4];
        if (wtot[w][5] < tot.first_pad) tot.first_pad = wtot[w][5];
    }
    if (decode) {
        // S_t and the sextets tile t starts with, into its record
        Carry ex;
        ex.d = __shfl_up((unsigned long long) inc.d, 1);
        ex.v = (uint32_t) __shfl_up((int) inc.v, 1);
        if (lane == 0) ex = Carry{0, 0};
        Carry run = join(pre, ex);
        for (uint64_t t = beg; t < end; t += kScanBatch) {
            Carry c[kScanBatch];
#pragma unroll
            for (uint32_t i = 0; i < kScanBatch; i++) {
                c[i] = Carry{0, 0};
                if (t + i < end) c[i] = Carry{recs[t + i].d, (uint32_t) recs[t + i].tail};
            }
#pragma unroll
            for (uint32_t i = 0; i < kScanBatch; i++) {
                if (t + i < end) {
                    recs[t + i].S = run.d;
                    recs[t + i].cs = front_sextets(run.v, (uint32_t) run.d & 3u);
                }
                run = join(run, c[i]);
            }
        }
    }
    if (wv != 0) return;
    finish_piece(st, sin, tot, all, (uintptr_t) in + uniform(head->beg), uniform(head->len), final,
                 decode, lane, head, res, a, k);
}

// The records of one piece of at most 64 tiles by one wave, a record to a lane.
DEV void scan_by_wave(const uint8_t *in, Head *head, uint32_t ntiles, uint64_t *st, bool final,
                      uint32_t decode, TileRec *all_recs, b64x_strict_result *res, const Alpha &a,
                      const SkipSet &k)
{
    const uint32_t lane = threadIdx.x % kLanes;
    TileRec *const rec = all_recs + uniform(head->first) + lane;
    const StateIn sin = load_state(st);
    const Carry pre = carry_of(sin);
    Slot s = {0, 0, kNone, kNone};
    Carry mine = {0, 0};
    if (lane < ntiles) {
        s.E = rec->kept;
        s.c = rec->pads;
        s.first_char = rec->first_char;
        s.first_pad = rec->first_pad;
        mine = Carry{rec->d, (uint32_t) rec->tail};
    }
    Carry inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < kLanes; d <<= 1) {
        Carry up;
        up.d = __shfl_up((unsigned long long) inc.d, d);
        up.v = (uint32_t) __shfl_up((int) inc.v, d);
        if (lane >= d) inc = join(up, inc);
    }
    // the lanes behind the last record hold nothing: the last lane has every tile
    Carry every;
    every.d = lane_value(inc.d, kLanes - 1);
    every.v = (uint32_t) __shfl((int) inc.v, (int) (kLanes - 1));
    const Carry all = join(pre, every);
    if (decode) {
        Carry ex;
        ex.d = __shfl_up((unsigned long long) inc.d, 1);
        ex.v = (uint32_t) __shfl_up((int) inc.v, 1);
        if (lane == 0) ex = Carry{0, 0};
        const Carry run = join(pre, ex);
        if (lane < ntiles) {
            rec->S = run.d;
            rec->cs = front_sextets(run.v, (uint32_t) run.d & 3u);
        }
    }
    const Slot tot = wave_fold(s);
    finish_piece(st, sin, tot, all, (uintptr_t) in + uniform(head->beg), uniform(head->len), final,
                 decode, lane, head, res, a, k);
}

// Per piece: the records' totals and prefixes, the verdict, the new state.
__global__ __launch_bounds__(kScanTH) void k_skip_pw_scan(
    const uint8_t *in, uint32_t npieces, b64x_skip_state *state, const uint32_t *__restrict__ sid,
    const uint8_t *__restrict__ flags, uint32_t decode, const uint64_t *__restrict__ ctl, Head *heads,
    TileRec *recs, const uint32_t *__restrict__ big, b64x_strict_result *res, Alpha a, SkipSet k)
{
    // d, sextets, E, c, first_char, first_pad of a wave; two rounds' worth, so
    // that a round's one barrier also parts its reads from the writes of the
    // round after the next
    __shared__ uint64_t wtot[2][kScanWaves][6];
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    if (uniform((uint32_t) ctl[kCtlBound])) {
        // the pieces are longer than the caller's bound: nothing was looked at
        b64x_strict_result r;
        r.out_len = 0;
        r.err_pos = uniform(ctl[kCtlText]);
        r.err = B64X_STRICT_BOUND;
        r.reserved = 0;
        for (uint64_t p = (uint64_t) blockIdx.x * kScanTH + threadIdx.x; p < npieces;
             p += (uint64_t) gridDim.x * kScanTH)
            res[p] = r;
        return;
    }
    // the pieces of more than 64 tiles, a workgroup each
    const uint32_t nbig = uniform((uint32_t) ctl[kCtlBig]);
    uint32_t round = 0;
    for (uint32_t j = blockIdx.x; j < nbig; j += gridDim.x) {
        const uint64_t p = uniform(big[j]);
        const bool final = flags && (uniform((uint32_t) flags[p]) & B64X_PIECE_FINAL);
        uint64_t *const st = state[sid ? (uint64_t) uniform(sid[p]) : p].w;
        const uint32_t kind = uniform((uint32_t) st[9]);
        if (kind != B64X_STRICT_OK) {  // the same for the whole workgroup
            if (wv == 0) repeat_report(st, kind, final, lane, &heads[p], &res[p]);
            continue;
        }
        scan_by_block(wtot[round & 1], in, &heads[p], st, final, decode, recs, &res[p], a, k);
        round++;
    }
    // the others, a wave each
    for (uint64_t p = (uint64_t) blockIdx.x * kScanWaves + wv; p < npieces;
         p += (uint64_t) gridDim.x * kScanWaves) {
        const uint32_t ntiles = uniform((uint32_t) heads[p].nt);
        if (ntiles > plan::kWaveTiles) continue;
        const bool final = flags && (uniform((uint32_t) flags[p]) & B64X_PIECE_FINAL);
        uint64_t *const st = state[sid ? (uint64_t) uniform(sid[p]) : p].w;
        const uint32_t kind = uniform((uint32_t) st[9]);
        if (kind != B64X_STRICT_OK) {
            repeat_report(st, kind, final, lane, &heads[p], &res[p]);
            continue;
        }
        scan_by_wave(in, &heads[p], ntiles, st, final, decode, recs, &res[p], a, k);
    }
}

// Wave g of G takes tiles g, g + G, ... of the map: a tile's groups to their place.
__global__ __launch_bounds__(kSkipTH) void k_skip_pw_decode(
    const uint8_t *__restrict__ in, uint64_t tile_chunks, uint8_t *__restrict__ out,
    const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ ctl,
    const Head *__restrict__ heads, const uint64_t *__restrict__ map,
    const TileRec *__restrict__ recs, Alpha a, SkipSet k)
{
    __shared__ uint32_t tab[256];
    // a wave's sextets, and behind them a byte per lane for what is no sextet
    __shared__ __attribute__((aligned(16))) uint8_t sextets[kSkipWaves][kSextets + kLanes];
    const uint64_t ntiles = uniform(ctl[kCtlTiles]);  // with BOUND: none
    build_row_table(tab, a, k);
    block_sync();
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    uint8_t *const sx = sextets[wv];
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    uint64_t t = (uint64_t) blockIdx.x * kSkipWaves + wv;
    // a tile's place is loaded a tile ahead, its piece's head behind that
    uint64_t m = 0, m_next = 0;
    if (t < ntiles) m = uniform(map[t]);
    if (t + waves < ntiles) m_next = uniform(map[t + waves]);
    for (; t < ntiles; t += waves) {
        const uint64_t piece = m & 0xFFFFFFFFu, tin = m >> 32;
        const Head &h = heads[piece];
        const uint64_t hflags = uniform(h.flags), beg = uniform(h.beg), len = uniform(h.len),
                       nt = uniform(h.nt);
        const uint64_t obase = uniform(out_off[piece]);
        m = m_next;
        if (t + 2 * waves < ntiles) m_next = uniform(map[t + 2 * waves]);
        if (hflags & kHeadIdle) continue;  // a report, old or new
        const uintptr_t lo = (uintptr_t) in + beg, hi = lo + len;
        const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
        const uint64_t chunks = chunk_count(lo, len);
        const TileSpan ts = tile_span(tin, tile_chunks, chunks);
        const uintptr_t At = A0 + kChunk * ts.first;
        Chunk next = {};
        if (lane < ts.n) next = load_chunk(At + kChunk * lane, lo, hi);
        const uint64_t S = uniform(recs[t].S);
        const uint32_t cs = uniform((uint32_t) recs[t].cs);
        uint8_t *rout = out + obase + 3 * (S >> 2);
        uint32_t carry = (uint32_t) S & 3u;  // sextets at the front of sx, < kUnit
        uint64_t units = 0;                  // units stored so far
        if (lane < carry) sx[lane] = (uint8_t) (cs >> (8 * (lane & 3u))) & 0x3Fu;
        wave_lds_order();
        for (uint64_t q0 = 0; q0 < ts.n; q0 += kLanes) {
            const Chunk ch = next;
            // the next pass's chunk is on its way while this one is worked on
            const uint64_t qn = q0 + kLanes + lane;
            next = Chunk{};
            if (qn < ts.n) next = load_chunk(At + kChunk * qn, lo, hi);
            uint32_t t16[kChunk];
            classify_chunk(tab, ch, t16);
            // place: this lane's data characters behind those of the lanes below
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t i = 0; i < kChunk; i++) mine += t16[i] >> 31;
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
                const bool is_data = (int32_t) t16[i] < 0;
                sx[is_data ? at : spare] = (uint8_t) t16[i];
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
        // the carry's whole groups and, behind the last tile of a final piece,
        // the text's partial one: byte i of them comes from two neighbouring
        // sextets; at most 11 bytes.  What is left is the next tile's front.
        const bool last = (hflags & kHeadFinal) && tin == nt - 1;
        const uint32_t nbytes = last ? (uint32_t) decoded_len(carry) : carry / 4 * 3;
        if (lane < nbytes) {
            const uint32_t g = lane / 3, r = lane % 3;
            const uint32_t x = sx[4 * g + r], y = sx[4 * g + r + 1];
            const uint32_t byte = r == 0 ? (x << 2) | (y >> 4) : r == 1 ? (x << 4) | (y >> 2) : (x << 6) | y;
            rout[12 * units + lane] = (uint8_t) byte;
        }
        wave_lds_order();  // the next tile's sextets come after these reads
    }
}

}  // namespace

extern "C" {

uint64_t b64x_strict_skip_pieces_wide_workspace_size(uint64_t total_cap, uint32_t npieces,
                                                     bool validate_only)
{
    (void) validate_only;  // the count pass and the scan want the records either way
    return plan::workspace_bytes(total_cap, npieces);
}

int b64x_decode_strict_skip_pieces_wide(const void *d_in, const uint64_t *d_in_off, uint32_t npieces,
                                        uint64_t total_cap, void *d_out, const uint64_t *d_out_off,
                                        b64x_skip_state *d_state, const uint32_t *d_sid,
                                        const uint8_t *d_flags, b64x_strict_result *d_res,
                                        const b64x_alphabet *abc, const b64x_skip *skip,
                                        void *d_workspace, void *stream)
{
    if (npieces == 0) return 0;
    if (!d_in || !d_in_off || !d_state || !d_res || !d_workspace) return -EINVAL;
    if ((((uintptr_t) d_res) | ((uintptr_t) d_state) | ((uintptr_t) d_workspace)) & 7) return -EINVAL;
    if (d_out && !d_out_off) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    SkipSet k;
    if (!make_skip(skip, a, &k)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t cus = 0;
    if ((rc = device_cus(&cus)) != 0) return rc;
    const uint8_t *in = (const uint8_t *) d_in;
    const uint64_t tile = plan::tile_bytes(total_cap);
    const uint64_t bound = plan::tile_bound(total_cap, npieces);
    const plan::Layout l = plan::layout(total_cap, npieces);
    uint8_t *const ws = (uint8_t *) d_workspace;
    uint64_t *ctl = (uint64_t *) ws;
    Head *heads = (Head *) (ws + l.heads);
    TileRec *recs = (TileRec *) (ws + l.records);
    uint64_t *map = (uint64_t *) (ws + l.map);
    uint32_t *big = (uint32_t *) (ws + l.big);
    const uint32_t grid = plan::tile_grid(total_cap, npieces, cus);
    const hipStream_t st = (hipStream_t) stream;
    hipLaunchKernelGGL(k_skip_pw_prep, dim3(1), dim3(kPrepTH), 0, st, in, d_in_off, npieces, total_cap,
                       tile, plan::tile_shift(total_cap), bound, ctl, heads, map, big);
    if ((rc = hip_status()) != 0) return rc;
    hipLaunchKernelGGL(k_skip_pw_count, dim3(grid), dim3(kSkipTH), 0, st, in, tile / kChunk,
                       (const uint64_t *) ctl, (const Head *) heads, (const uint64_t *) map,
                       (const b64x_skip_state *) d_state, d_sid, recs, a, k);
    if ((rc = hip_status()) != 0) return rc;
    hipLaunchKernelGGL(k_skip_pw_scan, dim3(plan::scan_grid(npieces, cus)), dim3(kScanTH), 0, st, in,
                       npieces, d_state, d_sid, d_flags, d_out ? 1u : 0u, (const uint64_t *) ctl, heads,
                       recs, (const uint32_t *) big, d_res, a, k);
    if ((rc = hip_status()) != 0) return rc;
    if (!d_out) return 0;
    hipLaunchKernelGGL(k_skip_pw_decode, dim3(grid), dim3(kSkipTH), 0, st, in, tile / kChunk,
                       (uint8_t *) d_out, d_out_off, (const uint64_t *) ctl, (const Head *) heads,
                       (const uint64_t *) map, (const TileRec *) recs, a, k);
    return hip_status();
}

}  // extern "C"
