// Strict skip decode of one large piece, spread over the GPU (include/b64x.h,
// b64x_decode_strict_skip_piece_dev): what b64x_decode_strict_skip_pieces does
// for a single piece, continued from and into the same 128-byte state, with a
// wave per tile instead of a wave per piece.  A translation unit and a code
// object of its own, linked after b64x_skip_pieces.o; no kernel of the other
// units is touched.
//
// Layout ("k_skip_wide_*").  The piece is cut into tiles of T
// bytes of address span from the 16-byte floor of its address; T is
// b64x_skip_wide_plan.h's function of the length (4,096 below 64 MiB, from
// there the multiple of the 1,024-byte pass that keeps the tiles at or below
// 16,384).  Every tile is a small piece whose state is computed, not carried:
// three launches in stream order, no hand-off inside a launch, no spin, no
// global atomic.
//   k_skip_wide_count   a wave per tile, the waves striding over the tiles.
//       The walk of b64x_skip_walk.h without compaction: chunks of 16 bytes at
//       aligned addresses, passes of 1,024 bytes with the next one loaded
//       ahead, classify_chunk.  A tile's record (64 bytes of the workspace):
//         0 kept bytes           3 lowest pad offset (in the piece; none: ~0)
//         1 pad characters       4 data characters d
//         2 lowest stranger      5 its last min(3, d) data sextets, 6 bits
//           offset (likewise)      each, the last one lowest
//         6 S, 7 the carried sextets: the scan's.
//   k_skip_wide_scan    one workgroup of 256 lanes.  A lane folds a strip of
//       consecutive records (64 at the most, loaded four at a time), a wave
//       scans its lanes, the four waves meet at the kernel's barrier.  What
//       is scanned is (d, last three sextets): joining two such pairs is
//       associative, so the exclusive prefix of tile t -- started
//       from the state's own carry -- holds S_t = carry + data characters
//       before t and, in its sextets, the S_t mod 4 that tile t must put in
//       front of its own.  Both go into the record, so the decode pass reads
//       its own record and nothing of the state.  Wave 0 then walks back from
//       the piece's end to its last three kept bytes (the state's tail fills
//       in where the piece has fewer), takes the verdict, writes the record
//       and the new state, and leaves in the workspace head whether the
//       decode pass has anything to do.
//   k_skip_wide_decode  a wave per tile, the same walk with compaction: the
//       carried sextets to the front of the wave's sextet buffer, whole units
//       with 12-byte stores from d_out + 3 floor(S_t / 4), the whole groups of
//       what is left bytewise, the partial group by the last tile of a final
//       piece only.
// The state is read by the first two launches and written by the second; the
// third reads the workspace alone, so the new state may stand before it runs.
// A state that holds a report ends each launch on one uniform load (the third:
// of the head).
//
// last_kept is b64x_skip.hip's and verdict_so_far b64x_skip_pieces.hip's, kept
// here as copies: moving them into a shared header would have to leave those
// units' code objects unchanged, and nothing else wants them.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>

#include "b64x.h"
#include "b64x_skip_walk.h"
#include "b64x_skip_wide_plan.h"

namespace {

namespace plan = skip_wide_plan;

static_assert(sizeof(b64x_skip_state) == B64X_SKIP_STATE_BYTES, "the state of b64x.h");
static_assert(plan::kPassBytes == kPass && plan::kWavesPerBlock == kSkipWaves &&
                  plan::kBlocksPerCU == kSkipBlocksPerCU && plan::kTileMin % kPass == 0,
              "the plan's sizes");

constexpr uint32_t kScanTH = kSkipTH;  // the scan's one workgroup
constexpr uint32_t kScanWaves = kScanTH / lines_plan::kPassLanes;
constexpr uint32_t kScanBatch = 4;  // records a lane has in flight

struct TileRec {
    uint64_t kept, pads, first_char, first_pad, d, tail, S, cs;
};
static_assert(sizeof(TileRec) == plan::kRecordBytes, "a tile's record");

// A value that is the same in every lane, as one.
DEV uint32_t uniform(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
DEV uint64_t uniform(uint64_t v)
{
    return ((uint64_t) uniform((uint32_t) (v >> 32)) << 32) | uniform((uint32_t) v);
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

// The chunks of tile t: its first one, and how many.
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

// ------------------------------------------------------------- kernels --

// Wave g of G takes tiles g, g + G, ...: a tile's totals into its record.
__global__ __launch_bounds__(kSkipTH) void k_skip_wide_count(
    const uint8_t *__restrict__ in, uint64_t len, uint64_t tile_chunks, uint64_t ntiles,
    const b64x_skip_state *__restrict__ state, TileRec *__restrict__ recs, Alpha a, SkipSet k)
{
    __shared__ uint32_t tab[256];
    const uint32_t held = uniform((uint32_t) state->w[9]);
    build_row_table(tab, a, k);
    block_sync();
    if (held != B64X_STRICT_OK) return;  // a text that was refused: the piece is not looked at
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    const uintptr_t lo = (uintptr_t) in, hi = lo + len;
    const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
    const uint64_t chunks = chunk_count(lo, len);
    for (uint64_t t = (uint64_t) blockIdx.x * kSkipWaves + wv; t < ntiles; t += waves) {
        const TileSpan ts = tile_span(t, tile_chunks, chunks);
        const uintptr_t At = A0 + kChunk * ts.first;
        const uint64_t base0 = (uint64_t) (At - lo);  // the piece offset of the tile's byte 0 (wraps)
        Chunk next = {};
        if (lane < ts.n) next = load_chunk(At + kChunk * lane, lo, hi);
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

// One workgroup: the records' totals and prefixes, the verdict, the new state.
__global__ __launch_bounds__(kScanTH) void k_skip_wide_scan(
    const uint8_t *in, uint64_t len, uint64_t ntiles, b64x_skip_state *state, uint32_t final,
    uint32_t decode, TileRec *recs, uint64_t *head, b64x_strict_result *res, Alpha a, SkipSet k)
{
    __shared__ uint64_t wtot[kScanWaves][6];  // d, sextets, E, c, first_char, first_pad of a wave
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    uint64_t *const st = state->w;
    // a text that was refused: the same record, and nothing else
    const uint32_t kind = uniform((uint32_t) st[9]);
    if (kind != B64X_STRICT_OK) {
        if (wv != 0) return;
        b64x_strict_result r;
        r.out_len = 0;
        r.err_pos = st[10];
        r.err = kind;
        r.reserved = 0;
        if (lane == 0) {
            *res = r;
            head[0] = 1;
        }
        if (final && lane < 16) st[lane] = 0;
        return;
    }
    const uint64_t pos = uniform(st[0]);  // the text offset of the piece's byte 0
    const uint64_t E0 = uniform(st[1]), c0 = uniform(st[2]);
    const uint64_t fc = uniform(st[3]), fp = uniform(st[4]);
    const uint64_t p0 = uniform(st[5]), p1 = uniform(st[6]), p2 = uniform(st[7]);
    const uint64_t w8 = uniform(st[8]);
    const uint32_t cin = (uint32_t) (w8 >> 24) & 3u;  // sextets the pieces before left over
    Carry pre = {cin, 0};
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
        if (i < cin) pre.v = (pre.v << 6) | ((uint32_t) (w8 >> (32 + 8 * i)) & 0x3Fu);
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
    // the text so far: the state's totals and the piece's
    Slot T;
    T.E = E0 + tot.E;
    T.c = c0 + tot.c;
    T.first_char = fc ? fc - 1 : tot.first_char != kNone ? pos + tot.first_char : kNone;
    T.first_pad = fp ? fp - 1 : tot.first_pad != kNone ? pos + tot.first_pad : kNone;
    // its last three kept bytes: the piece's, then the state's own
    const uint32_t want = tot.E < 3 ? (uint32_t) tot.E : 3u;
    Last3 f = {};
    if (want) f = last_kept((uintptr_t) in, (uintptr_t) in + len, lane, want, k);
    const uint32_t ob0 = (uint32_t) w8 & 0xFFu, ob1 = (uint32_t) (w8 >> 8) & 0xFFu,
                   ob2 = (uint32_t) (w8 >> 16) & 0xFFu;
    const uint32_t f0 = f.byte[0], f1 = f.byte[1], f2 = f.byte[2];
    const uint64_t g0 = pos + f.off[0], g1 = pos + f.off[1], g2 = pos + f.off[2];
    Last3 last;
    last.byte[0] = want >= 1 ? f0 : ob0;
    last.off[0] = want >= 1 ? g0 : p0;
    last.byte[1] = want >= 2 ? f1 : want == 1 ? ob0 : ob1;
    last.off[1] = want >= 2 ? g1 : want == 1 ? p0 : p1;
    last.byte[2] = want == 3 ? f2 : want == 2 ? ob0 : want == 1 ? ob1 : ob2;
    last.off[2] = want == 3 ? g2 : want == 2 ? p0 : want == 1 ? p1 : p2;
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
        head[0] = r.err != B64X_STRICT_OK;  // then the decode pass writes nothing
    }
}

// Wave g of G takes tiles g, g + G, ...: a tile's groups to their place.
__global__ __launch_bounds__(kSkipTH) void k_skip_wide_decode(
    const uint8_t *__restrict__ in, uint64_t len, uint64_t tile_chunks, uint64_t ntiles,
    uint8_t *__restrict__ out, uint32_t final, const TileRec *__restrict__ recs,
    const uint64_t *__restrict__ head, Alpha a, SkipSet k)
{
    __shared__ uint32_t tab[256];
    // a wave's sextets, and behind them a byte per lane for what is no sextet
    __shared__ __attribute__((aligned(16))) uint8_t sextets[kSkipWaves][kSextets + kLanes];
    const uint32_t idle = uniform((uint32_t) head[0]);
    build_row_table(tab, a, k);
    block_sync();
    if (idle) return;  // a report, old or new
    const uint32_t lane = threadIdx.x % kLanes;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
    uint8_t *const sx = sextets[wv];
    const uint64_t waves = (uint64_t) gridDim.x * kSkipWaves;
    const uintptr_t lo = (uintptr_t) in, hi = lo + len;
    const uintptr_t A0 = lo & ~(uintptr_t) (kChunk - 1);
    const uint64_t chunks = chunk_count(lo, len);
    for (uint64_t t = (uint64_t) blockIdx.x * kSkipWaves + wv; t < ntiles; t += waves) {
        const TileSpan ts = tile_span(t, tile_chunks, chunks);
        const uintptr_t At = A0 + kChunk * ts.first;
        Chunk next = {};
        if (lane < ts.n) next = load_chunk(At + kChunk * lane, lo, hi);
        const uint64_t S = uniform(recs[t].S);
        const uint32_t cs = uniform((uint32_t) recs[t].cs);
        uint8_t *rout = out + 3 * (S >> 2);
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
        const bool last = final && t == ntiles - 1;
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

uint64_t b64x_strict_skip_piece_workspace_size(uint64_t len, bool validate_only)
{
    (void) validate_only;  // the count pass and the scan want the records either way
    return plan::workspace_bytes(len);
}

int b64x_decode_strict_skip_piece_dev(const void *d_in, uint64_t len, void *d_out,
                                      b64x_skip_state *d_state, unsigned flags,
                                      b64x_strict_result *d_res, const b64x_alphabet *abc,
                                      const b64x_skip *skip, void *d_workspace, void *stream)
{
    if (!d_in || !d_state || !d_res || !d_workspace) return -EINVAL;
    if ((((uintptr_t) d_res) | ((uintptr_t) d_state) | ((uintptr_t) d_workspace)) & 7) return -EINVAL;
    if (flags & ~B64X_PIECE_FINAL) return -EINVAL;
    const Alpha a = lines_plan::make_alpha(abc);
    SkipSet k;
    if (!make_skip(skip, a, &k)) return -EINVAL;
    if (!lines_plan::alpha_ok(a)) return -EINVAL;
    int rc = b64x_device_check();
    if (rc) return rc;
    uint32_t cus = 0;
    if ((rc = device_cus(&cus)) != 0) return rc;
    const uint8_t *in = (const uint8_t *) d_in;
    const uint64_t tile_chunks = plan::tile_bytes(len) / kChunk;
    const uint64_t ntiles = plan::tile_count(len, (uint32_t) ((uintptr_t) d_in & (kChunk - 1)));
    const uint32_t grid = plan::grid_blocks(ntiles, cus);
    uint64_t *head = (uint64_t *) d_workspace;
    TileRec *recs = (TileRec *) ((uint8_t *) d_workspace + plan::kHeadBytes);
    const uint32_t final = flags & B64X_PIECE_FINAL;
    const hipStream_t st = (hipStream_t) stream;
    hipLaunchKernelGGL(k_skip_wide_count, dim3(grid), dim3(kSkipTH), 0, st, in, len, tile_chunks,
                       ntiles, (const b64x_skip_state *) d_state, recs, a, k);
    if ((rc = hip_status()) != 0) return rc;
    hipLaunchKernelGGL(k_skip_wide_scan, dim3(1), dim3(kScanTH), 0, st, in, len, ntiles, d_state,
                       final, d_out ? 1u : 0u, recs, head, d_res, a, k);
    if ((rc = hip_status()) != 0) return rc;
    if (!d_out) return 0;
    hipLaunchKernelGGL(k_skip_wide_decode, dim3(grid), dim3(kSkipTH), 0, st, in, len, tile_chunks,
                       ntiles, (uint8_t *) d_out, final, (const TileRec *) recs,
                       (const uint64_t *) head, a, k);
    return hip_status();
}

}  // extern "C"
