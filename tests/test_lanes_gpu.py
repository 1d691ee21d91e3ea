"""The batch lanes called directly: b64x_lane_encode_async (k_gather_host,
copy_from_host, k_stamp) and b64x_lane_decode_async (k_spell_head, the
single-buffer pipeline on the lane's private workspace), on lanes from
b64x_lane_open and arenas from b64x_host_alloc.

The host stages reach the GPU only through these two calls, and there the
hub's timers compose the batches.  Here every batch is built by hand: lent
segments at every alignment and at the gather's 64 KiB tile edges, a segment
table long enough to grow the lane's device copy, batches that make every lane
buffer grow, decode chains whose predecessor is chained itself, is a job of
128 KiB or more, or sits in an earlier batch still queued on the lane, and new
content at an address and length the lane's workspace holds a model for.

Every comparison is bit for bit against oracle.pyoracle.  Every output arena
is pinned, pre-filled with a sentinel, has 0-7 sentinel bytes after each job's
capacity and a 64-byte canary at both ends, and is compared whole; every input
arena, segment source and table is checked unchanged after the call.  The
CPU-only tests assert that the case tables hold what the GPU tests are for."""
import ctypes
import functools
import threading
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from async_amd import _lib
from oracle import pyoracle as orc
from tests.test_gpu_parity import _junk, _wrap
from tests.test_ragged_batch import (BIG, CHAINED, ENC_ABCS, ENC_IDS, HOLD, RECORD, SENT, _arena,
                                     _first_bad, _layout, _Pinned, _text_of_kind, alphabet,
                                     decoded_cap)

SEED = 0x1A9E
EINVAL = 22
CANARY = 64
T = 64 << 10  # kGatherTile: one block of k_gather_host covers this many batch bytes
SEG = np.dtype([("off", "<u8"), ("len", "<u8"), ("src", "<u8")])  # b64x_seg
DONE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)  # b64x_done_fn
# the lane's first-use sizes (b64x_sessions.cpp: kLaneInFloor, kLaneOffsFloor, kLaneSegFloor)
LANE_IN_FLOOR = (16 << 20) + (1 << 20)
LANE_OFFS_FLOOR = 3 * ((1 << 16) + 1) * 8
LANE_SEG_FLOOR_COUNT = 1 << 14
BIG_CHARS = 140001  # a job past the 128 KiB limit of the batch kernels

assert SEG.itemsize == 24 and BIG_CHARS >= BIG


@pytest.fixture
def lane():
    lib = _lib.load()
    torch.cuda.set_device(0)
    ln = lib.b64x_lane_open()
    assert ln, "b64x_lane_open failed"
    yield lib, ln
    lib.b64x_lane_close(ln)


# ---- encode: plans (plain numpy) -------------------------------------------


def _enc_len(lens, pad):
    """b64x_encoded_len, vectorised."""
    lens = np.asarray(lens, np.int64)
    return (lens + 2) // 3 * 4 if pad else (4 * lens + 2) // 3


@dataclass
class EncPlan:
    abc: tuple
    D: np.ndarray        # the batch's logical input
    lens: np.ndarray     # job lengths, tiling D
    in_off: np.ndarray
    out_off: np.ndarray  # capacity plus a gap of 0-7 after each job
    elen: np.ndarray
    wants: list          # orc.encode of every job
    expect: np.ndarray   # canary, the arena (_arena), canary
    segs: tuple          # (off, len, source address mod 16), sorted by off


def _enc_plan(D, lens, segs, abc, seed) -> EncPlan:
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    assert int(lens.sum()) == D.size
    elen = _enc_len(lens, abc[2])
    in_off, out_off = _layout(lens, elen, rng)
    wants = [orc.encode(D[in_off[i]:in_off[i + 1]], *abc, as_array=True) for i in range(lens.size)]
    _, _, arena, mask = _arena(out_off, elen, wants)
    assert mask.all()  # every byte is an encoded character or a gap
    canary = np.full(CANARY, SENT, np.uint8)
    return EncPlan(abc, D, lens, in_off, out_off, elen, wants,
                   np.concatenate([canary, arena, canary]), tuple(segs))


def _lay_jobs(total, rng, lo=1, hi=5000):
    """Job lengths of lo..hi bytes laid over [0, total), whatever the segments are."""
    lens = []
    while total:
        lens.append(min(total, int(rng.integers(lo, hi + 1))))
        total -= lens[-1]
    return np.array(lens, np.int64)


def _random(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


PLAIN_LENS = tuple(range(0, 51)) + (4095, 4096, 4097, 65535, 65536, 65537)


@functools.lru_cache(maxsize=None)
def plain_lens() -> np.ndarray:
    """The job lengths of the batch without segments, in a fixed random order."""
    rng = np.random.default_rng(SEED + 1)
    lens = np.concatenate([np.array(PLAIN_LENS), rng.integers(0, 3001, 200)])
    return rng.permutation(lens)


SWEEP_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
SWEEP_GAPS = (0, 1, 5, 16, 21)


@functools.lru_cache(maxsize=None)
def sweep_segments():
    """(segments, total): segments laid one after another over a batch, the
    arena gap in front of each cycling through SWEEP_GAPS, until every (source
    address mod 16, batch offset mod 16) pair has had every length of
    SWEEP_LENS.  The gap and the lengths before it fix a segment's offset;
    its length is one that this offset residue still lacks (else the next in
    turn, to move on) and its source residue the next one lacking."""
    need = {(b, n): list(range(16)) for b in range(16) for n in SWEEP_LENS}
    left = 16 * len(need)
    segs, pos, i = [], 0, 0
    while left:
        assert i < 40000, "the sweep does not close"
        pos += SWEEP_GAPS[i % len(SWEEP_GAPS)]
        b = pos % 16
        lacking = [n for n in SWEEP_LENS if need[(b, n)]]
        if lacking:
            n = max(lacking, key=lambda m: (len(need[(b, m)]), m))
            a = need[(b, n)].pop(0)
            left -= 1
        else:
            n, a = SWEEP_LENS[i % len(SWEEP_LENS)], i % 16
        segs.append((pos, n, a))
        pos += n
        i += 1
    return tuple(segs), pos + 21


@functools.lru_cache(maxsize=None)
def sweep_plan() -> EncPlan:
    segs, total = sweep_segments()
    return _enc_plan(_random(SEED + 2, total), _lay_jobs(total, np.random.default_rng(SEED + 3)),
                     segs, ENC_ABCS[0], SEED + 4)


TILE_TOTALS = (7, T, T + 1, 2 * T)


@functools.lru_cache(maxsize=None)
def tile_cases():
    """(name, batch total, ((off, len), ...)): one batch each."""
    cases = []
    for tot in TILE_TOTALS:
        cases.append((f"whole-{tot}", tot, ((0, tot),)))
        cases.append((f"both-ends-{tot}", tot, ((0, 3), (tot - 2, 2))))
    tot = 2 * T + 300
    for d in (-1, 0, 1):
        cases.append((f"start{d:+d}", tot, tuple((k * T + d, 100) for k in (1, 2))))
        cases.append((f"end{d:+d}", tot, tuple((k * T + d - 100, 100) for k in (1, 2))))
    cases.append(("meet", tot, tuple(s for k in (1, 2) for s in ((k * T - 50, 50), (k * T, 50)))))
    cases.append(("gap-ends", tot, tuple(s for k in (1, 2) for s in ((k * T - 100, 50), (k * T, 50)))))
    cases.append(("long", 4 * T + 11, ((T - 3, 3 * T + 7),)))
    return tuple(cases)


def _tile_relations(total, segs) -> set:
    """What a batch's segments do at the tile edges kT, k = 1, 2."""
    rel = set()
    for i, (off, n) in enumerate(segs):
        end = off + n
        for k in (1, 2):
            if abs(off - k * T) <= 1:
                rel.add(("start", k, off - k * T))
            if abs(end - k * T) <= 1:
                rel.add(("end", k, end - k * T))
            prev_end = segs[i - 1][0] + segs[i - 1][1] if i else 0
            if off == k * T and i and prev_end == off:
                rel.add(("meet", k))
            if off == k * T and prev_end < off:
                rel.add(("gap-ends", k))
        if off == 0:
            rel.add("starts-at-0")
        if end == total:
            rel.add("ends-at-in_bytes")
        if (off, n) == (0, total):
            rel.add("whole")
        if (off, n) == (T - 3, 3 * T + 7):
            rel.add("long")
    return rel


@functools.lru_cache(maxsize=None)
def tile_plans():
    plans = []
    for i, (name, total, segs) in enumerate(tile_cases()):
        rng = np.random.default_rng(SEED + 100 + i)
        with_mod = tuple((off, n, (5 * j + 3 * i + 1) % 16) for j, (off, n) in enumerate(segs))
        plans.append((name, _enc_plan(_random(SEED + 200 + i, total), _lay_jobs(total, rng),
                                      with_mod, ENC_ABCS[i % len(ENC_ABCS)], SEED + 300 + i)))
    return plans


LONG_NSEG = (1 << 14) + 3


@functools.lru_cache(maxsize=None)
def long_segments():
    """2^14 + 3 segments of 1-8 bytes with arena gaps of 0-3 in front of each."""
    rng = np.random.default_rng(SEED + 5)
    n = rng.integers(1, 9, LONG_NSEG)
    gap = rng.integers(0, 4, LONG_NSEG)
    off = np.cumsum(gap + n) - n
    mod = rng.integers(0, 16, LONG_NSEG)
    return tuple(zip(off.tolist(), n.tolist(), mod.tolist())), int(off[-1] + n[-1]) + 3


@functools.lru_cache(maxsize=None)
def long_plans():
    segs, total = long_segments()
    rng = np.random.default_rng(SEED + 6)
    first = _enc_plan(_random(SEED + 7, total), _lay_jobs(total, rng), segs, ENC_ABCS[0], SEED + 8)
    # five segments over a batch of the same size: every table entry past the
    # fifth is the long table's, left in the lane's device copy
    five = tuple((int(o), 700, m) for o, m in zip(np.linspace(10, total - 800, 5), (3, 0, 9, 15, 6)))
    second = _enc_plan(_random(SEED + 9, total), _lay_jobs(total, rng), five, ENC_ABCS[0], SEED + 10)
    return first, second


GROW_BYTES = (18 << 20) + 5
GROW_JOBS = 100003


@functools.lru_cache(maxsize=None)
def growth_plans():
    """The sweep batch, a batch of three jobs past the input floor, a batch of
    100,003 jobs past the offsets floor; the sweep's segments in all three."""
    segs, total = sweep_segments()
    rng = np.random.default_rng(SEED + 11)
    wide = _enc_plan(_random(SEED + 12, GROW_BYTES), [6 << 20, (6 << 20) + 5, 6 << 20], segs,
                     ENC_ABCS[0], SEED + 13)
    lens = rng.integers(0, 25, GROW_JOBS)
    many = _enc_plan(_random(SEED + 14, int(lens.sum())), lens, segs, ENC_ABCS[1], SEED + 15)
    assert lens.sum() > total
    return sweep_plan(), wide, many


# ---- encode: the case tables, no GPU ----------------------------------------


def test_plain_encode_lengths():
    lens = plain_lens().tolist()
    assert set(PLAIN_LENS) <= set(lens) and len(lens) == len(PLAIN_LENS) + 200
    assert set(range(51)) | {4095, 4096, 4097, 65535, 65536, 65537} == set(PLAIN_LENS)
    assert max(lens) == 65537 and sorted(lens) != lens


def test_sweep_table_covers_every_alignment_pair_with_every_length():
    segs, total = sweep_segments()
    seen = {(a, off % 16, n) for off, n, a in segs}
    assert seen >= {(a, b, n) for a in range(16) for b in range(16) for n in SWEEP_LENS}
    assert len({(a, b) for a, b, _ in seen}) == 256
    assert {n for _, n, _ in segs} == set(SWEEP_LENS) == {0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49}
    ends = [0] + [off + n for off, n, _ in segs]
    gaps = [segs[i][0] - ends[i] for i in range(len(segs))]
    assert gaps == [SWEEP_GAPS[i % 5] for i in range(len(segs))] and SWEEP_GAPS == (0, 1, 5, 16, 21)
    assert ends[-1] < total and total > T  # arena bytes after the last; more than one tile
    p = sweep_plan()
    assert p.lens.min() >= 1 and p.lens.max() <= 5000 and p.D.size == total


def test_tile_table_covers_every_edge_relation():
    rel, totals = set(), set()
    for name, total, segs in tile_cases():
        assert all(0 <= o and o + n <= total for o, n in segs), name
        assert all(segs[i][0] >= segs[i - 1][0] + segs[i - 1][1] for i in range(1, len(segs))), name
        rel |= _tile_relations(total, segs)
        totals.add(total)
    want = {(w, k, d) for w in ("start", "end") for k in (1, 2) for d in (-1, 0, 1)}
    want |= {(w, k) for w in ("meet", "gap-ends") for k in (1, 2)}
    want |= {"starts-at-0", "ends-at-in_bytes", "whole", "long"}
    assert rel >= want, want - rel
    assert totals >= {7, T, T + 1, 2 * T} and T == 65536
    for tot in TILE_TOTALS:  # each of the four totals: one segment over it all, and both ends
        mine = [segs for _, total, segs in tile_cases() if total == tot]
        assert ((0, tot),) in mine
        assert any(len(s) == 2 and s[0][0] == 0 and sum(s[1]) == tot for s in mine)
    for _, p in tile_plans():
        assert p.lens.min() >= 1 and p.lens.max() <= 5000


def test_long_and_growth_tables_pass_the_lane_floors():
    segs, total = long_segments()
    assert len(segs) == LONG_NSEG == 2 ** 14 + 3 > LANE_SEG_FLOOR_COUNT
    n = np.array([s[1] for s in segs])
    off = np.array([s[0] for s in segs])
    gap = off - np.concatenate([[0], (off + n)[:-1]])
    assert n.min() == 1 and n.max() == 8 and gap.min() == 0 and gap.max() == 3
    assert all(((off >= k * T) & (off < (k + 1) * T)).sum() >= 300 for k in range(-(-total // T)))
    first, second = long_plans()
    assert len(second.segs) == 5 and second.D.size == first.D.size
    small, wide, many = growth_plans()
    assert wide.D.size == 18 * 2 ** 20 + 5 > LANE_IN_FLOOR - 64 and wide.lens.size == 3
    assert many.lens.size == 100003 and many.lens.min() == 0 and many.lens.max() == 24
    assert 2 * (many.lens.size + 1) * 8 > LANE_OFFS_FLOOR  # the two offset tables of an encode batch
    assert small.D.size + 64 <= LANE_IN_FLOOR and wide.segs == many.segs == sweep_segments()[0]


# ---- encode: on the GPU ------------------------------------------------------


class _EncBatch:
    """An EncPlan in pinned arenas.  The arena h_in holds D, except that every
    byte under a segment is D ^ 0xFF; each segment's bytes lie in a separate
    pinned buffer at the chosen address mod 16, between 16 bytes of
    D's neighbours ^ 0xFF: a read from the wrong place gives wrong characters."""

    def __init__(self, lib, plan: EncPlan):
        self.lib, self.plan, self.pin = lib, plan, _Pinned(lib)
        try:
            self._fill()
        except BaseException:
            self.pin.close()
            raise

    def _fill(self):
        p, pin = self.plan, self.pin
        total, self.n = p.D.size, p.lens.size
        self.h_in, self.p_in = pin.array(total + 64, np.uint8)
        self.h_in[:total] = p.D
        self.h_in[total:] = 0xEE
        self.h_out, p_out = pin.array(p.expect.size, np.uint8)
        self.h_out[:] = SENT
        self.p_out = p_out + CANARY
        self.h_in_off, self.p_in_off = pin.array(self.n + 1, np.uint64)
        self.h_out_off, self.p_out_off = pin.array(self.n + 1, np.uint64)
        self.h_in_off[:] = p.in_off
        self.h_out_off[:] = p.out_off
        at, size = [], 64
        for off, n, mod in p.segs:  # 16 bytes of poison on both sides of every source
            at.append((size + 31) // 16 * 16 + mod)
            size = at[-1] + n + 16
        self.h_src, p_src = pin.array(size + 64, np.uint8)
        assert p_src % 16 == 0 and self.p_in % 16 == 0
        self.h_src[:] = 0xA5
        self.h_seg, self.p_seg = pin.array(len(p.segs), SEG)
        for i, ((off, n, mod), st) in enumerate(zip(p.segs, at)):
            lo, hi = max(off - 16, 0), min(off + n + 16, total)
            self.h_src[st - (off - lo):st + (hi - off)] = p.D[lo:hi]
            self.h_src[st - (off - lo):st] ^= 0xFF
            self.h_src[st + n:st + (hi - off)] ^= 0xFF
            self.h_in[off:off + n] ^= 0xFF
            self.h_seg[i] = (off, n, p_src + st)
            assert (p_src + st) % 16 == mod
        self.abc_c = _lib.alphabet(*p.abc)
        self.inputs = (self.h_in, self.h_src, self.h_in_off, self.h_out_off, self.h_seg)
        self.before = [a.copy() for a in self.inputs]

    def queue(self, lane, done=None, seg=None):
        p_seg, nseg = seg if seg is not None else (self.p_seg, len(self.plan.segs))
        return self.lib.b64x_lane_encode_async(lane, self.p_in, self.n, self.p_in_off, self.p_out,
                                               self.p_out_off, p_seg, nseg,
                                               ctypes.byref(self.abc_c), done, None)

    def inputs_unchanged(self):
        names = ("h_in", "sources", "in_off", "out_off", "h_seg")
        for a, b, name in zip(self.inputs, self.before, names):
            assert np.array_equal(a, b), f"{name} changed"

    def untouched(self):
        assert (self.h_out == SENT).all(), "a refused batch wrote to its output"
        self.inputs_unchanged()

    def check(self, what=""):
        p, got = self.plan, self.h_out.copy()
        self.inputs_unchanged()
        if np.array_equal(got, p.expect):
            return
        if (got[:CANARY] != SENT).any() or (got[-CANARY:] != SENT).any():
            pytest.fail(f"{what}: a canary was written")
        bad = _first_bad(got[CANARY:-CANARY], p.elen, p.out_off, p.elen, lambda i: p.wants[i],
                         lambda i: f"{p.lens[i]} bytes at {p.in_off[i]}, out_off {p.out_off[i]}")
        pytest.fail(f"{what}: {bad}")

    def close(self):
        self.pin.close()


def _run_encode(lib, ln, plan, what="", done=None):
    b = _EncBatch(lib, plan)
    try:
        rc = b.queue(ln, done)
        waited = lib.b64x_lane_wait(ln)
        assert rc == 0 and waited == 0, (what, rc, waited)
        assert lib.b64x_lane_encode_check(ln) == 0, what
        b.check(what)
    finally:
        lib.b64x_lane_wait(ln)
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("abc", ENC_ABCS, ids=ENC_IDS)
def test_lane_encode_without_segments(lane, abc):
    """Jobs of 0-50, 4095-4097, 65535-65537 and 200 random lengths in one
    batch (the H2D copy of the arena, then the ragged encode and the stamp)."""
    lib, ln = lane
    lens = plain_lens()
    _run_encode(lib, ln, _enc_plan(_random(SEED + 20, int(lens.sum())), lens, (), abc, SEED + 21))


@pytest.mark.gpu
def test_lane_encode_empty_batches(lane):
    """No job at all (the stamp only), jobs that are all empty, and those with
    one zero-length segment; a real batch between and after them."""
    lib, ln = lane
    empty = np.zeros(0, np.uint8)
    real = _enc_plan(_random(SEED + 22, 1000), [0, 999, 1], ((5, 40, 7),), ENC_ABCS[0], SEED + 23)
    _run_encode(lib, ln, _enc_plan(empty, [], (), ENC_ABCS[0], SEED + 24), "no jobs")
    _run_encode(lib, ln, real, "after no jobs")
    _run_encode(lib, ln, _enc_plan(empty, [0] * 9, (), ENC_ABCS[0], SEED + 25), "empty jobs")
    _run_encode(lib, ln, _enc_plan(empty, [0] * 9, ((0, 0, 5),), ENC_ABCS[1], SEED + 26),
                "empty jobs, one empty segment")
    _run_encode(lib, ln, real, "after empty jobs")


@pytest.mark.gpu
def test_lane_encode_callback_runs_before_wait_returns(lane):
    lib, ln = lane
    ev = threading.Event()
    cb = DONE_FN(lambda arg: ev.set())
    b = _EncBatch(lib, sweep_plan())
    try:
        assert b.queue(ln, ctypes.cast(cb, ctypes.c_void_p)) == 0
        assert lib.b64x_lane_wait(ln) == 0
        was_set = ev.is_set()
        assert ev.wait(10), "the done callback did not run"
        assert was_set, "b64x_lane_wait returned before the done callback had run"
        assert lib.b64x_lane_encode_check(ln) == 0
        b.check("callback batch")
    finally:
        lib.b64x_lane_wait(ln)
        b.close()


@pytest.mark.gpu
def test_lane_gather_every_alignment_pair(lane):
    """copy_from_host's aligned 16-byte loads reach up to 15 bytes outside a
    piece on both sides: segments of 0-49 bytes at every (source address,
    batch offset) pair mod 16, arena pieces of 0-21 bytes between them."""
    lib, ln = lane
    _run_encode(lib, ln, sweep_plan(), "alignment sweep")


@pytest.mark.gpu
def test_lane_gather_tile_edges(lane):
    """Segments that start, end and meet at, one before and one after the
    64 KiB edges between k_gather_host's blocks (the search for a block's
    first segment, the clipping of a piece to its block)."""
    lib, ln = lane
    for name, plan in tile_plans():
        _run_encode(lib, ln, plan, name)


@pytest.mark.gpu
def test_lane_gather_long_segment_table(lane):
    """More segments than the lane's table holds at first (it grows), hundreds
    per tile for the binary search; then five segments on the same lane, the
    long table's entries still behind them in the device copy."""
    lib, ln = lane
    first, second = long_plans()
    _run_encode(lib, ln, first, "2^14 + 3 segments")
    _run_encode(lib, ln, second, "five segments after")


@pytest.mark.gpu
def test_lane_buffers_grow_past_their_floors(lane):
    lib, ln = lane
    small, wide, many = growth_plans()
    _run_encode(lib, ln, small, "small")
    _run_encode(lib, ln, wide, "18 MiB + 5 in three jobs")
    _run_encode(lib, ln, many, "100,003 jobs")
    _run_encode(lib, ln, small, "small again")


@pytest.mark.gpu
def test_lane_encode_refuses_bad_segments(lane):
    """-EINVAL for segments unsorted, overlapping, past in_bytes (one of them
    with off + len wrapping round 64 bits), nseg without a table, no lane:
    nothing is written, the last good batch still checks, the next is exact."""
    lib, ln = lane
    good = sweep_plan()
    total = good.D.size
    _run_encode(lib, ln, good, "before")
    b = _EncBatch(lib, good)
    pin = _Pinned(lib)
    try:
        src = int(b.h_seg[0]["src"])
        tables = {
            "unsorted": [(100, 10, src), (50, 10, src)],
            "overlapping": [(100, 10, src), (109, 10, src)],
            "past in_bytes": [(total - 5, 6, src)],
            "off + len wraps": [(2 ** 64 - 1, 2, src)],
        }
        for name, rows in tables.items():
            tab, p_tab = pin.array(len(rows), SEG)
            tab[:] = np.array(rows, SEG)
            assert b.queue(ln, seg=(p_tab, len(rows))) == -EINVAL, name
            assert lib.b64x_lane_encode_check(ln) == 0, name
        assert b.queue(ln, seg=(None, 1)) == -EINVAL
        assert b.queue(None) == -EINVAL
        assert lib.b64x_lane_encode_check(ln) == 0 and lib.b64x_lane_wait(ln) == 0
        b.untouched()
        assert b.queue(ln) == 0 and lib.b64x_lane_wait(ln) == 0
        assert lib.b64x_lane_encode_check(ln) == 0
        b.check("after the refused batches")
    finally:
        lib.b64x_lane_wait(ln)
        pin.close()
        b.close()


# ---- decode: plans ------------------------------------------------------------

CHAIN_ABCS = [(-1, -1), ("-", "_")]
CHAIN_IDS = ["default", "url"]
NBATCH = 3
FILLERS = 120  # per batch


@dataclass
class Job:
    text: np.ndarray   # the job's characters, a chained job's 4-byte head included
    flags: int
    want: np.ndarray   # its bytes
    valid: int
    tail: np.ndarray   # the last valid % 4 sextets
    check_tail: bool
    key: float = 0.0   # place in its batch
    stream: int = -1
    k: int = 0         # block number in its stream
    batch: int = 0


@dataclass
class DecBatch:
    jobs: list
    data: np.ndarray
    lens: np.ndarray
    caps: np.ndarray
    in_off: np.ndarray
    out_off: np.ndarray
    flags: np.ndarray
    prev: list           # per job: (batch, job) of its predecessor, or None
    valid: np.ndarray
    tails: np.ndarray
    check_tail: np.ndarray
    out_len: np.ndarray
    expect: np.ndarray   # canary, arena, canary
    mask: np.ndarray


def _sextets(A, t):
    return A.tab[t[A.is_alpha[t]]].astype(np.uint8)


def _plain_job(A, text, hold, key=0.0) -> Job:
    """An unchained job: the whole of a stream of its own."""
    s = _sextets(A, text)
    full = orc.decode(text, *A.abc, as_array=True)
    n = s.size // 4 * 3 if hold else s.size * 6 // 8
    return Job(text, HOLD if hold else 0, full[:n], s.size, s[s.size - s.size % 4:], bool(hold), key)


def _stream_jobs(A, rng, sid, blocks, batches) -> list:
    """The jobs of one stream cut into `blocks` (texts without heads): block
    k > 0 is chained behind a 4-byte head outside the alphabet, every block
    but the last is HOLD.  With C_k the alphabet characters of blocks 0..k:
    bytes, the oracle's decode of the whole text from C_(k-1) // 4 * 3 up to
    C_k // 4 * 3 (the last block: 6 C_k // 8); valid, the block's own
    characters plus C_(k-1) % 4; tail, the stream's last C_k % 4 sextets."""
    text = np.concatenate(blocks)
    full = orc.decode(text, *A.abc, as_array=True)
    sext = _sextets(A, text)
    jobs, C = [], 0
    for k, own in enumerate(blocks):
        last = k == len(blocks) - 1
        c_own = int(A.is_alpha[own].sum())
        lo, C = C // 4 * 3, C + c_own
        hi = C * 6 // 8 if last else C // 4 * 3
        head = A.junk_run(rng, 4) if k else np.zeros(0, np.uint8)
        jobs.append(Job(np.concatenate([head, own]), (0 if last else HOLD) | (CHAINED if k else 0),
                        full[lo:hi], c_own + (C - c_own) % 4, sext[C - C % 4:C], True,
                        stream=sid, k=k, batch=batches[k]))
    assert hi == full.size
    return jobs


def _tuned(A, rng, bodies, cmods):
    """`bodies`, each followed by the 0-3 clean characters that make the
    stream's cumulative alphabet count after block k equal cmods[k] mod 4
    (None: the body as it is)."""
    out, C = [], 0
    for body, m in zip(bodies, cmods):
        own = int(A.is_alpha[body].sum())
        if m is not None:
            extra = (m - C - own) % 4
            body = np.concatenate([body, A.clean(rng, extra)])
            own += extra
        C += own
        out.append(body)
    return out


def _big_crlf(A, rng, n, C_before, cmod):
    """n characters of CRLF-76 text whose last 0-3 alphabet characters are
    '=' instead, so that C_before plus its alphabet count is cmod mod 4."""
    t = A.clean(rng, n)
    col = np.arange(n) % 78
    t[col == 76] = 13
    t[col == 77] = 10
    at = np.flatnonzero(A.is_alpha[t])
    drop = (C_before + at.size - cmod) % 4
    t[at[at.size - drop:]] = ord("=")
    assert (C_before + A.is_alpha[t].sum()) % 4 == cmod and not A.is_alpha[ord("=")]
    return t


def _chain_streams(A, rng):
    """[(blocks, batches)]: see test_chain_plan_covers_the_predecessor_cases."""
    def body(kind=None):
        kind = kind or "bcdghia"[int(rng.integers(0, 7))]
        return _text_of_kind(A, rng, kind, int(rng.integers(80, 2500)), False)

    c62, c63 = (np.array([ord(d) if c == -1 else ord(c)], np.uint8) for c, d in zip(A.abc, "+/"))
    assert A.tab[c62[0]] == 62 and A.tab[c63[0]] == 63
    cat = np.concatenate
    streams = []
    for r in range(4):
        # predecessors in the same batch: 3-6 blocks, all of them in one batch
        n = 3 + r
        streams.append((_tuned(A, rng, [body() for _ in range(n)], [(r + 3 * k) % 4 for k in range(n)]),
                        [r % NBATCH] * n))
        # predecessors in an earlier batch; the second predecessor is chained
        bat = [[0, 1, 2], [0, 1, 1, 2], [0, 0, 1, 2, 2], [0, 1, 2]][r]
        streams.append((_tuned(A, rng, [body("cdgh"[(r + k) % 4]) for k in range(len(bat))],
                               [(r + k) % 4 for k in range(len(bat))]), bat))
        # a predecessor of 140,001 characters, in the same batch and in an earlier one
        small = _tuned(A, rng, [body(), body()], [None, None])
        streams.append(([_big_crlf(A, rng, BIG_CHARS, 0, r)] + small, [[0, 0, 1], [0, 1, 2]][r % 2]))
        # a chained job of 140,001 characters (its head included), then its successor
        first = _tuned(A, rng, [body()], [r])[0]
        streams.append(([first, _big_crlf(A, rng, BIG_CHARS - 4, r, (r + 1) % 4), body()],
                        [[0, 1, 1], [1, 1, 2]][r % 2]))
    # cuts right after the characters of sextets 62 and 63
    streams.append(([cat([A.clean(rng, 8), c62]), c63, c62, cat([c63, A.clean(rng, 5)])], [0, 0, 1, 2]))
    streams.append(([cat([A.clean(rng, 4), c63, c62, c63]), cat([A.clean(rng, 1), c62, c62]),
                     cat([c63, A.junk_run(rng, 3), c63, c63]), A.clean(rng, 7)], [0, 1, 1, 2]))
    streams.append(([cat([A.clean(rng, 40), c63, c63]), cat([c62, A.junk_run(rng, 2)]), body()],
                    [1, 2, 2]))
    # blocks without a character of their own: nothing after the head, junk only
    streams.append((_tuned(A, rng, [body(), np.zeros(0, np.uint8), A.junk_run(rng, 9), A.clean(rng, 5),
                                    A.junk_run(rng, 70), body()], [3, None, None, 0, None, None]),
                    [0, 0, 1, 1, 2, 2]))
    return streams


@functools.lru_cache(maxsize=None)
def chain_plan(abc):
    """Three decode batches: the blocks of _chain_streams among FILLERS
    unchained jobs each, a stream's blocks in order within a batch."""
    A = alphabet(*abc)
    rng = np.random.default_rng(SEED + 30)
    jobs = []
    for sid, (blocks, batches) in enumerate(_chain_streams(A, rng)):
        mine = _stream_jobs(A, rng, sid, blocks, batches)
        for b in range(NBATCH):
            there = [j for j in mine if j.batch == b]
            for j, key in zip(there, sorted(rng.random(len(there)))):
                j.key = float(key)
        jobs += mine
    for b in range(NBATCH):
        for _ in range(FILLERS):
            t = _text_of_kind(A, rng, "abcdfghij"[int(rng.integers(0, 9))], int(rng.integers(0, 3001)),
                              False)
            j = _plain_job(A, t, rng.random() < 1 / 3, float(rng.random()))
            j.batch = b
            jobs.append(j)
    per_batch = [sorted((j for j in jobs if j.batch == b), key=lambda j: j.key) for b in range(NBATCH)]
    where = {(j.stream, j.k): (b, i) for b, js in enumerate(per_batch) for i, j in enumerate(js)
             if j.stream >= 0}
    return [_dec_batch(js, [where[(j.stream, j.k - 1)] if j.flags & CHAINED else None for j in js],
                       SEED + 31 + b) for b, js in enumerate(per_batch)]


def _dec_batch(jobs, prev, seed) -> DecBatch:
    rng = np.random.default_rng(seed)
    n = len(jobs)
    lens = np.fromiter((j.text.size for j in jobs), np.int64, n)
    caps = decoded_cap(lens)
    in_off, out_off = _layout(lens, caps, rng)
    flags = np.array([j.flags for j in jobs], np.uint8)
    valid = np.array([j.valid for j in jobs], np.int64)
    tails = np.zeros((n, 4), np.uint8)
    for i, j in enumerate(jobs):
        assert j.tail.size == j.valid % 4
        tails[i, :j.tail.size] = j.tail
    out_len = np.where(flags & HOLD, valid // 4 * 3, valid * 6 // 8)  # as in _lane_plan
    assert [j.want.size for j in jobs] == out_len.tolist()
    _, _, arena, mask = _arena(out_off, caps, [j.want for j in jobs])
    canary = np.full(CANARY, SENT, np.uint8)
    return DecBatch(jobs, np.concatenate([j.text for j in jobs]), lens, caps, in_off, out_off, flags,
                    prev, valid, tails, np.array([j.check_tail for j in jobs]), out_len,
                    np.concatenate([canary, arena, canary]),
                    np.concatenate([canary == SENT, mask, canary == SENT]))


def test_chain_plan_covers_the_predecessor_cases():
    """Conditions on the streams alone (no GPU): each predecessor case with
    the predecessor's cumulative V mod 4 going through 0-3."""
    for abc in CHAIN_ABCS:
        A = alphabet(*abc)
        plan = chain_plan(abc)
        assert len(plan) == 3
        cases = {w: set() for w in ("same batch", "earlier batch", "chained", "big", "self big")}
        held, per_stream, content = set(), {}, set()
        for b, bp in enumerate(plan):
            fill = [j for j in bp.jobs if j.stream < 0]
            assert len(fill) == FILLERS and not any(j.flags & CHAINED for j in fill)
            assert any(j.flags & HOLD for j in fill) and not all(j.flags & HOLD for j in fill)
            for i, j in enumerate(bp.jobs):
                if j.stream < 0:
                    continue
                per_stream.setdefault(j.stream, []).append(j)
                own = j.text[4:] if j.k else j.text
                content |= {name for name, hit in (("junk", (~A.is_alpha[own] & (own != 13) & (own != 10)
                                                            & (own != 61)).any()),
                                                   ("crlf", (own == 13).any() and (own == 10).any()),
                                                   ("=", (own == 61).any())) if hit}
                if not j.flags & CHAINED:
                    assert j.k == 0 and bp.prev[i] is None
                    continue
                assert j.k > 0 and not A.is_alpha[j.text[:4]].any()
                pb, pi = bp.prev[i]
                p = plan[pb].jobs[pi]
                assert (p.stream, p.k) == (j.stream, j.k - 1) and p.flags & HOLD
                assert pb < b or (pb == b and pi < i)
                r = p.tail.size  # the predecessor's cumulative V mod 4
                assert r == p.valid % 4 == (j.valid - A.is_alpha[own].sum())
                cases["same batch" if pb == b else "earlier batch"].add(r)
                if p.flags & CHAINED:
                    cases["chained"].add(r)
                if p.text.size >= BIG:
                    cases["big"].add(r)
                    own_p = p.text[4:] if p.k else p.text  # 140,001 characters of CRLF-76
                    assert p.text.size == BIG_CHARS and (own_p[76:78] == (13, 10)).all()
                if j.text.size >= BIG:
                    cases["self big"].add(r)
                # a cut right after a character of sextet 62 or 63, which is held back
                if r and p.tail[-1] >= 62 and A.tab[p.text[-1]] == p.tail[-1]:
                    held.add(int(p.tail[-1]))
        for what, seen in cases.items():
            assert seen == {0, 1, 2, 3}, (abc, what, seen)
        assert held == {62, 63} and content == {"junk", "crlf", "="}
        sizes = {len(js) for js in per_stream.values()}
        assert sizes == {3, 4, 5, 6}, sizes
        for js in per_stream.values():
            assert [j.k for j in sorted(js, key=lambda j: (j.batch, j.key))] == list(range(len(js)))
            assert all(j.flags & HOLD for j in js[:-1]) and not js[-1].flags & HOLD
        big_unchained = [j for bp in plan for j in bp.jobs
                         if j.text.size >= BIG and not j.flags & CHAINED]
        assert big_unchained and all(j.text.size == BIG_CHARS for j in big_unchained)
    assert [A.tab[c] for A in (alphabet("-", "_"),) for c in b"-_"] == [62, 63]
    assert [alphabet(-1, -1).tab[c] for c in b"+/"] == [62, 63]


REPEAT_KINDS = ("clean A", "clean B", "CRLF-76", "CRLF-76, other content", "junk, one byte in twenty",
                "other junk of the same density", "clean")


@functools.lru_cache(maxsize=None)
def repeat_plan():
    """Seven one-batch plans with a 140,001-character job at one offset."""
    A = alphabet(-1, -1)
    rng = np.random.default_rng(SEED + 40)

    def clean():
        return A.clean(rng, BIG_CHARS)

    def crlf():
        t = np.frombuffer(_wrap(A.clean(rng, BIG_CHARS).tobytes(), 76, b"\r\n"), np.uint8)
        return t[:BIG_CHARS].copy()

    def junk():  # the density of test_repeat_junk_decode_takes_the_hinted_single_pass
        t = np.frombuffer(_junk(rng, A.clean(rng, BIG_CHARS).tobytes(), 0.05), np.uint8)
        return t[:BIG_CHARS].copy()

    bigs = [clean(), clean(), crlf(), crlf(), junk(), junk(), clean()]
    front = rng.integers(0, 1500, 40)  # the same lengths in front of the big job every time
    plans = []
    for i, big in enumerate(bigs):
        jobs = [_plain_job(A, A.clean(rng, int(n)), k % 3 == 0, k) for k, n in enumerate(front)]
        jobs.append(_plain_job(A, big, i % 2 == 1, len(jobs)))
        jobs += [_plain_job(A, _text_of_kind(A, rng, "bcdgh"[k % 5], int(rng.integers(1, 2000)), False),
                            k % 2 == 0, len(jobs) + k) for k in range(20)]
        plans.append(_dec_batch(jobs, [None] * len(jobs), SEED + 41 + i))
    return plans


def test_repeat_plan_puts_new_content_at_one_offset():
    A = alphabet(-1, -1)
    plans = repeat_plan()
    assert len(plans) == len(REPEAT_KINDS) == 7
    bigs = []
    for bp in plans:
        (i,) = np.flatnonzero(bp.lens >= BIG)
        assert bp.lens[i] == BIG_CHARS and bp.in_off[i] == plans[0].in_off[40] and i == 40
        bigs.append(bp.jobs[i].text)
    junk = [1 - A.is_alpha[t].mean() for t in bigs]
    assert all(j == 0 for j in junk[:2] + junk[6:])
    assert all(abs(j - 2 / 78) < 1e-4 and (t[76:78] == (13, 10)).all()
               for j, t in zip(junk[2:4], bigs[2:4]))
    assert all(0.04 < j < 0.055 for j in junk[4:6])
    assert len({t.tobytes() for t in bigs}) == 7


# ---- decode: on the GPU --------------------------------------------------------


class _DecBatch:
    """A DecBatch in pinned arenas of its own."""

    def __init__(self, lib, bp: DecBatch, abc):
        self.lib, self.bp, self.pin = lib, bp, _Pinned(lib)
        pin, n = self.pin, bp.lens.size
        self.n = n
        self.h_in, self.p_in = pin.array(bp.data.size + 64, np.uint8)
        self.h_in[:bp.data.size] = bp.data
        self.h_in[bp.data.size:] = 0x0A
        self.h_out, p_out = pin.array(bp.expect.size, np.uint8)
        self.h_out[:] = SENT
        self.p_out = p_out + CANARY
        self.h_in_off, self.p_in_off = pin.array(n + 1, np.uint64)
        self.h_out_off, self.p_out_off = pin.array(n + 1, np.uint64)
        self.h_flags, self.p_flags = pin.array(n, np.uint8)
        self.h_res, self.p_res = pin.array(n, RECORD)
        self.h_spell, self.p_spell = pin.array(n, RECORD)
        self.h_prev, self.p_prev = pin.array(n, np.uint64)
        self.h_in_off[:] = bp.in_off
        self.h_out_off[:] = bp.out_off
        self.h_flags[:] = bp.flags
        self.h_prev[:] = 0
        self.h_res.view(np.uint8)[:] = 0
        self.h_spell.view(np.uint8)[:] = 0
        self.abc_c = _lib.alphabet(abc[0], abc[1])
        self.seq = ctypes.c_uint32(0)

    def link(self, batches):
        """h_prev: the predecessors' records in the arenas of `batches`."""
        for i, p in enumerate(self.bp.prev):
            if p is not None:
                self.h_prev[i] = batches[p[0]].p_res + RECORD.itemsize * p[1]
        self.inputs = (self.h_in, self.h_in_off, self.h_out_off, self.h_flags, self.h_prev)
        self.before = [a.copy() for a in self.inputs]

    def queue(self, lane):
        return self.lib.b64x_lane_decode_async(lane, self.p_in, self.n, self.p_in_off, self.p_out,
                                               self.p_out_off, self.p_flags, self.p_res, self.p_prev,
                                               self.p_spell, ctypes.byref(self.abc_c), None, None,
                                               ctypes.byref(self.seq))

    def lane_check(self, lane):
        return self.lib.b64x_lane_decode_check(lane, self.seq.value, self.p_in_off, self.p_flags,
                                               self.p_res, self.p_prev, self.p_spell, self.n)

    def check(self, batches, what):
        bp, res, got = self.bp, self.h_res.copy(), self.h_out.copy()
        names = ("h_in", "in_off", "out_off", "flags", "h_prev")
        for a, b, name in zip(self.inputs, self.before, names):
            assert np.array_equal(a, b), f"{what}: {name} changed"

        def about(j):
            return (f"{what}, job {j}: {bp.lens[j]} characters, flags {bp.flags[j]}, stream "
                    f"{bp.jobs[j].stream} block {bp.jobs[j].k}, in_off {bp.in_off[j]}, out_off "
                    f"{bp.out_off[j]}")

        def first(bad):
            j = int(np.flatnonzero(bad)[0])
            return f"{about(j)}: record {res[j]}, oracle valid {bp.valid[j]}, tail {bp.tails[j]}"

        assert self.seq.value != 0
        named = ((res["nchars"] == bp.lens) & (res["seq"] == self.seq.value) &
                 (res["flags"] == (bp.flags & HOLD)))
        assert named.all(), first(~named)
        assert (res["valid"] == bp.valid).all(), first(res["valid"] != bp.valid)
        assert (res["tail_n"] == bp.valid % 4).all(), first(res["tail_n"] != bp.valid % 4)
        bad_tail = bp.check_tail & (res["tail"] != bp.tails).any(axis=1)
        assert not bad_tail.any(), first(bad_tail)
        assert (res["out_len"] == bp.out_len).all(), first(res["out_len"] != bp.out_len)
        for i, p in enumerate(bp.prev):  # the head was spelled from the predecessor's record
            if p is not None:
                assert self.h_spell[i].tobytes() == batches[p[0]].h_res[p[1]].tobytes(), about(i)
        if ((got != bp.expect) & bp.mask).any():
            if (got[:CANARY] != SENT).any() or (got[-CANARY:] != SENT).any():
                pytest.fail(f"{what}: a canary was written")
            pytest.fail(_first_bad(got[CANARY:-CANARY], bp.out_len, bp.out_off, bp.caps,
                                   lambda j: bp.jobs[j].want, about))

    def close(self):
        self.pin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("abc", CHAIN_ABCS, ids=CHAIN_IDS)
def test_lane_decode_chains_across_queued_batches(lane, abc):
    """Three decode batches queued back to back on one lane, waited for once:
    streams of 3-6 chained blocks spread over them (k_spell_head reading the
    predecessor's record from an earlier job of the batch or from an earlier
    batch's arena; predecessors that are chained themselves or were written
    by the single-buffer pipeline), every record, byte and gap exact."""
    lib, ln = lane
    batches = []
    try:
        for bp in chain_plan(abc):
            batches.append(_DecBatch(lib, bp, abc))
        for b in batches:
            b.link(batches)
        for b in batches:  # no wait in between
            assert b.queue(ln) == 0
        assert lib.b64x_lane_wait(ln) == 0
        for i, b in enumerate(batches):
            assert b.lane_check(ln) == 0, f"batch {i}"
        assert len({b.seq.value for b in batches}) == len(batches)
        for i, b in enumerate(batches):
            b.check(batches, f"batch {i}")
    finally:
        lib.b64x_lane_wait(ln)
        for b in batches:
            b.close()


def _paths(lib):
    out = (ctypes.c_uint64 * 5)()
    lib.b64x_diag_paths(out)
    return [int(v) for v in out]


@pytest.mark.gpu
def test_lane_decode_new_content_at_a_repeated_address(lane):
    """A lane's big jobs decode on its private workspace at addresses inside
    its input buffer that repeat from batch to batch, so the held line model
    and the junk hint (keyed by workspace, address and length) meet new
    content every time: seven batches, every one exact, and the probe, the
    held model's reuse and the hinted single pass all taken on the way."""
    lib, ln = lane
    before = _paths(lib)
    for kind, bp in zip(REPEAT_KINDS, repeat_plan()):
        b = _DecBatch(lib, bp, (-1, -1))
        try:
            b.link([b])
            assert b.queue(ln) == 0 and lib.b64x_lane_wait(ln) == 0, kind
            assert b.lane_check(ln) == 0, kind
            b.check([b], kind)
        finally:
            lib.b64x_lane_wait(ln)
            b.close()
    took = [a - b for a, b in zip(_paths(lib), before)]
    assert min(took[:3]) >= 1, f"probes {took[0]}, held-model reuses {took[1]}, hinted passes {took[2]}"
