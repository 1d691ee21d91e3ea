"""The host's launch plans of the one-buffer and strided line-wrapped encode
and strict decode (plan_wrap_one, plan_wrap_rows, plan_strict of
async_amd/csrc/b64x_lines_plan.h): which kernel runs, its grid and its
WrapArgs / StrictArgs.

No GPU: the plans are plain host C++.  tests/csrc/lines_plan_check.cpp is
built as the per-buffer program of tests/test_lines_batch.py is: a stand-alone
program with ASan + UBSan linked in statically, run as a child process.  What
it prints is checked here for properties the kernels rely on, with the
positions taken from the layout itself (_layout of
tests/test_decode_strict.py), not from a second copy of the plan:

  cover        hot blocks or lanes and tail pieces or lanes tile a row once
  reads        every hot window lies inside what the call may read
  reciprocals  each multiply-high is the quotient for every value a kernel
               can feed it
  fallbacks    each condition of the hot path, failing alone, gives the
               bytewise kernel with a grid of at most 2^20
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from async_amd import _lib
from tests.test_decode_strict import _layout, enc_len, formula, strict_cap
from tests.test_lines_batch import (CRLF76, HOT_FORMATS, INEXACT, LAYOUT_LENGTHS, LF64, ROOT, SHORT,
                                    _ask, char_off, dec_plan, edge_lengths)

ANY, HOT = 0, 1
TH = 256  # lanes per block, one 16-byte block or 16 characters each

WRAP_FIELDS = ("kind grid len E W full_lines in_stride out_stride hot_blocks hot_slots tail_blocks "
               "tail_slots m64 m64_hb hot_tiles L P s sep last_len magic_p magic_hb "
               "hot_blocks32").split()
STRICT_FIELDS = ("kind grid length_error E W in_stride out_stride off_e1 off_e2 hot_lanes "
                 "hot_slots tail_lanes tail_slots m64 m64_hl hot_tiles L P s sep sep_mask magic_l "
                 "magic_hl hot_lanes32 trailing").split()
BIG = [3 * (1 << 30) + 7, (1 << 40) + 5]
HOT_COUNTS = ("hot_lanes", "tail_lanes", "hot_slots", "tail_slots")  # zero in a bytewise plan


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/lines_plan_check.cpp under ASan + UBSan: the sanitizers'
    runtimes are linked into the program itself, nothing is preloaded."""
    exe = str(tmp_path_factory.mktemp("plan") / "lines_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "lines_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def lengths(L, s):
    ns = set(LAYOUT_LENGTHS) | set(edge_lengths(L, s)) | {0, 1, 16, 17, 19, 20, 21} | set(BIG)
    for k in (1, 2, 53, 54):
        ns |= {k * L * 3 // 4 + d for d in range(-2, 3)}
    return sorted(ns)


def ask(exe, kind, fields, cases):
    """cases: (L, sep, trailing, pad, in_low4, out_low4, ...) -> one dict per case."""
    rows = _ask(exe, [f"{kind} {c[0] or 0} {len(c[1])} " + " ".join(str(int(v)) for v in c[2:])
                      for c in cases])
    for r in rows:
        assert len(r) == len(fields)
    return [dict(zip(fields, r)) for r in rows]


def up(x, m):
    return -(-x // m)


def a4(x):
    return up(x, 4) * 4


# ----------------------------------------------------------- the checks --

def check_recip32(magic, d, bound):
    """(x * magic) >> 32 == x // d for every x < bound."""
    if bound <= 1 << 20:
        x = np.arange(bound, dtype=np.uint64)
        got = (x * np.uint64(magic)) >> np.uint64(32)
        assert np.array_equal(got, x // np.uint64(d)), (d, bound)
        return
    for x in edge_values(d, bound - 1):
        assert (x * magic) >> 32 == x // d, (magic, d, bound, x)


def check_recip64(m64, d, top):
    """(x * m64) >> 64 == x // d for every x <= top."""
    for x in edge_values(d, top):
        assert (x * m64) >> 64 == x // d, (m64, d, top, x)


def edge_values(d, top):
    """q d - 1, q d, q d + 1 for the first and the last 64 quotients up to `top`, and top."""
    qmax = top // d
    qs = set(range(min(64, qmax + 1))) | set(range(max(qmax - 63, 0), qmax + 1))
    return sorted({x for q in qs for x in (q * d - 1, q * d, q * d + 1) if 0 <= x <= top} | {top})


def check_grid(p, hot, tail, rows):
    """The cover: hot and tail units tile the row, slots, tiles and grid follow."""
    if p["kind"] == ANY:
        assert p["hot_tiles"] == 0 and p["grid"] <= 1 << 20
        return
    assert p["hot_slots"] == p[hot] * rows and p["tail_slots"] == p[tail] * rows
    assert p["hot_tiles"] == up(p["hot_slots"], TH)
    assert p["grid"] == p["hot_tiles"] + up(p["tail_slots"], TH) < 1 << 31
    assert p[hot] > 0


def char_at_or_after(q, L, s):
    """The first character at or after offset q of a wrapped text."""
    k, c = divmod(q, L + s)
    return k * L + c if c < L else (k + 1) * L


def hot_block_chars(p, L, s, trailing):
    """(first, last) character of every hot block (small rows: all of them, from
    the layout; else the last three, by position)."""
    hot = p["hot_blocks"]
    if p["E"] <= 8000:
        off, _, _ = _layout(p["E"], L, s, trailing)
        q = 16 * np.arange(hot, dtype=np.int64)
        first, last = np.searchsorted(off, q), np.searchsorted(off, q + 16) - 1
        assert (first < p["E"]).all() and (off[first] < q + 16).all()  # no block of separators only
        return first, last
    js = range(max(hot - 3, 0), hot)
    first = np.array([char_at_or_after(16 * j, L, s) for j in js], dtype=object)
    last = np.array([char_at_or_after(16 * j + 16, L, s) - 1 for j in js], dtype=object)
    return first, last


def check_wrap_reads(p, L, s, trailing, readable):
    """Every hot block is made of characters of complete 3-byte groups, and its
    20-byte window (from the dword at or below the first byte of its first
    character's group) ends at or before byte `readable` of the row."""
    assert 16 * p["hot_blocks"] <= p["W"]
    assert p["hot_blocks"] + p["tail_blocks"] == up(p["W"], 16)
    first, last = hot_block_chars(p, L, s, trailing)
    if len(first) == 0:
        return
    assert max(last) < p["len"] // 3 * 4
    start = first // 4 * 3 // 4 * 4
    assert min(start) >= 0 and max(start) + 20 <= readable, (p, max(start) + 20, readable)


def check_strict_reads(p, L, s, trailing):
    """Every hot lane lies below character E - 4 and its 16- or 24-byte window
    (from the dword at or below its first character) ends at or before W."""
    hot, E, W = p["hot_lanes"], p["E"], p["W"]
    assert hot + p["tail_lanes"] == up(E, 16)
    if hot == 0:
        return
    assert 16 * hot <= E - 4
    win = 16 if L is None else 24
    if E <= 8000:
        off, _, _ = _layout(E, L, s, trailing)
        assert ((off[16 * np.arange(hot)] & ~3) + win <= W).all()
    else:
        e = 16 * (hot - 1)
        o = e if L is None else e // L * (L + s) + e % L
        assert (o & ~3) + win <= W


def public_lens(L, sep, trailing):
    lib = _lib.load()
    f = None if L is None else _lib.lines(L, sep, bool(trailing))
    ref = ctypes.byref(f) if f else None
    return (lambda n, pad: lib.b64x_encoded_lines_len(n, bool(pad), ref),
            lambda W: lib.b64x_strict_decoded_cap(W, ref))


def check_wrap_common(p, n, L, sep, trailing, pad, lens):
    s = len(sep)
    assert p["len"] == n and p["E"] == enc_len(n, bool(pad))
    assert p["W"] == formula(n, bool(pad), L, s, bool(trailing)) == lens[0](n, pad)
    assert (p["full_lines"], p["last_len"]) == divmod(p["E"], L)
    assert (p["L"], p["P"], p["s"]) == (L, L + s, s)
    assert p["sep"] == int.from_bytes(b"\r\n\n\r"[:s], "little")


# ------------------------------------------------------------ one buffer --

def test_wrap_one_buffer(plan_program):
    hot_seen = 0
    for L, sep in HOT_FORMATS + [SHORT, INEXACT]:
        s = len(sep)
        checked_magic = False
        for trailing in (0, 1):
            lens = public_lens(L, sep, trailing)
            cases = [(L, sep, trailing, pad, 0, 0, n) for pad in (0, 1) for n in lengths(L, s)]
            for c, p in zip(cases, ask(plan_program, "W", WRAP_FIELDS, cases)):
                pad, n = c[3], c[6]
                check_wrap_common(p, n, L, sep, trailing, pad, lens)
                assert (p["in_stride"], p["out_stride"]) == (0, 0)
                check_grid(p, "hot_blocks", "tail_blocks", 1)
                if p["kind"] == ANY:
                    assert p["grid"] == min(up(up(p["W"], 16), TH), 1 << 20)
                    assert (L, sep) not in HOT_FORMATS or n < 32
                    continue
                hot_seen += 1
                check_wrap_reads(p, L, s, trailing, n)
                if not checked_magic:  # the format's alone; a lane's position is below P + a tile
                    check_recip32(p["magic_p"], L + s, L + s + 16 * TH)
                    checked_magic = True
                check_recip64(p["m64"], L + s, p["W"])  # a tile's first byte
        assert checked_magic == ((L, sep) in HOT_FORMATS)
    assert hot_seen > 5000


def strict_texts(L, s, trailing):
    """Lengths of texts: what the encoder writes for the payload lengths, and
    the payload lengths themselves (mostly lengths no encoder output has)."""
    ns = lengths(L or 76, s)
    return sorted({formula(n, pad, L, s, bool(trailing)) for n in ns for pad in (True, False)} |
                  set(ns))


def check_strict_common(p, W, L, sep, trailing, pad, aligned, lens):
    s = len(sep)
    want = dec_plan(W, L, s, bool(trailing), bool(pad), aligned)
    assert (p["E"], p["length_error"]) == want[:2] and p["W"] == W
    assert 3 * up(p["E"], 4) == lens[1](W) == strict_cap(W, L, s, bool(trailing))
    assert (p["L"], p["P"], p["s"]) == (L or 0, (L or 0) + s, s)
    assert p["sep"] == int.from_bytes(b"\r\n\n\r"[:s], "little")
    assert p["sep_mask"] == (1 << 8 * s) - 1
    if not p["length_error"]:
        assert (p["off_e1"], p["off_e2"]) == want[4:]
    return want


def test_strict_one_buffer(plan_program):
    hot_seen = 0
    for L, sep in HOT_FORMATS + [SHORT, INEXACT, (None, b"")]:
        s = len(sep)
        checked_magic = False
        for trailing in ((0,) if L is None else (0, 1)):
            lens = public_lens(L, sep, trailing)
            cases = [(L, sep, trailing, pad, 0, 0, 1, 0, 0, W) for pad in (0, 1)
                     for W in strict_texts(L, s, trailing)]
            for c, p in zip(cases, ask(plan_program, "S", STRICT_FIELDS, cases)):
                pad, W = c[3], c[9]
                want = check_strict_common(p, W, L, sep, trailing, pad, True, lens)
                if p["length_error"]:
                    continue
                check_grid(p, "hot_lanes", "tail_lanes", 1)
                if p["kind"] == ANY:
                    assert not any(p[k] for k in HOT_COUNTS)
                    assert p["grid"] == min(up(up(p["E"], 16), TH), 1 << 20)
                    assert (L, sep) in (SHORT, INEXACT) or p["E"] < 36
                    continue
                hot_seen += 1
                assert p["hot_lanes"] == want[2]  # the per-buffer plan's (the batch kernels')
                check_strict_reads(p, L, s, trailing)
                if L is not None:
                    if not checked_magic:  # a lane's character is below L + a tile
                        check_recip32(p["magic_l"], L, L + 16 * TH)
                        checked_magic = True
                    check_recip64(p["m64"], L, p["E"])  # a tile's first character
        assert checked_magic == ((L, sep) in HOT_FORMATS)
    assert hot_seen > 4000


# ------------------------------------------------------------------ rows --

ROW_LENGTHS = [0, 1, 16, 17, 19, 20, 21, 23, 24, 47, 48, 49, 56, 57, 58, 100, 255, 256, 257, 1000,
               1023, 1024, 1025, 3001, 4095, 4096, (1 << 20) + 1, (1 << 22) + 3, (1 << 24) + 5,
               3 * (1 << 25) - 64]
NBUFS = (2, 3, 257)


def row_lengths(L):
    ns = set(ROW_LENGTHS)
    for k in (1, 2, 53, 54):
        ns |= {k * L * 3 // 4 + d for d in range(-2, 3)}
    return sorted(ns)


def test_wrap_rows(plan_program):
    hot_seen = any_seen = 0
    for L, sep in HOT_FORMATS + [SHORT, INEXACT]:
        s = len(sep)
        for trailing in (0, 1):
            lens = public_lens(L, sep, trailing)
            cases = []
            for pad in (0, 1):
                for n in row_lengths(L):
                    W = formula(n, bool(pad), L, s, bool(trailing))
                    for nbuf in NBUFS:
                        for slack in (0, 4):  # tight (rounded up to a dword) and tight + 4
                            cases.append((L, sep, trailing, pad, 0, 0, nbuf, up(n, 4) * 4 + slack,
                                          up(W, 4) * 4 + slack, n))
            cases.append((L, sep, trailing, 1, 0, 0, (1 << 32) - 1, 1024,
                          up(formula(1024, True, L, s, bool(trailing)), 4) * 4, 1024))
            for c, p in zip(cases, ask(plan_program, "R", WRAP_FIELDS, cases)):
                pad, nbuf, in_stride, out_stride, n = c[3], c[6], c[7], c[8], c[9]
                check_wrap_common(p, n, L, sep, trailing, pad, lens)
                assert (p["in_stride"], p["out_stride"]) == (in_stride, out_stride)
                check_grid(p, "hot_blocks", "tail_blocks", nbuf - 1)  # the last row goes alone
                if p["kind"] == ANY:
                    any_seen += 1
                    assert p["grid"] == min(up(up(p["W"], 16) * nbuf, TH), 1 << 20)
                    continue
                hot_seen += 1
                assert L >= 16 and n >= 20 and p["W"] < 1 << 28
                assert p["hot_blocks"] == p["hot_blocks32"] > 1
                # a window may reach into the next row, never past its own bytes there
                check_wrap_reads(p, L, s, trailing, in_stride + n)
                check_recip32(p["magic_p"], L + s, p["W"])       # a block's offset in its row
                check_recip32(p["magic_hb"], p["hot_blocks"], p["hot_blocks"] + TH)
                check_recip64(p["m64_hb"], p["hot_blocks"], p["hot_slots"])
                if nbuf == 3 and n in (1024, 3001):  # the last row: one buffer at its address
                    low = (2 * in_stride) & 15, (2 * out_stride) & 15
                    last, = ask(plan_program, "W", WRAP_FIELDS, [(L, sep, trailing, pad, *low, n)])
                    assert last["W"] == p["W"]
                    assert (last["kind"] == HOT) == (low[1] == 0 and (L, sep) in HOT_FORMATS)
                    if last["kind"] == HOT:
                        check_wrap_reads(last, L, s, trailing, n)
            # nbuf = 2^32 - 1 rows of 1 KiB (so short a row is below INEXACT's first inexact value)
            assert (p["kind"] == HOT) == ((L, sep) != SHORT)
    assert hot_seen > 1500 and any_seen > 1000


def test_strict_rows(plan_program):
    hot_seen = any_seen = 0
    for L, sep in HOT_FORMATS + [SHORT, INEXACT, (None, b"")]:
        s = len(sep)
        for trailing in ((0,) if L is None else (0, 1)):
            lens = public_lens(L, sep, trailing)
            cases = []
            for pad in (0, 1):
                texts = {formula(n, bool(pad), L, s, bool(trailing)) for n in row_lengths(L or 76)}
                for W in sorted(texts | {1, 2, 3, 5, 77, 78, 79, 80, 1001}):
                    cap = strict_cap(W, L, s, bool(trailing))
                    for nbuf in NBUFS:
                        for slack in (0, 4):
                            cases.append((L, sep, trailing, pad, 0, 0, nbuf, up(W, 4) * 4 + slack,
                                          up(cap, 4) * 4 + slack, W))
            W = formula(1024, True, L, s, bool(trailing))
            cases.append((L, sep, trailing, 1, 0, 0, (1 << 32) - 1, up(W, 4) * 4, 1024, W))
            for c, p in zip(cases, ask(plan_program, "S", STRICT_FIELDS, cases)):
                pad, nbuf, W = c[3], c[6], c[9]
                want = check_strict_common(p, W, L, sep, trailing, pad, True, lens)
                assert (p["in_stride"], p["out_stride"]) == (c[7], c[8])
                if p["length_error"]:
                    continue
                check_grid(p, "hot_lanes", "tail_lanes", nbuf)
                if p["kind"] == ANY:
                    any_seen += 1
                    assert not any(p[k] for k in HOT_COUNTS)
                    assert p["grid"] == min(up(up(p["E"], 16) * nbuf, TH), 1 << 20)
                    continue
                hot_seen += 1
                assert (L, sep) != SHORT and W < 1 << 28
                assert p["hot_lanes"] == p["hot_lanes32"] == want[2] > 1
                check_strict_reads(p, L, s, trailing)
                if L is not None:
                    check_recip32(p["magic_l"], L, p["E"])  # a lane's first character in its row
                check_recip32(p["magic_hl"], p["hot_lanes"], p["hot_lanes"] + TH)
                check_recip64(p["m64_hl"], p["hot_lanes"], p["hot_slots"])
            assert (p["kind"] == HOT) == ((L, sep) != SHORT)  # 2^32 - 1 rows of 1 KiB
    assert hot_seen > 1500 and any_seen > 500


# ------------------------------------------------------------- fallbacks --

def test_each_condition_alone_gives_the_bytewise_kernel(plan_program):
    """Pairs of cases: the first is hot, the second differs from it in one
    condition of the hot path and is bytewise."""
    def text(n, fmt=CRLF76):
        return formula(n, True, fmt[0], len(fmt[1]), True)

    def one(n=4000, fmt=CRLF76, in_low4=0, out_low4=0):
        return "W", (*fmt, 1, 1, in_low4, out_low4, n)

    def rows(n=4000, fmt=CRLF76, nbuf=3, in_low4=0, out_low4=0, in_skew=0, out_skew=0):
        return "R", (*fmt, 1, 1, in_low4, out_low4, nbuf, a4(n) + in_skew,
                     a4(text(n, fmt)) + out_skew, n)

    def strict(n=4000, fmt=CRLF76, nbuf=1, in_low4=0, out_low4=0, in_skew=0, out_skew=0):
        W = text(n, fmt)
        return "S", (*fmt, 1, 1, in_low4, out_low4, nbuf, a4(W) + in_skew,
                     a4(strict_cap(W, fmt[0], len(fmt[1]), True)) + out_skew, W)

    def strict_rows(**kw):
        return strict(**{"nbuf": 3, **kw})

    forms = (one, rows, strict, strict_rows)
    pairs = []
    # L < 16
    pairs += [(f(fmt=(16, b"\n")), f(fmt=(12, b"\n"))) for f in forms]
    # a misaligned pointer or stride
    for f in forms:
        for low in (1, 2, 3):
            pairs += [(f(), f(in_low4=low)), (f(), f(out_low4=low))]
    for f in (rows, strict_rows):
        pairs += [(f(in_low4=4, out_low4=12), f(in_skew=k)) for k in (1, 2)]
        pairs += [(f(in_low4=8, out_low4=4), f(out_skew=k)) for k in (2, 3)]
    # one buffer: the encode's output 16-byte aligned; strides are not looked at
    pairs += [(one(in_low4=4), one(out_low4=4)), (one(in_low4=12), one(out_low4=8))]
    pairs += [(strict(in_skew=1, out_skew=1, out_low4=12), strict(in_low4=5))]
    # P > 2^24 (powers of two: the reciprocals are exact)
    wide, wider = ((1 << 24) - 4, b"\r\n\n\r"), ((1 << 25) - 4, b"\r\n\n\r")
    pairs += [(f(fmt=wide), f(fmt=wider)) for f in (one, rows)]
    # an inexact reciprocal (more text than one of its lines)
    pairs += [(f(n=300000), f(n=300000, fmt=INEXACT)) for f in forms]
    # rows of 2^28 bytes of text or more.  Formats whose divisor is a power of two (the
    # reciprocal of 78 is inexact from 2^32 / 56 on), and hot counts whose reciprocals are
    # exact on both sides: 257 * 16,711,936 = 2^32 + 256 and 263 * 16,330,675 = 2^32 + 229
    p64, l64 = (60, b"\r\n\n\r"), LF64

    def payload_with_blocks(target):
        e = target * 16 * 60 // 64 // 4 * 4
        while char_off(e, 60, 4) // 16 < target:
            e += 4
        return e // 4 * 3

    below, above = payload_with_blocks(16711936), payload_with_blocks(1 << 24)
    assert text(below, p64) < 1 << 28 <= text(above, p64)
    pairs.append((rows(n=below, fmt=p64), rows(n=above, fmt=p64)))
    # (the lane in front of the last group has no 24 bytes of text behind its start)
    below, above = (16 * 16330676 + 4) // 4 * 3, (16 * ((1 << 24) + 1) + 4) // 4 * 3
    assert text(below, l64) < 1 << 28 <= text(above, l64)
    pairs.append((strict_rows(n=below, fmt=l64), strict_rows(n=above, fmt=l64)))
    near = [ask(plan_program, q, STRICT_FIELDS if q == "S" else WRAP_FIELDS, [c])[0]
            for (q, c), _ in pairs[-2:]]
    assert (near[0]["hot_blocks32"], near[1]["hot_lanes32"]) == (16711936, 16330675)
    # a grid of 2^31 blocks or more
    many = (1 << 32) - 1
    pairs += [(one(n=3 << 40), one(n=3 << 41)), (strict(n=3 << 40), strict(n=3 << 41)),
              (rows(n=1024, nbuf=many), rows(n=2048, nbuf=many)),
              (strict(n=1023, nbuf=many), strict(n=2046, nbuf=many))]
    # rows with one hot block or lane
    pairs += [(rows(n=24), rows(n=23)), (strict_rows(n=36), strict_rows(n=24))]
    fields = {"W": WRAP_FIELDS, "R": WRAP_FIELDS, "S": STRICT_FIELDS}
    for (q, hot), (q2, cold) in pairs:
        assert q == q2
        a, b = ask(plan_program, q, fields[q], [hot, cold])
        assert not a.get("length_error") and not b.get("length_error"), (q, hot, cold)
        assert a["kind"] == HOT, (q, hot, a)
        assert b["kind"] == ANY and 0 < b["grid"] <= 1 << 20, (q, cold, b)
        assert b["hot_tiles"] == 0


def test_pointer_and_stride_alignment_all_sixteen(plan_program):
    """Rows are hot exactly when both addresses and both strides are dword
    aligned; one buffer of text needs the addresses alone, one buffer of the
    encode a dword-aligned input and a 16-byte aligned output."""
    L, sep = LF64
    n = 3001
    W = formula(n, True, L, 1, True)
    cap = strict_cap(W, L, 1, True)
    r_cases, s_cases, o_cases = [], [], []
    for mis in range(16):
        il, ol, si, so = 2 * (mis & 1), 5 * (mis >> 1 & 1), mis >> 2 & 1, 3 * (mis >> 3 & 1)
        r_cases.append((L, sep, 1, 1, il, ol, 5, a4(n) + si, a4(W) + so, n))
        s_cases.append((L, sep, 1, 1, il, ol, 5, a4(W) + si, a4(cap) + so, W))
        o_cases.append((L, sep, 1, 1, il, ol, 1, a4(W) + si, a4(cap) + so, W))
    for mis, (r, d, o) in enumerate(zip(ask(plan_program, "R", WRAP_FIELDS, r_cases),
                                        ask(plan_program, "S", STRICT_FIELDS, s_cases),
                                        ask(plan_program, "S", STRICT_FIELDS, o_cases))):
        assert (r["kind"] == HOT) == (mis == 0), mis
        assert (d["kind"] == HOT) == (mis == 0), mis
        assert (o["kind"] == HOT) == (mis & 3 == 0), mis
    w_cases = [(L, sep, 1, 1, il, ol, n) for il in range(16) for ol in range(16)]
    for c, w in zip(w_cases, ask(plan_program, "W", WRAP_FIELDS, w_cases)):
        assert (w["kind"] == HOT) == (c[4] % 4 == 0 and c[5] == 0), c


def test_pitch_past_32_bits(plan_program):
    """line_len + sep_len past 2^32 - 1: every call refuses the format, and the
    two length functions still answer (the wrapped text's length as the
    formula gives it; capacity 0)."""
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    ns = [0, 1, 57, 4000] + BIG
    for L, sep in ((0xFFFFFFFC, b"\r\n\n\r"), (0xFFFFFFFE, b"\r\n\n"), (0xFFFFFFFF, b"\r\n\n\r"),
                   (0xFFFFFFFC, b"\r\n\n")):
        s = len(sep)
        for trailing in (False, True):
            f = _lib.lines(L, sep, trailing)
            for pad in (False, True):
                for n in ns:
                    assert lib.b64x_encoded_lines_len(n, pad, ctypes.byref(f)) == \
                        formula(n, pad, L, s, trailing), (L, s, trailing, pad, n)
            for W in ns + [L, L + s, L + s + 1]:
                want = 0 if L + s >= 1 << 32 else strict_cap(W, L, s, trailing)
                assert lib.b64x_strict_decoded_cap(W, ctypes.byref(f)) == want, (L, s, W)
            if L + s >= 1 << 32:
                ra, rf = ctypes.byref(a), ctypes.byref(f)
                assert lib.b64x_encode_lines_dev(p, 30, p, ra, rf, None) == -22
                assert lib.b64x_decode_strict_dev(p, 40, p, p, ra, rf, None) == -22
    # the plan of such a pitch is bytewise and divides by nothing
    for w in ask(plan_program, "W", WRAP_FIELDS, [(0xFFFFFFFC, b"\r\n\n\r", 1, 1, 0, 0, n)
                                                 for n in (30, 4000, BIG[1])]):
        assert w["kind"] == ANY and w["P"] == 0
        assert w["W"] == formula(w["len"], True, 0xFFFFFFFC, 4, True)
