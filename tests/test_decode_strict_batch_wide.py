"""The ragged strict decode balanced over the batch's bytes
(b64x_decode_strict_batch_wide, async_amd.b64.decode_strict_batch_wide): plain
and line-wrapped, texts of any size in one call, one record per text.

Expected records come from the scalar procedure of include/b64x.h written in
Python (tests/test_decode_strict.py's strict_ref, and np_ref, its vectorised
copy, for texts past a few hundred bytes), expected bytes from the payloads
the texts were made of (ref_text: the stdlib's encode, wrapped in Python) and,
on the GPU, both also from the existing ragged call (decode_strict_batch) on
the same tensors.  The new call is never compared with itself.  Every
comparison is exact.

CPU tests: the plan (async_amd/csrc/b64x_strict_wide_plan.h) built as a host
program under ASan + UBSan and checked against the same rules restated here in
Python -- the grid, the shares, the spans, and that the lane ranges owned over
any set of span boundaries partition a text's lanes exactly, each lane with
the span that holds its first character; the argument checks in order through
the C ABI; the exports; the new code object's kernels and barriers;
conditions on the GPU tests' own inputs.

GPU tests: every output capacity stands between 64-byte guards of 0xA5 and
the arena is compared whole except the capacities of refused texts; the input
arena has guard bytes before and after it in the same tensor and must be
unchanged; the records are filled with 0xA5 before each call and have a guard
behind them."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from async_amd import _lib
from tests import util
from tests.test_decode_strict import (BITS, CHAR, LENGTH, OK, PAD, SEP, STD, alpha, formula, np_ref,
                                      ref_text, stdlib_decode, strict_cap, strict_ref,
                                      text_chars)

ROOT = util.ROOT
GUARD = 64
FILL = 0xA5
REC = 24
URL_NOPAD = ("-", "_", False, -1)

# name -> (L, sep, trailing, abc); L None: plain.  tests/test_encode_batch_wide.py's seven.
FORMATS = {
    "plain_pad": (None, b"", True, STD),
    "plain_nopad_url": (None, b"", True, URL_NOPAD),
    "crlf76_trailing": (76, b"\r\n", True, STD),
    "crlf76": (76, b"\r\n", False, STD),
    "lf64": (64, b"\n", True, STD),
    "l16s4": (16, b"\r\n\r\n", True, STD),
    "l4s1": (4, b"\n", True, STD),   # L < 16: never fast, all bytewise
}
ALL = sorted(FORMATS)

# The constants of b64x_strict_wide_plan.h, restated (test_plan_constants
# reads them back from the program).
T = 16384          # text bytes a wave takes at least: 16 passes of 64 lanes of 16 characters
UNIT = 16          # shares are multiples of it
BLOCK_WAVES = 4
BLOCKS_PER_CU = 8
EMPTY_RUN = 8
CUS = 256          # an MI355X; the model takes any


# ------------------------------------------ the plan, written out in Python --

def grid_blocks(hint, cus=CUS):
    cap = BLOCKS_PER_CU * cus
    return cap if hint == 0 else min(max(-(-hint // (BLOCK_WAVES * T)), 1), cap)


def share(total, waves):
    return max(T, UNIT * -(-total // (UNIT * waves)))


def span(total, waves, w):
    """Wave w's arena span, or None."""
    S = share(total, waves)
    return (w * S, min(total, (w + 1) * S)) if w * S < total else None


def boundaries(total, hint, cus=CUS):
    """The arena positions at which one wave's span ends and the next one's
    begins."""
    S = share(total, BLOCK_WAVES * grid_blocks(hint, cus))
    return list(range(S, total, S))


def char_off(e, L, s):
    return e if L is None else e // L * (L + s) + e % L


def call_fast(L):
    """The call-level rule of the decode (lines_plan::make_call): the divisor
    is the line length."""
    if L is None:
        return True
    if L < 16:
        return False
    err = (0xFFFFFFFF + L) // L * L - (1 << 32)
    return (L + 4096) * err < 1 << 32


def text_plan(W, L, s, trailing, pad, aligned):
    """(length_error, E, hot_lanes, tail_lanes) of a text of W bytes
    (lines_plan::strict_plan)."""
    if W == 0:
        return 0, 0, 0, 0
    E, _ = text_chars(W, L, s, trailing)
    if E is None or (pad and E % 4) or (not pad and E % 4 == 1):
        return 1, None, 0, 0
    hot = 0
    if aligned and call_fast(L) and E >= 20:
        hot = (E - 4) // 16
        win = 24 if L is not None else 16
        while hot > 0 and (char_off((hot - 1) * 16, L, s) & ~3) + win > W:
            hot -= 1
    return 0, E, hot, -(-E // 16) - hot


def chars_below(x, L, s):
    return x if L is None else x // (L + s) * L + min(x % (L + s), L)


def cut(x, W, lanes, L, s):
    if x == 0:
        return 0
    if x >= W:
        return lanes
    return min(lanes, -(-chars_below(x, L, s) // 16))


# ------------------------------------------------------------------- CPU --

@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/strict_wide_plan_check.cpp built with the host compiler
    under ASan + UBSan: a stand-alone program, run as a child process, the
    sanitizers' runtimes linked into the program itself."""
    exe = str(tmp_path_factory.mktemp("plan") / "strict_wide_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "strict_wide_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _ask(exe, queries):
    run = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows


def test_plan_constants(plan_program):
    assert _ask(plan_program, ["K"]) == [(T, UNIT, BLOCK_WAVES, BLOCKS_PER_CU, EMPTY_RUN)]
    assert T == 16 * 64 * 16 and T % UNIT == 0 and UNIT == 16


TOTALS = sorted({0, 1, 15, 16, 17, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 100003,
                 31 << 20, (600 << 20) + 5}
                | {(1 << 32) + d for d in (-1, 0, 1)} | {(1 << 63) + d for d in (-1, 0, 1)}
                | {(1 << 64) - d for d in (1, 2, 15, 16, 17, 8192 * 16, 8192 * 16 + 1)})
WAVES = [4, 8, 12, 4 * 661, 4 * 2047, 8192, 4 * 8 * 304]


def test_grid_and_shares(plan_program):
    # the grid: within [1, 8 CUs], from the hint and the device alone
    hints = sorted({0, 1, T, 4 * T - 1, 4 * T, 4 * T + 1, 100 * T, 31 << 20, 64 << 20, 1 << 40,
                    (1 << 64) - 1})
    cases = [(h, cus) for h in hints for cus in (1, 64, 256, 304)]
    got = _ask(plan_program, [f"G {h} {cus}" for h, cus in cases])
    for (h, cus), (g,) in zip(cases, got):
        assert g == grid_blocks(h, cus) and 1 <= g <= BLOCKS_PER_CU * cus, (h, cus, g)
    assert grid_blocks(0) == grid_blocks(1 << 40) == BLOCKS_PER_CU * CUS
    assert grid_blocks(1) == grid_blocks(4 * T) == 1 and grid_blocks(4 * T + 1) == 2
    # the share: S Wv >= total up to 2^64 - 1 (the program multiplies in 128 bits)
    cases = [(t, w) for t in TOTALS for w in WAVES]
    got = _ask(plan_program, [f"S {t} {w}" for t, w in cases])
    for (t, w), (S, covers) in zip(cases, got):
        assert S == share(t, w) and covers == 1 and S * w >= t, (t, w, S)
        assert S >= T and S % UNIT == 0
    # the spans: end to end from 0 to total, nothing owned past it
    for t in TOTALS:
        for w in (4, 4 * 661, 8192):
            got = _ask(plan_program, [f"N {t} {w} {i}" for i in range(w)])
            at = 0
            for i, (owns, lo, hi) in enumerate(got):
                want = span(t, w, i)
                assert (owns, lo, hi) == ((1,) + want if want else (0, 0, 0)), (t, w, i)
                if owns:
                    assert lo == at and lo < hi <= t
                    at = hi
            assert at == t, (t, w)


# (L, s, trailing, pad) of the seven formats
PLAN_FORMATS = [(None, 0, True, True), (None, 0, True, False), (76, 2, True, True),
                (76, 2, False, True), (64, 1, True, True), (16, 4, True, True),
                (4, 1, True, True)]


def plan_lengths(L, s, trailing, pad):
    """Every W of a valid text of 0..300 payload bytes, every W from 1 to 400
    that is no encoder output, W near T, 2 T and 3 T, and W at 2^32 +- 3,
    3 2^30 + 7 and 2^40 + 5, each with the valid lengths next to it."""
    ws = {formula(n, pad, L, s, trailing) for n in range(301)}
    ws |= {W for W in range(1, 401) if text_plan(W, L, s, trailing, pad, False)[0]}
    far = ({k * T + d for k in (1, 2, 3) for d in range(-3, 4)}
           | {(1 << 32) + d for d in range(-3, 4)} | {3 * (1 << 30) + 7, (1 << 40) + 5})
    ws |= far
    for W in far:  # the texts of about that length
        n0 = W * 3 // 4 if L is None else W * L // (L + s) * 3 // 4
        ws |= {formula(n, pad, L, s, trailing) for n in range(max(n0 - 3, 0), n0 + 4)}
    return sorted(ws)


def test_owned_lanes_partition_every_text(plan_program):
    rng = np.random.default_rng(0x5D1C)
    cases = []
    for L, s, trailing, pad in PLAN_FORMATS:
        for W in plan_lengths(L, s, trailing, pad):
            for aligned in (0, 1):
                if W <= 400:  # a boundary at every byte, and past the end
                    xs = list(range(W + 3))
                else:
                    near = [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)]
                    xs = sorted({0, 1, 2, 3, W - 2, W - 1, W, W + 1, W + T}
                                | {x for x in near if x < W}
                                | {int(x) for x in rng.integers(1, W, 40, dtype=np.uint64)})
                cases.append((L, s, trailing, pad, aligned, W, xs))
    got = _ask(plan_program, [f"U {L or 0} {s} {int(t)} {int(p)} {al} {W} " + " ".join(map(str, xs))
                              for L, s, t, p, al, W, xs in cases])
    hot_seen = refused = past32 = 0
    for (L, s, trailing, pad, aligned, W, xs), row in zip(cases, got):
        key = (L, s, trailing, pad, aligned, W)
        bad, E, hot, tail = text_plan(W, L, s, trailing, pad, bool(aligned))
        assert row[0] == bad, key
        cuts = row[4:]
        if bad:  # a LENGTH verdict owns no lanes
            assert set(cuts) == {0}, key
            refused += 1
            continue
        assert row[1:4] == (E, hot, tail), (key, row[:4], (E, hot, tail))
        lanes = hot + tail
        assert lanes == -(-E // 16)
        assert list(cuts) == [cut(x, W, lanes, L, s) for x in xs], key
        # spans [xs[i], xs[i + 1]) of the text: ranges end to end from 0 to lanes
        assert cuts[0] == 0 and cuts[-1] == lanes, key
        assert all(a <= b for a, b in zip(cuts, cuts[1:])), key
        # the owner of a lane is the span that holds its first character: so for
        # the first and the last lane of every range, and char_off is monotone
        for a, z, ja, jz in zip(xs, xs[1:], cuts, cuts[1:]):
            if ja < jz:
                assert a <= char_off(16 * ja, L, s) and char_off(16 * (jz - 1), L, s) < z, (key, a, z)
        # a hot lane lies below character E - 4, its window inside the text
        assert hot == 0 or (aligned and 16 * hot <= E - 4)
        if hot:
            assert (char_off(16 * (hot - 1), L, s) & ~3) + (24 if L else 16) <= W
        hot_seen += hot > 0
        past32 += W >= 1 << 32
    assert hot_seen > 500 and refused > 500 and past32 > 20


def _raw(L, s, sep, flags):
    return _lib.Lines(L, s, (ctypes.c_uint8 * 4)(*sep), flags)


BAD_FORMATS = [(6, 2, b"\r\n", 1), (0, 2, b"\r\n", 1), (76, 5, b"\r\n\r\n", 1), (76, 0, b"", 1),
               (76, 1, b"A", 1), (76, 2, b"\n/", 0), (76, 2, b"\r\n", 2),
               (76, 2, b"\r\n", 0x80000001)]
BAD_ALPHABETS = [("-", "-", True, -1), ("A", "/", True, -1), ("+", "7", True, -1),
                 ("+", "/", True, "B"), ("+", "/", True, "+"), ("-", "_", True, "_")]


def test_invalid_arguments_in_order():
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    ok = _lib.lines(76, b"\r\n", True)
    nodev = lib.b64x_device_check() == -19

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def dec(fmt=ok, abc=a, nbuf=3, hint=0, d_in=p, in_off=p, d_out=p, out_off=p, d_res=p):
        return lib.b64x_decode_strict_batch_wide(d_in, in_off, nbuf, hint, d_out, out_off, d_res,
                                                 ref(abc), ref(fmt), None)

    bad_fmt = _raw(75, 9, b"AAAA", 6)
    bad_abc = _lib.alphabet("-", "-")
    # 1. nbuf == 0 returns 0 whatever else is wrong
    assert dec(nbuf=0, d_in=None, in_off=None, d_out=None, out_off=None, d_res=None, fmt=None) == 0
    assert dec(nbuf=0, fmt=bad_fmt, abc=bad_abc, d_res=p + 4) == 0
    # 2. NULL pointers and the records' alignment, before the format is looked at
    for k in ("d_in", "in_off", "d_out", "out_off", "d_res"):
        for fmt in (ok, None, bad_fmt):
            assert dec(fmt=fmt, **{k: None}) == -22, k
    for skew in (1, 2, 4, 7):
        assert dec(d_res=p + skew) == -22
        assert dec(d_res=p + skew, fmt=None, abc=bad_abc) == -22
    # 3. with fmt, the format rules of b64x_decode_strict_dev
    for L, s, sep, flags in BAD_FORMATS:
        f = _raw(L, s, sep, flags)
        for hint in (0, 1 << 20):
            assert dec(fmt=f, hint=hint) == -22, (L, s, sep, flags)
        assert lib.b64x_decode_strict_dev(p, 30, p, p, ref(a), ref(f), None) == -22
    url = _lib.alphabet("-", "_")
    assert dec(fmt=_raw(76, 1, b"-", 1), abc=url) == -22
    # 4. then the alphabet rules
    for abc in BAD_ALPHABETS:
        for fmt in (ok, None):
            assert dec(fmt=fmt, abc=_lib.alphabet(*abc)) == -22, abc
        assert lib.b64x_decode_strict_dev(p, 32, p, p, ref(_lib.alphabet(*abc)), None, None) == -22
    # 5. valid calls stop at the device check
    if nodev:
        for hint in (0, 1, 1 << 20, (1 << 64) - 1):
            assert dec(hint=hint) == -19
            assert dec(fmt=None, hint=hint) == -19
        assert dec(fmt=None, abc=None) == -19
        assert dec(fmt=_raw(76, 1, b"+", 1), abc=url) == -19
        assert dec(fmt=_raw(4, 1, b"\n", 0)) == -19
        assert dec(abc=_lib.alphabet("-", "_", False, "-")) == -19  # no pad: padchar is not read
        assert dec(nbuf=(1 << 32) - 1) == -19
        assert dec(d_res=p + 8) == -19


def test_symbol_exported_by_all_three_libraries():
    name = "b64x_decode_strict_batch_wide"
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "async_amd", "libasync_b64_core.so"),
                 os.path.join(ROOT, "tests", "csrc", "libb64x_hooks.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                             check=True).stdout
        assert re.search(rf"\bT {name}$", out, re.M), path
    lib = _lib.load()
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 10
    assert getattr(lib, name).restype is ctypes.c_int
    assert "abi=7" in lib.b64x_build_info().decode()
    with open(os.path.join(ROOT, "include", "b64x.h")) as f:
        assert re.search(rf"^int {name}\(", f.read(), re.M)
    from async_amd import b64
    assert callable(b64.decode_strict_batch_wide) and "decode_strict_batch_wide" in b64.__doc__


WIDE_KERNELS = {"k_decode_strict_wide<false>", "k_decode_strict_wide<true>",
                "k_strict_wide_clear", "k_strict_wide_record"}


def test_wide_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_strict_wide.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == WIDE_KERNELS, (got - WIDE_KERNELS, WIDE_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == 2  # one per decode kernel, after its table
    main = isa_check.kernel_symbols(isa_check.disassemble(_lib.LIB_PATH))
    assert not any("strict_wide" in n for n in main)


# ------------------------------------------------- the GPU tests' batches --

def _data(n, seed):
    return util.splitmix64(seed, n).tobytes()


@functools.lru_cache(maxsize=None)
def _text(n, seed, name):
    L, sep, trailing, abc = FORMATS[name]
    return ref_text(_data(n, seed), L, sep, trailing, abc)


@functools.lru_cache(maxsize=4096)
def _verdict(t, name):
    """(kind, pos, out_len) of text t: the scalar procedure, its vectorised
    copy from a few hundred bytes on."""
    L, sep, trailing, abc = FORMATS[name]
    if len(t) <= 400:
        return strict_ref(t, L, sep, trailing, abc)
    kind, pos, out_len = np_ref(np.frombuffer(t, np.uint8), L, sep, trailing, abc)
    return int(kind), int(pos), int(out_len)


class Batch:
    """Texts and where they stand: the input arena from byte in_base of its
    tensor, texts end to end; the capacity of output i at a 16-byte boundary
    plus skew[i], GUARD bytes or more of FILL before and after it.  payloads[i]
    is what an accepted text i decodes to (None: ask the stdlib)."""

    def __init__(self, name, texts, payloads=None, in_base=GUARD, skews=None):
        L, sep, trailing, abc = FORMATS[name]
        self.name = name
        self.texts = texts
        n = len(texts)
        self.lens = np.array([len(t) for t in texts], np.int64)
        self.in_base = in_base
        self.in_off = in_base + np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.total = int(self.lens.sum())
        self.skews = np.zeros(n, np.int64) if skews is None else np.asarray(skews, np.int64)
        data = np.full(in_base + self.total + GUARD, FILL, np.uint8)
        data[in_base:in_base + self.total] = np.frombuffer(b"".join(texts), np.uint8)
        self.data = data
        verdicts = [_verdict(t, name) for t in texts]
        self.kinds = np.array([v[0] for v in verdicts], np.int64)
        # a record as three 64-bit words: out_len, err_pos, err (reserved: 0)
        self.recs = np.array([[v[2], v[1], v[0]] for v in verdicts], np.uint64).reshape(n, 3)
        self.out_off = np.zeros(n, np.int64)
        pos = GUARD
        caps = [strict_cap(len(t), L, len(sep), trailing) for t in texts]
        for i in range(n):
            self.out_off[i] = -(-pos // 16) * 16 + self.skews[i]
            pos = int(self.out_off[i]) + caps[i] + GUARD
        self.expect = np.full(pos, FILL, np.uint8)
        self.compared = np.ones(pos, bool)  # all but the capacities of refused texts
        for i, (o, t) in enumerate(zip(self.out_off, texts)):
            if self.kinds[i] != OK:
                self.compared[o:o + caps[i]] = False
                continue
            d = payloads[i] if payloads is not None and payloads[i] is not None \
                else stdlib_decode(t, abc)
            assert len(d) == verdicts[i][2] <= caps[i], i
            self.expect[o:o + len(d)] = np.frombuffer(d, np.uint8)


def valid_batch(name, items, **kw):
    """A batch of encoder texts: items are (payload bytes, seed)."""
    return Batch(name, [_text(n, seed, name) for n, seed in items],
                 [_data(n, seed) for n, seed in items], **kw)


gpu = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _first_bad(bad, off):
    at = int(np.flatnonzero(bad)[0])
    i = int(np.searchsorted(off, at, side="right")) - 1
    return (f"{int(bad.sum())} bytes differ, the first at {at} of the arena "
            f"(text {i} starts at {off[max(i, 0)]})")


def _records(res, nbuf):
    got = res.cpu().numpy()
    assert (got[REC * nbuf:] == FILL).all(), "written behind the records"
    return got[:REC * nbuf].view(np.uint64).reshape(nbuf, 3)


def _check(batch, out, res, what):
    nbuf = len(batch.texts)
    recs = _records(res, nbuf)
    if not np.array_equal(recs, batch.recs):
        i = int(np.flatnonzero((recs != batch.recs).any(axis=1))[0])
        pytest.fail(f"{what}: record {i} of {nbuf} (text of {batch.lens[i]} bytes) is "
                    f"{recs[i].tolist()}, expected {batch.recs[i].tolist()} (out_len, err_pos, err)")
    got = out.cpu().numpy()
    bad = (got != batch.expect) & batch.compared
    if bad.any():
        pytest.fail(f"{what}: " + _first_bad(bad, batch.out_off))


def run_wide(batch, hint=None, existing=False):
    """One decode_strict_batch_wide over the batch: every record and the whole
    output arena against the references and, with `existing`, against the
    existing ragged call on the same tensors."""
    from async_amd import b64
    L, sep, trailing, abc = FORMATS[batch.name]
    nbuf = len(batch.texts)
    x, d_in_off, d_out_off = _dev(batch.data), _dev(batch.in_off), _dev(batch.out_off)
    out = torch.full((batch.expect.size,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
    b64.decode_strict_batch_wide(x, d_in_off, out, d_out_off, res, L, sep, trailing,
                                 total_hint=hint, abc=abc)
    _check(batch, out, res, f"{batch.name} hint={hint}")
    assert np.array_equal(x.cpu().numpy(), batch.data), "the input was written"
    if existing:
        old = torch.full((batch.expect.size,), FILL, dtype=torch.uint8, device=DEV)
        old_res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        b64.decode_strict_batch(x, d_in_off, old, d_out_off, old_res, L, sep, trailing, abc=abc)
        assert torch.equal(old_res, res), f"{batch.name}: records differ from the existing call's"
        keep = _dev(batch.compared)
        assert torch.equal(old[keep], out[keep]), f"{batch.name}: bytes differ from the existing call's"


def spoil(t, at, byte):
    """Text t with one byte replaced."""
    b = bytearray(t)
    b[at] = byte
    return bytes(b)


# Case 2: one text at the share's edges and the line's.
PLACEMENTS = [(0, 0), (1, 0), (0, 3), (2, 1), (3, 2)]  # (input, output) offsets off a dword


def edge_payloads(name):
    """Payload lengths whose texts are within 6 bytes of k T (k = 1..3), and
    the lengths next to whole lines (1, 2, 3, 215, 216 and 431 of them)."""
    L, sep, trailing, abc = FORMATS[name]
    pad = alpha(abc)[1]
    ns = set()
    for k in (1, 2, 3):
        n0 = k * T * 3 // 4 if L is None else k * T * L // (L + len(sep)) * 3 // 4
        ns |= {n for n in range(n0 - 40, n0 + 40)
               if abs(formula(n, pad, L, len(sep), trailing) - k * T) <= 6}
    line = 57 if L is None else 3 * L // 4
    ns |= {line * k + d for k in (1, 2, 3, 215, 216, 431) for d in (-1, 1)}
    return sorted(ns)


# Case 3: the sliding batch.
SLIDE_HINTS = (T, 64 << 20)  # one block: shares of a quarter of the arena; shares of T
SLIDE_TINY = range(10, 26)   # the small texts of 1..3 payload bytes
SLIDE_ODD = (12, 15, 18, 21)  # among them four single bytes that are no texts: the texts behind
                              # them start 1..4 bytes off the grid of the format's text lengths


@functools.lru_cache(maxsize=None)
def sliding_payloads(name):
    """Case 3 without its leading text: one long text, then 40 small ones of
    1..3,000 payload bytes, 16 of them of 1..3: the long text's length puts
    the middle of those 16 on arena byte 7 T when the leading text has 24
    payload bytes, so that with shares of T a boundary walks through their
    first and last bytes as the leading text grows.  -1 stands for the one
    byte "A", a length no encoder writes (where all texts have even lengths,
    or multiples of 5, a boundary would never stand on a last byte)."""
    L, sep, trailing, abc = FORMATS[name]
    pad = alpha(abc)[1]

    def f(n):
        return formula(n, pad, L, len(sep), trailing)
    rng = np.random.default_rng(0x511D)
    small = [int(n) for n in rng.integers(1, 3001, 40)]
    for k, i in enumerate(SLIDE_TINY):
        small[i] = 1 + k % 3
    for i in SLIDE_ODD:
        small[i] = 0  # (counted as empty here: a byte more or less)
    before = f(24) + sum(f(n) for n in small[:SLIDE_TINY[0]]) + \
        sum(f(small[i]) for i in SLIDE_TINY) // 2
    want = 7 * T - before
    n0 = want * 3 // 4 if L is None else want * L // (L + len(sep)) * 3 // 4
    long = min(range(n0 - 60, n0 + 60), key=lambda n: abs(f(n) - want))
    for i in SLIDE_ODD:
        small[i] = -1
    return [long] + small


def sliding_batch(name, lead):
    lens = [lead] + sliding_payloads(name)
    items = [(max(n, 0), 3 * i + 1 if i else 1000 + lead) for i, n in enumerate(lens)]
    texts = [_text(n, seed, name) for n, seed in items]
    payloads = [_data(n, seed) for n, seed in items]
    for i, n in enumerate(lens):
        if n < 0:
            texts[i], payloads[i] = b"A", None
    for i in range(5, len(texts), 9):  # a few refused ones among them
        if len(texts[i]) > 8:
            texts[i] = spoil(texts[i], len(texts[i]) // 2, 0x2A)
            payloads[i] = None
    return Batch(name, texts, payloads)


def test_sliding_cuts_reach_every_kind_of_boundary():
    """Conditions on case 3's inputs alone, from the model: over the formats,
    the 48 leading lengths and the two hints a span boundary stands in
    mid-quad, inside a separator, and on a text's first and last byte; with
    total_hint = T the grid is one block whose four waves take a quarter of
    the arena each, with 64 MiB the shares are T."""
    seen = set()
    for name in ALL:
        L, sep, trailing, abc = FORMATS[name]
        pad, s = alpha(abc)[1], len(sep)
        for lead in range(48):
            lens = np.array([formula(n, pad, L, s, trailing) if n >= 0 else 1
                             for n in [lead] + sliding_payloads(name)])
            start = np.concatenate([[0], np.cumsum(lens)])
            total = int(start[-1])
            for hint in SLIDE_HINTS:
                waves = BLOCK_WAVES * grid_blocks(hint)
                S = share(total, waves)
                if hint == T:
                    assert waves == 4 and S > T and 3 * S < total
                else:
                    assert S == T and waves * T > total
                for at in boundaries(total, hint):
                    i = int(np.searchsorted(start, at, side="right")) - 1
                    x, W = at - int(start[i]), int(lens[i])
                    if x == 0:
                        seen.add((name, "first"))
                    if x == W - 1:
                        seen.add((name, "last"))
                    if L is not None and x % (L + s) >= L:
                        seen.add((name, "separator"))
                    elif (x if L is None else x % (L + s)) % 4:
                        seen.add((name, "mid-quad"))
    kinds = {k for _, k in seen}
    assert kinds == {"first", "last", "separator", "mid-quad"}, kinds
    # a text's first and last byte in every format
    for name in ALL:
        assert {(name, "first"), (name, "last")} <= seen, name


# Case 4: the hub-like batch.
def _land(lens, i, f, mod):
    """Shorten small payloads among lens[:i] until the texts before text i
    take a multiple of `mod` bytes; False if that cannot be done."""
    small = [j for j in range(i) if 200 <= lens[j] <= 4096]
    r = sum(f(int(n)) for n in lens[:i]) % mod
    for j in small:  # coarse: whole steps while much is left
        while r > 100 and lens[j] > 200:
            d = f(int(lens[j])) - f(int(lens[j]) - 1)
            if d > r:
                break
            lens[j] -= 1
            r -= d
    if r == 0:
        return True
    for a in small[-6:]:  # fine: two texts, one of which may grow
        for b in small[-6:]:
            if a == b:
                continue
            for da in range(-60, 61):
                for db in range(-60, 61):
                    na, nb = int(lens[a]) + da, int(lens[b]) + db
                    if f(int(lens[a])) - f(na) + f(int(lens[b])) - f(nb) == r:
                        lens[a], lens[b] = na, nb
                        return True
    return False


def hub_batch(name, in_base=GUARD, big_aligned=True):
    return _hub_batch(name, in_base, big_aligned)


@functools.lru_cache(maxsize=None)
def _hub_lengths(name):
    """Payload lengths of case 4 and where its run of 500 empty texts begins:
    1 x 2 MiB + 15 x 64 KiB + 300 x 0..4 KiB shuffled, the run exactly on a
    span boundary where the shares are T, a run of 20 inside a span."""
    L, sep, trailing, abc = FORMATS[name]
    pad = alpha(abc)[1]

    def f(n):
        return formula(n, pad, L, len(sep), trailing)
    rng = np.random.default_rng(0x4B0B)
    small = rng.integers(0, 4097, 300)
    lens = np.concatenate([[2 << 20], np.full(15, 64 << 10), small]).astype(np.int64)
    rng.shuffle(lens)
    # every text length is a multiple of g: a boundary can stand between two
    # texts only at a multiple of lcm(T, g)
    g = functools.reduce(math.gcd, [f(n) for n in range(1, 400)])
    mod = T * g // math.gcd(T, g)
    c = np.cumsum([f(int(n)) for n in lens])
    i = min(range(100, 200), key=lambda i: (c[i - 1] % mod) if c[i - 1] > 3 * mod else mod)
    assert _land(lens, i, f, mod), name
    lens = np.concatenate([lens[:i], np.zeros(500, np.int64), lens[i:i + 40],
                           np.zeros(20, np.int64), lens[i + 40:]])
    return lens, i


@functools.lru_cache(maxsize=None)
def _hub_batch(name, in_base, big_aligned):
    lens, i = _hub_lengths(name)
    rng = np.random.default_rng(0x4B0C)
    big = int(np.argmax(lens))
    items = [(int(n), 7 * k + 5) for k, n in enumerate(lens)]
    texts = [_text(n, seed, name) for n, seed in items]
    start = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    # the 2 MiB text dword aligned (or not) on the input side
    in_base += (-(in_base + int(start[big])) + (0 if big_aligned else 1)) % 4
    skews = np.where(rng.integers(0, 4, lens.size) == 0, rng.integers(1, 16, lens.size), 0)
    skews[big] = 0
    payloads = [_data(n, seed) for n, seed in items]
    # offences among the small ones, and behind the run of 500 (whose place
    # they must not move) lengths no encoder writes
    for k in range(lens.size):
        if k == big or lens[k] >= 64 << 10:
            continue
        if k % 11 == 3 and len(texts[k]) > 8:
            texts[k] = spoil(texts[k], int(rng.integers(0, len(texts[k]))), 0x2A)
        elif k % 5 == 2 and k > i + 500 and lens[k] > 0:
            texts[k] = next(texts[k] + b"A" * q for q in (1, 2, 3, 4, 5)
                            if _verdict(texts[k] + b"A" * q, name)[0] == LENGTH)
        else:
            continue
        payloads[k] = None
    return Batch(name, texts, payloads, in_base, skews), i


def test_hub_batch_is_what_case_4_asks_for():
    for name in ALL:
        batch, i = hub_batch(name)
        L, sep, trailing, abc = FORMATS[name]
        lens = batch.lens
        assert lens.size == 836
        big = int(np.argmax(lens))
        assert lens[big] >= formula(2 << 20, alpha(abc)[1], L, len(sep), trailing)
        assert (lens >= 64 << 10).sum() == 16
        assert (lens[i:i + 500] == 0).all() and lens[i - 1] > 0 and lens[i + 500] > 0
        assert (lens[i + 540:i + 560] == 0).all() and lens[i + 539] > 0 and lens[i + 560] > 0
        for hint in (0, batch.total, 100 * batch.total):
            assert share(batch.total, BLOCK_WAVES * grid_blocks(hint)) == T
        # the 2 MiB text is spread over many spans under every hint but the smallest
        for hint, least in ((0, 100), (batch.total, 100), (100 * batch.total, 100),
                            (batch.total // 100, 2)):
            S = share(batch.total, BLOCK_WAVES * grid_blocks(hint))
            assert int(lens[big]) // S >= least, (name, hint)
        assert batch.in_off[big] % 4 == 0 and batch.skews[big] == 0
        other, _ = hub_batch(name, big_aligned=False)
        assert other.in_off[big] % 4 == 1
        fast = (batch.in_off[:-1] % 4 == 0) & (batch.skews % 4 == 0) & (lens > 32)
        assert fast.sum() > 50 and ((lens > 32) & ~fast).sum() > 50
        assert (batch.kinds == OK).sum() > 700 and (batch.kinds == LENGTH).sum() > 10
        assert ((batch.kinds != OK) & (batch.kinds != LENGTH)).sum() > 10
        # the run of 500 stands on a span boundary of every hint whose shares
        # are T, the run of 20 inside a span
        assert (int(batch.in_off[i]) - batch.in_base) % T == 0, name
        assert (int(batch.in_off[i + 540]) - batch.in_base) % T != 0, name


# Case 5: offences across spans.
OFFENCE_FORMATS = ["crlf76_trailing", "plain_pad"]
OFFENCE_HINT = 64 << 20
ROLES = ("char", "pad", "sep", "bits", "two_far", "length", "clean", "two_near", "clean", "sep")


@functools.lru_cache(maxsize=None)
def offence_batch(name):
    """About 300 texts of 20,000..50,000 bytes, laid end to end: each holds a
    span boundary under the 64 MiB hint (the shares are T).  By its role a
    text gets one spoilt byte at -24..+24 of a boundary inside it (CHAR, PAD,
    SEP), nonzero unused bits in character D - 1 with the text's end placed
    within 24 bytes of a boundary (BITS), two spoilt bytes on either side of a
    boundary, a length no encoder writes, or nothing.  Returns the batch and,
    per text, (role, the spoilt offsets)."""
    L, sep, trailing, abc = FORMATS[name]
    chars, pad, padc = alpha(abc)
    s = len(sep)
    P = (L or 0) + s
    rng = np.random.default_rng(0x0FFE + len(name))

    def f(n):
        return formula(n, pad, L, s, trailing)

    def is_char(x):
        return L is None or x % P < L

    def char_near(x, W, lo, hi):  # a character position at lo..hi of x, inside the text
        cands = [y for y in range(x + lo, x + hi + 1) if 0 <= y < W and is_char(y)]
        return cands[int(rng.integers(0, len(cands)))]
    texts, payloads, notes = [], [], []
    start = 0
    for i in range(300):
        role = ROLES[i % len(ROLES)]
        n = int(rng.integers(15200, 36000))
        if role == "bits":  # the text's end within 24 bytes of a boundary, D mod 4 in {2, 3}
            n = int(rng.integers(22000, 30000))
            end = (start + f(n) + T // 2) // T * T + int(rng.integers(-24, 25))
            n0 = (end - start) * 3 // 4 if L is None else (end - start) * L // P * 3 // 4
            n = min((m for m in range(n0 - 40, n0 + 40) if m % 3),
                    key=lambda m: abs(start + f(m) - end))
        t = _text(n, 100 + i, name)
        W = len(t)
        assert 20000 <= W <= 50000
        bound = (start // T + 1) * T - start  # the first boundary inside the text
        assert 0 < bound < W - 24
        spots = []
        if role == "char":
            spots = [(char_near(bound, W, -24, 24), 0x2A)]
        elif role == "pad":
            spots = [(char_near(bound, W, -24, 24), padc)]
        elif role == "sep":
            near = [x for x in range(max(bound - 24, 0), bound + 25) if not is_char(x)]
            if near:
                spots = [(near[int(rng.integers(0, len(near)))], 0x41)]
            else:
                spots = [(char_near(bound, W, -24, 24), 0x7E)]
        elif role == "bits":
            E = text_chars(W, L, s, trailing)[0]
            D = E - (3 - n % 3 if pad else 0)
            at = char_off(D - 1, L, s)
            v = chars.index(bytes([t[at]]))
            spots = [(at, chars[v | 1])]
        elif role in ("two_far", "two_near"):
            lo = char_near(bound, W, -24, -1)
            hi = char_near(bound, W, 19, 24) if role == "two_far" else char_near(bound, W, 0, 12)
            spots = [(lo, 0x2A if i % 4 else padc), (hi, padc if i % 4 else 0x2A)]
        elif role == "length":
            t = next(t + b"A" * k for k in (1, 2, 3) if _verdict(t + b"A" * k, name)[0] == LENGTH)
        for at, byte in spots:
            t = spoil(t, at, byte)
        texts.append(t)
        payloads.append(_data(n, 100 + i) if role == "clean" else None)
        notes.append((role, sorted(at for at, _ in spots)))
        start += len(t)
    return Batch(name, texts, payloads), notes


def test_offence_batch_is_what_case_5_asks_for():
    count = {k: 0 for k in (CHAR, SEP, PAD, BITS, LENGTH)}
    apart = clean = 0
    for name in OFFENCE_FORMATS:
        L, sep, trailing, abc = FORMATS[name]
        s = len(sep)
        batch, notes = offence_batch(name)
        assert share(batch.total, BLOCK_WAVES * grid_blocks(OFFENCE_HINT)) == T
        start = batch.in_off - batch.in_base

        def owner(i, x):
            """The span that checks byte x of text i: the one that holds the
            first character of the lane of the character at x (or before it)."""
            e = chars_below(x + 1, L, s) - 1
            return (int(start[i]) + char_off(e // 16 * 16, L, s)) // T
        for i, (role, spots) in enumerate(notes):
            W = int(batch.lens[i])
            assert 20000 <= W <= 50004
            assert int(start[i]) // T < (int(start[i]) + W - 1) // T, "a boundary inside"
            kind, pos, out_len = (int(v) for v in batch.recs[i][[2, 1, 0]])
            if role == "clean":
                assert kind == OK and out_len > 0
                clean += 1
                continue
            assert kind != OK and out_len == 0, (name, i, role)
            if role == "length":
                assert (kind, pos) == (LENGTH, W)
            else:
                assert pos == spots[0], (name, i, role)  # the lower one
                near = max(min(abs(int(start[i]) + x - b) for b in range(T, batch.total, T))
                           for x in spots)
                if role == "bits":  # at character D - 1, wherever that is
                    assert kind == BITS and spots[0] >= W - 3 - 2 * s
                else:
                    assert near <= 24, (name, i, role, near)
                if len(spots) == 2:
                    assert spots[0] < spots[1]
                    apart += owner(i, spots[0]) != owner(i, spots[1])
            if len(spots) < 2:
                count[kind] += 1
    assert all(v >= 20 for v in count.values()), count
    assert apart >= 40 and clean >= 100, (apart, clean)


# ------------------------------------------------------------------- GPU --

@gpu
@pytest.mark.parametrize("name", ALL)
def test_one_text_every_short_length(name):
    """Case 1: payload lengths 0..200, a call each: every tail, pad and
    short-line shape; the even lengths at an odd output offset.  Every fourth
    length also with one byte spoilt and with one byte appended."""
    rng = np.random.default_rng(5)
    for n in range(201):
        skews = [0 if n % 2 else 5]
        run_wide(valid_batch(name, [(n, 5 * n + 2)], skews=skews), existing=n % 8 == 0)
        if n % 4 == 1:
            t = _text(n, 5 * n + 2, name)
            run_wide(Batch(name, [spoil(t, int(rng.integers(0, len(t))), 0x2A)], skews=skews))
            run_wide(Batch(name, [t + b"\n"], skews=skews), existing=n % 8 == 1)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_one_text_at_share_and_line_edges(name):
    """Case 2."""
    for n in edge_payloads(name):
        for k, (in_skew, out_skew) in enumerate(PLACEMENTS):
            batch = valid_batch(name, [(n, n)], in_base=GUARD + in_skew, skews=[out_skew])
            run_wide(batch, hint=None if k % 2 else 0, existing=k == 0)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_sliding_cuts(name):
    """Case 3: each of the 48 leading lengths moves every span boundary
    through the texts behind it."""
    for lead in range(48):
        for hint in SLIDE_HINTS:
            run_wide(sliding_batch(name, lead), hint=hint, existing=lead % 16 == 5)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_hub_like_batch(name):
    """Case 4, against the references and the existing ragged call, the 2 MiB
    text on the fast path and on the bytewise one."""
    for big_aligned in (True, False):
        batch, _ = hub_batch(name, big_aligned=big_aligned)
        run_wide(batch, existing=True)


@gpu
@pytest.mark.parametrize("name", OFFENCE_FORMATS)
def test_offences_across_spans(name):
    """Case 5: the lowest offence of a text, whichever wave saw it."""
    batch, _ = offence_batch(name)
    run_wide(batch, hint=OFFENCE_HINT, existing=True)
    run_wide(batch, hint=0)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_any_hint_gives_the_same_records_and_bytes(name):
    """Case 6."""
    batch, _ = hub_batch(name)
    for hint in (0, batch.total, batch.total // 100, 100 * batch.total):
        run_wide(batch, hint=hint)
    far, _ = hub_batch(name, in_base=4099)
    assert far.in_off[0] in range(4099, 4103) and (far.data[:4099] == FILL).all()
    for hint in (0, far.total):
        run_wide(far, hint=hint)


@gpu
@pytest.mark.parametrize("name", ["plain_pad", "crlf76_trailing"])
def test_graph_replay_on_other_texts(name):
    """Case 7: one capture on fixed tensors with total_hint = the arena's
    capacity; each replay runs on other offsets, contents and offences written
    into those tensors: once a single text holds the whole arena, once a
    refused text stands where an accepted one stood (and the other way)."""
    from async_amd import b64
    L, sep, trailing, abc = FORMATS[name]
    s = len(sep)
    nbuf, top = 300, 900
    in_cap = nbuf * formula(top, True, L, s, trailing)
    out_cap = in_cap + nbuf * (GUARD + 32) + GUARD
    x = torch.full((GUARD + in_cap + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    in_off = torch.full((nbuf + 1,), GUARD, dtype=torch.int64, device=DEV)
    out_off = torch.full((nbuf,), GUARD, dtype=torch.int64, device=DEV)
    out = torch.full((out_cap,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device=DEV)

    def call():
        b64.decode_strict_batch_wide(x, in_off, out, out_off, res, L, sep, trailing,
                                     total_hint=in_cap, abc=abc)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()  # warm-up outside the capture (all lengths zero)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call()
    rng = np.random.default_rng(8)
    lens = rng.integers(0, top + 1, nbuf)
    lens[rng.choice(nbuf, 40, replace=False)] = 0
    lens[rng.choice(nbuf, 3, replace=False)] = (top, 1, 57)
    spoilt = set(int(i) for i in rng.choice(nbuf, 30, replace=False))
    seen = []
    for rep in range(3):
        if rep == 1:  # one text holds the whole arena
            n = next(n for n in range(in_cap, 0, -1) if formula(n, True, L, s, trailing) <= in_cap)
            items = [(0, i) for i in range(nbuf)]
            items[137] = (n, 977)
            texts = [_text(n, seed, name) for n, seed in items]
        else:
            items = [(int(n), i) for i, n in enumerate(lens)]
            texts = [_text(n, seed, name) for n, seed in items]
            for i in range(nbuf):
                # replay 2: refused where replay 0 accepted, and the other way
                if (i in spoilt) == (rep == 0) and len(texts[i]) > 4:
                    texts[i] = spoil(texts[i], len(texts[i]) * (i % 7) // 7, 0x2A) if i % 3 \
                        else texts[i] + b"\r"
        batch = Batch(name, texts, skews=rng.integers(0, 4, nbuf) * (rng.integers(0, 3, nbuf) == 0))
        seen.append(batch.kinds)
        assert batch.data.size <= x.numel() and batch.expect.size <= out_cap
        x.fill_(FILL)
        x[:batch.data.size].copy_(torch.from_numpy(batch.data))
        in_off.copy_(torch.from_numpy(batch.in_off))
        out_off.copy_(torch.from_numpy(batch.out_off))
        out.fill_(FILL)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert (out[batch.expect.size:] == FILL).all(), rep
        _check(batch, out[:batch.expect.size], res, f"replay {rep}")
    assert ((seen[0] == OK) & (seen[2] != OK)).sum() >= 15
    assert ((seen[0] != OK) & (seen[2] == OK)).sum() >= 15
    assert (seen[1] == OK).all()


@gpu
def test_wrapper_refuses_wrong_tensors():
    """Case 8."""
    from async_amd import b64
    batch = valid_batch("crlf76_trailing", [(100, 1), (50, 2)])
    x, in_off, out_off = _dev(batch.data), _dev(batch.in_off), _dev(batch.out_off)
    out = torch.full((batch.expect.size,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((REC * 2 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    b64.decode_strict_batch_wide(x, in_off, out, out_off, res, 76)
    _check(batch, out, res, "two texts")
    bad = [dict(x=x.to(torch.int8)), dict(out=out.to(torch.int32)), dict(x=x.cpu()),
           dict(in_off=in_off.to(torch.int32)), dict(out_off=out_off.to(torch.int32)),
           dict(out_off=out_off.to(torch.float64)), dict(in_off=in_off.cpu()),
           dict(out_off=out_off[:1]), dict(result=res[:47]), dict(result=res.to(torch.int8)),
           dict(result=res.cpu()), dict(total_hint=-1)]
    for kw in bad:
        args = dict(x=x, in_off=in_off, out=out, out_off=out_off, result=res)
        hint = kw.pop("total_hint", None)
        args.update(kw)
        for line_len in (None, 76):
            with pytest.raises(ValueError):
                b64.decode_strict_batch_wide(args["x"], args["in_off"], args["out"],
                                             args["out_off"], args["result"], line_len,
                                             total_hint=hint)
    with pytest.raises(ValueError):
        b64.decode_strict_batch_wide(x, in_off, out, out_off, res, 76, b"")
    with pytest.raises(b64.B64xError):  # the library's -EINVAL
        b64.decode_strict_batch_wide(x, in_off, out, out_off, res, 75)
    with pytest.raises(b64.B64xError):
        b64.decode_strict_batch_wide(x, in_off, out, out_off, res, abc=("-", "-", True, -1))
    # an empty batch and an empty arena are calls like any other
    none = torch.zeros(1, dtype=torch.int64, device=DEV)
    b64.decode_strict_batch_wide(x[:0], none, out, none[:0], res[:0])
    torch.cuda.synchronize()
    _check(batch, out, res, "after the empty batch")
    zeros = torch.full((4,), GUARD, dtype=torch.int64, device=DEV)
    res3 = torch.full((REC * 3 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    for hint in (0, None):
        b64.decode_strict_batch_wide(x, zeros, out, zeros[:3], res3, 76, total_hint=hint)
        torch.cuda.synchronize()
        assert not _records(res3, 3).any()  # {0, 0, OK} three times
    assert np.array_equal(out.cpu().numpy(), batch.expect)
