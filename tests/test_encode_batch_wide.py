"""The ragged encode balanced over the batch's bytes (b64x_encode_batch_wide,
async_amd.b64.encode_batch_wide): plain and line-wrapped, buffers of any size
in one call.

Expected bytes come from the stdlib (tests/test_decode_strict.py's ref_text:
base64.b64encode, the alphabet translated, the pads stripped, wrapped in
Python) and, on the GPU, from the existing ragged calls (encode_batch /
encode_lines_batch) on the same tensors.  The new call is never compared with
itself.  Every comparison is exact.

CPU tests: the plan (async_amd/csrc/b64x_encode_wide_plan.h) built as a host
program under ASan + UBSan and checked against the same rules restated here
in Python -- the grid, the shares, the spans, and that the block ranges owned
over any set of span boundaries partition a buffer's blocks exactly; the
argument checks in order through the C ABI; the exports; the new code
object's kernels and barriers; conditions on the GPU tests' own inputs.

GPU tests: every output stands between 64-byte guards of 0xA5 and the arena
is compared whole; the input arena has guard bytes before and after it in the
same tensor."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from async_amd import _lib
from tests import util
from tests.test_decode_strict import STD, enc_len, formula, ref_text

ROOT = util.ROOT
GUARD = 64
FILL = 0xA5
URL_NOPAD = ("-", "_", False, -1)

# name -> (L, sep, trailing, abc); L None: plain
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

# The constants of b64x_encode_wide_plan.h, restated (test_plan_constants
# reads them back from the program).
T = 12288          # input bytes a wave takes at least
UNIT = 48          # shares are multiples of it
BLOCK_WAVES = 4
BLOCKS_PER_CU = 8
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


def char_off(e, L, s):
    return e if L is None else e // L * (L + s) + e % L


def call_fast(L, s):
    """The call-level rule of the wrapped form (lines_plan::make_call)."""
    if L is None:
        return True
    d = L + s
    if L < 16 or d > 1 << 24:
        return False
    err = (0xFFFFFFFF + d) // d * d - (1 << 32)
    return (d + 4096) * err < 1 << 32


def blocks_hot(n, L, s, trailing, pad, aligned):
    """(B, hot_blocks) of a buffer of n bytes."""
    W = formula(n, pad, L, s, trailing)
    fast = aligned and call_fast(L, s)
    if L is None:
        hot = (n - 16) // 12 + 1 if fast and n >= 16 else 0
    else:
        hot = char_off((n - 17) // 3 * 4, L, s) // 16 if fast and n >= 17 else 0
    return -(-W // 16), hot


def cut(x, n, B, L, s):
    if x == 0:
        return 0
    if x >= n:
        return B
    return min(B, -(-char_off(4 * -(-x // 3), L, s) // 16))


def boundaries(total, hint, cus=CUS):
    """The arena positions at which one wave's span ends and the next one's
    begins."""
    waves = BLOCK_WAVES * grid_blocks(hint, cus)
    S = share(total, waves)
    return list(range(S, total, S))


# ------------------------------------------------------------------- CPU --

@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/encode_wide_plan_check.cpp built with the host compiler
    under ASan + UBSan: a stand-alone program, run as a child process, the
    sanitizers' runtimes linked into the program itself."""
    exe = str(tmp_path_factory.mktemp("plan") / "encode_wide_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "encode_wide_plan_check.cpp"), "-o", exe],
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
    assert _ask(plan_program, ["K"]) == [(T, UNIT, BLOCK_WAVES, BLOCKS_PER_CU)]
    assert T % UNIT == 0 and UNIT % 12 == 0


TOTALS = sorted({0, 1, 47, 48, 49, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 100003,
                 31 << 20, (600 << 20) + 5}
                | {(1 << 32) + d for d in (-1, 0, 1)} | {(1 << 63) + d for d in (-1, 0, 1)}
                | {(1 << 64) - d for d in (1, 2, 47, 48, 49, 8192 * 48, 8192 * 48 + 1)})
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


PLAN_FORMATS = [(None, 0, True, True), (None, 0, True, False), (76, 2, True, True),
                (76, 2, False, True), (64, 1, True, True), (16, 4, True, True),
                (16, 4, False, False)]


def plan_lengths(L):
    ns = set(range(301))
    ns |= {k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)}
    if L is not None:
        ns |= {k * 3 * L // 4 + d for k in (1, 2, 3, 100) for d in (-1, 0, 1, 2, 3)}
    ns |= {(1 << 32) + d for d in range(-3, 4)} | {3 * (1 << 30) + 7, (1 << 40) + 5}
    ns |= {(1 << 63) - d for d in range(1, 8)}
    return sorted(ns)


def test_owned_blocks_partition_every_buffer(plan_program):
    rng = np.random.default_rng(0xE4C)
    cases = []
    for L, s, trailing, pad in PLAN_FORMATS:
        for n in plan_lengths(L):
            for aligned in (0, 1):
                if n <= 300:  # a boundary at every byte, and past the end
                    xs = list(range(n + 3))
                else:
                    near = [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)]
                    xs = sorted({0, 1, 2, 3, n - 2, n - 1, n, n + 1, n + T}
                                | {x for x in near if x < n}
                                | {int(x) for x in rng.integers(1, n, 40, dtype=np.uint64)})
                cases.append((L, s, trailing, pad, aligned, n, xs))
    got = _ask(plan_program, [f"U {L or 0} {s} {int(t)} {int(p)} {al} {n} " + " ".join(map(str, xs))
                              for L, s, t, p, al, n, xs in cases])
    hot_seen = 0
    for (L, s, trailing, pad, aligned, n, xs), row in zip(cases, got):
        key = (L, s, trailing, pad, aligned, n)
        B, hot = blocks_hot(n, L, s, trailing, pad, bool(aligned))
        assert row[:2] == (B, hot), (key, row[:2], (B, hot))
        cuts = row[2:]
        assert list(cuts) == [cut(x, n, B, L, s) for x in xs], key
        # spans [xs[i], xs[i + 1]) of the buffer: ranges end to end from 0 to B
        assert cuts[0] == 0 and cuts[-1] == B, key
        assert all(a <= b for a, b in zip(cuts, cuts[1:])), key
        # a hot block lies inside the text and its loads inside the buffer
        assert hot <= B and (hot == 0 or aligned)
        if hot and L is None:
            assert 12 * (hot - 1) + 16 <= n < 12 * hot + 16
            assert 16 * hot <= enc_len(n, pad)
        hot_seen += hot > 0
    assert hot_seen > 500
    # a block's owner holds the bytes it is made of, or lies within a block of them
    for L, s, trailing, pad in PLAN_FORMATS:
        for n in (100, 5000):
            B, _ = blocks_hot(n, L, s, trailing, pad, False)
            for x in range(1, n):
                j = cut(x, n, B, L, s)
                if j < B:
                    assert 16 * j >= char_off(4 * (x // 3), L, s) - 3, (L, n, x)


def _raw(L, s, sep, flags):
    return _lib.Lines(L, s, (ctypes.c_uint8 * 4)(*sep), flags)


BAD_FORMATS = [(6, 2, b"\r\n", 1), (0, 2, b"\r\n", 1), (76, 5, b"\r\n\r\n", 1), (76, 0, b"", 1),
               (76, 1, b"A", 1), (76, 2, b"\n/", 0), (76, 2, b"\r\n", 2),
               (76, 2, b"\r\n", 0x80000001)]


def test_invalid_arguments_in_order():
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    ok = _lib.lines(76, b"\r\n", True)
    nodev = lib.b64x_device_check() == -19

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def enc(fmt=ok, abc=a, nbuf=3, hint=0, d_in=p, in_off=p, d_out=p, out_off=p):
        return lib.b64x_encode_batch_wide(d_in, in_off, nbuf, hint, d_out, out_off, ref(abc),
                                          ref(fmt), None)

    # 1. nbuf == 0 returns 0 whatever else is wrong
    bad_fmt = _raw(75, 9, b"AAAA", 6)
    assert enc(nbuf=0, d_in=None, in_off=None, d_out=None, out_off=None, fmt=None) == 0
    assert enc(nbuf=0, fmt=bad_fmt) == 0
    # 2. NULL pointers, before the format is looked at
    for k in ("d_in", "in_off", "d_out", "out_off"):
        assert enc(**{k: None}) == -22, k
        assert enc(fmt=None, **{k: None}) == -22, k
        assert enc(fmt=bad_fmt, **{k: None}) == -22, k
    # 3. with fmt, the format rules of b64x_encode_lines_dev
    for L, s, sep, flags in BAD_FORMATS:
        f = _raw(L, s, sep, flags)
        for hint in (0, 1 << 20):
            assert enc(fmt=f, hint=hint) == -22, (L, s, sep, flags)
        assert lib.b64x_encode_lines_dev(p, 30, p, ref(a), ref(f), None) == -22
    url = _lib.alphabet("-", "_")
    assert enc(fmt=_raw(76, 1, b"-", 1), abc=url) == -22
    # 4. valid calls stop at the device check
    if nodev:
        for hint in (0, 1, 1 << 20, (1 << 64) - 1):
            assert enc(hint=hint) == -19
            assert enc(fmt=None, hint=hint) == -19
        assert enc(fmt=None, abc=None) == -19
        assert enc(fmt=_raw(76, 1, b"+", 1), abc=url) == -19
        assert enc(fmt=_raw(4, 1, b"\n", 0)) == -19
        assert enc(abc=_lib.alphabet("-", "-")) == -19  # the encoder has no alphabet rules
        assert enc(nbuf=(1 << 32) - 1) == -19


def test_symbol_exported_by_all_three_libraries():
    name = "b64x_encode_batch_wide"
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "async_amd", "libasync_b64_core.so"),
                 os.path.join(ROOT, "tests", "csrc", "libb64x_hooks.so")):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                             check=True).stdout
        assert re.search(rf"\bT {name}$", out, re.M), path
    lib = _lib.load()
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 9
    assert getattr(lib, name).restype is ctypes.c_int
    assert "abi=7" in lib.b64x_build_info().decode()
    with open(os.path.join(ROOT, "include", "b64x.h")) as f:
        assert re.search(rf"^int {name}\(", f.read(), re.M)
    from async_amd import b64
    assert callable(b64.encode_batch_wide) and "encode_batch_wide" in b64.__doc__


WIDE_KERNELS = {"k_encode_wide<false>", "k_encode_wide<true>"}


def test_wide_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_encode_wide.o"))
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
    assert isa_check.barrier_count(dis) == 2  # one per kernel, after its tables
    main = isa_check.kernel_symbols(isa_check.disassemble(_lib.LIB_PATH))
    assert not any("encode_wide" in n for n in main)


# ------------------------------------------------- the GPU tests' batches --

def _data(n, seed):
    return util.splitmix64(seed, n).tobytes()


class Batch:
    """Payloads and where they stand: the input arena from byte in_base of its
    tensor, buffers end to end; output i at a 16-byte boundary plus skew[i],
    GUARD bytes or more of FILL before and after it."""

    def __init__(self, payloads, in_base=GUARD, skews=None):
        self.payloads = payloads
        self.lens = np.array([len(p) for p in payloads], np.int64)
        self.in_base = in_base
        self.in_off = in_base + np.concatenate([[0], np.cumsum(self.lens)])
        self.total = int(self.lens.sum())
        self.skews = np.zeros(len(payloads), np.int64) if skews is None else np.asarray(skews)
        data = np.full(in_base + self.total + GUARD, FILL, np.uint8)
        data[in_base:in_base + self.total] = np.frombuffer(b"".join(payloads), np.uint8)
        self.data = data

    @functools.lru_cache(maxsize=None)
    def texts(self, name):
        L, sep, trailing, abc = FORMATS[name]
        return [ref_text(p, L, sep, trailing, abc) for p in self.payloads]

    @functools.lru_cache(maxsize=None)
    def layout(self, name):
        """(out_off, the expected arena)."""
        texts = self.texts(name)
        off = np.zeros(len(texts), np.int64)
        pos = GUARD
        for i, t in enumerate(texts):
            off[i] = -(-pos // 16) * 16 + self.skews[i]
            pos = off[i] + len(t) + GUARD
        expect = np.full(pos, FILL, np.uint8)
        for o, t in zip(off, texts):
            expect[o:o + len(t)] = np.frombuffer(t, np.uint8)
        return off, expect


gpu = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _first_bad(got, expect, off):
    bad = np.flatnonzero(got != expect)
    i = int(np.searchsorted(off, bad[0], side="right")) - 1
    return (f"{bad.size} bytes differ, the first at {bad[0]} of the arena "
            f"(buffer {i} starts at {off[max(i, 0)]})")


def run_wide(batch, name, hint=None, existing=False):
    """One encode_batch_wide over the batch: the whole output arena against
    the stdlib's texts and, with `existing`, against the existing ragged call
    on the same tensors."""
    from async_amd import b64
    L, sep, trailing, abc = FORMATS[name]
    off, expect = batch.layout(name)
    x, d_in_off, d_out_off = _dev(batch.data), _dev(batch.in_off), _dev(off)
    out = torch.full((expect.size,), FILL, dtype=torch.uint8, device=DEV)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    b64.encode_batch_wide(x, d_in_off, out, d_out_off, L, sep, trailing, total_hint=hint, abc=abc)
    got = out.cpu().numpy()
    if not np.array_equal(got, expect):
        pytest.fail(f"{name} hint={hint}: " + _first_bad(got, expect, off))
    assert np.array_equal(x.cpu().numpy(), batch.data), "the input was written"
    if existing:
        old = torch.full((expect.size,), FILL, dtype=torch.uint8, device=DEV)
        if L is None:
            b64.encode_batch(x, d_in_off, old, d_out_off, abc=abc)
        else:
            b64.encode_lines_batch(x, d_in_off, old, d_out_off, L, sep, trailing, abc=abc)
        assert torch.equal(old, out), f"{name}: differs from the existing ragged call"


# Case 2: one buffer at the share's edges and the line's.
EDGE_LENGTHS = sorted({k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)}
                      | {57 * k + d for k in (1, 2, 3, 215, 216, 431) for d in (-1, 1)})
PLACEMENTS = [(0, 0), (1, 0), (0, 3), (2, 1), (3, 2)]  # (input, output) offsets off a dword


def sliding_lengths():
    """Case 3 without its leading buffer: 100,003 bytes, then 40 buffers of
    1..3,000 bytes, one of them ending 10,560 bytes into the small ones: with
    shares of T the ninth boundary (arena byte 9 T = 110,592) then stands on
    a buffer's first byte when the leading buffer has 29 bytes and on a
    buffer's last byte when it has 30."""
    rng = np.random.default_rng(0x511D)
    small = rng.integers(1, 3001, 40)
    c = np.cumsum(small)
    i = int(np.searchsorted(c, 9 * T - 100003 - 29))
    small[i] -= c[i] - (9 * T - 100003 - 29)
    assert 1 <= small[i] <= 3000
    return [100003] + [int(n) for n in small]


SLIDE_HINTS = (T, 64 << 20)  # one block: shares of a quarter of the arena; shares of T


@functools.lru_cache(maxsize=None)
def sliding_batch(lead):
    lens = [lead] + sliding_lengths()
    return Batch([_data(n, 3 * i + 1) if i else _data(n, 1000 + lead) for i, n in enumerate(lens)])


def test_sliding_cuts_reach_every_kind_of_boundary():
    """Conditions on case 3's inputs alone, from the model: over the 48
    leading lengths and the two hints a span boundary stands in mid-group, in
    a separator of the text, and on a buffer's first and last byte; with
    total_hint = T the grid is one block whose four waves take a quarter of
    the arena each, with 64 MiB the shares are T."""
    seen = set()
    for lead in range(48):
        lens = np.array([lead] + sliding_lengths())
        start = np.concatenate([[0], np.cumsum(lens)])
        total = int(start[-1])
        for hint in SLIDE_HINTS:
            waves = BLOCK_WAVES * grid_blocks(hint)
            S = share(total, waves)
            if hint == T:
                assert waves == 4 and S > 2 * T and 3 * S < total
            else:
                assert S == T and waves * T > total
            for at in boundaries(total, hint):
                i = int(np.searchsorted(start, at, side="right")) - 1
                x, n = at - int(start[i]), int(lens[i])
                seen.add("first" if x == 0 else "last" if x == n - 1 else "inside")
                if x % 3:
                    seen.add("mid-group")
                B, _ = blocks_hot(n, 76, 2, True, True, False)
                j = cut(x, n, B, 76, 2)
                if 0 < j < B and 16 * j % 78 >= 76:
                    seen.add("separator")
                if 0 < j < B and 16 * j % 78 < 76 and (16 * j % 78) % 4:
                    seen.add("mid-quad")
    assert seen == {"first", "last", "inside", "mid-group", "separator", "mid-quad"}, seen


def hub_batch(in_base=GUARD, big_aligned=True):
    return _hub_batch(in_base, big_aligned)


@functools.lru_cache(maxsize=None)
def _hub_batch(in_base, big_aligned):
    """Case 4: 1 x 2 MiB + 15 x 64 KiB + 300 x 0..4 KiB shuffled, a run of 500
    empty buffers that stands exactly on a span boundary where the shares are T
    (and inside a span under a small hint), a run of 20 inside a span,
    and outputs at odd offsets mixed with aligned ones."""
    rng = np.random.default_rng(0x4B0B)
    small = rng.integers(0, 4097, 300)
    small[::2] &= ~3  # half of them keep the input's alignment
    lens = np.concatenate([[2 << 20], np.full(15, 64 << 10), small])
    rng.shuffle(lens)
    total = int(lens.sum())
    S = share(total, BLOCK_WAVES * grid_blocks(total))
    c = np.cumsum(lens)
    # end buffer i - 1 on a boundary: shorten it, and lengthen the last buffer by as much
    i = next(i for i in range(100, 300)
             if 0 < c[i - 1] % S < lens[i - 1] and lens[i - 1] <= 4096)
    r = int(c[i - 1] % S)
    lens[i - 1] -= r
    lens[-1] += r
    lens = np.concatenate([lens[:i], np.zeros(500, np.int64), lens[i:i + 40],
                           np.zeros(20, np.int64), lens[i + 40:]])
    big = int(np.argmax(lens))
    start = np.concatenate([[0], np.cumsum(lens)])
    # the 2 MiB buffer dword aligned (or not) on the input side
    in_base += (-(in_base + int(start[big])) + (0 if big_aligned else 1)) % 4
    skews = np.where(rng.integers(0, 4, lens.size) == 0, rng.integers(1, 16, lens.size), 0)
    skews[big] = 0
    payloads = [_data(int(n), 7 * k + 5) for k, n in enumerate(lens)]
    return Batch(payloads, in_base, skews), i


def test_hub_batch_is_what_case_4_asks_for():
    batch, i = hub_batch()
    lens = batch.lens
    assert lens.size == 836 and batch.total < 4 << 20
    assert (lens == 2 << 20).sum() == 1 and (lens == 64 << 10).sum() >= 14
    assert (lens[i:i + 500] == 0).all() and lens[i - 1] > 0 and lens[i + 500] > 0
    at = int(batch.in_off[i]) - batch.in_base
    # on a boundary where the shares are T, inside a span of the smallest hint's
    for hint in (0, batch.total, 100 * batch.total):
        assert at % T == 0 and at in boundaries(batch.total, hint)
    assert at not in boundaries(batch.total, batch.total // 100)
    # the run of 20: inside a span under every hint
    assert (lens[i + 540:i + 560] == 0).all() and lens[i + 539] > 0 and lens[i + 560] > 0
    at = int(batch.in_off[i + 540]) - batch.in_base
    for hint in (0, batch.total, batch.total // 100, 100 * batch.total):
        assert at not in boundaries(batch.total, hint)
    big = int(np.argmax(lens))
    assert batch.in_off[big] % 4 == 0 and batch.skews[big] == 0
    other, _ = hub_batch(big_aligned=False)
    assert other.in_off[big] % 4 == 1
    fast = (batch.in_off[:-1] % 4 == 0) & (batch.skews % 4 == 0) & (lens > 16)
    assert fast.sum() > 50 and ((lens > 16) & ~fast).sum() > 50
    # the 2 MiB buffer is spread over many spans under every hint but the smallest
    for hint, least in ((0, 100), (batch.total, 100), (100 * batch.total, 100),
                        (batch.total // 100, 2)):
        S = share(batch.total, BLOCK_WAVES * grid_blocks(hint))
        assert (2 << 20) // S >= least, hint


# ------------------------------------------------------------------- GPU --

@gpu
@pytest.mark.parametrize("name", ALL)
def test_one_buffer_every_short_length(name):
    """Case 1: lengths 0..200, a call each: every tail, pad and short-line
    shape; the even lengths at an odd output offset."""
    for n in range(201):
        run_wide(Batch([_data(n, 5 * n + 2)], skews=[0 if n % 2 else 5]), name,
                 existing=n % 8 == 0)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_one_buffer_at_share_and_line_edges(name):
    """Case 2."""
    for n in EDGE_LENGTHS:
        payload = [_data(n, n)]
        for k, (in_skew, out_skew) in enumerate(PLACEMENTS):
            batch = Batch(payload, GUARD + in_skew, [out_skew])
            run_wide(batch, name, hint=None if k % 2 else 0, existing=k == 0)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_sliding_cuts(name):
    """Case 3: each of the 48 leading lengths moves every span boundary by one
    byte through the buffers behind it."""
    for lead in range(48):
        for hint in SLIDE_HINTS:
            run_wide(sliding_batch(lead), name, hint=hint, existing=lead % 16 == 5)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_hub_like_batch(name):
    """Case 4, against the stdlib and the existing ragged call, the 2 MiB
    buffer on the fast path and on the bytewise one."""
    for big_aligned in (True, False):
        batch, _ = hub_batch(big_aligned=big_aligned)
        run_wide(batch, name, existing=True)


@gpu
@pytest.mark.parametrize("name", ALL)
def test_any_hint_gives_the_same_bytes(name):
    """Case 5."""
    batch, _ = hub_batch()
    for hint in (0, batch.total, batch.total // 100, 100 * batch.total):
        run_wide(batch, name, hint=hint)
    far, _ = hub_batch(in_base=4099)
    assert far.in_off[0] in range(4099, 4103) and (far.data[:4099] == FILL).all()
    for hint in (0, far.total):
        run_wide(far, name, hint=hint)


@gpu
@pytest.mark.parametrize("name", ["plain_pad", "crlf76_trailing"])
def test_graph_replay_on_other_lengths(name):
    """Case 6: one capture on fixed tensors with total_hint = the arena's
    capacity; each replay runs on other offsets and contents written into
    those tensors, once with a single buffer that holds the whole arena."""
    from async_amd import b64
    L, sep, trailing, abc = FORMATS[name]
    nbuf, top = 300, 900
    in_cap = nbuf * top
    out_cap = GUARD + nbuf * (formula(top, True, L, len(sep), trailing) + GUARD + 32)
    out_cap = max(out_cap, formula(in_cap, True, L, len(sep), trailing) + nbuf * (GUARD + 32))
    x = torch.full((GUARD + in_cap + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    in_off = torch.full((nbuf + 1,), GUARD, dtype=torch.int64, device=DEV)
    out_off = torch.full((nbuf,), GUARD, dtype=torch.int64, device=DEV)
    out = torch.full((out_cap,), FILL, dtype=torch.uint8, device=DEV)

    def call():
        b64.encode_batch_wide(x, in_off, out, out_off, L, sep, trailing, total_hint=in_cap, abc=abc)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()  # warm-up outside the capture (all lengths zero)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call()
    rng = np.random.default_rng(8)
    for rep in range(3):
        if rep == 1:  # one buffer holds the whole arena
            lens = np.zeros(nbuf, np.int64)
            lens[137] = in_cap
        else:
            lens = rng.integers(0, top + 1, nbuf)
            lens[rng.choice(nbuf, 40, replace=False)] = 0
            lens[rng.choice(nbuf, 3, replace=False)] = (top, 1, 57)
        batch = Batch([_data(int(n), 31 * rep + i) for i, n in enumerate(lens)],
                      skews=rng.integers(0, 4, nbuf) * (rng.integers(0, 3, nbuf) == 0))
        off, expect = batch.layout(name)
        assert batch.data.size <= x.numel() and expect.size <= out_cap
        x[:batch.data.size].copy_(torch.from_numpy(batch.data))
        in_off.copy_(torch.from_numpy(batch.in_off))
        out_off.copy_(torch.from_numpy(off))
        out.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[expect.size:] == FILL).all(), rep
        if not np.array_equal(got[:expect.size], expect):
            pytest.fail(f"replay {rep}: " + _first_bad(got[:expect.size], expect, off))


@gpu
def test_wrapper_refuses_wrong_tensors():
    """Case 7."""
    from async_amd import b64
    batch = Batch([_data(100, 1), _data(50, 2)])
    off, expect = batch.layout("crlf76_trailing")
    x, in_off, out_off = _dev(batch.data), _dev(batch.in_off), _dev(off)
    out = torch.full((expect.size,), FILL, dtype=torch.uint8, device=DEV)
    b64.encode_batch_wide(x, in_off, out, out_off, 76)
    assert np.array_equal(out.cpu().numpy(), expect)
    bad = [dict(x=x.to(torch.int8)), dict(out=out.to(torch.int32)), dict(x=x.cpu()),
           dict(in_off=in_off.to(torch.int32)), dict(out_off=out_off.to(torch.int32)),
           dict(out_off=out_off.to(torch.float64)), dict(in_off=in_off.cpu()),
           dict(out_off=out_off[:1]), dict(total_hint=-1)]
    for kw in bad:
        args = dict(x=x, in_off=in_off, out=out, out_off=out_off)
        hint = kw.pop("total_hint", None)
        args.update(kw)
        for line_len in (None, 76):
            with pytest.raises(ValueError):
                b64.encode_batch_wide(args["x"], args["in_off"], args["out"], args["out_off"],
                                      line_len, total_hint=hint)
    with pytest.raises(ValueError):
        b64.encode_batch_wide(x, in_off, out, out_off, 76, b"")
    with pytest.raises(b64.B64xError):  # the library's -EINVAL
        b64.encode_batch_wide(x, in_off, out, out_off, 75)
    # an empty batch and an empty arena are calls like any other
    none = torch.zeros(1, dtype=torch.int64, device=DEV)
    b64.encode_batch_wide(x[:0], none, out, none[:0])
    zeros = torch.full((4,), GUARD, dtype=torch.int64, device=DEV)
    b64.encode_batch_wide(x, zeros, out, zeros[:3], 76, total_hint=0)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), expect)
