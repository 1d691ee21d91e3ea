"""Ragged batches of the line-wrapped encode and the strict decode
(b64x_encode_lines_batch / b64x_decode_strict_batch, async_amd.b64
encode_lines_batch / decode_strict_batch and their layout helpers).

Expected bytes and records come from the stdlib and the Python references of
tests/test_decode_strict.py (ref_text, strict_ref, np_ref), never from the
library.

CPU tests: symbols, every -EINVAL case in order, -ENODEV without a device, the
layout helpers against b64x_encoded_lines_len / b64x_strict_decoded_cap, the
kernels' per-buffer arithmetic (async_amd/csrc/b64x_lines_plan.h) built as a
host program under ASan + UBSan and checked field by field against formulas
written here, and the new code object's kernel list and barriers.

GPU tests: every output arena is pre-filled with a sentinel byte, with gaps of
0-7 sentinel bytes after each buffer's range (or none: packed tight), and is
compared whole, so a 16-byte store that runs past a buffer is seen wherever it
lands; record arrays are pre-filled with 0xA5 and have a guard behind them."""
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
from tests.test_decode_strict import (BITS, CHAR, LENGTH, NOPAD, OK, PAD, REC, SEP, STD, _layout,
                                      enc_len, formula, np_ref, records, ref_text, strict_cap,
                                      strict_ref, text_chars)
from tests.test_ragged_batch import NBUF

ROOT = util.ROOT
SENT = 0x5A   # 'Z': occurs in texts and payloads too; the arena is compared whole
FILL = 0xA5   # records before the call
HIGH = (0xE9, 0xE8, True, 0x80)

CRLF76 = (76, b"\r\n")
LF64 = (64, b"\n")
LONG3 = (60, b"\r\n\n")
SHORT = (4, b"\n")
INEXACT = (200000, b"\n")  # the 32-bit reciprocal of its pitch is not exact: all bytewise
HOT_FORMATS = [CRLF76, LF64, LONG3]

# A wave is the kernels' work unit: 64 lanes, 16 bytes of text (encode) or 16
# characters (decode) each; a 256-lane block holds four.
LANES, BLOCK_LANES = 64, 256
HOT_COUNTS = (0, 1, LANES - 1, LANES, LANES + 1, BLOCK_LANES - 1, BLOCK_LANES, BLOCK_LANES + 1)


# ------------------------------------------- the plan, written out in Python --

def recip_fast(L, s, decode):
    """The call-level rule (the one-buffer kernels' set_reciprocals): L >= 16
    and ceil(2^32 / d) exact for every value below d + 4,096."""
    if L is None:
        return True, 0
    d = L if decode else L + s
    if L < 16 or (not decode and d > 1 << 24):
        return False, 0
    magic = (0xFFFFFFFF + d) // d
    err = magic * d - (1 << 32)
    return d + 4096 < 1 << 32 and (d + 4096) * err < 1 << 32, magic


def char_off(e, L, s):
    return e if L is None else e // L * (L + s) + e % L


def enc_plan(n, L, s, trailing, pad, fast):
    """(E, W, full_lines, last_len, hot_blocks, tail_pieces) of n input bytes:
    hot are the 16-byte blocks wholly below the first character whose group
    does not have 20 readable bytes behind its first byte."""
    E = enc_len(n, pad)
    W = formula(n, pad, L, s, trailing)
    hot = char_off((n - 17) // 3 * 4, L, s) // 16 if fast and n >= 17 else 0
    return E, W, E // L, E % L, hot, -(-(W - 16 * hot) // 16)


def dec_plan(W, L, s, trailing, pad, fast):
    """(E, length_error, hot_lanes, tail_lanes, off_e1, off_e2) of W bytes of
    text: hot are the lanes of 16 characters below character E - 4 whose load
    window (24 bytes from the dword at or below the lane's first byte; plain:
    its 16 bytes) lies inside the text."""
    if W == 0:
        return 0, 0, 0, 0, 0, 0
    E, whole = text_chars(W, L, s, trailing)
    if E is None or (pad and E % 4) or (not pad and E % 4 == 1):
        return whole, 1, 0, 0, 0, 0
    hot = 0
    if fast and E >= 20:
        hot = (E - 4) // 16
        while hot and (char_off(16 * (hot - 1), L, s) & ~3) + (16 if L is None else 24) > W:
            hot -= 1
    e1, e2 = (char_off(E - 1, L, s), char_off(E - 2, L, s)) if E >= 2 else (0, 0)
    return E, 0, hot, -(-E // 16) - hot, e1, e2


def n_with_enc_hot(target, L, s):
    """The smallest n whose aligned buffer has `target` hot blocks (or the
    first that has more, where no n has exactly that many)."""
    n = 0
    while enc_plan(n, L, s, True, True, True)[4] < target:
        n += 1
    return n


def n_with_dec_hot(target, L, s, trailing):
    n = 0
    while dec_plan(formula(n, True, L, s, trailing), L, s, trailing, True, True)[2] < target:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def edge_lengths(L, s, trailing=True):
    """Payload lengths of GPU test 1: 0-20, the 64- and 76-character lines'
    neighbours, a last line of 1-4 characters or exactly full (with and
    without pad: 3L/4 - 1 .. 3L/4 + 3 and twice that), and the lengths that
    give a buffer 0, 1, 63-65 and 255-257 hot blocks (encode) or hot lanes
    (decode), from the plan."""
    ns = set(range(21)) | {47, 48, 49, 56, 57, 58}
    per = 3 * L // 4
    ns |= {per + d for d in range(-1, 4)} | {2 * per + d for d in range(-1, 4)}
    for k in HOT_COUNTS:
        for n in (n_with_enc_hot(k, L, s), n_with_dec_hot(k, L, s, trailing)):
            ns |= {max(n - 1, 0), n, n + 1}
    return tuple(sorted(ns))


def _data(n, seed):
    return util.splitmix64(seed, n).tobytes()


# ------------------------------------------------------------------- CPU --

def test_symbols_exported_and_bound():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    for name in ("b64x_encode_lines_batch", "b64x_decode_strict_batch"):
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(_lib.SIGNATURES["b64x_encode_lines_batch"][1]) == 8
    assert len(_lib.SIGNATURES["b64x_decode_strict_batch"][1]) == 9
    assert "abi=7" in lib.b64x_build_info().decode()
    from async_amd import b64
    for name in ("encode_lines_batch", "decode_strict_batch", "lines_batch_layout",
                 "strict_batch_layout"):
        assert callable(getattr(b64, name))


def _raw(L, s, sep, flags):
    return _lib.Lines(L, s, (ctypes.c_uint8 * 4)(*sep), flags)


BAD_FORMATS = [(0, 2, b"\r\n", 1), (6, 2, b"\r\n", 1), (75, 2, b"\r\n", 1), (2, 1, b"\n", 1),
               (76, 0, b"", 1), (76, 5, b"\r\n\r\n", 1), (76, 2, b"\r\n", 2),
               (76, 2, b"\r\n", 0x80000001), (76, 1, b"A", 1), (76, 2, b"\nz", 1),
               (76, 3, b"\r\n7", 1), (76, 1, b"+", 1), (76, 2, b"\n/", 0)]


def test_invalid_arguments_in_order():
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    a = _lib.alphabet()
    ok = _lib.lines(76, b"\r\n", True)
    nodev = lib.b64x_device_check() == -19

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def enc(fmt=ok, abc=a, nbuf=3, d_in=p, in_off=p, d_out=p, out_off=p):
        return lib.b64x_encode_lines_batch(d_in, in_off, nbuf, d_out, out_off, ref(abc), ref(fmt),
                                           None)

    def dec(fmt=ok, abc=a, nbuf=3, d_in=p, in_off=p, d_out=p, out_off=p, d_res=p):
        return lib.b64x_decode_strict_batch(d_in, in_off, nbuf, d_out, out_off, d_res, ref(abc),
                                            ref(fmt), None)

    # 1. nbuf == 0 returns 0 whatever else is wrong
    bad_fmt = _raw(75, 9, b"AAAA", 6)
    nonsense = _lib.alphabet("A", "A", True, "A")
    assert enc(nbuf=0, d_in=None, in_off=None, d_out=None, out_off=None, fmt=None) == 0
    assert enc(nbuf=0, fmt=bad_fmt) == 0
    assert dec(nbuf=0, d_in=None, in_off=None, d_out=None, out_off=None, d_res=None) == 0
    assert dec(nbuf=0, fmt=bad_fmt, abc=nonsense, d_res=p + 4) == 0
    # 2. NULL pointers (before the format is looked at); a misaligned record array
    for k in ("d_in", "in_off", "d_out", "out_off"):
        assert enc(**{k: None}) == -22, k
        assert enc(fmt=bad_fmt, **{k: None}) == -22, k
        assert dec(**{k: None}) == -22, k
    assert dec(d_res=None) == -22
    assert dec(fmt=None, d_res=None) == -22
    for skew in (1, 2, 4, 7):
        assert dec(d_res=p + skew) == -22, skew
    # 3. the format: b64x_encode_lines_dev's rules; NULL is plain for the decode only
    assert enc(fmt=None) == -22
    for L, s, sep, flags in BAD_FORMATS:
        f = _raw(L, s, sep, flags)
        assert enc(fmt=f) == -22, (L, s, sep, flags)
        assert dec(fmt=f) == -22, (L, s, sep, flags)
        assert lib.b64x_encode_lines_dev(p, 30, p, ref(a), ref(f), None) == -22
    url = _lib.alphabet("-", "_")
    assert enc(fmt=_raw(76, 1, b"-", 1), abc=url) == -22
    assert dec(fmt=_raw(76, 2, b"\n_", 1), abc=url) == -22
    #    then the alphabet (strict only): after the format, before the device
    for abc in (_lib.alphabet("-", "-"), _lib.alphabet("A", "/"), _lib.alphabet("+", "z"),
                _lib.alphabet(padchar="A"), _lib.alphabet(padchar="+"),
                _lib.alphabet("-", "_", True, "_")):
        assert dec(abc=abc) == -22, (abc.pos62, abc.pos63, abc.padchar)
        assert dec(fmt=None, abc=abc) == -22
    # 4. valid calls stop at the device check
    if nodev:
        assert enc() == -19
        assert enc(fmt=_raw(76, 1, b"+", 1), abc=url) == -19
        assert enc(fmt=_raw(76, 1, b"\nA", 1)) == -19  # a byte beyond sep_len is not looked at
        assert enc(abc=_lib.alphabet("-", "-")) == -19  # the encoder has no alphabet rules
        assert enc(fmt=_raw(4, 1, b"\n", 0)) == -19
        assert dec() == -19
        assert dec(fmt=None) == -19
        assert dec(abc=_lib.alphabet(pad=False, padchar="A")) == -19  # no pad: padchar unused
        assert dec(nbuf=1, fmt=_raw(200000, 1, b"\n", 1)) == -19


def test_no_gpu_is_enodev():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    assert lib.b64x_device_check() == -19
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    f = _lib.lines(76, b"\r\n", True)
    assert lib.b64x_encode_lines_batch(p, p, 2, p, p, ctypes.byref(a), ctypes.byref(f), None) == -19
    for fmt in (None, ctypes.byref(f)):
        assert lib.b64x_decode_strict_batch(p, p, 2, p, p, p, ctypes.byref(a), fmt, None) == -19


LAYOUT_LENGTHS = list(range(401)) + [(1 << 32) + d for d in range(-4, 5)]
LAYOUT_FORMATS = [CRLF76, LF64, LONG3, SHORT]


def test_layout_helpers_on_cpu_tensors():
    from async_amd import b64
    lib = _lib.load()
    lens = np.array(LAYOUT_LENGTHS, np.int64)
    in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]))
    for L, sep in LAYOUT_FORMATS:
        for trailing in (False, True):
            f = _lib.lines(L, sep, trailing)
            for align in (1, 4, 16):
                for pad in (False, True):
                    off = b64.lines_batch_layout(in_off, L, sep, trailing, pad=pad, align=align)
                    assert off.dtype == torch.int64 and off.device == in_off.device
                    off = off.numpy()
                    assert off.size == lens.size + 1 and off[0] == 0
                    for i, n in enumerate(LAYOUT_LENGTHS):
                        size = lib.b64x_encoded_lines_len(n, pad, ctypes.byref(f))
                        assert size == formula(n, pad, L, len(sep), trailing)
                        assert off[i] % align == 0
                        assert off[i + 1] - off[i] == -(-size // align) * align, (L, sep, n, pad)
                off = b64.strict_batch_layout(in_off, L, sep, trailing, align=align).numpy()
                assert off.size == lens.size + 1 and off[0] == 0
                for i, n in enumerate(LAYOUT_LENGTHS):
                    cap = lib.b64x_strict_decoded_cap(n, ctypes.byref(f))
                    assert cap == strict_cap(n, L, len(sep), trailing)
                    assert off[i] % align == 0
                    assert off[i + 1] - off[i] == -(-cap // align) * align, (L, sep, trailing, n)
    for align in (1, 4, 16):  # plain texts
        off = b64.strict_batch_layout(in_off, align=align).numpy()
        for i, n in enumerate(LAYOUT_LENGTHS):
            cap = lib.b64x_strict_decoded_cap(n, None)
            assert off[i] % align == 0 and off[i + 1] - off[i] == -(-cap // align) * align
    # an empty batch, and what the helpers refuse
    assert b64.lines_batch_layout(torch.zeros(1, dtype=torch.int64)).tolist() == [0]
    assert b64.strict_batch_layout(torch.zeros(1, dtype=torch.int64), 76).tolist() == [0]
    with pytest.raises(ValueError):
        b64.lines_batch_layout(in_off, 75)
    with pytest.raises(ValueError):
        b64.lines_batch_layout(in_off, 76, b"")
    with pytest.raises(ValueError):
        b64.lines_batch_layout(in_off.to(torch.int32))
    with pytest.raises(ValueError):
        b64.strict_batch_layout(in_off, 76, align=0)


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/lines_batch_plan_check.cpp built with the host compiler
    under ASan + UBSan: a stand-alone program, run as a child process.  The
    sanitizers' runtimes are linked into the program itself, so it runs
    whatever the environment preloads."""
    exe = str(tmp_path_factory.mktemp("plan") / "lines_batch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "lines_batch_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _ask(exe, queries):
    run = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == len(queries)
    return rows


def test_plan_program_matches_the_python_formulas(plan_program):
    formats = LAYOUT_FORMATS + [INEXACT, (None, b"")]
    # the call: what depends on the format alone
    calls = [(L, sep, dec) for L, sep in formats for dec in (0, 1) if L is not None or dec]
    got = _ask(plan_program, [f"C {L or 0} {len(sep)} {dec}" for L, sep, dec in calls])
    fast_of = {}
    for (L, sep, dec), (fast, magic, step_k, step_c) in zip(calls, got):
        want_fast, want_magic = recip_fast(L, len(sep), bool(dec))
        assert bool(fast) == want_fast, (L, sep, dec)
        fast_of[L, sep, dec] = bool(fast)
        if L is None:
            continue
        d = L if dec else L + len(sep)
        assert (step_k, step_c) == divmod(1024, d)
        if fast:  # the multiply-high is the quotient wherever a lane uses it
            assert magic == want_magic
            x = np.arange(d + 1024, dtype=np.uint64)
            assert np.array_equal((x * np.uint64(magic)) >> np.uint64(32), x // np.uint64(d))
    assert fast_of[76, b"\r\n", 0] and fast_of[76, b"\r\n", 1] and fast_of[60, b"\r\n\n", 0]
    assert not fast_of[4, b"\n", 0] and not fast_of[4, b"\n", 1]
    assert not fast_of[200000, b"\n", 0] and not fast_of[200000, b"\n", 1]
    # every buffer: the encode of n bytes, the strict decode of n bytes of text
    cases = [(kind, L, sep, trailing, pad, aligned, n)
             for L, sep in formats for kind in "ED" if L is not None or kind == "D"
             for trailing in ((1,) if L is None else (0, 1)) for pad in (0, 1)
             for aligned in (0, 1) for n in LAYOUT_LENGTHS + [3 * (1 << 30) + 7, (1 << 40) + 5]]
    got = _ask(plan_program, [f"{k} {L or 0} {len(sep)} {t} {p} {al} {n}"
                              for k, L, sep, t, p, al, n in cases])
    hot_seen = {"E": 0, "D": 0}
    for (kind, L, sep, trailing, pad, aligned, n), row in zip(cases, got):
        s = len(sep)
        fast = bool(aligned) and fast_of[L, sep, int(kind == "D")]
        want = (enc_plan if kind == "E" else dec_plan)(n, L, s, bool(trailing), bool(pad), fast)
        assert row == want, ((kind, L, sep, trailing, pad, aligned, n), row, want)
        if kind == "E":
            f = _lib.lines(L, sep, bool(trailing))
            assert row[1] == _lib.load().b64x_encoded_lines_len(n, bool(pad), ctypes.byref(f))
            hot_seen["E"] += row[4] > 0
        else:
            f = None if L is None else _lib.lines(L, sep, bool(trailing))
            cap = _lib.load().b64x_strict_decoded_cap(n, ctypes.byref(f) if f else None)
            assert 3 * -(-row[0] // 4) == cap == strict_cap(n, L, s, bool(trailing))
            hot_seen["D"] += row[2] > 0
            if not row[1] and 2 <= row[0] <= 400:  # the positions, from the layout itself
                off, _, _ = _layout(row[0], L, s, bool(trailing))
                assert (row[4], row[5]) == (off[-1], off[-2])
                for j in range(row[2]):  # a hot lane: below E - 4, its window inside the text
                    assert 16 * j + 16 <= row[0] - 4
                    assert (off[16 * j] & ~3) + (16 if L is None else 24) <= n
        if not fast:
            assert row[4 if kind == "E" else 2] == 0
    assert hot_seen["E"] > 500 and hot_seen["D"] > 500


# The kernels of b64x_lines_batch.hip; nothing else may be in its code object.
BATCH_KERNELS = {"k_encode_lines_batch", "k_decode_strict_batch<false>",
                 "k_decode_strict_batch<true>"}


def test_batch_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_lines_batch.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == BATCH_KERNELS, (got - BATCH_KERNELS, BATCH_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == 3  # one per kernel, after its tables
    # the product's first code object is still the main one (isa_check reads that)
    main = isa_check.kernel_symbols(isa_check.disassemble(_lib.LIB_PATH))
    assert not any("lines_batch" in n or "strict_batch" in n for n in main)


def test_edge_lengths_reach_every_hot_count():
    """Conditions on the GPU tests' inputs alone: the lengths derived from the
    plan do give 0, 1, 63-65 and 255-257 hot elements, on both sides."""
    for L, sep in HOT_FORMATS:
        s = len(sep)
        for trailing in (False, True):
            ns = edge_lengths(L, s, trailing)
            enc_hot = {enc_plan(n, L, s, trailing, True, True)[4] for n in ns}
            dec_hot = {dec_plan(formula(n, True, L, s, trailing), L, s, trailing, True, True)[2]
                       for n in ns}
            assert set(HOT_COUNTS) <= enc_hot, (L, sorted(enc_hot))
            assert set(HOT_COUNTS) <= dec_hot, (L, sorted(dec_hot))
            last = {enc_len(n, pad) % L for n in ns for pad in (True, False)}
            assert {0, 2, 3, 4} <= last
            assert len(ns) < 120 and max(ns) < 4000


# ------------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _b64():
    from async_amd import b64
    return b64


def _offsets(sizes, gaps):
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64) + gaps, out=off[1:])
    return off


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _first_bad(got, expect, mask, off):
    bad = np.flatnonzero((got != expect) & mask)
    i = int(np.searchsorted(off, bad[0], side="right")) - 1
    return f"byte {bad[0]} of the arena (buffer {i}, which starts at {off[min(i, off.size - 1)]})"


def run_encode(payloads, fmt, abc=STD, gaps=None, in_skew=0, out_skew=0):
    """One encode_lines_batch over `payloads` (back to back from byte in_skew
    of the input arena); output i at out_skew + sum of the earlier texts and
    gaps.  The whole output arena against the stdlib's text.  Returns the
    texts."""
    b64 = _b64()
    L, sep, trailing = fmt
    texts = [ref_text(p, L, sep, trailing, abc) for p in payloads]
    n = len(payloads)
    gaps = np.zeros(n, np.int64) if gaps is None else gaps
    in_off = _offsets([len(p) for p in payloads], 0) + in_skew
    out_off = _offsets([len(t) for t in texts], gaps) + out_skew
    data = np.zeros(int(in_off[-1]) + 8, np.uint8)
    data[in_skew:int(in_off[-1])] = np.frombuffer(b"".join(payloads), np.uint8)
    expect = np.full(int(out_off[-1]) + 64, SENT, np.uint8)
    for o, t in zip(out_off, texts):
        expect[o:o + len(t)] = np.frombuffer(t, np.uint8)
    x, out = _dev(data), torch.full((expect.size,), SENT, dtype=torch.uint8, device=DEV)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    d_in_off = _dev(in_off)
    if not gaps.any() and not out_skew:  # packed tight: the helper gives the same offsets
        lay = b64.lines_batch_layout(d_in_off, L, sep, trailing, pad=abc[2])
        assert lay.is_cuda and np.array_equal(lay.cpu().numpy(), out_off)
    b64.encode_lines_batch(x, d_in_off, out, _dev(out_off[:-1]), L, sep, trailing, abc=abc)
    got = out.cpu().numpy()
    if not np.array_equal(got, expect):
        pytest.fail(f"{fmt} {abc}: " + _first_bad(got, expect, np.ones(got.size, bool), out_off))
    return texts


def run_strict(texts, wants, datas, fmt, abc=STD, gaps=None, in_skew=0, out_skew=0):
    """One decode_strict_batch over `texts`; wants[i] = (kind, pos, out_len),
    datas[i] the bytes of an accepted text.  Every record, the decoded bytes
    of the accepted texts, and every byte outside the buffers' capacities."""
    b64 = _b64()
    L, sep, trailing = fmt
    n = len(texts)
    gaps = np.zeros(n, np.int64) if gaps is None else gaps
    caps = [strict_cap(len(t), L, len(sep), trailing) for t in texts]
    in_off = _offsets([len(t) for t in texts], 0) + in_skew
    out_off = _offsets(caps, gaps) + out_skew
    data = np.zeros(int(in_off[-1]) + 8, np.uint8)
    data[in_skew:int(in_off[-1])] = np.frombuffer(b"".join(texts), np.uint8)
    expect = np.full(int(out_off[-1]) + 64, SENT, np.uint8)
    mask = np.ones(expect.size, bool)
    for o, cap, w, d in zip(out_off, caps, wants, datas):
        done = 0
        if w[0] == OK:
            assert len(d) == w[2] <= cap
            expect[o:o + len(d)] = np.frombuffer(d, np.uint8)
            done = len(d)
        mask[o + done:o + cap] = False  # spare capacity; unspecified for a refused text
    x, out = _dev(data), torch.full((expect.size,), SENT, dtype=torch.uint8, device=DEV)
    res = torch.full((REC * n + 64,), FILL, dtype=torch.uint8, device=DEV)
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
    d_in_off = _dev(in_off)
    if not gaps.any() and not out_skew:
        lay = b64.strict_batch_layout(d_in_off, L, sep, trailing)
        assert lay.is_cuda and np.array_equal(lay.cpu().numpy(), out_off)
    b64.decode_strict_batch(x, d_in_off, out, _dev(out_off[:-1]), res[:REC * n], L, sep, trailing,
                            abc=abc)
    got = out.cpu().numpy()
    recs = records(res[:REC * n])
    assert (res[REC * n:].cpu().numpy() == FILL).all(), "a byte behind the records was written"
    for i, (r, w) in enumerate(zip(recs, wants)):
        assert r == (w[0], w[1], w[2], 0), (fmt, abc, i, len(texts[i]), int(in_off[i]) % 4,
                                            int(out_off[i]) % 4, r, w)
    if ((got != expect) & mask).any():
        pytest.fail(f"{fmt} {abc}: " + _first_bad(got, expect, mask, out_off))


def round_trip(payloads, fmt, abc=STD, seed=1, **kw):
    """Encode the batch, then feed the stdlib's texts back: every record
    {len_i, 0, OK} and the bytes the payloads."""
    rng = np.random.default_rng(seed)
    n = len(payloads)
    texts = run_encode(payloads, fmt, abc, rng.integers(0, 8, n), **kw)
    run_strict(texts, [(OK, 0, len(p)) for p in payloads], payloads, fmt, abc,
               rng.integers(0, 8, n), **kw)


def with_empties(ns):
    """Empty buffers first, last and between others."""
    ns = list(ns)
    return [0, 0] + ns[:5] + [0] + ns[5:40] + [0, 0, 0] + ns[40:] + [0]


@gpu
@pytest.mark.parametrize("L,sep", HOT_FORMATS, ids=["crlf76", "lf64", "crlfn60"])
def test_edge_lengths_both_calls(L, sep):
    for trailing in (False, True):
        for abc in (STD, NOPAD):
            ns = with_empties(edge_lengths(L, len(sep), trailing))
            payloads = [_data(n, 7 * n + L) for n in ns]
            round_trip(payloads, (L, sep, trailing), abc, seed=L + trailing)


def alignment_mix(L, s, trailing):
    """The edge lengths several times over, with fillers of 0-3 bytes between
    them, so that packed tight the buffers' input starts go through 0..3
    (mod 4) and their output starts through 0..15 (mod 16)."""
    ns = []
    for rep in range(5):
        for k, n in enumerate(edge_lengths(L, s, trailing)):
            ns += [(k + rep) % 4, n] if k % 3 != 2 else [n]
    return ns


def test_alignment_mix_covers_every_residue():
    """Packed tight, on both calls: input starts in every residue mod 4, output
    starts in every residue mod 16, fast and bytewise buffers next to each
    other.  Without pad characters, that is: padded CRLF texts all have even
    lengths."""
    for L, sep in HOT_FORMATS[:2]:
        for trailing in (False, True):
            ns = np.array(alignment_mix(L, len(sep), trailing))
            text = np.array([formula(int(n), False, L, len(sep), trailing) for n in ns])
            cap = np.array([strict_cap(int(w), L, len(sep), trailing) for w in text])
            big = ns > 16
            for sizes_in, sizes_out in ((ns, text), (text, cap)):
                i, o = _offsets(sizes_in, 0)[:-1], _offsets(sizes_out, 0)[:-1]
                assert set((i[big] % 4).tolist()) == {0, 1, 2, 3}
                assert set((o[big] % 16).tolist()) == set(range(16))
                fast = ((i | o) % 4 == 0) & big
                assert fast.sum() >= 10 and (big & ~fast).sum() >= 10
                assert (fast[1:] != fast[:-1]).sum() >= 20


@gpu
@pytest.mark.parametrize("L,sep", HOT_FORMATS[:2], ids=["crlf76", "lf64"])
def test_alignment_mix_packed_tight(L, sep):
    for trailing in (False, True):
        ns = alignment_mix(L, len(sep), trailing)
        payloads = [_data(n, 11 * n + L) for n in ns]
        fmt = (L, sep, trailing)
        for abc in (NOPAD, STD):
            texts = run_encode(payloads, fmt, abc)
            run_strict(texts, [(OK, 0, len(p)) for p in payloads], payloads, fmt, abc)
        # the whole batch shifted: arenas that start off a dword
        texts = run_encode(payloads[:200], fmt, in_skew=1, out_skew=3)
        run_strict(texts, [(OK, 0, len(p)) for p in payloads[:200]], payloads[:200], fmt,
                   in_skew=2, out_skew=1)


@functools.lru_cache(maxsize=None)
def production_lengths():
    """NBUF lengths log-uniform in 0..2,048 bytes with the edge lengths of the
    three formats planted."""
    rng = np.random.default_rng(0xB64 + 7)
    lens = np.floor(np.exp(rng.uniform(0, np.log(2049), NBUF))).astype(np.int64) - 1
    forced = sorted({n for L, sep in HOT_FORMATS for n in edge_lengths(L, len(sep)) if n <= 2048})
    lens[rng.choice(NBUF, len(forced), replace=False)] = forced
    assert lens.min() == 0 and lens.max() <= 2048 and set(forced) <= set(lens.tolist())
    return lens


def test_production_lengths():
    lens = production_lengths()
    assert lens.size == NBUF == 4 * 8192 + 5
    assert (lens == 0).sum() > 100 and (lens > 1024).sum() > 1000 and lens.sum() < 16 << 20


@gpu
@pytest.mark.parametrize("abc", [STD, NOPAD, HIGH], ids=["default", "nopad", "high"])
def test_production_shape(abc):
    """32,773 buffers: every persistent wave walks several, the last ones a
    different number."""
    lens = production_lengths()
    blob = util.splitmix64(0x9A0D, int(lens.sum())).tobytes()
    off = _offsets(lens, 0)
    payloads = [blob[off[i]:off[i + 1]] for i in range(NBUF)]
    round_trip(payloads, (76, b"\r\n", True), abc, seed=3)


@gpu
def test_short_lines_take_the_bytewise_call_path():
    ns = with_empties(list(range(40)) + [100, 255, 256, 1000, 3001])
    payloads = [_data(n, 13 * n + 4) for n in ns]
    for trailing in (False, True):
        for abc in (STD, NOPAD):
            round_trip(payloads, (4, b"\n", trailing), abc, seed=4)


def plain_cases():
    """Plain texts (fmt NULL): (text, want, data) per alphabet."""
    out = {}
    for abc in (STD, NOPAD):
        rows = []
        for n in with_empties(list(range(30)) + [47, 48, 49, 190, 191, 192, 193, 768, 769, 770,
                                                  3070, 3071, 3072, 3073, 12289]):
            d = _data(n, 17 * n + 1)
            rows.append((ref_text(d, abc=abc), (OK, 0, n), d))
        good = ref_text(_data(700, 5), abc=abc)
        for cut in range(1, 9):  # every residue of the length mod 4, short and long
            for t in (good[:cut], good[:400 + cut]):
                want = strict_ref(t, abc=abc)
                rows.append((t, want, _decode(t, abc) if want[0] == OK else None))
        out[abc] = rows
        kinds = {w[0] for _, w, _ in rows}
        assert LENGTH in kinds and OK in kinds
        bad_len = {len(t) % 4 for t, w, _ in rows if w[0] == LENGTH}
        assert bad_len == ({1, 2, 3} if abc[2] else {1}), bad_len
    return out


def _decode(t, abc):
    from tests.test_decode_strict import stdlib_decode
    return stdlib_decode(t, abc)


def test_plain_cases_hold_the_length_rules():
    plain_cases()


@gpu
def test_plain_texts():
    for abc, rows in plain_cases().items():
        rng = np.random.default_rng(5)
        run_strict([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                   (None, b"", True), abc, rng.integers(0, 8, len(rows)))
        run_strict([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                   (None, b"", True), abc)


def offence_cases():
    """Valid CRLF-76 texts in which chosen buffers carry one corruption each
    (or two), every corrupted buffer between valid neighbours:
    [(text, want, data or None)]."""
    L, sep = CRLF76
    P = L + len(sep)
    rows = []

    def valid(n, seed):
        d = _data(n, seed)
        rows.append((ref_text(d, L, sep), (OK, 0, n), d))

    def spoiled(n, seed, edit, kinds):
        t = bytearray(ref_text(_data(n, seed), L, sep))
        edit(t)
        want = strict_ref(bytes(t), L, sep)
        assert want[0] in kinds, (n, want, kinds)
        valid(300 + len(rows), 1000 + len(rows))
        rows.append((bytes(t), want, None))

    def put(pos, value):
        def edit(t):
            t[pos if pos >= 0 else len(t) + pos] = value
        return edit

    def both(*edits):
        def edit(t):
            for e in edits:
                e(t)
        return edit

    for n in (700, 5001, 61):  # hot lanes and a tail; many passes; all tail
        W = formula(n, True, L, 2, True)
        hot_at = 3 * P + 17 if n > 100 else 5          # a character in a hot lane
        tail_at = W - 2 - 6                            # a character of the last groups
        sep_hot = 2 * P + L if n > 100 else None       # a separator inside the hot part
        for value, kind in ((0x00, CHAR), (0x3D, PAD)):
            for pos in (hot_at, tail_at, 0):
                spoiled(n, n + pos, put(pos, value), {kind})
        spoiled(n, n + 1, put(-1, 0x20), {SEP})        # the buffer's last byte
        spoiled(n, n + 2, put(-2, 0x0A), {SEP})
        if sep_hot:
            spoiled(n, n + 3, put(sep_hot, 0x20), {SEP})
            spoiled(n, n + 4, put(sep_hot + 1, 0x0D), {SEP})
        # two offences in one buffer: the lower offset wins
        spoiled(n, n + 5, both(put(tail_at, 0x00), put(hot_at, 0x3D)), {PAD})
        spoiled(n, n + 6, both(put(hot_at + 1, 0x00), put(-1, 0x00)), {CHAR})
        assert rows[-1][1][1] == hot_at + 1
        # a length no encoder output has; a deleted and an added separator byte
        spoiled(n, n + 7, lambda t: t.append(0x41), {LENGTH})
        spoiled(n, n + 8, lambda t: t.pop(), {LENGTH})
        if n > 100:
            spoiled(n, n + 9, lambda t: t.pop(P + L), {LENGTH, CHAR, SEP})
            spoiled(n, n + 10, lambda t: t.insert(P + L, 0x0D), {LENGTH, CHAR, SEP})
            spoiled(n, n + 11, lambda t: (t.pop(P + L), t.append(0x0A)), {CHAR, SEP})
    # BITS on the last data character: one and two pad characters, hot and short texts
    for n in (700, 701, 4, 5, 58 + 57):
        if n % 3 == 0:
            n += 1
        t = ref_text(_data(n, n), L, sep)
        last = len(t) - 2 - (3 - n % 3) - 1
        assert t[last + 1:last + 2] == b"=" and t[last:last + 1] != b"="
        spoiled(n, n, put(last, ord("B") if t[last] != ord("B") else ord("C")), {BITS})
        assert rows[-1][1][1] == last
    valid(123, 9)
    kinds = {w[0] for _, w, _ in rows}
    assert kinds == {OK, CHAR, SEP, PAD, BITS, LENGTH}
    for i, (_, w, _) in enumerate(rows):  # the neighbours of every corrupted buffer are valid
        if w[0] != OK:
            assert rows[i - 1][1][0] == OK and rows[i + 1][1][0] == OK
    return rows


def test_offence_cases_cover_every_kind():
    rows = offence_cases()
    assert sum(w[0] != OK for _, w, _ in rows) >= 40
    for t, w, _ in rows[:60]:
        assert w == np_ref(np.frombuffer(t, np.uint8), *CRLF76)


@gpu
def test_every_kind_of_offence_per_buffer():
    """The batch packed tight at every input and output skew: in one of the
    sixteen runs each buffer, corrupted or not, is dword aligned on both sides
    and takes the hot path; in the others it is decoded bytewise."""
    rows = offence_cases()
    fmt = (76, b"\r\n", True)
    texts, wants, datas = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    run_strict(texts, wants, datas, fmt, gaps=np.random.default_rng(6).integers(0, 8, len(rows)))
    for in_skew in range(4):
        for out_skew in range(4):
            run_strict(texts, wants, datas, fmt, in_skew=in_skew, out_skew=out_skew)


@gpu
def test_graph_replay_on_other_lengths():
    """One capture of both calls on fixed tensors; each replay runs on other
    lengths and contents written into those tensors: nothing on the host
    depends on a length."""
    b64 = _b64()
    nbuf, top = 300, 900
    fmt = (76, b"\r\n", True)
    in_cap = nbuf * top
    text_cap = formula(top, True, 76, 2, True) * nbuf
    x = torch.zeros(in_cap, dtype=torch.uint8, device=DEV)
    in_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=DEV)
    out_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=DEV)
    out = torch.full((text_cap + 64,), SENT, dtype=torch.uint8, device=DEV)
    tx = torch.zeros(text_cap, dtype=torch.uint8, device=DEV)
    t_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=DEV)
    d_off = torch.zeros(nbuf + 1, dtype=torch.int64, device=DEV)
    dout = torch.full((in_cap + 3 * nbuf + 64,), SENT, dtype=torch.uint8, device=DEV)
    res = torch.full((REC * nbuf + 64,), FILL, dtype=torch.uint8, device=DEV)

    def both():
        b64.encode_lines_batch(x, in_off, out, out_off[:-1], *fmt)
        b64.decode_strict_batch(tx, t_off, dout, d_off[:-1], res[:REC * nbuf], *fmt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        both()  # warm-up outside the capture (all lengths zero)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            both()
    rng = np.random.default_rng(8)
    for rep in range(3):
        lens = rng.integers(0, top + 1, nbuf)
        lens[rng.choice(nbuf, 40, replace=False)] = 0
        lens[rng.choice(nbuf, 3, replace=False)] = (top, 1, 57)
        payloads = [_data(int(n), 31 * rep + i) for i, n in enumerate(lens)]
        texts = [bytearray(ref_text(p, *fmt)) for p in payloads]
        wants = [(OK, 0, len(p)) for p in payloads]
        for i in rng.choice(nbuf, 12, replace=False):  # a few refused texts per replay
            if len(texts[i]) > 8:
                texts[i][int(rng.integers(0, len(texts[i])))] = 0x21
                wants[i] = strict_ref(bytes(texts[i]), *fmt)
        gaps = rng.integers(0, 8, nbuf)
        tl = np.array([len(t) for t in texts])
        caps = np.array([strict_cap(int(n), 76, 2, True) for n in tl])
        h_in, h_out, h_t, h_d = (_offsets(lens, 0), _offsets(tl, gaps), _offsets(tl, 0),
                                 _offsets(caps, gaps))
        assert h_in[-1] <= in_cap and h_out[-1] <= text_cap + 64 and h_d[-1] <= dout.numel()
        for dst, src in ((in_off, h_in), (out_off, h_out), (t_off, h_t), (d_off, h_d)):
            dst.copy_(torch.from_numpy(src))
        x[:int(h_in[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(payloads), np.uint8).copy()))
        tx[:int(h_t[-1])].copy_(torch.from_numpy(np.frombuffer(b"".join(map(bytes, texts)),
                                                               np.uint8).copy()))
        out.fill_(SENT)
        dout.fill_(SENT)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        expect = np.full(out.numel(), SENT, np.uint8)
        for o, p in zip(h_out, payloads):
            t = ref_text(p, *fmt)
            expect[o:o + len(t)] = np.frombuffer(t, np.uint8)
        assert np.array_equal(out.cpu().numpy(), expect), rep
        got = dout.cpu().numpy()
        expect = np.full(got.size, SENT, np.uint8)
        mask = np.ones(got.size, bool)
        for o, cap, w, p in zip(h_d, caps, wants, payloads):
            done = len(p) if w[0] == OK else 0
            expect[o:o + done] = np.frombuffer(p[:done], np.uint8)
            mask[o + done:o + cap] = False
        assert not ((got != expect) & mask).any(), rep
        recs = records(res[:REC * nbuf])
        assert recs == [(w[0], w[1], w[2], 0) for w in wants], rep
        assert (res[REC * nbuf:].cpu().numpy() == FILL).all()


@gpu
def test_one_long_buffer():
    """nbuf == 1, 3 MiB + 1 byte: one wave's inner loop runs thousands of
    times."""
    n = (3 << 20) + 1
    payload = _data(n, 77)
    for fmt in ((76, b"\r\n", True), (64, b"\n", False)):
        texts = run_encode([payload], fmt)
        run_strict(texts, [(OK, 0, n)], [payload], fmt)
    plain = ref_text(payload)
    run_strict([plain], [(OK, 0, n)], [payload], (None, b"", True))
