"""Strict skip decode of many pieces of any size in one call
(b64x_decode_strict_skip_pieces_wide, async_amd.b64.decode_strict_skip_pieces_wide):
every record, every piece's bytes and every state, bit for bit, against the
chunked scalar procedure of tests/test_decode_strict_skip_pieces.py (RefState,
ref_piece, ref_stream), the whole-text references of
tests/test_decode_strict_skip.py, and the calls the unit stands next to on the
GPU: decode_strict_skip_pieces on the same pieces and twin states,
decode_strict_skip_piece taking turns on the same states, decode_strict_skip on
the whole text.  The new call is never compared with itself alone.

Pieces too long for the bytewise model (more than SMALL bytes) are clean by
construction -- data characters and skipped bytes only, whole groups where the
piece is final -- and go through fast_piece: bytes.translate and the stdlib's
base64.b64decode(validate=True) for the bytes, numpy for the state's totals.

The unit's rules (async_amd/csrc/b64x_skip_pieces_wide_plan.h), restated: with
total_cap the host bound on the call's text,
    T = max(4,096, ceil(ceil((total_cap + 15) / 16,384) / 1,024) * 1,024)
a piece of len bytes whose first byte stands head bytes behind a 16-byte
boundary has max(1, ceil((len + head) / T)) tiles, a call at most
    B = ceil(total_cap / T) + 2 npieces
of them, and the workspace is 64 bytes of control words, 64 bytes per piece,
64 + 8 bytes per tile of B and 4 bytes for each of the min(B // 65, npieces)
pieces that can have more than 64 tiles, every part rounded up to 64 bytes.
The scan takes a piece of up to 64 tiles in one wave, a record to a lane, and
a longer one in a workgroup of 256 lanes, a strip of ceil(tiles / 256) records
to a lane, loaded four at a time.

GPU tests lay a call out as tests/test_decode_strict_skip_pieces.py does: the
pieces of one call lie end to end, so the guard between two pieces is a piece
of its own, at least 64 bytes of 0xA5 that continues a state which holds a
report; it must get the report again and write nothing.  Every capacity stands
between 64 guard bytes, a guard stands behind the records, the states and the
workspace, which is handed over full of 0xA5: it needs no preparation.
"""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from async_amd import _lib
from tests import util
from tests.test_decode_strict import BITS, CHAR, FILL, GUARD, LENGTH, OK, PAD, REC, alpha, plain
from tests.test_decode_strict_skip import (CRLF, DOTPAD, NOPAD, STD, URL, crlf76, decode_kept,
                                           random_texts, records, skip_bytes, skip_ref, strip)
from tests.test_decode_strict_skip_pieces import RefState, cap_of, cut, ref_piece, ref_stream

ROOT = util.ROOT
T, P = 4096, 1024
MAX_TILES = 16384
WAVE_TILES, TH = 64, 256
STATE = 128
BOUND = 6
TOP = (1 << 64) - 1
SMALL = 512  # a longer piece goes through fast_piece where it can
ALL_KINDS = {OK, CHAR, PAD, BITS, LENGTH}
NAME = "b64x_decode_strict_skip_pieces_wide"
SIZE = "b64x_strict_skip_pieces_wide_workspace_size"


def tile_of(cap: int) -> int:
    per = -(-min(cap + 15, TOP) // MAX_TILES)
    return max(T, -(-per // P) * P)


def bound_of(cap: int, n: int) -> int:
    return -(-cap // tile_of(cap)) + 2 * n


def _up64(v: int) -> int:
    return -(-v // 64) * 64


def ws_of(cap: int, n: int) -> int:
    b = bound_of(cap, n)
    return 64 + 64 * n + 64 * b + _up64(8 * b) + _up64(4 * min(b // (WAVE_TILES + 1), n))


def tiles_of(n: int, head: int, tile: int = T) -> int:
    return max(1, -(-(n + head) // tile))


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


LINE = crlf76(_data(57, 2))  # 76 data characters, CR, LF
assert len(LINE) == 78 and b"=" not in LINE


def clean_text(n: int, seed: int = 1, whole: bool = True, abc=STD) -> bytes:
    """n bytes of CRLF-76 text without a pad character whose last data
    character has no low bits set; whole: its data characters are whole
    groups (the rest of the last line becomes line feeds)."""
    if n == 0:
        return b""
    line = np.frombuffer(crlf76(_data(57, seed), abc), np.uint8)
    a = np.roll(np.tile(line, n // 78 + 2), -(seed % 7))[:n].copy()
    at = np.flatnonzero((a != 0x0A) & (a != 0x0D))
    if whole and at.size % 4:
        a[at[at.size - at.size % 4:]] = 0x0A
        at = at[:at.size - at.size % 4]
    if at.size:
        a[at[-1]] = 0x41  # A
    return a.tobytes()


def spread(chars: bytes, gaps: dict) -> bytes:
    """chars with gaps[i] line feeds in front of chars[i] (i == len: behind)."""
    out = bytearray()
    for i, c in enumerate(chars):
        out += b"\n" * gaps.get(i, 0)
        out.append(c)
    return bytes(out + b"\n" * gaps.get(len(chars), 0))


def fast_piece(st: RefState, piece: bytes, final: bool, skip=CRLF, abc=STD):
    """ref_piece for a clean piece of a text that is clean so far: data
    characters and skipped bytes only; a final one ends its text on a whole
    group, on a length that is an offence, or, without pad, on a group of 2 or
    3 whose last character has no low bits.  None, and the state as it was,
    where the piece is not of that kind: it is ref_piece's."""
    chars, pad, padc = alpha(abc)
    if st.report is not None or st.c or st.first_char is not None:
        return None
    a = np.frombuffer(piece, np.uint8)
    keep = ~np.isin(a, np.frombuffer(bytes(skip), np.uint8))
    at = np.flatnonzero(keep)
    kept = a[at].tobytes()
    if kept.translate(None, bytes(chars)):
        return None
    if final:
        text = bytes(chars[s] for s in st.sextets) + kept
        if len(text) % 4 in (2, 3) and chars.index(text[-1]):
            return None
    for p in at[-3:]:
        st.tail = (st.tail + [(st.pos + int(p), int(a[p]))])[-3:]
    st.E += len(kept)
    st.pos += len(piece)
    text = bytes(chars[s] for s in st.sextets) + kept
    if not final:
        whole = len(text) // 4 * 4
        st.sextets = [chars.index(b) for b in text[whole:]]
        data = decode_kept(text[:whole], abc)
        return (OK, 0, len(data)), data
    r = len(text) % 4
    if (pad and st.E % 4) or (not pad and st.E % 4 == 1):
        rec = (LENGTH, st.pos, 0)
        st.reset()
        return rec, None
    data = decode_kept(text + bytes(chars[:1]) * (-len(text) % 4), abc)[:len(text) // 4 * 3 + (0, 0, 1, 2)[r]]
    st.reset()
    return (OK, 0, len(data)), data


# ----------------------------------------------------------------- CPU --

def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    assert hasattr(lib, NAME) and hasattr(lib, SIZE)
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 14 and getattr(lib, NAME).argtypes == args and res is ctypes.c_int
    assert args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint64
    res, args = _lib.SIGNATURES[SIZE]
    assert args == [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_bool] and res is ctypes.c_uint64
    header = open(os.path.join(ROOT, "include", "b64x.h")).read()
    assert re.search(r"^int b64x_decode_strict_skip_pieces_wide\(", header, re.M)
    assert re.search(r"^uint64_t b64x_strict_skip_pieces_wide_workspace_size\(uint64_t total_cap, "
                     r"uint32_t npieces, bool validate_only\);", header, re.M)
    assert re.search(r"^#define B64X_STRICT_BOUND 6u", header, re.M)
    assert "#define B64X_ABI_VERSION 7" in header and b"abi=7" in lib.b64x_build_info()
    from async_amd import b64
    assert b64.STRICT_BOUND == BOUND
    for name in ("decode_strict_skip_pieces_wide", "strict_skip_pieces_wide_workspace_size"):
        assert name in b64.__doc__ and callable(getattr(b64, name))
    check_fast_piece()


def _host_call():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def call(skip=None, abc=None, d_in=p, off=p, n=2, cap=100, d_out=p, out_off=p, state=p, sid=None,
             flags=None, d_res=p, ws=p + 4096):
        return lib.b64x_decode_strict_skip_pieces_wide(d_in, off, n, cap, d_out, out_off, state, sid,
                                                       flags, d_res, ref(abc), ref(skip), ws, None)
    return lib, p, call


def test_invalid_arguments_in_their_order():
    lib, p, call = _host_call()
    nodev = lib.b64x_device_check() == -19

    def raw(n, b):
        return _lib.Skip(n, (ctypes.c_uint8 * 8)(*b))
    a = _lib.alphabet()
    bad_abc = _lib.alphabet("+", "+")
    nine = raw(9, b"\r\n\t \x0b\x0c\x00\x01")
    # 1. no pieces: done before anything is looked at
    assert call(nine, bad_abc, d_in=None, off=None, state=None, d_res=None, out_off=None, ws=None,
                n=0) == 0
    # 2. NULL pointers and the alignment of records, states and workspace, before everything else
    for kw in ({"d_in": None}, {"off": None}, {"state": None}, {"d_res": None}, {"ws": None},
               {"d_res": p + 4}, {"state": p + 4}, {"ws": p + 4100}):
        assert call(**kw) == -22, kw
        assert call(nine, bad_abc, out_off=None, **kw) == -22, kw
        assert call(d_out=None, out_off=None, **kw) == -22, kw
    # 3. an output needs its offsets, before the skip set and the alphabet
    assert call(out_off=None) == -22
    assert call(nine, bad_abc, out_off=None) == -22
    # 4. the skip set, before the alphabet
    for skip, abc in ((nine, a), (raw(1, b"A"), a), (raw(2, b"\n="), a), (raw(2, b"\n+"), a),
                      (raw(1, b"_"), _lib.alphabet("-", "_")), (nine, bad_abc), (raw(1, b"z"), bad_abc)):
        assert call(skip, abc) == -22
        assert call(skip, abc, d_out=None, out_off=None) == -22
    # 5. the alphabet rules of the strict decoder
    for abc in (bad_abc, _lib.alphabet("A", "/"), _lib.alphabet(padchar="A"),
                _lib.alphabet("-", "_", True, "_")):
        assert call(None, abc) == -22
        assert call(None, abc, d_out=None, out_off=None) == -22
    # 6. valid calls reach the device check (with a device these host pointers
    # must never reach a kernel, so the calls are not made)
    if nodev:
        for kw in ({}, {"d_out": None, "out_off": None}, {"sid": p, "flags": p}, {"cap": 0},
                   {"cap": TOP}, {"n": (1 << 32) - 1}, {"skip": raw(0, b"")},
                   {"skip": raw(1, b"="), "abc": _lib.alphabet(pad=False)},
                   {"d_in": p + 1, "d_out": p + 3, "state": p + 8, "d_res": p + 8, "ws": p + 4104}):
            assert call(**kw) == -19, kw


def test_workspace_size():
    lib = _lib.load()
    from async_amd import b64
    big = (1 << 32) - 1
    caps = (0, 1, (64 << 20) - 16, (64 << 20) - 15, (64 << 20) - 14, 1 << 32, 1 << 40, TOP)
    assert [tile_of(c) for c in caps] == [T, T, T, T, T + P, 257 * P, (1 << 26) + P,
                                          1 << 50]
    for cap in caps:
        for n in (1, 2, 300, big):
            want = ws_of(cap, n)
            assert want < 1 << 41 and want % 64 == 0  # no wraparound anywhere
            assert want >= 64 + 64 * n + 72 * bound_of(cap, n)
            for validate_only in (False, True):
                assert lib.b64x_strict_skip_pieces_wide_workspace_size(cap, n, validate_only) == want, \
                    (cap, n)
            assert b64.strict_skip_pieces_wide_workspace_size(cap, n) == want
    assert ws_of(0, 1) == 64 + 64 + 2 * 64 + 64 + 0
    assert ws_of(1, 1) == 64 + 64 + 3 * 64 + 64 + 0
    assert bound_of(TOP, big) == -(-TOP // tile_of(TOP)) + 2 * big < 1 << 34
    # no piece within the bound has more tiles than one workgroup scans
    for cap in caps:
        assert tiles_of(min(cap, TOP - 15), 15, tile_of(cap)) <= MAX_TILES  # len + head saturates


def test_wrapper_value_errors():
    """What the wrapper refuses without a device: tensors that are not on one,
    and a skip set of nine bytes (test_wrapper_size_errors makes the size
    checks, on device tensors)."""
    from async_amd import b64
    cpu = torch.zeros(8192, dtype=torch.uint8)
    off = torch.tensor([0, 10, 20])
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces_wide(cpu, off, cpu, off, cpu, cpu, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces_wide(cpu, off, None, None, cpu, cpu, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces_wide(cpu, off, cpu, off, cpu, cpu, cpu, skip=b"123456789")


# The kernels of b64x_skip_pieces_wide.hip; nothing else may be in its code object.
PW_KERNELS = {"k_skip_pw_prep", "k_skip_pw_count", "k_skip_pw_scan", "k_skip_pw_decode"}


def test_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_skip_pieces_wide.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == PW_KERNELS, (got - PW_KERNELS, PW_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == len(PW_KERNELS)  # one each


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/skip_pieces_wide_plan_check.cpp built with the host compiler
    under ASan + UBSan: a stand-alone program, run as a child process.  The
    sanitizers' runtimes are linked into the program itself."""
    exe = str(tmp_path_factory.mktemp("plan") / "skip_pieces_wide_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "skip_pieces_wide_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def test_plan_program_matches_the_python_formulas(plan_program):
    caps = [0, 1, 15, 16, T - 1, T, T + 1, (64 << 20) - 16, (64 << 20) - 15, (64 << 20) - 14,
            (1 << 32) - 1, 1 << 32, 1 << 40, (1 << 63) + 3, TOP - 15, TOP]
    rng = random.Random(14)
    caps += [rng.randrange(1 << rng.randrange(1, 64)) for _ in range(200)]
    queries = [(c, n, cus) for c in caps for n in (1, 2, 77, 4097, (1 << 32) - 1) for cus in (1, 256)]
    run = subprocess.run([plan_program], input="".join("%d %d %d\n" % q for q in queries),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == len(queries)
    for (cap, n, cus), (tile, shift, bound, big, heads, recs, tmap, blist, size, tgrid, sgrid) in \
            zip(queries, rows):
        assert tile == tile_of(cap) and tile % P == 0, cap
        assert (1 << shift == tile) if tile & (tile - 1) == 0 else shift == 0
        assert bound == bound_of(cap, n) and big == min(bound // 65, n)
        assert heads == 64 and recs == heads + 64 * n and tmap == recs + 64 * bound
        assert blist == tmap + _up64(8 * bound) and size == blist + _up64(4 * big) == ws_of(cap, n)
        assert tgrid == min(-(-bound // 4), 8 * cus) >= 1 and sgrid == min(n, 8 * cus) >= 1


def test_plan_program_tile_bound_by_brute_force(plan_program):
    run = subprocess.run([plan_program, "brute"], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert int(run.stdout) == 20000 * 6


def check_fast_piece():
    """This file's own model against the bytewise one, before anything relies
    on it (a self-check of the tests, run by the test of the symbols)."""
    rng = random.Random(3)
    for abc in (STD, NOPAD):
        for _ in range(40):
            t = clean_text(rng.randrange(1, 900), rng.randrange(99), whole=abc == STD)
            pieces = cut(t, [rng.randrange(len(t) + 1) for _ in range(rng.randrange(4))])
            a, b = RefState(), RefState()
            for i, p in enumerate(pieces):
                final = i == len(pieces) - 1
                got = fast_piece(a, p, final, CRLF, abc)
                assert got is not None and got == ref_piece(b, p, final, CRLF, abc)
                assert vars(a) == vars(b)
    dirty = RefState()
    for piece, final in ((b"QU*D", False), (b"QQ==", True), (b"QR", True)):
        assert fast_piece(dirty, piece, final, CRLF, NOPAD if piece == b"QR" else STD) is None
        assert dirty.is_zero()


# ----------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


def _up16(n: int) -> int:
    return -(-n // 16) * 16


def _dev(b: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


class Hub:
    """n states on the device with their reference states, a guard behind
    them, and behind the n one more per piece of the largest call plus one:
    states that hold a report from the start, for the guard pieces.  call()
    runs one call of the named kind and checks all of it."""

    def __init__(self, n: int, skip=CRLF, abc=STD, widest=None):
        b64 = _b64()
        self.n, self.skip, self.abc = n, skip, abc
        self.spare = (widest or n) + 1
        total = n + self.spare
        self.all = torch.full((total * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.states = self.all[:total * STATE]
        self.states.zero_()
        assert self.states.data_ptr() % 8 == 0
        self.ref = [RefState() for _ in range(n)]
        # a stranger for every spare state: from now on it repeats {CHAR, 0}
        x = torch.full((self.spare,), 0x2A, dtype=torch.uint8, device="cuda")
        off = torch.arange(self.spare + 1, dtype=torch.int64, device="cuda")
        res = torch.zeros(REC * self.spare, dtype=torch.uint8, device="cuda")
        b64.decode_strict_skip_pieces(x, off, None, None, self.states[n * STATE:], res,
                                      skip=skip, abc=abc)
        assert records(res) == [(CHAR, 0, 0, 0)] * self.spare

    def call(self, items, how="pw", validate_only=False, in_at=None, out_at=None, total_cap=None,
             no_flags=False):
        """items: [(state index, piece, final)].  how: "pw" the new call,
        "pieces" the pieces call, "one" a one-piece call per item.  in_at[j] /
        out_at[j]: the address mod 16 of piece j and of its output (default
        0).  total_cap: the bound handed to the new call (default: the size
        of the text buffer); the workspace's size follows it.  no_flags: no
        flags are passed (no item may be final).
        Returns [(record, the piece's bytes or None)] as the device gave
        them; self.last keeps (records, capacities' bytes, states' bytes)."""
        b64 = _b64()
        assert len(items) < self.spare and len({s for s, _, _ in items}) == len(items)
        pieces, sids, flags, out_off, real = [], [], [], [], []
        pos, size = 0, GUARD
        for j, (sid, piece, final) in enumerate(items):
            gap = GUARD + ((in_at[j] if in_at else 0) - pos - GUARD) % 16
            pieces.append(bytes([FILL]) * gap)
            sids.append(self.n + j)
            flags.append(0)
            out_off.append(0)  # into the leading guard: a guard piece writes nothing
            pos += gap
            pieces.append(bytes(piece))
            sids.append(sid)
            flags.append(1 if final else 0)
            o = _up16(size) + (out_at[j] if out_at else 0)
            out_off.append(o)
            real.append((len(pieces) - 1, pos, o, cap_of(len(piece))))
            size = o + cap_of(len(piece)) + GUARD
            pos += len(piece)
        pieces.append(bytes([FILL]) * GUARD)
        sids.append(self.n + len(items))
        flags.append(0)
        out_off.append(0)
        size += GUARD
        assert not (no_flags and any(flags))
        npieces = len(pieces)
        in_off = np.zeros(npieces + 1, np.int64)
        np.cumsum([len(p) for p in pieces], out=in_off[1:])
        x = _dev(b"".join(pieces))
        out = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * npieces + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
        d_flags = None if no_flags else torch.tensor(flags, dtype=torch.uint8, device="cuda")
        d_sid = torch.tensor(sids, dtype=torch.int32, device="cuda")
        d_in_off = torch.from_numpy(in_off).cuda()
        d_out_off = None if validate_only else torch.tensor(out_off, dtype=torch.int64, device="cuda")
        ws = need = None
        if how == "pw":
            cap = x.numel() if total_cap is None else total_cap
            need = b64.strict_skip_pieces_wide_workspace_size(cap, npieces, validate_only)
            assert need == ws_of(cap, npieces)
            ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            b64.decode_strict_skip_pieces_wide(x, d_in_off, None if validate_only else out, d_out_off,
                                               self.states, res[:REC * npieces], ws[:need],
                                               total_cap=total_cap, sid=d_sid, flags=d_flags,
                                               skip=self.skip, abc=self.abc)
        elif how == "pieces":
            b64.decode_strict_skip_pieces(x, d_in_off, None if validate_only else out, d_out_off,
                                          self.states, res[:REC * npieces], final=d_flags, sid=d_sid,
                                          skip=self.skip, abc=self.abc)
        else:
            assert how == "one"
            for (sid, piece, final), (i, at, o, cap) in zip(items, real):
                b64.decode_strict_skip_piece(
                    x[at:at + len(piece)], self.states[sid * STATE:(sid + 1) * STATE],
                    res[REC * i:REC * (i + 1)], out=None if validate_only else out[o:o + cap],
                    final=final, skip=self.skip, abc=self.abc)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        recs = records(res)[:npieces]
        states = self.all.cpu().numpy()
        assert (res[REC * npieces:].cpu().numpy() == FILL).all(), "the guard behind the records"
        assert (states[-GUARD:] == FILL).all(), "the guard behind the states"
        if ws is not None:
            assert (ws[need:].cpu().numpy() == FILL).all(), "the guard behind the workspace"
        if how != "one":
            assert recs[0::2] == [(CHAR, 0, 0, 0)] * (len(items) + 1), "a guard piece's record"
        mask = np.ones(got.size, bool)
        result, caps = [], []
        for (sid, piece, final), (i, at, o, cap) in zip(items, real):
            had_report = self.ref[sid].report is not None
            fast = fast_piece(self.ref[sid], piece, final, self.skip, self.abc) \
                if len(piece) > SMALL else None
            want, data = fast or ref_piece(self.ref[sid], piece, final, self.skip, self.abc)
            label = (how, sid, len(piece), piece[:24], final, at % 16, o % 16, self.skip, self.abc,
                     validate_only)
            assert recs[i] == (want[0], want[1], want[2], 0), (label, recs[i], want)
            if not validate_only and data is not None:
                assert got[o:o + want[2]].tobytes() == data, label
            # Behind a report nothing at all is written; the new call and the
            # one-piece call write nothing with a new offence either.
            if not validate_only and not had_report and (want[0] == OK or how == "pieces"):
                mask[o:o + cap] = False
            st = states[sid * STATE:(sid + 1) * STATE]
            if final:
                assert not st.any(), (label, "state not zeroed")
            else:
                assert not st[88:].any(), (label, "words 11 to 15")
            result.append((recs[i], None if validate_only or data is None else data))
            caps.append(got[o:o + cap].copy())
        assert (got[mask] == FILL).all(), "a byte outside the capacities of accepted pieces was written"
        self.last = ([recs[i] for i, _, _, _ in real], caps, states[:self.n * STATE].copy())
        return result

    def all_zero(self):
        assert not self.states[:self.n * STATE].any(), "a finished text left its state armed"
        assert all(r.is_zero() for r in self.ref)


def same_as_the_pieces_call(mine: Hub, twin: Hub, items, one: Hub = None):
    """After the same items by the new call on `mine` and by the pieces call on
    `twin`: equal records, equal bytes of the accepted pieces, and states
    equal in all 16 words.  After a piece that is not final and reports PAD or
    CHAR the pieces call pins words 9 and 10 only (all any call reads of such
    a state; its own words 0 to 8 mix counts of kept bytes and of data
    characters there): words 11 to 15 must be zero, and with `one`, a third
    hub that took the same items through one-piece calls, all 16 words must be
    that call's, after an offence too."""
    (r1, c1, s1), (r2, c2, s2) = mine.last, twin.last
    if one is not None:
        assert one.last[0] == r1
        assert one.last[2].tobytes() == s1.tobytes(), "a state differs from the one-piece call's"
    assert r1 == r2
    for j, (sid, piece, final) in enumerate(items):
        if r1[j][0] == OK:
            assert c1[j][:r1[j][2]].tobytes() == c2[j][:r1[j][2]].tobytes(), (j, len(piece))
        a, b = (s[sid * STATE:(sid + 1) * STATE] for s in (s1, s2))
        if r1[j][0] == OK or final:
            assert a.tobytes() == b.tobytes(), (j, len(piece), a.view(np.uint64), b.view(np.uint64))
        else:
            assert a[72:88].tobytes() == b[72:88].tobytes(), (j, len(piece))
            assert not a[88:].any() and not b[88:].any(), (j, len(piece))


def both(n, items_of_calls, skip=CRLF, abc=STD, **kw):
    """Every call of items_of_calls on a fresh Hub by the new call, on a twin
    by the pieces call and on a third by one-piece calls, decoding and
    validate only."""
    widest = max(len(items) for items in items_of_calls)
    out = None
    for validate_only in (False, True):
        mine, twin, one = (Hub(n, skip, abc, widest) for _ in range(3))
        got = []
        for items in items_of_calls:
            got.append(mine.call(items, "pw", validate_only=validate_only, **kw))
            at = {k: v for k, v in kw.items() if k in ("in_at", "out_at")}
            twin.call(items, "pieces", validate_only=validate_only, **at)
            one.call(items, "one", validate_only=validate_only, **at)
            same_as_the_pieces_call(mine, twin, items, one)
        out = out or got
    return out


@gpu
def test_wrapper_size_errors():
    """The wrapper's size and type checks: no call reaches the library."""
    b64 = _b64()
    x = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 10, 20, 30], device="cuda")
    states = b64.skip_states(3)
    res = torch.zeros(REC * 3, dtype=torch.uint8, device="cuda")
    need = b64.strict_skip_pieces_wide_workspace_size(1000, 3)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    ok = dict(x=x, in_off=off, out=x, out_off=off, states=states, result=res, workspace=ws)
    for kw in ({"result": res[:REC * 3 - 1]}, {"states": states[:2 * STATE]},
               {"states": states[:STATE + 1]}, {"states": states[4:4 + STATE]},
               {"out_off": off.int()}, {"in_off": off.int()}, {"workspace": ws[:need - 1]},
               {"workspace": ws[4:]}, {"workspace": ws, "total_cap": 1 << 30}, {"total_cap": -1},
               {"flags": torch.zeros(3, dtype=torch.int32, device="cuda")},
               {"flags": torch.zeros(2, dtype=torch.uint8, device="cuda")},
               {"sid": torch.zeros(3, dtype=torch.int64, device="cuda")},
               {"sid": torch.zeros(2, dtype=torch.int32, device="cuda")},
               {"flags": torch.zeros(3, dtype=torch.uint8)}):
        with pytest.raises(ValueError):
            b64.decode_strict_skip_pieces_wide(**{**ok, **kw})


EDGE_LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]


def edge_items():
    """Every length of EDGE_LENS at every address mod 16, final and not, on a
    zeroed state and behind a carry of 1, 2 and 3 sextets: the carry pieces,
    then the one call's items with their addresses."""
    carries, items, in_at, out_at = [], [], [], []
    for n in EDGE_LENS:
        for at in range(16):
            for final in (False, True):
                for c in range(4):
                    sid = len(items)
                    if c:
                        carries.append((sid, b"QUJ"[:c], False))
                    items.append((sid, clean_text(n, n + at + c, whole=False), final))
                    in_at.append(at)
                    out_at.append((at + c + final) % 4)
    return carries, items, in_at, out_at


def check_edges(**kw):
    carries, items, in_at, out_at = edge_items()
    widest = len(items)
    kinds = set()
    for validate_only in (False, True):
        mine, twin = Hub(len(items), CRLF, NOPAD, widest), Hub(len(items), CRLF, NOPAD, widest)
        for h in (mine, twin):
            h.call(carries, "pieces", validate_only=validate_only)
        got = mine.call(items, "pw", validate_only=validate_only, in_at=in_at, out_at=out_at, **kw)
        twin.call(items, "pieces", validate_only=validate_only, in_at=in_at, out_at=out_at)
        same_as_the_pieces_call(mine, twin, items)
        kinds |= {r[0] for r, _ in got}
    # without pad a final group of one character is LENGTH; an empty final piece
    # behind the carry QU or QUJ ends its text on a character with low bits: BITS
    assert kinds == {OK, LENGTH, BITS}
    return got


@gpu
def test_tile_edges():
    """One call: 15 lengths x 16 addresses x final or not x carries of 0..3, the
    outputs at 0..3 mod 4, T = 4,096."""
    check_edges()


@gpu
def test_larger_tile():
    """The same pieces with total_cap = 2^30 passed as a bound only: T is
    65,536, the workspace is at its large size, every piece is one tile."""
    assert tile_of(1 << 30) == 65536 + P
    check_edges(total_cap=1 << 30)


CHARS16 = plain(_data(10, 3))  # 14 data characters and ==
BRANCH_TILES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


@gpu
def test_the_scans_branches():
    """One call: pieces of 1 .. 1,025 tiles of CRLF-76 text, 64 being the last
    tile count the scan gives to a wave, with 300 pieces under 100 bytes
    between them, texts whose tiles hold only skipped bytes -- d = 0, 1 and 2,
    the sextet fill-up crossing several tiles -- and a piece that ends in
    3,000 skipped bytes.  All final, then none (no flags), then final again
    behind it."""
    assert len(CHARS16) == 16 and CHARS16.endswith(b"==")
    rng = random.Random(64)
    large = [clean_text(tiles * T - 5, tiles) for tiles in BRANCH_TILES]
    assert [tiles_of(len(t), 0) for t in large] == list(BRANCH_TILES)
    assert 7_900_000 < sum(map(len, large)) < 8_200_000  # about 8 MB together
    sparse = [
        spread(CHARS16[:12], {5: T + 3, 6: 2 * T + 1, 8: 3 * T + 1, 9: T, 11: T + 7}),
        spread(CHARS16[:12], {0: T, 3: 3 * T + 2, 4: 1, 5: T + 1, 6: T + 1, 7: 2 * T + 5, 12: T}),
        spread(CHARS16[:12], {1: 4 * T, 2: T - 1, 3: T - 1, 10: T + 1, 11: 3, 12: T}),
        spread(b"QUJDQUJD", {5: T + 1, 6: 2 * T + 1, 7: T + 1}),
        clean_text(5 * T, 9) + b"\r\n" * 1500,
        clean_text(70 * T, 9) + b"\n" * 3000,
    ]
    small = [clean_text(rng.randrange(0, 100), i) for i in range(300)]
    texts = large + sparse + small
    rng.shuffle(texts)
    n = len(texts)
    in_at = [rng.randrange(16) if len(t) < 60 * T else 0 for t in texts]
    out_at = [rng.randrange(4) for _ in texts]
    mine, twin = Hub(n), Hub(n)
    for rounds, (final, no_flags) in enumerate(((True, False), (False, True), (True, False))):
        items = [(s, t, final) for s, t in enumerate(texts)]
        got = mine.call(items, "pw", in_at=in_at, out_at=out_at, no_flags=no_flags)
        twin.call(items, "pieces", in_at=in_at, out_at=out_at, no_flags=no_flags)
        same_as_the_pieces_call(mine, twin, items)
        assert all(r[0] == OK for r, _ in got)
    mine.all_zero()
    twin.all_zero()
    # validate only, once: the same records, no byte written
    items = [(s, t, True) for s, t in enumerate(texts)]
    mine.call(items, "pw", validate_only=True, in_at=in_at)
    twin.call(items, "pieces", validate_only=True, in_at=in_at)
    same_as_the_pieces_call(mine, twin, items)


@gpu
def test_no_sid_and_no_flags():
    """d_sid NULL: piece i continues state i; d_flags NULL: none is final.
    Then the same states by a permutation, final."""
    b64 = _b64()
    rng = random.Random(5)
    texts = [clean_text(rng.choice((0, 1, 50, 700, T + 9, 3 * T + 77)), i, whole=False)
             for i in range(40)]
    tails = [b"QUJD"[:-len(strip(t)) % 4] + b"QQ==" for t in texts]
    n = len(texts)
    perm = list(range(n))
    rng.shuffle(perm)

    def run(how, parts, sid, flags, states):
        in_off = np.zeros(n + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=in_off[1:])
        x = _dev(b"".join(parts) + b"\xa5")
        d_in_off = torch.from_numpy(in_off).cuda()
        out_off = b64.skip_pieces_layout(d_in_off)
        size = int(out_off[-1])
        out = torch.full((size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        d_sid = None if sid is None else torch.tensor(sid, dtype=torch.int32, device="cuda")
        d_flags = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device="cuda")
        if how == "pw":
            need = ws_of(x.numel(), n)
            ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            b64.decode_strict_skip_pieces_wide(x, d_in_off, out, out_off, states[:n * STATE],
                                               res[:REC * n], ws[:need], sid=d_sid, flags=d_flags)
            assert bool((ws[need:] == FILL).all())
        else:
            b64.decode_strict_skip_pieces(x, d_in_off, out, out_off, states[:n * STATE], res[:REC * n],
                                          final=d_flags, sid=d_sid)
        torch.cuda.synchronize()
        assert bool((res[REC * n:] == FILL).all()) and bool((out[size:] == FILL).all())
        assert bool((states[n * STATE:] == FILL).all())
        return records(res)[:n], out.cpu().numpy(), out_off.cpu().numpy(), states.cpu().numpy()
    both_states = []
    for how in ("pw", "pieces"):
        states = torch.full((n * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        states[:n * STATE].zero_()
        ref = [RefState() for _ in range(n)]
        first = run(how, texts, None, None, states)
        second = run(how, [tails[s] for s in perm], perm, [1] * n, states)
        for i, t in enumerate(texts):
            want, data = ref_piece(ref[i], t, False)
            assert first[0][i] == want + (0,)
            assert first[1][first[2][i]:first[2][i] + want[2]].tobytes() == data
        for i, s in enumerate(perm):
            want, data = ref_piece(ref[s], tails[s], True)
            assert want[0] == OK and second[0][i] == want + (0,)
            assert second[1][second[2][i]:second[2][i] + want[2]].tobytes() == data
        assert not second[3][:n * STATE].any()
        both_states.append(first[3])
    assert both_states[0].tobytes() == both_states[1].tobytes()  # all 16 words, every state


def big_texts(seed: int, count: int):
    """Texts of 5T..9T bytes from random_texts: each of its small texts behind
    a clean body under the same alphabet with the skip set's bytes sprinkled
    in, so the small text's verdict decides."""
    rng = random.Random(seed)
    for t, skip, abc in random_texts(count, seed=seed):
        target = rng.randrange(5 * T + 100, 9 * T - 300)
        run = rng.choice((T + 1, 2 * T + 3)) if skip else 0
        nchars = ((target - run) * 60 // 61 if skip else target) // 4 * 4
        body = bytearray(plain(rng.randbytes(nchars // 4 * 3), abc))
        for _ in range(target - run - nchars if skip else 0):
            body.insert(rng.randrange(len(body) + 1), rng.choice(skip))
        if skip:
            p = rng.randrange(len(body))
            body[p:p] = bytes([skip[0]]) * run
        yield bytes(body) + t, skip, abc


def whole_text(t: bytes, skip, abc):
    """decode_strict_skip on the whole text: (record, bytes)."""
    b64 = _b64()
    x = _dev(t + b"\xa5")[:len(t)]
    out = torch.full((cap_of(len(t)) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC,), FILL, dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip(x, out=out, result=res, skip=skip, abc=abc)
    torch.cuda.synchronize()
    rec = records(res)[0]
    return rec, out[:rec[2]].cpu().numpy().tobytes()


def feed(streams, skip=CRLF, abc=STD, hows=("pw", "pieces", "one"), validate_only=False, seed=0):
    """Stream s (a list of pieces, the last one final) on state s: round r is
    one call with piece r of every stream that still has one, the calls taking
    turns.  Returns [[(record, bytes)]] per stream."""
    hub = Hub(len(streams), skip, abc)
    rng = random.Random(seed)
    out = [[] for _ in streams]
    for r in range(max(map(len, streams))):
        items = [(s, p[r], r == len(p) - 1) for s, p in enumerate(streams) if r < len(p)]
        in_at = [rng.randrange(16) for _ in items]
        out_at = [rng.randrange(4) for _ in items]
        got = hub.call(items, hows[r % len(hows)], validate_only=validate_only, in_at=in_at,
                       out_at=out_at)
        for (s, _, _), g in zip(items, got):
            out[s].append(g)
    hub.all_zero()
    return out


@gpu
@pytest.mark.parametrize("validate_only", [False, True])
def test_streams_take_turns(validate_only):
    """16 seeded texts cut at random points, the three calls taking turns on
    their states: every piece against ref_piece (in Hub.call), the
    concatenated bytes and the final record against decode_strict_skip on the
    whole text, the states zeroed at the end."""
    rng = random.Random(0xC14 + validate_only)
    groups = {}
    for t, skip, abc in big_texts(0x51E0, 16):
        pieces = cut(t, [rng.randrange(len(t) + 1) for _ in range(rng.randrange(2, 6))])
        groups.setdefault((skip, abc), []).append(pieces)
    kinds = set()
    for g, ((skip, abc), streams) in enumerate(groups.items()):
        hows = ("pw", "pieces", "one")[g % 3:] + ("pw", "pieces", "one")[:g % 3]
        got = feed(streams, skip, abc, hows, validate_only, seed=g)
        for pieces, rows in zip(streams, got):
            t = b"".join(pieces)
            assert [r for r, _ in rows] == [r + (0,) for r, _ in ref_stream(pieces, skip, abc)]
            rec, data = whole_text(t, skip, abc)
            assert rows[-1][0][:2] == rec[:2]
            kinds.add(rec[0])
            if rec[0] == OK:
                assert sum(r[2] for r, _ in rows) == rec[2]
                if not validate_only:
                    assert b"".join(d for _, d in rows) == data == skip_bytes(t, skip, abc)
    assert OK in kinds and len(kinds) >= 3


def offence_texts():
    """Texts of 3T + P + 5 bytes with one offence each -- CHAR, PAD and BITS at
    a tile's first and last byte and in the last three kept bytes, LENGTH --
    and with several, of which the lowest wins: [(text, its whole verdict)]."""
    L = 3 * T + P + 5
    b = b"\n" * 40 + clean_text(L - 40 - 30, 8) + b"\n" * 30
    assert len(b) == L and skip_ref(b)[0] == OK
    J, Q = 0x2A, 0x3D

    def ch(p):  # the nearest character at or after p
        while b[p] in CRLF:
            p += 1
        return p
    kept = [p for p in range(L) if b[p] not in CRLF]
    assert b[T - 1] not in CRLF and b[T] not in CRLF and b[2 * T - 1] not in CRLF
    spots = [[(T - 1, J)], [(T, J)], [(2 * T - 1, Q)], [(2 * T + 1, Q)], [(T, Q)],
             [(kept[-1], J)], [(kept[-2], J)], [(kept[-3], J)], [(kept[-3], Q)], [(kept[-2], Q)],
             # the lowest of several
             [(ch(70), Q), (ch(T + 3), J)], [(ch(70), J), (ch(T + 3), Q)],
             [(T - 1, J), (T, Q)], [(T - 1, Q), (T, J)],
             [(ch(3 * T + 9), J), (ch(2 * T + 100), J), (ch(T + 500), J), (ch(900), J)],
             [(ch(3 * T + 9), J), (ch(2 * T + 9), Q), (ch(T + 9), Q)]]
    texts = []
    for sp in spots:
        u = bytearray(b)
        for p, v in sp:
            u[p] = v
        texts.append(bytes(u))
    # BITS: Q R = = with R at a tile's last and first byte, and as the last kept bytes
    body = clean_text(40, 4)
    for at in (T - 1, T, 3 * T - 1):
        texts.append(body + b"Q" + b"\n" * (at - 41) + b"R=" + b"\n" * 5 + b"=" + b"\n" * (T + 9))
    texts.append(b[:kept[-4]] + b"QR==" + b[kept[-1] + 1:])
    # LENGTH: a character short
    texts.append(b[:kept[-1]] + b[kept[-1] + 1:])
    texts.append(b)
    out = [(t, skip_ref(t)) for t in texts]
    assert {w[0] for _, w in out} == ALL_KINDS
    for t, w in out[:len(spots)]:
        assert w[0] in (CHAR, PAD)
    assert [w[:2] for _, w in out[len(spots):len(spots) + 3]] == [(BITS, T - 1), (BITS, T), (BITS, 3 * T - 1)]
    return out


@gpu
def test_offences_are_found_kept_and_repeated():
    """Each text whole, and cut so that the offence stands in an earlier, a
    middle and the last piece; the report is sticky -- later pieces repeat it
    and write nothing -- and an offending piece's output stays untouched
    (Hub.call's mask)."""
    cases = offence_texts()
    rng = random.Random(77)
    for cuts, hows in (([], ("pw",)), ([T + 100, 2 * T + 50], ("pieces", "pw")),
                       ([T, T + 1], ("pw", "one", "pw")), ([5, 3 * T], ("pw",))):
        streams = [cut(t, cuts) for t, _ in cases]
        got = feed(streams, hows=hows, seed=rng.randrange(99))
        for (t, want), rows in zip(cases, got):
            assert rows[-1][0][:2] == want[:2], (cuts, hows, want)
            assert want[0] != OK or sum(r[2] for r, _ in rows) == want[2]
            seen = [r for r, _ in rows if r[0] != OK]
            assert all(r == seen[0] for r in seen)
            if want[0] == OK and rows[-1][1] is not None:
                assert b"".join(d for _, d in rows) == skip_bytes(t)


@gpu
def test_empty_pieces():
    """A final empty piece behind a carry of 1, 2 and 3; an empty piece that
    is not final changes nothing."""
    streams = [[b"QUJDQ", b"", b""], [b"QUJDQQ", b"", b""], [b"QUJDQUI", b"", b""], [b"", b"", b""],
               [b"QQ==", b"", b""], [b"QUI=", b"", b""], [b"\r\n", b"", b"QUJD"], [b"QUJD", b"", b"QQ=="]]
    hub = Hub(len(streams), CRLF, NOPAD)
    rows = [[] for _ in streams]
    for r in range(3):
        items = [(s, p[r], r == 2) for s, p in enumerate(streams)]
        before = hub.states[:hub.n * STATE].cpu().numpy().copy()
        got = hub.call(items, "pw", out_at=[s % 4 for s in range(len(items))])
        if r == 1:  # not final, empty: the states as they were
            assert hub.last[2].tobytes() == before.tobytes()
            assert [g[0] for g in got] == [(OK, 0, 0, 0)] * 4 + [(CHAR, 2, 0, 0), (CHAR, 3, 0, 0)] + \
                [(OK, 0, 0, 0)] * 2  # without pad, = is a stranger
        for s, g in enumerate(got):
            rows[s].append(g)
    hub.all_zero()
    assert rows[0][2][0] == (LENGTH, 5, 0, 0)
    assert rows[1][2] == ((OK, 0, 1, 0), b"A") and rows[2][2] == ((OK, 0, 2, 0), b"AB")
    assert rows[3][2] == ((OK, 0, 0, 0), b"")
    both(len(streams), [[(s, p[r], r == 2) for s, p in enumerate(streams)] for r in range(3)],
         abc=STD)


@gpu
def test_alphabets_and_skip_sets():
    """STD, URL, NOPAD and DOTPAD with skip sets of 1 and 8 bytes: texts of
    2T + 7 bytes and small ones, clean and with one byte replaced, cut at a
    seeded point, against ref_piece and the pieces call."""
    kinds = set()
    for abc in (STD, URL, NOPAD, DOTPAD):
        chars, pad, padc = alpha(abc)
        for skip in (b"\n", b" \t\r\n\x0b\x0c\x01\x02"):
            rng = random.Random(len(skip) + chars[62])
            streams = []
            for n in (0, 2, 3, 100, 2 * T + 7):
                nchars = (n - n // 40) // 4 * 4 if n > 3 else n
                base = bytearray(plain(_data(nchars // 4 * 3 + (0, 0, 1, 2)[nchars % 4], n + 9), abc)
                                 [:nchars if not pad else None])
                while len(base) < n:
                    base.insert(rng.randrange(len(base) + 1), rng.choice(skip))
                texts = [bytes(base)]
                for p in (0, T - 1, T, len(base) - 1, len(base) - 2) if n else ():
                    for v in (0x2A, padc, 0x0D, chars[63]):
                        u = bytearray(base)
                        u[p % len(u)] = v
                        texts.append(bytes(u))
                streams += [cut(t, [rng.randrange(len(t) + 1)]) for t in texts]
            kinds |= {skip_ref(b"".join(p), skip, abc)[0] for p in streams}
            calls = [[(s, p[r], r == 1) for s, p in enumerate(streams)] for r in range(2)]
            at = [(len(skip) + s) % 16 for s in range(len(streams))]
            got = both(len(streams), calls, skip, abc, in_at=at, out_at=[a % 4 for a in at])
            for s, p in enumerate(streams):
                want = skip_ref(b"".join(p), skip, abc)
                assert got[1][s][0][:2] == want[:2]
    assert kinds == ALL_KINDS


@gpu
@pytest.mark.parametrize("many", [True, False])
def test_bound(many):
    """total_cap one less than the pieces' bytes: every record {0, total,
    BOUND}; states, outputs, every guard and the bytes behind the workspace
    untouched.  A checked error path: nothing faults, nothing is retried."""
    b64 = _b64()
    rng = random.Random(8)
    parts = [clean_text(rng.choice((0, 1, 77, 900, T, 40 * T + 3)), i) for i in range(500)] if many \
        else [clean_text(2 * T + 100, 3)]
    n = len(parts)
    in_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=in_off[1:])
    total = int(in_off[-1])
    lead = 48  # in_off[0] is not 0: the bound is on the difference
    in_off += lead
    x = _dev(b"\xa5" * lead + b"".join(parts) + b"\xa5" * GUARD)
    d_in_off = torch.from_numpy(in_off).cuda()
    out_off = b64.skip_pieces_layout(d_in_off)
    out = torch.full((int(out_off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((GUARD + REC * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states = torch.full((GUARD + n * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    live = states[GUARD:GUARD + n * STATE]
    live.zero_()
    # armed states: a carry, and one that holds a report
    live.view(n, STATE)[:, 64:72] = torch.tensor([0x51, 0, 0, 1, 0x10, 0, 0, 0], dtype=torch.uint8)
    live.view(n, STATE)[0, 72:88] = torch.tensor([1] + [0] * 7 + [9] + [0] * 7, dtype=torch.uint8)
    before = states.cpu().numpy().copy()
    cap = total - 1
    need = ws_of(cap, n)
    ws = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    flags = torch.ones(n, dtype=torch.uint8, device="cuda")
    for o in (out, None):
        b64.decode_strict_skip_pieces_wide(x, d_in_off, o, None if o is None else out_off, live,
                                           res[GUARD:GUARD + REC * n], ws[GUARD:GUARD + need],
                                           total_cap=cap, flags=flags)
        torch.cuda.synchronize()
        assert records(res[GUARD:GUARD + REC * n]) == [(BOUND, total, 0, 0)] * n
        r = res.cpu().numpy()
        assert (r[:GUARD] == FILL).all() and (r[GUARD + REC * n:] == FILL).all()
        assert (out.cpu().numpy() == FILL).all(), "an output byte was written"
        assert states.cpu().numpy().tobytes() == before.tobytes(), "a state was touched"
        w = ws.cpu().numpy()
        assert (w[:GUARD] == FILL).all() and (w[GUARD + need:] == FILL).all()
        assert (w[GUARD + 64:GUARD + need] == FILL).all(), "only the control words are written"
        res.fill_(FILL)
    # with the bound met the same buffers decode
    live.zero_()
    b64.decode_strict_skip_pieces_wide(x, d_in_off, out, out_off, live, res[GUARD:GUARD + REC * n],
                                       ws[GUARD:GUARD + ws_of(total, n)] if ws_of(total, n) <= need
                                       else torch.empty(ws_of(total, n), dtype=torch.uint8, device="cuda"),
                                       total_cap=total, flags=flags)
    torch.cuda.synchronize()
    got = records(res[GUARD:GUARD + REC * n])
    o = out.cpu().numpy()
    offs = out_off.cpu().numpy()
    for i, p in enumerate(parts):
        data = decode_kept(strip(p))
        assert got[i] == (OK, 0, len(data), 0)
        assert o[offs[i]:offs[i] + len(data)].tobytes() == data


@gpu
def test_graph_capture():
    """One captured call of 6 pieces, replayed after offsets, flags, state
    indices and text have been rewritten within the same total_cap -- a piece
    grows from 1 tile to 300 -- against a direct call and the pieces call on
    twin states, and the stdlib."""
    b64 = _b64()
    n = 6
    lines = (300 * T + 8 * T) // 78
    size = lines * 78
    x = torch.full((size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    cap_all = cap_of(size)
    in_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out_off = torch.arange(n, dtype=torch.int64, device="cuda") * (_up16(cap_all) + GUARD) + GUARD + 3
    osize = n * (_up16(cap_all) + GUARD) + GUARD
    sid = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    need = ws_of(size, n)
    assert tile_of(size) == T

    class Side:
        def __init__(self):
            self.states = torch.full((n * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            self.states[:n * STATE].zero_()
            self.out = torch.full((osize,), FILL, dtype=torch.uint8, device="cuda")
            self.res = torch.full((REC * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            self.ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")

        def pw(self):
            b64.decode_strict_skip_pieces_wide(x[:size], in_off, self.out, out_off,
                                               self.states[:n * STATE], self.res[:REC * n],
                                               self.ws[:need], total_cap=size, sid=sid, flags=flags)

        def pieces(self):
            b64.decode_strict_skip_pieces(x[:size], in_off, self.out, out_off, self.states[:n * STATE],
                                          self.res[:REC * n], final=flags, sid=sid)

        def look(self):
            assert bool((self.res[REC * n:] == FILL).all()) and bool((self.ws[need:] == FILL).all())
            assert bool((self.states[n * STATE:] == FILL).all())
            return records(self.res)[:n], self.out.cpu().numpy(), self.states[:n * STATE].cpu().numpy()
    graphed, direct, twin = Side(), Side(), Side()

    def write(text_seed, edges, sids, finals, spoil=None):
        a = np.roll(np.tile(np.frombuffer(crlf76(_data(57, text_seed)), np.uint8), lines), 0)
        if spoil is not None:
            a = a.copy()
            a[spoil] = 0x2A
        x[:size].copy_(torch.from_numpy(a))
        in_off.copy_(torch.tensor([78 * e for e in edges], dtype=torch.int64))
        sid.copy_(torch.tensor(sids, dtype=torch.int32))
        flags.copy_(torch.tensor(finals, dtype=torch.uint8))
        return a.tobytes()
    first = ([0, 10, 20, 60, 61, 61, 100], list(range(n)), [1] * n)
    write(1, *first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graphed.pw()  # warm-up; every piece final: the states end zeroed
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            graphed.pw()
    grown = [0, 3, 3, 3 + 300 * T // 78 + 1, lines - 40, lines - 1, lines]
    assert tiles_of(78 * (grown[3] - grown[2]), 78 * grown[2] % 16) >= 300
    spoil_at = 78 * 3 + 150 * T + 1
    plans = [(1, *first, None), (2, grown, [4, 2, 0, 5, 1, 3], [0] * n, None),
             (3, grown, [4, 2, 0, 5, 1, 3], [1, 1, 0, 1, 0, 1], spoil_at),
             (4, [0, 40, 80, 81, 90, 95, 99], [5, 4, 3, 2, 1, 0], [1] * n, None)]
    for seed, edges, sids, finals, spoil in plans:
        text = write(seed, edges, sids, finals, spoil)
        for s in (graphed, direct, twin):
            s.out.fill_(FILL)
            s.res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        direct.pw()
        twin.pieces()
        torch.cuda.synchronize()
        (r0, o0, s0), (r1, o1, s1), (r2, o2, s2) = graphed.look(), direct.look(), twin.look()
        assert r0 == r1 == r2
        assert o0.tobytes() == o1.tobytes() and s0.tobytes() == s1.tobytes()
        offs = out_off.cpu().numpy()
        mask = np.ones(o0.size, bool)
        for i in range(n):
            piece = text[78 * edges[i]:78 * edges[i + 1]]
            bad = spoil is not None and 78 * edges[i] <= spoil < 78 * edges[i + 1]
            held = seed == 4 and sids[i] == 0  # the spoiled piece was not final: its state holds the report
            if bad or held:
                assert r0[i] == (CHAR, spoil_at - 78 * 3 + 78 * (grown[3] - grown[2]), 0, 0)
                continue
            data = decode_kept(strip(piece))
            assert r0[i] == (OK, 0, len(data), 0)
            assert o0[offs[i]:offs[i] + len(data)].tobytes() == data
            assert o2[offs[i]:offs[i] + len(data)].tobytes() == data
            mask[offs[i]:offs[i] + cap_of(len(piece))] = False
            a, b = (s[sids[i] * STATE:(sids[i] + 1) * STATE] for s in (s0, s2))
            assert a.tobytes() == b.tobytes()
        assert (o0[mask] == FILL).all()
    assert not graphed.look()[2].any()


@gpu
def test_past_4gib():
    """The pieces start 4 GiB + 64 into one buffer, and their outputs past
    4 GiB into another: 64-bit offsets, a bound on their difference only.
    The memory in front is never touched (and never written by the test)."""
    b64 = _b64()
    far = (1 << 32) + 64
    free, _ = torch.cuda.mem_get_info()
    assert free > 2 * far + (1 << 30), "the device has no room for offsets past 2^32"
    parts = [clean_text(n, n) for n in (1538, 0, 5 * T + 9, 77, 70 * T)]
    n = len(parts)
    body = b"".join(parts)
    x = torch.empty(far + len(body) + GUARD, dtype=torch.uint8, device="cuda")
    x[far - GUARD:far].fill_(FILL)
    x[far:far + len(body)].copy_(_dev(body))
    x[far + len(body):].fill_(FILL)
    edges = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=edges[1:])
    d_in_off = torch.from_numpy(edges + far).cuda()
    rel = b64.skip_pieces_layout(d_in_off).cpu().numpy()
    osize = int(rel[-1])
    out = torch.empty(far + osize + GUARD, dtype=torch.uint8, device="cuda")
    out[far - GUARD:].fill_(FILL)
    out_off = torch.from_numpy(rel + far).cuda()
    states = torch.full((n * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states[:n * STATE].zero_()
    res = torch.full((REC * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    need = ws_of(len(body), n)
    ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    flags = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip_pieces_wide(x, d_in_off, out, out_off, states[:n * STATE], res[:REC * n],
                                       ws[:need], total_cap=len(body), flags=flags)
    torch.cuda.synchronize()
    got = records(res)[:n]
    o = out[far - GUARD:].cpu().numpy()
    mask = np.ones(o.size, bool)
    for i, p in enumerate(parts):
        data = decode_kept(strip(p))
        assert got[i] == (OK, 0, len(data), 0)
        at = GUARD + int(rel[i])
        assert o[at:at + len(data)].tobytes() == data
        mask[at:at + len(data)] = False
    assert (o[mask] == FILL).all()
    s = states.cpu().numpy()
    assert not s[:2 * STATE].any() and not s[3 * STATE:n * STATE].any() and (s[n * STATE:] == FILL).all()
    w = s[2 * STATE:3 * STATE].view(np.uint64)
    assert w[0] == len(parts[2]) and w[1] == len(strip(parts[2])) and not w[9:].any()
    assert bool((res[REC * n:] == FILL).all()) and bool((ws[need:] == FILL).all())
    del x, out
    torch.cuda.empty_cache()
