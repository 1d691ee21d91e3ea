"""Strict skip decode of one large piece, spread over the GPU
(b64x_decode_strict_skip_piece_dev, async_amd.b64.decode_strict_skip_piece):
every record, every piece's bytes and every state, bit for bit, against the
chunked scalar procedure of tests/test_decode_strict_skip_pieces.py (ref_piece,
ref_stream), the whole-text references of tests/test_decode_strict_skip.py
(skip_ref, skip_bytes) and the two GPU calls the unit stands next to
(decode_strict_skip_pieces on the same single piece, decode_strict_skip on the
whole text).  The new call is never compared with itself.

The unit's tile rule (async_amd/csrc/b64x_skip_wide_plan.h), restated: a piece
of len bytes is cut into tiles of
    T(len) = max(4,096, ceil(ceil((len + 15) / 16,384) / 1,024) * 1,024)
bytes of address span from the 16-byte floor of its address -- T = 4,096 for
every piece below 64 MiB -- which a wave walks in passes of P = 1,024 bytes; the
workspace is a head of 64 bytes and 64 bytes for each of the
ceil((len + 15) / T) tiles the worst alignment gives.  The scan runs in one
workgroup of 256 lanes, a strip of ceil(tiles / 256) consecutive records to a
lane, loaded four at a time.

CPU tests: the exports and their signatures, every -EINVAL case in its order,
-ENODEV without a device, the wrapper's ValueErrors, the workspace size against
the rule above, the new code object's kernels and barriers, and the launch plan
as a host program under ASan + UBSan.

GPU tests: every output capacity stands between 64 guard bytes, a guard stands
behind the record, the state and the workspace (which is handed over full of
0xA5: it needs no preparation), and 64 bytes of 0xA5 -- a stranger under every
alphabet here -- stand on both sides of the text, so that a byte read outside
it shows up as CHAR.
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
from tests.test_decode_strict import BITS, CHAR, FILL, GUARD, LENGTH, OK, PAD, REC, plain
from tests.test_decode_strict_skip import (CRLF, DOTPAD, NOPAD, STD, URL, crlf76, random_texts,
                                           records, skip_bytes, skip_ref)
from tests.test_decode_strict_skip_pieces import RefState, cap_of, cut, ref_piece, ref_stream

ROOT = util.ROOT
T, P = 4096, 1024
MAX_TILES = 16384
HEAD = RECORD = 64
LANES, TH = 64, 256
STATE = 128
ALL_KINDS = {OK, CHAR, PAD, BITS, LENGTH}
NAME = "b64x_decode_strict_skip_piece_dev"
SIZE = "b64x_strict_skip_piece_workspace_size"


def tile_of(n: int) -> int:
    per = -(-(n + 15) // MAX_TILES)
    return max(T, -(-per // P) * P)


def ws_of(n: int) -> int:
    return HEAD + RECORD * -(-(n + 15) // tile_of(n))


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


def text_of(n: int, seed: int = 1) -> bytes:
    """An accepted CRLF-76 text of exactly n bytes: the encoder's text of as
    much payload as fits, then line feeds."""
    m = n * 57 // 78
    while m and len(crlf76(_data(m, seed))) > n:
        m -= 1
    t = crlf76(_data(m, seed)) if m else b""
    return t + b"\n" * (n - len(t))


def spread(chars: bytes, gaps: dict) -> bytes:
    """chars with gaps[i] line feeds in front of chars[i] (i == len: behind)."""
    out = bytearray()
    for i, c in enumerate(chars):
        out += b"\n" * gaps.get(i, 0)
        out.append(c)
    return bytes(out + b"\n" * gaps.get(len(chars), 0))


# ----------------------------------------------------------------- CPU --

def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    assert hasattr(lib, NAME) and hasattr(lib, SIZE)
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 10 and getattr(lib, NAME).argtypes == args and res is ctypes.c_int
    res, args = _lib.SIGNATURES[SIZE]
    assert args == [ctypes.c_uint64, ctypes.c_bool] and res is ctypes.c_uint64
    header = open(os.path.join(ROOT, "include", "b64x.h")).read()
    assert re.search(r"^int b64x_decode_strict_skip_piece_dev\(", header, re.M)
    assert re.search(r"^uint64_t b64x_strict_skip_piece_workspace_size\(uint64_t len, "
                     r"bool validate_only\);", header, re.M)
    assert "#define B64X_ABI_VERSION 7" in header and b"abi=7" in lib.b64x_build_info()
    from async_amd import b64
    for name in ("decode_strict_skip_piece", "strict_skip_piece_workspace_size"):
        assert name in b64.__doc__ and callable(getattr(b64, name))


def _host_call():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def call(skip=None, abc=None, d_in=p, n=100, d_out=p, state=p + 1024, flags=0, d_res=p + 2048,
             ws=p + 3072):
        return lib.b64x_decode_strict_skip_piece_dev(d_in, n, d_out, state, flags, d_res, ref(abc),
                                                     ref(skip), ws, None)
    return lib, p, call


def test_invalid_arguments_in_their_order():
    lib, p, call = _host_call()
    nodev = lib.b64x_device_check() == -19

    def raw(n, b):
        return _lib.Skip(n, (ctypes.c_uint8 * 8)(*b))
    a = _lib.alphabet()
    bad_abc = _lib.alphabet("+", "+")
    nine = raw(9, b"\r\n\t \x0b\x0c\x00\x01")
    # 1. NULL pointers and the alignment of record, state and workspace, before everything else
    for kw in ({"d_in": None}, {"state": None}, {"d_res": None}, {"ws": None}, {"d_res": p + 4},
               {"state": p + 1028}, {"ws": p + 3076}, {"d_in": None, "n": 0}):
        assert call(**kw) == -22, kw
        assert call(nine, bad_abc, flags=2, **kw) == -22, kw
        assert call(d_out=None, **kw) == -22, kw
    # 2. the flags, before the skip set and the alphabet
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == -22
        assert call(nine, bad_abc, flags=flags) == -22
    # 3. the skip set, before the alphabet
    for skip, abc in ((nine, a), (raw(1, b"A"), a), (raw(2, b"\n="), a), (raw(2, b"\n+"), a),
                      (raw(1, b"_"), _lib.alphabet("-", "_")), (nine, bad_abc), (raw(1, b"z"), bad_abc)):
        assert call(skip, abc) == -22
        assert call(skip, abc, d_out=None, flags=1) == -22
    # 4. the alphabet rules of the strict decoder
    for abc in (bad_abc, _lib.alphabet("A", "/"), _lib.alphabet(padchar="A"),
                _lib.alphabet("-", "_", True, "_")):
        assert call(None, abc) == -22
        assert call(None, abc, d_out=None) == -22
    # 5. valid calls reach the device check (with a device these host pointers
    # must never reach a kernel, so the calls are not made)
    if nodev:
        for kw in ({}, {"d_out": None}, {"flags": 1}, {"n": 0}, {"n": (1 << 40) + 1},
                   {"skip": raw(0, b"")}, {"skip": raw(1, b"="), "abc": _lib.alphabet(pad=False)},
                   {"d_in": p + 1, "d_out": p + 3, "state": p + 1032, "d_res": p + 2056}):
            assert call(**kw) == -19, kw


def test_wrapper_value_errors():
    """What the wrapper refuses without a device: tensors that are not on one,
    and a skip set of nine bytes (test_wrapper_size_errors makes the size
    checks, on device tensors)."""
    from async_amd import b64
    cpu = torch.zeros(4096, dtype=torch.uint8)
    state = torch.zeros(STATE, dtype=torch.uint8)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_piece(cpu, state, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_piece(cpu, state, cpu, out=cpu, final=True)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_piece(cpu, state, cpu, skip=b"123456789")


def test_workspace_size():
    lib = _lib.load()
    from async_amd import b64
    assert tile_of(0) == tile_of(T * MAX_TILES - 15) == T and tile_of(T * MAX_TILES - 14) == T + P
    for n, want in ((0, 128), (1, 128), (T - 1, 192), (T, 192), (T + 1, 192), (T - 15, 128),
                    (T - 14, 192), (1 << 32, 64 + 64 * 16321), (1 << 40, 64 + 64 * 16384)):
        for validate_only in (False, True):
            assert lib.b64x_strict_skip_piece_workspace_size(n, validate_only) == want == ws_of(n), n
            assert b64.strict_skip_piece_workspace_size(n, validate_only) == want
    assert tile_of(1 << 32) == 257 * P and tile_of(1 << 40) == (1 << 26) + P
    for n in (T * MAX_TILES - 15, T * MAX_TILES - 14, (1 << 64) - 1, (1 << 64) - 16):
        assert lib.b64x_strict_skip_piece_workspace_size(n, False) == ws_of(min(n, (1 << 64) - 16))
        assert ws_of(n) <= HEAD + RECORD * MAX_TILES


# The kernels of b64x_skip_wide.hip; nothing else may be in its code object.
WIDE_KERNELS = {"k_skip_wide_count", "k_skip_wide_scan", "k_skip_wide_decode"}


def test_wide_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_skip_wide.o"))
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
    assert isa_check.barrier_count(dis) == len(WIDE_KERNELS)  # one each


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    """tests/csrc/skip_wide_plan_check.cpp built with the host compiler under
    ASan + UBSan: a stand-alone program, run as a child process.  The
    sanitizers' runtimes are linked into the program itself."""
    exe = str(tmp_path_factory.mktemp("plan") / "skip_wide_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "async_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "skip_wide_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def test_plan_program_matches_the_python_formulas(plan_program):
    top = (1 << 64) - 1
    lens = [0, 1, 15, 16, 17, T - 16, T - 15, T - 14, T, T + 1, 3 * T + P + 5, T * MAX_TILES - 15,
            T * MAX_TILES - 14, (1 << 32) - 1, 1 << 32, (1 << 32) + T + 5, 1 << 40, (1 << 63) + 3,
            top - 16, top - 15, top - 14, top]
    rng = random.Random(7)
    lens += [rng.randrange(1 << rng.randrange(1, 64)) for _ in range(300)]
    queries = [(n, head, cus) for n in lens for head in (0, 1, 15) for cus in (1, 256)]
    run = subprocess.run([plan_program], input="".join("%d %d %d\n" % q for q in queries),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
    assert len(rows) == len(queries)
    for (n, head, cus), (tile, tiles, ws, grid) in zip(queries, rows):
        span = min(n + 15, top)
        want_tile = max(T, -(-(-(-span // MAX_TILES)) // P) * P)
        want_tiles = 1 if n == 0 else -(-min(n + head, top) // want_tile)
        assert tile == want_tile and tile % P == 0, (n, head)
        assert tiles == want_tiles and 1 <= tiles <= MAX_TILES, (n, head)
        assert ws == HEAD + RECORD * -(-span // want_tile) >= HEAD + RECORD * tiles, (n, head)
        assert grid == min(-(-tiles // 4), 8 * cus) >= 1


# ----------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


def _dev(b: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


class Lane:
    """One state on the device, a guard behind it, and its reference state."""

    def __init__(self):
        self.all = torch.full((STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.state = self.all[:STATE]
        self.state.zero_()
        assert self.state.data_ptr() % 8 == 0
        self.ref = RefState()


def place(piece: bytes, at: int = 0):
    """The piece at an address that is `at` mod 16, strangers on both sides:
    (the buffer, the piece's view)."""
    n = len(piece)
    buf = torch.full((GUARD + 16 + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    start = GUARD + (at - GUARD) % 16
    if n:
        buf[start:start + n].copy_(_dev(piece))
    return buf, buf[start:start + n]


def one_call(lane, x, final, how, validate_only=False, out_at=0, skip=CRLF, abc=STD,
             untouched=False):
    """One piece (a device view) on the lane's state by the wide call or by
    the pieces call: ((err, err_pos, out_len, reserved), the capacity's bytes,
    the 128 state bytes); every guard is checked here.  untouched: the whole
    output must stay as it was."""
    b64 = _b64()
    n = x.numel()
    cap = 0 if validate_only else cap_of(n)
    out = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    o = GUARD + out_at
    outv = None if validate_only else out[o:o + cap]
    res = torch.full((REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    if how == "wide":
        need = ws_of(n)
        ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        b64.decode_strict_skip_piece(x, lane.state, res[:REC], out=outv, final=final, skip=skip,
                                     abc=abc, workspace=ws[:need])
    else:
        b64.decode_strict_skip_pieces(
            x, torch.tensor([0, n], dtype=torch.int64, device="cuda"), outv,
            None if validate_only else torch.zeros(1, dtype=torch.int64, device="cuda"),
            lane.state, res[:REC],
            final=torch.tensor([1 if final else 0], dtype=torch.uint8, device="cuda"),
            skip=skip, abc=abc)
    torch.cuda.synchronize()
    rec = records(res)[0]
    got = out.cpu().numpy()
    st = lane.all.cpu().numpy()
    assert (res[REC:].cpu().numpy() == FILL).all(), "the guard behind the record"
    assert (st[STATE:] == FILL).all(), "the guard behind the state"
    if how == "wide":
        assert (ws[need:].cpu().numpy() == FILL).all(), "the guard behind the workspace"
    assert (got[:o] == FILL).all() and (got[o + cap:] == FILL).all(), "outside the capacity"
    if validate_only or untouched:
        assert (got == FILL).all(), "an output byte was written"
    if final:
        assert not st[:STATE].any(), "a final piece left its state armed"
    return rec, got[o:o + cap], st[:STATE].copy()


def run_stream(pieces, hows=None, validate_only=False, in_at=0, out_at=0, skip=CRLF, abc=STD):
    """The pieces of one text, the last one final, on one state: piece i by
    hows[i] ("wide" where None), checked against ref_piece, and against a twin
    state that the pieces call alone drives: its records, its bytes and, where
    the contract pins it, its state.  Returns [(record, bytes or None)]."""
    hows = hows or ["wide"] * len(pieces)
    main, twin = Lane(), Lane()
    result = []
    for i, (piece, how) in enumerate(zip(pieces, hows)):
        final = i == len(pieces) - 1
        had_report = main.ref.report is not None
        want, data = ref_piece(main.ref, piece, final, skip, abc)
        buf, x = place(piece, in_at)
        label = (i, len(piece), piece[:16], final, how, in_at, out_at, skip, abc, validate_only)
        kw = dict(validate_only=validate_only, out_at=out_at, skip=skip, abc=abc)
        rec, got, st = one_call(main, x, final, how, untouched=had_report and how == "wide", **kw)
        assert rec == (want[0], want[1], want[2], 0), (label, rec, want)
        if data is not None and not validate_only:
            assert got[:want[2]].tobytes() == data, label
        rec2, got2, st2 = one_call(twin, x, final, "pieces", **kw)
        assert rec2 == rec, label
        if data is not None and not validate_only:
            assert got2[:want[2]].tobytes() == data, label
        if final:
            assert not st.any() and not st2.any(), label
        elif want[0] == OK:
            assert st.tobytes() == st2.tobytes(), (label, st.view(np.uint64), st2.view(np.uint64))
        else:
            assert st[72:88].tobytes() == st2[72:88].tobytes(), label  # words 9 and 10: the report
        result.append((rec, None if validate_only or data is None else data))
    assert main.ref.is_zero()
    return result


def check_whole(t: bytes, got, skip=CRLF, abc=STD):
    """A stream's results against the whole-text references."""
    want = skip_ref(t, skip, abc)
    assert got[-1][0][:2] == want[:2], (got[-1][0], want)
    if want[0] == OK:
        assert sum(r[2] for r, _ in got) == want[2]
        if got[-1][1] is not None:
            assert b"".join(d for _, d in got) == skip_bytes(t, skip, abc)
    return want[0]


@gpu
def test_wrapper_size_errors():
    """The wrapper's size and type checks: no call reaches the library."""
    b64 = _b64()
    x = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    state = b64.skip_states(1)
    res = torch.zeros(REC, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(ws_of(1000) + 8, dtype=torch.uint8, device="cuda")
    ok = dict(x=x, state=state, result=res, out=x, workspace=ws)
    for kw in ({"result": res[:REC - 1]}, {"state": b64.skip_states(2)}, {"state": state[:STATE - 1]},
               {"state": b64.skip_states(2)[4:4 + STATE]}, {"out": x[:cap_of(1000) - 1]},
               {"workspace": ws[:ws_of(1000) - 1]}, {"workspace": ws[4:]}, {"x": x.int()},
               {"out": x.cpu()}):
        with pytest.raises(ValueError):
            b64.decode_strict_skip_piece(**{**ok, **kw})


@gpu
def test_tile_and_pass_edges():
    """One final piece on a zero state, CRLF-76 text, at every input address
    mod 16 and output address mod 4: skip_ref / skip_bytes, the pieces call on
    that one piece (run_stream's twin) and decode_strict_skip."""
    b64 = _b64()
    lens = [0, 1, 15, 16, 17, P - 1, P + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T + P + 5]
    ws = torch.zeros(b64.strict_skip_workspace_size(max(lens)), dtype=torch.uint8, device="cuda")
    for n in lens:
        t = text_of(n, n + 1)
        want = skip_ref(t)
        data = skip_bytes(t)
        assert len(t) == n and want == (OK, 0, len(data))
        for in_at in range(16):
            out_at = (in_at + in_at // 4) % 4
            got = run_stream([t], in_at=in_at, out_at=out_at)
            assert got == [((OK, 0, want[2], 0), data)], (n, in_at)
            buf, x = place(t, in_at)
            out = torch.full((GUARD + cap_of(n),), FILL, dtype=torch.uint8, device="cuda")
            res = torch.full((REC,), FILL, dtype=torch.uint8, device="cuda")
            b64.decode_strict_skip(x, out=out[out_at:], workspace=ws, result=res)
            torch.cuda.synchronize()
            assert records(res)[0] == got[0][0]
            assert out[out_at:out_at + want[2]].cpu().numpy().tobytes() == got[0][1]


CHARS16 = plain(_data(10, 3))  # 14 data characters and ==


@gpu
def test_the_carry_between_tiles():
    """Data characters sparse around tile edges: runs of line feeds longer
    than T, 2T and 3T + 1, so that tiles hold 0, 1 and 2 data characters and a
    tile's carry comes from up to four tiles back and from the state."""
    assert len(CHARS16) == 16 and CHARS16.endswith(b"==")
    texts = [
        spread(CHARS16, {5: T + 3, 6: 2 * T + 1, 8: 3 * T + 1, 9: T, 11: T + 7}),
        spread(CHARS16, {0: T, 3: 3 * T + 2, 4: 1, 5: T + 1, 6: T + 1, 7: 2 * T + 5, 14: T, 16: T}),
        spread(CHARS16, {1: 4 * T, 2: T - 1, 3: T - 1, 13: T + 1, 14: 3, 15: T}),
        # a final partial group of three sextets, each in a tile of its own
        spread(b"QUJDQUI=", {5: T + 1, 6: 2 * T + 1, 7: T + 1}),
        spread(b"QUJDQQ==", {5: 3 * T + 1, 6: T, 7: 2}),
    ]
    for t in texts:
        data = skip_bytes(t)
        assert skip_ref(t) == (OK, 0, len(data))
        for in_at in (0, 5):
            got = run_stream([t], in_at=in_at, out_at=in_at % 4)
            assert got[0][1] == data
            # the same text in pieces: a carry from the state, and a partial
            # group whose sextets lie in the piece before
            at = [i for i, b in enumerate(t) if b != 0x0A]
            first = at + [at[-1]] * 16
            for points in ([first[1]], [first[2], first[6] + 1], [first[3], first[3] + T // 2],
                           [first[5], first[7]], [first[9] + 1, len(t) - 1]):
                pieces = cut(t, points)
                for hows in (None, ["pieces"] + ["wide"] * (len(pieces) - 1)):
                    got = run_stream(pieces, hows, in_at=in_at)
                    assert check_whole(t, got) == OK
    # a piece of skipped bytes only, behind a carry of 1, 2 and 3, final and not
    for c in (1, 2, 3):
        u = b"QUJD" + (b"Q", b"QQ", b"QUI")[c - 1]
        for run in (5, T + 5):
            got = run_stream([u, b"\n" * run, (b"UJD", b"==", b"=")[c - 1]])
            assert [r[2] for r, _ in got] == [3, 0, (3, 1, 2)[c - 1]]
            got = run_stream([u, b"\n" * run], abc=NOPAD)
            assert got[-1][0] == ((LENGTH, 5 + run, 0, 0) if c == 1 else (OK, 0, c - 1, 0))
            if c > 1:
                assert got[-1][1] == b"AB"[:c - 1]
            got = run_stream([u, b"\n" * run, b""], ["pieces", "wide", "wide"], abc=NOPAD)
            assert got[-1][0][0] == (LENGTH if c == 1 else OK)


@gpu
def test_the_tail_and_bits():
    """The last three kept bytes spread over three tiles and over the earlier
    piece; BITS whose offender stands in an earlier tile and in an earlier
    piece; the pads split across a tile edge and across a piece edge."""
    body = plain(_data(30, 4))  # 40 data characters
    assert len(body) == 40 and b"=" not in body
    # Q R = = with a tile between any two of them: BITS at R
    t = spread(body + b"QR==", {41: T + 1, 42: T + 9, 43: 2 * T, 44: T + 2})
    at_r = 40 + 1 + T + 1
    assert skip_ref(t) == (BITS, at_r, 0)
    for in_at in (0, 9):
        assert run_stream([t], in_at=in_at)[0][0] == (BITS, at_r, 0, 0)
        for points in ([at_r + 1], [at_r + 1, len(t) - 3], [at_r - 2, at_r + T], [len(t) - T - 3],
                       [at_r, at_r + 1, at_r + 2]):
            for hows in (None, ["pieces"] + ["wide"] * len(points)):
                got = run_stream(cut(t, points), hows, in_at=in_at)
                assert got[-1][0] == (BITS, at_r, 0, 0)
    # a clean tail spread the same way
    u = spread(body + b"QQ==", {41: T + 1, 42: T + 9, 43: 2 * T, 44: T + 2})
    assert skip_ref(u) == (OK, 0, 31)
    for points in ([], [at_r + 1], [at_r + T, len(u) - 1]):
        assert check_whole(u, run_stream(cut(u, points))) == OK
    # = | = at a tile edge (the text at a 16-byte boundary), skipped bytes between and behind
    for between, behind in ((0, 0), (0, 3), (2, T + 1), (T + 1, 2)):
        v = body + b"QQ" + b"\n" * (T - 1 - 42) + b"=" + b"\n" * between + b"=" + b"\n" * behind
        assert v[T - 1] == 0x3D and skip_ref(v) == (OK, 0, 31)
        for points in ([], [T - 1], [T], [T + between], [T + between + 1], [T - 1, T + between],
                       [41, T, len(v)]):
            for hows in (None, ["pieces"] + ["wide"] * len(points)):
                assert check_whole(v, run_stream(cut(v, points), hows)) == OK
    # a pad character with data behind it, a tile further on: PAD at the pad
    v = body + b"QQ=" + b"\n" * (T + 5) + b"QUJD"
    assert skip_ref(v) == (PAD, 42, 0)
    for points in ([], [43], [T], [43, T + 40]):
        assert run_stream(cut(v, points))[-1][0] == (PAD, 42, 0, 0)


@gpu
def test_lowest_offence_wins():
    L = 3 * T + P + 5
    b = b"\n" * 40 + text_of(L - 40 - 30, 8) + b"\n" * 30
    assert len(b) == L and skip_ref(b)[0] == OK
    J, Q = 0x00, 0x3D

    def ch(p):  # the nearest character at or after p
        while b[p] in CRLF:
            p += 1
        return p
    spots = [
        [(ch(70), Q), (ch(T + 3), J)],                       # a pad a tile before a stranger
        [(ch(70), J), (ch(T + 3), Q)],
        [(ch(T - 2), J), (ch(T + 2), Q)],                    # either side of a tile edge
        [(ch(T - 2), Q), (ch(T + 2), J)],
        [(ch(3 * T + 9), J), (ch(2 * T + 100), J), (ch(T + 500), J), (ch(900), J)],
        [(ch(900), J), (ch(T + 500), J), (ch(3 * T + P + 1 - 40), J)],
        [(ch(3 * T + 9), J), (ch(2 * T + 9), Q), (ch(T + 9), Q)],
        [(ch(P + 3), J), (ch(P - 20), Q)],                   # one tile, across its pass edge
    ]
    cuts = [T + 100, 2 * T + 50]
    for sp in spots:
        u = bytearray(b)
        for p, v in sp:
            u[p] = v
        first = min(sp)
        want = (PAD if first[1] == Q else CHAR, first[0], 0)
        assert skip_ref(bytes(u)) == want
        for in_at in (0, 11):
            assert run_stream([bytes(u)], in_at=in_at)[0][0] == want + (0,)
        # the same across pieces; the piece after a report, not final and then
        # final, gets the record again and leaves its output untouched
        for hows in (None, ["pieces", "wide", "wide"], ["wide", "pieces", "wide"]):
            got = run_stream(cut(bytes(u), cuts), hows, in_at=3)
            assert got[-1][0] == want + (0,)
            seen = [r for r, _ in got if r[0] != OK]
            assert seen and all(r == want + (0,) for r in seen)
        got = run_stream(cut(bytes(u), [first[0] + 1, first[0] + 1 + T, first[0] + 2 * T]))
        assert [r for r, _ in got][1:] == [want + (0,)] * 3


def big_texts(seed: int, count: int):
    """Texts of 5T..9T bytes from random_texts: each of its small texts behind
    a clean body under the same alphabet with the skip set's bytes sprinkled
    in, so the small text's verdict decides; every eighth body gets a stranger
    or a pad character of its own."""
    rng = random.Random(seed)
    for i, (t, skip, abc) in enumerate(random_texts(count, seed=seed)):
        target = rng.randrange(5 * T + 100, 9 * T - 300)
        run = rng.choice((T + 1, 2 * T + 3)) if skip else 0
        nchars = ((target - run) * 60 // 61 if skip else target) // 4 * 4
        body = bytearray(plain(rng.randbytes(nchars // 4 * 3), abc))
        assert len(body) == nchars
        for _ in range(target - run - nchars if skip else 0):
            body.insert(rng.randrange(len(body) + 1), rng.choice(skip))
        if skip:
            p = rng.randrange(len(body))
            body[p:p] = bytes([skip[0]]) * run
        if i % 8 == 7:
            p = rng.randrange(len(body) // 2)
            while skip and body[p] in skip:
                p += 1
            body[p] = rng.choice(b"=.\x00*")
        yield bytes(body) + t, skip, abc


BIG_SEED, BIG_COUNT = 0x51DF, 40


@gpu
@pytest.mark.parametrize("validate_only", [False, True])
def test_interleaving_with_the_pieces_call(validate_only):
    """Each piece is dealt to the wide call or to the pieces call by a seeded
    coin, on one state; run_stream compares every record and every piece's
    bytes with ref_piece and, after each piece that is not final and has no
    offence, the 128 state bytes with the twin the pieces call alone drives."""
    rng = random.Random(0xC01 + validate_only)
    kinds = []
    for t, skip, abc in big_texts(BIG_SEED, BIG_COUNT):
        assert 5 * T <= len(t) < 9 * T
        pieces = cut(t, [rng.randrange(len(t) + 1) for _ in range(rng.randrange(1, 5))])
        hows = [rng.choice(("wide", "pieces")) for _ in pieces]
        if "wide" not in hows:
            hows[rng.randrange(len(hows))] = "wide"
        want = ref_stream(pieces, skip, abc)
        got = run_stream(pieces, hows, validate_only=validate_only, in_at=rng.randrange(16),
                         out_at=rng.randrange(4), skip=skip, abc=abc)
        assert [r for r, _ in got] == [r + (0,) for r, _ in want]
        kinds.append(check_whole(t, got, skip, abc))
    assert set(kinds) == ALL_KINDS
    assert kinds.count(OK) * 3 >= len(kinds)


@gpu
def test_alphabets_and_skip_sets():
    """The four alphabets and the skip sets of the pieces test, at 2T + 7 bytes."""
    n = 2 * T + 7
    kinds = set()
    for abc in (STD, URL, NOPAD, DOTPAD):
        for skip in (b"", b"\n", b" \t\r\n"):
            rng = random.Random(len(skip) + 7)
            if skip:
                nchars = (n - n // 40) // 4 * 4
            else:  # without a skip set the text is its characters: 2T + 7 is 3 mod 4
                nchars = n if abc == NOPAD else n // 4 * 4
            base = bytearray(plain(_data(nchars // 4 * 3 + (0, 0, 0, 2)[nchars % 4], len(skip) + 9),
                                   abc))
            assert len(base) == nchars
            while skip and len(base) < n:
                base.insert(rng.randrange(len(base) + 1), rng.choice(skip))
            texts = [bytes(base)]
            for p in (0, T - 1, T, len(base) - 1, len(base) - 2):
                for v in (0x2A, 0x3D, 0x2E, 0x0D, 0x2F):
                    u = bytearray(base)
                    u[p] = v
                    texts.append(bytes(u))
            for t in texts:
                got = run_stream(cut(t, [rng.randrange(len(t))]) if rng.random() < 0.5 else [t],
                                 in_at=len(skip) + 1, out_at=len(skip) % 4, skip=skip, abc=abc)
                kinds.add(check_whole(t, got, skip, abc))
    assert kinds == ALL_KINDS


@gpu
def test_the_scans_branches():
    """Tile counts that reach each path of k_skip_wide_scan: one tile, a
    wave's worth and one more, the workgroup's lanes and one more (the first
    strip of two records), and strips of five -- a batch of four loads and a
    batch of one -- with a short last one and idle lanes behind it; one pad character in the first tile and one stranger in
    the last."""
    b64 = _b64()
    ws = None
    for tiles in (1, LANES, LANES + 1, TH, TH + 1, 4 * TH + 1, 4 * TH + 89, 5 * TH - 2):
        n = tiles * T - 5
        assert -(-n // T) == tiles
        line = np.frombuffer(crlf76(_data(57, tiles)), np.uint8)
        clean = np.tile(line, n // 78 + 1)[:n].copy()
        clean[n - 3:] = 0x0A
        first = np.flatnonzero((clean != 0x0A) & (clean != 0x0D))
        clean[first[first.size - first.size % 4:]] = 0x0A  # whole groups only
        first = first[:first.size - first.size % 4]
        kept = int(first.size)
        pad_at = int(first[7])
        char_at = int(first[first >= n - T + 100][0]) if tiles > 1 else int(first[-9])
        for spoil in ((), ((char_at, 0x2A),), ((pad_at, 0x3D),), ((pad_at, 0x3D), (char_at, 0x2A))):
            a = clean.copy()
            for p, v in spoil:
                a[p] = v
            x = torch.from_numpy(a).cuda()
            want = torch.full((REC,), FILL, dtype=torch.uint8, device="cuda")
            size = b64.strict_skip_workspace_size(n)
            if ws is None or ws.numel() < size:
                ws = torch.zeros(size, dtype=torch.uint8, device="cuda")
            ref_out = torch.full((cap_of(n),), FILL, dtype=torch.uint8, device="cuda")
            b64.decode_strict_skip(x, out=ref_out, workspace=ws, result=want)
            rec, got, _ = one_call(Lane(), x, True, "wide")
            assert rec == records(want)[0], (tiles, spoil)
            if not spoil:
                assert rec[0] == OK and rec[2] == kept // 4 * 3
                assert got[:rec[2]].tobytes() == ref_out[:rec[2]].cpu().numpy().tobytes()
            else:
                first_bad = min(spoil)
                assert rec[:2] == (PAD if first_bad[1] == 0x3D else CHAR, first_bad[0])
            # not final, by both calls: the same record, bytes and state
            main, twin = Lane(), Lane()
            r1, g1, s1 = one_call(main, x, False, "wide")
            r2, g2, s2 = one_call(twin, x, False, "pieces")
            assert r1 == r2 and (spoil or g1[:r1[2]].tobytes() == g2[:r2[2]].tobytes())
            assert s1[72:88].tobytes() == s2[72:88].tobytes()
            assert spoil or s1.tobytes() == s2.tobytes()


@gpu
def test_past_4gib():
    """Validate only, 2^32 + T + 5 bytes built on the device: a stranger at
    offset 2^32 + 9, then the clean text as a piece that is not final, and a
    stranger in the piece behind it."""
    b64 = _b64()
    n = (1 << 32) + T + 5
    free, _ = torch.cuda.mem_get_info()
    assert free > n + (1 << 30), "the device has no room for a text of 2^32 bytes"
    line = crlf76(_data(57, 2))
    assert len(line) == 78 and b"=" not in line
    lines = -(-n // 78)
    buf = torch.empty(GUARD + lines * 78 + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:GUARD].fill_(FILL)
    buf[GUARD:GUARD + lines * 78].view(lines, 78).copy_(_dev(line))
    buf[GUARD + n:].fill_(FILL)
    x = buf[GUARD:GUARD + n]
    bad = (1 << 32) + 9
    assert bad % 78 < 76
    keep = int(x[bad])
    x[bad] = 0x2A
    lane = Lane()
    rec, _, st = one_call(lane, x, False, "wide", validate_only=True)
    assert rec == (CHAR, bad, 0, 0)
    assert st.view(np.uint64)[9:11].tolist() == [CHAR, bad]
    rec, _, st = one_call(lane, x[:5], True, "wide", validate_only=True)  # repeated, then zeroed
    assert rec == (CHAR, bad, 0, 0)
    x[bad] = keep
    E = n // 78 * 76 + min(n % 78, 76)
    rec, _, st = one_call(lane, x, False, "wide", validate_only=True)
    assert rec == (OK, 0, E // 4 * 3, 0)
    w = st.view(np.uint64)
    assert w[0] == n and w[1] == E and w[0] > 1 << 32 and not w[2:5].any() and not w[9:].any()
    last = [n - 1 - i for i in range(8) if (n - 1 - i) % 78 < 76][:3]
    assert w[5:8].tolist() == last
    assert int(w[8]) >> 24 == E % 4 and [int(w[8]) >> (8 * i) & 255 for i in range(3)] == \
        [line[p % 78] for p in last]
    tail = b"A" * (4 - E % 4) + b"*"
    _, y = place(tail)
    rec, _, _ = one_call(lane, y, True, "wide", validate_only=True)
    assert rec == (CHAR, n + len(tail) - 1, 0, 0)
    del buf, x
    torch.cuda.empty_cache()


@gpu
def test_full_size():
    """1 GiB of payload through encode_lines (CRLF-76, trailing), one final
    piece: the payload again, and decode_strict_skip's record."""
    b64 = _b64()
    n = 1 << 30
    free, _ = torch.cuda.mem_get_info()
    assert free > 4 * n, "the device has no room for 1 GiB of payload, its text and its bytes"
    payload = torch.empty(n, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(payload, 0x1D)
    text = b64.encode_lines(payload)
    w = text.numel()
    assert w == b64.encoded_lines_len(n, 76, b"\r\n", True)
    out = torch.full((cap_of(w) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((2 * REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    need = ws_of(w)
    ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lane = Lane()
    b64.decode_strict_skip_piece(text, lane.state, res[:REC], out=out[:cap_of(w)], final=True,
                                 workspace=ws[:need])
    b64.decode_strict_skip(text, validate_only=True, result=res[REC:2 * REC])
    torch.cuda.synchronize()
    mine, theirs = records(res)[:2]
    assert mine == theirs == (OK, 0, n, 0)
    assert torch.equal(out[:n], payload)
    assert bool((out[n:cap_of(w)] == FILL).all()) and bool((out[cap_of(w):] == FILL).all())
    assert bool((ws[need:] == FILL).all()) and bool((res[2 * REC:] == FILL).all())
    assert not lane.all[:STATE].any() and bool((lane.all[STATE:] == FILL).all())
    del payload, text, out
    torch.cuda.empty_cache()


@gpu
def test_graph_capture():
    """One captured call, replayed twice on the same length with other
    contents; the second holds an offence."""
    b64 = _b64()
    n = 2 * T + P + 77
    texts = [text_of(n, 21), text_of(n, 22), text_of(n, 23)]
    spoiled = bytearray(texts[2])
    spoiled[T + 40] = 0x2A
    texts[2] = bytes(spoiled)
    assert skip_ref(texts[2]) == (CHAR, T + 40, 0)
    buf, x = place(texts[0], 7)
    cap = cap_of(n)
    out = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    need = ws_of(n)
    ws = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lane = Lane()

    def call():
        b64.decode_strict_skip_piece(x, lane.state, res[:REC], out=out[GUARD + 1:GUARD + 1 + cap],
                                     final=True, workspace=ws[:need])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()  # warm-up; the piece is final: the state ends zeroed
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call()
    for t in texts:
        x.copy_(_dev(t))
        out.fill_(FILL)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = skip_ref(t)
        assert records(res)[0] == want + (0,)
        o = out.cpu().numpy()
        if want[0] == OK:
            assert o[GUARD + 1:GUARD + 1 + want[2]].tobytes() == skip_bytes(t)
        else:
            assert (o == FILL).all()
        assert (o[:GUARD + 1] == FILL).all() and (o[GUARD + 1 + cap:] == FILL).all()
        assert (res[REC:].cpu().numpy() == FILL).all() and (ws[need:].cpu().numpy() == FILL).all()
        s = lane.all.cpu().numpy()
        assert not s[:STATE].any() and (s[STATE:] == FILL).all()
