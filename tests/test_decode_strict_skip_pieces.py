"""Strict skip decode of texts that arrive in pieces
(b64x_decode_strict_skip_pieces, async_amd.b64.decode_strict_skip_pieces):
every record and every piece's bytes, bit for bit, against the chunked scalar
procedure of include/b64x.h written here in plain Python (ref_piece), which is
itself checked on the CPU against the whole-text references of
tests/test_decode_strict_skip.py (skip_ref, skip_bytes, decode_kept).

CPU tests: the exports and their signatures, every -EINVAL case in its order,
-ENODEV without a device, the wrapper's ValueErrors, b64x_skip_piece_cap, the
chunked reference, and the new code object's kernels and barriers.

GPU tests go through one harness (Streams).  The pieces of one call lie end to
end in the input (piece i is d_in[d_in_off[i] .. d_in_off[i+1])), so the guard
between two pieces is a piece of its own: at least 64 bytes of 0xA5 that
continues a state which already holds a report.  Such a piece must get the
report again and write nothing; to the pieces around it, a guard byte that is
read is a stranger.  Every capacity on the output side stands between 64
guard bytes, a guard stands behind the records and behind the states; one copy
back per call, then records, bytes, guards and the states of finished texts.

b64x_skip_piece_cap(0) is 3, not 0: it is b64x_decoded_cap(len + 3), and a
final empty piece behind a carry of 3 writes 2 bytes.

The unit's sizes (async_amd/csrc/b64x_skip_pieces.hip): a lane takes a chunk of
16 bytes at a 16-byte aligned address, a wave a pass of 1,024, a block has four
waves; a lane decodes a unit of 16 sextets, up to 15 are carried from pass to
pass and up to 3 from piece to piece.
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
                                           np_skip_ref, random_texts, records, skip_bytes,
                                           skip_ref, strip)
from tests.test_decode_strict_skip_rows import kept_text

ROOT = util.ROOT
CHUNK, PASS, WAVES = 16, 1024, 4
STATE = 128
ALL_KINDS = {OK, CHAR, PAD, BITS, LENGTH}
NAME = "b64x_decode_strict_skip_pieces"


def cap_of(n: int) -> int:
    """b64x_skip_piece_cap: b64x_decoded_cap(n + 3)."""
    return (n + 6) // 4 * 3


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


# ------------------------------------------------------- the reference --

class RefState:
    """What a state holds, in the words of the procedure."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.pos = self.E = self.c = 0
        self.first_char = self.first_pad = None
        self.tail = []       # the last three kept bytes: (offset in T, byte)
        self.sextets = []    # carried, 0..3
        self.report = None   # an early report: (kind, pos, 0)

    def is_zero(self):
        return (self.pos, self.E, self.c, self.tail, self.sextets, self.report) == \
            (0, 0, 0, [], [], None)


def _groups(sx):
    """The bytes of the sextets sx: whole groups, and 1 or 2 bytes of a last
    group of 2 or 3."""
    out = bytearray()
    for i in range(0, len(sx) - len(sx) % 4, 4):
        v = (sx[i] << 18) | (sx[i + 1] << 12) | (sx[i + 2] << 6) | sx[i + 3]
        out += v.to_bytes(3, "big")
    r = sx[len(sx) - len(sx) % 4:]
    if len(r) == 2:
        out.append(((r[0] << 2) | (r[1] >> 4)) & 0xFF)
    elif len(r) == 3:
        v = (r[0] << 10) | (r[1] << 4) | (r[2] >> 2)
        out += (v & 0xFFFF).to_bytes(2, "big")
    return bytes(out)


def ref_piece(st: RefState, piece: bytes, final: bool, skip=CRLF, abc=STD):
    """One piece on state st, by the chunked procedure of include/b64x.h:
    ((kind, pos, out_len), the bytes this piece writes -- None where they are
    unspecified or the piece writes nothing because of a report)."""
    chars, pad, padc = alpha(abc)
    if st.report is not None:  # every later piece of that text: the same record
        rec = st.report
        if final:
            st.reset()
        return rec, None
    # 1. the piece's kept bytes join the totals
    for p, b in enumerate(piece):
        if b in skip:
            continue
        off = st.pos + p
        st.E += 1
        if pad and b == padc:
            st.c += 1
            if st.first_pad is None:
                st.first_pad = off
        elif b not in chars:
            if st.first_char is None:
                st.first_char = off
        else:
            st.sextets.append(chars.index(b))
        st.tail = (st.tail + [(off, b)])[-3:]
    st.pos += len(piece)
    npad = 0
    if pad and st.tail and st.tail[-1][1] == padc:
        npad = 2 if len(st.tail) >= 2 and st.tail[-2][1] == padc else 1
    inf = float("inf")
    fc = inf if st.first_char is None else st.first_char
    fp = inf if st.first_pad is None else st.first_pad
    rec = None
    if st.c > npad and fp < fc:
        rec = (PAD, st.first_pad, 0)
    elif st.first_char is not None:
        rec = (CHAR, st.first_char, 0)
    if rec is not None:
        st.report = rec
        if final:
            st.reset()
        return rec, None
    # 2. not final: the whole groups
    if not final:
        whole = len(st.sextets) // 4 * 4
        data = _groups(st.sextets[:whole])
        st.sextets = st.sextets[whole:]
        return (OK, 0, len(data)), data
    # 3. final: LENGTH, then BITS, then the partial group too
    E, D = st.E, st.E - npad
    if (pad and E % 4) or (not pad and E % 4 == 1):
        rec = (LENGTH, st.pos, 0)
    elif D and D % 4 in (2, 3) and \
            chars.index(st.tail[-1 - npad][1]) & (15 if D % 4 == 2 else 3):
        rec = (BITS, st.tail[-1 - npad][0], 0)
    if rec is not None:
        st.reset()
        return rec, None
    data = _groups(st.sextets)
    st.reset()
    return (OK, 0, len(data)), data


def cut(t: bytes, points):
    """t cut at the sorted offsets `points`: len(points) + 1 pieces."""
    edges = [0] + sorted(points) + [len(t)]
    return [t[a:b] for a, b in zip(edges, edges[1:])]


def random_cuts(t: bytes, rng):
    """t cut at 0..4 seeded points (pieces may be empty)."""
    return cut(t, [rng.randrange(len(t) + 1) for _ in range(rng.randrange(5))])


def ref_stream(pieces, skip=CRLF, abc=STD):
    """[(record, bytes)] of a text's pieces, the last one final, on a fresh state."""
    st = RefState()
    got = [ref_piece(st, p, i == len(pieces) - 1, skip, abc) for i, p in enumerate(pieces)]
    assert st.is_zero()
    return got


def check_stream_against_whole(pieces, skip, abc):
    """The chunked reference against skip_ref / skip_bytes on the whole text."""
    t = b"".join(pieces)
    want = skip_ref(t, skip, abc)
    got = ref_stream(pieces, skip, abc)
    assert got[-1][0][:2] == want[:2], (pieces, skip, abc, got, want)
    report = None
    for (rec, data), p in zip(got[:-1], pieces):
        if report is not None:
            assert rec == report and data is None          # repeated
        elif rec[0] != OK:
            assert rec[0] in (PAD, CHAR) and rec == want   # an early report is final
            report = rec
        else:
            assert rec[2] % 3 == 0 and len(data) == rec[2]
    if report is not None:
        assert got[-1][0] == report
    if want[0] == OK:
        data = b"".join(d for _, d in got)
        assert data == skip_bytes(t, skip, abc) == decode_kept(strip(t, skip), abc)
        assert sum(r[2] for r, _ in got) == want[2] == len(data)
    else:
        assert got[-1][0] == want
    return want[0]


# ----------------------------------------------------------------- CPU --

def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    assert hasattr(lib, NAME) and hasattr(lib, "b64x_skip_piece_cap")
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 12 and getattr(lib, NAME).argtypes == args and res is ctypes.c_int
    res, args = _lib.SIGNATURES["b64x_skip_piece_cap"]
    assert args == [ctypes.c_uint64] and res is ctypes.c_uint64
    header = open(os.path.join(ROOT, "include", "b64x.h")).read()
    assert re.search(r"^int b64x_decode_strict_skip_pieces\(", header, re.M)
    assert re.search(r"^uint64_t b64x_skip_piece_cap\(uint64_t len\);", header, re.M)
    assert "#define B64X_SKIP_STATE_BYTES 128" in header and "#define B64X_PIECE_FINAL 1u" in header
    assert "#define B64X_ABI_VERSION 7" in header and b"abi=7" in lib.b64x_build_info()
    from async_amd import b64
    assert b64.SKIP_STATE_BYTES == _lib.SKIP_STATE_BYTES == STATE and b64.PIECE_FINAL == 1
    for name in ("decode_strict_skip_pieces", "skip_states", "skip_pieces_layout"):
        assert name in b64.__doc__ and callable(getattr(b64, name))


def test_piece_cap():
    lib = _lib.load()
    # b64x_decoded_cap(len + 3); a final empty piece behind a carry of 3 writes 2 bytes
    for n, want in ((0, 3), (1, 3), (4, 6), (5, 6), (6, 9), (1000, 753), ((1 << 33) + 1, 3 * (1 << 31) + 3)):
        assert lib.b64x_skip_piece_cap(n) == want == lib.b64x_decoded_cap(n + 3) == cap_of(n)
    from async_amd import b64
    assert b64.skip_piece_cap(4) == 6
    off = b64.skip_pieces_layout(torch.tensor([0, 0, 1, 5, 13, 113]), align=4)
    assert off.tolist() == [0, 4, 8, 16, 28, 108]
    assert b64.skip_pieces_layout(torch.tensor([7, 7, 8, 12]), align=1).tolist() == [0, 3, 6, 12]


def _host_call():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def call(skip=None, abc=None, d_in=p, off=p, n=2, d_out=p, out_off=p, state=p, sid=None,
             flags=None, d_res=p):
        return lib.b64x_decode_strict_skip_pieces(d_in, off, n, d_out, out_off, state, sid, flags,
                                                  d_res, ref(abc), ref(skip), None)
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
    assert call(nine, bad_abc, d_in=None, off=None, state=None, d_res=None, out_off=None, n=0) == 0
    # 2. NULL pointers and the alignment of records and states, before everything else
    for kw in ({"d_in": None}, {"off": None}, {"state": None}, {"d_res": None}, {"d_res": p + 4},
               {"state": p + 4}):
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
        for kw in ({}, {"d_out": None, "out_off": None}, {"sid": p, "flags": p},
                   {"skip": raw(0, b"")}, {"skip": raw(1, b"="), "abc": _lib.alphabet(pad=False)},
                   {"d_in": p + 1, "d_out": p + 3, "state": p + 8, "d_res": p + 8}):
            assert call(**kw) == -19, kw


def test_no_gpu_is_enodev():
    lib, p, call = _host_call()
    if lib.b64x_device_check() != -19:
        return  # a device is there: the GPU tests make the valid calls
    for n in (1, 3):
        for out in (p, None):
            assert call(n=n, d_out=out) == -19


def test_wrapper_value_errors():
    """What the wrapper refuses without a device: tensors that are not on one,
    and a skip set of nine bytes (test_wrapper_size_errors makes the size
    checks, on device tensors)."""
    from async_amd import b64
    cpu = torch.zeros(4096, dtype=torch.uint8)
    off = torch.tensor([0, 10, 20])
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces(cpu, off, cpu, off, cpu, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces(cpu, off, None, None, cpu, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_pieces(cpu, off, cpu, off, cpu, cpu, skip=b"123456789")
    assert b64.skip_states(3, "cpu").tolist() == [0] * (3 * STATE)


def test_chunked_reference_agrees_with_the_whole_text():
    rng = random.Random(0xC07)
    kinds = []
    for t, skip, abc in random_texts(2000):
        kinds.append(check_stream_against_whole(random_cuts(t, rng), skip, abc))
    assert set(kinds) == ALL_KINDS
    assert kinds.count(OK) * 3 >= len(kinds)
    # the contract's own examples
    got = ref_stream([b"QUJ", b"DQUI"], CRLF, NOPAD)
    assert got == [((OK, 0, 0), b""), ((OK, 0, 5), b"ABCAB")]  # 4 characters behind a carry of 3
    assert ref_stream([b"QQ==", b""])[1] == ((OK, 0, 1), b"A")
    assert ref_stream([b"QUI=", b""])[1] == ((OK, 0, 2), b"AB")
    assert [r for r, _ in ref_stream([b"QQ=", b"QQ", b"=="])] == [(OK, 0, 0)] + [(PAD, 2, 0)] * 2
    assert ref_stream([b"QR", b"=", b"="])[-1][0] == (BITS, 1, 0)
    assert ref_stream([b"QUJ", b"D\nQ"])[-1][0] == (LENGTH, 6, 0)


# The kernels of b64x_skip_pieces.hip; nothing else may be in its code object.
PIECES_KERNELS = {"k_skip_decode_pieces<true>", "k_skip_decode_pieces<false>"}


def test_pieces_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_skip_pieces.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == PIECES_KERNELS, (got - PIECES_KERNELS, PIECES_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == len(PIECES_KERNELS)  # one each, after the table


# ----------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


def _up16(n: int) -> int:
    return -(-n // 16) * 16


class Streams:
    """n states on the device with their reference states, a guard behind
    them, and behind the n one more per piece of the largest call plus one:
    states that hold a report from the start, for the guard pieces.  call()
    runs one launch and checks all of it."""

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

    def call(self, items, validate_only=False, in_at=None, out_at=None, tight=False):
        """items: [(state index, piece, final)].  in_at[j] / out_at[j]: the
        address mod 16 of piece j and of its output (default 0).  tight: the
        capacities stand back to back, without the guards between them.
        Returns [(record, the piece's bytes or None)] as the device gave them."""
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
            assert pos % 16 == (in_at[j] if in_at else 0) % 16
            pieces.append(bytes(piece))
            sids.append(sid)
            flags.append(1 if final else 0)
            o = size if tight else _up16(size) + (out_at[j] if out_at else 0)
            out_off.append(o)
            real.append((len(pieces) - 1, o, cap_of(len(piece))))
            size = o + cap_of(len(piece)) + (0 if tight else GUARD)
            pos += len(piece)
        pieces.append(bytes([FILL]) * GUARD)
        sids.append(self.n + len(items))
        flags.append(0)
        out_off.append(0)
        size += GUARD
        npieces = len(pieces)
        in_off = np.zeros(npieces + 1, np.int64)
        np.cumsum([len(p) for p in pieces], out=in_off[1:])
        x = torch.from_numpy(np.frombuffer(b"".join(pieces), np.uint8).copy()).cuda()
        out = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * npieces + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
        b64.decode_strict_skip_pieces(
            x, torch.from_numpy(in_off).cuda(), None if validate_only else out,
            None if validate_only else torch.tensor(out_off, dtype=torch.int64, device="cuda"),
            self.states, res[:REC * npieces],
            final=torch.tensor(flags, dtype=torch.uint8, device="cuda"),
            sid=torch.tensor(sids, dtype=torch.int32, device="cuda"), skip=self.skip, abc=self.abc)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        recs = records(res)[:npieces]
        states = self.all.cpu().numpy()
        assert (res[REC * npieces:].cpu().numpy() == FILL).all(), "the guard behind the records"
        assert (states[-GUARD:] == FILL).all(), "the guard behind the states"
        assert recs[0::2] == [(CHAR, 0, 0, 0)] * (len(items) + 1), "a guard piece's record"
        mask = np.ones(got.size, bool)
        result = []
        for (sid, piece, final), (i, o, cap) in zip(items, real):
            had_report = self.ref[sid].report is not None
            want, data = ref_piece(self.ref[sid], piece, final, self.skip, self.abc)
            label = (sid, len(piece), piece[:24], final, int(in_off[i]) % 16, o % 16, self.skip,
                     self.abc, validate_only)
            assert recs[i] == (want[0], want[1], want[2], 0), (label, recs[i], want)
            if not validate_only and data is not None:
                assert got[o:o + want[2]].tobytes() == data, label
            if not had_report and not validate_only:  # behind a report nothing at all is written
                mask[o:o + cap] = False
            if final:
                assert not states[sid * STATE:(sid + 1) * STATE].any(), (label, "state not zeroed")
            result.append((recs[i], None if validate_only or data is None else data))
        assert (got[mask] == FILL).all(), "a byte outside the pieces' capacities was overwritten"
        return result

    def run(self, streams, **kw):
        """Stream s (a list of pieces, the last one final) on state s: round r
        is one call with piece r of every stream that still has one."""
        assert len(streams) <= self.n
        out = [[] for _ in streams]
        for r in range(max(map(len, streams))):
            items = [(s, p[r], r == len(p) - 1) for s, p in enumerate(streams) if r < len(p)]
            at = {}
            for key in ("in_at", "out_at"):
                if key in kw:
                    at[key] = [kw[key][s] for s, _, _ in items]
            rest = {k: v for k, v in kw.items() if k not in at}
            for (s, _, _), g in zip(items, self.call(items, **at, **rest)):
                out[s].append(g)
        self.all_zero()
        return out

    def all_zero(self):
        assert not self.states[:self.n * STATE].any(), "a finished text left its state armed"
        assert all(r.is_zero() for r in self.ref)


@gpu
def test_wrapper_size_errors():
    """The wrapper's size and type checks: no call reaches the library."""
    b64 = _b64()
    x = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 10, 20, 30], device="cuda")
    states = b64.skip_states(3)
    res = torch.zeros(REC * 3, dtype=torch.uint8, device="cuda")
    assert states.numel() == 3 * STATE and not states.any()
    ok = dict(x=x, in_off=off, out=x, out_off=off, states=states, result=res)
    for kw in ({"result": res[:REC * 3 - 1]}, {"states": states[:2 * STATE]},
               {"states": states[:STATE + 1]}, {"states": states[4:4 + STATE]},
               {"out_off": off.int()}, {"in_off": off.int()},
               {"final": torch.zeros(3, dtype=torch.int32, device="cuda")},
               {"final": torch.zeros(2, dtype=torch.uint8, device="cuda")},
               {"sid": torch.zeros(3, dtype=torch.int64, device="cuda")},
               {"sid": torch.zeros(2, dtype=torch.int32, device="cuda")},
               {"final": torch.zeros(3, dtype=torch.uint8)}):
        with pytest.raises(ValueError):
            b64.decode_strict_skip_pieces(**{**ok, **kw})


@gpu
def test_random_texts_in_pieces():
    """The 2,000 texts, each cut at 0..4 seeded points; the texts of one skip
    set and alphabet share their calls."""
    rng = random.Random(0xC07)
    groups = {}
    for t, skip, abc in random_texts(2000):
        groups.setdefault((skip, abc), []).append(random_cuts(t, rng))
    assert len(groups) == 16
    kinds, early, repeated = set(), 0, 0
    for (skip, abc), streams in groups.items():
        got = Streams(len(streams), skip, abc).run(streams)
        for pieces, g in zip(streams, got):
            want = skip_ref(b"".join(pieces), skip, abc)
            kinds.add(want[0])
            assert g[-1][0][:2] == want[:2]
            if want[0] == OK:
                assert sum(r[2] for r, _ in g) == want[2]
                assert b"".join(d for _, d in g) == decode_kept(strip(b"".join(pieces), skip), abc)
            bad = [i for i, (r, _) in enumerate(g) if r[0] != OK]
            if bad and bad[0] < len(g) - 1:
                early += 1
                repeated += len(g) - 1 - bad[0]
                assert all(r == g[bad[0]][0] for r, _ in g[bad[0]:])
    assert kinds == ALL_KINDS and early > 100 and repeated > early


def _mutants(t: bytes, spots):
    out = [t]
    for p, v in spots:
        u = bytearray(t)
        u[p] = v
        out.append(bytes(u))
    return out


@gpu
def test_every_cut_position():
    """A 100-byte text cut at every offset and a 2,200-byte CRLF-76 text cut
    around its pass edges, each into two pieces, clean and with a stranger, a
    pad character or a BITS offence on either side of the cut; one batch."""
    short = crlf76(_data(70, 2))
    assert len(short) == 100 and short.endswith(b"==\r\n")
    long_ = crlf76(_data(1604, 3))
    long_ += b"\n" * (2200 - len(long_))
    assert len(long_) == 2200 and long_.rstrip(b"\r\n").endswith(b"=")
    streams = []
    bits = short[:95] + b"/" + short[96:]  # u[D - 1] with its low four bits set
    assert skip_ref(bits) == (BITS, 95, 0) and skip_ref(short) == (OK, 0, 70)
    for c in range(101):
        for t in _mutants(short, [(40, 0x2A), (41, 0x3D)]) + [bits]:
            streams.append(cut(t, [c]))
    for c in list(range(1007, 1042)) + list(range(2031, 2066)):
        for t in _mutants(long_, [(c - 1, 0x2A), (c, 0x2A), (c - 1, 0x3D), (c, 0x3D)]):
            streams.append(cut(t, [c]))
    # the BITS character of the long text and its pad, either side of a cut
    end = len(long_.rstrip(b"\r\n"))
    lbits = long_[:end - 2] + b"/" + long_[end - 1:]
    assert skip_ref(lbits) == (BITS, end - 2, 0)
    streams += [cut(lbits, [c]) for c in (end - 3, end - 2, end - 1, end, 1024, 2048)]
    wants = [skip_ref(b"".join(p)) for p in streams]
    assert {w[0] for w in wants} == {OK, CHAR, PAD, BITS}
    got = Streams(len(streams)).run(streams)
    for p, g, w in zip(streams, got, wants):
        assert g[-1][0][:2] == w[:2]
        if w[0] == OK:
            assert sum(r[2] for r, _ in g) == w[2]
            assert b"".join(d for _, d in g) == decode_kept(strip(b"".join(p)))


@gpu
def test_the_carry():
    """Carry from piece to piece 0..3 x carry from pass to pass 0..15: the
    first piece holds 4 + cc characters, the second starts at a 16-byte
    boundary with j line feeds, so its first pass ends behind cc + 1,024 - j
    sextets; then the contract's small cases, with and without pad."""
    streams = []
    for cc in range(4):
        for j in range(16):
            u = kept_text(2400, 16 * cc + j)
            streams.append([u[:4 + cc], b"\n" * j + u[4 + cc:1500], u[1500:]])
    got = Streams(len(streams)).run(streams)
    for p, g in zip(streams, got):
        assert [r[0] for r, _ in g] == [OK] * 3 and g[0][0][2] == 3
        assert b"".join(d for _, d in g) == decode_kept(strip(b"".join(p)))
    small = [
        [b"QUJD", b"", b"QQ", b"==", b""],             # empty pieces, not final and final
        [b"", b"", b""],
        [b"QU", b"\r\n\r\n", b"JD", b"\n"],            # pieces of skipped bytes only
        [b"\r\n", b"\n" * 1025, b"\r"],
        [b"QQ==", b""],                                # a final empty piece behind a carry of 2
        [b"QUI=", b""],                                # and of 3
        [b"QQ=", b"="],                                # = | =
        [b"QQ", b"=", b"\r\n", b"=", b"\r\n"],
        [b"QQ==", b"\r\n", b"\r\n\r\n", b"\n"],        # pads, then line breaks only
        [b"QQ=", b"\r\n", b"QQ", b"QUJD"],             # a pad, then data: PAD at the pad's offset
        [b"QQ==", b"\n", b"Q"],
        [b"QR", b"=", b"="],                           # BITS in an earlier piece
        [b"QUJDQUJ", b"\r\n", b"="],
        [b"QUJ", b"D\nQ"],                             # LENGTH at |T|
        [b"QUJD", b"Q", b""],
        [b"Q", b"U", b"J", b"D", b"Q", b"Q", b"=", b"="],
    ]
    got = Streams(len(small)).run(small)
    first = [[r for r, _ in g] for g in got]
    assert first[0] == [(OK, 0, 3, 0), (OK, 0, 0, 0), (OK, 0, 0, 0), (OK, 0, 0, 0), (OK, 0, 1, 0)]
    assert got[4][1] == ((OK, 0, 1, 0), b"A") and got[5][1] == ((OK, 0, 2, 0), b"AB")
    assert first[6] == [(OK, 0, 0, 0), (OK, 0, 1, 0)]
    assert first[9] == [(OK, 0, 0, 0), (OK, 0, 0, 0), (PAD, 2, 0, 0), (PAD, 2, 0, 0)]
    assert first[11][-1] == (BITS, 1, 0, 0) and first[12][-1] == (BITS, 6, 0, 0)
    assert first[13][-1] == (LENGTH, 6, 0, 0) and first[14][-1] == (LENGTH, 5, 0, 0)
    nopad = [[b"QQ", b""], [b"QUI", b""], [b"QUJ", b"DQUI"], [b"QUJD", b"Q"], [b"QR", b"\n", b""],
             [b"QQ=", b"="]]
    got = Streams(len(nopad), abc=NOPAD).run(nopad)
    assert [g[-1][0] for g in got] == [(OK, 0, 1, 0), (OK, 0, 2, 0), (OK, 0, 5, 0), (LENGTH, 5, 0, 0),
                                       (BITS, 1, 0, 0), (CHAR, 2, 0, 0)]
    assert got[2][1][1] == b"ABCAB"


@gpu
def test_lowest_offset_wins_across_pieces():
    L = 3 * PASS + 5
    b = b"\n" * 40 + crlf76(_data(2200, 8))
    b += b"\n" * (L - len(b))
    assert len(b) == L and skip_ref(b)[0] == OK
    J, P = 0x00, 0x3D

    def ch(p):  # the nearest character at or after p
        while b[p] in CRLF:
            p += 1
        return p
    cuts = [1000, 2100]
    spots = [
        [(ch(70), P), (ch(1003), J)],                 # a PAD a piece before a CHAR
        [(ch(70), J), (ch(1003), P)],
        [(ch(999), J), (ch(1000), P)],                # either side of a cut
        [(ch(999), P), (ch(1000), J)],
        [(ch(1500), P), (ch(2200), J), (ch(3000), P)],
        [(ch(2200), P), (ch(1500), J), (ch(80), P)],
        [(ch(2900), J), (ch(2150), J), (ch(1100), P)],
        [(ch(1024 + 3), J), (ch(1024 - 20), P)],      # one piece, across its pass edge
    ]
    streams = [cut(b, cuts)]
    for sp in spots:
        u = bytearray(b)
        for p, v in sp:
            u[p] = v
        first = min(sp)
        assert skip_ref(bytes(u)) == (PAD if first[1] == P else CHAR, first[0], 0)
        streams.append(cut(bytes(u), cuts))
    for at in (None, [5] * len(streams)):
        kw = {} if at is None else {"in_at": at, "out_at": [11] * len(streams)}
        got = Streams(len(streams)).run(streams, **kw)
        for sp, g in zip(spots, got[1:]):
            first = min(sp)
            assert g[-1][0] == (PAD if first[1] == P else CHAR, first[0], 0, 0)


@gpu
def test_alignment_and_capacity():
    """Pieces at every address mod 16 with their outputs at odd addresses;
    then capacities back to back, filled to the last byte: a carry of 3 and
    4 m + 1 characters write exactly b64x_skip_piece_cap bytes."""
    text = crlf76(_data(1700, 4))
    streams = [cut(text, [700 + 3 * s, 1500 + s]) for s in range(16)]
    ins, outs = list(range(16)), [(2 * s + 1) % 16 for s in range(16)]
    Streams(16).run(streams, in_at=ins, out_at=outs)
    Streams(16).run(streams, in_at=ins[::-1], out_at=[(s + 8) % 16 for s in outs])
    b64 = _b64()
    full = []
    for m in (1, 2, 5, 64, 257):
        u = kept_text(3 + 4 * m + 1 + 4, m, NOPAD)
        assert b64.skip_piece_cap(4 * m + 1) == 3 * (m + 1)
        full.append([u[:3], u[3:4 * m + 4], u[4 * m + 4:]])
    full.append([b"QUJ", b"DQUI"])  # a final piece of 4 behind a carry of 3: 5 bytes of 6
    got = Streams(len(full), abc=NOPAD).run(full, tight=True)
    for m, g in zip((1, 2, 5, 64, 257), got):
        assert g[1][0] == (OK, 0, cap_of(4 * m + 1), 0)
    assert got[-1][1] == ((OK, 0, 5, 0), b"ABCAB")


@gpu
def test_alphabets_and_skip_sets():
    kinds = set()
    for abc in (URL, NOPAD, DOTPAD):
        chars, pad, padc = alpha(abc)
        for skip in (b"", b"\n", b" \t\r\n"):
            rng = random.Random(len(skip) + chars[62])
            streams = []
            for n in (0, 1, 2, 3, 100, 1001):
                base = bytearray(plain(_data(n, n + 9), abc))
                for _ in range(len(base) // 30 + 2 if skip else 0):
                    base.insert(rng.randrange(len(base) + 1), rng.choice(skip))
                texts = [bytes(base)]
                for p in (0, len(base) // 2, len(base) - 1, len(base) - 2) if n else ():
                    for v in (0x2A, padc, 0x0D, 0x20, chars[63]):
                        u = bytearray(base)
                        u[p % len(u)] = v
                        texts.append(bytes(u))
                streams += [random_cuts(t, rng) for t in texts]
            kinds |= {skip_ref(b"".join(p), skip, abc)[0] for p in streams}
            Streams(len(streams), skip, abc).run(streams, in_at=[len(skip)] * len(streams),
                                                 out_at=[3 * len(skip)] * len(streams))
    assert kinds == ALL_KINDS


@gpu
def test_validate_only():
    """The same records (the harness compares both with the reference), and
    no byte of the output written (its mask covers all of it)."""
    rng = random.Random(5)
    streams = [random_cuts(t, rng) for t, skip, abc in random_texts(2000, seed=11)
               if (skip, abc) == (CRLF, STD)]
    text = crlf76(_data(3000, 6))
    streams += [cut(text, [1024, 2048, 4000]), cut(text[:2000] + b"*" + text[2000:], [1000, 2500]),
                [b"QR", b"=\r\n", b"="], [b"QUJDQUJ=", b""]]
    dec = Streams(len(streams)).run(streams)
    val = Streams(len(streams)).run(streams, validate_only=True)
    assert [[r for r, _ in g] for g in dec] == [[r for r, _ in g] for g in val]
    assert {g[-1][0][0] for g in dec} == ALL_KINDS


@gpu
def test_more_pieces_than_waves():
    """2 x CUs x 32 + 3 streams, two pieces of 40 bytes each."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 8 * WAVES + 3
    rng = random.Random(cus)
    pool = b"AQz9+/=-_. \t\x00\xff"
    streams = []
    for i in range(n):
        t = bytearray(plain(rng.randbytes(57)))
        if i % 3 == 0:
            t[rng.choice((rng.randrange(76), 75 - rng.randrange(4)))] = rng.choice(pool)
        for _ in range(4):
            t.insert(rng.randrange(len(t) + 1), rng.choice(CRLF))
        streams.append([bytes(t[:40]), bytes(t[40:])])
    assert all(len(p[0]) == len(p[1]) == 40 for p in streams)
    got = Streams(n).run(streams, tight=True)
    kinds = [g[-1][0][0] for g in got]
    assert set(kinds) >= {OK, CHAR, PAD} and kinds.count(OK) * 3 >= len(kinds)


@gpu
def test_pieces_past_4gib_apart():
    """Two pieces more than 4 GiB apart in one allocation, on both sides; the
    bytes between them are a piece of a state that holds a report, which is
    not walked (its memory is never written)."""
    b64 = _b64()
    far = (1 << 32) + 4096 + 7
    t = crlf76(_data(1538, 3))
    L = len(t)
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * (far + L) + (1 << 30):
        pytest.skip("the device has no room for pieces 2^32 bytes apart")
    t2 = crlf76(_data(1538, 5))
    assert len(t2) == L
    x = torch.empty(far + L + GUARD, dtype=torch.uint8, device="cuda")
    out = torch.empty(far + cap_of(L) + GUARD, dtype=torch.uint8, device="cuda")
    x[:L + GUARD].fill_(FILL)
    x[far - GUARD:].fill_(FILL)
    out[:cap_of(L) + GUARD].fill_(FILL)
    out[far - GUARD:].fill_(FILL)
    x[:L].copy_(torch.from_numpy(np.frombuffer(t, np.uint8).copy()))
    x[far:far + L].copy_(torch.from_numpy(np.frombuffer(t2, np.uint8).copy()))
    all_states = torch.full((3 * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states = all_states[:3 * STATE]
    states.zero_()
    res = torch.full((3 * REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    star = torch.full((1,), 0x2A, dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip_pieces(star, torch.tensor([0, 1], device="cuda"), None, None,
                                  states[STATE:2 * STATE], res[:REC])  # state 1 holds a report
    in_off = torch.tensor([0, L, far, far + L], dtype=torch.int64, device="cuda")
    out_off = torch.tensor([0, 0, far], dtype=torch.int64, device="cuda")
    final = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip_pieces(x, in_off, out, out_off, states, res[:3 * REC], final=final)
    torch.cuda.synchronize()
    assert records(res)[:3] == [(OK, 0, 1538, 0), (CHAR, 0, 0, 0), (OK, 0, 1538, 0)]
    assert out[:1538].cpu().numpy().tobytes() == _data(1538, 3)
    assert bool((out[cap_of(L):cap_of(L) + GUARD] == FILL).all())
    assert bool((out[far - GUARD:far] == FILL).all()) and bool((out[far + cap_of(L):] == FILL).all())
    assert out[far:far + 1538].cpu().numpy().tobytes() == _data(1538, 5)
    assert (res[3 * REC:].cpu().numpy() == FILL).all()
    s = all_states.cpu().numpy()
    assert not s[:STATE].any() and s[STATE:2 * STATE].any() and not s[2 * STATE:3 * STATE].any()
    assert (s[3 * STATE:] == FILL).all()


@gpu
def test_one_final_piece_is_the_ragged_call():
    """One final piece on a zero state: the records and bytes of
    decode_strict_skip_batch on the same buffers."""
    b64 = _b64()
    texts = [t for t, skip, abc in random_texts(2000) if (skip, abc) == (CRLF, STD)]
    texts += [crlf76(_data(n, n)) for n in (700, 1024, 5000)] + [b"QR==", b"QUJDQUJ=\r\n"]
    nbuf = len(texts)
    in_off = np.zeros(nbuf + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=in_off[1:])
    x = torch.from_numpy(np.frombuffer(b"".join(texts), np.uint8).copy()).cuda()
    d_in_off = torch.from_numpy(in_off).cuda()
    out_off = b64.skip_pieces_layout(d_in_off)
    size = int(out_off[-1])
    got = []
    for pieces in (False, True):
        out = torch.full((size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if pieces:
            states = b64.skip_states(nbuf)
            b64.decode_strict_skip_pieces(x, d_in_off, out, out_off, states, res[:REC * nbuf],
                                          final=torch.ones(nbuf, dtype=torch.uint8, device="cuda"))
            assert not states.any()
        else:
            b64.decode_strict_skip_batch(x, d_in_off, out, out_off, res[:REC * nbuf])
        torch.cuda.synchronize()
        assert (res[REC * nbuf:].cpu().numpy() == FILL).all()
        assert (out[size:].cpu().numpy() == FILL).all()
        got.append((records(res)[:nbuf], out.cpu().numpy()))
    assert got[0][0] == got[1][0]
    offs = out_off.cpu().numpy()
    kinds = set()
    for i, t in enumerate(texts):
        want = skip_ref(t)
        kinds.add(want[0])
        assert got[1][0][i] == (want[0], want[1], want[2], 0)
        if want[0] == OK:
            a, b = (g[1][offs[i]:offs[i] + want[2]].tobytes() for g in got)
            assert a == b == decode_kept(strip(t)), i
    assert kinds == ALL_KINDS


@gpu
def test_round_trip():
    """encode_lines (MIME) of 300 KB, cut into pieces of 1,000 bytes and fed
    call by call to state 0 next to 63 streams of other lengths; then a second
    text on the same states, without a memset."""
    b64 = _b64()
    rng = random.Random(64)
    P, S = 1000, 64
    sizes = [300 * 1000] + [rng.randrange(0, 300 * 1000) for _ in range(S - 1)]
    states = b64.skip_states(S)
    for second in (False, True):
        if second:
            sizes = [rng.randrange(0, 5000) for _ in range(S)]
        data = [util.splitmix64(100 * second + s, n) for s, n in enumerate(sizes)]
        texts = [b64.encode_lines(torch.from_numpy(d).cuda()).cpu().numpy() if d.size
                 else np.zeros(0, np.uint8) for d in data]
        rounds = [max(1, -(-t.size // P)) for t in texts]
        # round r holds piece r of every stream that still has one, end to end
        parts, lens, sids, flags, starts = [], [], [], [], [0]
        for r in range(max(rounds)):
            for s in range(S):
                if r < rounds[s]:
                    parts.append(texts[s][r * P:(r + 1) * P])
                    lens.append(parts[-1].size)
                    sids.append(s)
                    flags.append(r == rounds[s] - 1)
            starts.append(len(lens))
        in_off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=in_off[1:])
        x = torch.from_numpy(np.concatenate(parts)).cuda()
        d_in_off = torch.from_numpy(in_off).cuda()
        d_out_off = b64.skip_pieces_layout(d_in_off)
        d_sid = torch.tensor(sids, dtype=torch.int32, device="cuda")
        d_final = torch.tensor(flags, dtype=torch.uint8, device="cuda")
        out = torch.full((int(d_out_off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * len(lens) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        for a, b in zip(starts, starts[1:]):
            b64.decode_strict_skip_pieces(x, d_in_off[a:b + 1], out, d_out_off[a:b], states,
                                          res[REC * a:REC * b], final=d_final[a:b], sid=d_sid[a:b])
        torch.cuda.synchronize()
        assert not states.any()
        r = res.cpu().numpy()
        assert (r[REC * len(lens):] == FILL).all()
        rec = r[:REC * len(lens)].reshape(-1, REC)
        assert not rec[:, 8:].any()  # every piece accepted
        out_len = rec[:, :8].copy().view(np.uint64).reshape(-1).astype(np.int64)
        o = out.cpu().numpy()
        assert (o[int(d_out_off[-1]):] == FILL).all()
        offs = d_out_off.cpu().numpy()
        got = [[] for _ in range(S)]
        for i, s in enumerate(sids):
            got[s].append(o[offs[i]:offs[i] + out_len[i]])
            assert flags[i] or out_len[i] % 3 == 0
        for s in range(S):
            assert np.array_equal(np.concatenate(got[s]), data[s]), (second, s)


@gpu
def test_graph_capture():
    """One captured call, replayed after the offsets, the flags and the state
    indices have been rewritten."""
    b64 = _b64()
    n = 9
    text = crlf76(_data(1538, 3))
    spoiled = text[:1500] + b" " + text[1501:]
    arena = text + spoiled + text
    x = torch.from_numpy(np.frombuffer(arena, np.uint8).copy()).cuda()
    L = len(text)
    in_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    out_off = torch.arange(n, dtype=torch.int64, device="cuda") * (cap_of(3 * L) + GUARD) + GUARD
    size = n * (cap_of(3 * L) + GUARD) + GUARD
    sid = torch.zeros(n, dtype=torch.int32, device="cuda")
    final = torch.zeros(n, dtype=torch.uint8, device="cuda")
    all_states = torch.full((n * STATE + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    states = all_states[:n * STATE]
    states.zero_()
    out = torch.full((size,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    def write(edges, sids, finals):
        in_off.copy_(torch.tensor(edges, dtype=torch.int64))
        sid.copy_(torch.tensor(sids, dtype=torch.int32))
        final.copy_(torch.tensor(finals, dtype=torch.uint8))
    rng = random.Random(9)

    def edges():
        return [0] + sorted(rng.sample(range(1, 3 * L), n - 1)) + [3 * L]
    first = (edges(), list(range(n)), [1] * n)
    write(*first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.decode_strict_skip_pieces(x, in_off, out, out_off, states, res[:REC * n], final=final,
                                      sid=sid)  # warm-up; every piece final: the states end zeroed
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b64.decode_strict_skip_pieces(x, in_off, out, out_off, states, res[:REC * n],
                                          final=final, sid=sid)
    perm = list(range(n))
    rng.shuffle(perm)
    ref = [RefState() for _ in range(n)]
    seen = []
    # all final; other cuts, the states permuted, none final; the same pieces
    # again, final: each state has then taken its piece twice
    second = (edges(), perm, [0] * n)
    for e, sids, finals in (first, second, (second[0], perm, [1] * n), first):
        write(e, sids, finals)
        out.fill_(FILL)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        recs = records(res)[:n]
        o = out.cpu().numpy()
        offs = out_off.cpu().numpy()
        mask = np.ones(o.size, bool)
        for i in range(n):
            piece = arena[e[i]:e[i + 1]]
            had_report = ref[sids[i]].report is not None
            want, data = ref_piece(ref[sids[i]], piece, bool(finals[i]))
            assert recs[i] == (want[0], want[1], want[2], 0), (i, recs[i], want)
            if data is not None:
                assert o[offs[i]:offs[i] + want[2]].tobytes() == data
            if not had_report:
                mask[offs[i]:offs[i] + cap_of(len(piece))] = False
        assert (o[mask] == FILL).all()
        seen.append(recs)
        assert (res[REC * n:].cpu().numpy() == FILL).all()
        s = all_states.cpu().numpy()
        assert (s[n * STATE:] == FILL).all()
        assert s[:n * STATE].any() == (not all(finals))
    assert seen[0] == seen[3] and len({tuple(r) for r in seen}) == 3
