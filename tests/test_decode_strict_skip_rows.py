"""One-pass strict skip decode of strided rows
(b64x_decode_strict_skip_strided, async_amd.b64.decode_strict_skip_strided):
every record and the bytes of every accepted row, bit for bit, against the
references of tests/test_decode_strict_skip.py (skip_ref, its vectorised copy
np_skip_ref, the stdlib's decode of the kept bytes).

CPU tests: the export and its signature, every -EINVAL case in its order,
-ENODEV without a device, the wrapper's ValueErrors, the new code object's
kernels and barriers, and the random row generator's coverage.  GPU tests lay
their rows out with 64 guard bytes of 0xA5 between them where the stride
leaves room (on the input side a guard byte is a stranger: a row that read it
would be refused), put a guard behind the records, copy back once and check
records, bytes and guards.

The unit's sizes (async_amd/csrc/b64x_skip_rows.hip): a lane takes a chunk of
16 bytes at a 16-byte aligned address, a wave a pass of 1,024, a block has four
waves; a lane decodes a unit of 16 sextets, and up to 15 are carried from pass
to pass.
"""
import base64
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
                                           guarded, np_skip_ref, records, skip_ref, strip)

ROOT = util.ROOT
CHUNK, PASS, WAVES = 16, 1024, 4
LF = 0x0A
ALL_KINDS = {OK, CHAR, PAD, BITS, LENGTH}


def cap_of(n: int) -> int:
    return (n + 3) // 4 * 3


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


# ---------------------------------------------------------------- rows --

def kept_text(E: int, seed: int, abc=STD, pads=None) -> bytes:
    """E characters the strict decoder accepts as plain text under abc: with
    pad E is a multiple of 4 and the text ends in `pads` (0..2, by the seed
    when None) pad characters; without pad E mod 4 is not 1."""
    _, pad, _ = alpha(abc)
    if pad:
        assert E % 4 == 0
        j = min(seed % 3 if pads is None else pads, E // 4 * 3)
        t = plain(_data(E // 4 * 3 - j, seed), abc)
    else:
        assert E % 4 != 1
        t = plain(_data(E // 4 * 3 + (0, 0, 1, 2)[E % 4], seed), abc)
    assert len(t) == E
    return t


def row_with(L: int, skipped, seed: int, abc=STD, sk: int = LF, pads=None) -> np.ndarray:
    """A row of L bytes the call accepts: the offsets in `skipped` (and up to
    three more at the end, to make the kept count one a text can have) hold
    the skipped byte sk, the others a valid text."""
    skipped = set(skipped)
    _, pad, _ = alpha(abc)
    p = L
    while (L - len(skipped)) % 4 if pad else (L - len(skipped)) % 4 == 1:
        p -= 1
        skipped.add(p)
    row = np.full(L, sk, np.uint8)
    keep = np.ones(L, bool)
    keep[np.array(sorted(skipped), np.int64)] = False
    row[keep] = np.frombuffer(kept_text(L - len(skipped), seed, abc, pads), np.uint8)
    return row


def fit(text: bytes, L: int) -> np.ndarray:
    """`text`, then line feeds up to L bytes."""
    assert len(text) <= L
    return np.frombuffer(text + b"\n" * (L - len(text)), np.uint8)


def want_of(row: np.ndarray, skip=CRLF, abc=STD):
    """((kind, pos, out_len), the bytes or None) of one row."""
    want = np_skip_ref(row, skip, abc)
    return want, (decode_kept(strip(row.tobytes(), skip), abc) if want[0] == OK else None)


def random_rows(count: int, L: int, seed: int = 0xD0E5):
    """Seeded rows of L bytes (90..110): encoder output of 60..72 bytes,
    skipped bytes sprinkled in up to the row's length, and -- for half of the
    rows -- one or two substitutions, deletions or insertions before that."""
    assert 90 <= L <= 110
    rng = random.Random(seed)
    pool = b"AQz9+/=-_. \t\x00\xff"
    rows = np.empty((count, L), np.uint8)
    for i in range(count):
        t = bytearray(base64.b64encode(rng.randbytes(rng.randrange(60, 64))))
        for _ in range(rng.choice((0, 0, 1, 2))):
            op = rng.randrange(3)
            p = len(t) - 1 - rng.randrange(5) if rng.random() < 0.5 else rng.randrange(len(t))
            if op == 0:
                t[p] = rng.choice(pool)
            elif op == 1:
                del t[p]
            else:
                t.insert(p, rng.choice(pool))
        while len(t) < L:
            t.insert(rng.randrange(len(t) + 1), rng.choice(CRLF))
        rows[i] = np.frombuffer(bytes(t), np.uint8)
    return rows


RANDOM_LEN = 107  # odd: with in_stride == len the rows start at every address mod 16


# ----------------------------------------------------------------- CPU --

def test_symbol_is_exported_and_declared():
    lib = _lib.load()
    name = "b64x_decode_strict_skip_strided"
    assert hasattr(lib, name)
    res, args = _lib.SIGNATURES[name]
    assert len(args) == 10 and getattr(lib, name).argtypes == args and res is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "b64x.h")).read()
    assert re.search(r"^int b64x_decode_strict_skip_strided\(", header, re.M)
    assert "#define B64X_ABI_VERSION 7" in header and b"abi=7" in lib.b64x_build_info()
    from async_amd import b64
    assert "decode_strict_skip_strided" in b64.__doc__ and callable(b64.decode_strict_skip_strided)


def _host_call():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def call(skip=None, abc=None, d_in=p, in_stride=64, length=40, nbuf=2, d_out=p, out_stride=64,
             d_res=p):
        return lib.b64x_decode_strict_skip_strided(d_in, in_stride, length, nbuf, d_out, out_stride,
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
    # 1. an empty batch is done before anything is looked at
    assert call(nine, bad_abc, d_in=None, d_res=None, nbuf=0, in_stride=0, out_stride=0) == 0
    # 2. NULL pointers and the records' alignment, before everything else
    for kw in ({"d_in": None}, {"d_res": None}, {"d_res": p + 4}):
        assert call(**kw) == -22, kw
        assert call(nine, bad_abc, in_stride=1, out_stride=1, **kw) == -22, kw
    # 3. the input stride, before the output stride, the skip set and the alphabet
    assert call(in_stride=39) == -22
    assert call(in_stride=39, d_out=None) == -22
    # 4. the output stride counts only with an output
    assert cap_of(40) == 30 and cap_of(41) == 33
    assert call(out_stride=29) == -22
    assert call(length=41, out_stride=32) == -22
    # 5. the skip set, before the alphabet
    for skip, abc in ((nine, a), (raw(1, b"A"), a), (raw(2, b"\n="), a), (raw(2, b"\n+"), a),
                      (raw(1, b"_"), _lib.alphabet("-", "_")), (nine, bad_abc), (raw(1, b"z"), bad_abc)):
        assert call(skip, abc) == -22
        assert call(skip, abc, d_out=None, out_stride=0) == -22
    # 6. the alphabet rules of the strict decoder
    for abc in (bad_abc, _lib.alphabet("A", "/"), _lib.alphabet(padchar="A"),
                _lib.alphabet("-", "_", True, "_")):
        assert call(None, abc) == -22
        assert call(None, abc, d_out=None) == -22
    # 7. valid calls reach the device check (with a device these host pointers
    # must never reach a kernel, so the calls are not made)
    if nodev:
        for kw in ({}, {"d_out": None, "out_stride": 0}, {"in_stride": 40, "out_stride": 30},
                   {"length": 0, "in_stride": 0, "out_stride": 0}, {"skip": raw(0, b"")},
                   {"skip": raw(1, b"="), "abc": _lib.alphabet(pad=False)},
                   {"d_in": p + 1, "d_out": p + 3, "in_stride": 41, "out_stride": 31}):
            assert call(**kw) == -19, kw


def test_no_gpu_is_enodev():
    lib, p, call = _host_call()
    if lib.b64x_device_check() != -19:
        return  # a device is there: the GPU tests make the valid calls
    for n in (0, 40, 41):
        for out in (p, None):
            assert call(length=n, d_out=out, nbuf=3) == -19


def test_wrapper_value_errors():
    """What the wrapper refuses without a device: a tensor that is not on one,
    and a skip set of nine bytes.  The wrapper refuses a CPU tensor before it
    looks at any size, so its size checks (buffers too small for the batch, a
    result under 24 * nbuf) cannot be reached here: test_wrapper_size_errors
    makes them, on device tensors."""
    from async_amd import b64
    cpu = torch.zeros(4096, dtype=torch.uint8)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_strided(cpu, 100, 100, 4, cpu, 80, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_strided(cpu, 100, 100, 4, None, 0, cpu)
    with pytest.raises(ValueError):
        b64.decode_strict_skip_strided(cpu, 100, 100, 4, cpu, 80, cpu, skip=b"123456789")


# The kernels of b64x_skip_rows.hip; nothing else may be in its code object.
ROWS_KERNELS = {"k_skip_decode_rows<true>", "k_skip_decode_rows<false>"}
TABLE_KERNELS = ROWS_KERNELS  # each builds the table behind its only barrier


def test_rows_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_skip_rows.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == ROWS_KERNELS, (got - ROWS_KERNELS, ROWS_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == len(TABLE_KERNELS)  # one each, after the table


def test_random_rows_cover_their_cases():
    assert hasattr(_lib.load(), "b64x_decode_strict_skip_strided")
    rows = random_rows(3000, RANDOM_LEN)
    kinds = [np_skip_ref(r)[0] for r in rows]
    assert set(kinds) == ALL_KINDS
    assert kinds.count(OK) * 3 >= len(kinds)
    for r in rows[:200]:
        assert np_skip_ref(r) == skip_ref(r.tobytes())


# ----------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


@gpu
def test_wrapper_size_errors():
    """The size checks of decode_strict_strided: no call reaches the library."""
    b64 = _b64()
    x = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    res = torch.zeros(REC * 4, dtype=torch.uint8, device="cuda")
    for kw in ({"nbuf": 5},                              # result under 24 * nbuf
               {"in_stride": 301},                       # 3 * 301 + 100 > 1,000
               {"out_stride": 309},                      # 3 * 309 + 75 > 1,000
               {"length": 400, "in_stride": 400}):       # 3 * 400 + 400 > 1,000
        args = {"in_stride": 300, "length": 100, "nbuf": 4, "out_stride": 300}
        args.update(kw)
        with pytest.raises(ValueError):
            b64.decode_strict_skip_strided(x, args["in_stride"], args["length"], args["nbuf"], out,
                                           args["out_stride"], res)
        if "out_stride" not in kw:
            with pytest.raises(ValueError):  # validate only: the same, less the output's size
                b64.decode_strict_skip_strided(x, args["in_stride"], args["length"], args["nbuf"],
                                               None, 0, res)


def run_rows(rows, skip=CRLF, abc=STD, in_stride=None, out_stride=None, in_base=0, out_base=0,
             validate_only=False, wants=None):
    """One call over `rows` (a 2-D uint8 array, or a list of equally long
    arrays): row i at in_base + i*in_stride of an input of FILL bytes, its
    bytes to out_base + i*out_stride of an output of FILL bytes (both strides
    leave GUARD bytes between rows unless given), a guard behind the records;
    one copy back.  Returns the records."""
    b64 = _b64()
    rows = np.asarray(rows, np.uint8)
    nbuf, L = rows.shape
    cap = cap_of(L)
    if in_stride is None:
        in_stride = -(-(L + GUARD) // 16) * 16
    if out_stride is None:
        out_stride = -(-(cap + GUARD) // 16) * 16
    in_base += GUARD
    out_base += GUARD
    host = np.full(in_base + nbuf * in_stride + L + GUARD, FILL, np.uint8)
    for i in range(nbuf):
        host[in_base + i * in_stride:in_base + i * in_stride + L] = rows[i]
    x = torch.from_numpy(host).cuda()
    out = torch.full((out_base + nbuf * out_stride + cap + GUARD,), FILL, dtype=torch.uint8,
                     device="cuda")
    res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
    if wants is None:
        wants = [want_of(r, skip, abc) for r in rows]
    b64.decode_strict_skip_strided(x[in_base:], in_stride, L, nbuf,
                                   None if validate_only else out[out_base:], out_stride,
                                   res[:REC * nbuf], skip, abc)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    recs = records(res)[:nbuf]
    assert (res[REC * nbuf:].cpu().numpy() == FILL).all(), "the guard behind the records"
    mask = np.ones(got.size, bool)
    for i, (rec, (want, data)) in enumerate(zip(recs, wants)):
        o = out_base + i * out_stride
        label = (i, L, (in_base + i * in_stride) % 16, o % 16, skip, abc, validate_only)
        assert rec == (want[0], want[1], want[2], 0), (label, rec, want)
        if not validate_only:
            mask[o:o + cap] = False
    if not validate_only:
        for i, (want, data) in enumerate(wants):  # after every row's mask: strides may be tight
            if want[0] == OK and data is not None:
                o = out_base + i * out_stride
                assert got[o:o + want[2]].tobytes() == data, (i, L, o % 16)
    assert (got[mask] == FILL).all(), "a byte outside the rows' capacities was overwritten"
    return recs


def good_row():
    """A CRLF-76 row of 2,106 bytes ending in one pad character and CRLF."""
    t = crlf76(_data(1538, 3))
    assert len(t) == 2106 and t.endswith(b"=\r\n") and not t.endswith(b"==\r\n")
    return np.frombuffer(t, np.uint8)


REPLACEMENTS = (0x00, 0x3D, 0x0A, 0x2F)  # junk, the pad character, a skipped byte, low bits set


@gpu
def test_every_byte_is_judged():
    t = good_row()
    W = t.size
    rows = np.tile(t, (W * len(REPLACEMENTS), 1))
    for p in range(W):
        for j, v in enumerate(REPLACEMENTS):
            rows[p * len(REPLACEMENTS) + j, p] = v
    wants = [want_of(r) for r in rows]
    assert {w[0][0] for w in wants} == ALL_KINDS
    for i in range(0, len(rows), 97):
        assert wants[i][0] == skip_ref(rows[i].tobytes())
    for p in range(W - 8):  # the junk byte itself, wherever it stands
        assert wants[p * len(REPLACEMENTS)][0] == (CHAR, p, 0)
    # every row at address 0 mod 16 on both sides; then with odd strides, the rows at
    # every address mod 16 on both sides
    run_rows(rows, wants=wants)
    in_stride, out_stride = W + GUARD + 1, cap_of(W) + GUARD + 2
    assert in_stride % 2 == 1 and out_stride % 2 == 1
    run_rows(rows, wants=wants, in_stride=in_stride, in_base=5, out_stride=out_stride, out_base=7)


LENGTHS = list(range(0, 22)) + [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]


def length_rows(n: int):
    """Rows of n bytes: accepted ones of every kept count mod 4 that fits,
    with the skipped bytes nowhere, in CRLF-76 lines and scattered; one byte
    too many; skipped bytes only; one offence of each kind at a byte; and for
    n <= 3 every text over "Q=\\nA*"."""
    rng = random.Random(n)
    rows = [np.full(n, LF, np.uint8), np.frombuffer((b"\r\n" * n)[:n], np.uint8)]
    for nskip in range(0, min(n, 7) + 1):
        if (n - nskip) % 4 == 0:
            rows.append(row_with(n, rng.sample(range(n), nskip), n + nskip))
            rows.append(row_with(n, range(n - nskip, n), n + nskip + 1))
            rows.append(row_with(n, range(nskip), n + nskip + 2))
        elif n > nskip:  # a kept count no text with pad has
            bad = row_with(n + 4 - (n - nskip) % 4, [], n)[:n].copy()
            bad[np.array(rng.sample(range(n), nskip), np.int64)] = LF
            rows.append(bad)
    if n >= 4 and n % 4 == 0:
        for p, v in ((n - 2, ord("/")), (0, ord("=")), (n - 1, ord("*"))):  # BITS, PAD, CHAR
            row = row_with(n, [], n + 3, pads=1)
            row[p] = v
            rows.append(row)
    if n >= 78:
        lines = crlf76(_data(n, n))[:n]
        rows.append(row_with(n, [i for i in range(n) if lines[i] in CRLF], n))
    if n <= 3:
        import itertools
        rows += [np.frombuffer(bytes(c), np.uint8) for c in itertools.product(b"Q=\nA*", repeat=n)]
    return np.array(rows, np.uint8).reshape(len(rows), n)


@gpu
def test_lengths():
    kinds = set()
    for n in LENGTHS:
        rows = length_rows(n)
        wants = [want_of(r) for r in rows]
        kinds |= {w[0][0] for w in wants}
        assert wants[0][0] == (OK, 0, 0) and wants[1][0] == (OK, 0, 0)  # skipped bytes only
        if n % 4 == 0:
            assert wants[2][0][0] == OK
        for abc in (STD, NOPAD):
            w = wants if abc == STD else None
            run_rows(rows, abc=abc, wants=w)
            run_rows(rows, abc=abc, wants=w, in_stride=n + GUARD + 1, in_base=9,
                     out_stride=cap_of(n) + GUARD + 1, out_base=2)
    assert kinds == ALL_KINDS


@gpu
def test_the_carry():
    """A row that starts at address s mod 16 has its passes end at row offsets
    1,024 - s and 2,048 - s; r = 0..3 skipped bytes before one of them leave
    every count of kept bytes mod 4 (and, with the rows' own starts, every
    carry 0..15) behind the pass.  The odd stride gives every s."""
    L = 2100
    stride = L + GUARD + 1
    assert {i * stride % 16 for i in range(16)} == set(range(16))
    rows = []
    for i in range(16 * 8):
        s, edge, r = i * stride % 16, 1 + (i // 16) % 2, i // 32
        end = PASS * edge - s
        rows.append(row_with(L, range(end - 5 - r, end - 5), i))
    wants = [want_of(r) for r in rows]
    assert all(w[0][0] == OK for w in wants)
    assert (cap_of(L) + GUARD) % 2 == 1  # outputs at every address mod 16, then all at 0 mod 4
    run_rows(rows, wants=wants, in_stride=stride, out_stride=cap_of(L) + GUARD)
    run_rows(rows, wants=wants, in_stride=stride, out_stride=cap_of(L) + GUARD + 1)
    # passes without a kept byte, pads and the BITS character across passes
    L = 7400
    body = kept_text(2000, 5, pads=0)
    two = kept_text(1024, 6, pads=2)
    one = kept_text(1024, 7, pads=1)
    assert two.endswith(b"==") and one.endswith(b"=") and not one.endswith(b"==")
    bits = bytearray(kept_text(1024, 8, pads=2))
    bits[-3] = ord("/")   # u[D - 1] with its low four bits set
    low = bytearray(kept_text(904, 9, pads=1))
    low[-2] = ord("/")    # u[D - 1] with its low two bits set
    texts = [
        body[:1000] + b"\n" * 1024 + body[1000:],                 # a pass of skipped bytes only
        body[:1001] + b"\n" * 2049 + body[1001:],
        b"\n" * 1024 + body, b"\r\n" * 1024 + b"\n" + body,
        two[:-1] + b"\r\n=" + b"\n" * 5000,                       # 5,000 skipped bytes behind the pads
        two[:-2] + b"\n" * 5000 + b"=\r\n=",
        b"\n" + two,                                              # the pads either side of a pass edge
        b"\n" * 1025 + two,
        one[:-1] + b"\n" * 1024 + b"=",
        bytes(bits[:-2]) + b"\n" * 10 + b"==",                    # BITS: the character before the pads'
        bytes(bits[:-2]) + b"\n" * 1024 + b"=" + b"\n" * 2049 + b"=",   # pass, and two passes earlier
        bytes(low[:-1]) + b"\n" * 3000 + b"=",
        bytes(low[:-1]) + b"\n" * 100 + b"=" + b"\n" * 3000,
    ]
    rows = [fit(t, L) for t in texts]
    wants = [want_of(r) for r in rows]
    assert [w[0] for w in wants[:9]] == [(OK, 0, 1500)] * 4 + [(OK, 0, 766)] * 4 + [(OK, 0, 767)]
    assert [w[0] for w in wants[9:]] == [(BITS, 1021, 0), (BITS, 1021, 0), (BITS, 902, 0),
                                         (BITS, 902, 0)]
    for r, w in zip(rows, wants):
        assert w[0] == skip_ref(r.tobytes())
    for base in (0, 3):
        run_rows(rows, wants=wants, in_base=base, out_base=base)


@gpu
def test_lowest_offset_wins():
    L = 3 * PASS + 5
    b = fit(b"\n" * 40 + crlf76(_data(2200, 8)), L)
    assert np_skip_ref(b)[0] == OK
    J, P = 0x00, 0x3D

    def ch(p):  # the nearest character at or after p
        while int(b[p]) in CRLF:
            p += 1
        return p
    spots = [
        [(ch(5 * CHUNK + 2), J), (ch(5 * CHUNK + 13), P)],            # one chunk, both orders
        [(ch(5 * CHUNK + 3), P), (ch(5 * CHUNK + 12), J)],
        [(ch(70), P), (ch(PASS + 3), J)],                             # a PAD a pass before a CHAR
        [(ch(70), J), (ch(PASS + 3), P)],
        [(ch(PASS + 3), P), (ch(2 * PASS + 70), J), (ch(3 * PASS - 40), P)],
        [(ch(PASS - 1), J), (ch(PASS + 1), P)],                       # across a pass edge
        [(ch(PASS - 1), P), (ch(PASS + 1), J)],
        [(ch(2 * PASS + 300), P), (ch(2 * PASS - 1), J), (ch(80), P)],
        [(ch(2 * PASS + 100), J), (ch(9 * CHUNK), J), (ch(PASS + 9), P)],
    ]
    rows, wants = [b], [want_of(b)]
    for sp in spots:
        u = b.copy()
        for p, v in sp:
            u[p] = v
        w = want_of(u)
        first = min(sp)
        assert w[0] == (PAD if first[1] == P else CHAR, first[0], 0), (sp, w)
        rows.append(u)
        wants.append(w)
    for base in (0, 11):
        run_rows(rows, wants=wants, in_base=base, out_base=16 - base)


@gpu
def test_alignment_and_capacity():
    """in_stride 1,403 and out_stride 1,053 == b64x_decoded_cap(1,402), both
    odd: 64 rows start at every address mod 16 on either side, back to back on
    the output side, so a byte too many would spoil the next row's."""
    b64 = _b64()
    L, nbuf = 1402, 64
    cap = b64.decoded_cap(L)
    assert cap == cap_of(L) == 1053
    mime = [np.frombuffer(crlf76(_data(1024, i))[:-2], np.uint8) for i in range(nbuf)]
    full = [row_with(L, [], i, NOPAD) for i in range(nbuf)]  # 1,402 characters: 1,051 bytes of 1,053
    assert all(r.size == L for r in mime + full)
    for rows, abc, out_len in ((mime, STD, 1024), (full, NOPAD, 1051)):
        wants = [want_of(r, CRLF, abc) for r in rows]
        assert all(w[0] == (OK, 0, out_len) for w in wants)
        run_rows(rows, abc=abc, wants=wants, in_stride=L + 1, out_stride=cap)
        run_rows(rows, abc=abc, wants=wants, in_stride=L, out_stride=cap, in_base=1, out_base=1)
        # every third row offending, late enough for most of its bytes to be written
        rng = random.Random(out_len)
        spoiled = [r.copy() for r in rows]
        for i in range(0, nbuf, 3):
            spoiled[i][rng.randrange(L - 300, L - 8)] = rng.choice(b"*\x00 \xff")
        wants = [want_of(r, CRLF, abc) for r in spoiled]
        assert all((w[0][0] == CHAR) == (i % 3 == 0) for i, w in enumerate(wants))
        run_rows(spoiled, abc=abc, wants=wants, in_stride=L + 1, out_stride=cap)


EIGHT = b"\r\n\t \x0b\x0c\x00\xff"


@gpu
def test_alphabets_and_skip_sets():
    L = 1100
    kinds = set()
    for abc in (STD, NOPAD, URL, DOTPAD):
        chars, pad, padc = alpha(abc)
        for skip in (CRLF, b"\n", b" \t\r\n", b"", EIGHT):
            rng = random.Random(len(skip))
            rows = []
            for seed in range(3):
                where = rng.sample(range(L), 37 + seed) if skip else []
                row = row_with(L, where, seed, abc, sk=skip[0] if skip else 0)
                for p in np.flatnonzero(row == skip[0]) if skip else []:
                    row[p] = rng.choice(skip)
                rows.append(row)
            base = rows[1]
            kept = [p for p in range(L) if base[p] not in skip]
            # a stranger, the pad character, bytes that some sets skip, low bits set
            for p in (kept[0], kept[len(kept) // 2], kept[-1], kept[-2]):
                for v in (0x2A, padc, 0x0D, 0x20, chars[63]):
                    u = base.copy()
                    u[p] = v
                    rows.append(u)
            wants = [want_of(r, skip, abc) for r in rows]
            assert all(w[0][0] == OK for w in wants[:3])
            for r, w in zip(rows[::5], wants[::5]):
                assert w[0] == skip_ref(r.tobytes(), skip, abc)
            kinds |= {w[0][0] for w in wants}
            run_rows(rows, skip, abc, wants=wants, in_base=len(skip), out_base=3 * len(skip))
    assert kinds == ALL_KINDS


@gpu
def test_validate_only():
    rows = random_rows(600, RANDOM_LEN, seed=7)
    wants = [want_of(r) for r in rows]
    dec = run_rows(rows, wants=wants, in_stride=RANDOM_LEN)
    val = run_rows(rows, wants=wants, in_stride=RANDOM_LEN, validate_only=True)  # `out` keeps its FILL
    assert dec == val
    t = good_row()
    rows = np.tile(t, (40, 1))
    for i in range(1, 40):
        rows[i, (i * 53) % t.size] = (0x00, 0x3D, 0x2F)[i % 3]
    assert run_rows(rows) == run_rows(rows, validate_only=True)


_many = {}


def many_rows():
    """The rows of the two tests below, their records and bytes: made once."""
    if not _many:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        nbuf = 2 * (cus * 8 * WAVES) + 5
        rows = random_rows(nbuf, RANDOM_LEN, seed=cus)
        rows.setflags(write=False)
        _many.update(cus=cus, rows=rows, wants=[want_of(r) for r in rows])
    return _many


@gpu
def test_more_rows_than_waves():
    m = many_rows()
    assert len(m["rows"]) == 2 * (m["cus"] * 32) + 5
    kinds = [w[0][0] for w in m["wants"]]
    assert set(kinds) == ALL_KINDS and kinds.count(OK) * 3 >= len(kinds)
    run_rows(m["rows"], wants=m["wants"], in_stride=RANDOM_LEN, out_stride=cap_of(RANDOM_LEN) + 1)


@gpu
def test_same_answer_as_the_ragged_call():
    b64 = _b64()
    m = many_rows()
    rows, wants = m["rows"], m["wants"]
    nbuf, L = rows.shape
    cap = cap_of(L)
    x = torch.from_numpy(rows.reshape(-1).copy()).cuda()
    in_off = torch.arange(nbuf + 1, dtype=torch.int64, device="cuda") * L
    out_off = torch.arange(nbuf, dtype=torch.int64, device="cuda") * cap
    got = []
    for ragged in (False, True):
        out = torch.full((nbuf * cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if ragged:
            b64.decode_strict_skip_batch(x, in_off, out, out_off, res[:REC * nbuf])
        else:
            b64.decode_strict_skip_strided(x, L, L, nbuf, out, cap, res[:REC * nbuf])
        torch.cuda.synchronize()
        assert (res[REC * nbuf:].cpu().numpy() == FILL).all()
        assert (out[nbuf * cap:].cpu().numpy() == FILL).all()
        got.append((records(res)[:nbuf], out.cpu().numpy()))
    assert got[0][0] == got[1][0]
    for i, (want, data) in enumerate(wants):
        assert got[0][0][i] == (want[0], want[1], want[2], 0)
        if want[0] == OK:
            a, b = (g[1][i * cap:i * cap + want[2]].tobytes() for g in got)
            assert a == b == data, i


@gpu
def test_round_trip():
    b64 = _b64()
    nbuf, n = 4099, 1024
    payload = torch.from_numpy(util.splitmix64(23, nbuf * n)).cuda()
    for line_len, sep, trailing, W in ((76, b"\r\n", True, 1404), (64, b"\n", False, 1389)):
        assert b64.encoded_lines_len(n, line_len, sep, trailing) == W
        stride = W + 3
        text = torch.full((nbuf * stride + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        b64.encode_lines_strided(payload, n, n, nbuf, text, stride, line_len, sep, trailing)
        cap = b64.decoded_cap(W)
        out = torch.full((nbuf * cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        b64.decode_strict_skip_strided(text, stride, W, nbuf, out, cap, res[:REC * nbuf])
        torch.cuda.synchronize()
        o = out[:nbuf * cap].view(nbuf, cap)
        assert torch.equal(o[:, :n], payload.view(nbuf, n))
        assert bool((o[:, n:] == FILL).all()) and (out[nbuf * cap:].cpu().numpy() == FILL).all()
        r = res.cpu().numpy()
        assert (r[REC * nbuf:] == FILL).all()
        rec = r[:REC * nbuf].reshape(nbuf, REC)
        assert (rec[:, :8].copy().view(np.uint64) == n).all() and not rec[:, 8:].any()


@gpu
def test_rows_past_2gib_apart():
    """Three rows 2^31 + 48 bytes apart: i*in_stride needs 64 bits."""
    b64 = _b64()
    stride = (1 << 31) + 48
    t = good_row()
    L = t.size
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * stride + L + (1 << 30):
        pytest.skip("the device has no room for rows 2^31 bytes apart")
    x = torch.empty(2 * stride + L, dtype=torch.uint8, device="cuda")
    rows = np.tile(t, (3, 1))
    rows[1, 0], rows[1, 1] = rows[1, 1], rows[1, 0]  # another row, still accepted
    rows[2, 1777] = 0x7E
    for i in range(3):
        x[i * stride:i * stride + L].copy_(torch.from_numpy(rows[i].copy()))
    cap = cap_of(L)
    out_all, out = guarded(3 * cap)
    res = torch.full((3 * REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip_strided(x, stride, L, 3, out, cap, res[:3 * REC])
    torch.cuda.synchronize()
    got = records(res)
    wants = [want_of(r) for r in rows]
    assert wants[0][0][0] == OK and wants[1][0][0] == OK and wants[2][0] == (CHAR, 1777, 0)
    o = out.cpu().numpy()
    for i, (want, data) in enumerate(wants):
        assert got[i] == (want[0], want[1], want[2], 0)
        if data is not None:
            assert o[i * cap:i * cap + want[2]].tobytes() == data
    assert (res[3 * REC:].cpu().numpy() == FILL).all()
    a = out_all.cpu().numpy()
    assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all()


@gpu
def test_graph_capture():
    b64 = _b64()
    t = good_row()
    L, nbuf = t.size, 9
    stride, cap = L + 7, cap_of(L)
    good = np.full(nbuf * stride, FILL, np.uint8)
    for i in range(nbuf):
        good[i * stride:i * stride + L] = t
    spoiled = good.copy()
    spoiled[4 * stride + 1500] = 0x20
    spoiled[7 * stride + 3] = 0x3D
    x = torch.from_numpy(good.copy()).cuda()
    out_all, out = guarded(nbuf * cap)
    res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.decode_strict_skip_strided(x, stride, L, nbuf, out, cap, res[:REC * nbuf])  # warm-up
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b64.decode_strict_skip_strided(x, stride, L, nbuf, out, cap, res[:REC * nbuf])
    payload = _data(1538, 3)
    seen = []
    for content in (good, spoiled, good):
        x.copy_(torch.from_numpy(content.copy()).cuda())
        out.fill_(FILL)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        recs = records(res)[:nbuf]
        o = out.cpu().numpy()
        for i in range(nbuf):
            want = np_skip_ref(content[i * stride:i * stride + L])
            assert recs[i] == (want[0], want[1], want[2], 0), (i, recs[i], want)
            if want[0] == OK:
                assert o[i * cap:i * cap + want[2]].tobytes() == payload
        seen.append(recs)
        assert (res[REC * nbuf:].cpu().numpy() == FILL).all()
        a = out_all.cpu().numpy()
        assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all()
    assert seen[0] == seen[2] != seen[1]
    assert seen[1][4] == (CHAR, 1500, 0, 0) and seen[1][7] == (PAD, 3, 0, 0)
