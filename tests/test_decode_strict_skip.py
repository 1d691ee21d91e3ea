"""Strict decode that skips line breaks (b64x_decode_strict_skip_dev / _batch,
async_amd.b64 decode_strict_skip / decode_strict_skip_batch): the record and
the bytes, bit for bit, against the scalar procedure of include/b64x.h written
here in plain Python (skip_ref), a vectorised copy of it for the large cases
(np_skip_ref, checked against the scalar one on the CPU), the strict
decoder's reference on the text with the skipped bytes taken out, and the
stdlib.

CPU tests: the references against each other and the contract's consequence
(accepted <=> the plain strict decoder accepts the kept bytes, same bytes),
the exports, the workspace sizes, every -EINVAL case in its order, -ENODEV
without a device, and the new code object's kernel list and barriers.  GPU
tests lay their cases out in one arena with 64 guard bytes of 0xA5 around
every output, behind the records and around the workspace, copy back once and
check outputs, records and guards.
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
from tests.test_decode_strict import (BITS, CHAR, FILL, GUARD, LENGTH, NOPAD, OK, PAD, REC, SEP,
                                      STD, _STD, _table, alpha, plain, records, ref_text,
                                      stdlib_decode, strict_ref)

ROOT = util.ROOT

# The unit's sizes (async_amd/csrc/b64x_skip.hip): a lane takes a chunk of 16
# bytes at a 16-byte aligned address (kChunk), a wave a pass of 1,024
# (the batch kernel's pass and the backward walk's step, kWalkStep), a
# 256-lane block a tile of 4,096; the one-buffer grid has at most 2,048 blocks
# (kSkipMaxGrid: 8 MiB to a round), each with a 32-byte slot behind the 64
# bytes of the lenient decoder's record in the workspace head (kHeadBytes).
LANE, WAVE, TILE = 16, 1024, 4096
STEP = 1024
MAX_GRID = 2048
HEAD = (64 + MAX_GRID * 32 + 255) // 256 * 256

CRLF = b"\r\n"
URL = ("-", "_", True, -1)
DOTPAD = (-1, -1, True, ".")


# ------------------------------------------------------------ references --

def strip(t: bytes, skip=CRLF) -> bytes:
    return t.translate(None, skip)


def decode_kept(u: bytes, abc=STD) -> bytes:
    """The stdlib's decode of the kept bytes of an accepted text."""
    chars, pad, padc = alpha(abc)
    body = u.translate(bytes.maketrans(chars, _STD[:64]), bytes([padc]) if pad else b"")
    return base64.b64decode(body + b"=" * (-len(body) % 4), validate=True)


def skip_ref(t: bytes, skip=CRLF, abc=STD):
    """The scalar procedure of the contract: (kind, pos, out_len)."""
    chars, pad, padc = alpha(abc)
    # 1. kept bytes
    kept = [(p, b) for p, b in enumerate(t) if b not in skip]
    E = len(kept)
    # 2. pads
    npad = 0
    if pad and E and kept[E - 1][1] == padc:
        npad = 2 if E >= 2 and kept[E - 2][1] == padc else 1
    D = E - npad
    # 3. offences at a byte, in offset order
    for p, b in kept[:D]:
        if pad and b == padc:
            return PAD, p, 0
        if b not in chars:
            return CHAR, p, 0
    # 4. length
    if (pad and E % 4) or (not pad and E % 4 == 1):
        return LENGTH, len(t), 0
    # 5. unused bits
    if D and D % 4 in (2, 3):
        p, b = kept[D - 1]
        if chars.index(b) & (15 if D % 4 == 2 else 3):
            return BITS, p, 0
    # 6. accepted
    return OK, 0, 3 * (D // 4) + (0, 0, 1, 2)[D % 4]


def skip_bytes(t: bytes, skip=CRLF, abc=STD) -> bytes:
    """The bytes of the D sextets of an accepted text, bit by bit."""
    chars, pad, padc = alpha(abc)
    acc = nbits = 0
    out = bytearray()
    for b in t:
        if b in skip or (pad and b == padc):
            continue
        acc = (acc << 6) | chars.index(b)
        nbits += 6
        if nbits >= 8:
            nbits -= 8
            out.append((acc >> nbits) & 0xFF)
    return bytes(out)


def np_skip_ref(t: np.ndarray, skip=CRLF, abc=STD):
    """skip_ref, vectorised: (kind, pos, out_len) for a uint8 array."""
    tab, pad, padc = _table(abc)
    n = int(t.size)
    keep = np.ones(n, bool)
    for b in set(skip):
        keep &= t != b
    pos = np.flatnonzero(keep)
    E = int(pos.size)
    npad = 0
    if pad and E and t[pos[E - 1]] == padc:
        npad = 2 if E >= 2 and t[pos[E - 2]] == padc else 1
    D = E - npad
    cls = tab[t[pos[:D]]]
    bad = np.flatnonzero(cls & 0x80)
    if bad.size:
        return (PAD if cls[bad[0]] & 0x40 else CHAR), int(pos[bad[0]]), 0
    if (pad and E % 4) or (not pad and E % 4 == 1):
        return LENGTH, n, 0
    if D and D % 4 in (2, 3) and cls[D - 1] & (15 if D % 4 == 2 else 3):
        return BITS, int(pos[D - 1]), 0
    return OK, 0, 3 * (D // 4) + (0, 0, 1, 2)[D % 4]


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


def crlf76(data: bytes, abc=STD) -> bytes:
    return ref_text(data, 76, CRLF, True, abc)


# ------------------------------------------------------------------- CPU --

def random_texts(count, seed=0x5C1B):
    """Seeded small texts: encoder output under a random line format, skipped
    bytes sprinkled in, then up to two substitutions, deletions or insertions;
    with the skip set and the alphabet to judge them under."""
    rng = random.Random(seed)
    pool = b"AQz9+/=-_. \t\r\n\x00\xff"
    for i in range(count):
        abc = (STD, NOPAD, URL, DOTPAD)[i % 4]
        skip = (CRLF, b"\n", b" \t\r\n", b"")[(i // 4) % 4]
        n = rng.choice((rng.randrange(0, 8), rng.randrange(0, 120)))
        t = bytearray(plain(bytes(rng.randrange(256) for _ in range(n)), abc))
        for _ in range(rng.randrange(0, 6)):
            t.insert(rng.randrange(len(t) + 1), rng.choice(skip or b"\n"))
        for _ in range(rng.randrange(0, 3)):
            op = rng.randrange(3)
            near_end = rng.random() < 0.5
            if op == 0 and t:
                p = len(t) - 1 - rng.randrange(min(len(t), 5)) if near_end else rng.randrange(len(t))
                t[p] = rng.choice(pool)
            elif op == 1 and t:
                del t[len(t) - 1 - rng.randrange(min(len(t), 5)) if near_end
                      else rng.randrange(len(t))]
            elif op == 2:
                t.insert(rng.randrange(len(t) + 1), rng.choice(pool))
        yield bytes(t), skip, abc


def check_contract(t: bytes, skip, abc):
    """skip_ref against the strict reference on the kept bytes; the kind."""
    kind, pos, out_len = got = skip_ref(t, skip, abc)
    u = strip(t, skip)
    assert (kind == OK) == (strict_ref(u, None, b"", True, abc)[0] == OK), (t, skip, abc)
    if kind == OK:
        assert out_len == strict_ref(u, None, b"", True, abc)[2]
        data = skip_bytes(t, skip, abc)
        assert len(data) == out_len and data == stdlib_decode(u, abc) == decode_kept(u, abc), \
            (t, skip, abc)
        if abc == STD:
            assert data == base64.b64decode(u, validate=True)
    elif kind == LENGTH:
        assert pos == len(t)
    else:
        assert kind != SEP and 0 <= pos < len(t) and t[pos] not in skip
    return got


def test_np_reference_agrees():
    kinds = set()
    for t, skip, abc in random_texts(2000):
        want = skip_ref(t, skip, abc)
        assert np_skip_ref(np.frombuffer(t, np.uint8), skip, abc) == want, (t, skip, abc)
        kinds.add(want[0])
    assert kinds == {OK, CHAR, PAD, BITS, LENGTH}


MUTANTS = (0x00, 0x3D, 0x0D, 0x0A, 0x41, 0x42, 0x51, 0x2F, 0x20, 0xFF)


def test_reference_self_check():
    kinds = set()
    for t, skip, abc in random_texts(3000, seed=7):
        kinds.add(check_contract(t, skip, abc)[0])
    assert kinds == {OK, CHAR, PAD, BITS, LENGTH}
    # every single-byte mutation of a 200-byte CRLF-76 text
    text = crlf76(_data(143, 5)) + b"\r\n"
    assert len(text) == 200 and text.endswith(b"=\r\n\r\n") and not text.endswith(b"==\r\n\r\n")
    assert check_contract(text, CRLF, STD) == (OK, 0, 143)
    kinds = set()
    for i in range(len(text)):
        for v in MUTANTS:
            u = bytearray(text)
            u[i] = v
            kinds.add(check_contract(bytes(u), CRLF, STD)[0])
    assert kinds == {OK, CHAR, PAD, BITS, LENGTH}


def test_exports_and_sizes():
    lib = _lib.load()
    want = {"b64x_strict_skip_workspace_size": 2, "b64x_decode_strict_skip_dev": 8,
            "b64x_decode_strict_skip_batch": 10}
    for name, arity in want.items():
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity and getattr(lib, name).argtypes == args
    for n in (0, 1, 4096, 1 << 20, 1 << 30, (1 << 32) + 4101):
        assert lib.b64x_strict_skip_workspace_size(n, True) == HEAD
        assert lib.b64x_strict_skip_workspace_size(n, False) == \
            HEAD + lib.b64x_decode_workspace_size(n)
    assert b"abi=7" in lib.b64x_build_info()
    from async_amd import b64
    assert b64.strict_skip_workspace_size(100, True) == HEAD
    off = b64.skip_batch_layout(torch.tensor([0, 0, 1, 5, 13, 113]), align=4)
    assert off.tolist() == [0, 0, 4, 8, 16, 92]
    with pytest.raises(ValueError):
        _lib.skip_set(b"123456789")


def test_invalid_arguments():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * (HEAD + 256))()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    a = _lib.alphabet()
    url = _lib.alphabet("-", "_")
    nopad = _lib.alphabet(pad=False)
    bad_abc = _lib.alphabet("+", "+")
    nodev = lib.b64x_device_check() == -19

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def raw(n, b):
        return _lib.Skip(n, (ctypes.c_uint8 * 8)(*b))

    def dev(skip=None, abc=a, n=40, d_in=p, d_out=p, d_res=p, ws=p):
        return lib.b64x_decode_strict_skip_dev(d_in, n, d_out, d_res, ref(abc), ref(skip), ws, None)

    def batch(skip=None, abc=a, nbuf=2, d_in=p, off=p, d_out=p, out_off=p, d_res=p, ws=p):
        return lib.b64x_decode_strict_skip_batch(d_in, off, nbuf, d_out, out_off, d_res, ref(abc),
                                                 ref(skip), ws, None)

    def valid(call, *args, **kw):
        # a valid call stops at the device check; with a device these host
        # pointers must never reach a kernel, so it is not made
        if nodev:
            assert call(*args, **kw) == -19, (args, kw)

    nine = raw(9, b"\r\n\t \x0b\x0c\x00\x01")
    # 1. an empty batch is done before anything is looked at
    assert batch(nbuf=0, d_in=None, off=None, d_res=None, skip=nine, abc=bad_abc) == 0
    # 2. NULL pointers and alignment, before the skip set and the alphabet
    for kw in ({"d_in": None}, {"d_res": None}, {"ws": None}, {"d_res": p + 4}, {"ws": p + 4}):
        for n in (0, 40):
            assert dev(n=n, **kw) == -22, kw
            assert dev(n=n, skip=nine, **kw) == -22
    for kw in ({"d_in": None}, {"d_res": None}, {"off": None}, {"out_off": None}, {"ws": None},
               {"d_res": p + 4}):
        assert batch(**kw) == -22, kw
    # d_out may be NULL; a validate-only batch needs neither out_off nor a workspace
    valid(dev, d_out=None)
    valid(batch, d_out=None, out_off=None, ws=None)
    # 3. the skip set, before the alphabet
    for skip, abc in ((nine, a), (raw(1, b"A"), a), (raw(2, b"\n+"), a), (raw(2, b"\n="), a),
                      (raw(3, b"\r\n-"), url), (raw(1, b"_"), url), (raw(8, b"\r\n\t \x0b\x0c\x009"), a),
                      (nine, bad_abc), (raw(1, b"z"), bad_abc)):
        assert dev(skip, abc) == -22, (skip.n, bytes(skip.bytes))
        assert dev(skip, abc, d_out=None) == -22
        assert batch(skip, abc) == -22
        assert batch(skip, abc, d_out=None, out_off=None, ws=None) == -22
    # 4. the alphabet rules of the strict decoder
    for abc in (bad_abc, _lib.alphabet("A", "/"), _lib.alphabet(padchar="A"),
                _lib.alphabet("-", "_", True, "_")):
        assert dev(None, abc) == -22
        assert batch(None, abc) == -22
    # 5. valid calls reach the device check: '=' may be skipped without pad,
    # '-' and '+' where they are no characters, duplicates, the empty set
    for skip, abc in ((None, a), (raw(0, b""), a), (raw(1, b"="), nopad), (raw(2, b"-_"), a),
                      (raw(2, b"+/"), url), (raw(4, b"\n\n\n\n"), a),
                      (raw(8, b"\r\n\t \x0b\x0c\x00\x01"), a),
                      (raw(1, b"\nA"), a)):  # a byte beyond n is not looked at
        valid(dev, skip, abc)
        valid(dev, skip, abc, n=0)
        valid(batch, skip, abc)


def test_no_gpu_is_enodev():
    lib = _lib.load()
    if lib.b64x_device_check() != -19:
        return  # a device is there: the GPU tests make the valid calls
    buf = (ctypes.c_uint8 * (HEAD + 256))()
    p = ctypes.addressof(buf)
    for n in (0, 40, 41):
        for out in (p, None):
            assert lib.b64x_decode_strict_skip_dev(p, n, out, p, None, None, p, None) == -19
    assert lib.b64x_decode_strict_skip_batch(p, p, 3, p, p, p, None, None, p, None) == -19
    assert lib.b64x_decode_strict_skip_batch(p, p, 3, None, None, p, None, None, None, None) == -19


# The kernels of b64x_skip.hip; nothing else may be in its code object.
SKIP_KERNELS = {"k_skip_check", "k_skip_finish", "k_skip_check_batch"}
TABLE_KERNELS = {"k_skip_check", "k_skip_check_batch"}  # k_skip_finish is one wave, no table


def test_skip_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_skip.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == SKIP_KERNELS, (got - SKIP_KERNELS, SKIP_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == len(TABLE_KERNELS)  # one each, after the table


# ------------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


def cap_of(n: int) -> int:
    return (n + 3) // 4 * 3


def _want(t, skip, abc):
    """(record, bytes or None) of a text given as bytes or as a uint8 array."""
    if isinstance(t, np.ndarray):
        want = np_skip_ref(t, skip, abc)
        t = t.tobytes() if want[0] == OK else b""
    else:
        want = skip_ref(t, skip, abc)
    return want, (decode_kept(strip(t, skip), abc) if want[0] == OK else None)


def guarded(nbytes: int, zero: bool = False):
    """A device buffer of nbytes with GUARD bytes of FILL on either side:
    (the whole tensor, the inner view)."""
    whole = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    inner = whole[GUARD:GUARD + nbytes]
    if zero:
        inner.zero_()
    return whole, inner


def guards_intact(whole: torch.Tensor) -> bool:
    return bool((whole[:GUARD] == FILL).all() and (whole[-GUARD:] == FILL).all())


class Single:
    """One-buffer calls laid out in one input buffer, one output buffer with
    GUARD bytes of FILL around every output, one record array with a guard
    behind it and one guarded workspace for all of them (one stream); run()
    makes every call, then one copy back and the checks."""

    def __init__(self):
        self.calls = []
        self.in_size = 0
        self.out_size = GUARD

    def add(self, text, skip=CRLF, abc=STD, in_shift=0, out_shift=0, validate_only=False,
            want=None):
        text = bytes(text)
        ioff = -(-self.in_size // 16) * 16 + in_shift
        self.in_size = ioff + len(text)
        cap = cap_of(len(text))
        ooff = -(-self.out_size // 16) * 16 + out_shift
        self.out_size = ooff + cap + GUARD
        want, data = (want, None) if want is not None else _want(text, skip, abc)
        self.calls.append((ioff, text, ooff, cap, want, data, skip, abc, validate_only))

    def run(self):
        b64 = _b64()
        host = np.zeros(self.in_size + 64, np.uint8)
        for ioff, text, *_ in self.calls:
            host[ioff:ioff + len(text)] = np.frombuffer(text, np.uint8)
        x = torch.from_numpy(host).cuda()
        out = torch.full((self.out_size + 64,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * len(self.calls) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        longest = max(len(c[1]) for c in self.calls)
        ws_all, ws = guarded(b64.strict_skip_workspace_size(longest), zero=True)
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
        for i, (ioff, text, ooff, cap, want, data, skip, abc, vo) in enumerate(self.calls):
            b64.decode_strict_skip(x[ioff:ioff + len(text)], skip, out=out[ooff:ooff + cap],
                                   validate_only=vo, abc=abc, workspace=ws,
                                   result=res[REC * i:REC * (i + 1)])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        recs = records(res)
        assert (res[REC * len(self.calls):].cpu().numpy() == FILL).all()
        assert guards_intact(ws_all), "a guard byte of the workspace was overwritten"
        mask = np.ones(got.size, bool)
        for rec, (ioff, text, ooff, cap, want, data, skip, abc, vo) in zip(recs, self.calls):
            label = (len(text), text[:40], skip, abc, ioff % 16, ooff % 16, vo)
            assert rec == (want[0], want[1], want[2], 0), (label, rec, want)
            if want[0] == OK and not vo and data is not None:
                assert got[ooff:ooff + want[2]].tobytes() == data, label
            if not vo:
                mask[ooff:ooff + cap] = False
        assert (got[mask] == FILL).all(), "a guard byte was overwritten"


def run_batch(texts, skip=CRLF, abc=STD, validate_only=False, out_shift=0, wants=None):
    """One decode_strict_skip_batch call over `texts` (bytes or uint8 arrays),
    laid end to end; every output between guards, a guard behind the records
    and around the 8-bytes-per-buffer workspace."""
    b64 = _b64()
    nbuf = len(texts)
    lens = [len(t) for t in texts]
    in_off = np.zeros(nbuf + 1, np.int64)
    np.cumsum(lens, out=in_off[1:])
    host = np.zeros(int(in_off[-1]) + 64, np.uint8)
    for o, t in zip(in_off, texts):
        host[o:o + len(t)] = np.frombuffer(t, np.uint8) if isinstance(t, bytes) else t
    out_off = np.zeros(nbuf, np.int64)
    size = GUARD
    for i, n in enumerate(lens):
        out_off[i] = -(-size // 16) * 16 + (out_shift * (i % 16 + 1)) % 16
        size = int(out_off[i]) + cap_of(n) + GUARD
    if wants is None:
        wants = [_want(t, skip, abc) for t in texts]
    x = torch.from_numpy(host).cuda()
    d_in_off = torch.from_numpy(in_off).cuda()
    d_out_off = torch.from_numpy(out_off).cuda()
    out = torch.full((size + 64,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws_all, ws = guarded(8 * nbuf)
    if validate_only:
        b64.decode_strict_skip_batch(x, d_in_off, None, None, res[:REC * nbuf], skip, abc)
    else:
        b64.decode_strict_skip_batch(x, d_in_off, out, d_out_off, res[:REC * nbuf], skip, abc,
                                     workspace=ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    recs = records(res)[:nbuf]
    assert (res[REC * nbuf:].cpu().numpy() == FILL).all()
    assert guards_intact(ws_all)
    mask = np.ones(got.size, bool)
    for i, (rec, (want, data)) in enumerate(zip(recs, wants)):
        label = (i, lens[i], int(in_off[i]) % 16, int(out_off[i]) % 16, skip, abc)
        assert rec == (want[0], want[1], want[2], 0), (label, rec, want)
        o = int(out_off[i])
        if not validate_only:
            if want[0] == OK and data is not None:
                assert got[o:o + want[2]].tobytes() == data, label
            mask[o:o + cap_of(lens[i])] = False
    assert (got[mask] == FILL).all(), "a guard byte was overwritten"
    return recs


def edge_text():
    """A CRLF-76 text of two tiles + 17 bytes (a line feed at its end makes up
    the length), ending in one pad character: (text, payload)."""
    n = 5996
    assert n % 3 == 2
    t = crlf76(_data(n, 31))
    fill = 2 * TILE + 17 - len(t)
    assert 0 <= fill <= 8
    return t + b"\n" * fill, _data(n, 31)


def edge_positions(W: int):
    """Offsets within +-2 of every lane, wave and tile edge, and the first
    and last 80."""
    pos = set(range(80)) | set(range(W - 80, W))
    for k in range(0, W // LANE + 1):
        pos.update(k * LANE + d for d in range(-2, 3))
    return sorted(p for p in pos if 0 <= p < W)


# a junk byte, the pad character, a skipped byte, a character with low bits set
REPLACEMENTS = (0x00, 0x3D, 0x0A, 0x2F)


@gpu
def test_every_byte_is_judged_batch():
    """One buffer per (position, replacement), each followed by a buffer of 15
    skipped bytes so that every text starts at a 16-byte boundary and the
    edges are where edge_positions() puts them."""
    text, payload = edge_text()
    t = np.frombuffer(text, np.uint8)
    W = t.size
    plan = [(p, v) for p in edge_positions(W) for v in REPLACEMENTS]
    assert 3000 <= len(plan) <= 12000
    rows = np.tile(t, (len(plan), 1))
    for i, (p, v) in enumerate(plan):
        rows[i, p] = v
    filler = np.full(15, 0x0A, np.uint8)
    texts, wants = [], []
    kinds = set()
    for i in range(len(plan)):
        want = np_skip_ref(rows[i])
        kinds.add(want[0])
        data = decode_kept(strip(rows[i].tobytes())) if want[0] == OK else None
        texts += [rows[i], filler]
        wants += [(want, data), ((OK, 0, 0), b"")]
    assert kinds == {OK, CHAR, PAD, BITS, LENGTH}
    for (p, v), (want, _) in zip(plan, wants[::2]):
        if v == 0x00:  # the junk byte itself, or the text's pad that it leaves in the middle
            assert want == (CHAR, p, 0) or (want[0] == PAD and want[1] < p and p >= W - 4)
    texts.append(t)
    wants.append(((OK, 0, len(payload)), payload))
    run_batch(texts, wants=wants)


@gpu
def test_every_byte_is_judged_one_buffer():
    """The same mutations at about 60 positions, one call each on the device's
    copy of the text; the records in one array, one synchronisation."""
    b64 = _b64()
    text, payload = edge_text()
    t = np.frombuffer(text, np.uint8)
    W = t.size
    positions = sorted({e + d for e in (0, LANE, WAVE, TILE, TILE + WAVE, 2 * TILE, W)
                        for d in range(-4, 4) if 0 <= e + d < W} | {W - 5, W - 6, W - 7, W - 8})
    assert 40 <= len(positions) <= 70
    plan = [(p, v) for p in positions for v in REPLACEMENTS]
    x = torch.from_numpy(t.copy()).cuda()
    clean = x.clone()
    cap = cap_of(W)
    out_all, out = guarded(cap)
    res = torch.full((REC * (len(plan) + 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws_all, ws = guarded(b64.strict_skip_workspace_size(W), zero=True)
    want = []
    for c, (p, v) in enumerate(plan):
        x[p:p + 1].fill_(v)
        b64.decode_strict_skip(x, out=out, workspace=ws, result=res[REC * c:REC * c + REC])
        x[p:p + 1].copy_(clean[p:p + 1])
        u = t.copy()
        u[p] = v
        want.append(np_skip_ref(u))
    b64.decode_strict_skip(x, out=out, workspace=ws,
                           result=res[REC * len(plan):REC * len(plan) + REC])
    want.append((OK, 0, len(payload)))
    torch.cuda.synchronize()
    got = records(res)
    for c, w in enumerate(want):
        assert got[c] == (w[0], w[1], w[2], 0), (plan[c] if c < len(plan) else None, got[c], w)
    assert {w[0] for w in want} == {OK, CHAR, PAD, BITS, LENGTH}
    assert (res[REC * len(want):].cpu().numpy() == FILL).all()
    assert out.cpu().numpy()[:len(payload)].tobytes() == payload
    assert guards_intact(out_all) and guards_intact(ws_all)


@gpu
def test_lowest_offset_wins():
    """Two and three offences of different kinds in different lanes, waves,
    tiles and grid-stride rounds of a 9 MiB + 17 byte text (2,304 tiles for a
    grid of at most 2,048 blocks); the batch form on a buffer of 3 passes + 5
    bytes."""
    b64 = _b64()
    W = 9 * (1 << 20) + 17
    n = W // 78 * 57 - 58  # one pad character, a short last line
    t = np.frombuffer(crlf76(util.splitmix64(3, n).tobytes()), np.uint8)
    assert W - 200 < t.size <= W
    t = np.concatenate([t, np.full(W - t.size, 0x0A, np.uint8)])
    assert t.size == W and W // TILE + 1 > MAX_GRID
    assert np_skip_ref(t) == (OK, 0, n)
    ROUND = MAX_GRID * TILE

    def ch(p):  # the nearest character at or after p
        while int(t[p]) in CRLF:
            p += 1
        return p
    J, P = 0x00, 0x3D
    spots = [
        [(ch(5 * LANE + 2), J), (ch(5 * LANE + 13), P)],                 # one lane
        [(ch(5 * LANE + 3), P), (ch(5 * LANE + 12), J)],
        [(ch(TILE + 70), P), (ch(TILE + WAVE + 3), J)],                  # waves of one tile
        [(ch(TILE + 3 * WAVE), P), (ch(TILE + 2 * WAVE + 3), J)],
        [(ch(3 * TILE + 9), J), (ch(700 * TILE + 77), P)],               # tiles of one round
        [(ch(1999 * TILE + 77), P), (ch(3 * TILE + 9), J), (ch(12 * TILE), P)],
        [(ch(ROUND + 5 * TILE + 100), J), (ch(5 * TILE + 200), P)],      # block 5, both rounds
        [(ch(ROUND + 5 * TILE + 100), P), (ch(5 * TILE + 200), J), (ch(ROUND + 9), J)],
        [(ch(ROUND - 3), J), (ch(ROUND + 40), P)],                       # across the rounds' seam
        [(ch(W - 300), P), (ch(100), P)],
        [(ch(W - 600), J), (ch(W - 400), P)],
    ]
    x = torch.from_numpy(t.copy()).cuda()
    out_all, out = guarded(cap_of(W))
    res = torch.full((REC * (len(spots) + 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws_all, ws = guarded(b64.strict_skip_workspace_size(W), zero=True)
    want = []
    for c, sp in enumerate(spots):
        u = t.copy()
        for p, v in sp:
            u[p] = v
            x[p:p + 1].fill_(v)
        b64.decode_strict_skip(x, out=out, workspace=ws, validate_only=c % 2 == 1,
                               result=res[REC * c:REC * c + REC])
        for p, v in sp:
            x[p:p + 1].fill_(int(t[p]))
        want.append(np_skip_ref(u))
        assert want[-1][0] in (CHAR, PAD) and want[-1][1] == min(p for p, _ in sp), (sp, want[-1])
    b64.decode_strict_skip(x, out=out, workspace=ws, result=res[REC * len(spots):REC * len(spots) + REC])
    want.append((OK, 0, n))
    torch.cuda.synchronize()
    got = records(res)
    for c, w in enumerate(want):
        assert got[c] == (w[0], w[1], w[2], 0), (c, got[c], w)
    assert (res[REC * len(want):].cpu().numpy() == FILL).all()
    assert torch.equal(out[:n], torch.from_numpy(util.splitmix64(3, n)).cuda())
    assert guards_intact(out_all) and guards_intact(ws_all)
    # the batch form
    m = 3 * WAVE + 5
    b = np.frombuffer(crlf76(_data(2240, 8)), np.uint8)
    b = np.concatenate([np.full(m - b.size, 0x0A, np.uint8), b])  # the text ends the last pass
    assert b.size == m and np_skip_ref(b)[0] == OK
    texts = [b]
    for sp in ([(5 * LANE + 2, J), (5 * LANE + 13, P)], [(5 * LANE + 3, P), (5 * LANE + 12, J)],
               [(WAVE + 3, J), (70, P)], [(WAVE + 3, P), (2 * WAVE + 70, J), (3 * WAVE + 1, P)],
               [(3 * WAVE - 1, J), (3 * WAVE, P)], [(3 * WAVE + 1, P), (2 * WAVE - 1, J), (80, P)]):
        u = b.copy()
        for p, v in sp:
            assert int(u[p]) not in CRLF
            u[p] = v
        assert np_skip_ref(u)[1] == min(p for p, _ in sp)
        texts.append(u)
    run_batch(texts)


def _kept(E: int, seed: int):
    """E kept bytes that are valid with pad for E mod 4 == 0 (0, 1 or 2 pads
    by E), valid without pad for E mod 4 in {2, 3}, and one character too many
    for either otherwise."""
    if E % 4 == 0:
        return plain(_data(E // 4 * 3 - (E // 4) % 3 if E else 0, seed))
    if E % 4 == 1:
        return plain(_data(E // 4 * 3, seed), NOPAD) + b"A"
    return plain(_data(E // 4 * 3 + E % 4 - 1, seed), NOPAD)


def _place(u: bytes, n: int, how: str, rng):
    """A text of n bytes whose kept bytes are u, the skipped ones placed as
    `how` says; None if there is no such text."""
    extra = n - len(u)
    if extra < 0:
        return None
    if how == "none":
        return u if extra == 0 else None
    if how == "crlf76":
        lines = [u[i:i + 76] for i in range(0, len(u), 76)]
        body = CRLF.join(lines)
        rest = n - len(body)
        if rest < 0:
            return None
        return body + (CRLF * (rest // 2) + b"\n" * (rest % 2))
    assert how == "random"
    where = set(rng.sample(range(n), extra))
    it = iter(u)
    return bytes(0x0A if i in where else next(it) for i in range(n))


LENGTHS = list(range(0, 21)) + [1023, 1024, 1025, 4095, 4096, 4097]


def placement_texts():
    rng = random.Random(0x9A)
    texts = []
    for how in ("none", "crlf76", "random"):
        for n in LENGTHS:
            for r in (0, 2, 3, 1):
                # the largest E = r (mod 4) that leaves room for the skipped bytes
                lo = {"none": n, "crlf76": max(0, n - n // 38 - 8), "random": n * 20 // 21}[how]
                E = next((e for e in range(min(lo, n), -1, -1) if e % 4 == r), None)
                t = None if E is None else _place(_kept(E, n + r), n, how, rng)
                if t is not None:
                    assert len(t) == n
                    texts.append(t)
    # a run of 5,000 skipped bytes (longer than two steps of the backward walk)
    assert 5000 > 2 * STEP
    run = b"\n" * 5000
    for E in (4, 5, 6, 7, 8, 1024, 1026, 1027, 1029):
        u = _kept(E, E)
        texts += [run + u, u[:E // 2] + run + u[E // 2:], u + run,
                  u[:-1] + run + u[-1:], u[:-2] + run + u[-2:-1] + CRLF + u[-1:] + run]
    # between and after the pads
    texts += [b"QQ=\r\n=\n", b"QQ\r\n==", b"QQ=\n=", b"QUI\r\n=\r\n\r\n", b"QR=\r\n=\n", b"Q\nQ=\r\n=\n=",
              b"=\r\n", b"\r\n=", b"=\n=", b"QQ=\n=\nQ", b"QUJD\n=", b"QUJD=\n=\n=", b"QR\n", b"QUJ\r\n"]
    # skipped bytes only
    texts += [b"\n" * k for k in (1, 2, 15, 16, 17, 1023, 1024, 1025, 5000)]
    texts += [b"\r\n" * 40, b""]
    return texts


def test_placement_texts_cover_their_cases():
    texts = placement_texts()
    assert len(texts) > 200 and len(set(map(len, texts))) >= len(LENGTHS)
    for abc in (STD, NOPAD):
        kinds = {skip_ref(t, CRLF, abc)[0] for t in texts}
        assert kinds >= {OK, LENGTH, BITS, CHAR if abc == NOPAD else PAD}
    assert skip_ref(b"QQ=\r\n=\n") == (OK, 0, 1)


@gpu
def test_where_skipped_bytes_stand():
    texts = placement_texts()
    ar = Single()
    for abc in (STD, NOPAD):
        for t in texts:
            ar.add(t, CRLF, abc)
    ar.run()
    for abc in (STD, NOPAD):
        run_batch(texts, CRLF, abc)


@gpu
def test_alignment():
    text = crlf76(_data(3701, 4)) + b"\n"
    ar = Single()
    for o in range(16):
        ar.add(text, in_shift=o)
        ar.add(text, out_shift=o)
        ar.add(text[:100 + o], in_shift=o, out_shift=15 - o)
        ar.add(text, in_shift=o, validate_only=True)
    bad = bytearray(text)
    bad[17] = 0x2A
    for o in range(16):
        ar.add(bytes(bad), in_shift=o, out_shift=(3 * o + 1) % 16)
    ar.run()
    # a batch of aligned and unaligned buffers, empty ones among them, outputs at odd offsets
    rng = random.Random(5)
    texts = []
    for i in range(300):
        n = rng.choice((0, 0, rng.randrange(1, 40), rng.randrange(40, 3000), 16 * rng.randrange(1, 70)))
        t = bytearray(crlf76(_data(n, i)))
        if i % 7 == 3 and t:
            t[rng.randrange(len(t))] = rng.choice(b"*=\n A")
        texts.append(bytes(t))
    run_batch(texts, out_shift=3)
    run_batch(texts, out_shift=0)


@gpu
def test_alphabets_and_skip_sets():
    ar = Single()
    eight = b"\r\n\t \x0b\x0c\x00\xff"
    for abc in (URL, NOPAD, DOTPAD, ("-", "_", False, -1), STD):
        chars, pad, padc = alpha(abc)
        for skip in (b"\n", b" \t\r\n", eight, b""):
            for n in (0, 1, 2, 3, 1000, 1001, 5000):
                canon = plain(_data(n, n + 9), abc)
                rng = random.Random(n)
                sprinkled = bytearray(canon)
                for _ in range(len(canon) // 30 + 2 if skip else 0):
                    sprinkled.insert(rng.randrange(len(sprinkled) + 1), rng.choice(skip))
                ar.add(bytes(sprinkled), skip, abc)
                if not canon:
                    continue
                # mutations of the canonical text: a stranger, a pad, a byte that
                # is skipped under some sets and a stranger under the others
                for p in (0, len(canon) // 2, len(canon) - 1):
                    for v in (0x2A, padc, 0x0D, 0x20, chars[63]):
                        u = bytearray(sprinkled if skip else canon)
                        u[p] = v
                        ar.add(bytes(u), skip, abc)
    kinds = {c[4][0] for c in ar.calls}
    assert kinds == {OK, CHAR, PAD, BITS, LENGTH}
    ar.run()
    texts = [c[1] for c in ar.calls if c[6] == eight and c[7] == URL]
    run_batch(texts, eight, URL)
    texts = [c[1] for c in ar.calls if c[6] == b"" and c[7] == DOTPAD]
    run_batch(texts, b"", DOTPAD)


@gpu
def test_validate_only():
    """With d_out NULL the records are those of the decoding call, and nothing
    but the record and the workspace head changes: the guards sit right behind
    the head, and the buffer the bytes would have gone to keeps its poison."""
    b64 = _b64()
    texts = placement_texts()[::3] + [crlf76(_data(20000, 2)), crlf76(_data(20000, 2))[:-9] + b"*" * 9]
    # one-buffer
    ins = [torch.from_numpy(np.frombuffer(t or b"\0", np.uint8).copy()).cuda()[:len(t)] for t in texts]
    ws_all, ws = guarded(HEAD)
    stand_in = torch.full((cap_of(max(map(len, texts))) + 2 * GUARD,), FILL, dtype=torch.uint8,
                          device="cuda")
    res = torch.full((REC * len(texts) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    for i, x in enumerate(ins):
        d = b64.decode_strict_skip(x, validate_only=True, workspace=ws, out=stand_in[GUARD:GUARD],
                                   result=res[REC * i:REC * i + REC])
        assert d.out.numel() == 0
    torch.cuda.synchronize()
    got = records(res)[:len(texts)]
    for t, rec in zip(texts, got):
        want = skip_ref(t)
        assert rec == (want[0], want[1], want[2], 0), (t[:40], rec, want)
    assert guards_intact(ws_all)
    assert (stand_in == FILL).all() and (res[REC * len(texts):] == FILL).all()
    # batch: the validate-only records against the decoding call's
    dec = run_batch(texts)
    val = run_batch(texts, validate_only=True)
    assert dec == val == got


@gpu
def test_round_trip():
    b64 = _b64()
    N = 201
    payload = torch.from_numpy(util.splitmix64(21, N)).cuda()
    formats = [(76, b"\r\n"), (64, b"\n"), (60, b"\r\n\n")]
    outs = torch.full((len(formats) * N, 256), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC * len(formats) * N + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(b64.strict_skip_workspace_size(400), dtype=torch.uint8, device="cuda")
    for f, (L, sep) in enumerate(formats):
        for n in range(N):
            text = b64.encode_lines(payload[:n], L, sep)
            c = f * N + n
            b64.decode_strict_skip(text, out=outs[c], workspace=ws, result=res[REC * c:REC * c + REC])
    torch.cuda.synchronize()
    got = records(res)
    o = outs.cpu().numpy()
    p = payload.cpu().numpy()
    for f in range(len(formats)):
        for n in range(N):
            c = f * N + n
            assert got[c] == (OK, 0, n, 0), (formats[f], n, got[c])
            assert (o[c, :n] == p[:n]).all() and (o[c, 216:] == FILL).all()  # cap <= 213
    n = 3 * (1 << 20) + 1
    x = torch.from_numpy(util.splitmix64(22, n)).cuda()
    for L, sep in formats:
        text = b64.encode_lines(x, L, sep)
        d = b64.decode_strict_skip(text)
        r = d.info()
        assert (r.err, r.err_pos, r.out_len, r.reserved) == (OK, 0, n, 0)
        assert torch.equal(d.bytes(), x)
    text[n:n + 1].fill_(0x7E)
    with pytest.raises(b64.B64xFormatError) as e:
        b64.decode_strict_skip(text).bytes()
    assert (e.value.kind, e.value.pos) == (CHAR, n)


@gpu
def test_graph_capture():
    b64 = _b64()
    n = 100001
    data = util.splitmix64(11, n)
    text = np.frombuffer(crlf76(data.tobytes()), np.uint8)
    W = text.size
    cap = cap_of(W)
    x = torch.from_numpy(text.copy()).cuda()
    out_all, out = guarded(cap)
    res = torch.full((REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws_all, ws = guarded(b64.strict_skip_workspace_size(W), zero=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.decode_strict_skip(x, out=out, workspace=ws, result=res[:REC])  # warm-up
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b64.decode_strict_skip(x, out=out, workspace=ws, result=res[:REC])
    spoiled = text.copy()
    spoiled[W // 2] = 0x20
    want_bad = np_skip_ref(spoiled)
    assert want_bad == (CHAR, W // 2, 0)
    seen = []
    for t, want in ((text, (OK, 0, n)), (spoiled, want_bad), (text, (OK, 0, n))):
        x.copy_(torch.from_numpy(t.copy()).cuda())
        out.fill_(FILL)
        res.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        rec = records(res)[0]
        assert rec == (want[0], want[1], want[2], 0)
        seen.append(rec)
        if want[0] == OK:
            assert out.cpu().numpy()[:n].tobytes() == data.tobytes()
        assert guards_intact(out_all) and guards_intact(ws_all)
        assert (res[REC:].cpu().numpy() == FILL).all()
    assert seen[0] == seen[2] != seen[1]
    # a validate-only batch, replayed on other lengths written into the same offsets
    nbuf = 40
    arena = np.frombuffer(crlf76(_data(6000, 6)), np.uint8)
    xb = torch.from_numpy(arena.copy()).cuda()

    def offsets(seed):
        rng = random.Random(seed)
        cuts = sorted(rng.sample(range(arena.size), nbuf - 2))
        cuts.insert(5, cuts[5])  # an empty buffer
        return np.array([0] + cuts + [arena.size], np.int64)
    first = offsets(1)
    d_off = torch.from_numpy(first.copy()).cuda()
    resb = torch.full((REC * nbuf + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    graph_b = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.decode_strict_skip_batch(xb, d_off, None, None, resb[:REC * nbuf])
        side.synchronize()
        with torch.cuda.graph(graph_b, stream=side):
            b64.decode_strict_skip_batch(xb, d_off, None, None, resb[:REC * nbuf])
    for off in (first, offsets(2), offsets(3)):
        d_off.copy_(torch.from_numpy(off.copy()).cuda())
        resb.fill_(FILL)
        torch.cuda.synchronize()
        graph_b.replay()
        torch.cuda.synchronize()
        got = records(resb)
        for i in range(nbuf):
            w = np_skip_ref(arena[off[i]:off[i + 1]])
            assert got[i] == (w[0], w[1], w[2], 0), (i, got[i], w)
        assert (resb[REC * nbuf:].cpu().numpy() == FILL).all()


@gpu
def test_past_4gib_text():
    """A validate-only text of 2^32 + 4,096 + 5 bytes made on the device is
    accepted; one junk byte above offset 2^32 is found at its 64-bit offset."""
    b64 = _b64()
    W = (1 << 32) + 4096 + 5
    n = W // 78 * 57 - 57
    free, _ = torch.cuda.mem_get_info()
    if free < n + W + (1 << 30):
        pytest.skip("the device has no room for a text past 2^32 bytes")
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0xB17)
    text = torch.full((W,), 0x0A, dtype=torch.uint8, device="cuda")
    made = b64.encode_lines(x, out=text)
    assert W - 200 < made.numel() <= W
    del x
    ws_all, ws = guarded(HEAD)
    res = torch.full((2 * REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b64.decode_strict_skip(text, validate_only=True, workspace=ws, result=res[:REC])
    bad = (1 << 32) + 78 * 20 + 33
    text[bad:bad + 1].fill_(0x2A)
    text[W - 100:W - 99].fill_(0x2A)
    b64.decode_strict_skip(text, validate_only=True, workspace=ws, result=res[REC:2 * REC])
    torch.cuda.synchronize()
    got = records(res)
    assert got[0] == (OK, 0, n, 0)
    assert got[1] == (CHAR, bad, 0, 0)
    assert (res[2 * REC:].cpu().numpy() == FILL).all() and guards_intact(ws_all)
