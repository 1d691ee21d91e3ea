"""Strict decode (b64x_decode_strict_dev / _strided, async_amd.b64
decode_strict / decode_strict_strided): the record and the bytes, bit for
bit, against the scalar procedure of include/b64x.h written here in plain
Python (strict_ref), a vectorised copy of it for the large cases (np_ref,
checked against the scalar one on the CPU) and the stdlib.

CPU tests: the reference against "re-encoding the stdlib's decode gives the
text back", the capacity formula, every -EINVAL case, -ENODEV without a
device, and the new code object's kernel list and barriers.  GPU tests lay
their cases out in one arena with 64 guard bytes of 0xA5 around every output
and behind the records, copy back once and check outputs, records and guards.
"""
import base64
import binascii
import ctypes
import functools
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

ROOT = util.ROOT
GUARD = 64
FILL = 0xA5
REC = 24

# The hot kernel's units (async_amd/csrc/b64x_strict.hip): a lane owns 16
# characters of text (12 bytes out), a wave 1,024, a 256-lane block
# (kTileChars) 4,096.
LANE, WAVE, TILE = 16, 1024, 4096

OK, CHAR, SEP, PAD, BITS, LENGTH = range(6)

CRLF76 = (76, b"\r\n")
LF64 = (64, b"\n")
PLAIN = (None, b"")
FORMATS = [CRLF76, LF64, (4, b"\n"), (16, b"\n"), (60, b"\r\n\n"), (300, b"\r\n"),
           (5000, b"\r\n\r\n")]

_STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/="
STD = (-1, -1, True, -1)
NOPAD = (-1, -1, False, -1)


# ------------------------------------------------------------ references --

def _byte(v, default):
    if v == -1:
        return default
    return v if isinstance(v, int) else v.encode("latin-1")[0]


def alpha(abc):
    """(the 64 characters, pad flag, pad character) of abc = (pos62, pos63, pad, padchar)."""
    p62, p63, pad, padc = abc
    return _STD[:62] + bytes([_byte(p62, 0x2B), _byte(p63, 0x2F)]), bool(pad), _byte(padc, 0x3D)


def plain(data: bytes, abc=STD) -> bytes:
    """What b64x_encode_dev writes, from the stdlib."""
    chars, pad, padc = alpha(abc)
    c = base64.b64encode(data)
    if not pad:
        c = c.rstrip(b"=")
    return c.translate(bytes.maketrans(_STD, chars + bytes([padc])))


def wrap(chars: bytes, L, sep: bytes, trailing: bool) -> bytes:
    if L is None:
        return chars
    lines = [chars[i:i + L] for i in range(0, len(chars), L)]
    return sep.join(lines) + (sep if trailing and lines else b"")


def ref_text(data: bytes, L=None, sep=b"", trailing=True, abc=STD) -> bytes:
    """The encoder's text for `data` (b64x_encode_dev / b64x_encode_lines_dev)."""
    return wrap(plain(data, abc), L, sep, trailing)


def enc_len(n: int, pad: bool) -> int:
    return (n + 2) // 3 * 4 if pad else (4 * n + 2) // 3


def formula(n: int, pad: bool, L, s: int, trailing: bool) -> int:
    E = enc_len(n, pad)
    if L is None:
        return E
    return E + s * (-(-E // L) - (0 if trailing else 1)) if E else 0


def text_chars(nchars: int, L, s: int, trailing: bool):
    """Step 1 without the pad rules: (E or None, the characters of the whole
    lines when there is no E)."""
    if L is None or nchars == 0:
        return nchars, nchars
    P = L + s
    k, r = divmod(nchars if trailing else nchars + s, P)
    if 0 < r <= s:
        return None, k * L
    E = k * L + (r - s if r else 0)
    if (E + s * (-(-E // L) - (0 if trailing else 1)) if E else 0) != nchars:
        return None, E
    return E, E


def strict_cap(nchars: int, L, s: int, trailing: bool) -> int:
    return 3 * -(-text_chars(nchars, L, s, trailing)[1] // 4)


def strict_ref(t: bytes, L=None, sep=b"", trailing=True, abc=STD):
    """The scalar procedure of the contract: (kind, pos, out_len)."""
    chars, pad, padc = alpha(abc)
    s = len(sep)
    n = len(t)
    # 1. length
    E, _ = text_chars(n, L, s, trailing)
    if E is None or (pad and E % 4) or (not pad and E % 4 == 1):
        return LENGTH, n, 0
    # 2. positions
    P = (L or 0) + s

    def off(e):
        return e if L is None else e // L * P + e % L
    # 3. pads
    npad = 0
    if pad and E and t[off(E - 1)] == padc:
        npad = 2 if t[off(E - 2)] == padc else 1
    D = E - npad
    # 4. offences, in offset order
    for e in range(E):
        p = off(e)
        if e < D:
            if pad and t[p] == padc:
                return PAD, p, 0
            v = chars.find(bytes([t[p]]))
            if v < 0:
                return CHAR, p, 0
            if e == D - 1 and D % 4 in (2, 3) and v & (15 if D % 4 == 2 else 3):
                return BITS, p, 0
        if L is not None and ((e + 1) % L == 0 or e == E - 1) and (e != E - 1 or trailing):
            for j in range(s):
                if t[p + 1 + j] != sep[j]:
                    return SEP, p + 1 + j, 0
    # 5. no offence
    return OK, 0, 3 * (D // 4) + (0, 0, 1, 2)[D % 4]


@functools.lru_cache(maxsize=64)
def _layout(E, L, s, trailing):
    e = np.arange(E, dtype=np.int64)
    if L is None:
        return e, np.zeros(0, np.int64), np.zeros(0, np.int64)
    off = e // L * (L + s) + e % L
    ends = np.flatnonzero((e + 1) % L == 0)
    ends = ends[ends != E - 1]
    if trailing and E:
        ends = np.append(ends, E - 1)
    pos = (off[ends][:, None] + 1 + np.arange(s)[None, :]).ravel()
    return off, pos, np.tile(np.arange(s), ends.size)


@functools.lru_cache(maxsize=16)
def _table(abc):
    chars, pad, padc = alpha(abc)
    tab = np.full(256, 0x80, np.uint8)
    tab[list(chars)] = np.arange(64)
    if pad:
        tab[padc] = 0xC0
    return tab, pad, padc


def np_ref(t: np.ndarray, L=None, sep=b"", trailing=True, abc=STD):
    """strict_ref, vectorised: (kind, pos, out_len) for a uint8 array."""
    tab, pad, padc = _table(abc)
    s = len(sep)
    n = int(t.size)
    E, _ = text_chars(n, L, s, trailing)
    if E is None or (pad and E % 4) or (not pad and E % 4 == 1):
        return LENGTH, n, 0
    if E == 0:
        return OK, 0, 0
    off, spos, sidx = _layout(E, L, s, trailing)
    npad = 0
    if pad and t[off[E - 1]] == padc:
        npad = 2 if t[off[E - 2]] == padc else 1
    D = E - npad
    cls = tab[t[off[:D]]]
    cand = []
    bad = np.flatnonzero(cls & 0x80)
    if bad.size:
        cand.append((int(off[bad[0]]), PAD if cls[bad[0]] & 0x40 else CHAR))
    if D % 4 in (2, 3) and cls[D - 1] < 64 and cls[D - 1] & (15 if D % 4 == 2 else 3):
        cand.append((int(off[D - 1]), BITS))
    if spos.size:
        wrong = np.flatnonzero(t[spos] != np.frombuffer(sep, np.uint8)[sidx])
        if wrong.size:
            cand.append((int(spos[wrong].min()), SEP))
    if cand:
        pos, kind = min(cand)
        return kind, pos, 0
    return OK, 0, 3 * (D // 4) + (0, 0, 1, 2)[D % 4]


def stdlib_decode(t: bytes, abc=STD):
    """The stdlib's lenient decode of the text's alphabet characters, or None."""
    chars, pad, padc = alpha(abc)
    body = bytes(c for c in t if c in chars).translate(bytes.maketrans(chars, _STD[:64]))
    if len(body) % 4 == 1:
        return None
    try:
        return base64.b64decode(body + b"=" * (-len(body) % 4), validate=True)
    except binascii.Error:
        return None


def is_encoder_output(t: bytes, L, sep, trailing, abc) -> bool:
    d = stdlib_decode(t, abc)
    return d is not None and ref_text(d, L, sep, trailing, abc) == t


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


# ------------------------------------------------------------------- CPU --

SELF_FORMATS = [(None, b"", True), (76, b"\r\n", True), (76, b"\r\n", False), (64, b"\n", True),
                (4, b"\n", True), (16, b"\r\n\n", True)]


def corruptions(count, seed=0xB64):
    """Seeded random corruptions of encoder text: substitutions, deletions
    and insertions, over SELF_FORMATS and both pad modes."""
    rng = random.Random(seed)
    pool = b"AQz9+/=-_ \r\n\x00\xff"
    for i in range(count):
        L, sep, trailing = SELF_FORMATS[i % len(SELF_FORMATS)]
        abc = STD if rng.random() < 0.5 else NOPAD
        n = rng.choice((rng.randrange(0, 12), rng.randrange(0, 200), rng.randrange(0, 200)))
        t = bytearray(ref_text(bytes(rng.randrange(256) for _ in range(n)), L, sep, trailing, abc))
        op = rng.randrange(6)
        for _ in range(rng.randrange(1, 3) if op else 0):
            near_end = rng.random() < 0.4
            if op in (1, 2, 3) and t:
                p = len(t) - 1 - rng.randrange(min(len(t), 6)) if near_end else rng.randrange(len(t))
                t[p] = rng.choice(pool) if op < 3 else rng.randrange(256)
            elif op == 4 and t:
                del t[len(t) - 1 - rng.randrange(min(len(t), 6)) if near_end
                      else rng.randrange(len(t))]
            elif op == 5:
                t.insert(len(t) - rng.randrange(min(len(t), 6) + 1) if near_end
                         else rng.randrange(len(t) + 1), rng.choice(pool))
        yield bytes(t), L, sep, trailing, abc


def test_reference_self_check():
    kinds = set()
    accepted = 0
    for t, L, sep, trailing, abc in corruptions(5000):
        kind, pos, out_len = got = strict_ref(t, L, sep, trailing, abc)
        assert got == np_ref(np.frombuffer(t, np.uint8), L, sep, trailing, abc), (t, L, sep)
        assert (kind == OK) == is_encoder_output(t, L, sep, trailing, abc), (t, L, sep, trailing, abc)
        if kind == OK:
            assert out_len == len(stdlib_decode(t, abc))
            accepted += 1
        elif kind == LENGTH:
            assert pos == len(t)
        else:
            assert 0 <= pos < len(t)
        kinds.add(kind)
    assert kinds == {OK, CHAR, SEP, PAD, BITS, LENGTH}
    assert accepted >= 500


def test_strict_decoded_cap():
    lib = _lib.load()
    assert lib.b64x_strict_decoded_cap(0, None) == 0
    for L, sep in [PLAIN] + FORMATS[:5]:
        for trailing in (False, True):
            f = None if L is None else _lib.lines(L, sep, trailing)
            ref = None if f is None else ctypes.byref(f)
            ns = list(range(400)) + [(1 << 32) + d for d in range(-3, 4)] + [3 * (1 << 30) + 7]
            for n in ns:
                got = lib.b64x_strict_decoded_cap(n, ref)
                assert got == strict_cap(n, L, len(sep), trailing), (L, sep, trailing, n)
                assert got <= lib.b64x_decoded_cap(n)
                # every text of that length fits: the encoder's inverse
                E, _ = text_chars(n, L, len(sep), trailing)
                if E is not None:
                    assert got == 3 * -(-E // 4)


def _raw(L, s, sep, flags):
    return _lib.Lines(L, s, (ctypes.c_uint8 * 4)(*sep), flags)


def test_invalid_arguments():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    a = _lib.alphabet()
    ok = _lib.lines(76, b"\r\n", True)
    nodev = lib.b64x_device_check() == -19

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def dev(fmt, abc=a, n=40, d_in=p, d_out=p, d_res=p):
        return lib.b64x_decode_strict_dev(d_in, n, d_out, d_res, ref(abc), ref(fmt), None)

    def strided(fmt, in_stride=44, out_stride=32, abc=a, length=42, d_in=p, d_out=p, d_res=p,
                nbuf=2):
        return lib.b64x_decode_strict_strided(d_in, in_stride, length, nbuf, d_out, out_stride,
                                              d_res, ref(abc), ref(fmt), None)

    # NULL buffers or record, an empty text included
    for n in (0, 40):
        assert dev(ok, n=n, d_in=None) == -22
        assert dev(ok, n=n, d_out=None) == -22
        assert dev(None, n=n, d_res=None) == -22
    assert strided(ok, d_in=None) == -22
    assert strided(ok, d_out=None) == -22
    assert strided(None, d_res=None) == -22
    # the formats b64x_encode_lines_dev refuses (tests/test_encode_lines.py); NULL is plain here
    bad = [_raw(0, 2, b"\r\n", 1), _raw(6, 2, b"\r\n", 1), _raw(75, 2, b"\r\n", 1),
           _raw(2, 1, b"\n", 1),
           _raw(76, 0, b"", 1), _raw(76, 5, b"\r\n\r\n", 1),
           _raw(76, 2, b"\r\n", 2), _raw(76, 2, b"\r\n", 0x80000001),
           _raw(76, 1, b"A", 1), _raw(76, 2, b"\nz", 1), _raw(76, 3, b"\r\n7", 1),
           _raw(76, 1, b"+", 1), _raw(76, 2, b"\n/", 0)]
    for f in bad:
        what = (f.line_len, f.sep_len, bytes(f.sep), f.flags)
        assert dev(f) == -22, what
        assert strided(f) == -22, what
        # the encoder agrees (the two units repeat the check)
        assert lib.b64x_encode_lines_dev(p, 30, p, ref(a), ref(f), None) == -22, what
    url = _lib.alphabet("-", "_")
    assert dev(_raw(76, 1, b"-", 1), url) == -22
    assert dev(_raw(76, 2, b"\n_", 1), url) == -22
    # alphabets no decoder can tell apart
    for abc in (_lib.alphabet("-", "-"), _lib.alphabet("+", "+"), _lib.alphabet("A", "/"),
                _lib.alphabet("+", "z"), _lib.alphabet("5", "_"),
                _lib.alphabet(padchar="A"), _lib.alphabet(padchar="+"), _lib.alphabet(padchar="/"),
                _lib.alphabet("-", "_", True, "_"), _lib.alphabet("-", "_", True, "0")):
        assert dev(ok, abc) == -22, (abc.pos62, abc.pos63, abc.padchar)
        assert dev(None, abc) == -22
        assert strided(ok, abc=abc) == -22
    # strided: strides below the row's lengths (42 bytes of text hold 40 characters: 30 bytes)
    assert strided(ok, in_stride=41) == -22
    assert strided(ok, out_stride=29) == -22
    assert strided(None, length=40, in_stride=39) == -22
    assert strided(None, length=40, out_stride=29) == -22
    # valid calls stop at the device check
    if nodev:
        assert dev(_raw(76, 1, b"+", 1), url) == -19
        assert dev(_raw(76, 1, b"\nA", 1)) == -19  # a byte beyond sep_len is not looked at
        assert dev(ok, _lib.alphabet(pad=False, padchar="A")) == -19  # no pad: padchar unused
        assert dev(ok, _lib.alphabet("-", "_", True, "+")) == -19
        assert strided(ok, out_stride=30, in_stride=42) == -19
        assert strided(None, length=40, in_stride=40, out_stride=30) == -19
    # the Python layer refuses what it can see
    from async_amd import b64
    with pytest.raises(ValueError):
        b64.strict_decoded_cap(10, 76, b"")
    with pytest.raises(ValueError):
        b64.strict_decoded_cap(10, 76, b"\r\n\r\n\r")
    e = b64.B64xFormatError(BITS, 77)
    assert isinstance(e, ValueError) and (e.kind, e.pos) == (BITS, 77)


def test_no_gpu_is_enodev():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    assert lib.b64x_device_check() == -19
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    f = _lib.lines(76, b"\r\n", True)
    for fmt in (None, ctypes.byref(f)):
        for n in (0, 40, 41):  # an empty text writes its record too
            assert lib.b64x_decode_strict_dev(p, n, p, p, ctypes.byref(a), fmt, None) == -19
        assert lib.b64x_decode_strict_strided(p, 44, 42, 2, p, 36, p, ctypes.byref(a), fmt,
                                              None) == -19


# The kernels of b64x_strict.hip; nothing else may be in its code object.
STRICT_KERNELS = {
    "k_decode_strict<false, false>", "k_decode_strict<false, true>",
    "k_decode_strict<true, false>", "k_decode_strict<true, true>",
    "k_decode_strict_any", "k_strict_record",
}


def test_strict_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_strict.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == STRICT_KERNELS, (got - STRICT_KERNELS, STRICT_KERNELS - got)
    assert isa_check.barrier_report(dis) == []
    assert isa_check.barrier_count(dis) == 5  # one per decode kernel, after the table


# ------------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


def records(t: torch.Tensor):
    """[(err, err_pos, out_len, reserved)] of a records tensor copied back."""
    a = t.cpu().numpy()
    n = a.size // REC
    r = a[:n * REC].reshape(n, REC)
    u64 = r[:, :16].copy().view(np.uint64)
    u32 = r[:, 16:].copy().view(np.uint32)
    return [(int(u32[i, 0]), int(u64[i, 1]), int(u64[i, 0]), int(u32[i, 1])) for i in range(n)]


class Arena:
    """One-buffer calls laid out in one input buffer, one output buffer with
    GUARD bytes of FILL around every output, and one record array with a
    guard behind it; run() makes every call, then one copy back and check()."""

    def __init__(self):
        self.calls = []
        self.in_size = 0
        self.out_size = GUARD

    def add(self, text: bytes, want, data=None, L=None, sep=b"", trailing=True, abc=STD,
            in_shift=0, out_shift=0):
        """want: (kind, pos, out_len); data: the bytes an accepted text decodes to."""
        ioff = -(-self.in_size // 16) * 16 + in_shift
        self.in_size = ioff + len(text)
        cap = strict_cap(len(text), L, len(sep), trailing)
        ooff = -(-self.out_size // 16) * 16 + out_shift
        self.out_size = ooff + cap + GUARD
        if want[0] == OK:
            assert data is not None and len(data) == want[2] <= cap
        self.calls.append((ioff, text, ooff, cap, want, data, L, sep, trailing, abc))

    def run(self):
        b64 = _b64()
        host = np.zeros(self.in_size + 64, np.uint8)
        for ioff, text, *_ in self.calls:
            host[ioff:ioff + len(text)] = np.frombuffer(text, np.uint8)
        x = torch.from_numpy(host).cuda()
        out = torch.full((self.out_size + 64,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * len(self.calls) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and res.data_ptr() % 8 == 0
        for i, (ioff, text, ooff, cap, want, data, L, sep, trailing, abc) in enumerate(self.calls):
            d = b64.decode_strict(x[ioff:ioff + len(text)], L, sep, trailing,
                                  out=out[ooff:ooff + cap], abc=abc,
                                  result=res[REC * i:REC * (i + 1)])
            assert d.out.numel() == cap
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        recs = records(res)
        assert (res[REC * len(self.calls):].cpu().numpy() == FILL).all()
        mask = np.ones(got.size, bool)
        for rec, (ioff, text, ooff, cap, want, data, L, sep, trailing, abc) in zip(recs, self.calls):
            label = (len(text), L, sep, trailing, abc, ioff % 16, ooff % 16)
            assert rec == (want[0], want[1], want[2], 0), (label, rec, want)
            if want[0] == OK:
                assert got[ooff:ooff + want[2]].tobytes() == data, label
            mask[ooff:ooff + cap] = False
        assert (got[mask] == FILL).all(), "a guard byte was overwritten"


def add_valid(ar, n, L=None, sep=b"", trailing=True, abc=STD, **kw):
    d = _data(n, n + (L or 0))
    ar.add(ref_text(d, L, sep, trailing, abc), (OK, 0, n), d, L, sep, trailing, abc, **kw)


def valid_sweep_arena():
    ar = Arena()
    for L, sep in [PLAIN] + FORMATS:
        per = 3 * (L or 76) // 4
        if (L or 76) <= 76:
            ns = range(0, 3 * per + 5)
        else:
            ns = sorted({max(0, k * per + d) for k in range(4) for d in range(-2, 3)})
        for n in ns:
            for trailing in ((True,) if L is None else (False, True)):
                for abc in (STD, NOPAD):
                    add_valid(ar, n, L, sep, trailing, abc)
    return ar


@gpu
def test_valid_sweep():
    valid_sweep_arena().run()


def n_for_text(target: int, L, s: int) -> int:
    """The smallest n whose padded, trailing text has at least `target` bytes."""
    lo, hi = 0, target
    while lo < hi:
        mid = (lo + hi) // 2
        if formula(mid, True, L, s, True) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


def tiling_cases():
    """Texts of k * unit - 1, + 0 and + 1 bytes for the kernel's units and
    65,536, over both pad and both trailing values (the few lengths no text
    has are replaced by the nearest on either side), plus 1 MiB + 5 bytes of
    payload: (n, L, sep, trailing, abc)."""
    cases = []
    for L, sep in (CRLF76, LF64, PLAIN):
        s = len(sep)
        for unit in (LANE, WAVE, TILE, 65536):
            for k in (1, 2, 3):
                for target in (k * unit - 1, k * unit, k * unit + 1):
                    n0 = n_for_text(target, L, s)
                    near = [(formula(n, abc[2], L, s, trailing), (n, L, sep, trailing, abc))
                            for n in range(max(n0 - 9, 0), n0 + 10)
                            for trailing in ((True,) if L is None else (True, False))
                            for abc in (STD, NOPAD)]
                    hits = [c for m, c in near if m == target]
                    if not hits:
                        below = max(m for m, _ in near if m < target)
                        above = min(m for m, _ in near if m > target)
                        assert target - below <= 2 and above - target <= 2
                        hits = [c for m, c in near if m in (below, above)]
                    cases += hits
        cases.append(((1 << 20) + 5, L, sep, True, STD))
        cases.append(((1 << 20) + 5, L, sep, L is None, NOPAD))
    return cases


def test_tiling_cases_reach_every_edge():
    assert len(tiling_cases()) >= 3 * (4 * 3 * 3 + 2)


def tiling_arena():
    ar = Arena()
    for n, L, sep, trailing, abc in tiling_cases():
        add_valid(ar, n, L, sep, trailing, abc)
    return ar


@gpu
def test_tiling_edges():
    tiling_arena().run()


def alignment_arena():
    n = 10007
    ar = Arena()
    for L, sep in (PLAIN, CRLF76):
        for o in range(16):
            add_valid(ar, n, L, sep, out_shift=o)
            add_valid(ar, n, L, sep, in_shift=o)
        add_valid(ar, n, L, sep, in_shift=3, out_shift=5)
        add_valid(ar, n, L, sep, in_shift=4, out_shift=12)
        add_valid(ar, n, L, sep, L is None, NOPAD, in_shift=1, out_shift=15)
    return ar


@gpu
def test_alignment():
    alignment_arena().run()


def alphabets_arena():
    ar = Arena()
    for abc in (("-", "_", True, -1), (-1, -1, True, "."), (0xE9, 0xE8, True, -1), NOPAD,
                ("-", "_", False, -1)):
        for L, sep in (PLAIN, CRLF76):
            for n in (1000, 1001, 5000):
                add_valid(ar, n, L, sep, True, abc)
                # the standard '+' planted: not a character of these alphabets
                # (two of them keep '+': there the standard pad '=' is the stranger)
                t = bytearray(ref_text(_data(n, n + (L or 0)), L, sep, True, abc))
                stranger = 0x3D if abc[0] == -1 else 0x2B
                for p in (0, len(t) // 2 // 78 * 78 + 5, len(t) - 9):
                    u = bytearray(t)
                    u[p] = stranger
                    want = strict_ref(bytes(u), L, sep, True, abc)
                    assert want == (CHAR, p, 0)
                    ar.add(bytes(u), want, None, L, sep, True, abc)
    return ar


@gpu
def test_alphabets():
    alphabets_arena().run()


def _edge_text(L, sep, extra):
    """A valid padded, trailing text a little over one tile, with a short
    last line, ending in one pad character: (text, payload)."""
    s = len(sep)
    n = n_for_text(TILE + extra, L, s)
    while n % 3 != 2 or (L is not None and enc_len(n, True) % L == 0):
        n += 1
    d = _data(n, 77 + (L or 0))
    return ref_text(d, L, sep), d


def _is_sep_position(i, L, s, E):
    if L is None:
        return False
    return i % (L + s) >= L or i >= E // L * (L + s) + E % L


def _every_byte_rows(text, L, sep, value):
    """Row i = text with byte i replaced by `value` (a separator position
    always by 0x20): (rows as one array, expected records)."""
    t = np.frombuffer(text, np.uint8)
    W = t.size
    E = text_chars(W, L, len(sep), True)[0]
    rows = np.tile(t, (W, 1))
    for i in range(W):
        rows[i, i] = 0x20 if _is_sep_position(i, L, len(sep), E) else value
    return rows, [np_ref(rows[i], L, sep) for i in range(W)]


def _closed_form(text, L, sep, value, i):
    """The record of `text` with byte i replaced, for a text that ends in
    exactly one pad character, without running the procedure."""
    W = len(text)
    E = text_chars(W, L, len(sep), True)[0]
    chars, pad, padc = alpha(STD)
    if _is_sep_position(i, L, len(sep), E):
        return SEP, i, 0
    last = W - len(sep) - 1          # the pad character's offset
    if value == padc:
        if i < last - 1:
            return PAD, i, 0
        if i == last:                 # the text itself
            return OK, 0, (E - 4) // 4 * 3 + 2
        # xxx= became xx==: the character before now ends the data
        low = chars.find(text[last - 2:last - 1]) & 15
        return (BITS, last - 2, 0) if low else (OK, 0, (E - 4) // 4 * 3 + 1)
    v = chars.find(bytes([value]))
    if v < 0:
        return CHAR, i, 0
    if i == last:                     # xxx= became xxxA: a whole group
        return OK, 0, E // 4 * 3
    if i == last - 1 and v & 3:       # the last data character of xxx=
        return BITS, i, 0
    return OK, 0, (E - 4) // 4 * 3 + 2


def test_every_byte_expectations_agree():
    """On a 200-byte text: the closed form, the scalar procedure and its
    vectorised copy give the same record for every replaced byte."""
    for L, sep in (CRLF76, LF64, PLAIN):
        n = 140
        while n % 3 != 2:
            n += 1
        text = ref_text(_data(n, 5), L, sep)
        assert 180 <= len(text) <= 200 and text.rstrip(sep)[-2:-1] != b"="
        for value in (0x00, 0x41, 0x42, 0x3D):
            rows, want = _every_byte_rows(text, L, sep, value)
            kinds = set()
            for i in range(len(text)):
                assert want[i] == strict_ref(rows[i].tobytes(), L, sep), (L, value, i)
                v = 0x20 if _is_sep_position(i, L, len(sep), text_chars(len(text), L, len(sep),
                                                                        True)[0]) else value
                assert want[i] == _closed_form(text, L, sep, v, i), (L, value, i)
                kinds.add(want[i][0])
                if value == 0x00:
                    assert want[i][1] == i and want[i][0] in (CHAR, SEP)
            if value == 0x3D:
                assert PAD in kinds
            if value == 0x42:
                assert BITS in kinds


def _run_strided(batches):
    """batches: (rows array [nbuf, W], in_stride, out_stride, L, sep, trailing,
    abc, want records, payloads or None).  One input arena, one guarded
    output arena, one record array; one call per batch, one copy back."""
    b64 = _b64()
    ins, outs, recs = [], [], []
    in_size, out_size, nrec = 0, GUARD, 0
    for rows, istr, ostr, L, sep, trailing, abc, want, data in batches:
        nbuf, W = rows.shape
        cap = strict_cap(W, L, len(sep), trailing)
        ioff = -(-in_size // 16) * 16
        in_size = ioff + (nbuf - 1) * istr + W
        ooff = -(-out_size // 16) * 16
        out_size = ooff + (nbuf - 1) * ostr + cap + GUARD
        ins.append(ioff)
        outs.append((ooff, cap))
        recs.append(nrec)
        nrec += nbuf
    host = np.zeros(in_size + 64, np.uint8)
    for ioff, (rows, istr, *_) in zip(ins, batches):
        nbuf, W = rows.shape
        for b in range(nbuf):
            host[ioff + b * istr:ioff + b * istr + W] = rows[b]
    x = torch.from_numpy(host).cuda()
    out = torch.full((out_size + 64,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC * nrec + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    for ioff, (ooff, cap), r0, (rows, istr, ostr, L, sep, trailing, abc, want, data) in zip(
            ins, outs, recs, batches):
        nbuf, W = rows.shape
        b64.decode_strict_strided(x[ioff:ioff + (nbuf - 1) * istr + W], istr, W, nbuf,
                                  out[ooff:ooff + (nbuf - 1) * ostr + cap], ostr,
                                  res[REC * r0:REC * (r0 + nbuf)], L, sep, trailing, abc=abc)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    got_recs = records(res)
    assert (res[REC * nrec:].cpu().numpy() == FILL).all()
    mask = np.ones(got.size, bool)
    for (ooff, cap), r0, (rows, istr, ostr, L, sep, trailing, abc, want, data) in zip(
            outs, recs, batches):
        nbuf, W = rows.shape
        for b in range(nbuf):
            label = (L, sep, nbuf, W, istr, ostr, b)
            assert got_recs[r0 + b] == (want[b][0], want[b][1], want[b][2], 0), \
                (label, got_recs[r0 + b], want[b])
            o = ooff + b * ostr
            if want[b][0] == OK and data is not None:
                assert got[o:o + want[b][2]].tobytes() == data[b], label
            mask[o:o + cap] = False
    assert (got[mask] == FILL).all(), "a guard byte was overwritten"


@gpu
@pytest.mark.parametrize("L,sep", [CRLF76, LF64, PLAIN])
def test_every_byte_is_checked_strided(L, sep):
    """W rows in one call, row i being the text with byte i replaced: the
    record of row i names byte i.  An odd in_stride (the bytewise kernel) and
    a dword-aligned one (the hot kernel)."""
    text, payload = _edge_text(L, sep, 300 if L is not None else TILE * 3 // 10)
    W = len(text)
    cap = strict_cap(W, L, len(sep), True)
    batches = []
    for value in (0x00, 0x41, 0x42, 0x3D):
        rows, want = _every_byte_rows(text, L, sep, value)
        for i in range(W):
            v = 0x20 if _is_sep_position(i, L, len(sep), text_chars(W, L, len(sep), True)[0]) \
                else value
            assert want[i] == _closed_form(text, L, sep, v, i)
        if value == 0x00:
            assert all(w[1] == i and w[0] in (CHAR, SEP) for i, w in enumerate(want))
        # an accepted row differs from the text in its last group only
        for istr in (W + 11, -(-(W + 11) // 4) * 4):
            batches.append((rows, istr, -(-cap // 4) * 4 + 8, L, sep, True, STD, want, None))
    _run_strided(batches)


def _chosen_offsets(W, L, s):
    """The first and last byte of each lane, wave and tile boundary, each
    byte of the first, a middle and the last separator, the last four
    characters: offsets in the text."""
    P = (L + s) if L is not None else None
    E = text_chars(W, L, s, True)[0]

    def off(e):
        return e if L is None else e // L * P + e % L
    chosen = set()
    for unit in (LANE, WAVE, TILE):
        for k in range(0, E // unit + 1):
            if unit == LANE and not (k < 6 or k % 5 == 0 or k >= E // unit - 3):
                continue
            for e in (k * unit - 1, k * unit):
                if 0 <= e < E:
                    chosen.add(off(e))
    if L is not None:
        lines = -(-E // L)
        for k in (0, lines // 2, lines - 1):
            end = off(min((k + 1) * L, E) - 1) + 1
            chosen.update(range(end, end + s))
    chosen.update(off(e) for e in range(E - 4, E))
    return sorted(chosen)


@gpu
def test_every_byte_is_checked_one_buffer():
    """~200 chosen offsets per text, corrupted one call at a time on the
    device; the records in one array, one synchronisation at the end."""
    b64 = _b64()
    for L, sep in (CRLF76, LF64, PLAIN):
        s = len(sep)
        text, payload = _edge_text(L, sep, 300 if L is not None else TILE * 3 // 10)
        t = np.frombuffer(text, np.uint8)
        W = t.size
        E = text_chars(W, L, s, True)[0]
        cap = strict_cap(W, L, s, True)
        offsets = _chosen_offsets(W, L, s)
        assert 120 <= len(offsets) <= 320
        plan = [(i, 0x20 if _is_sep_position(i, L, s, E) else 0x00) for i in offsets]
        plan += [(i, 0x41) for i in offsets[-2:]] + [(i, 0x3D) for i in offsets[:3]]
        x = torch.from_numpy(t.copy()).cuda()
        clean = x.clone()
        out = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((REC * (len(plan) + 1) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        want = []
        for c, (i, v) in enumerate(plan):
            x[i:i + 1].fill_(v)
            b64.decode_strict(x, L, sep, out=out[GUARD:GUARD + cap], result=res[REC * c:REC * c + REC])
            x[i:i + 1].copy_(clean[i:i + 1])
            u = t.copy()
            u[i] = v
            want.append(np_ref(u, L, sep))
            assert want[-1] == _closed_form(text, L, sep, v, i)
        b64.decode_strict(x, L, sep, out=out[GUARD:GUARD + cap],
                          result=res[REC * len(plan):REC * len(plan) + REC])
        want.append((OK, 0, len(payload)))
        torch.cuda.synchronize()
        got = records(res)
        for c, w in enumerate(want):
            assert got[c] == (w[0], w[1], w[2], 0), (L, plan[c] if c < len(plan) else None, got[c], w)
        assert (res[REC * len(want):].cpu().numpy() == FILL).all()
        o = out.cpu().numpy()
        assert o[GUARD:GUARD + len(payload)].tobytes() == payload
        assert (o[:GUARD] == FILL).all() and (o[GUARD + cap:] == FILL).all()


def lowest_arena():
    ar = Arena()
    for L, sep in (CRLF76, PLAIN):
        s = len(sep)
        n = n_for_text(3 * TILE + 500, L, s)
        text = ref_text(_data(n, 3), L, sep)
        W = len(text)
        E = text_chars(W, L, s, True)[0]
        P = (L + s) if L is not None else None

        def off(e):
            return e if L is None else e // L * P + e % L
        spots = [
            [(off(TILE + 9), 0x00), (off(2 * TILE + 77), 0x3D)],          # different tiles
            [(off(2 * TILE + 77), 0x3D), (off(TILE + 9), 0x00)],
            [(off(TILE + 70), 0x3D), (off(TILE + WAVE + 3), 0x00)],       # waves of one tile
            [(off(TILE + 2 * WAVE + 3), 0x20), (off(TILE + 3 * WAVE), 0x3D)],
            [(off(5 * LANE + 2), 0x00), (off(5 * LANE + 13), 0x3D)],      # one lane
            [(off(5 * LANE + 3), 0x3D), (off(5 * LANE + 12), 0x00)],
            [(off(100), 0x00), (off(E - 2), 0x00)],                       # hot part + tail
            [(off(E - 2), 0x00), (off(E - 30), 0x3D)],
            [(off(E - 3), 0x00), (W - 1, 0x00)],
        ]
        if L is not None:
            line_end = off(L - 1) + 1
            spots += [[(line_end, 0x20), (line_end + 1, 0x20)],            # one separator
                      [(line_end + s, 0x00), (line_end + 1, 0x0D)],        # separator, then a character
                      [(line_end - 1, 0x3D), (line_end, 0x00)]]
        for sp in spots:
            u = np.frombuffer(text, np.uint8).copy()
            for p, v in sp:
                u[p] = v
            want = np_ref(u, L, sep)
            assert want[1] == min(p for p, _ in sp) and want[0] != OK, (sp, want)
            ar.add(u.tobytes(), want, None, L, sep)
        # 64 offences spread over a 1 MiB text
        big = np.frombuffer(ref_text(_data(3 << 18, 9), L, sep), np.uint8).copy()
        rng = random.Random(64 + (L or 0))
        where = sorted(rng.sample(range(5000, big.size), 64))
        for q, p in enumerate(where):
            big[p] = (0x00, 0x3D, 0x20, 0x80)[q % 4]
        want = np_ref(big, L, sep)
        assert want[1] == where[0]
        ar.add(big.tobytes(), want, None, L, sep)
    return ar


@gpu
def test_lowest_offset_wins():
    lowest_arena().run()


def structure_arena():
    ar = Arena()

    def case(text, want, L=None, sep=b"", trailing=True, abc=STD):
        assert strict_ref(text, L, sep, trailing, abc) == want, (text, want)
        data = stdlib_decode(text, abc) if want[0] == OK else None
        ar.add(text, want, data, L, sep, trailing, abc)

    # plain
    case(b"QQ==", (OK, 0, 1))
    case(b"QR==", (BITS, 1, 0))
    case(b"QUI=", (OK, 0, 2))
    case(b"QUJ=", (BITS, 2, 0))
    case(b"QUJD", (OK, 0, 3))
    case(b"QUJDQQ", (LENGTH, 6, 0))                      # missing pad
    case(b"QUJDQQ=", (LENGTH, 7, 0))
    case(b"QUJDQQ", (OK, 0, 4), abc=NOPAD)
    case(b"QUJDQ", (LENGTH, 5, 0), abc=NOPAD)            # unpadded E mod 4 = 1
    case(b"QUJDQR", (BITS, 5, 0), abc=NOPAD)
    case(b"QUJDQQ==", (CHAR, 6, 0), abc=NOPAD)           # without pad, '=' is a stranger
    case(b"QUJDQQ======", (PAD, 6, 0))                   # excess pad
    case(b"QUJD====", (PAD, 4, 0))
    case(b"====", (PAD, 0, 0))
    case(b"x=y=", (PAD, 1, 0))
    case(b"QU=DQUJD", (PAD, 2, 0))                       # a pad in the middle
    case(b"QUJDQ=Q=", (PAD, 5, 0))
    case(b"QUJD\n", (LENGTH, 5, 0))
    case(b"QUJ\n", (CHAR, 3, 0))
    # 76/CRLF
    L, sep = CRLF76
    d = _data(57 * 3 + 20, 12)
    good = ref_text(d, L, sep)
    assert len(good) == 3 * 78 + 28 + 2 and good.endswith(b"=\r\n")
    case(good, (OK, 0, len(d)), L, sep)
    case(good[:-2], (OK, 0, len(d)), L, sep, False)
    case(good[:-2], (LENGTH, len(good) - 2, 0), L, sep)             # missing trailing separator
    case(good, (LENGTH, len(good), 0), L, sep, False)               # an extra one
    case(good[:-1], (LENGTH, len(good) - 1, 0), L, sep)             # cut inside a separator
    case(good[:-1], (LENGTH, len(good) - 1, 0), L, sep, False)
    case(good + b"\r\n", (LENGTH, len(good) + 2, 0), L, sep)
    case(good[:-3] + b"\r\n", (LENGTH, len(good) - 1, 0), L, sep)   # missing pad
    case(good[:-2] + b"====\r\n", (PAD, 3 * 78 + 27, 0), L, sep)    # excess pad: xxx=====
    case(good[:-4] + b"=Q\r\n", (PAD, 3 * 78 + 26, 0), L, sep)
    mid = bytearray(good)
    mid[78 + 30] = 0x3D
    case(bytes(mid), (PAD, 78 + 30, 0), L, sep)                     # a pad in the middle
    lf = good.replace(b"\r\n", b"\n\n", 1)
    case(lf, (SEP, 76, 0), L, sep)                                  # LF where CR is due
    lf = good[:76] + b"\n" + good[78:]
    case(lf, (LENGTH, len(good) - 1, 0), L, sep)                    # LF where CRLF is due: no text has this length
    short = good[:72] + good[76:]                                   # a 72-character line
    case(short, (CHAR, 72, 0), L, sep)                              # the CR stands at a character position
    short4 = good[:72] + b"\r\n" + good[72:76] + good[78:]          # ... the text as long as before
    case(short4, (CHAR, 72, 0), L, sep)
    q = ref_text(b"A", L, sep)
    assert q == b"QQ==\r\n"
    case(q, (OK, 0, 1), L, sep)
    case(b"QR==\r\n", (BITS, 1, 0), L, sep)
    case(b"QQ==\n\n", (SEP, 4, 0), L, sep)
    case(b"QQ==\r\r", (SEP, 5, 0), L, sep)
    unp = ref_text(d + b"x", L, sep, True, NOPAD)
    case(unp, (OK, 0, len(d) + 1), L, sep, True, NOPAD)
    case(unp[:-5] + b"\r\n", (LENGTH, len(unp) - 3, 0), L, sep, True, NOPAD)  # E mod 4 = 1
    return ar


@gpu
def test_structure():
    structure_arena().run()


def strided_shape_batches():
    batches = []
    for L, sep in (CRLF76, PLAIN):
        for nbuf in (2, 65, 257):
            for length in (1, 56, 57, 58, 767, 768, 769, 1024):
                for slack in (0, 1, 2):
                    W = formula(length, True, L, len(sep), True)
                    cap = strict_cap(W, L, len(sep), True)
                    # no slack; odd slack; dword-aligned pitches with slack
                    istr = (W, W + 5, -(-W // 4) * 4 + 4)[slack]
                    ostr = (cap, cap + 11, -(-cap // 4) * 4 + 8)[slack]
                    rows = np.empty((nbuf, W), np.uint8)
                    data = []
                    for b in range(nbuf):
                        d = _data(length, nbuf * 4099 + length * 7 + b)
                        data.append(d)
                        rows[b] = np.frombuffer(ref_text(d, L, sep), np.uint8)
                    want = [(OK, 0, length)] * nbuf
                    rng = random.Random(nbuf * 131 + length)
                    for b in {0, 1, nbuf // 2, nbuf - 1} if length > 1 else {1}:
                        if rng.random() < 0.7:
                            rows[b, rng.randrange(W)] = rng.choice((0x00, 0x3D, 0x20, 0x0A))
                            want[b] = np_ref(rows[b], L, sep)
                            if want[b][0] == OK:
                                data[b] = stdlib_decode(rows[b].tobytes())
                    batches.append((rows, istr, ostr, L, sep, True, STD, want, data))
    return batches


@gpu
def test_strided_shapes():
    _run_strided(strided_shape_batches())


def test_gpu_case_tables_build():
    """The GPU tests' case tables and the expectations they assert while
    being built hold on the CPU."""
    assert len(valid_sweep_arena().calls) > 2000
    assert len(tiling_arena().calls) >= 114
    assert len(alignment_arena().calls) == 2 * 35
    assert len(alphabets_arena().calls) == 5 * 2 * 3 * 4
    kinds = {c[4][0] for c in lowest_arena().calls}
    assert kinds >= {CHAR, PAD, SEP}
    kinds = {c[4][0] for c in structure_arena().calls}
    assert kinds == {OK, CHAR, SEP, PAD, BITS, LENGTH}
    b = strided_shape_batches()
    assert len(b) == 2 * 3 * 8 * 3 and any(w[0] != OK for x in b for w in x[7])
    for L, sep in (CRLF76, LF64, PLAIN):
        text, _ = _edge_text(L, sep, 300 if L is not None else TILE * 3 // 10)
        assert 120 <= len(_chosen_offsets(len(text), L, len(sep))) <= 320


@gpu
@pytest.mark.parametrize("L,sep", [CRLF76, LF64, (60, b"\r\n\n"), PLAIN])
def test_round_trip(L, sep):
    b64 = _b64()
    n = 1000003
    x = torch.from_numpy(util.splitmix64(L or 1, n)).cuda()
    text = b64.encode(x) if L is None else b64.encode_lines(x, L, sep)
    assert text.numel() == formula(n, True, L, len(sep), True)
    d = b64.decode_strict(text, L, sep)
    r = d.info()
    assert (r.err, r.err_pos, r.out_len, r.reserved) == (OK, 0, n, 0)
    assert torch.equal(d.bytes(), x)
    lenient = b64.decode(text)
    assert lenient.info().out_len == n and torch.equal(lenient.bytes(), x)
    # refused: the exception carries the kind and the offset
    text[n // 2:n // 2 + 1].fill_(0x7E if L is None or (n // 2) % (L + len(sep)) < L else 0x20)
    with pytest.raises(b64.B64xFormatError) as e:
        b64.decode_strict(text, L, sep).bytes()
    assert e.value.pos == n // 2 and e.value.kind in (CHAR, SEP)


@gpu
def test_past_4gib_text():
    """The 76/CRLF text of 3 GiB + 7 bytes passes 2^32 bytes: the whole
    output against the input (1 MiB windows at the start, across 2^31, at the
    output of text offset 2^32 and at the end, then all of it), and one bad
    byte beyond offset 2^32 found at its 64-bit offset."""
    b64 = _b64()
    n = 3 * (1 << 30) + 7
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0xB16)
    W = formula(n, True, 76, 2, True)
    assert W > 1 << 32
    text = b64.encode_lines(x)
    assert text.numel() == W
    cap = b64.strict_decoded_cap(W, 76)
    assert cap == strict_cap(W, 76, 2, True) == n + 2
    out = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((2 * REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b64.decode_strict(text, 76, out=out[GUARD:GUARD + cap], result=res[:REC])
    MiB = 1 << 20
    at_4g = (1 << 32) // 78 * 57
    for start in (0, (1 << 31) - MiB // 2, at_4g - MiB // 2, n - MiB):
        assert torch.equal(out[GUARD + start:GUARD + start + MiB], x[start:start + MiB]), start
    assert torch.equal(out[GUARD:GUARD + n], x)
    assert (out[:GUARD].cpu().numpy() == FILL).all()
    assert (out[GUARD + cap:].cpu().numpy() == FILL).all()
    bad = (1 << 32) + 78 * 1000 + 33
    text[bad:bad + 1].fill_(0x2A)
    text[W - 100:W - 99].fill_(0x2A)
    b64.decode_strict(text, 76, out=out[GUARD:GUARD + cap], result=res[REC:2 * REC])
    torch.cuda.synchronize()
    got = records(res)
    assert got[0] == (OK, 0, n, 0)
    assert got[1] == (CHAR, bad, 0, 0)
    assert (res[2 * REC:].cpu().numpy() == FILL).all()
    assert (out[:GUARD].cpu().numpy() == FILL).all()
    assert (out[GUARD + cap:].cpu().numpy() == FILL).all()


@gpu
def test_graph_capture():
    b64 = _b64()
    n = 100001
    data = util.splitmix64(11, n)
    text = np.frombuffer(ref_text(data.tobytes(), 76, b"\r\n"), np.uint8)
    W = text.size
    cap = strict_cap(W, 76, 2, True)
    x = torch.from_numpy(text.copy()).cuda()
    out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((REC + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.decode_strict(x, 76, out=out[:cap], result=res[:REC])  # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b64.decode_strict(x, 76, out=out[:cap], result=res[:REC])
    spoiled = text.copy()
    spoiled[W // 2] = 0x20
    want_bad = np_ref(spoiled, 76, b"\r\n")
    assert want_bad[0] in (CHAR, SEP) and want_bad[1] == W // 2
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
        got = out.cpu().numpy()
        if want[0] == OK:
            assert got[:n].tobytes() == data.tobytes()
        assert (got[cap:] == FILL).all()
        assert (res[REC:].cpu().numpy() == FILL).all()
    assert seen[0] == seen[2] != seen[1]
