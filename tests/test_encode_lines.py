"""Line-wrapped encode (b64x_encode_lines_dev / _strided, async_amd.b64
encode_lines / encode_lines_strided): bit-exact against a reference built
here from the stdlib (base64.b64encode, a translate for pos62/pos63/pad, a
strip of the pad characters, the cut-and-join).

CPU tests: the length formula, every -EINVAL case, -ENODEV without a device,
and the new code object's kernel list and barriers.  GPU tests lay their
cases out in one arena with 64 guard bytes of 0xA5 around every case's
output, copy the arena back once and check the bytes and the guards."""
import base64
import ctypes
import hashlib
import os
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

# The hot kernel's tiles (async_amd/csrc/b64x_wrap.hip): a lane writes one
# 16-byte block, a wave 1,024 bytes, a 256-lane block (kWrapTile) 4,096.
BLOCK, WAVE_BYTES, TILE = 16, 1024, 4096

CRLF76 = (76, b"\r\n")
LF64 = (64, b"\n")
FORMATS = [CRLF76, LF64, (4, b"\n"), (16, b"\n"), (60, b"\r\n\n"), (300, b"\r\n"),
           (5000, b"\r\n\r\n")]

_STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/="


def plain(data: bytes, abc=(-1, -1, True, -1)) -> bytes:
    """What b64x_encode_dev writes: abc = (pos62, pos63, pad, padchar)."""
    p62, p63, pad, padc = abc
    c = base64.b64encode(data)
    if not pad:
        c = c.rstrip(b"=")
    to = bytearray(_STD)
    for i, v in ((62, p62), (63, p63), (64, padc)):
        if v != -1:
            to[i] = v if isinstance(v, int) else v.encode("latin-1")[0]
    return c.translate(bytes.maketrans(_STD, bytes(to)))


def wrap(chars: bytes, L: int, sep: bytes, trailing: bool) -> bytes:
    lines = [chars[i:i + L] for i in range(0, len(chars), L)]
    return sep.join(lines) + (sep if trailing and lines else b"")


def ref(data: bytes, L, sep, trailing, abc=(-1, -1, True, -1)) -> bytes:
    return wrap(plain(data, abc), L, sep, trailing)


def enc_len(n: int, pad: bool) -> int:
    return (n + 2) // 3 * 4 if pad else (4 * n + 2) // 3


def formula(n: int, pad: bool, L: int, s: int, trailing: bool) -> int:
    E = enc_len(n, pad)
    return E + s * (-(-E // L) - (0 if trailing else 1)) if E else 0


def n_for_output(target: int, L: int, s: int) -> int:
    """The smallest n whose padded, trailing text has at least `target`
    bytes (the text grows by 4 or 4 + s per 3 input bytes, so the result is
    within a group of the target; the tests take a few n around it)."""
    lo, hi = 0, target
    while lo < hi:
        mid = (lo + hi) // 2
        if formula(mid, True, L, s, True) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


# ------------------------------------------------------------------- CPU --

def test_encoded_lines_len_formula():
    lib = _lib.load()
    for L in (4, 16, 64, 76, 300):
        for s in (1, 2, 3):
            sep = b"\r\n\n"[:s]
            for trailing in (False, True):
                f = _lib.lines(L, sep, trailing)
                for pad in (False, True):
                    for n in range(400):
                        want = len(wrap(b"x" * enc_len(n, pad), L, sep, trailing))
                        assert want == formula(n, pad, L, s, trailing)
                        got = lib.b64x_encoded_lines_len(n, pad, ctypes.byref(f))
                        assert got == want, (L, s, trailing, pad, n)
                    for n in ((1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1,
                              (1 << 32) + 2, 3 * (1 << 30) + 7):
                        assert lib.b64x_encoded_lines_len(n, pad, ctypes.byref(f)) == \
                            formula(n, pad, L, s, trailing), (L, s, trailing, pad, n)


def _raw(L, s, sep, flags):
    return _lib.Lines(L, s, (ctypes.c_uint8 * 4)(*sep), flags)


def test_invalid_arguments():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    ok = _lib.lines(76, b"\r\n", True)

    def dev(fmt, abc=a, n=30):
        return lib.b64x_encode_lines_dev(p, n, p, ctypes.byref(abc),
                                         ctypes.byref(fmt) if fmt is not None else None, None)

    def strided(fmt, in_stride=30, out_stride=64, abc=a):
        return lib.b64x_encode_lines_strided(
            p, in_stride, 30, 2, p, out_stride, ctypes.byref(abc),
            ctypes.byref(fmt) if fmt is not None else None, None)

    # n == 0 first, then NULL buffers, then the format
    assert lib.b64x_encode_lines_dev(None, 0, None, ctypes.byref(a), None, None) == 0
    assert lib.b64x_encode_lines_dev(None, 5, p, ctypes.byref(a), ctypes.byref(ok), None) == -22
    assert lib.b64x_encode_lines_dev(p, 5, None, ctypes.byref(a), ctypes.byref(ok), None) == -22
    assert lib.b64x_encode_lines_strided(None, 30, 30, 2, p, 64, ctypes.byref(a),
                                         ctypes.byref(ok), None) == -22
    assert lib.b64x_encode_lines_strided(p, 30, 30, 0, p, 64, ctypes.byref(a), None, None) == 0
    bad = [None,
           _raw(0, 2, b"\r\n", 1), _raw(6, 2, b"\r\n", 1), _raw(75, 2, b"\r\n", 1),
           _raw(2, 1, b"\n", 1),
           _raw(76, 0, b"", 1), _raw(76, 5, b"\r\n\r\n", 1),
           _raw(76, 2, b"\r\n", 2), _raw(76, 2, b"\r\n", 0x80000001),
           _raw(76, 1, b"A", 1), _raw(76, 2, b"\nz", 1), _raw(76, 3, b"\r\n7", 1),
           _raw(76, 1, b"+", 1), _raw(76, 2, b"\n/", 0)]
    for f in bad:
        assert dev(f) == -22, f and (f.line_len, f.sep_len, bytes(f.sep), f.flags)
        assert strided(f) == -22
    # the effective pos62/pos63 are alphabet characters, '+' and '/' then are not
    url = _lib.alphabet("-", "_")
    assert dev(_raw(76, 1, b"-", 1), url) == -22
    assert dev(_raw(76, 2, b"\n_", 1), url) == -22
    if lib.b64x_device_check() == -19:  # valid calls stop at the device check
        assert dev(_raw(76, 1, b"+", 1), url) == -19
        # a separator byte beyond sep_len is not looked at
        assert dev(_raw(76, 1, b"\nA", 1)) == -19
    # strided: strides below the row's lengths (30 bytes -> 40 + 2 wrapped)
    assert strided(ok, in_stride=29) == -22
    assert strided(ok, out_stride=41) == -22
    if lib.b64x_device_check() == -19:
        assert strided(ok, out_stride=42) == -19
    # the Python layer refuses what it can see
    from async_amd import b64
    with pytest.raises(ValueError):
        b64.encoded_lines_len(10, 75)
    with pytest.raises(ValueError):
        b64.encoded_lines_len(10, 76, b"")
    with pytest.raises(ValueError):
        b64.encoded_lines_len(10, 76, b"\r\n\r\n\r")


def test_no_gpu_is_enodev():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    assert lib.b64x_device_check() == -19
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    a = _lib.alphabet()
    f = _lib.lines(76, b"\r\n", True)
    assert lib.b64x_encode_lines_dev(p, 30, p, ctypes.byref(a), ctypes.byref(f), None) == -19
    assert lib.b64x_encode_lines_strided(p, 30, 30, 2, p, 64, ctypes.byref(a),
                                         ctypes.byref(f), None) == -19


# The kernels of b64x_wrap.hip; nothing else may be in its code object.
WRAP_KERNELS = {
    "k_encode_lines<false, false>", "k_encode_lines<false, true>",
    "k_encode_lines<true, false>", "k_encode_lines_any",
}


def test_wrap_code_object_kernels_and_barriers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import isa_check
    dis = isa_check.disassemble(os.path.join(ROOT, "build", "b64x_wrap.o"))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(isa_check.kernel_symbols(dis))),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    got = set()
    for n in names:
        if not n:
            continue
        m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?([\w]+(?:<[^>]*>)?)\(", n)
        got.add(m.group(1) if m else n)
    assert got == WRAP_KERNELS, (got - WRAP_KERNELS, WRAP_KERNELS - got)
    assert isa_check.barrier_report(dis) == []


# ------------------------------------------------------------------- GPU --

gpu = pytest.mark.gpu


def _b64():
    from async_amd import b64
    return b64


class Arena:
    """Cases laid out in one input and one output buffer, GUARD bytes of
    FILL around every output; run() per case, then check() once."""

    def __init__(self):
        self.cases = []   # (in_off, n, out_off, want, label)
        self.in_parts = []
        self.in_size = 0
        self.out_size = GUARD

    def add(self, data: bytes, want: bytes, label, in_align=16, in_shift=0, out_align=16,
            out_shift=0, span=None):
        """span: output bytes the case owns (strided: gaps included)."""
        ioff = -(-self.in_size // in_align) * in_align + in_shift
        self.in_parts.append((ioff, data))
        self.in_size = ioff + len(data)
        ooff = -(-self.out_size // out_align) * out_align + out_shift
        span = len(want) if span is None else span
        self.cases.append((ioff, len(data), ooff, want, label, span))
        self.out_size = ooff + span + GUARD
        return len(self.cases) - 1

    def build(self):
        host = np.zeros(self.in_size + 64, np.uint8)
        for off, d in self.in_parts:
            host[off:off + len(d)] = np.frombuffer(d, np.uint8)
        self.x = torch.from_numpy(host).cuda()
        self.out = torch.full((self.out_size + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert self.x.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def views(self, i):
        ioff, n, ooff, want, _, span = self.cases[i]
        return self.x[ioff:ioff + n], self.out[ooff:ooff + max(span, 1)]

    def check(self):
        got = self.out.cpu().numpy()
        mask = np.ones(got.size, bool)
        for ioff, n, ooff, want, label, span in self.cases:
            w = np.frombuffer(want, np.uint8)
            seg = got[ooff:ooff + span]
            assert seg.size == w.size and np.array_equal(seg, w), \
                (label, int(np.flatnonzero(seg != w)[0]) if seg.size == w.size else seg.size)
            mask[ooff:ooff + span] = False
        assert (got[mask] == FILL).all(), "a guard byte was overwritten"


def _data(n: int, seed: int = 1) -> bytes:
    return util.splitmix64(seed, n).tobytes()


def _run_single(cases):
    """cases: (n, L, sep, trailing, abc, in_shift, out_shift, label)."""
    b64 = _b64()
    ar = Arena()
    idx = []
    for n, L, sep, trailing, abc, ishift, oshift in cases:
        d = _data(n, n + L)
        idx.append(ar.add(d, ref(d, L, sep, trailing, abc),
                          (n, L, sep, trailing, abc, ishift, oshift),
                          in_shift=ishift, out_shift=oshift))
    ar.build()
    for i, (n, L, sep, trailing, abc, _, _) in zip(idx, cases):
        x, out = ar.views(i)
        got = b64.encode_lines(x, L, sep, trailing, out=out,
                               abc=(abc[0], abc[1], abc[2], abc[3]))
        assert got.numel() == len(ar.cases[i][3])
    torch.cuda.synchronize()
    ar.check()


STD = (-1, -1, True, -1)
NOPAD = (-1, -1, False, -1)


@gpu
def test_small_sweep():
    cases = []
    for L, sep in FORMATS:
        per = 3 * L // 4
        if L <= 76:
            ns = range(0, 3 * per + 5)
        else:
            ns = sorted({max(0, k * per + d) for k in range(4) for d in range(-2, 3)})
        for n in ns:
            for trailing in (False, True):
                for abc in (STD, NOPAD):
                    cases.append((n, L, sep, trailing, abc, 0, 0))
    _run_single(cases)


def tiling_cases():
    """(76, CRLF) and (64, LF) texts whose length is k * unit - 1, + 0 and
    + 1 for the kernel's units (BLOCK, WAVE_BYTES, TILE) and 65,536, over
    both pad and both trailing values (a padded text's length is even for
    CRLF, so the odd lengths come from the unpadded ones), plus 1 MiB + 5.
    The few lengths no n gives are replaced by the nearest on either side."""
    cases = []
    for L, sep in (CRLF76, LF64):
        s = len(sep)
        for unit in (BLOCK, WAVE_BYTES, TILE, 65536):
            for k in (1, 2, 3):
                for target in (k * unit - 1, k * unit, k * unit + 1):
                    n0 = n_for_output(target, L, s)
                    near = [(formula(n, abc[2], L, s, trailing), (n, L, sep, trailing, abc, 0, 0))
                            for n in range(max(n0 - 9, 0), n0 + 10)
                            for trailing in (True, False) for abc in (STD, NOPAD)]
                    hits = [c for m, c in near if m == target]
                    if not hits:
                        # a length the format cannot produce (a line end falls
                        # there): the nearest ones on either side instead
                        below = max(m for m, _ in near if m < target)
                        above = min(m for m, _ in near if m > target)
                        assert target - below <= 2 and above - target <= 2
                        hits = [c for m, c in near if m in (below, above)]
                    cases += hits
        cases.append(((1 << 20) + 5, L, sep, True, STD, 0, 0))
        cases.append(((1 << 20) + 5, L, sep, False, NOPAD, 0, 0))
    return cases


def test_tiling_cases_reach_every_edge():
    assert len(tiling_cases()) >= 2 * (4 * 3 * 3 + 2)


@gpu
def test_tiling_edges():
    _run_single(tiling_cases())


@gpu
def test_alignment():
    n = 10007
    cases = []
    for L, sep in (CRLF76, LF64):
        for o in range(16):
            cases.append((n, L, sep, True, STD, 0, o))
            cases.append((n, L, sep, True, STD, o, 0))
        cases.append((n, L, sep, True, STD, 3, 5))
        cases.append((n, L, sep, False, STD, 1, 15))
    _run_single(cases)


@gpu
def test_alphabets():
    cases = []
    for abc in (STD, ("-", "_", True, -1), (-1, -1, True, "."), (0xE9, 0xE8, True, -1), NOPAD):
        for n in (1000, 1001):
            cases.append((n, 76, b"\r\n", True, abc, 0, 0))
            cases.append((n, 76, b"\r\n", False, abc, 0, 0))
    _run_single(cases)


@gpu
@pytest.mark.parametrize("L,sep", [CRLF76, LF64, (60, b"\r\n\n")])
def test_round_trip(L, sep):
    b64 = _b64()
    n = 1000003
    host = util.splitmix64(L, n)
    x = torch.from_numpy(host).cuda()
    text = b64.encode_lines(x, L, sep)
    assert text.numel() == formula(n, True, L, len(sep), True)
    d = b64.decode(text)
    assert d.info().out_len == n
    assert torch.equal(d.bytes(), x)


@gpu
def test_strided():
    b64 = _b64()
    ar = Arena()
    runs = []
    for L, sep in (CRLF76, LF64):
        for nbuf in (2, 65, 257):
            for length in (1, 56, 57, 58, 767, 768, 769, 1024):
                for slack in (False, True):
                    W = formula(length, True, L, len(sep), True)
                    istr = length + (5 if slack else 0)
                    ostr = W + (11 if slack else 0)
                    d = bytearray(_data(istr * (nbuf - 1) + length, nbuf * 4099 + length))
                    want = bytearray([FILL]) * (ostr * (nbuf - 1) + W)
                    for b in range(nbuf):
                        row = bytes(d[b * istr:b * istr + length])
                        want[b * ostr:b * ostr + W] = ref(row, L, sep, True)
                    i = ar.add(bytes(d), bytes(want), (L, sep, nbuf, length, slack))
                    runs.append((i, istr, length, nbuf, ostr, L, sep))
    ar.build()
    for i, istr, length, nbuf, ostr, L, sep in runs:
        x, out = ar.views(i)
        b64.encode_lines_strided(x, istr, length, nbuf, out, ostr, L, sep, True)
    torch.cuda.synchronize()
    ar.check()


@gpu
@pytest.mark.slow
def test_cfg4_crlf76_digest():
    """Config 4 (1,048,576 x 1 KiB) written as RFC 2045 rows of 1,404 bytes
    in one call: the whole text and its decode against the digests of
    tests/golden/batch_digests.json."""
    b64 = _b64()
    g = util.golden("batch_digests.json")["cfg4"]
    nbuf, L = g["nbuf"], g["len"]
    D = g["crlf76"]["row_bytes"]
    assert D == b64.encoded_lines_len(L) == 1404
    x = torch.empty(nbuf * L, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    text = torch.full((nbuf * D + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    b64.encode_lines_strided(x, L, L, nbuf, text, D)
    host = text.cpu().numpy()
    assert (host[nbuf * D:] == FILL).all()
    assert hashlib.sha256(host[:nbuf * D]).hexdigest() == g["crlf76"]["text_sha256"]
    del host
    cap = 12 * ((D + 15) // 16)
    dec = torch.empty(nbuf * cap, dtype=torch.uint8, device="cuda")
    outlen = torch.zeros(nbuf, dtype=torch.int64, device="cuda")
    b64.decode_strided(text[:nbuf * D], D, D, nbuf, dec, cap, outlen)
    assert int(outlen.min()) == L and int(outlen.max()) == L
    got = dec.view(nbuf, cap)[:, :L].contiguous().cpu().numpy()
    assert hashlib.sha256(got).hexdigest() == g["crlf76"]["dec_sha256"]


@gpu
def test_past_4gib_output():
    """n = 3 GiB + 7: the text passes 2^32 bytes.  1 MiB windows of it (the
    start, across 2^31 and 2^32, the end with the tail and the trailing
    separator) against the encoding of the input slices that hold those
    whole lines."""
    b64 = _b64()
    n = 3 * (1 << 30) + 7
    L, sep, P, per = 76, b"\r\n", 78, 57
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0xB16)
    W = formula(n, True, L, 2, True)
    assert W > 1 << 32
    text = torch.full((W + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    got = b64.encode_lines(x, out=text)
    assert got.numel() == W
    torch.cuda.synchronize()
    assert (text[W:].cpu().numpy() == FILL).all()
    MiB = 1 << 20
    for start in (0, (1 << 31) - MiB // 2, (1 << 32) - MiB // 2, W - MiB):
        k0 = start // P                      # first line that the window touches
        k1 = min(-(-(start + MiB) // P), -(-n // per))  # one past the last
        data = x[k0 * per:min(k1 * per, n)].cpu().numpy().tobytes()
        want = ref(data, L, sep, True)       # lines k0 .. k1 - 1, whole
        lo = start - k0 * P
        win = text[start:start + MiB].cpu().numpy().tobytes()
        assert win == want[lo:lo + MiB], start


@gpu
def test_graph_capture():
    b64 = _b64()
    n = 100001
    a = util.splitmix64(11, n)
    b = util.splitmix64(12, n)
    x = torch.from_numpy(a).cuda()
    W = formula(n, True, 76, 2, True)
    out = torch.full((W + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b64.encode_lines(x, out=out)  # warm-up outside the capture
        side.synchronize()
        out.fill_(FILL)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b64.encode_lines(x, out=out)
    for data in (a, b):
        x.copy_(torch.from_numpy(data).cuda())
        out.fill_(FILL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got[:W].tobytes() == ref(data.tobytes(), 76, b"\r\n", True)
        assert (got[W:] == FILL).all()
