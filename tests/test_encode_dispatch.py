"""The uniform-batch and single-buffer encoders at every branch of their
launcher (encode_choice in b64x_kernels.hip): k_encode_tight2 next to the
guard of its 32-bit multiply-high division, every reason for falling back to
k_encode_strided, and k_encode past one pass of its capped grid.

Every GPU case first asks the hooks library (b64x__test_encode_path) which
kernel the call's own addresses and shape select, and asserts that it is the
one the case is about; the call itself runs from the product library.  The
output lives in an arena filled with a sentinel that is in no tested alphabet
and is no pad character; the expectation is built on the host from the
oracle, row by row, and the arena is compared whole: the bytes before the
first row, the gaps between rows and at least 64 bytes behind the last row
must keep the sentinel."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from async_amd import _lib, b64
from oracle import pyoracle as orc
from tests import util
from tests.test_ragged_batch import SENT as ARENA_SENT
from tests.test_ragged_batch import _arena, _first_bad

DEV = "cuda:0"
SENT = 0xA5      # output arena filler: not an alphabet or pad character of any case
IN_FILL = 0x3C   # input buffer filler around the view
CANARY = 64
PATHS = {0: "nothing", 1: "flat", 2: "generic", 3: "tight2", 4: "strided"}

DEFAULT = (-1, -1, True, -1)
URL_HASH = ("-", "_", True, "#")
DOT_NOPAD = (".", "_", False, -1)


@functools.lru_cache(maxsize=None)
def hooks():
    """util.hooks() with the encode launcher's two hooks bound:
    b64x__test_encode_path(in, in_stride, len, nbuf, out, out_stride, pad,
    &magic, &rel_bound) -> path, and b64x__test_encode_grid_cap()."""
    L = util.hooks()
    L.b64x__test_encode_path.argtypes = [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
        ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32),
        ctypes.POINTER(ctypes.c_uint64)]
    L.b64x__test_encode_path.restype = ctypes.c_int
    L.b64x__test_encode_grid_cap.argtypes = []
    L.b64x__test_encode_grid_cap.restype = ctypes.c_int64
    return L


def test_encode_hooks_are_in_the_test_build_only():
    """Both hooks are exported by the hooks library and by neither product
    library (tests/test_abi.py::test_product_has_no_variant_knobs checks the
    product libraries for every b64x__ name)."""
    def names(path):
        return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True,
                              text=True, check=True).stdout
    exported = names(util.HOOKS)
    assert "b64x__test_encode_path" in exported
    assert "b64x__test_encode_grid_cap" in exported
    for path in (_lib.LIB_PATH, os.path.join(util.ROOT, "async_amd", "libasync_b64_core.so")):
        assert "b64x__" not in names(path), path


def encode_path(in_ptr, in_stride, length, nbuf, out_ptr, out_stride, pad):
    """(path name, magic, rel bound) of the launcher's decision for a call."""
    magic, bound = ctypes.c_uint32(0), ctypes.c_uint64(0)
    p = hooks().b64x__test_encode_path(in_ptr, in_stride, length, nbuf, out_ptr, out_stride,
                                       int(bool(pad)), ctypes.byref(magic), ctypes.byref(bound))
    return PATHS.get(p, p), magic.value, bound.value


def _placed(nbytes, mod, fill):
    """A device buffer filled with `fill` and the offset of a view of nbytes
    in it whose address is `mod` modulo 16, with at least 16 bytes before the
    view and CANARY behind it."""
    t = torch.full((nbytes + 32 + CANARY,), fill, dtype=torch.uint8, device=DEV)
    lead = 16 + (mod - (t.data_ptr() + 16)) % 16
    assert (t.data_ptr() + lead) % 16 == mod and t.numel() - lead - nbytes >= CANARY
    return t, lead


def _check_arena(got, lead, stride, E, wants, what):
    """The whole arena `got` against rows `wants` of E characters at lead +
    i * stride, everything else at SENT.  The layout and the report of the
    first bad row are test_ragged_batch's; its filler is an alphabet
    character, so the bytes outside the rows are set to SENT here, and for
    the report mapped back: its filler where they are intact, another byte
    where they are not."""
    nbuf = len(wants)
    out_off = np.append(lead + stride * np.arange(nbuf, dtype=np.int64), got.size)
    caps = np.full(nbuf, E, np.int64)
    _, _, expect, mask = _arena(out_off, caps, wants)
    assert mask.all() and expect.size == got.size
    outside = np.ones(got.size, bool)
    outside[(out_off[:-1, None] + np.arange(E)).ravel()] = False
    assert (expect[outside] == ARENA_SENT).all() and outside.sum() == got.size - nbuf * E
    expect[outside] = SENT
    if np.array_equal(got, expect):
        return
    seen = got.copy()
    seen[outside] = np.where(got[outside] == SENT, ARENA_SENT, ARENA_SENT ^ 0xFF)
    bad = _first_bad(seen, caps, out_off, caps, lambda i: wants[i], what)
    if bad is None:
        k = int(np.flatnonzero(got != expect)[0])
        bad = f"byte {k} of the arena, before the first row at {lead}, was written"
    pytest.fail(bad)


def _strided_case(length, nbuf, abc, path, in_mod=0, out_mod=0, in_gap=0, out_gap=0):
    """One b64x_encode_strided call of nbuf rows of `length` bytes, the bases
    at in_mod / out_mod modulo 16 and the strides in_gap / out_gap past tight:
    the path asserted, then the whole output arena against the oracle and the
    input buffer unchanged."""
    pad = abc[2]
    E = b64.encoded_len(length, pad)
    ins, outs = length + in_gap, E + out_gap
    rng = np.random.default_rng([length, nbuf, in_mod, out_mod, in_gap, out_gap])
    host = rng.integers(0, 256, (nbuf - 1) * ins + length, dtype=np.uint8)
    xbuf, il = _placed(host.size, in_mod, IN_FILL)
    xbuf[il:il + host.size] = torch.from_numpy(host).to(DEV)
    before = xbuf.cpu().numpy()
    obuf, ol = _placed((nbuf - 1) * outs + E, out_mod, SENT)
    x, o = xbuf[il:il + host.size], obuf[ol:]
    got_path = encode_path(x.data_ptr(), ins, length, nbuf, o.data_ptr(), outs, pad)[0]
    assert got_path == path, (length, E, nbuf, in_mod, out_mod, in_gap, out_gap)
    b64.encode_strided(x, ins, length, nbuf, o, outs, abc=abc)
    torch.cuda.synchronize()
    wants = [orc.encode(host[i * ins:i * ins + length], *abc, as_array=True) for i in range(nbuf)]
    assert all(w.size == E for w in wants)
    _check_arena(obuf.cpu().numpy(), ol, outs, E, wants, lambda i: (
        f"{path}, len {length}, E {E}, E mod 16 {E % 16}, nbuf {nbuf}, row at {i * outs} "
        f"(mod 16 {(out_mod + i * outs) % 16}), input base mod 16 {in_mod}, strides {ins}/{outs}, "
        f"alphabet {abc}"))
    assert np.array_equal(xbuf.cpu().numpy(), before), "the input buffer was written"


# ---- (a) k_encode_tight2 next to its guard ---------------------------------

# E, its lengths, the row counts: the passing E closest to the guard's limit
# in each class of E mod 16 (for every len mod 3), the largest passing E, and
# the passing neighbours of the first failure.  nbuf = 7 varies the blocks'
# start offsets and, for E mod 16 != 0, ends the output inside a slot.
TIGHT_PASS = [
    (61696, (46270, 46271, 46272), (2, 3, 7)),
    (69492, (52117, 52118, 52119), (2, 3, 7)),
    (78104, (58576, 58577, 58578), (2, 3, 7)),
    (372828, (279619, 279620, 279621), (2, 3)),
    (1046788, (785089, 785090, 785091), (2, 3)),
    (61876, (46406,), (2, 3, 7)),
    (61884, (46411,), (2, 3, 7)),
]
# The first E the guard refuses, three that fail it by less than 1e-4 of
# 2^32, and the E < 2^20 limit.
TIGHT_FAIL = [
    (61880, (46408, 46409, 46410)),
    (80744, (60557,)),
    (81788, (61340,)),
    (93028, (69770,)),
    (1 << 20, (786432,)),
]


def test_guard_cases_cover_the_classes():
    """The table itself (no GPU): the lengths give the E they stand under,
    the passing rows cover all four classes of E mod 16 and, at the E closest
    to the limit, every len mod 3."""
    for E, lens, *_ in TIGHT_PASS + TIGHT_FAIL:
        assert all((n + 2) // 3 * 4 == E for n in lens), E
    assert {E % 16 for E, _, _ in TIGHT_PASS} == {0, 4, 8, 12}
    for E, lens, _ in TIGHT_PASS[:5]:
        assert sorted(n % 3 for n in lens) == [0, 1, 2], E
    assert [E % 16 for E, _, _ in TIGHT_PASS[:4]] == [0, 4, 8, 12]


@pytest.mark.gpu
@pytest.mark.parametrize(
    "E,length,nbufs", [(E, n, nb) for E, lens, nb in TIGHT_PASS for n in lens],
    ids=lambda v: "nbuf" + "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tight_kernel_next_to_its_guard(E, length, nbufs):
    """Tight rows whose E passes the guard of the multiply-high division with
    little or nothing to spare: k_encode_tight2, whole arena."""
    assert b64.encoded_len(length) == E
    for nbuf in nbufs:
        _strided_case(length, nbuf, DEFAULT, "tight2")


@pytest.mark.gpu
@pytest.mark.parametrize("E,length", [(E, n) for E, lens in TIGHT_FAIL for n in lens])
def test_tight_layout_refused_by_the_guard(E, length):
    """Tight rows whose E the guard refuses (or E >= 2^20): the fallback
    k_encode_strided, whole arena."""
    assert b64.encoded_len(length) == E
    _strided_case(length, 3, DEFAULT, "strided")


@pytest.mark.gpu
def test_tight_and_refused_other_alphabets():
    """One passing and one refused E again under ('-', '_', pad '#'), and a
    passing one without padding (len mod 3 == 0 keeps it on k_encode_tight2)."""
    for nbuf in (2, 3, 7):
        _strided_case(58577, nbuf, URL_HASH, "tight2")
        _strided_case(58578, nbuf, DOT_NOPAD, "tight2")
    _strided_case(46409, 3, URL_HASH, "strided")


# ---- (b) every reason for the fallback -------------------------------------

LEN_B = 1000  # E = 1,336 (E mod 16 = 8), len mod 3 = 1: tight, aligned rows take k_encode_tight2


@pytest.mark.gpu
def test_fallback_base_shape_is_tight():
    """The shape the cases below each change in one respect is tight2's."""
    _strided_case(LEN_B, 5, DEFAULT, "tight2")


@pytest.mark.gpu
@pytest.mark.parametrize("out_mod", [4, 8, 12])
def test_fallback_output_not_16_aligned(out_mod):
    _strided_case(LEN_B, 5, DEFAULT, "strided", out_mod=out_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("in_mod", [1, 2, 3])
def test_fallback_input_not_4_aligned(in_mod):
    _strided_case(LEN_B, 5, DEFAULT, "strided", in_mod=in_mod)


@pytest.mark.gpu
def test_fallback_input_stride_not_tight():
    _strided_case(LEN_B, 5, DEFAULT, "strided", in_gap=4)


@pytest.mark.gpu
def test_fallback_output_stride_not_tight():
    _strided_case(LEN_B, 5, DEFAULT, "strided", out_gap=16)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [13, 14, 15])
def test_fallback_rows_shorter_than_16(length):
    _strided_case(length, 5, DEFAULT, "strided")


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1000, 1001])
def test_fallback_no_pad_partial_group(length):
    assert length % 3 in (1, 2)
    _strided_case(length, 5, DOT_NOPAD, "strided")


@pytest.mark.gpu
@pytest.mark.parametrize("in_gap,out_gap", [(1, 1), (3, 3), (2, 1), (0, 3)])
def test_fallback_odd_strides_every_alignment(in_gap, out_gap):
    """len = 1,027 (E = 1,372) with gaps of 1 and 3 bytes.  The output stride
    is odd in every case, so the five rows start at all four output
    alignments; an input gap of 1 or 3 makes the input stride even, so the
    gaps 2 and 0 (strides 1,029 and 1,027) are added to put the rows at all
    four input alignments too.  A row's last slot has 7 bytes: enc_tail where
    the row is dword aligned, enc_bytes elsewhere."""
    length, E = 1027, 1372
    ins, outs = length + in_gap, E + out_gap
    assert {i * outs % 4 for i in range(5)} == {0, 1, 2, 3}
    if ins % 2:
        assert {i * ins % 4 for i in range(5)} == {0, 1, 2, 3}
    _strided_case(length, 5, DEFAULT, "strided", in_gap=in_gap, out_gap=out_gap)


@pytest.mark.gpu
@pytest.mark.parametrize("in_mod,out_mod,path", [(0, 0, "flat"), (4, 8, "flat"), (1, 0, "generic"),
                                                 (0, 2, "generic"), (3, 5, "generic")])
def test_one_row_with_any_strides_is_a_single_buffer(in_mod, out_mod, path):
    """nbuf == 1 ignores the strides and takes the single-buffer kernels,
    k_encode_flat or k_encode by alignment: the same bytes."""
    for length in (LEN_B, 4097):
        _strided_case(length, 1, DEFAULT, path, in_mod=in_mod, out_mod=out_mod, in_gap=7,
                      out_gap=5)


# ---- (c) k_encode past one pass of its grid --------------------------------

SLOTS_PER_BLOCK = 1024  # kThreads x kEncUnroll slots of 12 bytes


@functools.lru_cache(maxsize=None)
def _generic_input(n):
    """n random bytes and the oracle's encoding of them, shared by the
    placements (read-only)."""
    data = np.random.default_rng(0xE1C).integers(0, 256, n, dtype=np.uint8)
    want = orc.encode(data, as_array=True)
    data.setflags(write=False)
    want.setflags(write=False)
    return data, want


def _grid_cap():
    cap = int(hooks().b64x__test_encode_grid_cap())
    assert 0 < cap <= 256 * 8 * 4, cap  # at most 2,048 threads a CU: 8 blocks of 256
    return cap


def _generic_case(n, in_mod, out_mod):
    data, want = _generic_input(n)
    xbuf, il = _placed(n, in_mod, IN_FILL)
    xbuf[il:il + n] = torch.tensor(data, device=DEV)  # a copy: data is read-only
    obuf, ol = _placed(want.size, out_mod, SENT)
    x, o = xbuf[il:il + n], obuf[ol:]
    assert encode_path(x.data_ptr(), n, n, 1, o.data_ptr(), 0, True)[0] == "generic"
    b64.encode(x, out=o)
    torch.cuda.synchronize()
    _check_arena(obuf.cpu().numpy(), ol, want.size, want.size, [want], lambda i: (
        f"generic, n {n}, input mod 16 {in_mod}, output mod 16 {out_mod}"))
    xh = xbuf.cpu().numpy()
    assert (xh[:il] == IN_FILL).all() and (xh[il + n:] == IN_FILL).all(), \
        "bytes around the input view changed"
    assert np.array_equal(xh[il:il + n], data), "the input view changed"


@pytest.mark.gpu
@pytest.mark.parametrize("in_mod,out_mod", [(1, 0), (0, 1), (2, 3)])
def test_generic_kernel_three_grid_passes(in_mod, out_mod):
    """A misaligned buffer of two full passes of k_encode's capped grid, then
    a partial pass with a tail (about 48 MiB on 256 CUs)."""
    n = 2 * _grid_cap() * SLOTS_PER_BLOCK * 12 + 5 * 12 + 7
    _generic_case(n, in_mod, out_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_generic_kernel_pass_boundary(extra):
    """Exactly one pass (the second is empty), then one byte more (the second
    pass holds one byte)."""
    _generic_case(_grid_cap() * SLOTS_PER_BLOCK * 12 + extra, 1, 0)


# ---- (d) the guard's arithmetic, on the CPU --------------------------------

EXHAUSTIVE_E = (24, 61696, 69492, 78104, 372828, 1046788, 61876, 61884)


def test_guard_admits_only_exact_divisions():
    """For every E (a multiple of 4) from 24 to 2^20 + 64, ask the launcher's
    own decision function, with aligned addresses and a tight padded layout.
    Where it answers tight2, its magic must divide exactly below its bound on
    rel: (rel * magic) >> 32 == rel // E.  Within [kE, (k+1)E) the error of
    the multiply-high grows with rel, so the worst cases are every kE - 1
    below the bound and bound - 1; for a few E every rel is checked.  The
    bound must cover the shipped kernel's offsets: rel = p0 + 16 * slot with
    p0 < E and slot < U * 256 lanes, U = 2 (k_encode_tight2<2> in
    tests/test_abi.py's SHIPPED_KERNELS)."""
    L = hooks()
    magic, bound = ctypes.c_uint32(0), ctypes.c_uint64(0)
    mref, bref = ctypes.byref(magic), ctypes.byref(bound)
    src, dst = 1 << 30, 1 << 31
    passing = []
    first_fail = None
    for E in range(24, (1 << 20) + 64 + 1, 4):
        n = E // 4 * 3
        p = L.b64x__test_encode_path(src, n, n, 2, dst, E, 1, mref, bref)
        assert PATHS[p] in ("tight2", "strided"), (E, p)
        if PATHS[p] != "tight2":
            if first_fail is None:
                first_fail = E
            continue
        passing.append(E)
        m, b = magic.value, bound.value
        assert b - E == 16 * 2 * 256, (E, b)
        if E in EXHAUSTIVE_E:
            rel = np.arange(b, dtype=np.uint64)
        else:
            rel = np.append(np.arange(E, b + 1, E, dtype=np.uint64) - np.uint64(1),
                            np.uint64(b - 1))
        q = (rel * np.uint64(m)) >> np.uint64(32)
        assert np.array_equal(q, rel // np.uint64(E)), (E, m, b)
    assert set(EXHAUSTIVE_E) <= set(passing)
    assert first_fail == 61880
    assert 61876 in passing and 61884 in passing
    assert max(passing) == 1046788
    assert sum(1 for E in passing if E < (1 << 20)) == len(passing) == 30654
    for E in (80744, 81788, 93028, 1 << 20):
        assert E not in passing
