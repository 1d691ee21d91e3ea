"""b64x_decode_strided at every branch of its launcher (decode_choice in
b64x_kernels.hip) and of k_rows_prep's choice among the four bodies of
k_decode_rows_lines.

Every GPU case first asks the hooks library (b64x__test_decode_rows_path)
which route the call's own addresses and shape take -- the ragged kernels,
the rows trio (k_rows_prep, k_decode_rows_lines<U, O32>, k_rows_finish) or
k_decode_slots + the fix-up -- and, for the rows trio, whether O32 is set,
and asserts both against the launcher's arithmetic restated here.  A case
that names a body runs in the hooks library (the same source) and reads the
RowModel its k_decode_rows_lines read (b64x__test_rows_model).  The model
selects the body:

    L == 0 and rcpS != 0                         clean rows, __umul24 division
    L == 0 and rcpS == 0                         clean rows, __umulhi division
    L != 0 and O32 and rcpS and L % 4 == 0 and rg    line-structured, row bands
    L != 0 otherwise                             line-structured, slot by slot

The other cases run in the product library, where b64x_diag_paths entries 3
and 4 (prep run, model reused) tell whether the rows trio ran.

The input arena is filled with 'Q' (an alphabet character of every tested
alphabet) outside the rows, so a kernel that decodes one byte too many
reports a wrong length (for a row whose alphabet characters are no multiple
of 4; two bytes too many always do); the output arena is filled with 0xA5.  Every row's
length and bytes are compared with oracle.pyoracle.decode of that row's
`len` characters, bit-exactly.  Bytes a row may use as scratch -- from its
length up to min(out_stride, 12 ceil(len / 16)) in a row with room, up to
decoded_cap(len) on the slots route and in the last row -- are gathered
with the rows; every other byte of the output arena must keep 0xA5 and every
byte of the input arena its value, both counted on the device."""
import ctypes
import functools
import os
import struct
import subprocess
from collections import namedtuple

import numpy as np
import pytest
import torch

from async_amd import _lib, b64
from oracle import pyoracle as orc
from tests import util
from tests.test_rows_bounds import REL_SPAN, launcher_gate, prep_gate, rcp_s

DEV = "cuda:0"
SENT = 0xA5          # output arena filler
IN_FILL = ord("Q")   # input arena filler: an alphabet character
JUNK = ord("*")      # in no tested alphabet, no separator, no pad character
LEAD = 64            # bytes of each arena before row 0 (plus the base's misalignment)
CANARY = 64
ROUTES = {0: "nothing", 1: "ragged", 2: "rows", 3: "slots"}

DEFAULT = (-1, -1, True, -1)
NL_CR = ("\n", "\r", True, -1)
URL = ("-", "_", True, -1)
BANG_EQ = ("!", "=", True, "#")

LF64 = (64, b"\n")
CRLF76 = (76, b"\r\n")
LF19 = (19, b"\n")
LF16 = (16, b"\n")

RowModel = namedtuple("RowModel", "L s P rcp S magic m64 F m k mL j0 rcpS len0 Sx pad m64x "
                                  "nb ru mx rg")
ROW_MODEL = struct.Struct("<6IQ6IQ2IQ4I")
assert ROW_MODEL.size == 96


@functools.lru_cache(maxsize=None)
def hooks():
    """util.hooks() with the decode launcher's two hooks bound:
    b64x__test_decode_rows_path(in, in_stride, len, nbuf, out, out_stride,
    &o32) -> route, and b64x__test_rows_model(stream, out[96])."""
    L = util.hooks()
    L.b64x__test_decode_rows_path.argtypes = [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
        ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    L.b64x__test_decode_rows_path.restype = ctypes.c_int
    L.b64x__test_rows_model.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.b64x__test_rows_model.restype = ctypes.c_int
    return L


def test_decode_hooks_are_in_the_test_build_only():
    """Both hooks are exported by the hooks library and by neither product
    library (tests/test_abi.py::test_product_has_no_variant_knobs checks the
    product libraries for every b64x__ name)."""
    def names(path):
        return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True,
                              text=True, check=True).stdout
    exported = names(util.HOOKS)
    assert "b64x__test_decode_rows_path" in exported
    assert "b64x__test_rows_model" in exported
    for path in (_lib.LIB_PATH, os.path.join(util.ROOT, "async_amd", "libasync_b64_core.so")):
        assert "b64x__" not in names(path), path


def decode_path(in_ptr, in_stride, length, nbuf, out_ptr, out_stride):
    """(route name, O32) of the launcher's decision for a call."""
    o32 = ctypes.c_int(-1)
    r = hooks().b64x__test_decode_rows_path(in_ptr, in_stride, length, nbuf, out_ptr, out_stride,
                                            ctypes.byref(o32))
    return ROUTES.get(r, r), bool(o32.value)


def expected_path(in_ptr, in_stride, length, nbuf, out_ptr, out_stride):
    """decode_choice restated: (route, O32, why the slots route)."""
    S = (length + 15) // 16
    if S * nbuf > 0xFFFFFFFF - 4096 or length > 0xFFFFFFFF:
        return "ragged", False, None
    if (in_ptr | out_ptr) & 3:
        return "slots", False, "alignment"
    if not (nbuf >= 2 and S >= 2 and out_stride >= 12 * S and in_stride % 4 == 0 and
            out_stride % 4 == 0):
        return "slots", False, "layout"
    if S >= 1 << 20:
        return "slots", False, "S >= 2^20"
    if not launcher_gate(S)[1]:
        return "slots", False, "gate"
    brows = (S + REL_SPAN) // S + 1
    if brows * in_stride >= 1 << 40:
        return "slots", False, "2^40"
    o32 = (in_stride < 1 << 24 and out_stride < 1 << 24 and brows * in_stride < 1 << 31 and
           brows * out_stride < 1 << 31)
    return "rows", o32, None


def body_of(m, o32):
    """Which body of k_decode_rows_lines<U, O32> a model selects (the rule
    in the module docstring)."""
    if m.L == 0:
        return "clean umul24" if m.rcpS else "clean umulhi"
    return "bands" if o32 and m.rcpS and m.L % 4 == 0 and m.rg else "lined slots"


def expected_body(length, fmt, abc, in_stride, out_stride, o32):
    """k_rows_prep's choice restated, for rows whose first row follows fmt."""
    S = (length + 15) // 16
    F, Sm = model_slots(length, fmt)
    chars = set(alphabet_chars(abc).tolist())
    lined = (fmt is not None and not (set(fmt[1]) & chars) and length >= 32 and
             prep_gate(Sm, in_stride))
    if not lined:
        return "clean umul24" if rcp_s(S) else "clean umulhi"
    Sx = min(out_stride // 12, S) if out_stride % 12 == 0 else Sm
    low = Sx & -Sx
    ru = 256 // min(low, 256)
    rg = (Sx < 4096 and 4 * ru * in_stride + length + 32 < 1 << 31 and
          4 * ru * out_stride < 1 << 31 and in_stride < 1 << 24 and out_stride < 1 << 24)
    rcps = rcp_s(Sx) if 16 * Sm <= 4096 else 0
    return "bands" if o32 and rcps and fmt[0] % 4 == 0 and rg else "lined slots"


def read_model(stream):
    buf = ctypes.create_string_buffer(96)
    rc = hooks().b64x__test_rows_model(stream, buf)
    assert rc == 0, rc
    return RowModel(*ROW_MODEL.unpack(buf.raw))


def alphabet_chars(abc):
    a = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/",
                      np.uint8).copy()
    for k, c in ((62, abc[0]), (63, abc[1])):
        if c != -1:
            a[k] = ord(c)
    return a


def model_slots(length, fmt):
    """(F, Sm): the model positions of a row of `length` characters in lines
    of fmt = (L, separator), and its slots (k_rows_prep's F and Sm); clean
    rows: (length, S)."""
    if fmt is None:
        return length, (length + 15) // 16
    L, P = fmt[0], fmt[0] + len(fmt[1])
    F = length // P * L + min(length % P, L)
    return F, (F + 15) // 16


def model_pos(i, fmt):
    """The position in the row of model character i."""
    if fmt is None:
        return i
    L, P = fmt[0], fmt[0] + len(fmt[1])
    return i // L * P + i % L


def junk_rows(nbuf):
    """(rows with a junk byte in an interior slot, rows with one in their
    last slot): never only row 0, never the last row."""
    if nbuf >= 100:
        return (1, nbuf // 2), (2, nbuf - 2)
    if nbuf >= 4:
        return (1,), (2,)
    assert nbuf == 3
    return (0,), (1,)


def make_rows(length, nbuf, fmt, abc, tail="", junk=None, seed=0):
    """nbuf rows of `length` characters (host, nbuf x length): random alphabet
    characters, in lines of fmt = (L, separator) if given; tail "pad" ends
    every row in two pad characters.  Junk bytes as junk_rows says (or the
    given pair of row lists): in an interior slot at the middle of the row,
    and at the first character of the row's last slot."""
    rng = np.random.default_rng([length, nbuf, seed, 0 if fmt is None else fmt[0]])
    rows = alphabet_chars(abc)[rng.integers(0, 64, (nbuf, length))]
    if fmt is not None:
        L, sep = fmt
        col = np.arange(length) % (L + len(sep))
        for j, b in enumerate(sep):
            rows[:, col == L + j] = b
    if tail == "pad":
        assert fmt is None and ord("=") not in alphabet_chars(abc)
        rows[:, -2:] = ord("=")
    F, Sm = model_slots(length, fmt)
    interior, last = junk_rows(nbuf) if junk is None else junk
    p_in = model_pos(16 * ((Sm - 1) // 2) + 5, fmt)
    p_last = model_pos(16 * (Sm - 1), fmt)
    assert p_in < p_last < length and Sm >= 2
    for r in interior:
        # row 0 gives the model: its junk lies past the 256 bytes the probe reads
        assert r != nbuf - 1 and (r != 0 or p_in >= 256 or junk is not None)
        rows[r, p_in] = JUNK
    for r in last:
        assert r != nbuf - 1
        rows[r, p_last] = JUNK
    return rows


def oracle_rows(rows, abc):
    return [orc.decode(r, abc[0], abc[1], as_array=True) for r in rows]


def _arena(nbytes, mod, fill):
    """A device arena filled with `fill` and the offset of row 0 in it, whose
    address is `mod` modulo 4 (LEAD bytes before it, CANARY past nbytes)."""
    t = torch.full((LEAD + 4 + nbytes + CANARY,), fill, dtype=torch.uint8, device=DEV)
    lead = LEAD + (mod - (t.data_ptr() + LEAD)) % 4
    assert (t.data_ptr() + lead) % 4 == mod and t.numel() - lead - nbytes >= CANARY
    return t, lead


def _rows_view(t, lead, nbuf, width, stride):
    assert lead + (nbuf - 1) * stride + width <= t.numel()
    return torch.as_strided(t, (nbuf, width), (stride, 1), lead)


def _other(t, fill):
    return int(torch.count_nonzero(t != fill))


def _diag(lib):
    out = (ctypes.c_uint64 * 5)()
    lib.b64x_diag_paths(out)
    return out[3] + out[4]


def run_case(rows, fmt, abc, in_stride, out_stride, route, o32=None, body=None, why=None,
             in_mod=0, out_mod=0, tight_end=False, wants=None, xbuf=None):
    """One b64x_decode_strided call of the rows (host, nbuf x len) at the
    given strides, bases at in_mod / out_mod modulo 4: the route (and O32)
    asserted from the hook and from the launcher's arithmetic restated, the
    call, the model and body where `body` is given, then every row's length
    and bytes against the oracle, the guard bytes of the output arena and
    the input arena unchanged.  Returns the model (or None)."""
    nbuf, length = rows.shape
    S, cap = (length + 15) // 16, b64.decoded_cap(length)
    what = (f"len {length}, S {S}, nbuf {nbuf}, fmt {fmt}, strides {in_stride}/{out_stride}, "
            f"bases mod 4 {in_mod}/{out_mod}, alphabet {abc}")
    if wants is None:
        wants = oracle_rows(rows, abc)
    assert len(rows[-1]) and JUNK not in rows[-1], "the last row is not deviant"
    # arenas: rows through a strided view; the last row may end the input arena
    in_bytes = (nbuf - 1) * in_stride + length
    if xbuf is None:
        xbuf, il = _arena(in_bytes, in_mod, IN_FILL)
        if tight_end:
            xbuf = xbuf[:il + in_bytes]
    else:
        xbuf, il = xbuf
        xbuf.fill_(IN_FILL)
    dev_rows = torch.tensor(rows, device=DEV)  # a copy: shared rows are read-only
    _rows_view(xbuf, il, nbuf, length, in_stride).copy_(dev_rows)
    n_in_other = _other(xbuf, IN_FILL)
    width = min(out_stride, 12 * S) if route == "rows" else cap
    obuf, ol = _arena((nbuf - 1) * out_stride + max(width, cap), out_mod, SENT)
    outlen = torch.full((nbuf,), -1, dtype=torch.int64, device=DEV)
    x, o = xbuf[il:], obuf[ol:]
    # the route, from the hook and from the restated arithmetic
    args = (x.data_ptr(), in_stride, length, nbuf, o.data_ptr(), out_stride)
    exp_route, exp_o32, exp_why = expected_path(*args)
    got_route, got_o32 = decode_path(*args)
    assert (got_route, got_o32) == (exp_route, exp_o32), what
    assert got_route == route and exp_why == why, (got_route, exp_why, what)
    if o32 is not None:
        assert got_o32 == o32, what
    if body is not None:
        assert expected_body(length, fmt, abc, in_stride, out_stride, got_o32) == body, what
    # the call: in the hooks library where the model is read
    lib = hooks() if body is not None else _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    lib.b64x_release_stream(stream)  # no model of an earlier batch of this shape is reused
    before = _diag(lib)
    a = _lib.alphabet(*abc)
    torch.cuda.synchronize()
    _lib.check("b64x_decode_strided", lib.b64x_decode_strided(
        x.data_ptr(), in_stride, length, nbuf, o.data_ptr(), out_stride, outlen.data_ptr(),
        ctypes.byref(a), stream))
    torch.cuda.synchronize()
    assert _diag(lib) - before == (1 if route == "rows" else 0), what
    model = None
    if body is not None:
        model = read_model(stream)
        assert body_of(model, got_o32) == body, (model, what)
    # lengths and bytes
    lens = outlen.cpu().numpy()
    want_lens = np.array([w.size for w in wants], np.int64)
    bad = np.flatnonzero(lens != want_lens)
    assert bad.size == 0, (f"row {bad[0]}: length {lens[bad[0]]}, the oracle's "
                           f"{want_lens[bad[0]]}; {bad.size} rows differ; {what}")
    got = _rows_view(obuf, ol, nbuf, max(width, cap), out_stride).cpu().numpy()
    for i, w in enumerate(wants):
        if not np.array_equal(got[i, :w.size], w):
            k = int(np.flatnonzero(got[i, :w.size] != w)[0])
            pytest.fail(f"row {i}: byte {k} of {w.size} is {got[i, k]:#x}, the oracle's "
                        f"{w[k]:#x}; {what}")
    # guards: nothing but the rows' windows was written
    allowed = int(np.count_nonzero(got[:-1, :width] != SENT)) + \
        int(np.count_nonzero(got[-1, :cap] != SENT))
    written = _other(obuf, SENT)
    assert written == allowed, (f"{written - allowed} bytes outside the rows' windows were "
                                f"written; {what}")
    assert (got[:-1, width:] == SENT).all() and (got[-1, cap:] == SENT).all(), what
    # the input: the rows as written, everything else the filler
    assert torch.equal(_rows_view(xbuf, il, nbuf, length, in_stride), dev_rows), what
    assert _other(xbuf, IN_FILL) == n_in_other, f"the input arena was written; {what}"
    return model


def up4(n):
    return (n + 3) // 4 * 4


# ---- (a) clean rows on either side of rcpS -----------------------------------

# S, len mod 16 (0 = 16), the rows' ends: 657 and 670 are the first S for
# which the prep sets no rcpS (tests/test_rows_bounds.py), 656 and 658 have it.
CLEAN_A = [(656, 15, ""), (657, 1, ""), (658, 16, ""), (670, 4, "pad")]


def test_clean_cases_cover_the_ends():
    """The table itself (no GPU): both divisions, every len mod 16 asked
    for, and ends that are padded, unpadded and cut inside a group -- with
    the oracle decoding each to the length the end implies."""
    assert [bool(rcp_s(S)) for S, _, _ in CLEAN_A] == [True, False, True, False]
    assert sorted(r % 16 for _, r, _ in CLEAN_A) == [0, 1, 4, 15]
    for S, r, tail in CLEAN_A:
        length = 16 * (S - 1) + r
        rows = make_rows(length, 5, None, DEFAULT, tail)
        want = orc.decode(rows[-1], as_array=True).size
        assert want == ((length - 2) * 6 // 8 if tail else length * 6 // 8)
        assert orc.decode(rows[1], as_array=True).size == (length - 1 - 2 * bool(tail)) * 6 // 8
    assert {(16 * (S - 1) + r) % 4 for S, r, _ in CLEAN_A} >= {0, 1, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("S,r,tail", CLEAN_A)
def test_clean_rows_either_division(S, r, tail):
    """301 clean rows at S slots: the __umul24 body where rcpS is set, the
    __umulhi body at S = 657 and 670."""
    length = 16 * (S - 1) + r
    rows = make_rows(length, 301, None, DEFAULT, tail)
    m = run_case(rows, None, DEFAULT, up4(length), 12 * S, "rows", o32=True,
                 body="clean umul24" if rcp_s(S) else "clean umulhi")
    assert (m.L, m.rcpS) == (0, rcp_s(S))


# ---- (b), (c) the launcher's gate and S < 2^20 --------------------------------

@functools.lru_cache(maxsize=2)
def _big_clean(S):
    """Three clean rows of 16 S - 3 characters and the oracle's decoding,
    shared by the placements (read-only)."""
    rows = make_rows(16 * S - 3, 3, None, DEFAULT)
    wants = oracle_rows(rows, DEFAULT)
    rows.setflags(write=False)
    return rows, wants


@pytest.mark.gpu
@pytest.mark.parametrize("S,route", [(65093, "rows"), (65094, "slots"), (65536, "rows"),
                                     (65537, "slots")])
def test_clean_rows_next_to_the_launcher_gate(S, route):
    """relmax * e < 2^32 holds below S = 65,094 and at 65,536, fails at
    65,094 and 65,537: the rows trio at the largest rel * e of its
    neighbourhood, k_decode_slots past it."""
    rows, wants = _big_clean(S)
    assert launcher_gate(S)[1] == (route == "rows")
    body = ("clean umul24" if rcp_s(S) else "clean umulhi") if route == "rows" else None
    run_case(rows, None, DEFAULT, 16 * S, 12 * S, route, o32=route == "rows" or None,
             body=body, why=None if route == "rows" else "gate", wants=wants)


@pytest.mark.gpu
@pytest.mark.parametrize("in_stride,o32", [(16 * 1048321, True), (1 << 24, False)])
def test_clean_rows_at_the_largest_passing_S(in_stride, o32):
    """S = 1,048,321, the largest S the gate admits: rows of 16 MiB.  Tight
    rows still have 32-bit offsets (two rows of a block span under 2^31
    bytes, the strides are below 2^24); an input stride of 2^24 takes the
    64-bit form."""
    S = 1048321
    rows, wants = _big_clean(S)
    m = run_case(rows, None, DEFAULT, in_stride, 12 * S, "rows", o32=o32, body="clean umulhi",
                 wants=wants)
    assert m.L == 0 and m.S == 0 and m.j0 == 13


@pytest.mark.gpu
def test_clean_rows_of_2_20_slots_take_the_slots_route():
    S = 1 << 20
    rows, wants = _big_clean(S)
    run_case(rows, None, DEFAULT, 16 * S, 12 * S, "slots", why="S >= 2^20", wants=wants)


# ---- (d) O32 false with small rows -------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fmt,body", [(None, "clean umul24"), (CRLF76, "lined slots")],
                         ids=["clean", "crlf76"])
@pytest.mark.parametrize("wide", ["in", "out"])
def test_small_rows_with_a_stride_of_2_24(wide, fmt, body):
    """Rows of 1,368 characters with an input or an output stride of 2^24:
    k_decode_rows_lines<U, false>; for CRLF-76 rows rg == 0, the lined body
    slot by slot."""
    length = 1368
    rows = make_rows(length, 5, fmt, DEFAULT)
    ins, outs = (1 << 24, 12 * 86) if wide == "in" else (length, 1 << 24)
    m = run_case(rows, fmt, DEFAULT, ins, outs, "rows", o32=False, body=body)
    assert (m.L, m.rg) == (76 if fmt else 0, 0)


# ---- (e) the 2^31 edge of O32 -------------------------------------------------

def _edge_stride(length, nbuf, out_stride, want):
    """The largest in_stride (a multiple of 4) for which the hook answers
    want(route, o32), the next multiple failing it; by bisection."""
    src, dst = 1 << 32, 1 << 44
    lo, hi = up4(length) // 4, 1 << 40
    assert want(*decode_path(src, 4 * lo, length, nbuf, dst, out_stride))
    assert not want(*decode_path(src, 4 * hi, length, nbuf, dst, out_stride))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if want(*decode_path(src, 4 * mid, length, nbuf, dst, out_stride)):
            lo = mid
        else:
            hi = mid
    return 4 * lo


@pytest.mark.gpu
@pytest.mark.parametrize("length,fmt,out_stride", [(32, None, 24), (33, LF16, 36)],
                         ids=["clean", "lf16"])
def test_o32_edge_of_the_input_stride(length, fmt, out_stride):
    """600 rows of 32 clean characters (S = 2: 514 rows to a block), and of
    33 characters in lines of 16 + LF (the model's Sm = 2 where the
    launcher's S = 3: a block spans more rows than the launcher's brows), at
    the largest input stride with O32 and the smallest without.  The arenas
    are built on the device."""
    nbuf, S = 600, (length + 15) // 16
    brows = (S + REL_SPAN) // S + 1
    edge = _edge_stride(length, nbuf, out_stride, lambda route, o32: route == "rows" and o32)
    assert edge == ((1 << 31) - 1) // brows // 4 * 4
    assert (nbuf - 1) * (edge + 4) + length + 256 < 1 << 32
    rows = make_rows(length, nbuf, fmt, DEFAULT, junk=((1, 300), (2, 598)))
    wants = oracle_rows(rows, DEFAULT)
    xbuf = _arena((nbuf - 1) * (edge + 4) + length, 0, IN_FILL)
    for stride, o32 in ((edge, True), (edge + 4, False)):
        m = run_case(rows, fmt, DEFAULT, stride, out_stride, "rows", o32=o32,
                     body=("lined slots" if fmt else "clean umul24"), wants=wants, xbuf=xbuf)
        assert (m.L, m.S) == ((16, 2) if fmt else (0, 0))


# ---- (f) the 2^40 gate ---------------------------------------------------------

@pytest.mark.gpu
def test_input_stride_gate_of_2_40():
    """Two rows of 32 characters (S = 2, 514 rows to a block) at the largest
    input stride on the rows route, 2^40 / 514 rounded down, and at the next
    multiple of 4, which takes k_decode_slots.  With two rows and a last row
    that is not deviant, row 0 carries the junk: once in its interior slot,
    once in its last."""
    length, nbuf = 32, 2
    edge = _edge_stride(length, nbuf, 24, lambda route, o32: route == "rows")
    assert edge == ((1 << 40) - 1) // 514 // 4 * 4
    xbuf = _arena(edge + 4 + length, 0, IN_FILL)
    assert xbuf[0].numel() < 1 << 32
    for junk in (((0,), ()), ((), (0,))):
        rows = make_rows(length, nbuf, None, DEFAULT, junk=junk)
        # (a junk byte at row 0's character 16 reads as a line of 16 to the
        # probe: that variant names no body)
        run_case(rows, None, DEFAULT, edge, 24, "rows", o32=False,
                 body=None if junk[1] else "clean umul24", xbuf=xbuf)
        run_case(rows, None, DEFAULT, edge + 4, 24, "slots", why="2^40", xbuf=xbuf)


# ---- (g) CRLF-76 rows at the launcher's and the prep's gates -------------------

# lines, the launcher's gate on S, the prep's gate on Sm
GATES_G = [(13000, True, True), (13437, False, True), (13704, True, False),
           (14058, False, False)]


@functools.lru_cache(maxsize=1)
def _big_lined(lines):
    rows = make_rows(78 * lines, 3, CRLF76, DEFAULT)
    wants = oracle_rows(rows, DEFAULT)
    rows.setflags(write=False)
    return rows, wants


def test_gate_cases_decode_to_whole_lines():
    """The tables of the lined cases (no GPU): the oracle decodes a row that
    is not deviant to floor(6 F / 8) bytes of its F model characters, one
    with a junk byte to one character less."""
    for lines, launcher, prep in GATES_G:
        length = 78 * lines
        F, Sm = model_slots(length, CRLF76)
        assert F == 76 * lines
        assert launcher_gate((length + 15) // 16)[1] == launcher
        assert prep_gate(Sm, up4(length)) == prep
    rows, wants = _big_lined(13000)
    assert [w.size for w in wants] == [(76 * 13000 - 1) * 6 // 8] * 2 + [76 * 13000 * 6 // 8]
    for fmt, length in ((LF64, 1368), (CRLF76, 5464), (LF19, 1400), (LF16, 33)):
        F, _ = model_slots(length, fmt)
        rows = make_rows(length, 5, fmt, DEFAULT)
        assert [w.size for w in oracle_rows(rows, DEFAULT)] == \
            [F * 6 // 8, (F - 1) * 6 // 8, (F - 1) * 6 // 8, F * 6 // 8, F * 6 // 8]


@pytest.mark.gpu
@pytest.mark.parametrize("lines,launcher,prep", GATES_G)
def test_crlf76_rows_at_both_gates(lines, launcher, prep):
    """Three CRLF-76 rows of about 1 MB at the four outcomes of (launcher's
    gate on S, prep's gate on Sm).  The launcher passing and the prep
    declining: the rows are decoded under the clean model, every row fails
    it and k_rows_finish decodes them all.  Both passing: the lined body slot
    by slot (Sx >= 4,096: no bands)."""
    rows, wants = _big_lined(lines)
    length = 78 * lines
    F, Sm = model_slots(length, CRLF76)
    if not launcher:
        run_case(rows, CRLF76, DEFAULT, up4(length), 12 * ((length + 15) // 16), "slots",
                 why="gate", wants=wants)
        return
    m = run_case(rows, CRLF76, DEFAULT, up4(length), 12 * ((length + 15) // 16), "rows", o32=True,
                 body="lined slots" if prep else "clean umulhi", wants=wants)
    if prep:
        assert (m.L, m.s, m.S, m.F) == (76, 2, Sm, F)
        assert m.rg == 0 or m.Sx >= 4096
    else:
        assert m.L == 0


# ---- (h) line-structured rows on either side of Sx = 4,096 ----------------------

def _len_for_slots(fmt, sm):
    """A row length whose model has exactly sm slots, the last one partial."""
    L, P = fmt[0], fmt[0] + len(fmt[1])
    F = 16 * sm - 8
    length = F // L * P + F % L
    assert model_slots(length, fmt) == (F, sm)
    return length


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [LF64, CRLF76], ids=["lf64", "crlf76"])
@pytest.mark.parametrize("form,sx", [("whole", 4095), ("whole", 4097), ("plain", 4095),
                                     ("plain", 4097)])
def test_lined_rows_around_4096_slots(fmt, form, sx):
    """Rows of 64 Ki to 70 Ki characters with Sx just below and just above
    4,096, in both forms of Sx: out_stride a whole number of 12-byte slots
    (Sx = the launcher's S) and not (Sx = the model's Sm).  Below 4,096 the
    prep fills the band mapping, above it does not; rows this long have no
    rcpS (16 Sm > 4,096), so both sides decode slot by slot, the line
    division __umulhi(i, mL) running at i up to 65,536."""
    if form == "whole":
        length = 16 * sx - 1          # S = sx
        out_stride = 12 * sx
    else:
        length = _len_for_slots(fmt, sx)
        out_stride = 12 * ((length + 15) // 16) + 4
    assert 65000 < length < 70 * 1024 and out_stride % 12 == (0 if form == "whole" else 4)
    rows = make_rows(length, 5, fmt, DEFAULT)
    m = run_case(rows, fmt, DEFAULT, up4(length), out_stride, "rows", o32=True, body="lined slots")
    assert (m.L, m.s, m.Sx, m.rcpS) == (fmt[0], len(fmt[1]), sx, 0)
    assert m.S == model_slots(length, fmt)[1]
    assert (m.nb != 0) == (sx < 4096) and (m.rg != 0) == (sx < 4096)


# ---- (i) line-structured rows with gaps between them ----------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fmt,length,body", [(CRLF76, 1404, "bands"), (CRLF76, 1380, "bands"),
                                             (CRLF76, 1324, "bands"),
                                             (LF19, 1400, "lined slots"),
                                             (LF19, 1388, "lined slots")])
@pytest.mark.parametrize("gap", [4, 24, 4096])
def test_lined_rows_with_gaps_of_alphabet_characters(fmt, length, body, gap):
    """in_stride = len + gap with 'Q' in the gaps, rows that end in a
    separator (1,404 and 1,400), with a line's last character (1,324) and
    inside a line: no gap byte is decoded.  One character too many adds a
    byte wherever the row's characters are no multiple of 4 (1,380, 1,400,
    1,388).  The last row ends the input arena."""
    rows = make_rows(length, 5, fmt, DEFAULT)
    S = (length + 15) // 16
    m = run_case(rows, fmt, DEFAULT, length + gap, 12 * S + 8, "rows", o32=True, body=body,
                 tight_end=True)
    assert (m.L, m.S) == (fmt[0], model_slots(length, fmt)[1])


# ---- (j) misaligned bases ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [None, CRLF76], ids=["clean", "crlf76"])
@pytest.mark.parametrize("in_mod,out_mod", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3)])
def test_misaligned_bases_take_the_slots_route(in_mod, out_mod, fmt):
    """Strides that are multiples of 4 and rows with room, but a base at 1, 2
    or 3 modulo 4: k_decode_slots, reached through the alignment condition."""
    length = 1368
    rows = make_rows(length, 5, fmt, DEFAULT)
    run_case(rows, fmt, DEFAULT, length + 4, 12 * 86, "slots", why="alignment", in_mod=in_mod,
             out_mod=out_mod)


@pytest.mark.gpu
def test_aligned_bases_of_the_same_shape_take_the_rows_route():
    run_case(make_rows(1368, 5, None, DEFAULT), None, DEFAULT, 1372, 12 * 86, "rows", o32=True)


@pytest.mark.gpu
def test_rows_model_of_a_stream_without_a_workspace():
    """b64x__test_rows_model answers -ENOENT for a stream that holds no
    library workspace."""
    s = torch.cuda.Stream()
    buf = ctypes.create_string_buffer(96)
    assert hooks().b64x__test_rows_model(s.cuda_stream, buf) == -2


# ---- (k) alphabets ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("abc", [NL_CR, URL, BANG_EQ], ids=["nl-cr", "url", "bang-eq"])
@pytest.mark.parametrize("fmt", [None, LF64, CRLF76], ids=["clean", "lf64", "crlf76"])
@pytest.mark.parametrize("length", [1368, 5464])
def test_rows_under_other_alphabets(length, fmt, abc):
    """301 rows under alphabets whose 62 and 63 are separator bytes, URL
    characters, and '!' with '=' (the pad character of the others).  With LF
    in the alphabet, lines ending in LF are not line-structured at all: the
    model is clean, and with CR in it too, CRLF-76 rows are all alphabet."""
    rows = make_rows(length, 301, fmt, abc)
    S = (length + 15) // 16
    clean = "clean umul24" if rcp_s(S) else "clean umulhi"
    m = run_case(rows, fmt, abc, length, 12 * S, "rows", o32=True,
                 body=(clean if fmt is None or abc is NL_CR else
                       "bands" if length == 1368 else "lined slots"))
    if fmt is None or abc is NL_CR:
        assert m.L == 0
    else:
        assert (m.L, m.s) == (fmt[0], len(fmt[1]))
