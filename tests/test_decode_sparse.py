"""The lenient decoder's exact paths on alphabet-sparse text and at the edges
of their units (ranges, tiles, 64-byte completion windows, scan tiles, the
hand-off from k_decode_lines), bytes and result record against the oracle.

The texts come from tests/sparse_corpus.py; test_corpus_reaches_every_case
(no GPU) asserts that they hold what dense text never does: ranges with fewer
alphabet characters than the group open at their start needs, completion
windows holding some but not all of the characters needed, completions that
run two ranges on, start at a tile edge or reach the end of the stream at
every V mod 4, and tails that span several windows.

Every single-buffer case lays its texts out in one input arena ('Q', an
alphabet character, between them) and one output arena (0xA5, 64 guard bytes
on both sides of each text's decoded_cap), decodes each text on its own and
copies the arena back once.  Per text: the bytes up to out_len, the whole
record (read through Decoded.info()), tail[] against the sextets of the last
V mod 4 alphabet characters, and both guards.  Bytes from out_len up to the
capacity are unspecified and not looked at.

Routes, each asserted by the deltas of b64x_diag_paths:
    auto    a caller's workspace, zeroed, after a call of another length on
            it (nothing held): the probe, k_decode_lines, the suffix from
            the probe's cut -- and the same call again at once, which the
            probe's hint sends to the single pass
    junk    B64X_DEC_EXPECT_JUNK: the single pass, no counter moves
    3, 8    the hooks library with ranges of 3 and 8 chunks: pass 1, the
            scan, pass 2 (the corpus generated for that range length)
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from async_amd import _lib, b64
from async_amd.session import Session
from oracle import pyoracle as orc
from tests import sparse_corpus as sc
from tests import test_decode_dispatch as dd
from tests import util
from tests.test_gpu_parity import _junk, _sfx_start, _wrap

DEV = "cuda:0"
SENT = 0xA5
GUARD = 64
DEFAULT = (-1, -1)
NL_CR = ("\n", "\r")
NONE = 2**64 - 1   # sfx_start of a call whose suffix decode had nothing to do
PROBE, HELD, HINT = 0, 1, 2

Item = namedtuple("Item", "name text ia oa ref")
Ref = namedtuple("Ref", "want V tail")

# input arenas and workspaces of this module stay allocated: the probe's hint
# is keyed on (workspace, input address, length), and an address handed out
# twice would let one case's hint pick another case's route
_KEEP = []


# ---- the corpus and its reference (no GPU) --------------------------------------

def reference(text: np.ndarray, abc=DEFAULT) -> Ref:
    """The oracle's bytes, V and the sextets of the last V mod 4 alphabet
    characters."""
    table = np.array(orc.decode_table(*abc), np.int16)
    vals = table[text]
    sext = vals[vals >= 0]
    V = int(sext.size)
    want = orc.decode(text, abc[0], abc[1], as_array=True)
    assert want.size == V * 6 // 8
    return Ref(want, V, [int(v) for v in sext[V - V % 4:]] if V % 4 else [])


def _items(texts, abc=DEFAULT, aligns=((0, 0),)):
    out = []
    for name, t in texts:
        ref = reference(t, abc)
        t.setflags(write=False)
        for ia, oa in aligns:
            out.append(Item(f"{name} in+{ia} out+{oa}" if (ia, oa) != (0, 0) else name, t, ia, oa,
                            ref))
    return out


ALIGNS = ((0, 1), (1, 0), (1, 1))  # (0, 0) is in the corpus itself


@functools.lru_cache(maxsize=None)
def corpus_items(R):
    """The whole corpus at range length R, aligned."""
    return _items(sc.corpus(R))


@functools.lru_cache(maxsize=None)
def edge_items(R):
    """The thirteen `every` texts at the base length: at the three other
    placements of input and output modulo 16, and under the alphabet whose
    62 and 63 are LF and CR."""
    n0 = sc.base_len(R)
    return (_items(sc.every_at(R, n0), DEFAULT, ALIGNS),
            _items(sc.every_at(R, n0, NL_CR), NL_CR))


@functools.lru_cache(maxsize=None)
def group_items():
    """65 tiles of the single pass and 37 characters: a block's prefix
    crosses a group sum (64 tiles)."""
    R = 2048
    n = 65 * sc.TILE * R + 37
    assert n == 2_129_957
    return _items([(f"every({g},0,{n})", sc.every(g, 0, n)) for g in (2, 64, R + 1)])


@pytest.mark.parametrize("R", [2048, 3072])
def test_corpus_reaches_every_case(R):
    """Over the corpus at range length R (16 ranges to a tile), every count
    of sparse_corpus.range_stats is reached by some text, and completions run
    out of stream at V mod 4 = 1, 2 and 3."""
    texts = sc.corpus(R)
    assert len(texts) == 4 * (15 + 28)
    tot = sc.corpus_stats(texts, R, sc.TILE)
    for k in sc.COUNTS:
        assert tot[k] > 0, (k, tot)
    assert all(tot["to_end"][v] > 0 for v in (1, 2, 3)), tot
    # every text shows junk in its first 16 bytes: the probe cuts at slot 0
    for name, t in texts:
        assert sc.JUNK in t[:16], name
    # the junk byte is in no tested alphabet, the arena's filler in all
    for abc in (DEFAULT, NL_CR):
        assert orc.decode_table(*abc)[sc.JUNK] < 0 <= orc.decode_table(*abc)[ord("Q")]


def test_group_texts_cross_a_group_sum():
    """The 2,129,957-character texts: 66 tiles, so the last two take the sum
    of a whole group of 64 as their prefix; with one character to a range
    and a byte, every fourth range completes its group three ranges on."""
    R, n = 2048, 65 * sc.TILE * 2048 + 37
    assert (n + R - 1) // R == 65 * sc.TILE + 1
    s = sc.range_stats(sc.every(R + 1, 0, n), R)
    assert s["far"] >= 65 * sc.TILE // 4 - 1 and s["few"] > 0, s


# ---- one group of single-buffer decodes ------------------------------------------

def _up(x, a):
    return (x + a - 1) // a * a


def _cap(n):
    return (n + 3) // 4 * 3


def _paths(lib):
    out = (ctypes.c_uint64 * 5)()
    lib.b64x_diag_paths(out)
    return [int(v) for v in out]


def _decode(lib, x, n, out, res, abc, flags, ws):
    """b64x_decode_dev_seq of `lib` on the current stream; the Decoded."""
    seq = ctypes.c_uint32(0)
    a = _lib.alphabet(abc[0], abc[1], True, -1)
    _lib.check("b64x_decode_dev_seq", lib.b64x_decode_dev_seq(
        x.data_ptr(), n, out.data_ptr(), res.data_ptr(), ctypes.byref(a), flags,
        ws.data_ptr() if ws is not None else None, torch.cuda.current_stream().cuda_stream,
        ctypes.byref(seq)))
    return b64.Decoded(out, res, n, flags & b64.HOLD_TAIL, seq.value)


def check_record(info, ref, n, hold, what):
    assert (info.nchars, info.flags) == (n, int(hold)) and info.seq != 0, what
    assert info.valid == ref.V, (info.valid, ref.V, what)
    assert info.tail_n == ref.V % 4, (info.tail_n, ref.V, what)
    assert info.out_len == (ref.V // 4 * 3 if hold else ref.want.size), (info.out_len, what)
    assert list(info.tail[:info.tail_n]) == ref.tail, (list(info.tail), ref.tail, what)
    assert all(v == 0 for v in info.tail[info.tail_n:]), (list(info.tail), what)


def check_bytes(got, out_len, ref, what):
    want = ref.want[:out_len]
    if not np.array_equal(got[:out_len], want):
        k = int(np.flatnonzero(got[:out_len] != want)[0])
        pytest.fail(f"byte {k} of {out_len} is {got[k]:#x}, the oracle's {want[k]:#x}; {what}")


class Arena:
    """The texts of a group in one device buffer and their outputs in
    another: text i at in_off[i] (16-aligned plus its ia), its capacity at
    out_off[i] (16-aligned plus its oa) between two guards."""

    def __init__(self, items, outputs=1):
        self.items = items
        self.in_off, self.out_off = [], []
        pi = po = 0
        for it in items:
            n = it.text.size
            io = _up(pi, 64) + GUARD + it.ia
            oo = _up(po, 16) + GUARD + it.oa
            self.in_off.append(io)
            self.out_off.append(oo)
            pi, po = io + n, oo + _cap(n) + GUARD
        host = np.full(pi + GUARD, ord("Q"), np.uint8)
        for it, io in zip(items, self.in_off):
            host[io:io + it.text.size] = it.text
        self.x = torch.from_numpy(host).to(DEV)
        _KEEP.append(self.x)
        assert self.x.data_ptr() % 16 == 0
        self.outs = [torch.full((po + 16,), SENT, dtype=torch.uint8, device=DEV)
                     for _ in range(outputs)]
        assert all(o.data_ptr() % 16 == 0 for o in self.outs)
        self.res = torch.zeros(max(len(items), 1) * outputs * 48, dtype=torch.uint8, device=DEV)

    def text(self, i):
        return self.x[self.in_off[i]:self.in_off[i] + self.items[i].text.size]

    def out(self, i, k=0):
        return self.outs[k][self.out_off[i]:self.out_off[i] + _cap(self.items[i].text.size)]

    def result(self, i, k=0):
        j = 48 * (k * len(self.items) + i)
        return self.res[j:j + b64.RES_BYTES]

    def check(self, infos, hold, k=0, label=""):
        """Bytes and guards of output arena k against the oracle, the input
        arena unchanged; infos[i] is text i's record, already checked."""
        host = self.outs[k].cpu().numpy()
        free = np.ones(host.size, bool)
        for i, it in enumerate(self.items):
            what = f"{it.name}, {label}, hold {hold}"
            oo, cap = self.out_off[i], _cap(it.text.size)
            check_bytes(host[oo:oo + cap], infos[i].out_len, it.ref, what)
            assert (host[oo - GUARD:oo] == SENT).all(), f"the guard before was written; {what}"
            assert (host[oo + cap:oo + cap + GUARD] == SENT).all(), \
                f"the guard after was written; {what}"
            free[oo:oo + cap] = False
        assert (host[free] == SENT).all(), f"bytes outside every capacity were written; {label}"


def _ws_for(items):
    ws = torch.zeros(b64.workspace_size(max(it.text.size for it in items)), dtype=torch.uint8,
                     device=DEV)
    _KEEP.append(ws)
    return ws


def run_group(items, route, hold, abc=DEFAULT, again=True, starts=None):
    """Decode every text of the group by `route` (module docstring) and check
    bytes, records and guards.  auto: also the same call again (`again`), and
    the workspace's sfx_start after the first call into `starts`."""
    flags = b64.HOLD_TAIL if hold else 0
    auto = route == "auto"
    ar = Arena(items, outputs=2 if auto and again else 1)
    ws = _ws_for(items)
    lib = util.hooks() if route in (3, 8) else _lib.load()
    tiny = ar.x[GUARD // 2:GUARD // 2 + 5]  # five 'Q': a call of another length
    tiny_out = torch.empty(16, dtype=torch.uint8, device=DEV)
    tiny_res = torch.zeros(48, dtype=torch.uint8, device=DEV)
    old = lib.b64x__test_range_chunks(route) if route in (3, 8) else None
    infos = [[], []]
    try:
        for i, it in enumerate(items):
            n = it.text.size
            what = f"{it.name}, route {route}, hold {hold}"
            if auto:
                # nothing held for this length on the workspace, and the
                # workspace as a caller first hands it over
                _decode(lib, tiny, 5, tiny_out, tiny_res, abc, 0, ws).info()
                ws.zero_()
            torch.cuda.synchronize()
            before = _paths(lib)
            d = _decode(lib, ar.text(i), n, ar.out(i), ar.result(i), abc,
                        flags | (b64.EXPECT_JUNK if route == "junk" else 0), ws)
            info = d.info()  # waits: the hint is written by the device
            took = [a - b for a, b in zip(_paths(lib), before)]
            if auto and again:
                assert took == [1, 0, 0, 0, 0], (took, what)
            elif auto:
                assert took[HINT] == 0 and took[PROBE] + took[HELD] == 1, (took, what)
            else:
                assert took == [0] * 5, (took, what)
            check_record(info, it.ref, n, hold, what)
            infos[0].append(info)
            if starts is not None:
                starts.append(_sfx_start(ws))
            if auto and again:
                # junk in the text's first 16 bytes: the probe cut at slot 0,
                # and the suffix decode took the whole text
                assert sc.JUNK in it.text[:16] and _sfx_start(ws) == 0, what
                before = _paths(lib)
                d = _decode(lib, ar.text(i), n, ar.out(i, 1), ar.result(i, 1), abc, flags, ws)
                info = d.info()
                took = [a - b for a, b in zip(_paths(lib), before)]
                assert took == [1, 0, 1, 0, 0], (took, what + ", again")
                check_record(info, it.ref, n, hold, what + ", again")
                infos[1].append(info)
    finally:
        if old is not None:
            lib.b64x__test_range_chunks(old)
    ar.check(infos[0], hold, 0, f"route {route}")
    if auto and again:
        ar.check(infos[1], hold, 1, "route auto, again")
    assert torch.equal(ar.x.cpu(), torch.from_numpy(_host_arena(ar))), "the input arena was written"


def _host_arena(ar):
    host = np.full(ar.x.numel(), ord("Q"), np.uint8)
    for it, io in zip(ar.items, ar.in_off):
        host[io:io + it.text.size] = it.text
    return host


# ---- 2. single buffer, every route -------------------------------------------------

ROUTES = ["auto", "junk", 3, 8]


def _R(route):
    return 1024 * route if route in (3, 8) else 2048


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_sparse_corpus(route, hold):
    """The whole corpus, aligned: every(g, phase) and islands(a, j) at the
    four lengths."""
    run_group(corpus_items(_R(route)), route, hold)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_sparse_alignments(route, hold):
    """The thirteen `every` texts with input and output at 1 modulo 16 (the
    per-lane loads instead of the copy to LDS, the window placed for an
    output that is not 16-aligned)."""
    run_group(edge_items(_R(route))[0], route, hold)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("route", ROUTES)
def test_sparse_alphabet_of_separators(route, hold):
    """The thirteen `every` texts under the alphabet whose 62 and 63 are LF
    and CR."""
    run_group(edge_items(_R(route))[1], route, hold, abc=NL_CR)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("route", ["auto", "junk"])
def test_sparse_across_a_group_sum(route, hold):
    """Three texts of 65 tiles and 37 characters."""
    run_group(group_items(), route, hold)


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
def test_sparse_through_a_session(hold):
    """Four corpus texts through Session.decode, whose record the kernels
    mirror into host memory."""
    R = 2048
    n0 = sc.base_len(R)
    texts = [("every(2,0)", sc.every(2, 0, n0)), ("every(R+1,0)", sc.every(R + 1, 0, n0 + 1)),
             ("islands(1,R-1)", sc.islands(1, R - 1, n0 + 2)),
             ("islands(3,63)", sc.islands(3, 63, n0 + 3))]
    with Session(n0 + 3) as s:
        for name, t in texts:
            ref = reference(t)
            s.host_in[:t.size] = t
            s.host_out[:_cap(t.size)] = SENT
            info = s.decode(t.size, DEFAULT + (True, -1), b64.HOLD_TAIL if hold else 0)
            what = f"{name}, session, hold {hold}"
            check_record(info, ref, t.size, hold, what)
            check_bytes(np.array(s.host_out[:_cap(t.size)]), info.out_len, ref, what)


# ---- 3. scan tiles on the three-kernel route -----------------------------------------

@functools.lru_cache(maxsize=None)
def scan_items():
    """Two scan tiles (1,024 ranges each), three ranges and 37 characters
    at 3 chunks to the range."""
    R = 3072
    n = 2 * 1024 * R + 3 * R + 37
    assert n == 6_300_709
    rng = np.random.default_rng(61)
    chars = orc.encode(rng.integers(0, 256, n * 3 // 4, dtype=np.uint8))
    dense = np.frombuffer(_junk(rng, chars, 0.3)[:n], np.uint8).copy()
    mixed = sc.islands(1, R - 1, n)
    mixed[:500 * R] = np.frombuffer(chars[:500 * R], np.uint8)
    assert dense.size == n
    return _items([("clean + 0.3 junk", dense), ("every(2)", sc.every(2, 0, n)),
                   ("every(3073)", sc.every(R + 1, 0, n)),
                   ("500 clean ranges + islands(1,3071)", mixed)])


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
def test_scan_tiles(hold):
    """Texts that cross two edges of k_decode_scan2's tiles: the look-back
    between tiles runs, once from a first dirty range in mid-tile."""
    run_group(scan_items(), 3, hold)


# ---- 4. the hand-off position, exactly ------------------------------------------------

HAND_N = 2 * sc.TILE * 2048 + 3 * 2048 + 37
HAND_P = sorted({U + d for U in (2048, 4096, 32768, 65536) for d in (-17, -16, -1, 0, 1, 15, 16)} |
                {HAND_N - 40, HAND_N - 100})
FIRST_WINDOW_P = [0, 15, 16, 255]
CRLF76 = (76, 2)


def _F(p, fmt):
    if fmt is None:
        return p
    L, P = fmt[0], fmt[0] + fmt[1]
    return p // P * L + min(p % P, L)


def _pos(i, fmt):
    if fmt is None:
        return i
    L, P = fmt[0], fmt[0] + fmt[1]
    return i // L * P + i % L


def _interior_slots(n, fmt):
    """T as k_decode_probe derives it: the slots whose spans lie wholly
    inside the input."""
    if fmt is None:
        return n // 16
    L, P = fmt[0], fmt[0] + fmt[1]
    T = _F(n, fmt) // 16
    if T and 16 * T % L == 0 and 16 * T // L * P > n:
        T -= 1
    return T


def expected_start(p, n, fmt):
    """Where the suffix decode starts when the byte at p breaks the model of
    a text of n bytes: the start of the slot holding model position F(p), or
    nothing to do when that slot is not interior (the tail's owner decodes it
    exactly)."""
    slot = _F(p, fmt) // 16
    return _pos(16 * slot, fmt) if slot < _interior_slots(n, fmt) else NONE


@functools.lru_cache(maxsize=None)
def handoff_items():
    """[(Item, p, expected sfx_start or None)]: clean and CRLF-76 text of
    HAND_N bytes with '*' in place of, or in front of, the line character at
    p."""
    rng = np.random.default_rng(67)
    n = HAND_N
    assert n < 1 << 18  # the probe takes no samples: only the first window decides the model
    clean = np.frombuffer(orc.encode(rng.integers(0, 256, n, dtype=np.uint8))[:n], np.uint8)
    lines, rest = divmod(n, 78)
    assert rest > 2
    chars = orc.encode(rng.integers(0, 256, n, dtype=np.uint8))[:lines * 76 + rest - 2]
    mime = np.frombuffer(_wrap(chars, 76, b"\r\n"), np.uint8)
    assert clean.size == mime.size == n and bytes(mime[-2:]) == b"\r\n"
    out = []
    for label, base, fmt in (("clean", clean, None), ("crlf76", mime, CRLF76)):
        for p0 in HAND_P + FIRST_WINDOW_P:
            p = p0
            if fmt is not None and p % 78 >= 76:  # to the nearest line character
                p = p - 1 if p % 78 == 76 else p + 1
            assert base[p] not in b"\r\n"
            for kind in ("replaced", "inserted"):
                t = base.copy()
                if kind == "replaced":
                    t[p] = sc.JUNK
                else:
                    t = np.insert(t, p, sc.JUNK)
                exp = None if p0 in FIRST_WINDOW_P else expected_start(p, t.size, fmt)
                out.append((f"{label}, {kind} at {p}", t, p, exp))
    items = _items([(name, t) for name, t, _, _ in out])
    return [(it, p, exp) for it, (_, _, p, exp) in zip(items, out)]


def test_handoff_cases_are_interior():
    """The table itself (no GPU): every position past the first window lies
    in an interior slot of its text, so each case names a start."""
    cases = handoff_items()
    assert len(cases) == 2 * 2 * (len(HAND_P) + 4) and len(HAND_P) == 30
    for it, p, exp in cases:
        assert it.text[p] == sc.JUNK and (it.text == sc.JUNK).sum() == 1
        if p > 255:
            assert exp is not None and exp != NONE and 0 <= p - exp < 16 + 2, it.name
    assert expected_start(HAND_N - 3, HAND_N, None) == NONE
    assert expected_start(HAND_N - 3, HAND_N, CRLF76) == NONE


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [False, True])
def test_handoff_position(hold):
    """One junk byte in clean and in CRLF-76 text: k_decode_lines keeps every
    slot before the one that holds it, and the suffix decode starts exactly
    at that slot's first character (the workspace's sfx_start)."""
    cases = handoff_items()
    starts = []
    run_group([it for it, _, _ in cases], "auto", hold, again=False, starts=starts)
    for (it, p, exp), got in zip(cases, starts):
        if exp is None:
            assert got <= p and got % 16 == 0, (it.name, got)
        else:
            assert got == exp, (it.name, got, exp)


# ---- 5. batches ---------------------------------------------------------------------------

ROW_LEN = 4133


@functools.lru_cache(maxsize=None)
def batch_rows(sparse_first):
    """The corpus at row length 4,133 as the rows of one batch, between a
    first row that is clean or sparse (it sets the model) and a clean last
    row (dd.run_case's)."""
    rng = np.random.default_rng(71)
    clean = dd.alphabet_chars(dd.DEFAULT)[rng.integers(0, 64, (2, ROW_LEN))]
    rows = [t for _, t in sc.corpus(2048, ns=[ROW_LEN])]
    first = sc.islands(3, 61, ROW_LEN, seed=1) if sparse_first else clean[0]
    rows = np.stack([first] + rows + [clean[1]])
    wants = dd.oracle_rows(rows, dd.DEFAULT)
    rows.setflags(write=False)
    return rows, wants


@pytest.mark.gpu
@pytest.mark.parametrize("sparse_first", [False, True])
@pytest.mark.parametrize("route", ["rows", "slots"])
def test_sparse_rows(route, sparse_first):
    """b64x_decode_strided of the sparse rows: the rows trio (bases and
    strides 4-aligned, whole 12-byte slots per row), every row but a clean
    one failing its model and going to k_rows_finish, and k_decode_slots
    with the fix-up (the input base at 1 modulo 4)."""
    rows, wants = batch_rows(sparse_first)
    S = (ROW_LEN + 15) // 16
    if route == "rows":
        dd.run_case(rows, None, dd.DEFAULT, dd.up4(ROW_LEN), 12 * S, "rows", o32=True,
                    wants=wants)
    else:
        dd.run_case(rows, None, dd.DEFAULT, dd.up4(ROW_LEN), 12 * S, "slots", why="alignment",
                    in_mod=1, wants=wants)


RAGGED_LENS = (0, 37, 1029, 2048, 2049, 4133, 8229)


@functools.lru_cache(maxsize=None)
def ragged_items():
    texts = sc.corpus(2048, ns=[sc.base_len(2048)])
    return _items([(f"{name}[:{m}]", t[:m].copy()) for name, t in texts for m in RAGGED_LENS])


@pytest.mark.gpu
def test_sparse_ragged_batch():
    """b64x_decode_batch of the corpus texts cut to seven lengths and laid
    end to end (starts at every alignment modulo 16), 64 guard bytes between
    the outputs: d_outlen and bytes against the oracle."""
    items = ragged_items()
    lens = np.array([it.text.size for it in items], np.int64)
    in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert set((in_off[:-1] % 16).tolist()) == set(range(16))
    caps = np.array([_cap(int(m)) for m in lens], np.int64)
    out_off = (np.concatenate([[0], np.cumsum(caps + GUARD)[:-1]]) + GUARD).astype(np.int64)
    x = torch.from_numpy(np.concatenate([it.text for it in items] + [np.full(GUARD, ord("Q"),
                                                                             np.uint8)])).to(DEV)
    out = torch.full((int(out_off[-1] + caps[-1]) + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    outlen = torch.full((len(items),), -1, dtype=torch.int64, device=DEV)
    b64.decode_batch(x, torch.from_numpy(in_off).to(DEV), out, torch.from_numpy(out_off).to(DEV),
                     outlen)
    torch.cuda.synchronize()
    got_len = outlen.cpu().numpy()
    host = out.cpu().numpy()
    free = np.ones(host.size, bool)
    for i, it in enumerate(items):
        assert got_len[i] == it.ref.want.size, (it.name, got_len[i], it.ref.want.size)
        oo = int(out_off[i])
        check_bytes(host[oo:oo + caps[i]], it.ref.want.size, it.ref, it.name)
        free[oo:oo + caps[i]] = False
    assert (host[free] == SENT).all(), "bytes outside every capacity were written"
