"""The ragged batch kernels at their production shape: tens of thousands of
small buffers in one batch, so that every persistent wave of
k_decode_batch_fast walks several buffers (the hand-over: pos, V, ok,
aligned, beg/len/obeg reset or swapped; the reload after a buffer was
abandoned early; next buffers that are empty, skipped or aligned differently)
and k_batch_finish's `j += nw` loop runs.  Every comparison is bit for bit
against the oracle (orc.decode / orc.encode / orc.decode_table); outputs sit
in one arena with 0-7 sentinel bytes after each buffer's capacity, compared
whole, so a store past a buffer's end is seen wherever it lands."""
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from async_amd import _lib, b64
from oracle import pyoracle as orc
from tests.test_decode_fuzz import JUNK

DEV = "cuda:0"
SEED = 0xB64
# A CU holds at most 2,048 threads, so at most 8 blocks of 256; that gives at
# most 256 CUs x 8 blocks x 4 waves = 8,192 resident waves on this part.
# 4 x 8,192 + 5 buffers therefore make every wave of the persistent grid
# (min(ceil(nbuf / 4), cus x occupancy) blocks of 4 waves) walk at least 4
# buffers, whatever the occupancy query returns, and the odd tail gives the
# last waves a different count.  (Measured with a kernel trace on a 256-CU
# MI355X: k_decode_batch_fast runs 1,024 blocks, so a wave walks 8 buffers.)
NBUF = 4 * 8192 + 5
SENT = 0x5A  # 'Z': occurs in decoded data too; gaps are compared whole
KINDS = "abcdefghij"
FORCED_SMALL = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65)
FORCED_MID = (1023, 1024, 1025, 2047, 2048, 2049)
CHUNK = 1024  # characters per chunk; the fast kernel takes two (a pair) per step
HOLD, CHAINED = 1, 4  # B64X_DEC_HOLD_TAIL, B64X_LANE_CHAINED
BIG = 128 << 10  # lane jobs this long take the single-buffer pipeline

DEC_ABCS = [(-1, -1), ("-", "_"), ("\n", "\r"), ("!", "=")]
DEC_IDS = ["default", "url", "nl-cr", "bang-eq"]
ENC_ABCS = [(-1, -1, True, -1), (-1, -1, False, -1), (".", "_", True, "-"),
            (0xE9, 0xE8, True, 0x80)]
ENC_IDS = ["default", "nopad", "dot-dash", "high"]


def decoded_cap(n):
    """b64x_decoded_cap, vectorised: 3 * ceil(n / 4)."""
    return (n + 3) // 4 * 3


class Alphabet:
    """What the corpus needs of one decode alphabet: the oracle's table,
    which bytes count, the JUNK bytes that are junk under it and a pool of
    clean characters to cut texts from."""

    def __init__(self, pos62, pos63):
        self.abc = (pos62, pos63)
        self.tab = np.array(orc.decode_table(pos62, pos63), dtype=np.int16)
        self.is_alpha = (self.tab >= 0) & (self.tab < 64)
        junk = np.frombuffer(b"".join(JUNK), dtype=np.uint8)
        self.junk = junk[~self.is_alpha[junk]]
        raw = np.random.default_rng(62 * 256 + 63).integers(0, 256, 3 << 19, dtype=np.uint8)
        self.pool = orc.encode(raw, pos62, pos63, as_array=True)  # 2 Mi characters, no padding
        assert self.junk.size >= 4 and self.is_alpha[self.pool].all()

    def clean(self, rng, n):
        """n clean characters starting on a group boundary (a copy)."""
        off = 4 * int(rng.integers(0, (self.pool.size - n) // 4 + 1))
        return self.pool[off:off + n].copy()

    def junk_run(self, rng, n):
        return self.junk[rng.integers(0, self.junk.size, n)]


@functools.lru_cache(maxsize=None)
def alphabet(pos62, pos63) -> Alphabet:
    return Alphabet(pos62, pos63)


@dataclass
class Corpus:
    abc: tuple
    kinds: np.ndarray      # per buffer, an index into KINDS
    second_pair: np.ndarray  # kind (e) with junk in the second pair only
    data: np.ndarray       # the texts back to back
    in_off: np.ndarray     # nbuf + 1, tight
    out_off: np.ndarray    # nbuf + 1: capacity plus a gap of 0-7 after each buffer
    caps: np.ndarray
    valid: np.ndarray      # alphabet characters per buffer (orc.decode_table)
    want: np.ndarray       # orc.decode of every text, back to back
    want_off: np.ndarray   # nbuf + 1
    expect: np.ndarray     # the output arena: wants in place, sentinel elsewhere
    mask: np.ndarray       # arena bytes that are constrained (wants and gaps)

    @property
    def nbuf(self):
        return self.kinds.size

    @property
    def lens(self):
        return np.diff(self.in_off)

    @property
    def want_len(self):
        return np.diff(self.want_off)

    def text(self, i):
        return self.data[self.in_off[i]:self.in_off[i + 1]]

    def wanted(self, i):
        return self.want[self.want_off[i]:self.want_off[i + 1]]


def _text_of_kind(A: Alphabet, rng, kind: str, n: int, second_pair: bool) -> np.ndarray:
    """One text of about n characters (exactly n for kinds c-i)."""
    if kind == "j" or (n == 0 and kind not in "ab"):
        return np.zeros(0, np.uint8)
    if kind == "a":  # clean and padded: whole groups, the last with 0-2 pad characters
        n = max(n // 4 * 4, 4)
        r = int(rng.integers(0, 3))
        t = A.clean(rng, n)
        t[n - r:] = ord("=")
        return t
    if kind == "b":  # clean and cut inside a group
        return A.clean(rng, n // 4 * 4 + int(rng.integers(1, 4)))
    t = A.clean(rng, n)
    if kind == "c":  # junk only in the last 16 characters
        w = min(16, n)
        k = int(rng.integers(1, w + 1))
        t[n - w + rng.choice(w, k, replace=False)] = A.junk_run(rng, k)
    elif kind == "d":  # junk only in the last chunk
        lo = (n - 1) // CHUNK * CHUNK
        k = min(int(rng.integers(1, 9)), n - lo)
        t[lo + rng.choice(n - lo, k, replace=False)] = A.junk_run(rng, k)
    elif kind == "e":  # junk before the last pair: the buffer is abandoned early
        lo = 2 * CHUNK if second_pair else 0
        hi = 4 * CHUNK if second_pair else CHUNK
        assert n > hi
        k = int(rng.integers(1, 4))
        t[lo + rng.choice(hi - lo, k, replace=False)] = A.junk_run(rng, k)
    elif kind == "f":  # all junk
        t = A.junk_run(rng, n)
    elif kind == "g":  # '=' in the middle
        t[n // 2] = ord("=")
    elif kind == "h":  # CRLF-76 lines
        col = np.arange(n) % 78
        t[col == 76] = 13
        t[col == 77] = 10
    elif kind == "i":  # an alphabet prefix, then junk to the end (fast_prefix's shape)
        run = int(min(n, rng.integers(1, 41) if rng.random() < 0.8 else rng.integers(1, n + 1)))
        t[n - run:] = A.junk_run(rng, run)
    return t


def _layout(lens: np.ndarray, caps: np.ndarray, rng):
    in_off = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=in_off[1:])
    out_off = np.zeros(lens.size + 1, np.int64)
    np.cumsum(caps + rng.integers(0, 8, lens.size), out=out_off[1:])
    return in_off, out_off


def _arena(out_off: np.ndarray, caps: np.ndarray, wants: list):
    """(want, want_off, expect, mask) for outputs `wants` at out_off: expect
    holds each want at its offset and the sentinel elsewhere; mask is false
    on [out_off_i + len(want_i), out_off_i + cap_i), a buffer's own spare
    capacity, and true on the wants and the gaps."""
    n = len(wants)
    wl = np.fromiter((w.size for w in wants), np.int64, n)
    want_off = np.zeros(n + 1, np.int64)
    np.cumsum(wl, out=want_off[1:])
    want = np.concatenate(wants) if n else np.zeros(0, np.uint8)
    assert (wl <= caps).all()
    size = int(out_off[-1])
    expect = np.full(size, SENT, np.uint8)
    expect[np.repeat(out_off[:-1] - want_off[:-1], wl) + np.arange(want.size)] = want
    d = np.zeros(size + 1, np.int32)
    np.add.at(d, out_off[:-1] + wl, -1)
    np.add.at(d, out_off[:-1] + caps, 1)
    mask = np.cumsum(d[:-1]) == 0
    return want, want_off, expect, mask


@functools.lru_cache(maxsize=None)
def ragged_corpus(seed: int, nbuf: int, abc: tuple) -> Corpus:
    """nbuf texts for one ragged decode batch under alphabet abc = (pos62,
    pos63), their tight input offsets, output offsets (capacity plus a gap of
    0-7 bytes after each buffer, so input alignment, output skew and the
    kernel's `aligned` change from one buffer to the next) and the oracle's
    expectation as one arena (see _arena).  Plain numpy; the same seed gives
    the same corpus.

    nbuf is NBUF = 32,773 in the tests: a CU holds at most 2,048 threads, so
    at most 8 blocks of 256; at most 256 CUs x 8 blocks x 4 waves = 8,192
    waves are resident, and 4 x 8,192 + 5 buffers make every wave walk at
    least 4 buffers whatever the occupancy query returns, the odd tail giving
    the last waves a different count.

    Lengths: about 74 % 0-200 characters, 16 % 900-2,200, 10 % 2,049-7,000
    (two to four pairs), the FORCED_* lengths planted; the middle class is
    smaller than a fifth to keep the total under 32 MB.  The kind (KINDS, a-j
    as in _text_of_kind) is drawn independently of the length, except that
    (e) draws its own length past one pair (past two when the junk is in the
    second pair only) and (j) is empty."""
    A = alphabet(*abc)
    rng = np.random.default_rng(seed)
    share = np.full(len(KINDS), (1 - 0.045 - 0.03) / 8)
    share[KINDS.index("e")] = 0.045
    share[KINDS.index("j")] = 0.03
    kinds = rng.choice(len(KINDS), nbuf, p=share)
    cls = rng.choice(3, nbuf, p=[0.74, 0.16, 0.10])
    target = np.where(cls == 0, rng.integers(0, 201, nbuf),
                      np.where(cls == 1, rng.integers(900, 2201, nbuf),
                               rng.integers(2049, 7001, nbuf)))
    is_e = kinds == KINDS.index("e")
    second_pair = is_e & (rng.random(nbuf) < 0.3)
    target = np.where(is_e, rng.integers(2049, 4501, nbuf), target)
    target = np.where(second_pair, rng.integers(4097, 7001, nbuf), target)
    # the forced lengths, three times each, on kinds that keep the length
    exact = np.flatnonzero(np.isin(kinds, [KINDS.index(k) for k in "cdfgi"]))
    forced = np.repeat(FORCED_SMALL + FORCED_MID, 3)
    target[rng.choice(exact, forced.size, replace=False)] = forced
    texts = [_text_of_kind(A, rng, KINDS[k], int(n), bool(s))
             for k, n, s in zip(kinds, target, second_pair)]
    lens = np.fromiter((t.size for t in texts), np.int64, nbuf)
    caps = decoded_cap(lens)
    in_off, out_off = _layout(lens, caps, rng)
    data = np.concatenate(texts)
    wants = [orc.decode(t, abc[0], abc[1], as_array=True) for t in texts]
    want, want_off, expect, mask = _arena(out_off, caps, wants)
    cnt = np.zeros(data.size + 1, np.int32)
    np.cumsum(A.is_alpha[data], out=cnt[1:])
    valid = (cnt[in_off[1:]] - cnt[in_off[:-1]]).astype(np.int64)
    return Corpus(abc, kinds, second_pair, data, in_off, out_off, caps, valid, want, want_off,
                  expect, mask)


def test_ragged_corpus_covers_the_hand_over_cases():
    """Conditions on the inputs alone (no GPU), so that the GPU tests below
    cannot pass on a corpus that misses what they are for."""
    for abc in DEC_ABCS:
        c = ragged_corpus(SEED, NBUF, abc)
        assert c.nbuf == NBUF == 32773
        lens = c.lens
        count = np.bincount(c.kinds, minlength=len(KINDS))
        assert (count >= 500).all(), count
        e = c.kinds == KINDS.index("e")
        assert e.sum() >= 1000 and c.second_pair.sum() >= 100
        assert (lens[e] > 2 * CHUNK).all() and (lens[c.second_pair] > 4 * CHUNK).all()
        A = alphabet(*abc)
        for i in np.flatnonzero(e):  # the junk sits where the kind says, and only there
            bad = np.flatnonzero(~A.is_alpha[c.text(i)])
            lo, hi = (2 * CHUNK, 4 * CHUNK) if c.second_pair[i] else (0, CHUNK)
            assert bad.size and lo <= bad[0] and bad[-1] < hi, i
        assert (lens[c.kinds == KINDS.index("j")] == 0).all()
        assert not A.is_alpha[c.data[np.repeat(c.kinds == KINDS.index("f"), lens)]].any()
        assert set(FORCED_SMALL + FORCED_MID) <= set(lens.tolist())
        pairs = set(zip(c.kinds[:-1024].tolist(), c.kinds[1024:].tolist()))
        assert len(pairs) == len(KINDS) ** 2
        for k in "ea":
            sel = c.kinds == KINDS.index(k)
            skews = set(zip((c.in_off[:-1][sel] % 4).tolist(), (c.out_off[:-1][sel] % 4).tolist()))
            assert len(skews) == 16, (k, skews)
        assert (np.bincount(c.valid % 4, minlength=4)[1:] >= 300).all()
        assert c.data.size <= 32_000_000
        # the expectation arena: every gap constrained, every want in place
        gaps = c.out_off[1:] - c.out_off[:-1] - c.caps
        assert gaps.min() == 0 and gaps.max() == 7
        assert int(c.mask.sum()) == int(c.want.size + gaps.sum())
        i = int(np.argmax(lens))
        assert c.expect[c.out_off[i]:c.out_off[i] + c.want_len[i]].tobytes() == \
            orc.decode(c.text(i).tobytes(), abc[0], abc[1])


def _first_bad(got, ol, off, caps, wants_of, what):
    """Walk the buffers (only on a mismatch) and name the first bad one."""
    for i in range(len(ol)):
        w = wants_of(i)
        o = int(off[i])
        if ol[i] != w.size:
            return f"buffer {i} ({what(i)}): length {ol[i]}, oracle {w.size}"
        if not np.array_equal(got[o:o + w.size], w):
            k = int(np.flatnonzero(got[o:o + w.size] != w)[0])
            return f"buffer {i} ({what(i)}): byte {k} of {w.size} differs"
        if (got[o + int(caps[i]):int(off[i + 1])] != SENT).any():
            return f"buffer {i} ({what(i)}): the gap after its capacity was written"
    return None


def _check_decode(c: Corpus, got: np.ndarray, ol: np.ndarray):
    if np.array_equal(ol, c.want_len) and not ((got != c.expect) & c.mask).any():
        return
    bad = _first_bad(got, ol, c.out_off, c.caps, c.wanted, lambda i: (
        f"kind {KINDS[c.kinds[i]]}, {c.lens[i]} characters, in_off {c.in_off[i]}, "
        f"out_off {c.out_off[i]}"))
    pytest.fail(bad or "arena mismatch outside every buffer")


@pytest.mark.gpu
@pytest.mark.parametrize("abc", DEC_ABCS, ids=DEC_IDS)
def test_ragged_decode_many_buffers_vs_oracle(abc):
    """One decode_batch call over the 32,773-buffer corpus: every length and
    the whole output arena (decoded bytes and the gaps between capacities)
    exact; then once more on another stream with outlen full of ~0, the
    fix-up's own marker."""
    c = ragged_corpus(SEED, NBUF, abc)
    assert b64.decoded_cap(int(c.lens.max())) == int(c.caps.max())
    x = torch.from_numpy(c.data).to(DEV)
    in_off = torch.from_numpy(c.in_off).to(DEV)
    out_off = torch.from_numpy(c.out_off).to(DEV)
    for stream, fill in ((None, 0), (torch.cuda.Stream(), -1)):
        out = torch.full((c.expect.size,), SENT, dtype=torch.uint8, device=DEV)
        outlen = torch.full((c.nbuf,), fill, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        b64.decode_batch(x, in_off, out, out_off, outlen, abc=(abc[0], abc[1], True, -1),
                         stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        _check_decode(c, out.cpu().numpy(), outlen.cpu().numpy())


@pytest.mark.gpu
def test_ragged_fixup_unaligned_output_few_characters():
    """The exact fix-up (decode_buf_bits) flushes whole dwords after every
    2,048 characters.  With an unaligned output and fewer alphabet characters
    so far than reach the output's first whole dword there is nothing to
    flush yet: buffers longer than one pair whose first pair (or first two)
    holds 0-5 alphabet characters, at every output skew, each followed by a
    gap that must stay untouched."""
    A = alphabet(-1, -1)
    rng = np.random.default_rng(SEED + 3)
    texts = []
    for skew in range(4):
        for few in range(6):
            for junk_pairs in (1, 2):
                for rest in (1, 700, 2048, 2500):
                    t = A.junk_run(rng, 2 * CHUNK * junk_pairs)
                    t[rng.choice(t.size, few, replace=False)] = A.clean(rng, few)
                    texts.append((skew, np.concatenate([t, A.clean(rng, rest)])))
    lens = np.array([t.size for _, t in texts])
    caps = decoded_cap(lens)
    in_off, out_off = _layout(lens, caps, rng)
    # place buffer i at skew s_i: shift every later offset by what that takes
    shift = 0
    for i, (s, _) in enumerate(texts):
        shift += (s - (out_off[i] + shift)) % 4
        out_off[i] += shift
    out_off[-1] += shift + 8
    assert [int(o) % 4 for o in out_off[:-1]] == [s for s, _ in texts]
    assert (out_off[1:] - out_off[:-1] >= caps).all()
    wants = [orc.decode(t, as_array=True) for _, t in texts]
    _, _, expect, mask = _arena(out_off, caps, wants)
    out = torch.full((expect.size,), SENT, dtype=torch.uint8, device=DEV)
    outlen = torch.zeros(lens.size, dtype=torch.int64, device=DEV)
    b64.decode_batch(torch.from_numpy(np.concatenate([t for _, t in texts])).to(DEV),
                     torch.from_numpy(in_off).to(DEV), out, torch.from_numpy(out_off).to(DEV),
                     outlen)
    got, ol = out.cpu().numpy(), outlen.cpu().numpy()
    if not np.array_equal(ol, [w.size for w in wants]) or ((got != expect) & mask).any():
        pytest.fail(_first_bad(got, ol, out_off, caps, lambda i: wants[i], lambda i: (
            f"{lens[i]} characters, out_off {out_off[i]}")))


@pytest.mark.gpu
@pytest.mark.parametrize("abc", ENC_ABCS, ids=ENC_IDS)
def test_ragged_encode_many_buffers_vs_oracle(abc):
    """encode_batch over 32,773 buffers of 0-300 bytes and a few long ones,
    0-7 sentinel bytes after each output: the whole arena exact."""
    rng = np.random.default_rng(SEED + 1)
    lens = rng.integers(0, 301, NBUF)
    longs = np.array([3000, 4097, 12345, 33333, 65536, 70000])
    lens[rng.choice(NBUF, longs.size, replace=False)] = longs
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    elen = (lens + 2) // 3 * 4 if abc[2] else (4 * lens + 2) // 3
    assert all(b64.encoded_len(int(n), abc[2]) == int(m) for n, m in zip(lens[:400], elen[:400]))
    in_off, out_off = _layout(lens, elen, rng)
    wants = [orc.encode(data[in_off[i]:in_off[i + 1]], *abc, as_array=True) for i in range(NBUF)]
    _, _, expect, mask = _arena(out_off, elen, wants)
    assert mask.all()  # every byte is an encoded character or a gap
    out = torch.full((expect.size,), SENT, dtype=torch.uint8, device=DEV)
    b64.encode_batch(torch.from_numpy(data).to(DEV), torch.from_numpy(in_off).to(DEV), out,
                     torch.from_numpy(out_off).to(DEV), abc=abc)
    got = out.cpu().numpy()
    if not np.array_equal(got, expect):
        pytest.fail(_first_bad(got, elen, out_off, elen, lambda i: wants[i],
                               lambda i: f"{lens[i]} bytes, out_off {out_off[i]}"))


# ---- the lane entry point (RV = true, k_batch_finish) ---------------------

RECORD = np.dtype([("out_len", "<u8"), ("valid", "<u8"), ("tail_n", "<u4"), ("tail", "u1", 4),
                   ("nchars", "<u8"), ("seq", "<u4"), ("flags", "<u4")])
assert RECORD.itemsize == _lib.RES_BYTES


def _hold_shapes(A: Alphabet, rng) -> list:
    """HOLD jobs aimed at k_batch_finish's backward search in 64-byte
    windows for the last V mod 4 alphabet characters."""
    cat = np.concatenate
    out = []
    for r in (1, 2, 3):
        for trail in (0, 63, 64, 65, 200):  # the tail, then junk up to past three windows
            for body in (0, 4 * int(rng.integers(1, 600))):
                out.append(cat([A.clean(rng, body + r), A.junk_run(rng, trail)]))
        # the needed characters on both sides of a window edge
        parts = []
        for k in range(r - 1):
            parts += [A.clean(rng, 1), A.junk_run(rng, 70 - 3 * k)]
        parts += [A.clean(rng, 1), A.junk_run(rng, 3)]
        out.append(cat(parts))
        out.append(cat([A.clean(rng, 260)] + parts))
        out.append(cat([A.clean(rng, r - 1), A.junk_run(rng, 61), A.clean(rng, 1),
                        A.junk_run(rng, 64)]))
    out.append(A.junk_run(rng, 100))  # all junk
    out.append(np.zeros(0, np.uint8))  # length 0
    return out


def _lane_jobs(c: Corpus, rng):
    """(texts, flags, prev): the corpus with about a third of its jobs HOLD,
    and, merged in at random places, the HOLD shapes, two jobs past the 128
    KiB limit and sixteen chained pairs (A HOLD, B CHAINED later on, A's
    V mod 4 going through 0-3)."""
    A = alphabet(*c.abc)
    jobs = [(float(i), c.text(i), HOLD * int(h), -1)
            for i, h in enumerate(rng.random(c.nbuf) < 1 / 3)]
    place = lambda lo, hi: float(rng.uniform(lo, hi) * c.nbuf)  # noqa: E731
    for t in _hold_shapes(A, rng):
        jobs.append((place(0, 1), t, HOLD, -1))
    big = A.clean(rng, BIG + 8929)
    big[np.arange(big.size) % 78 >= 76] = A.junk[0]
    jobs.append((place(0.1, 0.9), A.clean(rng, BIG), 0, -1))
    jobs.append((place(0.1, 0.9), big, HOLD, -1))
    assert big.size == 140001
    for k in range(16):
        a = _text_of_kind(A, rng, "bcdgih"[k % 6], int(rng.integers(8, 2000)), False)
        a = np.concatenate([a, A.clean(rng, int(k - A.is_alpha[a].sum()) % 4)])  # V mod 4 = k mod 4
        assert A.is_alpha[a].sum() % 4 == k % 4
        b = np.concatenate([A.junk_run(rng, 4), _text_of_kind(A, rng, "abcdghi"[k % 7],
                                                               int(rng.integers(0, 3000)), False)])
        jobs.append((place(0, 0.5), a, HOLD, -1))
        jobs.append((place(0.5, 1), b, CHAINED, len(jobs) - 1))
    order = sorted(range(len(jobs)), key=lambda j: jobs[j][0])
    where = {j: p for p, j in enumerate(order)}
    texts = [jobs[j][1] for j in order]
    flags = np.array([jobs[j][2] for j in order], np.uint8)
    prev = np.array([where[jobs[j][3]] if jobs[j][3] >= 0 else -1 for j in order], np.int64)
    return texts, flags, prev


class _Pinned:
    """Arenas from b64x_host_alloc as numpy arrays; freed by close()."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def array(self, count, dtype):
        dtype = np.dtype(dtype)
        p = self.lib.b64x_host_alloc(max(count, 1) * dtype.itemsize)
        assert p, "b64x_host_alloc failed"
        self.ptrs.append(p)
        raw = (ctypes.c_uint8 * (max(count, 1) * dtype.itemsize)).from_address(p)
        return np.frombuffer(raw, dtype=dtype)[:count], p

    def close(self):
        for p in self.ptrs:
            self.lib.b64x_host_free(p)
        self.ptrs = []


def _lane_plan(abc):
    """The jobs of one lane batch, their layout and the oracle's expectation
    per job (plain numpy)."""
    c = ragged_corpus(SEED, NBUF, abc)
    A = alphabet(*abc)
    rng = np.random.default_rng(SEED + 2)
    texts, flags, prev = _lane_jobs(c, rng)
    n = len(texts)
    lens = np.fromiter((t.size for t in texts), np.int64, n)
    caps = decoded_cap(lens)
    in_off, out_off = _layout(lens, caps, rng)
    data = np.concatenate(texts)
    hold = (flags & HOLD) != 0
    chained = np.flatnonzero(flags & CHAINED)
    assert chained.size == 16 and (lens >= BIG).sum() == 2 and (prev[chained] < chained).all()
    assert sorted((A.is_alpha[texts[a]].sum() % 4 for a in prev[chained])) == sorted([0, 1, 2, 3] * 4)

    # the oracle's expectation per job
    cnt = np.zeros(data.size + 1, np.int32)
    np.cumsum(A.is_alpha[data], out=cnt[1:])
    valid = (cnt[in_off[1:]] - cnt[in_off[:-1]]).astype(np.int64)
    at = np.flatnonzero(A.is_alpha[data])  # where the alphabet characters are
    tails = np.zeros((n, 4), np.uint8)  # HOLD jobs: the sextets of the last V mod 4 of them
    for k in range(3):
        sel = np.flatnonzero(hold & (valid % 4 > k))
        tails[sel, k] = A.tab[data[at[cnt[in_off[sel + 1]] - valid[sel] % 4 + k]]]
    wants = [None] * n
    for b in chained:  # A's bytes followed by B's are the decode of text_A + text_B[4:]
        a = prev[b]
        assert not A.is_alpha[texts[b][:4]].any()
        both = orc.decode(np.concatenate([texts[a], texts[b][4:]]), *abc, as_array=True)
        wants[a], wants[b] = both[:valid[a] // 4 * 3], both[valid[a] // 4 * 3:]
        valid[b] += valid[a] % 4  # the spelled head counts
    out_len = np.where(hold, valid // 4 * 3, valid * 6 // 8)
    for j in range(n):
        if wants[j] is None:
            wants[j] = orc.decode(texts[j], *abc, as_array=True)[:out_len[j]]
    _, _, expect, mask = _arena(out_off, caps, wants)
    return (data, lens, caps, in_off, out_off, flags, prev, valid, tails, out_len, wants, expect,
            mask)


def _lane_batch(lib, lane, abc):
    (data, lens, caps, in_off, out_off, flags, prev, valid, tails, out_len, wants, expect,
     mask) = _lane_plan(abc)
    n = lens.size
    hold = (flags & HOLD) != 0
    chained = np.flatnonzero(flags & CHAINED)
    pin = _Pinned(lib)
    try:
        h_in, p_in = pin.array(data.size, np.uint8)
        h_out, p_out = pin.array(expect.size, np.uint8)
        h_in_off, p_in_off = pin.array(n + 1, np.uint64)
        h_out_off, p_out_off = pin.array(n + 1, np.uint64)
        h_flags, p_flags = pin.array(n, np.uint8)
        h_res, p_res = pin.array(n, RECORD)
        h_spell, p_spell = pin.array(n, RECORD)
        h_prev, p_prev = pin.array(n, np.uint64)
        h_in[:] = data
        h_out[:] = SENT
        h_in_off[:] = in_off
        h_out_off[:] = out_off
        h_flags[:] = flags
        h_prev[:] = 0
        h_prev[chained] = p_res + RECORD.itemsize * prev[chained]
        h_spell.view(np.uint8)[:] = 0
        seq = ctypes.c_uint32(0)
        abc_c = _lib.alphabet(abc[0], abc[1])
        rc = lib.b64x_lane_decode_async(lane, p_in, n, p_in_off, p_out, p_out_off, p_flags,
                                        p_res, p_prev, p_spell, ctypes.byref(abc_c), None, None,
                                        ctypes.byref(seq))
        assert rc == 0, rc
        assert lib.b64x_lane_wait(lane) == 0
        assert lib.b64x_lane_decode_check(lane, seq.value, p_in_off, p_flags, p_res, p_prev,
                                          p_spell, n) == 0
        res = h_res.copy()
        got = h_out.copy()
    finally:
        pin.close()

    def what(j):
        return (f"{lens[j]} characters, flags {flags[j]}, in_off {in_off[j]}, "
                f"out_off {out_off[j]}, alphabet {abc}")

    def first(bad):
        j = int(np.flatnonzero(bad)[0])
        return f"job {j} ({what(j)}): record {res[j]}"

    assert seq.value != 0
    named = (res["nchars"] == lens) & (res["seq"] == seq.value) & (res["flags"] == (flags & HOLD))
    assert named.all(), first(~named)
    assert (res["valid"] == valid).all(), first(res["valid"] != valid)
    assert (res["tail_n"] == valid % 4).all(), first(res["tail_n"] != valid % 4)
    bad_tail = hold & (res["tail"] != tails).any(axis=1)
    assert not bad_tail.any(), first(bad_tail) + f", oracle tail {tails[np.flatnonzero(bad_tail)[0]]}"
    assert (res["out_len"] == out_len).all(), first(res["out_len"] != out_len)
    if ((got != expect) & mask).any():
        pytest.fail(_first_bad(got, out_len, out_off, caps, lambda j: wants[j], what))


@pytest.mark.gpu
def test_lane_decode_many_jobs_vs_oracle():
    """The corpus as one lane decode batch (k_decode_batch_fast/fix2<true>,
    then k_batch_finish's records), a third of the jobs HOLD_TAIL, with jobs
    the batch kernels must skip (two past 128 KiB, sixteen chained) among
    them: every record, every output byte and every gap in the pinned arena
    against the oracle."""
    lib = _lib.load()
    torch.cuda.set_device(0)
    lane = lib.b64x_lane_open()
    assert lane, "b64x_lane_open failed"
    try:
        for abc in (DEC_ABCS[0], DEC_ABCS[2]):
            _lane_batch(lib, lane, abc)
    finally:
        lib.b64x_lane_close(lane)
