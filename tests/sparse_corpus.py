"""Alphabet-sparse texts for the lenient decoder's exact paths, and the
bookkeeping those paths have to get right, restated from the contract
(plain numpy; shared by tests/test_decode_sparse.py).

The exact decode cuts a stream into ranges of R characters.  With B alphabet
characters before a range, the 4-character group that is open at the range's
start is owned by an earlier range, which takes the range's first
k = (4 - B % 4) % 4 alphabet characters; the range owns the groups that begin
in it and completes its last one from the characters after its end, read in
windows of 64 bytes.  Dense text never has a range with fewer than k
characters, a window that holds some but not all of the characters a
completion needs, or a completion that runs to the end of the stream;
the texts here do:

    every(g, phase, n)   one alphabet character every g bytes (g = 2 and 4 at
                         phases 0 and 1: base64 inside UTF-16 and UTF-32 text
                         of either byte order)
    islands(a, j, n)     a alphabet characters, then j junk bytes, repeated

Every other byte is JUNK, which lies outside every tested alphabet.
range_stats() counts, for one text, the situations above; the self-check in
tests/test_decode_sparse.py asserts that the corpus reaches each of them."""
from __future__ import annotations

import numpy as np

JUNK = ord("*")  # in no tested alphabet, no separator, no pad character
WINDOW = 64      # bytes a completion (and the tail search) reads at a time
TILE = 16        # ranges per tile of the single pass

_STD = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def alphabet_chars(abc=(-1, -1)) -> np.ndarray:
    """The 64 characters of the alphabet whose positions 62 and 63 are abc
    (-1: the default's)."""
    a = np.frombuffer(_STD, np.uint8).copy()
    for k, c in ((62, abc[0]), (63, abc[1])):
        if c != -1:
            a[k] = ord(c) if isinstance(c, str) else int(c)
    assert JUNK not in a
    return a


def base_len(R: int, tiles: int = 3) -> int:
    """`tiles` tiles of the single pass, one range and a ragged end."""
    return tiles * TILE * R + R + 37


def lengths(R: int):
    """V mod 4 and the end of the stream move against the last range."""
    return [base_len(R) + d for d in range(4)]


def gaps(R: int):
    return [2, 4, 17, 33, 63, 64, 65, 100, 700, R - 1, R, R + 1, 5000]


def island_shapes(R: int):
    return [(a, j) for a in (1, 2, 3, 5) for j in (61, 63, 64, 67, R - 3, R - 1, R + 3)]


def _fill(mask: np.ndarray, abc, seed) -> np.ndarray:
    rng = np.random.default_rng(seed)
    text = np.full(mask.size, JUNK, np.uint8)
    text[mask] = alphabet_chars(abc)[rng.integers(0, 64, int(mask.sum()))]
    return text


def every(g: int, phase: int, n: int, abc=(-1, -1), seed: int = 0) -> np.ndarray:
    """One alphabet character at phase, phase + g, phase + 2 g, ... of n bytes."""
    assert 0 <= phase < g
    mask = np.zeros(n, bool)
    mask[phase::g] = True
    return _fill(mask, abc, [g, phase, n, seed, 1])


def islands(a: int, j: int, n: int, abc=(-1, -1), seed: int = 0) -> np.ndarray:
    """a alphabet characters, then j junk bytes, repeated over n bytes."""
    mask = np.arange(n) % (a + j) < a
    return _fill(mask, abc, [a, j, n, seed, 2])


def every_cases(R: int):
    """(g, phase) of the `every` texts: phases 0 and 1 where g <= 4."""
    return [(g, p) for g in gaps(R) for p in ((0, 1) if g <= 4 else (0,))]


def corpus(R: int = 2048, abc=(-1, -1), ns=None):
    """[(name, text)] of every `every` and `islands` text at the lengths ns
    (default: lengths(R))."""
    out = []
    for n in (lengths(R) if ns is None else ns):
        for g, p in every_cases(R):
            out.append((f"every({g},{p},{n})", every(g, p, n, abc)))
        for a, j in island_shapes(R):
            out.append((f"islands({a},{j},{n})", islands(a, j, n, abc)))
    return out


def every_at(R: int, n: int, abc=(-1, -1)):
    """The thirteen `every` texts (phase 0) at one length."""
    return [(f"every({g},0,{n})", every(g, 0, n, abc)) for g in gaps(R)]


def is_alpha(text: np.ndarray, abc=(-1, -1)) -> np.ndarray:
    t = np.zeros(256, bool)
    t[alphabet_chars(abc)] = True
    return t[text]


def range_stats(text: np.ndarray, R: int, ranges_per_tile: int = TILE, abc=(-1, -1)) -> dict:
    """What the exact decode of `text` in ranges of R characters meets:

    few         ranges holding 0 < count < k alphabet characters
    exact       ranges holding count == k > 0 of them
    completions ranges (not the last) that own a group (count > k) and end
                inside one: they take the 4 - (B + count) % 4 next characters
    partial     completions with a 64-byte window that holds some, but not
                all, of the characters still needed
    far         completions whose last character (or the end of the stream)
                lies at least 2 R past the range's end
    tile_edge   completions of a tile's last range
    to_end      {V mod 4: completions that run out of stream}
    tail_far    1 if the last V mod 4 alphabet characters do not all lie in
                the stream's last 64 bytes
    """
    n = text.size
    ap = np.flatnonzero(is_alpha(text, abc))  # positions of the alphabet characters
    V = ap.size
    s = dict(few=0, exact=0, completions=0, partial=0, far=0, tile_edge=0,
             to_end={1: 0, 2: 0, 3: 0}, tail_far=0, V=V)
    nranges = (n + R - 1) // R
    for r in range(nranges):
        rb, re = r * R, min(r * R + R, n)
        B = int(np.searchsorted(ap, rb))
        E = int(np.searchsorted(ap, re))  # alphabet characters before the range's end
        c, k = E - B, (4 - B % 4) % 4
        if 0 < c < k:
            s["few"] += 1
        if c == k > 0:
            s["exact"] += 1
        if r == nranges - 1 or c <= k or E % 4 == 0:
            continue
        s["completions"] += 1
        need = 4 - E % 4
        took = ap[E:E + need]
        ended = took.size < need
        if ended:
            s["to_end"][V % 4] += 1
            reach = n - re
            s["partial"] += int(took.size > 0)
        else:
            reach = int(took[-1]) + 1 - re
            w = (took - re) // WINDOW
            s["partial"] += int(w[0] != w[-1])
        s["far"] += int(reach >= 2 * R)
        s["tile_edge"] += int((r + 1) % ranges_per_tile == 0)
    if V % 4 and ap[V - V % 4] < n - WINDOW:
        s["tail_far"] = 1
    return s


COUNTS = ("few", "exact", "partial", "far", "tile_edge", "tail_far")


def corpus_stats(texts, R: int, ranges_per_tile: int = TILE, abc=(-1, -1)) -> dict:
    """Over [(name, text)]: for each count of range_stats, the number of
    texts that reach it; to_end by V mod 4."""
    tot = {k: 0 for k in COUNTS}
    tot["to_end"] = {1: 0, 2: 0, 3: 0}
    for _, t in texts:
        s = range_stats(t, R, ranges_per_tile, abc)
        for k in COUNTS:
            tot[k] += int(s[k] > 0)
        for v in (1, 2, 3):
            tot["to_end"][v] += int(s["to_end"][v] > 0)
    return tot
