"""The flat encode's plain-store window (k_encode_flat: the last 65,536 whole
tiles, 256 MiB of characters, are stored with the plain policy so that they
stay in the memory-side cache for the reader; everything before them, and
every store of a buffer no longer than the window, is non-temporal) must not
be observable in the bytes.

Lengths sit around N0 = 65,536 tiles x 3,072 input bytes, the longest
buffer without a window: one tile under, exactly N0, one byte and one quad
past (a partial last tile and a tail, still no window), one tile over (one
non-temporal tile, then the window), a partial tile over, two tiles over;
each with n % 12 in {0, 1, 11}.  Plus a length under one tile, a length far
under the window, and one of more than twice the window (both policies in
one launch, most tiles non-temporal).

The reference is the oracle's encode of the longest input, computed once:
base64 is prefix-stable at 3-byte groups, so the first 4 * (n // 3)
characters of every shorter case are its prefix, and the last group of each
case is encoded by the oracle on its own.  One case is also checked against
the oracle's encode of exactly its bytes.  Every output buffer is poisoned
before the call and carries a canary behind its end.

The decode's side is unchanged (its loads stay non-temporal and hit the
cache); it is run here on the encoder's output fresh from the encode, clean
and with one junk byte before the window, inside it and in the last wave,
against the oracle, with the path it took.
"""
import ctypes

import numpy as np
import pytest
import torch

from async_amd import _lib, b64
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE_IN, TILE_CH = 3072, 4096
WIN_TILES = (256 << 20) // TILE_CH
N0 = WIN_TILES * TILE_IN
NMAX = 2 * N0 + 3 * TILE_IN + 11
CANARY = 64

BASES = {"tile_under": N0 - TILE_IN, "edge": N0, "quad_past": N0 + 12,
         "tile_over": N0 + TILE_IN, "partial_tile_over": N0 + TILE_IN + 1500,
         "two_tiles_over": N0 + 2 * TILE_IN}


@pytest.fixture(scope="module")
def ref():
    """The input stream on the device and the host, the oracle's characters
    of all of it on the device, and the poisoned work buffers."""
    x = torch.empty(NMAX, dtype=torch.uint8, device=DEV)
    b64.fill_splitmix64(x, 0xB0A7)
    host = x.cpu().numpy()
    chars = torch.from_numpy(orc.encode(host, as_array=True)).to(DEV)
    enc = torch.empty(b64.encoded_len(NMAX) + CANARY, dtype=torch.uint8, device=DEV)
    dec = torch.empty(b64.decoded_cap(b64.encoded_len(NMAX)) + CANARY, dtype=torch.uint8,
                      device=DEV)
    return x, host, chars, enc, dec


def _encode_checked(ref, n):
    """Encode x[:n] into the poisoned buffer; check it against the oracle."""
    x, host, chars, enc, _ = ref
    m = b64.encoded_len(n)
    enc[:m + CANARY].fill_(0xAA)  # no alphabet character, no padding
    got = b64.encode(x[:n], out=enc)
    assert got.numel() == m
    g = n // 3
    assert torch.equal(got[:4 * g], chars[:4 * g]), n
    if n % 3:
        assert got[4 * g:].cpu().numpy().tobytes() == orc.encode(host[3 * g:n]), n
    else:
        assert m == 4 * g
    assert bool((enc[m:m + CANARY] == 0xAA).all()), n
    return got


def _round_trip(ref, got, n):
    x, _, _, _, dec = ref
    cap = b64.decoded_cap(got.numel())
    dec[:cap + CANARY].fill_(0x55)
    d = b64.decode(got, out=dec)
    assert d.info().out_len == n
    assert torch.equal(dec[:n], x[:n]), n
    assert bool((dec[cap:cap + CANARY] == 0x55).all()), n


@pytest.mark.parametrize("rem", [0, 1, 11])
@pytest.mark.parametrize("where", sorted(BASES))
def test_boundary_lengths(ref, where, rem):
    n = BASES[where] + rem
    assert n % 12 == rem
    _round_trip(ref, _encode_checked(ref, n), n)


@pytest.mark.parametrize("n", [1000, (5 << 20) + 7, NMAX])
def test_short_and_long(ref, n):
    """Under one tile, far under the window (both wholly non-temporal), and
    more than twice the window (both policies in one launch)."""
    _round_trip(ref, _encode_checked(ref, n), n)


def test_edge_case_against_the_oracle_directly(ref):
    """The prefix argument above, tied down once: one boundary case against
    the oracle's encode of exactly its bytes."""
    x, host, _, _, _ = ref
    n = BASES["tile_over"] + 11
    got = _encode_checked(ref, n)
    want = torch.from_numpy(orc.encode(host[:n], as_array=True)).to(DEV)
    assert torch.equal(got, want)


def _paths():
    out = (ctypes.c_uint64 * 5)()
    _lib.load().b64x_diag_paths(out)
    return [int(v) for v in out]


@pytest.mark.parametrize("case, where", [(0, "before_window"), (1, "in_window"),
                                         (2, "last_wave")])
def test_decode_of_fresh_characters_with_a_failing_slot(ref, case, where):
    """One junk byte in the characters the encode has just written: before
    the window (a non-temporal tile), inside it, and in the decode's last
    wave.  out_len, the bytes and the path against the oracle; a length of
    its own per case, so that no held model or hint of another case applies
    and the call probes."""
    _, _, _, _, dec = ref
    n = N0 + 2 * TILE_IN + 7 + 12 * case
    got = _encode_checked(ref, n)
    m = got.numel()
    p = {"before_window": TILE_CH + 100, "in_window": m // 2 + 3, "last_wave": m - 100}[where]
    assert (p >= 2 * TILE_CH) == (where != "before_window")  # the window starts at tile 2
    got[p] = 0x21
    text = got.cpu().numpy()
    want = torch.from_numpy(orc.decode(text.tobytes(), as_array=True)).to(DEV)
    cap = b64.decoded_cap(m)
    dec[:cap + CANARY].fill_(0x55)
    ws = torch.zeros(b64.workspace_size(m), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = _paths()
    d = b64.decode(got, out=dec, workspace=ws)
    info = d.info()
    after = _paths()
    assert info.out_len == want.numel()
    assert torch.equal(dec[:want.numel()], want)
    assert bool((dec[cap:cap + CANARY] == 0x55).all())
    # probes launched, held-model skips, hinted single passes
    assert [after[k] - before[k] for k in range(3)] == [1, 0, 0]
