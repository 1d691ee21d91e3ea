"""Host-side mirror of the base64 byte-stream engine over device tensors.

Thin wrappers over the b64x C ABI (include/b64x.h): torch provides device
memory and the stream, libasync_b64.so does the work.  The names follow the
reference's operations (src/base64encoder.c ``base64_encode`` /
src/base64decoder.c ``base64_decode``), applied to whole device-resident
buffers and batches instead of a pull-model stream:

    encode(x)                  one buffer      (b64x_encode_dev)
    decode(x)                  one buffer      (b64x_decode_dev)
    encode_lines(x)            one buffer, line-wrapped text: MIME 76/CRLF,
                               PEM 64/LF      (b64x_encode_lines_dev)
    decode_strict(x)           one buffer, strict: accepts exactly what
                               encode / encode_lines write, else the kind and
                               offset of the first offence
                                              (b64x_decode_strict_dev)
    encode_strided / decode_strided            uniform batches
    decode_strict_strided                      uniform batches, strict
    encode_lines_strided                       uniform batches, each row wrapped
    encode_batch / decode_batch                ragged batches (offsets)
    encode_lines_batch                         ragged batches, each buffer wrapped
                                              (b64x_encode_lines_batch)
    decode_strict_batch                        ragged batches, strict, one record
                               per buffer     (b64x_decode_strict_batch)
    lines_batch_layout / strict_batch_layout   their output offsets, from the
                               input offsets, on the tensor's own device
    encode_batch_wide                          ragged batches, plain or wrapped,
                               balanced over bytes: buffers of any size in
                               one call       (b64x_encode_batch_wide)
    decode_strict_batch_wide                   ragged batches, strict, balanced
                               over bytes: texts of any size in one call, one
                               record per text (b64x_decode_strict_batch_wide)
    decode_strict_skip(x)      one buffer, strict, ignoring CR and LF (or another
                               small set of bytes) wherever they stand; also
                               validate-only   (b64x_decode_strict_skip_dev)
    decode_strict_skip_batch                   ragged batches of it, one record
                               per buffer      (b64x_decode_strict_skip_batch)
    skip_batch_layout                          its output offsets
    decode_strict_skip_strided                 uniform batches of it, each row read
                               once by one kernel, no workspace; also
                               validate-only   (b64x_decode_strict_skip_strided)
    decode_strict_skip_pieces                  texts that arrive in pieces: many
                               streams per call, each continued from a state
                               in device memory (b64x_decode_strict_skip_pieces)
    skip_states / skip_pieces_layout           its zeroed states and its output
                               offsets; SKIP_STATE_BYTES, PIECE_FINAL
    decode_strict_skip_piece                   one large piece of one text on the
                               same state, a wave per tile of it
                                          (b64x_decode_strict_skip_piece_dev)
    strict_skip_piece_workspace_size           its workspace
    decode_strict_skip_pieces_wide             many pieces of any size in one call, a
                               wave per tile of each, every length read on the
                               device        (b64x_decode_strict_skip_pieces_wide)
    strict_skip_pieces_wide_workspace_size     its workspace; STRICT_BOUND

Every function raises (B64xError / RuntimeError) if the HIP library is
missing or a call fails; nothing here computes base64 on the CPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import (PIECE_FINAL, RES_BYTES, SKIP_STATE_BYTES, STRICT_RES_BYTES,  # noqa: F401
                   B64xError, DecResult, StrictResult, alphabet)

HOLD_TAIL = 1  # B64X_DEC_HOLD_TAIL
EXPECT_JUNK = 2  # B64X_DEC_EXPECT_JUNK
STRICT_BOUND = 6  # B64X_STRICT_BOUND: decode_strict_skip_pieces_wide's pieces exceed total_cap


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream(stream) -> int | None:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def _u8(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous uint8 CUDA tensor")
    return t


def encoded_len(n: int, pad: bool = True) -> int:
    return int(_lib.load().b64x_encoded_len(n, pad))


def decoded_cap(nchars: int) -> int:
    return int(_lib.load().b64x_decoded_cap(nchars))


def workspace_size(nchars: int = 0) -> int:
    return int(_lib.load().b64x_decode_workspace_size(nchars))


_DEFAULT_ABC: list = []  # the reference's alphabet, built once (read-only to the library)


def _abc(abc) -> _lib.Alphabet:
    if abc is None:
        if not _DEFAULT_ABC:
            _DEFAULT_ABC.append(alphabet())
        return _DEFAULT_ABC[0]
    return abc if isinstance(abc, _lib.Alphabet) else alphabet(*abc) if abc else alphabet()


def encode(x: torch.Tensor, out: torch.Tensor | None = None, abc=None,
           stream=None) -> torch.Tensor:
    """Base64-encode a device buffer; returns the character tensor."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    n = x.numel()
    m = encoded_len(n, a.pad)
    if out is None:
        out = torch.empty(max(m, 1), dtype=torch.uint8, device=x.device)
    _u8(out, "output")
    if out.numel() < m:
        raise ValueError("output too small")
    _lib.check("b64x_encode_dev", lib.b64x_encode_dev(
        _ptr(x), n, _ptr(out), ctypes.byref(a), _stream(stream)))
    return out[:m]


def encoded_lines_len(n: int, line_len: int = 76, sep: bytes = b"\r\n",
                      trailing: bool = True, pad: bool = True) -> int:
    """Bytes encode_lines() writes for n input bytes."""
    fmt = _lib.lines(line_len, sep, trailing)
    if line_len <= 0 or line_len % 4:
        raise ValueError("line_len must be a positive multiple of 4")
    return int(_lib.load().b64x_encoded_lines_len(n, pad, ctypes.byref(fmt)))


def encode_lines(x: torch.Tensor, line_len: int = 76, sep: bytes = b"\r\n",
                 trailing: bool = True, out: torch.Tensor | None = None, abc=None,
                 stream=None) -> torch.Tensor:
    """Base64-encode a device buffer as line-wrapped text: lines of line_len
    characters, `sep` after each (after the last one only with `trailing`).
    The defaults are RFC 2045 (MIME); 64, b"\\n" is a PEM body; 76, b"\\n" is
    base64.encodebytes.  Returns the text tensor."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    n = x.numel()
    m = encoded_lines_len(n, line_len, sep, trailing, a.pad)
    fmt = _lib.lines(line_len, sep, trailing)
    if out is None:
        out = torch.empty(max(m, 1), dtype=torch.uint8, device=x.device)
    _u8(out, "output")
    if out.numel() < m:
        raise ValueError("output too small")
    _lib.check("b64x_encode_lines_dev", lib.b64x_encode_lines_dev(
        _ptr(x), n, _ptr(out), ctypes.byref(a), ctypes.byref(fmt), _stream(stream)))
    return out[:m]


@dataclass
class Decoded:
    out: torch.Tensor          # capacity-sized output buffer
    result: torch.Tensor       # b64x_dec_result (RES_BYTES) on the device
    nchars: int = 0            # the call's character count, flags and the
    flags: int = 0             # sequence number it drew: what its record
    seq: int = 0               # must echo (b64x_result_check)
    stream: object = None      # the stream the decode ran on

    def info(self) -> DecResult:
        """The call's result record, checked: waits for the decode's own
        stream, copies the record back and refuses one that is not this
        call's or is inconsistent (b64x_result_check)."""
        s = self.stream if self.stream is not None else torch.cuda.current_stream()
        s.synchronize()
        host = self.result[:RES_BYTES].cpu().numpy()  # keep alive across the copy
        r = DecResult.from_buffer_copy(host.tobytes())
        if self.seq:
            _lib.check("b64x_result_check", _lib.load().b64x_result_check(
                ctypes.byref(r), self.nchars, self.flags, self.seq))
        return r

    def bytes(self) -> torch.Tensor:
        """The decoded bytes (synchronises to read the length)."""
        return self.out[: self.info().out_len]


def decode(x: torch.Tensor, out: torch.Tensor | None = None, abc=None,
           hold_tail: bool = False, workspace: torch.Tensor | None = None,
           result: torch.Tensor | None = None, stream=None,
           expect_junk: bool = False) -> Decoded:
    """Leniently decode a device buffer of base64 characters.
    expect_junk: the input holds non-alphabet bytes throughout (MIME line
    breaks) -- decode in one pass (B64X_DEC_EXPECT_JUNK); same result."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    n = x.numel()
    cap = decoded_cap(n)
    if out is None:
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=x.device)
    _u8(out, "output")
    if out.numel() < cap:
        raise ValueError("output too small")
    if result is None:
        result = torch.zeros(RES_BYTES, dtype=torch.uint8, device=x.device)
    # workspace: a caller's (zeroed before its first use; the library keeps
    # it re-armed), else the library's own for the stream (NULL), which also
    # keeps the line model of its last probe for the next call of a length
    # Under graph capture with no workspace given, a torch-allocated one (the
    # library will not allocate or rebind one inside a capture: -EBUSY).
    if workspace is None and torch.cuda.is_current_stream_capturing():
        workspace = torch.zeros(workspace_size(n), dtype=torch.uint8, device=x.device)
    flags = (HOLD_TAIL if hold_tail else 0) | (EXPECT_JUNK if expect_junk else 0)
    seq = ctypes.c_uint32(0)
    # the stream looked up once (torch.cuda.current_stream() costs ~3 us of
    # the call's host time, and a junk-laden or small decode is timed with it)
    s = stream if stream is not None else torch.cuda.current_stream()
    _lib.check("b64x_decode_dev_seq", lib.b64x_decode_dev_seq(
        _ptr(x), n, _ptr(out), _ptr(result), ctypes.byref(a), flags,
        _ptr(workspace) if workspace is not None else None, s.cuda_stream,
        ctypes.byref(seq)))
    return Decoded(out, result, n, flags & HOLD_TAIL, seq.value, s)


class B64xFormatError(ValueError):
    """A strict decode refused its text: `kind` is the B64X_STRICT_* code of
    the first offence and `pos` its byte offset in the text."""

    def __init__(self, kind: int, pos: int):
        self.kind = kind
        self.pos = pos
        name = _lib.STRICT_NAMES[kind] if 0 <= kind < len(_lib.STRICT_NAMES) else str(kind)
        super().__init__(f"not canonical base64: {name} at offset {pos}")


def _fmt(line_len, sep, trailing):
    """(b64x_lines or None, a byref of it or None) for line_len (None: plain)."""
    if line_len is None:
        return None, None
    fmt = _lib.lines(line_len, sep, trailing)
    return fmt, ctypes.byref(fmt)


def strict_decoded_cap(nchars: int, line_len: int | None = None, sep: bytes = b"\r\n",
                       trailing: bool = True) -> int:
    """Output capacity decode_strict() needs for nchars bytes of text."""
    _, ref = _fmt(line_len, sep, trailing)
    return int(_lib.load().b64x_strict_decoded_cap(nchars, ref))


@dataclass
class StrictDecoded:
    out: torch.Tensor          # capacity-sized output buffer
    result: torch.Tensor       # b64x_strict_result (STRICT_RES_BYTES) on the device
    stream: object = None      # the stream the decode ran on

    def info(self) -> StrictResult:
        """The call's record: waits for the decode's own stream and copies
        the record back."""
        s = self.stream if self.stream is not None else torch.cuda.current_stream()
        s.synchronize()
        host = self.result[:STRICT_RES_BYTES].cpu().numpy()
        return StrictResult.from_buffer_copy(host.tobytes())

    def bytes(self) -> torch.Tensor:
        """The decoded bytes, or B64xFormatError with the first offence."""
        r = self.info()
        if r.err:
            raise B64xFormatError(r.err, r.err_pos)
        return self.out[: r.out_len]


def decode_strict(x: torch.Tensor, line_len: int | None = None, sep: bytes = b"\r\n",
                  trailing: bool = True, out: torch.Tensor | None = None, abc=None,
                  result: torch.Tensor | None = None, stream=None) -> StrictDecoded:
    """Strictly decode a device buffer of base64 text: plain (line_len None,
    what encode() writes) or line-wrapped (what encode_lines() writes for the
    same line_len, sep and trailing).  Any other text is refused: the record
    (StrictDecoded.info()) names the kind and offset of the first offence."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    n = x.numel()
    fmt, ref = _fmt(line_len, sep, trailing)
    cap = int(lib.b64x_strict_decoded_cap(n, ref))
    if out is None:
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=x.device)
    _u8(out, "output")
    if out.numel() < cap:
        raise ValueError("output too small")
    if result is None:
        result = torch.empty(STRICT_RES_BYTES, dtype=torch.uint8, device=x.device)
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES:
        raise ValueError("result too small")
    s = stream if stream is not None else torch.cuda.current_stream()
    # an empty tensor has no address; nothing is read through the stand-in
    _lib.check("b64x_decode_strict_dev", lib.b64x_decode_strict_dev(
        _ptr(x) if n else _ptr(result), n, _ptr(out) if out.numel() else _ptr(result),
        _ptr(result), ctypes.byref(a), ref, s.cuda_stream))
    return StrictDecoded(out, result, s)


def decode_strict_strided(x: torch.Tensor, in_stride: int, length: int, nbuf: int,
                          out: torch.Tensor, out_stride: int, result: torch.Tensor,
                          line_len: int | None = None, sep: bytes = b"\r\n",
                          trailing: bool = True, abc=None, stream=None) -> None:
    """Row i (`length` bytes of text at x + i*in_stride) strictly decoded on
    its own into out + i*out_stride; its b64x_strict_result goes to bytes
    [24 i, 24 i + 24) of `result` (a uint8 tensor of 24*nbuf bytes)."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    _u8(out, "output")
    _u8(result, "result")
    fmt, ref = _fmt(line_len, sep, trailing)
    cap = int(lib.b64x_strict_decoded_cap(length, ref))
    if result.numel() < STRICT_RES_BYTES * nbuf:
        raise ValueError("result must hold 24 bytes per row")
    if nbuf and (x.numel() < (nbuf - 1) * in_stride + length or
                 out.numel() < (nbuf - 1) * out_stride + cap):
        raise ValueError("buffers too small for the batch")
    _lib.check("b64x_decode_strict_strided", lib.b64x_decode_strict_strided(
        _ptr(x) if x.numel() else _ptr(result), in_stride, length, nbuf,
        _ptr(out) if out.numel() else _ptr(result), out_stride, _ptr(result),
        ctypes.byref(a), ref, _stream(stream)))


def encode_strided(x: torch.Tensor, in_stride: int, length: int, nbuf: int,
                   out: torch.Tensor, out_stride: int, abc=None, stream=None) -> None:
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    _u8(out, "output")
    if nbuf and (x.numel() < (nbuf - 1) * in_stride + length or
                 out.numel() < (nbuf - 1) * out_stride + encoded_len(length, a.pad)):
        raise ValueError("buffers too small for the batch")
    _lib.check("b64x_encode_strided", lib.b64x_encode_strided(
        _ptr(x), in_stride, length, nbuf, _ptr(out), out_stride, ctypes.byref(a),
        _stream(stream)))


def encode_lines_strided(x: torch.Tensor, in_stride: int, length: int, nbuf: int,
                         out: torch.Tensor, out_stride: int, line_len: int = 76,
                         sep: bytes = b"\r\n", trailing: bool = True, abc=None,
                         stream=None) -> None:
    """Row i (`length` bytes at x + i*in_stride) wrapped on its own into
    out + i*out_stride; every row gets encoded_lines_len(length, ...) bytes."""
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    _u8(out, "output")
    m = encoded_lines_len(length, line_len, sep, trailing, a.pad)
    fmt = _lib.lines(line_len, sep, trailing)
    if nbuf and (x.numel() < (nbuf - 1) * in_stride + length or
                 out.numel() < (nbuf - 1) * out_stride + m):
        raise ValueError("buffers too small for the batch")
    _lib.check("b64x_encode_lines_strided", lib.b64x_encode_lines_strided(
        _ptr(x), in_stride, length, nbuf, _ptr(out), out_stride, ctypes.byref(a),
        ctypes.byref(fmt), _stream(stream)))


def decode_strided(x: torch.Tensor, in_stride: int, length: int, nbuf: int,
                   out: torch.Tensor, out_stride: int, outlen: torch.Tensor,
                   abc=None, stream=None) -> None:
    lib = _lib.load()
    a = _abc(abc)
    _u8(x, "input")
    _u8(out, "output")
    if outlen.dtype != torch.int64 or outlen.numel() < nbuf or not outlen.is_cuda:
        raise ValueError("outlen must be an int64 CUDA tensor with nbuf entries")
    if nbuf and (x.numel() < (nbuf - 1) * in_stride + length or
                 out.numel() < (nbuf - 1) * out_stride + decoded_cap(length)):
        raise ValueError("buffers too small for the batch")
    _lib.check("b64x_decode_strided", lib.b64x_decode_strided(
        _ptr(x), in_stride, length, nbuf, _ptr(out), out_stride, _ptr(outlen),
        ctypes.byref(a), _stream(stream)))


def _offsets(t: torch.Tensor, n: int, what: str) -> torch.Tensor:
    if t.dtype != torch.int64 or not t.is_cuda or t.numel() < n:
        raise ValueError(f"{what} must be an int64 CUDA tensor of {n} entries")
    return t


def encode_batch(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                 out_off: torch.Tensor, abc=None, stream=None) -> None:
    """Ragged batch: buffer i = x[in_off[i]:in_off[i+1]] -> out[out_off[i]:]."""
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    _lib.check("b64x_encode_batch", lib.b64x_encode_batch(
        _ptr(_u8(x, "input")), _ptr(in_off), nbuf, _ptr(_u8(out, "output")),
        _ptr(out_off), ctypes.byref(a), _stream(stream)))


def decode_batch(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                 out_off: torch.Tensor, outlen: torch.Tensor, abc=None,
                 stream=None) -> None:
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    _offsets(outlen, nbuf, "outlen")
    _lib.check("b64x_decode_batch", lib.b64x_decode_batch(
        _ptr(_u8(x, "input")), _ptr(in_off), nbuf, _ptr(_u8(out, "output")),
        _ptr(out_off), _ptr(outlen), ctypes.byref(a), _stream(stream)))


def _lengths(in_off: torch.Tensor) -> torch.Tensor:
    if in_off.dtype != torch.int64 or in_off.dim() != 1 or in_off.numel() < 1:
        raise ValueError("in_off must be a 1-D int64 tensor of nbuf + 1 entries")
    return in_off[1:] - in_off[:-1]


def _starts(sizes: torch.Tensor, align: int) -> torch.Tensor:
    """nbuf + 1 offsets of buffers of `sizes` bytes laid out in order, every
    start rounded up to `align`; the last entry is the arena's size."""
    if align < 1:
        raise ValueError("align must be at least 1")
    out = torch.zeros(sizes.numel() + 1, dtype=torch.int64, device=sizes.device)
    torch.cumsum((sizes + (align - 1)) // align * align, 0, out=out[1:])
    return out


def lines_batch_layout(in_off: torch.Tensor, line_len: int = 76, sep: bytes = b"\r\n",
                       trailing: bool = True, pad: bool = True, align: int = 1) -> torch.Tensor:
    """Output offsets for encode_lines_batch(): nbuf + 1 int64 entries, entry
    i the start of buffer i's wrapped text (rounded up to `align`), the last
    the size of the arena.  Computed from in_off on its own device with
    integer tensor ops: no host synchronisation (a CPU tensor works too)."""
    s = len(bytes(sep))
    if line_len <= 0 or line_len % 4 or not 1 <= s <= 4:
        raise ValueError("line_len must be a positive multiple of 4, the separator 1 to 4 bytes")
    n = _lengths(in_off)
    chars = (n + 2) // 3 * 4 if pad else (4 * n + 2) // 3
    lines = (chars + (line_len - 1)) // line_len
    text = chars + s * (lines - (0 if trailing else 1))
    return _starts(torch.where(chars > 0, text, torch.zeros_like(text)), align)


def strict_batch_layout(in_off: torch.Tensor, line_len: int | None = None,
                        sep: bytes = b"\r\n", trailing: bool = True,
                        align: int = 1) -> torch.Tensor:
    """Output offsets for decode_strict_batch(): nbuf + 1 int64 entries, entry
    i the start of text i's decode capacity (strict_decoded_cap of its length,
    the start rounded up to `align`), the last the size of the arena.  Like
    lines_batch_layout(), tensor ops on in_off's own device."""
    n = _lengths(in_off)
    if line_len is None:
        chars = n
    else:
        s = len(bytes(sep))
        if line_len <= 0 or not 1 <= s <= 4:
            raise ValueError("line_len must be positive, the separator 1 to 4 bytes")
        pitch = line_len + s
        m = n if trailing else n + s
        k = m // pitch
        chars = k * line_len + torch.clamp(m - k * pitch - s, min=0)
    return _starts((chars + 3) // 4 * 3, align)


def encode_lines_batch(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                       out_off: torch.Tensor, line_len: int = 76, sep: bytes = b"\r\n",
                       trailing: bool = True, abc=None, stream=None) -> None:
    """Ragged batch of encode_lines(): buffer i = x[in_off[i]:in_off[i+1]] is
    wrapped on its own into out[out_off[i]:] (lines_batch_layout() gives the
    offsets).  The lengths are read on the device: a call captured into a
    graph replays on other lengths written into the same offset tensors."""
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    fmt = _lib.lines(line_len, sep, trailing)
    # an empty tensor has no address; nothing is read through the stand-in
    _u8(x, "input")
    _u8(out, "output")
    _lib.check("b64x_encode_lines_batch", lib.b64x_encode_lines_batch(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), nbuf,
        _ptr(out) if out.numel() else _ptr(in_off), _ptr(out_off), ctypes.byref(a),
        ctypes.byref(fmt), _stream(stream)))


def encode_batch_wide(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                      out_off: torch.Tensor, line_len: int | None = None, sep: bytes = b"\r\n",
                      trailing: bool = True, total_hint: int | None = None, abc=None,
                      stream=None) -> None:
    """encode_batch() (line_len None) or encode_lines_batch() balanced over the
    batch's bytes instead of its buffers: the same addressing, the same bytes
    written, but a buffer of MiB among buffers of KiB is spread over the
    device like the rest.  out_off is encode_batch's encoded_len layout, or
    lines_batch_layout()'s.  total_hint sizes the grid and nothing else (None:
    x.numel(); 0: fill the device); the lengths are read on the device, the
    call makes no host synchronisation and replays on other offsets."""
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    fmt, ref = _fmt(line_len, sep, trailing)  # fmt: alive until the call has read it
    _u8(x, "input")
    _u8(out, "output")
    hint = x.numel() if total_hint is None else int(total_hint)
    if hint < 0:
        raise ValueError("total_hint must not be negative")
    # an empty tensor has no address; nothing is read through the stand-in
    _lib.check("b64x_encode_batch_wide", lib.b64x_encode_batch_wide(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), nbuf, hint,
        _ptr(out) if out.numel() else _ptr(in_off), _ptr(out_off), ctypes.byref(a), ref,
        _stream(stream)))


def decode_strict_batch(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                        out_off: torch.Tensor, result: torch.Tensor,
                        line_len: int | None = None, sep: bytes = b"\r\n",
                        trailing: bool = True, abc=None, stream=None) -> None:
    """Ragged batch of decode_strict(): text i = x[in_off[i]:in_off[i+1]] is
    strictly decoded on its own into out[out_off[i]:] (strict_batch_layout()
    gives the offsets); its b64x_strict_result goes to bytes [24 i, 24 i + 24)
    of `result` (a uint8 tensor of 24*nbuf bytes), err_pos an offset in text
    i.  Replays on other lengths like encode_lines_batch()."""
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * nbuf:
        raise ValueError("result must hold 24 bytes per buffer")
    fmt, ref = _fmt(line_len, sep, trailing)
    _u8(x, "input")
    _u8(out, "output")
    _lib.check("b64x_decode_strict_batch", lib.b64x_decode_strict_batch(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), nbuf,
        _ptr(out) if out.numel() else _ptr(in_off), _ptr(out_off), _ptr(result),
        ctypes.byref(a), ref, _stream(stream)))


def decode_strict_batch_wide(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor,
                             out_off: torch.Tensor, result: torch.Tensor,
                             line_len: int | None = None, sep: bytes = b"\r\n",
                             trailing: bool = True, total_hint: int | None = None, abc=None,
                             stream=None) -> None:
    """decode_strict_batch() balanced over the batch's bytes instead of its
    texts: the same addressing (strict_batch_layout() gives out_off), the same
    records and, for an accepted text, the same bytes, but a text of MiB among
    texts of KiB is spread over the device like the rest.  total_hint sizes
    the grid and nothing else (None: x.numel(); 0: fill the device); the
    lengths are read on the device, the call makes no host synchronisation and
    replays on other offsets and contents."""
    lib = _lib.load()
    a = _abc(abc)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _offsets(out_off, nbuf, "out_off")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * nbuf:
        raise ValueError("result must hold 24 bytes per buffer")
    fmt, ref = _fmt(line_len, sep, trailing)  # fmt: alive until the call has read it
    _u8(x, "input")
    _u8(out, "output")
    hint = x.numel() if total_hint is None else int(total_hint)
    if hint < 0:
        raise ValueError("total_hint must not be negative")
    # an empty tensor has no address; nothing is read through the stand-in
    _lib.check("b64x_decode_strict_batch_wide", lib.b64x_decode_strict_batch_wide(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), nbuf, hint,
        _ptr(out) if out.numel() else _ptr(in_off), _ptr(out_off), _ptr(result),
        ctypes.byref(a), ref, _stream(stream)))


def strict_skip_workspace_size(nchars: int, validate_only: bool = False) -> int:
    """Workspace bytes decode_strict_skip() needs for nchars bytes of text."""
    return int(_lib.load().b64x_strict_skip_workspace_size(nchars, validate_only))


def decode_strict_skip(x: torch.Tensor, skip: bytes = b"\r\n", out: torch.Tensor | None = None,
                       validate_only: bool = False, abc=None,
                       workspace: torch.Tensor | None = None,
                       result: torch.Tensor | None = None, stream=None) -> StrictDecoded:
    """Strictly decode a device buffer of base64 text, ignoring the bytes of
    `skip` wherever they stand (the default: CR and LF): accepts exactly the
    texts whose other bytes decode_strict() accepts as plain text, with the
    same bytes; any other text is refused, the record naming the kind and the
    offset of the first offence.  validate_only: the text is read once and
    only the record is written (`out` stays as it is, or is an empty tensor).
    workspace: strict_skip_workspace_size(len, validate_only) bytes, zeroed
    before their first use; allocated and zeroed here when None."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    _u8(x, "input")
    n = x.numel()
    if validate_only:
        if out is None:
            out = torch.empty(0, dtype=torch.uint8, device=x.device)
    else:
        cap = decoded_cap(n)
        if out is None:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=x.device)
        _u8(out, "output")
        if out.numel() < cap:
            raise ValueError("output too small")
    if result is None:
        result = torch.empty(STRICT_RES_BYTES, dtype=torch.uint8, device=x.device)
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES:
        raise ValueError("result too small")
    # an empty text needs the head alone (a length of 0 asks the lenient
    # decoder's size function for its largest workspace)
    need = strict_skip_workspace_size(n, validate_only or n == 0)
    if workspace is None:
        workspace = torch.zeros(need, dtype=torch.uint8, device=x.device)
    _u8(workspace, "workspace")
    if workspace.numel() < need:
        raise ValueError("workspace too small")
    s = stream if stream is not None else torch.cuda.current_stream()
    # an empty tensor has no address; nothing is read or written through the stand-in
    _lib.check("b64x_decode_strict_skip_dev", lib.b64x_decode_strict_skip_dev(
        _ptr(x) if n else _ptr(result),
        n, None if validate_only else (_ptr(out) if out.numel() else _ptr(result)),
        _ptr(result), ctypes.byref(a), ctypes.byref(k), _ptr(workspace), s.cuda_stream))
    return StrictDecoded(out, result, s)


def skip_batch_layout(in_off: torch.Tensor, align: int = 4) -> torch.Tensor:
    """Output offsets for decode_strict_skip_batch(): nbuf + 1 int64 entries,
    entry i the start of text i's decode capacity (decoded_cap of its length,
    the start rounded up to `align`), the last the size of the arena.  Like
    lines_batch_layout(), tensor ops on in_off's own device."""
    return _starts((_lengths(in_off) + 3) // 4 * 3, align)


def decode_strict_skip_batch(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor | None,
                             out_off: torch.Tensor | None, result: torch.Tensor,
                             skip: bytes = b"\r\n", abc=None,
                             workspace: torch.Tensor | None = None, stream=None) -> None:
    """Ragged batch of decode_strict_skip(): text i = x[in_off[i]:in_off[i+1]]
    is judged on its own, its b64x_strict_result in bytes [24 i, 24 i + 24) of
    `result`, and decoded into out[out_off[i]:] (skip_batch_layout() gives the
    offsets).  out None: validate only (out_off and workspace are not used).
    workspace: 8 bytes per buffer, allocated here when None.  Replays on other
    lengths like decode_strict_batch()."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    nbuf = in_off.numel() - 1
    _offsets(in_off, nbuf + 1, "in_off")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * nbuf:
        raise ValueError("result must hold 24 bytes per buffer")
    _u8(x, "input")
    if out is not None:
        _u8(out, "output")
        _offsets(out_off, nbuf, "out_off")
        if workspace is None:
            workspace = torch.empty(8 * max(nbuf, 1), dtype=torch.uint8, device=x.device)
        _u8(workspace, "workspace")
        if workspace.numel() < 8 * nbuf:
            raise ValueError("workspace must hold 8 bytes per buffer")
    _lib.check("b64x_decode_strict_skip_batch", lib.b64x_decode_strict_skip_batch(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), nbuf,
        None if out is None else (_ptr(out) if out.numel() else _ptr(in_off)),
        None if out is None else _ptr(out_off), _ptr(result), ctypes.byref(a), ctypes.byref(k),
        None if out is None else _ptr(workspace), _stream(stream)))


def decode_strict_skip_strided(x: torch.Tensor, in_stride: int, length: int, nbuf: int,
                               out: torch.Tensor | None, out_stride: int, result: torch.Tensor,
                               skip: bytes = b"\r\n", abc=None, stream=None) -> None:
    """Uniform batch of decode_strict_skip(): row i (`length` bytes of text at
    x + i*in_stride) is judged on its own, ignoring the bytes of `skip`
    wherever they stand; its b64x_strict_result goes to bytes [24 i, 24 i + 24)
    of `result`, and the bytes of an accepted row to out + i*out_stride
    (decoded_cap(length) bytes of room each).  out None: validate only
    (out_stride is not used).  One kernel that reads every row once; no
    workspace."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    _u8(x, "input")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * nbuf:
        raise ValueError("result must hold 24 bytes per row")
    if nbuf and x.numel() < (nbuf - 1) * in_stride + length:
        raise ValueError("buffers too small for the batch")
    if out is not None:
        _u8(out, "output")
        if nbuf and out.numel() < (nbuf - 1) * out_stride + decoded_cap(length):
            raise ValueError("buffers too small for the batch")
    # an empty tensor has no address; nothing is read or written through the stand-in
    _lib.check("b64x_decode_strict_skip_strided", lib.b64x_decode_strict_skip_strided(
        _ptr(x) if x.numel() else _ptr(result), in_stride, length, nbuf,
        None if out is None else (_ptr(out) if out.numel() else _ptr(result)),
        out_stride if out is not None else 0, _ptr(result),
        ctypes.byref(a), ctypes.byref(k), _stream(stream)))


def skip_piece_cap(length: int) -> int:
    """Output bytes a piece of `length` bytes may write: decoded_cap(length + 3)."""
    return int(_lib.load().b64x_skip_piece_cap(length))


def skip_states(n: int, device="cuda") -> torch.Tensor:
    """n states for decode_strict_skip_pieces(), each at the start of a text:
    a zeroed uint8 tensor of n * SKIP_STATE_BYTES bytes."""
    return torch.zeros(n * SKIP_STATE_BYTES, dtype=torch.uint8, device=device)


def skip_pieces_layout(in_off: torch.Tensor, align: int = 4) -> torch.Tensor:
    """Output offsets for decode_strict_skip_pieces(): npieces + 1 int64
    entries, entry i the start of piece i's capacity (skip_piece_cap of its
    length, the start rounded up to `align`), the last the size of the arena.
    Like skip_batch_layout(), tensor ops on in_off's own device."""
    return _starts((_lengths(in_off) + 6) // 4 * 3, align)


def decode_strict_skip_pieces(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor | None,
                              out_off: torch.Tensor | None, states: torch.Tensor,
                              result: torch.Tensor, final: torch.Tensor | None = None,
                              sid: torch.Tensor | None = None, skip: bytes = b"\r\n", abc=None,
                              stream=None) -> None:
    """decode_strict_skip() of texts that arrive in pieces, many streams in one
    call: piece i = x[in_off[i]:in_off[i+1]] continues the text of state
    sid[i] (an int32 tensor; None: state i) of `states` (skip_states(); the
    indices of one call must be distinct), writes its bytes to
    out[out_off[i]:] (skip_pieces_layout() gives the offsets) and its
    b64x_strict_result to bytes [24 i, 24 i + 24) of `result`.  A piece with
    final[i] & PIECE_FINAL (a uint8 tensor; None: none is) ends its text,
    takes the whole verdict and leaves its state zeroed for the next text.
    out None: validate only (out_off is not used).  Lengths, flags and
    indices are read on the device: a captured call replays on others."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    npieces = in_off.numel() - 1
    _offsets(in_off, npieces + 1, "in_off")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * npieces:
        raise ValueError("result must hold 24 bytes per piece")
    _u8(x, "input")
    _u8(states, "states")
    if states.numel() % SKIP_STATE_BYTES or states.data_ptr() % 8:
        raise ValueError("states must be whole 8-byte aligned states (skip_states())")
    if sid is None:
        if states.numel() < SKIP_STATE_BYTES * npieces:
            raise ValueError("states must hold 128 bytes per piece")
    elif sid.dtype != torch.int32 or not sid.is_cuda or sid.numel() < npieces:
        raise ValueError(f"sid must be an int32 CUDA tensor of {npieces} entries")
    if final is not None and (final.dtype != torch.uint8 or not final.is_cuda
                              or final.numel() < npieces):
        raise ValueError(f"final must be a uint8 CUDA tensor of {npieces} entries")
    if out is not None:
        _u8(out, "output")
        _offsets(out_off, npieces, "out_off")
    # an empty tensor has no address; nothing is read or written through the stand-in
    _lib.check("b64x_decode_strict_skip_pieces", lib.b64x_decode_strict_skip_pieces(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), npieces,
        None if out is None else (_ptr(out) if out.numel() else _ptr(in_off)),
        None if out is None else _ptr(out_off), _ptr(states) if states.numel() else None,
        _ptr(sid), _ptr(final), _ptr(result), ctypes.byref(a), ctypes.byref(k), _stream(stream)))


def strict_skip_piece_workspace_size(length: int, validate_only: bool = False) -> int:
    """Workspace bytes decode_strict_skip_piece() needs for a piece of `length` bytes."""
    return int(_lib.load().b64x_strict_skip_piece_workspace_size(length, validate_only))


def decode_strict_skip_piece(x: torch.Tensor, state: torch.Tensor, result: torch.Tensor,
                             out: torch.Tensor | None = None, final: bool = False,
                             skip: bytes = b"\r\n", abc=None,
                             workspace: torch.Tensor | None = None, stream=None) -> None:
    """decode_strict_skip_pieces() of one piece, spread over the GPU: x continues
    the text of `state` (one state of skip_states(), 128 bytes), writes its
    bytes to `out` (at least skip_piece_cap(len) bytes; None: validate only)
    and its b64x_strict_result to the first 24 bytes of `result`.  final: the
    piece ends its text, takes the whole verdict and leaves the state zeroed.
    The two calls may take turns on one state.  workspace:
    strict_skip_piece_workspace_size(len, out is None) bytes, 8-byte aligned,
    no preparation; allocated here when None.  A captured call replays on the
    same length only."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    _u8(x, "input")
    n = x.numel()
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES:
        raise ValueError("result too small")
    _u8(state, "state")
    if state.numel() != SKIP_STATE_BYTES or state.data_ptr() % 8:
        raise ValueError("state must be one 8-byte aligned state (skip_states(1))")
    if out is not None:
        _u8(out, "output")
        if out.numel() < skip_piece_cap(n):
            raise ValueError("output too small")
    need = strict_skip_piece_workspace_size(n, out is None)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    _u8(workspace, "workspace")
    if workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError("workspace too small or not 8-byte aligned")
    # an empty tensor has no address; nothing is read or written through the stand-in
    _lib.check("b64x_decode_strict_skip_piece_dev", lib.b64x_decode_strict_skip_piece_dev(
        _ptr(x) if n else _ptr(result), n, None if out is None else _ptr(out), _ptr(state),
        PIECE_FINAL if final else 0, _ptr(result), ctypes.byref(a), ctypes.byref(k),
        _ptr(workspace), _stream(stream)))


def strict_skip_pieces_wide_workspace_size(total_cap: int, npieces: int,
                                           validate_only: bool = False) -> int:
    """Workspace bytes decode_strict_skip_pieces_wide() needs for npieces pieces
    of at most total_cap bytes together."""
    return int(_lib.load().b64x_strict_skip_pieces_wide_workspace_size(total_cap, npieces,
                                                                       validate_only))


def decode_strict_skip_pieces_wide(x: torch.Tensor, in_off: torch.Tensor, out: torch.Tensor | None,
                                   out_off: torch.Tensor | None, states: torch.Tensor,
                                   result: torch.Tensor, workspace: torch.Tensor,
                                   total_cap: int | None = None, sid: torch.Tensor | None = None,
                                   flags: torch.Tensor | None = None, skip: bytes = b"\r\n",
                                   abc=None, stream=None) -> None:
    """decode_strict_skip_pieces() with a wave on every tile of every piece:
    the same pieces, states, records and bytes, for pieces of any size in a
    constant number of launches.  total_cap (default x.numel()) bounds
    in_off[-1] - in_off[0] and is the only length the host sees, so a captured
    call replays on other lengths, flags and indices within it; pieces that
    exceed it get the record {0, their bytes, STRICT_BOUND} and nothing is
    looked at.  flags: a uint8 tensor, flags[i] & PIECE_FINAL ends text i
    (None: none is).  A piece with an offence writes nothing to `out`.
    workspace: strict_skip_pieces_wide_workspace_size(total_cap, npieces,
    out is None) bytes, 8-byte aligned, no preparation."""
    lib = _lib.load()
    a = _abc(abc)
    k = _lib.skip_set(skip)
    npieces = in_off.numel() - 1
    _offsets(in_off, npieces + 1, "in_off")
    _u8(result, "result")
    if result.numel() < STRICT_RES_BYTES * npieces:
        raise ValueError("result must hold 24 bytes per piece")
    _u8(x, "input")
    if total_cap is None:
        total_cap = x.numel()
    if total_cap < 0:
        raise ValueError("total_cap must not be negative")
    _u8(states, "states")
    if states.numel() % SKIP_STATE_BYTES or states.data_ptr() % 8:
        raise ValueError("states must be whole 8-byte aligned states (skip_states())")
    if sid is None:
        if states.numel() < SKIP_STATE_BYTES * npieces:
            raise ValueError("states must hold 128 bytes per piece")
    elif sid.dtype != torch.int32 or not sid.is_cuda or sid.numel() < npieces:
        raise ValueError(f"sid must be an int32 CUDA tensor of {npieces} entries")
    if flags is not None and (flags.dtype != torch.uint8 or not flags.is_cuda
                              or flags.numel() < npieces):
        raise ValueError(f"flags must be a uint8 CUDA tensor of {npieces} entries")
    if out is not None:
        _u8(out, "output")
        _offsets(out_off, npieces, "out_off")
    _u8(workspace, "workspace")
    need = strict_skip_pieces_wide_workspace_size(total_cap, npieces, out is None)
    if workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError("workspace too small or not 8-byte aligned")
    # an empty tensor has no address; nothing is read or written through the stand-in
    _lib.check("b64x_decode_strict_skip_pieces_wide", lib.b64x_decode_strict_skip_pieces_wide(
        _ptr(x) if x.numel() else _ptr(in_off), _ptr(in_off), npieces, total_cap,
        None if out is None else (_ptr(out) if out.numel() else _ptr(in_off)),
        None if out is None else _ptr(out_off), _ptr(states) if states.numel() else None,
        _ptr(sid), _ptr(flags), _ptr(result), ctypes.byref(a), ctypes.byref(k), _ptr(workspace),
        _stream(stream)))


def release_stream(stream=None) -> None:
    """Hand back the library decode workspace bound to `stream`
    (b64x_release_stream).  Required before the stream's handle is destroyed
    if it decoded without a workspace of its own: a later takeover of the
    workspace records an event on the handle it is bound to.  torch's own
    streams (torch.cuda.Stream(), the default stream) come from pools that
    live as long as the process, so this matters for handles wrapped with
    torch.cuda.ExternalStream whose owner destroys them; for the others it
    only frees the workspace at once instead of when the least recently used
    one is taken over.  The next decode on the stream binds one again; work
    already queued is not affected."""
    _lib.load().b64x_release_stream(_stream(stream))


def fill_splitmix64(x: torch.Tensor, seed: int, stream=None) -> torch.Tensor:
    """Fill a device buffer with the synthetic splitmix64 byte stream."""
    lib = _lib.load()
    _u8(x, "buffer")
    _lib.check("b64x_fill_splitmix64", lib.b64x_fill_splitmix64(
        _ptr(x), x.numel(), seed, _stream(stream)))
    return x


def device_numa_node(device: int = -1) -> int:
    """The NUMA node the GPU hangs off (b64x_device_numa_node); negative
    errno when unknown."""
    return _lib.load().b64x_device_numa_node(device)


def bind_thread(device: int = -1) -> int:
    """Bind the calling thread to the GPU's NUMA node (b64x_bind_thread):
    threads it starts afterwards inherit the mask.  Returns the node or a
    negative errno (the thread unchanged)."""
    return _lib.load().b64x_bind_thread(device)


def device_check() -> None:
    """Raise unless a gfx950 device is usable by the library."""
    _lib.check("b64x_device_check", _lib.load().b64x_device_check())


def build_info() -> str:
    return _lib.load().b64x_build_info().decode()
