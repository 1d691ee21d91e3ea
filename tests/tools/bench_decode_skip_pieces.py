#!/usr/bin/env python3
"""Timing of the strict skip decode of texts that arrive in pieces
(b64.decode_strict_skip_pieces); a tool of its own, not a part of bench.py.
Writes profiles/r12_skip_pieces.json.

  strided  64 Ki x 5,608-byte CRLF-76 pieces, 4 KiB of payload each, 256 MiB
           in all; yardstick decode_strict_skip_strided on the same bytes:
           the same walk, less the 128 bytes of state read and written per
           piece
  ragged   the 136,411-buffer set of bench_lines_batch.py (about 1 GiB of
           payload, 16 B .. 64 KiB); yardstick decode_strict_skip_batch on
           the same bytes (two kernels, the text read twice)

Every piece is a whole text: final, on a zeroed state, which the call leaves
zeroed, so every repetition does the same work.  Three legs on each shape, in
one process, on the same text:
  (a) the new call, decoding         decode_strict_skip_pieces
  (b) the new call, validate only    decode_strict_skip_pieces, no output
  (c) the yardstick, decoding

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Records and bytes are checked
before anything is timed.  The legs are timed twice, the second time in the
opposite order; the smaller median counts and the difference between the two
shows the run-to-run spread.

    python tests/tools/bench_decode_skip_pieces.py [--steps 20] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402,F401  (preheat, through bench_lines_batch.timed)
from async_amd import b64  # noqa: E402
from bench_lines_batch import timed, wrapped_multiple_of_4  # noqa: E402

L, SEP = 76, b"\r\n"
REC = 24


def records_ok(res: torch.Tensor, lens) -> bool:
    """Every record is {len_i, 0, OK}."""
    r = res.cpu().numpy().reshape(-1, REC)
    out_len = r[:, :8].copy().view(np.uint64).ravel()
    return bool(np.array_equal(out_len, np.asarray(lens, np.uint64)) and not r[:, 8:].any())


def legs(fns: dict, steps: int, payload: int, text_bytes: int, npieces: int) -> dict:
    """Each leg's median, forwards and then backwards; the smaller counts."""
    first = {k: timed(f, steps) for k, f in fns.items()}
    second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
    out = {}
    for k in fns:
        ms = min(first[k], second[k])
        out[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                  "order_spread_ms": abs(first[k] - second[k]),
                  "payload_GiBps": payload / ms / 1e-3 / 2**30,
                  "text_GBps": text_bytes / ms / 1e-3 / 1e9}
    a, c = out["a_pieces_decode"], out["c_yardstick_decode"]
    out["a_over_c"] = a["ms"] / c["ms"]
    # what the states add to leg (a)'s traffic: 128 bytes read and written per piece
    out["state_bytes_moved"] = 2 * b64.SKIP_STATE_BYTES * npieces
    out["state_share_of_bytes_moved"] = out["state_bytes_moved"] / (
        text_bytes + payload + out["state_bytes_moved"])
    return out


def check(fns, out, res, lens, same) -> None:
    for k, f in fns.items():
        out.zero_()
        res.fill_(0xA5)
        f()
        torch.cuda.synchronize()
        ok = records_ok(res, lens)
        if k != "b_pieces_validate":
            ok = ok and same(k)
        if not ok:
            raise AssertionError(f"{k}: wrong records or bytes")


def strided(nbuf: int, n: int, steps: int) -> dict:
    dev = "cuda"
    W = b64.encoded_lines_len(n, L, SEP, True)
    stride = (b64.skip_piece_cap(W) + 3) // 4 * 4
    x = torch.empty(nbuf * n, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    text = torch.empty(nbuf * W, dtype=torch.uint8, device=dev)
    b64.encode_lines_strided(x, n, n, nbuf, text, W, L, SEP, True)
    out = torch.empty(nbuf * stride, dtype=torch.uint8, device=dev)
    res = torch.empty(REC * nbuf, dtype=torch.uint8, device=dev)
    in_off = torch.arange(nbuf + 1, dtype=torch.int64, device=dev) * W
    out_off = torch.arange(nbuf, dtype=torch.int64, device=dev) * stride
    states = b64.skip_states(nbuf, dev)
    final = torch.ones(nbuf, dtype=torch.uint8, device=dev)
    fns = {
        "a_pieces_decode": lambda: b64.decode_strict_skip_pieces(text, in_off, out, out_off, states,
                                                                 res, final=final),
        "b_pieces_validate": lambda: b64.decode_strict_skip_pieces(text, in_off, None, None, states,
                                                                   res, final=final),
        "c_yardstick_decode": lambda: b64.decode_strict_skip_strided(text, W, W, nbuf, out, stride,
                                                                     res),
    }
    check(fns, out, res, [n] * nbuf,
          lambda k: torch.equal(out.view(nbuf, stride)[:, :n], x.view(nbuf, n)))
    if bool(states.any()):
        raise AssertionError("a final piece left its state armed")
    r = {"shape": "strided", "pieces": nbuf, "piece_bytes": W, "piece_payload": n,
         "out_stride": stride, "payload_bytes": nbuf * n, "text_bytes": nbuf * W, "steps": steps,
         "yardstick": "decode_strict_skip_strided"}
    r.update(legs(fns, steps, nbuf * n, nbuf * W, nbuf))
    return r


def ragged(mib: int, steps: int) -> dict:
    dev = "cuda"
    rng = np.random.default_rng(0xB64)
    target = mib << 20
    draw = np.exp(rng.uniform(np.log(16), np.log(65536), int(target / 7000) + 64))
    lens = wrapped_multiple_of_4((draw.astype(np.int64) + 3) // 4 * 4)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), target)) + 1]
    nbuf = lens.size
    in_off_h = np.zeros(nbuf + 1, np.int64)
    np.cumsum(lens, out=in_off_h[1:])
    in_off = torch.from_numpy(in_off_h).to(dev)
    x = torch.empty(int(in_off_h[-1]), dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    t_off = b64.lines_batch_layout(in_off, L, SEP, True)
    text = torch.empty(int(t_off[-1]), dtype=torch.uint8, device=dev)
    b64.encode_lines_batch(x, in_off, text, t_off[:-1], L, SEP, True)
    o_off = b64.skip_pieces_layout(t_off, align=4)
    out = torch.empty(int(o_off[-1]), dtype=torch.uint8, device=dev)
    res = torch.empty(REC * nbuf, dtype=torch.uint8, device=dev)
    ws = torch.zeros(8 * nbuf, dtype=torch.uint8, device=dev)
    states = b64.skip_states(nbuf, dev)
    final = torch.ones(nbuf, dtype=torch.uint8, device=dev)
    fns = {
        "a_pieces_decode": lambda: b64.decode_strict_skip_pieces(text, t_off, out, o_off[:-1],
                                                                 states, res, final=final),
        "b_pieces_validate": lambda: b64.decode_strict_skip_pieces(text, t_off, None, None, states,
                                                                   res, final=final),
        "c_yardstick_decode": lambda: b64.decode_strict_skip_batch(text, t_off, out, o_off[:-1], res,
                                                                   workspace=ws),
    }
    picks = sorted({0, nbuf - 1, int(np.argmax(lens)), int(np.argmin(lens)),
                    *np.random.default_rng(1).integers(0, nbuf, 12).tolist()})
    o = o_off.cpu().numpy()

    def same(k):
        return all(torch.equal(out[int(o[i]):int(o[i]) + int(lens[i])],
                               x[int(in_off_h[i]):int(in_off_h[i + 1])]) for i in picks)
    check(fns, out, res, lens, same)
    if bool(states.any()):
        raise AssertionError("a final piece left its state armed")
    payload, chars = int(lens.sum()), int(t_off[-1])
    r = {"shape": "ragged", "pieces": int(nbuf), "payload_bytes": payload, "text_bytes": chars,
         "steps": steps, "yardstick": "decode_strict_skip_batch",
         "lengths": {"min": int(lens.min()), "max": int(lens.max()), "median": int(np.median(lens)),
                     "law": "the set of bench_lines_batch.py: log-uniform 16 B..64 KiB"}}
    r.update(legs(fns, steps, payload, chars, nbuf))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_skip_pieces.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_skip_pieces.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    for name, run in (("pieces_64Ki_x_5608", lambda: strided(1 << 16, 4096, args.steps)),
                      ("ragged", lambda: ragged(args.mib, args.steps))):
        result[name] = run()
        print(json.dumps({name: result[name]}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
