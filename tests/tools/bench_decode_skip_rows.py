#!/usr/bin/env python3
"""Timing of the one-pass strict skip decode of strided rows
(b64.decode_strict_skip_strided); a tool of its own, not a part of bench.py.
Writes profiles/r11_skip_rows.json.

  1 M x 1,404-byte CRLF-76 rows    1 KiB of payload each, 1 GiB in all
  64 Ki x 5,608-byte CRLF-76 rows  4 KiB of payload each, 256 MiB in all

Rows at 4-byte aligned addresses on both sides (in_stride = the row's length,
out_stride = its decode capacity rounded up to 4).  Four legs on each shape,
in one process, on the same text:
  (a) the new call, decoding         decode_strict_skip_strided
  (b) the new call, validate only    decode_strict_skip_strided, no output
  (c) the route there was before     decode_strict_skip_batch with
                                     in_off = i*in_stride (two kernels, the
                                     text read twice, 8 bytes of workspace
                                     per row)
  (d) the canonical-format yardstick decode_strict_strided on the same rows:
                                     the same text read, the same payload
                                     written

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Records and bytes are checked
before anything is timed.  The legs are timed twice, the second time in the
opposite order; the smaller median counts and the difference between the two
shows the run-to-run spread.  The copy ceiling is a device-to-device copy that
moves as many bytes (read + written) as leg (a): the text once and the payload.

    python tests/tools/bench_decode_skip_rows.py [--steps 20] [--out PATH]
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
from bench_lines_batch import timed  # noqa: E402

L, SEP = 76, b"\r\n"
REC = 24


def records_ok(res: torch.Tensor, nbuf: int, n: int) -> bool:
    """Every record is {n, 0, OK}."""
    r = res.cpu().numpy()[:REC * nbuf].reshape(nbuf, REC)
    return bool((r[:, :8].copy().view(np.uint64) == n).all() and not r[:, 8:].any())


def shape(nbuf: int, n: int, steps: int) -> dict:
    dev = "cuda"
    W = b64.encoded_lines_len(n, L, SEP, True)
    cap = b64.decoded_cap(W)
    out_stride = (cap + 3) // 4 * 4
    assert W % 4 == 0 and out_stride >= b64.strict_decoded_cap(W, L, SEP, True)
    x = torch.empty(nbuf * n, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    text = torch.empty(nbuf * W, dtype=torch.uint8, device=dev)
    b64.encode_lines_strided(x, n, n, nbuf, text, W, L, SEP, True)
    out = torch.empty(nbuf * out_stride, dtype=torch.uint8, device=dev)
    res = torch.empty(REC * nbuf, dtype=torch.uint8, device=dev)
    in_off = torch.arange(nbuf + 1, dtype=torch.int64, device=dev) * W
    out_off = torch.arange(nbuf, dtype=torch.int64, device=dev) * out_stride
    ws = torch.zeros(8 * nbuf, dtype=torch.uint8, device=dev)
    fns = {
        "a_skip_rows_decode": lambda: b64.decode_strict_skip_strided(text, W, W, nbuf, out, out_stride,
                                                                     res),
        "b_skip_rows_validate": lambda: b64.decode_strict_skip_strided(text, W, W, nbuf, None, 0, res),
        "c_skip_batch_decode": lambda: b64.decode_strict_skip_batch(text, in_off, out, out_off, res,
                                                                    workspace=ws),
        "d_strict_strided": lambda: b64.decode_strict_strided(text, W, W, nbuf, out, out_stride, res,
                                                              L, SEP, True),
    }
    want = x.view(nbuf, n)
    for k, f in fns.items():
        out.zero_()
        res.fill_(0xA5)
        f()
        torch.cuda.synchronize()
        ok = records_ok(res, nbuf, n)
        if k != "b_skip_rows_validate":
            ok = ok and torch.equal(out.view(nbuf, out_stride)[:, :n], want)
        if not ok:
            raise AssertionError(f"{k}: wrong records or bytes")
    # the copy ceiling for leg (a)'s bytes
    moved = nbuf * (W + n)
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = min(timed(lambda: dst.copy_(src), steps), timed(lambda: dst.copy_(src), steps))
    del src, dst
    first = {k: timed(f, steps) for k, f in fns.items()}
    second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
    r = {"rows": nbuf, "row_bytes": W, "row_payload": n, "in_stride": W, "out_stride": out_stride,
         "payload_bytes": nbuf * n, "text_bytes": nbuf * W, "steps": steps}
    for k in fns:
        ms = min(first[k], second[k])
        r[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                "order_spread_ms": abs(first[k] - second[k]),
                "payload_GiBps": nbuf * n / ms / 1e-3 / 2**30,
                "text_GBps": nbuf * W / ms / 1e-3 / 1e9}
    a, c, d = r["a_skip_rows_decode"], r["c_skip_batch_decode"], r["d_strict_strided"]
    r["copy_ceiling"] = {"bytes_moved": moved, "ms": copy_ms, "GBps": moved / copy_ms / 1e-3 / 1e9}
    r["a_moved_GBps"] = moved / a["ms"] / 1e-3 / 1e9
    r["a_share_of_copy_ceiling"] = copy_ms / a["ms"]
    r["a_over_c"] = a["ms"] / c["ms"]
    r["a_over_d"] = a["ms"] / d["ms"]
    # required: (a) below (c) by more than the two orders' medians differ
    r["a_below_c_by_ms"] = c["ms"] - a["ms"]
    r["a_below_c_beyond_spread"] = bool(
        c["ms"] - a["ms"] > max(a["order_spread_ms"], c["order_spread_ms"]))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_skip_rows.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_skip_rows.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    for name, nbuf, n in (("rows_1Mi_x_1404", 1 << 20, 1024), ("rows_64Ki_x_5608", 1 << 16, 4096)):
        result[name] = shape(nbuf, n, args.steps)
        print(json.dumps({name: result[name]}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
