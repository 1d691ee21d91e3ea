#!/usr/bin/env python3
"""Timing of the strict skip decode of one large piece
(b64.decode_strict_skip_piece); a tool of its own, not a part of bench.py.
Writes profiles/r13_skip_wide.json.

CRLF-76 text of 64 KiB, 1 MiB, 8 MiB, 64 MiB and 1 GiB of payload, decoding
and validate only, and of 4 KiB and 16 KiB to find where legs (a) and (b)
cross.  Every call is a final piece on a zeroed state, which the
call leaves zeroed, so every repetition does the same work.  Three legs, in
one process, on the same text:
  (a) the wide call                    decode_strict_skip_piece
  (b) the pieces call on that one piece, up to 64 MiB (it runs at one wave's
      rate)                            decode_strict_skip_pieces
  (c) the whole-text call              decode_strict_skip

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Records and bytes are checked
before anything is timed.  The legs are timed twice, the second time in the
opposite order; the smaller median counts and the difference between the two
shows the run-to-run spread.  No figure of (a) is compared with (a).

    python tests/tools/bench_decode_skip_wide.py [--steps 20] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402,F401  (preheat, through bench_lines_batch.timed)
from async_amd import b64  # noqa: E402
from bench_lines_batch import timed  # noqa: E402

L, SEP = 76, b"\r\n"
REC = 24
PIECES_LIMIT = 64 << 20  # leg (b) walks the piece in one wave


def record(res: torch.Tensor):
    r = res.cpu().numpy()
    return int(r[:8].view("<u8")[0]), int(r[8:16].view("<u8")[0]), int(r[16:20].view("<u4")[0])


def one_size(n: int, steps: int) -> dict:
    dev = "cuda"
    x = torch.empty(n, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    text = b64.encode_lines(x)
    W = text.numel()
    assert W == b64.encoded_lines_len(n, L, SEP, True)
    out = torch.empty(b64.skip_piece_cap(W), dtype=torch.uint8, device=dev)
    res = torch.empty(REC, dtype=torch.uint8, device=dev)
    state = b64.skip_states(1, dev)
    ws_a = torch.empty(b64.strict_skip_piece_workspace_size(W), dtype=torch.uint8, device=dev)
    ws_c = torch.zeros(b64.strict_skip_workspace_size(W), dtype=torch.uint8, device=dev)
    in_off = torch.tensor([0, W], dtype=torch.int64, device=dev)
    out_off = torch.zeros(1, dtype=torch.int64, device=dev)
    final = torch.ones(1, dtype=torch.uint8, device=dev)
    r = {"payload_bytes": n, "text_bytes": W, "steps": steps,
         "workspace_bytes": {"a_wide": ws_a.numel(), "c_whole_text": ws_c.numel()}}
    for mode in ("decode", "validate"):
        o = out if mode == "decode" else None
        fns = {"a_wide": lambda: b64.decode_strict_skip_piece(text, state, res, out=o, final=True,
                                                              workspace=ws_a)}
        if n <= PIECES_LIMIT:
            fns["b_pieces"] = lambda: b64.decode_strict_skip_pieces(
                text, in_off, o, None if o is None else out_off, state, res, final=final)
        fns["c_whole_text"] = lambda: b64.decode_strict_skip(
            text, out=out, validate_only=o is None, workspace=ws_c, result=res)
        for k, f in fns.items():
            out.zero_()
            res.fill_(0xA5)
            f()
            torch.cuda.synchronize()
            if record(res) != (n, 0, 0) or bool(state.any()):
                raise AssertionError(f"{k} {mode}: wrong record or an armed state")
            if o is not None and not torch.equal(out[:n], x):
                raise AssertionError(f"{k} {mode}: wrong bytes")
        first = {k: timed(f, steps) for k, f in fns.items()}
        second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
        legs = {}
        moved = {"a_wide": (2 * W + n) if o is not None else W}
        for k in fns:
            ms = min(first[k], second[k])
            legs[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                       "order_spread_ms": abs(first[k] - second[k]),
                       "payload_GiBps": n / ms / 1e-3 / 2**30, "text_GBps": W / ms / 1e-3 / 1e9}
            if k in moved:
                legs[k]["bytes_moved"] = moved[k]
                legs[k]["moved_GBps"] = moved[k] / ms / 1e-3 / 1e9
        if "b_pieces" in legs:
            legs["b_over_a"] = legs["b_pieces"]["ms"] / legs["a_wide"]["ms"]
        legs["a_over_c"] = legs["a_wide"]["ms"] / legs["c_whole_text"]["ms"]
        r[mode] = legs
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*",
                    default=[4 << 10, 16 << 10, 64 << 10, 1 << 20, 8 << 20, 64 << 20, 1 << 30])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_skip_wide.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_skip_wide.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts",
              "sizes": {}}
    for n in args.sizes:
        result["sizes"][str(n)] = one_size(n, args.steps)
        print(json.dumps({str(n): result["sizes"][str(n)]}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
