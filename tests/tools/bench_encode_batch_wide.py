#!/usr/bin/env python3
"""Timing of the ragged encode balanced over bytes (b64.encode_batch_wide); a
tool of its own, not a part of bench.py.  Writes
profiles/r15_encode_batch_wide.json.

Five batches, each plain and CRLF-76 (trailing):
  1_hub         1 x 8 MiB + 15 x 1 MiB + 2,000 x 4 KiB
  2_600_x_1M    600 buffers of 1 MiB
  3_ragged      the 136,411-buffer set of bench_lines_batch.py (60 B .. 64 KiB)
  4_1M_x_1K     1 Mi buffers of 1 KiB
  5_crossing    2,048 equal buffers of 4 KiB .. 1 MiB: where the two calls cross
Every timing is taken on the new call (total_hint = the arena's bytes, and 0)
and on the existing ragged call (encode_batch / encode_lines_batch) on the
same tensors, and beside the one-buffer call (encode / encode_lines) on the
same total bytes.  Lengths are multiples of 4 whose CRLF-76 text is one too,
packed tight: every buffer is dword aligned on both sides in both forms.

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  The new call's bytes are compared
with the existing ragged call's before anything is timed.  The legs are timed
twice, the second time in the opposite order; the smaller median counts and
the difference between the two shows the run-to-run spread.

    python tests/tools/bench_encode_batch_wide.py [--steps 20] [--out PATH]
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
from bench_decode_skip_pieces_wide import ragged_lens  # noqa: E402
from bench_lines_batch import timed, wrapped_multiple_of_4  # noqa: E402

L, SEP = 76, b"\r\n"


def shape(name: str, lens: np.ndarray, steps: int) -> dict:
    dev = "cuda"
    lens = wrapped_multiple_of_4(np.asarray(lens, np.int64))
    n = int(lens.size)
    in_off_h = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=in_off_h[1:])
    total = int(in_off_h[-1])
    in_off = torch.from_numpy(in_off_h).to(dev)
    x = torch.empty(total, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    r = {"buffers": n, "payload_bytes": total, "steps": steps,
         "lengths": {"min": int(lens.min()), "max": int(lens.max()), "median": int(np.median(lens))}}
    for form in ("plain", "crlf76"):
        if form == "plain":
            o_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum((in_off[1:] - in_off[:-1] + 2) // 3 * 4, 0, out=o_off[1:])
            fmt = ()
        else:
            o_off = b64.lines_batch_layout(in_off, L, SEP, True)
            fmt = (L, SEP, True)
        if bool((o_off % 4).any()):
            raise AssertionError("an output is not dword aligned")
        size = int(o_off[-1])
        new = torch.empty(size, dtype=torch.uint8, device=dev)
        old = torch.empty(size, dtype=torch.uint8, device=dev)
        one = torch.empty(size + 16, dtype=torch.uint8, device=dev)
        oo = o_off[:-1]
        fns = {"new_wide": lambda: b64.encode_batch_wide(x, in_off, new, oo, *fmt, total_hint=total),
               "new_wide_hint0": lambda: b64.encode_batch_wide(x, in_off, new, oo, *fmt,
                                                               total_hint=0)}
        if form == "plain":
            fns["ragged"] = lambda: b64.encode_batch(x, in_off, old, oo)
            fns["one_buffer"] = lambda: b64.encode(x, out=one)
        else:
            fns["ragged"] = lambda: b64.encode_lines_batch(x, in_off, old, oo, *fmt)
            fns["one_buffer"] = lambda: b64.encode_lines(x, *fmt, out=one)
        for k in ("new_wide", "new_wide_hint0"):
            new.fill_(0xA5)
            old.fill_(0xA5)
            fns[k]()
            fns["ragged"]()
            torch.cuda.synchronize()
            if not torch.equal(new, old):
                raise AssertionError(f"{name} {form} {k}: differs from the existing ragged call")
        first = {k: timed(f, steps) for k, f in fns.items()}
        second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
        legs = {"text_bytes": size}
        for k in fns:
            ms = min(first[k], second[k])
            legs[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                       "order_spread_ms": abs(first[k] - second[k]),
                       "payload_GiBps": total / ms / 1e-3 / 2**30}
        for k in ("ragged", "one_buffer"):
            legs["new_over_" + k] = legs["new_wide"]["ms"] / legs[k]["ms"]
        r[form] = legs
        del new, old, one
    return r


def crossing(steps: int) -> dict:
    """2,048 buffers of one size each: the size at which the new call passes
    the existing ragged one."""
    out = {}
    for kib in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        r = shape(f"x_{kib}K", np.full(2048, kib << 10), steps)
        out[str(kib << 10)] = {f: {"new_ms": r[f]["new_wide"]["ms"], "ragged_ms": r[f]["ragged"]["ms"],
                                   "one_buffer_ms": r[f]["one_buffer"]["ms"],
                                   "new_over_ragged": r[f]["new_over_ragged"]}
                               for f in ("plain", "crlf76")}
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_encode_batch_wide.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_encode_batch_wide.py",
              "formats": "plain (padded) and CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    s = args.steps
    hub = np.concatenate([np.full(1, 8 << 20), np.full(15, 1 << 20), np.full(2000, 4 << 10)])
    np.random.default_rng(0xB64).shuffle(hub)
    runs = (("1_hub", lambda: shape("hub", hub, s)),
            ("2_600_x_1M", lambda: shape("600", np.full(600, 1 << 20), s)),
            ("3_ragged", lambda: shape("ragged", ragged_lens(args.mib), s)),
            ("4_1M_x_1K", lambda: shape("1M", np.full(1 << 20, 1024), s)),
            ("5_crossing_2048_buffers", lambda: crossing(s)))
    for name, run in runs:
        if args.only and name not in args.only:
            continue
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
