#!/usr/bin/env python3
"""Timing of the ragged strict decode balanced over bytes
(b64.decode_strict_batch_wide); a tool of its own, not a part of bench.py.
Writes profiles/r16_decode_strict_batch_wide.json.

Five batches, each plain and CRLF-76 (trailing):
  1_hub         1 x 8 MiB + 15 x 1 MiB + 2,000 x 4 KiB, and the same with one
                offence in its last text
  2_600_x_1M    600 texts of 1 MiB of payload
  3_ragged      the 136,411-text set of bench_lines_batch.py (60 B .. 64 KiB)
  4_1M_x_1K     1 Mi texts of 1 KiB of payload
  5_crossing    2,048 equal texts of 4 KiB .. 1 MiB: where the two calls cross
Every timing is taken on the new call (total_hint = the arena's bytes, and 0)
and on the existing ragged call (decode_strict_batch) on the same tensors, and
beside the one-buffer call (decode_strict) on one text of the same payload.
The texts are written by encode_batch_wide; payload lengths are multiples of 4
whose CRLF-76 text is one too, packed tight, and the outputs start on dwords:
every text is dword aligned on both sides in both forms.

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  The new call's records and bytes
are compared with the existing ragged call's before anything is timed.  The
legs are timed twice, the second time in the opposite order; the smaller
median counts and the difference between the two shows the run-to-run spread.

    python tests/tools/bench_decode_strict_batch_wide.py [--steps 20] [--out PATH]
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
REC = b64.STRICT_RES_BYTES


def shape(name: str, lens: np.ndarray, steps: int, offence: bool = False) -> dict:
    dev = "cuda"
    lens = wrapped_multiple_of_4(np.asarray(lens, np.int64))
    n = int(lens.size)
    in_off_h = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=in_off_h[1:])
    total = int(in_off_h[-1])
    in_off = torch.from_numpy(in_off_h).to(dev)
    x = torch.empty(total, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    r = {"texts": n, "payload_bytes": total, "steps": steps,
         "lengths": {"min": int(lens.min()), "max": int(lens.max()), "median": int(np.median(lens))}}
    for form in ("plain", "crlf76"):
        if form == "plain":
            t_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum((in_off[1:] - in_off[:-1] + 2) // 3 * 4, 0, out=t_off[1:])
            fmt = ()
        else:
            t_off = b64.lines_batch_layout(in_off, L, SEP, True)
            fmt = (L, SEP, True)
        d_off = b64.strict_batch_layout(t_off, *(fmt or (None,)), align=4)
        if bool((t_off % 4).any()) or bool((d_off % 4).any()):
            raise AssertionError("a text or an output is not dword aligned")
        size = int(t_off[-1])
        text = torch.empty(size, dtype=torch.uint8, device=dev)
        b64.encode_batch_wide(x, in_off, text, t_off[:-1], *fmt, total_hint=total)
        # one text of the same payload for the one-buffer call
        one_text = (b64.encode_lines(x, *fmt) if fmt else b64.encode(x)).clone()
        if offence:  # one byte that is no character, in the middle of the last text
            last = int(t_off[-2])
            text[last + (size - last) // 2 // 78 * 78 + 8] = 0x2A
        cap = int(d_off[-1])
        new = torch.empty(cap, dtype=torch.uint8, device=dev)
        old = torch.empty(cap, dtype=torch.uint8, device=dev)
        one = torch.empty(b64.strict_decoded_cap(one_text.numel(), *(fmt or (None,))) + 16,
                          dtype=torch.uint8, device=dev)
        res_new = torch.empty(REC * n, dtype=torch.uint8, device=dev)
        res_old = torch.empty(REC * n, dtype=torch.uint8, device=dev)
        res_one = torch.empty(REC, dtype=torch.uint8, device=dev)
        dd = d_off[:-1]
        ll = fmt or (None,)
        fns = {"new_wide": lambda: b64.decode_strict_batch_wide(text, t_off, new, dd, res_new, *ll,
                                                                total_hint=size),
               "new_wide_hint0": lambda: b64.decode_strict_batch_wide(text, t_off, new, dd,
                                                                      res_new, *ll, total_hint=0),
               "ragged": lambda: b64.decode_strict_batch(text, t_off, old, dd, res_old, *ll),
               "one_buffer": lambda: b64.decode_strict(one_text, *ll, out=one, result=res_one)}
        for k in ("new_wide", "new_wide_hint0"):
            new.fill_(0xA5)
            old.fill_(0xA5)
            res_new.fill_(0xA5)
            fns[k]()
            fns["ragged"]()
            torch.cuda.synchronize()
            if not torch.equal(res_new, res_old):
                raise AssertionError(f"{name} {form} {k}: records differ from the existing call's")
            recs = res_new.cpu().numpy().view(np.uint64).reshape(n, 3)
            bad = np.flatnonzero(recs[:, 2])
            if bad.tolist() != ([n - 1] if offence else []):
                raise AssertionError(f"{name} {form} {k}: refused texts {bad[:8].tolist()}")
            if not offence:
                if not torch.equal(new, old):
                    raise AssertionError(f"{name} {form} {k}: bytes differ from the existing call's")
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
        del text, one_text, new, old, one
    return r


def crossing(steps: int) -> dict:
    """2,048 texts of one size each: the size at which the new call passes
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
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "r16_decode_strict_batch_wide.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_strict_batch_wide.py",
              "formats": "plain (padded) and CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    s = args.steps
    hub = np.concatenate([np.full(1, 8 << 20), np.full(15, 1 << 20), np.full(2000, 4 << 10)])
    np.random.default_rng(0xB64).shuffle(hub)
    runs = (("1_hub", lambda: shape("hub", hub, s)),
            ("1_hub_one_offence_in_last_text", lambda: shape("hub_offence", hub, s, offence=True)),
            ("2_600_x_1M", lambda: shape("600", np.full(600, 1 << 20), s)),
            ("3_ragged", lambda: shape("ragged", ragged_lens(args.mib), s)),
            ("4_1M_x_1K", lambda: shape("1M", np.full(1 << 20, 1024), s)),
            ("5_crossing_2048_texts", lambda: crossing(s)))
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
