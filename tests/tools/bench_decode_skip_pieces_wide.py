#!/usr/bin/env python3
"""Timing of the strict skip decode of many pieces of any size in one call
(b64.decode_strict_skip_pieces_wide); a tool of its own, not a part of bench.py.
Writes profiles/r14_skip_pieces_wide.json.

Five shapes of CRLF-76 text, each decoding and validate only.  Every piece is
a whole text: final, on a zeroed state, which every call leaves zeroed, so
every repetition does the same work.  The yardsticks are timed in the same
process on the same bytes:
  a_ragged     the 136,411-buffer set of bench_lines_batch.py (60 B .. 64 KiB)
               against decode_strict_skip_pieces and decode_strict_skip_batch
  b_64Ki_x_4K  64 Ki pieces of 5,608 bytes against decode_strict_skip_pieces
  c_1M_x_1K    1 Mi pieces of 1,404 bytes against decode_strict_skip_pieces:
               what prep's prefix over a million pieces costs
  d_16_x_8M, d_600_x_1M   large pieces against a loop of
               decode_strict_skip_piece calls on one stream and against
               decode_strict_skip_pieces
  e_mix        1 x 8 MiB + 15 x 1 MiB + 2,000 x 4 KiB of payload against the
               routing the other calls allow: decode_strict_skip_pieces for
               the small pieces plus one decode_strict_skip_piece per large one

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Records and bytes are checked
before anything is timed.  The legs are timed twice, the second time in the
opposite order; the smaller median counts and the difference between the two
shows the run-to-run spread.  No figure of the new call is compared with
itself.

    python tests/tools/bench_decode_skip_pieces_wide.py [--steps 20] [--out PATH]
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
STATE = b64.SKIP_STATE_BYTES
LARGE = 256 << 10  # payload bytes from which the routed legs give a piece a call of its own


def records_ok(res: torch.Tensor, lens) -> bool:
    """Every record is {len_i, 0, OK}."""
    r = res.cpu().numpy().reshape(-1, REC)
    out_len = r[:, :8].copy().view(np.uint64).ravel()
    return bool(np.array_equal(out_len, np.asarray(lens, np.uint64)) and not r[:, 8:].any())


def ragged_lens(mib: int) -> np.ndarray:
    """The set of bench_lines_batch.py: log-uniform 16 B .. 64 KiB, raised to
    lengths whose CRLF-76 text is a multiple of 4 bytes (60 B at the least)."""
    rng = np.random.default_rng(0xB64)
    target = mib << 20
    draw = np.exp(rng.uniform(np.log(16), np.log(65536), int(target / 7000) + 64))
    lens = wrapped_multiple_of_4((draw.astype(np.int64) + 3) // 4 * 4)
    return lens[:int(np.searchsorted(np.cumsum(lens), target)) + 1]


def shape(name: str, lens: np.ndarray, steps: int, batch: bool = False, loop: bool = False,
          routed: bool = False) -> dict:
    """The new call and the pieces call over pieces of `lens` payload bytes;
    batch: decode_strict_skip_batch too; loop: a one-piece call per piece;
    routed: the pieces call for the pieces below LARGE (which come first) and
    a one-piece call for each of the others."""
    dev = "cuda"
    lens = wrapped_multiple_of_4(np.asarray(lens, np.int64))
    n = int(lens.size)
    in_off_h = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=in_off_h[1:])
    in_off = torch.from_numpy(in_off_h).to(dev)
    x = torch.empty(int(in_off_h[-1]), dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    t_off = b64.lines_batch_layout(in_off, L, SEP, True)
    text = torch.empty(int(t_off[-1]), dtype=torch.uint8, device=dev)
    b64.encode_lines_batch(x, in_off, text, t_off[:-1], L, SEP, True)
    o_off = b64.skip_pieces_layout(t_off, align=4)
    out = torch.empty(int(o_off[-1]), dtype=torch.uint8, device=dev)
    res = torch.empty(REC * n, dtype=torch.uint8, device=dev)
    states = b64.skip_states(n, dev)
    final = torch.ones(n, dtype=torch.uint8, device=dev)
    W = text.numel()
    ws = torch.empty(b64.strict_skip_pieces_wide_workspace_size(W, n), dtype=torch.uint8, device=dev)
    t_h, o_h = t_off.cpu().numpy(), o_off.cpu().numpy()
    nsmall = int((lens < LARGE).sum())
    if routed and not (lens[:nsmall] < LARGE).all():
        raise AssertionError("the routed leg wants the small pieces first")
    singles = list(range(n)) if loop else list(range(nsmall, n)) if routed else []
    # the one-piece calls' views, cut once: a call costs its three launches, not the slicing
    views = [(text[int(t_h[i]):int(t_h[i + 1])], states[STATE * i:STATE * (i + 1)],
              res[REC * i:REC * (i + 1)],
              out[int(o_h[i]):int(o_h[i]) + b64.skip_piece_cap(int(t_h[i + 1] - t_h[i]))])
             for i in singles]
    ws_one = torch.empty(b64.strict_skip_piece_workspace_size(int(np.diff(t_h).max())),
                         dtype=torch.uint8, device=dev) if singles else None
    ws_batch = torch.zeros(8 * n, dtype=torch.uint8, device=dev) if batch else None

    def one_by_one(o):
        for t, s, r, w in views:
            b64.decode_strict_skip_piece(t, s, r, out=w if o is not None else None, final=True,
                                         workspace=ws_one)

    def route(o):
        if nsmall:
            b64.decode_strict_skip_pieces(text, t_off[:nsmall + 1], o,
                                          None if o is None else o_off[:nsmall], states, res,
                                          final=final)
        one_by_one(o)
    picks = sorted({0, n - 1, int(np.argmax(lens)), int(np.argmin(lens)),
                    *np.random.default_rng(1).integers(0, n, 12).tolist()})
    r = {"pieces": n, "payload_bytes": int(lens.sum()), "text_bytes": W, "steps": steps,
         "workspace_bytes": ws.numel(),
         "lengths": {"min": int(lens.min()), "max": int(lens.max()), "median": int(np.median(lens))}}
    for mode in ("decode", "validate"):
        o = out if mode == "decode" else None
        oo = None if o is None else o_off[:-1]
        fns = {"new_pieces_wide": lambda: b64.decode_strict_skip_pieces_wide(
                   text, t_off, o, oo, states, res, ws, total_cap=W, flags=final),
               "pieces": lambda: b64.decode_strict_skip_pieces(text, t_off, o, oo, states, res,
                                                               final=final)}
        if batch and o is not None:
            fns["batch"] = lambda: b64.decode_strict_skip_batch(text, t_off, out, o_off[:-1], res,
                                                                workspace=ws_batch)
        if loop:
            fns["one_piece_loop"] = lambda: one_by_one(o)
        if routed:
            fns["routed"] = lambda: route(o)
        for k, f in fns.items():
            out.zero_()
            res.fill_(0xA5)
            f()
            torch.cuda.synchronize()
            ok = records_ok(res, lens) and not bool(states.any())
            if o is not None:
                ok = ok and all(torch.equal(out[int(o_h[i]):int(o_h[i]) + int(lens[i])],
                                            x[int(in_off_h[i]):int(in_off_h[i + 1])]) for i in picks)
            if not ok:
                raise AssertionError(f"{name} {mode} {k}: wrong records, bytes or states")
        first = {k: timed(f, steps) for k, f in fns.items()}
        second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
        legs = {}
        for k in fns:
            ms = min(first[k], second[k])
            legs[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                       "order_spread_ms": abs(first[k] - second[k]),
                       "payload_GiBps": int(lens.sum()) / ms / 1e-3 / 2**30,
                       "text_GBps": W / ms / 1e-3 / 1e9}
        for k in fns:
            if k != "new_pieces_wide":
                legs["new_over_" + k] = legs["new_pieces_wide"]["ms"] / legs[k]["ms"]
        r[mode] = legs
    return r


def crossover(steps: int) -> dict:
    """2,048 pieces of one size each, 2 KiB .. 256 KiB of payload: the size at
    which the new call passes the pieces call."""
    out = {}
    for kib in (2, 4, 8, 16, 32, 64, 128, 256):
        r = shape(f"x_{kib}K", np.full(2048, kib << 10), steps)
        out[str(kib << 10)] = {m: {"new_ms": r[m]["new_pieces_wide"]["ms"], "pieces_ms": r[m]["pieces"]["ms"],
                                   "new_over_pieces": r[m]["new_over_pieces"]}
                               for m in ("decode", "validate")}
        out[str(kib << 10)]["piece_text_bytes"] = r["text_bytes"] // 2048
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_skip_pieces_wide.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_skip_pieces_wide.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    s = args.steps
    mix = np.concatenate([np.full(2000, 4 << 10), np.full(15, 1 << 20), np.full(1, 8 << 20)])
    runs = (("a_ragged", lambda: shape("a", ragged_lens(args.mib), s, batch=True)),
            ("b_64Ki_x_4K", lambda: shape("b", np.full(1 << 16, 4096), s)),
            ("c_1M_x_1K", lambda: shape("c", np.full(1 << 20, 1024), s)),
            ("d_16_x_8M", lambda: shape("d16", np.full(16, 8 << 20), s, loop=True)),
            ("d_600_x_1M", lambda: shape("d600", np.full(600, 1 << 20), s, loop=True)),
            ("e_mix", lambda: shape("e", mix, s, routed=True)),
            ("crossover_2048_pieces", lambda: crossover(s)))
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
