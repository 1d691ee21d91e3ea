#!/usr/bin/env python3
"""Timing of the strict decode that skips line breaks (b64.decode_strict_skip /
b64.decode_strict_skip_batch); a tool of its own, not a part of bench.py.
Writes profiles/r10_decode_skip.json.

  one buffer  1 GiB of payload as CRLF-76 text
  ragged      the 136,411-buffer set of bench_lines_batch.py (about 1 GiB of
              payload, log-uniform 16 B..64 KiB), as CRLF-76 texts packed tight

Four legs on each, in one process, on the same text:
  (a) the decoding call                  decode_strict_skip[_batch]
  (b) the lenient decode of the text     decode / decode_batch, on the same
                                         workspace the decoding call hands it
  (c) validate only                      decode_strict_skip[_batch], no output
  (d) the strict decode of the same canonical text
                                         decode_strict / decode_strict_batch

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Records and bytes are checked
before anything is timed.  The legs are timed twice, the second time in the
opposite order, to show the run-to-run spread.

    python tests/tools/bench_decode_skip.py [--steps 20] [--mib 1024] [--out PATH]
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
    rest = r[:, 8:].copy().view(np.uint64)
    return bool(np.array_equal(out_len, np.asarray(lens, np.uint64)) and not rest.any())


def legs(fns: dict, steps: int, payload: int, text_bytes: int) -> dict:
    """Each leg's median, forwards and then backwards; the smaller counts."""
    first = {k: timed(f, steps) for k, f in fns.items()}
    second = {k: timed(fns[k], steps) for k in reversed(list(fns))}
    out = {}
    for k in fns:
        ms = min(first[k], second[k])
        out[k] = {"ms": ms, "ms_first": first[k], "ms_second": second[k],
                  "payload_GiBps": payload / ms / 1e-3 / 2**30,
                  "text_GBps": text_bytes / ms / 1e-3 / 1e9}
    out["a_over_b_plus_c"] = out["a_decode_strict_skip"]["ms"] / (
        out["b_lenient_decode"]["ms"] + out["c_validate_only"]["ms"])
    out["c_over_d"] = out["c_validate_only"]["ms"] / out["d_decode_strict"]["ms"]
    return out


def one_buffer(mib: int, steps: int) -> dict:
    dev = "cuda"
    n = mib << 20
    x = torch.empty(n, dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    text = b64.encode_lines(x, L, SEP)
    W = text.numel()
    out = torch.empty(b64.decoded_cap(W), dtype=torch.uint8, device=dev)
    res = torch.empty(REC, dtype=torch.uint8, device=dev)
    lres = torch.zeros(b64.RES_BYTES, dtype=torch.uint8, device=dev)
    ws = torch.zeros(b64.strict_skip_workspace_size(W), dtype=torch.uint8, device=dev)
    head = b64.strict_skip_workspace_size(W, True)
    fns = {
        "a_decode_strict_skip": lambda: b64.decode_strict_skip(text, out=out, workspace=ws, result=res),
        "b_lenient_decode": lambda: b64.decode(text, out=out, workspace=ws[head:], result=lres),
        "c_validate_only": lambda: b64.decode_strict_skip(text, validate_only=True, workspace=ws,
                                                          result=res),
        "d_decode_strict": lambda: b64.decode_strict(text, L, SEP, out=out, result=res),
    }
    for k, f in fns.items():
        out.zero_()
        res.fill_(0xA5)
        d = f()
        torch.cuda.synchronize()
        if k == "b_lenient_decode":
            ok = d.info().out_len == n
        else:
            ok = records_ok(res, [n])
        if k != "c_validate_only":
            ok = ok and torch.equal(out[:n], x)
        if not ok:
            raise AssertionError(f"{k}: wrong record or bytes")
    r = {"shape": "one buffer", "payload_bytes": n, "text_bytes": W, "steps": steps}
    r.update(legs(fns, steps, n, W))
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
    o_skip = b64.skip_batch_layout(t_off, align=4)
    o_strict = b64.strict_batch_layout(t_off, L, SEP, True, align=4)
    out = torch.empty(int(o_skip[-1]), dtype=torch.uint8, device=dev)
    res = torch.empty(REC * nbuf, dtype=torch.uint8, device=dev)
    outlen = torch.zeros(nbuf, dtype=torch.int64, device=dev)
    ws = outlen.view(torch.uint8)
    fns = {
        "a_decode_strict_skip": lambda: b64.decode_strict_skip_batch(
            text, t_off, out, o_skip[:-1], res, workspace=ws),
        "b_lenient_decode": lambda: b64.decode_batch(text, t_off, out, o_skip[:-1], outlen),
        "c_validate_only": lambda: b64.decode_strict_skip_batch(text, t_off, None, None, res),
        "d_decode_strict": lambda: b64.decode_strict_batch(
            text, t_off, out, o_strict[:-1], res, L, SEP, True),
    }
    picks = sorted({0, nbuf - 1, int(np.argmax(lens)), int(np.argmin(lens)),
                    *np.random.default_rng(1).integers(0, nbuf, 12).tolist()})
    for k, f in fns.items():
        out.zero_()
        res.fill_(0xA5)
        outlen.zero_()
        f()
        torch.cuda.synchronize()
        if k == "b_lenient_decode":
            ok = bool(np.array_equal(outlen.cpu().numpy(), lens))
        else:
            ok = records_ok(res, lens)
        if k != "c_validate_only":
            o = (o_strict if k == "d_decode_strict" else o_skip).cpu().numpy()
            for i in picks:
                ok = ok and torch.equal(out[int(o[i]):int(o[i]) + int(lens[i])],
                                        x[int(in_off_h[i]):int(in_off_h[i + 1])])
        if not ok:
            raise AssertionError(f"{k} (ragged): wrong records or bytes")
    payload, chars = int(lens.sum()), int(t_off[-1])
    r = {"shape": "ragged", "nbuf": int(nbuf), "payload_bytes": payload, "text_bytes": chars,
         "steps": steps,
         "lengths": {"min": int(lens.min()), "max": int(lens.max()), "median": int(np.median(lens)),
                     "law": "the set of bench_lines_batch.py: log-uniform 16 B..64 KiB"}}
    r.update(legs(fns, steps, payload, chars))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_decode_skip.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_decode_skip.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region; each leg "
                        "timed twice (the legs in opposite orders), the smaller median counts"}
    result["one_buffer"] = one_buffer(args.mib, args.steps)
    print(json.dumps({"one_buffer": result["one_buffer"]}), flush=True)
    torch.cuda.empty_cache()
    result["ragged"] = ragged(args.mib, args.steps)
    print(json.dumps({"ragged": result["ragged"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
