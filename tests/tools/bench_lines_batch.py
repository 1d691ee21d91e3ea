#!/usr/bin/env python3
"""Timing of the ragged line-wrapped encode and strict decode
(b64.encode_lines_batch / b64.decode_strict_batch); a tool of its own, not a
part of bench.py.  Writes profiles/r09_lines_batch.json.

  uniform   1 Mi rows of 1 KiB as CRLF-76 through the batch calls, each timed
            next to encode_lines_strided / decode_strict_strided of the same
            rows in the same run (the strided code is the yardstick); the
            batch/strided ratio is recorded.
  ragged    about 1 GiB of payload in buffers log-uniform over 16 B..64 KiB,
            both calls: GiB/s of payload and the fraction of the copy ceiling
            of the same read/write mix (bench.copy_ceilings).

Clocks are pre-heated before every timed region and every figure is the
median of HIP-event times, as in bench.py.  Outputs are spot-checked against
the stdlib before anything is timed.

    python tests/tools/bench_lines_batch.py [--steps 20] [--rows 1048576]
                                            [--ragged-mib 1024] [--out PATH]
"""
from __future__ import annotations

import argparse
import base64
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (preheat, copy_ceilings)
from async_amd import b64  # noqa: E402

L, SEP = 76, b"\r\n"
REC = 24


def timed(fn, steps):
    ts = []
    bench.preheat()
    for i in range(steps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def text_of(data: bytes) -> bytes:
    c = base64.b64encode(data)
    return b"".join(c[i:i + L] + SEP for i in range(0, len(c), L))


def check_batch(x, in_off, text, t_off, dec, d_off, res, lens, picks):
    """A few buffers of the batch against the stdlib; every record OK."""
    h_in, h_t, h_d = in_off.cpu().numpy(), t_off.cpu().numpy(), d_off.cpu().numpy()
    for i in picks:
        data = x[int(h_in[i]):int(h_in[i + 1])].cpu().numpy().tobytes()
        want = text_of(data)
        got = text[int(h_t[i]):int(h_t[i]) + len(want)].cpu().numpy().tobytes()
        back = dec[int(h_d[i]):int(h_d[i]) + len(data)].cpu().numpy().tobytes()
        if got != want or back != data:
            raise AssertionError(f"buffer {i} ({len(data)} bytes) differs from the stdlib")
    r = res.cpu().numpy().reshape(-1, REC)
    out_len = r[:, :8].copy().view(np.uint64).ravel()
    rest = r[:, 8:].copy().view(np.uint64)
    if not (np.array_equal(out_len, lens.astype(np.uint64)) and not rest.any()):
        raise AssertionError("a record is not {len, 0, OK}")


def wrapped_multiple_of_4(lens):
    """lens (multiples of 4) raised in steps of 4 until the CRLF-76 text of
    each is a multiple of 4 bytes too (an even number of lines)."""
    lens = lens.copy()
    for _ in range(64):
        chars = (lens + 2) // 3 * 4
        odd = ((chars + L - 1) // L) % 2 == 1
        if not odd.any():
            return lens
        lens[odd] += 4
    raise AssertionError("no such lengths")


def run_shape(name, lens, steps, strided_rows=None):
    """Both batch calls over buffers of `lens` bytes (dword-aligned starts on
    both sides); with strided_rows = (nbuf, length) the strided calls too."""
    dev = "cuda"
    nbuf = lens.size
    in_sizes = (lens + 3) // 4 * 4
    in_off_h = np.zeros(nbuf + 1, np.int64)
    np.cumsum(in_sizes, out=in_off_h[1:])
    # the ragged calls take buffer i as [in_off[i], in_off[i+1]): to keep every
    # start on a dword the lengths themselves are multiples of 4 in the ragged
    # shape (the uniform shape's 1 KiB rows are anyway)
    assert np.array_equal(in_sizes, lens)
    in_off = torch.from_numpy(in_off_h).to(dev)
    x = torch.empty(int(in_off_h[-1]), dtype=torch.uint8, device=dev)
    b64.fill_splitmix64(x, 0xB64)
    # the decode takes text i as [t_off[i], t_off[i+1]): packed tight, so the
    # lengths are chosen (wrapped_multiple_of_4) to keep every text on a dword
    t_off = b64.lines_batch_layout(in_off, L, SEP, True)
    if bool((t_off % 4 != 0).any()):
        raise AssertionError("a text does not start on a dword")
    text = torch.empty(int(t_off[-1]), dtype=torch.uint8, device=dev)
    tlen = t_off[1:] - t_off[:-1]
    d_off = b64.strict_batch_layout(t_off, L, SEP, True, align=4)
    dec = torch.empty(int(d_off[-1]), dtype=torch.uint8, device=dev)
    res = torch.empty(REC * nbuf, dtype=torch.uint8, device=dev)

    def enc():
        b64.encode_lines_batch(x, in_off, text, t_off[:-1], L, SEP, True)

    def dcd():
        b64.decode_strict_batch(text, t_off, dec, d_off[:-1], res, L, SEP, True)

    enc()
    dcd()
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    picks = sorted({0, nbuf - 1, int(np.argmax(lens)), int(np.argmin(lens)),
                    *rng.integers(0, nbuf, 12).tolist()})
    check_batch(x, in_off, text, t_off, dec, d_off, res, lens, picks)
    payload = int(lens.sum())
    chars = int(tlen.sum())
    out = {"shape": name, "nbuf": int(nbuf), "payload_bytes": payload, "text_bytes": chars,
           "steps": steps}
    ms_e, ms_d = timed(enc, steps), timed(dcd, steps)
    out["encode_lines_batch"] = {"ms": ms_e, "payload_GiBps": payload / ms_e / 1e-3 / 2**30,
                                 "moved_GBps": (payload + chars) / ms_e / 1e-3 / 1e9}
    out["decode_strict_batch"] = {"ms": ms_d, "payload_GiBps": payload / ms_d / 1e-3 / 2**30,
                                  "moved_GBps": (payload + chars) / ms_d / 1e-3 / 1e9}
    if strided_rows:
        rows, length = strided_rows
        W = b64.encoded_lines_len(length, L, SEP, True)
        cap = b64.strict_decoded_cap(W, L, SEP, True)
        cstride = (cap + 3) // 4 * 4
        text2 = torch.empty(rows * W, dtype=torch.uint8, device=dev)
        dec2 = torch.empty(rows * cstride, dtype=torch.uint8, device=dev)

        def enc_s():
            b64.encode_lines_strided(x, length, length, rows, text2, W, L, SEP, True)

        def dcd_s():
            b64.decode_strict_strided(text2, W, W, rows, dec2, cstride, res, L, SEP, True)

        enc_s()
        dcd_s()
        torch.cuda.synchronize()
        if not torch.equal(text2, text[:rows * W]):
            raise AssertionError("the strided and the batch encode disagree")
        ms_es, ms_ds = timed(enc_s, steps), timed(dcd_s, steps)
        # interleaved once more, the other way round, to see the run-to-run spread
        ms_e2, ms_es2 = timed(enc, steps), timed(enc_s, steps)
        ms_d2, ms_ds2 = timed(dcd, steps), timed(dcd_s, steps)
        out["encode_lines_strided"] = {"ms": ms_es, "payload_GiBps": payload / ms_es / 1e-3 / 2**30}
        out["decode_strict_strided"] = {"ms": ms_ds, "payload_GiBps": payload / ms_ds / 1e-3 / 2**30}
        out["second_pass_ms"] = {"encode_lines_batch": ms_e2, "encode_lines_strided": ms_es2,
                                 "decode_strict_batch": ms_d2, "decode_strict_strided": ms_ds2}
        out["batch_over_strided"] = {"encode": min(ms_e, ms_e2) / min(ms_es, ms_es2),
                                     "decode": min(ms_d, ms_d2) / min(ms_ds, ms_ds2)}
    return out, payload, chars


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--ragged-mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lines_batch.json"))
    ap.add_argument("--no-ceiling", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b64.device_check()
    result = {"tool": "tests/tools/bench_lines_batch.py", "format": "CRLF-76, trailing",
              "build": b64.build_info(), "device": torch.cuda.get_device_name(0),
              "timing": "median of HIP-event times after 3 warm-ups, clocks pre-heated "
                        f"({bench.PREHEAT_MS} ms of scratch copies) before each region"}
    uni, _, _ = run_shape("uniform", np.full(args.rows, 1024, np.int64), args.steps,
                          strided_rows=(args.rows, 1024))
    result["uniform"] = uni
    print(json.dumps({"uniform": uni}), flush=True)
    torch.cuda.empty_cache()
    rng = np.random.default_rng(0xB64)
    target = args.ragged_mib << 20
    draw = np.exp(rng.uniform(np.log(16), np.log(65536), int(target / 7000) + 64))
    lens = wrapped_multiple_of_4((draw.astype(np.int64) + 3) // 4 * 4)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), target)) + 1]
    rag, payload, chars = run_shape("ragged", lens, args.steps)
    rag["lengths"] = {"min": int(lens.min()), "max": int(lens.max()),
                      "median": int(np.median(lens)), "law": "log-uniform 16 B..64 KiB, raised to the "
                      "next multiple of 4 whose text is one too (packed tight, every buffer and "
                      "every text starts on a dword)"}
    if not args.no_ceiling:
        torch.cuda.empty_cache()
        ceil = bench.copy_ceilings(payload, chars, steps=args.steps)
        if ceil:
            rag["copy_ceiling"] = ceil
            rag["encode_lines_batch"]["fraction_of_ceiling"] = \
                rag["encode_lines_batch"]["moved_GBps"] / ceil["encode"]["GBps"]
            rag["decode_strict_batch"]["fraction_of_ceiling"] = \
                rag["decode_strict_batch"]["moved_GBps"] / ceil["decode"]["GBps"]
    result["ragged"] = rag
    print(json.dumps({"ragged": rag}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
