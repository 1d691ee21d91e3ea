"""Strict decode against the lenient decode of the same text, in one process
on one GPU:

    1 GiB of payload as plain text, one buffer           decode_strict vs decode
    the same payload as (76, CRLF) text, one buffer      decode_strict vs decode
                                                         (automatic path, model held)
    config 4's rows (1,048,576 x 1,404-byte RFC 2045 rows of 1 KiB)
                                                         decode_strict_strided vs decode_strided

  (a) the strict call   (b) the lenient call   (e) the strict call on the same
  text with one offence in its last tile (the error path's cost)

Each figure: clocks pre-heated as bench.py does, HIP events around every
call, the median of `--steps` calls after `--warmup`.  Both decodes' outputs
are compared with the payload before timing.  Algorithmic bytes are text +
payload, reported against 8 TB/s.  Prints one JSON line and keeps it in --out.

    python scripts/bench_decode_strict.py [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12  # bytes/s, HBM3E of one MI355X
BOUND = 1.10  # the strict call should cost no more than this times the lenient one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_decode_strict.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from async_amd import b64
    b64.device_check()
    scratch = torch.empty(2, 256 << 20, dtype=torch.uint8, device="cuda")

    def preheat(ms=25.0):
        for _ in range(max(1, int(ms / 0.085))):  # ~0.085 ms per 256 MiB copy
            scratch[0].copy_(scratch[1])

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        preheat()
        per = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            per.append(a.elapsed_time(b) * 1e3)
        return {"median_us": round(statistics.median(per), 1), "min_us": round(min(per), 1),
                "max_us": round(max(per), 1)}

    def record(res, i=0):
        r = b64.StrictResult.from_buffer_copy(res[24 * i:24 * i + 24].cpu().numpy().tobytes())
        return r.err, r.err_pos, r.out_len

    def finish(r, nbytes):
        a, b, e = (r[k]["median_us"] for k in ("a_strict", "b_lenient", "e_strict_one_offence"))
        r["a_bytes_per_s"] = round(nbytes / (a * 1e-6))
        r["a_of_8TBps"] = round(nbytes / (a * 1e-6) / PEAK, 3)
        r["a_over_b"] = round(a / b, 3)
        r["e_over_a"] = round(e / a, 3)
        r["within_bound"] = a <= BOUND * b
        return r

    def one_buffer(name, n, L, sep):
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        b64.fill_splitmix64(x, 0x5EED)
        text = b64.encode(x) if L is None else b64.encode_lines(x, L, sep)
        W = text.numel()
        out_s = torch.empty(b64.strict_decoded_cap(W, L, sep), dtype=torch.uint8, device="cuda")
        out_l = torch.empty(b64.decoded_cap(W), dtype=torch.uint8, device="cuda")
        res_s = torch.empty(24, dtype=torch.uint8, device="cuda")
        res_l = torch.zeros(b64.RES_BYTES, dtype=torch.uint8, device="cuda")

        def strict():
            b64.decode_strict(text, L, sep, out=out_s, result=res_s)

        def lenient():
            return b64.decode(text, out=out_l, result=res_l)

        strict()
        same = record(res_s) == (0, 0, n) and torch.equal(out_s[:n], x)
        d = lenient()
        same_l = d.info().out_len == n and torch.equal(out_l[:n], x)
        r = {"leg": name, "payload_bytes": n, "text_bytes": W, "line_len": L or 0,
             "sep_len": len(sep), "strict_exact": same, "lenient_exact": same_l,
             "a_strict": timed(strict), "b_lenient": timed(lenient)}
        # a character inside the last tile of the hot part
        bad = W - 3000 if L is None else (W // (L + len(sep)) - 40) * (L + len(sep)) + 10
        text[bad:bad + 1].fill_(0x2A)
        r["e_strict_one_offence"] = timed(strict)
        r["offence_found"] = record(res_s)[:2] == (1, bad)
        return finish(r, n + W)

    def rows(name, nbuf, length, L, sep):
        x = torch.empty(nbuf * length, dtype=torch.uint8, device="cuda")
        b64.fill_splitmix64(x, 0x5EED)
        W = b64.encoded_lines_len(length, L, sep)
        text = torch.empty(nbuf * W, dtype=torch.uint8, device="cuda")
        b64.encode_lines_strided(x, length, length, nbuf, text, W, L, sep)
        cap_s = -(-b64.strict_decoded_cap(W, L, sep) // 4) * 4  # a dword-aligned pitch
        cap_l = 12 * ((W + 15) // 16)                           # the lenient batch's row with room
        out_s = torch.empty(nbuf * cap_s, dtype=torch.uint8, device="cuda")
        out_l = torch.empty(nbuf * cap_l, dtype=torch.uint8, device="cuda")
        res_s = torch.empty(24 * nbuf, dtype=torch.uint8, device="cuda")
        outlen = torch.zeros(nbuf, dtype=torch.int64, device="cuda")

        def strict():
            b64.decode_strict_strided(text, W, W, nbuf, out_s, cap_s, res_s, L, sep)

        def lenient():
            b64.decode_strided(text, W, W, nbuf, out_l, cap_l, outlen)

        strict()
        recs = res_s.view(nbuf, 24)
        same = (record(res_s) == (0, 0, length) and record(res_s, nbuf - 1) == (0, 0, length) and
                bool((recs == recs[0]).all()) and
                torch.equal(out_s.view(nbuf, cap_s)[:, :length], x.view(nbuf, length)))
        lenient()
        same_l = (int(outlen.min()) == length == int(outlen.max()) and
                  torch.equal(out_l.view(nbuf, cap_l)[:, :length], x.view(nbuf, length)))
        r = {"leg": name, "nbuf": nbuf, "payload_bytes": nbuf * length, "text_bytes": nbuf * W,
             "row_text_bytes": W, "strict_out_stride": cap_s, "lenient_out_stride": cap_l,
             "line_len": L, "sep_len": len(sep), "strict_exact": same, "lenient_exact": same_l,
             "a_strict": timed(strict), "b_lenient": timed(lenient)}
        bad = (nbuf - 1) * W + 710  # character 8 of the last row's line 9
        text[bad:bad + 1].fill_(0x2A)
        r["e_strict_one_offence"] = timed(strict)
        r["offence_found"] = record(res_s, nbuf - 1)[:2] == (1, 710) and \
            record(res_s, nbuf - 2) == (0, 0, length)
        return finish(r, nbuf * (length + W))

    legs = [one_buffer("1GiB_plain", 1 << 30, None, b""),
            one_buffer("1GiB_crlf76", 1 << 30, 76, b"\r\n"),
            rows("cfg4_rows_crlf76", 1 << 20, 1024, 76, b"\r\n")]
    res = {"bench": "decode_strict", "device": torch.cuda.get_device_name(0),
           "build": b64.build_info(), "steps": args.steps, "warmup": args.warmup,
           "bound": BOUND,
           "exact": all(g["strict_exact"] and g["lenient_exact"] and g["offence_found"]
                        for g in legs),
           "within_bound": all(g["within_bound"] for g in legs),
           "legs": legs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if res["exact"] else 1


if __name__ == "__main__":
    sys.exit(main())
