"""Line-wrapped encode against the plain encode and against today's recipe
(encode, then torch.cat of a separator column onto a (lines, L) view), in one
process on one GPU:

    1 GiB of payload as (76, CRLF) and as (64, LF), one buffer
    config 4's tight rows (1,048,576 x 1 KiB -> 1,404-byte RFC 2045 rows)

  (a) encode_lines / encode_lines_strided
  (b) encode / encode_strided of the same input
  (c) (b) + the torch.cat of tests/test_gpu_parity.py (needs E to be a
      multiple of L, so the 1 GiB legs take the multiple of 912 bytes below
      1 GiB: whole lines for both formats)

Each figure: clocks pre-heated as bench.py does, HIP events around every
call, the median of `--steps` calls after `--warmup`.  (a)'s output is
compared with (c)'s before timing.  Algorithmic bytes are N + wrapped
length, reported against 8 TB/s.  Prints one JSON line and keeps it in --out.

    python scripts/bench_encode_lines.py [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12  # bytes/s, HBM3E of one MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_encode_lines.json"))
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

    def leg(name, nbuf, length, L, sep):
        n = nbuf * length
        E = b64.encoded_len(length)
        W = b64.encoded_lines_len(length, L, sep)
        assert E % L == 0 and W == E + len(sep) * (E // L)
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        b64.fill_splitmix64(x, 0x5EED)
        text = torch.empty(nbuf * W, dtype=torch.uint8, device="cuda")
        enc = torch.empty(nbuf * E, dtype=torch.uint8, device="cuda")
        col = torch.tensor(list(sep), dtype=torch.uint8, device="cuda").expand(
            nbuf * (E // L), len(sep))

        if nbuf == 1:
            def lines():
                b64.encode_lines(x, L, sep, out=text)

            def plain():
                b64.encode(x, out=enc)
        else:
            def lines():
                b64.encode_lines_strided(x, length, length, nbuf, text, W, L, sep)

            def plain():
                b64.encode_strided(x, length, length, nbuf, enc, E)

        def recipe():
            plain()
            return torch.cat([enc.view(-1, L), col], dim=1).reshape(-1).contiguous()

        lines()
        same = torch.equal(text, recipe())
        r = {"leg": name, "nbuf": nbuf, "len": length, "line_len": L, "sep_len": len(sep),
             "wrapped_bytes": nbuf * W, "same_bytes_as_recipe": same,
             "a_encode_lines": timed(lines), "b_encode": timed(plain),
             "c_encode_cat": timed(recipe)}
        a, b, c = (r[k]["median_us"] for k in ("a_encode_lines", "b_encode", "c_encode_cat"))
        r["a_bytes_per_s"] = round((n + nbuf * W) / (a * 1e-6))
        r["a_of_8TBps"] = round((n + nbuf * W) / (a * 1e-6) / PEAK, 3)
        r["a_over_b"] = round(a / b, 3)
        r["a_over_c"] = round(a / c, 3)
        r["a_faster_than_c"] = a < c
        return r

    one = (1 << 30) // 912 * 912
    legs = [leg("1GiB_crlf76", 1, one, 76, b"\r\n"),
            leg("1GiB_lf64", 1, one, 64, b"\n"),
            leg("cfg4_rows_crlf76", 1 << 20, 1024, 76, b"\r\n")]
    res = {"bench": "encode_lines", "device": torch.cuda.get_device_name(0),
           "build": b64.build_info(), "steps": args.steps, "warmup": args.warmup,
           "ok": all(g["same_bytes_as_recipe"] and g["a_faster_than_c"] for g in legs),
           "legs": legs}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
