#!/usr/bin/env python3
"""Interleaved A/B timing of the headline *pair*: bench.py's own step loop
(`encode(x, out=enc)`, then `decode(enc, ...)` of those characters, K times
between two HIP events, nothing else on the stream), which scripts/ab_time.py
never runs -- it times the encode repeated alone and the decode repeated
alone, so whatever the encode leaves in the memory-side cache for the decode
is invisible to it.  The same child also times those two legs alone, so a
leg that pays for a gain of the pair is seen.

One child process per (round, library), the libraries alternating on one
box (in reverse order in odd rounds); the first library is the parent the others are judged against:

    python scripts/ab_pair.py [--rounds 5] [--steps 20] [--reps 5] [--rot 4]
                              [--sizes 1073741824[,...]] PARENT_LIB [LIB ...]

The legs `pair_rot`, `enc_rot` and `dec_rot` are the same three over `rot`
distinct inputs and character buffers taken in turn, so that no encode
overwrites characters still dirty in the memory-side cache from the step
before: what a caller sees who encodes a buffer once and then reads it.

A child prints one JSON line per size: every region's us per step (`reps`
regions of K steps per leg, each behind bench.py's clock pre-heat).  A
round's figure is the median of its regions.  The summary gives, per
library, size and leg, the median, minimum and maximum over the rounds, and
for each candidate the rule a gain has to meet: every round faster than
every round of the parent, and a median gain of at least twice the parent's
own spread (max - min over its rounds).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("pair", "enc", "dec", "pair_rot", "enc_rot", "dec_rot", "pair_other", "dec_sync")


def steps_for(n, steps):
    """K for a buffer of n bytes: `steps` at 1 GiB, more for small buffers so
    that a region stays several milliseconds long."""
    return min(2000, max(steps, steps * (1 << 30) // n // 8))


def child(lib, sizes, steps, reps, rot):
    sys.path.insert(0, ROOT)
    import torch
    from async_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    from async_amd import b64
    from bench import preheat
    stream = torch.cuda.current_stream()
    for n in sizes:
        E = b64.encoded_len(n)
        x = torch.empty(n, dtype=torch.uint8, device="cuda")
        b64.fill_splitmix64(x, 0x5EED)
        enc = torch.empty(E, dtype=torch.uint8, device="cuda")
        dec = torch.empty(b64.decoded_cap(E), dtype=torch.uint8, device="cuda")
        ws = torch.zeros(b64.workspace_size(E), dtype=torch.uint8, device="cuda")
        res = torch.zeros(b64.RES_BYTES, dtype=torch.uint8, device="cuda")

        def f_enc():
            b64.encode(x, out=enc, stream=stream)

        def f_dec():
            b64.decode(enc, out=dec, workspace=ws, result=res, stream=stream)

        def f_pair():
            f_enc()
            f_dec()

        # The same three legs over `rot` distinct inputs and character
        # buffers taken in turn (one output buffer): no encode writes over
        # characters that the step before it wrote, so lines still dirty in
        # the memory-side cache are never overwritten there, and every
        # buffer's characters go to HBM as they do for a caller that encodes
        # a buffer once.  A gain of `pair` that `pair_rot` does not show comes
        # from the loop's reuse of one buffer.
        xs, encs = [x], [enc]
        for i in range(1, rot):
            xs.append(torch.empty(n, dtype=torch.uint8, device="cuda"))
            b64.fill_splitmix64(xs[i], 0x5EED + i)
            encs.append(torch.empty(E, dtype=torch.uint8, device="cuda"))
        turn = [0, 0, 0]

        def r_enc(k=1):
            i = turn[k] = (turn[k] + 1) % rot
            b64.encode(xs[i], out=encs[i], stream=stream)
            return i

        def r_dec(k=2, i=None):
            if i is None:
                i = turn[k] = (turn[k] + 1) % rot
            b64.decode(encs[i], out=dec, workspace=ws, result=res, stream=stream)
            return i

        def r_pair():
            return r_dec(i=r_enc(0))

        def r_other():
            # an encode, then a neighbour that does not read its characters:
            # the decode of the buffer encoded `rot - 1` steps ago
            r_dec(i=(r_enc(0) + 1) % rot)

        for _ in range(3):
            f_pair()
        torch.cuda.synchronize()
        ok = b64.Decoded(dec, res).info().out_len == n and bool(torch.equal(dec[:n], x))
        for _ in range(rot):
            i = r_pair()
            torch.cuda.synchronize()
            ok = ok and b64.Decoded(dec, res).info().out_len == n and bool(torch.equal(dec[:n], xs[i]))
        K = steps_for(n, steps)
        out = {"lib": lib, "n": n, "K": K, "rot": rot, "ok": ok}
        for name, fn in (("pair", f_pair), ("enc", f_enc), ("dec", f_dec),
                         ("pair_rot", r_pair), ("enc_rot", r_enc), ("dec_rot", r_dec),
                         ("pair_other", r_other)):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                preheat()
                e0.record(stream)
                for _ in range(K):
                    fn()
                e1.record(stream)
                e1.synchronize()
                ts.append(round(e0.elapsed_time(e1) * 1e3 / K, 2))
            out[name] = ts
        # scripts/ab_time.py's lone decode: right after an encode of the same
        # buffer, no pre-heat, every call between its own events with a
        # synchronize after it (a region's figure is the median call)
        ts = []
        for _ in range(reps):
            f_enc()
            f_dec()
            torch.cuda.synchronize()
            one = []
            for _ in range(K):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f_dec()
                e1.record(stream)
                e1.synchronize()
                one.append(e0.elapsed_time(e1) * 1e3)
            ts.append(round(statistics.median(one), 2))
        out["dec_sync"] = ts
        i = r_pair()
        torch.cuda.synchronize()
        ok = ok and b64.Decoded(dec, res).info().out_len == n and bool(torch.equal(dec[:n], xs[i]))
        out["ok"] = ok
        print(json.dumps(out), flush=True)
        del x, enc, dec, ws, res, xs, encs


def verdict(parent, cand):
    """The stop rule for one leg: rounds of the parent and of a candidate."""
    spread = max(parent) - min(parent)
    gain = statistics.median(parent) - statistics.median(cand)
    return {"parent_spread_us": round(spread, 2), "median_gain_us": round(gain, 2),
            "every_round_faster": max(cand) < min(parent),
            "gain_ge_2x_spread": gain >= 2 * spread,
            "gain": max(cand) < min(parent) and gain >= 2 * spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=str(1 << 30), help="comma-separated input bytes")
    ap.add_argument("--rot", type=int, default=4,
                    help="distinct buffers of the *_rot legs (1: the same buffer, as the plain legs)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    if a.child:
        return child(a.libs[0], sizes, a.steps, a.reps, max(1, a.rot))
    agg = {}  # (lib, n, leg) -> one figure per round
    for r in range(a.rounds):
        # odd rounds run the libraries in the reverse order, so that no
        # library always follows the same neighbour
        for lib in (a.libs if r % 2 == 0 else a.libs[::-1]):
            p = subprocess.run([sys.executable, __file__, "--child", "--steps", str(a.steps),
                                "--reps", str(a.reps), "--sizes", a.sizes,
                                "--rot", str(a.rot), lib],
                               capture_output=True, text=True, timeout=300)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode or len(lines) != len(sizes):
                print(p.stdout, p.stderr, file=sys.stderr)
                sys.exit(p.returncode or 1)
            for ln in lines:
                d = json.loads(ln)
                d["round"] = r
                print(json.dumps(d), flush=True)
                if not d["ok"]:
                    print(f"{lib}: round trip mismatch at n={d['n']}", file=sys.stderr)
                    sys.exit(1)
                for leg in LEGS:
                    agg.setdefault((lib, d["n"], leg), []).append(statistics.median(d[leg]))
    for lib in a.libs:
        for n in sizes:
            row = {"summary": lib, "n": n}
            for leg in LEGS:
                v = agg[(lib, n, leg)]
                row[leg] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2),
                            "max": round(max(v), 2)}
                if lib != a.libs[0]:
                    row[leg]["vs_parent"] = verdict(agg[(a.libs[0], n, leg)], v)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
