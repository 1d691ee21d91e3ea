#!/usr/bin/env python3
"""bench.py -- device-resident base64 encode+decode throughput on MI355X.

Metric (BASELINE.json): GiB/s of base64 encode+decode, device-resident.
A "step" = encode one 1 GiB buffer (BASELINE config 2: splitmix64 seed
0x5EED, standard alphabet with padding) and decode the result back, both on
the GPU, inputs already in HBM.  value = payload bytes (N per GPU per step)
/ wall time of the K timed steps, summed over ranks (weak scaling: each
rank owns its own 1 GiB buffer; the path shards by independent buffers and
needs no collective on the data path).  Each device-timed region is preceded
by ~25 ms of untimed scratch copies (`preheat`, `preheat_ms` on the line):
the GPU's clocks ramp back only tens of ms after it idles, which otherwise
slows the first milliseconds of a short timed region by up to 8 %.

A plain run does only that: set up, W warmup steps, the bit check, the K
timed steps, the outputs if --dump-outputs is given, the line.  On the line,
`ms_per_step` is the wall time of one timed step in milliseconds, and the
keys of the legs below are null.

--dump-outputs DIR writes what the last timed step computed, as a caller of
the path receives it: DIR/encoded.npy (the characters), DIR/decoded.npy (the
bytes decoded back) and DIR/decode_result.npy (out_len, valid, tail_n of the
decode's result record), float32 / float64.  Of the two 1 GiB-scale arrays a
fixed sample is kept (the first and last 65,536 elements whole and seeded
random positions between them, DUMP_ELEMS each); the inputs are the same
splitmix64 stream on every run, so two builds can be compared file by file.

With --full, also reported on the same JSON line:
  roofline      the dominant kernel's algorithmic bytes per launch
                (N + 4*ceil(N/3): read + write) / its average launch time
                from HIP events (a second pass of the K steps right after
                the timed region, each call bracketed), against 8 TB/s;
                `traffic` = HBM bytes per launch from the committed rocprofv3
                PMC summary (profiles/pmc_<round>.json) when present;
  cpu_baseline  the oracle's scalar C restatement of the reference
                (oracle/, "port"), 1 thread, on a bounded sample of the same
                data, rank 0 at N=1 only; `all_core`: the same oracle over
                config 4's shape on up to 16 threads (the box's CPU share);
  batch_cfg4    BASELINE config 4: 1,048,576 x 1 KiB buffers split across
                the ranks by index range, strided encode + decode, plus the
                one exchange step (allgather of per-rank output totals);
                whole-job and per-rank GiB/s and roofline fractions;
  mime_decode   MIME-formatted (CRLF-76) decode of config 2's characters and
                config 4's rows, and config 2's characters with unstructured
                junk at densities 0.001 and 0.05, bit-checked (rank 0 at N=1);
  cfg5_egress   BASELINE config 5 through the product's stage stack, host
                memory in and out, 1 and 16 loops, with the oracle's stack
                timed beside it (rank 0 at N=1; skipped with --no-cpu);
  root_scatter  N > 1: rank 0 scatters config 4's 1 GiB to the ranks (reported,
                not used by the primary metric: SURVEY.md §8(e));
  host_fd       the path's real ends: config 2 through a pipe / socket
                read() by the event loop's pipestream into the GPU decoder
                stage, and the encoder stack drained by fdsink into write(2)
                on a pipe (rank 0, N=1); never `value`;
  host_inclusive  the same 1 GiB round trip starting and ending in pinned
                host memory (rank 0): the kernels read and write the pinned
                buffers in place over PCIe (the sessions' zero-copy path),
                and the staged form (H2D, kernel, D2H on k streams); bit-
                checked; never `value`.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
                        [--full]
        N > 1 without WORLD_SIZE in the environment: bench.py starts
        `python -m torch.distributed.run --nproc-per-node N` itself (before
        touching the GPU) and relays its line; every rank checks that the
        process group has exactly N ranks, and the line reports RCCL's count.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "GiB/s base64 encode+decode, device-resident, at 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
ROUND = "r06"  # the committed PMC summary (profiles/pmc_<ROUND>.json) used for `traffic`


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=1 << 30, help="bytes per GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg (roofline, CPU baselines, batch, host, "
                         "MIME, config 5); the --no-* options select among them")
    ap.add_argument("--cpu-sample", type=int, default=512 << 20,
                    help="bytes of the CPU baseline sample (rank 0, N=1)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-threads", type=int,
                    default=min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity")
                                else (os.cpu_count() or 1)),
                    help="threads of the all-core CPU baseline (the GPU box's CPU share is 16)")
    ap.add_argument("--cpu-batch-bufs", type=int, default=1 << 18,
                    help="1 KiB buffers in the all-core CPU baseline sample")
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--batch-steps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host_inclusive leg")
    ap.add_argument("--no-mime", action="store_true", help="skip the mime_decode leg")
    ap.add_argument("--no-cfg5", action="store_true", help="skip the cfg5_egress leg")
    ap.add_argument("--host-block", type=int, default=24 << 20,
                    help="bytes per block of the host_inclusive leg (a multiple of 3)")
    ap.add_argument("--host-streams", type=int, default=4)
    ap.add_argument("--dry-run", action="store_true",
                    help="launch and check the process group only, no GPU work (tests)")
    ap.add_argument("--backend", default="nccl",
                    help="torch.distributed backend for N>1 (nccl = RCCL over xGMI; "
                         "gloo only to rehearse the multi-rank logic on one GPU)")
    return ap.parse_args()


def coll_device():
    return "cpu" if dist.is_initialized() and dist.get_backend() == "gloo" else "cuda"



def max_over_ranks(x: float, world: int) -> float:
    if world == 1:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=coll_device())
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_floats(vals, world: int):
    """Every rank's `vals` (a short list of floats), in rank order."""
    if world == 1:
        return [list(vals)]
    t = torch.tensor(vals, dtype=torch.float64, device=coll_device())
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [o.tolist() for o in out]


def sync_all(world: int):
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()


def load_traffic(kernels):
    """HBM bytes per launch of `kernels` (summed) from the committed PMC
    summary (scripts/pmc_traffic.sh + scripts/summarize_pmc.py)."""
    path = os.path.join(ROOT, "profiles", f"pmc_{ROUND}.json")
    try:
        with open(path) as f:
            pmc = json.load(f)["kernels"]
        total = 0.0
        for k in kernels:
            if k in pmc:
                total += pmc[k]["hbm_bytes_per_launch"]
            else:  # grid-qualified entries
                hits = [v for n, v in pmc.items() if n.startswith(k + "@")]
                if not hits:
                    return None
                total += max(h["hbm_bytes_per_launch"] for h in hits)
        return total
    except (OSError, KeyError, ValueError):
        return None


PREHEAT_MS = 25.0
_scratch = []


def preheat(ms: float = PREHEAT_MS):
    """Untimed GPU clock pre-heat right before a timed region: ~`ms` of
    256 MiB device-to-device copies between two scratch buffers (never the
    measured buffers; they only push the measured data out of the caches).
    After the GPU idles or runs only short bursts (setup, the bit checks,
    W warmup steps of ~1 ms each), its clocks take tens of ms to ramp back,
    and the first milliseconds of a timed region run slow:
    profiles/r05_clock_ramp.jsonl, one process, interleaved -- the 1 GiB
    step 811-816 us after 0.2 s idle vs 789-792 after a long warm-up, the
    config-4 encode 424-433 vs 400-404; 10 ms of these copies already gives
    794-797 / 400-403.  The timed region itself is unchanged: K steps
    between a barrier + synchronize on both sides."""
    if not _scratch:
        _scratch.append(torch.empty(2, 256 << 20, dtype=torch.uint8, device="cuda"))
    a = _scratch[0]
    for _ in range(max(1, int(ms / 0.085))):  # ~0.085 ms per 256 MiB copy
        a[0].copy_(a[1])


def bench_placement(b64):
    """Put this rank's host side on its GPU's NUMA node and say where it is.
    The main thread is bound (b64x_bind_thread) before anything else runs,
    so the buffers it fills and every thread it starts (the CPU baseline's,
    the harness's loops) live on the GPU's node; each loop's hub binds its
    thread again (ASYNC_B64_BIND).  One loop of config 5 ran 6.1-6.2 GiB/s
    on the GPU's node and 4.4-4.5 on the other socket of the same box: the
    scheduler's choice was round 5's box-to-box spread
    (profiles/r06_numa_probe.jsonl)."""
    from async_amd import placement as pl
    dev = torch.cuda.current_device()
    node = b64.bind_thread(dev)
    topo = pl.topology(dev)
    cpus = sorted(os.sched_getaffinity(0))
    return {"gpu_node": topo["gpu_node"], "gpu_pci": topo["gpu_pci"], "link": topo["link"],
            "numa_nodes": topo["nodes"], "main_thread_node": node,
            "main_thread_cpus": pl.cpulist(cpus),
            "loops": "bound to the GPU's node by their hub" if
                     os.environ.get("ASYNC_B64_BIND", "1") != "0" else "unbound (ASYNC_B64_BIND=0)"}


def bench_single(args, world, rank, b64):
    N = args.size
    E = b64.encoded_len(N)
    x = torch.empty(N, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    enc = torch.empty(E, dtype=torch.uint8, device="cuda")
    dec = torch.empty(b64.decoded_cap(E), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(b64.workspace_size(E), dtype=torch.uint8, device="cuda")
    res = torch.zeros(b64.RES_BYTES, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()

    def step():
        b64.encode(x, out=enc, stream=stream)
        b64.decode(enc, out=dec, workspace=ws, result=res, stream=stream)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    # correctness of the warmed-up result (bit-exact round trip)
    info = b64.Decoded(dec, res).info()
    ok = info.out_len == N and bool(torch.equal(dec[:N], x))
    if not ok:
        raise SystemExit(f"rank {rank}: round trip mismatch (out_len={info.out_len})")

    K = args.steps
    # Timed region: K steps back to back with nothing else on the stream.  A
    # timing event between two kernels costs ~7 us of GPU idle time on this
    # runtime (A/B in one process: 0.813 vs 0.797 ms per step), so the
    # per-kernel events that feed the roofline run in a second pass of the
    # same K steps right after it.
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    preheat()
    sync_all(world)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(K):
        step()
    ev1.record(stream)
    sync_all(world)
    wall = time.perf_counter() - t0
    wall = max_over_ranks(wall, world)
    gpu_ms = ev0.elapsed_time(ev1) / K
    out = {"N": N, "E": E, "K": K, "wall": wall, "gpu_ms_per_step": gpu_ms}
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, enc[:E], b64.Decoded(dec, res))
    if not args.full:
        return out
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(K)]
    for k in range(K):
        evs[k][0].record(stream)
        b64.encode(x, out=enc, stream=stream)
        evs[k][1].record(stream)
        b64.decode(enc, out=dec, workspace=ws, result=res, stream=stream)
        evs[k][2].record(stream)
    torch.cuda.synchronize()
    enc_ms = [evs[k][0].elapsed_time(evs[k][1]) for k in range(K)]
    dec_ms = [evs[k][1].elapsed_time(evs[k][2]) for k in range(K)]
    out.update({"enc_ms": statistics.mean(enc_ms), "dec_ms": statistics.mean(dec_ms),
                "enc_ms_min": min(enc_ms), "dec_ms_min": min(dec_ms)})
    return out


DUMP_ELEMS = 4 << 20  # elements kept of each large output (float32: 16 MiB a file)
DUMP_EDGE = 1 << 16   # of which the first and the last this many, whole


def dump_sample(t: torch.Tensor, seed: int):
    """`t` as float32 on the host: whole if it has at most DUMP_ELEMS
    elements, else its first and last DUMP_EDGE elements and the elements at
    seeded random positions between them (sorted; the same positions on every
    run for a given length)."""
    import numpy as np

    n = t.numel()
    if n > DUMP_ELEMS:
        inner = np.random.default_rng(seed).integers(DUMP_EDGE, n - DUMP_EDGE,
                                                     DUMP_ELEMS - 2 * DUMP_EDGE)
        idx = np.concatenate([np.arange(DUMP_EDGE), np.sort(inner),
                              np.arange(n - DUMP_EDGE, n)])
        t = t[torch.from_numpy(idx).to(t.device)]
    return t.to(torch.float32).cpu().numpy()


def dump_outputs(dirname, rank, chars, decoded):
    """--dump-outputs: the last timed step's outputs as .npy files (rank 0's
    under the plain names, rank r's as <name>.rank<r>.npy)."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    info = decoded.info()
    arrays = {"encoded": dump_sample(chars, 0x5EED),
              "decoded": dump_sample(decoded.out[:info.out_len], 0x5EED + 1),
              "decode_result": np.array([info.out_len, info.valid, info.tail_n], np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + (f".rank{rank}" if rank else "") + ".npy"), a)


def bench_batch(args, world, rank, b64, total_buf=1 << 20, L=1024, name="cfg4"):
    """A uniform batch of independent buffers (BASELINE config 4: 1 M x
    1 KiB; config 3: 65,536 x 4 KiB), split across the ranks by index range
    (strong scaling: the batch is fixed, each rank owns 1/N of it), strided
    encode + decode, plus the one exchange step (all-gather of per-rank
    output totals).  Buffer i holds bytes [i L, (i+1) L) of the splitmix64
    (0x5EED) stream; every buffer round-trips bit-exactly before timing and
    the whole output is checked against its digest (_batch_digest_check)."""
    from async_amd import shard

    lo, nbuf = shard.by_index(total_buf, world, rank)
    Es = b64.encoded_len(L)
    # decode rows: 12 bytes per 16-character slot (>= capacity; the row kernel
    # writes whole slots, so consecutive rows form one contiguous byte stream)
    cap = 12 * ((Es + 15) // 16)
    # this rank's share of the one splitmix64 stream: word k of the stream is
    # a function of seed + k * 0x9E3779B97F4A7C15, so the share starting at
    # byte lo*L (a multiple of 8) is the stream of a shifted seed
    assert (lo * L) % 8 == 0
    x = torch.empty(nbuf * L, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, (0x5EED + (lo * L // 8) * 0x9E3779B97F4A7C15) % (1 << 64))
    enc = torch.empty(nbuf * Es, dtype=torch.uint8, device="cuda")
    dec = torch.empty(nbuf * cap, dtype=torch.uint8, device="cuda")
    outlen = torch.zeros(nbuf, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    totals = torch.zeros(world, dtype=torch.int64, device="cuda")

    def step():
        b64.encode_strided(x, L, L, nbuf, enc, Es, stream=stream)
        b64.decode_strided(enc, Es, Es, nbuf, dec, cap, outlen, stream=stream)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ok = bool((outlen == L).all()) and bool(torch.equal(dec.view(nbuf, cap)[:, :L],
                                                        x.view(nbuf, L)))
    if not ok:
        raise SystemExit(f"rank {rank}: {name} batch round trip mismatch")
    digest = _batch_digest_check(name, lo, nbuf, L, Es, x, enc, dec, cap)
    # warm the exchange path too (first reduction / collective launches load
    # their code objects and set up communicators)
    for _ in range(2):
        _, tot_list = shard.exchange_totals(int(outlen.sum()), device=coll_device())
    K = args.batch_steps
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    preheat()
    sync_all(world)
    t0 = time.perf_counter()
    ev[0].record(stream)
    for _ in range(K):
        b64.encode_strided(x, L, L, nbuf, enc, Es, stream=stream)
    ev[1].record(stream)
    for _ in range(K):
        b64.decode_strided(enc, Es, Es, nbuf, dec, cap, outlen, stream=stream)
    ev[2].record(stream)
    # the one exchange step: every rank learns every rank's output total
    _, tot_list = shard.exchange_totals(int(outlen.sum()), device=coll_device())
    totals.copy_(torch.tensor(tot_list, dtype=torch.int64))
    sync_all(world)
    mine = time.perf_counter() - t0
    wall = max_over_ranks(mine, world)
    assert int(totals.sum()) == total_buf * L
    enc_ms = ev[0].elapsed_time(ev[1]) / K
    dec_ms = ev[1].elapsed_time(ev[2]) / K
    kern_ms = enc_ms + dec_ms
    alg = nbuf * (L + Es)  # per leg: read + written
    rank_frac = 2 * alg / (kern_ms * 1e-3) / (HBM_PEAK_GBS * 1e9)
    per_rank = gather_floats([nbuf * L * K / mine / 2**30, rank_frac, enc_ms, dec_ms], world)
    # the exchange step on its own (after the timed region): its latency
    # decides how many ranks a batch of this size amortises (shard.ranks_for)
    exchange_ms, advice = None, None
    if world > 1:
        ts = []
        for _ in range(10):
            sync_all(world)
            t1 = time.perf_counter()
            shard.exchange_totals(int(outlen.sum()), device=coll_device())
            ts.append(time.perf_counter() - t1)
        exchange_ms = max_over_ranks(statistics.median(ts), world) * 1e3
        advice = shard.ranks_for(kern_ms * 1e-3 * world, world, exchange_ms * 1e-3)
    return {
        "workload": f"{name}: {total_buf:,} x {L} B buffers split across ranks, strided "
                    "encode then decode, + allgather of per-rank output totals",
        "scaling": "strong",
        "buffers_per_rank": nbuf,
        "value": total_buf * L * K / wall / 2**30,
        "unit": "GiB/s",
        "ms_per_step": wall / K * 1e3,
        "encode_kernel_ms": enc_ms,
        "decode_kernel_ms": dec_ms,
        "encode_roofline_frac": alg / (enc_ms * 1e-3) / (HBM_PEAK_GBS * 1e9),
        "decode_roofline_frac": alg / (dec_ms * 1e-3) / (HBM_PEAK_GBS * 1e9),
        "roofline_frac": rank_frac,
        "whole_output_check": digest,
        "per_rank_GiB_s": [p[0] for p in per_rank],
        "per_rank_roofline_frac": [p[1] for p in per_rank],
        "per_rank_kernel_ms": [[p[2], p[3]] for p in per_rank],
        "exchange_ms": exchange_ms,
        "ranks_amortised": advice,
    }


def _batch_digest_check(name, lo, nbuf, L, Es, x, enc, dec, cap):
    """The batch's whole output against tests/golden/batch_digests.json
    (oracle-checked, make_golden.py --batch): with every buffer on this rank
    (N = 1), the SHA-256 of all characters and of the decoded rows (= the
    input stream's); on a share, every digested chunk of buffers the share
    holds whole.  Outside the timed region; exits on a mismatch."""
    import hashlib
    try:
        with open(os.path.join(ROOT, "tests", "golden", "batch_digests.json")) as f:
            g = json.load(f)[name]
    except (OSError, KeyError, ValueError):
        return None
    if g["nbuf"] == nbuf and lo == 0:
        e_ok = hashlib.sha256(enc.cpu().numpy()).hexdigest() == g["out_sha256"]
        rows = dec.view(nbuf, cap)[:, :L].contiguous().cpu().numpy()
        d_ok = hashlib.sha256(rows).hexdigest() == g["in_sha256"]
        del rows
        if not (e_ok and d_ok):
            raise SystemExit(f"{name}: whole-output digest mismatch (encode {e_ok}, "
                             f"decode {d_ok})")
        return {"scope": "whole batch", "encode_sha256_ok": e_ok, "decode_sha256_ok": d_ok}
    c = g["chunk_buffers"]
    first = (lo + c - 1) // c
    checked = 0
    for k in range(first, (lo + nbuf) // c):
        b0 = k * c - lo
        got = hashlib.sha256(enc[b0 * Es:(b0 + c) * Es].cpu().numpy()).hexdigest()
        if got != g["chunk_out_sha256"][k]:
            raise SystemExit(f"{name}: chunk {k} digest mismatch on this rank")
        checked += 1
    return {"scope": f"{checked} chunks of {c} buffers held whole by the rank",
            "encode_sha256_ok": True if checked else None}


def bench_host_inclusive(args, b64):
    """BASELINE config 2 starting and ending in pinned host memory: 1 GiB of
    bytes in pinned memory -> characters in pinned memory -> bytes back,
    bit-checked.  Two forms, each over blocks of --host-block bytes on
    --host-streams streams: "in_place" (the kernels read and write the
    pinned buffers over PCIe; what b64x_session_* does for encodes and clean
    head-free decodes) and "staged" (H2D, kernel, D2H through device
    buffers).  Rates are payload GiB/s (N bytes per direction)."""
    import ctypes

    import numpy as np

    from async_amd import _lib

    L = _lib.load()
    N, blk = args.size, args.host_block - args.host_block % 3
    E = b64.encoded_len(N)
    eblk = blk // 3 * 4
    slack = 64  # decode's last vector loads may reach past its input

    def pinned(nbytes):
        p = L.b64x_host_alloc(nbytes + slack)
        if not p:
            raise SystemExit("b64x_host_alloc failed")
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)),
                                    (nbytes + slack,))
        return p, arr

    p_src, src = pinned(N)
    p_chr, chars = pinned(E)
    p_dst, dst = pinned(N)
    k = args.host_streams
    streams = [torch.cuda.Stream() for _ in range(k)]
    dev_in = [torch.empty(eblk + slack, dtype=torch.uint8, device="cuda") for _ in range(k)]
    dev_out = [torch.empty(eblk + slack, dtype=torch.uint8, device="cuda") for _ in range(k)]
    res = [torch.zeros(_lib.RES_BYTES, dtype=torch.uint8, device="cuda") for _ in range(k)]
    ws = [torch.zeros(b64.workspace_size(eblk), dtype=torch.uint8, device="cuda")
          for _ in range(k)]
    a = _lib.alphabet()
    x = torch.empty(N, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    src[:N] = x.cpu().numpy()
    del x
    h_src = torch.from_numpy(src[:N])
    h_chr = torch.from_numpy(chars[:E])
    h_dst = torch.from_numpy(dst[:N])

    def run(direction, form):
        nblocks = (N + blk - 1) // blk
        for i in range(nblocks):
            j = i % k
            s = streams[j]
            b0 = i * blk
            n = min(blk, N - b0)
            e0 = b0 // 3 * 4
            m = b64.encoded_len(n)  # last block padded; others exact
            st = s.cuda_stream
            if direction == "encode":
                if form == "in_place":
                    _lib.check("b64x_encode_dev", L.b64x_encode_dev(
                        p_src + b0, n, p_chr + e0, ctypes.byref(a), st))
                else:
                    with torch.cuda.stream(s):
                        dev_in[j][:n].copy_(h_src[b0:b0 + n], non_blocking=True)
                        b64.encode(dev_in[j][:n], out=dev_out[j], stream=s)
                        h_chr[e0:e0 + m].copy_(dev_out[j][:m], non_blocking=True)
            else:
                if form == "in_place":
                    _lib.check("b64x_decode_dev", L.b64x_decode_dev(
                        p_chr + e0, m, p_dst + b0, res[j].data_ptr(), ctypes.byref(a), 0,
                        ws[j].data_ptr(), st))
                else:
                    with torch.cuda.stream(s):
                        dev_in[j][:m].copy_(h_chr[e0:e0 + m], non_blocking=True)
                        b64.decode(dev_in[j][:m], out=dev_out[j], workspace=ws[j],
                                   result=res[j], stream=s)
                        h_dst[b0:b0 + n].copy_(dev_out[j][:n], non_blocking=True)
        torch.cuda.synchronize()

    out = {"workload": f"cfg2 from/to pinned host memory: {N >> 20} MiB, blocks of "
                       f"{blk} B on {k} streams, payload GiB/s per direction",
           "unit": "GiB/s"}
    for form in ("in_place", "staged"):
        dst[:N] = 0
        chars[:E] = 0
        run("encode", form)  # warm-up (code objects, page mappings)
        run("decode", form)
        t = {}
        for direction in ("encode", "decode"):
            t0 = time.perf_counter()
            run(direction, form)
            t[direction] = time.perf_counter() - t0
        ok = bool(np.array_equal(dst[:N], src[:N]))
        if not ok:
            raise SystemExit(f"host_inclusive {form}: round trip mismatch")
        out[form] = {"encode": N / t["encode"] / 2**30, "decode": N / t["decode"] / 2**30,
                     "round_trip": N / (t["encode"] + t["decode"]) / 2**30, "exact": ok}
    for p in (p_src, p_chr, p_dst):
        L.b64x_host_free(p)
    return out


def bench_host_fd(args, b64):
    """The path's real ends: bytes crossing a pipe
    or socket through read(2)/write(2) on the product's event loop.
      ingress  a peer thread writes config 2's characters (clean, and in
               CRLF-76 lines) into a pipe (and, clean, an AF_UNIX
               socketpair) in 1 MiB writes -> pipestream -> base64_decode
               stage (GPU) -> consumer reading 256 KiB at a time;
      egress   config 2's bytes on a queuestream -> base64_encode stage (GPU)
               -> chunk_encode(1 MiB) -> fdsink (10,240-byte pulls, the
               reference's tcp_connection.c:22, write(2)) -> a pipe a peer
               thread drains.
    One stream each way, one loop thread; payload GiB/s (N bytes), wall time
    from the first byte to the last, bit-checked (ingress: == the input;
    egress: de-chunked == G3's digest, every chunk but the last two full)."""
    import hashlib

    import numpy as np

    from tests import util

    N = args.size
    x = torch.empty(N, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    chars_d = b64.encode(x)
    xh = x.cpu().numpy()
    out = np.empty(N + 16, np.uint8)
    out.fill(0)  # fault in outside the timed region
    res = {"workload": f"cfg2 ({N >> 20} MiB) through a pipe/socket and the event loop, one "
                       "stream each way", "unit": "GiB/s of payload"}
    # the same stream from memory (blobstream -> decoder stage -> consumer):
    # the loop and the GPU stage without the pipe's copies
    import ctypes
    H = util.harness()
    ch = chars_d.cpu().numpy()
    best = None
    for _ in range(2):
        err = ctypes.c_int(0)
        t0 = time.perf_counter()
        n = H.h_decode_stream(ch.ctypes.data, ch.size, 0, 1 << 18, util.cch(-1), util.cch(-1),
                              out.ctypes.data, out.size, ctypes.byref(err))
        dt = time.perf_counter() - t0
        if n != N or not np.array_equal(out[:N], xh):
            raise SystemExit(f"host_fd blob stream: decode mismatch (errno {err.value})")
        best = dt if best is None else min(best, dt)
    res["ingress_blob_clean"] = {"GiB_s": N / best / 2**30, "seconds": best,
                                 "bytes_in": int(ch.size)}
    # the channel alone, as calibration: the same characters written by the
    # same peer thread and read(2) by one thread straight into a buffer, no
    # decode (payload-equivalent GiB/s, to set beside the ingress legs)
    sink = np.empty(ch.size + 16, np.uint8)
    sink.fill(0)
    for name, sock in (("channel_raw_pipe", False), ("channel_raw_socket", True)):
        best = None
        for _ in range(2):
            got, err, dt = util.fd_raw(ch, write_chunk=1 << 20, read_size=1 << 18, sock=sock,
                                       out=sink)
            if got is None or got.size != ch.size:
                raise SystemExit(f"host_fd {name}: errno {err}")
            best = dt if best is None else min(best, dt)
        res[name] = {"GiB_s_payload_equiv": N / best / 2**30, "seconds": best,
                     "bytes": int(ch.size)}
    del sink, ch
    legs = [("ingress_pipe_clean", chars_d, False), ("ingress_socket_clean", chars_d, True),
            ("ingress_pipe_crlf76", None, False)]
    for name, text_d, sock in legs:
        if text_d is None:
            text_d = crlf76(chars_d)
        text = text_d.cpu().numpy()
        if name == "ingress_pipe_crlf76":
            del text_d
        best = None
        for _ in range(2):  # the first pass also pools the hub's arenas and lanes
            got, err, dt = util.fd_decode(text, write_chunk=1 << 20, read_size=1 << 18,
                                          sock=sock, out=out)
            if got is None or got.size != N or not np.array_equal(got, xh):
                raise SystemExit(f"host_fd {name}: decode mismatch (errno {err})")
            best = dt if best is None else min(best, dt)
        res[name] = {"GiB_s": N / best / 2**30, "seconds": best,
                     "bytes_in": int(text.size)}
        del text
    del out
    chunk = 1 << 20
    framed = np.empty(util.framed_cap(N, chunk), np.uint8)
    framed.fill(0)
    g3 = _g3_digest()
    best = None
    for _ in range(2):
        got, err, dt = util.fd_encode(xh, max_chunk=chunk, out=framed)
        if got is None:
            raise SystemExit(f"host_fd egress failed (errno {err})")
        best = dt if best is None else min(best, dt)
    body = got.tobytes()
    h, pos, sizes = hashlib.sha256(), 0, []
    while True:
        eol = body.index(b"\r\n", pos)
        size = int(body[pos:eol], 16)
        pos = eol + 2
        if size == 0:
            break
        h.update(memoryview(body)[pos:pos + size])
        sizes.append(size)
        pos += size + 2
    # every chunk full but the last two: the body's last read comes up short
    # at EOF and the finalize characters are a read of their own (ref
    # src/base64encoder.c:124-131 -> finalize(), :61-99)
    ok = (g3 is None or h.hexdigest() == g3) and all(k == chunk for k in sizes[:-2])
    if not ok:
        raise SystemExit("host_fd egress: framed output mismatch")
    res["egress_pipe"] = {"GiB_s": N / best / 2**30, "seconds": best,
                          "framed_bytes": int(got.size), "chunks": len(sizes)}
    return res


def _g3_digest():
    try:
        with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as f:
            return json.load(f)["G3"]["out_sha256"]
    except (OSError, KeyError, ValueError):
        return None


def crlf76(chars: torch.Tensor) -> torch.Tensor:
    """RFC 2045 formatting on the device: 76-character lines, each followed
    by CRLF (the last, shorter one too)."""
    n = chars.numel()
    rows = (n + 75) // 76
    pad = rows * 76 - n
    body = torch.cat([chars, torch.zeros(pad, dtype=torch.uint8, device=chars.device)])
    crlf = torch.tensor([13, 10], dtype=torch.uint8, device=chars.device).expand(rows, 2)
    out = torch.cat([body.view(rows, 76), crlf], dim=1).reshape(-1)
    if pad:  # drop the zero padding of the last line (keep its CRLF)
        keep = torch.ones(out.numel(), dtype=torch.bool, device=chars.device)
        start = (rows - 1) * 78 + (76 - pad)
        keep[start:start + pad] = False
        out = out[keep]
    return out.contiguous()


def bench_mime(args, b64, steps=20):
    """MIME-formatted decode (SURVEY.md §8(d) dirty input): config 2's
    characters and config 4's rows in 76-character CRLF lines, decoded back
    and checked; device-resident, HIP events around each call.  Algorithmic
    bytes = characters read + bytes written."""
    N = args.size
    x = torch.empty(N, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    text = crlf76(b64.encode(x))
    out = torch.empty(b64.decoded_cap(text.numel()), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(b64.workspace_size(text.numel()), dtype=torch.uint8, device="cuda")
    res = torch.zeros(b64.RES_BYTES, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()

    spread = {}

    def timed(fn, name, sync_each=False):
        # calls back to back, each between two events of its own, one host
        # sync at the end (a sync after every call left the GPU idle between
        # calls, and the call after a longer host pause ran slow); the junk
        # legs sync after every call, so that each call finds the hint its
        # predecessor's probe left (the path the host picks reads it)
        fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(steps)]
        # the clock pre-heat, then two untimed calls (the copies leave the
        # leg's buffers cold in the caches and TLBs), queued right before the
        # first timed call: no idle gap
        preheat()
        fn()
        fn()
        for e0, e1 in evs:
            e0.record(stream)
            fn()
            e1.record(stream)
            if sync_each:
                e1.synchronize()
        torch.cuda.synchronize()
        ts = [e0.elapsed_time(e1) for e0, e1 in evs]
        spread[name] = {"ms_min": min(ts), "ms_median": statistics.median(ts), "ms_max": max(ts),
                        "ms_all": [round(t, 4) for t in ts]}
        return statistics.median(ts)

    ms = timed(lambda: b64.decode(text, out=out, workspace=ws, result=res, stream=stream),
               "cfg2_crlf76")
    info = b64.Decoded(out, res).info()
    if info.out_len != N or not torch.equal(out[:N], x):
        raise SystemExit("mime decode mismatch")
    alg = text.numel() + N
    single = {"workload": f"cfg2 characters in CRLF-76 lines: {text.numel()} bytes -> {N}",
              "ms": ms, "GiB_s": N / (ms * 1e-3) / 2**30,
              "alg_GBps": alg / (ms * 1e-3) / 1e9,
              "roofline_frac": alg / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9)}
    del text, out, ws
    # unstructured junk (not a BASELINE workload; the verdict's sparse and
    # 5 % cases): a '!' before each character with probability d
    junk = {}
    chars = b64.encode(x)
    for d in (0.001, 0.05):
        g = torch.Generator(device="cuda").manual_seed(7)
        mask = torch.rand(chars.numel(), device="cuda", generator=g) < d
        idx = torch.arange(chars.numel(), device="cuda") + torch.cumsum(mask, 0)
        text = torch.full((chars.numel() + int(mask.sum()),), ord("!"), dtype=torch.uint8,
                          device="cuda")
        text[idx] = chars
        del mask, idx
        out = torch.empty(b64.decoded_cap(text.numel()), dtype=torch.uint8, device="cuda")
        ws = torch.zeros(b64.workspace_size(text.numel()), dtype=torch.uint8, device="cuda")
        ms_j = timed(lambda: b64.decode(text, out=out, workspace=ws, result=res, stream=stream),
                     f"cfg2_junk{d:g}", sync_each=True)
        info = b64.Decoded(out, res).info()
        if info.out_len != N or not torch.equal(out[:N], x):
            raise SystemExit(f"junk {d} decode mismatch")
        # `ms` repeats one buffer, so from the second call on the probe's
        # hint (keyed on workspace, input address and length) picks the
        # single pass.  First calls: copies of the text at addresses the
        # hint has never seen, each decoded once (all alive, so no address
        # repeats), on the same workspace.
        copies = [text.clone() for _ in range(5)]
        preheat()
        torch.cuda.synchronize()
        cold = []
        for c in copies:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            b64.decode(c, out=out, workspace=ws, result=res, stream=stream)
            e1.record(stream)
            e1.synchronize()
            cold.append(e0.elapsed_time(e1))
            if not torch.equal(out[:N], x):
                raise SystemExit(f"junk {d} first-call decode mismatch")
        del copies
        cold_ms = statistics.median(cold)
        alg_j = text.numel() + N
        junk[f"cfg2_junk{d:g}"] = {
            "workload": f"cfg2 characters with junk density {d:g}: {text.numel()} bytes -> {N}",
            "ms": ms_j, "GiB_s": N / (ms_j * 1e-3) / 2**30,
            "alg_GBps": alg_j / (ms_j * 1e-3) / 1e9,
            "roofline_frac": alg_j / (ms_j * 1e-3) / (HBM_PEAK_GBS * 1e9),
            "ms_note": "repeat decodes of one buffer (the probe's hint applies from the second)",
            "cold_ms": cold_ms, "cold_ms_all": cold,
            "cold_roofline_frac": alg_j / (cold_ms * 1e-3) / (HBM_PEAK_GBS * 1e9),
            "cold_note": "first decode of each of 5 copies at new addresses (no hint)"}
        del text, out, ws
    del x, chars
    # config 4's rows, each in CRLF-76 lines (1,368 characters -> 18 lines)
    nbuf, L = 1 << 20, 1024
    E = b64.encoded_len(L)
    xr = torch.empty(nbuf * L, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(xr, 0x5EED)
    enc = torch.empty(nbuf * E, dtype=torch.uint8, device="cuda")
    b64.encode_strided(xr, L, L, nbuf, enc, E, stream=stream)
    lines = (E + 75) // 76
    rows = enc.view(nbuf, E)
    if lines * 76 != E:
        rows = torch.cat([rows, torch.full((nbuf, lines * 76 - E), 10, dtype=torch.uint8,
                                           device="cuda")], dim=1)
    crlf = torch.tensor([13, 10], dtype=torch.uint8, device="cuda").expand(nbuf, lines, 2)
    D = lines * 78
    mime = torch.cat([rows.reshape(nbuf, lines, 76), crlf], dim=2).reshape(-1).contiguous()
    del enc, rows
    cap = 12 * ((D + 15) // 16)
    dec = torch.empty(nbuf * cap, dtype=torch.uint8, device="cuda")
    outlen = torch.zeros(nbuf, dtype=torch.int64, device="cuda")
    ms4 = timed(lambda: b64.decode_strided(mime, D, D, nbuf, dec, cap, outlen, stream=stream),
                "cfg4_crlf76")
    if not (bool((outlen == L).all()) and
            bool(torch.equal(dec.view(nbuf, cap)[:, :L], xr.view(nbuf, L)))):
        raise SystemExit("mime batch decode mismatch")
    alg4 = nbuf * (D + L)
    batch = {"workload": f"cfg4 rows in CRLF-76 lines: {nbuf} x {D} bytes -> {L}",
             "ms": ms4, "GiB_s": nbuf * L / (ms4 * 1e-3) / 2**30,
             "alg_GBps": alg4 / (ms4 * 1e-3) / 1e9,
             "roofline_frac": alg4 / (ms4 * 1e-3) / (HBM_PEAK_GBS * 1e9)}
    for k, v in (("cfg2_crlf76", single), ("cfg4_crlf76", batch), *junk.items()):
        v.update(spread[k])
    return {"cfg2_crlf76": single, "cfg4_crlf76": batch, **junk, "unit": "ms, GiB/s payload",
            "steps": steps}


def bench_cfg5(args, world=1, rank=0):
    """BASELINE config 5: 16,384 Zipf messages (64 B - 1 MiB, SURVEY.md
    §8(d)), each its own queuestream -> GPU base64encoder stage ->
    chunkencoder(1 MiB) stack of the product's C API, drained 10,240 bytes
    per read (the reference's tcp_connection.c:22 pull size); host memory in,
    framed host memory out, so the rate includes every pinned copy and PCIe
    crossing.  T event loops (threads, one batching hub each) share the
    messages.

    One GPU: T = 1 and 16 (the box's CPU share), with the oracle's
    restatement of the same stack timed beside it on the same thread counts
    (whose outputs check a sample of the GPU stacks': cpu_baseline's checker
    role).  N GPUs: each rank takes its byte-balanced share of the messages
    (shard.by_bytes) on its own GPU, every loop of the rank on that GPU, 16
    loops per rank; the aggregate is all messages' bytes over the slowest
    rank's time (median of three passes, each started from a barrier); a
    sample of each rank's messages is checked against the oracle."""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    from async_amd import shard
    from oracle import pyoracle as orc
    from tests import util

    lens = util.zipf_lengths()
    nbytes_all = int(lens.sum())
    offs_all = np.concatenate([[0], np.cumsum(lens)])
    bounds = shard.by_bytes(lens.tolist(), world)
    b0, b1 = bounds[rank], bounds[rank + 1]
    payload = util.splitmix64(0x5EED, int(offs_all[b1]))[int(offs_all[b0]):]
    lens = lens[b0:b1]
    nbytes = int(lens.sum())
    offs = np.concatenate([[0], np.cumsum(lens)])
    device = torch.cuda.current_device()
    util.egress_stacks(payload[:4096], [64] * 64, 1 << 20, 10240, device=device)  # warm-up
    out = {"workload": f"cfg5: {offs_all.size - 1} Zipf messages, {nbytes_all} bytes, "
                       "queuestream -> encoder -> chunkencoder(1 MiB), 10,240-byte reads",
           "unit": "GiB/s of payload, host memory to host memory"}
    if world > 1:
        out["shards"] = {"by": "shard.by_bytes", "messages_per_rank":
                         [bounds[i + 1] - bounds[i] for i in range(world)]}
    sample = list(range(0, lens.size, max(1, lens.size // 64)))
    loop_counts = (1, min(16, args.cpu_threads)) if world == 1 else (min(16, args.cpu_threads),)
    for T in loop_counts:
        # one untimed pass first: T loops' hubs, lanes (HIP streams) and pinned
        # arenas come from process-wide pools, filled on first use
        util.egress_stacks(payload, lens, 1 << 20, 10240, raw=True, threads=T, device=device)
        # three timed passes, the median reported: the leg is host-bound and a
        # single pass varied 2x from box to box (profiles/README.md, r02_v25)
        passes = []
        for _ in range(3):
            times = np.zeros(2)
            sync_all(world)
            res, err = util.egress_stacks(payload, lens, 1 << 20, 10240, times=times,
                                          raw=True, threads=T, device=device)
            if res is None:
                raise SystemExit(f"cfg5 egress failed on rank {rank}: errno {err}")
            # the C side's clock: stack setup + the loops to completion (the
            # harness's output arrays are allocated and faulted in before it)
            wall = max_over_ranks(float(times.sum()), world)
            passes.append((wall, times.copy()))
            if len(passes) < 3:
                del res
        order = sorted(range(3), key=lambda i: passes[i][0])
        dt, times = passes[order[1]]
        framed, f_off, f_len = res
        for i in sample:
            want = orc.chunked_encode(payload[offs[i]:offs[i + 1]], max_chunk=1 << 20,
                                      read_size=10240)
            if framed[int(f_off[i]):int(f_off[i]) + int(f_len[i])].tobytes() != want:
                raise SystemExit(f"cfg5 egress mismatch at message {b0 + i}")
        leg = {"GiB_s": nbytes_all / dt / 2**30, "seconds": dt,
               "GiB_s_passes": [nbytes_all / p[0] / 2**30 for p in passes],
               "setup_s": float(times[0]), "loop_s": float(times[1]),
               "loops_per_gpu": T, "n_gpus": world}
        if world == 1:
            def work(t, T=T):
                cuts = np.searchsorted(offs, np.linspace(0, nbytes, T + 1))
                for i in range(cuts[t], cuts[t + 1]):
                    orc.chunked_encode(payload[offs[i]:offs[i + 1]], max_chunk=1 << 20,
                                       read_size=10240)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(T) as ex:
                list(ex.map(work, range(T)))
            cpu_dt = time.perf_counter() - t0
            leg.update({"framed_bytes": int(f_len.sum()),
                        "cpu_port_GiB_s": nbytes / cpu_dt / 2**30, "cpu_threads": T})
        else:
            leg["framed_bytes"] = int(sum(v[0] for v in gather_floats([float(f_len.sum())],
                                                                        world)))
        out[f"loops_{T}"] = leg
        del framed, res
    return out


def copy_ceilings(N: int, E: int, steps: int = 20) -> dict | None:
    """The measured copy bandwidth SURVEY.md 8(d) asks the roofline to be
    read against, per leg: the best of several copy kernels moving the same
    bytes as one launch of the leg (test-hooks build of the kernels,
    tests/csrc/libb64x_hooks.so; HIP's blit copy reaches only ~5.1 TB/s):
      - plain 16-byte non-temporal copies (half the bytes read, half
        written) in the sweep's shapes (1, 4 lanes' loads in flight; 256-
        and 1024-thread blocks; profiles/r02_copy_sweep.jsonl);
      - copies with the leg's own read/write mix: encode reads 12 bytes per
        lane and writes 16 (3 : 4), decode reads 16 and writes 12 (4 : 3),
        1, 2 or 4 in flight per lane.
    Each candidate: median of `steps` runs after 3 warm-ups, HIP events on
    torch's stream; the ceiling is the fastest candidate (GB/s of read +
    written bytes)."""
    import ctypes
    path = os.path.join(ROOT, "tests", "csrc", "libb64x_hooks.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    for fn in (lib.b64x__test_copy_mode,):
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                       ctypes.c_int]
        fn.restype = ctypes.c_int
    lib.b64x__test_copy_mix.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.b64x__test_copy_mix.restype = ctypes.c_int
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.empty(max(N, E) + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.fill_(7)

    def timed(launch):
        ts = []
        preheat()
        for i in range(steps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = launch()
            b.record()
            b.synchronize()
            if rc:
                raise RuntimeError(f"test copy: {rc}")
            if i >= 3:
                ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    plain = {}
    half = (N + E) // 2 // (1024 * 4 * 16) * (1024 * 4 * 16)
    for mode, shape in ((0, "U4 TH256"), (1, "U1 TH256"), (8, "U1 TH1024")):
        ms = timed(lambda: lib.b64x__test_copy_mode(src.data_ptr(), dst.data_ptr(), half,
                                                    stream, mode))
        plain[shape] = 2 * half / (ms * 1e-3) / 1e9
    ok = bool((dst[:half:1 << 16] == 7).all())  # the copies did move the bytes
    out = {"plain_GBps": plain, "checked": ok}
    for leg, mix, ib, ob, n_in in (("encode", 0, 12, 16, N), ("decode", 1, 16, 12, E)):
        best = max(plain.values())
        how = "plain " + max(plain, key=plain.get)
        for shape, U in enumerate((1, 2, 4)):
            units = n_in // ib // (256 * U) * (256 * U)
            ms = timed(lambda: lib.b64x__test_copy_mix(src.data_ptr(), dst.data_ptr(), units,
                                                       stream, mix, shape))
            gbps = units * (ib + ob) / (ms * 1e-3) / 1e9
            if gbps > best:
                best, how = gbps, f"mix {ib}->{ob} U{U} TH256"
        out[leg] = {"GBps": best, "best": how}
    del src, dst
    out["how"] = ("fastest of plain 16-B nt copies (sweep shapes) and copies with the leg's "
                  f"read/write mix, median of {steps} after 3 warm-ups")
    return out


def bench_root_scatter(world, rank, nbytes=1 << 30, steps=3):
    """SURVEY.md §8(e), reported, not optimised: rank 0 holds config 4's
    1 GiB and scatters each rank its 1/N share over the process group (RCCL
    over xGMI on a node).  Compare with `batch_cfg4`: encoding a share
    locally takes far less time than moving it, so the primary metric keeps
    inputs resident per rank."""
    if world == 1:
        return None
    dev = coll_device()
    share = nbytes // world
    mine = torch.empty(share, dtype=torch.uint8, device=dev)
    parts = [torch.empty(share, dtype=torch.uint8, device=dev) for _ in range(world)] \
        if rank == 0 else None
    try:
        dist.scatter(mine, parts, src=0)  # warm-up
        sync_all(world) if dev == "cuda" else dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            dist.scatter(mine, parts, src=0)
        sync_all(world) if dev == "cuda" else dist.barrier()
        dt = max_over_ranks((time.perf_counter() - t0) / steps, world)
    except RuntimeError as e:  # reported, never fatal to the line
        return {"error": str(e)[:200]}
    moved = share * (world - 1)
    return {"workload": f"{nbytes} B on rank 0, {share} B to each of {world - 1} ranks",
            "ms": dt * 1e3, "GB_s_out_of_rank0": moved / dt / 1e9}


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_batch(args):
    """The same oracle over config 4's shape (independent 1 KiB buffers, one
    reference stage each), one thread per core of this process's CPU share
    (ctypes drops the GIL), on a bounded sample of the batch."""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    from oracle import pyoracle

    threads = args.cpu_threads
    nbuf, L = args.cpu_batch_bufs, 1024
    E = (L + 2) // 3 * 4
    rows = np.random.default_rng(0x5EED).integers(0, 256, (nbuf, L), dtype=np.uint8)
    enc = np.empty((nbuf, E), dtype=np.uint8)
    dec = np.empty((nbuf, (E + 3) // 4 * 3), dtype=np.uint8)
    enc.fill(0)  # fault the pages in outside the timed region
    dec.fill(0)
    sl = [slice(i * nbuf // threads, (i + 1) * nbuf // threads) for i in range(threads)]
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda q: pyoracle.encode_rows(rows[q], enc[q]), sl))
        t1 = time.perf_counter()
        list(ex.map(lambda q: pyoracle.decode_rows(enc[q], dec[q]), sl))
        t2 = time.perf_counter()
    if not np.array_equal(dec[:, :L], rows):
        raise SystemExit("cpu batch baseline round trip mismatch")
    b = nbuf * L
    return {"value": b / (t2 - t0) / 2**30, "unit": "GiB/s", "cores": threads,
            "sample": f"cfg4 shape, {nbuf} x 1 KiB buffers ({b >> 20} MiB), "
                      f"encode {b / (t1 - t0) / 2**30:.2f} GiB/s, "
                      f"decode {b / (t2 - t1) / 2**30:.2f} GiB/s"}


def cpu_baseline(args, b64):
    import numpy as np

    from oracle import pyoracle

    n = args.cpu_sample
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    b64.fill_splitmix64(x, 0x5EED)
    host = x.cpu().numpy()
    t0 = time.perf_counter()
    e = pyoracle.encode(host, as_array=True)
    t1 = time.perf_counter()
    d = pyoracle.decode(e, as_array=True)
    t2 = time.perf_counter()
    if not np.array_equal(d, host):
        raise SystemExit("cpu baseline round trip mismatch")
    return {
        "value": n / (t2 - t0) / 2**30,
        "unit": "GiB/s",
        "cores": 1,
        "kind": "port",
        "cpu_model": cpu_model(),
        "all_core": cpu_baseline_batch(args),
        "sample": f"first {n >> 20} MiB of the cfg2 buffer: oracle/b64_oracle.c "
                  f"(scalar restatement of src/base64encoder.c + src/base64decoder.c, "
                  f"-O2, 1 thread), encode {n / (t1 - t0) / 2**30:.3f} GiB/s, "
                  f"decode {n / (t2 - t1) / 2**30:.3f} GiB/s; host "
                  f"{os.cpu_count()} logical CPUs",
    }


def dry_run_plans(world: int, rank: int) -> dict:
    """What the scaled legs do across ranks, without a GPU: config 4's and
    config 3's index shares and the one exchange (the all-gather of per-rank
    output totals, each rank contributing what its share would decode to),
    and config 5's byte-balanced message shares."""
    from async_amd import shard
    from tests import util

    curve = {"leg": "batch_cfg4", "scaling": "strong", "n_gpus": world}
    for name, total_buf, L in (("cfg4", 1 << 20, 1024), ("cfg3", 1 << 16, 4096)):
        lo, nbuf = shard.by_index(total_buf, world, rank)
        off, totals = shard.exchange_totals(nbuf * L, device=coll_device())
        if sum(totals) != total_buf * L or off != lo * L:
            raise SystemExit(f"{name}: exchange gave {totals}, offset {off}")
        shares = [int(v[0]) for v in gather_floats([float(nbuf)], world)]
        if name == "cfg4":
            curve.update({"buffers_per_rank": shares, "output_offsets_ok": True})
        else:
            curve["cfg3_buffers_per_rank"] = shares
    lens = util.zipf_lengths()
    bounds = shard.by_bytes(lens.tolist(), world)
    per_rank_bytes = [int(lens[bounds[i]:bounds[i + 1]].sum()) for i in range(world)]
    return {"scaling_curve": curve,
            "cfg5_egress": {"shards": {"by": "shard.by_bytes",
                                       "messages_per_rank": [bounds[i + 1] - bounds[i]
                                                             for i in range(world)],
                                       "bytes_per_rank": per_rank_bytes}}}


def launch_ranks(args) -> int:
    """--gpus N > 1 without a launcher: start one rank per GPU under
    torch.distributed.run as a child process (nothing here has touched the
    GPU yet) and relay its output; returns its exit code."""
    import socket
    import subprocess

    with socket.socket() as so:  # a free rendezvous port on the loopback
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
           f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def per_kernel_figures(r, ceiling, full):
    """The line's per-kernel keys: from bench_single's second pass (HIP events
    around each call), the copy ceilings and the committed PMC summary with
    --full; null in a plain run, which makes none of these measurements."""
    if not full:
        return dict.fromkeys(("encode_ms", "decode_ms", "encode_GBps", "decode_GBps",
                              "roundtrip_hbm_frac", "roofline"))
    N = r["N"]
    per_launch = N + r["E"]  # algorithmic bytes per launch (read + write)
    dom = "encode" if r["enc_ms"] >= r["dec_ms"] else "decode"
    dom_ms = max(r["enc_ms"], r["dec_ms"])
    achieved = per_launch / (dom_ms * 1e-3) / 1e9
    knames = ["k_encode_flat"] if dom == "encode" else \
        ["k_decode_probe", "k_decode_lines", "k_decode_suffix_held"]
    return {
        "encode_ms": r["enc_ms"],
        "decode_ms": r["dec_ms"],
        "encode_GBps": per_launch / (r["enc_ms"] * 1e-3) / 1e9,
        "decode_GBps": per_launch / (r["dec_ms"] * 1e-3) / 1e9,
        "roundtrip_hbm_frac": 2 * per_launch / ((r["enc_ms"] + r["dec_ms"]) * 1e-3)
                              / (HBM_PEAK_GBS * 1e9),
        "roofline": {
            "bound": "hbm",
            "kernel": "+".join(knames),
            "timing": "HIP events around each b64x call on its stream, mean over a second "
                      "pass of the K steps right after the timed region (events inside it "
                      "would add ~7 us of GPU idle per event)",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "copy_ceiling_GBps": ceiling[dom]["GBps"] if ceiling else None,
            "frac_of_copy": achieved / ceiling[dom]["GBps"] if ceiling else None,
            "frac_of_copy_per_leg": {
                "encode": per_launch / (r["enc_ms"] * 1e-3) / 1e9 / ceiling["encode"]["GBps"],
                "decode": per_launch / (r["dec_ms"] * 1e-3) / 1e9 / ceiling["decode"]["GBps"],
            } if ceiling else None,
            "copy_ceiling": ceiling,
            # the committed PMC summary is for the 1 GiB workload
            "traffic": load_traffic(knames) if N == 1 << 30 else None,
        },
    }


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # never report a line for a different GPU count than asked for
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    ndev = torch.cuda.device_count()
    if args.backend == "nccl" and world > ndev:
        print(f"bench.py: {world} ranks but {ndev} visible GPUs (RCCL needs one GPU per "
              "rank)", file=sys.stderr)
        sys.exit(2)
    if ndev:
        torch.cuda.set_device(local % ndev)
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.backend)
        if dist.get_world_size() != args.gpus:
            print(f"bench.py: process group has {dist.get_world_size()} ranks, "
                  f"--gpus {args.gpus}", file=sys.stderr)
            sys.exit(2)
    if args.dry_run:
        # the launch, the process group and the multi-rank plans of the
        # scaled legs, with their collectives (CPU tests, gloo): no GPU work
        ranks = gather_floats([float(rank)], world)
        scatter = bench_root_scatter(world, rank, nbytes=1 << 20, steps=2)
        plan = dry_run_plans(world, rank)
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world,
                              "process_group": {"backend": dist.get_backend() if world > 1
                                                else None, "world_size": world},
                              "ranks_seen": [int(r[0]) for r in ranks],
                              "root_scatter": scatter, **plan}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    from async_amd import b64

    b64.device_check()
    placement = bench_placement(b64)
    r = bench_single(args, world, rank, b64)
    full = args.full  # every leg but the headline's timed steps runs only with --full
    ceiling = copy_ceilings(r["N"], r["E"]) if full and rank == 0 else None
    batch = None if not full or args.no_batch else bench_batch(args, world, rank, b64)
    batch3 = None if not full or args.no_batch else bench_batch(args, world, rank, b64, 1 << 16,
                                                                4096, "cfg3")
    scatter = bench_root_scatter(world, rank) if full else None
    cpu = None
    if full and rank == 0 and world == 1 and not args.no_cpu:
        cpu = cpu_baseline(args, b64)
    host = None
    if full and rank == 0 and not args.no_host:
        host = bench_host_inclusive(args, b64)
    hostfd = None
    if full and rank == 0 and world == 1 and not args.no_host:
        hostfd = bench_host_fd(args, b64)
    mime = None
    if full and rank == 0 and world == 1 and not args.no_mime and args.size == 1 << 30:
        mime = bench_mime(args, b64)
    cfg5 = None
    if full and not args.no_cfg5 and (world > 1 or not args.no_cpu):
        cfg5 = bench_cfg5(args, world, rank)

    if rank == 0:
        N, E, K = r["N"], r["E"], r["K"]
        per_launch = N + E  # algorithmic bytes per launch (read + write)
        out = {
            "metric": METRIC,
            "value": world * N * K / r["wall"] / 2**30,
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "ms_per_step": r["wall"] / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic: splitmix64(0x5EED) bytes generated in HBM; round trip "
                    "verified bit-exact before timing",
            "config": {
                "workload": f"cfg2: one {N / 2**30:g} GiB buffer per GPU, encode (std "
                            "alphabet, pad) then decode, device-resident",
                "bytes_per_gpu": N,
                "chars_per_gpu": E,
                "parallelism": f"independent buffers x{world} (no data-path collective)",
            },
            "gpu_ms_per_step": r["gpu_ms_per_step"],
            "preheat_ms": PREHEAT_MS,
            # the headline fraction: both legs' algorithmic bytes over the
            # timed region's own GPU time per step (HIP events around the K
            # steps, nothing between them)
            "timed_region_frac": 2 * per_launch / (r["gpu_ms_per_step"] * 1e-3)
                                 / (HBM_PEAK_GBS * 1e9),
            "full": full,
            "dumped_outputs": args.dump_outputs,
            **per_kernel_figures(r, ceiling, full),
            # the north star's 1 -> 2 -> 4 -> 8 curve: config 4's fixed batch of
            # 1 M buffers, strong-scaled over the ranks (batch_cfg4); `value`
            # above is config 2, one buffer per rank (weak)
            "scaling_curve": {
                "leg": "batch_cfg4", "scaling": "strong", "n_gpus": world,
                "GiB_s": batch["value"] if batch else None,
                "per_rank_kernel_ms": batch["per_rank_kernel_ms"] if batch else None,
                "exchange_ms": batch["exchange_ms"] if batch else None,
                "ranks_amortised": batch["ranks_amortised"] if batch else None,
            } if full else None,
            "cpu_baseline": cpu,
            "batch_cfg4": batch,
            "batch_cfg3": batch3,
            "host_inclusive": host,
            "host_fd": hostfd,
            "root_scatter": scatter,
            "mime_decode": mime,
            "cfg5_egress": cfg5,
            "placement": placement,
            "process_group": {"backend": dist.get_backend() if world > 1 else None,
                              "world_size": dist.get_world_size() if world > 1 else 1},
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
