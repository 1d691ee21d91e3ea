"""bench.py's command line: a plain run times only the headline's steps and
leaves the other legs' keys null, --dump-outputs writes what the last timed
step computed, and the dump's sample of a large output is the same on every
run."""
import base64
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util

# what the line keeps null unless --full is given
FULL_ONLY = ("encode_ms", "decode_ms", "roofline", "scaling_curve", "cpu_baseline", "batch_cfg4",
             "batch_cfg3", "host_inclusive", "host_fd", "root_scatter", "mime_decode",
             "cfg5_egress")


def test_dump_sample_is_fixed_and_keeps_the_ends():
    """An output larger than DUMP_ELEMS is sampled: the first and last
    DUMP_EDGE elements whole, seeded sorted positions between them, float32;
    the same sample on every call, and a changed element at a kept position
    shows.  A small output is kept whole."""
    import bench
    n = bench.DUMP_ELEMS + 12345
    t = torch.arange(n, dtype=torch.int64).remainder(251).to(torch.uint8)
    a = bench.dump_sample(t, 7)
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ELEMS,)
    assert np.array_equal(a, bench.dump_sample(t, 7))
    edge = bench.DUMP_EDGE
    want = t.numpy().astype(np.float32)
    assert np.array_equal(a[:edge], want[:edge]) and np.array_equal(a[-edge:], want[-edge:])
    assert not np.array_equal(a, bench.dump_sample(t, 8))
    t[n - 1] ^= 1
    assert bench.dump_sample(t, 7)[-1] != a[-1]
    small = torch.tensor([1, 2, 250], dtype=torch.uint8)
    assert np.array_equal(bench.dump_sample(small, 7), np.array([1, 2, 250], np.float32))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR` on a small buffer:
    one line with the headline's keys, `steps` as asked, `ms_per_step` the
    wall time of one step, every other leg's key null; the dumped arrays are
    the characters and the bytes of the splitmix64 input (kept whole at this
    size), and the result record's lengths."""
    n = 300001  # not a multiple of 3: the last quantum is padded
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--size", str(n),
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3) / 2**30, rel=1e-9)
    for k in FULL_ONLY:
        assert line[k] is None, k
    x = util.splitmix64(0x5EED, n)
    chars = np.frombuffer(base64.b64encode(x.tobytes()), np.uint8)
    enc = np.load(tmp_path / "out" / "encoded.npy")
    dec = np.load(tmp_path / "out" / "decoded.npy")
    res = np.load(tmp_path / "out" / "decode_result.npy")
    assert enc.dtype == np.float32 and dec.dtype == np.float32 and res.dtype == np.float64
    assert np.array_equal(enc, chars.astype(np.float32))
    assert np.array_equal(dec, x.astype(np.float32))
    valid = int((chars != ord("=")).sum())  # out_len, alphabet characters seen, those mod 4
    assert valid == chars.size - 2 and res.tolist() == [n, valid, valid % 4]
    assert sorted(os.listdir(tmp_path / "out")) == ["decode_result.npy", "decoded.npy",
                                                    "encoded.npy"]
