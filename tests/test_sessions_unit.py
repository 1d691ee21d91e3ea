"""Where the ABI's host side lives: the sessions unit is host
code only, and the kernel unit holds none of it.  CPU only; reads source
text, in the style of test_abi.py::test_kernel_barriers_wait_for_lds."""
import os
import re

from tests import util

ROOT = util.ROOT


def _code(name):
    src = open(os.path.join(ROOT, "async_amd", "csrc", name)).read()
    return re.sub(r"//[^\n]*", "", src)


def test_sessions_unit_is_host_only():
    """Thread placement, sessions and batch lanes are host code in a unit of
    their own (b64x_sessions.cpp) that holds no device code and launches no
    kernel, and none of them is left in the kernel unit: a change to them
    cannot change the kernels' code."""
    host = _code("b64x_sessions.cpp")
    for word in ("__global__", "__device__", "hipLaunchKernelGGL", "<<<"):
        assert word not in host, word
    kernels = _code("b64x_kernels.hip")
    for word in ("b64x_session_", "b64x_lane_", "b64x_bind_thread", "b64x_host_alloc"):
        assert word not in kernels, word
