"""CPU checks of the reciprocal divisions behind b64x_decode_strided's rows
with room (async_amd/csrc/b64x_kernels.hip): the launcher's gate on
magic = ceil(2^32 / S) (decode_choice), and k_rows_prep's rcpS, rcp, mL and
m, k.  Each is restated here and checked over the whole range its gate
claims, the extreme operand first; tests/test_decode_dispatch.py ties the
restatements to the kernels.  No GPU needed."""
import ctypes

import numpy as np

from tests import util

K_THREADS = 256
K_ROWS_U = 4
REL_SPAN = K_ROWS_U * K_THREADS  # a block's lane slots: rel < S + REL_SPAN
U64 = np.uint64


def launcher_gate(s):
    """decode_choice's magic for S slots per row and whether relmax * e < 2^32."""
    magic = (0xFFFFFFFF + s) // s
    e = magic * s - (1 << 32)
    return magic, (s + REL_SPAN) * e < (1 << 32)


def prep_gate(sm, in_stride):
    """k_rows_prep's gate on the model's slot count (len >= 32 besides)."""
    _, ok = launcher_gate(sm)
    return sm >= 2 and ok and ((sm + REL_SPAN) // sm + 1) * in_stride < (1 << 40)


def rcp_s(sq):
    """k_rows_prep's rcpS for Sq slots per row (0: the 32-bit multiply-high)."""
    rs = ((1 << 20) + sq - 1) // sq
    return rs if (sq + REL_SPAN) * (rs * sq - (1 << 20)) < (1 << 20) else 0


def umul24(a, b):
    """__umul24 on arrays: the low 24 bits of each operand, the low 32 of the product."""
    return ((a & U64(0xFFFFFF)) * (b & U64(0xFFFFFF))) & U64(0xFFFFFFFF)


def test_launcher_gate_admits_only_exact_divisions():
    """For every S in [2, 2^20) that passes relmax * e < 2^32, the
    multiply-high splits rel exactly at S - 1, S and relmax - 1 (the error
    rel * e grows with rel).  The named S lie on the side the gate's
    arithmetic puts them, and the launcher's own decision function agrees
    with the restatement for every S."""
    s = np.arange(2, 1 << 20, dtype=U64)
    magic = (U64(0xFFFFFFFF) + s) // s
    e = magic * s - U64(1 << 32)
    ok = (s + U64(REL_SPAN)) * e < U64(1 << 32)
    for rel in (s + U64(REL_SPAN - 1), s, s - U64(1)):
        q = (rel * magic) >> U64(32)
        assert np.array_equal(q[ok], (rel // s)[ok])
    passing = set(s[ok].tolist())
    assert all(x in passing for x in range(2, 65094))
    for want, x in ((True, 65093), (False, 65094), (True, 65536), (False, 65537),
                    (True, 1048321)):
        assert (x in passing) == want == launcher_gate(x)[1], x
    assert max(passing) == 1048321
    assert int((~ok[65094 - 2:]).sum()) == 922270
    # past the gate the division does go wrong for some S, at the last rel
    # before a multiple of S (so a gate is needed; this one is sufficient)
    bad = s[~ok]
    rel = (bad + U64(REL_SPAN - 1)) // bad * bad - U64(1)
    assert ((rel * magic[~ok]) >> U64(32) != rel // bad).any()
    L = util.hooks()
    L.b64x__test_decode_rows_path.argtypes = [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
        ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    L.b64x__test_decode_rows_path.restype = ctypes.c_int
    fn, src, dst = L.b64x__test_decode_rows_path, 1 << 30, 1 << 40
    for x in range(2, (1 << 20) + 2):
        route = fn(src, 16 * x, 16 * x, 3, dst, 12 * x, None)
        assert route == (2 if x in passing else 3), x


def test_rcps_is_exact_wherever_the_prep_sets_it():
    """For every Sq in [1, 2^20) where k_rows_prep sets rcpS, the 24-bit
    product splits every rel < Sq + 1,024 exactly; the product is taken as
    __umul24 gives it (32 bits).  The first Sq it refuses are the issue's."""
    sq = np.arange(1, 1 << 20, dtype=U64)
    rs = (U64((1 << 20) - 1) + sq) // sq
    ok = (sq + U64(REL_SPAN)) * (rs * sq - U64(1 << 20)) < U64(1 << 20)
    assert [int(x) for x in sq[~ok][:4]] == [657, 670, 673, 680]
    assert all(rcp_s(x) == 0 for x in (657, 670, 673, 680))
    assert all(rcp_s(x) for x in (2, 86, 417, 656, 658, 1 << 19))
    for x, r in zip(sq[ok].tolist(), rs[ok].tolist()):
        rel = np.arange(x + REL_SPAN, dtype=U64)[::-1]
        bl = umul24(rel, U64(r)) >> U64(20)
        assert np.array_equal(bl, rel // U64(x)), x
        assert np.array_equal(rel - umul24(bl, U64(x)), rel % U64(x)), x


def test_rcp_divides_by_the_line_length_in_the_bands():
    """The bands' line division, 16 S <= 4,096: (i * ceil(2^20 / L)) >> 20 ==
    i // L for every L in [16, 252] and i = 16 q <= 4,080 (4,080 * 251 against
    2^20 is the margin)."""
    i = np.arange(4080, -1, -16, dtype=U64)
    for L in range(16, 253):
        rcp = U64(((1 << 20) + L - 1) // L)
        assert np.array_equal(umul24(i, rcp) >> U64(20), i // U64(L)), L


def test_ml_divides_by_the_line_length_below_2_24():
    """Slot by slot: umulhi(i, ceil(2^32 / L)) == i // L for every L in
    [16, 252] at the largest i = 16 (2^20 - 1) = 2^24 - 16, at every i = 16 q
    next to a multiple of L near it, and for a few L at every i = 16 q."""
    top = (1 << 24) - 16
    for L in range(16, 253):
        ml = (0xFFFFFFFF + L) // L
        assert ml < (1 << 32)
        near = {top}
        for k in range(top // L - 40, top // L + 1):
            near.update(x for x in (k * L - 1, k * L, k * L + 15) if x % 16 == 0 and x <= top)
            near.add((k * L - 1) // 16 * 16)
        for i in sorted(near, reverse=True):
            assert (i * ml) >> 32 == i // L, (L, i)
    i = np.arange(top, -1, -16, dtype=U64)
    for L in (16, 19, 64, 76, 251, 252):
        ml = U64((0xFFFFFFFF + L) // L)
        assert np.array_equal((i * ml) >> U64(32), i // U64(L)), L


def test_m_k_divide_by_the_line_length_below_2_31():
    """(i * m) >> (31 + k) == i // L with k = bits of L - 1 and m =
    ceil(2^(31 + k) / L), a 32-bit value, at i = 2^31 - 1, L and L - 1."""
    for L in range(16, 253):
        k = (L - 1).bit_length()
        m = ((1 << (31 + k)) + L - 1) // L
        assert m < (1 << 32), L
        for i in ((1 << 31) - 1, (1 << 31) - L, L, L - 1):
            assert (i * m) >> (31 + k) == i // L, (L, i)


def test_prep_and_launcher_gates_on_the_named_crlf76_rows():
    """The four (launcher gate, prep gate) outcomes for CRLF-76 rows: the
    sample (lines, bytes, S, Sm) tuples give those S and Sm and fall where
    they are said to."""
    for lines, nbytes, s, sm, launcher, prep in (
            (13000, 1014000, 63375, 61750, True, True),
            (13437, 1048086, 65506, 63826, False, True),
            (13704, 1068912, 66807, 65094, True, False),
            (14058, 1096524, 68533, 66776, False, False)):
        assert nbytes == 78 * lines and s == (nbytes + 15) // 16
        assert sm == (76 * lines + 15) // 16
        assert launcher_gate(s)[1] == launcher, s
        assert prep_gate(sm, nbytes) == prep, sm
