"""CPU: include/qzstd_planecost.h alone — the order-0 cost of a block from its byte histogram and the rule that predicts a Raw_Block from it —
through tests/planecost/planecost_check.c: built -shared for the comparisons with numpy's floating-point entropy, and as an executable
with -fsanitize=address,undefined that checks the exact cases in a process of its own (no Python process loads sanitized code)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "planecost", "planecost_check.c")
INC = ["-I" + os.path.join(ROOT, "include")]
LEN_MAX = 131072


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("planecost") / "libplanecost.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + INC + ["-o", so, SRC])
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "hip" not in undefined.lower() and "ZSTD" not in undefined, undefined
    L = C.CDLL(so)
    L.pc_log2.restype = C.c_uint32
    L.pc_log2.argtypes = [C.c_uint32]
    L.pc_cost.restype = C.c_uint32
    L.pc_cost.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    L.pc_is_raw.restype = C.c_int
    L.pc_is_raw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return L


def cost(pc, hist):
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    assert len(h) == 256
    return pc.pc_cost(h.ctypes.data_as(C.POINTER(C.c_uint32)), int(h.sum()))


def exact(hist):
    """the order-0 cost in bytes, in floating point: sum c * log2(len / c) / 8"""
    h = np.asarray(hist, dtype=np.float64)
    h = h[h > 0]
    return float((h * np.log2(h.sum() / h)).sum() / 8.0) if len(h) else 0.0


def slack(n):
    """the header's stated rounding: two values of L per term, about one unit of 1 / 256 bit each, over 2048 units a byte; the final ceil"""
    return n / 1024.0 + 1.0


def test_log2_table_against_numpy(pc):
    xs = np.unique(np.concatenate([np.arange(1, 4097), np.random.default_rng(1).integers(1, LEN_MAX + 1, 4000), [LEN_MAX - 1, LEN_MAX]]))
    got = np.array([pc.pc_log2(int(x)) for x in xs], dtype=np.float64)
    assert np.abs(got - 256.0 * np.log2(xs)).max() <= 1.001  # 0.5 (the table) + 0.5 (the interpolation's rounding) + the chord's 0.001
    assert pc.pc_log2(0) == 0


def histograms():
    rng = np.random.default_rng(7)
    one = np.zeros(256, dtype=np.uint32)
    one[9] = 5000
    two = np.zeros(256, dtype=np.uint32)
    two[3], two[200] = 1000, 3000
    top = np.zeros(256, dtype=np.uint32)
    top[0] = LEN_MAX
    out = [("one value", one), ("two values", two), ("uniform", np.full(256, 512, dtype=np.uint32)), ("one bin at 131072", top),
           ("uniform, not a multiple of 256", np.bincount(np.arange(100001) % 256, minlength=256))]
    for i, n in enumerate((1, 64, 255, 4097, 65536, LEN_MAX)):
        out.append(("random bytes %d" % n, np.bincount(rng.integers(0, 256, n), minlength=256)))
        skew = np.minimum(rng.geometric(0.3, n), 255)  # an exponent-like plane: a handful of values
        out.append(("skewed %d" % n, np.bincount(skew, minlength=256)))
        out.append(("random histogram %d" % i, rng.multinomial(n, rng.dirichlet(np.full(256, 0.1)))))
    return out


def test_cost_against_the_float_computation(pc):
    for name, h in histograms():
        n = int(np.sum(h))
        got, want = cost(pc, h), exact(h)
        assert abs(got - want) <= slack(n), (name, got, want)
    assert cost(pc, histograms()[0][1]) == 0 and cost(pc, histograms()[3][1]) == 0
    assert cost(pc, np.zeros(256, dtype=np.uint32)) == 0  # an empty block


def test_uniform_block_is_never_above_len_by_more_than_the_rounding(pc):
    for n in (256, 4096, LEN_MAX):
        assert cost(pc, np.full(256, n // 256)) == n  # 256 equal counts: exactly len
    for n in (257, 1000, 4097, 100001, LEN_MAX - 1):
        assert cost(pc, np.bincount(np.arange(n) % 256, minlength=256)) <= n + slack(n)


def test_is_raw_at_both_edges(pc):
    for n in (64, 4096, 65536, LEN_MAX):
        gain = (n >> 6) + 2
        assert pc.pc_is_raw(n - (gain - 1), n, 0) == 1 and pc.pc_is_raw(n - gain, n, 0) == 0
        assert pc.pc_is_raw(n, n, gain - 1) == 1 and pc.pc_is_raw(n, n, gain) == 0
        assert pc.pc_is_raw(n + 100, n, 0) == 1  # min(cost, len)


def test_short_and_failed_blocks_are_never_raw(pc):
    for n in range(0, 64):
        assert pc.pc_is_raw(n, n, 0) == 0
    assert pc.pc_is_raw(64, 64, 0) == 1
    assert pc.pc_is_raw(4096, 4096, 0xFFFFFFFF) == 0  # QZSTD_PLANE_MATCH_FAILED
    assert pc.pc_is_raw(LEN_MAX + 1, LEN_MAX + 1, 0) == 0


def test_flat_histogram_with_long_repeats_stays_out(pc):
    block = np.arange(8192, dtype=np.uint32) % 256  # bytes 0..255 tiled
    h = np.bincount(block, minlength=256)
    c = cost(pc, h)
    assert c == 8192  # flat: the histogram alone says raw ...
    assert pc.pc_is_raw(c, 8192, 0) == 1
    assert pc.pc_is_raw(c, 8192, 8192 - 256) == 0  # ... the matches (everything behind the first tile) say otherwise


def test_standalone_checker_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "planecost_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + INC + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-1500:], out.stderr[-3000:])
