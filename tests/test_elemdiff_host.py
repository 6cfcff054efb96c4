"""CPU: element differences and their sum (include/qzstd_elemdiff.h) from qat-zstd-plugin_amd/frontend/qzstd_elemdiff.c built ALONE — no
HIP, no libzstd — against numpy, and the stand-alone checker tests/elemdiff/elemdiff_check.c (round trips out of place and in place, guard
bytes, tails, hand-worked vectors) compiled with -fsanitize=address,undefined and run as a process of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(B.PKG_DIR, "frontend", "qzstd_elemdiff.c")
INC = ["-I" + os.path.join(ROOT, "include")]
KS = (1, 2, 4, 8)


def lengths(k):
    return [0, 1, k - 1, k, k + 1, 16384 - k, 16384, 16384 + k, 100003]


@pytest.fixture(scope="module")
def ed(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("elemdiff") / "libqzelemdiff.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + INC + ["-o", so, SRC])
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "hip" not in undefined.lower() and "ZSTD" not in undefined, undefined
    return D.bind_elemdiff(C.CDLL(so))


def numpy_diff(data: bytes, k: int) -> bytes:
    """the header's rule, restated: d = x - previous x (mod 2^(8k)), z = (d << 1) ^ (0 - (d >> (8k - 1))), the tail unchanged"""
    a = np.frombuffer(data, dtype=np.uint8)
    n = len(a) // k
    x = a[:n * k].view("<u%d" % k)
    with np.errstate(over="ignore"):
        d = x - np.concatenate([np.zeros(1, dtype=x.dtype), x[:-1]])[:n]
        z = (d << x.dtype.type(1)) ^ (x.dtype.type(0) - (d >> x.dtype.type(8 * k - 1)))
    return z.astype("<u%d" % k).tobytes() + a[n * k:].tobytes()


def inputs(n, k, rng):
    m = n // k
    yield "random", rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    yield "all 0xFF", b"\xff" * n
    tail = bytes(rng.integers(0, 256, n - m * k, dtype=np.uint8))
    top = (1 << (8 * k)) - 1
    desc = (top - 3 * np.arange(m, dtype=np.uint64)) & np.uint64(top)
    yield "descending", desc.astype("<u%d" % k).tobytes() + tail
    wrap = np.where(np.arange(m) % 2 == 0, 0, top).astype(np.uint64)
    yield "wrapping", wrap.astype("<u%d" % k).tobytes() + tail


@pytest.mark.parametrize("k", KS)
def test_diff_matches_the_rule_and_sum_inverts_it(ed, k):
    rng = np.random.default_rng(k)
    for n in lengths(k):
        for name, data in inputs(n, k, rng):
            z = D.elem_diff(data, k, ed)
            assert z == numpy_diff(data, k), (k, n, name)
            assert z[n // k * k:] == data[n // k * k:], (k, n, name)  # the tail: untouched
            assert D.elem_sum(z, k, ed) == data, (k, n, name)
            buf = C.create_string_buffer(data, max(n, 1))  # in place, both ways
            assert ed.QZSTD_elemDiff(buf, buf, n, k) == n and buf.raw[:n] == z, (k, n, name)
            assert ed.QZSTD_elemSum(buf, buf, n, k) == n and buf.raw[:n] == data, (k, n, name)


def test_hand_worked_vectors(ed):
    x = np.array([1, 0, 0xFFFF], dtype="<u2").tobytes()
    assert D.elem_diff(x, 2, ed) == np.array([2, 1, 1], dtype="<u2").tobytes()
    assert D.elem_diff(bytes([0, 255, 0, 128]), 1, ed) == bytes([0, 1, 2, 255])
    assert D.elem_diff(np.array([10, 13, 12, 12], dtype="<u4").tobytes() + b"xyz", 4, ed) == np.array([20, 6, 1, 0], dtype="<u4").tobytes() + b"xyz"
    assert D.elem_diff(np.array([1 << 63, 0], dtype="<u8").tobytes(), 8, ed) == b"\xff" * 16
    assert D.elem_sum(np.array([2] * 5, dtype="<u8").tobytes(), 8, ed) == np.arange(1, 6, dtype="<u8").tobytes()


def test_bad_element_sizes(ed):
    for k in (0, 3, 5, 6, 7, 9, 16, 0x81):
        with pytest.raises(ValueError):
            D.elem_diff(b"abcdefgh", k, ed)
        with pytest.raises(ValueError):
            D.elem_sum(b"abcdefgh", k, ed)


def test_the_front_end_exports_the_same_functions():
    F = D.bind_elemdiff(B.Front().lib)
    data = np.random.default_rng(1).integers(0, 256, 40003, dtype=np.uint8).tobytes()
    for k in KS:
        assert D.elem_diff(data, k, F) == numpy_diff(data, k) and D.elem_sum(D.elem_diff(data, k, F), k, F) == data


def test_standalone_checker_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "elemdiff_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + INC +
                          ["-o", exe, os.path.join(ROOT, "tests", "elemdiff", "elemdiff_check.c"), SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])
