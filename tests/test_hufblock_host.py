"""CPU: include/qzstd_hufblock.h alone — code lengths, canonical codes, the two tree descriptions, the four streams, the block body and the
rule — through tests/hufblock/hufblock_check.c: built -shared, each input wrapped in a frame of one Huffman-only block and handed to
libzstd's decoder, which must return the input; and as an executable with -fsanitize=address,undefined that runs the same kinds of input
in a process of its own (no Python process loads sanitized code)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hufblock", "hufblock_check.c")
INC = ["-I" + os.path.join(ROOT, "include")]
LENS = (1024, 1025, 1026, 1027, 16383, 16384, 65536, 131072)
AUTO, DIRECT, FSE = 0, 1, 2
GAIN = ("two symbols", "fibonacci counts", "symbols 200-255", "255 with 0 present", "bf16 high plane", "fp32 plane 0")
NOISE = ("bf16 low plane", "fp32 plane 1", "fp32 plane 2", "fp32 plane 3")  # mantissa bytes: nothing to gain, perhaps no tree of under 128 bytes


@pytest.fixture(scope="module")
def hb(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hufblock") / "libhufblock.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + INC + ["-o", so, SRC])
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "hip" not in undefined.lower() and "ZSTD" not in undefined, undefined
    L = C.CDLL(so)
    L.hb_lengths.restype = C.c_uint
    L.hb_lengths.argtypes = [C.c_char_p, C.c_uint, C.c_void_p]
    L.hb_kraft.restype = C.c_uint
    L.hb_kraft.argtypes = [C.c_void_p]
    L.hb_tree.restype = C.c_size_t
    L.hb_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hb_frame.restype = C.c_size_t
    L.hb_frame.argtypes = [C.c_char_p, C.c_uint, C.c_int, C.c_void_p, C.c_size_t]
    L.hb_takes.restype = C.c_int
    L.hb_takes.argtypes = [C.c_uint] * 5
    return L


@pytest.fixture(scope="module")
def zstd():
    return B.Zstd()


def planes(kind, size, nbytes):
    """the byte planes of typed_corpus(kind), most significant first"""
    raw = np.frombuffer(D.typed_corpus(kind, nbytes * size, seed=3), dtype=np.uint8).reshape(-1, size)
    return [np.ascontiguousarray(raw[:, j]) for j in range(size - 1, -1, -1)]


def inputs(n):
    """name -> n bytes"""
    rng = np.random.default_rng(n)
    out = {}
    out["two symbols"] = rng.choice(np.array([3, 90], dtype=np.uint8), n, p=[0.9, 0.1])
    out["256 equal counts"] = (np.arange(n) % 256).astype(np.uint8)
    fib = [1, 1]
    while sum(fib) < n:
        fib.append(fib[-1] + fib[-2])
    out["fibonacci counts"] = rng.permutation(np.repeat(np.arange(len(fib)), fib).astype(np.uint8)[:n] + 10)
    out["symbols 200-255"] = (200 + np.minimum(rng.geometric(0.2, n) - 1, 55)).astype(np.uint8)
    out["255 with 0 present"] = rng.choice(np.array([0, 255, 17, 99], dtype=np.uint8), n, p=[0.5, 0.3, 0.15, 0.05])
    p129 = np.full(129, 0.2 / 120)
    p129[:9] = 0.8 / 9
    few = rng.choice(129, n, p=p129 / p129.sum()).astype(np.uint8)
    few[:129] = np.arange(129)  # all of them occur: 128 weights are listed
    out["129 symbols"] = few
    out["bf16 high plane"] = planes("bf16", 2, n)[0]
    out["bf16 low plane"] = planes("bf16", 2, n)[1]
    for j, p in enumerate(planes("fp32", 4, n)):
        out["fp32 plane %d" % j] = p
    return out


def frame(hb, data, form):
    cap = len(data) * 2 + 1024
    dst = C.create_string_buffer(cap)
    n = hb.hb_frame(data.tobytes(), len(data), form, dst, cap)
    return dst.raw[:n]


@pytest.mark.parametrize("n", LENS)
def test_every_input_decodes_through_libzstd_in_both_tree_forms(hb, zstd, n):
    seen = set()
    for name, data in inputs(n).items():
        raw = data.tobytes()
        nbits = (C.c_ubyte * 256)()
        depth = hb.hb_lengths(raw, n, nbits)
        lens = np.frombuffer(nbits, dtype=np.uint8)
        present = np.bincount(data, minlength=256) > 0
        assert 1 <= depth <= 11 and lens.max() == depth, (name, depth)
        assert ((lens > 0) == present).all(), name
        assert hb.hb_kraft(nbits) == 2048, (name, hb.hb_kraft(nbits))  # complete: sum of 2^-nbits is exactly 1
        assert int((2.0 ** (11 - lens[present].astype(np.int64))).sum()) == 2048
        tree = C.create_string_buffer(129)
        sizes = {form: hb.hb_tree(nbits, tree, 129, form) for form in (AUTO, DIRECT, FSE)}
        last = int(np.flatnonzero(present)[-1])
        assert (sizes[DIRECT] > 0) == (last <= 128), (name, last)  # at most 128 listed weights
        if sizes[DIRECT]:
            assert sizes[DIRECT] == 1 + (last + 1) // 2
        usable = [s for s in (sizes[DIRECT], sizes[FSE]) if s]
        assert sizes[AUTO] == (min(usable) if usable else 0), (name, sizes)
        for form in (AUTO, DIRECT, FSE):
            f = frame(hb, data, form)
            if not f:  # no tree in this form; or noise that does not fit the section header's size field
                assert not sizes[form] or name in NOISE, (name, form)
                continue
            if len(f) - 12 > n:  # a block may not be larger than what it holds: no such frame is ever written
                assert name in NOISE, (name, form, len(f))
                continue
            assert zstd.decompress(f, n) == raw, (name, form)
            seen.add((name, form))
            if form == AUTO and name in GAIN:
                assert len(f) < n * 3 // 4, (name, len(f))
        if name == "256 equal counts":
            assert not usable  # weights all equal, too many for the direct form: not coded
        elif name not in NOISE:
            assert (name, AUTO) in seen, name
    # what the cases are there for
    assert ("two symbols", DIRECT) in seen and ("symbols 200-255", FSE) in seen and ("255 with 0 present", FSE) in seen
    assert ("129 symbols", DIRECT) in seen and ("129 symbols", FSE) in seen
    assert ("bf16 high plane", FSE) in seen and ("fp32 plane 0", FSE) in seen  # the sign bit: symbols above 128
    assert ("symbols 200-255", DIRECT) not in seen


def test_the_workload_forces_length_limiting(hb):
    """an unlimited Huffman code of these inputs is deeper than 11: the limit is met by the halving, not by chance"""
    def unlimited_depth(data):
        import heapq
        h = [(int(c), i, 0) for i, c in enumerate(np.bincount(data, minlength=256)) if c]
        heapq.heapify(h)
        tick = 256
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            heapq.heappush(h, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
            tick += 1
        return h[0][2]
    for name in ("fibonacci counts", "bf16 high plane"):
        data = inputs(65536)[name]
        assert unlimited_depth(data) > 11, name
        nbits = (C.c_ubyte * 256)()
        assert hb.hb_lengths(data.tobytes(), len(data), nbits) == 11, name


def test_fewer_than_two_symbols_is_not_coded(hb):
    nbits = (C.c_ubyte * 256)()
    assert hb.hb_lengths(bytes([61]) * 4096, 4096, nbits) == 0 and not any(nbits)
    assert not frame(hb, np.full(4096, 61, dtype=np.uint8), AUTO)


def test_the_rule(hb):
    assert hb.hb_takes(500, 600, 1024, 0xFFFFFFFF, 1) == 0  # the matcher failed the block
    assert hb.hb_takes(0, 600, 4096, 4096, 1) == 0 and hb.hb_takes(500, 0, 4096, 4096, 1) == 0  # not coded
    assert hb.hb_takes(500, 1024 - 18, 1024, 1024, 1) == 1 and hb.hb_takes(500, 1024 - 17, 1024, 1024, 1) == 0  # (len >> 6) + 2
    assert hb.hb_takes(512, 600, 1024, 1024 - 6, 2) == 1 and hb.hb_takes(512, 600, 1024, 1024 - 7, 2) == 0  # 24 eighths a sequence
    assert hb.hb_takes(8225, 8300, 65536, 300, 40) == 0  # zero runs: matches win
    assert hb.hb_takes(40000, 40100, 131072, 131072, 1) == 1 and hb.hb_takes(400, 500, 1023, 1023, 1) == 0


def test_standalone_checker_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "hufblock_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + INC + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-1500:], out.stderr[-3000:])
