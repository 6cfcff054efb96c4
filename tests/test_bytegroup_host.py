"""CPU: the byte-grouped layout and its block rule (include/qzstd_bytegroup.h) from qat-zstd-plugin_amd/frontend/qzstd_bytegroup.c built ALONE
— no HIP, no libzstd — against numpy, and the stand-alone checker tests/bytegroup/bytegroup_check.c (round trips, qzbgRebuild and its
refusals) compiled with -fsanitize=address,undefined and run as a process of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(B.PKG_DIR, "frontend", "qzstd_bytegroup.c")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(B.PKG_DIR, "frontend")]
KS = (1, 2, 4, 8)


def lengths(k):
    return [0, 1, k - 1, k, k + 1, 15, 16, 17, 4095, 4096, 4097, 131072 + k + 1]


@pytest.fixture(scope="module")
def bg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bytegroup") / "libqzbytegroup.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + INC + ["-o", so, SRC])
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "hip" not in undefined.lower() and "ZSTD" not in undefined, undefined
    return D.bind_bytegroup(C.CDLL(so))


def numpy_group(data: bytes, k: int) -> bytes:
    a = np.frombuffer(data, dtype=np.uint8)
    n = len(a) // k
    return a[:n * k].reshape(n, k).T.tobytes() + a[n * k:].tobytes()


@pytest.mark.parametrize("k", KS)
def test_group_is_a_transpose_and_ungroup_inverts_it(bg, k):
    rng = np.random.default_rng(k)
    for n in lengths(k):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        g = D.group_bytes(data, k, bg)
        assert g == numpy_group(data, k), (k, n)
        assert D.ungroup_bytes(g, k, bg) == data, (k, n)
        if k == 1:
            assert g == data


def test_bad_element_sizes(bg):
    for k in (0, 3, 5, 6, 7, 9, 16):
        with pytest.raises(ValueError):
            D.group_bytes(b"abcdefgh", k, bg)
        with pytest.raises(ValueError):
            D.ungroup_bytes(b"abcdefgh", k, bg)
        with pytest.raises(ValueError):
            D.group_blocks(8, k, bg)


def expected_ends(n_bytes, k):
    """the rule, spelled out: cuts at (j * n) & ~15 from n = 4096 on, every piece cut every 128 KiB from its own start"""
    n = n_bytes // k
    cuts = [(j * n) & ~15 for j in range(1, k)] if k > 1 and n >= 4096 else []
    ends, start = [], 0
    for piece_end in cuts + [n_bytes]:
        while start < piece_end:
            start = min(start + 131072, piece_end)
            ends.append(start)
    return ends


@pytest.mark.parametrize("k", KS)
def test_block_rule(bg, k):
    sizes = lengths(k) + [4096 * k - 1, 4096 * k, 4096 * k + 1, 4096 * k + k - 1, 8192 * k + 3, 32768, 131072, 131073, 393216, 393216 + 5,
                          1048576 + 3 * k + 1]
    for L in sizes:
        ends = D.group_blocks(L, k, bg)
        n = L // k
        if L == 0:
            assert ends == []
            continue
        assert ends == sorted(set(ends)) and ends[-1] == L, (k, L)
        starts = [0] + ends[:-1]
        assert all(s % 16 == 0 for s in starts), (k, L)
        assert all(0 < e - s <= 131072 for s, e in zip(starts, ends)), (k, L)
        if k == 1 or n < 4096:
            assert ends == [min(o + 131072, L) for o in range(0, L, 131072)], (k, L)  # today's blocks: no cuts below n = 4096
        else:
            for j in range(1, k):
                assert (j * n) & ~15 in ends, (k, L, j)
        assert ends == expected_ends(L, k), (k, L)
        # sizing call: the count without an array, and a short array is not overrun
        assert bg.QZSTD_byteGroupBlocks(L, k, None, 0) == len(ends)
        few = (C.c_size_t * 2)(7, 7)
        assert bg.QZSTD_byteGroupBlocks(L, k, few, 1) == len(ends) and few[0] == ends[0] and few[1] == 7


def test_planes_of_192k_are_cut_again_at_128k(bg):
    assert D.group_blocks(393216, 2, bg) == [131072, 196608, 196608 + 131072, 393216]
    assert D.group_blocks(4096 * 2, 2, bg) == [4096, 8192] and D.group_blocks(4096 * 2 - 2, 2, bg) == [8190]
    assert D.group_blocks(131072, 8, bg) == [16384 * j for j in range(1, 9)]
    # a plane that does not start on a multiple of 16: the cut falls just in front of it
    assert D.group_blocks(2 * 5001, 2, bg) == [4992, 10002]


def test_standalone_checker_under_asan_ubsan(tmp_path):
    """round trips, qzbgRebuild on generated entries, and every malformed case refused with the guard bytes intact — in a process of its own"""
    exe = str(tmp_path / "bytegroup_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + INC +
                          ["-o", exe, os.path.join(ROOT, "tests", "bytegroup", "bytegroup_check.c"), SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-3000:])
