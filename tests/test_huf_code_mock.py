"""CPU: qzstd_hip_huf_code's outputs as the CPU stand-in gives them (tests/mock/mock_hip_huf_code.c, built alone) are what a frame needs: for every
row with a size word, the 128 bytes of code lengths and the jump table + streams from the dense area, put into QZSTD_hufBlockBody
(include/qzstd_hufblock.h, through tests/hufblock/hufblock_check.c) and a frame of one block, decode through libzstd to the row's bytes.  Rows
at odd offsets, rows that are not coded among them; the dense area is packed in row order at multiples of 16, zeros between; nothing is
written outside the outputs; the launcher's refusals."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = "-I" + os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hufmock")
    mock, chk = str(d / "libmockhufcode.so"), str(d / "libhufblock.so")
    flags = ["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", INC]
    subprocess.check_call(flags + ["-std=c11", "-o", mock, os.path.join(ROOT, "tests", "mock", "mock_hip_huf_code.c")])
    subprocess.check_call(flags + ["-std=c99", "-o", chk, os.path.join(ROOT, "tests", "hufblock", "hufblock_check.c")])
    H = C.CDLL(chk)
    H.hb_body.restype = C.c_size_t
    H.hb_body.argtypes = [C.c_void_p, C.c_uint, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    H.hb_lengths.restype = C.c_uint
    H.hb_lengths.argtypes = [C.c_char_p, C.c_uint, C.c_void_p]
    return D.bind_huf_kernel(C.CDLL(mock)), H


def rows_of(rng):
    """[(name, bytes)]"""
    expo = lambda n: (rng.normal(0.0, 0.02, n).astype(np.float32).view(np.uint32) >> 24).astype(np.uint8)  # noqa: E731
    return [("exponent 131072", expo(131072)), ("empty", np.zeros(0, dtype=np.uint8)), ("exponent 1024", expo(1024)),
            ("below 1 KiB", expo(1023)), ("one symbol", np.full(5000, 9, dtype=np.uint8)), ("noise", rng.integers(0, 256, 65536, dtype=np.uint8)),
            ("exponent 16383", expo(16383)), ("exponent 16384", expo(16384)), ("two symbols", rng.choice(np.array([0, 255], dtype=np.uint8), 1027)),
            ("high symbols", (200 + np.minimum(rng.geometric(0.2, 4097) - 1, 55)).astype(np.uint8))]


def launch(M, data, spans, dense_extra=0):
    n = len(spans)
    rows = (D.PlaneRow * n)(*[D.PlaneRow(o, ln, 0) for o, ln in spans])
    need = M.qzstd_hip_huf_code_bytes(rows, n)
    assert need == sum(D.huf_row_bytes(ln) for _, ln in spans)
    cost, size, off = (np.full(k + 2, 0xEEEEEEEE, dtype=np.uint32) for k in (n, n, n + 1))
    dense = np.full(need + 48, 0xA5, dtype=np.uint8)
    at = (-dense.ctypes.data) % 16 + 16
    scratch = np.full(D.huf_scratch_bytes(n, need) + 32, 0x5A, dtype=np.uint8)
    sat = (-scratch.ctypes.data) % 16
    d_rows = (D.PlaneRow * n)()
    rc = M.qzstd_hip_huf_code(0, None, data.ctypes.data, rows, n, d_rows, cost.ctypes.data + 4, size.ctypes.data + 4, off.ctypes.data + 4,
                              dense.ctypes.data + at, need, scratch.ctypes.data + sat, D.huf_scratch_bytes(n, need))
    assert rc == 0
    for a in (cost, size, off):
        assert a[0] == 0xEEEEEEEE and a[-1] == 0xEEEEEEEE
    used = int(off[n + 1])
    assert (dense[:at] == 0xA5).all() and (dense[at + used:] == 0xA5).all() and (scratch == 0x5A).all()
    return cost[1:-1], size[1:-1], off[1:-1], dense[at:at + used]


def test_dense_rows_make_frames_that_libzstd_decodes(libs):
    M, H = libs
    z = B.Zstd()
    rng = np.random.default_rng(11)
    named = rows_of(rng)
    pieces, spans, pos = [], [], 0
    for i, (_, r) in enumerate(named):  # row i starts at 3 * i + 1 mod 16, other bytes between the rows
        gap = (3 * i + 1 - pos) % 16 + 16
        pieces += [np.full(gap, 77, dtype=np.uint8), r]
        spans.append((pos + gap, len(r)))
        pos += gap + len(r)
    data = np.concatenate(pieces + [np.full(16, 77, dtype=np.uint8)])
    cost, size, off, dense = launch(M, data, spans)
    coded = 0
    for i, (name, r) in enumerate(named):
        n = len(r)
        if name in ("empty", "below 1 KiB", "one symbol", "noise"):
            assert size[i] == 0 and off[i + 1] == off[i], name
            assert (cost[i] == 0) == (name in ("empty", "one symbol")), name
            continue
        assert 0 < size[i] < n - ((n >> 6) + 2) and off[i] % 16 == 0, name
        assert off[i + 1] - off[i] == (128 + int(size[i]) + 15) // 16 * 16, name
        seg = dense[off[i]:off[i + 1]]
        assert not seg[128 + size[i]:].any(), name  # zeros up to the next multiple of 16
        nbits = np.empty(256, dtype=np.uint8)
        nbits[0::2], nbits[1::2] = seg[:128] & 15, seg[:128] >> 4
        want = (C.c_ubyte * 256)()
        assert H.hb_lengths(r.tobytes(), n, want) == nbits.max() and bytes(want) == nbits.tobytes(), name
        body = C.create_string_buffer(n + 200)
        b = H.hb_body(nbits.ctypes.data, n, seg[128:128 + size[i]].tobytes(), int(size[i]), body, n + 200, 0)
        assert 0 < b <= n - ((n >> 6) + 2) + 140, name
        frame = b"\x28\xb5\x2f\xfd\xa0" + struct.pack("<I", n) + struct.pack("<I", 1 | (2 << 1) | (b << 3))[:3] + body.raw[:b]
        assert z.decompress(frame, n) == r.tobytes(), name
        coded += 1
    assert coded == 6 and len(dense) == off[len(named)]


def test_refusals_touch_nothing(libs):
    M, _ = libs
    data = np.arange(8192, dtype=np.uint32).astype(np.uint8)
    out = np.full(4096, 0x33, dtype=np.uint8)
    base = out.ctypes.data + (-out.ctypes.data) % 16

    def call(spans, src=data.ctypes.data, reserved=0, null=None, dense_at=1024, dense_bytes=2500, scratch_bytes=None):
        n = len(spans)
        rows = (D.PlaneRow * n)(*[D.PlaneRow(o, ln, reserved) for o, ln in spans])
        d_rows = (D.PlaneRow * max(n, 1))()
        a = {"rows": rows, "d_rows": d_rows, "cost": base, "size": base + 64, "off": base + 128, "dense": base + dense_at, "scratch": base + 256}
        if null:
            a[null] = None
        return M.qzstd_hip_huf_code(0, None, src, a["rows"], n, a["d_rows"], a["cost"], a["size"], a["off"], a["dense"], dense_bytes,
                                    a["scratch"], D.huf_scratch_bytes(n, 0) + 2500 if scratch_bytes is None else scratch_bytes)
    good = [(5, 1100), (0, 0), (2000, 1040)]
    need = sum(D.huf_row_bytes(ln) for _, ln in good)
    assert need == 1104 + 128 + 1040 + 128
    for name in ("rows", "d_rows", "cost", "size", "off", "dense", "scratch"):
        assert call(good, null=name) < 0, name
    assert call(good, src=None) < 0 and call([(0, 131073)]) < 0 and call(good, reserved=1) < 0
    assert call(good, dense_at=1032) < 0 and call(good, dense_bytes=need - 1) < 0 and call(good, scratch_bytes=D.huf_scratch_bytes(3, need) - 1) < 0
    assert (out == 0x33).all()
    assert call([]) == 0 and call([(0, 0)], src=None) == 0 and call(good, dense_bytes=need) == 0
