"""CPU: QZSTD_frontCompressDevice (include/qzstd_frontend_device.h) over the mock device layer — qat-zstd-plugin_amd/host/qatseqprod.c and the
front-end linked against tests/mock/mock_hip.c (malloc as device memory, the oracle as the match-finder) plus
tests/mock/mock_hip_device.c (the device-input entry points: a registered range stands for device memory, the compaction on the CPU).
Checks the framing, the per-part pipeline, the raw-bytes fallback, the statistics and the error returns without a GPU: frames must be
the ones libzstd builds with ZSTD_compress2 from the ORACLE's sequences."""
import ctypes as C
import os
import subprocess

import pytest

import qz_bind as B
import qz_corpus as K
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK_SO = os.path.join(ROOT, "tests", "mock", "libqatseqprod_devmock.so")
FRONT_SO = os.path.join(ROOT, "tests", "mock", "libqzstdfront_devmock.so")


def build_shared(cmd, out):
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call([tmp if x == out else x for x in cmd])
    os.replace(tmp, out)


@pytest.fixture(scope="module")
def devmock(oracle, zstd):
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "tests", "mock", "mock_hip.c"), os.path.join(ROOT, "tests", "mock", "mock_hip_device.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    build_shared(["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-o", MOCK_SO] + srcs, MOCK_SO)
    build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-o", FRONT_SO, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                  MOCK_SO, zstd.path, "-Wl,-rpath," + os.path.dirname(MOCK_SO), "-Wl,-rpath," + os.path.dirname(zstd.path)], FRONT_SO)
    plug = B.Plugin(MOCK_SO)
    F = C.CDLL(FRONT_SO)
    plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    return plug, F


class DevBuf:
    """host memory the mock treats as device memory of device 0; data placed at `offset` from a 64-byte aligned start"""

    def __init__(self, plug, data: bytes, offset: int = 0):
        self.raw = C.create_string_buffer(len(data) + offset + 128)
        base = (C.addressof(self.raw) + 63) & ~63
        self.addr = base + offset
        C.memmove(self.addr, data, len(data))
        plug.lib.qzstd_mock_device_range(0, self.addr, max(len(data), 1), 0)


def reference(zstd, oracle, data, chunk, level, ext_rep=False):
    return D.reference_frames(zstd, oracle, data, chunk, level, ext_rep)


@pytest.mark.parametrize("level,chunk,size,part", [(1, 32768, 20 * 32768 + 777, 4 * 32768), (1, 131072, 9 * 131072 + 5000, 2 * 131072),
                                                   (6, 131072, 5 * 131072 + 4000, 0), (3, 393216, 3 * 393216 + 70000, 393216),
                                                   (12, 32768, 7 * 32768, 3 * 32768)])
def test_device_frames_equal_the_oracles(devmock, zstd, oracle, level, chunk, size, part, monkeypatch):
    plug, F = devmock
    if part:  # several parts: the double-buffered pipeline, parts fetched while the workers code the one before
        monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(part))
    data = K.by_name("text", size, seed=level + 3)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, level, chunk, lib=F)
    try:
        got = fr.compress_device(buf.addr, len(data))
        assert got == reference(zstd, oracle, data, chunk, level)
        st = fr.stats()
        n = (len(data) + chunk - 1) // chunk
        assert st[0] == n and st[1] == 0 and st[3] == len(data), st
        assert st[2] > 0, st
        for c in (0, n - 1):
            assert zstd.decompress(got[c], chunk) == data[c * chunk:(c + 1) * chunk]
    finally:
        fr.close()


def test_device_frames_external_repcodes(devmock, zstd, oracle, monkeypatch):
    plug, F = devmock
    monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    data = K.by_name("system", 6 * 65536 + 99, seed=5)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 65536, ext_rep=1, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 65536, 1, ext_rep=True)
    finally:
        fr.close()


@pytest.mark.parametrize("offset,size", [(1, 5 * 32768 + 3), (3, 40000), (15, 32768 * 2), (0, 32768 + 7), (5, 11), (0, 15), (0, 1)])
def test_device_misaligned_and_short(devmock, zstd, oracle, offset, size):
    plug, F = devmock
    data = K.by_name("mix", size, seed=offset + size)
    buf = DevBuf(plug, data, offset)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 32768, 1)
    finally:
        fr.close()


def test_device_empty_input(devmock):
    plug, F = devmock
    buf = DevBuf(plug, b"x" * 64)
    fr = D.DeviceFront(1, 1, 32768, lib=F)
    try:
        r, frames = fr.compress_device_raw(buf.addr, 0)
        assert r == 0 and frames == []
    finally:
        fr.close()


def test_device_incompressible_takes_the_raw_bytes(devmock, zstd, oracle):
    plug, F = devmock
    data = os.urandom(3 * 65536) + K.by_name("text", 2 * 65536 + 11, seed=9)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 65536, lib=F)
    try:
        got = fr.compress_device(buf.addr, len(data))
        assert got == reference(zstd, oracle, data, 65536, 1)
        st = fr.stats()
        assert st[1] >= 3 and st[0] + st[1] == 6, st
        assert st[2] >= 3 * 65536, st  # the raw bytes came back
    finally:
        fr.close()


def test_device_error_returns_launch_nothing(devmock, zstd):
    plug, F = devmock
    data = K.by_name("text", 4 * 32768, seed=2)
    host = C.create_string_buffer(data, len(data))
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    sw = D.DeviceFront(2, 1, 32768, use_producer=0, lib=F)
    try:
        before = plug.lib.qzstd_mock_launches()
        assert fr.compress_device_raw(C.addressof(host), len(data))[0] == D.ERROR  # a host pointer
        assert fr.compress_device_raw(buf.addr, len(data), dst_capacity=3 * fr.stride)[0] == D.ERROR  # dst too small
        assert fr.compress_device_raw(buf.addr, len(data) + 4096)[0] == D.ERROR  # runs past the device range
        assert sw.compress_device_raw(buf.addr, len(data))[0] == D.ERROR  # useProducer = 0
        assert plug.lib.qzstd_mock_launches() == before
        assert fr.stats() == [0, 0, 0, 0]
        # and the front still works afterwards, both ways in
        assert fr.compress_device(buf.addr, len(data)) == fr.compress_host(data)
    finally:
        fr.close()
        sw.close()


def test_device_d2h_traffic_is_the_compacted_results(devmock, zstd, oracle):
    """level 1: what comes back is the headers, 8 bytes per entry and the literal bytes — no raw input"""
    plug, F = devmock
    chunk = 131072
    data = K.by_name("system", 12 * chunk, seed=17)
    buf = DevBuf(plug, data)
    prof = oracle.profile(1, chunk)
    lits = seqs = 0
    for o in range(0, len(data), chunk):
        n, s = oracle.find(prof, data[o:o + chunk])
        seqs += n
        lits += sum(s[i].litLength for i in range(n))
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        fr.compress_device(buf.addr, len(data))
        st = fr.stats()
        assert st[1] == 0 and st[2] <= lits + 8 * seqs + 16 * 12 and st[2] < len(data), (st, lits, seqs)
    finally:
        fr.close()


def test_device_second_concurrent_call_is_refused(devmock, zstd, oracle):
    """a call while another one runs on the same front returns (size_t)-1 at once; the first one is not disturbed"""
    import threading
    plug, F = devmock
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    data = K.by_name("text", 6 * 32768 + 5, seed=21)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    other = C.create_string_buffer(7 * fr.stride)
    sizes = (C.c_size_t * 8)()
    got = {}
    try:
        plug.lib.qzstd_mock_stall_ms(1500)  # every stream looks busy: the first call waits for its first part
        th = threading.Thread(target=lambda: got.update(frames=fr.compress_device(buf.addr, len(data))))
        th.start()
        import time
        time.sleep(0.3)
        r = fr.lib.QZSTD_frontCompressDevice(fr.f, C.c_void_p(buf.addr), len(data), None, other, len(other), sizes)
        th.join(60)
        assert r == D.ERROR
        assert got["frames"] == reference(zstd, oracle, data, 32768, 1)
        assert fr.stats()[3] == len(data)  # one call's input
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


def test_device_without_seqlit_every_frame_takes_the_raw_bytes(devmock, zstd, oracle):
    """a libzstd without ZSTD_compressSequencesAndLiterals (QZSTD_FRONT_NO_SEQLIT=1 makes the front-end ignore it; the look-up is made
    once per process, hence a process of its own): every frame is built from its raw bytes, and the frames are the same"""
    import json
    import sys
    script = """
import ctypes as C, json, sys
sys.path[:0] = [%r, %r]
import qz_bind as B, qz_corpus as K, qz_device as D
z, o = B.Zstd(), B.Oracle()
plug = B.Plugin(%r)
F = C.CDLL(%r)
plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
data = K.by_name("system", 5 * 65536 + 321)
raw = C.create_string_buffer(data, len(data) + 64)
plug.lib.qzstd_mock_device_range(0, C.addressof(raw), len(data), 0)
fr = D.DeviceFront(2, 1, 65536, lib=F)
same = fr.compress_device(C.addressof(raw), len(data)) == D.reference_frames(z, o, data, 65536, 1)
print(json.dumps({"same": same, "stats": fr.stats()}))
""" % (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), MOCK_SO, FRONT_SO)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, QZSTD_FRONT_NO_SEQLIT="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["same"] and res["stats"][0] == 0 and res["stats"][1] == 6, res
