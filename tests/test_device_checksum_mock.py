"""CPU: content checksums (QZSTD_frontSetChecksum, include/qzstd_frontend_device.h) over the mock device layer — the front-end and
qatseqprod.c linked against tests/mock/mock_hip.c, mock_hip_device.c, mock_hip_gather.c and mock_hip_xxh64.c (qzstd_hip_xxh64 in plain C
from the XXH64 specification), as shared objects of their own names.  With the setting on, every frame of the device calls carries the
Content_Checksum_Flag, decodes, and is byte for byte the frame QZSTD_frontCompress builds from the same bytes with the setting on —
whichever of the three frame-building paths served it; with the setting off again nothing of it is left."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import pytest
import xxhash

import qz_bind as B
import qz_corpus as K
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
MOCK_SO = os.path.join(MOCK, "libqatseqprod_cksummock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_cksummock.so")
NOHASH_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nohashmock.so")
NOHASH_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nohashmock.so")


def build_shared(cmd, out):
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call([tmp if x == out else x for x in cmd])
    os.replace(tmp, out)


def build_pair(zstd_path, mock_so, front_so, xxh64: bool):
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(MOCK, "mock_hip.c"), os.path.join(MOCK, "mock_hip_device.c"), os.path.join(MOCK, "mock_hip_gather.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    if xxh64:
        srcs.append(os.path.join(MOCK, "mock_hip_xxh64.c"))
    build_shared(["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-o", mock_so] + srcs, mock_so)
    build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                  mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def load_pair(mock_so, front_so):
    plug = B.Plugin(mock_so)
    F = C.CDLL(front_so)
    plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    return plug, F


@pytest.fixture(scope="module")
def cksummock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, xxh64=True)
    plug, F = load_pair(MOCK_SO, FRONT_SO)
    plug.lib.qzstd_mock_xxh64.restype = C.c_uint64
    plug.lib.qzstd_mock_xxh64.argtypes = [C.c_void_p, C.c_uint64]
    plug.lib.qzstd_mock_xxh64_rows.restype = C.c_ulonglong
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    return plug, F


class Pool:
    """host memory the mock treats as device memory: every buffer at `offset` bytes past a 64-byte aligned start of its own, guard bytes
    between the buffers, the whole pool one registered range"""

    def __init__(self, plug, datas, offsets, slot=0, dev=0):
        place, pos = [], 0
        for d, o in zip(datas, offsets):
            place.append(pos + o)
            pos = (pos + o + len(d) + 64 + 63) & ~63
        self.raw = C.create_string_buffer(pos + 128)
        base = (C.addressof(self.raw) + 63) & ~63
        C.memset(base, 0xA5, pos + 64)
        self.bufs = []
        for d, p in zip(datas, place):
            C.memmove(base + p, d, len(d))
            self.bufs.append((base + p, len(d)))
        plug.lib.qzstd_mock_device_range(slot, base, pos + 64, dev)


def flagged(frame: bytes) -> bool:
    """Content_Checksum_Flag: bit 2 of the frame header descriptor, the byte behind the magic number"""
    return frame[:4] == b"\x28\xb5\x2f\xfd" and bool(frame[4] & 4)


def host_frames(F, threads, level, chunk, datas, checksum=True):
    """QZSTD_frontCompress over each buffer's bytes on a front of its own"""
    fr = D.DeviceFront(threads, level, chunk, lib=F)
    try:
        assert fr.set_checksum(checksum) == 0
        return [fr.compress_host(d) if d else [] for d in datas]
    finally:
        fr.close()


def check_frames(zstd, got, want, datas, chunk, flag=True):
    assert len(got) == len(want) == len(datas)
    for i, (g, w, d) in enumerate(zip(got, want, datas)):
        assert len(g) == len(w) == (len(d) + chunk - 1) // chunk, i
        for c, f in enumerate(g):
            assert flagged(f) == flag, (i, c)
            assert zstd.decompress(f, chunk) == d[c * chunk:(c + 1) * chunk], (i, c)
            assert f == w[c], "buffer %d frame %d differs from QZSTD_frontCompress's" % (i, c)


CASES = {
    "chunk128k": (131072, [3 * 131072]),
    "chunk4k": (4096, [9 * 4096]),
    "partial_last_frame": (131072, [2 * 131072 + 4321]),
    "partial_last_frame_4k": (4096, [5 * 4096 + 1]),
    "multi_block_frames": (262144, [2 * 262144 + 140000]),
    "batch_unequal_unaligned": (32768, [0, 1, 15, 16, 32767, 32768, 32769, 3 * 32768 + 777, 0, 40000]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_checksummed_frames_equal_the_host_path(cksummock, zstd, name):
    """both device calls with the setting on: every frame flagged, decoding (the decoder verifies the hash), and byte for byte the host
    path's frame with ZSTD_c_checksumFlag = 1"""
    plug, F = cksummock
    chunk, sizes = CASES[name]
    datas = [K.by_name(("text", "mix", "system")[i % 3], n, seed=3 + i) if n else b"" for i, n in enumerate(sizes)]
    want = host_frames(F, 2, 1, chunk, datas)
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        assert fr.get_checksum() == 0 and fr.set_checksum(1) == 0 and fr.get_checksum() == 1
        for offsets in ([0] * len(datas), [(1, 3, 15, 0)[i % 4] for i in range(len(datas))]):
            pool = Pool(plug, datas, offsets)
            h0 = plug.lib.qzstd_mock_xxh64_launches()
            check_frames(zstd, fr.compress_device_batch(pool.bufs), want, datas, chunk)
            assert plug.lib.qzstd_mock_xxh64_launches() == h0 + 1  # one part: one hash launch
            single = [fr.compress_device(p, n) if n else [] for p, n in pool.bufs]
            check_frames(zstd, single, want, datas, chunk)
    finally:
        fr.close()


def test_decoder_rejects_a_frame_with_a_wrong_checksum(cksummock, zstd):
    plug, F = cksummock
    data = K.by_name("text", 50000, seed=2)
    pool = Pool(plug, [data], [3])
    fr = D.DeviceFront(2, 1, 131072, lib=F)
    try:
        fr.set_checksum(1)
        (frame,) = fr.compress_device(*pool.bufs[0])
        assert zstd.decompress(frame, len(data)) == data
        with pytest.raises(RuntimeError):
            zstd.decompress(frame[:-1] + bytes([frame[-1] ^ 1]), len(data))
    finally:
        fr.close()


def test_sequences_and_literals_path_and_raw_block_path(cksummock, zstd):
    """compressible text: the GPU's hash, patched into the frame ZSTD_compressSequencesAndLiterals built; random bytes: the raw-bytes
    path, hashed by libzstd — checksum_stats says which"""
    plug, F = cksummock
    chunk = 65536
    for datas, gpu in (([K.by_name("text", 5 * chunk + 100, seed=1)], True), ([os.urandom(3 * chunk + 50)], False)):
        want = host_frames(F, 2, 1, chunk, datas)
        n = len(want[0])
        pool = Pool(plug, datas, [1])
        fr = D.DeviceFront(2, 1, chunk, lib=F)
        try:
            fr.set_checksum(1)
            check_frames(zstd, [fr.compress_device(*pool.bufs[0])], want, datas, chunk)
            assert fr.checksum_stats() == ([n, 0] if gpu else [0, n])
            assert fr.stats()[:2] == ([n, 0] if gpu else [0, n])
            check_frames(zstd, fr.compress_device_batch(pool.bufs), want, datas, chunk)
            assert fr.checksum_stats() == ([2 * n, 0] if gpu else [0, 2 * n])
            fr.compress_host(datas[0])
            assert fr.checksum_stats() == ([2 * n, n] if gpu else [0, 3 * n])  # the host path's frames: libzstd's
        finally:
            fr.close()


CHILD = """
import ctypes as C, json, os, sys
sys.path[:0] = [%(tools)r, %(tests)r]
import qz_bind as B, qz_corpus as K, qz_device as D
import test_device_checksum_mock as T
z = B.Zstd()
plug, F = T.load_pair(%(mock)r, %(front)r)
"""


def run_child(body, mock_so, front_so, env=None):
    script = CHILD % dict(tools=os.path.join(ROOT, "tools"), tests=os.path.join(ROOT, "tests"), mock=mock_so, front=front_so) + body
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_compress_sequences_path(cksummock, zstd):
    """QZSTD_FRONT_NO_SEQLIT=1 (a libzstd without ZSTD_compressSequencesAndLiterals; read once per process, hence a child): every frame
    from ZSTD_compressSequences over its raw bytes, hashed by libzstd, and still the host path's frame"""
    res = run_child("""
chunk = 65536
datas = [K.by_name("text", 4 * chunk + 9, seed=6), K.by_name("mix", 3000, seed=7)]
want = T.host_frames(F, 2, 1, chunk, datas)
pool = T.Pool(plug, datas, [3, 0])
fr = D.DeviceFront(2, 1, chunk, lib=F)
fr.set_checksum(1)
T.check_frames(z, fr.compress_device_batch(pool.bufs), want, datas, chunk)
T.check_frames(z, [fr.compress_device(*pool.bufs[0])], want[:1], datas[:1], chunk)
fr.set_checksum(0)
off = fr.compress_device_batch(pool.bufs)
T.check_frames(z, off, T.host_frames(F, 2, 1, chunk, datas, checksum=False), datas, chunk, flag=False)
print(json.dumps({"cksum": fr.checksum_stats(), "dev": fr.stats()[:2]}))
""", MOCK_SO, FRONT_SO, env={"QZSTD_FRONT_NO_SEQLIT": "1"})
    assert res == {"cksum": [0, 11], "dev": [0, 17]}, res


def test_alternating_the_setting_leaves_nothing_behind(cksummock, zstd):
    """on, off, on on one front, compressible and random buffers together (all three ways of building a frame set the sticky
    ZSTD_c_checksumFlag themselves): the off call's frames are those of a front that never had it on, none flagged"""
    plug, F = cksummock
    chunk = 32768
    datas = [K.by_name("text", 3 * chunk + 5, seed=11), os.urandom(2 * chunk + 7), K.by_name("mix", 900, seed=12), os.urandom(100)]
    pool = Pool(plug, datas, [0, 3, 1, 15])
    never = D.DeviceFront(1, 1, chunk, lib=F)
    fr = D.DeviceFront(1, 1, chunk, lib=F)  # one worker: every frame meets the context the one before it left
    try:
        plain = never.compress_device_batch(pool.bufs)
        plain_host = [never.compress_host(d) for d in datas]
        assert never.checksum_stats() == [0, 0]
        want_on = host_frames(F, 1, 1, chunk, datas)
        for on in (1, 0, 1):
            assert fr.set_checksum(on) == 0
            got = fr.compress_device_batch(pool.bufs)
            if on:
                check_frames(zstd, got, want_on, datas, chunk)
                assert [fr.compress_host(d) for d in datas] == want_on
            else:
                assert got == plain and not any(flagged(f) for b in got for f in b)
                assert [fr.compress_device(p, n) for p, n in pool.bufs] == plain
                assert [fr.compress_host(d) for d in datas] == plain_host
    finally:
        never.close()
        fr.close()


def test_off_by_default_queues_no_hash_and_copies_no_more(cksummock, zstd):
    """the setting off: the hash entry point is not called; on: 8 bytes more device->host per frame, one launch per part"""
    plug, F = cksummock
    chunk = 32768
    datas = [K.by_name("text", 5 * chunk + 5, seed=21), K.by_name("mix", 2 * chunk, seed=22)]
    pool = Pool(plug, datas, [0, 3])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        h0, r0, s0 = plug.lib.qzstd_mock_xxh64_launches(), plug.lib.qzstd_mock_xxh64_rows(), fr.stats()
        fr.compress_device_batch(pool.bufs)
        s1 = fr.stats()
        assert plug.lib.qzstd_mock_xxh64_launches() == h0 and fr.checksum_stats() == [0, 0]
        fr.set_checksum(1)
        fr.compress_device_batch(pool.bufs)
        s2 = fr.stats()
        assert plug.lib.qzstd_mock_xxh64_launches() == h0 + 1 and plug.lib.qzstd_mock_xxh64_rows() == r0 + 8
        assert (s2[2] - s1[2]) - (s1[2] - s0[2]) == 8 * 8, (s0, s1, s2)
    finally:
        fr.close()


def test_parts_hash_their_own_frames(cksummock, zstd, monkeypatch):
    """small parts: a launch per part on alternating slots, every frame with its own hash"""
    plug, F = cksummock
    chunk = 32768
    datas = [K.by_name(("mix", "text")[i % 2], n, seed=40 + i) for i, n in enumerate([2000, 17, 3000, 5 * chunk, 900, chunk + 5, 64, 2 * chunk, 7])]
    want = host_frames(F, 2, 1, chunk, datas)
    pool = Pool(plug, datas, [(0, 1, 3, 15)[i % 4] for i in range(len(datas))])
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(2 * chunk))
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        fr.set_checksum(1)
        h0 = plug.lib.qzstd_mock_xxh64_launches()
        check_frames(zstd, fr.compress_device_batch(pool.bufs), want, datas, chunk)
        assert plug.lib.qzstd_mock_xxh64_launches() - h0 == 6
    finally:
        fr.close()


def test_setting_is_refused_while_a_call_runs(cksummock, zstd):
    """QZSTD_frontSetChecksum from a second thread while a device call waits for its first part (the mock's streams held busy): -1, the
    call's frames are what it started with; afterwards the setter works again"""
    plug, F = cksummock
    chunk = 32768
    datas = [K.by_name("text", 3 * chunk + 5, seed=31)]
    want = host_frames(F, 2, 1, chunk, datas)
    pool = Pool(plug, datas, [3])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    got = {}
    try:
        assert fr.set_checksum(1) == 0
        plug.lib.qzstd_mock_stall_ms(50000)  # every stream looks busy until released below
        th = threading.Thread(target=lambda: got.update(frames=fr.compress_device_batch(pool.bufs)))
        th.start()
        deadline = time.monotonic() + 50
        seen = []
        while time.monotonic() < deadline:  # (setting it to what it is: the call sees the same value whenever it starts)
            r = fr.set_checksum(1)
            if r != 0:
                seen = [r, fr.set_checksum(0), fr.get_checksum()]
                break
        plug.lib.qzstd_mock_stall_ms(0)
        th.join(60)
        assert seen == [-1, -1, 1], seen
        check_frames(zstd, got["frames"], want, datas, chunk)
        assert fr.set_checksum(0) == 0 and fr.get_checksum() == 0
        assert fr.lib.QZSTD_frontSetChecksum(None, 1) == -1 and fr.lib.QZSTD_frontGetChecksum(None) == 0
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


def test_device_layer_without_the_hash_kernel(zstd, oracle):
    """the front-end linked against the mock WITHOUT mock_hip_xxh64.c: with the setting on the device calls return (size_t)-1 before
    anything is queued, with it off they work; the host call works either way (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOHASH_MOCK_SO, NOHASH_FRONT_SO, xxh64=False)
    res = run_child("""
chunk = 65536
data = K.by_name("system", 3 * chunk + 321)
pool = T.Pool(plug, [data], [0])
fr = D.DeviceFront(2, 1, chunk, lib=F)
plain = fr.compress_device(*pool.bufs[0])
host_plain = fr.compress_host(data)
assert fr.set_checksum(1) == 0
before, st = plug.lib.qzstd_mock_launches(), fr.stats()
r1 = fr.compress_device_raw(*pool.bufs[0])[0]
r2 = fr.compress_device_batch_raw(pool.bufs)[0]
refused = r1 == D.ERROR and r2 == D.ERROR and plug.lib.qzstd_mock_launches() == before and fr.stats() == st
host_on = fr.compress_host(data)
host_ok = all(T.flagged(f) and z.decompress(f, chunk) == data[c * chunk:(c + 1) * chunk] for c, f in enumerate(host_on))
fr.set_checksum(0)
print(json.dumps({"refused": refused, "host_on": host_ok, "off_same": fr.compress_device(*pool.bufs[0]) == plain == host_plain,
                  "has_xxh64": hasattr(plug.lib, "qzstd_hip_xxh64")}))
""", NOHASH_MOCK_SO, NOHASH_FRONT_SO)
    assert res == {"refused": True, "host_on": True, "off_same": True, "has_xxh64": False}, res


HASH_LENGTHS = list(range(0, 101)) + [1023, 1024, 1025, 131071, 131072, 131073]


def test_mock_xxh64_against_xxhash(cksummock):
    """the mock's XXH64 against python-xxhash, directly and through qzstd_hip_xxh64 (rows at 16-aligned offsets, bytes behind a row's
    end are its neighbour's); the launcher's refusals"""
    import numpy as np
    plug, _ = cksummock
    L = plug.lib
    assert xxhash.xxh64(b"").intdigest() == 0xEF46DB3751D8E999 == L.qzstd_mock_xxh64(None, 0)
    src = np.random.default_rng(7).integers(0, 256, 131073 + 64, dtype=np.uint8)
    for n in HASH_LENGTHS:
        assert L.qzstd_mock_xxh64(src.ctypes.data + 5, n) == xxhash.xxh64(src[5:5 + n].tobytes()).intdigest(), n
    L.qzstd_hip_xxh64.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    raw = np.random.default_rng(8).integers(0, 256, 600000, dtype=np.uint8)
    o = (-raw.ctypes.data) % 16
    base, view = raw.ctypes.data + o, raw[o:]
    rows, drows = (D.HashRow * len(HASH_LENGTHS))(), (D.HashRow * len(HASH_LENGTHS))()
    pos = 0
    for r, n in zip(rows, HASH_LENGTHS):
        r.srcOff, r.len = pos, n
        pos += (n + 15) & ~15
    assert pos <= len(view)
    out = np.full(len(HASH_LENGTHS) + 2, 0x1234, dtype=np.uint64)
    assert L.qzstd_hip_xxh64(0, None, base, rows, len(rows), drows, out.ctypes.data + 8) == 0
    assert out[0] == 0x1234 and out[-1] == 0x1234
    for k, r in enumerate(rows):
        assert int(out[1 + k]) == xxhash.xxh64(view[r.srcOff:r.srcOff + r.len].tobytes()).intdigest(), r.len
    n = len(rows)
    bad = (D.HashRow * n)()
    C.memmove(bad, rows, C.sizeof(rows))
    bad[40].srcOff += 8
    out[:] = 0x1234
    assert L.qzstd_hip_xxh64(0, None, base, bad, n, drows, out.ctypes.data + 8) < 0
    assert L.qzstd_hip_xxh64(0, None, base + 8, rows, n, drows, out.ctypes.data + 8) < 0
    assert L.qzstd_hip_xxh64(0, None, None, rows, n, drows, out.ctypes.data + 8) < 0  # rows that are not empty, no base
    assert L.qzstd_hip_xxh64(0, None, base, None, n, drows, out.ctypes.data + 8) < 0
    assert L.qzstd_hip_xxh64(0, None, base, rows, n, None, out.ctypes.data + 8) < 0
    assert L.qzstd_hip_xxh64(0, None, base, rows, n, drows, None) < 0
    assert L.qzstd_hip_xxh64(0, None, base, None, 0, None, None) == 0
    assert (out == 0x1234).all()
    assert L.qzstd_hip_xxh64(0, None, None, rows, 1, drows, out.ctypes.data + 8) == 0  # one empty row needs no base
    assert int(out[1]) == 0xEF46DB3751D8E999
