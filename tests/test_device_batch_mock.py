"""CPU: QZSTD_frontCompressDeviceBatch (include/qzstd_frontend_device.h) over the mock device layer — the front-end and qatseqprod.c linked
against tests/mock/mock_hip.c, mock_hip_device.c and mock_hip_gather.c (qzstd_hip_gather with memcpy / memset), as shared objects of their
own names.  A batch of buffers of unequal sizes and alignments must give, per buffer, byte for byte the frames libzstd builds from the
ORACLE's sequences for that buffer alone (tools/qz_device.reference_frames) — the frames of one QZSTD_frontCompressDevice call per buffer —
whatever its neighbours and however the parts fall."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import qz_bind as B
import qz_corpus as K
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock")
MOCK_SO = os.path.join(MOCK, "libqatseqprod_batchmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_batchmock.so")
NOGATHER_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nogathermock.so")
NOGATHER_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nogathermock.so")


def build_shared(cmd, out):
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call([tmp if x == out else x for x in cmd])
    os.replace(tmp, out)


def build_pair(zstd, mock_so, front_so, gather: bool):
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(MOCK, "mock_hip.c"), os.path.join(MOCK, "mock_hip_device.c"), os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    if gather:
        srcs.append(os.path.join(MOCK, "mock_hip_gather.c"))
    build_shared(["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-o", mock_so] + srcs, mock_so)
    build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                  mock_so, zstd.path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd.path)], front_so)


@pytest.fixture(scope="module")
def batchmock(oracle, zstd):
    build_pair(zstd, MOCK_SO, FRONT_SO, gather=True)
    plug = B.Plugin(MOCK_SO)
    F = C.CDLL(FRONT_SO)
    plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    plug.lib.qzstd_mock_gather_rows.restype = C.c_ulonglong
    return plug, F


class Pool:
    """host memory the mock treats as device memory: every buffer at `offset` bytes past a 64-byte aligned start of its own, guard bytes
    between the buffers, the whole pool one registered range (slot, device)"""

    def __init__(self, plug, datas, offsets, slot=0, dev=0):
        self.plug, self.slot = plug, slot
        place, pos = [], 0
        for d, o in zip(datas, offsets):
            place.append(pos + o)
            pos = (pos + o + len(d) + 64 + 63) & ~63
        self.raw = C.create_string_buffer(pos + 128)
        base = (C.addressof(self.raw) + 63) & ~63
        self.bufs = []
        for d, p in zip(datas, place):
            C.memmove(base + p, d, len(d))
            self.bufs.append((base + p, len(d)))
        plug.lib.qzstd_mock_device_range(slot, base, pos + 64, dev)

    def release(self):
        self.plug.lib.qzstd_mock_device_range(self.slot, None, 0, 0)


def reference(zstd, oracle, datas, chunk, level, ext_rep=False):
    return [D.reference_frames(zstd, oracle, d, chunk, level, ext_rep) if d else [] for d in datas]


def prefix(datas, chunk):
    out = [0]
    for d in datas:
        out.append(out[-1] + (len(d) + chunk - 1) // chunk)
    return out


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = [c for c in range(len(w)) if c >= len(g) or g[c] != w[c]]
        assert len(g) == len(w) and not bad, "buffer %d: frames %s differ (%d frames, want %d)" % (i, bad[:6], len(g), len(w))


OFFSETS = (0, 1, 3, 15)


def mixed_sizes(chunk):
    return [0, 1, 15, 16, chunk - 1, chunk, chunk + 1, 3 * chunk + 777, 0, 40000]


@pytest.mark.parametrize("level", [1, 3, 6, 12])
@pytest.mark.parametrize("chunk", [32768, 131072, 393216])
def test_batch_mixed_sizes_and_alignments(batchmock, zstd, oracle, level, chunk):
    """the issue's size list, every buffer at each of the offsets 0, 1, 3, 15 in turn: per buffer the reference's frames, firstFrame the
    prefix sums, every frame decodes to its slice, every frame counted once"""
    plug, F = batchmock
    gens = ("text", "mix", "system")
    datas = [K.by_name(gens[i % 3], n, seed=level + i) for i, n in enumerate(mixed_sizes(chunk))]
    want = reference(zstd, oracle, datas, chunk, level)
    fr = D.DeviceFront(3, level, chunk, lib=F)
    try:
        for rot in range(4):
            pool = Pool(plug, datas, [OFFSETS[(i + rot) % 4] for i in range(len(datas))])
            s0 = fr.stats()
            r, got, first = fr.compress_device_batch_raw(pool.bufs)
            s1 = fr.stats()
            assert r == prefix(datas, chunk)[-1] and first == prefix(datas, chunk)
            same(got, want)
            assert (s1[0] + s1[1]) - (s0[0] + s0[1]) == r and s1[3] - s0[3] == sum(len(d) for d in datas), (s0, s1)
            for d, frames in zip(datas, got):
                for c, f in enumerate(frames):
                    assert zstd.decompress(f, chunk) == d[c * chunk:(c + 1) * chunk]
    finally:
        fr.close()


def part_case(chunk):
    sizes = [2000, 17, 3000, 5 * chunk, 900, chunk + 5, 64, 2 * chunk, 7]
    return [K.by_name(("mix", "text")[i % 2], n, seed=40 + i) for i, n in enumerate(sizes)]


def test_batch_part_boundaries(batchmock, zstd, oracle, monkeypatch):
    """the part size changes how the frames are grouped into launches and nothing else: 1000 bytes (a frame per part, small buffers share
    one), 3 chunks + 1, and 2 chunks — the 5-chunk buffer spans three parts while the small ones around it share theirs"""
    plug, F = batchmock
    chunk = 32768
    datas = part_case(chunk)
    pool = Pool(plug, datas, [OFFSETS[i % 4] for i in range(len(datas))])
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        g0 = plug.lib.qzstd_mock_gather_launches()
        base = fr.compress_device_batch(pool.bufs)
        assert plug.lib.qzstd_mock_gather_launches() == g0 + 1  # the default part holds the whole batch: ONE gather, one compaction
        same(base, reference(zstd, oracle, datas, chunk, 1))
        for part, launches in ((1000, None), (3 * chunk + 1, None), (2 * chunk, 6)):
            monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(part))
            c0 = plug.lib.qzstd_mock_compact_launches()
            assert fr.compress_device_batch(pool.bufs) == base, part
            if launches is not None:
                # [2000 17 3000 chunk | 2 chunks | 2 chunks | 900 chunk 5 64 | 2 chunks | 7]: the 5-chunk buffer in three parts, the first shared
                assert plug.lib.qzstd_mock_compact_launches() - c0 == launches
    finally:
        fr.close()


def test_batch_equals_single_calls(batchmock, zstd, oracle):
    """the batch's frames are those of one QZSTD_frontCompressDevice call per buffer on the same front, and it copies no more bytes
    device->host than they do together"""
    plug, F = batchmock
    chunk = 65536
    datas = [K.by_name(("system", "mix", "text")[i % 3], n, seed=70 + i)
             for i, n in enumerate([5, 70000, 65536, 3 * 65536 + 11, 1, 4096, 200000, 33])]
    pool = Pool(plug, datas, [OFFSETS[i % 4] for i in range(len(datas))])
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        s0 = fr.stats()
        single = [fr.compress_device(p, n) for p, n in pool.bufs]
        s1 = fr.stats()
        batch = fr.compress_device_batch(pool.bufs)
        s2 = fr.stats()
        same(batch, single)
        assert s2[2] - s1[2] <= s1[2] - s0[2], (s0, s1, s2)
        assert s2[0] - s1[0] == s1[0] - s0[0] and s2[1] - s1[1] == s1[1] - s0[1] and s2[3] - s1[3] == s1[3] - s0[3]
    finally:
        fr.close()


def test_batch_incompressible_between_compressible(batchmock, zstd, oracle):
    """random buffers between text: their frames take the raw-bytes path, which must copy from the right buffer at the right offset"""
    plug, F = batchmock
    chunk = 65536
    datas = [K.by_name("text", 70000, seed=1), os.urandom(2 * chunk + 100), K.by_name("text", 3000, seed=2), os.urandom(500),
             K.by_name("system", chunk, seed=3), os.urandom(chunk)]
    pool = Pool(plug, datas, [3, 1, 0, 15, 0, 0])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        same(fr.compress_device_batch(pool.bufs), reference(zstd, oracle, datas, chunk, 1))
        st = fr.stats()
        assert st[1] >= 5 and st[0] + st[1] == prefix(datas, chunk)[-1], st
    finally:
        fr.close()


def test_batch_external_repcodes(batchmock, zstd, oracle, monkeypatch):
    plug, F = batchmock
    monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    datas = [K.by_name("system", n, seed=5 + i) for i, n in enumerate([3 * 65536 + 99, 1000, 65536, 31])]
    pool = Pool(plug, datas, [0, 1, 3, 15])
    fr = D.DeviceFront(2, 1, 65536, ext_rep=1, lib=F)
    try:
        same(fr.compress_device_batch(pool.bufs), reference(zstd, oracle, datas, 65536, 1, ext_rep=True))
    finally:
        fr.close()


def test_batch_refusals_queue_nothing(batchmock, zstd, oracle):
    """every refusal returns (size_t)-1 before a launch, a gather or a counter moves; the front works afterwards"""
    plug, F = batchmock
    chunk = 32768
    datas = [K.by_name("text", n, seed=9 + i) for i, n in enumerate([4 * chunk, 100, chunk + 1])]
    pool = Pool(plug, datas, [0, 1, 3])
    other = Pool(plug, [datas[1]], [0], slot=1, dev=1)  # "device memory" of another device
    host = C.create_string_buffer(datas[1], len(datas[1]))
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    sw = D.DeviceFront(2, 1, chunk, use_producer=0, lib=F)
    try:
        launches, gathers = plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_gather_launches()
        n = prefix(datas, chunk)[-1]
        a, b, c = pool.bufs
        assert fr.compress_device_batch_raw(pool.bufs, dst_capacity=(n - 1) * fr.stride)[0] == D.ERROR  # dst too small
        assert sw.compress_device_batch_raw(pool.bufs)[0] == D.ERROR  # useProducer = 0
        sizes = (C.c_size_t * 8)()
        dst = C.create_string_buffer(8 * fr.stride)
        assert fr.lib.QZSTD_frontCompressDeviceBatch(fr.f, None, 3, None, dst, len(dst), sizes, None) == D.ERROR  # bufs NULL
        assert fr.lib.QZSTD_frontDeviceBatchFrames(fr.f, None, 3) == D.ERROR
        assert fr.compress_device_batch_raw([a, (0, 100), c])[0] == D.ERROR  # a null buffer of a size
        assert fr.compress_device_batch_raw([a, (C.addressof(host), len(host)), c])[0] == D.ERROR  # host memory in the middle
        assert fr.compress_device_batch_raw([a, b, (c[0], c[1] + (1 << 20))])[0] == D.ERROR  # last byte outside device memory
        assert fr.compress_device_batch_raw([a, other.bufs[0], c])[0] == D.ERROR  # two devices
        assert plug.lib.qzstd_mock_launches() == launches and plug.lib.qzstd_mock_gather_launches() == gathers
        assert fr.stats() == [0, 0, 0, 0]
        # no buffers, empty buffers (a null pointer of size 0 among them): 0 frames, nothing touched
        assert fr.compress_device_batch_raw([])[:2] == (0, [])
        r, got, first = fr.compress_device_batch_raw([(0, 0), (a[0], 0)])
        assert r == 0 and got == [[], []] and first == [0, 0, 0]
        assert plug.lib.qzstd_mock_launches() == launches and fr.stats() == [0, 0, 0, 0]
        same(fr.compress_device_batch(pool.bufs), reference(zstd, oracle, datas, chunk, 1))
        assert fr.compress_device(a[0], a[1]) == fr.compress_host(datas[0])
    finally:
        other.release()
        fr.close()
        sw.close()


def test_batch_second_concurrent_call_is_refused(batchmock, zstd, oracle):
    """a batch or a single call while a batch runs on the same front returns (size_t)-1 at once; the first one is not disturbed"""
    import threading
    import time
    plug, F = batchmock
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    chunk = 32768
    datas = [K.by_name("text", n, seed=21 + i) for i, n in enumerate([3 * chunk + 5, 77, 2 * chunk])]
    pool = Pool(plug, datas, [0, 3, 1])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    dst = C.create_string_buffer(8 * fr.stride)
    sizes = (C.c_size_t * 8)()
    got = {}
    try:
        bufs, nb, n = fr.batch(pool.bufs)
        plug.lib.qzstd_mock_stall_ms(1500)  # every stream looks busy: the first call waits for its first part
        th = threading.Thread(target=lambda: got.update(frames=fr.compress_device_batch(pool.bufs)))
        th.start()
        time.sleep(0.3)
        r1 = fr.lib.QZSTD_frontCompressDeviceBatch(fr.f, bufs, nb, None, dst, len(dst), sizes, None)
        r2 = fr.lib.QZSTD_frontCompressDevice(fr.f, C.c_void_p(pool.bufs[0][0]), pool.bufs[0][1], None, dst, len(dst), sizes)
        th.join(60)
        assert r1 == D.ERROR and r2 == D.ERROR
        same(got["frames"], reference(zstd, oracle, datas, chunk, 1))
        assert fr.stats()[3] == sum(len(d) for d in datas)
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


def test_batch_front_reused_across_shapes(batchmock, zstd, oracle, monkeypatch):
    """one front: a large batch, a tiny one, a single call, a batch of another shape — the slot buffers and the row table grow and are reused"""
    plug, F = batchmock
    chunk = 32768
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(8 * chunk))
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        shapes = ([20 * chunk + 5, 100, 3 * chunk, 9], [7], None, [1, 2, 3, 12 * chunk + 1, 4, 5] + [300] * 40, [chunk] * 9)
        for k, sizes in enumerate(shapes):
            if sizes is None:
                data = K.by_name("mix", 11 * chunk + 3, seed=k)
                pool = Pool(plug, [data], [5])
                assert fr.compress_device(*pool.bufs[0]) == D.reference_frames(zstd, oracle, data, chunk, 1)
                continue
            datas = [K.by_name(("mix", "text")[i % 2], n, seed=k * 100 + i) for i, n in enumerate(sizes)]
            pool = Pool(plug, datas, [OFFSETS[(i + k) % 4] for i in range(len(datas))])
            same(fr.compress_device_batch(pool.bufs), reference(zstd, oracle, datas, chunk, 1))
    finally:
        fr.close()


def test_batch_many_small_buffers_share_one_part(batchmock, zstd, oracle):
    """600 buffers of 1 .. 3000 bytes: one gather of 600 rows, one match-finder launch, one compaction"""
    plug, F = batchmock
    chunk = 131072
    datas = [K.by_name(("mix", "text", "system")[i % 3], 1 + (i * 37) % 3000, seed=i) for i in range(600)]
    pool = Pool(plug, datas, [i % 16 for i in range(600)])
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        g0, r0, c0 = plug.lib.qzstd_mock_gather_launches(), plug.lib.qzstd_mock_gather_rows(), plug.lib.qzstd_mock_compact_launches()
        same(fr.compress_device_batch(pool.bufs), reference(zstd, oracle, datas, chunk, 1))
        assert plug.lib.qzstd_mock_gather_launches() == g0 + 1 and plug.lib.qzstd_mock_gather_rows() == r0 + 600
        assert plug.lib.qzstd_mock_compact_launches() == c0 + 1
    finally:
        fr.close()


def test_single_call_stages_through_the_gather_when_present(batchmock, zstd, oracle):
    """QZSTD_frontCompressDevice is the batch of one buffer: a misaligned buffer goes through the gather, an aligned one is read in place"""
    plug, F = batchmock
    data = K.by_name("text", 5 * 32768 + 3, seed=8)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    try:
        for off, gathers in ((3, 1), (0, 1)):  # (offset 0: the ragged size keeps the part out of place)
            pool = Pool(plug, [data], [off])
            g0 = plug.lib.qzstd_mock_gather_launches()
            assert fr.compress_device(*pool.bufs[0]) == D.reference_frames(zstd, oracle, data, 32768, 1)
            assert plug.lib.qzstd_mock_gather_launches() - g0 == gathers
        pool = Pool(plug, [data[:4 * 32768]], [0])
        g0 = plug.lib.qzstd_mock_gather_launches()
        assert fr.compress_device(*pool.bufs[0]) == D.reference_frames(zstd, oracle, data[:4 * 32768], 32768, 1)
        assert fr.compress_device_batch([pool.bufs[0]]) == [D.reference_frames(zstd, oracle, data[:4 * 32768], 32768, 1)]
        assert plug.lib.qzstd_mock_gather_launches() == g0
    finally:
        fr.close()


def test_mock_gather_contract(batchmock):
    """the mock's qzstd_hip_gather: payload, zero padding, everything else untouched; the launcher's refusals write nothing"""
    import numpy as np
    plug, _ = batchmock
    L = plug.lib
    L.qzstd_hip_gather.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    src = np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8)
    raw = np.full(4096 + 64, 0xA5, dtype=np.uint8)
    o = (-raw.ctypes.data) % 16
    stage = raw[o:o + 4096]
    spec = [(3, 0, 1, 15), (100, 16, 0, 16), (7, 64, 33, 15), (1000, 112, 16, 0), (2000, 2048, 1500, 4)]
    rows = (D.GatherRow * len(spec))()
    drows = (D.GatherRow * len(spec))()
    for r, (s, d, n, p) in zip(rows, spec):
        r.src, r.dstOff, r.len, r.pad = src.ctypes.data + s, d, n, p
    assert L.qzstd_hip_gather(0, None, rows, len(spec), drows, stage.ctypes.data, 4096) == 0
    want = np.full(4096, 0xA5, dtype=np.uint8)
    for s, d, n, p in spec:
        want[d:d + n] = src[s:s + n]
        want[d + n:d + n + p] = 0
    assert np.array_equal(stage, want) and (raw[:o] == 0xA5).all() and (raw[o + 4096:] == 0xA5).all()
    for k, change in enumerate([dict(dstOff=8), dict(pad=14), dict(dstOff=4096), dict(dstOff=16), dict(src=0)]):
        stage[:] = 0xA5
        bad = (D.GatherRow * len(spec))()
        C.memmove(bad, rows, C.sizeof(rows))
        for name, v in change.items():
            setattr(bad[2], name, v)
        assert L.qzstd_hip_gather(0, None, bad, len(spec), drows, stage.ctypes.data, 4096) < 0, change
        assert (stage == 0xA5).all(), change
    assert L.qzstd_hip_gather(0, None, rows, len(spec), drows, stage.ctypes.data + 8, 4096) < 0
    assert L.qzstd_hip_gather(0, None, rows, len(spec), drows, stage.ctypes.data, 2048 + 1500) < 0  # the last row ends past the stage
    assert L.qzstd_hip_gather(0, None, rows, 0, drows, stage.ctypes.data, 4096) == 0 and (stage == 0xA5).all()


def test_batch_is_refused_by_a_device_layer_without_the_gather(zstd, oracle):
    """the front-end linked against the mock WITHOUT mock_hip_gather.c (an older device layer): the batch call returns (size_t)-1, the
    single call works as before (a process of its own: one set of mock libraries per process)"""
    build_pair(zstd, NOGATHER_MOCK_SO, NOGATHER_FRONT_SO, gather=False)
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
addr = C.addressof(raw) + 3
C.memmove(addr, data, len(data))
plug.lib.qzstd_mock_device_range(0, addr, len(data), 0)
fr = D.DeviceFront(2, 1, 65536, lib=F)
before = plug.lib.qzstd_mock_launches()
r = fr.compress_device_batch_raw([(addr, len(data)), (addr, 100)])[0]
refused = r == D.ERROR and plug.lib.qzstd_mock_launches() == before and fr.stats() == [0, 0, 0, 0]
same = fr.compress_device(addr, len(data)) == D.reference_frames(z, o, data, 65536, 1)
print(json.dumps({"refused": refused, "single_same": same, "has_gather": hasattr(plug.lib, "qzstd_hip_gather")}))
""" % (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), NOGATHER_MOCK_SO, NOGATHER_FRONT_SO)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"refused": True, "single_same": True, "has_gather": False}, res
