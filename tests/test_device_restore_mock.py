"""CPU: the restore calls (QZSTD_frontRestoreDeviceBatchTyped, QZSTD_frontRestoreDevice, QZSTD_frontRestoreStats:
include/qzstd_frontend_device.h) over the mock device layer — the mock of tests/test_device_group_mock.py plus tests/mock/mock_hip_ungroup.c
(qzstd_hip_ungroup in plain C).  What the typed compress call wrote must come back byte for byte, into buffers at any alignment, with
nothing written outside them; every refusal happens before anything is queued (the mock's counters); a frame of the wrong length fails
the call; the compress side is not affected.  Every comparison is byte-exact."""
import ctypes as C
import os
import subprocess
import threading
import time

import pytest

import qz_bind as B
import qz_corpus as K
import qz_device as D
import test_device_checksum_mock as T

ROOT = T.ROOT
MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_restoremock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_restoremock.so")
NOUNGROUP_MOCK_SO = os.path.join(MOCK, "libqatseqprod_noungroupmock.so")
NOUNGROUP_FRONT_SO = os.path.join(MOCK, "libqzstdfront_noungroupmock.so")
GUARD = 64
CHUNK = 32768
SIZES = (0, 1, 7, 8191, CHUNK, CHUNK + 1, 100001, 4 * CHUNK)
ELEMS = (2, 1, 4, 2, 0, 8, 4, 2)  # 0: the front's setting
KINDS = ("bf16", "text", "fp32", "bf16", "fp32", "ids64", "ids32", "fp16")


def build_pair(zstd_path, mock_so, front_so, ungroup: bool):
    """the mock of tests/test_device_group_mock.py (group = True), with tests/mock/mock_hip_ungroup.c or — an older device layer — without"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c")]
    if ungroup:
        srcs.append(os.path.join(MOCK, "mock_hip_ungroup.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def bind_hooks(plug):
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    plug.lib.qzstd_mock_ungroup_rows.restype = C.c_ulonglong
    return plug


@pytest.fixture(scope="module")
def restoremock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, ungroup=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    return bind_hooks(plug), F


class OutPool:
    """host memory the mock treats as device memory, filled with 0xA5: buffer i at `offsets[i]` bytes past a 16-aligned place behind its
    neighbour, or packed: every buffer right behind the one before it, wherever that ends; guards on both sides"""

    def __init__(self, plug, sizes, offsets, slot=1, dev=0, packed=False):
        self.place, pos = [], GUARD
        for n, o in zip(sizes, offsets):
            pos = pos if packed else ((pos + 15) & ~15) + o
            self.place.append(pos)
            pos += n
        self.size = pos + GUARD
        self.raw = C.create_string_buffer(self.size + 64)
        self.base = (C.addressof(self.raw) + 63) & ~63
        C.memset(self.base, 0xA5, self.size)
        self.bufs = [(self.base + p, n) for p, n in zip(self.place, sizes)]
        plug.lib.qzstd_mock_device_range(slot, self.base, self.size, dev)

    def bytes(self):
        return C.string_at(self.base, self.size)

    def expected(self, datas):
        want = bytearray(b"\xa5" * self.size)
        for p, d in zip(self.place, datas):
            want[p:p + len(d)] = d
        return bytes(want)

    def untouched(self):
        return self.bytes() == b"\xa5" * self.size


def corpus():
    return [D.typed_corpus(kind, n, 40 + i) if kind != "text" else K.by_name("text", n, seed=40 + i) for i, (kind, n) in enumerate(zip(KINDS, SIZES))]


def queued(plug, fr):
    """what moves when a restore call gets as far as the GPU: the event wait on the caller's stream, the launches, the call's own counters"""
    return plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_ungroup_launches(), plug.lib.qzstd_mock_ungroup_rows(), fr.restore_stats()


def parts_of(sizes, chunk, part):
    """the restore's parts: whole frames, at most `part` bytes of content, at least one frame -> (parts, frames, stage bytes)"""
    lens = [min(chunk, n - o) for n in sizes for o in range(0, n, chunk)]
    parts, cur = 0, None
    for n in lens:
        if cur is None or cur + n > part:
            parts, cur = parts + 1, 0
        cur += n
    return parts, len(lens), sum((n + 15) & ~15 for n in lens)


@pytest.mark.parametrize("checksum", (False, True))
@pytest.mark.parametrize("compact", (False, True))
def test_what_the_typed_call_wrote_comes_back(restoremock, zstd, monkeypatch, checksum, compact):
    plug, F = restoremock
    datas = corpus()
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * CHUNK))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_byte_group(4) == 0 and fr.set_checksum(checksum) == 0
        src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))])
        frames = fr.compress_device_batch_typed(src.bufs, ELEMS)
        assert all(T.flagged(f) == checksum for per in frames for f in per)
        out = OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5)[i] for i in range(len(SIZES))])
        st0, ev0, l0 = fr.restore_stats(), plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_ungroup_launches()
        n = fr.restore_batch(frames, out.bufs, ELEMS, compact=compact)
        parts, nf, stage = parts_of(SIZES, CHUNK, 3 * CHUNK)
        assert n == nf and parts >= 3
        assert out.bytes() == out.expected(datas)
        st1 = fr.restore_stats()
        assert [a - b for a, b in zip(st1, st0)] == [nf, sum(SIZES), stage, parts]
        assert plug.lib.qzstd_mock_ungroup_launches() == l0 + parts and plug.lib.qzstd_mock_event_waits() == ev0 + 2
    finally:
        fr.close()


def test_buffers_packed_back_to_back_and_the_single_buffer_call(restoremock, zstd):
    plug, F = restoremock
    datas = [d for d in corpus() if d]
    sizes = [len(d) for d in datas]
    elems = [e or 4 for e, n in zip(ELEMS, SIZES) if n]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [0] * len(datas))
        frames = fr.compress_device_batch_typed(src.bufs, elems)
        out = OutPool(plug, sizes, [0] * len(sizes), packed=True)  # no gap: neighbours share 16-byte words
        assert fr.restore_batch(frames, out.bufs, elems) == sum(len(f) for f in frames)
        assert out.bytes() == out.expected(datas)
        # one buffer, the front's element size
        assert fr.set_byte_group(8) == 0
        one = fr.compress_device(*src.bufs[-1])
        out = OutPool(plug, sizes[-1:], [9])
        assert fr.restore_device_raw(one, out.bufs[0][0], sizes[-1]) == len(one)
        assert out.bytes() == out.expected(datas[-1:])
        assert fr.restore_device_raw([], out.bufs[0][0], 0) == 0
    finally:
        fr.close()


@pytest.mark.parametrize("checksum", (False, True))
def test_foreign_frames_and_a_front_without_the_producer(restoremock, zstd, checksum):
    """ZSTD_compress2 over the grouped chunks (libzstd's own blocks, other content-size fields); restored by a front created with
    useProducer = 0, whose checksum setting is off: the decoder verifies what the frames carry"""
    plug, F = restoremock
    datas = corpus()
    ks = [e or 2 for e in ELEMS]
    frames = [D.foreign_frames(zstd, d, CHUNK, k, checksum=checksum, lib=F) for d, k in zip(datas, ks)]
    assert all(T.flagged(f) == checksum for per in frames for f in per)
    fr = D.DeviceFront(2, 1, CHUNK, use_producer=0, lib=F)
    try:
        assert fr.set_byte_group(2) == 0
        out = OutPool(plug, SIZES, [i % 16 for i in range(len(SIZES))])
        assert fr.restore_batch(frames, out.bufs, ELEMS) == sum(len(f) for f in frames)
        assert out.bytes() == out.expected(datas)
        assert fr.compress_device_raw(*out.bufs[3])[0] == D.ERROR  # (the compress calls still refuse such a front)
    finally:
        fr.close()


def test_refusals_before_anything_is_queued(restoremock, zstd):
    plug, F = restoremock
    datas = [D.typed_corpus("bf16", 2 * CHUNK + 5, 1), D.typed_corpus("fp32", 1000, 2)]
    sizes = [len(d) for d in datas]
    frames = [D.foreign_frames(zstd, d, CHUNK, 2, lib=F) for d in datas]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        out = OutPool(plug, sizes, [3, 0])
        other = OutPool(plug, sizes, [0, 0], slot=2, dev=1)
        host = C.create_string_buffer(sizes[1])
        before = queued(plug, fr)
        assert fr.restore_batch_raw(frames, out.bufs, [2, 2], n_frames=3) == D.ERROR  # wrong nFrames: 4 it is
        assert fr.restore_batch_raw(frames, out.bufs, [2, 2], n_frames=5) == D.ERROR
        for bad in (3, 5, 16, 255):
            assert fr.restore_batch_raw(frames, out.bufs, [2, bad]) == D.ERROR
        assert fr.restore_batch_raw(frames, [out.bufs[0], (C.addressof(host), sizes[1])], [2, 2]) == D.ERROR  # a host pointer
        assert fr.restore_batch_raw(frames, [out.bufs[0], (0, sizes[1])], [2, 2]) == D.ERROR  # a null one
        assert fr.restore_batch_raw(frames, [out.bufs[0], other.bufs[1]], [2, 2]) == D.ERROR  # two devices
        big = out.size  # from the first buffer's place on, that ends behind the device memory
        assert fr.restore_batch_raw(frames, [(out.bufs[0][0], big), out.bufs[1]], [2, 2], n_frames=-(-big // CHUNK) + 1) == D.ERROR
        assert F.QZSTD_frontRestoreDeviceBatchTyped(None, None, 0, None, 0, None, None, 0, None) == D.ERROR
        assert queued(plug, fr) == before and out.untouched() and other.untouched()
        assert fr.restore_batch_raw([[], []], [(0, 0), (out.bufs[1][0], 0)], None) == 0  # nothing to do: no GPU touched
        assert queued(plug, fr) == before
        assert fr.restore_batch(frames, out.bufs, [2, 2]) == 4 and out.bytes() == out.expected(datas)
    finally:
        fr.close()


def test_a_call_while_another_one_runs_is_refused(restoremock, zstd):
    plug, F = restoremock
    datas = [D.typed_corpus("bf16", 3 * CHUNK + 5, 31)]
    frames = [D.foreign_frames(zstd, datas[0], CHUNK, 2, lib=F)]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    got = {}
    try:
        out = OutPool(plug, [len(datas[0])], [5])
        second = OutPool(plug, [len(datas[0])], [0], slot=2)
        plug.lib.qzstd_mock_stall_ms(50000)  # every stream looks busy until released below: the first call waits for its slot's stream
        th = threading.Thread(target=lambda: got.update(r=fr.restore_batch_raw(frames, out.bufs, [2])))
        th.start()
        deadline = time.monotonic() + 50
        seen = None
        while time.monotonic() < deadline:  # (the setting is refused while a call runs: that is how the test sees the call has begun)
            if fr.set_byte_group(1) != 0:
                before = plug.lib.qzstd_mock_ungroup_launches(), plug.lib.qzstd_mock_event_waits()
                seen = fr.restore_batch_raw(frames, second.bufs, [2])
                after = plug.lib.qzstd_mock_ungroup_launches(), plug.lib.qzstd_mock_event_waits()
                break
        plug.lib.qzstd_mock_stall_ms(0)
        th.join(60)
        assert seen == D.ERROR and before == after and second.untouched()
        assert got["r"] == 4 and out.bytes() == out.expected(datas)
        assert fr.restore_batch(frames, second.bufs, [2]) == 4 and second.bytes() == second.expected(datas)
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


@pytest.mark.parametrize("delta", (-1, 1))
def test_a_frame_of_another_length_fails_the_call(restoremock, zstd, delta):
    """one frame decodes to a byte fewer / a byte more than its chunk: (size_t)-1, nothing outside the buffers written, and the next good
    call on the same front succeeds"""
    plug, F = restoremock
    data = K.by_name("text", 5 * CHUNK + 100, seed=9)
    frames = D.foreign_frames(zstd, data, CHUNK, 1, lib=F)
    zc = zstd.cctx(3)
    piece = data[3 * CHUNK:4 * CHUNK]
    wrong = list(frames)
    wrong[3] = zstd.compress2(zc, piece[:-1] if delta < 0 else piece + b"x")
    zstd.free(zc)
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        out = OutPool(plug, [len(data)], [7])
        assert fr.restore_batch_raw([wrong], out.bufs, [1]) == D.ERROR
        got = out.bytes()
        assert got[:out.place[0]] == b"\xa5" * out.place[0] and got[out.place[0] + len(data):] == b"\xa5" * GUARD
        assert fr.restore_batch([frames], out.bufs, [1]) == 6 and out.bytes() == out.expected([data])
    finally:
        fr.close()


def test_a_damaged_checksummed_frame_fails_the_call(restoremock, zstd):
    plug, F = restoremock
    data = D.typed_corpus("bf16", 3 * CHUNK, 4)
    frames = D.foreign_frames(zstd, data, CHUNK, 2, checksum=True, lib=F)
    bad = list(frames)
    bad[1] = bad[1][:-1] + bytes([bad[1][-1] ^ 1])  # (the stored hash itself: the content decodes, the comparison fails)
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        out = OutPool(plug, [len(data)], [1])
        assert fr.restore_batch_raw([bad], out.bufs, [2]) == D.ERROR
        assert fr.restore_batch([frames], out.bufs, [2]) == 3 and out.bytes() == out.expected([data])
    finally:
        fr.close()


def test_the_compress_calls_are_unchanged_by_a_restore_in_between(restoremock, zstd):
    plug, F = restoremock
    datas = [d for d in corpus() if d][:5]
    elems = [2, 1, 4, 8, 2]
    never = D.DeviceFront(2, 1, CHUNK, lib=F)
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [1, 0, 3, 0, 15])
        want = never.compress_device_batch_typed(src.bufs, elems)
        st = [fr.stats(), fr.byte_group_stats(), fr.checksum_stats()]
        first = fr.compress_device_batch_typed(src.bufs, elems)
        d1 = [fr.stats(), fr.byte_group_stats(), fr.checksum_stats()]
        out = OutPool(plug, [len(d) for d in datas], [2] * len(datas))
        fr.restore_batch(first, out.bufs, elems)
        assert [fr.stats(), fr.byte_group_stats(), fr.checksum_stats()] == d1  # a restore moves none of the compress side's counters
        second = fr.compress_device_batch_typed(src.bufs, elems)
        d2 = [fr.stats(), fr.byte_group_stats(), fr.checksum_stats()]
        assert first == second == want
        delta = lambda a, b: [[y - x for x, y in zip(p, q)] for p, q in zip(a, b)]  # noqa: E731
        assert delta(st, d1) == delta(d1, d2)
        assert fr.compress_host(datas[1]) == never.compress_host(datas[1])
        assert never.restore_stats() == [0, 0, 0, 0]
    finally:
        never.close()
        fr.close()


def test_device_layer_without_the_ungroup_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT mock_hip_ungroup.c: the restore returns (size_t)-1 with no launch, no event wait and
    nothing counted; the compress calls work as before (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOUNGROUP_MOCK_SO, NOUNGROUP_FRONT_SO, ungroup=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
pool = T.Pool(plug, [data], [0])
fr = D.DeviceFront(2, 1, chunk, lib=F)
frames = fr.compress_device_batch_typed(pool.bufs, [2])
out = R.OutPool(plug, [len(data)], [3])
before = plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches()
r1 = fr.restore_batch_raw(frames, out.bufs, [2])
r2 = fr.restore_device_raw(frames[0], out.bufs[0][0], len(data))
same = (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches()) == before
print(json.dumps({"refused": [r1, r2] == [D.ERROR] * 2, "nothing_queued": same and out.untouched(), "stats": fr.restore_stats(),
                  "has_ungroup": hasattr(plug.lib, "qzstd_hip_ungroup"),
                  "round_trip": all(D.ungroup_bytes(z.decompress(f, chunk), 2, F) == data[c * chunk:(c + 1) * chunk] for c, f in enumerate(frames[0]))}))
""", NOUNGROUP_MOCK_SO, NOUNGROUP_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "stats": [0, 0, 0, 0], "has_ungroup": False, "round_trip": True}, res
