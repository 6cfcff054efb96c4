"""CPU: byte-grouped frames (QZSTD_frontSetByteGroup, QZSTD_frontCompressDeviceBatchTyped: include/qzstd_frontend_device.h) over the mock device
layer — the mock of tests/test_device_checksum_mock.py plus tests/mock/mock_hip_group.c (qzstd_hip_group in plain C) and
tests/mock/mock_fail_block.c (a matcher error on demand).  Every frame of the
single call, the batch call and the typed batch call must be byte for byte the frame libzstd builds from the ORACLE's sequences over the grouped
content, one block per plane (qz_device.reference_frames_grouped), decode, and ungroup to the input."""
import ctypes as C
import json
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
MOCK_SO = os.path.join(MOCK, "libqatseqprod_groupmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_groupmock.so")
NOGROUP_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nogroupmock.so")
NOGROUP_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nogroupmock.so")


def build_pair(zstd_path, mock_so, front_so, group: bool):
    """group: with tests/mock/mock_hip_group.c, and with tests/mock/mock_fail_block.c in front of mock_hip.c's match-finder (mock_hip.c alone
    is compiled with its qzstd_hip_find_sequences renamed; every caller, the host path included, then reaches it through the hook)"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(MOCK, "mock_hip_device.c"), os.path.join(MOCK, "mock_hip_gather.c"), os.path.join(MOCK, "mock_hip_xxh64.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    if group:
        obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
        subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
        srcs += [obj, os.path.join(MOCK, "mock_hip_group.c"), os.path.join(MOCK, "mock_fail_block.c")]
    else:
        obj = None
        srcs.append(os.path.join(MOCK, "mock_hip.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if obj and os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def groupmock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, group=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    plug.lib.qzstd_mock_fail_block.argtypes = [C.c_int]
    plug.lib.qzstd_mock_group_rows.restype = C.c_ulonglong
    D.bind(F)
    return plug, F


def typed(kind, n, seed):
    return D.typed_corpus(kind, n, seed) if kind in ("bf16", "fp16", "fp32", "ids32", "ids64") else K.by_name(kind, n, seed=seed)


def check(zstd, F, got, want, datas, chunk, ks, flag=False):
    assert len(got) == len(want) == len(datas)
    for i, (g, w, d, k) in enumerate(zip(got, want, datas, ks)):
        assert len(g) == len(w) == (len(d) + chunk - 1) // chunk, i
        for c, f in enumerate(g):
            assert f == w[c], "buffer %d frame %d (k = %d) differs from the reference" % (i, c, k)
            assert T.flagged(f) == flag, (i, c)
            content = zstd.decompress(f, chunk)  # (libzstd's decoder verifies the checksum of a flagged frame)
            assert D.ungroup_bytes(content, k, F) == d[c * chunk:(c + 1) * chunk], (i, c)


CASES = {
    "chunk4k_no_cuts": (4096, [("bf16", 5 * 4096 + 7), ("text", 4096), ("ids32", 3 * 4096 - 1)]),
    "chunk128k_partial": (131072, [("bf16", 2 * 131072 + 4321), ("mix", 50001), ("ids64", 131072 + 9)]),
    "unequal_unaligned_empty": (32768, [("fp32", 0), ("fp32", 1), ("text", 15), ("fp16", 16), ("ids32", 32767), ("fp32", 32769), ("bf16", 0),
                                        ("system", 40003)]),
}


@pytest.mark.parametrize("k", (2, 4, 8))
@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_frames_equal_the_reference(groupmock, zstd, oracle, name, k):
    plug, F = groupmock
    chunk, spec = CASES[name]
    datas = [typed(kind, n, 3 + i) if n else b"" for i, (kind, n) in enumerate(spec)]
    want = [D.reference_frames_grouped(zstd, oracle, d, chunk, 1, k, lib=F) for d in datas]
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        for offsets in ([0] * len(datas), [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))]):
            pool = T.Pool(plug, datas, offsets)
            assert fr.get_byte_group() == 1
            typed_got = fr.compress_device_batch_typed(pool.bufs, [k] * len(datas))  # the front's setting is 1: the entries decide
            check(zstd, F, typed_got, want, datas, chunk, [k] * len(datas))
            assert fr.set_byte_group(k) == 0 and fr.get_byte_group() == k
            check(zstd, F, fr.compress_device_batch(pool.bufs), want, datas, chunk, [k] * len(datas))
            check(zstd, F, fr.compress_device_batch_typed(pool.bufs, None), want, datas, chunk, [k] * len(datas))
            single = [fr.compress_device(p, n) if n else [] for p, n in pool.bufs]
            check(zstd, F, single, want, datas, chunk, [k] * len(datas))
            assert fr.set_byte_group(1) == 0
    finally:
        fr.close()


def test_planes_of_192k_in_384k_frames(groupmock, zstd, oracle):
    """chunk 384 KiB, k = 2: planes of 192 KiB, each cut again at 128 KiB — four blocks per full frame; several parts"""
    plug, F = groupmock
    chunk = 393216
    datas = [typed("bf16", chunk + 70001, 5), typed("text", chunk, 6)]
    want = [D.reference_frames_grouped(zstd, oracle, d, chunk, 1, 2, lib=F) for d in datas]
    pool = T.Pool(plug, datas, [3, 0])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.set_byte_group(2) == 0
        check(zstd, F, fr.compress_device_batch(pool.bufs), want, datas, chunk, [2, 2])
        check(zstd, F, [fr.compress_device(*b) for b in pool.bufs], want, datas, chunk, [2, 2])
    finally:
        fr.close()


def test_mixed_element_sizes_in_one_typed_batch(groupmock, zstd, oracle, monkeypatch):
    """a checkpoint: bf16 weights, fp32 norms, int64 ids and plain bytes in one call; 0 means the front's setting; small parts, so that
    grouped and plain frames share parts and slots alternate"""
    plug, F = groupmock
    chunk = 32768
    spec = [("bf16", 3 * chunk + 2, 0), ("fp32", chunk + 5, 4), ("text", 2 * chunk + 1, 1), ("ids64", 70000, 8), ("fp32", 4097 * 4, 0),
            ("bf16", 9000, 2), ("mix", 100, 1)]
    datas = [typed(kind, n, 20 + i) for i, (kind, n, _) in enumerate(spec)]
    elems = [e for _, _, e in spec]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        assert fr.set_byte_group(4) == 0
        ks = [e or 4 for e in elems]
        want = [D.reference_frames_grouped(zstd, oracle, d, chunk, 1, k, lib=F) if k > 1 else D.reference_frames(zstd, oracle, d, chunk, 1)
                for d, k in zip(datas, ks)]
        pool = T.Pool(plug, datas, [(0, 1, 3, 15)[i % 4] for i in range(len(datas))])
        check(zstd, F, fr.compress_device_batch_typed(pool.bufs, elems), want, datas, chunk, ks)
        n_frames = sum(len(w) for w in want)
        assert fr.lib.QZSTD_frontDeviceBatchFrames(fr.f, fr.batch(pool.bufs)[0], len(datas)) == n_frames
    finally:
        fr.close()


@pytest.mark.parametrize("level,chunk", [(6, 131072), (12, 32768)])
def test_chain_levels(groupmock, zstd, oracle, level, chunk):
    plug, F = groupmock
    datas = [typed("fp32", 2 * chunk + 4321, 9), typed("ids32", chunk + 3, 10)]
    want = [D.reference_frames_grouped(zstd, oracle, d, chunk, level, 4, lib=F) for d in datas]
    pool = T.Pool(plug, datas, [1, 0])
    fr = D.DeviceFront(2, level, chunk, lib=F)
    try:
        assert fr.set_byte_group(4) == 0
        check(zstd, F, fr.compress_device_batch(pool.bufs), want, datas, chunk, [4, 4])
    finally:
        fr.close()


def test_checksums_cover_the_grouped_content(groupmock, zstd, oracle):
    plug, F = groupmock
    chunk = 65536
    datas = [typed("bf16", 3 * chunk + 11, 1), typed("text", chunk + 100, 2)]
    want = [D.reference_frames_grouped(zstd, oracle, d, chunk, 1, 2, checksum=True, lib=F) for d in datas]
    pool = T.Pool(plug, datas, [3, 0])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.set_byte_group(2) == 0 and fr.set_checksum(1) == 0
        got = fr.compress_device_batch(pool.bufs)
        check(zstd, F, got, want, datas, chunk, [2, 2], flag=True)
        gpu, lib = fr.checksum_stats()
        assert gpu > 0 and lib > 0 and gpu + lib == 6, (gpu, lib)  # text frames: the GPU's hash; weights: raw mantissa blocks, libzstd's
        bad = got[1][0][:-1] + bytes([got[1][0][-1] ^ 1])
        with pytest.raises(RuntimeError):
            zstd.decompress(bad, chunk)
    finally:
        fr.close()


def test_refusals(groupmock, zstd):
    plug, F = groupmock
    chunk = 32768
    data = typed("bf16", 2 * chunk + 5, 1)
    pool = T.Pool(plug, [data], [0])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        for k in (0, 3, 5, 6, 7, 9, 16, 256):
            assert fr.set_byte_group(k) == -1 and fr.get_byte_group() == 1
        assert F.QZSTD_frontSetByteGroup(None, 2) == -1 and F.QZSTD_frontGetByteGroup(None) == 1
        before, rows, st = plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_rows(), fr.stats()
        for bad in (3, 5, 16, 255):
            assert fr.compress_device_batch_typed_raw(pool.bufs + pool.bufs, [2, bad])[0] == D.ERROR
        assert (plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_rows(), fr.stats()) == (before, rows, st)  # nothing queued
        host_plain = fr.compress_host(data)
        assert fr.set_byte_group(2) == 0
        assert fr.call_host(C.addressof(pool.raw), len(data))[0] == D.ERROR  # the host call while grouping is on
        assert fr.set_byte_group(1) == 0 and fr.compress_host(data) == host_plain
    finally:
        fr.close()


def test_setting_is_refused_while_a_call_runs(groupmock, zstd, oracle):
    plug, F = groupmock
    chunk = 32768
    datas = [typed("bf16", 3 * chunk + 5, 31)]
    want = [D.reference_frames_grouped(zstd, oracle, datas[0], chunk, 1, 2, lib=F)]
    pool = T.Pool(plug, datas, [3])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    got = {}
    try:
        assert fr.set_byte_group(2) == 0
        plug.lib.qzstd_mock_stall_ms(50000)  # every stream looks busy until released below
        th = threading.Thread(target=lambda: got.update(frames=fr.compress_device_batch(pool.bufs)))
        th.start()
        deadline = time.monotonic() + 50
        seen = []
        while time.monotonic() < deadline:  # (setting it to what it is: the call sees the same value whenever it starts)
            r = fr.set_byte_group(2)
            if r != 0:
                seen = [r, fr.set_byte_group(1), fr.get_byte_group()]
                break
        plug.lib.qzstd_mock_stall_ms(0)
        th.join(60)
        assert seen == [-1, -1, 2], seen
        # (a stalled mock publishes no counts: that call's blocks may count as failed, and its frames are then any valid frames)
        for c, f in enumerate(got["frames"][0]):
            assert D.ungroup_bytes(zstd.decompress(f, chunk), 2, F) == datas[0][c * chunk:(c + 1) * chunk], c
        check(zstd, F, fr.compress_device_batch(pool.bufs), want, datas, chunk, [2])
        assert fr.set_byte_group(1) == 0 and fr.get_byte_group() == 1
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


def test_device_layer_without_the_group_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT mock_hip_group.c: grouping asked for -> (size_t)-1 before anything is queued, by the
    setting and by the typed call's entries; without it everything works (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOGROUP_MOCK_SO, NOGROUP_FRONT_SO, group=False)
    res = T.run_child("""
chunk = 65536
data = K.by_name("system", 3 * chunk + 321)
pool = T.Pool(plug, [data], [0])
fr = D.DeviceFront(2, 1, chunk, lib=F)
plain = fr.compress_device(*pool.bufs[0])
assert fr.set_byte_group(2) == 0
before, st = plug.lib.qzstd_mock_launches(), fr.stats()
r1 = fr.compress_device_raw(*pool.bufs[0])[0]
r2 = fr.compress_device_batch_raw(pool.bufs)[0]
r3 = fr.compress_device_batch_typed_raw(pool.bufs, [0])[0]
fr.set_byte_group(1)
r4 = fr.compress_device_batch_typed_raw(pool.bufs, [4])[0]
refused = [r1, r2, r3, r4] == [D.ERROR] * 4 and plug.lib.qzstd_mock_launches() == before and fr.stats() == st
typed_plain = fr.compress_device_batch_typed(pool.bufs, [1])[0]
print(json.dumps({"refused": refused, "off_same": fr.compress_device(*pool.bufs[0]) == plain == typed_plain,
                  "has_group": hasattr(plug.lib, "qzstd_hip_group")}))
""", NOGROUP_MOCK_SO, NOGROUP_FRONT_SO)
    assert res == {"refused": True, "off_same": True, "has_group": False}, res


def test_weights_rebuild_their_content_and_copy_nothing_back(groupmock, zstd, oracle):
    """seeded bf16 weights: the mantissa plane is a raw block, so frames need their content — rebuilt from the arena (s[1]), none copied
    back (s[2]); device->host traffic stays below the input plus 8 bytes per sequence and per block header"""
    plug, F = groupmock
    chunk = 131072
    data = typed("bf16", 6 * chunk + 1000, 0)
    counts = {}
    want = [D.reference_frames_grouped(zstd, oracle, data, chunk, 1, 2, lib=F, counts=counts)]
    pool = T.Pool(plug, [data], [0])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.set_byte_group(2) == 0
        st0 = fr.stats()
        check(zstd, F, fr.compress_device_batch(pool.bufs), want, [data], chunk, [2])
        st1, s = fr.stats(), fr.byte_group_stats()
        assert s[1] > 0 and s[2] == 0 and sum(s) == 7, s
        assert st1[0] - st0[0] == s[0] and st1[1] - st0[1] == s[1], (st0, st1, s)
        assert counts["blocks"] == 13  # six frames of two planes, the last (500 elements) one block
        assert st1[2] - st0[2] <= len(data) + 8 * (counts["entries"] + counts["blocks"]), (st0, st1, counts)
        assert st1[3] - st0[3] == len(data)
    finally:
        fr.close()


def test_a_failed_block_copies_the_bytes_back_and_still_round_trips(groupmock, zstd, oracle):
    plug, F = groupmock
    chunk = 65536
    data = typed("bf16", 3 * chunk + 77, 2)
    want = D.reference_frames_grouped(zstd, oracle, data, chunk, 1, 2, lib=F)
    pool = T.Pool(plug, [data], [1])
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.set_byte_group(2) == 0
        plug.lib.qzstd_mock_fail_block(3)  # the second frame's second block (its mantissa plane)
        st0 = fr.stats()
        got = fr.compress_device(*pool.bufs[0])
        plug.lib.qzstd_mock_fail_block(-1)
        s, st1 = fr.byte_group_stats(), fr.stats()
        assert s[2] == 1 and sum(s) == 4, s
        assert st1[2] - st0[2] >= chunk  # that frame's bytes came back
        for c, f in enumerate(got):
            assert D.ungroup_bytes(zstd.decompress(f, chunk), 2, F) == data[c * chunk:(c + 1) * chunk], c
            if c != 1:
                assert f == want[c], c  # (the failed frame is any valid frame of the grouped content)
    finally:
        plug.lib.qzstd_mock_fail_block(-1)
        fr.close()


def test_back_at_one_the_frames_are_the_ungrouped_ones(groupmock, zstd, oracle):
    plug, F = groupmock
    chunk = 32768
    datas = [typed("bf16", 3 * chunk + 5, 11), K.by_name("text", 2 * chunk + 7, seed=12), os.urandom(chunk + 100)]
    pool = T.Pool(plug, datas, [0, 3, 1])
    never = D.DeviceFront(1, 1, chunk, lib=F)
    fr = D.DeviceFront(1, 1, chunk, lib=F)
    try:
        plain = never.compress_device_batch(pool.bufs)
        assert plain == [D.reference_frames(zstd, oracle, d, chunk, 1) for d in datas]
        plain_host = [never.compress_host(d) for d in datas]
        for k in (2, 1, 8, 1):
            assert fr.set_byte_group(k) == 0
            got = fr.compress_device_batch(pool.bufs)
            if k == 1:
                assert got == plain
                assert [fr.compress_device(p, n) for p, n in pool.bufs] == plain
                assert [fr.compress_host(d) for d in datas] == plain_host
                assert fr.compress_device_batch_typed(pool.bufs, [1, 0, 1]) == plain
            else:
                assert got != plain
        assert never.byte_group_stats() == [0, 0, 0]
    finally:
        never.close()
        fr.close()
