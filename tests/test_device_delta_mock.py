"""CPU: the delta calls (QZSTD_frontCompressDeviceBatchDelta, QZSTD_frontRestoreDeviceBatchDelta, QZSTD_frontDeltaStats:
include/qzstd_frontend_device.h) over the mock device layer — the mock of tests/test_device_restore_mock.py plus tests/mock/mock_hip_group_xor.c
and mock_hip_ungroup_xor.c (the two XOR kernels in plain C).  A delta frame must be byte for byte the Typed call's frame of the pre-XORed
buffer; what the delta compress wrote must come back onto the bases, also in place; a buffer without a base is untouched by its neighbours'
bases; every refusal happens before anything is queued (the mock's counters).  Every comparison is byte-exact."""
import ctypes as C
import os

import pytest

import qz_bind as B
import qz_corpus as K
import qz_device as D
import test_device_checksum_mock as T
import test_device_restore_mock as R

ROOT = T.ROOT
MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_deltamock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_deltamock.so")
NOXOR_MOCK_SO = os.path.join(MOCK, "libqatseqprod_noxormock.so")
NOXOR_FRONT_SO = os.path.join(MOCK, "libqzstdfront_noxormock.so")
CHUNK = 32768
SIZES = (0, 1, 7, 8191, CHUNK, CHUNK + 1, 100001, 4 * CHUNK, 0, 3 * CHUNK + 5)
ELEMS = (2, 1, 4, 2, 1, 8, 4, 2, 4, 8)
KINDS = ("bf16", "text", "fp32", "bf16", "text", "ids64", "fp32", "fp16", "fp32", "ids64")
BASED = tuple(i % 3 != 2 for i in range(len(SIZES)))  # every third buffer has no base


def build_pair(zstd_path, mock_so, front_so, xor: bool):
    """the mock of tests/test_device_restore_mock.py (group, ungroup, fail-block), with the two XOR stand-ins or — an older device layer — without"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    import subprocess
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c")]
    if xor:
        srcs += [os.path.join(MOCK, n) for n in ("mock_hip_group_xor.c", "mock_hip_ungroup_xor.c")]
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def bind_hooks(plug):
    plug.lib.qzstd_mock_fail_block.argtypes = [C.c_int]
    for n in ("qzstd_mock_group_xor_rows", "qzstd_mock_ungroup_xor_rows", "qzstd_mock_group_rows", "qzstd_mock_ungroup_rows"):
        if hasattr(plug.lib, n):
            getattr(plug.lib, n).restype = C.c_ulonglong
    return plug


@pytest.fixture(scope="module")
def deltamock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, xor=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    return bind_hooks(plug), F


def xor(a: bytes, b: bytes) -> bytes:
    return (int.from_bytes(a, "little") ^ int.from_bytes(b, "little")).to_bytes(len(a), "little")


def corpus():
    """(the new buffers, their bases): typed data and a base that differs from it in few bits (a small step), text and a base of other text"""
    import numpy as np
    datas, bases = [], []
    for i, (kind, n) in enumerate(zip(KINDS, SIZES)):
        d = D.typed_corpus(kind, n, 60 + i) if kind != "text" else K.by_name("text", n, seed=60 + i)
        if kind == "text":
            b = K.by_name("mix", n, seed=90 + i)
        else:
            flips = (np.random.default_rng(i).random(n) < 0.2) * np.random.default_rng(100 + i).integers(0, 8, n)
            b = (np.frombuffer(d, dtype=np.uint8) ^ flips.astype(np.uint8)).tobytes()
        datas.append(d)
        bases.append(b)
    return datas, bases


def pools(plug, datas, bases, based=BASED):
    """three device pools: the buffers at odd offsets, their bases at OTHER offsets (src and base differ mod 16), the pre-XORed buffers"""
    src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))], slot=0)
    bas = T.Pool(plug, bases, [(7, 0, 2, 9, 15, 4)[i % 6] for i in range(len(datas))], slot=1)
    pre = T.Pool(plug, [xor(d, b) if on else d for d, b, on in zip(datas, bases, based)], [0] * len(datas), slot=2)
    return src, bas, pre, [b if on else None for b, on in zip(bas.bufs, based)]


def launches(plug):
    L = plug.lib
    return (L.qzstd_mock_group_xor_launches(), L.qzstd_mock_ungroup_xor_launches(), L.qzstd_mock_group_launches(), L.qzstd_mock_ungroup_launches(),
            L.qzstd_mock_gather_launches(), L.qzstd_mock_event_waits())


@pytest.mark.parametrize("checksum", (False, True))
def test_delta_frames_are_the_typed_frames_of_the_prexored_buffers_and_come_back(deltamock, zstd, monkeypatch, checksum):
    plug, F = deltamock
    datas, bases = corpus()
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * CHUNK))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_checksum(checksum) == 0
        src, bas, pre, given = pools(plug, datas, bases)
        want = fr.compress_device_batch_typed(pre.bufs, ELEMS)
        plain = fr.compress_device_batch_typed(src.bufs, ELEMS)
        d0, g0, l0 = fr.delta_stats(), fr.byte_group_stats(), launches(plug)
        got = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        assert got == want
        assert all(T.flagged(f) == checksum for per in got for f in per)
        for i, on in enumerate(BASED):
            if not on:
                assert got[i] == plain[i]  # a buffer without a base: the Typed call's frames, whatever its neighbours are
        # every frame decodes to the grouped delta
        for i, (d, b, k, on) in enumerate(zip(datas, bases, ELEMS, BASED)):
            content = xor(d, b) if on else d
            for c, f in enumerate(got[i]):
                assert D.ungroup_bytes(zstd.decompress(f, CHUNK), k, F) == content[c * CHUNK:(c + 1) * CHUNK], (i, c)
        d1 = fr.delta_stats()
        n_based = sum(len(per) for per, on in zip(got, BASED) if on)
        assert sum(d1[:3]) - sum(d0[:3]) == n_based and d1[2] == d0[2] and d1[3] == d0[3]
        assert bas.bufs and all(C.string_at(p, n) == b for (p, n), b in zip(bas.bufs, bases))  # the bases are only read
        # back: into fresh buffers with guards ...
        out = R.OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11)[i] for i in range(len(SIZES))], slot=3)
        r0 = fr.restore_stats()
        assert fr.restore_batch_delta(got, out.bufs, given, ELEMS) == sum(len(per) for per in got)
        assert out.bytes() == out.expected(datas)
        assert fr.delta_stats()[3] == d1[3] + n_based and fr.restore_stats()[0] == r0[0] + sum(len(per) for per in got)
        # ... and in place over the bases (the buffers without one: over whatever is there)
        assert fr.restore_batch_delta(got, bas.bufs, [b if on else None for b, on in zip(bas.bufs, BASED)], ELEMS) == sum(len(per) for per in got)
        assert all(C.string_at(p, n) == d for (p, n), d in zip(bas.bufs, datas))
        assert launches(plug)[0] > l0[0] and launches(plug)[1] > l0[1]
        assert fr.byte_group_stats()[2] == g0[2]
    finally:
        fr.close()


def test_in_place_over_buffers_packed_back_to_back(deltamock, zstd):
    """the bases ARE the destinations, neighbours share 16-byte words: old ^ delta everywhere, the guards untouched"""
    plug, F = deltamock
    datas, bases = corpus()
    keep = [i for i, n in enumerate(SIZES) if n]
    datas, bases, elems = [datas[i] for i in keep], [bases[i] for i in keep], [ELEMS[i] for i in keep]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [0] * len(datas), slot=0)
        bas = T.Pool(plug, bases, [3] * len(datas), slot=1)
        frames = fr.compress_device_batch_delta(src.bufs, bas.bufs, elems)
        out = R.OutPool(plug, [len(d) for d in datas], [0] * len(datas), slot=2, packed=True)
        for (p, n), b in zip(out.bufs, bases):
            C.memmove(p, b, n)
        assert fr.restore_batch_delta(frames, out.bufs, out.bufs, elems) == sum(len(f) for f in frames)
        assert out.bytes() == out.expected(datas)
    finally:
        fr.close()


def test_no_base_anywhere_is_the_typed_call_launch_for_launch(deltamock, zstd, monkeypatch):
    """bases NULL, or an array of {NULL, 0} only: no *_xor launch, the Typed call's launches and frames; and in a mixed call the parts that hold
    only base-less buffers launch none either"""
    plug, F = deltamock
    datas, bases = corpus()
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(2 * CHUNK))
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src, bas, pre, given = pools(plug, datas, bases)
        l0 = launches(plug)
        want = fr.compress_device_batch_typed(src.bufs, ELEMS)
        l1 = launches(plug)
        typed = [b - a for a, b in zip(l0, l1)]
        assert typed[0] == typed[1] == 0
        for none in (None, [None] * len(datas)):
            assert fr.compress_device_batch_delta(src.bufs, none, ELEMS) == want
            l2 = launches(plug)
            assert [b - a for a, b in zip(l1, l2)] == typed
            l1 = l2
        out = R.OutPool(plug, SIZES, [5] * len(SIZES), slot=3)
        assert fr.restore_batch_delta(want, out.bufs, None, ELEMS) == sum(len(f) for f in want)
        assert out.bytes() == out.expected(datas)
        assert launches(plug)[1] == l1[1] and launches(plug)[3] > l1[3]
        assert fr.delta_stats() == [0, 0, 0, 0]
        # one based buffer only, the last: only parts that hold its frames (at most one part per frame) use the XOR kernels
        only = [None] * (len(datas) - 1) + [bas.bufs[-1]]
        n_last = -(-SIZES[-1] // CHUNK)
        l3 = launches(plug)
        got = fr.compress_device_batch_delta(src.bufs, only, ELEMS)
        l4 = launches(plug)
        assert got[:-1] == want[:-1] and got[-1] != want[-1]
        assert 1 <= l4[0] - l3[0] <= n_last
        assert (l4[0] - l3[0]) + (l4[2] - l3[2]) + (l4[4] - l3[4]) == sum(typed[2:5])  # a launch per staged part, as the Typed call's
        assert l4[2] - l3[2] > 0
        out2 = R.OutPool(plug, SIZES, [9] * len(SIZES), slot=3)
        assert fr.restore_batch_delta(got, out2.bufs, only, ELEMS) == sum(len(f) for f in got)
        l5 = launches(plug)
        assert out2.bytes() == out2.expected(datas)
        assert 1 <= l5[1] - l4[1] <= n_last and l5[3] - l4[3] > 0
    finally:
        fr.close()


@pytest.mark.parametrize("k", (1, 4))
def test_failed_block_copies_back_both_buffers(deltamock, zstd, k):
    """the matcher fails block 0 of every launch: that frame has the caller's bytes AND the base's copied back (device stats [2] grows by twice
    its length beyond what the clean call moves), XORed and grouped on the host; it decodes to the grouped delta"""
    plug, F = deltamock
    n = 3 * CHUNK + 100
    data = D.typed_corpus("fp32", n, 5)
    base = D.typed_corpus("fp32", n, 6)
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, [data], [3], slot=0)
        bas = T.Pool(plug, [base], [8], slot=1)
        s0, d0 = fr.stats(), fr.delta_stats()
        clean = fr.compress_device_batch_delta(src.bufs, bas.bufs, [k])
        s1, d1 = fr.stats(), fr.delta_stats()
        assert d1[2] == d0[2]
        plug.lib.qzstd_mock_fail_block(0)
        try:
            got = fr.compress_device_batch_delta(src.bufs, bas.bufs, [k])
        finally:
            plug.lib.qzstd_mock_fail_block(-1)
        s2, d2 = fr.stats(), fr.delta_stats()
        assert d2[2] == d1[2] + 1
        assert s2[2] - s1[2] >= 2 * CHUNK and (s2[2] - s1[2]) - (s1[2] - s0[2]) <= 2 * CHUNK
        want = xor(data, base)
        for c, f in enumerate(got[0]):
            assert D.ungroup_bytes(zstd.decompress(f, CHUNK), k, F) == want[c * CHUNK:(c + 1) * CHUNK], c
        assert got[0][1:] == clean[0][1:]
        out = R.OutPool(plug, [n], [7], slot=2)
        assert fr.restore_batch_delta(got, out.bufs, bas.bufs, [k]) == len(got[0])
        assert out.bytes() == out.expected([data])
    finally:
        fr.close()


def test_k1_frame_that_needs_its_content_is_rebuilt_not_copied_back(deltamock, zstd):
    """elem = 1 and a delta of noise (two unrelated random buffers): libzstd stores the block raw, the content is rebuilt from the frame's own
    entries and literals — delta stats [1], no copy of either buffer"""
    plug, F = deltamock
    n = 2 * CHUNK
    data, base = os.urandom(n), os.urandom(n)
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, [data], [1], slot=0)
        bas = T.Pool(plug, [base], [6], slot=1)
        pre = T.Pool(plug, [xor(data, base)], [0], slot=2)
        t0 = fr.stats()
        want = fr.compress_device_batch_typed(pre.bufs, [1])
        s0 = fr.stats()
        got = fr.compress_device_batch_delta(src.bufs, bas.bufs, [1])
        s1 = fr.stats()
        assert got == want
        assert fr.delta_stats()[:3] == [0, 2, 0]
        # the Typed call of the pre-XORed buffer copies the arena and then both frames' raw bytes back; the delta call the arena only
        assert (s0[2] - t0[2]) - (s1[2] - s0[2]) == n
    finally:
        fr.close()


def test_refusals_before_anything_is_queued(deltamock, zstd):
    plug, F = deltamock
    datas = [D.typed_corpus("bf16", 2 * CHUNK + 5, 1), D.typed_corpus("fp32", 1000, 2)]
    bases = [D.typed_corpus("bf16", 2 * CHUNK + 5, 3), D.typed_corpus("fp32", 1000, 4)]
    sizes = [len(d) for d in datas]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [3, 0], slot=0)
        bas = T.Pool(plug, bases, [1, 2], slot=1)
        other = T.Pool(plug, bases, [0, 0], slot=2, dev=1)
        host = C.create_string_buffer(sizes[1])
        frames = fr.compress_device_batch_delta(src.bufs, bas.bufs, [2, 4])
        out = R.OutPool(plug, sizes, [3, 0], slot=3)
        before = launches(plug), fr.stats(), fr.delta_stats(), fr.restore_stats()
        bad_bases = {
            "shorter": [bas.bufs[0], (bas.bufs[1][0], sizes[1] - 1)],
            "longer": [(bas.bufs[0][0], sizes[0] + 1), bas.bufs[1]],
            "null with a size": [bas.bufs[0], (0, sizes[1])],
            "a size of 0 for a buffer that has bytes": [bas.bufs[0], (bas.bufs[1][0], 0)],
            "host memory": [bas.bufs[0], (C.addressof(host), sizes[1])],
            "another device": [bas.bufs[0], other.bufs[1]],
            "ends behind the device memory": [bas.bufs[0], (bas.bufs[1][0] + (1 << 30), sizes[1])],
        }
        for name, bb in bad_bases.items():
            assert fr.compress_device_batch_delta_raw(src.bufs, bb, [2, 4])[0] == D.ERROR, name
            assert fr.restore_batch_delta_raw(frames, out.bufs, bb, [2, 4]) == D.ERROR, name
        # what the Typed calls refuse
        assert fr.compress_device_batch_delta_raw(src.bufs, bas.bufs, [2, 3])[0] == D.ERROR
        assert fr.restore_batch_delta_raw(frames, out.bufs, bas.bufs, [2, 3]) == D.ERROR
        assert fr.compress_device_batch_delta_raw([src.bufs[0], (0, sizes[1])], bas.bufs, [2, 4])[0] == D.ERROR
        assert fr.restore_batch_delta_raw(frames, out.bufs, bas.bufs, [2, 4], n_frames=3) == D.ERROR
        assert F.QZSTD_frontCompressDeviceBatchDelta(None, None, None, None, 0, None, None, 0, None, None) == D.ERROR
        assert F.QZSTD_frontRestoreDeviceBatchDelta(None, None, 0, None, 0, None, None, None, 0, None) == D.ERROR
        assert (launches(plug), fr.stats(), fr.delta_stats(), fr.restore_stats()) == before and out.untouched()
        # nothing to do: no GPU touched
        assert fr.compress_device_batch_delta_raw([(0, 0)], [(0, 0)], [2])[0] == 0
        assert fr.restore_batch_delta_raw([[]], [(0, 0)], [(0, 0)], [2]) == 0
        assert launches(plug) == before[0]
        assert fr.restore_batch_delta(frames, out.bufs, bas.bufs, [2, 4]) == 4 and out.bytes() == out.expected(datas)
    finally:
        fr.close()


def test_byte_xor(deltamock):
    plug, F = deltamock
    a, b = os.urandom(1000), os.urandom(1000)
    dst = C.create_string_buffer(1000)
    F.QZSTD_byteXor(dst, a, b, 1000)
    assert dst.raw == xor(a, b)
    buf = C.create_string_buffer(a, 1000)
    F.QZSTD_byteXor(buf, buf, b, 1000)  # dst may be a
    assert buf.raw == xor(a, b)
    F.QZSTD_byteXor(None, None, None, 0)


def test_device_layer_without_the_xor_entry_points(zstd, oracle):
    """the front-end linked against a mock WITHOUT the two XOR stand-ins: both delta calls return (size_t)-1 with a base given, with no launch,
    no event wait and nothing counted; without a base they are the Typed calls, which work as before (a process of its own: one set of mock
    libraries each)"""
    build_pair(zstd.path, NOXOR_MOCK_SO, NOXOR_FRONT_SO, xor=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
base = D.typed_corpus("bf16", 3 * chunk + 321, 2)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [base], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
frames = fr.compress_device_batch_typed(pool.bufs, [2])
out = R.OutPool(plug, [len(data)], [3], slot=2)
before = plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_launches(), plug.lib.qzstd_mock_ungroup_launches()
r1 = fr.compress_device_batch_delta_raw(pool.bufs, bas.bufs, [2])[0]
r2 = fr.restore_batch_delta_raw(frames, out.bufs, bas.bufs, [2])
same = (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_launches(), plug.lib.qzstd_mock_ungroup_launches()) == before
nothing = same and out.untouched() and fr.delta_stats() == [0, 0, 0, 0] and fr.restore_stats() == [0, 0, 0, 0]
typed_ok = fr.compress_device_batch_delta(pool.bufs, None, [2]) == frames and fr.restore_batch_delta(frames, out.bufs, None, [2]) == len(frames[0])
print(json.dumps({"refused": [r1, r2] == [D.ERROR] * 2, "nothing_queued": nothing, "typed": typed_ok and out.bytes() == out.expected([data]),
                  "has_xor": hasattr(plug.lib, "qzstd_hip_group_xor") or hasattr(plug.lib, "qzstd_hip_ungroup_xor")}))
""", NOXOR_MOCK_SO, NOXOR_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "typed": True, "has_xor": False}, res
