"""CPU: the fingerprint calls (QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch / QZSTD_frontFingerprintStats:
include/qzstd_frontend_device.h) over the mock device layer — the mock pair of tests/test_device_verify_mock.py (the skip test's, with the
ungrouping comparison) plus tests/mock/mock_hip_fingerprint.c (the launcher's checks and include/qzstd_fingerprint.h's QZSTD_fpTile in plain
C).  The skip test's batch (sizes 0, 256, 65791, 65792, 128 KiB + 255, 2 - 3 chunks with odd tails; element sizes 1 / 2 / 4; buffers with a
base and without): fp[c] is QZSTD_fingerprintOf of chunk c's bytes and the restatement's (tools/qz_device.py: fingerprint_ref), firstFrame
is right; after delta compress -> delta restore the check says 0; after a restore with ANOTHER base it counts exactly the frames whose base
chunks differ; after a restore with the wrong element size exactly the frames the swap does not leave byte-identical (worked out from the
bytes); a device layer without the entry point refuses the two calls and serves compress, restore and verify as before; the counters add
up.  Every comparison is exact."""
import ctypes as C
import os

import pytest

import qz_device as D
import test_device_checksum_mock as T
import test_device_restore_mock as R
import test_device_skip_mock as SK
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_fpmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_fpmock.so")
NOFP_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nofpmock.so")
NOFP_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nofpmock.so")
CHUNK = SK.CHUNK
BUFS, KINDS, SIZES, ELEMS, BASED = SK.BUFS, SK.KINDS, SK.SIZES, SK.ELEMS, SK.BASED
assert {0, 256, 65791, CHUNK + 255, 2 * CHUNK + 1, 3 * CHUNK + 9} <= set(SIZES)


def build_pair(zstd_path, mock_so, front_so, fingerprint: bool):
    """the verify test's mock pair, with the fingerprint's stand-in or — an older device layer — without"""
    import subprocess

    import qz_bind as B
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c")]
    if fingerprint:
        srcs.append(os.path.join(MOCK, "mock_hip_fingerprint.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def load(zstd_path):
    """the pair with the stand-in, built and loaded (tests/test_fingerprint_host.py takes the front-end's export from here too)"""
    build_pair(zstd_path, MOCK_SO, FRONT_SO, fingerprint=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    for n in ("qzstd_mock_fingerprint_rows", "qzstd_mock_fingerprint_tiles"):
        getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def fpmock(oracle, zstd):
    return load(zstd.path)


@pytest.fixture(scope="module")
def batch():
    """(the buffers' bytes, their bases' bytes), computed once and never changed"""
    return SK.corpus(BUFS, KINDS, CHUNK)


def chunks(d):
    return [d[o:o + CHUNK] for o in range(0, len(d), CHUNK)]


def mem(buf):
    return C.string_at(buf[0], buf[1])


def test_fingerprints_are_the_functions_and_the_restatements(fpmock, batch):
    plug, F = fpmock
    datas, _ = batch
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))], slot=0)
        before = (plug.lib.qzstd_mock_fingerprint_launches(), plug.lib.qzstd_mock_fingerprint_rows(), plug.lib.qzstd_mock_fingerprint_tiles())
        assert fr.fingerprint_stats() == [0, 0, 0, 0]
        r, fp, first = fr.fingerprint_raw(src.bufs)
        n_frames = sum(len(chunks(d)) for d in datas)
        assert r == n_frames == len(fp)
        want_first, c = [], 0
        for d in datas:
            want_first.append(c)
            c += len(chunks(d))
        assert first == want_first + [n_frames]
        flat = [ch for d in datas for ch in chunks(d)]
        assert fp == [D.fingerprint_of(ch, lib=F) for ch in flat]
        assert fp == [D.fingerprint_ref(ch) for ch in flat]
        assert len(set(fp)) == len({bytes(ch) for ch in flat})  # chunks of other bytes or another length: another value
        # one launch, a row per frame, a tile per 16 KiB; the buffers only read
        tiles = sum(D.fp_tiles(len(ch)) for ch in flat)
        after = (plug.lib.qzstd_mock_fingerprint_launches(), plug.lib.qzstd_mock_fingerprint_rows(), plug.lib.qzstd_mock_fingerprint_tiles())
        assert [a - b for a, b in zip(after, before)] == [1, n_frames, tiles]
        assert fr.fingerprint_stats() == [n_frames, sum(SIZES), 1, 0]
        assert all(mem(b) == d for b, d in zip(src.bufs, datas))
        assert fr.fingerprint(src.bufs) == [[D.fingerprint_of(ch, lib=F) for ch in chunks(d)] for d in datas]
        # the value does not depend on where the bytes lie, nor on any setting of the front
        moved = T.Pool(plug, datas, [(9, 0, 2, 7)[i % 4] for i in range(len(datas))], slot=1)
        assert fr.set_byte_group(4) == 0 and fr.set_checksum(1) == 0 and fr.set_delta_skip(1) == 0 and fr.set_plane_probe(1) == 0
        assert fr.check(moved.bufs, fr.fingerprint(src.bufs)) == []
        assert fr.fingerprint_stats() == [4 * n_frames, 4 * sum(SIZES), 4, 0]
    finally:
        fr.close()


def test_compress_restore_check_wrong_base_and_wrong_element_size(fpmock, batch, zstd):
    plug, F = fpmock
    datas, bases = batch
    n_frames = sum(len(chunks(d)) for d in datas)
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))], slot=0)
        bas = T.Pool(plug, bases, [(7, 0, 2, 9, 15, 4)[i % 6] for i in range(len(datas))], slot=1)
        given = [b if on else None for b, on in zip(bas.bufs, BASED)]
        kept = fr.fingerprint(src.bufs)  # what the caller keeps with the frames: 8 bytes per frame
        frames = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        # ---- the right base, the right element sizes: into fresh buffers and in place over a copy of the bases
        out = R.OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11)[i] for i in range(len(SIZES))], slot=3)
        assert fr.restore_batch_delta(frames, out.bufs, given, ELEMS) == n_frames
        assert fr.check(out.bufs, kept) == [] and [mem(b) for b in out.bufs] == list(datas)
        inp = T.Pool(plug, [b if on else bytes(len(b)) for b, on in zip(bases, BASED)], [2] * len(datas), slot=4)
        assert fr.restore_batch_delta(frames, inp.bufs, [b if on else None for b, on in zip(inp.bufs, BASED)], ELEMS) == n_frames
        assert fr.check(inp.bufs, kept) == []
        st0 = fr.fingerprint_stats()
        assert st0[3] == 0
        # ---- ANOTHER base for buffer 9 (its own new bytes, as if the previous checkpoint were this one): exactly the frames whose base
        # chunks differ, which is what BUFS says of it
        other = list(given)
        other[9] = src.bufs[9]
        out2 = R.OutPool(plug, SIZES, [5] * len(SIZES), slot=3)
        assert fr.restore_batch_delta(frames, out2.bufs, other, ELEMS) == n_frames
        want = [(9, c) for c, (a, b) in enumerate(zip(chunks(bases[9]), chunks(datas[9]))) if a != b]
        assert want == [(9, c) for c in sorted(BUFS[9][3])] and want
        assert [(9, c) for c, (a, b) in enumerate(zip(chunks(mem(out2.bufs[9])), chunks(datas[9]))) if a != b] == want
        r, flags = fr.check_raw(out2.bufs, [v for fp in kept for v in fp])
        first9 = sum(len(k) for k in kept[:9])
        assert r == len(want) and [c for c, x in enumerate(flags) if x] == [first9 + c for _, c in want] and set(flags) <= {0, 1}
        assert fr.check(out2.bufs, kept) == want
        # ---- the wrong element size for two buffers: every frame the swap does not leave byte-identical, from the bytes
        elems = list(ELEMS)
        elems[9], elems[8] = 4, 2
        assert (ELEMS[9], ELEMS[8]) == (2, 1)
        out3 = R.OutPool(plug, SIZES, [9] * len(SIZES), slot=3)
        assert fr.restore_batch_delta(frames, out3.bufs, given, elems) == n_frames
        want = []
        for i in (8, 9):
            for c, (d, b) in enumerate(zip(chunks(datas[i]), chunks(bases[i]))):
                delta = bytes(x ^ y for x, y in zip(d, b)) if BASED[i] else d
                back = D.ungroup_bytes(D.group_bytes(delta, ELEMS[i], lib=F), elems[i], lib=F)
                back = bytes(x ^ y for x, y in zip(back, b)) if BASED[i] else back
                assert back == chunks(mem(out3.bufs[i]))[c]  # (the expectation is what the restore left)
                if back != d:
                    want.append((i, c))
        assert fr.check(out3.bufs, kept) == want
        assert {i for i, _ in want} == {8, 9} and (9, 0) not in want  # (buffer 9's frame 0 equals its base: a delta of zeros groups to itself)
        st1 = fr.fingerprint_stats()
        assert st1[3] - st0[3] == 2 * len([(9, c) for c in BUFS[9][3]]) + len(want)
        assert st1[2] - st0[2] == 3 and st1[0] - st0[0] == 3 * n_frames and st1[1] - st0[1] == 3 * sum(SIZES)
        # the sources were only read
        assert all(mem(b) == d for b, d in zip(src.bufs, datas)) and all(mem(b) == d for b, d in zip(bas.bufs, bases))
    finally:
        fr.close()


def test_refusals(fpmock, batch):
    plug, F = fpmock
    datas, _ = batch
    fr = D.DeviceFront(2, 1, CHUNK, use_producer=0, lib=F)  # (accepted without the producer, like the restore)
    try:
        src = T.Pool(plug, datas, [4] * len(datas), slot=0)
        kept = fr.fingerprint(src.bufs)
        flat = [v for fp in kept for v in fp]
        state = lambda: (plug.lib.qzstd_mock_fingerprint_launches(), plug.lib.qzstd_mock_event_waits(), fr.fingerprint_stats())  # noqa: E731
        before = state()
        assert fr.fingerprint_raw(src.bufs, null_fp=True)[0] == D.ERROR
        assert fr.check_raw(src.bufs, None, n_frames=len(flat))[0] == D.ERROR
        r, flags = fr.check_raw(src.bufs, flat[:-1])
        assert r == D.ERROR and set(flags) == {7}
        assert fr.check_raw(src.bufs, flat + [0])[0] == D.ERROR
        assert fr.fingerprint_raw(src.bufs[:3] + [(0, 5)])[0] == D.ERROR                       # a null pointer with a size
        host = C.create_string_buffer(4096)
        assert fr.fingerprint_raw(src.bufs[:3] + [(C.addressof(host), 4096)])[0] == D.ERROR   # host memory
        assert F.QZSTD_frontFingerprintDeviceBatch(None, None, 0, None, None, None) == D.ERROR
        assert F.QZSTD_frontCheckDeviceBatch(None, None, 0, None, None, 0, None) == D.ERROR
        assert F.QZSTD_frontFingerprintDeviceBatch(fr.f, None, 2, None, None, None) == D.ERROR
        # no buffers, or only empty ones: 0
        assert fr.fingerprint_raw([])[0] == 0 and fr.fingerprint_raw([(0, 0), (src.bufs[1][0], 0)], null_fp=True)[0] == 0
        assert fr.check_raw([(0, 0)], [], want_flags=False)[0] == 0
        assert state() == before
        st = (C.c_ulonglong * 4)(9, 9, 9, 9)
        F.QZSTD_frontFingerprintStats(None, st)
        assert list(st) == [0, 0, 0, 0]
        F.QZSTD_frontFingerprintStats(None, None)
        assert fr.check(src.bufs, kept) == []
    finally:
        fr.close()
    # the launcher's own refusals, before anything is touched
    L = D.bind_fingerprint_kernel(plug.lib)
    a = C.create_string_buffer(40000)
    rows, d_rows = (D.FpRow * 2)(), (D.FpRow * 2)()
    tiles = (C.c_uint64 * 6)(*([7] * 6))
    rows[0].src, rows[0].len, rows[0].tile0 = C.addressof(a) + 3, 20000, 99
    rows[1].src, rows[1].len, rows[1].tile0 = 0, 0, 99
    assert L.qzstd_hip_fingerprint(0, None, None, 2, d_rows, tiles) < 0 and L.qzstd_hip_fingerprint(0, None, rows, 2, None, tiles) < 0
    assert L.qzstd_hip_fingerprint(0, None, rows, 2, d_rows, None) < 0
    rows[1].len = 1
    assert L.qzstd_hip_fingerprint(0, None, rows, 2, d_rows, tiles) < 0
    rows[1].src, rows[1].len = C.addressof(a), 0xFFFFFFE1
    assert L.qzstd_hip_fingerprint(0, None, rows, 2, d_rows, tiles) < 0
    assert [r.tile0 for r in rows] == [99, 99] and list(tiles) == [7] * 6
    assert L.qzstd_hip_fingerprint(0, None, rows, 0, d_rows, tiles) == 0 and list(tiles) == [7] * 6
    rows[1].src, rows[1].len = C.addressof(a) + 30000, 5
    assert L.qzstd_hip_fingerprint(0, None, rows, 2, d_rows, tiles) == 0
    assert [r.tile0 for r in rows] == [0, 2] and list(tiles)[3:] == [7, 7, 7]
    assert list(tiles)[:3] == [D.fp_tile_ref(a.raw[3:3 + 16384]), D.fp_tile_ref(a.raw[3 + 16384:20003]), D.fp_tile_ref(a.raw[30000:30005])]


def test_device_layer_without_the_fingerprint_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the fingerprint's stand-in: the two calls return (size_t)-1 with no event wait and
    nothing counted; compress, restore and verify are served as before (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOFP_MOCK_SO, NOFP_FRONT_SO, fingerprint=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
base = D.typed_corpus("bf16", 3 * chunk + 321, 2)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [base], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), fr.stats(), fr.fingerprint_stats())
before = state()
r1 = fr.fingerprint_raw(pool.bufs)[0]
r2 = fr.check_raw(pool.bufs, [1, 2, 3, 4])[0]
nothing = state() == before
frames = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2])
out = R.OutPool(plug, [len(data)], [3], slot=2)
back = fr.restore_batch_delta(frames, out.bufs, bas.bufs, [2]) == len(frames[0]) and out.bytes() == out.expected([data])
verified = fr.verify(frames, pool.bufs, bas.bufs, [2]) == []
print(json.dumps({"refused": [r1 == D.ERROR, r2 == D.ERROR], "nothing_queued": nothing, "restore": back, "verify": verified,
                  "has_kernel": hasattr(plug.lib, "qzstd_hip_fingerprint"), "has_calls": hasattr(F, "QZSTD_frontCheckDeviceBatch")}))
""", NOFP_MOCK_SO, NOFP_FRONT_SO)
    assert res == {"refused": [True, True], "nothing_queued": True, "restore": True, "verify": True, "has_kernel": False, "has_calls": True}, res
