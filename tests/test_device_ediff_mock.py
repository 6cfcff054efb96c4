"""CPU: element differences in the device calls (QZSTD_ELEM_DIFF in an elemSizes entry, QZSTD_frontElemDiffStats:
include/qzstd_frontend_device.h) over the mock device layer — the mock pair of tests/test_device_fingerprint_mock.py plus
tests/mock/mock_hip_group_ediff.c and tests/mock/mock_hip_esum.c (the launchers' checks and include/qzstd_elemdiff.h's functions in plain C).
The skip test's sizes (0, 256, 65791, 65792, 128 KiB + 255, 2 - 3 chunks with odd tails), some buffers flagged at every element size: every
flagged frame, decoded by libzstd and taken through QZSTD_byteUngroup and QZSTD_elemSum, is the buffer's chunk; unflagged buffers' frames are
byte for byte those of the same call without flags; the restore is exact into misaligned destinations; levels 1 / 6 / 12 with checksum and
plane probe on; a failed block yields a frame of the same content; every refusal returns (size_t)-1 with nothing queued; the counters add
up; a device layer without the two entry points refuses flagged calls and serves all others.  Every comparison is byte-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import qz_device as D
import test_device_checksum_mock as T
import test_device_restore_mock as R
import test_device_skip_mock as SK
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_ediffmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_ediffmock.so")
OLD_MOCK_SO = os.path.join(MOCK, "libqatseqprod_noediffmock.so")
OLD_FRONT_SO = os.path.join(MOCK, "libqzstdfront_noediffmock.so")
CHUNK = SK.CHUNK
SIZES = SK.SIZES
assert {0, 256, 65791, 65792, CHUNK + 255, 2 * CHUNK + 1, 3 * CHUNK + 9} <= set(SIZES)
ELEMS = (2, 1, 4, 1, 8, 2, 4, 2, 1, 8)
DIFF = (True, True, True, False, True, False, False, True, False, True)  # element sizes 2, 1, 4, 8, 2 (empty), 8 flagged
FLAGS = tuple(k | (D.ELEM_DIFF if d else 0) for k, d in zip(ELEMS, DIFF))
PART = 2 * CHUNK


def build_pair(zstd_path, mock_so, front_so, ediff: bool):
    """the fingerprint test's mock pair, with the two stand-ins or — an older device layer — without"""
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
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c", "mock_hip_plane_cost.c")]
    if ediff:
        srcs += [os.path.join(MOCK, "mock_hip_group_ediff.c"), os.path.join(MOCK, "mock_hip_esum.c"),
                 os.path.join(B.PKG_DIR, "frontend", "qzstd_elemdiff.c")]
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def load(zstd_path, mock_so, front_so, ediff):
    build_pair(zstd_path, mock_so, front_so, ediff)
    plug, F = T.load_pair(mock_so, front_so)
    D.bind(F)
    D.bind_elemdiff(F)
    S.bind_hooks(plug)
    plug.lib.qzstd_mock_fail_block.argtypes = [C.c_int]
    if ediff:
        for n in ("qzstd_mock_group_ediff_rows", "qzstd_mock_esum_rows", "qzstd_mock_esum_tiles"):
            getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def mock(oracle, zstd):
    return load(zstd.path, MOCK_SO, FRONT_SO, True)


def column(n, k, seed):
    """n bytes of an integer column of k-byte elements with order: steps U(5, 40) from a start near the top of k bytes' range (it wraps)"""
    rng = np.random.default_rng(seed)
    m = n // k
    top = (1 << (8 * k)) - 1
    with np.errstate(over="ignore"):
        x = np.cumsum(rng.integers(5, 41, m, dtype=np.uint64)) + np.uint64(top - 100)
    return (x & np.uint64(top)).astype("<u%d" % k).tobytes() + bytes(rng.integers(0, 256, n - m * k, dtype=np.uint8))


@pytest.fixture(scope="module")
def batch():
    """the buffers' bytes, computed once and never changed: columns where flagged, the skip test's typed corpus elsewhere"""
    base, _ = SK.corpus(SK.BUFS, SK.KINDS, CHUNK)
    return [column(n, k, 40 + i) if d else base[i] for i, (n, k, d) in enumerate(zip(SIZES, ELEMS, DIFF))]


def chunks(d):
    return [d[o:o + CHUNK] for o in range(0, len(d), CHUNK)]


def mem(buf):
    return C.string_at(buf[0], buf[1])


def launches(plug):
    L = plug.lib
    return dict(find=L.qzstd_mock_launches(), ediff=L.qzstd_mock_group_ediff_launches(), rows=L.qzstd_mock_group_ediff_rows(),
                esum=L.qzstd_mock_esum_launches(), srows=L.qzstd_mock_esum_rows(), compact=L.qzstd_mock_compact_launches())


def check_content(zstd, F, frames, datas, flags):
    for i, (fr, d, e) in enumerate(zip(frames, datas, flags)):
        assert len(fr) == len(chunks(d)), i
        for c, (f, ch) in enumerate(zip(fr, chunks(d))):
            got = D.ungroup_bytes(zstd.decompress(f, len(ch)), e & 0x7F, lib=F)
            if e & D.ELEM_DIFF:
                got = D.elem_sum(got, e & 0x7F, lib=F)
            assert got == ch, (i, c)


N_FLAGGED = sum(len(chunks(bytes(n))) for n, d in zip(SIZES, DIFF) if d)
N_FRAMES = sum(len(chunks(bytes(n))) for n in SIZES)


@pytest.mark.parametrize("level", (1, 6, 12))
def test_round_trip_with_checksum_and_plane_probe(mock, batch, zstd, monkeypatch, level):
    plug, F = mock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(3, level, CHUNK, lib=F)
    try:
        assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0
        src = T.Pool(plug, batch, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(batch))], slot=0)
        plain = fr.compress_device_batch_typed(src.bufs, ELEMS)
        assert fr.elem_diff_stats() == [0, 0, 0, 0]
        before = launches(plug)
        frames = fr.compress_device_batch_typed(src.bufs, FLAGS)
        after = launches(plug)
        assert all(T.flagged(f) for x in frames for f in x)
        check_content(zstd, F, frames, batch, FLAGS)
        # unflagged buffers: byte for byte the frames of the call without flags, whatever their neighbours are
        for i, d in enumerate(DIFF):
            if not d:
                assert frames[i] == plain[i], i
            elif SIZES[i] > 64:
                assert frames[i] != plain[i], i
        # every flagged frame was differenced by the stand-in, no unflagged one; as many matcher launches as without flags
        assert after["rows"] - before["rows"] == N_FLAGGED and 1 <= after["ediff"] - before["ediff"] <= after["find"] - before["find"]
        st = fr.elem_diff_stats()
        assert st[0] == N_FLAGGED and st[1] == 0 and st[2:] == [0, 0]
        # ordered columns shrink against plain grouping
        for i, d in enumerate(DIFF):
            if d and SIZES[i] >= 65536:
                assert sum(map(len, frames[i])) < sum(map(len, plain[i])), i
        # the way back, into misaligned destinations; the Delta call without any base is the Typed call
        out = R.OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11)[i] for i in range(len(SIZES))], slot=3)
        assert fr.restore_batch(frames, out.bufs, FLAGS) == N_FRAMES
        assert [mem(b) for b in out.bufs] == list(batch)
        mid = launches(plug)
        assert mid["srows"] - after["srows"] == N_FLAGGED
        st = fr.elem_diff_stats()
        assert st[2] == N_FLAGGED and st[3] == mid["esum"] - after["esum"] >= 2
        out2 = R.OutPool(plug, SIZES, [(5, 9, 2)[i % 3] for i in range(len(SIZES))], slot=4)
        assert fr.restore_batch_delta(frames, out2.bufs, [None] * len(SIZES), FLAGS) == N_FRAMES
        assert [mem(b) for b in out2.bufs] == list(batch)
        kept = fr.fingerprint(src.bufs)
        assert fr.check(out.bufs, kept) == [] and fr.check(out2.bufs, kept) == []
        # the wrong setting on the way back is what the fingerprints catch
        wrong = list(FLAGS)
        wrong[0] = ELEMS[0]
        assert fr.restore_batch(frames, out.bufs, wrong) == N_FRAMES
        assert {i for i, _ in fr.check(out.bufs, kept)} == {0}
        assert all(mem(b) == d for b, d in zip(src.bufs, batch))  # the sources were only read
    finally:
        fr.close()


def test_a_failed_block_yields_a_frame_of_the_same_content(mock, batch, zstd, monkeypatch):
    plug, F = mock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(batch))], slot=0)
        plug.lib.qzstd_mock_fail_block(0)
        try:
            frames = fr.compress_device_batch_typed(src.bufs, FLAGS)
        finally:
            plug.lib.qzstd_mock_fail_block(-1)
        check_content(zstd, F, frames, batch, FLAGS)
        st = fr.elem_diff_stats()
        assert st[0] == N_FLAGGED and 1 <= st[1] <= N_FLAGGED  # block 0 of every part: some of those frames are flagged ones
        out = R.OutPool(plug, SIZES, [7] * len(SIZES), slot=3)
        assert fr.restore_batch(frames, out.bufs, FLAGS) == N_FRAMES and [mem(b) for b in out.bufs] == list(batch)
    finally:
        fr.close()


def test_refusals_queue_nothing(mock, batch):
    plug, F = mock
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, [2] * len(batch), slot=0)
        bas = T.Pool(plug, batch, [6] * len(batch), slot=1)
        frames = fr.compress_device_batch_typed(src.bufs, FLAGS)
        out = R.OutPool(plug, SIZES, [4] * len(SIZES), slot=3)
        before, st = launches(plug), (fr.elem_diff_stats(), fr.stats(), fr.restore_stats(), fr.verify_stats(), fr.slice_stats())
        for bad in (0x80, 0x83, 0x90, 0xC2, 0xFF):  # 0x80 alone: "the front's setting, with differences"
            es = list(FLAGS)
            es[5] = bad
            assert fr.compress_device_batch_typed_raw(src.bufs, es)[0] == D.ERROR, bad
            assert fr.restore_batch_raw(frames, out.bufs, es) == D.ERROR, bad
        # a flagged buffer with a base, in either direction (buffer 0 is flagged, buffer 3 is not)
        based = [None] * len(SIZES)
        based[0] = bas.bufs[0]
        assert fr.compress_device_batch_delta_raw(src.bufs, based, FLAGS)[0] == D.ERROR
        assert fr.restore_batch_delta_raw(frames, out.bufs, based, FLAGS) == D.ERROR
        # a flagged buffer in the verify call
        assert fr.verify_raw(frames, src.bufs, None, FLAGS)[0] == D.ERROR
        # a non-empty slice that touches a flagged buffer; an empty one does not count
        dst = out.bufs[0][0]
        assert fr.restore_slices_raw(frames, SIZES, FLAGS, [(0, 16, 100, dst, None)]) == D.ERROR
        assert fr.restore_slices_raw(frames, SIZES, FLAGS, [(0, 16, 0, dst, None), (9, 8, 64, dst, None)]) == D.ERROR
        assert launches(plug) == before
        assert (fr.elem_diff_stats(), fr.stats(), fr.restore_stats(), fr.verify_stats(), fr.slice_stats()) == st
        # ...while slices of the unflagged buffers of the same checkpoint are served
        assert fr.restore_slices_raw(frames, SIZES, FLAGS, [(0, 16, 0, dst, None), (3, 5, 1000, out.bufs[3][0], None)]) == 1
        assert C.string_at(out.bufs[3][0], 1000) == batch[3][5:1005]
        # ...and the same calls with a base on an unflagged buffer are accepted
        based = [None] * len(SIZES)
        based[3] = bas.bufs[3]
        fd = fr.compress_device_batch_delta(src.bufs, based, FLAGS)
        assert fr.restore_batch_delta(fd, out.bufs, based, FLAGS) == N_FRAMES and [mem(b) for b in out.bufs] == list(batch)
    finally:
        fr.close()


def test_a_call_without_flags_is_what_it_was(mock, batch):
    plug, F = mock
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, [1] * len(batch), slot=0)
        out = R.OutPool(plug, SIZES, [9] * len(SIZES), slot=3)
        before = launches(plug)
        frames = fr.compress_device_batch_typed(src.bufs, ELEMS)
        assert fr.restore_batch(frames, out.bufs, ELEMS) == N_FRAMES
        after = launches(plug)
        assert (after["ediff"], after["esum"]) == (before["ediff"], before["esum"]) and fr.elem_diff_stats() == [0, 0, 0, 0]
    finally:
        fr.close()


def test_device_layer_without_the_two_entry_points(zstd, oracle, batch):
    plug, F = load(zstd.path, OLD_MOCK_SO, OLD_FRONT_SO, False)
    assert not hasattr(plug.lib, "qzstd_hip_group_ediff") and not hasattr(plug.lib, "qzstd_hip_esum")
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, [3] * len(batch), slot=0)
        out = R.OutPool(plug, SIZES, [1] * len(SIZES), slot=3)
        find = plug.lib.qzstd_mock_launches()
        assert fr.compress_device_batch_typed_raw(src.bufs, FLAGS)[0] == D.ERROR
        assert plug.lib.qzstd_mock_launches() == find
        frames = fr.compress_device_batch_typed(src.bufs, ELEMS)
        st = fr.restore_stats()
        assert fr.restore_batch_raw(frames, out.bufs, FLAGS) == D.ERROR and fr.restore_stats() == st
        assert fr.restore_batch(frames, out.bufs, ELEMS) == N_FRAMES and [mem(b) for b in out.bufs] == list(batch)
        assert fr.verify(frames, src.bufs, None, ELEMS) == []
        assert fr.elem_diff_stats() == [0, 0, 0, 0]
    finally:
        fr.close()
