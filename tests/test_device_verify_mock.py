"""CPU: QZSTD_frontVerifyDeviceBatch / QZSTD_frontVerifyStats (include/qzstd_frontend_device.h) over the mock device layer — the mock pair of
tests/test_device_skip_mock.py plus tests/mock/mock_hip_ungroup_cmp.c (the ungrouping comparison in plain C).  The mixed batch of that file
(sizes 0, 256, 65791, 65792, 128 KiB + 255, 2 - 3 chunks with odd tails; element sizes 1 / 2 / 4; buffers with a base and without) and two
buffers of one size whose bases can be swapped, three frames per part so that both slots are used again.  What the call must say is worked
out on the host for every frame — decode, QZSTD_byteUngroup with the element size GIVEN, XOR with the base GIVEN, compare with the live
bytes — and compared exactly: after a compress; with one bit of a live buffer or of a base changed; with a wrong element size and swapped
bases; with a corrupt frame; for frames libzstd built; with delta skip on (zero frames are not decoded, a frozen buffer changed after the
save is caught, an all-frozen call still compares); against a device layer without the entry point; and the counters add up."""
import ctypes as C
import os

import numpy as np
import pytest

import qz_device as D
import test_device_checksum_mock as T
import test_device_skip_mock as SK
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_verifymock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_verifymock.so")
NOCMP_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nocmpmock.so")
NOCMP_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nocmpmock.so")
CHUNK = SK.CHUNK
PART = 3 * CHUNK  # three frames per part
TWIN = 70000      # two buffers of one size: their bases can be swapped
BUFS = SK.BUFS + ((TWIN, 2, True, "all"), (TWIN, 2, True, "all"))
KINDS = SK.KINDS + ("bf16", "bf16")
SIZES = tuple(b[0] for b in BUFS)
ELEMS = tuple(b[1] for b in BUFS)
BASED = tuple(b[2] for b in BUFS)
SAME, UNDECODED = D.VERIFY_SAME, D.VERIFY_UNDECODED


def build_pair(zstd_path, mock_so, front_so, cmp: bool):
    """the skip test's mock pair, with the ungrouping comparison's stand-in or — an older device layer — without"""
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
                                             "mock_hip_diff.c")]
    if cmp:
        srcs.append(os.path.join(MOCK, "mock_hip_ungroup_cmp.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def verifymock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, cmp=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    for n in ("qzstd_mock_diff_rows", "qzstd_mock_ungroup_cmp_rows", "qzstd_mock_ungroup_cmp_zero_rows", "qzstd_mock_ungroup_cmp_stage_bytes"):
        getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def batch():
    """(the buffers' bytes, their bases' bytes), computed once and never changed"""
    return SK.corpus(BUFS, KINDS, CHUNK)


def mem(buf):
    """the bytes of a pool's (address, size) as they are now"""
    return C.string_at(buf[0], buf[1])


def poke(buf, at, bit=1):
    C.c_ubyte.from_address(buf[0] + at).value ^= bit


def expected(zstd, F, frames, live, bases, elems):
    """firstDiff as the header defines it, on the host: per frame decode, ungroup with the element size given, XOR the base chunk given,
    and the lowest offset at which that differs from the live chunk (SAME: none)"""
    out = []
    for fr, lv, bs, k in zip(frames, live, bases, elems):
        for c, f in enumerate(fr):
            want = np.frombuffer(lv[c * CHUNK:(c + 1) * CHUNK], dtype=np.uint8)
            u = np.frombuffer(D.ungroup_bytes(zstd.decompress(f, CHUNK), k, lib=F), dtype=np.uint8)
            assert len(u) == len(want)
            if bs is not None:
                u = u ^ np.frombuffer(bs[c * CHUNK:(c + 1) * CHUNK], dtype=np.uint8)
            bad = np.flatnonzero(u != want)
            out.append(int(bad[0]) if len(bad) else SAME)
    return out


def plan(lens, zero, part=PART):
    """the call's parts as the header describes them: whole frames, at most `part` bytes of DECODED content; a recognised zero frame joins
    the part it falls into -> [(rows, decoded stage bytes)]"""
    parts, cur = [], None
    for n, z in zip(lens, zero):
        if cur is None or (not z and cur[2] + n > part):
            cur = [0, 0, 0]
            parts.append(cur)
        cur[0] += 1
        if not z:
            cur[1] += (n + 15) & ~15
            cur[2] += n
    return [(p[0], p[1]) for p in parts]


def counters(plug, fr):
    L = plug.lib
    return dict(cmp=L.qzstd_mock_ungroup_cmp_launches(), rows=L.qzstd_mock_ungroup_cmp_rows(), zero=L.qzstd_mock_ungroup_cmp_zero_rows(),
                stage=L.qzstd_mock_ungroup_cmp_stage_bytes(), unxor=L.qzstd_mock_ungroup_xor_launches(), un=L.qzstd_mock_ungroup_launches(),
                diff=L.qzstd_mock_diff_launches(), find=L.qzstd_mock_launches(), verify=fr.verify_stats(), restore=fr.restore_stats(),
                delta=fr.delta_stats(), skip=fr.delta_skip_stats(), dev=fr.stats(), group=fr.byte_group_stats(), slices=fr.slice_stats())


OTHERS = ("unxor", "un", "diff", "find", "restore", "delta", "skip", "dev", "group", "slices")


def lens_of(sizes=SIZES):
    return [min(CHUNK, n - o) for n in sizes for o in range(0, n, CHUNK)]


class Saved:
    """a front, the batch on the `device`, and the frames a delta compress call left for it"""

    def __init__(self, plug, F, batch, monkeypatch, skip=False, checksum=False, keep=None, threads=3):
        monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
        datas, bases = batch
        self.keep = list(range(len(BUFS))) if keep is None else keep
        self.datas, self.based = [datas[i] for i in self.keep], [BASED[i] for i in self.keep]
        self.base_bytes = [bases[i] if BASED[i] else None for i in self.keep]
        self.elems = [ELEMS[i] for i in self.keep]
        self.fr = D.DeviceFront(threads, 1, CHUNK, lib=F)
        assert self.fr.set_checksum(checksum) == 0 and self.fr.set_delta_skip(skip) == 0
        self.src = T.Pool(plug, self.datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(self.keep))], slot=0)
        self.bas = T.Pool(plug, [bases[i] for i in self.keep], [(7, 0, 2, 9, 15, 4)[i % 6] for i in range(len(self.keep))], slot=1)
        self.given = [b if on else None for b, on in zip(self.bas.bufs, self.based)]
        self.frames = self.fr.compress_device_batch_delta(self.src.bufs, self.given, self.elems)
        self.lens = lens_of([len(d) for d in self.datas])

    def live(self):
        return [mem(b) for b in self.src.bufs]

    def bases_now(self):
        return [mem(b) if on else None for b, on in zip(self.bas.bufs, self.based)]

    def close(self):
        self.fr.close()


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
def test_verify_after_compress_and_one_bit_changed(verifymock, zstd, batch, monkeypatch, checksum):
    plug, F = verifymock
    s = Saved(plug, F, batch, monkeypatch, checksum=checksum)
    try:
        n = len(s.lens)
        c0 = counters(plug, s.fr)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        c1 = counters(plug, s.fr)
        assert r == 0 and first == [SAME] * n
        parts = plan(s.lens, [False] * n)
        assert len(parts) > 4 and max(p[1] for p in parts) <= PART  # both slots are used again
        assert c1["verify"] == [n, 0, sum(SIZES), len(parts)]
        assert (c1["cmp"] - c0["cmp"], c1["rows"] - c0["rows"], c1["zero"] - c0["zero"], c1["stage"] - c0["stage"]) == \
            (len(parts), n, 0, sum(p[1] for p in parts))
        assert all(c1[k] == c0[k] for k in OTHERS)  # the other calls' counters do not move, and nothing of theirs is launched
        assert s.live() == s.datas and [mem(b) for b in s.bas.bufs] == list(batch[1])  # only read
        # compacted frames (frameStride 0) and no firstDiff
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems, compact=True, want_offsets=False) == (0, None)
        # ---- one bit of a live buffer: byte 0, the last byte of a 1-byte tail frame, offset 16384 of a frame
        poke(s.src.bufs[0], 0, 0x40)
        poke(s.src.bufs[0], 2 * CHUNK, 0x01)
        poke(s.src.bufs[6], CHUNK + 16384, 0x08)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        want = [SAME] * n
        want[0], want[2] = 0, 0
        f6 = sum(len(x) for x in s.frames[:6])
        want[f6 + 1] = 16384
        assert (r, first) == (3, want) and first == expected(zstd, F, s.frames, s.live(), s.bases_now(), s.elems)
        assert s.fr.verify(s.frames, s.src.bufs, s.given, s.elems) == [(0, 0, 0), (0, 2, 0), (6, 1, 16384)]
        assert s.fr.verify_stats()[1] == 6
        poke(s.src.bufs[0], 0, 0x40)
        poke(s.src.bufs[0], 2 * CHUNK, 0x01)
        poke(s.src.bufs[6], CHUNK + 16384, 0x08)
        # ---- the same for a bit of a base: byte 0 of a buffer, the 1-byte tail frame, offset 16385 of a frame, a frame's last byte
        poke(s.bas.bufs[0], 0, 0x02)
        poke(s.bas.bufs[0], 2 * CHUNK, 0x80)
        poke(s.bas.bufs[9], 2 * CHUNK + 16385, 0x10)
        poke(s.bas.bufs[1], CHUNK + 254, 0x04)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        want = [SAME] * n
        want[0], want[2], want[4] = 0, 0, 254
        want[sum(len(x) for x in s.frames[:9]) + 2] = 16385
        assert (r, first) == (4, want) and first == expected(zstd, F, s.frames, s.live(), s.bases_now(), s.elems)
        # a bit of a base that is not given changes nothing (buffers 5 and 8 have none)
        poke(s.bas.bufs[5], 77)
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)[0] == 4
    finally:
        s.close()


def test_wrong_element_size_swapped_bases_and_frames_out_of_order(verifymock, zstd, batch, monkeypatch):
    """the caller's bookkeeping gone wrong is reported as differences, frame by frame what the host works out, and never crashes"""
    plug, F = verifymock
    s = Saved(plug, F, batch, monkeypatch)
    try:
        elems = list(s.elems)
        elems[6] = 2  # written with 4
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, elems)
        want = expected(zstd, F, s.frames, s.live(), s.bases_now(), elems)
        f6 = sum(len(x) for x in s.frames[:6])
        assert first == want and r == 3 and all(x != SAME for x in want[f6:f6 + 3]) and want.count(SAME) == len(want) - 3
        given = list(s.given)
        given[10], given[11] = given[11], given[10]
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, given, s.elems)
        bases = s.bases_now()
        bases[10], bases[11] = bases[11], bases[10]
        want = expected(zstd, F, s.frames, s.live(), bases, s.elems)
        assert first == want and r == 2 and [x != SAME for x in want] == [False] * (len(want) - 2) + [True] * 2
        frames = list(s.frames)
        frames[10], frames[11] = frames[11], frames[10]
        r, first = s.fr.verify_raw(frames, s.src.bufs, s.given, s.elems)
        assert r == 2 and first == expected(zstd, F, frames, s.live(), s.bases_now(), s.elems)
        # a base forgotten, and a base given for a buffer that was written without one
        given = list(s.given)
        given[6] = None
        given[8] = s.bas.bufs[8]
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, given, s.elems)
        bases = s.bases_now()
        bases[6], bases[8] = None, mem(s.bas.bufs[8])
        assert r == 5 and first == expected(zstd, F, s.frames, s.live(), bases, s.elems)
        # bases == NULL: the Typed counterpart — the buffers written without a base verify, the others differ
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, None, s.elems)
        assert first == expected(zstd, F, s.frames, s.live(), [None] * len(BUFS), s.elems) and r == sum(x != SAME for x in first)
        f5 = sum(len(x) for x in s.frames[:5])
        assert first[f5:f5 + 4] == [SAME] * 4
    finally:
        s.close()


def test_a_corrupt_frame_with_checksums_on(verifymock, zstd, batch, monkeypatch):
    plug, F = verifymock
    s = Saved(plug, F, batch, monkeypatch, checksum=True)
    try:
        c = sum(len(x) for x in s.frames[:6]) + 1  # buffer 6, frame 1: a changed chunk, far from a zero frame
        frames = [list(x) for x in s.frames]
        f = bytearray(frames[6][1])
        f[len(f) // 2] ^= 0x20
        frames[6][1] = bytes(f)
        before = counters(plug, s.fr)
        r, first = s.fr.verify_raw(frames, s.src.bufs, s.given, s.elems)
        assert r == D.ERROR and first[c] == UNDECODED
        assert s.live() == s.datas
        assert all(counters(plug, s.fr)[k] == before[k] for k in OTHERS)
        # the front is free again, and the good frames verify
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)[0] == 0
        # a frame cut short, without firstDiff
        frames[6][1] = s.frames[6][1][:-5]
        assert s.fr.verify_raw(frames, s.src.bufs, s.given, s.elems, want_offsets=False) == (D.ERROR, None)
    finally:
        s.close()


def test_frames_libzstd_built(verifymock, zstd, batch, monkeypatch):
    """ZSTD_compress2 over QZSTD_byteGroup's output (of the XOR with the base, where there is one) verifies too; a front without the
    producer is accepted"""
    plug, F = verifymock
    datas, bases = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    frames = []
    for d, b, k, on in zip(datas, bases, ELEMS, BASED):
        x = (np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() if on else d
        frames.append(D.foreign_frames(zstd, x, CHUNK, k, checksum=True, lib=F))
    fr = D.DeviceFront(2, 1, CHUNK, lib=F, use_producer=0)
    try:
        src = T.Pool(plug, datas, [5] * len(datas), slot=0)
        bas = T.Pool(plug, bases, [11] * len(datas), slot=1)
        given = [b if on else None for b, on in zip(bas.bufs, BASED)]
        assert fr.verify(frames, src.bufs, given, ELEMS) == []
        poke(src.bufs[3], 65790, 0x80)
        assert fr.verify(frames, src.bufs, given, ELEMS) == [(3, 0, 65790)]
        assert fr.verify_stats()[:3] == [2 * len(lens_of()), 1, 2 * sum(SIZES)]
    finally:
        fr.close()


def test_delta_skip_zero_frames_are_compared_not_decoded(verifymock, zstd, batch, monkeypatch):
    plug, F = verifymock
    s = Saved(plug, F, batch, monkeypatch, skip=True)
    try:
        eq = [e for per in SK.equal_map(s.datas, [b or b"" for b in s.base_bytes], s.based, CHUNK) for e in per]
        n, n_equal = len(s.lens), sum(eq)
        assert n_equal == 10 and [f for per in s.frames for f in per][0] == D.zero_frame(CHUNK)
        c0 = counters(plug, s.fr)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        c1 = counters(plug, s.fr)
        assert r == 0 and first == [SAME] * n
        parts = plan(s.lens, eq)
        assert (c1["cmp"] - c0["cmp"], c1["rows"] - c0["rows"], c1["zero"] - c0["zero"], c1["stage"] - c0["stage"]) == \
            (len(parts), n, n_equal, sum((x + 15) & ~15 for x, e in zip(s.lens, eq) if not e))
        assert [c1["verify"][k] - c0["verify"][k] for k in range(4)] == [n, 0, sum(SIZES), len(parts)]  # the zero frames count as compared
        assert all(c1[k] == c0[k] for k in OTHERS)  # QZSTD_frontRestoreStats and QZSTD_frontDeltaSkipStats included
        # a frozen buffer modified after the save: caught at the right offset (buffer 0, frame 1; buffer 3's only frame; buffer 9's tail)
        poke(s.src.bufs[0], CHUNK + 12345, 0x20)
        poke(s.src.bufs[3], 65790, 0x01)
        poke(s.src.bufs[9], 3 * CHUNK + 8, 0x04)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        assert r == 3 and first == expected(zstd, F, s.frames, s.live(), s.bases_now(), s.elems)
        assert s.fr.verify(s.frames, s.src.bufs, s.given, s.elems) == [(0, 1, 12345), (3, 0, 65790), (9, 3, 8)]
        # the setting off: such a frame is decoded like any other, and the answer is the same
        assert s.fr.set_delta_skip(False) == 0
        c2 = counters(plug, s.fr)
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems) == (r, first)
        c3 = counters(plug, s.fr)
        assert c3["zero"] == c2["zero"] and c3["stage"] - c2["stage"] == sum((x + 15) & ~15 for x in s.lens)
        assert c3["cmp"] - c2["cmp"] == len(plan(s.lens, [False] * n))
    finally:
        s.close()


def test_delta_skip_an_all_frozen_call_still_compares(verifymock, zstd, batch, monkeypatch):
    plug, F = verifymock
    keep = [i for i, b in enumerate(SK.BUFS) if b[2] and b[3] == "none"]
    s = Saved(plug, F, batch, monkeypatch, skip=True, keep=keep)
    try:
        n = len(s.lens)
        assert [f for per in s.frames for f in per] == [D.zero_frame(x) for x in s.lens]
        c0 = counters(plug, s.fr)
        r, first = s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)
        c1 = counters(plug, s.fr)
        assert r == 0 and first == [SAME] * n
        assert (c1["cmp"] - c0["cmp"], c1["rows"] - c0["rows"], c1["zero"] - c0["zero"], c1["stage"] - c0["stage"]) == (1, n, n, 0)
        assert c1["verify"] == [n, 0, sum(s.lens), 1] and all(c1[k] == c0[k] for k in OTHERS)
        poke(s.src.bufs[0], 2 * CHUNK, 0x10)  # the 1-byte tail frame
        poke(s.bas.bufs[3], 40000, 0x01)  # (the fourth kept buffer: 65792 bytes)
        assert s.fr.verify(s.frames, s.src.bufs, s.given, s.elems) == [(0, 2, 0), (3, 0, 40000)]
        # a base that IS the live buffer: the frames' content is compared with zero, which it is
        assert s.fr.verify(s.frames, s.src.bufs, s.src.bufs, s.elems) == []
    finally:
        s.close()


def test_refusals_before_anything_is_queued(verifymock, zstd, batch, monkeypatch):
    plug, F = verifymock
    assert F.QZSTD_frontVerifyDeviceBatch(None, None, 0, None, 0, None, None, None, 0, None, None) == D.ERROR
    st = (C.c_ulonglong * 4)(9, 9, 9, 9)
    F.QZSTD_frontVerifyStats(None, st)
    assert list(st) == [0, 0, 0, 0]
    F.QZSTD_frontVerifyStats(None, None)
    s = Saved(plug, F, batch, monkeypatch)
    try:
        waits = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_ungroup_cmp_launches(), s.fr.verify_stats())  # noqa: E731
        before = waits()
        n = len(s.lens)
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems, n_frames=n - 1)[0] == D.ERROR        # the nFrames rule
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, [3] + s.elems[1:])[0] == D.ERROR              # a bad element size
        host = C.create_string_buffer(SIZES[2])
        bufs = list(s.src.bufs)
        bufs[2] = (C.addressof(host), SIZES[2])
        assert s.fr.verify_raw(s.frames, bufs, s.given, s.elems)[0] == D.ERROR                              # not device memory
        given = list(s.given)
        given[2] = (C.addressof(host), SIZES[2])
        assert s.fr.verify_raw(s.frames, s.src.bufs, given, s.elems)[0] == D.ERROR                          # a base that is not
        given[2] = (s.given[2][0], SIZES[2] - 1)
        assert s.fr.verify_raw(s.frames, s.src.bufs, given, s.elems)[0] == D.ERROR                          # a base of another size
        bufs[2] = (0, SIZES[2])
        assert s.fr.verify_raw(s.frames, bufs, s.given, s.elems)[0] == D.ERROR                              # a NULL buffer of a size above 0
        assert waits() == before
        # no buffers, or only empty ones: 0 and no GPU is touched
        assert s.fr.verify_raw([], [], None, None)[0] == 0 and s.fr.verify_raw([[]], [(0, 0)], None, [2])[0] == 0 and waits() == before
        assert s.fr.verify_raw(s.frames, s.src.bufs, s.given, s.elems)[0] == 0
    finally:
        s.close()


def test_mock_kernel_against_the_numpy_reference(verifymock):
    """the plain-C definition and qz_device.ungroup_cmp_ref agree on the GPU test's own rows (host memory here), tile words and tile0"""
    import test_gpu_ungroup_cmp as G
    plug, _ = verifymock
    L = D.bind_cmp_kernel(plug.lib)
    case = G.every_case()
    case.add(3 * 16384 + 5, 4, 7, 8, "base", (40000, 16385))
    live, base, stage = case.build()
    keep = [np.ascontiguousarray(x) for x in (live, base)]
    aligned = np.zeros(len(stage) + 16, dtype=np.uint8)
    off = (-aligned.ctypes.data) % 16
    aligned[off:off + len(stage)] = stage
    rows = (D.UngroupCmpRow * len(case.rows))()
    d_rows = (D.UngroupCmpRow * len(case.rows))()
    case.fill(rows, keep[0].ctypes.data, keep[1].ctypes.data)
    t0, total = case.tile0()
    tiles = np.full(total + 2, 7, dtype=np.uint32)
    assert L.qzstd_hip_ungroup_cmp(0, None, rows, len(case.rows), d_rows, aligned.ctypes.data + off, len(stage), tiles.ctypes.data + 4) == 0
    assert np.array_equal(tiles[1:-1], case.want(live, base, stage)) and tiles[0] == 7 and tiles[-1] == 7
    assert [r.tile0 for r in rows] == t0
    assert list(tiles[1 + t0[-1]:1 + t0[-1] + 4]) == [D.CMP_SAME, 16385, 40000, D.CMP_SAME]
    rows[3].flags = 2
    for r in rows:
        r.tile0 = G.SENTINEL
    assert L.qzstd_hip_ungroup_cmp(0, None, rows, len(case.rows), d_rows, aligned.ctypes.data + off, len(stage), tiles.ctypes.data + 4) < 0
    assert all(r.tile0 == G.SENTINEL for r in rows)


def test_device_layer_without_the_cmp_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the comparison's stand-in: the verify call returns (size_t)-1 with no event wait and
    nothing counted; compress and restore are served by the same library (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOCMP_MOCK_SO, NOCMP_FRONT_SO, cmp=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [data[::-1]], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
frames = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2])
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_ungroup_xor_launches(), fr.stats(), fr.restore_stats(), fr.verify_stats())
before = state()
r1 = fr.verify_raw(frames, pool.bufs, bas.bufs, [2])[0]
r2 = fr.verify_raw(frames, pool.bufs, None, [2])[0]
nothing = state() == before
out = R.OutPool(plug, [len(data)], [3], slot=2)
back = fr.restore_batch_delta(frames, out.bufs, bas.bufs, [2]) == len(frames[0]) and out.bytes() == out.expected([data])
again = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2]) == frames
print(json.dumps({"refused": r1 == D.ERROR and r2 == D.ERROR, "nothing_queued": nothing, "restore": back, "compress": again,
                  "has_cmp": hasattr(plug.lib, "qzstd_hip_ungroup_cmp")}))
""", NOCMP_MOCK_SO, NOCMP_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "restore": True, "compress": True, "has_cmp": False}, res
