"""CPU: QZSTD_frontCompressDeviceSlices (include/qzstd_frontend_device.h) over the mock device layer — the cycle test's mock pair plus
tests/mock/mock_hip_group_pieces.c (the gather from pieces in plain C).  The oracle is code that exists: every frame of a call whose buffers
are lists of source slices, scattered over "device" memory at every misalignment and in another order than the buffers', must be byte for
byte the frame QZSTD_frontCompressDeviceBatchDelta returns for the same bytes held contiguously — with and without bases, with checksum, plane
probe and delta skip off and on, at levels 1 and 6, at chunk sizes 16400 and 100003, for one slice per buffer, column-shard widths, cuts at
and around the frame boundaries, random cuts and empty slices in between.  Also: a failed block (the bytes come back piece by piece), one
slice per buffer launch for launch the Delta call, the round trip through QZSTD_frontRestoreDeviceSlices with the same cutting, every refusal
with nothing queued and nothing counted, and a device layer without the new entry point.  Every comparison is byte-exact.
One narrowing of the cases, for the slice list's length: the width-1 column shard is applied to the buffers up to 2 x 16400 + 5 bytes (its
frames are cut at 16400, so one-byte slices cross frame boundaries there); the 300001-byte buffer is cut into width 17 in that cutting, not
into 300001 slices."""
import ctypes as C
import mmap
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D
import test_device_checksum_mock as T
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_srcslicesmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_srcslicesmock.so")
NOPIECES_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nopiecesmock.so")
NOPIECES_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nopiecesmock.so")
SIZES = (0, 1, 7, 16383, 2 * 16400 + 5, 300001)
ELEMS = (2, 1, 4, 8, 2, 4)
KINDS = ("bf16", "text", "fp32", "ids64", "bf16", "fp32")
BASED = (True, True, False, True, True, True)  # (in the calls with bases)
CHUNKS = (16400, 100003)
CUTTINGS = ("one", "w1", "w17", "w2048", "frame", "random", "empties")
ONE_BYTE = 300001 // 2 + 11  # buffer 5 equals its base except for this byte, inside a slice in the middle of a frame
FILL = 0xA5


def build_pair(zstd_path, mock_so, front_so, pieces: bool):
    """the cycle test's mock pair, with the gather from pieces or — an older device layer — without"""
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle"), "-I" + os.path.join(B.PKG_DIR, "frontend")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c", "mock_hip_plane_cost.c")]
    if pieces:  # (its definition is the headers' own QZSTD_byteXor and QZSTD_byteGroup)
        srcs += [os.path.join(MOCK, "mock_hip_group_pieces.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_bytegroup.c"),
                 os.path.join(MOCK, "mock_hip_pointer_extent.c")]  # (and the allocations' extents, which an older layer does not tell either)
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def srcmock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, pieces=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    for n in ("qzstd_mock_group_pieces_rows", "qzstd_mock_group_pieces_pieces", "qzstd_mock_diff_rows", "qzstd_mock_xxh64_rows",
              "qzstd_mock_plane_cost_rows", "qzstd_mock_gather_rows"):
        getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


class Arena:
    """host memory the mock treats as device memory, one registered range: allocations at a chosen misalignment, guard bytes between them"""

    def __init__(self, plug, size, slot):
        # (a mapping of its own, not heap memory: freeing MiB-sized heap blocks would change where the allocator places the pools of the
        # test modules that run after this one in the same process)
        self.map = mmap.mmap(-1, size + 64)
        self.mem = np.frombuffer(self.map, dtype=np.uint8)
        self.mem[:] = FILL
        self.base = (self.mem.ctypes.data + 63) & ~63
        self.pos, self.size = 0, size
        plug.lib.qzstd_mock_device_range(slot, self.base, size, 0)
        if hasattr(plug.lib, "qzstd_mock_extent_range"):  # (one allocation)
            plug.lib.qzstd_mock_extent_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
            plug.lib.qzstd_mock_extent_range(slot, self.base, size)

    def put(self, data: bytes, mis: int) -> int:
        at = ((self.pos + 15) & ~15) + 16 + mis  # (at least 16 guard bytes in front: no two allocations follow each other in memory)
        assert at + len(data) + 16 <= self.size
        C.memmove(self.base + at, data, len(data))
        self.pos = at + len(data)
        return self.base + at

    def snapshot(self) -> bytes:
        return C.string_at(self.base, self.size)


def corpus():
    """(the buffers, their bases): buffer 3 equals its base, buffer 5 equals it except for ONE byte, the others differ in a fifth of their bytes"""
    import qz_corpus as K
    datas, bases = [], []
    for i, (kind, n) in enumerate(zip(KINDS, SIZES)):
        d = D.typed_corpus(kind, n, 210 + i) if kind != "text" else K.by_name("text", n, seed=210 + i)
        b = np.frombuffer(d, dtype=np.uint8).copy()
        if i == 5:
            b[ONE_BYTE] ^= 0x40
        elif i != 3 and n:
            b ^= ((np.random.default_rng(i).random(n) < 0.2) * np.random.default_rng(100 + i).integers(1, 8, n)).astype(np.uint8)
        datas.append(d)
        bases.append(b.tobytes())
    return datas, bases


def cut(name, n, chunk, seed):
    """-> the slice sizes of a buffer of n bytes, zeros included: they tile [0, n)"""
    rng = np.random.default_rng(seed)
    if name == "one" or n == 0:
        return [n] if name != "empties" else [0, n, 0]
    if name[0] == "w":
        w = int(name[1:])
        if w == 1 and n > 40000:
            w = 17  # (the largest buffer in one-byte slices would be 300001 of them: its one-byte slices are the 32805-byte buffer's)
        return [min(w, n - o) for o in range(0, n, w)]
    if name == "frame":
        points = sorted({p for c in range(chunk, n + chunk, chunk) for p in (c - 1, c, c + 1) if 0 < p < n})
    else:
        points = sorted(set(rng.integers(1, n, min(n - 1, 3 + n // 3000)).tolist())) if n > 1 else []
    sizes = [b - a for a, b in zip([0] + points, points + [n])]
    if name == "empties":
        sizes = [x for s in sizes for x in (s, 0)]
    return sizes


class Case:
    """one cutting of the corpus at one chunk size: every slice of every buffer (and of every base) an allocation of its own, placed in a
    shuffled order, the sources' misalignment cycling through 0 .. 15 and the bases' through another cycle"""

    def __init__(self, plug, datas, bases, name, chunk, slot):
        self.sizes = [cut(name, n, chunk, 31 * i + chunk % 97) for i, n in enumerate(SIZES)]
        flat = [(i, o, s) for i, ss in enumerate(self.sizes) for o, s in zip(np.cumsum([0] + ss[:-1]).tolist(), ss)]
        total = sum(SIZES)
        self.arena = Arena(plug, 2 * total + 2 * 48 * len(flat) + 4096, slot)
        order = np.random.default_rng(len(flat)).permutation(len(flat))
        src, bas = [0] * len(flat), [0] * len(flat)
        for rank, at in enumerate(order.tolist()):
            i, o, s = flat[at]
            if s:
                src[at] = self.arena.put(datas[i][o:o + s], rank % 16)
                bas[at] = self.arena.put(bases[i][o:o + s], (7 * rank + 3) % 16)
        self.flat, self.src, self.bas = flat, src, bas
        self.before = self.arena.snapshot()

    def slices(self, based):
        """based: per buffer, whether its slices carry their base"""
        return [(i, o, s, self.src[at] if s else 0, self.bas[at] if s and based[i] else None) for at, (i, o, s) in enumerate(self.flat)]

    def multi_frames(self, chunk, skipped=()):
        """frames made of more than one slice, but for those a delta skip left out ((buffer, frame) pairs)"""
        n = 0
        for i, ss in enumerate(self.sizes):
            ends = np.cumsum(ss)
            for c, lo in enumerate(range(0, SIZES[i], chunk)):
                hi = min(SIZES[i], lo + chunk)
                first = int(np.searchsorted(ends, lo, side="right"))
                n += ends[first] < hi and (i, c) not in skipped
        return int(n)


@pytest.fixture(scope="module")
def world(srcmock):
    """the corpus contiguous in two pools (the Delta call's input) and cut every way at both chunk sizes, built once"""
    plug, F = srcmock
    datas, bases = corpus()
    whole = Arena(plug, 2 * sum(SIZES) + 4096, 0)
    bufs = [(whole.put(d, (5 * i + 1) % 16), len(d)) for i, d in enumerate(datas)]
    bbufs = [(whole.put(b, (3 * i + 2) % 16), len(b)) for i, b in enumerate(bases)]
    cases = {(name, chunk): Case(plug, datas, bases, name, chunk, 1 + k) for k, (name, chunk) in
             enumerate((n, c) for c in CHUNKS for n in CUTTINGS)}
    return dict(datas=datas, bases=bases, bufs=bufs, bbufs=bbufs, cases=cases, whole=whole)


def counters(plug, fr):
    L = plug.lib
    return dict(find=L.qzstd_mock_launches(), xor=L.qzstd_mock_group_xor_launches(), xor_rows=L.qzstd_mock_group_xor_rows(),
                group=L.qzstd_mock_group_launches(), group_rows=L.qzstd_mock_group_rows(), gather=L.qzstd_mock_gather_launches(),
                gather_rows=L.qzstd_mock_gather_rows(), compact=L.qzstd_mock_compact_launches(), diff=L.qzstd_mock_diff_launches(),
                diff_rows=L.qzstd_mock_diff_rows(), hash=L.qzstd_mock_xxh64_launches(), hash_rows=L.qzstd_mock_xxh64_rows(),
                plane=L.qzstd_mock_plane_cost_launches(), plane_rows=L.qzstd_mock_plane_cost_rows(), waits=L.qzstd_mock_event_waits(),
                pieces=L.qzstd_mock_group_pieces_launches())


def front_stats(fr):
    return dict(dev=fr.stats(), group=fr.byte_group_stats(), delta=fr.delta_stats(), skip=fr.delta_skip_stats(), cksum=fr.checksum_stats(),
                probe=fr.plane_probe_stats())


def grown(a, b):
    return {k: ([y - x for x, y in zip(a[k], b[k])] if isinstance(a[k], list) else b[k] - a[k]) for k in a}


@pytest.mark.parametrize("with_bases", (False, True), ids=("nobase", "bases"))
@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
@pytest.mark.parametrize("level", (1, 6))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_frames_equal_the_delta_calls_on_the_contiguous_bytes(srcmock, world, monkeypatch, chunk, level, settings, with_bases):
    plug, F = srcmock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    based = BASED if with_bases else (False,) * len(SIZES)
    fr = D.DeviceFront(3, level, chunk, lib=F)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        given = [b if on else None for b, on in zip(world["bbufs"], based)]
        s0 = front_stats(fr)
        want = fr.compress_device_batch_delta(world["bufs"], given, ELEMS)
        s1 = front_stats(fr)
        assert [len(x) for x in want] == [-(-n // chunk) for n in SIZES]
        skipped = set()
        if settings and with_bases:
            # the delta skip's cases are there: whole buffers equal to their base, and one that differs in a single byte
            zero = [[f == S_zero(plug, min(chunk, n - c * chunk), True) for c, f in enumerate(fs)] for fs, n in zip(want, SIZES)]
            assert all(zero[3]) and sum(not z for z in zero[5]) == 1 and not zero[5][ONE_BYTE // chunk] and not any(zero[4])
            skipped = {(i, c) for i, zs in enumerate(zero) for c, z in enumerate(zs) if z}
        for name in CUTTINGS:
            case = world["cases"][(name, chunk)]
            sl = case.slices(based)
            c0, t0, p0, e0 = counters(plug, fr), front_stats(fr), fr.src_slice_stats(), plug.lib.qzstd_mock_extent_lookups()
            got = fr.compress_device_slices(SIZES, ELEMS, sl)
            c1, t1, p1 = counters(plug, fr), front_stats(fr), fr.src_slice_stats()
            assert 1 <= plug.lib.qzstd_mock_extent_lookups() - e0 <= 2, name  # the slices lie in ONE allocation: looked up once, the bases once
            for i in range(len(SIZES)):
                for c, (g, w) in enumerate(zip(got[i], want[i])):
                    assert g == w, (name, "buffer", i, "frame", c)
            assert [len(x) for x in got] == [len(x) for x in want]
            assert case.arena.snapshot() == case.before, name  # the sources and bases are only read
            assert grown(t0, t1) == grown(s0, s1), name        # every statistic counts this call as it counts the Delta call
            multi = case.multi_frames(chunk, skipped)
            d = [b - a for a, b in zip(p0, p1)]
            assert d[:3] == [sum(1 for x in sl if x[2]), sum(SIZES), multi], name
            assert d[3] == c1["pieces"] - c0["pieces"] and (d[3] >= 1) == (multi > 0) and d[3] <= -(-sum(SIZES) // chunk), name
            if name == "one":
                assert multi == 0
            elif name in ("w17", "frame", "random"):
                assert multi > 0
    finally:
        fr.close()


def S_zero(plug, n, checksum):
    import test_device_skip_mock as K
    plug.lib.qzstd_mock_xxh64.restype = C.c_uint64
    plug.lib.qzstd_mock_xxh64.argtypes = [C.c_void_p, C.c_uint64]
    return K.canonical(plug, n, checksum)


@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
def test_one_slice_per_buffer_is_the_delta_call_launch_for_launch(srcmock, world, monkeypatch, settings):
    plug, F = srcmock
    chunk = CHUNKS[0]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        for based in (BASED, (False,) * len(SIZES)):
            given = [b if on else None for b, on in zip(world["bbufs"], based)]
            sl = [(i, 0, n, p, given[i][0] if given[i] else None) for i, (p, n) in enumerate(world["bufs"])]
            c0 = counters(plug, fr)
            want = fr.compress_device_batch_delta(world["bufs"], given, ELEMS)
            c1 = counters(plug, fr)
            got = fr.compress_device_slices(SIZES, ELEMS, sl)
            c2 = counters(plug, fr)
            assert got == want and grown(c1, c2) == grown(c0, c1) and c2["pieces"] == c0["pieces"]
            # slices that follow each other in memory are the buffer they are cut from: still no launch from pieces
            cutup = [(i, o, min(1000, n - o), p + o, (given[i][0] + o) if given[i] else None) for i, (p, n) in enumerate(world["bufs"])
                     for o in range(0, n, 1000)]
            assert fr.compress_device_slices(SIZES, ELEMS, cutup) == want
            c3 = counters(plug, fr)
            assert grown(c2, c3) == grown(c0, c1) and c3["pieces"] == c0["pieces"]
    finally:
        fr.close()


@pytest.mark.parametrize("k", (1, 4))
def test_a_failed_block_brings_the_bytes_back_piece_by_piece(srcmock, zstd, k):
    """the matcher fails block 0 of every launch: frame 0, made of several slices, has its bytes AND its base's copied back piece by piece,
    XORed and grouped on the host — the frame the Delta call builds from the contiguous bytes under the same failure"""
    plug, F = srcmock
    chunk = CHUNKS[0]
    n = 3 * chunk + 100
    data, base = D.typed_corpus("fp32", n, 5), D.typed_corpus("fp32", n, 6)
    arena = Arena(plug, 8 * n, 15)
    whole = [(arena.put(data, 3), n)], [(arena.put(base, 8), n)]
    sl = [(0, o, min(2050, n - o), arena.put(data[o:o + 2050], o % 16), arena.put(base[o:o + 2050], (o + 5) % 16)) for o in range(0, n, 2050)]
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        clean = fr.compress_device_slices([n], [k], sl)
        assert clean == fr.compress_device_batch_delta(whole[0], whole[1], [k])
        plug.lib.qzstd_mock_fail_block(0)
        try:
            d0, s0 = fr.delta_stats(), fr.stats()
            want = fr.compress_device_batch_delta(whole[0], whole[1], [k])
            d1, s1 = fr.delta_stats(), fr.stats()
            got = fr.compress_device_slices([n], [k], sl)
            d2, s2 = fr.delta_stats(), fr.stats()
        finally:
            plug.lib.qzstd_mock_fail_block(-1)
        assert got == want and got[0][1:] == clean[0][1:]
        assert d1[2] == d0[2] + 1 and d2[2] == d1[2] + 1 and [b - a for a, b in zip(s1, s2)] == [b - a for a, b in zip(s0, s1)]
        delta = (int.from_bytes(data[:chunk], "little") ^ int.from_bytes(base[:chunk], "little")).to_bytes(chunk, "little")
        assert D.ungroup_bytes(zstd.decompress(got[0][0], chunk), k, F) == delta
    finally:
        fr.close()


@pytest.mark.parametrize("name", ("w2048", "random", "empties"))
def test_round_trip_through_restore_slices_with_the_same_cutting(srcmock, world, name):
    plug, F = srcmock
    chunk = CHUNKS[1]
    case = world["cases"][(name, chunk)]
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        frames = fr.compress_device_slices(SIZES, ELEMS, case.slices(BASED))
        out = Arena(plug, sum(SIZES) + 48 * len(case.flat) + 4096, 15)
        dst = [out.put(bytes(s), (3 * at + 1) % 16) if s else 0 for at, (_, _, s) in enumerate(case.flat)]
        back = [(i, o, s, dst[at], case.bas[at] if s and BASED[i] else None) for at, (i, o, s) in enumerate(case.flat)]
        assert fr.restore_slices(frames, SIZES, ELEMS, back) == sum(len(f) for f in frames)
        for at, (i, o, s) in enumerate(case.flat):
            assert C.string_at(dst[at], s) == world["datas"][i][o:o + s], (i, o, s)
            if s:
                assert C.string_at(dst[at] - 16, 16) == bytes([FILL]) * 16 and C.string_at(dst[at] + s, 16) == bytes([FILL]) * 16
    finally:
        fr.close()


def test_refusals_queue_nothing_and_count_nothing(srcmock, world):
    plug, F = srcmock
    chunk = CHUNKS[0]
    case = world["cases"][("w2048", chunk)]
    good = case.slices(BASED)
    host = C.create_string_buffer(4096)  # (not registered: host memory)
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        def refused(sizes, elems, slices, what):
            c0, t0, p0 = counters(plug, fr), front_stats(fr), fr.src_slice_stats()
            r, frames = fr.compress_device_slices_raw(sizes, elems, slices)
            assert r == D.ERROR and frames is None, what
            assert (counters(plug, fr), front_stats(fr), fr.src_slice_stats()) == (c0, t0, p0), what

        def change(at, **kw):
            names = ("buf", "offset", "size", "src", "base")
            out = list(good)
            out[at] = tuple(kw.get(n, v) for n, v in zip(names, good[at]))
            return out

        mid = next(at for at, x in enumerate(good) if x[0] == 5 and x[1] > 0)  # a slice in the middle of the largest buffer
        refused(None, ELEMS, good, "null bufSizes")
        r = F.QZSTD_frontCompressDeviceSlices(fr.f, (C.c_size_t * 6)(*SIZES), None, 6, None, 3, None, fr._dst, len(fr._dst), (C.c_size_t * 64)(), None)
        assert r == D.ERROR
        refused(SIZES, ELEMS, change(mid, buf=len(SIZES)), "buf >= nBufs")
        refused(SIZES, ELEMS, good[:mid] + [good[mid + 1], good[mid]] + good[mid + 2:], "out of order")
        refused(SIZES, ELEMS, list(reversed(good)), "buffers out of order")
        refused(SIZES, ELEMS, good[:mid] + good[mid + 1:], "a gap")
        refused(SIZES, ELEMS, good[:mid] + [good[mid]] + good[mid:], "an overlap")
        refused(SIZES, ELEMS, change(mid, offset=good[mid][1] - 1), "an overlap by one byte")
        refused(SIZES, ELEMS, change(len(good) - 1, size=good[-1][2] + 1), "an end past its buffer")
        refused(SIZES, ELEMS, good[:-1], "a buffer that ends short")
        refused(SIZES, ELEMS, good + [(5, SIZES[5] + 1, 0, 0, None)], "an empty slice past its buffer")
        refused(SIZES, ELEMS, change(mid, base=None), "based and unbased slices in one buffer")
        refused(SIZES, ELEMS, change(mid, src=0), "null d_src")
        refused(SIZES, ELEMS, change(mid, src=C.addressof(host)), "a source in host memory")
        refused(SIZES, ELEMS, change(mid, base=C.addressof(host)), "a base in host memory")
        refused(SIZES, ELEMS, change(mid, src=case.arena.base + case.arena.size - 10), "a source whose last byte is not device memory")
        refused(SIZES, (2, 1, 4, 8, 2, 4 | D.ELEM_DIFF), good, "QZSTD_ELEM_DIFF")
        refused(SIZES, (2, 1, 3, 8, 2, 4), good, "element size 3")
        plug.lib.qzstd_mock_device_range(14, C.addressof(host), 4096, 1)  # another device
        refused(SIZES, ELEMS, change(mid, src=C.addressof(host)), "a source on another device")
        plug.lib.qzstd_mock_device_range(14, None, 0, 0)
        c0 = counters(plug, fr)
        small = (C.c_size_t * 64)()
        bs = (C.c_size_t * 6)(*SIZES)
        arr = fr.src_slice_array(good)
        assert F.QZSTD_frontCompressDeviceSlices(fr.f, bs, bytes(ELEMS), 6, arr, len(good), None, fr._dst, fr.stride, small, None) == D.ERROR  # capacity
        assert F.QZSTD_frontCompressDeviceSlices(None, bs, bytes(ELEMS), 6, arr, len(good), None, fr._dst, len(fr._dst), small, None) == D.ERROR
        assert F.QZSTD_frontCompressDeviceSlices(fr.f, bs, bytes(ELEMS), 6, arr, len(good), None, None, len(fr._dst), small, None) == D.ERROR
        assert counters(plug, fr) == c0 and fr.src_slice_stats() == [0, 0, 0, 0]
        st = (C.c_ulonglong * 4)(9, 9, 9, 9)
        F.QZSTD_frontSrcSliceStats(None, st)
        assert list(st) == [0, 0, 0, 0]
        F.QZSTD_frontSrcSliceStats(fr.f, None)
        # no buffers, and only empty ones: no frames, no GPU touched
        assert fr.compress_device_slices_raw([], [], [])[0] == 0 and fr.compress_device_slices_raw([0, 0], [2, 4], [(1, 0, 0, 0, None)])[0] == 0
        assert counters(plug, fr) == c0
        assert fr.compress_device_slices(SIZES, ELEMS, good) == fr.compress_device_batch_delta(
            world["bufs"], [b if on else None for b, on in zip(world["bbufs"], BASED)], ELEMS)
    finally:
        fr.close()


def test_the_launchers_checks_and_definition_in_the_mock(srcmock):
    """qzstd_hip_group_pieces of the mock itself: a row of three pieces with and without a base, its refusals before anything is touched"""
    plug, F = srcmock
    L = D.bind_pieces_kernel(plug.lib)
    src = bytes(range(1, 101))
    bas = bytes((7 * i) & 255 for i in range(100))
    a, b = C.create_string_buffer(src, 100), C.create_string_buffer(bas, 100)
    stage = (C.c_ubyte * (256 + 16))(*([FILL] * 272))
    st = (C.addressof(stage) + 15) & ~15

    def launch(cuts, rows_spec, n_pieces=None, null=None):
        pieces = (D.GroupPiece * max(len(cuts), 1))()
        for p, (off, ln, so, bo) in zip(pieces, cuts):
            p.src, p.base, p.off, p.len = (C.addressof(a) + so if so is not None else 0), (C.addressof(b) + bo if bo is not None else 0), off, ln
        rows = (D.GroupPiecesRow * max(len(rows_spec), 1))()
        for r, (dst, ln, pad, k, p0, np_, res) in zip(rows, rows_spec):
            r.dstOff, r.len, r.pad, r.elem, r.piece0, r.nPieces, r.reserved = dst, ln, pad, k, p0, np_, res
        d_rows, d_pieces = (D.GroupPiecesRow * max(len(rows_spec), 1))(), (D.GroupPiece * max(len(cuts), 1))()
        C.memset(st, FILL, 256)
        rc = L.qzstd_hip_group_pieces(0, None, None if null == "rows" else rows, len(rows_spec), None if null == "d_rows" else d_rows,
                                      None if null == "pieces" else pieces, len(cuts) if n_pieces is None else n_pieces,
                                      None if null == "d_pieces" else d_pieces, None if null == "stage" else st, 256)
        return rc, C.string_at(st, 256)

    three = [(0, 1, 0, 50), (1, 60, 20, 0), (61, 39, 1, 61)]
    want = bytes(x ^ y for x, y in zip(src[0:1] + src[20:80] + src[1:40], bas[50:51] + bas[0:60] + bas[61:100]))
    n0 = L.qzstd_mock_group_pieces_launches()
    rc, got = launch(three, [(16, 100, 12, 4, 0, 3, 0)])
    assert rc == 0 and got == bytes([FILL]) * 16 + D.group_bytes(want, 4, F) + bytes(12) + bytes([FILL]) * 128
    rc, got = launch([(o, n, s, None) for o, n, s, _ in three], [(0, 100, 12, 2, 0, 3, 0), (112, 0, 16, 8, 3, 0, 0)])
    assert rc == 0 and got == D.group_bytes(src[0:1] + src[20:80] + src[1:40], 2, F) + bytes(28) + bytes([FILL]) * 128
    assert L.qzstd_mock_group_pieces_launches() == n0 + 2
    row = (16, 100, 12, 4, 0, 3, 0)
    bad = {"a gap": ([(0, 1, 0, 50), (2, 59, 20, 0), (61, 39, 1, 61)], [row]), "an overlap": ([(0, 2, 0, 50), (1, 60, 20, 0), (61, 39, 1, 61)], [row]),
           "short": (three[:2], [(16, 100, 12, 4, 0, 2, 0)]), "long": (three, [(16, 99, 13, 4, 0, 3, 0)]),
           "an empty piece": ([(0, 1, 0, 50), (1, 0, 20, 0), (1, 60, 20, 0), (61, 39, 1, 61)], [(16, 100, 12, 4, 0, 4, 0)]),
           "a null source": ([(0, 1, 0, 50), (1, 60, None, 0), (61, 39, 1, 61)], [row]), "past the table": (three, [(16, 100, 12, 4, 1, 3, 0)]),
           "no pieces for a row with bytes": (three, [(16, 100, 12, 4, 0, 0, 0)]), "elem 3": (three, [(16, 100, 12, 3, 0, 3, 0)]),
           "reserved": (three, [(16, 100, 12, 4, 0, 3, 1)]), "dstOff": (three, [(8, 100, 12, 4, 0, 3, 0)]), "len + pad": (three, [(16, 100, 11, 4, 0, 3, 0)]),
           "past stageBytes": (three, [(160, 100, 12, 4, 0, 3, 0)]), "rows overlap": (three, [(16, 100, 12, 4, 0, 3, 0), (96, 100, 12, 4, 0, 3, 0)])}
    for name, (cuts, rows_spec) in bad.items():
        rc, got = launch(cuts, rows_spec)
        assert rc < 0 and got == bytes([FILL]) * 256, name
    for null in ("rows", "d_rows", "pieces", "d_pieces", "stage"):
        rc, got = launch(three, [row], null=null)
        assert rc < 0 and got == bytes([FILL]) * 256, null
    rc, got = launch(three, [row], n_pieces=2)
    assert rc < 0 and got == bytes([FILL]) * 256
    rc, got = launch(three, [])
    assert rc == 0 and got == bytes([FILL]) * 256 and L.qzstd_mock_group_pieces_launches() == n0 + 2


def test_device_layer_without_the_pieces_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the new sources (no gather from pieces, no extents of allocations: every range is looked up at
    its first and its last byte): a call with a frame of several slices returns (size_t)-1 with no launch, no
    event wait and nothing counted; a call in which every frame lies in one slice, and the Delta call, are served (a process of its own)"""
    build_pair(zstd.path, NOPIECES_MOCK_SO, NOPIECES_FRONT_SO, pieces=False)
    res = T.run_child("""
chunk = 16400
n = 3 * chunk + 321
data = D.typed_corpus("bf16", n, 1)
base = D.typed_corpus("bf16", n, 2)
pool = T.Pool(plug, [data, data[:chunk], data[chunk:2 * chunk + 7], data[2 * chunk + 7:]], [0, 3, 9, 6], slot=0)
bas = T.Pool(plug, [base, base[:chunk], base[chunk:2 * chunk + 7], base[2 * chunk + 7:]], [5, 1, 0, 2], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
want = fr.compress_device_batch_delta(pool.bufs[:1], bas.bufs[:1], [2])
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_xor_launches(), fr.stats(), fr.delta_stats(), fr.src_slice_stats())
before = state()
cut = [(0, 0, chunk, pool.bufs[1][0], bas.bufs[1][0]), (0, chunk, chunk + 7, pool.bufs[2][0], bas.bufs[2][0]),
       (0, 2 * chunk + 7, n - 2 * chunk - 7, pool.bufs[3][0], bas.bufs[3][0])]
r1 = fr.compress_device_slices_raw([n], [2], cut)[0]
nothing = state() == before
one = fr.compress_device_slices([n], [2], [(0, 0, n, pool.bufs[0][0], bas.bufs[0][0])]) == want
pool2 = T.Pool(plug, [data[:2 * chunk], data[2 * chunk:]], [7, 4], slot=2)
bas2 = T.Pool(plug, [base[:2 * chunk], base[2 * chunk:]], [2, 11], slot=3)
at_frames = fr.compress_device_slices([n], [2], [(0, 0, 2 * chunk, pool2.bufs[0][0], bas2.bufs[0][0]), (0, 2 * chunk, n - 2 * chunk, pool2.bufs[1][0], bas2.bufs[1][0])]) == want
print(json.dumps({"refused": r1 == D.ERROR, "nothing_queued": nothing, "one_slice": one, "cut_at_frames": at_frames,
                  "delta": fr.compress_device_batch_delta(pool.bufs[:1], bas.bufs[:1], [2]) == want,
                  "has_pieces": hasattr(plug.lib, "qzstd_hip_group_pieces")}))
""", NOPIECES_MOCK_SO, NOPIECES_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "one_slice": True, "cut_at_frames": True, "delta": True, "has_pieces": False}, res
