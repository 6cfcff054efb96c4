"""CPU: delta skip (QZSTD_frontSetDeltaSkip / QZSTD_frontGetDeltaSkip / QZSTD_frontDeltaSkipStats: include/qzstd_frontend_device.h) over the
mock device layer — the mock pair of tests/test_device_slices_mock.py plus tests/mock/mock_hip_diff.c (the comparison in plain C).  With the
setting off the delta calls are what they were and the comparison is never launched; with it on, every frame of a changed chunk is byte for
byte the setting-off frame and every frame of a chunk equal to its base chunk is exactly the canonical zero frame of its length (1, 255,
256, 65791, 65792, 128 KiB, and 256 KiB + 3 on a front of its own: two blocks and a tail); a buffer of zeros without a base is not skipped;
a call whose frames are all equal queues no part; the restore recognises the zero frames, decodes only the others and is exact in place and
into fresh buffers; with the setting off it decodes them all to the same bytes; a device layer without qzstd_hip_diff refuses the call with
the setting on and a base, and serves it with the setting off.  Every comparison is byte-exact."""
import ctypes as C
import os

import pytest

import qz_device as D
import test_device_checksum_mock as T
import test_device_restore_mock as R
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_skipmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_skipmock.so")
NODIFF_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nodiffmock.so")
NODIFF_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nodiffmock.so")
CHUNK = 131072
# per buffer: (size, element size, has a base, which frames differ from the base: "none", "all", or a set of frame numbers)
BUFS = (
    (2 * CHUNK + 1, 2, True, "none"),       # frozen: frames of 128 KiB, 128 KiB and 1 byte, all equal
    (CHUNK + 255, 1, True, {0}),            # the tail of 255 bytes is equal
    (256, 4, True, "none"),
    (65791, 1, True, "none"),
    (65792, 4, True, "none"),
    (3 * CHUNK + 77, 2, False, "zeros"),    # zeros, no base: never compared, never skipped
    (2 * CHUNK + 100, 4, True, "all"),
    (0, 2, True, "none"),
    (CHUNK + 5, 1, False, "all"),
    (3 * CHUNK + 9, 2, True, {1}),          # an equal frame, a changed one, an equal one, an equal tail: frames around a skipped one
)
KINDS = ("bf16", "text", "fp32", "text", "fp32", "bf16", "fp32", "bf16", "text", "bf16")
SIZES = tuple(b[0] for b in BUFS)
ELEMS = tuple(b[1] for b in BUFS)
BASED = tuple(b[2] for b in BUFS)
BIG = 2 * CHUNK + 3  # the chunk size of the second front: a zero frame of two full blocks and a tail


def build_pair(zstd_path, mock_so, front_so, diff: bool):
    """the slices test's mock pair, with the comparison's stand-in or — an older device layer — without"""
    import qz_bind as B
    import subprocess
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c")]
    if diff:
        srcs.append(os.path.join(MOCK, "mock_hip_diff.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def skipmock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, diff=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    S.bind_hooks(plug)
    plug.lib.qzstd_mock_diff_rows.restype = C.c_ulonglong
    plug.lib.qzstd_mock_xxh64.restype = C.c_uint64
    plug.lib.qzstd_mock_xxh64.argtypes = [C.c_void_p, C.c_uint64]
    return plug, F


def corpus(bufs=BUFS, kinds=KINDS, chunk=CHUNK):
    """(the new buffers, their bases): a base equals its buffer except in the frames named, where a few bits differ"""
    import numpy as np
    import qz_corpus as K
    datas, bases = [], []
    for i, ((n, _, _, changed), kind) in enumerate(zip(bufs, kinds)):
        if changed == "zeros":
            d = bytes(n)
        else:
            d = D.typed_corpus(kind, n, 160 + i) if kind != "text" else K.by_name("text", n, seed=160 + i)
        b = np.frombuffer(d, dtype=np.uint8).copy()
        for c in range(-(-n // chunk)):
            if changed == "all" or (isinstance(changed, set) and c in changed):
                lo, hi = c * chunk, min(n, (c + 1) * chunk)
                flips = (np.random.default_rng(7 * i + c).random(hi - lo) < 0.2) * np.random.default_rng(300 + i + c).integers(1, 8, hi - lo)
                b[lo:hi] ^= flips.astype(np.uint8)
                b[hi - 1] ^= 1  # (at least the frame's last byte differs)
        datas.append(d)
        bases.append(b.tobytes())
    return datas, bases


def equal_map(datas, bases, based, chunk):
    """per buffer, per frame: True where the frame's chunk has a base and equals it — the counts every check below is worked out from"""
    return [[on and d[o:o + chunk] == b[o:o + chunk] for o in range(0, len(d), chunk)] for d, b, on in zip(datas, bases, based)]


def canonical(plug, n, checksum):
    """the canonical zero frame of n bytes, the checksum field from the mock's XXH64 of n zero bytes"""
    fr = D.zero_frame(n, checksum)
    if checksum:
        zeros = C.create_string_buffer(n)
        fr += (plug.lib.qzstd_mock_xxh64(zeros, n) & 0xFFFFFFFF).to_bytes(4, "little")
    return fr


def counters(plug, fr):
    L = plug.lib
    return dict(diff=L.qzstd_mock_diff_launches(), rows=L.qzstd_mock_diff_rows(), find=L.qzstd_mock_launches(), xor=L.qzstd_mock_group_xor_launches(),
                compact=L.qzstd_mock_compact_launches(), unxor=L.qzstd_mock_ungroup_xor_launches(), dev=fr.stats(), delta=fr.delta_stats(),
                group=fr.byte_group_stats(), skip=fr.delta_skip_stats(), restore=fr.restore_stats())


def pad16(n):
    return (n + 15) & ~15


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
def test_skip_on_and_off_compress_and_restore(skipmock, zstd, monkeypatch, checksum):
    plug, F = skipmock
    datas, bases = corpus()
    eq = equal_map(datas, bases, BASED, CHUNK)
    lens = [[min(CHUNK, n - o) for o in range(0, n, CHUNK)] for n in SIZES]
    n_frames = sum(len(x) for x in lens)
    n_based = sum(len(x) for x, on in zip(lens, BASED) if on)
    n_equal = sum(sum(x) for x in eq)
    assert {n for ls, es in zip(lens, eq) for n, e in zip(ls, es) if e} == {1, 255, 256, 65791, 65792, CHUNK, 9}
    assert not any(eq[5]) and datas[5] == bytes(SIZES[5])
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(2 * CHUNK))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_checksum(checksum) == 0
        assert fr.get_delta_skip() == 0 and fr.delta_skip_stats() == [0, 0, 0, 0]
        src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))], slot=0)
        bas = T.Pool(plug, bases, [(7, 0, 2, 9, 15, 4)[i % 6] for i in range(len(datas))], slot=1)
        given = [b if on else None for b, on in zip(bas.bufs, BASED)]
        # ---- off: today's frames, no comparison
        c0 = counters(plug, fr)
        off = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        c1 = counters(plug, fr)
        assert c1["diff"] == c0["diff"] and c1["skip"] == [0, 0, 0, 0]
        # ---- on
        assert fr.set_delta_skip(True) == 0 and fr.get_delta_skip() == 1
        on = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        c2 = counters(plug, fr)
        assert [len(x) for x in on] == [len(x) for x in lens]
        for i in range(len(BUFS)):
            for c, (n, e) in enumerate(zip(lens[i], eq[i])):
                if e:
                    assert on[i][c] == canonical(plug, n, checksum), (i, c)
                    assert zstd.decompress(on[i][c], CHUNK) == bytes(n), (i, c)  # (with a checksum: libzstd verifies it)
                else:
                    assert on[i][c] == off[i][c], (i, c)
        assert on[5] == off[5] and all(f != canonical(plug, n, checksum) for f, n in zip(on[5], lens[5]))  # zeros without a base
        assert c2["diff"] == c1["diff"] + 1 and c2["rows"] == c1["rows"] + n_based
        assert c2["skip"] == [n_based, n_equal, sum(n for n, on_ in zip(SIZES, BASED) if on_), 0]
        assert c2["dev"][3] - c1["dev"][3] == sum(SIZES) == c1["dev"][3] - c0["dev"][3]
        assert sum(c2["dev"][:2]) - sum(c1["dev"][:2]) == n_frames - n_equal and sum(c1["dev"][:2]) - sum(c0["dev"][:2]) == n_frames
        assert sum(c2["delta"][:3]) - sum(c1["delta"][:3]) == n_based - n_equal
        grouped = lambda skip: sum(1 for i, k in enumerate(ELEMS) if k > 1 for e in eq[i] if not (skip and e))  # noqa: E731
        assert sum(c2["group"]) - sum(c1["group"]) == grouped(True) and sum(c1["group"]) - sum(c0["group"]) == grouped(False)
        assert c2["dev"][2] - c1["dev"][2] < c1["dev"][2] - c0["dev"][2]
        assert all(C.string_at(p, n) == b for (p, n), b in zip(bas.bufs, bases)) and all(C.string_at(p, n) == d for (p, n), d in zip(src.bufs, datas))
        # ---- restore, setting on: into fresh buffers ...
        decoded = [n for ls, es in zip(lens, eq) for n, e in zip(ls, es) if not e]
        out = R.OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11)[i] for i in range(len(SIZES))], slot=3)
        assert fr.restore_batch_delta(on, out.bufs, given, ELEMS) == n_frames
        c3 = counters(plug, fr)
        assert out.bytes() == out.expected(datas)
        assert c3["restore"][0] - c2["restore"][0] == len(decoded) and c3["restore"][1] - c2["restore"][1] == sum(decoded)
        assert c3["restore"][2] - c2["restore"][2] == sum(pad16(n) for n in decoded)
        assert c3["skip"][3] - c2["skip"][3] == n_equal and c3["skip"][:3] == c2["skip"][:3]
        assert c3["delta"][3] - c2["delta"][3] == n_based - n_equal
        # ... and in place over a copy of the bases
        inp = T.Pool(plug, bases, [(2, 9, 0, 4, 15, 7)[i % 6] for i in range(len(datas))], slot=4)
        assert fr.restore_batch_delta(on, inp.bufs, [b if on_ else None for b, on_ in zip(inp.bufs, BASED)], ELEMS, compact=True) == n_frames
        c4 = counters(plug, fr)
        assert all(C.string_at(p, n) == d for (p, n), d in zip(inp.bufs, datas))
        assert [c4["restore"][k] - c3["restore"][k] for k in range(3)] == [len(decoded), sum(decoded), sum(pad16(n) for n in decoded)]
        assert c4["skip"][3] - c3["skip"][3] == n_equal
        # ---- restore, setting off: the zero frames are ordinary frames
        assert fr.set_delta_skip(False) == 0
        out2 = R.OutPool(plug, SIZES, [5] * len(SIZES), slot=3)
        assert fr.restore_batch_delta(on, out2.bufs, given, ELEMS) == n_frames
        c5 = counters(plug, fr)
        assert out2.bytes() == out2.expected(datas)
        assert c5["restore"][0] - c4["restore"][0] == n_frames and c5["skip"] == c4["skip"]
        # the Typed restore (out of scope for the recognition) reads a zero frame as the frame of zeros it is
        out3 = R.OutPool(plug, SIZES[:1], [1], slot=3)
        assert fr.restore_batch(on[:1], out3.bufs, ELEMS[:1]) == len(on[0]) and out3.bytes() == out3.expected([bytes(SIZES[0])])
    finally:
        fr.close()


def test_all_frames_equal_queues_nothing(skipmock, zstd):
    """every frame of the call equals its base: no staging, no match-finder launch, no compaction, no arena copy, no job — and on the way back
    no part either: in place nothing at all happens, into fresh buffers one copy per buffer"""
    plug, F = skipmock
    datas, bases = corpus()
    keep = [i for i, b in enumerate(BUFS) if b[2] and b[3] == "none"]
    datas, elems = [datas[i] for i in keep], [ELEMS[i] for i in keep]
    lens = [min(CHUNK, len(d) - o) for d in datas for o in range(0, len(d), CHUNK)]
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        assert fr.set_delta_skip(1) == 0
        src = T.Pool(plug, datas, [3] * len(datas), slot=0)
        bas = T.Pool(plug, datas, [8] * len(datas), slot=1)
        c0 = counters(plug, fr)
        frames = fr.compress_device_batch_delta(src.bufs, bas.bufs, elems)
        c1 = counters(plug, fr)
        assert [f for per in frames for f in per] == [canonical(plug, n, False) for n in lens]
        assert (c1["find"], c1["xor"], c1["compact"]) == (c0["find"], c0["xor"], c0["compact"])
        assert c1["dev"][:3] == c0["dev"][:3] and c1["dev"][3] == c0["dev"][3] + sum(len(d) for d in datas)
        assert c1["delta"] == c0["delta"] and c1["group"] == c0["group"]
        assert c1["diff"] == c0["diff"] + 1 and c1["skip"] == [len(lens), len(lens), sum(lens), 0]
        # a == b (the base IS the buffer) is equal too
        assert fr.compress_device_batch_delta(src.bufs, src.bufs, elems) == frames
        out = R.OutPool(plug, [len(d) for d in datas], [7] * len(datas), slot=2)
        c2 = counters(plug, fr)
        assert fr.restore_batch_delta(frames, out.bufs, bas.bufs, elems) == len(lens)
        assert out.bytes() == out.expected(datas)
        before = C.string_at(bas.bufs[0][0] - 64, 128 + len(datas[0]))
        assert fr.restore_batch_delta(frames, bas.bufs, bas.bufs, elems) == len(lens)
        c3 = counters(plug, fr)
        assert C.string_at(bas.bufs[0][0] - 64, 128 + len(datas[0])) == before
        assert c3["restore"] == c2["restore"] and c3["unxor"] == c2["unxor"] and c3["skip"][3] == c2["skip"][3] + 2 * len(lens)
    finally:
        fr.close()


def test_a_chunk_of_two_blocks_and_a_tail(skipmock, zstd):
    """chunk size 256 KiB + 3: the zero frame of a full chunk has two 128 KiB RLE blocks and one of 3 bytes"""
    plug, F = skipmock
    import numpy as np
    d0 = D.typed_corpus("bf16", BIG + 10, 5)
    d1 = D.typed_corpus("fp32", BIG, 6)
    b1 = np.frombuffer(d1, dtype=np.uint8).copy()
    b1[BIG // 2] ^= 0x10
    for checksum in (False, True):
        fr = D.DeviceFront(2, 1, BIG, lib=F)
        try:
            assert fr.set_checksum(checksum) == 0 and fr.set_delta_skip(1) == 0
            src = T.Pool(plug, [d0, d1], [5, 0], slot=0)
            bas = T.Pool(plug, [d0, b1.tobytes()], [0, 9], slot=1)
            frames = fr.compress_device_batch_delta(src.bufs, bas.bufs, [2, 4])
            assert frames[0] == [canonical(plug, BIG, checksum), canonical(plug, 10, checksum)]
            assert len(frames[0][0]) == 4 + 1 + 4 + 3 * 4 + (4 if checksum else 0)
            assert zstd.decompress(frames[0][0], BIG) == bytes(BIG)
            assert fr.set_delta_skip(0) == 0
            assert fr.compress_device_batch_delta(src.bufs, bas.bufs, [2, 4])[1] == frames[1]
            assert fr.set_delta_skip(1) == 0
            out = R.OutPool(plug, [BIG + 10, BIG], [3, 6], slot=2)
            assert fr.restore_batch_delta(frames, out.bufs, bas.bufs, [2, 4]) == 3
            assert out.bytes() == out.expected([d0, d1])
            assert fr.delta_skip_stats() == [3, 2, 2 * BIG + 10, 2] and fr.restore_stats()[0] == 1
        finally:
            fr.close()


def test_refusals_and_the_setting(skipmock):
    plug, F = skipmock
    assert F.QZSTD_frontSetDeltaSkip(None, 1) == -1 and F.QZSTD_frontGetDeltaSkip(None) == 0
    st = (C.c_ulonglong * 4)(9, 9, 9, 9)
    F.QZSTD_frontDeltaSkipStats(None, st)
    assert list(st) == [0, 0, 0, 0]
    F.QZSTD_frontDeltaSkipStats(None, None)
    # the comparison's own refusals, before anything is touched
    D.bind_diff_kernel(plug.lib)
    a = C.create_string_buffer(64)
    rows = (D.DiffRow * 2)()
    d_rows = (D.DiffRow * 2)()
    flags = (C.c_uint32 * 4)(7, 7, 7, 7)
    rows[0].a, rows[0].b, rows[0].len, rows[0].tile0 = C.addressof(a), C.addressof(a) + 32, 20, 99
    rows[1].a, rows[1].b, rows[1].len, rows[1].tile0 = 0, 0, 0, 99
    L = plug.lib
    assert L.qzstd_hip_diff(0, None, None, 2, d_rows, flags) < 0 and L.qzstd_hip_diff(0, None, rows, 2, None, flags) < 0
    assert L.qzstd_hip_diff(0, None, rows, 2, d_rows, None) < 0
    rows[1].len = 1
    assert L.qzstd_hip_diff(0, None, rows, 2, d_rows, flags) < 0
    rows[1].a, rows[1].b, rows[1].len = C.addressof(a), C.addressof(a), 0xFFFFFFE1
    assert L.qzstd_hip_diff(0, None, rows, 2, d_rows, flags) < 0
    assert [r.tile0 for r in rows] == [99, 99] and list(flags) == [7, 7, 7, 7]
    assert L.qzstd_hip_diff(0, None, rows, 0, d_rows, flags) == 0 and list(flags) == [7, 7, 7, 7]
    rows[1].len = 0
    a[40] = b"\x01"
    assert L.qzstd_hip_diff(0, None, rows, 2, d_rows, flags) == 0
    assert list(flags) == [1, 0, 7, 7] and [r.tile0 for r in rows] == [0, 1]


def test_device_layer_without_the_diff_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the comparison's stand-in: the delta compress call with the setting on and a base returns
    (size_t)-1 with no launch, no event wait and nothing counted; with the setting off, or without a base, the same library serves it (a
    process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NODIFF_MOCK_SO, NODIFF_FRONT_SO, diff=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [data], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
off = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2])
assert fr.set_delta_skip(1) == 0
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_group_xor_launches(), fr.stats(), fr.delta_stats(), fr.delta_skip_stats())
before = state()
r1 = fr.compress_device_batch_delta_raw(pool.bufs, bas.bufs, [2])[0]
nothing = state() == before
no_base = fr.compress_device_batch_delta(pool.bufs, None, [2]) == fr.compress_device_batch_typed(pool.bufs, [2])
assert fr.set_delta_skip(0) == 0
served = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2]) == off
out = R.OutPool(plug, [len(data)], [3], slot=2)
assert fr.set_delta_skip(1) == 0
back = fr.restore_batch_delta(off, out.bufs, bas.bufs, [2]) == len(off[0]) and out.bytes() == out.expected([data])
print(json.dumps({"refused": r1 == D.ERROR, "nothing_queued": nothing, "no_base": no_base, "served_off": served, "restore": back,
                  "has_diff": hasattr(plug.lib, "qzstd_hip_diff")}))
""", NODIFF_MOCK_SO, NODIFF_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "no_base": True, "served_off": True, "restore": True, "has_diff": False}, res
