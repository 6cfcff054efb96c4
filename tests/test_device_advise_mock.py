"""CPU: the adviser (QZSTD_frontAdviseDeviceBatch / QZSTD_frontAdviseStats / QZSTD_ediffCostOf / QZSTD_ediffAdvisedOf:
include/qzstd_frontend_device.h) over the mock device layer — the mock pair of tests/test_device_ediff_mock.py plus
tests/mock/mock_hip_ediff_cost.c (the launcher's checks and include/qzstd_ediffcost.h's tile function in plain C).  Buffers of sizes 0, k - 1,
256, 65791, 100003, 128 KiB + 255 and 2 - 3 chunks with odd tails at odd addresses, element sizes 1 / 2 / 4 / 8, ordered columns and data
without order: est is QZSTD_ediffCostOf summed over each buffer's chunks; advised is the resolved element size with QZSTD_ELEM_DIFF exactly
where QZSTD_ediffAdvisedOf holds, and goes as it is through the Typed compress and restore calls, byte for byte; exactly one launch per
call, none for input without an element; every refusal leaves every counter as it was; a device layer without the entry point refuses
the call and serves the others.  Every comparison is exact."""
import ctypes as C
import os

import pytest

import qz_device as D
import test_device_checksum_mock as T
import test_device_ediff_mock as ED
import test_device_restore_mock as R
import test_device_slices_mock as S

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_advisemock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_advisemock.so")
OLD_MOCK_SO = os.path.join(MOCK, "libqatseqprod_noadvisemock.so")
OLD_FRONT_SO = os.path.join(MOCK, "libqzstdfront_noadvisemock.so")
CHUNK = ED.CHUNK
# (size, element size or 0 for the front's setting, content)
BUFS = (
    (2 * CHUNK + 1, 2, "column"),
    (CHUNK + 255, 1, "text"),
    (256, 4, "column"),
    (0, 8, "column"),
    (7, 8, "column"),         # shorter than its element: no tile, never flagged
    (65791, 0, "column"),     # the front's setting (4)
    (100003, 8, "column"),
    (3 * CHUNK + 9, 4, "ids32"),
    (2 * CHUNK + 100, 2, "bf16"),
    (3, 4, "column"),
    (CHUNK, 8, "zeros"),      # P == D == 0: off is the default
)
FRONT_GROUP = 4
SIZES = tuple(b[0] for b in BUFS)
GIVEN = tuple(b[1] for b in BUFS)
ELEMS = tuple(b[1] or FRONT_GROUP for b in BUFS)
OFFSETS = tuple((1, 3, 15, 0, 5, 7, 9)[i % 7] for i in range(len(BUFS)))


def build_pair(zstd_path, mock_so, front_so, advise: bool):
    """the element-difference test's mock pair, with the cost kernel's stand-in or — an older device layer — without"""
    import subprocess

    import qz_bind as B
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_elemdiff.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_fingerprint.c", "mock_hip_plane_cost.c",
                                             "mock_hip_group_ediff.c", "mock_hip_esum.c")]
    if advise:
        srcs.append(os.path.join(MOCK, "mock_hip_ediff_cost.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def load(zstd_path, mock_so, front_so, advise):
    build_pair(zstd_path, mock_so, front_so, advise)
    plug, F = T.load_pair(mock_so, front_so)
    D.bind(F)
    D.bind_elemdiff(F)
    S.bind_hooks(plug)
    if advise:
        for n in ("qzstd_mock_ediff_cost_rows", "qzstd_mock_ediff_cost_tiles"):
            getattr(plug.lib, n).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def mock(oracle, zstd):
    return load(zstd.path, MOCK_SO, FRONT_SO, True)


@pytest.fixture(scope="module")
def batch():
    """the buffers' bytes, computed once and never changed"""
    out = []
    for i, (n, _, kind) in enumerate(BUFS):
        if kind == "column":
            out.append(ED.column(n, ELEMS[i], 90 + i))
        elif kind == "zeros":
            out.append(bytes(n))
        elif kind == "text":
            import qz_corpus as K
            out.append(K.by_name("text", n, seed=3))
        else:
            out.append(D.typed_corpus(kind, n, 5 + i))
    return out


def mem(buf):
    return C.string_at(buf[0], buf[1])


def counters(plug):
    L = plug.lib
    return (L.qzstd_mock_ediff_cost_launches(), L.qzstd_mock_ediff_cost_rows(), L.qzstd_mock_ediff_cost_tiles(), L.qzstd_mock_event_waits())


def all_stats(fr):
    return (fr.advise_stats(), fr.stats(), fr.restore_stats(), fr.elem_diff_stats(), fr.fingerprint_stats(), fr.verify_stats(), fr.slice_stats())


def expected(F, batch):
    est = [D.ediff_cost(d, k, CHUNK, lib=F) for d, k in zip(batch, ELEMS)]
    adv = [k | (D.ELEM_DIFF if D.ediff_advised(p, dd, lib=F) else 0) for k, (p, dd) in zip(ELEMS, est)]
    return est, adv


def test_estimates_advice_one_launch_and_the_round_trip(mock, batch, zstd):
    plug, F = mock
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_byte_group(FRONT_GROUP) == 0
        src = T.Pool(plug, batch, OFFSETS, slot=0)
        est_want, adv_want = expected(F, batch)
        before = counters(plug)
        assert fr.advise_stats() == [0, 0, 0, 0]
        r, adv, est = fr.advise_raw(src.bufs, GIVEN)
        after = counters(plug)
        assert est == est_want and adv == adv_want and r == sum(1 for a in adv if a & D.ELEM_DIFF)
        # the rule, restated: D + (D >> shift) < P, and never for P == D
        for (p, dd), a in zip(est, adv):
            assert bool(a & D.ELEM_DIFF) == bool(D.ediff_advised(p, dd, lib=F)) and not (p == dd and a & D.ELEM_DIFF)
        flagged = {i for i, a in enumerate(adv) if a & D.ELEM_DIFF}
        assert {0, 6} <= flagged and not flagged & {1, 3, 4, 7, 8, 9, 10}  # the long ordered columns; never text, noise, Zipf ids, zeros or no element
        assert est[10] == (0, 0) and est[3] == est[4] == est[9] == (0, 0)
        # exactly one launch, a row per chunk, a tile per 16 KiB of elements; one wait for the caller's stream
        rows = sum(-(-n // CHUNK) for n in SIZES)
        tiles = sum(D.esum_tiles(len(d[o:o + CHUNK]), k) for d, k in zip(batch, ELEMS) for o in range(0, len(d), CHUNK))
        assert [a - b for a, b in zip(after, before)] == [1, rows, tiles, 1]
        assert fr.advise_stats() == [len(BUFS), len(flagged), sum(n // k * k for n, k in zip(SIZES, ELEMS)), 1]
        assert all(mem(b) == d for b, d in zip(src.bufs, batch))  # only read
        # est is optional; the front's setting resolves entries of 0 and a NULL array
        r2, adv2, none = fr.advise_raw(src.bufs, GIVEN, want_est=False)
        assert (r2, adv2, none) == (r, adv, None)
        r3, adv3, est3 = fr.advise_raw(src.bufs[5:6], None)
        assert adv3 == [adv[5]] and est3 == [est[5]] and adv3[0] & 0x7F == FRONT_GROUP
        # the array as it is through the Typed calls, and byte for byte back
        frames = fr.compress_device_batch_typed(src.bufs, adv)
        assert fr.elem_diff_stats()[0] == sum(-(-SIZES[i] // CHUNK) for i in flagged)
        ED.check_content(zstd, F, frames, batch, adv)
        out = R.OutPool(plug, SIZES, [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11, 4)[i] for i in range(len(SIZES))], slot=3)
        assert fr.restore_batch(frames, out.bufs, adv) == rows
        assert [mem(b) for b in out.bufs] == list(batch)
        # where differences are advised the frames are smaller than without, where not they are what they were
        plain = fr.compress_device_batch_typed(src.bufs, ELEMS)
        for i in range(len(BUFS)):
            if i in flagged and SIZES[i] >= 65536:
                assert sum(map(len, frames[i])) < sum(map(len, plain[i])), i
            elif i not in flagged:
                assert frames[i] == plain[i], i
    finally:
        fr.close()


def test_input_without_an_element_touches_no_gpu(mock, batch):
    plug, F = mock
    fr = D.DeviceFront(2, 1, CHUNK, use_producer=0, lib=F)  # (accepted without the producer, like the fingerprint calls)
    try:
        src = T.Pool(plug, batch, OFFSETS, slot=0)
        before = counters(plug)
        assert fr.advise_raw([], None) == (0, [], [])
        short = [src.bufs[3], src.bufs[4], src.bufs[9], (0, 0)]
        r, adv, est = fr.advise_raw(short, [8, 8, 4, 0])
        assert (r, adv, est) == (0, [8, 8, 4, 1], [(0, 0)] * 4)  # (this front's setting is 1)
        assert counters(plug) == before and fr.advise_stats()[1:] == [0, 0, 0]
        # and the same front serves a call with elements
        r, adv, est = fr.advise_raw(src.bufs, ELEMS)
        assert (est, adv) == expected(F, batch) and counters(plug)[0] == before[0] + 1
    finally:
        fr.close()


def test_refusals_leave_every_counter_unchanged(mock, batch):
    plug, F = mock
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, OFFSETS, slot=0)
        fr.advise(src.bufs, ELEMS)
        before, st = counters(plug), all_stats(fr)
        for bad in (0x80, 0x81, 0x82, 0x84, 0x88, 3, 5, 16, 0xFF):  # flagged already, or no element size
            es = list(ELEMS)
            es[2] = bad
            r, adv, _ = fr.advise_raw(src.bufs, es)
            assert r == D.ERROR and set(adv) == {7}, bad
        assert fr.advise_raw(src.bufs, ELEMS, null_advised=True)[0] == D.ERROR
        assert fr.advise_raw(src.bufs[:3] + [(0, 5)], ELEMS[:4])[0] == D.ERROR                      # a null pointer with a size
        host = C.create_string_buffer(4096)
        assert fr.advise_raw(src.bufs[:3] + [(C.addressof(host), 4096)], ELEMS[:4])[0] == D.ERROR  # host memory
        other = T.Pool(plug, batch[:1], [0], slot=1, dev=1)
        assert fr.advise_raw(src.bufs[:2] + other.bufs, ELEMS[:3])[0] == D.ERROR                   # two devices
        assert F.QZSTD_frontAdviseDeviceBatch(None, None, None, 0, None, None, None) == D.ERROR
        assert F.QZSTD_frontAdviseDeviceBatch(fr.f, None, None, 2, None, C.create_string_buffer(2), None) == D.ERROR
        assert counters(plug) == before and all_stats(fr) == st
        stats = (C.c_ulonglong * 4)(9, 9, 9, 9)
        F.QZSTD_frontAdviseStats(None, stats)
        assert list(stats) == [0, 0, 0, 0]
        F.QZSTD_frontAdviseStats(None, None)
        # the exports: a NULL chunk without bytes, a bad k
        assert D.ediff_cost_of(b"", 4, lib=F) == (0, 0) and D.ediff_cost_of(b"abcdefgh", 3, lib=F) == (0, 0)
        s = (C.c_ulonglong * 2)(5, 5)
        F.QZSTD_ediffCostOf(None, 100, 4, s)
        assert list(s) == [0, 0]
        assert not D.ediff_advised(0, 0, lib=F) and not D.ediff_advised(10, 10, lib=F) and D.ediff_advised(10, 0, lib=F)
    finally:
        fr.close()
    # the launcher's own refusals, before anything is touched
    L = D.bind_ediff_cost_kernel(plug.lib)
    a = C.create_string_buffer(40000)
    rows, d_rows = (D.EdiffCostRow * 2)(), (D.EdiffCostRow * 2)()
    tiles = (C.c_uint32 * 12)(*([7] * 12))

    def setrow(r, src, ln, elem, reserved=0):
        r.src, r.len, r.elem, r.tile0, r.reserved = src, ln, elem, 99, reserved

    base = C.addressof(a)
    setrow(rows[0], base + 3, 20000, 2)
    setrow(rows[1], 0, 0, 4)
    call = lambda r=rows, n=2, dr=d_rows, t=tiles: L.qzstd_hip_ediff_cost(0, None, r, n, dr, t)  # noqa: E731
    assert call(r=None) < 0 and call(dr=None) < 0 and call(t=None) < 0
    assert call(t=C.addressof(tiles) + 4) < 0                 # the 8-byte store
    setrow(rows[1], 0, 4, 4)
    assert call() < 0                                         # a null src with an element
    setrow(rows[1], 0, 3, 4)
    for elem, reserved in ((3, 0), (0, 0), (16, 0), (4, 1)):
        setrow(rows[0], base + 3, 20000, elem, reserved)
        assert call() < 0, (elem, reserved)
    setrow(rows[0], base, 0xFFFFFFE1, 1)
    assert call() < 0
    assert [r.tile0 for r in rows] == [99, 99] and list(tiles) == [7] * 12
    assert call(n=0) == 0 and list(tiles) == [7] * 12
    setrow(rows[0], base + 3, 20000, 2)                       # (a null src without an element is fine)
    assert call() == 0 and [r.tile0 for r in rows] == [0, 2] and list(tiles)[4:] == [7] * 8
    raw = a.raw
    assert D.ediff_cost_of(raw[3:20003], 2, lib=F) == (tiles[0] + tiles[2], tiles[1] + tiles[3])


def test_device_layer_without_the_entry_point(zstd, oracle, batch):
    plug, F = load(zstd.path, OLD_MOCK_SO, OLD_FRONT_SO, False)
    assert not hasattr(plug.lib, "qzstd_hip_ediff_cost") and hasattr(F, "QZSTD_frontAdviseDeviceBatch")
    fr = D.DeviceFront(2, 1, CHUNK, lib=F)
    try:
        src = T.Pool(plug, batch, OFFSETS, slot=0)
        st, waits = all_stats(fr), plug.lib.qzstd_mock_event_waits()
        assert fr.advise_raw(src.bufs, ELEMS)[0] == D.ERROR and fr.advise_raw([], None)[0] == D.ERROR
        assert all_stats(fr) == st and plug.lib.qzstd_mock_event_waits() == waits
        # every other call is served: flags chosen by the header's rule on the host, compress, restore, fingerprints
        _, adv = expected(F, batch)
        frames = fr.compress_device_batch_typed(src.bufs, adv)
        out = R.OutPool(plug, SIZES, [1] * len(SIZES), slot=3)
        assert fr.restore_batch(frames, out.bufs, adv) == sum(map(len, frames)) and [mem(b) for b in out.bufs] == list(batch)
        assert fr.check(out.bufs, fr.fingerprint(src.bufs)) == []
    finally:
        fr.close()
