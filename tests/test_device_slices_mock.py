"""CPU: QZSTD_frontRestoreDeviceSlices / QZSTD_frontSliceStats (include/qzstd_frontend_device.h) over the mock device layer — the mock pair of
tests/test_device_delta_mock.py plus tests/mock/mock_hip_ungroup_window.c (the windowed scatter in plain C).  What the delta compress call
wrote must come back slice by slice: one odd-placed slice per buffer onto the bases' matching slices, the same in place, a column shard of
two matrices as 96 slices each, slices that cover everything (the Delta restore's bytes), empty slices only.  Only the frames a non-empty
slice intersects are decoded — the others may hold garbage —, every refusal happens before anything is queued (the mock's counters), and
the existing calls launch no window rows.  Every comparison is byte-exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D
import test_device_checksum_mock as T
import test_device_delta_mock as M
import test_device_restore_mock as R

ROOT = T.ROOT
MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_slicesmock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_slicesmock.so")
NOWIN_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nowindowmock.so")
NOWIN_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nowindowmock.so")
CHUNK = M.CHUNK
MAT_R, MAT_C = 96, 4096  # the two matrices of the column shard: bf16 (with a base) and fp32 (without)
SIZES = M.SIZES + (MAT_R * MAT_C * 2, MAT_R * MAT_C * 4)
ELEMS = M.ELEMS + (2, 4)
BASED = tuple(i % 3 != 2 for i in range(len(SIZES)))
MATS = (len(M.SIZES), len(M.SIZES) + 1)


def build_pair(zstd_path, mock_so, front_so, window: bool):
    """the delta test's mock pair (group, ungroup, both XOR stand-ins, fail-block), with the windowed scatter's stand-in or — an older device
    layer — without"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c")]
    if window:
        srcs.append(os.path.join(MOCK, "mock_hip_ungroup_window.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


def bind_hooks(plug):
    M.bind_hooks(plug)
    if hasattr(plug.lib, "qzstd_mock_ungroup_window_rows"):
        plug.lib.qzstd_mock_ungroup_window_rows.restype = C.c_ulonglong
    return plug


def corpus(sizes=SIZES):
    """the delta test's buffers and bases, and behind them the two matrices with a base that differs in few bits"""
    datas, bases = M.corpus()
    for j, (kind, n) in enumerate(zip(("bf16", "fp32"), sizes[len(M.SIZES):])):
        d = D.typed_corpus(kind, n, 75 + j)
        flips = (np.random.default_rng(20 + j).random(n) < 0.2) * np.random.default_rng(30 + j).integers(0, 8, n)
        datas.append(d)
        bases.append((np.frombuffer(d, dtype=np.uint8) ^ flips.astype(np.uint8)).tobytes())
    return datas, bases


# ---- the slicing, worked out from the sizes alone (tests/test_gpu_device_slices.py uses these too)
def frames_of(sizes, chunk):
    return sum(-(-n // chunk) for n in sizes)


def touched(sizes, chunk, slices):
    """the frames (buffer, chunk index) that intersect a non-empty slice"""
    return {(b, c) for b, off, n in slices if n for c in range(off // chunk, (off + n - 1) // chunk + 1)}


def pieces(chunk, slices):
    """rows the call launches: a piece per (non-empty slice, frame it intersects)"""
    return sum((off + n - 1) // chunk - off // chunk + 1 for _, off, n in slices if n)


def odd_slices(sizes):
    """(a): per buffer (size / 3 rounded to an odd number, size / 2), kept inside the buffer"""
    out = []
    for b, n in enumerate(sizes):
        off = min((n // 3) | 1, n)
        out.append((b, off, min(n // 2, n - off)))
    return out


def column_slices(buf, rows, cols, item, c0, c1):
    """(c): columns [c0, c1) of a [rows, cols] matrix of `item`-byte elements: a slice per row"""
    return [(buf, (r * cols + c0) * item, (c1 - c0) * item) for r in range(rows)]


def whole_slices(sizes):
    return [(b, 0, n) for b, n in enumerate(sizes)]


def expected(datas, slices):
    return [datas[b][off:off + n] for b, off, n in slices]


def give(slices, dsts, base_bufs, in_place=False):
    """-> the call's slice list: destinations `dsts` [(address, size)] in slice order, bases the matching slices of base_bufs (None: no base)"""
    out = []
    for (b, off, n), (p, _) in zip(slices, dsts):
        base = None if base_bufs[b] is None else (p if in_place else base_bufs[b][0] + off)
        out.append((b, off, n, p, base))
    return out


def counters(plug, fr):
    L = plug.lib
    return (M.launches(plug), L.qzstd_mock_ungroup_window_launches(), L.qzstd_mock_ungroup_window_rows(), L.qzstd_mock_ungroup_xor_rows(),
            L.qzstd_mock_ungroup_rows(), fr.stats(), fr.delta_stats(), fr.restore_stats(), fr.slice_stats())


@pytest.fixture(scope="module")
def slicesmock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, window=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    return bind_hooks(plug), F


@pytest.fixture(scope="module", params=(False, True), ids=("plain", "checksum"))
def written(slicesmock, request):
    """compressed ONCE per setting with the delta call: (front, datas, bases, the pools, per buffer its base or None, the frames)"""
    plug, F = slicesmock
    datas, bases = corpus()
    os.environ["QZSTD_FRONT_DEVICE_PART"] = str(4 * CHUNK)
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    assert fr.set_checksum(request.param) == 0
    src, bas, pre, given = M.pools(plug, datas, bases, BASED)
    frames = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
    assert all(T.flagged(f) == request.param for per in frames for f in per)
    yield fr, datas, bases, (src, bas, pre), given, frames
    fr.close()
    del os.environ["QZSTD_FRONT_DEVICE_PART"]


def check_call(plug, fr, frames, slices, out, given, want, in_place=False, compact=False):
    """one slices call into the OutPool `out` (a buffer per slice): the return value, the counters, the bytes, the guards"""
    need = touched(SIZES, CHUNK, slices)
    before = counters(plug, fr)
    r = fr.restore_slices(frames, SIZES, ELEMS, give(slices, out.bufs, given, in_place), compact=compact)
    after = counters(plug, fr)
    assert r == len(need)
    assert out.bytes() == out.expected(want)
    s0, s1 = before[-1], after[-1]
    assert [b - a for a, b in zip(s0, s1)] == [sum(1 for s in slices if s[2]), sum(s[2] for s in slices), len(need), pieces(CHUNK, slices)]
    assert after[2] - before[2] == pieces(CHUNK, slices)
    assert after[7][0] - before[7][0] == len(need) and after[7][3] - before[7][3] == after[1] - before[1]
    assert after[6][3] - before[6][3] == sum(1 for b, c in need if given[b] is not None)
    assert after[3] == before[3] and after[4] == before[4]  # no row of the whole-frame kernels
    return r


@pytest.mark.parametrize("compact", (False, True))
def test_one_odd_slice_per_buffer_fresh_and_in_place(slicesmock, written, compact):
    plug, F = slicesmock
    fr, datas, bases, _, given, frames = written
    slices = odd_slices(SIZES)
    want = expected(datas, slices)
    # (a) fresh destinations with guards, the bases' matching slices
    out = R.OutPool(plug, [n for _, _, n in slices], [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11, 9, 4)[i] for i in range(len(slices))], slot=3)
    r = check_call(plug, fr, frames, slices, out, given, want, compact=compact)
    assert r < frames_of(SIZES, CHUNK)
    # (b) in place over a copy of the base slices
    out = R.OutPool(plug, [n for _, _, n in slices], [(5, 1, 0, 2, 15, 7, 3, 9, 0, 6, 1, 13)[i] for i in range(len(slices))], slot=3)
    for (p, n), (b, off, _) in zip(out.bufs, slices):
        C.memmove(p, bases[b][off:off + n], n)
    check_call(plug, fr, frames, slices, out, given, want, in_place=True, compact=compact)


def test_column_shard_of_two_matrices(slicesmock, written):
    """(c): columns [3 C / 8, 4 C / 8) as 96 slices per matrix, each matrix into ONE contiguous [R, C / 8] destination"""
    plug, F = slicesmock
    fr, datas, bases, (src, bas, pre), given, frames = written
    c0, c1 = MAT_C // 8 * 3, MAT_C // 8 * 4
    slices = [s for m, item in zip(MATS, (2, 4)) for s in column_slices(m, MAT_R, MAT_C, item, c0, c1)]
    out = R.OutPool(plug, [MAT_R * (c1 - c0) * item for item in (2, 4)], [7, 3], slot=3)
    dsts = [(out.bufs[j][0] + r * (c1 - c0) * item, 0) for j, item in enumerate((2, 4)) for r in range(MAT_R)]
    # the torch-free half of the helper: the same slices
    for j, (m, item) in enumerate(zip(MATS, (2, 4))):
        mine = D.shard_slices(m, (MAT_R, MAT_C), item, 1, c0, c1 - c0, out.bufs[j][0])
        assert [(b, o, n, p) for b, o, n, p, _ in mine] == [(b, o, n, p) for (b, o, n), (p, _) in zip(slices[j * MAT_R:(j + 1) * MAT_R],
                                                                                                     dsts[j * MAT_R:(j + 1) * MAT_R])]
    need = touched(SIZES, CHUNK, slices)
    before = counters(plug, fr)
    r = fr.restore_slices(frames, SIZES, ELEMS, give(slices, dsts, given))
    after = counters(plug, fr)
    assert r == len(need) and r < frames_of(SIZES, CHUNK)
    want = []
    for m, item in zip(MATS, (2, 4)):
        a = np.frombuffer(datas[m], dtype=np.uint8).reshape(MAT_R, MAT_C * item)
        want.append(a[:, c0 * item:c1 * item].tobytes())
    assert out.bytes() == out.expected(want)
    assert after[-1][2] - before[-1][2] == len(need) and after[-1][3] - before[-1][3] == pieces(CHUNK, slices) == after[2] - before[2]
    assert after[-1][0] - before[-1][0] == 2 * MAT_R
    assert D.shard_slices(0, (4, 6), 2, 0, 1, 2, 1000, 2000) == [(0, 12, 24, 1000, 2000)]


def test_slices_that_cover_everything_are_the_delta_restore(slicesmock, written):
    """(d)"""
    plug, F = slicesmock
    fr, datas, bases, _, given, frames = written
    offs = [(3, 0, 1, 15, 8, 2, 7, 5, 0, 11, 6, 9)[i] for i in range(len(SIZES))]
    ref = R.OutPool(plug, SIZES, offs, slot=3)
    assert fr.restore_batch_delta(frames, ref.bufs, given, ELEMS) == frames_of(SIZES, CHUNK)
    assert ref.bytes() == ref.expected(datas)
    out = R.OutPool(plug, SIZES, offs, slot=4)
    r = check_call(plug, fr, frames, whole_slices(SIZES), out, given, datas)
    assert r == frames_of(SIZES, CHUNK) and out.bytes() == ref.bytes()


def test_empty_slices_only(slicesmock, written):
    """(e): 0, and no counter moves"""
    plug, F = slicesmock
    fr, datas, bases, _, given, frames = written
    out = R.OutPool(plug, [16], [0], slot=3)
    before = counters(plug, fr)
    for slices in ([], [(b, min(5, n), 0, out.bufs[0][0], None) for b, n in enumerate(SIZES)], [(1, 1, 0, 0, None)]):
        assert fr.restore_slices_raw(frames, SIZES, ELEMS, slices) == 0
    assert fr.restore_slices_raw(frames, SIZES, ELEMS, None) == 0
    assert counters(plug, fr) == before and out.untouched()


def test_frames_no_slice_needs_are_never_read_and_a_needed_one_is(slicesmock, written):
    plug, F = slicesmock
    fr, datas, bases, _, given, frames = written
    slices = odd_slices(SIZES)
    need = touched(SIZES, CHUNK, slices)
    want = expected(datas, slices)
    sizes = [n for _, _, n in slices]
    garbage = [[f if (b, c) in need else os.urandom(len(f)) for c, f in enumerate(per)] for b, per in enumerate(frames)]
    assert sum(len(p) for p in garbage) > len(need)
    for compact in (False, True):
        out = R.OutPool(plug, sizes, [3] * len(slices), slot=3)
        check_call(plug, fr, garbage, slices, out, given, want, compact=compact)
    # one needed frame damaged: its content, or cut short
    b, c = sorted(need)[len(need) // 2]
    for bad in (frames[b][c][:-3], frames[b][c][:8] + bytes(x ^ 0x5A for x in frames[b][c][8:])):
        broken = [list(per) for per in frames]
        broken[b][c] = bad
        out = R.OutPool(plug, sizes, [3] * len(slices), slot=3)
        assert fr.restore_slices_raw(broken, SIZES, ELEMS, give(slices, out.bufs, given)) == D.ERROR
        assert out.bytes()[:R.GUARD] == b"\xa5" * R.GUARD and out.bytes()[-R.GUARD:] == b"\xa5" * R.GUARD
    # and the front goes on working
    out = R.OutPool(plug, sizes, [3] * len(slices), slot=3)
    check_call(plug, fr, frames, slices, out, given, want)


def test_refusals_before_anything_is_queued(slicesmock, written):
    plug, F = slicesmock
    fr, datas, bases, (src, bas, pre), given, frames = written
    out = R.OutPool(plug, [4096, 4096], [3, 9], slot=3)
    other = T.Pool(plug, [b"\0" * 4096], [0], slot=5, dev=1)
    host = C.create_string_buffer(4096)
    d0, d1 = out.bufs[0][0], out.bufs[1][0]
    b6 = bas.bufs[6][0]
    n6 = SIZES[6]
    good = [(6, 100, 4096, d0, b6 + 100), (6, 50000, 4096, d1, b6 + 50000)]
    before = counters(plug, fr)
    bad = {
        "buf past nBufs": [(len(SIZES), 0, 16, d0, None)],
        "ends past its buffer": [(6, n6 - 10, 11, d0, None)],
        "offset past its buffer": [(6, n6 + 1, 0, d0, None)],
        "buffers out of order": [good[1], (5, 0, 16, d0, None)],
        "offsets out of order": [good[1], good[0]],
        "overlapping": [good[0], (6, 4195, 16, d1, None)],
        "an empty slice inside its predecessor": [good[0], (6, 200, 0, d1, None)],
        "null destination": [(6, 100, 4096, 0, None)],
        "destination in host memory": [(6, 100, 4096, C.addressof(host), None)],
        "destination ends behind the device memory": [(MATS[1], 0, (1 << 20) + 4321, d0, None)],
        "destinations on two devices": [good[0], (6, 50000, 4096, other.bufs[0][0], None)],
        "base in host memory": [(6, 100, 4096, d0, C.addressof(host))],
        "base on another device": [(6, 100, 4096, d0, other.bufs[0][0])],
        "base ends behind the device memory": [(6, 100, 4096, d0, bas.bufs[-1][0] + (1 << 30))],
    }
    for name, slices in bad.items():
        assert fr.restore_slices_raw(frames, SIZES, ELEMS, slices) == D.ERROR, name
    # what the Typed call refuses
    assert fr.restore_slices_raw(frames, SIZES, [3] + list(ELEMS[1:]), good) == D.ERROR
    assert fr.restore_slices_raw(frames, SIZES, ELEMS, good, n_frames=frames_of(SIZES, CHUNK) - 1) == D.ERROR
    assert fr.restore_slices_raw(frames, SIZES[:-1], ELEMS[:-1], good) == D.ERROR  # (nFrames no longer fits the sizes)
    arr = fr.slice_array(good)
    packed = fr.pack_frames([f for per in frames for f in per])
    n = frames_of(SIZES, CHUNK)
    assert fr.call_restore_slices(packed, n, None, ELEMS, arr, 2) == D.ERROR  # (nBufs 0: the slices' buffers do not exist, nFrames is wrong)
    assert fr.lib.QZSTD_frontRestoreDeviceSlices(fr.f, packed[0], packed[1], packed[2], n, (C.c_size_t * len(SIZES))(*SIZES), None, len(SIZES), None, 2,
                                                 None) == D.ERROR
    assert fr.lib.QZSTD_frontRestoreDeviceSlices(fr.f, packed[0], packed[1], packed[2], n, None, None, len(SIZES), arr, 2, None) == D.ERROR
    assert fr.lib.QZSTD_frontRestoreDeviceSlices(fr.f, None, packed[1], packed[2], n, (C.c_size_t * len(SIZES))(*SIZES), None, len(SIZES), arr, 2,
                                                 None) == D.ERROR
    assert fr.lib.QZSTD_frontRestoreDeviceSlices(None, None, 0, None, 0, None, None, 0, None, 0, None) == D.ERROR
    assert counters(plug, fr) == before and out.untouched()
    assert fr.restore_slices(frames, SIZES, ELEMS, good) == 2
    want = bytearray(b"\xa5" * out.size)
    want[out.place[0]:out.place[0] + 4096] = datas[6][100:4196]
    want[out.place[1]:out.place[1] + 4096] = datas[6][50000:54096]
    assert out.bytes() == bytes(want)


def test_a_call_while_another_one_runs_is_refused(slicesmock, written):
    import threading
    import time
    plug, F = slicesmock
    fr, datas, bases, _, given, frames = written
    slices = whole_slices(SIZES)
    out = R.OutPool(plug, SIZES, [0] * len(SIZES), slot=3)
    second = R.OutPool(plug, [64], [0], slot=4)
    got = {}
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    try:
        plug.lib.qzstd_mock_stall_ms(50000)  # every stream looks busy until released below: the first call waits for its slot's stream
        waits = plug.lib.qzstd_mock_event_waits()
        th = threading.Thread(target=lambda: got.update(r=fr.restore_slices_raw(frames, SIZES, ELEMS, give(slices, out.bufs, given))))
        th.start()
        deadline = time.monotonic() + 50
        seen = None
        while time.monotonic() < deadline:  # (the first call has queued its event pair and now waits for its slot's stream: it moves nothing more)
            if plug.lib.qzstd_mock_event_waits() == waits + 2 and fr.set_byte_group(1) != 0:
                before = counters(plug, fr)
                seen = fr.restore_slices_raw(frames, SIZES, ELEMS, [(6, 0, 64, second.bufs[0][0], None)])
                after = counters(plug, fr)
                break
        plug.lib.qzstd_mock_stall_ms(0)
        th.join(60)
        assert seen == D.ERROR and before == after and second.untouched()
        assert got["r"] == frames_of(SIZES, CHUNK) and out.bytes() == out.expected(datas)
    finally:
        plug.lib.qzstd_mock_stall_ms(0)


def test_a_front_without_the_producer_and_the_existing_calls(slicesmock, written):
    """useProducer = 0 is accepted; the Typed and Delta calls launch what they launched, and no window row"""
    plug, F = slicesmock
    fr, datas, bases, (src, bas, pre), given, frames = written
    slices = odd_slices(SIZES)
    f2 = D.DeviceFront(2, 1, CHUNK, use_producer=0, lib=F)
    try:
        out = R.OutPool(plug, [n for _, _, n in slices], [1] * len(slices), slot=3)
        assert f2.restore_slices(frames, SIZES, ELEMS, give(slices, out.bufs, given)) == len(touched(SIZES, CHUNK, slices))
        assert out.bytes() == out.expected(expected(datas, slices))
    finally:
        f2.close()
    L = plug.lib
    w0 = L.qzstd_mock_ungroup_window_launches(), L.qzstd_mock_ungroup_window_rows()
    l0, x0, u0 = M.launches(plug), L.qzstd_mock_ungroup_xor_rows(), L.qzstd_mock_ungroup_rows()
    again = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
    assert again == frames
    ref = R.OutPool(plug, SIZES, [2] * len(SIZES), slot=3)
    n = frames_of(SIZES, CHUNK)
    assert fr.restore_batch_delta(frames, ref.bufs, given, ELEMS) == n
    l1, x1, u1 = M.launches(plug), L.qzstd_mock_ungroup_xor_rows(), L.qzstd_mock_ungroup_rows()
    typed = fr.compress_device_batch_typed(pre.bufs, ELEMS)
    assert fr.restore_batch(typed, ref.bufs, ELEMS) == n
    l2, u2 = M.launches(plug), L.qzstd_mock_ungroup_rows()
    assert (L.qzstd_mock_ungroup_window_launches(), L.qzstd_mock_ungroup_window_rows()) == w0
    # every frame is a row of one of the two whole-frame kernels, as before: the Delta restore's parts with a base among their frames
    # go to the XOR kernel, the others and the Typed restore's to the plain one
    assert (x1 - x0) + (u1 - u0) == n and x1 > x0 and u2 - u1 == n
    assert l1[1] > l0[1] and l2[1] == l1[1] and l2[3] > l1[3]


def test_device_layer_without_the_window_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the stand-in: the slices call returns (size_t)-1 with nothing queued; the Typed and Delta
    calls work as before (a process of its own: one set of mock libraries each)"""
    build_pair(zstd.path, NOWIN_MOCK_SO, NOWIN_FRONT_SO, window=False)
    res = T.run_child("""
import test_device_restore_mock as R
chunk = R.CHUNK
data = D.typed_corpus("bf16", 3 * chunk + 321, 1)
base = D.typed_corpus("bf16", 3 * chunk + 321, 2)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [base], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
frames = fr.compress_device_batch_delta(pool.bufs, bas.bufs, [2])
out = R.OutPool(plug, [len(data)], [3], slot=2)
def seen():
    return (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), plug.lib.qzstd_mock_ungroup_launches(),
            plug.lib.qzstd_mock_ungroup_xor_launches(), fr.restore_stats(), fr.delta_stats(), fr.slice_stats())
before = seen()
r = fr.restore_slices_raw(frames, [len(data)], [2], [(0, 5, 1000, out.bufs[0][0], bas.bufs[0][0] + 5)])
nothing = seen() == before and out.untouched()
delta_ok = fr.restore_batch_delta(frames, out.bufs, bas.bufs, [2]) == len(frames[0]) and out.bytes() == out.expected([data])
typed = fr.compress_device_batch_typed(pool.bufs, [2])
out2 = R.OutPool(plug, [len(data)], [3], slot=2)
typed_ok = fr.restore_batch(typed, out2.bufs, [2]) == len(typed[0]) and out2.bytes() == out2.expected([data])
print(json.dumps({"refused": r == D.ERROR, "nothing_queued": nothing, "delta": delta_ok, "typed": typed_ok,
                  "has_window": hasattr(plug.lib, "qzstd_hip_ungroup_window")}))
""", NOWIN_MOCK_SO, NOWIN_FRONT_SO)
    assert res == {"refused": True, "nothing_queued": True, "delta": True, "typed": True, "has_window": False}, res
