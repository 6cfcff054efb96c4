"""CPU: the plane probe (QZSTD_frontSetPlaneProbe, QZSTD_frontPlaneProbeStats: include/qzstd_frontend_device.h) over the mock device layer —
the mock of tests/test_device_verify_mock.py plus tests/mock/mock_hip_plane_cost.c (qzstd_hip_plane_cost in plain C, over the one definition of
include/qzstd_planecost.h).  Setting off: today's frames and no probe launch.  Setting on, over bf16 and fp32 N(0, 0.02) weights and text:
every frame is byte for byte qz_device.reference_frames_probe's — the oracle's sequences, the header's rule, libzstd — decodes with libzstd
(which verifies the appended hash with checksums on) to the grouped content, and is the setting-off frame where no block is raw-predicted;
the counters hold what the reference counted.  Delta frames go through the delta restore, the slices restore and the verify call.  A failed
sub-frame (the front's test switch) yields the setting-off frame and counts as a fallback; a device layer without the kernel refuses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D
import test_device_checksum_mock as T
import test_device_restore_mock as R

MOCK = T.MOCK
MOCK_SO = os.path.join(MOCK, "libqatseqprod_probemock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_probemock.so")
NOPROBE_MOCK_SO = os.path.join(MOCK, "libqatseqprod_noprobemock.so")
NOPROBE_FRONT_SO = os.path.join(MOCK, "libqzstdfront_noprobemock.so")
CHUNK = 65536
PART = 3 * CHUNK  # three frames per part: both slots are used again
# (kind, bytes, element size): bf16 and fp32 weights with odd tails, text grouped by 2 (no noise plane: never raw-predicted), a tiled row
SPEC = (("bf16", 3 * CHUNK + 4321, 2), ("fp32", 2 * CHUNK + 5, 4), ("text", CHUNK + 77, 2), ("bf16", 8192 + 6, 2), ("tiled", CHUNK, 2),
        ("fp32", 4097 * 4, 4))
ELEMS = [k for _, _, k in SPEC]


def build_pair(zstd_path, mock_so, front_so, plane: bool):
    """the verify test's mock pair, with the plane cost's stand-in or — an older device layer — without"""
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c")]
    if plane:
        srcs.append(os.path.join(MOCK, "mock_hip_plane_cost.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def probemock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, plane=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    plug.lib.qzstd_mock_plane_cost_rows.restype = C.c_ulonglong
    plug.lib.qzstd_mock_fail_block.argtypes = [C.c_int]
    return plug, F


def corpus(kind, n, seed):
    if kind == "tiled":  # the low plane is bytes 0..255 over and over: a flat histogram and long repeats
        return (np.arange(n // 2, dtype=np.uint32) % 256).astype(np.uint16).tobytes()
    if kind == "text":
        import qz_corpus as K
        return K.by_name("text", n, seed=seed)
    return D.typed_corpus(kind, n, seed)


@pytest.fixture(scope="module")
def batch(probemock, zstd, oracle):
    """the buffers' bytes, their bases' bytes (a second draw: the XOR of two weight tensors is weights-like noise), and per checksum setting
    the reference frames with the setting off and on with what the reference counted — computed once and never changed"""
    _, F = probemock
    datas = [corpus(kind, n, 40 + i) for i, (kind, n, _) in enumerate(SPEC)]
    bases = [corpus(kind, n, 90 + i) for i, (kind, n, _) in enumerate(SPEC)]
    ref = {}
    for ck in (False, True):
        counts = {}
        off = [D.reference_frames_grouped(zstd, oracle, d, CHUNK, 1, k, checksum=ck, lib=F) for d, k in zip(datas, ELEMS)]
        on = [D.reference_frames_probe(zstd, oracle, d, CHUNK, 1, k, checksum=ck, lib=F, counts=counts) for d, k in zip(datas, ELEMS)]
        ref[ck] = (off, on, counts)
    return datas, bases, ref


def parts(datas, F):
    """the call's parts as the front plans them: whole frames, at most PART bytes and at most 4 * PART / CHUNK blocks each"""
    n, size, blocks = 0, None, 0
    for d, k in zip(datas, ELEMS):
        for o in range(0, len(d), CHUNK):
            m = min(CHUNK, len(d) - o)
            nb = len(D.group_blocks(m, k, F))
            if size is None or size + m > PART or blocks + nb > 4 * (PART // CHUNK):
                n, size, blocks = n + 1, 0, 0
            size, blocks = size + m, blocks + nb
    return n


def launches(plug):
    return plug.lib.qzstd_mock_plane_cost_launches(), plug.lib.qzstd_mock_plane_cost_rows()


def test_setting_off_is_today_and_never_probes(probemock, zstd, batch, monkeypatch):
    plug, F = probemock
    datas, _, ref = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.get_plane_probe() == 0
        pool = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))])
        before = launches(plug)
        assert fr.compress_device_batch_typed(pool.bufs, ELEMS) == ref[False][0]
        assert launches(plug) == before and fr.plane_probe_stats() == [0, 0, 0, 0]
        # on, but nothing grouped and no base: untouched
        assert fr.set_plane_probe(True) == 0 and fr.get_plane_probe() == 1
        plain = fr.compress_device_batch(pool.bufs)
        assert launches(plug) == before and fr.plane_probe_stats() == [0, 0, 0, 0]
        assert fr.set_plane_probe(False) == 0
        assert fr.compress_device_batch(pool.bufs) == plain
    finally:
        fr.close()
    assert F.QZSTD_frontSetPlaneProbe(None, 1) == -1 and F.QZSTD_frontGetPlaneProbe(None) == 0
    st = (C.c_ulonglong * 4)(9, 9, 9, 9)
    F.QZSTD_frontPlaneProbeStats(None, st)
    assert list(st) == [0, 0, 0, 0]


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
def test_setting_on_equals_the_reference(probemock, zstd, batch, monkeypatch, checksum):
    plug, F = probemock
    datas, _, ref = batch
    off, on, counts = ref[checksum]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    # the reference itself: the noise planes are found, text and the tiled row are left alone
    assert counts["assembled"] > 0 and counts["raw"] > 0 and counts["fallback"] == 0
    # (an assembled frame may well BE the setting-off frame: libzstd stores the same raw blocks and codes the others alike)
    assert on[2] == off[2] and on[4] == off[4]
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_checksum(checksum) == 0 and fr.set_plane_probe(True) == 0
        pool = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))])
        l0 = launches(plug)
        got = fr.compress_device_batch_typed(pool.bufs, ELEMS)
        n_frames = sum(len(x) for x in got)
        assert got == on
        for g, w, d, k in zip(got, off, datas, ELEMS):
            for c, f in enumerate(g):
                assert T.flagged(f) == checksum
                content = zstd.decompress(f, CHUNK)  # (libzstd's decoder verifies the checksum of a flagged frame)
                assert D.ungroup_bytes(content, k, F) == d[c * CHUNK:(c + 1) * CHUNK]
                # at most minGain per raw block larger than the setting-off frame
                assert len(f) <= len(w[c]) + sum((n >> 6) + 2 for t, b in D.frame_blocks(f) if t == 0 for n in [len(b) - 3])
        assert fr.plane_probe_stats() == [counts["blocks"], counts["raw"], counts["assembled"], 0]
        l1 = launches(plug)
        assert l1[1] - l0[1] == counts["blocks"] and l1[0] - l0[0] == parts(datas, F) and n_frames > 6  # one launch per part
        assert fr.stats()[0] >= counts["assembled"] and fr.byte_group_stats()[0] >= counts["assembled"]
        assert fr.checksum_stats()[0] >= (counts["assembled"] if checksum else 0)
        # the setting off again on the same front: today's frames
        assert fr.set_plane_probe(False) == 0
        assert fr.compress_device_batch_typed(pool.bufs, ELEMS) == off and launches(plug) == l1
    finally:
        fr.close()


def test_delta_frames_restore_slices_and_verify(probemock, zstd, oracle, batch, monkeypatch):
    plug, F = probemock
    datas, bases, _ = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    based = [True, True, False, True, True, False]
    xored = [(np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() if on else d for d, b, on in zip(datas, bases, based)]
    counts = {}
    want = [D.reference_frames_probe(zstd, oracle, x, CHUNK, 1, k, lib=F, counts=counts) for x, k in zip(xored, ELEMS)]
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_plane_probe(True) == 0
        src = T.Pool(plug, datas, [(1, 3, 15, 0, 5)[i % 5] for i in range(len(datas))], slot=0)
        bas = T.Pool(plug, bases, [(7, 0, 2, 9, 15, 4)[i % 6] for i in range(len(datas))], slot=1)
        given = [b if on else None for b, on in zip(bas.bufs, based)]
        frames = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        assert frames == want
        assert fr.plane_probe_stats() == [counts["blocks"], counts["raw"], counts["assembled"], counts["fallback"]] and counts["assembled"] > 0
        assert fr.delta_stats()[0] > 0
        n = sum(len(x) for x in frames)
        # the delta restore
        out = R.OutPool(plug, [len(d) for d in datas], [3] * len(datas), slot=2)
        assert fr.restore_batch_delta(frames, out.bufs, given, ELEMS) == n and out.bytes() == out.expected(datas)
        # slices: the middle of every buffer
        slices = [(i, len(d) // 3, len(d) // 2) for i, d in enumerate(datas)]
        dst = R.OutPool(plug, [s[2] for s in slices], [5] * len(slices), slot=3)
        give = [(b, o, m, p, None if given[b] is None else given[b][0] + o) for (b, o, m), (p, _) in zip(slices, dst.bufs)]
        assert fr.restore_slices(frames, [len(d) for d in datas], ELEMS, give) > 0
        assert dst.bytes() == dst.expected([datas[b][o:o + m] for b, o, m in slices])
        # verify: the frames reproduce the live tensors; one changed bit is found
        assert fr.verify(frames, src.bufs, given, ELEMS) == []
        C.c_ubyte.from_address(src.bufs[1][0] + CHUNK + 100).value ^= 4
        assert fr.verify(frames, src.bufs, given, ELEMS) == [(1, 1, 100)]
    finally:
        fr.close()


def test_a_failed_sub_frame_falls_back_to_the_setting_off_frame(probemock, zstd, batch, monkeypatch):
    plug, F = probemock
    datas, _, ref = batch
    off, on, counts = ref[False]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    monkeypatch.setenv("QZSTD_FRONT_PROBE_FAIL_SUB", "1")
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_plane_probe(True) == 0
        pool = T.Pool(plug, datas, [0] * len(datas))
        got = fr.compress_device_batch_typed(pool.bufs, ELEMS)
        mixed = counts["assembled"] - counts["allraw"]
        assert mixed > 0
        # a frame whose blocks are ALL raw-predicted needs no libzstd call and is still assembled; every other one is the setting-off frame
        for g, a, b in zip(got, off, on):
            for c, f in enumerate(g):
                assert f == a[c] or (f == b[c] and all(t == 0 for t, _ in D.frame_blocks(f)))
        st = fr.plane_probe_stats()
        assert st[0] == counts["blocks"] and st[2] == counts["allraw"] and st[3] == mixed
    finally:
        fr.close()


def test_a_failed_block_is_never_assembled(probemock, zstd, batch, monkeypatch):
    """a block the matcher failed: its frame takes libzstd's own match-finder as with the setting off, and still decodes"""
    plug, F = probemock
    datas, _, _ = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(1, 1, CHUNK, lib=F)
    try:
        assert fr.set_plane_probe(True) == 0
        pool = T.Pool(plug, datas[:1], [0])
        plug.lib.qzstd_mock_fail_block(1)
        try:
            got = fr.compress_device_batch_typed(pool.bufs, ELEMS[:1])
        finally:
            plug.lib.qzstd_mock_fail_block(-1)
        for c, f in enumerate(got[0]):
            assert D.ungroup_bytes(zstd.decompress(f, CHUNK), 2, F) == datas[0][c * CHUNK:(c + 1) * CHUNK]
        assert fr.stats()[1] >= 1  # the failed block's frame was built from its bytes
    finally:
        fr.close()


def test_mock_kernel_rows_at_any_offset(probemock):
    """the plain-C restatement itself against numpy: rows at odd offsets, an empty row, only nRows words written, the refusals"""
    plug, F = probemock
    L = D.bind_plane_kernel(plug.lib)
    rng = np.random.default_rng(3)
    buf = np.ascontiguousarray(rng.integers(0, 256, 300000, dtype=np.uint8))
    spans = [(1, 1), (3, 15), (17, 4097), (5000, 0), (70001, 131072), (250000, 4096)]
    rows = (D.PlaneRow * len(spans))(*[D.PlaneRow(o, n, 0) for o, n in spans])
    d_rows = (D.PlaneRow * len(spans))()
    out = np.full(len(spans) + 2, 7, dtype=np.uint32)
    assert L.qzstd_hip_plane_cost(0, None, buf.ctypes.data, rows, len(spans), d_rows, out.ctypes.data + 4) == 0
    assert list(out[1:-1]) == [D.plane_cost(buf[o:o + n].tobytes(), F) for o, n in spans] and out[0] == 7 and out[-1] == 7
    assert out[1] == 0 and out[4] == 0 and abs(int(out[5]) - 131072) <= 131072 // 1024 + 1 + 200  # noise: about len (the sampling bias of 512 per bin)
    rows[2].len = 131073
    assert L.qzstd_hip_plane_cost(0, None, buf.ctypes.data, rows, len(spans), d_rows, out.ctypes.data + 4) < 0
    rows[2].len, rows[2].reserved = 16, 1
    assert L.qzstd_hip_plane_cost(0, None, buf.ctypes.data, rows, len(spans), d_rows, out.ctypes.data + 4) < 0
    assert L.qzstd_hip_plane_cost(0, None, buf.ctypes.data, rows, 0, d_rows, None) == 0


def test_device_layer_without_the_plane_cost_entry_point(zstd, oracle):
    """the front-end linked against a mock WITHOUT the kernel's stand-in: with the setting on a grouped or delta call returns (size_t)-1 before
    anything is queued; ungrouped calls, and every call with the setting off, are served as before (a process of its own)"""
    build_pair(zstd.path, NOPROBE_MOCK_SO, NOPROBE_FRONT_SO, plane=False)
    res = T.run_child("""
chunk = 65536
data = D.typed_corpus("bf16", 2 * chunk + 321, 1)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [data[::-1]], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
off = fr.compress_device_batch_typed(pool.bufs, [2])
plain = fr.compress_device_batch(pool.bufs)
ok = fr.set_plane_probe(True) == 0
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), fr.stats(), fr.plane_probe_stats())
before = state()
r1 = fr.compress_device_batch_typed_raw(pool.bufs, [2])[0]
r2 = fr.compress_device_batch_delta_raw(pool.bufs, bas.bufs, [1])[0]
nothing = state() == before
same = fr.compress_device_batch(pool.bufs) == plain
fr.set_plane_probe(False)
again = fr.compress_device_batch_typed(pool.bufs, [2]) == off
print(json.dumps({"set": ok, "refused": r1 == D.ERROR and r2 == D.ERROR, "nothing_queued": nothing, "ungrouped": same, "off": again,
                  "has_kernel": hasattr(plug.lib, "qzstd_hip_plane_cost")}))
""", NOPROBE_MOCK_SO, NOPROBE_FRONT_SO)
    assert res == {"set": True, "refused": True, "nothing_queued": True, "ungrouped": True, "off": True, "has_kernel": False}, res
