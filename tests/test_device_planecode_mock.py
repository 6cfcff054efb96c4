"""CPU: the plane code (QZSTD_frontSetPlaneCode, QZSTD_frontPlaneCodeStats: include/qzstd_frontend_device.h) over the mock device layer — the
probe test's mock plus tests/mock/mock_hip_huf_code.c (qzstd_hip_huf_code in plain C over include/qzstd_hufblock.h).  Setting off: today's
frames and no coder launch.  Setting on, over bf16 and fp32 N(0, 0.02) weights and text, at levels 1 and 6, checksums off and on: every
frame is byte for byte qz_device.reference_frames_code's — the oracle's sequences, the probe's rule, the header alone through
tests/hufblock/hufblock_check.c, libzstd for the frames that are the probe's — and decodes with libzstd to the grouped content; the
counters hold what the reference counted.  A delta call whose high plane is zero runs takes none of those blocks, and the delta restore,
the slices restore and verify read its frames.  A device layer without the coder refuses."""
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
MOCK_SO = os.path.join(MOCK, "libqatseqprod_codemock.so")
FRONT_SO = os.path.join(MOCK, "libqzstdfront_codemock.so")
NOCODE_MOCK_SO = os.path.join(MOCK, "libqatseqprod_nocodemock.so")
NOCODE_FRONT_SO = os.path.join(MOCK, "libqzstdfront_nocodemock.so")
CHUNK = 65536
PART = 3 * CHUNK  # three frames per part: both slots are used again
# the probe test's three tensors, and one whose frames hold a taken block (bf16's high bytes) beside one that is neither taken nor raw (a
# tiled row in the low bytes: a flat histogram and long repeats): they fall back
SPEC = (("bf16", 3 * CHUNK + 4321, 2), ("fp32", 2 * CHUNK + 5, 4), ("text", CHUNK + 77, 2), ("mixed", CHUNK + 4096, 2))
ELEMS = [k for _, _, k in SPEC]
LEVELS = (1, 6)


def build_pair(zstd_path, mock_so, front_so, coder: bool):
    """the probe test's mock pair, with the coder's stand-in or — an older device layer — without"""
    inc = ["-I" + os.path.join(T.ROOT, "include"), "-I" + os.path.join(T.ROOT, "oracle")]
    cc = ["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-fPIC", "-pthread"] + inc
    obj = "%s.mock_hip.%d.o" % (mock_so, os.getpid())
    subprocess.check_call(cc + ["-Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner", "-c", os.path.join(MOCK, "mock_hip.c"), "-o", obj])
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"), obj,
            os.path.join(T.ROOT, "oracle", "qzstd_oracle.c")]
    srcs += [os.path.join(MOCK, n) for n in ("mock_hip_device.c", "mock_hip_gather.c", "mock_hip_xxh64.c", "mock_hip_group.c", "mock_fail_block.c",
                                             "mock_hip_ungroup.c", "mock_hip_group_xor.c", "mock_hip_ungroup_xor.c", "mock_hip_ungroup_window.c",
                                             "mock_hip_diff.c", "mock_hip_ungroup_cmp.c", "mock_hip_plane_cost.c")]
    if coder:
        srcs.append(os.path.join(MOCK, "mock_hip_huf_code.c"))
    try:
        T.build_shared(cc + ["-shared", "-o", mock_so] + srcs, mock_so)
    finally:
        if os.path.exists(obj):
            os.remove(obj)
    T.build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                    "-I" + os.path.join(T.ROOT, "include"), "-o", front_so, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                    mock_so, zstd_path, "-Wl,-rpath," + os.path.dirname(mock_so), "-Wl,-rpath," + os.path.dirname(zstd_path)], front_so)


@pytest.fixture(scope="module")
def codemock(oracle, zstd):
    build_pair(zstd.path, MOCK_SO, FRONT_SO, coder=True)
    plug, F = T.load_pair(MOCK_SO, FRONT_SO)
    D.bind(F)
    for name in ("qzstd_mock_plane_cost_rows", "qzstd_mock_huf_code_rows", "qzstd_mock_huf_code_coded"):
        getattr(plug.lib, name).restype = C.c_ulonglong
    return plug, F


@pytest.fixture(scope="module")
def huf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hufblock") / "libhufblock.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(T.ROOT, "include"), "-o", so,
                           os.path.join(T.ROOT, "tests", "hufblock", "hufblock_check.c")])
    return D.bind_hufblock(C.CDLL(so))


def corpus(kind, n, seed):
    if kind == "text":
        import qz_corpus as K
        return K.by_name("text", n, seed=seed)
    if kind == "mixed":
        v = np.frombuffer(D.typed_corpus("bf16", n, seed), dtype=np.uint8).copy()
        v[0::2] = np.arange(len(v[0::2])) % 256
        return v.tobytes()
    return D.typed_corpus(kind, n, seed)


def stepped(data, kind, seed):
    """the tensor after an N(0, 1e-5) step: the XOR with it has a high plane of zero runs"""
    if kind in ("text", "mixed"):
        return data
    rng = np.random.default_rng(seed)
    if kind == "bf16":
        w = (np.frombuffer(data[:len(data) & ~1], dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
        w2 = ((w + rng.normal(0.0, 1e-5, len(w)).astype(np.float32)).view(np.uint32) >> 16).astype(np.uint16).tobytes()
    else:
        w = np.frombuffer(data[:len(data) & ~3], dtype=np.float32)
        w2 = (w + rng.normal(0.0, 1e-5, len(w)).astype(np.float32)).tobytes()
    return w2 + data[len(w2):]


@pytest.fixture(scope="module")
def batch(codemock, zstd, oracle, huf):
    """the buffers' bytes, and per (level, checksum) the reference frames with the setting off and on with what the reference counted —
    computed once and never changed"""
    _, F = codemock
    datas = [corpus(kind, n, 40 + i) for i, (kind, n, _) in enumerate(SPEC)]
    ref = {}
    for level in LEVELS:
        for ck in (False, True):
            counts = {}
            off = [D.reference_frames_grouped(zstd, oracle, d, CHUNK, level, k, checksum=ck, lib=F) for d, k in zip(datas, ELEMS)]
            on = [D.reference_frames_code(zstd, oracle, huf, d, CHUNK, level, k, checksum=ck, lib=F, counts=counts) for d, k in zip(datas, ELEMS)]
            ref[(level, ck)] = (off, on, counts)
    return datas, ref


def launches(plug):
    return (plug.lib.qzstd_mock_huf_code_launches(), plug.lib.qzstd_mock_huf_code_rows(), plug.lib.qzstd_mock_huf_code_coded(),
            plug.lib.qzstd_mock_plane_cost_launches())


def test_setting_off_is_today_and_never_codes(codemock, zstd, batch, monkeypatch):
    plug, F = codemock
    datas, ref = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.get_plane_code() == 0
        pool = T.Pool(plug, datas, [(1, 3, 15, 0)[i % 4] for i in range(len(datas))])
        before = launches(plug)
        assert fr.compress_device_batch_typed(pool.bufs, ELEMS) == ref[(1, False)][0]
        assert launches(plug) == before and fr.plane_code_stats() == [0, 0, 0, 0]
        # the probe alone: the cost kernel, not the coder
        assert fr.set_plane_probe(True) == 0
        probed = fr.compress_device_batch_typed(pool.bufs, ELEMS)
        now = launches(plug)
        assert now[:3] == before[:3] and now[3] > before[3] and fr.plane_code_stats() == [0, 0, 0, 0]
        assert fr.set_plane_probe(False) == 0
        # on, but nothing grouped and no base: untouched
        assert fr.set_plane_code(True) == 0 and fr.get_plane_code() == 1
        plain = fr.compress_device_batch(pool.bufs)
        assert launches(plug) == now and fr.plane_code_stats() == [0, 0, 0, 0]
        assert fr.set_plane_code(False) == 0
        assert fr.compress_device_batch(pool.bufs) == plain
        assert [zstd.decompress(f, CHUNK) for g in probed for f in g] == [zstd.decompress(f, CHUNK) for g in ref[(1, False)][0] for f in g]
    finally:
        fr.close()
    assert F.QZSTD_frontSetPlaneCode(None, 1) == -1 and F.QZSTD_frontGetPlaneCode(None) == 0
    st = (C.c_ulonglong * 4)(9, 9, 9, 9)
    F.QZSTD_frontPlaneCodeStats(None, st)
    assert list(st) == [0, 0, 0, 0]


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("level", LEVELS)
def test_setting_on_equals_the_reference(codemock, zstd, batch, monkeypatch, level, checksum):
    plug, F = codemock
    datas, ref = batch
    off, on, counts = ref[(level, checksum)]
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    # the reference itself: exponent planes are taken and whole frames need no libzstd; a frame with one block that is neither falls back
    assert counts["taken"] > 0 and counts["nolib"] > 0 and counts["code_fallback"] > 0 and counts["coded"] >= counts["taken"]
    assert on[2] == off[2]  # text: no block is taken, none is raw
    fr = D.DeviceFront(3, level, CHUNK, lib=F)
    try:
        assert fr.set_checksum(checksum) == 0 and fr.set_plane_code(True) == 0
        pool = T.Pool(plug, datas, [(1, 3, 15, 0)[i % 4] for i in range(len(datas))])
        l0 = launches(plug)
        got = fr.compress_device_batch_typed(pool.bufs, ELEMS)
        assert got == on
        smaller = 0
        for g, w, d, k in zip(got, off, datas, ELEMS):
            for c, f in enumerate(g):
                assert T.flagged(f) == checksum
                content = zstd.decompress(f, CHUNK)  # (libzstd's decoder verifies the checksum of a flagged frame)
                assert D.ungroup_bytes(content, k, F) == d[c * CHUNK:(c + 1) * CHUNK]
                smaller += len(f) < len(w[c])
        assert smaller > 0
        assert fr.plane_code_stats() == [counts["coded"], counts["taken"], counts["nolib"], counts["code_fallback"]]
        assert fr.plane_probe_stats() == [counts["blocks"], counts["raw"], counts["assembled"], counts["fallback"]]
        l1 = launches(plug)
        # the coder INSTEAD of the cost kernel: a row per block, no cost launch
        assert l1[1] - l0[1] == counts["blocks"] and l1[2] - l0[2] == counts["coded"] and l1[0] > l0[0] and l1[3] == l0[3]
        # the setting off again on the same front: today's frames
        assert fr.set_plane_code(False) == 0
        assert fr.compress_device_batch_typed(pool.bufs, ELEMS) == off and launches(plug) == l1
    finally:
        fr.close()


def test_delta_frames_of_zero_runs_restore_slices_and_verify(codemock, zstd, oracle, huf, batch, monkeypatch):
    plug, F = codemock
    datas, _ = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    bases = [stepped(d, kind, 7 + i) for i, (d, (kind, _, _)) in enumerate(zip(datas, SPEC))]
    based = [True, True, False, False]
    xored = [(np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() if on else d for d, b, on in zip(datas, bases, based)]
    counts = {}
    want = [D.reference_frames_code(zstd, oracle, huf, x, CHUNK, 1, k, lib=F, counts=counts) for x, k in zip(xored, ELEMS)]
    # the high plane of the bf16 delta is zero runs: matches win, the rule takes none of those blocks
    prof, runs = oracle.profile(1, CHUNK), 0
    for c in range(0, len(xored[0]), CHUNK):
        g = D.group_bytes(xored[0][c:c + CHUNK], 2, F)
        ends = D.group_blocks(len(g), 2, F)
        if len(ends) < 2:  # (a short tail is one block)
            continue
        high = g[ends[-2]:ends[-1]]
        assert np.count_nonzero(np.frombuffer(high, dtype=np.uint8)) < len(high) // 4
        n, sq = oracle.find(prof, high, cap=B.sequence_bound(CHUNK))
        size, body = D.huf_block(huf, high, sum(s.litLength for s in sq[:n]), n)
        assert size > 0 and body is None
        runs += 1
    assert runs >= 3
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_plane_code(True) == 0
        src = T.Pool(plug, datas, [(1, 3, 15, 0)[i % 4] for i in range(len(datas))], slot=0)
        bas = T.Pool(plug, bases, [(7, 0, 2, 9)[i % 4] for i in range(len(datas))], slot=1)
        given = [b if on else None for b, on in zip(bas.bufs, based)]
        frames = fr.compress_device_batch_delta(src.bufs, given, ELEMS)
        assert frames == want
        assert fr.plane_code_stats() == [counts["coded"], counts["taken"], counts["nolib"], counts["code_fallback"]]
        assert fr.delta_stats()[0] > 0
        n = sum(len(x) for x in frames)
        out = R.OutPool(plug, [len(d) for d in datas], [3] * len(datas), slot=2)
        assert fr.restore_batch_delta(frames, out.bufs, given, ELEMS) == n and out.bytes() == out.expected(datas)
        slices = [(i, len(d) // 3, len(d) // 2) for i, d in enumerate(datas)]
        dst = R.OutPool(plug, [s[2] for s in slices], [5] * len(slices), slot=3)
        give = [(b, o, m, p, None if given[b] is None else given[b][0] + o) for (b, o, m), (p, _) in zip(slices, dst.bufs)]
        assert fr.restore_slices(frames, [len(d) for d in datas], ELEMS, give) > 0
        assert dst.bytes() == dst.expected([datas[b][o:o + m] for b, o, m in slices])
        assert fr.verify(frames, src.bufs, given, ELEMS) == []
        C.c_ubyte.from_address(src.bufs[1][0] + CHUNK + 100).value ^= 4
        assert fr.verify(frames, src.bufs, given, ELEMS) == [(1, 1, 100)]
    finally:
        fr.close()


def test_coded_frames_restore_and_verify(codemock, zstd, batch, monkeypatch):
    """frames with Huffman-only blocks through the restore and verify calls"""
    plug, F = codemock
    datas, ref = batch
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(3, 1, CHUNK, lib=F)
    try:
        assert fr.set_plane_code(True) == 0
        src = T.Pool(plug, datas, [0] * len(datas), slot=0)
        frames = fr.compress_device_batch_typed(src.bufs, ELEMS)
        assert frames == ref[(1, False)][1] and fr.plane_code_stats()[1] > 0
        out = R.OutPool(plug, [len(d) for d in datas], [3] * len(datas), slot=2)
        assert fr.restore_batch_delta(frames, out.bufs, [None] * len(datas), ELEMS) == sum(len(x) for x in frames)
        assert out.bytes() == out.expected(datas)
        assert fr.verify(frames, src.bufs, [None] * len(datas), ELEMS) == []
    finally:
        fr.close()


def test_device_layer_without_the_coder(zstd, oracle):
    """the front-end linked against a mock WITHOUT the coder's stand-in: with the setting on a grouped or delta call returns (size_t)-1 before
    anything is queued; the probe, ungrouped calls, and every call with the setting off, are served as before (a process of its own)"""
    build_pair(zstd.path, NOCODE_MOCK_SO, NOCODE_FRONT_SO, coder=False)
    res = T.run_child("""
chunk = 65536
data = D.typed_corpus("bf16", 2 * chunk + 321, 1)
pool = T.Pool(plug, [data], [0], slot=0)
bas = T.Pool(plug, [data[::-1]], [5], slot=1)
D.bind(F)
fr = D.DeviceFront(2, 1, chunk, lib=F)
off = fr.compress_device_batch_typed(pool.bufs, [2])
plain = fr.compress_device_batch(pool.bufs)
ok = fr.set_plane_code(True) == 0
state = lambda: (plug.lib.qzstd_mock_event_waits(), plug.lib.qzstd_mock_launches(), fr.stats(), fr.plane_code_stats(), fr.plane_probe_stats())
before = state()
r1 = fr.compress_device_batch_typed_raw(pool.bufs, [2])[0]
r2 = fr.compress_device_batch_delta_raw(pool.bufs, bas.bufs, [1])[0]
nothing = state() == before
same = fr.compress_device_batch(pool.bufs) == plain
fr.set_plane_code(False)
again = fr.compress_device_batch_typed(pool.bufs, [2]) == off
fr.set_plane_probe(True)
probed = len(fr.compress_device_batch_typed(pool.bufs, [2])[0]) == len(off[0]) and fr.plane_probe_stats()[0] > 0
print(json.dumps({"set": ok, "refused": r1 == D.ERROR and r2 == D.ERROR, "nothing_queued": nothing, "ungrouped": same, "off": again,
                  "probe": probed, "has_kernel": hasattr(plug.lib, "qzstd_hip_huf_code")}))
""", NOCODE_MOCK_SO, NOCODE_FRONT_SO)
    assert res == {"set": True, "refused": True, "nothing_queued": True, "ungrouped": True, "off": True, "probe": True, "has_kernel": False}, res
