"""CPU: QZSTD_frontCompressDevice (include/qzstd_frontend_device.h) over the mock device layer — qat-zstd-plugin_amd/host/qatseqprod.c and the
front-end linked against tests/mock/mock_hip.c (malloc as device memory, the oracle as the match-finder) plus
tests/mock/mock_hip_device.c (the device-input entry points: a registered range stands for device memory, the compaction on the CPU).
Checks the framing, the per-part pipeline, the raw-bytes fallback, the statistics and the error returns without a GPU: frames must be
the ones libzstd builds with ZSTD_compress2 from the ORACLE's sequences."""
import ctypes as C
import os
import subprocess

import pytest

import qz_bind as B
import qz_corpus as K
import qz_device as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK_SO = os.path.join(ROOT, "tests", "mock", "libqatseqprod_devmock.so")
FRONT_SO = os.path.join(ROOT, "tests", "mock", "libqzstdfront_devmock.so")


def build_shared(cmd, out):
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.check_call([tmp if x == out else x for x in cmd])
    os.replace(tmp, out)


@pytest.fixture(scope="module")
def devmock(oracle, zstd):
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "tests", "mock", "mock_hip.c"), os.path.join(ROOT, "tests", "mock", "mock_hip_device.c"),
            os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    build_shared(["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-o", MOCK_SO] + srcs, MOCK_SO)
    build_shared(["gcc", "-O2", "-g", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-o", FRONT_SO, os.path.join(B.PKG_DIR, "frontend", "qzstd_frontend.c"),
                  MOCK_SO, zstd.path, "-Wl,-rpath," + os.path.dirname(MOCK_SO), "-Wl,-rpath," + os.path.dirname(zstd.path)], FRONT_SO)
    plug = B.Plugin(MOCK_SO)
    F = C.CDLL(FRONT_SO)
    plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    return plug, F


class DevBuf:
    """host memory the mock treats as device memory of device 0; data placed at `offset` from a 64-byte aligned start"""

    def __init__(self, plug, data: bytes, offset: int = 0):
        self.raw = C.create_string_buffer(len(data) + offset + 128)
        base = (C.addressof(self.raw) + 63) & ~63
        self.addr = base + offset
        C.memmove(self.addr, data, len(data))
        plug.lib.qzstd_mock_device_range(0, self.addr, max(len(data), 1), 0)


def reference(zstd, oracle, data, chunk, level, ext_rep=False):
    return D.reference_frames(zstd, oracle, data, chunk, level, ext_rep)


@pytest.mark.parametrize("level,chunk,size,part", [(1, 32768, 20 * 32768 + 777, 4 * 32768), (1, 131072, 9 * 131072 + 5000, 2 * 131072),
                                                   (6, 131072, 5 * 131072 + 4000, 0), (3, 393216, 3 * 393216 + 70000, 393216),
                                                   (12, 32768, 7 * 32768, 3 * 32768)])
def test_device_frames_equal_the_oracles(devmock, zstd, oracle, level, chunk, size, part, monkeypatch):
    plug, F = devmock
    if part:  # several parts: the double-buffered pipeline, parts fetched while the workers code the one before
        monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(part))
    data = K.by_name("text", size, seed=level + 3)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, level, chunk, lib=F)
    try:
        got = fr.compress_device(buf.addr, len(data))
        assert got == reference(zstd, oracle, data, chunk, level)
        st = fr.stats()
        n = (len(data) + chunk - 1) // chunk
        assert st[0] == n and st[1] == 0 and st[3] == len(data), st
        assert st[2] > 0, st
        for c in (0, n - 1):
            assert zstd.decompress(got[c], chunk) == data[c * chunk:(c + 1) * chunk]
    finally:
        fr.close()


def test_device_frames_external_repcodes(devmock, zstd, oracle, monkeypatch):
    plug, F = devmock
    monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    data = K.by_name("system", 6 * 65536 + 99, seed=5)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 65536, ext_rep=1, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 65536, 1, ext_rep=True)
    finally:
        fr.close()


@pytest.mark.parametrize("offset,size", [(1, 5 * 32768 + 3), (3, 40000), (15, 32768 * 2), (0, 32768 + 7), (5, 11), (0, 15), (0, 1)])
def test_device_misaligned_and_short(devmock, zstd, oracle, offset, size):
    plug, F = devmock
    data = K.by_name("mix", size, seed=offset + size)
    buf = DevBuf(plug, data, offset)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 32768, 1)
    finally:
        fr.close()


def test_device_empty_input(devmock):
    plug, F = devmock
    buf = DevBuf(plug, b"x" * 64)
    fr = D.DeviceFront(1, 1, 32768, lib=F)
    try:
        r, frames = fr.compress_device_raw(buf.addr, 0)
        assert r == 0 and frames == []
    finally:
        fr.close()


def test_device_incompressible_takes_the_raw_bytes(devmock, zstd, oracle):
    plug, F = devmock
    data = os.urandom(3 * 65536) + K.by_name("text", 2 * 65536 + 11, seed=9)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 65536, lib=F)
    try:
        got = fr.compress_device(buf.addr, len(data))
        assert got == reference(zstd, oracle, data, 65536, 1)
        st = fr.stats()
        assert st[1] >= 3 and st[0] + st[1] == 6, st
        assert st[2] >= 3 * 65536, st  # the raw bytes came back
    finally:
        fr.close()


def test_device_error_returns_launch_nothing(devmock, zstd):
    plug, F = devmock
    data = K.by_name("text", 4 * 32768, seed=2)
    host = C.create_string_buffer(data, len(data))
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    sw = D.DeviceFront(2, 1, 32768, use_producer=0, lib=F)
    try:
        before = plug.lib.qzstd_mock_launches()
        assert fr.compress_device_raw(C.addressof(host), len(data))[0] == D.ERROR  # a host pointer
        assert fr.compress_device_raw(buf.addr, len(data), dst_capacity=3 * fr.stride)[0] == D.ERROR  # dst too small
        assert fr.compress_device_raw(buf.addr, len(data) + 4096)[0] == D.ERROR  # runs past the device range
        assert sw.compress_device_raw(buf.addr, len(data))[0] == D.ERROR  # useProducer = 0
        assert plug.lib.qzstd_mock_launches() == before
        assert fr.stats() == [0, 0, 0, 0]
        # and the front still works afterwards, both ways in
        assert fr.compress_device(buf.addr, len(data)) == fr.compress_host(data)
    finally:
        fr.close()
        sw.close()


def test_device_d2h_traffic_is_the_compacted_results(devmock, zstd, oracle):
    """level 1: what comes back is the headers, 8 bytes per entry and the literal bytes — no raw input"""
    plug, F = devmock
    chunk = 131072
    data = K.by_name("system", 12 * chunk, seed=17)
    buf = DevBuf(plug, data)
    prof = oracle.profile(1, chunk)
    lits = seqs = 0
    for o in range(0, len(data), chunk):
        n, s = oracle.find(prof, data[o:o + chunk])
        seqs += n
        lits += sum(s[i].litLength for i in range(n))
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        fr.compress_device(buf.addr, len(data))
        st = fr.stats()
        assert st[1] == 0 and st[2] <= lits + 8 * seqs + 16 * 12 and st[2] < len(data), (st, lits, seqs)
    finally:
        fr.close()


def test_device_second_concurrent_call_is_refused(devmock, zstd, oracle):
    """a call while another one runs on the same front returns (size_t)-1 at once; the first one is not disturbed"""
    import threading
    plug, F = devmock
    plug.lib.qzstd_mock_stall_ms.argtypes = [C.c_int]
    data = K.by_name("text", 6 * 32768 + 5, seed=21)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, 32768, lib=F)
    other = C.create_string_buffer(7 * fr.stride)
    sizes = (C.c_size_t * 8)()
    got = {}
    try:
        plug.lib.qzstd_mock_stall_ms(1500)  # every stream looks busy: the first call waits for its first part
        th = threading.Thread(target=lambda: got.update(frames=fr.compress_device(buf.addr, len(data))))
        th.start()
        import time
        time.sleep(0.3)
        r = fr.lib.QZSTD_frontCompressDevice(fr.f, C.c_void_p(buf.addr), len(data), None, other, len(other), sizes)
        th.join(60)
        assert r == D.ERROR
        assert got["frames"] == reference(zstd, oracle, data, 32768, 1)
        assert fr.stats()[3] == len(data)  # one call's input
    finally:
        plug.lib.qzstd_mock_stall_ms(0)
        fr.close()


def test_device_without_seqlit_every_frame_takes_the_raw_bytes(devmock, zstd, oracle):
    """a libzstd without ZSTD_compressSequencesAndLiterals (QZSTD_FRONT_NO_SEQLIT=1 makes the front-end ignore it; the look-up is made
    once per process, hence a process of its own): every frame is built from its raw bytes, and the frames are the same"""
    import json
    import sys
    script = """
import ctypes as C, json, sys
sys.path[:0] = [%r, %r]
import qz_bind as B, qz_corpus as K, qz_device as D
z, o = B.Zstd(), B.Oracle()
plug = B.Plugin(%r)
F = C.CDLL(%r)
plug.lib.qzstd_mock_device_range.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int]
data = K.by_name("system", 5 * 65536 + 321)
raw = C.create_string_buffer(data, len(data) + 64)
plug.lib.qzstd_mock_device_range(0, C.addressof(raw), len(data), 0)
fr = D.DeviceFront(2, 1, 65536, lib=F)
same = fr.compress_device(C.addressof(raw), len(data)) == D.reference_frames(z, o, data, 65536, 1)
print(json.dumps({"same": same, "stats": fr.stats()}))
""" % (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests"), MOCK_SO, FRONT_SO)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, QZSTD_FRONT_NO_SEQLIT="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["same"] and res["stats"][0] == 0 and res["stats"][1] == 6, res


# ------------------------------------------------------------------ the compaction contract: the mock against tools/qz_compact_ref.py
import numpy as np  # noqa: E402

import qz_compact_ref as R  # noqa: E402


def aligned(n: int, fill: np.ndarray | None = None, align: int = 64, skew: int = 0) -> np.ndarray:
    """n bytes at an `align`-aligned address plus `skew`, holding `fill` (zeros by default)"""
    raw = np.zeros(n + align + skew, dtype=np.uint8)
    o = (-raw.ctypes.data) % align + skew
    a = raw[o:o + n]
    if fill is not None:
        a[:] = fill[:n]
    return a


def canary(n: int, seed: int = 99) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def mock_compact(plug, batch, arena_bytes, slack=4096, n=None, work_bytes=None, arena_skew=0, work_skew=0, null=()):
    """the mock's qzstd_hip_compact on a batch -> (return value, arena + slack bytes after the call, the canary they held before).
    arena_skew / work_skew: bytes past an aligned address; null: the pointers passed as NULL"""
    L = plug.lib
    L.qzstd_hip_compact.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_size_t]
    nb = len(batch.blocks) if n is None else n
    before = canary(arena_bytes + slack, seed=arena_bytes & 0xFFFF)
    arena = aligned(arena_bytes + slack, before, skew=arena_skew)
    work_bytes = R.workspace_bytes(len(batch.blocks)) if work_bytes is None else work_bytes
    work = aligned(work_bytes, skew=work_skew)
    ptr = {"src": batch.src, "blocks": batch.blocks, "seqs": batch.seqs, "counts": batch.counts, "arena": arena, "work": work}
    ptr = {k: None if k in null else v.ctypes.data for k, v in ptr.items()}
    r = L.qzstd_hip_compact(0, None, ptr["src"], ptr["blocks"], nb, ptr["seqs"], ptr["counts"], ptr["arena"], arena_bytes, ptr["work"],
                            work_bytes)
    return r, arena.copy(), before


def check_against_reference(plug, batch, arena_bytes, slack=4096):
    r, got, before = mock_compact(plug, batch, arena_bytes, slack)
    assert r == 0
    want, used, kept = batch.reference(arena_bytes, before)
    assert used <= arena_bytes
    bad = np.flatnonzero(got[:arena_bytes] != want)
    assert not len(bad), "arena bytes differ from the contract from %d (of %d; used %d)" % (bad[0], arena_bytes, used)
    assert np.array_equal(got[arena_bytes:], before[arena_bytes:]), "bytes past arenaBytes were written"
    return kept


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mock_compaction_follows_the_contract(devmock, seed):
    """random valid batches, every block kept: headers, packed entries and literals byte for byte"""
    plug, _ = devmock
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, 131073, 20)] + [131072, 16, 7, 1]
    batch = R.make_batch(rng, lens, order="shuffled" if seed == 2 else "block", gap=48 if seed == 3 else 0)
    assert check_against_reference(plug, batch, batch.need() + 3).all()


def test_mock_compaction_mutations(devmock):
    """one block per rejection rule, each at its boundary: accepted and rejected exactly as the contract says"""
    plug, _ = devmock
    for seed in range(4):
        batch, where = R.mutation_batch(np.random.default_rng(100 + seed))
        kept = check_against_reference(plug, batch, batch.need())
        for b, name in where.items():
            assert kept[b] == R.MUTATIONS[name], (name, b)
        assert sum(kept) == len(kept) - sum(not v for v in R.MUTATIONS.values())


def test_mock_compaction_capacity(devmock):
    """an arena of exactly the needed size keeps every block; one byte less drops the last one only; the first block that does not fit
    and every block after it (a failed one among them) contribute nothing; an arena of headers alone keeps nothing"""
    plug, _ = devmock
    rng = np.random.default_rng(7)
    lens = [int(x) for x in rng.integers(1, 3000, 40)]
    batch = R.make_batch(rng, lens, mutations={30: "count_error"})
    need = batch.need()
    assert check_against_reference(plug, batch, need).sum() == 39
    kept = check_against_reference(plug, batch, need - 1)
    assert kept.sum() == 38 and not kept[39]
    for first in (1, 17, 25):
        kept = check_against_reference(plug, batch, batch.need(first))
        assert kept[:first].sum() == first and not kept[first:].any()
        kept = check_against_reference(plug, batch, batch.need(first + 1) - 1)
        assert kept[:first].sum() == first and not kept[first:].any()
    assert not check_against_reference(plug, batch, R.entries_off(40)).any()


@pytest.mark.parametrize("odd", [1, 3, 513])
def test_mock_compaction_header_padding(devmock, odd):
    """n odd: the 8 bytes between the headers and the entries keep what they held"""
    plug, _ = devmock
    rng = np.random.default_rng(odd)
    batch = R.make_batch(rng, [int(x) for x in rng.integers(1, 400, odd)])
    check_against_reference(plug, batch, batch.need())


def test_mock_compaction_refusals(devmock):
    """the refusals the kernel makes, and nothing written: misaligned arena or workspace, a short workspace, an arena smaller than its
    headers, each null pointer; nBlocks 0 returns 0"""
    plug, _ = devmock
    batch = R.make_batch(np.random.default_rng(5), [100, 200, 300])
    need = batch.need()
    cases = [dict(arena_skew=8), dict(work_skew=4), dict(work_bytes=R.workspace_bytes(3) - 1)]
    cases += [dict(null=(k,)) for k in ("src", "blocks", "seqs", "counts", "arena", "work")]
    for case in cases:
        r, got, before = mock_compact(plug, batch, need, **case)
        assert r != 0 and np.array_equal(got, before), case
    r, got, before = mock_compact(plug, batch, R.entries_off(3) - 1)
    assert r != 0 and np.array_equal(got, before)
    r, got, before = mock_compact(plug, batch, need, n=0)
    assert r == 0 and np.array_equal(got, before)


# ------------------------------------------------------------------ near-raw blocks: libzstd stores them raw, so must the device path
def near_raw_input(chunk: int, seed: int) -> bytes:
    """random bytes with 0-3 % planted repeats per 128 KiB block (per chunk, when smaller); 256 KiB chunks: one block of each frame
    near-raw, the other text that compresses well"""
    if chunk > 131072:
        return K.near_raw_text(seed, 4 * chunk)
    size = {16: 1024 * 16, 100: 600 * 100, 1024: 256 * 1024, 4096: 96 * 4096, 32768: 24 * 32768, 131072: 8 * 131072}[chunk] + chunk // 3
    return K.near_raw(seed, size, chunk)


NEAR_RAW_CHUNKS = [16, 100, 1024, 4096, 32768, 131072, 262144]
NEAR_RAW_LEVELS = [(1, False), (3, False), (6, False), (12, False), (1, True)]


@pytest.mark.parametrize("level,ext_rep", NEAR_RAW_LEVELS)
@pytest.mark.parametrize("chunk", NEAR_RAW_CHUNKS)
def test_device_near_raw_blocks(devmock, zstd, oracle, chunk, level, ext_rep, monkeypatch):
    """a block whose compressed body does not beat its size by (size >> 6) + 2 bytes is stored raw by libzstd: the frame takes the
    raw-bytes path and equals the reference; every frame is counted once"""
    plug, F = devmock
    if ext_rep:
        monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    data = near_raw_input(chunk, seed=chunk + level)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, level, chunk, ext_rep=int(ext_rep), lib=F)
    try:
        got = fr.compress_device(buf.addr, len(data))
        want = reference(zstd, oracle, data, chunk, level, ext_rep)
        bad = [c for c in range(len(want)) if got[c] != want[c]]
        assert len(got) == len(want) and not bad, "%d of %d frames differ, first %s" % (len(bad), len(want), bad[:8])
        st = fr.stats()
        assert st[0] + st[1] == len(want) and st[3] == len(data), st
    finally:
        fr.close()


@pytest.mark.parametrize("chunk", [131072, 393216])
def test_device_rle_blocks(devmock, zstd, oracle, chunk):
    """blocks of one repeated byte or of "ab" repeats (libzstd's RLE blocks, not the first block of a frame): the frames are the reference's"""
    plug, F = devmock
    data = bytes(chunk) + b"ab" * chunk + bytes(chunk // 2) + b"x" * 1000
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(2, 1, chunk, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, chunk, 1)
    finally:
        fr.close()


@pytest.mark.parametrize("chunk", [16, 32, 64, 100])
def test_device_tiny_chunks_of_mixed_data(devmock, zstd, oracle, chunk):
    plug, F = devmock
    data = K.by_name("mix", 2000 * chunk // 4 + 5, seed=chunk)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, chunk, 1)
        assert sum(fr.stats()[:2]) == (len(data) + chunk - 1) // chunk
    finally:
        fr.close()


# ------------------------------------------------------------------ chunk and part layouts
@pytest.mark.parametrize("chunk,offset", [(200000, 0), (100003, 0), (300001, 3)])
def test_device_ragged_chunks(devmock, zstd, oracle, chunk, offset):
    """chunks that are no multiple of 16 (staged at another pitch) and chunks above 128 KiB that are no multiple of it (a short block
    inside every frame); near-raw and text data in turn, so that both ways of building a frame run"""
    plug, F = devmock
    data = K.near_raw_text(chunk, 3 * chunk + 3999, chunk)
    buf = DevBuf(plug, data, offset)
    fr = D.DeviceFront(3, 1, chunk, lib=F)
    try:
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, chunk, 1)
        st = fr.stats()
        assert st[0] + st[1] == 4 and st[1] >= 1, st
    finally:
        fr.close()


def test_device_many_blocks_in_one_part(devmock, zstd, oracle):
    """1000-byte chunks: 700 blocks in one compaction launch (more than one 512-block step of the scan)"""
    plug, F = devmock
    data = K.by_name("mix", 700 * 1000 - 17, seed=4)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, 1, 1000, lib=F)
    try:
        before = plug.lib.qzstd_mock_compact_launches()
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 1000, 1)
        assert plug.lib.qzstd_mock_compact_launches() == before + 1
    finally:
        fr.close()


@pytest.mark.parametrize("part,parts", [(3 * 65536 + 1, 4), (1000, 11)])
def test_device_part_sizes(devmock, zstd, oracle, part, parts, monkeypatch):
    """a part size that is no whole number of chunks (rounded down: 3 chunks) and one below a chunk (one chunk per part); the part
    count does not divide the chunk count"""
    plug, F = devmock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(part))
    data = K.by_name("text", 10 * 65536 + 999, seed=6)
    buf = DevBuf(plug, data)
    fr = D.DeviceFront(3, 1, 65536, lib=F)
    try:
        before = plug.lib.qzstd_mock_compact_launches()
        assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 65536, 1)
        assert plug.lib.qzstd_mock_compact_launches() == before + parts
    finally:
        fr.close()


def test_device_front_reused_across_sizes(devmock, zstd, oracle, monkeypatch):
    """one front for a large, a small and a large call: the slot buffers grow, then are reused"""
    plug, F = devmock
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(8 * 32768))
    fr = D.DeviceFront(3, 1, 32768, lib=F)
    try:
        for size, seed in ((40 * 32768 + 5, 1), (3 * 32768 - 7, 2), (50 * 32768 + 11, 3)):
            data = K.by_name("mix", size, seed=seed)
            buf = DevBuf(plug, data, seed)
            assert fr.compress_device(buf.addr, len(data)) == reference(zstd, oracle, data, 32768, 1), size
    finally:
        fr.close()
