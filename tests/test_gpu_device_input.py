"""GPU: QZSTD_frontCompressDevice (include/qzstd_frontend_device.h) — data already in a GPU tensor compressed without a host copy of the
input: match-finder and compaction on the tensor's device, one dense D2H copy of entries + literals per part, frames built with
ZSTD_compressSequencesAndLiterals.  Frames must equal, byte for byte, the frames libzstd builds with ZSTD_compress2 from the ORACLE's
sequences (tools/qz_device.reference_frames); plus the compaction kernel itself, through the C ABI, against a numpy extraction."""
import ctypes as C
import os

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B
import qz_corpus as K

torch = D.torch
pytestmark = pytest.mark.gpu


def on_gpu(data: bytes):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0") if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


def check(front_lib, zstd, oracle, data, chunk, level, threads=8, ext_rep=False, offset=0):
    fr = D.DeviceFront(threads, level, chunk, ext_rep=1 if ext_rep else 0, lib=front_lib)
    try:
        t = on_gpu(b"\0" * offset + data)[offset:]
        got = D.compress_tensor(fr, t)
        want = D.reference_frames(zstd, oracle, data, chunk, level, ext_rep)
        bad = [c for c in range(len(want)) if c >= len(got) or got[c] != want[c]]
        assert len(got) == len(want) and not bad, "frames %s differ (level %d, chunk %d, offset %d)" % (bad[:8], level, chunk, offset)
        for c in (0, len(got) - 1) if got else ():
            blk = data[c * chunk:(c + 1) * chunk]
            assert zstd.decompress(got[c], len(blk)) == blk
        return fr.stats()
    finally:
        fr.close()


@pytest.mark.parametrize("level", [1, 3, 6, 12])
@pytest.mark.parametrize("chunk", [32768, 131072, 1 << 20])
def test_device_frames_equal_the_oracles(front_lib, zstd, oracle, level, chunk):
    blocks = {32768: 40, 131072: 24, 1 << 20: 4}[chunk]
    data = K.by_name("system", blocks * chunk + 4321, seed=level)  # a ragged last chunk
    st = check(front_lib, zstd, oracle, data, chunk, level)
    n = (len(data) + chunk - 1) // chunk
    assert st[0] + st[1] == n and st[3] == len(data), st


def test_device_frames_external_repcodes(front_lib, zstd, oracle, monkeypatch):
    monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    check(front_lib, zstd, oracle, K.by_name("system", 30 * 131072 + 999, seed=7), 131072, 1, ext_rep=True)


def test_device_several_parts(front_lib, zstd, oracle, monkeypatch):
    """the double-buffered pipeline: many parts, each fetched while the workers code the one before"""
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(4 << 20))
    check(front_lib, zstd, oracle, K.by_name("system", 37 * (1 << 20) + 12345, seed=8), 131072, 1, threads=16)


@pytest.mark.parametrize("gen,raw", [("text", False), ("incompressible", True), ("mix", None)])
def test_device_fallback_path(front_lib, zstd, oracle, gen, raw):
    if gen == "incompressible":
        data = np.random.default_rng(3).integers(0, 256, 16 * 131072, dtype=np.uint8).tobytes() + K.by_name("text", 8 * 131072, seed=3)
    else:
        data = K.by_name(gen, 24 * 131072 + 77, seed=4)
    st = check(front_lib, zstd, oracle, data, 131072, 1)
    n = (len(data) + 131071) // 131072
    assert st[0] + st[1] == n, st
    if raw is True:
        assert st[1] > 0, st
    elif raw is False:
        assert st[1] == 0, st


@pytest.mark.parametrize("offset,size", [(1, 10 * 32768 + 5), (3, 32768 * 3), (15, 123457), (0, 32768 * 4 + 9), (0, 11), (7, 5), (0, 0)])
def test_device_misaligned_and_short(front_lib, zstd, oracle, offset, size):
    check(front_lib, zstd, oracle, K.by_name("mix", size, seed=offset + 1), 32768, 1, threads=4, offset=offset)


def test_device_d2h_traffic(front_lib, zstd, oracle):
    chunk = 131072
    data = K.by_name("system", 32 * chunk, seed=11)
    prof = oracle.profile(1, chunk)
    lits = seqs = 0
    for o in range(0, len(data), chunk):
        n, s = oracle.find(prof, data[o:o + chunk])
        seqs += n
        lits += int(np.frombuffer(s, dtype=np.uint32).reshape(-1, 4)[:n, 1].sum())
    st = check(front_lib, zstd, oracle, data, chunk, 1)
    assert st[1] == 0 and st[2] <= lits + 8 * seqs + 16 * 32 and st[2] < len(data), (st, lits, seqs)


def test_device_stream_ordering(front_lib, zstd, oracle):
    """the tensor is written on a side stream right before the call, that stream is passed, the host never synchronises"""
    data = K.by_name("system", 64 * 131072 + 333, seed=12)
    src = on_gpu(data)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    t = torch.empty_like(src)
    fr = D.DeviceFront(8, 1, 131072, lib=front_lib)
    try:
        with torch.cuda.stream(side):
            t.zero_()
            for _ in range(20):  # keep the side stream busy for a while before the bytes land
                t.add_(1)
            t.copy_(src)
        got = D.compress_tensor(fr, t, stream=side)
        assert got == D.reference_frames(zstd, oracle, data, 131072, 1)
    finally:
        fr.close()


def test_device_host_pointers_and_software_fronts_are_refused(front_lib, gpu_plugin):
    data = K.by_name("text", 4 * 32768, seed=2)
    host = C.create_string_buffer(data, len(data))
    pinned = gpu_plugin.lib.qzstd_hip_host_alloc(len(data))
    t = on_gpu(data)
    fr = D.DeviceFront(2, 1, 32768, lib=front_lib)
    sw = D.DeviceFront(2, 1, 32768, use_producer=0, lib=front_lib)
    try:
        assert fr.compress_device_raw(C.addressof(host), len(data))[0] == D.ERROR
        assert fr.compress_device_raw(pinned, len(data))[0] == D.ERROR
        assert fr.compress_device_raw(t.data_ptr(), len(data), dst_capacity=fr.stride)[0] == D.ERROR
        assert sw.compress_device_raw(t.data_ptr(), len(data))[0] == D.ERROR
        assert fr.stats() == [0, 0, 0, 0]
    finally:
        fr.close()
        sw.close()
        gpu_plugin.lib.qzstd_hip_host_free(pinned)


@pytest.mark.parametrize("level,short", [(1, False), (6, False), (1, True), (3, False), (12, False), (0x101, False)])
def test_compaction_kernel_bit_exact(gpu_plugin, oracle, level, short):
    """qzstd_hip_compact on a random ragged batch (one block marked failed): headers, packed entries and literal stream against a
    numpy extraction from the oracle's sequences.  short: an arena that holds the first blocks only — every block from the first one that
    does not fit is flagged and contributes nothing"""
    L = gpu_plugin.lib
    L.qzstd_hip_compact.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_size_t]
    L.qzstd_hip_compact_workspace_bytes.argtypes = [C.c_uint32]
    L.qzstd_hip_compact_workspace_bytes.restype = C.c_size_t
    rng = np.random.default_rng(level)
    lens = [int(x) for x in rng.integers(1, 131073, 23)] + [131072, 16, 7]
    blocks = [K.by_name(("system", "mix", "text")[i % 3], n, seed=i) for i, n in enumerate(lens)]
    bad = 5
    nb, cap = len(blocks), B.sequence_bound(131072)
    offs, total = [], 0
    for b in blocks:
        offs.append(total)
        total += (len(b) + 15) & ~15
    host = bytearray(total + 16)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = b
    desc = (B.HipBlock * nb)()
    for i, b in enumerate(blocks):
        desc[i].srcOff, desc[i].seqOff, desc[i].srcLen, desc[i].seqCap = offs[i], i * cap, len(b), cap
    arena_bytes = ((8 * nb + 15) & ~15) + 8 * nb * cap + total
    fit = nb
    if short:  # room for the entries and literals of blocks 0 .. 11 (block 5, failed, takes none)
        need = 0
        for i, b in enumerate(blocks[:12]):
            if i != bad:
                n, s = oracle.find(oracle.profile(level, len(b)), b, cap=cap)
                need += 8 * n + int(np.frombuffer(s, dtype=np.uint32).reshape(-1, 4)[:n, 1].sum())
        arena_bytes, fit = ((8 * nb + 15) & ~15) + need + 3, 12
    work = L.qzstd_hip_workspace_bytes(level, nb, 131072)
    cwork = L.qzstd_hip_compact_workspace_bytes(nb)
    ptrs = [L.qzstd_hip_malloc(0, n) for n in (len(host), C.sizeof(desc), nb * cap * 16, nb * 4, work, cwork, arena_bytes)]
    d_src, d_desc, d_seqs, d_cnt, d_work, d_cwork, d_arena = ptrs
    try:
        assert all(ptrs), gpu_plugin.err()
        hb = (C.c_char * len(host)).from_buffer(host)
        gpu_plugin.check(L.qzstd_hip_memcpy_h2d(0, None, d_src, hb, len(host)), "h2d")
        gpu_plugin.check(L.qzstd_hip_memcpy_h2d(0, None, d_desc, desc, C.sizeof(desc)), "h2d")
        gpu_plugin.check(L.qzstd_hip_find_sequences(0, None, level, d_src, d_desc, nb, 131072, d_seqs, d_cnt, d_work, work), "find")
        gpu_plugin.check(L.qzstd_hip_memset(0, None, d_cnt + 4 * bad, 0xFF, 4), "memset")  # the matcher "failed" this block
        gpu_plugin.check(L.qzstd_hip_compact(0, None, d_src, d_desc, nb, d_seqs, d_cnt, d_arena, arena_bytes, d_cwork, cwork), "compact")
        out = (C.c_char * arena_bytes)()
        gpu_plugin.check(L.qzstd_hip_memcpy_d2h(0, None, out, d_arena, arena_bytes), "d2h")
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        for p in ptrs:
            if p:
                L.qzstd_hip_free(0, p)
    arena = np.frombuffer(out, dtype=np.uint8)
    hdr = arena[:8 * nb].view(np.uint32).reshape(nb, 2)
    want_ent, want_lit = [], []
    for i, b in enumerate(blocks):
        if i == bad or i >= fit:
            assert hdr[i, 0] == 0xFFFFFFFF and hdr[i, 1] == 0, (i, hdr[i])
            continue
        n, s = oracle.find(oracle.profile(level, len(b)), b, cap=cap)
        q = np.frombuffer(s, dtype=np.uint32).reshape(-1, 4)[:n].astype(np.uint64)
        assert hdr[i, 0] == n and hdr[i, 1] == int(q[:, 1].sum()), (i, hdr[i], n)
        want_ent.append(q[:, 0] | (q[:, 1] << np.uint64(17)) | (q[:, 2] << np.uint64(35)))
        pos, src = 0, np.frombuffer(b, dtype=np.uint8)
        for off, lit, ml in q[:, :3].astype(np.int64):
            want_lit.append(src[pos:pos + lit])
            pos += lit + ml
    ent = np.concatenate(want_ent)
    lit = np.concatenate(want_lit)
    eo = (8 * nb + 15) & ~15
    assert eo + 8 * len(ent) + len(lit) <= arena_bytes
    assert np.array_equal(arena[eo:eo + 8 * len(ent)].view(np.uint64), ent)
    assert np.array_equal(arena[eo + 8 * len(ent):eo + 8 * len(ent) + len(lit)], lit)


# ------------------------------------------------------------------ near-raw blocks: libzstd stores them raw, so must the device path
def near_raw_input(chunk: int, seed: int) -> bytes:
    """random bytes with 0-3 % planted repeats per 128 KiB block (per chunk, when smaller); above 128 KiB: one block of each frame
    near-raw, the other text"""
    if chunk > 131072:
        return K.near_raw_text(seed, 4 * chunk)
    size = {16: 1024 * 16, 100: 600 * 100, 1024: 256 * 1024, 4096: 96 * 4096, 32768: 24 * 32768, 131072: 8 * 131072}[chunk] + chunk // 3
    return K.near_raw(seed, size, chunk)


@pytest.mark.parametrize("level,ext_rep", [(1, False), (3, False), (6, False), (12, False), (1, True)])
@pytest.mark.parametrize("chunk", [16, 100, 1024, 4096, 32768, 131072, 262144])
def test_device_near_raw_blocks(front_lib, zstd, oracle, chunk, level, ext_rep, monkeypatch):
    """a block whose compressed body does not beat its size by (size >> 6) + 2 bytes is stored raw by libzstd: such frames take the
    raw-bytes path and equal the reference; every frame is counted once"""
    if ext_rep:
        monkeypatch.setenv("QZSTD_HIP_EXT_REPCODES", "1")
    data = near_raw_input(chunk, seed=chunk + level)
    st = check(front_lib, zstd, oracle, data, chunk, level, threads=4, ext_rep=ext_rep)
    assert st[0] + st[1] == (len(data) + chunk - 1) // chunk and st[3] == len(data), st


@pytest.mark.parametrize("chunk,offset", [(200000, 0), (100003, 0), (300001, 3)])
def test_device_ragged_chunks(front_lib, zstd, oracle, chunk, offset):
    """chunks that are no multiple of 16 (staged at another pitch by a 2D copy) and chunks above 128 KiB that are no multiple of it (a
    short block inside every frame, read in place); near-raw and text chunks, so that both ways of building a frame run"""
    st = check(front_lib, zstd, oracle, K.near_raw_text(chunk, 3 * chunk + 3999, chunk), chunk, 1, threads=4, offset=offset)
    assert st[0] + st[1] == 4 and st[1] >= 1, st


def test_device_many_small_chunks_in_one_part(front_lib, zstd, oracle):
    """1000-byte chunks: 700 blocks in one compaction launch, more than one 512-block step of the scan"""
    check(front_lib, zstd, oracle, K.by_name("mix", 700 * 1000 - 17, seed=4), 1000, 1, threads=4)


def test_device_default_part_of_640_blocks(front_lib, zstd, oracle):
    """20 MiB at 32 KiB chunks with the default part size: one launch of 640 blocks"""
    st = check(front_lib, zstd, oracle, K.by_name("system", 20 << 20, seed=5), 32768, 1, threads=16)
    assert st[0] + st[1] == 640, st


@pytest.mark.parametrize("part", [3 * 65536 + 1, 1000])
def test_device_part_sizes(front_lib, zstd, oracle, part, monkeypatch):
    """a part size that is no whole number of chunks (rounded down to 3) and one below a chunk (one chunk per part); the part count
    does not divide the chunk count"""
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(part))
    check(front_lib, zstd, oracle, K.by_name("text", 10 * 65536 + 999, seed=6), 65536, 1, threads=4)


def test_device_front_reused_across_sizes(front_lib, zstd, oracle, monkeypatch):
    """one front for a large, a small and a large call: the slot buffers grow, then are reused"""
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(8 * 32768))
    fr = D.DeviceFront(4, 1, 32768, lib=front_lib)
    try:
        for size, seed in ((40 * 32768 + 5, 1), (3 * 32768 - 7, 2), (50 * 32768 + 11, 3)):
            data = K.by_name("mix", size, seed=seed)
            t = on_gpu(b"\0" * seed + data)[seed:]
            assert D.compress_tensor(fr, t) == D.reference_frames(zstd, oracle, data, 32768, 1), size
    finally:
        fr.close()
