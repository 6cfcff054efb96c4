"""GPU: QZSTD_frontCompressDeviceBatch (include/qzstd_frontend_device.h) and the gather kernel under it (qzstd_hip_gather,
include/qzstd_hip_device.h).  A list of GPU tensors of unequal sizes, dtypes and alignments compressed in one call must give, per tensor,
byte for byte the frames libzstd builds from the ORACLE's sequences for that tensor alone — the frames of one QZSTD_frontCompressDevice
call per tensor.  No tolerance anywhere."""
import ctypes as C

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


def tensor_bytes(t) -> bytes:
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = [c for c in range(len(w)) if c >= len(g) or g[c] != w[c]]
        assert len(g) == len(w) and not bad, "tensor %d: frames %s differ (%d frames, want %d)" % (i, bad[:6], len(g), len(w))


def reference(zstd, oracle, datas, chunk, level):
    return [D.reference_frames(zstd, oracle, d, chunk, level) if d else [] for d in datas]


# ------------------------------------------------------------------ the gather kernel alone, through the C ABI
GATHER_LENS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 131072, (1 << 20) + 3]
GUARD = 64


def gather_api(plug):
    L = plug.lib
    L.qzstd_hip_gather.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def gather_case():
    """rows at each of the 16 source alignments x every length, long and short interleaved, cut out of ONE byte tensor so that the last
    rows end on the tensor's last byte -> (source bytes, [(source offset, stage offset, len, pad)], stage bytes)"""
    rng = np.random.default_rng(16)
    order = [(a, n) for a in range(16) for n in GATHER_LENS]
    order = [order[i] for i in rng.permutation(len(order))]
    spec, pos, so = [], 0, 0
    for k, (a, n) in enumerate(order):
        pos = ((pos + 15) & ~15) + a  # this row's source alignment
        pad = (-n) % 16 + (16 if k % 5 == 0 else 0)
        so += 32 if k % 7 == 0 else 0  # some gaps in the stage: they keep what they held
        spec.append((pos, so, n, pad))
        pos += n
        so += n + pad
    # the tail: rows that end exactly on the source's last byte, at each alignment of their start
    total = pos + 4096
    for a in range(16):
        n = 100 + a
        spec.append((total - n, so, n, (-n) % 16))
        so += n + (-n) % 16
    return rng.integers(0, 256, total, dtype=np.uint8), spec, so


def run_gather(plug, L, src_t, spec, stage_bytes, stage_skew=0):
    """-> (return value, the stage with its guards as numpy)"""
    stage = torch.full((GUARD + stage_bytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    base = stage.data_ptr() + (-stage.data_ptr()) % 16  # (torch allocations are aligned: 0)
    rows = (D.GatherRow * max(len(spec), 1))()
    for r, (s, d, n, p) in zip(rows, spec):
        r.src, r.dstOff, r.len, r.pad = src_t.data_ptr() + s, d, n, p
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_gather(0, None, rows, len(spec), d_rows, base + GUARD + stage_skew, stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, stage.cpu().numpy()[base - stage.data_ptr():]


def test_gather_kernel_every_alignment_and_length(gpu_plugin):
    L = gather_api(gpu_plugin)
    src, spec, stage_bytes = gather_case()
    src_t = torch.from_numpy(src).to("cuda:0")
    assert any(s + n == len(src) for s, _, n, _ in spec)  # rows end on the tensor's last byte
    assert {(src_t.data_ptr() + s) % 16 for s, _, n, _ in spec if n == 131072} == set(range(16))
    rc, got = run_gather(gpu_plugin, L, src_t, spec, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    want = np.full(len(got), 0xA5, dtype=np.uint8)
    for s, d, n, p in spec:
        want[GUARD + d:GUARD + d + n] = src[s:s + n]
        want[GUARD + d + n:GUARD + d + n + p] = 0
    bad = np.flatnonzero(got != want)
    assert not len(bad), "stage differs from the numpy gather at byte %d (of %d), %d bytes in all" % (bad[0] - GUARD, stage_bytes, len(bad))


def test_gather_launcher_refusals_leave_the_stage_untouched(gpu_plugin):
    L = gather_api(gpu_plugin)
    src = np.arange(8192, dtype=np.uint8)
    src_t = torch.from_numpy(src).to("cuda:0")
    good = [(3, 0, 100, 12), (500, 112, 0, 16), (1000, 128, 4000, 0)]
    cases = {"misaligned dstOff": [(3, 8, 100, 12)], "len + pad": [(3, 0, 100, 11)], "past stageBytes": good[:2] + [(1000, 128, 4000, 16)],
             "overlap": [good[0], (500, 96, 16, 0)], "not ascending": [good[2], good[0]]}
    for name, spec in cases.items():
        rc, got = run_gather(gpu_plugin, L, src_t, spec, 4128)
        assert rc < 0 and (got == 0xA5).all(), name
    rc, got = run_gather(gpu_plugin, L, src_t, good, 4128, stage_skew=8)
    assert rc < 0 and (got == 0xA5).all()
    rc, got = run_gather(gpu_plugin, L, src_t, [], 4128)
    assert rc == 0 and (got == 0xA5).all()
    rc, got = run_gather(gpu_plugin, L, src_t, good, 4128)
    assert rc == 0 and bytes(got[GUARD:GUARD + 100]) == bytes(src[3:103]) and (got[GUARD + 100:GUARD + 128] == 0).all()


# ------------------------------------------------------------------ the batch call
def mixed_tensors(chunk, seed):
    """separately allocated tensors of mixed dtypes, 1 byte .. 3 MiB, some of them views at odd byte offsets of a larger uint8 tensor"""
    sizes = [1, 15, 16, 4097, chunk - 1, chunk, chunk + 1, 3 * chunk + 777, 40000, 3 << 20, (1 << 20) + 8, 1 << 16]
    dtypes = [torch.uint8, torch.float16, torch.float32, torch.int64]
    gens = ("system", "mix", "text")
    out = []
    big = on_gpu(K.by_name("system", 700000, seed=seed))
    for i, n in enumerate(sizes):
        dt = dtypes[i % 4]
        n -= n % torch.empty(0, dtype=dt).element_size()
        if n == 0:
            dt, n = torch.uint8, sizes[i]
        out.append(on_gpu(K.by_name(gens[i % 3], n, seed=seed + i)).view(dt))
        if i % 3 == 0:  # a view with a storage offset, odd addresses among them
            o = 1 + 2 * i
            out.append(big[o:o + 5000 * (i + 1) + i])
    out.append(torch.empty(0, dtype=torch.float32, device="cuda:0"))
    return out


@pytest.mark.parametrize("level", [1, 3, 6, 12])
@pytest.mark.parametrize("chunk", [32768, 131072, 1 << 20])
def test_batch_frames_equal_the_oracles(front_lib, zstd, oracle, level, chunk):
    tensors = mixed_tensors(chunk, seed=level)
    assert any(t.data_ptr() % 2 for t in tensors)
    datas = [tensor_bytes(t) for t in tensors]
    fr = D.DeviceFront(8, level, chunk, lib=front_lib)
    try:
        got = D.compress_tensors(fr, tensors)
        same(got, reference(zstd, oracle, datas, chunk, level))
        st = fr.stats()
        assert st[0] + st[1] == sum(len(g) for g in got) and st[3] == sum(len(d) for d in datas), st
        for d, frames in zip(datas, got):
            for c in {0, len(frames) - 1} if frames else ():
                assert zstd.decompress(frames[c], chunk) == d[c * chunk:(c + 1) * chunk]
    finally:
        fr.close()


def test_batch_larger_than_one_part(front_lib, zstd, oracle):
    """80 MiB as 640 tensors of 128 KiB plus a few ragged ones: more than one default part (64 MiB), filled across tensor boundaries"""
    chunk = 131072
    data = K.by_name("system", 640 * chunk, seed=31)
    whole = on_gpu(data)
    want = D.reference_frames(zstd, oracle, data, chunk, 1)  # (the 640 tensors are the chunks of `data`: its frames, one each)
    tensors = [whole[i * chunk:(i + 1) * chunk].clone() for i in range(640)]
    expect = [[w] for w in want]
    for at, n in ((100, 77777), (400, 3), (len(tensors) + 2, 2 * chunk + 9)):
        d = K.by_name("mix", n, seed=n)
        tensors.insert(at, on_gpu(d))
        expect.insert(at, D.reference_frames(zstd, oracle, d, chunk, 1))
    fr = D.DeviceFront(16, 1, chunk, lib=front_lib)
    try:
        got = D.compress_tensors(fr, tensors)
        same(got, expect)
        assert sum(len(g) for g in got) == 640 + 1 + 1 + 3 and fr.stats()[3] == 640 * chunk + 77777 + 3 + 2 * chunk + 9
    finally:
        fr.close()


def test_batch_4096_small_buffers(front_lib, zstd, oracle):
    """4096 tensors of 4 KiB in one call: every frame decodes, the counters add up, and a call per tensor gives the same frames"""
    whole = K.by_name("system", 4096 * 4096, seed=41)
    tensors = [on_gpu(whole[i * 4096:(i + 1) * 4096]) for i in range(4096)]
    fr = D.DeviceFront(16, 1, 32768, lib=front_lib)
    try:
        hints = (C.c_ulong * 2)()
        fr.lib.QZSTD_frontStats.argtypes = [C.c_void_p, C.POINTER(C.c_ulong * 2)]
        got = D.compress_tensors(fr, tensors)
        st = fr.stats()
        fr.lib.QZSTD_frontStats(fr.f, C.byref(hints))  # (the announcement counters of the host path: the call must stay usable)
        assert all(len(g) == 1 for g in got) and st[0] + st[1] == 4096 and st[3] == len(whole), st
        assert st[2] < len(whole) + 4096 * 8 + 4096 * st[1], st
        for i, g in enumerate(got):
            assert zstd.decompress(g[0], 4096) == whole[i * 4096:(i + 1) * 4096], i
        for i in range(0, 4096, 97):
            assert got[i] == D.reference_frames(zstd, oracle, whole[i * 4096:(i + 1) * 4096], 32768, 1), i
    finally:
        fr.close()


def test_batch_equals_single_calls(front_lib):
    """the real kernels: the batch's frames are those of one QZSTD_frontCompressDevice call per tensor, with no more bytes device->host"""
    chunk = 131072
    tensors = [t for t in mixed_tensors(chunk, seed=9) if t.numel()]
    fr = D.DeviceFront(8, 1, chunk, lib=front_lib)
    try:
        s0 = fr.stats()
        single = [D.compress_tensor(fr, t) for t in tensors]
        s1 = fr.stats()
        batch = D.compress_tensors(fr, tensors)
        s2 = fr.stats()
        same(batch, single)
        assert s2[2] - s1[2] <= s1[2] - s0[2], (s0, s1, s2)
        assert s2[0] - s1[0] == s1[0] - s0[0] and s2[1] - s1[1] == s1[1] - s0[1] and s2[3] - s1[3] == s1[3] - s0[3]
    finally:
        fr.close()


def test_batch_stream_ordering(front_lib, zstd, oracle):
    """the tensors are written on a side stream right before the call, that stream is passed, the host never synchronises"""
    datas = [K.by_name("system", n, seed=12 + i) for i, n in enumerate([20 * 131072 + 333, 5000, 7 * 131072, 131072 + 1])]
    srcs = [on_gpu(d) for d in datas]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ts = [torch.empty_like(s) for s in srcs]
    fr = D.DeviceFront(8, 1, 131072, lib=front_lib)
    try:
        with torch.cuda.stream(side):
            for t, s in zip(ts, srcs):
                t.zero_()
                for _ in range(10):  # keep the side stream busy for a while before the bytes land
                    t.add_(1)
                t.copy_(s)
        got = D.compress_tensors(fr, ts, stream=side)
        same(got, reference(zstd, oracle, datas, 131072, 1))
        for d, frames in zip(datas, got):
            assert b"".join(zstd.decompress(f, 131072) for f in frames) == d
    finally:
        fr.close()


def test_batch_refusals_queue_nothing(front_lib, gpu_plugin):
    data = K.by_name("text", 4 * 32768, seed=2)
    host = C.create_string_buffer(data, len(data))
    pinned = gpu_plugin.lib.qzstd_hip_host_alloc(len(data))
    a, b = on_gpu(data), on_gpu(data[:1000])
    A, Bb = (a.data_ptr(), len(data)), (b.data_ptr(), 1000)
    fr = D.DeviceFront(2, 1, 32768, lib=front_lib)
    sw = D.DeviceFront(2, 1, 32768, use_producer=0, lib=front_lib)
    try:
        assert fr.compress_device_batch_raw([A, (C.addressof(host), len(data)), Bb])[0] == D.ERROR  # host memory in the middle
        assert fr.compress_device_batch_raw([A, (pinned, len(data)), Bb])[0] == D.ERROR  # pinned host memory
        assert fr.compress_device_batch_raw([A, Bb], dst_capacity=4 * fr.stride)[0] == D.ERROR  # 5 frames
        assert fr.compress_device_batch_raw([A, (0, 10)])[0] == D.ERROR
        assert sw.compress_device_batch_raw([A, Bb])[0] == D.ERROR
        assert fr.stats() == [0, 0, 0, 0]
        with pytest.raises(ValueError):
            D.compress_tensors(fr, [a, a.view(64, -1).t()])  # not contiguous
        with pytest.raises(ValueError):
            D.compress_tensors(fr, [a, torch.zeros(4)])  # a CPU tensor
        assert fr.compress_device_batch([A, Bb])[1] == fr.compress_device(*Bb)
    finally:
        fr.close()
        sw.close()
        gpu_plugin.lib.qzstd_hip_host_free(pinned)
