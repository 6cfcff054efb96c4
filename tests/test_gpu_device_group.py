"""GPU: byte-grouped frames from GPU tensors (QZSTD_frontSetByteGroup, QZSTD_frontCompressDeviceBatchTyped: include/qzstd_frontend_device.h).
Separately allocated tensors of mixed dtypes, sizes and alignments, through compress_tensors(group="dtype") and through the single call: every
frame byte for byte the frame libzstd builds from the ORACLE's sequences over the grouped content, a block per plane
(qz_device.reference_frames_grouped), and restore_tensor() gives the tensor back.  No tolerance anywhere."""
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B
import qz_corpus as K

torch = D.torch
pytestmark = pytest.mark.gpu

KINDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32", torch.int64: "ids64", torch.uint8: "text"}


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


def on_gpu(data: bytes, dtype=torch.uint8):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0") if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")
    return t.view(dtype)


def tensor_bytes(t) -> bytes:
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def typed_tensors(chunk, seed, largest):
    """separately allocated tensors of bf16, fp16, fp32, int64 and uint8, 1 byte .. `largest`, byte views of a larger tensor at odd
    offsets, and typed views that start at an element offset of their allocation"""
    sizes = [1, 15, 16, 4097, 2 * 4096 * 2, chunk - 1, largest, chunk + 1, 2 * chunk + 4321, 40000, chunk, 65536 + 8]  # (largest: bf16)
    dtypes = [torch.uint8, torch.bfloat16, torch.float16, torch.float32, torch.int64]
    out = []
    big = on_gpu(D.typed_corpus("bf16", 300000, seed))
    for i, n in enumerate(sizes):
        dt = dtypes[i % 5]
        n -= n % torch.empty(0, dtype=dt).element_size()
        if n == 0:
            dt, n = torch.uint8, sizes[i]
        kind = KINDS[dt]
        data = K.by_name(kind, n, seed=seed + i) if kind == "text" else D.typed_corpus(kind, n, seed + i)
        out.append(on_gpu(data, dt))
        if i % 4 == 0:  # a view with a storage offset, odd addresses among them (bytes: a typed view needs an aligned address)
            o = 1 + 2 * i
            out.append(big[o:o + 9000 * (i + 1) + i])
    # typed views at element offsets: grouped rows whose source is not 16-byte aligned (2, 6, 4, 12 and 8 mod 16)
    for kind, dt, first, n in (("bf16", torch.bfloat16, 1, 70001), ("bf16", torch.bfloat16, 3, chunk // 2 + 5), ("fp32", torch.float32, 1, 40003),
                               ("fp16", torch.float16, 6, 9000), ("ids64", torch.int64, 1, 5000)):
        size = torch.empty(0, dtype=dt).element_size()
        whole = on_gpu(D.typed_corpus(kind, (first + n) * size, seed + first + n), dt)
        out.append(whole[first:first + n])
    out.append(torch.empty(0, dtype=torch.float32, device="cuda:0"))
    return out


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = [c for c in range(len(w)) if c >= len(g) or g[c] != w[c]]
        assert len(g) == len(w) and not bad, "tensor %d: frames %s differ (%d frames, want %d)" % (i, bad[:6], len(g), len(w))


def reference(zstd, oracle, data, chunk, level, k, checksum=False):
    if not data:
        return []
    if k == 1 and not checksum:
        return D.reference_frames(zstd, oracle, data, chunk, level)
    return D.reference_frames_grouped(zstd, oracle, data, chunk, level, k, checksum=checksum)


@pytest.mark.parametrize("level,chunk,largest", [(1, 4096, 1 << 20), (1, 131072, 3 << 20), (1, 393216, 3 << 20), (6, 131072, 1 << 20),
                                                 (12, 393216, 1 << 20), (12, 4096, 300000)])
def test_typed_batch_and_single_calls(front_lib, zstd, oracle, level, chunk, largest):
    tensors = typed_tensors(chunk, seed=level, largest=largest)
    assert any(t.data_ptr() % 2 for t in tensors)
    datas = [tensor_bytes(t) for t in tensors]
    ks = [D.element_group(t) for t in tensors]
    assert set(ks) == {1, 2, 4, 8}
    assert {k for t, k in zip(tensors, ks) if t.data_ptr() % 16} == {1, 2, 4, 8}  # unaligned sources at every element size
    want = [reference(zstd, oracle, d, chunk, level, k) for d, k in zip(datas, ks)]
    fr = D.DeviceFront(8, level, chunk, lib=front_lib)
    try:
        got = D.compress_tensors(fr, tensors, group="dtype")
        same(got, want)
        st, s = fr.stats(), fr.byte_group_stats()
        assert st[0] + st[1] == sum(len(g) for g in got) and st[3] == sum(len(d) for d in datas), st
        assert s[2] == 0 and sum(s) == sum(len(g) for g, k in zip(got, ks) if k > 1), s
        for t, frames, k in zip(tensors, got, ks):
            back = D.restore_tensor(frames, t.dtype, tuple(t.shape), k, "cuda:0", zstd=zstd)
            assert back.dtype == t.dtype and back.shape == t.shape and torch.equal(back.view(torch.uint8), t.contiguous().view(torch.uint8))
        # the single call, under the front's setting: every third tensor
        for t, w, k in list(zip(tensors, want, ks))[::3]:
            assert fr.set_byte_group(k) == 0
            if t.numel():
                same([D.compress_tensor(fr, t)], [w])
    finally:
        fr.close()


def test_checksums_on(front_lib, zstd, oracle):
    chunk = 131072
    tensors = [on_gpu(D.typed_corpus("bf16", 3 * chunk + 10, 1), torch.bfloat16), on_gpu(K.by_name("text", chunk + 77, seed=2)),
               on_gpu(D.typed_corpus("ids64", 2 * chunk, 3), torch.int64)]
    datas = [tensor_bytes(t) for t in tensors]
    ks = [2, 1, 8]
    fr = D.DeviceFront(4, 1, chunk, lib=front_lib)
    try:
        assert fr.set_checksum(1) == 0
        got = D.compress_tensors(fr, tensors, group="dtype")
        same(got, [reference(zstd, oracle, d, chunk, 1, k, checksum=True) for d, k in zip(datas, ks)])
        assert all(f[4] & 4 for g in got for f in g)  # Content_Checksum_Flag; restore_tensor's decoder verifies the hash
        for t, frames, k in zip(tensors, got, ks):
            assert torch.equal(D.restore_tensor(frames, t.dtype, tuple(t.shape), k, "cuda:0", zstd=zstd), t)
        assert sum(fr.checksum_stats()) == sum(len(g) for g in got)
    finally:
        fr.close()


def test_small_parts_reuse_a_stage_while_frames_are_rebuilt(front_lib, zstd, oracle, monkeypatch):
    """parts of two frames: a slot's stage takes part p + 2 while the workers still rebuild part p's frames from its arena"""
    chunk = 131072
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(2 * chunk))
    t = on_gpu(D.typed_corpus("bf16", 24 * chunk + 5000, 7), torch.bfloat16)
    data = tensor_bytes(t)
    fr = D.DeviceFront(4, 1, chunk, lib=front_lib)
    try:
        got = D.compress_tensors(fr, [t], group="dtype")
        same(got, [reference(zstd, oracle, data, chunk, 1, 2)])
        s = fr.byte_group_stats()
        assert s[1] > 0 and s[2] == 0 and sum(s) == 25, s
        assert torch.equal(D.restore_tensor(got[0], t.dtype, tuple(t.shape), 2, "cuda:0", zstd=zstd), t)
    finally:
        fr.close()
