"""GPU: delta skip end to end on the real library (QZSTD_frontSetDeltaSkip with QZSTD_frontCompressDeviceBatchDelta /
QZSTD_frontRestoreDeviceBatchDelta: include/qzstd_frontend_device.h).  Six torch tensors, bf16 and fp32, from 1 KiB to 600 KiB at odd element
offsets of their pools: two identical to their bases, one that differs in a single element of its middle frame, one that differs in its last
byte only, one without a base, one changed everywhere.  With the setting on, the frames of chunks equal to their base chunk are the canonical
zero frames and every other frame is byte for byte the setting-off call's; the restore gives tensors torch.equal to the originals, into fresh
tensors and in place over copies of the bases; the stats match the counts worked out from the inputs.  Every comparison is byte-exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
PART = 2 * CHUNK
# (dtype, elements, what its base is)
SPEC = (
    ("bf16", 512, "same"),                    # 1 KiB
    ("fp32", 153600, "same"),                 # 600 KiB: four frames and a tail
    ("bf16", 3 * CHUNK // 2 + 5, "middle"),   # three frames and a tail of 10 bytes; one element of frame 1 differs
    ("fp32", 2 * CHUNK // 4 + 1, "last"),     # two frames and a tail of 4 bytes; its last byte differs
    ("bf16", 100000, None),                   # no base
    ("fp32", 50000, "step"),                  # every frame changed
)


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def tensors():
    """-> per tensor (the tensor, its base or None, element size), views at odd element offsets of two pools per dtype"""
    gen = torch.Generator().manual_seed(5)
    out = []
    pools = {}
    for dt, tdt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        total = sum(n + 64 for d, n, _ in SPEC if d == dt) + 64
        w = torch.empty(total, dtype=torch.float32).normal_(0.0, 0.02, generator=gen).to(tdt)
        pools[dt] = [w.to("cuda:0"), w.to("cuda:0").clone(), 1]
    for dt, n, kind in SPEC:
        cur, base, pos = pools[dt]
        pos |= 1  # an odd element offset: never 16-byte aligned
        t, b = cur[pos:pos + n], base[pos:pos + n]
        pools[dt][2] = pos + n + 33
        raw = b.view(torch.uint8)
        if kind == "middle":
            b[(CHUNK + CHUNK // 2) // t.element_size()] += 1.0
        elif kind == "last":
            raw[-1] ^= 1
        elif kind == "step":
            b += torch.empty(n, dtype=torch.float32).normal_(0.0, 1e-3, generator=gen).to(b.dtype).to("cuda:0") + 1e-3
        assert t.data_ptr() % 16 != 0
        out.append((t, None if kind is None else b, t.element_size()))
    torch.cuda.synchronize()
    return out


def bytes_of(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def xxh64_low_of_zeros(zstd, n):
    """the checksum field a frame of n zero bytes carries: the last four bytes of libzstd's own frame of them"""
    zc = zstd.cctx(1, checksumFlag=1)
    try:
        return zstd.compress2(zc, bytes(n))[-4:]
    finally:
        zstd.free(zc)


@pytest.mark.parametrize("checksum", (False, True), ids=("plain", "checksum"))
def test_skip_on_equals_off_and_restores(front_lib, zstd, tensors, monkeypatch, checksum):
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [(t.data_ptr(), t.numel() * k) for t, _, k in tensors]
    bases = [None if b is None else (b.data_ptr(), b.numel() * k) for _, b, k in tensors]
    elems = [k for _, _, k in tensors]
    datas = [bytes_of(t) for t, _, _ in tensors]
    bdatas = [None if b is None else bytes_of(b) for _, b, _ in tensors]
    lens = [[min(CHUNK, len(d) - o) for o in range(0, len(d), CHUNK)] for d in datas]
    eq = [[bd is not None and d[o:o + CHUNK] == bd[o:o + CHUNK] for o in range(0, len(d), CHUNK)] for d, bd in zip(datas, bdatas)]
    assert [sum(e) for e in eq] == [1, 5, 3, 2, 0, 0] and [len(e) for e in eq] == [1, 5, 4, 3, 2, 2]
    n_frames, n_equal = sum(len(e) for e in eq), sum(sum(e) for e in eq)
    n_based = sum(len(e) for e, bd in zip(eq, bdatas) if bd is not None)
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0 and fr.get_delta_skip() == 0
        off = fr.compress_device_batch_delta(bufs, bases, elems, stream)
        assert fr.delta_skip_stats() == [0, 0, 0, 0]
        dev0, d0 = fr.stats(), fr.delta_stats()
        assert fr.set_delta_skip(True) == 0
        on = fr.compress_device_batch_delta(bufs, bases, elems, stream)
        dev1, d1 = fr.stats(), fr.delta_stats()
        for i in range(len(tensors)):
            for c, (n, e) in enumerate(zip(lens[i], eq[i])):
                if e:
                    want = D.zero_frame(n, checksum) + (xxh64_low_of_zeros(zstd, n) if checksum else b"")
                    assert on[i][c] == want, (i, c)
                    assert zstd.decompress(on[i][c], CHUNK) == bytes(n)
                else:
                    assert on[i][c] == off[i][c], (i, c)
        assert fr.delta_skip_stats() == [n_based, n_equal, sum(len(d) for d, bd in zip(datas, bdatas) if bd is not None), 0]
        assert sum(dev1[:2]) - sum(dev0[:2]) == n_frames - n_equal and dev1[3] - dev0[3] == sum(len(d) for d in datas)
        assert sum(d1[:3]) - sum(d0[:3]) == n_based - n_equal
        # back into fresh tensors (0xA5-filled, with room around them) ...
        r0 = fr.restore_stats()
        fresh = [torch.full((len(d) + 128,), 0xA5, dtype=torch.uint8, device="cuda:0") for d in datas]
        outs = [(f.data_ptr() + 64 + (i % 2), len(d)) for i, (f, d) in enumerate(zip(fresh, datas))]
        assert fr.restore_batch_delta(on, outs, bases, elems, stream) == n_frames
        for i, (f, (t, _, _)) in enumerate(zip(fresh, tensors)):
            lo = 64 + (i % 2)
            assert torch.equal(f[lo:lo + len(datas[i])], t.contiguous().view(torch.uint8)), i
            assert bool((f[:lo] == 0xA5).all()) and bool((f[lo + len(datas[i]):] == 0xA5).all()), i
        r1 = fr.restore_stats()
        assert r1[0] - r0[0] == n_frames - n_equal and fr.delta_skip_stats()[3] == n_equal
        assert fr.delta_stats()[3] - d1[3] == n_based - n_equal
        # ... and in place over copies of the bases
        place = [torch.full_like(t, 7.0) if b is None else b.clone() for t, b, _ in tensors]
        pb = [(p.data_ptr(), len(d)) for p, d in zip(place, datas)]
        assert fr.restore_batch_delta(on, pb, [x if bd is not None else None for x, bd in zip(pb, bdatas)], elems, stream) == n_frames
        for i, (p, (t, _, _)) in enumerate(zip(place, tensors)):
            assert torch.equal(p, t), i
        assert fr.restore_stats()[0] - r1[0] == n_frames - n_equal and fr.delta_skip_stats()[3] == 2 * n_equal
        # the setting off: the same frames decode like any other
        assert fr.set_delta_skip(False) == 0
        again = [torch.empty_like(t) for t, _, _ in tensors]
        assert fr.restore_batch_delta(on, [(a.data_ptr(), len(d)) for a, d in zip(again, datas)], bases, elems, stream) == n_frames
        assert all(torch.equal(a, t) for a, (t, _, _) in zip(again, tensors))
    finally:
        fr.close()
    for (t, b, _), d, bd in zip(tensors, datas, bdatas):  # the calls only read their inputs
        assert bytes_of(t) == d and (b is None or bytes_of(b) == bd)
