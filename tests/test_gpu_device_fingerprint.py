"""GPU: QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch end to end on the real library and the real kernel
(include/qzstd_frontend_device.h).  Torch tensors of tests/test_gpu_device_verify.py's kind — bf16 and fp32, 1 KiB to 600 KiB, views at odd
element offsets of larger allocations, odd sizes, 128 KiB chunks: fp equals QZSTD_fingerprintOf (the plain-C function) over t.cpu()'s bytes;
after delta compress -> restore, in place over the bases and into fresh tensors, the check says 0; after a restore with the wrong base it
names exactly the frames whose base chunks differ; one bit flipped on the device is one frame; a front created with useProducer = 0 serves
the calls.  Under 4 MiB in all; every comparison is exact."""
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
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
    gen = torch.Generator().manual_seed(23)
    out, pools = [], {}
    for dt, tdt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        total = sum(n + 64 for d, n, _ in SPEC if d == dt) + 64
        w = torch.empty(total, dtype=torch.float32).normal_(0.0, 0.02, generator=gen).to(tdt)
        pools[dt] = [w.to("cuda:0"), w.to("cuda:0").clone(), 1]
    for dt, n, kind in SPEC:
        cur, base, pos = pools[dt]
        pos |= 1  # an odd element offset: never 16-byte aligned
        t, b = cur[pos:pos + n], base[pos:pos + n]
        pools[dt][2] = pos + n + 33
        if kind == "middle":
            b[(CHUNK + CHUNK // 2) // t.element_size()] += 1.0
        elif kind == "last":
            b.view(torch.uint8)[-1] ^= 1
        elif kind == "step":
            b += torch.empty(n, dtype=torch.float32).normal_(0.0, 1e-3, generator=gen).to(b.dtype).to("cuda:0") + 1e-3
        assert t.data_ptr() % 16 != 0
        out.append((t, None if kind is None else b, t.element_size()))
    torch.cuda.synchronize()
    return out


def bytes_of(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def chunks(d):
    return [d[o:o + CHUNK] for o in range(0, len(d), CHUNK)]


def test_fingerprints_equal_the_plain_c_function_over_the_tensors_bytes(front_lib, tensors):
    stream = torch.cuda.current_stream().cuda_stream
    live = [t for t, _, _ in tensors]
    bufs = [(t.data_ptr(), t.numel() * k) for t, _, k in tensors]
    datas = [bytes_of(t) for t in live]
    assert sum(len(d) for d in datas) < 2 << 20
    for producer in (1, 0):  # (a front without the producer serves the calls, like the restore)
        fr = D.DeviceFront(4, 1, CHUNK, use_producer=producer, lib=front_lib)
        try:
            r, fp, first = fr.fingerprint_raw(bufs, stream)
            want = [[D.fingerprint_of(ch, lib=front_lib) for ch in chunks(d)] for d in datas]
            assert r == sum(len(w) for w in want) and fp == [v for w in want for v in w]
            assert first[-1] == r and [first[i + 1] - first[i] for i in range(len(bufs))] == [len(w) for w in want]
            assert fp[:2] == [D.fingerprint_ref(chunks(datas[0])[0]), D.fingerprint_ref(chunks(datas[1])[0])]  # the second specification
            assert D.fingerprint_tensors(fr, live) == want
            assert D.check_tensors(fr, live, want) == []
            # one bit flipped on the device: just behind a 16 KiB tile boundary in the last full frame of the 600 KiB tensor, and the last byte
            # of a 10-byte tail frame
            live[1].view(torch.uint8)[3 * CHUNK + 16385] ^= 0x80
            live[2].view(torch.uint8)[3 * CHUNK + 9] ^= 0x10
            assert D.check_tensors(fr, live, want) == [(1, 3), (2, 3)]
            live[1].view(torch.uint8)[3 * CHUNK + 16385] ^= 0x80
            live[2].view(torch.uint8)[3 * CHUNK + 9] ^= 0x10
            assert D.check_tensors(fr, live, want) == []
            n = sum(len(w) for w in want)
            assert fr.fingerprint_stats() == [5 * n, 5 * sum(len(d) for d in datas), 5, 2]
            # refused before anything is queued: host memory, a wrong frame count
            assert fr.check_raw(bufs, [v for w in want for v in w][:-1])[0] == D.ERROR
            host = torch.zeros(4096, dtype=torch.uint8)
            assert fr.fingerprint_raw(bufs + [(host.data_ptr(), 4096)], stream)[0] == D.ERROR
            assert fr.fingerprint_stats()[2] == 5
        finally:
            fr.close()
    assert [bytes_of(t) for t in live] == datas  # only read


def test_compress_restore_check_and_the_wrong_base(front_lib, tensors):
    stream = torch.cuda.current_stream().cuda_stream
    live = [t for t, _, _ in tensors]
    bufs = [(t.data_ptr(), t.numel() * k) for t, _, k in tensors]
    bases = [None if b is None else (b.data_ptr(), b.numel() * k) for _, b, k in tensors]
    elems = [k for _, _, k in tensors]
    datas = [bytes_of(t) for t in live]
    bdatas = [None if b is None else bytes_of(b) for _, b, _ in tensors]
    n_frames = sum(len(chunks(d)) for d in datas)
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        kept = D.fingerprint_tensors(fr, live)  # 8 bytes per frame, kept with the frames
        frames = fr.compress_device_batch_delta(bufs, bases, elems, stream)
        # ---- fresh tensors
        fresh = [torch.full((t.numel() + 3,), 7, dtype=t.dtype, device="cuda:0")[3:] for t in live]
        fbufs = [(t.data_ptr(), t.numel() * k) for t, k in zip(fresh, elems)]
        assert fr.restore_batch_delta(frames, fbufs, bases, elems, stream) == n_frames
        assert D.check_tensors(fr, fresh, kept) == [] and [bytes_of(t) for t in fresh] == datas
        # ---- in place over copies of the bases (a tensor without a base: any bytes)
        inplace = [(t if b is None else b).clone() for t, b, _ in tensors]
        ibufs = [(t.data_ptr(), t.numel() * k) for t, k in zip(inplace, elems)]
        assert fr.restore_batch_delta(frames, ibufs, [None if b is None else ib for b, ib in zip(bases, ibufs)], elems, stream) == n_frames
        assert D.check_tensors(fr, inplace, kept) == []
        # ---- the wrong base for two tensors: the live tensor itself, as if the previous checkpoint were this one
        wrong = list(bases)
        wrong[2], wrong[3] = bufs[2], bufs[3]
        again = [torch.zeros_like(t) for t in live]
        abufs = [(t.data_ptr(), t.numel() * k) for t, k in zip(again, elems)]
        assert fr.restore_batch_delta(frames, abufs, wrong, elems, stream) == n_frames
        want = [(i, c) for i in (2, 3) for c, (a, b) in enumerate(zip(chunks(datas[i]), chunks(bdatas[i]))) if a != b]
        assert want == [(2, 1), (3, 2)]
        assert D.check_tensors(fr, again, kept) == want
        assert [(i, c) for i, t in enumerate(again) for c, (a, b) in enumerate(zip(chunks(bytes_of(t)), chunks(datas[i]))) if a != b] == want
        assert fr.fingerprint_stats()[3] == len(want)
    finally:
        fr.close()
    for (t, b, _), d, bd in zip(tensors, datas, bdatas):  # live tensors and bases: byte-identical before and after
        assert bytes_of(t) == d and (b is None or bytes_of(b) == bd)
