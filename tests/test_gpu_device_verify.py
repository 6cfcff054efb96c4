"""GPU: QZSTD_frontVerifyDeviceBatch end to end on the real library and the real kernels (include/qzstd_frontend_device.h).  The six torch
tensors of tests/test_gpu_device_skip.py's kind — bf16 and fp32, 1 KiB to 600 KiB, at odd element offsets of their pools; two identical to
their bases, one that differs in one element, one in its last byte, one without a base, one changed everywhere — compressed as delta frames
with delta skip off and on, then verified in parts of two frames: 0 after the compress; one bit flipped on the device in three places gives
exactly those frames and offsets; a base that IS the live tensor is accepted and compares the frames' content with zero; live tensors and
bases are byte-identical before and after.  Under 3 MiB in all; every comparison is exact."""
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
SAME = D.VERIFY_SAME


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def tensors():
    """-> per tensor (the tensor, its base or None, element size), views at odd element offsets of two pools per dtype"""
    gen = torch.Generator().manual_seed(11)
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


def flip(t, at, bit):
    """one bit of byte `at` of a tensor's memory, on the device"""
    t.view(torch.uint8)[at] ^= bit
    torch.cuda.synchronize()


@pytest.mark.parametrize("skip", (False, True), ids=("skip_off", "skip_on"))
def test_verify_after_compress_and_three_flipped_bits(front_lib, tensors, monkeypatch, skip):
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [(t.data_ptr(), t.numel() * k) for t, _, k in tensors]
    bases = [None if b is None else (b.data_ptr(), b.numel() * k) for _, b, k in tensors]
    elems = [k for _, _, k in tensors]
    datas = [bytes_of(t) for t, _, _ in tensors]
    bdatas = [None if b is None else bytes_of(b) for _, b, _ in tensors]
    sizes = [len(d) for d in datas]
    n_frames = sum(-(-n // CHUNK) for n in sizes)
    assert sum(sizes) + sum(len(b) for b in bdatas if b) < 3 << 20
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        assert fr.set_delta_skip(skip) == 0
        frames = fr.compress_device_batch_delta(bufs, bases, elems, stream)
        r0, s0, d0 = fr.restore_stats(), fr.delta_skip_stats(), fr.delta_stats()
        r, first = fr.verify_raw(frames, bufs, bases, elems, stream)
        assert (r, first) == (0, [SAME] * n_frames)
        st = fr.verify_stats()
        assert st[:3] == [n_frames, 0, sum(sizes)] and st[3] >= 3  # several parts: a slot is used again
        assert D.verify_tensors(fr, frames, [t for t, _, _ in tensors], [b for _, b, _ in tensors], group="dtype") == []
        # one bit flipped on the device in three places: byte 0 of the first tensor (a chunk equal to its base: a ZERO row with skip on), a byte
        # just behind a 16 KiB tile boundary in the last frame of the 600 KiB tensor, the last byte of a 10-byte tail frame
        flip(tensors[0][0], 0, 0x01)
        flip(tensors[1][0], 4 * CHUNK + 16385, 0x80)
        flip(tensors[2][0], 3 * CHUNK + 9, 0x10)
        assert fr.verify(frames, bufs, bases, elems, stream) == [(0, 0, 0), (1, 4, 16385), (2, 3, 9)]
        flip(tensors[0][0], 0, 0x01)
        flip(tensors[1][0], 4 * CHUNK + 16385, 0x80)
        flip(tensors[2][0], 3 * CHUNK + 9, 0x10)
        # ... and one bit of a base, in the middle of a frame
        flip(tensors[5][1], CHUNK + 777, 0x04)
        assert fr.verify(frames, bufs, bases, elems, stream) == [(5, 1, 777)]
        flip(tensors[5][1], CHUNK + 777, 0x04)
        assert fr.verify(frames, bufs, bases, elems, stream, compact=True) == []
        # a wrong element size is a difference, not a crash
        wrong = list(elems)
        wrong[5] = 2
        assert [x[0] for x in fr.verify(frames, bufs, bases, wrong, stream)] == [5, 5]
        # the restore's and the skip's counters do not count the verify
        assert (fr.restore_stats(), fr.delta_skip_stats(), fr.delta_stats()) == (r0, s0, d0)
    finally:
        fr.close()
    for (t, b, _), d, bd in zip(tensors, datas, bdatas):  # live tensors and bases: byte-identical before and after
        assert bytes_of(t) == d and (b is None or bytes_of(b) == bd)


def test_a_base_that_is_the_live_tensor(front_lib, tensors, monkeypatch):
    """bases[i].d_ptr == bufs[i].d_ptr: the frames of a tensor compressed against ITSELF are zeros, and verifying them against the tensor
    as its own base compares u[] with zero — accepted, 0; frames with other content differ at their first non-zero delta byte"""
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    stream = torch.cuda.current_stream().cuda_stream
    picked = [tensors[1], tensors[5]]
    bufs = [(t.data_ptr(), t.numel() * k) for t, _, k in picked]
    elems = [k for _, _, k in picked]
    datas = [bytes_of(t) for t, _, _ in picked]
    for skip in (False, True):
        fr = D.DeviceFront(4, 1, CHUNK, lib=front_lib)
        try:
            assert fr.set_delta_skip(skip) == 0
            frames = fr.compress_device_batch_delta(bufs, bufs, elems, stream)
            assert fr.verify(frames, bufs, bufs, elems, stream) == []
            # the frames written against the real base of the second tensor hold its delta: against itself they differ in every frame
            real = fr.compress_device_batch_delta(bufs[1:], [(picked[1][1].data_ptr(), bufs[1][1])], elems[1:], stream)
            got = fr.verify(real, bufs[1:], bufs[1:], elems[1:], stream)
            delta = bytes(x ^ y for x, y in zip(datas[1], bytes_of(picked[1][1])))
            want = [(0, c, next(i for i, v in enumerate(delta[c * CHUNK:(c + 1) * CHUNK]) if v)) for c in range(2)]
            assert got == want
        finally:
            fr.close()
    assert [bytes_of(t) for t, _, _ in picked] == datas
