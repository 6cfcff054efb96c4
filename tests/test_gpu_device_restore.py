"""GPU: the restore calls end to end on the real kernels (QZSTD_frontRestoreDeviceBatchTyped, include/qzstd_frontend_device.h): what
QZSTD_frontCompressDeviceBatchTyped wrote from buffers cut out of one tensor at odd offsets, with mixed element sizes, comes back byte for
byte into fresh tensors — strided and compacted frames, foreign frames, checksums off and on — with the guard bytes around every buffer
intact; a damaged frame fails the call and leaves the front usable.  128 KiB chunks in parts of two, so that at least three parts run and
both restore slots are reused.  Every comparison is byte-exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
PART = 262144
SIZES = (0, 1, 7, 8191, 131072, 131073, 300001, 1 << 20)
ELEMS = (4, 1, 2, 8, 0, 2, 4, 2)  # 0: the front's setting
FRONT_ELEM = 8
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def source():
    """one byte tensor of bf16 weights; buffer i is SIZES[i] bytes of it from an odd offset on -> (tensor, [(address, bytes)], [bytes])"""
    offs, pos = [], 1
    for i, n in enumerate(SIZES):
        offs.append(pos)
        pos += n + (2 * i + 1)  # the next buffer's offset: odd distances, every alignment class over the eight
    data = np.frombuffer(D.typed_corpus("bf16", pos + 16, 7), dtype=np.uint8)
    t = torch.from_numpy(data.copy()).to("cuda:0")
    return t, [(t.data_ptr() + o, n) for o, n in zip(offs, SIZES)], [data[o:o + n].tobytes() for o, n in zip(offs, SIZES)]


class Out:
    """a fresh 0xA5-filled byte tensor; buffer i at an odd offset of its own, GUARD bytes in front of the first and behind every one"""

    def __init__(self):
        self.place, pos = [], GUARD + 3
        for i, n in enumerate(SIZES):
            self.place.append(pos)
            pos += n + GUARD + (2 * i + 1)
        self.t = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda:0")
        self.bufs = [(self.t.data_ptr() + p, n) for p, n in zip(self.place, SIZES)]

    def check(self, datas):
        want = np.full(self.t.numel(), FILL, dtype=np.uint8)
        for p, d in zip(self.place, datas):
            want[p:p + len(d)] = np.frombuffer(d, dtype=np.uint8)
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert not len(bad), "byte %d differs (%d in all): got 0x%02x, want 0x%02x; buffers at %s" % (bad[0], len(bad), got[bad[0]], want[bad[0]],
                                                                                                     self.place)

    def guards_intact(self):
        got = self.t.cpu().numpy()
        keep = np.ones(len(got), dtype=bool)
        for p, n in zip(self.place, SIZES):
            keep[p:p + n] = False
        return bool((got[keep] == FILL).all())


@pytest.mark.parametrize("checksum", (False, True))
@pytest.mark.parametrize("level", (1, 6))
def test_typed_frames_come_back(front_lib, zstd, source, monkeypatch, level, checksum):
    t, bufs, datas = source
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_byte_group(FRONT_ELEM) == 0 and fr.set_checksum(checksum) == 0
        frames = fr.compress_device_batch_typed(bufs, ELEMS)
        n, sizes = fr.last
        assert n == sum(len(f) for f in frames) == 17 and all(bool(f[4] & 4) == checksum for per in frames for f in per)
        st0 = fr.restore_stats()
        out = Out()
        assert fr.restore_last(n, sizes, out.bufs, ELEMS) == n  # at the front's stride, where the compress call left them
        out.check(datas)
        st1 = fr.restore_stats()
        assert st1[0] - st0[0] == n and st1[1] - st0[1] == sum(SIZES) and st1[3] - st0[3] >= 3
        out = Out()
        assert fr.restore_last(n, sizes, out.bufs, ELEMS, compacted=True) == n  # QZSTD_frontCompact, frameStride 0
        out.check(datas)
        out = Out()
        assert fr.restore_batch(frames, out.bufs, ELEMS, stream=torch.cuda.current_stream().cuda_stream) == n  # from a copy of the frames
        out.check(datas)
    finally:
        fr.close()


@pytest.mark.parametrize("checksum", (False, True))
def test_foreign_frames(front_lib, zstd, source, monkeypatch, checksum):
    """ZSTD_compress2 over numpy-grouped chunks; a front created without the producer restores them"""
    t, bufs, datas = source
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))

    def numpy_group(b, k):
        a = np.frombuffer(b, dtype=np.uint8)
        m = len(a) // k
        return np.concatenate([a[:m * k].reshape(m, k).T.reshape(-1), a[m * k:]]).tobytes()

    zc = zstd.cctx(3, checksumFlag=1 if checksum else 0)
    try:
        frames = [[zstd.compress2(zc, numpy_group(d[o:o + CHUNK], e or FRONT_ELEM)) for o in range(0, len(d), CHUNK)] for d, e in zip(datas, ELEMS)]
    finally:
        zstd.free(zc)
    fr = D.DeviceFront(8, 1, CHUNK, use_producer=0, lib=front_lib)
    try:
        assert fr.set_byte_group(FRONT_ELEM) == 0
        for compact in (False, True):
            out = Out()
            assert fr.restore_batch(frames, out.bufs, ELEMS, compact=compact) == 17
            out.check(datas)
    finally:
        fr.close()


def test_a_damaged_checksummed_frame_fails_the_call_and_the_next_one_succeeds(front_lib, zstd, source, monkeypatch):
    t, bufs, datas = source
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        assert fr.set_byte_group(FRONT_ELEM) == 0 and fr.set_checksum(1) == 0
        frames = fr.compress_device_batch_typed(bufs, ELEMS)
        victim = frames[7][5]  # a frame of the last buffer: parts before it have been scattered when it is met
        bad = [list(per) for per in frames]
        bad[7][5] = victim[:len(victim) // 2] + bytes([victim[len(victim) // 2] ^ 0x40]) + victim[len(victim) // 2 + 1:]
        out = Out()
        assert fr.restore_batch_raw(bad, out.bufs, ELEMS) == D.ERROR
        assert out.guards_intact()
        assert fr.restore_batch(frames, out.bufs, ELEMS) == 17
        out.check(datas)
    finally:
        fr.close()
