"""GPU: the delta calls end to end on the real kernels (QZSTD_frontCompressDeviceBatchDelta, QZSTD_frontRestoreDeviceBatchDelta:
include/qzstd_frontend_device.h).  Buffers and their bases are cut out of one allocation each at odd offsets, element sizes 1, 2, 4 and 8
mixed, every third buffer without a base, some bases identical to their buffers (frames of zeros).  The frames must be byte for byte those
of QZSTD_frontCompressDeviceBatchTyped over torch.bitwise_xor of the same buffers — checksums off and on — and decode with libzstd; the
restore must return the original bytes exactly, once into fresh buffers with guards and once in place over the bases.  Levels 1 and 6.
Every comparison is byte-exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
PART = 4 * CHUNK
GUARD = 64
FILL = 0xA5
ELEMS = [k for k in (2, 1, 8, 4) for _ in range(8)]
SIZES = [n for k in (2, 1, 8, 4) for n in (0, 1, 4095 * k + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + k + 1, (1 << 20) + 3)]
BASED = [i % 3 != 2 for i in range(len(SIZES))]          # every third buffer has no base
SAME = [on and i % 5 == 0 for i, on in enumerate(BASED)]  # a base identical to its buffer: a delta of zeros


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def tensors():
    """-> (source tensor, base tensor, [(address, bytes)] of the buffers, the same of the bases (None: none), per buffer its bytes, per buffer
    its base's bytes).  bf16 weights; a base is its buffer a small optimiser step earlier: most high bytes agree, the low bytes differ"""
    offs, boffs, pos, bpos = [], [], 1, 3
    for i, n in enumerate(SIZES):
        offs.append(pos)
        boffs.append(bpos)
        pos += n + (2 * i + 1)  # odd distances: every alignment class
        bpos += n + (2 * i + 5) % 16 + 1
    data = np.frombuffer(D.typed_corpus("bf16", pos + 16, 7), dtype=np.uint8).copy()
    rng = np.random.default_rng(8)
    bas = np.zeros(bpos + 16, dtype=np.uint8)
    for i, (o, bo, n) in enumerate(zip(offs, boffs, SIZES)):
        step = (rng.random(n) < 0.45) * rng.integers(1, 256, n) * (np.arange(n) % 2 == 0) + (rng.random(n) < 0.02) * (np.arange(n) % 2 == 1)
        bas[bo:bo + n] = data[o:o + n] if SAME[i] else data[o:o + n] ^ step.astype(np.uint8)
    t, b = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(bas).to("cuda:0")
    bufs = [(t.data_ptr() + o, n) for o, n in zip(offs, SIZES)]
    bases = [(b.data_ptr() + o, n) if on else None for o, n, on in zip(boffs, SIZES, BASED)]
    assert any((p - q[0]) % 16 for (p, _), q in zip(bufs, bases) if q)  # src and base differ mod 16
    views = [(t[o:o + n], b[bo:bo + n]) for o, bo, n in zip(offs, boffs, SIZES)]
    return t, b, bufs, bases, [data[o:o + n].tobytes() for o, n in zip(offs, SIZES)], [bas[o:o + n].tobytes() for o, n in zip(boffs, SIZES)], views


class Out:
    """a fresh 0xA5-filled byte tensor; buffer i at an odd offset of its own, GUARD bytes in front of the first and behind every one"""

    def __init__(self):
        self.place, pos = [], GUARD + 3
        for i, n in enumerate(SIZES):
            self.place.append(pos)
            pos += n + GUARD + (2 * i + 1)
        self.t = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda:0")
        self.bufs = [(self.t.data_ptr() + p, n) for p, n in zip(self.place, SIZES)]

    def fill(self, datas):
        for p, d in zip(self.place, datas):
            if d:
                self.t[p:p + len(d)] = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to("cuda:0")

    def check(self, datas):
        want = np.full(self.t.numel(), FILL, dtype=np.uint8)
        for p, d in zip(self.place, datas):
            want[p:p + len(d)] = np.frombuffer(d, dtype=np.uint8)
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert not len(bad), "byte %d differs (%d in all): got 0x%02x, want 0x%02x; buffers at %s" % (bad[0], len(bad), got[bad[0]], want[bad[0]],
                                                                                                     self.place)


def numpy_ungroup(b, k):
    a = np.frombuffer(b, dtype=np.uint8)
    m = len(a) // k
    return np.concatenate([a[:m * k].reshape(k, m).T.reshape(-1), a[m * k:]]).tobytes()


@pytest.mark.parametrize("checksum", (False, True))
@pytest.mark.parametrize("level", (1, 6))
def test_delta_frames_are_the_typed_frames_of_the_xored_buffers_and_come_back(front_lib, zstd, tensors, monkeypatch, level, checksum):
    t, b, bufs, bases, datas, bdatas, views = tensors
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(checksum) == 0
        # what a caller does today: torch.bitwise_xor into temporaries, then the Typed call
        xored = [torch.bitwise_xor(v, w) if on else v.clone() for (v, w), on in zip(views, BASED)]
        want = fr.compress_device_batch_typed([(x.data_ptr(), x.numel()) for x in xored], ELEMS, stream)
        plain = fr.compress_device_batch_typed(bufs, ELEMS, stream)
        dev0, d0 = fr.stats(), fr.delta_stats()
        got = fr.compress_device_batch_delta(bufs, bases, ELEMS, stream)
        dev1, d1 = fr.stats(), fr.delta_stats()
        n_frames = sum(len(per) for per in got)
        n_based = sum(len(per) for per, on in zip(got, BASED) if on)
        assert n_frames == sum(-(-n // CHUNK) for n in SIZES)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "buffer %d (%d bytes, elem %d, base %s): frames differ from the Typed call's over the XORed buffer" % (
                i, SIZES[i], ELEMS[i], BASED[i])
        assert all(got[i] == plain[i] for i, on in enumerate(BASED) if not on)
        assert all(bool(f[4] & 4) == checksum for per in got for f in per)
        # every frame decodes (libzstd verifies a checksum) to the grouped delta
        for i, (d, bd, k, on) in enumerate(zip(datas, bdatas, ELEMS, BASED)):
            content = (np.frombuffer(d, dtype=np.uint8) ^ np.frombuffer(bd, dtype=np.uint8)).tobytes() if on else d
            for c, f in enumerate(got[i]):
                assert numpy_ungroup(zstd.decompress(f, CHUNK), k) == content[c * CHUNK:(c + 1) * CHUNK], (i, c)
        # the stats add up: every frame built one way or the other, every frame with a base counted once, no block failed
        assert (dev1[0] - dev0[0]) + (dev1[1] - dev0[1]) == n_frames and dev1[3] - dev0[3] == sum(SIZES)
        assert sum(d1[:3]) - sum(d0[:3]) == n_based and d1[2] == d0[2] and d1[3] == d0[3]
        # back: into fresh buffers with guards ...
        out = Out()
        r0 = fr.restore_stats()
        assert fr.restore_batch_delta(got, out.bufs, bases, ELEMS, stream) == n_frames
        out.check(datas)
        r1 = fr.restore_stats()
        assert r1[0] - r0[0] == n_frames and r1[1] - r0[1] == sum(SIZES) and fr.delta_stats()[3] == d1[3] + n_based
        # ... and in place over a copy of the bases (the buffers without one: over 0xA5)
        place = Out()
        place.fill([bd if on else b"" for bd, on in zip(bdatas, BASED)])
        assert fr.restore_batch_delta(got, place.bufs, [pb if on else None for pb, on in zip(place.bufs, BASED)], ELEMS, stream) == n_frames
        place.check(datas)
    finally:
        fr.close()
    # the compress call only read its inputs
    for (v, w), d, bd in zip(views, datas, bdatas):
        assert v.cpu().numpy().tobytes() == d and w.cpu().numpy().tobytes() == bd
