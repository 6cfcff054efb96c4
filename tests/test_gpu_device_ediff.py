"""GPU: element differences in the device calls end to end on the real kernels (QZSTD_ELEM_DIFF in an elemSizes entry:
include/qzstd_frontend_device.h) — the mock test's batch (sizes 0, 256, 65791, 65792, 128 KiB + 255, 2 - 3 chunks with odd tails; element
sizes 1, 2, 4 and 8; six buffers flagged) cut out of one allocation at odd offsets.  Every flagged frame, decoded by libzstd (any decoder)
and taken through QZSTD_byteUngroup and QZSTD_elemSum, is its chunk; the unflagged buffers' frames are byte for byte those of the call
without flags; the restore into fresh buffers with guards leaves exactly the original bytes and QZSTD_frontCheckDeviceBatch says 0; the
refusals queue nothing.  Levels 1 and 6.  Every comparison is byte-exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
PART = 2 * CHUNK
GUARD = 64
FILL = 0xA5
SIZES = (2 * CHUNK + 1, CHUNK + 255, 256, 65791, 65792, 3 * CHUNK + 77, 2 * CHUNK + 100, 0, CHUNK + 5, 3 * CHUNK + 9)
ELEMS = (2, 1, 4, 1, 8, 2, 4, 2, 1, 8)
DIFF = (True, True, True, False, True, False, False, True, False, True)
FLAGS = tuple(k | (D.ELEM_DIFF if d else 0) for k, d in zip(ELEMS, DIFF))
N_FRAMES = sum(-(-n // CHUNK) for n in SIZES)
N_FLAGGED = sum(-(-n // CHUNK) for n, d in zip(SIZES, DIFF) if d)


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return D.bind_elemdiff(B.Front().lib)


def column(n, k, seed):
    """an integer column with order: steps U(5, 40) from a start just below the top of k bytes' range (it wraps), and a random tail"""
    rng = np.random.default_rng(seed)
    m, top = n // k, (1 << (8 * k)) - 1
    with np.errstate(over="ignore"):
        x = np.cumsum(rng.integers(5, 41, m, dtype=np.uint64)) + np.uint64(top - 100)
    return (x & np.uint64(top)).astype("<u%d" % k).tobytes() + bytes(rng.integers(0, 256, n - m * k, dtype=np.uint8))


@pytest.fixture(scope="module")
def tensors():
    """-> (the source tensor, [(address, bytes)] of the buffers, per buffer its bytes): computed once and never changed"""
    offs, pos = [], 1
    for i, n in enumerate(SIZES):
        offs.append(pos)
        pos += n + (2 * i + 1)  # odd distances: every alignment class, also ones that are no multiple of the element size
    data = np.frombuffer(D.typed_corpus("bf16", pos + 16, 7), dtype=np.uint8).copy()
    for i, (o, n, k, d) in enumerate(zip(offs, SIZES, ELEMS, DIFF)):
        if d:
            data[o:o + n] = np.frombuffer(column(n, k, 70 + i), dtype=np.uint8)
    t = torch.from_numpy(data).to("cuda:0")
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


@pytest.mark.parametrize("level", (1, 6))
def test_flagged_frames_decode_anywhere_and_come_back(front_lib, zstd, tensors, monkeypatch, level):
    t, bufs, datas = tensors
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(PART))
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    try:
        assert fr.set_checksum(1) == 0
        plain = fr.compress_device_batch_typed(bufs, ELEMS, stream)
        frames = fr.compress_device_batch_typed(bufs, FLAGS, stream)
        st = fr.elem_diff_stats()
        assert st[0] == N_FLAGGED and st[2:] == [0, 0]
        for i, (x, d, e) in enumerate(zip(frames, datas, FLAGS)):
            assert len(x) == -(-len(d) // CHUNK)
            for c, f in enumerate(x):
                ch = d[c * CHUNK:(c + 1) * CHUNK]
                got = D.ungroup_bytes(zstd.decompress(f, len(ch)), e & 0x7F, lib=front_lib)
                if e & D.ELEM_DIFF:
                    got = D.elem_sum(got, e & 0x7F, lib=front_lib)
                assert got == ch, (i, c)
            if not DIFF[i]:
                assert x == plain[i], i  # unflagged: byte for byte the call without flags
            elif len(d) >= 65536:
                assert sum(map(len, x)) < sum(map(len, plain[i])), i  # a column with order shrinks
        kept = fr.fingerprint(bufs, stream)
        out = Out()
        assert fr.restore_batch(frames, out.bufs, FLAGS, stream) == N_FRAMES
        out.check(datas)
        assert fr.check(out.bufs, kept, stream) == []
        st = fr.elem_diff_stats()
        assert st[2] == N_FLAGGED and st[3] >= 2
        assert np.array_equal(t.cpu().numpy()[bufs[0][0] - t.data_ptr():][:SIZES[0]], np.frombuffer(datas[0], dtype=np.uint8))  # only read
    finally:
        fr.close()


def test_refusals(front_lib, tensors):
    t, bufs, datas = tensors
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(4, 1, CHUNK, lib=front_lib)
    try:
        frames = fr.compress_device_batch_typed(bufs, FLAGS, stream)
        out = Out()
        st = (fr.elem_diff_stats(), fr.stats(), fr.restore_stats(), fr.verify_stats(), fr.slice_stats())
        for bad in (0x80, 0x83, 0xFF):
            es = list(FLAGS)
            es[5] = bad
            assert fr.compress_device_batch_typed_raw(bufs, es, stream)[0] == D.ERROR
            assert fr.restore_batch_raw(frames, out.bufs, es, stream) == D.ERROR
        based = [None] * len(SIZES)
        based[0] = (t.data_ptr() + 7, SIZES[0])
        assert fr.compress_device_batch_delta_raw(bufs, based, FLAGS, stream)[0] == D.ERROR
        assert fr.restore_batch_delta_raw(frames, out.bufs, based, FLAGS, stream) == D.ERROR
        assert fr.verify_raw(frames, bufs, None, FLAGS, stream)[0] == D.ERROR
        assert fr.restore_slices_raw(frames, SIZES, FLAGS, [(0, 16, 100, out.bufs[0][0], None)], stream) == D.ERROR
        assert (fr.elem_diff_stats(), fr.stats(), fr.restore_stats(), fr.verify_stats(), fr.slice_stats()) == st
        out.check([b""] * len(SIZES))  # nothing was written
    finally:
        fr.close()
