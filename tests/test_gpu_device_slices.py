"""GPU: QZSTD_frontRestoreDeviceSlices end to end on the real kernels (include/qzstd_frontend_device.h).  The buffers of
tests/test_gpu_device_delta.py (element sizes 2 / 1 / 8 / 4, sizes around chunk multiples up to 1 MiB + 3, every third without a base) and behind
them a [96, 4096] bf16 and fp32 matrix are compressed ONCE per level and checksum setting by QZSTD_frontCompressDeviceBatchDelta; then
slices of them come back: (a) one odd-placed slice per buffer onto the bases' matching slices, (b) the same in place, (c) a column shard of
the matrices as 96 slices each into one contiguous destination, (d) slices that cover everything — the Delta restore's bytes —, (e) empty
slices only.  Every destination equals the numpy slice of the original, the guards stay 0xA5, and the frames decoded are exactly those that
intersect a non-empty slice, counted here from the sizes.  Levels 1 and 6, checksums off and on.  Every comparison is byte-exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import qz_bind as B
import test_device_slices_mock as S
import test_gpu_device_delta as G

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = G.CHUNK
PART = G.PART
GUARD = G.GUARD
FILL = G.FILL
MAT_R, MAT_C = 96, 4096
MATS = (len(G.SIZES), len(G.SIZES) + 1)  # the bf16 matrix, the fp32 matrix
SIZES = G.SIZES + [MAT_R * MAT_C * 2, MAT_R * MAT_C * 4]
ELEMS = G.ELEMS + [2, 4]
BASED = [i % 3 != 2 for i in range(len(SIZES))]
N_FRAMES = S.frames_of(SIZES, CHUNK)


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


@pytest.fixture(scope="module")
def tensors():
    """-> (source tensor, base tensor, [(address, bytes)] of the buffers, the same of the bases (None: none), per buffer its bytes, per buffer its
    base's bytes): buffers and bases cut out of one allocation each at odd offsets, a base a small step away from its buffer"""
    offs, boffs, pos, bpos = [], [], 1, 3
    for i, n in enumerate(SIZES):
        offs.append(pos)
        boffs.append(bpos)
        pos += n + (2 * i + 1)
        bpos += n + (2 * i + 5) % 16 + 1
    data = np.frombuffer(D.typed_corpus("bf16", pos + 16, 11), dtype=np.uint8).copy()
    m = MATS[1]
    data[offs[m]:offs[m] + SIZES[m]] = np.frombuffer(D.typed_corpus("fp32", SIZES[m], 12), dtype=np.uint8)
    rng = np.random.default_rng(13)
    step = (rng.random(bpos + 16) < 0.3) * rng.integers(1, 256, bpos + 16)
    bas = np.zeros(bpos + 16, dtype=np.uint8)
    for o, bo, n in zip(offs, boffs, SIZES):
        bas[bo:bo + n] = data[o:o + n] ^ step[bo:bo + n].astype(np.uint8)
    t, b = torch.from_numpy(data).to("cuda:0"), torch.from_numpy(bas).to("cuda:0")
    bufs = [(t.data_ptr() + o, n) for o, n in zip(offs, SIZES)]
    bases = [(b.data_ptr() + o, n) if on else None for o, n, on in zip(boffs, SIZES, BASED)]
    return t, b, bufs, bases, [data[o:o + n].tobytes() for o, n in zip(offs, SIZES)], [bas[o:o + n].tobytes() for o, n in zip(boffs, SIZES)]


@pytest.fixture(scope="module", params=[(1, False), (1, True), (6, False)], ids=("level1", "level1-checksum", "level6"))
def written(request, front_lib, tensors):
    """compressed once: (front, the frames per buffer)"""
    import os
    level, checksum = request.param
    t, b, bufs, bases, datas, bdatas = tensors
    old = os.environ.get("QZSTD_FRONT_DEVICE_PART")
    os.environ["QZSTD_FRONT_DEVICE_PART"] = str(PART)
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    assert fr.set_checksum(checksum) == 0
    frames = fr.compress_device_batch_delta(bufs, bases, ELEMS, torch.cuda.current_stream().cuda_stream)
    assert sum(len(per) for per in frames) == N_FRAMES and all(bool(f[4] & 4) == checksum for per in frames for f in per)
    yield fr, frames
    fr.close()
    if old is None:
        del os.environ["QZSTD_FRONT_DEVICE_PART"]
    else:
        os.environ["QZSTD_FRONT_DEVICE_PART"] = old


class Out:
    """a fresh 0xA5-filled byte tensor; destination i (sizes[i] bytes) at an odd offset of its own, GUARD bytes in front of the first and behind
    every one"""

    def __init__(self, sizes):
        self.place, pos = [], GUARD + 3
        for i, n in enumerate(sizes):
            self.place.append(pos)
            pos += n + GUARD + (2 * i + 1)
        self.t = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda:0")
        self.bufs = [(self.t.data_ptr() + p, n) for p, n in zip(self.place, sizes)]

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
        assert not len(bad), "byte %d differs (%d in all): got 0x%02x, want 0x%02x; destinations at %s" % (bad[0], len(bad), got[bad[0]],
                                                                                                         want[bad[0]], self.place)


def call(fr, frames, slices, dsts, bases, in_place=False):
    """one slices call -> the frames it must decode, counted from the sizes; its return value and the counters are checked against that"""
    need = len(S.touched(SIZES, CHUNK, slices))
    s0, r0, d0 = fr.slice_stats(), fr.restore_stats(), fr.delta_stats()
    r = D.restore_slices(fr, frames, SIZES, ELEMS, S.give(slices, dsts, bases, in_place), torch.cuda.current_stream())
    s1, r1, d1 = fr.slice_stats(), fr.restore_stats(), fr.delta_stats()
    assert r == need
    assert [b - a for a, b in zip(s0, s1)] == [sum(1 for s in slices if s[2]), sum(s[2] for s in slices), need, S.pieces(CHUNK, slices)]
    assert r1[0] - r0[0] == need
    assert d1[3] - d0[3] == len({(b, c) for b, c in S.touched(SIZES, CHUNK, slices) if bases[b] is not None}) and d1[:3] == d0[:3]
    return need


def test_one_odd_slice_per_buffer_fresh_and_in_place(written, tensors):
    fr, frames = written
    t, b, bufs, bases, datas, bdatas = tensors
    slices = S.odd_slices(SIZES)
    want = S.expected(datas, slices)
    out = Out([n for _, _, n in slices])  # (a)
    assert call(fr, frames, slices, out.bufs, bases) < N_FRAMES
    out.check(want)
    place = Out([n for _, _, n in slices])  # (b): over a copy of the base slices (the buffers without a base: over 0xA5)
    place.fill([bdatas[i][off:off + n] if BASED[i] else b"" for i, off, n in slices])
    call(fr, frames, slices, place.bufs, bases, in_place=True)
    place.check(want)


def test_column_shard_of_the_two_matrices(written, tensors):
    """(c): columns [3 C / 8, 4 C / 8) of each matrix, 96 slices, into ONE contiguous [R, C / 8] destination per matrix"""
    fr, frames = written
    t, b, bufs, bases, datas, bdatas = tensors
    c0, c1 = MAT_C // 8 * 3, MAT_C // 8 * 4
    slices = [s for m, item in zip(MATS, (2, 4)) for s in S.column_slices(m, MAT_R, MAT_C, item, c0, c1)]
    out = Out([MAT_R * (c1 - c0) * item for item in (2, 4)])
    dsts = [(out.bufs[j][0] + r * (c1 - c0) * item, 0) for j, item in enumerate((2, 4)) for r in range(MAT_R)]
    need = call(fr, frames, slices, dsts, bases)
    assert need == S.frames_of([SIZES[m] for m in MATS], CHUNK) < N_FRAMES  # every frame of the two matrices, none of the others
    want = []
    for m, item in zip(MATS, (2, 4)):
        a = np.frombuffer(datas[m], dtype=np.uint8).reshape(MAT_R, MAT_C * item)
        want.append(a[:, c0 * item:c1 * item].tobytes())
    out.check(want)


def test_column_shard_through_the_torch_helper(written, tensors):
    """restore_shards: the same shard and a row shard as tensors, the bases given as the shards of the base tensors"""
    fr, frames = written
    t, b, bufs, bases, datas, bdatas = tensors
    shapes = [(1, n) for n in G.SIZES] + [(MAT_R, MAT_C)] * 2
    dtypes = [torch.uint8] * len(G.SIZES) + [torch.bfloat16, torch.float32]
    full = [torch.from_numpy(np.frombuffer(datas[m], dtype=np.uint8).copy()).view(dt).reshape(MAT_R, MAT_C) for m, dt in zip(MATS, dtypes[-2:])]
    fullb = [torch.from_numpy(np.frombuffer(bdatas[m], dtype=np.uint8).copy()).view(dt).reshape(MAT_R, MAT_C) for m, dt in zip(MATS, dtypes[-2:])]
    c0, w = MAT_C // 8 * 3, MAT_C // 8
    # (the uint8 buffers in front of the matrices are described for the frame count alone, with the element sizes they were written with)
    shards = [(MATS[0], 1, c0, w), (MATS[1], 0, 12, 12)]
    sb = [fullb[0][:, c0:c0 + w].contiguous().to("cuda:0") if BASED[MATS[0]] else None,
          fullb[1][12:24].contiguous().to("cuda:0") if BASED[MATS[1]] else None]
    s0 = fr.slice_stats()
    outs = D.restore_shards(fr, frames, shapes, dtypes, shards, bases=sb, elems=ELEMS)
    s1 = fr.slice_stats()
    assert s1[0] - s0[0] == MAT_R + 1 and s1[2] - s0[2] == -(-SIZES[MATS[0]] // CHUNK) + 2  # (rows 12..23 of 16 KiB: frames 1 and 2 of the matrix)
    assert [tuple(o.shape) for o in outs] == [(MAT_R, w), (12, MAT_C)] and [o.dtype for o in outs] == dtypes[-2:]
    assert torch.equal(outs[0].cpu().view(torch.uint8), full[0][:, c0:c0 + w].contiguous().view(torch.uint8))
    assert torch.equal(outs[1].cpu().view(torch.uint8), full[1][12:24].contiguous().view(torch.uint8))


def test_slices_that_cover_everything_are_the_delta_restore(written, tensors):
    """(d)"""
    fr, frames = written
    t, b, bufs, bases, datas, bdatas = tensors
    ref = Out(SIZES)
    assert fr.restore_batch_delta(frames, ref.bufs, bases, ELEMS, torch.cuda.current_stream().cuda_stream) == N_FRAMES
    ref.check(datas)
    out = Out(SIZES)
    assert call(fr, frames, S.whole_slices(SIZES), out.bufs, bases) == N_FRAMES
    out.check(datas)
    assert torch.equal(out.t, ref.t)


def test_empty_slices_only(written, tensors):
    """(e): 0, and no counter moves"""
    fr, frames = written
    t, b, bufs, bases, datas, bdatas = tensors
    out = Out([16])
    before = fr.slice_stats(), fr.restore_stats(), fr.delta_stats(), fr.stats()
    for slices in ([], [(i, min(5, n), 0, out.bufs[0][0], None) for i, n in enumerate(SIZES)]):
        assert fr.restore_slices_raw(frames, SIZES, ELEMS, slices, torch.cuda.current_stream().cuda_stream) == 0
    assert (fr.slice_stats(), fr.restore_stats(), fr.delta_stats(), fr.stats()) == before
    out.check([b""])
