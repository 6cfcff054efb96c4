"""GPU: QZSTD_frontCompressDeviceSlices end to end on the real kernels (include/qzstd_frontend_device.h), with torch tensors that are NOT
contiguous: the column views [:, :333] and [:, 333:] of a [300, 1000]-byte matrix as two logical buffers (a slice per row), a tensor cut at
random into slices that lie scattered in another tensor, and one contiguous tensor as a single slice.  Every frame must be byte for byte
the frame QZSTD_frontCompressDeviceBatchDelta returns for `.contiguous()` copies — levels 1 and 6, chunk 16400, bf16 and fp32 element sizes,
with and without a strided base, with checksum, plane probe and delta skip off and on; the frames come back through
QZSTD_frontRestoreDeviceSlices into a second strided tensor; the sources are bit-identical afterwards; QZSTD_frontSrcSliceStats adds up."""
import numpy as np
import pytest

import qz_bind as B
import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 16400
ROWS, COLS, SPLIT = 300, 1000, 333
RAGGED = 5 * CHUNK + 77  # the tensor cut at random
WHOLE = 3 * CHUNK + 5    # the contiguous one
SIZES = (ROWS * SPLIT, ROWS * (COLS - SPLIT), RAGGED, WHOLE)
FILL = 0xA5


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


def view_slices(buf, view, base_view=None):
    """a 2-D uint8 view whose rows are contiguous -> a source slice per row"""
    rows, width = view.shape
    assert view.stride(1) == 1
    return [(buf, r * width, width, view.data_ptr() + r * view.stride(0), None if base_view is None else base_view.data_ptr() + r * base_view.stride(0))
            for r in range(rows)]


def multi_frames(slices):
    """per buffer: the frames that hold bytes of more than one slice"""
    out = []
    for i, n in enumerate(SIZES):
        ends = np.cumsum([x[2] for x in slices if x[0] == i and x[2]])
        out.append(sum(1 for lo in range(0, n, CHUNK) if ends[int(np.searchsorted(ends, lo, side="right"))] < min(n, lo + CHUNK)))
    return out


@pytest.fixture(scope="module")
def world():
    """the tensors, their bases (a small step away; the left view's last 100 rows and the whole contiguous tensor equal their base), the slices"""
    rng = np.random.default_rng(21)
    mat = np.frombuffer(D.typed_corpus("bf16", ROWS * COLS, 31), dtype=np.uint8).reshape(ROWS, COLS).copy()
    mat[:, SPLIT:] = np.frombuffer(D.typed_corpus("fp32", ROWS * (COLS - SPLIT), 32), dtype=np.uint8).reshape(ROWS, COLS - SPLIT)
    step = ((rng.random((ROWS, COLS)) < 0.25) * rng.integers(1, 256, (ROWS, COLS))).astype(np.uint8)
    step[200:, :SPLIT] = 0
    bmat = mat ^ step
    ragged = np.frombuffer(D.typed_corpus("fp32", RAGGED, 33), dtype=np.uint8).copy()
    bragged = ragged ^ ((rng.random(RAGGED) < 0.25) * rng.integers(1, 256, RAGGED)).astype(np.uint8)
    whole = np.frombuffer(D.typed_corpus("bf16", WHOLE, 34), dtype=np.uint8).copy()
    # the ragged tensor's slices: random cuts, scattered in another order and at every misalignment over one allocation (bases: another)
    points = sorted(set(rng.integers(1, RAGGED, 60).tolist()) | {CHUNK, 2 * CHUNK - 1, 3 * CHUNK + 1})
    cuts = list(zip([0] + points, points + [RAGGED]))
    order = rng.permutation(len(cuts)).tolist()
    place, bplace, pos, bpos = {}, {}, 64, 64
    for rank, at in enumerate(order):
        lo, hi = cuts[at]
        pos = ((pos + 15) & ~15) + 16 + rank % 16
        bpos = ((bpos + 15) & ~15) + 16 + (5 * rank + 3) % 16
        place[at], bplace[at] = pos, bpos
        pos += hi - lo
        bpos += hi - lo
    scat, bscat = np.full(pos + 64, FILL, dtype=np.uint8), np.full(bpos + 64, FILL, dtype=np.uint8)
    for at, (lo, hi) in enumerate(cuts):
        scat[place[at]:place[at] + hi - lo] = ragged[lo:hi]
        bscat[bplace[at]:bplace[at] + hi - lo] = bragged[lo:hi]
    dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    t = dict(mat=dev(mat), bmat=dev(bmat), scat=dev(scat), bscat=dev(bscat), whole=dev(whole))
    host = dict(mat=mat, bmat=bmat, scat=scat, bscat=bscat, whole=whole)

    def slices(with_bases):
        left, right = t["mat"][:, :SPLIT], t["mat"][:, SPLIT:]
        out = view_slices(0, left, t["bmat"][:, :SPLIT] if with_bases else None) + view_slices(1, right, t["bmat"][:, SPLIT:] if with_bases else None)
        out += [(2, lo, hi - lo, t["scat"].data_ptr() + place[at], t["bscat"].data_ptr() + bplace[at] if with_bases else None)
                for at, (lo, hi) in enumerate(cuts)]
        out.append((2, RAGGED, 0, 0, None))  # (an empty slice)
        out.append((3, 0, WHOLE, t["whole"].data_ptr(), t["whole"].data_ptr() if with_bases else None))  # (src == base: equal to its base)
        return out

    def contiguous(with_bases):
        """what a caller does today: .contiguous() copies, handed to the Delta call"""
        keep = [t["mat"][:, :SPLIT].contiguous(), t["mat"][:, SPLIT:].contiguous(), dev(ragged), t["whole"]]
        kb = [t["bmat"][:, :SPLIT].contiguous(), t["bmat"][:, SPLIT:].contiguous(), dev(bragged), t["whole"]] if with_bases else None
        return keep, kb

    return dict(t=t, host=host, slices=slices, contiguous=contiguous, cuts=cuts,
                datas=[mat[:, :SPLIT].tobytes(), mat[:, SPLIT:].tobytes(), ragged.tobytes(), whole.tobytes()],
                bases=[bmat[:, :SPLIT].tobytes(), bmat[:, SPLIT:].tobytes(), bragged.tobytes(), whole.tobytes()])


@pytest.mark.parametrize("with_bases", (False, True), ids=("nobase", "strided-bases"))
@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
@pytest.mark.parametrize("elems", ((2, 4, 4, 2), (4, 2, 1, 8)), ids=("bf16-fp32", "fp32-bf16-bytes-8"))
@pytest.mark.parametrize("level", (1, 6))
def test_frames_equal_the_delta_calls_and_come_back(front_lib, world, monkeypatch, level, elems, settings, with_bases):
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(4 * CHUNK))
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(8, level, CHUNK, lib=front_lib)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        keep, kb = world["contiguous"](with_bases)
        t0 = [fr.stats(), fr.byte_group_stats(), fr.delta_stats(), fr.delta_skip_stats(), fr.checksum_stats(), fr.plane_probe_stats()]
        want = fr.compress_device_batch_delta([(x.data_ptr(), x.numel()) for x in keep],
                                              None if kb is None else [(x.data_ptr(), x.numel()) for x in kb], elems, stream)
        t1 = [fr.stats(), fr.byte_group_stats(), fr.delta_stats(), fr.delta_skip_stats(), fr.checksum_stats(), fr.plane_probe_stats()]
        assert [len(x) for x in want] == [-(-n // CHUNK) for n in SIZES]
        sl = world["slices"](with_bases)
        p0 = fr.src_slice_stats()
        got = fr.compress_device_slices(SIZES, elems, sl, stream)
        t2 = [fr.stats(), fr.byte_group_stats(), fr.delta_stats(), fr.delta_skip_stats(), fr.checksum_stats(), fr.plane_probe_stats()]
        p1 = fr.src_slice_stats()
        for i in range(len(SIZES)):
            assert len(got[i]) == len(want[i])
            for c, (g, w) in enumerate(zip(got[i], want[i])):
                assert g == w, ("buffer", i, "frame", c)
        # every statistic but the bytes copied back (the raw-bytes path is taken by whichever frames the entropy stage decides) counts alike
        diff = lambda a, b: [[y - x for x, y in zip(p, q)] for p, q in zip(a, b)]  # noqa: E731
        d01, d12 = diff(t0, t1), diff(t1, t2)
        assert d12[0][3] == d01[0][3] == sum(SIZES) and d12[3] == d01[3] and sum(d12[0][:2]) == sum(d01[0][:2])
        if settings and with_bases:
            assert d12[3][0] == sum(len(x) for x in want) and d12[3][1] >= len(want[3]) + 1  # the equal frames were found piece by piece
        # the slice statistics add up: the slices, their bytes, frames of more than one slice (none skipped but where a skip can be), launches
        d = [b - a for a, b in zip(p0, p1)]
        assert d[0] == sum(1 for x in sl if x[2]) and d[1] == sum(SIZES)
        multi = multi_frames(sl)
        assert multi[0] == len(want[0]) and multi[1] == len(want[1]) and multi[2] >= len(want[2]) - 1 and multi[3] == 0
        # (with the skip on, the frames found equal outside the contiguous tensor are frames of the left view's last rows: of several slices)
        assert d[2] == sum(multi) - (d12[3][1] - len(want[3]) if settings and with_bases else 0) and 1 <= d[3] <= sum(len(x) for x in want)
        # the sources and the bases are bit-identical afterwards
        for name, a in world["host"].items():
            assert np.array_equal(world["t"][name].cpu().numpy(), a), name
        # back through the slices restore into a SECOND strided tensor and a second scattered one
        out = torch.full((ROWS, COLS + 24), FILL, dtype=torch.uint8, device="cuda:0")
        oscat = torch.full_like(world["t"]["scat"], FILL)
        owhole = torch.full((WHOLE + 32,), FILL, dtype=torch.uint8, device="cuda:0")
        back = []
        for (buf, off, size, src, base) in sl:
            if buf == 0:
                dst = out.data_ptr() + (off // SPLIT) * out.stride(0) + 5
            elif buf == 1:
                dst = out.data_ptr() + (off // (COLS - SPLIT)) * out.stride(0) + 5 + SPLIT
            elif buf == 2:
                dst = oscat.data_ptr() + (src - world["t"]["scat"].data_ptr()) if size else 0
            else:
                dst = owhole.data_ptr() + 7
            back.append((buf, off, size, dst, base))
        assert fr.restore_slices(got, SIZES, elems, back, stream) == sum(len(x) for x in got)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:, 5:5 + COLS], world["host"]["mat"]) and (o[:, :5] == FILL).all() and (o[:, 5 + COLS:] == FILL).all()
        assert np.array_equal(oscat.cpu().numpy(), world["host"]["scat"])
        w = owhole.cpu().numpy()
        assert np.array_equal(w[7:7 + WHOLE], world["host"]["whole"]) and (w[:7] == FILL).all() and (w[7 + WHOLE:] == FILL).all()
    finally:
        fr.close()


def test_one_contiguous_tensor_as_a_single_slice_is_the_typed_call(front_lib, world):
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(4, 1, CHUNK, lib=front_lib)
    try:
        t = world["t"]["whole"]
        want = fr.compress_device_batch_typed([(t.data_ptr(), WHOLE)], [2], stream)
        p0 = fr.src_slice_stats()
        assert fr.compress_device_slices([WHOLE], [2], [(0, 0, WHOLE, t.data_ptr(), None)], stream) == want
        # cut up but contiguous in memory: still the buffer it is cut from, and no frame is assembled from pieces
        cut = [(0, o, min(999, WHOLE - o), t.data_ptr() + o, None) for o in range(0, WHOLE, 999)]
        assert fr.compress_device_slices([WHOLE], [2], cut, stream) == want
        d = [b - a for a, b in zip(p0, fr.src_slice_stats())]
        assert d == [1 + len(cut), 2 * WHOLE, 0, 0]
        assert fr.compress_device_slices_raw([WHOLE], [2 | D.ELEM_DIFF], cut, stream)[0] == D.ERROR
        assert fr.compress_device_slices_raw([WHOLE], [2], cut[:-1], stream)[0] == D.ERROR
        host = np.zeros(64, dtype=np.uint8)
        assert fr.compress_device_slices_raw([64], [2], [(0, 0, 64, host.ctypes.data, None)], stream)[0] == D.ERROR
    finally:
        fr.close()
