"""GPU: QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and QZSTD_frontVerifyDeviceSlices end to end on the real library
and kernels (include/qzstd_frontend_device.h).  The mock test's matrix, reduced: its buffers and element sizes, chunk sizes 16400 and
100003, the cuttings w17, w2048, frame, random and empties — every slice (and its base slice) a range of its own at a cycling misalignment
in one device tensor, in another order than the buffers' — level 1, every setting off and then all on.  Fingerprints, the frame a check
flags and the verify call's count and firstDiff[] must be exactly what the contiguous calls give for contiguous copies, unchanged and with
a planted byte on the live and on the base side; the sources are bit-identical afterwards.  And the whole cycle on real column views of a
[R, C] tensor: save the views, verify them, fingerprint them, restore into the views of a second tensor with guards around every
destination row, check those."""
import numpy as np
import pytest

import qz_bind as B
import qz_device as D  # (imports torch first: one HIP runtime)
import test_device_srcslices_mock as SS

torch = D.torch
pytestmark = pytest.mark.gpu

SIZES, ELEMS, BASED, CHUNKS = SS.SIZES, SS.ELEMS, SS.BASED, SS.CHUNKS
CUTTINGS = ("w17", "w2048", "frame", "random", "empties")
PLANT = (5, 300001 // 2 + 4321)  # (buffer, offset): inside a slice in the middle of a frame at both chunk sizes
FILL = 0xA5
ROWS, COLS, SPLIT = 300, 1000, 333


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return B.Front().lib


class Scattered:
    """one cutting of the corpus: every slice and every base slice a range of its own in ONE device tensor, placed in a shuffled order, the
    sources' misalignment cycling through 0 .. 15 and the bases' through another cycle, guard bytes between them"""

    def __init__(self, datas, bases, name, chunk):
        sizes = [SS.cut(name, n, chunk, 31 * i + chunk % 97) for i, n in enumerate(SIZES)]
        self.flat = [(i, o, s) for i, ss in enumerate(sizes) for o, s in zip(np.cumsum([0] + ss[:-1]).tolist(), ss)]
        order = np.random.default_rng(len(self.flat)).permutation(len(self.flat)).tolist()
        self.src, self.bas, pos = [0] * len(self.flat), [0] * len(self.flat), 64
        for rank, at in enumerate(order):
            s = self.flat[at][2]
            if s:
                self.src[at] = ((pos + 15) & ~15) + 16 + rank % 16
                pos = self.src[at] + s
                self.bas[at] = ((pos + 15) & ~15) + 16 + (7 * rank + 3) % 16
                pos = self.bas[at] + s
        self.host = np.full(pos + 64, FILL, dtype=np.uint8)
        for at, (i, o, s) in enumerate(self.flat):
            if s:
                self.host[self.src[at]:self.src[at] + s] = np.frombuffer(datas[i][o:o + s], dtype=np.uint8)
                self.host[self.bas[at]:self.bas[at] + s] = np.frombuffer(bases[i][o:o + s], dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).to("cuda:0")
        ends = [np.cumsum(ss) for ss in sizes]
        self.multi = int(sum(ends[i][int(np.searchsorted(ends[i], lo, side="right"))] < min(n, lo + chunk)
                             for i, n in enumerate(SIZES) for lo in range(0, n, chunk)))

    def slices(self, based):
        p = self.dev.data_ptr()
        return [(i, o, s, p + self.src[at] if s else 0, p + self.bas[at] if s and based[i] else None) for at, (i, o, s) in enumerate(self.flat)]

    def index(self, i, o, base=False):
        """where byte o of buffer i (of its base) lies in the tensor"""
        at = next(k for k, (b, off, s) in enumerate(self.flat) if b == i and s and off <= o < off + s)
        return (self.bas if base else self.src)[at] + o - self.flat[at][1]


@pytest.fixture(scope="module")
def world():
    datas, bases = SS.corpus()
    place, pos = [], 64
    for k, d in enumerate(datas + bases):  # the contiguous copies: one tensor, every buffer at a misalignment of its own
        pos = ((pos + 15) & ~15) + 16 + (5 * k + 1) % 16
        place.append(pos)
        pos += len(d)
    host = np.full(pos + 64, FILL, dtype=np.uint8)
    for at, d in zip(place, datas + bases):
        host[at:at + len(d)] = np.frombuffer(d, dtype=np.uint8)
    return dict(datas=datas, bases=bases, host=host, dev=torch.from_numpy(host).to("cuda:0"), place=place, cases={})


@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
@pytest.mark.parametrize("chunk", CHUNKS)
def test_answers_equal_the_contiguous_calls(front_lib, world, monkeypatch, chunk, settings):
    monkeypatch.setenv("QZSTD_FRONT_DEVICE_PART", str(3 * chunk))
    stream = torch.cuda.current_stream().cuda_stream
    whole = world["dev"]
    nb = len(SIZES)
    bufs = [(whole.data_ptr() + world["place"][i], n) for i, n in enumerate(SIZES)]
    bbufs = [(whole.data_ptr() + world["place"][nb + i], n) if on else None for i, (n, on) in enumerate(zip(SIZES, BASED))]
    fr = D.DeviceFront(8, 1, chunk, lib=front_lib)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        frames = fr.compress_device_batch_delta(bufs, bbufs, ELEMS, stream)
        n = sum(len(x) for x in frames)
        first = np.cumsum([0] + [len(x) for x in frames]).tolist()
        hit = first[PLANT[0]] + PLANT[1] // chunk
        fps = fr.fingerprint(bufs, stream)
        flat = [v for fp in fps for v in fp]
        assert fr.verify_raw(frames, bufs, bbufs, ELEMS, stream) == (0, [D.VERIFY_SAME] * n)
        for name in CUTTINGS:
            case = world["cases"].get((name, chunk)) or world["cases"].setdefault((name, chunk), Scattered(world["datas"], world["bases"], name, chunk))
            sl = case.slices(BASED)
            p0 = fr.slice_check_stats()
            assert fr.compress_device_slices(SIZES, ELEMS, sl, stream) == frames, name  # frames from the slices call and the Delta call alike
            assert fr.fingerprint_slices(SIZES, sl, stream) == fps, name
            assert fr.check_slices_raw(SIZES, sl, flat, stream) == (0, [0] * n), name
            assert fr.verify_slices_raw(frames, SIZES, ELEMS, sl, stream) == (0, [D.VERIFY_SAME] * n), name
            d = [b - a for a, b in zip(p0, fr.slice_check_stats())]
            assert case.multi > 0 and d[:3] == [3 * sum(1 for x in sl if x[2]), 3 * sum(SIZES), 3 * case.multi] and d[3] >= 3, name
            for base in (False, True):  # one planted byte, on the live side and on the base side, in the slices and in the contiguous copy
                a, b = case.index(*PLANT, base=base), world["place"][(nb if base else 0) + PLANT[0]] + PLANT[1]
                case.dev[a] ^= 0x40
                whole[b] ^= 0x40
                try:
                    got = fr.verify_slices_raw(frames, SIZES, ELEMS, sl, stream)
                    assert got == fr.verify_raw(frames, bufs, bbufs, ELEMS, stream), name
                    assert got == (1, [PLANT[1] % chunk if c == hit else D.VERIFY_SAME for c in range(n)]), name
                    chk = fr.check_slices_raw(SIZES, sl, flat, stream)
                    assert chk == fr.check_raw(bufs, flat, stream) and chk == ((0, [0] * n) if base else (1, [int(c == hit) for c in range(n)])), name
                finally:
                    case.dev[a] ^= 0x40
                    whole[b] ^= 0x40
            # a swapped element size and a wrong base (buffer 4 against itself) give the contiguous call's answers
            swapped = (2, 1, 4, 8, 4, 2)
            got = fr.verify_slices_raw(frames, SIZES, swapped, sl, stream)
            assert got == fr.verify_raw(frames, bufs, bbufs, swapped, stream) and got[0] >= 1, name
            wrong = [(i, o, s, p, (p if i == 4 else q)) for i, o, s, p, q in sl]
            got = fr.verify_slices_raw(frames, SIZES, ELEMS, wrong, stream)
            assert got == fr.verify_raw(frames, bufs, [bufs[4] if i == 4 else q for i, q in enumerate(bbufs)], ELEMS, stream) and got[0] >= 1, name
            assert np.array_equal(case.dev.cpu().numpy(), case.host), name  # the sources, the bases and the bytes between them: only read
        assert np.array_equal(whole.cpu().numpy(), world["host"])
    finally:
        fr.close()


def view_slices(buf, view, base_view=None):
    """a 2-D uint8 view whose rows are contiguous -> a source slice per row"""
    rows, width = view.shape
    assert view.stride(1) == 1
    return [(buf, r * width, width, view.data_ptr() + r * view.stride(0), None if base_view is None else base_view.data_ptr() + r * base_view.stride(0))
            for r in range(rows)]


@pytest.mark.parametrize("settings", (False, True), ids=("off", "checksum+probe+skip"))
def test_cycle_on_column_views(front_lib, settings):
    """save the views [:, :333] and [:, 333:] of a [300, 1000]-byte matrix against the views of a base, verify them, fingerprint them, restore
    them into the views of a second, wider matrix, check those — never a contiguous copy but for the oracle"""
    chunk = 16400
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    mat = np.frombuffer(D.typed_corpus("bf16", ROWS * COLS, 41), dtype=np.uint8).reshape(ROWS, COLS).copy()
    step = ((rng.random((ROWS, COLS)) < 0.25) * rng.integers(1, 256, (ROWS, COLS))).astype(np.uint8)
    step[200:, :SPLIT] = 0  # (the left view's last 100 rows equal their base: zero frames under the skip)
    t, tb = torch.from_numpy(mat).to("cuda:0"), torch.from_numpy(mat ^ step).to("cuda:0")
    sizes, elems = (ROWS * SPLIT, ROWS * (COLS - SPLIT)), (2, 4)
    sl = view_slices(0, t[:, :SPLIT], tb[:, :SPLIT]) + view_slices(1, t[:, SPLIT:], tb[:, SPLIT:])
    fr = D.DeviceFront(8, 1, chunk, lib=front_lib)
    try:
        if settings:
            assert fr.set_checksum(1) == 0 and fr.set_plane_probe(1) == 0 and fr.set_delta_skip(1) == 0
        frames = fr.compress_device_slices(sizes, elems, sl, stream)
        n = sum(len(x) for x in frames)
        assert fr.verify_slices_raw(frames, sizes, elems, sl, stream) == (0, [D.VERIFY_SAME] * n)
        fps = fr.fingerprint_slices(sizes, sl, stream)
        keep = [t[:, :SPLIT].contiguous(), t[:, SPLIT:].contiguous()]  # (the oracle)
        assert fps == fr.fingerprint([(x.data_ptr(), x.numel()) for x in keep], stream)
        assert fr.slice_check_stats()[2] == 2 * n  # every frame of a view is made of several rows
        out = torch.full((ROWS, COLS + 24), FILL, dtype=torch.uint8, device="cuda:0")
        back = [(b, o, s, out.data_ptr() + (o // (SPLIT if b == 0 else COLS - SPLIT)) * out.stride(0) + 5 + (SPLIT if b else 0), q) for b, o, s, _, q in sl]
        assert fr.restore_slices(frames, sizes, elems, back, stream) == n
        flat = [v for fp in fps for v in fp]
        assert fr.check_slices_raw(sizes, back, flat, stream) == (0, [0] * n)
        assert fr.verify_slices_raw(frames, sizes, elems, back, stream)[0] == 0
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:, 5:5 + COLS], mat) and (o[:, :5] == FILL).all() and (o[:, 5 + COLS:] == FILL).all()
        # a byte of the restored view changes: the check names its frame, the verify call its offset
        out[77, 5 + 100] ^= 1
        at = 77 * SPLIT + 100
        assert fr.check_slices_raw(sizes, back, flat, stream) == (1, [int(c == at // chunk) for c in range(n)])
        assert fr.verify_slices_raw(frames, sizes, elems, back, stream) == (1, [at % chunk if c == at // chunk else D.VERIFY_SAME for c in range(n)])
        assert np.array_equal(t.cpu().numpy(), mat)
    finally:
        fr.close()
