"""GPU: the adviser end to end on the real library (QZSTD_frontAdviseDeviceBatch: include/qzstd_frontend_device.h) — the seven columns of
tools/ediff_ratio.py at 256 KiB each, plus buffers of sizes 0, k - 1 and 100003, all cut out of one allocation at odd addresses (also ones
that are no multiple of the element size).  est is the host function's (QZSTD_ediffCostOf summed over each buffer's chunks), advised is
the resolved element size with QZSTD_ELEM_DIFF exactly where the rule holds; the array goes as it is through
QZSTD_frontCompressDeviceBatchTyped and QZSTD_frontRestoreDeviceBatchTyped and the buffers come back byte for byte; the ordered columns
are advised and the Zipf ids are not; every refusal happens before anything is queued.  Every comparison is exact."""
import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import ediff_ratio as E
import qz_bind as B

torch = D.torch
pytestmark = pytest.mark.gpu

CHUNK = 131072
GUARD = 64
FILL = 0xA5
# (content, element size, bytes)
BUFS = tuple((kind, k, 262144) for kind, k in E.INPUTS) + (("offsets32", 4, 0), ("offsets32", 4, 3), ("timestamps64", 8, 7), ("walk16", 2, 1),
                                                          ("offsets32", 4, 100003), ("zipf_ids32", 4, 100003), ("timestamps64", 8, 100003))
ELEMS = tuple(k for _, k, _ in BUFS)
SIZES = tuple(n for _, _, n in BUFS)
N_FRAMES = sum(-(-n // CHUNK) for n in SIZES)


@pytest.fixture(scope="module")
def front_lib(gpu_plugin, zstd):
    return D.bind_elemdiff(D.bind(B.Front().lib))


@pytest.fixture(scope="module")
def tensors():
    """-> (the source tensor, [(address, bytes)] of the buffers, per buffer its bytes): computed once and never changed"""
    offs, pos = [], 1
    for i, n in enumerate(SIZES):
        offs.append(pos)
        pos += n + (2 * i + 1)  # odd distances: every alignment class, also ones that are no multiple of the element size
    data = np.full(pos + 16, FILL, dtype=np.uint8)
    for i, (o, (kind, k, n)) in enumerate(zip(offs, BUFS)):
        data[o:o + n] = np.frombuffer(E.column(kind, k, nbytes=(n + k - 1) // k * k, seed=i), dtype=np.uint8)[:n]
    t = torch.from_numpy(data).to("cuda:0")
    return t, [(t.data_ptr() + o, n) for o, n in zip(offs, SIZES)], [data[o:o + n].tobytes() for o, n in zip(offs, SIZES)]


def test_estimates_equal_the_host_function_and_the_advice_round_trips(front_lib, zstd, tensors):
    t, bufs, datas = tensors
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(8, 1, CHUNK, lib=front_lib)
    try:
        want_est = [D.ediff_cost(d, k, CHUNK, lib=front_lib) for d, k in zip(datas, ELEMS)]
        want_adv = [k | (D.ELEM_DIFF if D.ediff_advised(p, dd, lib=front_lib) else 0) for k, (p, dd) in zip(ELEMS, want_est)]
        r, adv, est = fr.advise_raw(bufs, ELEMS, stream)
        for i, (g, w) in enumerate(zip(est, want_est)):
            print("%-14s %6d bytes: P %d D %d (host %d %d) advised %#x" % (BUFS[i][0], SIZES[i], g[0], g[1], w[0], w[1], adv[i]))
        assert est == want_est and adv == want_adv and r == sum(1 for a in adv if a & D.ELEM_DIFF)
        flagged = {i for i, a in enumerate(adv) if a & D.ELEM_DIFF}
        for i, (kind, _, n) in enumerate(BUFS):
            if n >= 100003 and kind in ("offsets32", "timestamps64", "sorted_ids64", "walk16", "arange64"):
                assert i in flagged, (i, kind)
            if kind == "zipf_ids32" or n < ELEMS[i]:
                assert i not in flagged, (i, kind)
        assert fr.advise_stats() == [len(BUFS), len(flagged), sum(n // k * k for n, k in zip(SIZES, ELEMS)), 1]
        # the array as it is through the Typed calls
        frames = fr.compress_device_batch_typed(bufs, adv, stream)
        place, pos = [], GUARD + 3
        for i, n in enumerate(SIZES):
            place.append(pos)
            pos += n + GUARD + (2 * i + 1)
        out = torch.full((pos,), FILL, dtype=torch.uint8, device="cuda:0")
        assert fr.restore_batch(frames, [(out.data_ptr() + p, n) for p, n in zip(place, SIZES)], adv, stream) == N_FRAMES
        want = np.full(pos, FILL, dtype=np.uint8)
        for p, d in zip(place, datas):
            want[p:p + len(d)] = np.frombuffer(d, dtype=np.uint8)
        assert np.array_equal(out.cpu().numpy(), want)
        # where differences are advised they pay against plain grouping, buffer by buffer
        plain = fr.compress_device_batch_typed(bufs, ELEMS, stream)
        for i in flagged:
            assert sum(map(len, frames[i])) < sum(map(len, plain[i])), (i, BUFS[i])
        assert np.array_equal(t.cpu().numpy()[bufs[0][0] - t.data_ptr():][:SIZES[0]], np.frombuffer(datas[0], dtype=np.uint8))  # only read
        # a second call on the same front: the scratch is kept, the result is the same
        assert fr.advise_raw(bufs, ELEMS, stream) == (r, adv, est) and fr.advise_stats()[3] == 2
    finally:
        fr.close()


def test_refusals_and_input_without_an_element(front_lib, tensors):
    t, bufs, datas = tensors
    stream = torch.cuda.current_stream().cuda_stream
    fr = D.DeviceFront(2, 1, CHUNK, use_producer=0, lib=front_lib)  # (accepted without the producer)
    try:
        st = (fr.advise_stats(), fr.stats(), fr.restore_stats(), fr.fingerprint_stats())
        for bad in (0x80, 0x84, 3, 0xFF):
            es = list(ELEMS)
            es[4] = bad
            r, adv, _ = fr.advise_raw(bufs, es, stream)
            assert r == D.ERROR and set(adv) == {7}, bad
        assert fr.advise_raw(bufs, ELEMS, stream, null_advised=True)[0] == D.ERROR
        assert fr.advise_raw(bufs[:2] + [(0, 5)], ELEMS[:3], stream)[0] == D.ERROR  # a null pointer with a size
        host = np.zeros(4096, dtype=np.uint8)
        assert fr.advise_raw(bufs[:2] + [(host.ctypes.data, 4096)], ELEMS[:3], stream)[0] == D.ERROR  # host memory
        assert (fr.advise_stats(), fr.stats(), fr.restore_stats(), fr.fingerprint_stats()) == st
        # no buffers, or only buffers shorter than their element: the resolved sizes, 0, and no launch
        assert fr.advise_raw([], None, stream) == (0, [], [])
        short = [b for b, n, k in zip(bufs, SIZES, ELEMS) if n < k]
        assert len(short) == 4
        r, adv, est = fr.advise_raw(short, [k for n, k in zip(SIZES, ELEMS) if n < k], stream)
        assert (r, adv, est) == (0, [4, 4, 8, 2], [(0, 0)] * 4) and fr.advise_stats()[1:] == [0, 0, 0]
        r, adv, est = fr.advise_raw(bufs[:1], None, stream)  # the front's setting: 1
        assert r != D.ERROR and adv[0] & 0x7F == 1 and est[0] == D.ediff_cost(datas[0], 1, CHUNK, lib=front_lib)
    finally:
        fr.close()
