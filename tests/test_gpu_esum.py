"""GPU: the element sum (qzstd_hip_esum, include/qzstd_hip_device.h) alone, through the C ABI, byte for byte against QZSTD_elemSum of
include/qzstd_elemdiff.h: every row of one launch becomes the running sum of its un-zigzagged elements, in place, at any alignment, and no
byte outside [dst, dst + n * k) of a row changes — not its tail, not its neighbours, not the guards.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
TILE = 16384
BIG = (1 << 20) + 3


def lens(k):
    return [0, 1, k - 1, k, TILE - k, TILE, TILE + k, 3 * TILE + 5]


@pytest.fixture(scope="module")
def L(gpu_plugin):
    return D.bind_ediff_kernels(gpu_plugin.lib)


def case(seed=11):
    """-> (buffer with 0xA5 between the rows, [(offset, len, elem)]): every alignment x element size x length in a shuffled order with guard
    bytes between the rows; one row of 1 MiB + 3 per element size (64 tiles and a bit: the rows behind have tile0 > 0); pairs of rows packed
    back to back that share a 16-byte word; at k = 8 a row of all-ones differences and one whose sums cross 2^32 in every tile."""
    rng = np.random.default_rng(seed)
    order = [(a, k, n) for a in range(16) for k in ELEMS for n in lens(k)]
    order = [order[i] for i in rng.permutation(len(order))]
    for i, k in enumerate(ELEMS):
        order.insert(7 + 90 * i, (5 * i + 1, k, BIG))
    spec, fill, pos = [], [], 64
    for a, k, n in order:
        pos = ((pos + 15) & ~15) + 16 + a
        spec.append((pos, n, k))
        fill.append(rng.integers(0, 256, n, dtype=np.uint8))
        pos += n
    for k in ELEMS:  # back to back: the second starts where the first ends, mid-word, at an offset that is no multiple of k
        pos = ((pos + 15) & ~15) + 16 + 3
        for n in (2 * TILE + 5 * k + (k - 1 if k > 1 else 0) + 6, TILE + 3 * k + 1, 40):
            spec.append((pos, n, k))
            fill.append(rng.integers(0, 256, n, dtype=np.uint8))
            pos += n
    for a, z in ((9, 2), (2, 2 * ((1 << 31) + 1))):  # d = 1 everywhere; d = 2^31 + 1 everywhere
        pos = ((pos + 15) & ~15) + 16 + a
        n = 5 * TILE + 24
        spec.append((pos, n, 8))
        fill.append(np.frombuffer(np.full(n // 8, z, dtype="<u8").tobytes(), dtype=np.uint8))
        pos += n
    buf = np.full(pos + 64, 0xA5, dtype=np.uint8)
    for (o, n, _), f in zip(spec, fill):
        buf[o:o + len(f)] = f
    return buf, spec


def launch(plug, L, base_ptr, spec, scratch_bytes=None, reserved=0, scratch_skew=0):
    rows = (D.EsumRow * max(len(spec), 1))()
    for r, (o, n, k) in zip(rows, spec):
        r.dst, r.len, r.elem, r.tile0, r.reserved = base_ptr + o, n, k, 0xDEAD, reserved
    tiles = sum(D.esum_tiles(n, k) for _, n, k in spec if k in ELEMS)
    need = D.esum_scratch_bytes(tiles)
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    d_scratch = L.qzstd_hip_malloc(0, need + 32)
    assert d_rows and d_scratch, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_esum(0, None, rows, len(spec), d_rows, d_scratch + scratch_skew, need if scratch_bytes is None else scratch_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_scratch)
    return rc, [r.tile0 for r in rows[:len(spec)]]


def expected(buf, spec):
    want = buf.copy()
    for o, n, k in spec:
        m = n // k * k
        want[o:o + m] = np.frombuffer(D.elem_sum(buf[o:o + m].tobytes(), k), dtype=np.uint8)
    return want


def test_every_alignment_element_size_and_length_in_place(gpu_plugin, L):
    buf, spec = case()
    t = torch.from_numpy(buf).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    rc, tile0 = launch(gpu_plugin, L, t.data_ptr(), spec)
    assert rc == 0, gpu_plugin.err()
    run = 0
    for (o, n, k), t0 in zip(spec, tile0):
        assert t0 == run
        run += D.esum_tiles(n, k)
    got, want = t.cpu().numpy(), expected(buf, spec)
    bad = np.flatnonzero(got != want)
    if len(bad):
        row = max((r for r in spec if r[0] <= bad[0]), key=lambda r: r[0], default=None)
        raise AssertionError("differs from QZSTD_elemSum at byte %d, %d bytes in all; row (offset, len, elem) = %s, %d bytes into it" %
                             (bad[0], len(bad), row, bad[0] - (row[0] if row else 0)))
    # the rows did change (the guards and tails were checked above by equality with `want`)
    assert not np.array_equal(got, buf)


def test_all_ones_differences_count_up_and_carries_cross_32_bits(gpu_plugin, L):
    n = 5 * TILE + 24
    for z, step in ((2, 1), (2 * ((1 << 31) + 1), (1 << 31) + 1)):
        buf = np.full(n + 64, 0x5A, dtype=np.uint8)
        buf[7:7 + n] = np.frombuffer(np.full(n // 8, z, dtype="<u8").tobytes(), dtype=np.uint8)
        t = torch.from_numpy(buf).to("cuda:0")
        rc, _ = launch(gpu_plugin, L, t.data_ptr(), [(7, n, 8)])
        assert rc == 0, gpu_plugin.err()
        got = t.cpu().numpy()
        sums = np.frombuffer(got[7:7 + n].tobytes(), dtype="<u8")
        assert np.array_equal(sums, (np.arange(1, n // 8 + 1, dtype=np.uint64) * np.uint64(step)))
        assert (got[:7] == 0x5A).all() and (got[7 + n:] == 0x5A).all()


def test_launcher_refusals_leave_memory_and_rows_untouched(gpu_plugin, L):
    buf = np.arange(40000, dtype=np.uint32).view(np.uint8)[:40000].copy()
    t = torch.from_numpy(buf).to("cuda:0")
    good = [(3, 100, 2), (500, 0, 8), (1000, 3 * TILE + 1, 4)]
    for name, spec, kw in (("elem 0", [(3, 100, 0)], {}), ("elem 3", good[:2] + [(1000, 4000, 3)], {}), ("elem 16", [(3, 100, 16)], {}),
                           ("reserved", good, {"reserved": 1}), ("scratch too small", good, {"scratch_bytes": 24 * 4 - 1}),
                           ("scratch misaligned", good, {"scratch_skew": 8})):
        rc, tile0 = launch(gpu_plugin, L, t.data_ptr(), spec, **kw)
        assert rc < 0 and all(x == 0xDEAD for x in tile0), name
        assert np.array_equal(t.cpu().numpy(), buf), name
    rows = (D.EsumRow * 1)()
    rows[0].dst, rows[0].len, rows[0].elem = 0, 8, 8
    assert L.qzstd_hip_esum(0, None, rows, 1, 16, 16, 1 << 20) < 0  # null dst with an element (refused before anything is dereferenced)
    rows[0].dst, rows[0].len = t.data_ptr(), 0xFFFFFFE1
    assert L.qzstd_hip_esum(0, None, rows, 1, 16, 16, 1 << 40) < 0
    assert L.qzstd_hip_esum(0, None, None, 1, 16, 16, 1 << 20) < 0 and L.qzstd_hip_esum(0, None, rows, 1, None, 16, 1 << 20) < 0
    assert L.qzstd_hip_esum(0, None, rows, 1, 16, None, 1 << 20) < 0
    rc, _ = launch(gpu_plugin, L, t.data_ptr(), [])
    assert rc == 0
    rc, _ = launch(gpu_plugin, L, t.data_ptr(), [(3, 1, 2), (9, 7, 8), (30, 0, 1)])  # no row with an element: nothing is queued
    assert rc == 0 and np.array_equal(t.cpu().numpy(), buf)
    rc, tile0 = launch(gpu_plugin, L, t.data_ptr(), good)
    assert rc == 0 and tile0 == [0, 1, 1]
    assert np.array_equal(t.cpu().numpy(), expected(buf, good))
