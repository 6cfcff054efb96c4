"""GPU: the element-difference cost kernel (qzstd_hip_ediff_cost, include/qzstd_hip_device.h) alone, through the C ABI, against the C
definition (include/qzstd_ediffcost.h's QZSTD_ediffCostTile, through tests/mock/mock_hip_ediff_cost.c built alone and run over the same
bytes in host memory), word for word.  Rows at source offsets 0 .. 15 mod 16 — also ones that are no multiple of the element size — for
every k in {1, 2, 4, 8}, the lengths around an element and a tile of tests/ediffcost/ediffcost_check.c, and its contents (all zero, an
arange, noise, values that jump exactly at tile borders, a large first element, descending values that wrap) plus a column with order; rows
packed back to back so that neighbours share a 16-byte word; one launch that mixes one-byte rows with a row of 1 MiB + 3.  Everything
around the rows is 0xA5 and must never be counted: the definition reads the row alone.  Only d_tiles[0 .. 2 * total tiles) may be written,
only tile0 of the caller's rows, and the sources are only read.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_WORDS = 16  # (even: the tile words stay 8-byte aligned)
GUARD_VALUE = 0xDEADBEEF
PREFILL = 7
SENTINEL = 0x5A5A5A5A  # tile0 before the call
FILL = 0xA5
CONTENTS = ("zero", "arange", "noise", "steps_at_tiles", "large_first", "descending", "column")


def lengths(k):
    return (0, k - 1, k, k + 1, 16384 - k, 16384, 16384 + 1, 16384 + k, 3 * 16384 + 5, 131072 + 3)


@pytest.fixture(scope="module")
def definition(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ediffcost") / "libmockediffcost.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "mock", "mock_hip_ediff_cost.c")])
    return D.bind_ediff_cost_kernel(C.CDLL(so))


def content(kind, L, k, seed):
    """L bytes: n = L // k little-endian elements of the kind, and a noise tail"""
    rng = np.random.default_rng(seed)
    n, T, top = L // k, 16384 // k, (1 << (8 * k)) - 1
    e = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        if kind == "zero":
            x = np.zeros(n, dtype=np.uint64)
        elif kind == "arange":
            x = e + np.uint64(1)
        elif kind == "noise":
            x = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        elif kind == "steps_at_tiles":
            x = np.uint64(0x0123456789ABCDEF) * (e // np.uint64(T) + np.uint64(1))
        elif kind == "large_first":
            x = np.uint64(5) + e % np.uint64(3)
            x[:1] = top - 1
        elif kind == "descending":
            x = np.uint64(1000) - np.uint64(7) * e
        else:
            x = np.cumsum(rng.integers(5, 41, n, dtype=np.uint64)) + np.uint64(top - 100)
    body = (x & np.uint64(top)).astype("<u%d" % k).view(np.uint8)
    return np.concatenate([body, rng.integers(0, 256, L - n * k, dtype=np.uint8)])


class Case:
    """rows (offset or None, len, elem) over one host array that is 0xA5 wherever no row lies"""

    def __init__(self):
        self.rows, self.contents, self.pos = [], [], 64

    def add(self, data, k, align=0, packed=False):
        if data is None:
            self.rows.append((None, 0, k))
            self.contents.append(np.zeros(0, dtype=np.uint8))
            return
        if not packed:
            self.pos = ((self.pos + 15) & ~15) + 16 + align
        self.rows.append((self.pos, len(data), k))
        self.contents.append(np.asarray(data, dtype=np.uint8))
        self.pos += len(data)

    def build(self):
        buf = np.full(self.pos + 64, FILL, dtype=np.uint8)
        for (o, n, _), d in zip(self.rows, self.contents):
            if n:
                buf[o:o + n] = d
        return buf


def total_tiles(spec):
    return sum(D.esum_tiles(n, k) for _, n, k in spec if k in (1, 2, 4, 8))  # (a row with another elem is one the launcher refuses)


def tile0_ref(spec):
    out, total = [], 0
    for _, n, k in spec:
        out.append(total)
        total += D.esum_tiles(n, k)
    return out


def launch(L, spec, base, null=None, n_rows=None, device=True, plug=None, reserved=0, skew=0):
    """qzstd_hip_ediff_cost over rows [(offset from base or None, len, elem)] -> (return value, the tile words with their guards as numpy
    uint32, the rows' tile0 as they came back); device=False: the C definition's stand-in over host memory"""
    n, nt = len(spec), total_tiles(spec)
    rows = (D.EdiffCostRow * max(n, 1))()
    for r, (o, ln, k) in zip(rows, spec):
        r.src, r.len, r.elem, r.tile0, r.reserved = (base + o if o is not None else 0), ln, k, SENTINEL, reserved
    words = 2 * max(nt, 1)
    host = np.full(GUARD_WORDS + words + GUARD_WORDS, GUARD_VALUE, dtype=np.uint32)
    host[GUARD_WORDS:GUARD_WORDS + words] = PREFILL
    args = lambda d_rows, out: (0, None, None if null == "rows" else rows, n if n_rows is None else n_rows,  # noqa: E731
                                None if null == "d_rows" else d_rows, None if null == "tiles" else out + skew)
    if not device:
        scratch = (D.EdiffCostRow * max(n, 1))()
        rc = L.qzstd_hip_ediff_cost(*args(scratch, host.ctypes.data + 4 * GUARD_WORDS))
        return rc, host, [r.tile0 for r in rows[:n]]
    out = torch.from_numpy(host.view(np.int32)).to("cuda:0")
    assert out.data_ptr() % 8 == 0
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ediff_cost(*args(d_rows, out.data_ptr() + 4 * GUARD_WORDS))
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, out.cpu().numpy().view(np.uint32), [r.tile0 for r in rows[:n]]


def check(plug, definition, case):
    """the case on the GPU and under the C definition -> the tile words [[plain, diff], ...], row after row"""
    L = D.bind_ediff_cost_kernel(plug.lib)
    nt = total_tiles(case.rows)
    buf = case.build()
    t = torch.from_numpy(buf).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    rc, tiles, tile0 = launch(L, case.rows, t.data_ptr(), plug=plug)
    assert rc == 0, plug.err()
    assert (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and (tiles[GUARD_WORDS + 2 * nt:GUARD_WORDS + 2 * max(nt, 1)] == PREFILL).all() and \
        (tiles[GUARD_WORDS + 2 * max(nt, 1):] == GUARD_VALUE).all()  # nothing but the tile words
    assert tile0 == tile0_ref(case.rows)
    assert np.array_equal(t.cpu().numpy(), buf)  # only read
    got = tiles[GUARD_WORDS:GUARD_WORDS + 2 * nt].reshape(-1, 2)
    rc, ref, tile0 = launch(definition, case.rows, buf.ctypes.data, device=False)
    assert rc == 0 and tile0 == tile0_ref(case.rows)
    want = ref[GUARD_WORDS:GUARD_WORDS + 2 * nt].reshape(-1, 2)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        row = max(i for i, t0 in enumerate(tile0) if t0 <= bad[0] and case.rows[i][1] >= case.rows[i][2])
        raise AssertionError("tile %d (row %d: offset %s, len %d, elem %d): kernel %s, definition %s; %d of %d tiles wrong" % (
            bad[0], row, case.rows[row][0], case.rows[row][1], case.rows[row][2], got[bad[0]], want[bad[0]], len(bad), nt))
    case.tile0 = tile0
    return want


@pytest.mark.parametrize("k", (1, 2, 4, 8))
def test_every_offset_length_and_content(gpu_plugin, definition, k):
    case, index = Case(), {}
    for li, n in enumerate(lengths(k)):
        for ci, kind in enumerate(CONTENTS):
            data = content(kind, n, k, 100 * li + ci)
            for off in range(16):
                index[(n, kind, off)] = len(case.rows)
                case.add(data, k, off)
    want = check(gpu_plugin, definition, case)
    assert len(want) == 16 * len(CONTENTS) * sum(D.esum_tiles(n, k) for n in lengths(k))
    for (n, kind, off), i in index.items():
        w = want[case.tile0[i]:case.tile0[i] + D.esum_tiles(n, k)]
        if off:  # the words do not depend on where the row lies
            j = index[(n, kind, 0)]
            assert np.array_equal(w, want[case.tile0[j]:case.tile0[j] + D.esum_tiles(n, k)]), (n, kind, off)
        if kind == "zero":
            assert not w.any()
        if kind == "arange":
            assert not w[:, 1].any() and (n // k < 2 or w[:, 0].any())
        if kind == "steps_at_tiles" and len(w):
            full = len(w) if n // k - (len(w) - 1) * (16384 // k) >= 2 else len(w) - 1  # (a last tile of one element costs 0 whatever it holds)
            assert not w[:, 0].any() and w[1:full, 1].all()  # a wrong element in front of a tile changes its diff word


def test_rows_packed_back_to_back_share_words(gpu_plugin, definition):
    """neighbours in memory share 16-byte words on both sides, element sizes mixed; rows without an element (null addresses too) take no
    tile and do not shift the others'"""
    case = Case()
    spec = ((1, 1), (5, 2), (16, 4), (33, 8), (16384, 2), (16385, 1), (40, 8), (7, 8), (0, 4), (100, 4), (16383, 2), (0, 1), (3, 4),
            (3 * 16384 + 5, 8), (1, 1), (16384 + 8, 8), (2, 2))
    for i, (n, k) in enumerate(spec):
        case.add(content(("column", "noise", "arange")[i % 3], n, k, 300 + i), k, 3, packed=i > 0)
    case.add(None, 4)
    case.add(content("column", 17, 1, 40), 1, 15)
    case.add(None, 8)
    want = check(gpu_plugin, definition, case)
    assert len(want) == total_tiles(case.rows) == 1 + 1 + 1 + 1 + 1 + 2 + 1 + 0 + 0 + 1 + 1 + 0 + 0 + 3 + 1 + 2 + 1 + 0 + 1 + 0


def test_rows_of_one_byte_and_a_row_of_a_mebibyte_in_one_launch(gpu_plugin, definition):
    case = Case()
    one = content("noise", 1000, 1, 3)
    for i in range(1000):
        case.add(one[i:i + 1], (1, 2)[i % 2], i % 16)  # k = 2: a row without an element between rows of one
    case.add(content("column", (1 << 20) + 3, 4, 4), 4, 7)
    for i in range(500):
        case.add(one[i:i + 1], 1, (3 * i) % 16)
    case.add(content("noise", (1 << 20) + 3, 8, 5), 8, 1)
    want = check(gpu_plugin, definition, case)
    assert len(want) == 500 + 64 + 500 + 64
    assert not want[:500].any()  # one element: one bin, cost 0 either way
    big = want[case.tile0[1000]:case.tile0[1000] + 64]
    assert (big[:, 1] < big[:, 0]).all()  # the column with order: differences cost less in every tile


def test_launcher_refusals_and_rows_without_tiles(gpu_plugin, definition):
    L = D.bind_ediff_cost_kernel(gpu_plugin.lib)
    a = content("column", 40000, 4, 9)
    a_t = torch.from_numpy(a).to("cuda:0")
    p = a_t.data_ptr()
    good = [(3, 100, 4), (500, 3, 4), (1001, 20000, 2)]

    def untouched(res):
        rc, tiles, tile0 = res
        return rc < 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and \
            (tiles[-GUARD_WORDS:] == GUARD_VALUE).all() and all(t == SENTINEL for t in tile0)

    for null in ("rows", "d_rows", "tiles"):
        assert untouched(launch(L, good, p, null=null, plug=gpu_plugin)), null
    assert untouched(launch(L, good, p, skew=4, plug=gpu_plugin))                          # tile words not 8-byte aligned
    assert untouched(launch(L, good[:2] + [(None, 2000, 8)], p, plug=gpu_plugin))          # a null src with an element
    for bad in (0, 3, 5, 16):
        assert untouched(launch(L, good[:2] + [(0, 64, bad)], p, plug=gpu_plugin)), bad     # elem outside {1, 2, 4, 8}
    assert untouched(launch(L, good, p, reserved=1, plug=gpu_plugin))
    assert untouched(launch(L, [good[0], (0, 0xFFFFFFE1, 1)], p, plug=gpu_plugin))         # len > 0xFFFFFFE0
    many = 8193                                                                            # 8193 x 262144 tiles: more than 2^31 - 1
    rows = (D.EdiffCostRow * many)()
    for r in rows:
        r.src, r.len, r.elem, r.tile0, r.reserved = p, 0xFFFFFFE0, 1, SENTINEL, 0
    words = torch.full((GUARD_WORDS,), PREFILL, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    try:
        assert L.qzstd_hip_ediff_cost(0, None, rows, many, d_rows, words.data_ptr()) < 0
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert all(r.tile0 == SENTINEL for r in rows) and (words.cpu().numpy() == PREFILL).all()
    # no rows: nothing happens; no row with an element (null addresses allowed): nothing is queued, tile0 is 0
    rc, tiles, tile0 = launch(L, good, p, n_rows=0, plug=gpu_plugin)
    assert rc == 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and all(t == SENTINEL for t in tile0)
    rc, tiles, tile0 = launch(L, [(None, 3, 4), (5, 7, 8), (None, 0, 1)], p, plug=gpu_plugin)
    assert rc == 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and tile0 == [0, 0, 0]
    assert (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and (tiles[-GUARD_WORDS:] == GUARD_VALUE).all()
    # and the good rows, against the definition
    rc, tiles, tile0 = launch(L, good, p, plug=gpu_plugin)
    assert rc == 0 and tile0 == [0, 1, 1]
    rc, ref, _ = launch(definition, good, a.ctypes.data, device=False)
    assert rc == 0 and np.array_equal(tiles, ref) and tiles[GUARD_WORDS:GUARD_WORDS + 6].any()
    assert np.array_equal(a_t.cpu().numpy(), a)
