"""GPU: the fingerprint kernel (qzstd_hip_fingerprint, include/qzstd_hip_device.h) alone, through the C ABI, against the C definition
(include/qzstd_fingerprint.h's QZSTD_fpTile, through tests/mock/mock_hip_fingerprint.c built alone and run over the same bytes in host
memory), tile digest for tile digest.  Rows hold the host checker's inputs (tools/qz_device.py: fp_corpus, FP_LENS) at source alignments 0,
1, 7, 8, 15 mod 16, one launch per case list; every case is built TWICE with complementary bytes around the rows and must give identical
digests, so a masking slip at a row's first or last word shows; rows packed back to back, empty rows between full ones, a row of 64 tiles
among one-byte rows; the changed copies the host checker asserts to differ under the plain-C function differ here too and equal the
definition's.  Only d_tiles[0 .. total tiles) may be written and only tile0 of the caller's rows.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGNS = (0, 1, 7, 8, 15)
GUARD_WORDS = 16
GUARD_VALUE = 0xDEADBEEFDEADBEEF
PREFILL = 7
SENTINEL = 0x5A5A5A5A  # tile0 before the call


@pytest.fixture(scope="module")
def definition(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fingerprint") / "libmockfingerprint.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "mock", "mock_hip_fingerprint.c")])
    return D.bind_fingerprint_kernel(C.CDLL(so))


class Case:
    """rows (offset, len) over one host array that holds each row's content at its place and, everywhere else, bytes that build(False) and
    build(True) give complementary values"""

    def __init__(self, seed=0):
        self.seed, self.rows, self.contents, self.pos = seed, [], [], 64

    def add(self, data, align=0, packed=False):
        """a row of these bytes (None: a row with a null address and no bytes) at the given alignment mod 16, or packed: right behind the
        row before it"""
        if data is None:
            self.rows.append((None, 0))
            self.contents.append(np.zeros(0, dtype=np.uint8))
            return
        if not packed:
            self.pos = ((self.pos + 15) & ~15) + 16 + align
        self.rows.append((self.pos, len(data)))
        self.contents.append(np.asarray(data, dtype=np.uint8))
        self.pos += len(data)

    def build(self, flipped):
        buf = np.random.default_rng(self.seed).integers(0, 256, self.pos + 64, dtype=np.uint8)
        if flipped:
            buf ^= 0xFF
        for (o, n), d in zip(self.rows, self.contents):
            if n:
                buf[o:o + n] = d
        return buf


def total_tiles(spec):
    return sum(D.fp_tiles(n) for _, n in spec)


def launch(L, spec, base, null=None, n_rows=None, device=True, plug=None):
    """qzstd_hip_fingerprint over rows [(offset from base or None, len)] -> (return value, the tile words with their guards as numpy uint64,
    the rows as they came back); device=False: the C definition's stand-in over host memory"""
    n, nt = len(spec), total_tiles(spec)
    rows = (D.FpRow * max(n, 1))()
    for r, (o, ln) in zip(rows, spec):
        r.src, r.len, r.tile0 = (base + o if o is not None else 0), ln, SENTINEL
    host = np.full(GUARD_WORDS + max(nt, 1) + GUARD_WORDS, GUARD_VALUE, dtype=np.uint64)
    host[GUARD_WORDS:GUARD_WORDS + max(nt, 1)] = PREFILL
    args = lambda d_rows, out: (0, None, None if null == "rows" else rows, n if n_rows is None else n_rows,  # noqa: E731
                                None if null == "d_rows" else d_rows, None if null == "tiles" else out)
    if not device:
        scratch = (D.FpRow * max(n, 1))()
        rc = L.qzstd_hip_fingerprint(*args(scratch, host.ctypes.data + 8 * GUARD_WORDS))
        return rc, host, [(r.src, r.len, r.tile0) for r in rows[:n]]
    out = torch.from_numpy(host.view(np.int64)).to("cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_fingerprint(*args(d_rows, out.data_ptr() + 8 * GUARD_WORDS))
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, out.cpu().numpy().view(np.uint64), [(r.src, r.len, r.tile0) for r in rows[:n]]


def tile0_ref(spec):
    out, total = [], 0
    for _, n in spec:
        out.append(total)
        total += D.fp_tiles(n)
    return out


def check(plug, definition, case):
    """both builds of the case on the GPU and the first one under the C definition -> the tile digests, row after row"""
    L = D.bind_fingerprint_kernel(plug.lib)
    nt = total_tiles(case.rows)
    got = []
    for flipped in (False, True):
        buf = case.build(flipped)
        t = torch.from_numpy(buf).to("cuda:0")
        assert t.data_ptr() % 16 == 0
        rc, tiles, rows = launch(L, case.rows, t.data_ptr(), plug=plug)
        assert rc == 0, plug.err()
        assert (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and (tiles[GUARD_WORDS + nt:GUARD_WORDS + max(nt, 1)] == PREFILL).all() and \
            (tiles[GUARD_WORDS + max(nt, 1):] == GUARD_VALUE).all()  # nothing but the tile words
        assert rows == [(t.data_ptr() + o if o is not None else 0, n, t0) for (o, n), t0 in zip(case.rows, tile0_ref(case.rows))]
        assert np.array_equal(t.cpu().numpy(), buf)  # only read
        got.append(tiles[GUARD_WORDS:GUARD_WORDS + nt].copy())
    buf = np.ascontiguousarray(case.build(False))
    rc, tiles, rows = launch(definition, case.rows, buf.ctypes.data, device=False)
    assert rc == 0 and [r[2] for r in rows] == tile0_ref(case.rows)
    want = tiles[GUARD_WORDS:GUARD_WORDS + nt]
    bad = np.flatnonzero(got[0] != want)
    assert not len(bad), "tile %d: kernel %#x, definition %#x; %d of %d tiles wrong" % (bad[0], got[0][bad[0]], want[bad[0]], len(bad), nt)
    bad = np.flatnonzero(got[1] != got[0])
    assert not len(bad), "tile %d changes with the bytes AROUND its row; %d of %d tiles do" % (bad[0], len(bad), nt)
    case.tile0 = tile0_ref(case.rows)
    return want


def row_tiles(case, want, i):
    t0 = case.tile0[i]  # (check() left it)
    return [int(v) for v in want[t0:t0 + D.fp_tiles(case.rows[i][1])]]


def test_every_length_and_alignment_and_every_changed_copy(gpu_plugin, definition):
    """the host checker's inputs and every copy it changes, at every alignment, in one launch: each digest is the definition's, the original's
    and the copy's fingerprints differ (as they do under the plain-C function on the CPU), and the restatement agrees on the originals"""
    case, index = Case(1), {}
    for k, n in enumerate(D.FP_LENS):
        data = D.fp_corpus(n, 11 + k)
        for al in ALIGNS:
            index[(n, al, None)] = len(case.rows)
            case.add(data, al)
            for name, d in D.fp_variants(data):
                index[(n, al, name)] = len(case.rows)
                case.add(d, al)
    want = check(gpu_plugin, definition, case)
    pairs = 0
    for (n, al, name), i in index.items():
        fp = D.fp_fold_ref(row_tiles(case, want, i), case.rows[i][1])
        if name is None:
            assert fp == D.fingerprint_ref(case.contents[i].tobytes()), (n, al)  # the second specification
            assert al == ALIGNS[0] or fp == D.fp_fold_ref(row_tiles(case, want, index[(n, ALIGNS[0], None)]), n)
        else:
            assert fp != D.fp_fold_ref(row_tiles(case, want, index[(n, al, None)]), n), (n, al, name)
            pairs += 1
    assert pairs == len(ALIGNS) * sum(len(D.fp_variants(D.fp_corpus(n, 1))) for n in D.FP_LENS) and pairs > 250


def test_rows_of_one_byte_and_a_row_of_64_tiles_in_one_launch(gpu_plugin, definition):
    case = Case(2)
    one = D.fp_corpus(1000, 3)
    for i in range(1000):
        case.add(one[i:i + 1], i % 16)
    case.add(D.fp_corpus(1 << 20, 4), 7)
    for i in range(1000):
        case.add(one[i:i + 1], (3 * i) % 16)
    case.add(D.fp_corpus((1 << 20) - 3, 5), 1)
    want = check(gpu_plugin, definition, case)
    assert len(want) == 2000 + 64 + 64 and len(set(row_tiles(case, want, 1000))) == 64
    # a one-byte row's digest depends on its byte alone
    assert row_tiles(case, want, 0) == [D.fp_tile_ref(one[0:1].tobytes())]
    first = {}
    for i in list(range(1000)) + list(range(1001, 2001)):
        b = int(case.contents[i][0])
        assert first.setdefault(b, row_tiles(case, want, i)) == row_tiles(case, want, i)


def test_rows_packed_back_to_back_and_empty_rows_between_full_ones(gpu_plugin, definition):
    """neighbours in memory share 16-byte words on both sides; empty rows (null addresses too) take no tile and do not shift the others'"""
    case = Case(3)
    for k, n in enumerate((1, 5, 16, 33, 16384, 16385, 40, 7, 0, 100, 16383, 0, 0, 3 * 16384 + 5, 1)):
        case.add(D.fp_corpus(n, 20 + k), 3, packed=k > 0)
    case.add(None)
    case.add(D.fp_corpus(17, 40), 15)
    case.add(None)
    want = check(gpu_plugin, definition, case)
    assert len(want) == total_tiles(case.rows) == 1 + 1 + 1 + 1 + 1 + 2 + 1 + 1 + 0 + 1 + 1 + 0 + 0 + 4 + 1 + 0 + 1 + 0
    for i in (5, 13):
        data = case.contents[i].tobytes()
        assert row_tiles(case, want, i) == [D.fp_tile_ref(data[o:o + 16384]) for o in range(0, len(data), 16384)]


def test_launcher_refusals_empty_rows_and_no_rows(gpu_plugin, definition):
    L = D.bind_fingerprint_kernel(gpu_plugin.lib)
    a = D.fp_corpus(40000, 9)
    a_t = torch.from_numpy(a).to("cuda:0")
    p = a_t.data_ptr()
    good = [(3, 100), (500, 0), (1001, 20000)]

    def untouched(res):
        rc, tiles, rows = res
        return rc < 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and \
            (tiles[-GUARD_WORDS:] == GUARD_VALUE).all() and all(r[2] == SENTINEL for r in rows)

    for null in ("rows", "d_rows", "tiles"):
        assert untouched(launch(L, good, p, null=null, plug=gpu_plugin)), null
    assert untouched(launch(L, good[:2] + [(None, 2000)], p, plug=gpu_plugin))          # a null src with len > 0
    assert untouched(launch(L, [good[0], (0, 0xFFFFFFE1)], p, plug=gpu_plugin))         # len > 0xFFFFFFE0
    many = [(0, 0xFFFFFFE0)] * 8193                                                     # 8193 x 262144 workgroups: more than 2^31 - 1
    rows = (D.FpRow * len(many))()
    for r in rows:
        r.src, r.len, r.tile0 = p, 0xFFFFFFE0, SENTINEL
    words = torch.full((GUARD_WORDS,), PREFILL, dtype=torch.int64, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    try:
        assert L.qzstd_hip_fingerprint(0, None, rows, len(many), d_rows, words.data_ptr()) < 0
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert all(r.tile0 == SENTINEL for r in rows) and (words.cpu().numpy() == PREFILL).all()
    # no rows: nothing happens; nothing but empty rows (null addresses allowed): nothing is queued, tile0 is 0
    rc, tiles, rows = launch(L, good, p, n_rows=0, plug=gpu_plugin)
    assert rc == 0 and (tiles[GUARD_WORDS:GUARD_WORDS + 3] == PREFILL).all() and all(r[2] == SENTINEL for r in rows)
    rc, tiles, rows = launch(L, [(None, 0), (5, 0)], p, plug=gpu_plugin)
    assert rc == 0 and tiles[GUARD_WORDS] == PREFILL and [r[2] for r in rows] == [0, 0]
    assert (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and (tiles[GUARD_WORDS + 1:] == GUARD_VALUE).all()
    # and the good rows
    rc, tiles, rows = launch(L, good, p, plug=gpu_plugin)
    assert rc == 0 and [r[2] for r in rows] == [0, 1, 1]
    assert [int(v) for v in tiles[GUARD_WORDS:GUARD_WORDS + 3]] == [D.fp_tile_ref(a[3:103].tobytes()), D.fp_tile_ref(a[1001:1001 + 16384].tobytes()),
                                                                 D.fp_tile_ref(a[1001 + 16384:21001].tobytes())]
    assert np.array_equal(a_t.cpu().numpy(), a)
