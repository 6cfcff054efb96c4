"""GPU: the fingerprint from pieces (qzstd_hip_fingerprint_pieces, include/qzstd_hip_device.h) alone, through the C ABI, against its definition
in plain C (tests/mock/mock_hip_fingerprint_pieces.c, built here on its own and run over a host copy of the same memory) AND against
qzstd_hip_fingerprint on a contiguous copy of every row: the rows and cuttings of tests/test_gpu_group_pieces.py (every edge length; one
piece, single bytes, a cut at every offset 1 .. 33, around the tile boundary, widths 3, 17, 2048 and 2050, random; every piece an allocation
of its own whose misalignment cycles through 0 .. 15; width 3 narrowed to rows up to 3 x 16 KiB + 1 as there) in ONE launch.  Nothing but
the tile words may change: the guards around them, the sources and the guards around every piece.  A piece with a base is refused with
nothing queued, and a refused launch leaves the rows as they were.  Every comparison is word-exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D  # (imports torch first: one HIP runtime)
import test_gpu_group_pieces as GP

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = GP.ROOT
REF_SO = os.path.join(ROOT, "tests", "mock", "libcheck_pieces_ref.so")
GUARD = 8  # tile words on either side
FILL = 0x5A5A5A5A5A5A5A5A
FPROW = np.dtype([("len", "<u4"), ("tile0", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4")])
assert FPROW.itemsize == C.sizeof(D.FpPiecesRow)


def build_ref():
    """the two definitions, built on their own: the mocks' sources and the byte-grouped layout's"""
    tmp = "%s.%d.tmp" % (REF_SO, os.getpid())
    mock = os.path.join(ROOT, "tests", "mock")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(B.PKG_DIR, "frontend"), "-o", tmp, os.path.join(mock, "mock_hip_fingerprint_pieces.c"),
                           os.path.join(mock, "mock_hip_ungroup_cmp_pieces.c"), os.path.join(B.PKG_DIR, "frontend", "qzstd_bytegroup.c")])
    os.replace(tmp, REF_SO)
    return D.bind_check_pieces_kernels(C.CDLL(REF_SO))


@pytest.fixture(scope="module")
def ref():
    return build_ref()


def fp_rows(rows):
    out = np.zeros(len(rows), dtype=FPROW)
    out["len"], out["piece0"], out["nPieces"], out["tile0"] = rows["len"], rows["piece0"], rows["nPieces"], 77
    return out


def run_gpu(plug, L, rows, pieces, npieces, null=None, n_rows=None):
    """-> (return value, the tile words with their guards as numpy uint64)"""
    total = sum(D.fp_tiles(int(n)) for n in rows["len"])
    tiles = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int64, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, max(rows.nbytes, 16))
    d_pieces = L.qzstd_hip_malloc(0, max(pieces.nbytes, 16))
    assert d_rows and d_pieces, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_fingerprint_pieces(0, None, None if null == "rows" else rows.ctypes.data, len(rows) if n_rows is None else n_rows,
                                            None if null == "d_rows" else d_rows, None if null == "pieces" else pieces.ctypes.data, npieces,
                                            None if null == "d_pieces" else d_pieces, None if null == "tiles" else tiles.data_ptr() + 8 * GUARD)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_pieces)
    return rc, tiles.cpu().numpy().view(np.uint64)


def api(plug):
    return D.bind_check_pieces_kernels(D.bind_fingerprint_kernel(plug.lib))


@pytest.mark.parametrize("k", GP.ELEMS)
def test_fingerprint_pieces_kernel_against_its_definition_and_the_contiguous_kernel(gpu_plugin, ref, k):
    L = api(gpu_plugin)
    grows, pieces, npieces, src_at, _, src_mem, _, _ = GP.build(k, "none", 60 + k)
    assert len({int(a) % 16 for a in src_at}) == 16 and int(pieces["len"].min()) == 1
    src = GP.Memory(src_mem)
    total = sum(D.fp_tiles(int(n)) for n in grows["len"])
    # the definition, over the host copy
    rows = fp_rows(grows)
    want = np.full(GUARD + total + GUARD, FILL, dtype=np.uint64)
    d_rows, d_pieces = np.zeros_like(rows), np.zeros_like(pieces)
    assert ref.qzstd_hip_fingerprint_pieces(0, None, rows.ctypes.data, len(rows), d_rows.ctypes.data,
                                            GP.addresses(pieces, npieces, src_at, None, src.h0, 0).ctypes.data, npieces, d_pieces.ctypes.data,
                                            want.ctypes.data + 8 * GUARD) == 0
    tile0 = rows["tile0"].copy()
    assert tile0.tolist() == np.concatenate([[0], np.cumsum([D.fp_tiles(int(n)) for n in grows["len"]])[:-1]]).tolist()
    # the kernel
    rows = fp_rows(grows)
    rc, got = run_gpu(gpu_plugin, L, rows, GP.addresses(pieces, npieces, src_at, None, src.d0, 0), npieces)
    assert rc == 0, gpu_plugin.err()
    assert np.array_equal(rows["tile0"], tile0)
    bad = np.flatnonzero(got != want)
    if len(bad):
        t = int(bad[0]) - GUARD
        r = int(np.searchsorted(tile0, t, side="right")) - 1
        ps = pieces[int(rows["piece0"][r]):int(rows["piece0"][r] + rows["nPieces"][r])]
        raise AssertionError("tile word %d (of %d) differs from the definition, %d in all; row %d: len %d, tile %d, piece lengths %s..." %
                             (t, total, len(bad), r, rows["len"][r], t - tile0[r], ps["len"][:8].tolist()))
    assert src.unchanged()  # the sources and the guards around every piece: only read
    # qzstd_hip_fingerprint on a contiguous copy of every row, at every misalignment
    content, at, pos = [], [], 0
    for r in range(len(grows)):
        p0, n = int(grows["piece0"][r]), int(grows["nPieces"][r])
        c = np.concatenate([src_mem[int(src_at[p]):int(src_at[p]) + int(pieces["len"][p])] for p in range(p0, p0 + n)]) if n else np.zeros(0, np.uint8)
        pos = ((pos + 15) & ~15) + r % 16
        at.append(pos)
        content.append(c)
        pos += len(c)
    flat = np.zeros(pos + 16, dtype=np.uint8)
    for a, c in zip(at, content):
        flat[a:a + len(c)] = c
    dev = torch.from_numpy(flat).to("cuda:0")
    crow = (D.FpRow * len(grows))()
    for r, (a, c) in enumerate(zip(at, content)):
        crow[r].src, crow[r].len, crow[r].tile0 = dev.data_ptr() + a, len(c), 0
    ctiles = torch.full((total,), 0, dtype=torch.int64, device="cuda:0")
    d_crow = L.qzstd_hip_malloc(0, C.sizeof(crow))
    try:
        torch.cuda.synchronize()
        assert L.qzstd_hip_fingerprint(0, None, crow, len(grows), d_crow, ctiles.data_ptr()) == 0, gpu_plugin.err()
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_crow)
    assert np.array_equal(ctiles.cpu().numpy().view(np.uint64), got[GUARD:GUARD + total])


def test_fingerprint_pieces_launcher_refusals_leave_rows_and_tiles_untouched(gpu_plugin):
    L = api(gpu_plugin)
    mem = torch.from_numpy(np.arange(8192, dtype=np.uint8)).to("cuda:0")
    a = mem.data_ptr()

    def table(ps):
        t = np.zeros(max(len(ps), 1), dtype=GP.PIECE)
        for i, (src, base, off, n) in enumerate(ps):
            t[i] = (a + src if src is not None else 0, a + base if base is not None else 0, off, n)
        return t

    def rowsof(rs):
        t = np.zeros(max(len(rs), 1), dtype=FPROW)
        for i, (ln, p0, n) in enumerate(rs):
            t[i] = (ln, 77, p0, n)
        return t[:len(rs)]

    three = [(3, None, 0, 1), (200, None, 1, 60), (1000, None, 61, 39)]
    good = (three + [(1000, None, 0, 39)], [(100, 0, 3), (0, 3, 0), (39, 3, 1)])
    bad = {"a gap": ([(3, None, 0, 1), (200, None, 2, 59), (1000, None, 61, 39)], [(100, 0, 3)]),
           "an overlap": ([(3, None, 0, 2), (200, None, 1, 60), (1000, None, 61, 39)], [(100, 0, 3)]),
           "descending": ([three[1], three[0], three[2]], [(100, 0, 3)]), "short": (three[:2], [(100, 0, 2)]), "long": (three, [(99, 0, 3)]),
           "an empty piece": (three[:1] + [(7, None, 1, 0)] + three[1:], [(100, 0, 4)]),
           "a null source": ([three[0], (None, None, 1, 60), three[2]], [(100, 0, 3)]), "past the table": (three, [(100, 1, 3)]),
           "no pieces for a row with bytes": (three, [(100, 0, 0)]), "a row too long": (three, [(0xFFFFFFE1, 0, 3)]),
           "a base": ([three[0], (200, 900, 1, 60), three[2]], [(100, 0, 3)]), "src as base": ([three[0], (200, 200, 1, 60), three[2]], [(100, 0, 3)])}
    for name, (ps, rs) in bad.items():
        rows = rowsof(rs)
        rc, got = run_gpu(gpu_plugin, L, rows, table(ps), len(ps))
        assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all(), name
    for null in ("rows", "d_rows", "pieces", "d_pieces", "tiles"):
        rows = rowsof(good[1])
        rc, got = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, null=null)
        assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all(), null
    rows = rowsof(good[1])
    rc, got = run_gpu(gpu_plugin, L, rows, table(good[0]), 3)  # a table shorter than the rows say
    assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all()
    rc, got = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, n_rows=0)
    assert rc == 0 and (got == FILL).all() and (rows["tile0"] == 77).all()
    rc, got = run_gpu(gpu_plugin, L, rowsof([(0, 0, 0), (0, 0, 0)]), table([]), 0, null="pieces")  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    rc, got = run_gpu(gpu_plugin, L, rows, table(good[0]), 4)
    assert rc == 0, gpu_plugin.err()
    src = np.arange(8192, dtype=np.uint8)
    c = np.concatenate([src[3:4], src[200:260], src[1000:1039]])
    assert rows["tile0"].tolist() == [0, 1, 1]
    assert got.tolist() == [FILL] * GUARD + [D.fp_tile_ref(c), D.fp_tile_ref(src[1000:1039])] + [FILL] * GUARD
