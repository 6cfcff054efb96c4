"""GPU: the ungrouping comparison with pieces (qzstd_hip_ungroup_cmp_pieces, include/qzstd_hip_device.h) alone, through the C ABI, against its
definition in plain C (tests/mock/mock_hip_ungroup_cmp_pieces.c, built here on its own and run over a host copy of the same memory): the
rows and cuttings of tests/test_gpu_group_pieces.py (every edge length; one piece, single bytes, a cut at every offset 1 .. 33, around the
tile boundary, widths 3, 17, 2048 and 2050, random; every piece an allocation of its own whose misalignment cycles through 0 .. 15; width 3
narrowed to rows up to 3 x 16 KiB + 1 as there) in ONE launch, for k = 1, 2, 4, 8, with no base, a base at another alignment and src
itself as the base, ZERO rows among them.  First every staged frame reproduces its pieces (every word SAME but the ZERO rows'); then single
bytes are planted — at a row's first and last byte, at the first and last byte of a piece in the middle, in the tail behind the elements,
two in one tile, on the live side and on the base side (in the stage where src is its own base) — and every tile word must be the
definition's lowest differing offset.  Nothing but the tile words may change.  Every comparison is word-exact."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)
import test_gpu_fingerprint_pieces as FP
import test_gpu_group_pieces as GP

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 8  # tile words on either side
FILL = 0x5A5A5A5A
CROW = np.dtype([("srcOff", "<u8"), ("len", "<u4"), ("elem", "<u4"), ("flags", "<u4"), ("tile0", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4")])
assert CROW.itemsize == C.sizeof(D.UngroupCmpPiecesRow)


@pytest.fixture(scope="module")
def ref():
    return FP.build_ref()


def grouped(u, k):
    e = len(u) // k
    return np.concatenate([np.ascontiguousarray(u[:e * k].reshape(e, k).T).reshape(-1), u[e * k:]]) if e else u.copy()


def run_gpu(plug, L, rows, pieces, npieces, stage, null=None, n_rows=None, skew=0):
    """stage: numpy bytes -> (return value, the tile words with their guards as numpy uint32)"""
    total = sum(D.cmp_tiles(int(n), int(k)) for n, k in zip(rows["len"], rows["elem"]) if k in (1, 2, 4, 8))
    tiles = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int32, device="cuda:0")
    d_stage = torch.from_numpy(np.concatenate([stage, np.zeros(32, np.uint8)])).to("cuda:0")
    assert d_stage.data_ptr() % 16 == 0
    d_rows = L.qzstd_hip_malloc(0, max(rows.nbytes, 16))
    d_pieces = L.qzstd_hip_malloc(0, max(pieces.nbytes, 16))
    assert d_rows and d_pieces, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ungroup_cmp_pieces(0, None, None if null == "rows" else rows.ctypes.data, len(rows) if n_rows is None else n_rows,
                                            None if null == "d_rows" else d_rows, None if null == "pieces" else pieces.ctypes.data, npieces,
                                            None if null == "d_pieces" else d_pieces, None if null == "stage" else d_stage.data_ptr() + skew,
                                            len(stage), None if null == "tiles" else tiles.data_ptr() + 4 * GUARD)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_pieces)
    return rc, tiles.cpu().numpy().view(np.uint32), np.array_equal(d_stage.cpu().numpy()[:len(stage)], stage)


def run_ref(ref, rows, pieces, npieces, stage):
    total = sum(D.cmp_tiles(int(n), int(k)) for n, k in zip(rows["len"], rows["elem"]))
    out = np.full(GUARD + total + GUARD, FILL, dtype=np.uint32)
    raw = np.zeros(len(stage) + 32, dtype=np.uint8)
    s0 = (raw.ctypes.data + 15) & ~15
    raw[s0 - raw.ctypes.data:][:len(stage)] = stage
    d_rows, d_pieces = np.zeros_like(rows), np.zeros_like(pieces)
    rc = ref.qzstd_hip_ungroup_cmp_pieces(0, None, rows.ctypes.data, len(rows), d_rows.ctypes.data, pieces.ctypes.data, npieces,
                                          d_pieces.ctypes.data, s0, len(stage), out.ctypes.data + 4 * GUARD)
    return rc, out


def api(plug):
    return D.bind_check_pieces_kernels(plug.lib)


@pytest.mark.parametrize("mode", GP.BASES)
@pytest.mark.parametrize("k", GP.ELEMS)
def test_ungroup_cmp_pieces_kernel_against_its_definition(gpu_plugin, ref, k, mode):
    L = api(gpu_plugin)
    grows, pieces, npieces, src_at, base_at, src_mem, base_mem, _ = GP.build(k, mode, 80 + k)
    assert len({int(a) % 16 for a in src_at}) == 16 and int(pieces["len"].min()) == 1
    plen = pieces["len"][:npieces].astype(np.int64)
    bmem = src_mem if mode == "self" else base_mem
    # the stage: every row's frame is what its pieces say — group(src ^ base) — at 16-aligned offsets in the rows' order; ZERO rows take no room
    rows = np.zeros(len(grows), dtype=CROW)
    stage, so, content = [], 0, []
    for r in range(len(grows)):
        p0, n = int(grows["piece0"][r]), int(grows["nPieces"][r])
        ps = range(p0, p0 + n)
        c = np.concatenate([src_mem[int(src_at[p]):int(src_at[p] + plen[p])] for p in ps]) if n else np.zeros(0, np.uint8)
        if base_at is not None and n:
            c = c ^ np.concatenate([bmem[int(base_at[p]):int(base_at[p] + plen[p])] for p in ps])
        zero = r % 4 == 3
        rows[r] = (0 if zero else so, len(c), k, D.CMP_ZERO if zero else 0, 77, p0, n)
        content.append(c)
        if not zero:
            g = grouped(c, k)
            stage.append(np.concatenate([g, np.zeros((-len(g)) % 16, np.uint8)]))
            so += len(stage[-1])
    stage = np.concatenate(stage)
    tile0 = np.concatenate([[0], np.cumsum([D.cmp_tiles(int(n), k) for n in rows["len"]])]).astype(np.int64)

    def both(src_bytes, base_bytes, stage_bytes):
        src, bas = GP.Memory(src_bytes), GP.Memory(base_bytes)
        hrows = rows.copy()
        rc, want = run_ref(ref, hrows, GP.addresses(pieces, npieces, src_at, base_at, src.h0, bas.h0 if mode == "other" else src.h0), npieces, stage_bytes)
        assert rc == 0 and hrows["tile0"].tolist() == tile0[:-1].tolist()
        grows_ = rows.copy()
        rc, got, stage_same = run_gpu(gpu_plugin, L, grows_, GP.addresses(pieces, npieces, src_at, base_at, src.d0, bas.d0 if mode == "other" else src.d0),
                                      npieces, stage_bytes)
        assert rc == 0, gpu_plugin.err()
        assert np.array_equal(grows_["tile0"], hrows["tile0"])
        bad = np.flatnonzero(got != want)
        if len(bad):
            t = int(bad[0]) - GUARD
            r = int(np.searchsorted(tile0, t, side="right")) - 1
            ps = pieces[int(rows["piece0"][r]):int(rows["piece0"][r] + rows["nPieces"][r])]
            raise AssertionError("tile word %d (of %d) is %#x, the definition's %#x, %d differ in all; row %d: len %d elem %d flags %d, tile %d, piece lengths %s..."
                                 % (t, tile0[-1], got[bad[0]], want[bad[0]], len(bad), r, rows["len"][r], k, rows["flags"][r], t - tile0[r],
                                    ps["len"][:8].tolist()))
        assert src.unchanged() and bas.unchanged() and stage_same  # sources, bases, the guards around every piece and the stage: only read
        return want[GUARD:-GUARD]

    # 1. nothing planted: every word of a row that is not ZERO says SAME; a ZERO row says where its content is not zero
    words = both(src_mem, base_mem, stage)
    for r in range(len(rows)):
        w = words[tile0[r]:tile0[r + 1]]
        if rows["flags"][r] == 0 or not content[r].any():
            assert (w == D.CMP_SAME).all(), r
        else:
            assert int(w[w != D.CMP_SAME][0]) == int(np.flatnonzero(content[r])[0]), r
    if mode == "self":
        assert any(rows["flags"][r] and rows["len"][r] > GP.TILE for r in range(len(rows)))  # ZERO rows of several tiles that match

    # 2. planted bytes.  (row, offset, side): side "src", "base" (mode other), or "stage" where src is its own base
    plants, expect, kinds = [], {}, set()
    for r in range(len(rows)):
        n, np_ = int(rows["len"][r]), int(rows["nPieces"][r])
        if n == 0 or r % 6 == 0:
            continue
        offs = pieces["off"][int(rows["piece0"][r]):int(rows["piece0"][r]) + np_].astype(np.int64)
        mid = np_ // 2
        tail = (n // k) * k
        kind = r % 6
        if kind == 1:
            at = [0]
        elif kind == 2:
            at = [n - 1]
        elif kind == 3:  # the first byte of a piece in the middle, and a second difference behind it in the same tile
            at = [int(offs[mid])] + ([int(offs[mid]) + 5] if int(offs[mid]) + 5 < n and (int(offs[mid]) + 5) >> 14 == int(offs[mid]) >> 14 else [])
        elif kind == 4:  # the last byte of a piece in the middle
            at = [int(offs[mid + 1]) - 1 if mid + 1 < np_ else n - 1]
        else:  # the tail behind the elements (the last byte where there is none)
            at = [tail if tail < n else n - 1]
        side = "stage" if mode == "self" else ("base" if mode == "other" and kind in (2, 4) else "src")
        if side == "stage" and rows["flags"][r]:
            continue  # (a ZERO row reads no stage)
        plants.append((r, at, side))
        expect[r] = min(at)
        kinds.add((kind, n > GP.TILE))
    assert {(kd, True) for kd in range(1, 6)} <= kinds  # every kind of plant hits a row of several tiles
    src2, base2, stage2 = src_mem.copy(), base_mem.copy(), stage.copy()
    for r, at, side in plants:
        p0 = int(rows["piece0"][r])
        offs = pieces["off"][p0:p0 + int(rows["nPieces"][r])].astype(np.int64)
        for o in at:
            if side == "stage":
                n, e = int(rows["len"][r]), int(rows["len"][r]) // k
                g = (o % k) * e + o // k if o < e * k else o
                stage2[int(rows["srcOff"][r]) + g] ^= 0x21
            else:
                p = int(np.searchsorted(offs, o, side="right")) - 1
                (src2 if side == "src" else base2)[int((src_at if side == "src" else base_at)[p0 + p]) + o - int(offs[p])] ^= 0x21
    words = both(src2, base2, stage2)
    for r, at in expect.items():
        w = words[tile0[r]:tile0[r + 1]]
        if rows["flags"][r] == 0:
            assert int(w[w != D.CMP_SAME][0]) == at, (r, at)  # the definition's lowest offset is the planted one
            assert (w != D.CMP_SAME).sum() == 1, r


def test_ungroup_cmp_pieces_launcher_refusals_leave_rows_and_tiles_untouched(gpu_plugin):
    L = api(gpu_plugin)
    mem = torch.from_numpy(np.arange(8192, dtype=np.uint8)).to("cuda:0")
    a = mem.data_ptr()
    stage = np.zeros(4096, dtype=np.uint8)

    def table(ps):
        t = np.zeros(max(len(ps), 1), dtype=GP.PIECE)
        for i, (src, base, off, n) in enumerate(ps):
            t[i] = (a + src if src is not None else 0, a + base if base is not None else 0, off, n)
        return t

    def rowsof(rs):
        t = np.zeros(max(len(rs), 1), dtype=CROW)
        for i, (so, ln, k, fl, p0, n) in enumerate(rs):
            t[i] = (so, ln, k, fl, 77, p0, n)
        return t[:len(rs)]

    three = [(3, 900, 0, 1), (200, None, 1, 60), (1000, 2001, 61, 39)]
    row = (16, 100, 4, 0, 0, 3)
    good = (three + [(1000, 1000, 0, 39)], [row, (128, 0, 8, 0, 3, 0), (0, 39, 2, D.CMP_ZERO, 3, 1)])
    bad = {"a gap": ([(3, 900, 0, 1), (200, None, 2, 59), (1000, 2001, 61, 39)], [row]),
           "an overlap": ([(3, 900, 0, 2), (200, None, 1, 60), (1000, 2001, 61, 39)], [row]),
           "descending": ([three[1], three[0], three[2]], [row]), "short": (three[:2], [(16, 100, 4, 0, 0, 2)]),
           "long": (three, [(16, 99, 4, 0, 0, 3)]), "an empty piece": (three[:1] + [(7, None, 1, 0)] + three[1:], [(16, 100, 4, 0, 0, 4)]),
           "a null source": ([three[0], (None, None, 1, 60), three[2]], [row]), "past the table": (three, [(16, 100, 4, 0, 1, 3)]),
           "no pieces for a row with bytes": (three, [(16, 100, 4, 0, 0, 0)]), "elem 3": (three, [(16, 100, 3, 0, 0, 3)]),
           "elem 0": (three, [(16, 100, 0, 0, 0, 3)]), "unknown flags": (three, [(16, 100, 4, 2, 0, 3)]),
           "misaligned srcOff": (three, [(8, 100, 4, 0, 0, 3)]), "past stageBytes": (three, [(4000, 100, 4, 0, 0, 3)]),
           "frames overlap": (three, [row, (96, 100, 4, 0, 0, 3)]), "frames not ascending": (three, [(256, 100, 4, 0, 0, 3), row]),
           "a row too long": (three, [(16, 0xFFFFFFE1, 4, D.CMP_ZERO, 0, 3)])}
    for name, (ps, rs) in bad.items():
        rows = rowsof(rs)
        rc, got, _ = run_gpu(gpu_plugin, L, rows, table(ps), len(ps), stage)
        assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all(), name
    for null in ("rows", "d_rows", "pieces", "d_pieces", "stage", "tiles"):
        rows = rowsof(good[1])
        rc, got, _ = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, stage, null=null)
        assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all(), null
    rows = rowsof(good[1])
    rc, got, _ = run_gpu(gpu_plugin, L, rows, table(good[0]), 3, stage)  # a table shorter than the rows say
    assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all()
    rc, got, _ = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, stage, skew=8)
    assert rc < 0 and (got == FILL).all() and (rows["tile0"] == 77).all()
    rc, got, _ = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, stage, n_rows=0)
    assert rc == 0 and (got == FILL).all() and (rows["tile0"] == 77).all()
    rc, got, _ = run_gpu(gpu_plugin, L, rowsof([(16, 0, 4, 0, 0, 0), (32, 0, 1, 0, 0, 0)]), table([]), 0, stage, null="pieces")  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    # the good launch: a zero stage against src ^ base of three pieces; an empty row; a ZERO row whose source is its own base
    rc, got, _ = run_gpu(gpu_plugin, L, rows, table(good[0]), 4, stage)
    assert rc == 0, gpu_plugin.err()
    src = np.arange(8192, dtype=np.uint8)
    c = np.concatenate([src[3:4] ^ src[900:901], src[200:260], src[1000:1039] ^ src[2001:2040]])
    assert rows["tile0"].tolist() == [0, 1, 1]
    assert got.tolist() == [FILL] * GUARD + [int(np.flatnonzero(c)[0]), D.CMP_SAME] + [FILL] * GUARD
