"""GPU: the byte-grouping gather from pieces (qzstd_hip_group_pieces, include/qzstd_hip_device.h) alone, through the C ABI, against its
definition in plain C (tests/mock/mock_hip_group_pieces.c, built here on its own and run over a host copy of the same memory): every row of
one launch must land in the stage as group(concatenated pieces ^ concatenated bases) for its own element size — rows of every edge length,
cut into one piece, into single bytes, at every offset 1 .. 33, around the 16 KiB tile boundary, into fixed widths 3, 17, 2048 and 2050 and
at random; every piece an allocation of its own whose misalignment cycles through 0 .. 15, its base at another one, absent, or the source
itself — and nothing else may change: the guards before, between and behind the rows, the sources, the bases.  No tolerance anywhere.
One narrowing of the cases, for the table's size: the width-3 cutting is applied to the rows up to 3 x 16 KiB + 1, not to the row of
131072 + 3 bytes (43 692 more pieces per element size and base mode); that row is cut into widths 17, 2048 and 2050, at the tile boundary and
at random."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_bind as B
import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "tests", "mock", "libgroup_pieces_ref.so")
GUARD = 64
FILL = 0xA5
ELEMS = (1, 2, 4, 8)
BASES = ("none", "other", "self")
TILE = 16384
PIECE = np.dtype([("src", "<u8"), ("base", "<u8"), ("off", "<u4"), ("len", "<u4")])
ROW = np.dtype([("dstOff", "<u8"), ("len", "<u4"), ("pad", "<u4"), ("elem", "<u4"), ("piece0", "<u4"), ("nPieces", "<u4"), ("reserved", "<u4")])
assert PIECE.itemsize == C.sizeof(D.GroupPiece) and ROW.itemsize == C.sizeof(D.GroupPiecesRow)


def lens(k):
    return [0, 1, k - 1, 15, 16, 17, TILE - 1, TILE, TILE + 1 + k, 3 * TILE - 1, 3 * TILE + 1, 131072 + 3]


def widths(n, w):
    return [min(w, n - o) for o in range(0, n, w)]


def cuttings(k, seed):
    """-> [(content length, [piece lengths])]: the pieces tile the content"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens(k):
        out.append((n, [n] if n else []))
        if 0 < n <= 17:
            out.append((n, [1] * n))  # every byte a piece: sixteen pieces feed one lane's 16 bytes
        if n > TILE:
            out.append((n, [TILE - 1, 1, 1, n - TILE - 1]))  # cuts at the tile boundary and one byte to either side
        for w in (3, 17, 2048, 2050):
            if n > w and (w > 3 or n <= 3 * TILE + 1):
                out.append((n, widths(n, w)))
        if n > 1:
            points = sorted(set(rng.integers(1, n, min(n - 1, 2 + n // 1500)).tolist()))
            out.append((n, [b - a for a, b in zip([0] + points, points + [n])]))
    for c in range(1, 34):  # a cut inside an element, inside a word, around the 16-byte boundary, of a row of a tile and one byte
        out.append((TILE + 1, [c, TILE + 1 - c]))
    return out


@pytest.fixture(scope="module")
def ref():
    """the definition, built on its own: the mock's source and the byte-grouped layout's"""
    tmp = "%s.%d.tmp" % (REF_SO, os.getpid())
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(B.PKG_DIR, "frontend"), "-o", tmp, os.path.join(ROOT, "tests", "mock", "mock_hip_group_pieces.c"),
                           os.path.join(B.PKG_DIR, "frontend", "qzstd_bytegroup.c")])
    os.replace(tmp, REF_SO)
    return D.bind_pieces_kernel(C.CDLL(REF_SO))


class Memory:
    """the same bytes on the host and on the device, both starts 16-aligned: an address on one side is the same offset on the other"""

    def __init__(self, content: np.ndarray):
        self.host = np.empty(len(content) + 16, dtype=np.uint8)
        self.h0 = (self.host.ctypes.data + 15) & ~15
        self.view = self.host[self.h0 - self.host.ctypes.data:][:len(content)]
        self.view[:] = content
        self.dev = torch.from_numpy(content).to("cuda:0")
        self.d0 = self.dev.data_ptr()
        assert self.d0 % 16 == 0

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.view)


def build(k, mode, seed):
    """one launch: -> (rows, the piece table without addresses, its length, every piece's offset in the source memory, in the base's memory
    (None: no bases; the source's: src == base), the two memories' bytes, stage bytes)"""
    rng = np.random.default_rng(seed)
    spec = cuttings(k, seed)
    spec = [spec[i] for i in rng.permutation(len(spec))]
    plen = np.array([p for _, ps in spec for p in ps], dtype=np.int64)
    npieces = len(plen)
    idx = np.arange(npieces)
    mis, bmis = idx % 16, (7 * idx + 5) % 16
    slot = ((plen + 15 + 15) // 16 + 2) * 16  # a slot per piece: 16 guard bytes, the misalignment, the piece, at least a byte of guard behind
    order = rng.permutation(npieces)           # (the pieces lie in memory in another order than in their rows)
    start = np.empty(npieces, dtype=np.int64)
    start[order] = np.cumsum(np.concatenate([[0], slot[order][:-1]]))
    src_at, base_at = start + 16 + mis, start + 16 + bmis
    # the piece placed last ends on its memory's last byte
    last = order[-1]
    src_total, base_total = int(src_at[last] + plen[last]), int(base_at[last] + plen[last])
    content = rng.integers(0, 256, int(plen.sum()), dtype=np.uint8)
    content[::7] = 0  # (some bytes the XOR leaves alone)
    bcontent = rng.integers(0, 256, int(plen.sum()), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(plen)[:-1]])
    within = np.arange(int(plen.sum())) - np.repeat(first, plen)
    src_mem = np.full(max(src_total, 16), FILL, dtype=np.uint8)
    base_mem = np.full(max(base_total, 16), FILL, dtype=np.uint8)
    src_mem[np.repeat(src_at, plen) + within] = content
    base_mem[np.repeat(base_at, plen) + within] = bcontent
    pieces = np.zeros(max(npieces, 1), dtype=PIECE)
    rows = np.zeros(len(spec), dtype=ROW)
    p0, so = 0, 0
    for r, (n, ps) in enumerate(spec):
        pad = (-n) % 16 + (16 if r % 5 == 0 else 0)
        so += 32 if r % 7 == 0 else 0  # some gaps in the stage: they keep what they held; the other rows are neighbours
        rows[r] = (so, n, pad, k, p0, len(ps), 0)
        pieces["off"][p0:p0 + len(ps)] = np.concatenate([[0], np.cumsum(ps)[:-1]]) if ps else []
        p0 += len(ps)
        so += n + pad
    pieces["len"][:npieces] = plen
    return rows, pieces, npieces, src_at, (None if mode == "none" else (src_at if mode == "self" else base_at)), src_mem, base_mem, so


def addresses(pieces, npieces, src_at, base_at, src0, base0):
    out = pieces.copy()
    out["src"][:npieces] = src0 + src_at
    out["base"][:npieces] = 0 if base_at is None else base0 + base_at
    return out


def run_gpu(plug, L, rows, pieces, npieces, stage_bytes, skew=0, null=None, n_rows=None):
    """-> (return value, the stage with its guards as numpy)"""
    stage = torch.full((GUARD + stage_bytes + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    s0 = stage.data_ptr() + (-stage.data_ptr()) % 16
    d_rows = L.qzstd_hip_malloc(0, max(rows.nbytes, 16))
    d_pieces = L.qzstd_hip_malloc(0, max(pieces.nbytes, 16))
    assert d_rows and d_pieces, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_group_pieces(0, None, None if null == "rows" else rows.ctypes.data, len(rows) if n_rows is None else n_rows,
                                      None if null == "d_rows" else d_rows, None if null == "pieces" else pieces.ctypes.data, npieces,
                                      None if null == "d_pieces" else d_pieces, None if null == "stage" else s0 + GUARD + skew, stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
        L.qzstd_hip_free(0, d_pieces)
    return rc, stage.cpu().numpy()[s0 - stage.data_ptr():][:GUARD + stage_bytes + GUARD]


def run_ref(ref, rows, pieces, npieces, stage_bytes):
    raw = np.full(GUARD + stage_bytes + GUARD + 16, FILL, dtype=np.uint8)
    s0 = (raw.ctypes.data + 15) & ~15
    d_rows, d_pieces = np.zeros_like(rows), np.zeros_like(pieces)
    rc = ref.qzstd_hip_group_pieces(0, None, rows.ctypes.data, len(rows), d_rows.ctypes.data, pieces.ctypes.data, npieces, d_pieces.ctypes.data,
                                    s0 + GUARD, stage_bytes)
    return rc, raw[s0 - raw.ctypes.data:][:GUARD + stage_bytes + GUARD]


def api(plug):
    L = D.bind_pieces_kernel(D.bind_xor_kernels(plug.lib))
    return L


@pytest.mark.parametrize("mode", BASES)
@pytest.mark.parametrize("k", ELEMS)
def test_group_pieces_kernel_against_its_definition(gpu_plugin, ref, k, mode):
    L = api(gpu_plugin)
    rows, pieces, npieces, src_at, base_at, src_mem, base_mem, stage_bytes = build(k, mode, 40 + k)
    assert len({int(a) % 16 for a in src_at}) == 16 and int(pieces["len"].min()) == 1
    if mode == "other":
        assert np.any((src_at - base_at) % 16 != 0)
    src, bas = Memory(src_mem), Memory(base_mem)
    rc, want = run_ref(ref, rows, addresses(pieces, npieces, src_at, base_at, src.h0, bas.h0 if mode == "other" else src.h0), npieces, stage_bytes)
    assert rc == 0
    rc, got = run_gpu(gpu_plugin, L, rows, addresses(pieces, npieces, src_at, base_at, src.d0, bas.d0 if mode == "other" else src.d0), npieces,
                      stage_bytes)
    assert rc == 0, gpu_plugin.err()
    if mode == "self":  # (src == base: rows of zeros, their padding included; the gaps keep what they held)
        assert not want[GUARD + int(rows["dstOff"][1]):GUARD + int(rows["dstOff"][1] + rows["len"][1])].any()
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = int(bad[0]) - GUARD
        r = int(np.searchsorted(rows["dstOff"], at, side="right")) - 1
        ps = pieces[int(rows["piece0"][r]):int(rows["piece0"][r] + rows["nPieces"][r])]
        raise AssertionError("stage differs from the definition at byte %d (of %d), %d bytes in all; row %d: dstOff %d len %d elem %d, piece lengths %s..." %
                             (at, stage_bytes, len(bad), r, rows["dstOff"][r], rows["len"][r], k, ps["len"][:8].tolist()))
    assert (got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all()
    assert src.unchanged() and bas.unchanged()  # the sources, the bases and their guards: only read


def test_rows_of_one_piece_give_the_group_xor_kernels_stage(gpu_plugin):
    L = api(gpu_plugin)
    rng = np.random.default_rng(9)
    spec, so, pos = [], 0, 0
    for i, (k, n) in enumerate((k, n) for k in ELEMS for n in lens(k)):
        pos = ((pos + 15) & ~15) + i % 16
        spec.append((pos, (pos + 4099 + 3 * i) if i % 3 else None, so, n, (-n) % 16, k))
        pos += n
        so += n + (-n) % 16
    size = max(max(s, b or 0) + n for s, b, _, n, _, _ in spec)  # (the memory is sized from the layout: the last base range ends on its last byte)
    mem = torch.from_numpy(rng.integers(0, 256, size, dtype=np.uint8)).to("cuda:0")
    assert all(0 <= s and s + n <= mem.numel() and (b is None or b + n <= mem.numel()) for s, b, _, n, _, _ in spec)
    rows = np.zeros(len(spec), dtype=ROW)
    pieces = np.zeros(len(spec), dtype=PIECE)
    xrows = (D.GroupXorRow * len(spec))()
    p = 0
    for r, (s, b, d, n, pad, k) in enumerate(spec):
        rows[r] = (d, n, pad, k, p, 1 if n else 0, 0)
        if n:
            pieces[p] = (mem.data_ptr() + s, mem.data_ptr() + b if b is not None else 0, 0, n)
            p += 1
        x = xrows[r]
        x.src, x.base, x.dstOff, x.len, x.pad, x.elem, x.reserved = mem.data_ptr() + s, (mem.data_ptr() + b if b is not None else 0), d, n, pad, k, 0
    rc, got = run_gpu(gpu_plugin, L, rows, pieces, p, so)
    assert rc == 0, gpu_plugin.err()
    stage = torch.full((GUARD + so + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    s0 = stage.data_ptr() + (-stage.data_ptr()) % 16
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(xrows))
    try:
        torch.cuda.synchronize()
        assert L.qzstd_hip_group_xor(0, None, xrows, len(spec), d_rows, s0 + GUARD, so) == 0, gpu_plugin.err()
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert np.array_equal(got, stage.cpu().numpy()[s0 - stage.data_ptr():][:GUARD + so + GUARD])


def test_group_pieces_launcher_refusals_leave_the_stage_untouched(gpu_plugin):
    L = api(gpu_plugin)
    mem = torch.from_numpy(np.arange(8192, dtype=np.uint8)).to("cuda:0")
    a = mem.data_ptr()

    def table(ps):
        t = np.zeros(max(len(ps), 1), dtype=PIECE)
        for i, (src, base, off, n) in enumerate(ps):
            t[i] = (a + src if src is not None else 0, a + base if base is not None else 0, off, n)
        return t

    def rowsof(rs):
        t = np.zeros(max(len(rs), 1), dtype=ROW)
        for i, r in enumerate(rs):
            t[i] = r
        return t[:len(rs)] if rs else t[:0]

    three = [(3, 900, 0, 1), (200, None, 1, 60), (1000, 2001, 61, 39)]
    row = (16, 100, 12, 4, 0, 3, 0)
    good = (three + [(1000, 2001, 0, 39)], [row, (128, 0, 16, 8, 3, 0, 0), (144, 39, 9, 2, 3, 1, 0)])
    bad = {"a gap": ([(3, 900, 0, 1), (200, None, 2, 59), (1000, 2001, 61, 39)], [row]),
           "an overlap": ([(3, 900, 0, 2), (200, None, 1, 60), (1000, 2001, 61, 39)], [row]),
           "descending": ([three[1], three[0], three[2]], [row]), "short": (three[:2], [(16, 100, 12, 4, 0, 2, 0)]),
           "long": (three, [(16, 99, 13, 4, 0, 3, 0)]), "an empty piece": (three[:1] + [(7, None, 1, 0)] + three[1:], [(16, 100, 12, 4, 0, 4, 0)]),
           "a null source": ([three[0], (None, None, 1, 60), three[2]], [row]), "past the table": (three, [(16, 100, 12, 4, 1, 3, 0)]),
           "no pieces for a row with bytes": (three, [(16, 100, 12, 4, 0, 0, 0)]), "elem 3": (three, [(16, 100, 12, 3, 0, 3, 0)]),
           "elem 0": (three, [(16, 100, 12, 0, 0, 3, 0)]), "reserved": (three, [(16, 100, 12, 4, 0, 3, 1)]),
           "misaligned dstOff": (three, [(8, 100, 12, 4, 0, 3, 0)]), "len + pad": (three, [(16, 100, 11, 4, 0, 3, 0)]),
           "past stageBytes": (three, [(4032, 100, 12, 4, 0, 3, 0)]), "rows overlap": (three, [row, (96, 100, 12, 4, 0, 3, 0)]),
           "rows not ascending": (good[0], [good[1][2], row])}
    for name, (ps, rs) in bad.items():
        rc, got = run_gpu(gpu_plugin, L, rowsof(rs), table(ps), len(ps), 4128)
        assert rc < 0 and (got == FILL).all(), name
    for null in ("rows", "d_rows", "pieces", "d_pieces", "stage"):
        rc, got = run_gpu(gpu_plugin, L, rowsof(good[1]), table(good[0]), 4, 4128, null=null)
        assert rc < 0 and (got == FILL).all(), null
    rc, got = run_gpu(gpu_plugin, L, rowsof(good[1]), table(good[0]), 3, 4128)  # a table shorter than the rows say
    assert rc < 0 and (got == FILL).all()
    rc, got = run_gpu(gpu_plugin, L, rowsof(good[1]), table(good[0]), 4, 4128, skew=8)
    assert rc < 0 and (got == FILL).all()
    rc, got = run_gpu(gpu_plugin, L, rowsof(good[1]), table(good[0]), 4, 4128, n_rows=0)
    assert rc == 0 and (got == FILL).all()
    rc, got = run_gpu(gpu_plugin, L, rowsof([(16, 0, 0, 4, 0, 0, 0), (32, 0, 0, 1, 0, 0, 0)]), table([]), 0, 4128, null="pieces")  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    rc, got = run_gpu(gpu_plugin, L, rowsof(good[1]), table(good[0]), 4, 4128)
    assert rc == 0, gpu_plugin.err()
    src = np.arange(8192, dtype=np.uint8)
    c = np.concatenate([src[3:4] ^ src[900:901], src[200:260], src[1000:1039] ^ src[2001:2040]])
    want = np.full(len(got), FILL, dtype=np.uint8)
    want[GUARD + 16:GUARD + 128] = np.concatenate([c.reshape(25, 4).T.reshape(-1), np.zeros(12, dtype=np.uint8)])
    want[GUARD + 128:GUARD + 144] = 0
    d = src[1000:1039] ^ src[2001:2040]
    want[GUARD + 144:GUARD + 192] = np.concatenate([d[:38].reshape(19, 2).T.reshape(-1), d[38:], np.zeros(9, dtype=np.uint8)])
    assert np.array_equal(got, want)
