"""GPU: the ungrouping scatter (qzstd_hip_ungroup, include/qzstd_hip_device.h) alone, through the C ABI, against numpy: every row of one
launch must leave the stage for its destination with the byte-grouped layout of include/qzstd_bytegroup.h undone for its own element size,
exactly the rows' bytes may change — neighbours that share a 16-byte word included — and the stage's padding must never show.  No tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)
FILL, PAD = 0xA5, 0xEE


def lens(k):
    return [0, 1, k - 1, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1, 4095, 4096, 4097, 16384 - 1, 16384, 16384 + k + 1, 131072 + k + 1,
            (1 << 20) + 3]


def api(plug):
    L = plug.lib
    for fn in (L.qzstd_hip_ungroup, L.qzstd_hip_group, L.qzstd_hip_gather):
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def payload(rng, n):
    """random bytes without the two marker values: a 0xEE or a 0xA5 in the wrong place is then visible as such"""
    a = rng.integers(0, 254, n, dtype=np.uint8)
    a[a >= FILL] += 1  # skips 0xA5 ...
    a[a >= PAD] += 1   # ... and 0xEE
    return a


def build(order, seed, packed=False, reverse=False):
    """order: [(destination alignment, elem, len)] in DESTINATION order -> (spec [(dst offset, srcOff, len, elem)] in STAGE order, the stage
    (grouped rows at 16-aligned offsets, 0xEE between len and pad16(len) and in the gaps), the expected destination bytes behind the guard).
    packed: every row right behind the one before it, whatever its alignment; reverse: stage order is the reverse of the destination's"""
    rng = np.random.default_rng(seed)
    pos, rows = 5 if packed else 0, []
    for i, (a, k, n) in enumerate(order):
        if not packed:
            pos = ((pos + 15) & ~15) + a + (32 if i % 7 == 0 else 0)
        rows.append((pos, k, n, payload(rng, n)))
        pos += n
    size = pos + 16
    want = np.full(size, FILL, dtype=np.uint8)
    for p, k, n, data in rows:
        want[p:p + n] = data
    staged = rows[::-1] if reverse else rows
    spec, so, pieces = [], 0, []
    for i, (p, k, n, data) in enumerate(staged):
        gap = 32 if i % 5 == 0 else 0
        pieces.append(np.full(gap, PAD, dtype=np.uint8))
        so += gap
        spec.append((p, so, n, k))
        pieces.append(numpy_group(data, k))
        pieces.append(np.full((-n) % 16, PAD, dtype=np.uint8))
        so += n + (-n) % 16
    return spec, np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8), want


def run(plug, L, spec, stage, dst_size, stage_skew=0, stage_bytes=None, null=None, null_dst=False):
    """-> (return value, the destination with its guards as numpy)"""
    dst = torch.full((GUARD + dst_size + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    st = torch.full((len(stage) + 32,), PAD, dtype=torch.uint8, device="cuda:0")
    base = st.data_ptr() + (-st.data_ptr()) % 16
    o = base - st.data_ptr()
    st[o:o + len(stage)] = torch.from_numpy(stage).to("cuda:0")
    rows = (D.UngroupRow * max(len(spec), 1))()
    for r, (p, so, n, k) in zip(rows, spec):
        r.dst, r.srcOff, r.len, r.elem = (0 if null_dst else dst.data_ptr() + GUARD + p), so, n, k
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ungroup(0, None, None if null == "rows" else rows, len(spec), None if null == "d_rows" else d_rows,
                                 None if null == "stage" else base + stage_skew, len(stage) if stage_bytes is None else stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, dst.cpu().numpy()


def compare(got, want, spec):
    full = np.full(len(got), FILL, dtype=np.uint8)
    full[GUARD:GUARD + len(want)] = want
    bad = np.flatnonzero(got != full)
    if len(bad):
        at = int(bad[0]) - GUARD
        row = max((r for r in spec if r[0] <= at), key=lambda r: r[0], default=None)
        raise AssertionError("destination differs from numpy at byte %d, %d bytes in all (got 0x%02x, want 0x%02x); row (dst, srcOff, len, elem) = %s"
                             % (at, len(bad), got[bad[0]], full[bad[0]], row))
    assert not (got == PAD).any()  # no byte of the stage's padding anywhere


def test_ungroup_kernel_every_alignment_element_size_and_length(gpu_plugin):
    L = api(gpu_plugin)
    rng = np.random.default_rng(16)
    order = [(a, k, n) for a in range(16) for k in ELEMS for n in lens(k)]
    order = [order[i] for i in rng.permutation(len(order))]  # long and short rows interleaved
    spec, stage, want = build(order, seed=1)
    rc, got = run(gpu_plugin, L, spec, stage, len(want))
    assert rc == 0, gpu_plugin.err()
    compare(got, want, spec)


def test_destination_alignments_are_all_met(gpu_plugin):
    """the case above puts every (alignment, elem) pair's largest row at that DEVICE alignment: torch allocations are 16-aligned and the
    guard is a multiple of 16, so a row's destination offset mod 16 is its address mod 16"""
    t = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 16 == 0 and GUARD % 16 == 0
    order = [(a, k, n) for a in range(16) for k in ELEMS for n in lens(k)]
    spec, _, _ = build(order, seed=1)
    for k in ELEMS:
        assert {p % 16 for p, _, n, e in spec if e == k and n == (1 << 20) + 3} == set(range(16))


@pytest.mark.parametrize("reverse", (False, True))
def test_rows_packed_back_to_back_share_their_words(gpu_plugin, reverse):
    """no gap between neighbours, boundaries that are no multiple of 16: every shared word has two owners, in two workgroups"""
    L = api(gpu_plugin)
    order = [(0, k, n) for n in (1, 7, 33, 15, 4097, 17, 16384 + 9, 3, 100003, 31, 16383, 5) for k in ELEMS]
    spec, stage, want = build(order, seed=2, packed=True, reverse=reverse)
    ends = {(p + n) % 16 for p, _, n, _ in spec}
    assert len(ends) > 8 and sum(1 for p, _, n, _ in spec if (p + n) % 16) > len(spec) // 2
    rc, got = run(gpu_plugin, L, spec, stage, len(want))
    assert rc == 0, gpu_plugin.err()
    compare(got, want, spec)


def staged(plug, L, fn, rows_t, src_t, spec, stage_bytes):
    """qzstd_hip_gather / qzstd_hip_group of (source offset, stage offset, len, pad, elem) rows -> the stage tensor and its 16-aligned base"""
    st = torch.full((stage_bytes + 32,), PAD, dtype=torch.uint8, device="cuda:0")
    base = st.data_ptr() + (-st.data_ptr()) % 16
    rows = (rows_t * len(spec))()
    for r, (s, d, n, p, k) in zip(rows, spec):
        r.src, r.dstOff, r.len, r.pad = src_t.data_ptr() + s, d, n, p
        if rows_t is D.GroupRow:
            r.elem, r.reserved = k, 0
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        assert getattr(L, fn)(0, None, rows, len(spec), d_rows, base, stage_bytes) == 0, plug.err()
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return st, base


@pytest.mark.parametrize("fn", ("qzstd_hip_gather", "qzstd_hip_group"))
def test_ungroup_inverts_the_gather_and_the_group(gpu_plugin, fn):
    """elem = 1 rows round-trip with qzstd_hip_gather; qzstd_hip_group followed by qzstd_hip_ungroup is the identity"""
    L = api(gpu_plugin)
    rng = np.random.default_rng(5)
    elems = (1,) if fn == "qzstd_hip_gather" else ELEMS
    order = [(a, k, n) for a in (0, 1, 7, 8, 15) for k in elems for n in (0, 1, 15, 16, 17, 4097, 16384 + k + 1, 70001)]
    order = [order[i] for i in rng.permutation(len(order))]
    src = payload(rng, sum(n + 31 for _, _, n in order) + 64)
    src_t = torch.from_numpy(src).to("cuda:0")
    gspec, uspec, pos, so, dpos = [], [], 0, 0, 0
    want_rows = []
    for a, k, n in order:
        pos = ((pos + 15) & ~15) + a
        dpos = ((dpos + 15) & ~15) + (a * 7 + 3) % 16
        gspec.append((pos, so, n, (-n) % 16, k))
        uspec.append((dpos, so, n, k))
        want_rows.append((dpos, src[pos:pos + n]))
        pos += n
        dpos += n
        so += n + (-n) % 16
    st, base = staged(gpu_plugin, L, fn, D.GatherRow if fn == "qzstd_hip_gather" else D.GroupRow, src_t, gspec, so)
    dst = torch.full((GUARD + dpos + 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    rows = (D.UngroupRow * len(uspec))()
    for r, (p, o, n, k) in zip(rows, uspec):
        r.dst, r.srcOff, r.len, r.elem = dst.data_ptr() + GUARD + p, o, n, k
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, gpu_plugin.err()
    try:
        assert L.qzstd_hip_ungroup(0, None, rows, len(uspec), d_rows, base, so) == 0, gpu_plugin.err()
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    want = np.full(dpos + 16, FILL, dtype=np.uint8)
    for p, data in want_rows:
        want[p:p + len(data)] = data
    compare(dst.cpu().numpy(), want, uspec)
    del st


def test_ungroup_launcher_refusals_leave_the_destination_untouched(gpu_plugin):
    L = api(gpu_plugin)
    good = [(3, 0, 100, 2), (500, 112, 0, 8), (1000, 128, 4000, 4)]  # (dst offset, srcOff, len, elem): the stage spans 4128 bytes
    stage = payload(np.random.default_rng(3), 4128)
    cases = {"misaligned srcOff": [(3, 8, 100, 2)], "past stageBytes": good[:2] + [(1000, 144, 4000, 4)], "overlap": [good[0], (500, 96, 16, 1)],
             "not ascending": [good[2], good[0]], "elem 0": [(3, 0, 100, 0)],
             "elem 3": good[:2] + [(1000, 128, 4000, 3)], "elem 16": [(3, 0, 100, 16)], "starts past stageBytes": [(3, 4144, 0, 1)]}
    for name, spec in cases.items():
        rc, got = run(gpu_plugin, L, spec, stage, 8192)
        assert rc < 0 and (got == FILL).all(), name
    for null in ("rows", "d_rows", "stage"):
        rc, got = run(gpu_plugin, L, good, stage, 8192, null=null)
        assert rc < 0 and (got == FILL).all(), null
    rc, got = run(gpu_plugin, L, good, stage, 8192, null_dst=True)
    assert rc < 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, good, stage, 8192, stage_skew=8)
    assert rc < 0 and (got == FILL).all()
    # the group launcher's span limit: 16-byte words of the stage are counted in 32 bits (nothing is read: the refusal comes first)
    rc, got = run(gpu_plugin, L, [good[0], (500, 1 << 36, 16, 1)], stage, 8192, stage_bytes=1 << 37)
    assert rc < 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, [], stage, 8192)
    assert rc == 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, [(3, 0, 0, 2), (500, 112, 0, 8)], stage, 8192)  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, good, stage, 8192)
    assert rc == 0
    want = np.full(8192, FILL, dtype=np.uint8)
    for p, so, n, k in good:
        g = stage[so:so + n]
        nn = n // k
        want[p:p + n] = np.concatenate([g[:nn * k].reshape(k, nn).T.reshape(-1), g[nn * k:]])
    compare(got, want, good)
