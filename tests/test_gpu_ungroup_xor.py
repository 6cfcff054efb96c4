"""GPU: the ungrouping scatter with a base XORed in (qzstd_hip_ungroup_xor, include/qzstd_hip_device.h) alone, through the C ABI, against
numpy: every row of one launch must leave the stage for its destination as ungroup(stage row) ^ base, with the destination and the base at
alignments chosen independently, rows without a base between rows with one, and — base == dst — in place over what the destination held,
neighbours that share a 16-byte word included.  Exactly the rows' bytes may change, a disjoint base never does, and the stage's padding must
never show.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)
ALIGNS = (0, 1, 7, 8, 15)
FILL, PAD = 0xA5, 0xEE


def lens(k):
    """the lengths of tests/test_gpu_ungroup.py"""
    return [0, 1, k - 1, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1, 4095, 4096, 4097, 16384 - 1, 16384, 16384 + k + 1, 131072 + k + 1,
            (1 << 20) + 3]


def api(plug):
    return D.bind_xor_kernels(plug.lib)


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def payload(rng, n):
    """random bytes without the two marker values: a 0xEE or a 0xA5 in the wrong place is then visible as such"""
    a = rng.integers(0, 254, n, dtype=np.uint8)
    a[a >= FILL] += 1
    a[a >= PAD] += 1
    return a


def build(order, seed, packed=False, reverse=False):
    """order: [(destination alignment, base alignment, elem, len, kind)] in DESTINATION order, kind "base" (a base of its own), "none" or
    "self" (base == dst: in place over the destination's old bytes) -> (spec [(dst offset, base offset | None | "self", srcOff, len, elem)] in
    STAGE order, the stage (grouped rows of DELTA bytes at 16-aligned offsets, 0xEE between len and pad16(len) and in the gaps), the initial
    destination bytes, the expected ones, the base bytes).  The rows' final content is marker-free (payload) so that a marker byte in the
    wrong place shows; the delta in the stage is that content XOR the base (or XOR the destination's old bytes).
    packed: every row right behind the one before it, whatever its alignment; reverse: stage order is the reverse of the destination's"""
    rng = np.random.default_rng(seed)
    pos, bpos, rows = 5 if packed else 0, GUARD, []
    for i, (a, b, k, n, kind) in enumerate(order):
        if not packed:
            pos = ((pos + 15) & ~15) + a + (32 if i % 7 == 0 else 0)
        bpos = ((bpos + 15) & ~15) + b
        rows.append((pos, bpos if kind == "base" else (None if kind == "none" else "self"), k, n, payload(rng, n)))
        pos += n
        bpos += n if kind == "base" else 0
    size = pos + 16
    bas = rng.integers(0, 256, bpos + GUARD, dtype=np.uint8)
    init = np.full(size, FILL, dtype=np.uint8)
    want = np.full(size, FILL, dtype=np.uint8)
    deltas = []
    for p, b, k, n, data in rows:
        want[p:p + n] = data
        if b == "self":
            init[p:p + n] = rng.integers(0, 256, n, dtype=np.uint8)  # the previous checkpoint's bytes
            deltas.append(data ^ init[p:p + n])
        else:
            deltas.append(data if b is None else data ^ bas[b:b + n])
    staged = list(zip(rows, deltas))
    staged = staged[::-1] if reverse else staged
    spec, so, pieces = [], 0, []
    for i, ((p, b, k, n, _), delta) in enumerate(staged):
        gap = 32 if i % 5 == 0 else 0
        pieces.append(np.full(gap, PAD, dtype=np.uint8))
        so += gap
        spec.append((p, b, so, n, k))
        pieces.append(numpy_group(delta, k))
        pieces.append(np.full((-n) % 16, PAD, dtype=np.uint8))
        so += n + (-n) % 16
    return spec, np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8), init, want, bas


def run(plug, L, spec, stage, init, bas, stage_skew=0, stage_bytes=None, null=None, null_dst=False):
    """-> (return value, the destination with its guards as numpy, the base tensor as numpy)"""
    dst = torch.full((GUARD + len(init) + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    dst[GUARD:GUARD + len(init)] = torch.from_numpy(init).to("cuda:0")
    base_t = torch.from_numpy(bas).to("cuda:0")
    st = torch.full((len(stage) + 32,), PAD, dtype=torch.uint8, device="cuda:0")
    base = st.data_ptr() + (-st.data_ptr()) % 16
    o = base - st.data_ptr()
    st[o:o + len(stage)] = torch.from_numpy(stage).to("cuda:0")
    assert dst.data_ptr() % 16 == 0 and base_t.data_ptr() % 16 == 0
    rows = (D.UngroupXorRow * max(len(spec), 1))()
    for r, (p, b, so, n, k) in zip(rows, spec):
        r.dst, r.srcOff, r.len, r.elem = (0 if null_dst else dst.data_ptr() + GUARD + p), so, n, k
        r.base = 0 if b is None else (r.dst if b == "self" else base_t.data_ptr() + b)
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ungroup_xor(0, None, None if null == "rows" else rows, len(spec), None if null == "d_rows" else d_rows,
                                     None if null == "stage" else base + stage_skew, len(stage) if stage_bytes is None else stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, dst.cpu().numpy(), base_t.cpu().numpy()


def compare(got, want, spec):
    full = np.full(len(got), FILL, dtype=np.uint8)
    full[GUARD:GUARD + len(want)] = want
    bad = np.flatnonzero(got != full)
    if len(bad):
        at = int(bad[0]) - GUARD
        row = max((r for r in spec if r[0] <= at), key=lambda r: r[0], default=None)
        raise AssertionError("destination differs from numpy at byte %d, %d bytes in all (got 0x%02x, want 0x%02x); row (dst, base, srcOff, len, elem) = %s"
                             % (at, len(bad), got[bad[0]], full[bad[0]], row))
    assert not (got == PAD).any()  # no byte of the stage's padding anywhere


def align_pairs(n):
    """(destination alignment, base alignment): all 25 pairs of ALIGNS, for the longest rows five that differ and one that agrees"""
    if n < (1 << 20):
        return [(a, b) for a in ALIGNS for b in ALIGNS]
    return [(ALIGNS[i], ALIGNS[(i + 2) % 5]) for i in range(5)] + [(7, 7)]


def kinds(i):
    return "none" if i % 3 == 1 else ("self" if i % 4 == 2 else "base")


def test_ungroup_xor_kernel_every_length_element_size_and_both_alignments(gpu_plugin):
    L = api(gpu_plugin)
    rng = np.random.default_rng(16)
    order = [(a, b, k, n) for k in ELEMS for n in lens(k) for a, b in align_pairs(n)]  # (agreeing pairs: the one-load path)
    order = [order[i] for i in rng.permutation(len(order))]  # long and short rows interleaved
    order = [(a, b, k, n, kinds(i)) for i, (a, b, k, n) in enumerate(order)]
    for k in ELEMS:  # every element size meets base != dst mod 16, base == dst mod 16, no base and in place, on rows of whole tiles
        big = [r for r in order if r[2] == k and r[3] >= 16384]
        assert any(r[4] == "base" and r[0] != r[1] for r in big) and any(r[4] == "base" and r[0] == r[1] for r in big)
        assert any(r[4] == "none" for r in big) and any(r[4] == "self" for r in big)
    spec, stage, init, want, bas = build(order, seed=1)
    rc, got, bas_after = run(gpu_plugin, L, spec, stage, init, bas)
    assert rc == 0, gpu_plugin.err()
    compare(got, want, spec)
    assert np.array_equal(bas_after, bas)  # a disjoint base is only read


@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("mode", ("self", "mixed"))
def test_rows_packed_back_to_back_share_their_words(gpu_plugin, reverse, mode):
    """no gap between neighbours, boundaries that are no multiple of 16: every shared word has two owners, in two workgroups.  "self": every
    row restores in place (base == dst), for every element size; "mixed": rows with a base of their own, without one and in place side by side"""
    L = api(gpu_plugin)
    sizes = (1, 7, 33, 15, 4097, 17, 16384 + 9, 3, 100003, 31, 16383, 5)
    order = [(0, ALIGNS[(i + j) % 5], k, n, "self" if mode == "self" else kinds(i * 4 + j)) for i, n in enumerate(sizes) for j, k in enumerate(ELEMS)]
    spec, stage, init, want, bas = build(order, seed=2, packed=True, reverse=reverse)
    assert sum(1 for p, _, _, n, _ in spec if (p + n) % 16) > len(spec) // 2
    rc, got, bas_after = run(gpu_plugin, L, spec, stage, init, bas)
    assert rc == 0, gpu_plugin.err()
    compare(got, want, spec)
    assert np.array_equal(bas_after, bas)


def test_rows_without_a_base_are_the_ungroup_kernels(gpu_plugin):
    L = api(gpu_plugin)
    L.qzstd_hip_ungroup.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    order = [(a, 0, k, n, "none") for a in ALIGNS for k in ELEMS for n in (0, 1, 15, 16, 17, 4097, 16384 + k + 1, 70001)]
    spec, stage, init, want, bas = build(order, seed=4)
    rc, got, _ = run(gpu_plugin, L, spec, stage, init, bas)
    assert rc == 0, gpu_plugin.err()
    compare(got, want, spec)
    # the plain kernel on the same rows
    dst = torch.full((GUARD + len(init) + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    st = torch.full((len(stage) + 32,), PAD, dtype=torch.uint8, device="cuda:0")
    base = st.data_ptr() + (-st.data_ptr()) % 16
    st[base - st.data_ptr():base - st.data_ptr() + len(stage)] = torch.from_numpy(stage).to("cuda:0")
    rows = (D.UngroupRow * len(spec))()
    for r, (p, _, so, n, k) in zip(rows, spec):
        r.dst, r.srcOff, r.len, r.elem = dst.data_ptr() + GUARD + p, so, n, k
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, gpu_plugin.err()
    try:
        torch.cuda.synchronize()
        assert L.qzstd_hip_ungroup(0, None, rows, len(spec), d_rows, base, len(stage)) == 0, gpu_plugin.err()
        gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert np.array_equal(dst.cpu().numpy(), got)


def test_ungroup_xor_launcher_refusals_leave_the_destination_untouched(gpu_plugin):
    L = api(gpu_plugin)
    good = [(3, 70, 0, 100, 2), (500, None, 112, 0, 8), (1000, 300, 128, 4000, 4)]  # (dst offset, base offset, srcOff, len, elem): the stage spans 4128 bytes
    stage = payload(np.random.default_rng(3), 4128)
    bas = np.random.default_rng(4).integers(0, 256, 8192, dtype=np.uint8)
    init = np.full(8192, FILL, dtype=np.uint8)
    cases = {"misaligned srcOff": [(3, 70, 8, 100, 2)], "past stageBytes": good[:2] + [(1000, 300, 144, 4000, 4)], "overlap": [good[0], (500, 9, 96, 16, 1)],
             "not ascending": [good[2], good[0]], "elem 0": [(3, 70, 0, 100, 0)], "elem 3": good[:2] + [(1000, 300, 128, 4000, 3)],
             "elem 16": [(3, 70, 0, 100, 16)], "starts past stageBytes": [(3, 70, 4144, 0, 1)]}
    for name, spec in cases.items():
        rc, got, _ = run(gpu_plugin, L, spec, stage, init, bas)
        assert rc < 0 and (got == FILL).all(), name
    for null in ("rows", "d_rows", "stage"):
        rc, got, _ = run(gpu_plugin, L, good, stage, init, bas, null=null)
        assert rc < 0 and (got == FILL).all(), null
    rc, got, _ = run(gpu_plugin, L, good, stage, init, bas, null_dst=True)
    assert rc < 0 and (got == FILL).all()
    rc, got, _ = run(gpu_plugin, L, good, stage, init, bas, stage_skew=8)
    assert rc < 0 and (got == FILL).all()
    rc, got, _ = run(gpu_plugin, L, [good[0], (500, 9, 1 << 36, 16, 1)], stage, init, bas, stage_bytes=1 << 37)
    assert rc < 0 and (got == FILL).all()
    rc, got, _ = run(gpu_plugin, L, [], stage, init, bas)
    assert rc == 0 and (got == FILL).all()
    rc, got, _ = run(gpu_plugin, L, [(3, 70, 0, 0, 2), (500, None, 112, 0, 8)], stage, init, bas)  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    rc, got, bas_after = run(gpu_plugin, L, good, stage, init, bas)
    assert rc == 0 and np.array_equal(bas_after, bas)
    want = np.full(8192, FILL, dtype=np.uint8)
    for p, b, so, n, k in good:
        g = stage[so:so + n]
        nn = n // k
        row = np.concatenate([g[:nn * k].reshape(k, nn).T.reshape(-1), g[nn * k:]])
        want[p:p + n] = row if b is None else row ^ bas[b:b + n]
    full = np.full(len(got), FILL, dtype=np.uint8)
    full[GUARD:GUARD + 8192] = want
    assert np.array_equal(got, full)
