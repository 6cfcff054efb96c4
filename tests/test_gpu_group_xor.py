"""GPU: the byte-grouping gather with a base XORed in (qzstd_hip_group_xor, include/qzstd_hip_device.h) alone, through the C ABI, against
numpy: every row of one launch must land in the stage as group(src ^ base) for its own element size, with the source and the base at
alignments chosen independently (so that they differ mod 16), rows without a base between rows with one, zero padding behind every row,
and nothing else may change — the stage between the rows, the base and the guards around it.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)
ALIGNS = (0, 1, 7, 8, 15)
FILL = 0xA5


def lens(k):
    """the lengths of tests/test_gpu_ungroup.py"""
    return [0, 1, k - 1, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1, 4095, 4096, 4097, 16384 - 1, 16384, 16384 + k + 1, 131072 + k + 1,
            (1 << 20) + 3]


def api(plug):
    L = D.bind_xor_kernels(plug.lib)
    L.qzstd_hip_group.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def align_pairs(n):
    """(source alignment, base alignment): all 25 pairs of ALIGNS, for the longest rows five that differ and one that agrees"""
    if n < (1 << 20):
        return [(a, b) for a in ALIGNS for b in ALIGNS]
    return [(ALIGNS[i], ALIGNS[(i + 2) % 5]) for i in range(5)] + [(7, 7)]


def xor_case(seed=16):
    """every element size x every length x source and base alignments chosen independently from ALIGNS, every third row without a base and
    some rows whose base IS their source, cut out of ONE source tensor and ONE base tensor (rows end on both tensors' last bytes)
    -> (source bytes, base bytes, [(source offset, base offset or None, stage offset, len, pad, elem)], stage bytes)"""
    rng = np.random.default_rng(seed)
    order = [(a, b, k, n) for k in ELEMS for n in lens(k) for a, b in align_pairs(n)]
    order = [order[i] for i in rng.permutation(len(order))]
    spec, pos, bpos, so = [], 0, GUARD, 0
    for i, (a, b, k, n) in enumerate(order):
        pos = ((pos + 15) & ~15) + a
        bpos = ((bpos + 15) & ~15) + b
        pad = (-n) % 16 + (16 if i % 5 == 0 else 0)
        so += 32 if i % 7 == 0 else 0  # some gaps in the stage: they keep what they held
        kind = "none" if i % 3 == 1 else ("self" if i % 11 == 5 else "base")
        spec.append((pos, {"none": None, "self": "self", "base": bpos}[kind], so, n, pad, k))
        pos += n
        bpos += n if kind == "base" else 0
        so += n + pad
    # rows that end exactly on the last byte of the source AND of the base, at different alignments of their starts
    total, btotal = pos + 4096, bpos + 4096 + GUARD
    for a in range(8):
        n = 100 + a
        spec.append((total - n, btotal - GUARD - n - (0 if a % 2 else 3), so, n, (-n) % 16, ELEMS[a % 4]))
        so += n + (-n) % 16
    return rng.integers(0, 256, total, dtype=np.uint8), rng.integers(0, 256, btotal, dtype=np.uint8), spec, so


def run(plug, L, src_t, base_t, spec, stage_bytes, stage_skew=0, reserved=0, fn="qzstd_hip_group_xor", null=None):
    """-> (return value, the stage with its guards as numpy)"""
    stage = torch.full((GUARD + stage_bytes + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    base = stage.data_ptr() + (-stage.data_ptr()) % 16
    if fn == "qzstd_hip_group_xor":
        rows = (D.GroupXorRow * max(len(spec), 1))()
        for r, (s, b, d, n, p, k) in zip(rows, spec):
            r.src, r.dstOff, r.len, r.pad, r.elem, r.reserved = (0 if null == "src" else src_t.data_ptr() + s), d, n, p, k, reserved
            r.base = 0 if b is None else (r.src if b == "self" else base_t.data_ptr() + b)
    else:
        rows = (D.GroupRow * max(len(spec), 1))()
        for r, (s, b, d, n, p, k) in zip(rows, spec):
            r.src, r.dstOff, r.len, r.pad, r.elem, r.reserved = src_t.data_ptr() + s, d, n, p, k, reserved
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = getattr(L, fn)(0, None, None if null == "rows" else rows, len(spec), None if null == "d_rows" else d_rows,
                            None if null == "stage" else base + GUARD + stage_skew, stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, stage.cpu().numpy()[base - stage.data_ptr():]


def expected(src, bas, spec, size):
    want = np.full(size, FILL, dtype=np.uint8)
    for s, b, d, n, p, k in spec:
        row = src[s:s + n]
        if b == "self":
            row = np.zeros(n, dtype=np.uint8)
        elif b is not None:
            row = row ^ bas[b:b + n]
        want[GUARD + d:GUARD + d + n] = numpy_group(row, k)
        want[GUARD + d + n:GUARD + d + n + p] = 0
    return want


def test_group_xor_kernel_every_length_element_size_and_both_alignments(gpu_plugin):
    L = api(gpu_plugin)
    src, bas, spec, stage_bytes = xor_case()
    src_t, base_t = torch.from_numpy(src).to("cuda:0"), torch.from_numpy(bas).to("cuda:0")
    assert src_t.data_ptr() % 16 == 0 and base_t.data_ptr() % 16 == 0
    based = [r for r in spec if isinstance(r[1], int)]
    for k in ELEMS:  # src and base differ mod 16 for every element size, also on the longest rows; some agree
        mine = [r for r in based if r[5] == k]
        assert any((s - b) % 16 for s, b, _, n, _, _ in mine if n >= 131072) and any((s - b) % 16 == 0 for s, b, _, _, _, _ in mine)
        assert any(r[1] is None and r[5] == k for r in spec)
    assert any(r[1] == "self" and r[3] > 16 for r in spec)
    assert any(s + n == len(src) for s, _, _, n, _, _ in spec) and any(b + n == len(bas) - GUARD for _, b, _, n, _, _ in based)
    rc, got = run(gpu_plugin, L, src_t, base_t, spec, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    want = expected(src, bas, spec, len(got))
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = bad[0] - GUARD
        row = max((r for r in spec if r[2] <= at), key=lambda r: r[2], default=None)
        raise AssertionError("stage differs from numpy at byte %d (of %d), %d bytes in all; row (src, base, dstOff, len, pad, elem) = %s" %
                             (at, stage_bytes, len(bad), row))
    assert np.array_equal(base_t.cpu().numpy(), bas) and np.array_equal(src_t.cpu().numpy(), src)  # the base, its guards, the source: only read


def test_rows_without_a_base_give_the_group_kernels_stage(gpu_plugin):
    L = api(gpu_plugin)
    src, bas, spec, stage_bytes = xor_case(seed=3)
    spec = [(s, None, d, n, p, k) for s, _, d, n, p, k in spec]
    src_t = torch.from_numpy(src).to("cuda:0")
    rc, got = run(gpu_plugin, L, src_t, None, spec, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    rc, plain = run(gpu_plugin, L, src_t, None, spec, stage_bytes, fn="qzstd_hip_group")
    assert rc == 0, gpu_plugin.err()
    assert np.array_equal(got, plain)
    assert np.array_equal(got, expected(src, bas, spec, len(got)))


def test_group_xor_launcher_refusals_leave_the_stage_untouched(gpu_plugin):
    L = api(gpu_plugin)
    src = np.arange(8192, dtype=np.uint8)
    bas = (np.arange(8192, dtype=np.uint32) * 7 % 251).astype(np.uint8)
    src_t, base_t = torch.from_numpy(src).to("cuda:0"), torch.from_numpy(bas).to("cuda:0")
    good = [(3, 9, 0, 100, 12, 2), (500, None, 112, 0, 16, 8), (1000, 2001, 128, 4000, 0, 4)]
    cases = {"misaligned dstOff": [(3, 9, 8, 100, 12, 2)], "len + pad": [(3, 9, 0, 100, 11, 2)], "past stageBytes": good[:2] + [(1000, 2001, 128, 4000, 16, 4)],
             "overlap": [good[0], (500, 7, 96, 16, 0, 1)], "not ascending": [good[2], good[0]], "elem 0": [(3, 9, 0, 100, 12, 0)],
             "elem 3": good[:2] + [(1000, 2001, 128, 4000, 0, 3)], "elem 16": [(3, 9, 0, 100, 12, 16)]}
    for name, spec in cases.items():
        rc, got = run(gpu_plugin, L, src_t, base_t, spec, 4128)
        assert rc < 0 and (got == FILL).all(), name
    rc, got = run(gpu_plugin, L, src_t, base_t, good, 4128, reserved=1)
    assert rc < 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, src_t, base_t, good, 4128, stage_skew=8)
    assert rc < 0 and (got == FILL).all()
    for null in ("rows", "d_rows", "stage", "src"):
        rc, got = run(gpu_plugin, L, src_t, base_t, good, 4128, null=null)
        assert rc < 0 and (got == FILL).all(), null
    rc, got = run(gpu_plugin, L, src_t, base_t, [], 4128)
    assert rc == 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, src_t, base_t, [(3, 9, 0, 0, 0, 2), (500, None, 112, 0, 0, 8)], 4128)  # nothing but empty rows
    assert rc == 0 and (got == FILL).all()
    rc, got = run(gpu_plugin, L, src_t, base_t, good, 4128)
    assert rc == 0 and np.array_equal(got, expected(src, bas, good, len(got)))
