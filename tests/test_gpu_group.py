"""GPU: the byte-grouping gather (qzstd_hip_group, include/qzstd_hip_device.h) alone, through the C ABI, against numpy: every row of one
launch must land in the stage in the byte-grouped layout of include/qzstd_bytegroup.h for its own element size, zero padding behind it, and
nothing else may change.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)


def lens(k):
    return [0, 1, k - 1, k + 1, 15, 16, 17, 16 * k - 1, 16 * k, 16 * k + 1, 4095, 4096, 4097, 131072, 131072 + k + 1, (1 << 20) + 3]


def api(plug):
    L = plug.lib
    L.qzstd_hip_group.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    L.qzstd_hip_gather.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def group_case(elems=ELEMS, seed=16):
    """rows at each of the 16 source alignments x every element size x every length, long and short interleaved, cut out of ONE byte
    tensor so that the last rows end on the tensor's last byte -> (source bytes, [(source offset, stage offset, len, pad, elem)], stage bytes)"""
    rng = np.random.default_rng(seed)
    order = [(a, k, n) for a in range(16) for k in elems for n in lens(k)]
    order = [order[i] for i in rng.permutation(len(order))]
    spec, pos, so = [], 0, 0
    for i, (a, k, n) in enumerate(order):
        pos = ((pos + 15) & ~15) + a  # this row's source alignment
        pad = (-n) % 16 + (16 if i % 5 == 0 else 0)
        so += 32 if i % 7 == 0 else 0  # some gaps in the stage: they keep what they held
        spec.append((pos, so, n, pad, k))
        pos += n
        so += n + pad
    # the tail: rows that end exactly on the source's last byte, at each alignment of their start, every element size
    total = pos + 4096
    for a in range(16):
        n = 100 + a
        spec.append((total - n, so, n, (-n) % 16, elems[a % len(elems)]))
        so += n + (-n) % 16
    return rng.integers(0, 256, total, dtype=np.uint8), spec, so


def run(plug, L, src_t, spec, stage_bytes, stage_skew=0, reserved=0, fn="qzstd_hip_group"):
    """-> (return value, the stage with its guards as numpy)"""
    stage = torch.full((GUARD + stage_bytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    base = stage.data_ptr() + (-stage.data_ptr()) % 16
    if fn == "qzstd_hip_group":
        rows = (D.GroupRow * max(len(spec), 1))()
        for r, (s, d, n, p, k) in zip(rows, spec):
            r.src, r.dstOff, r.len, r.pad, r.elem, r.reserved = src_t.data_ptr() + s, d, n, p, k, reserved
    else:
        rows = (D.GatherRow * max(len(spec), 1))()
        for r, (s, d, n, p, k) in zip(rows, spec):
            r.src, r.dstOff, r.len, r.pad = src_t.data_ptr() + s, d, n, p
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = getattr(L, fn)(0, None, rows, len(spec), d_rows, base + GUARD + stage_skew, stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, stage.cpu().numpy()[base - stage.data_ptr():]


def expected(src, spec, size):
    want = np.full(size, 0xA5, dtype=np.uint8)
    for s, d, n, p, k in spec:
        want[GUARD + d:GUARD + d + n] = numpy_group(src[s:s + n], k)
        want[GUARD + d + n:GUARD + d + n + p] = 0
    return want


def test_group_kernel_every_alignment_element_size_and_length(gpu_plugin):
    L = api(gpu_plugin)
    src, spec, stage_bytes = group_case()
    src_t = torch.from_numpy(src).to("cuda:0")
    assert any(s + n == len(src) for s, _, n, _, _ in spec)  # rows end on the tensor's last byte
    for k in ELEMS:
        assert {(src_t.data_ptr() + s) % 16 for s, _, n, _, e in spec if e == k and n == (1 << 20) + 3} == set(range(16))
    rc, got = run(gpu_plugin, L, src_t, spec, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    want = expected(src, spec, len(got))
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = bad[0] - GUARD
        row = max((r for r in spec if r[1] <= at), key=lambda r: r[1], default=None)
        raise AssertionError("stage differs from numpy at byte %d (of %d), %d bytes in all; row (src, dstOff, len, pad, elem) = %s" %
                             (at, stage_bytes, len(bad), row))


def test_elem_1_rows_are_the_gathers(gpu_plugin):
    L = api(gpu_plugin)
    src, spec, stage_bytes = group_case(elems=(1,), seed=3)
    src_t = torch.from_numpy(src).to("cuda:0")
    rc, got = run(gpu_plugin, L, src_t, spec, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    rc, gathered = run(gpu_plugin, L, src_t, spec, stage_bytes, fn="qzstd_hip_gather")
    assert rc == 0, gpu_plugin.err()
    assert np.array_equal(got, gathered)
    assert np.array_equal(got, expected(src, spec, len(got)))


def test_group_launcher_refusals_leave_the_stage_untouched(gpu_plugin):
    L = api(gpu_plugin)
    src = np.arange(8192, dtype=np.uint8)
    src_t = torch.from_numpy(src).to("cuda:0")
    good = [(3, 0, 100, 12, 2), (500, 112, 0, 16, 8), (1000, 128, 4000, 0, 4)]
    cases = {"misaligned dstOff": [(3, 8, 100, 12, 2)], "len + pad": [(3, 0, 100, 11, 2)], "past stageBytes": good[:2] + [(1000, 128, 4000, 16, 4)],
             "overlap": [good[0], (500, 96, 16, 0, 1)], "not ascending": [good[2], good[0]], "elem 0": [(3, 0, 100, 12, 0)],
             "elem 3": good[:2] + [(1000, 128, 4000, 0, 3)], "elem 16": [(3, 0, 100, 12, 16)]}
    for name, spec in cases.items():
        rc, got = run(gpu_plugin, L, src_t, spec, 4128)
        assert rc < 0 and (got == 0xA5).all(), name
    rc, got = run(gpu_plugin, L, src_t, good, 4128, reserved=1)
    assert rc < 0 and (got == 0xA5).all()
    rc, got = run(gpu_plugin, L, src_t, good, 4128, stage_skew=8)
    assert rc < 0 and (got == 0xA5).all()
    rc, got = run(gpu_plugin, L, src_t, [], 4128)
    assert rc == 0 and (got == 0xA5).all()
    rc, got = run(gpu_plugin, L, src_t, good, 4128)
    assert rc == 0 and np.array_equal(got, expected(src, good, len(got)))
