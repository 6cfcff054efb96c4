"""GPU: the byte-grouping gather with element differences (qzstd_hip_group_ediff, include/qzstd_hip_device.h) alone, through the C ABI,
byte for byte against the header's own C functions: a flagged row must land as QZSTD_byteGroup(QZSTD_elemDiff(row)), an unflagged one as
qzstd_hip_group lands it, zero padding behind each, and nothing else may change.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

GUARD = 64
ELEMS = (1, 2, 4, 8)
TILE = 16384


def lens(k):
    return [0, 1, k - 1, k, TILE - k, TILE, TILE + k, 3 * TILE + 5]


@pytest.fixture(scope="module")
def L(gpu_plugin):
    lib = D.bind_ediff_kernels(gpu_plugin.lib)
    lib.qzstd_hip_group.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    return lib


def numpy_group(a, k):
    n = len(a) // k
    return np.concatenate([a[:n * k].reshape(n, k).T.reshape(-1), a[n * k:]])


def want_row(a, k, flag):
    if flag:
        a = np.frombuffer(D.elem_diff(a.tobytes(), k), dtype=np.uint8)
    return numpy_group(a, k)


def case(seed=5):
    """rows at each of the 16 source alignments (so every offset mod k) x every element size x every length, flagged and unflagged in turn,
    in a shuffled order, cut out of ONE byte tensor with gaps between them -> (source, [(src off, stage off, len, pad, elem, flag)], stage
    bytes, mask of the source bytes that belong to no row).  Every third row holds 0, 2^(8k) - 1, 0, ...: every difference wraps."""
    rng = np.random.default_rng(seed)
    order = [(a, k, n, f) for a in range(16) for k in ELEMS for n in lens(k) for f in (True, False)]
    order = [order[i] for i in rng.permutation(len(order))]
    spec, pos, so = [], 0, 0
    for i, (a, k, n, f) in enumerate(order):
        pos = ((pos + 15) & ~15) + 16 + a
        pad = (-n) % 16 + (16 if i % 5 == 0 else 0)
        so += 32 if i % 7 == 0 else 0  # some gaps in the stage: they keep what they held
        spec.append((pos, so, n, pad, k, f))
        pos += n
        so += n + pad
    total = pos
    for a in range(16):  # rows that end exactly on the source's last byte
        n = 100 + a
        spec.append((total + 4096 - n, so, n, (-n) % 16, ELEMS[a % 4], True))
        so += n + (-n) % 16
    total += 4096
    src = rng.integers(0, 256, total, dtype=np.uint8)
    outside = np.ones(total, dtype=bool)
    for i, (s, _, n, _, k, _) in enumerate(spec):
        if i % 3 == 0:
            src[s:s + n] = np.resize(np.repeat(np.array([0, 255], dtype=np.uint8), k), n)
        elif i % 3 == 1:  # a slowly rising column, wherever the row starts
            m = n // k
            src[s:s + m * k] = np.frombuffer((np.cumsum(rng.integers(0, 9, m)).astype("<u8") + 250).astype("<u%d" % k).tobytes(), dtype=np.uint8)
        outside[s:s + n] = False
    return src, spec, so, outside


def launch(plug, L, fn, src_ptr, spec, stage_ptr, stage_bytes, flags_field=True, bad_flags=None):
    rows = ((D.GroupEdiffRow if flags_field else D.GroupRow) * max(len(spec), 1))()
    for r, (s, d, n, p, k, f) in zip(rows, spec):
        r.src, r.dstOff, r.len, r.pad, r.elem = src_ptr + s, d, n, p, k
        if flags_field:
            r.flags = bad_flags if bad_flags is not None else (D.EDIFF_DIFF if f else 0)
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = getattr(L, fn)(0, None, rows, len(spec), d_rows, stage_ptr, stage_bytes)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc


def new_stage(stage_bytes):
    stage = torch.full((GUARD + stage_bytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
    skew = (-stage.data_ptr()) % 16
    return stage, stage.data_ptr() + skew + GUARD, lambda: stage.cpu().numpy()[skew:]


def expected(src, spec, size):
    want = np.full(size, 0xA5, dtype=np.uint8)
    for s, d, n, p, k, f in spec:
        want[GUARD + d:GUARD + d + n] = want_row(src[s:s + n], k, f)
        want[GUARD + d + n:GUARD + d + n + p] = 0
    return want


def explain(got, want, spec, stage_bytes):
    bad = np.flatnonzero(got != want)
    if len(bad):
        at = bad[0] - GUARD
        row = max((r for r in spec if r[1] <= at), key=lambda r: r[1], default=None)
        raise AssertionError("stage differs at byte %d (of %d), %d bytes in all; row (src, dstOff, len, pad, elem, flag) = %s" %
                             (at, stage_bytes, len(bad), row))


@pytest.fixture(scope="module")
def mixed(gpu_plugin, L):
    src, spec, stage_bytes, outside = case()
    src_t = torch.from_numpy(src).to("cuda:0")
    stage, ptr, read = new_stage(stage_bytes)
    rc = launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), spec, ptr, stage_bytes)
    assert rc == 0, gpu_plugin.err()
    return src, spec, stage_bytes, outside, read()


def test_every_alignment_element_size_and_length_against_the_c_definition(mixed):
    src, spec, stage_bytes, _, got = mixed
    assert any(s + n == len(src) for s, _, n, _, _, _ in spec)
    for k in ELEMS:
        for f in (True, False):
            assert {s % 16 for s, _, n, _, e, g in spec if e == k and g == f and n == 3 * TILE + 5} == set(range(16))
    explain(got, expected(src, spec, len(got)), spec, stage_bytes)


def test_wrapping_values_by_hand(gpu_plugin, L):
    """x = {0, 2^(8k) - 1, 0, ...}: d = {0, -1, +1, -1, ...}, z = {0, 1, 2, 1, 2, ...}; at src offset 3, over two tiles and a tail"""
    for k in ELEMS:
        n = TILE // k + 7
        data = np.concatenate([np.resize(np.repeat(np.array([0, 255], dtype=np.uint8), k), n * k), np.arange(1, k, dtype=np.uint8)])
        src_t = torch.from_numpy(np.concatenate([np.full(3, 0x5A, dtype=np.uint8), data, np.full(20, 0x5A, dtype=np.uint8)])).to("cuda:0")
        ln = len(data)
        stage, ptr, read = new_stage(ln + (-ln) % 16)
        assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), [(3, 0, ln, (-ln) % 16, k, True)], ptr, ln + (-ln) % 16) == 0
        got = read()[GUARD:GUARD + ln]
        z = np.array([0] + [1 if e % 2 else 2 for e in range(1, n)], dtype=np.uint8)
        want = np.concatenate([z, np.zeros(n * (k - 1), dtype=np.uint8), np.arange(1, k, dtype=np.uint8)])
        assert np.array_equal(got, want), k


def test_unflagged_rows_are_qzstd_hip_groups_and_two_launches_over_subsets_do_not_disturb_each_other(gpu_plugin, L, mixed):
    src, spec, stage_bytes, _, got = mixed
    src_t = torch.from_numpy(src).to("cuda:0")
    plain = [r for r in spec if not r[5]]
    flagged = [r for r in spec if r[5]]
    assert plain and flagged
    stage, ptr, read = new_stage(stage_bytes)
    assert launch(gpu_plugin, L, "qzstd_hip_group", src_t.data_ptr(), plain, ptr, stage_bytes, flags_field=False) == 0, gpu_plugin.err()
    only_plain = read()
    for s, d, n, p, k, f in plain:
        assert np.array_equal(only_plain[GUARD + d:GUARD + d + n + p], got[GUARD + d:GUARD + d + n + p]), (s, d, n, p, k)
    for s, d, n, p, k, f in flagged:  # ...and qzstd_hip_group left the other rows' places alone
        assert (only_plain[GUARD + d:GUARD + d + n + p] == 0xA5).all()
    assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), flagged, ptr, stage_bytes) == 0, gpu_plugin.err()
    assert np.array_equal(read(), got)


def test_nothing_outside_a_row_influences_the_stage(gpu_plugin, L, mixed):
    src, spec, stage_bytes, outside, got = mixed
    other = src.copy()
    other[outside] ^= 0xFF
    src_t = torch.from_numpy(other).to("cuda:0")
    stage, ptr, read = new_stage(stage_bytes)
    assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), spec, ptr, stage_bytes) == 0, gpu_plugin.err()
    assert np.array_equal(read(), got)


def test_launcher_refusals_leave_the_stage_untouched(gpu_plugin, L):
    src = np.arange(8192, dtype=np.uint8)
    src_t = torch.from_numpy(src).to("cuda:0")
    good = [(3, 0, 100, 12, 2, True), (500, 112, 0, 16, 8, True), (1000, 128, 4000, 0, 4, False)]
    cases = {"misaligned dstOff": [(3, 8, 100, 12, 2, True)], "len + pad": [(3, 0, 100, 11, 2, True)],
             "past stageBytes": good[:2] + [(1000, 128, 4000, 16, 4, True)], "overlap": [good[0], (500, 96, 16, 0, 1, True)],
             "not ascending": [good[2], good[0]], "elem 0": [(3, 0, 100, 12, 0, True)], "elem 3": good[:2] + [(1000, 128, 4000, 0, 3, True)],
             "elem 16": [(3, 0, 100, 12, 16, False)]}
    for name, spec in cases.items():
        stage, ptr, read = new_stage(4128)
        assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), spec, ptr, 4128) < 0, name
        assert (read() == 0xA5).all(), name
    for bad in (2, 3, 0x80000000):
        stage, ptr, read = new_stage(4128)
        assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), good, ptr, 4128, bad_flags=bad) < 0
        assert (read() == 0xA5).all()
    stage, ptr, read = new_stage(4128)
    assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), good, ptr + 8, 4128) < 0 and (read() == 0xA5).all()
    assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), [], ptr, 4128) == 0 and (read() == 0xA5).all()
    assert launch(gpu_plugin, L, "qzstd_hip_group_ediff", src_t.data_ptr(), good, ptr, 4128) == 0
    got = read()
    assert np.array_equal(got, expected(src, good, len(got)))
