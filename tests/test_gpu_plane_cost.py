"""GPU: the plane cost kernel (qzstd_hip_plane_cost, include/qzstd_hip_device.h) alone, through the C ABI, against the CPU suite's sequential
restatement of it (tests/mock/mock_hip_plane_cost.c, built alone: a histogram byte by byte and QZSTD_planeCost of include/qzstd_planecost.h),
word for word.  One launch of mixed rows: every length of LENS with every content of KINDS, row starts at every offset mod 16, the rows packed
with 1 .. 16 bytes between them that hold a value no row holds (255) — a byte counted in front of or behind a row changes its word.  Then a
single row, and 1000 rows of 64 bytes.  Only d_cost[0 .. nRows) may be written: guard words on both sides.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (1, 15, 16, 17, 4095, 4096, 4097, 65536, 131071, 131072)
KINDS = ("one", "two", "uniform", "skewed", "noise")
GUARD_WORDS = 16
GUARD_VALUE = 0xDEADBEEF
GAP = 255  # between the rows; no row holds it


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("planecost") / "libmockplanecost.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "mock", "mock_hip_plane_cost.c")])
    return D.bind_plane_kernel(C.CDLL(so))


def content(kind, n, rng):
    if kind == "one":
        return np.full(n, 61, dtype=np.uint8)
    if kind == "two":
        return rng.choice(np.array([3, 250], dtype=np.uint8), n)
    if kind == "uniform":
        return (np.arange(n) % 255).astype(np.uint8)
    if kind == "skewed":  # an exponent-like plane: a handful of values, one of them most of the time
        return (56 + np.minimum(rng.geometric(0.45, n), 12)).astype(np.uint8)
    return rng.integers(0, 255, n, dtype=np.uint8)


def pack(specs, seed):
    """rows [(kind, len)] -> (the bytes, [(offset, len)]): row i starts at offset i mod 16 (mod 16), 1 .. 16 gap bytes in front of it"""
    rng = np.random.default_rng(seed)
    pieces, rows, pos = [], [], 0
    for i, (kind, n) in enumerate(specs):
        gap = (i % 16 - pos - 1) % 16 + 1
        pieces.append(np.full(gap, GAP, dtype=np.uint8))
        pos += gap
        assert pos % 16 == i % 16
        pieces.append(content(kind, n, rng))
        rows.append((pos, n))
        pos += n
    pieces.append(np.full(32, GAP, dtype=np.uint8))
    return np.concatenate(pieces), rows


def run(plug, restatement, data, spans):
    """-> (the kernel's words with their guards, the restatement's words)"""
    L = D.bind_plane_kernel(plug.lib)
    n = len(spans)
    rows = (D.PlaneRow * n)(*[D.PlaneRow(o, ln, 0) for o, ln in spans])
    want = np.zeros(n, dtype=np.uint32)
    scratch = (D.PlaneRow * n)()
    host = np.ascontiguousarray(data)
    assert restatement.qzstd_hip_plane_cost(0, None, host.ctypes.data, rows, n, scratch, want.ctypes.data) == 0
    t = torch.from_numpy(host).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    guard = np.full(GUARD_WORDS + n + GUARD_WORDS, GUARD_VALUE, dtype=np.uint32)
    out = torch.from_numpy(guard.view(np.int32)).to("cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_plane_cost(0, None, t.data_ptr(), rows, n, d_rows, out.data_ptr() + 4 * GUARD_WORDS)
        assert rc == 0, plug.err()
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert np.array_equal(t.cpu().numpy(), host)  # only read
    return out.cpu().numpy().view(np.uint32), want


def check(plug, restatement, specs, seed):
    data, spans = pack(specs, seed)
    got, want = run(plug, restatement, data, spans)
    n = len(spans)
    words = got[GUARD_WORDS:GUARD_WORDS + n]
    bad = np.flatnonzero(words != want)
    assert not len(bad), "row %d %s at offset %d: kernel %d, restatement %d; %d rows wrong in all" % (
        bad[0], specs[bad[0]], spans[bad[0]][0], words[bad[0]], want[bad[0]], len(bad))
    assert (got[:GUARD_WORDS] == GUARD_VALUE).all() and (got[GUARD_WORDS + n:] == GUARD_VALUE).all()
    return want


def test_mixed_rows_in_one_launch(gpu_plugin, restatement):
    specs = [(kind, n) for n in LENS for kind in KINDS]
    want = check(gpu_plugin, restatement, specs, 1)
    by = dict(zip(specs, want))
    # what the words mean: one value costs nothing, two values a bit a byte, noise about its length; a gap byte would have shown
    assert all(by[("one", n)] == 0 for n in LENS)
    assert abs(int(by[("two", 131072)]) - 16384) <= 131072 // 1024 + 2 and by[("uniform", 131071)] > 130000 and by[("noise", 131072)] > 130000
    assert by[("skewed", 65536)] < 65536 // 3
    # every start offset mod 16 occurred
    assert {o % 16 for o, _ in pack(specs, 1)[1]} == set(range(16))


def test_a_single_row(gpu_plugin, restatement):
    check(gpu_plugin, restatement, [("noise", 4097)], 2)
    check(gpu_plugin, restatement, [("skewed", 131072)], 3)


def test_a_thousand_rows_of_64_bytes(gpu_plugin, restatement):
    check(gpu_plugin, restatement, [(KINDS[i % len(KINDS)], 64) for i in range(1000)], 4)


def test_launcher_refusals_and_empty_rows(gpu_plugin, restatement):
    L = D.bind_plane_kernel(gpu_plugin.lib)
    t = torch.arange(4096, dtype=torch.int32, device="cuda:0").to(torch.uint8)
    out = torch.full((8,), 7, dtype=torch.int32, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, 64 * C.sizeof(D.PlaneRow))
    try:
        def call(spans, base=t.data_ptr(), rows_null=False, d_null=False, out_null=False, reserved=0):
            rows = (D.PlaneRow * len(spans))(*[D.PlaneRow(o, n, reserved) for o, n in spans])
            rc = L.qzstd_hip_plane_cost(0, None, base, None if rows_null else rows, len(spans), None if d_null else d_rows,
                                        None if out_null else out.data_ptr() + 8)
            gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
            return rc
        good = [(3, 100), (500, 0), (1000, 2000)]
        assert call(good, rows_null=True) < 0 and call(good, d_null=True) < 0 and call(good, out_null=True) < 0
        assert call(good, base=None) < 0 and call([(0, 131073)]) < 0 and call(good, reserved=1) < 0
        assert out.cpu().tolist() == [7] * 8  # nothing was written
        assert call([]) == 0 and call([(0, 0)], base=None) == 0  # an empty row loads nothing, also without a base
        assert out.cpu().tolist() == [7, 7, 0, 7, 7, 7, 7, 7]
        assert call(good) == 0
        host = t.cpu().numpy()
        want = [D.plane_cost(host[o:o + n].tobytes()) for o, n in good]
        assert out.cpu().tolist() == [7, 7] + want + [7, 7, 7] and want[1] == 0
    finally:
        L.qzstd_hip_free(0, d_rows)
