"""GPU: the Huffman literals coder (qzstd_hip_huf_code, include/qzstd_hip_device.h) alone, through the C ABI, against the CPU suite's sequential
restatement of it (tests/mock/mock_hip_huf_code.c, built alone over include/qzstd_hufblock.h), byte for byte: cost words, size words, dense
offsets, and in the dense area the code lengths, jump tables, streams and padding.  One launch of mixed rows: every length of LENS with every
content of KINDS, rows that are not coded among them (empty, below 1 KiB, one symbol, noise), row starts at every offset mod 16, 1 .. 16
bytes between the rows that hold a value the rows hold nowhere or hardly anywhere — a byte coded from in front of or behind a row changes its streams.  Every output has
guard bytes on both sides.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (1024, 1025, 1026, 1027, 16383, 16384, 65536, 131072)
KINDS = ("two", "skew", "all256", "high", "one", "noise", "exponent")
GUARD = 64  # bytes, on both sides of every output
GAP = 7  # between the rows; no row's content holds it (see content)


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hufcode") / "libmockhufcode.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "mock", "mock_hip_huf_code.c")])
    return D.bind_huf_kernel(C.CDLL(so))


def content(kind, n, rng):
    if kind == "one":
        return np.full(n, 61, dtype=np.uint8)
    if kind == "two":
        return rng.choice(np.array([3, 250], dtype=np.uint8), n, p=[0.8, 0.2])
    if kind == "skew":  # counts 1, 1, 2, 3, 5, ...: plain Huffman is deeper than 11
        fib = [1, 1]
        while sum(fib) < n:
            fib.append(fib[-1] + fib[-2])
        return rng.permutation(np.repeat(np.arange(len(fib)), fib).astype(np.uint8)[:n] + 10)
    if kind == "all256":  # all 256 values occur (GAP in the first 256 bytes only), a few of them most of the time
        v = np.where(rng.random(n) < 0.85, rng.integers(40, 48, n), rng.integers(0, 256, n)).astype(np.uint8)
        v[v == GAP] = 8
        v[:256] = np.arange(256)
        return v
    if kind == "high":
        return (200 + np.minimum(rng.geometric(0.2, n) - 1, 55)).astype(np.uint8)
    if kind == "exponent":  # the high byte of bf16 N(0, 0.02) weights
        w = rng.normal(0.0, 0.02, n).astype(np.float32)
        return (w.view(np.uint32) >> 24).astype(np.uint8)
    v = rng.integers(0, 256, n, dtype=np.uint8)
    v[v == GAP] = 8
    return v


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


def guarded(nbytes, value):
    """a device tensor of GUARD + nbytes + GUARD bytes of `value`, 16-byte aligned inside"""
    t = torch.full((GUARD + nbytes + GUARD,), value, dtype=torch.uint8, device="cuda:0")
    assert (t.data_ptr() + GUARD) % 16 == 0
    return t


def run(plug, restatement, data, spans):
    """-> per output (the kernel's bytes with their guards, the restatement's bytes)"""
    L = D.bind_huf_kernel(plug.lib)
    n = len(spans)
    rows = (D.PlaneRow * n)(*[D.PlaneRow(o, ln, 0) for o, ln in spans])
    need = sum(D.huf_row_bytes(ln) for _, ln in spans)
    assert L.qzstd_hip_huf_code_bytes(rows, n) == need == restatement.qzstd_hip_huf_code_bytes(rows, n)
    host = np.ascontiguousarray(data)
    want = {"cost": np.zeros(n, dtype=np.uint32), "size": np.zeros(n, dtype=np.uint32), "off": np.zeros(n + 1, dtype=np.uint32),
            "dense": np.full(need + 16, 0xA5, dtype=np.uint8)}
    scratch_rows = (D.PlaneRow * n)()
    dense_host = np.zeros(need + 64, dtype=np.uint8)
    base16 = (-dense_host.ctypes.data) % 16
    scratch_host = np.zeros(D.huf_scratch_bytes(n, need) + 64, dtype=np.uint8)
    sbase16 = (-scratch_host.ctypes.data) % 16
    assert restatement.qzstd_hip_huf_code(0, None, host.ctypes.data, rows, n, scratch_rows, want["cost"].ctypes.data, want["size"].ctypes.data,
                                          want["off"].ctypes.data, dense_host.ctypes.data + base16, need,
                                          scratch_host.ctypes.data + sbase16, D.huf_scratch_bytes(n, need)) == 0
    used = int(want["off"][n])
    want["dense"][:used] = dense_host[base16:base16 + used]
    t = torch.from_numpy(host).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    outs = {"cost": guarded(4 * n, 0xEE), "size": guarded(4 * n, 0xEE), "off": guarded(4 * (n + 1), 0xEE), "dense": guarded(need + 16, 0xA5)}
    scratch = guarded(D.huf_scratch_bytes(n, need), 0x5A)
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_huf_code(0, None, t.data_ptr(), rows, n, d_rows, outs["cost"].data_ptr() + GUARD, outs["size"].data_ptr() + GUARD,
                                  outs["off"].data_ptr() + GUARD, outs["dense"].data_ptr() + GUARD, need, scratch.data_ptr() + GUARD,
                                  D.huf_scratch_bytes(n, need))
        assert rc == 0, plug.err()
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    assert np.array_equal(t.cpu().numpy(), host)  # only read
    sc = scratch.cpu().numpy()
    assert (sc[:GUARD] == 0x5A).all() and (sc[-GUARD:] == 0x5A).all()
    return {k: outs[k].cpu().numpy() for k in outs}, want, used


def check(plug, restatement, specs, seed):
    data, spans = pack(specs, seed)
    got, want, used = run(plug, restatement, data, spans)
    n = len(spans)
    for name, fill in (("cost", 0xEE), ("size", 0xEE), ("off", 0xEE), ("dense", 0xA5)):
        g = got[name]
        assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), name + ": guard bytes written"
    cost, size, off = (got[k][GUARD:-GUARD].view(np.uint32) for k in ("cost", "size", "off"))
    for name, words in (("cost", cost), ("size", size), ("off", off)):
        bad = np.flatnonzero(words != want[name])
        assert not len(bad), "%s word of row %d %s at offset %d: kernel %d, restatement %d; %d wrong in all" % (
            name, bad[0], specs[min(bad[0], n - 1)], spans[min(bad[0], n - 1)][0], words[bad[0]], want[name][bad[0]], len(bad))
    dense = got["dense"][GUARD:-GUARD]
    for i in range(n):  # lengths, jump table, streams, padding: row by row, for a message that says where
        if not size[i]:
            assert off[i + 1] == off[i]
            continue
        a, b = int(off[i]), int(off[i + 1])
        assert a % 16 == 0 and b - a == (D.HUF_LENGTHS_BYTES + int(size[i]) + 15) // 16 * 16
        g, w = dense[a:b], want["dense"][a:b]
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            part = "lengths" if at < 128 else "jump table" if at < 134 else "streams" if at < 128 + size[i] else "padding"
            raise AssertionError("row %d %s at offset %d: %s differ at byte %d of %d (kernel %d, restatement %d)" % (
                i, specs[i], spans[i][0], part, at, b - a, g[at], w[at]))
    assert np.array_equal(dense[:used], want["dense"][:used])
    assert (dense[used:] == 0xA5).all(), "dense area written behind its end"
    return dict(zip(specs, zip(size.tolist(), cost.tolist())))


def test_mixed_rows_in_one_launch(gpu_plugin, restatement):
    specs = [(kind, n) for n in LENS for kind in KINDS]
    # rows that are never coded, spread among them: empty, short, just below the limit
    for at, extra in ((5, ("noise", 0)), (17, ("two", 1023)), (30, ("exponent", 64)), (41, ("two", 0)), (50, ("skew", 700))):
        specs.insert(at, extra)
    by = check(gpu_plugin, restatement, specs, 1)
    # what the words mean
    assert all(by[("one", n)] == (0, 0) for n in LENS)  # one symbol: costs nothing, not coded
    assert all(by[("noise", n)][0] == 0 for n in LENS if n >= 16383) and by[("noise", 0)] == (0, 0)  # (1 KiB of noise is not flat)
    assert by[("two", 1023)][0] == 0 and by[("exponent", 64)][0] == 0 and by[("skew", 700)][0] == 0 and by[("two", 1023)][1] > 0
    for kind in ("two", "skew", "all256", "high", "exponent"):
        for n in LENS:
            size, cost = by[(kind, n)]
            # no code beats the order-0 cost, which the cost word states to within n / 1024 + 1 (include/qzstd_planecost.h)
            assert cost - (n // 1024 + 1) <= size < n - ((n >> 6) + 2), (kind, n, size, cost)
    assert by[("exponent", 131072)][0] < 131072 * 0.4
    assert {o % 16 for o, _ in pack(specs, 1)[1]} == set(range(16))


def test_a_single_row_and_every_start_offset(gpu_plugin, restatement):
    check(gpu_plugin, restatement, [("exponent", 131072)], 2)
    check(gpu_plugin, restatement, [("two", 1024)], 3)
    check(gpu_plugin, restatement, [("exponent", 4099 + i) for i in range(16)] + [("high", 1029)] * 16, 4)


def test_many_short_rows(gpu_plugin, restatement):
    kinds = ("two", "one", "exponent", "noise", "high")
    check(gpu_plugin, restatement, [(kinds[i % 5], (0, 1024, 1500, 100, 2047)[i % 5]) for i in range(600)], 5)


def test_launcher_refusals(gpu_plugin, restatement):
    L = D.bind_huf_kernel(gpu_plugin.lib)
    t = torch.arange(8192, dtype=torch.int32, device="cuda:0").to(torch.uint8)
    words = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    dense = torch.full((16384,), 9, dtype=torch.uint8, device="cuda:0")
    scratch = torch.full((16384,), 9, dtype=torch.uint8, device="cuda:0")
    d_rows = L.qzstd_hip_malloc(0, 64 * C.sizeof(D.PlaneRow))
    try:
        def call(spans, base=t.data_ptr(), reserved=0, null=None, dense_at=0, dense_bytes=16000, scratch_at=0, scratch_bytes=16000):
            rows = (D.PlaneRow * len(spans))(*[D.PlaneRow(o, n, reserved) for o, n in spans])
            args = {"rows": rows, "d_rows": d_rows, "cost": words.data_ptr(), "size": words.data_ptr() + 64, "off": words.data_ptr() + 128,
                    "dense": dense.data_ptr() + dense_at, "scratch": scratch.data_ptr() + scratch_at}
            if null:
                args[null] = None
            rc = L.qzstd_hip_huf_code(0, None, base, args["rows"], len(spans), args["d_rows"], args["cost"], args["size"], args["off"],
                                      args["dense"], dense_bytes, args["scratch"], scratch_bytes)
            gpu_plugin.check(L.qzstd_hip_stream_sync(0, None), "sync")
            return rc
        good = [(3, 2000), (500, 0), (4000, 3000)]
        need = sum(D.huf_row_bytes(n) for _, n in good)
        for name in ("rows", "d_rows", "cost", "size", "off", "dense", "scratch"):
            assert call(good, null=name) < 0, name
        assert call(good, base=None) < 0 and call([(0, 131073)]) < 0 and call(good, reserved=1) < 0
        assert call(good, dense_at=8) < 0 and call(good, scratch_at=4) < 0
        assert call(good, dense_bytes=need - 1) < 0 and call(good, scratch_bytes=D.huf_scratch_bytes(3, need) - 1) < 0
        assert words.cpu().tolist() == [7] * 64 and (dense.cpu() == 9).all() and (scratch.cpu() == 9).all()  # nothing was written
        assert call([]) == 0 and call(good, dense_bytes=need, scratch_bytes=D.huf_scratch_bytes(3, need)) == 0
        host = t.cpu().numpy()
        assert words.cpu().tolist()[:3] == [D.plane_cost(host[o:o + n].tobytes()) for o, n in good]
    finally:
        L.qzstd_hip_free(0, d_rows)
