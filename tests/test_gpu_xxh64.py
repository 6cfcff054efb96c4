"""GPU: the content-checksum kernel through the C ABI (qzstd_hip_xxh64, include/qzstd_hip_device.h).  Every row's 64-bit hash must be
python-xxhash's xxh64 (seed 0) of the host copy of its bytes, whatever its length, its neighbours in the wave and the bytes around it;
only d_out[0 .. nRows) is written; the launcher's refusals queue nothing."""
import ctypes as C

import numpy as np
import pytest
import xxhash

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

T = 1024  # QZSTD_HIP_XXH64_TILE: bytes of a row the kernel fetches at a time
GUARD = 8  # 64-bit words in front of and behind d_out
SENTINEL = 0x5EA15EA15EA15EA1
MIXED = [0, 1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1,
         131071, 131072, 131073]


def api(plug):
    L = plug.lib
    L.qzstd_hip_xxh64.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def layout(lens, seed, fill=0xA5):
    """rows at 16-aligned offsets of one stage, gaps of 0, 16 or 32 bytes between them; every byte that belongs to no row — the gaps and
    what lies behind a row's end in its last 16-byte word — holds `fill` -> (stage bytes as numpy, [(srcOff, len)])"""
    rng = np.random.default_rng(seed)
    spec, pos = [], 0
    for k, n in enumerate(lens):
        spec.append((pos, n))
        pos += ((n + 15) & ~15) + 16 * (k % 3)
    stage = np.full(pos + 64, fill, dtype=np.uint8)
    for o, n in spec:
        stage[o:o + n] = rng.integers(0, 256, n, dtype=np.uint8)
    return stage, spec


def run(plug, L, stage_t, spec, base_skew=0, rows_null=False, d_rows_null=False, out_null=False, base_null=False):
    """one launch -> (return value, d_out with its guards as a list of python ints)"""
    n = len(spec)
    out = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda:0")
    rows = (D.HashRow * max(n, 1))()
    for r, (o, ln) in zip(rows, spec):
        r.srcOff, r.len = o, ln
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    assert stage_t.data_ptr() % 16 == 0
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_xxh64(0, None, None if base_null else stage_t.data_ptr() + base_skew, None if rows_null else rows, n,
                               None if d_rows_null else d_rows, None if out_null else out.data_ptr() + 8 * GUARD)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, [int(v) & (2 ** 64 - 1) for v in out.cpu().numpy()]


def expected(stage, spec):
    return [xxhash.xxh64(stage[o:o + n].tobytes()).intdigest() for o, n in spec]


def check(plug, L, stage, spec):
    rc, out = run(plug, L, torch.from_numpy(stage).to("cuda:0"), spec)
    assert rc == 0, plug.err()
    assert out[:GUARD] == [SENTINEL] * GUARD and out[GUARD + len(spec):] == [SENTINEL] * GUARD  # only [0, nRows) is written
    got, want = out[GUARD:GUARD + len(spec)], expected(stage, spec)
    bad = [(k, spec[k][1]) for k in range(len(spec)) if got[k] != want[k]]
    assert not bad, "rows (index, len) with a wrong hash: %s" % bad[:8]
    return got


@pytest.fixture(scope="module")
def mixed_case():
    """every length three times and one row of 1 MiB + 5, shuffled: long and short rows share a wave"""
    lens = MIXED * 3 + [(1 << 20) + 5]
    lens = [lens[i] for i in np.random.default_rng(5).permutation(len(lens))]
    return lens, layout(lens, seed=6)


def test_mixed_lengths_in_one_launch(gpu_plugin, mixed_case):
    lens, (stage, spec) = mixed_case
    waves = [set(lens[i:i + 16]) for i in range(0, len(lens), 16)]
    assert any(max(w) >= 131071 and min(w) <= 8 for w in waves)
    check(gpu_plugin, api(gpu_plugin), stage, spec)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 65])
def test_row_counts_at_the_edges_of_a_wave(gpu_plugin, rows):
    stage, spec = layout([4096 + i for i in range(rows)], seed=rows)
    check(gpu_plugin, api(gpu_plugin), stage, spec)


def test_bytes_around_a_row_do_not_reach_its_hash(gpu_plugin, mixed_case):
    """the gaps between the rows and the bytes behind each row up to the end of its 16-byte word: 0xA5, then 0x5A — the same hashes"""
    lens, (stage, spec) = mixed_case
    other, spec2 = layout(lens, seed=6, fill=0x5A)
    assert spec2 == spec and (stage != other).any()
    for o, n in spec:
        assert (stage[o:o + n] == other[o:o + n]).all()
    L = api(gpu_plugin)
    assert check(gpu_plugin, L, stage, spec) == check(gpu_plugin, L, other, spec)


def test_launcher_refusals_queue_nothing(gpu_plugin):
    L = api(gpu_plugin)
    stage, spec = layout([100, 0, 5000, 33], seed=2)
    st = torch.from_numpy(stage).to("cuda:0")
    untouched = [SENTINEL] * (2 * GUARD + len(spec))
    for name, kw in (("rows", dict(rows_null=True)), ("d_rows", dict(d_rows_null=True)), ("d_out", dict(out_null=True)),
                     ("d_base with rows that are not empty", dict(base_null=True)), ("d_base not 16-aligned", dict(base_skew=8))):
        rc, out = run(gpu_plugin, L, st, spec, **kw)
        assert rc < 0 and (kw.get("out_null") or out == untouched), name
    rc, out = run(gpu_plugin, L, st, [spec[0], (spec[1][0] + 8, 0), spec[2]])
    assert rc < 0 and out == [SENTINEL] * (2 * GUARD + 3)  # a srcOff that is no multiple of 16, even of an empty row
    rc, out = run(gpu_plugin, L, st, [])
    assert rc == 0 and out == [SENTINEL] * (2 * GUARD)
    rc, out = run(gpu_plugin, L, st, [(0, 0), (0, 0)], base_null=True)  # nothing but empty rows needs no base
    assert rc == 0 and out[GUARD:GUARD + 2] == [0xEF46DB3751D8E999] * 2
    check(gpu_plugin, L, stage, spec)  # and a valid launch afterwards
