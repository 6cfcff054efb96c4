"""GPU: the comparison kernel (qzstd_hip_diff, include/qzstd_hip_device.h) alone, through the C ABI, against numpy: flag i is 1 exactly when
the row's two byte ranges differ.  Rows are cut out of two larger arrays whose surroundings ALWAYS differ (one array holds bytes below 128
everywhere, the other bytes from 128 on everywhere outside its rows), so a masking mistake at a row's first or last word turns a 0
into a 1; a and b take every pair of alignments mod 16; a single differing bit sits in the first byte, the last byte and around the 16 KiB tile
boundary; one launch per case list.  Only d_flags[0 .. nRows) may be written and only tile0 of the caller's rows.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

LENS = (0, 1, 15, 16, 17, 31, 16383, 16384, 16385, 3 * 16384 + 5)
ALIGNS = (0, 1, 7, 8, 15)
GUARD_WORDS = 16
GUARD_VALUE = 0xDEADBEEF
SENTINEL = 0x5A5A5A5A  # tile0 before the call


def variants(n):
    """what differs: nothing, or one bit of the byte at an offset that exists"""
    return [None] + sorted({p for p in (0, n - 1, 16383, 16384, 16385) if 0 <= p < n})


class Case:
    """rows (a offset, b offset, len) over two host arrays; B holds A's row content at the row's place, changed as asked, and bytes that no
    byte of A equals everywhere else"""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.rows, self.patches, self.apos, self.bpos = [], [], 64, 64

    def add(self, n, a_al, b_al, flip=None, packed=False):
        """a row of n bytes at the given alignments mod 16 (packed: right behind the row before it, on both sides); flip: the offset of the
        byte whose bit differs"""
        if not packed:
            self.apos = ((self.apos + 15) & ~15) + 16 + a_al
            self.bpos = ((self.bpos + 15) & ~15) + 16 + b_al
        self.rows.append((self.apos, self.bpos, n))
        if flip is not None:
            self.patches.append((self.bpos + flip, 1 << (len(self.rows) % 7)))
        self.apos += n
        self.bpos += n

    def build(self):
        a = self.rng.integers(0, 128, self.apos + 64, dtype=np.uint8)
        b = self.rng.integers(128, 256, self.bpos + 64, dtype=np.uint8)
        for ao, bo, n in self.rows:
            b[bo:bo + n] = a[ao:ao + n]
        for at, bit in self.patches:
            b[at] ^= bit
        return a, b


def launch(plug, rows_spec, a_ptr, b_ptr, null=None, n_rows=None, prefill=7):
    """-> (return value, the flags with their guard words as numpy, the rows as they came back)"""
    L = D.bind_diff_kernel(plug.lib)
    n = len(rows_spec)
    rows = (D.DiffRow * max(n, 1))()
    for r, (ao, bo, ln) in zip(rows, rows_spec):
        r.a, r.b, r.len, r.tile0 = (a_ptr + ao if ao is not None else 0), (b_ptr + bo if bo is not None else 0), ln, SENTINEL
    host = np.full(GUARD_WORDS + max(n, 1) + GUARD_WORDS, GUARD_VALUE, dtype=np.uint32)
    host[GUARD_WORDS:GUARD_WORDS + max(n, 1)] = prefill
    flags = torch.from_numpy(host.view(np.int32)).to("cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_diff(0, None, None if null == "rows" else rows, n if n_rows is None else n_rows, None if null == "d_rows" else d_rows,
                              None if null == "flags" else flags.data_ptr() + 4 * GUARD_WORDS)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, flags.cpu().numpy().view(np.uint32), [(r.a, r.b, r.len, r.tile0) for r in rows[:n]]


def check(plug, case):
    a, b = case.build()
    a_t, b_t = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    assert a_t.data_ptr() % 16 == 0 and b_t.data_ptr() % 16 == 0
    rc, flags, rows = launch(plug, case.rows, a_t.data_ptr(), b_t.data_ptr())
    assert rc == 0, plug.err()
    n = len(case.rows)
    want = D.diff_flags_ref([(a[ao:ao + ln], b[bo:bo + ln]) for ao, bo, ln in case.rows])
    got = flags[GUARD_WORDS:GUARD_WORDS + n]
    bad = np.flatnonzero(got != want)
    assert not len(bad), "row %d (a offset, b offset, len) = %s: flag %d, numpy %d; %d rows wrong in all" % (
        bad[0], case.rows[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    assert (flags[:GUARD_WORDS] == GUARD_VALUE).all() and (flags[GUARD_WORDS + n:] == GUARD_VALUE).all()  # the guard words
    assert rows == [(a_t.data_ptr() + ao, b_t.data_ptr() + bo, ln, t0) for (ao, bo, ln), t0 in zip(case.rows, D.diff_tile0_ref([r[2] for r in case.rows]))]
    assert np.array_equal(a_t.cpu().numpy(), a) and np.array_equal(b_t.cpu().numpy(), b)  # only read
    return want


def test_every_length_alignment_pair_and_bit_position(gpu_plugin):
    """identical rows give 0 although the bytes just before and just after them differ; one bit anywhere gives 1"""
    case = Case(1)
    for n in LENS:
        for a_al in ALIGNS:
            for b_al in ALIGNS:
                for flip in variants(n):
                    case.add(n, a_al, b_al, flip)
    want = check(gpu_plugin, case)
    assert want.sum() == len(case.patches) and 0 < want.sum() < len(want)
    # (the arrays' construction: what surrounds a row differs on the two sides, so only masking makes an identical row a 0)
    a, b = case.build()
    for ao, bo, n in case.rows[::97]:
        assert a[ao - 1] != b[bo - 1] and a[ao + n] != b[bo + n]


def test_rows_of_one_byte_and_a_row_of_a_mib_in_one_launch(gpu_plugin):
    case = Case(2)
    for i in range(1000):
        case.add(1, i % 16, (5 * i + 3) % 16, 0 if i % 3 == 0 else None)
    case.add(1 << 20, 7, 8, 37 * 16384 + 5)  # one bit in tile 37 of 64
    for i in range(1000):
        case.add(1, (3 * i) % 16, i % 16, 0 if i % 2 else None)
    case.add(1 << 20, 1, 1, None)
    want = check(gpu_plugin, case)
    assert want[1000] == 1 and want[-1] == 0


def test_a_equal_to_b_and_neighbours_in_memory(gpu_plugin):
    """a == b is a row of no differences; rows packed back to back share 16-byte words on both sides, and a difference in one does not show in
    its neighbours"""
    case = Case(3)
    for k, n in enumerate((1, 5, 16, 33, 16384, 16385, 40, 7, 0, 100, 16383)):
        case.add(n, 3, 9, packed=k > 0, flip=(n - 1 if k % 2 and n else None))
    for n in (0, 1, 17, 16384, 3 * 16384 + 5):  # a == b: the same range on both sides (what the b side holds there differs in one bit)
        case.add(n, 5, 5, flip=0 if n else None)
    a, b = case.build()
    a_t, b_t = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    spec = [(ao, bo, n) if k < 11 else (ao, ao - (b_t.data_ptr() - a_t.data_ptr()), n) for k, (ao, bo, n) in enumerate(case.rows)]
    rc, flags, rows = launch(gpu_plugin, spec, a_t.data_ptr(), b_t.data_ptr())
    assert rc == 0, gpu_plugin.err()
    want = D.diff_flags_ref([(a[ao:ao + n], b[bo:bo + n] if k < 11 else a[ao:ao + n]) for k, (ao, bo, n) in enumerate(case.rows)])
    assert list(flags[GUARD_WORDS:GUARD_WORDS + len(spec)]) == list(want)
    assert list(want[:11]) == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0] and not want[11:].any()
    assert all(r[0] == r[1] for r in rows[11:])
    assert (flags[:GUARD_WORDS] == GUARD_VALUE).all() and (flags[GUARD_WORDS + len(spec):] == GUARD_VALUE).all()


def test_launcher_refusals_empty_rows_and_no_rows(gpu_plugin):
    a = np.arange(4096, dtype=np.uint8)
    a_t = torch.from_numpy(a).to("cuda:0")
    b_t = torch.from_numpy(a).to("cuda:0")
    p, q = a_t.data_ptr(), b_t.data_ptr()
    good = [(3, 9, 100), (500, 7, 0), (1000, 2001, 2000)]

    def untouched(res, n):
        rc, flags, rows = res
        return rc < 0 and (flags[GUARD_WORDS:GUARD_WORDS + n] == 7).all() and (flags[:GUARD_WORDS] == GUARD_VALUE).all() and \
            (flags[GUARD_WORDS + n:] == GUARD_VALUE).all() and all(r[3] == SENTINEL for r in rows)

    for null in ("rows", "d_rows", "flags"):
        assert untouched(launch(gpu_plugin, good, p, q, null=null), 3), null
    assert untouched(launch(gpu_plugin, good[:2] + [(None, 2001, 2000)], p, q), 3)  # a null a with len > 0
    assert untouched(launch(gpu_plugin, good[:2] + [(1000, None, 2000)], p, q), 3)  # a null b with len > 0
    assert untouched(launch(gpu_plugin, [good[0], (0, 0, 0xFFFFFFE1)], p, q), 2)    # len > 0xFFFFFFE0
    many = [(0, 0, 0xFFFFFFE0)] * 8193                                              # 8193 x 262144 workgroups: more than 2^31 - 1
    assert untouched(launch(gpu_plugin, many, p, q), len(many))
    # no rows: nothing happens; nothing but empty rows (null addresses allowed): their flags are 0
    rc, flags, _ = launch(gpu_plugin, good, p, q, n_rows=0)
    assert rc == 0 and (flags[GUARD_WORDS:GUARD_WORDS + 3] == 7).all()
    rc, flags, rows = launch(gpu_plugin, [(None, None, 0), (5, 6, 0)], p, q)
    assert rc == 0 and list(flags[GUARD_WORDS:GUARD_WORDS + 2]) == [0, 0] and [r[3] for r in rows] == [0, 0]
    assert (flags[:GUARD_WORDS] == GUARD_VALUE).all() and (flags[GUARD_WORDS + 2:] == GUARD_VALUE).all()
    # and the good rows: both tensors hold the same bytes, the offsets decide
    rc, flags, rows = launch(gpu_plugin, good + [(10, 10, 3000)], p, q)
    assert rc == 0 and list(flags[GUARD_WORDS:GUARD_WORDS + 4]) == [1, 0, 1, 0] and [r[3] for r in rows] == [0, 1, 1, 2]
