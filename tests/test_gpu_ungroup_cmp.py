"""GPU: the ungrouping comparison (qzstd_hip_ungroup_cmp, include/qzstd_hip_device.h) alone, through the C ABI, against numpy
(qz_device.ungroup_cmp_ref): every tile word is QZSTD_HIP_CMP_SAME or the lowest row offset of its tile at which ungrouped(frame) ^ base
differs from the live bytes.  Rows are cut out of arrays whose surroundings can NEVER match: the live array holds bytes from 128 on outside
its rows, stage and base hold bytes below 128 everywhere (so does every u ^ base), and a masking mistake at a row's first or last word
turns a match into a difference.  Every element size; lengths around the element, the 16-byte word and the 16 KiB tile, with tails that
are no multiple of the element; ref and base at every pair of alignments mod 16; rows with a base, without one, and ZERO rows; one bit
planted in the first byte, the last, around the tile boundary and in the tail, and two in different tiles.  Only d_tiles[0 .. tiles) and
tile0 of the caller's rows may be written; ref, base and stage read back unchanged.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # (imports torch first: one HIP runtime)

torch = D.torch
pytestmark = pytest.mark.gpu

ELEMS = (1, 2, 4, 8)
ALIGNS = (0, 1, 7, 8, 15)
PAIRS = [(a, b) for a in ALIGNS for b in ALIGNS]
MODES = ("base", "nobase", "zero")
BIG = (16383, 16384, 16385, 3 * 16384 + 5)
GUARD_WORDS = 16
GUARD_VALUE = 0xDEADBEEF
PREFILL = 7           # d_tiles before the call
SENTINEL = 0x5A5A5A5A  # tile0 before the call


def small_lens(k):
    return sorted({0, 1, k - 1, k, k + 1, 15, 16, 17})


def flips(n, k):
    """what differs: nothing, or one bit of the byte at an offset that exists — first, last, around the tile boundary, the tail's first byte"""
    tail = n // k * k
    return [None] + sorted({p for p in (0, n - 1, 16383, 16384, 16385, tail) if 0 <= p < n})


class Case:
    """rows over three host arrays — live (ref), base, stage — built so that only a correct kernel calls an unplanted row a match"""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.rows, self.lpos, self.bpos, self.spos = [], 64, 64, 0

    def add(self, n, k, ref_al, base_al, mode="base", flip=(), packed=False):
        """a frame of n content bytes in the grouped layout for k; mode: "base", "nobase" or "zero" (a ZERO row, with a base); flip: offsets
        of the live bytes that get one bit changed; packed: ref and base right behind the row before, sharing its last 16-byte words"""
        if not packed:
            self.lpos = ((self.lpos + 15) & ~15) + 16 + ref_al
            self.bpos = ((self.bpos + 15) & ~15) + 16 + base_al
        zero = mode == "zero"
        self.rows.append(dict(len=n, elem=k, ref=self.lpos, base=None if mode == "nobase" else self.bpos, src=0 if zero else self.spos,
                              zero=zero, pair=(ref_al, base_al), flip=tuple(p for p in ([flip] if isinstance(flip, int) else flip or ()) if p is not None)))
        self.lpos += n
        self.bpos += n
        if not zero:
            self.spos += (n + 15) & ~15

    def build(self):
        """-> (live, base, stage) as numpy uint8; every row's live bytes are ungrouped(frame) ^ base with the planted bits changed"""
        live = self.rng.integers(128, 256, self.lpos + 64, dtype=np.uint8)
        base = self.rng.integers(0, 128, self.bpos + 64, dtype=np.uint8)
        stage = self.rng.integers(0, 128, max(self.spos, 16), dtype=np.uint8)
        for i, r in enumerate(self.rows):
            n, k = r["len"], r["elem"]
            u = np.zeros(n, dtype=np.uint8) if r["zero"] else np.frombuffer(D.ungroup_bytes(stage[r["src"]:r["src"] + n].tobytes(), k), dtype=np.uint8)
            if r["base"] is not None:
                u = u ^ base[r["base"]:r["base"] + n]
            live[r["ref"]:r["ref"] + n] = u
            for p in r["flip"]:
                live[r["ref"] + p] ^= 1 << ((i + p) % 7)
        return live, base, stage

    def want(self, live, base, stage):
        return D.ungroup_cmp_ref([(None if r["zero"] else stage[r["src"]:r["src"] + r["len"]],
                                   None if r["base"] is None else base[r["base"]:r["base"] + r["len"]],
                                   live[r["ref"]:r["ref"] + r["len"]], r["elem"]) for r in self.rows])

    def fill(self, rows, live_ptr, base_ptr):
        for c, r in zip(rows, self.rows):
            c.ref, c.base, c.srcOff = live_ptr + r["ref"], (0 if r["base"] is None else base_ptr + r["base"]), r["src"]
            c.len, c.elem, c.flags, c.tile0 = r["len"], r["elem"], (D.CMP_ZERO if r["zero"] else 0), SENTINEL

    def tile0(self):
        out, total = [], 0
        for r in self.rows:
            out.append(total)
            total += D.cmp_tiles(r["len"], r["elem"])
        return out, total


def every_case(seed=1):
    """the issue's grid.  Lengths up to 17: every element size x length x alignment pair, the mode and the planted bit cycling; lengths
    around the tile: every element size x length x mode x planted bit for rows with a base, the unplanted row and two planted bits (cycling)
    for rows without one and ZERO rows, the alignment pairs cycling over all 25"""
    case, turn = Case(seed), 0
    for k in ELEMS:
        for n in small_lens(k):
            for ra, ba in PAIRS:
                opts = [(m, f) for m in MODES for f in flips(n, k)]
                m, f = opts[turn % len(opts)]
                case.add(n, k, ra, ba, m, f)
                turn += 1
    for k in ELEMS:
        for n in BIG:
            fl = flips(n, k)
            for m in MODES:
                for f in (fl if m == "base" else [None, fl[1 + turn % (len(fl) - 1)], fl[1 + (turn + 3) % (len(fl) - 1)]]):
                    ra, ba = PAIRS[turn % len(PAIRS)]
                    case.add(n, k, ra, ba, m, f)
                    turn += 7  # (coprime to 25: every pair comes up)
    return case


def launch(plug, case, live_t, base_t, stage_t, null=None, n_rows=None, stage_bytes=None, stage_shift=0, mutate=None, tiles_cap=None):
    """-> (return value, the tile words with their guard words as numpy, the rows as they came back)"""
    L = D.bind_cmp_kernel(plug.lib)
    n = len(case.rows)
    rows = (D.UngroupCmpRow * max(n, 1))()
    case.fill(rows, live_t.data_ptr(), base_t.data_ptr())
    if mutate:
        mutate(rows)
    total = case.tile0()[1] if tiles_cap is None else tiles_cap  # (tiles_cap: a launch that must be refused)
    host = np.full(GUARD_WORDS + max(total, 1) + GUARD_WORDS, GUARD_VALUE, dtype=np.uint32)
    host[GUARD_WORDS:GUARD_WORDS + max(total, 1)] = PREFILL
    tiles = torch.from_numpy(host.view(np.int32)).to("cuda:0")
    d_rows = L.qzstd_hip_malloc(0, C.sizeof(rows))
    assert d_rows, plug.err()
    try:
        torch.cuda.synchronize()
        rc = L.qzstd_hip_ungroup_cmp(0, None, None if null == "rows" else rows, n if n_rows is None else n_rows, None if null == "d_rows" else d_rows,
                                     None if null == "stage" else stage_t.data_ptr() + stage_shift,
                                     stage_t.numel() if stage_bytes is None else stage_bytes,
                                     None if null == "tiles" else tiles.data_ptr() + 4 * GUARD_WORDS)
        plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
    finally:
        L.qzstd_hip_free(0, d_rows)
    return rc, tiles.cpu().numpy().view(np.uint32), [(r.ref, r.base, r.srcOff, r.len, r.elem, r.flags, r.tile0) for r in rows[:n]]


def upload(live, base, stage):
    ts = [torch.from_numpy(x).to("cuda:0") for x in (live, base, stage)]
    assert all(t.data_ptr() % 16 == 0 for t in ts)
    return ts


def check(plug, case):
    live, base, stage = case.build()
    live_t, base_t, stage_t = upload(live, base, stage)
    rc, tiles, rows = launch(plug, case, live_t, base_t, stage_t)
    assert rc == 0, plug.err()
    want = case.want(live, base, stage)
    t0, total = case.tile0()
    assert len(want) == total
    got = tiles[GUARD_WORDS:GUARD_WORDS + total]
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = max(j for j in range(len(t0)) if t0[j] <= bad[0])
        raise AssertionError("tile word %d (row %d: %s): %#x, numpy %#x; %d words wrong in all" % (bad[0], i, case.rows[i], got[bad[0]], want[bad[0]], len(bad)))
    assert (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and (tiles[GUARD_WORDS + max(total, 1):] == GUARD_VALUE).all()  # the guard words
    assert [r[6] for r in rows] == t0 and [r[:6] for r in rows] == [
        (live_t.data_ptr() + r["ref"], 0 if r["base"] is None else base_t.data_ptr() + r["base"], r["src"], r["len"], r["elem"], int(r["zero"]))
        for r in case.rows]  # only tile0 of the caller's rows changed
    assert np.array_equal(live_t.cpu().numpy(), live) and np.array_equal(base_t.cpu().numpy(), base) and np.array_equal(stage_t.cpu().numpy(), stage)
    return want, t0


def first_of(want, t0, case, i):
    """the host's rule: the first word of row i that is not CMP_SAME, or None"""
    w = want[t0[i]:t0[i] + D.cmp_tiles(case.rows[i]["len"], case.rows[i]["elem"])]
    hit = np.flatnonzero(w != D.CMP_SAME)
    return int(w[hit[0]]) if len(hit) else None


def test_every_element_size_length_alignment_pair_mode_and_bit_position(gpu_plugin):
    case = every_case()
    want, t0 = check(gpu_plugin, case)
    # what the numpy reference says is what was planted: an unplanted row matches although everything around it differs
    for i, r in enumerate(case.rows):
        assert first_of(want, t0, case, i) == (min(r["flip"]) if r["flip"] else None), (i, r)
    assert {(r["elem"], r["len"]) for r in case.rows} >= {(k, n) for k in ELEMS for n in tuple(small_lens(k)) + BIG}
    assert {r["pair"] for r in case.rows if r["len"] >= 16383 and r["base"] is not None} == set(PAIRS)
    assert all((r["ref"] % 16, r["base"] % 16) == r["pair"] for r in case.rows if r["base"] is not None)
    live, base, stage = case.build()
    for r in case.rows[::53]:
        assert live[r["ref"] - 1] >= 128 and live[r["ref"] + r["len"]] >= 128 and (stage < 128).all() and (base < 128).all()


def test_two_differences_in_different_tiles_and_neighbours_in_memory(gpu_plugin):
    """the lower of two planted offsets is the row's answer and each tile reports its own; rows packed back to back share 16-byte words of
    ref and base, and a difference in one does not show in its neighbours; ref == base compares the frame with zero"""
    case = Case(2)
    for k in ELEMS:
        case.add(3 * 16384 + 5, k, 7, 8, "base", (40000, 16385))
        case.add(3 * 16384 + 5, k, 1, 15, "zero", (3 * 16384 + 4, 5))
        case.add(2 * 16384 + 3, k, 15, 0, "nobase", (16383, 16384))
    for j, n in enumerate((1, 5, 16, 33, 16384, 16385, 40, 7, 0, 100, 16383)):
        case.add(n, ELEMS[j % 4], 3, 9, MODES[j % 3], flip=(n - 1 if j % 2 and n else None), packed=j > 0)
    want, t0 = check(gpu_plugin, case)
    for i, r in enumerate(case.rows):
        assert first_of(want, t0, case, i) == (min(r["flip"]) if r["flip"] else None), (i, r)
    assert list(want[t0[0]:t0[0] + 4]) == [D.CMP_SAME, 16385, 40000, D.CMP_SAME]
    # ref == base: u[] ^ base == base exactly where u[] is zero
    stage = np.zeros(64, dtype=np.uint8)
    stage[20] = 4
    live = np.arange(64, dtype=np.uint8)
    live_t, base_t, stage_t = upload(live, live.copy(), stage)
    one = Case(0)
    one.add(40, 1, 0, 0, "base")
    one.rows[0].update(ref=3, base=3, src=0)
    rc, tiles, rows = launch(gpu_plugin, one, live_t, live_t, stage_t)
    assert rc == 0 and list(tiles[GUARD_WORDS:GUARD_WORDS + 1]) == [20] and rows[0][0] == rows[0][1]


def test_rows_of_one_byte_and_a_row_of_a_mib_in_one_launch(gpu_plugin):
    case = Case(3)
    for i in range(1000):
        case.add(1, ELEMS[i % 4], i % 16, (5 * i + 3) % 16, MODES[i % 3], 0 if i % 4 == 0 else None)
    case.add(1 << 20, 4, 7, 8, "base", 37 * 16384 + 5)  # one bit in tile 37 of 64
    want, t0 = check(gpu_plugin, case)
    assert first_of(want, t0, case, 1000) == 37 * 16384 + 5 and (want[t0[1000]:] != D.CMP_SAME).sum() == 1


def test_launcher_refusals_empty_rows_and_no_rows(gpu_plugin):
    case = Case(4)
    case.add(100, 2, 3, 9, "base")
    case.add(0, 4, 0, 0, "nobase")
    case.add(20000, 4, 1, 2, "zero")
    case.add(2000, 8, 5, 5, "nobase", 1999)
    live, base, stage = case.build()
    ts = upload(live, base, stage)
    total = case.tile0()[1]

    def untouched(res):
        rc, tiles, rows = res
        return rc < 0 and (tiles[GUARD_WORDS:GUARD_WORDS + total] == PREFILL).all() and (tiles[:GUARD_WORDS] == GUARD_VALUE).all() and \
            (tiles[GUARD_WORDS + total:] == GUARD_VALUE).all() and all(r[6] == SENTINEL for r in rows)

    def setter(i, **kw):
        def f(rows):
            for name, v in kw.items():
                setattr(rows[i], name, v)
        return f

    for null in ("rows", "d_rows", "tiles", "stage"):  # (a null stage: row 0 is neither ZERO nor empty)
        assert untouched(launch(gpu_plugin, case, *ts, null=null)), null
    assert untouched(launch(gpu_plugin, case, *ts, stage_shift=8))                    # d_stage not 16-aligned
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(3, srcOff=120)))     # a srcOff that is no multiple of 16
    for elem in (0, 3, 16):
        assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(0, elem=elem))), elem
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(2, flags=3)))        # a flags bit other than bit 0
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(1, flags=2)))
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(2, ref=0)))          # a null ref with len > 0
    assert untouched(launch(gpu_plugin, case, *ts, stage_bytes=112 + 1999))           # the last frame ends past stageBytes
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(2, len=0xFFFFFFE1)))  # len > 0xFFFFFFE0 (a ZERO row: no stage needed)
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(3, srcOff=96)))      # overlaps row 0's pad16(100) = 112
    assert untouched(launch(gpu_plugin, case, *ts, mutate=setter(0, srcOff=4096)))    # not in ascending stage order
    many = Case(5)                                                                    # 8193 x 262144 workgroups: more than 2^31 - 1
    many.rows = [dict(len=0xFFFFFFE0, elem=1, ref=64, base=None, src=0, zero=True, pair=(0, 0), flip=())] * 8193
    rc, tiles, rows = launch(gpu_plugin, many, *ts, tiles_cap=64)
    assert rc < 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and all(r[6] == SENTINEL for r in rows)
    # no rows, and nothing but empty rows (null addresses allowed): nothing is queued, 0
    rc, tiles, rows = launch(gpu_plugin, case, *ts, n_rows=0)
    assert rc == 0 and (tiles[GUARD_WORDS:GUARD_WORDS + total] == PREFILL).all() and all(r[6] == SENTINEL for r in rows)
    empty = Case(6)
    empty.rows = [dict(len=0, elem=2, ref=0, base=None, src=0, zero=False, pair=(0, 0), flip=()),
                  dict(len=0, elem=8, ref=64, base=64, src=16, zero=True, pair=(0, 0), flip=())]
    rc, tiles, rows = launch(gpu_plugin, empty, *ts, mutate=setter(0, ref=0))
    assert rc == 0 and (tiles[GUARD_WORDS:-GUARD_WORDS] == PREFILL).all() and (tiles[:GUARD_WORDS] == GUARD_VALUE).all()
    # the good launch; ZERO rows alone need no stage at all
    rc, tiles, rows = launch(gpu_plugin, case, *ts)
    assert rc == 0 and list(tiles[GUARD_WORDS:GUARD_WORDS + total]) == list(case.want(live, base, stage)) and [r[6] for r in rows] == case.tile0()[0]
    zeros = Case(7)
    zeros.rows = [dict(case.rows[2], src=0x1234567)]  # (a ZERO row's srcOff is not looked at)
    rc, tiles, rows = launch(gpu_plugin, zeros, *ts, null="stage", stage_bytes=0)
    assert rc == 0 and list(tiles[GUARD_WORDS:GUARD_WORDS + 2]) == [D.CMP_SAME, D.CMP_SAME]
