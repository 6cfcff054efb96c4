"""The write footprint of qzstd_hip_find_sequences (include/qzstd_hip.h), pinned: a guarded launch and its checker.

`launch()` runs one launch through the C ABI — against the product library on a GPU or against the CPU mock (tests/mock/mock_hip.c) —
with every buffer followed by a guard, the result buffer, the guards and (optionally) the scratch pre-filled from a seeded random byte
stream, the result regions laid out as production lays them (exactly adjacent), with gaps, or shuffled, and returns every buffer read
back whole.  `check_footprint()` compares the read-back with the CPU oracle and with the fill, byte for byte:

    count        every block's count word equals the oracle's count for that seqCap (QZO_ERROR <-> QZSTD_HIP_NSEQ_ERROR)
    entries      a block with a valid count: entries [0, count) are the oracle's, the fourth word (or the packed tag) the item's mark
    tail         ... and every byte of its region behind entry `count` still holds the fill
    outside      everything outside the regions — gaps, the guard behind the last region — holds the fill; an error block may have
                 written inside its own region and nowhere else
    count guard  the guard behind the count words holds the fill
    source, descriptors   unchanged, their guards included
    scratch guard         the guard right behind qzstd_hip_workspace_bytes(level, nBlocks, maxBlockLen) holds the fill

The guards are as long as the farthest a kernel that has lost a bound could reach from inside its own data: a whole block's worth of
entries (sequence_bound(128 KiB)) behind the results, a whole 128 KiB block's scratch region behind the scratch.  A defect is then
detected inside the test's own allocations, never provoked into a fault.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import qz_bind as B

BLOCK_MAX = 1 << 17
SEQ_GUARD_ENTRIES = B.sequence_bound(BLOCK_MAX)  # 16 bytes each: a block that lost its capacity guard writes at most this many entries
SMALL_GUARD = 4096                               # behind buffers the kernels index by block (counts) or only read (source, descriptors)
WORK_FILLS = ("zeros", "ff", "random", "keep")


def stream(seed: int, n: int) -> np.ndarray:
    """n bytes of the seeded fill: random, so that neither an entry of zeros nor a repeated mark can hide in it"""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


class DeviceBuffers:
    """the device allocations of one launch, kept when the caller wants the next launch to find what this one left"""

    def __init__(self, plug, device):
        self.plug, self.device, self.ptr, self.size = plug, device, {}, {}

    def alloc(self, name: str, nbytes: int):
        p = self.plug.lib.qzstd_hip_malloc(self.device, nbytes)
        if not p:
            raise RuntimeError("qzstd_hip_malloc(%d): %s" % (nbytes, self.plug.err()))
        self.ptr[name], self.size[name] = p, nbytes
        return p

    def free(self):
        for p in self.ptr.values():
            self.plug.lib.qzstd_hip_free(self.device, p)
        self.ptr, self.size = {}, {}


class Readback:
    """what launch() returns: the launch's parameters, what every buffer held before the launch (`before`) and after it (`after`),
    both as uint8 arrays over the WHOLE buffer, guard included; `regions[i]` = (first byte, bytes) of block i's result region"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def counts(self) -> np.ndarray:
        return self.after["counts"][:4 * len(self.blocks)].view(np.uint32)


def region_units(cap: int, packed: bool) -> int:
    """16-byte units a region of `cap` entries occupies (qzstd_hip.h: seqOff stays in 16-byte units; packed entries are 8 bytes)"""
    return (cap + 1) // 2 if packed else cap


def launch(plug, blocks: list[bytes], level: int, caps: list[int], *, parse_from: list[int] | None = None, packed_tag: int = 0,
           launch_max_len: int | None = None, layout: str = "adjacent", seed: int = 1, work_fill: str = "random",
           count_fill: int | None = None, reuse: DeviceBuffers | None = None, keep: bool = False, work_room: int = 0,
           device: int = 0) -> Readback:
    """One guarded launch.  layout: "adjacent" (seqOff_{i+1} = seqOff_i + seqCap_i, as production lays the regions), "gaps" (1..6 units
    between them) or "shuffled" (adjacent, in a random order).  work_fill: the scratch before the launch — "zeros", "ff", "random", or
    "keep" = whatever `reuse` (the buffers of an earlier launch(keep=True)) holds; with `reuse` the result buffer keeps the earlier
    launch's bytes too and only the guards are rewritten.  count_fill: the value of every count word before the launch (None: random).
    work_room: that many more bytes of guard behind the scratch (a launch whose buffers a later, larger-scratch launch is to find)."""
    assert layout in ("adjacent", "gaps", "shuffled") and work_fill in WORK_FILLS and len(caps) == len(blocks)
    assert (work_fill == "keep") == (reuse is not None)
    L = plug.lib
    nb = len(blocks)
    packed = packed_tag != 0
    entry = 8 if packed else 16
    rng = np.random.default_rng(seed)
    maxlen = max([len(b) for b in blocks] + [1]) if launch_max_len is None else launch_max_len

    # ---- source: blocks at 16-byte boundaries, guard behind
    offs, total = [], 0
    for b in blocks:
        offs.append(total)
        total += (len(b) + 15) & ~15
    src_bytes = max(total, 16)
    h_src = stream(seed * 7 + 1, src_bytes + SMALL_GUARD)
    h_src[:src_bytes] = 0
    for o, b in zip(offs, blocks):
        h_src[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)

    # ---- result regions
    order = list(range(nb))
    if layout == "shuffled":
        rng.shuffle(order)
    seq_off, at = [0] * nb, 0
    for i in order:
        if layout == "gaps":
            at += int(rng.integers(1, 7))
        seq_off[i] = at
        at += region_units(caps[i], packed)
    seq_bytes = at * 16
    regions = [(seq_off[i] * 16, caps[i] * entry) for i in range(nb)]

    desc = (B.HipBlock * nb)()
    for i, b in enumerate(blocks):
        desc[i].srcOff, desc[i].seqOff, desc[i].srcLen, desc[i].seqCap = offs[i], seq_off[i], len(b), caps[i]
        desc[i].parseFrom = parse_from[i] if parse_from else 0
        desc[i].mark = (B.MARK_COMPACT | (packed_tag & 0xFFF)) if packed else 0
    h_desc = stream(seed * 7 + 2, C.sizeof(desc) + SMALL_GUARD)
    h_desc[:C.sizeof(desc)] = np.frombuffer(desc, dtype=np.uint8)

    h_seqs = stream(seed * 7 + 3, seq_bytes + SEQ_GUARD_ENTRIES * 16)
    cnt_guard = max(SMALL_GUARD, 4 * nb)
    h_cnt = stream(seed * 7 + 4, 4 * nb + cnt_guard)
    if count_fill is not None:
        h_cnt[:4 * nb].view(np.uint32)[:] = count_fill
    work = L.qzstd_hip_workspace_bytes(level, nb, maxlen)
    assert work, "qzstd_hip_workspace_bytes(%#x, %d, %d) = 0" % (level, nb, maxlen)
    work_guard = L.qzstd_hip_workspace_bytes(level, 1, BLOCK_MAX)  # one whole block's region: scratch indexed by a real length reaches no farther
    h_work = stream(seed * 7 + 5, work + work_guard + work_room)
    if work_fill in ("zeros", "ff"):
        h_work[:work] = 0 if work_fill == "zeros" else 0xFF

    host = {"src": h_src, "desc": h_desc, "seqs": h_seqs, "counts": h_cnt, "work": h_work}
    dev = reuse if reuse is not None else DeviceBuffers(plug, device)

    def h2d(name, arr, at=0):
        plug.check(L.qzstd_hip_memcpy_h2d(device, None, dev.ptr[name] + at, arr.ctypes.data, arr.nbytes), "h2d " + name)

    def d2h(name, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        plug.check(L.qzstd_hip_memcpy_d2h(device, None, out.ctypes.data, dev.ptr[name], nbytes), "d2h " + name)
        plug.check(L.qzstd_hip_stream_sync(device, None), "sync")
        return out

    try:
        if reuse is None:
            for k, h in host.items():
                dev.alloc(k, h.nbytes)
                h2d(k, h)
            before = dict(host)
        else:
            # the earlier launch's scratch and results stay; everything else, and the guards right behind what THIS launch may use, are rewritten
            for k, h in host.items():
                assert dev.size[k] >= h.nbytes, "the kept %s buffer (%d bytes) is smaller than this launch needs (%d)" % (k, dev.size[k], h.nbytes)
            for k in ("src", "desc", "counts"):
                h2d(k, host[k])
            h2d("seqs", h_seqs[seq_bytes:], seq_bytes)
            h2d("work", h_work[work:], work)
            plug.check(L.qzstd_hip_stream_sync(device, None), "sync")
            before = dict(host)
            before["seqs"] = d2h("seqs", h_seqs.nbytes)
            before["work"] = d2h("work", h_work.nbytes)
        plug.check(L.qzstd_hip_stream_sync(device, None), "sync")
        plug.check(L.qzstd_hip_find_sequences(device, None, level, dev.ptr["src"], dev.ptr["desc"], nb, maxlen, dev.ptr["seqs"],
                                              dev.ptr["counts"], dev.ptr["work"], work), "qzstd_hip_find_sequences")
        plug.check(L.qzstd_hip_stream_sync(device, None), "sync")
        after = {k: d2h(k, h.nbytes) for k, h in host.items()}
    except Exception:
        if reuse is None:
            dev.free()
        raise
    if not keep:
        dev.free()
    return Readback(level=level, blocks=list(blocks), caps=list(caps), parse_from=list(parse_from) if parse_from else [0] * nb,
                    packed_tag=packed_tag & 0xFFF, entry=entry, mark=desc[0].mark if nb else 0, maxlen=maxlen, layout=layout,
                    regions=regions, seq_bytes=seq_bytes, src_bytes=src_bytes, desc_bytes=C.sizeof(desc), work_bytes=work,
                    before=before, after=after, dev=dev if keep else None)


# ---------------------------------------------------------------------------------------------------------------- the oracle's side
_memo: dict = {}


def oracle_find(oracle, level: int, block: bytes, parse_from: int, cap: int):
    """(count or B.SEQ_ERROR, the oracle's entries as an [n, 4] uint32 array) for exactly this capacity — no default put in the place of a
    capacity of 0 — memoised by (level, block, parse_from, cap).  The oracle writes into a region of `cap` entries with a guard behind
    it; that it left the guard alone is asserted here, every time."""
    key = (level, block, parse_from, cap)
    hit = _memo.get(key)
    if hit is None:
        guard = 64
        buf = stream(cap + 11, (cap + guard) * 16)
        fill = buf.copy()
        arr = (B.Sequence * (cap + guard)).from_buffer(buf)
        prof = oracle.profile(level, len(block))
        n = oracle.lib.qzo_find_sequences_from(C.byref(prof), block, len(block), parse_from, arr, cap)
        del arr
        assert np.array_equal(buf[cap * 16:], fill[cap * 16:]), "the oracle wrote behind a region of %d entries" % cap
        if cap == 0 or (n == B.SEQ_ERROR and cap < 2):
            assert np.array_equal(buf, fill), "the oracle wrote into a region of %d entries that it refuses" % cap
        hit = _memo[key] = (n, buf[:(0 if n == B.SEQ_ERROR else n) * 16].view(np.uint32).reshape(-1, 4).copy())
    return hit


def expected_entries(seqs: np.ndarray, mark: int, packed_tag: int) -> np.ndarray:
    """the bytes the launch must have written for the oracle's entries `seqs` ([n, 4] uint32)"""
    if packed_tag:
        v = seqs[:, 0].astype(np.uint64) | (seqs[:, 1].astype(np.uint64) << np.uint64(17)) | (seqs[:, 2].astype(np.uint64) << np.uint64(35)) \
            | (np.uint64(packed_tag) << np.uint64(52))
        return v.view(np.uint8)
    e = seqs.copy()
    e[:, 3] = mark
    return e.reshape(-1).view(np.uint8)


def _first_diff(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.nonzero(a != b)[0][0])


def check_footprint(rb: Readback, oracle, refused=()):
    """Every assertion of the module's header, on one read-back.  `refused`: blocks the launch must refuse whatever their capacity (a
    descriptor longer than the launch's maxBlockLen): NSEQ_ERROR, and their whole region still holds the fill."""
    nb = len(rb.blocks)
    seqs_b, seqs_a = rb.before["seqs"], rb.after["seqs"]
    counts = rb.counts()
    outside = np.ones(seqs_a.nbytes, dtype=bool)  # bytes no block may have touched
    for i, blk in enumerate(rb.blocks):
        off, length = rb.regions[i]
        cap = rb.caps[i]
        what = "block %d (level %#x, %d bytes from %d, seqCap %d, region at byte %d)" % (i, rb.level, len(blk), rb.parse_from[i], cap, off)
        if i in refused:
            assert counts[i] == B.NSEQ_ERROR, "%s: a refused block came back with count %d" % (what, counts[i])
            continue  # (its region stays in `outside`)
        want_n, want = oracle_find(oracle, rb.level, blk, rb.parse_from[i], cap)
        # ---- count
        assert counts[i] == (B.NSEQ_ERROR if want_n == B.SEQ_ERROR else want_n), "%s: count %d, oracle %d" % (
            what, counts[i], -1 if want_n == B.SEQ_ERROR else want_n)
        if want_n == B.SEQ_ERROR:
            outside[off:off + length] = False  # an error block: anything inside its own region, nothing anywhere else
            continue
        # ---- entries [0, count)
        used = want_n * rb.entry
        assert used <= length, "%s: the oracle's %d entries do not fit the region" % (what, want_n)
        exp = expected_entries(want, rb.mark, rb.packed_tag)
        got = seqs_a[off:off + used]
        if not np.array_equal(got, exp):
            k = _first_diff(got, exp) // rb.entry
            raise AssertionError("%s: entry %d of %d is %s, oracle (with the mark) %s" % (
                what, k, want_n, got[k * rb.entry:(k + 1) * rb.entry].tobytes().hex(), exp[k * rb.entry:(k + 1) * rb.entry].tobytes().hex()))
        # ---- the region behind entry `count`
        tail_a, tail_b = seqs_a[off + used:off + length], seqs_b[off + used:off + length]
        if not np.array_equal(tail_a, tail_b):
            d = _first_diff(tail_a, tail_b)
            raise AssertionError("%s: byte %d behind its %d entries (entry %d of the region) was written: %#04x, fill %#04x" % (
                what, d, want_n, want_n + d // rb.entry, tail_a[d], tail_b[d]))
        outside[off:off + length] = False
    # ---- gaps, refused regions, the guard behind the last region
    bad = outside & (seqs_a != seqs_b)
    if bad.any():
        d = int(np.nonzero(bad)[0][0])
        where = "the guard behind the last region (byte %d of it)" % (d - rb.seq_bytes) if d >= rb.seq_bytes else "a gap or a refused block's region"
        owner = [i for i in range(nb) if rb.regions[i][0] + rb.regions[i][1] <= d]
        near = max(owner, key=lambda i: rb.regions[i][0]) if owner else None
        raise AssertionError("level %#x: byte %d of the result buffer, outside every region (%s; the region before it is block %s's), was written: "
                             "%#04x, fill %#04x" % (rb.level, d, where, near, seqs_a[d], seqs_b[d]))
    # ---- counts' guard, source, descriptors, scratch guard
    for name, first, text in (("counts", 4 * nb, "the guard behind the count words"), ("src", 0, "the source or its guard"),
                              ("desc", 0, "the descriptors or their guard"), ("work", rb.work_bytes, "the guard behind the workspace")):
        a, b = rb.after[name][first:], rb.before[name][first:]
        if not np.array_equal(a, b):
            d = _first_diff(a, b)
            raise AssertionError("level %#x: %s changed at byte %d: %#04x, before the launch %#04x" % (rb.level, text, d, a[d], b[d]))


# ------------------------------------------------------------------------------------------------------------------ the case lists
OVERFLOW_CAPS = (100, 16, 4, 3, 2, 1, 0)
GENEROUS_ROOM = 16  # entries on top of ZSTD_sequenceBound: an empty block's single delimiter needs seqCap >= 3


def generous_cap(block_len: int, parse_from: int = 0) -> int:
    return B.sequence_bound(block_len - parse_from) + GENEROUS_ROOM


def capacity_cases(oracle, level: int, blocks: list[bytes], froms: list[int] | None = None):
    """The capacity rule's batch: every block once per seqCap in {n + 2, n + 1, n, n - 1, 100, 16, 4, 3, 2, 1, 0} (n = the oracle's count
    with room to spare), and after every third such item one with a generous capacity, whose result must be the oracle's although its
    neighbours overflow.  Returns (items, parse_from, caps, far): far = the largest n // seqCap over the items with 16 <= seqCap < n —
    how many times its capacity the farthest-overflowing block would write had it lost its guard."""
    froms = froms or [0] * len(blocks)
    items, pf, caps, far = [], [], [], 0
    for blk, f in zip(blocks, froms):
        room = generous_cap(len(blk), f)
        n, _ = oracle_find(oracle, level, blk, f, room)
        assert n != B.SEQ_ERROR and n + 2 <= room, "block of %d bytes from %d: oracle count %d with %d entries of room" % (len(blk), f, n, room)
        for k, cap in enumerate(dict.fromkeys([n + 2, n + 1, n, max(n - 1, 0)] + list(OVERFLOW_CAPS))):
            items.append(blk), pf.append(f), caps.append(cap)
            if 16 <= cap < n:
                far = max(far, n // cap)
            if k % 3 == 2:
                items.append(blk), pf.append(f), caps.append(room)
    return items, pf, caps, far
