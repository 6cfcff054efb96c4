"""GPU: the write footprint and the capacity rule of qzstd_hip_find_sequences on every emission path (tools/qz_footprint.py: guarded
launches, every buffer read back whole and compared with the oracle and with a seeded random fill, byte for byte).

The launch kernels parse after their tile loop and emit in the deferred plain parse (levels 1-4 and, on the chain levels' scratch
layout, levels 5-9) or in the deferred repeat-aware parse (levels 10-12 and every level | 0x100); the resident service's workers emit
window by window (emit_window) behind a parse wave that stores the delimiter.  Each has its own `idx < seqCap` guard, delimiter store
and capacity rule.  Which case overflows which guard far (n >= 8 x seqCap, asserted on the oracle's count):

    deferred plain parse      test_capacity_rule_whole_blocks[1 / 2 / 3]       128 KiB text, seqCap 16 (and 100, 4, 3, 2, 1, 0)
    ... at the chain levels   test_capacity_rule_whole_blocks[6 / 9]           the same block
    repeat-aware parse        test_capacity_rule_whole_blocks[12 / 0x101 / 0x106]
    emit_window + parse wave  test_service_items_keep_to_their_regions         4 KiB text items against seqCapPerItem 4

Every guard is long enough for a block that lost its bound to stay inside the test's allocations (qz_footprint.py)."""
import numpy as np
import pytest

import qz_bind as B
import qz_corpus as K
import qz_footprint as F

pytestmark = pytest.mark.gpu

LEVELS = [1, 2, 3, 6, 9, 12, 0x101, 0x106]
RAGGED = [0, 1, 5, 4095, 4097, 131071]  # from test_gpu_parity.test_edge_sizes


def whole_blocks(near: bool):
    text = K.text(3, 140000)
    if near:  # every block <= 32 KiB: the launch takes the NEAR kernels
        return [text[:32768], K.by_name("system", 32768), K.weblog(4, 32768), bytes(32768), K.incompressible(5, 32768), b"ab" * 16384] + \
               [text[:s] for s in RAGGED if s <= 32768]
    return [K.text(5, 131072), text[:32768], K.by_name("system", 32768), K.weblog(4, 32768), bytes(131072), K.incompressible(5, 131072),
            b"ab" * 65536] + [text[:s] for s in RAGGED]


def segment_items(near: bool):
    """(item, parseFrom): segments at the 4 KiB granularity of the service and at 32 KiB"""
    if near:
        text = K.text(6, 32768)
        return [(text[:s0 + 4096], s0) for s0 in (0, 4096, 28672)] + [(text[:20001], 16384), (bytes(32768), 28672)]
    text, web = K.text(6, 131072), K.weblog(7, 50001)
    return [(text[:s0 + 4096], s0) for s0 in (0, 4096, 61440, 126976)] + [(text[:s0 + 32768], s0) for s0 in (0, 32768, 98304)] + \
           [(web, 49152), (web[:36864], 32768), (bytes(131072), 98304), (b"ab" * 65536, 126976)]


@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("level", LEVELS)
def test_capacity_rule_whole_blocks(gpu_plugin, oracle, level, near):
    """every block with seqCap in {n + 2, n + 1, n, n - 1, 100, 16, 4, 3, 2, 1, 0} in ONE launch with exactly adjacent regions, blocks
    with generous capacities in between (their results are the oracle's although their neighbours overflow); 16-byte and packed
    entries; then the same batch with the regions shuffled and with gaps"""
    items, pf, caps, far = F.capacity_cases(oracle, level, whole_blocks(near))
    assert far >= 8, "level %#x: no block overflows its capacity far any more (n // seqCap = %d): the corpus changed" % (level, far)
    for tag, layout in ((0, "adjacent"), (0x7E5, "adjacent"), (0, "shuffled"), (0x001, "gaps")):
        F.check_footprint(F.launch(gpu_plugin, items, level, caps, parse_from=pf, packed_tag=tag, layout=layout, seed=level), oracle)


@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("level", LEVELS)
def test_capacity_rule_segment_items(gpu_plugin, oracle, level, near):
    """the same for segment items (parseFrom): the item inserts the block before its segment and emits the segment's sequences only"""
    segs = segment_items(near)
    items, pf, caps, far = F.capacity_cases(oracle, level, [s[0] for s in segs], [s[1] for s in segs])
    assert far >= 8, "level %#x: no item overflows its capacity far any more (n // seqCap = %d): the corpus changed" % (level, far)
    for tag in (0, 0xFFF):
        F.check_footprint(F.launch(gpu_plugin, items, level, caps, parse_from=pf, packed_tag=tag, seed=level + 50), oracle)


@pytest.mark.parametrize("level", [1, 3, 0x101, 6, 12])
def test_descriptor_longer_than_the_launch_says_keeps_to_its_footprint(gpu_plugin, oracle, level):
    """a launch that understates its longest block: the block that does not fit the launch's scratch regions (sized by maxBlockLen) is
    refused — at the chain levels too, whose chain entries would otherwise land in the neighbour's region — its result region and the
    scratch guard stay untouched, and the blocks that fit are the oracle's.  Once with blocks beyond the ring, once inside it (NEAR)"""
    for blocks, says in (([K.by_name("text", 70000, seed=3), K.by_name("system", 40000, seed=4), K.by_name("mix", 39999, seed=5)], 40000),
                         ([K.by_name("text", 30000, seed=3), K.by_name("weblog", 20000, seed=4), K.by_name("mix", 19999, seed=5)], 20000)):
        caps = [F.generous_cap(len(b)) for b in blocks]
        for tag in (0, 0x0F0):
            rb = F.launch(gpu_plugin, blocks, level, caps, launch_max_len=says, packed_tag=tag, seed=level + 70)
            F.check_footprint(rb, oracle, refused={0})


@pytest.mark.parametrize("level", [1, 3, 6, 12, 0x106])
def test_state_left_by_earlier_work_does_not_matter(gpu_plugin, oracle, level):
    """the same ragged batch (maxBlockLen no multiple of 512) with the scratch zeroed, all 0xFF, random, and as a launch at another
    level with a larger maxBlockLen left it and the result buffer (production scratch is grow-only and shared by the levels: level 1
    after a chain level, a chain level after level 1); and with the count words pre-filled.  No launch path of the plugin clears the
    count words (host/qatseqprod.c hands over a slot's dCount as the last launch left it, the front-end its grown dCount; announcements
    preset 0xFFFFFFFF): the loosest value a caller leaves there is anything, 0xFFFFFFFF among it."""
    text = K.text(7, 80000)
    sizes = [0, 1, 5, 4095, 4097, 10000, 32769, 50001, 65537, 70001]
    blocks = [text[:s] for s in sizes]
    caps = [F.generous_cap(100001)] * len(blocks)
    for fill in ("zeros", "ff", "random"):
        F.check_footprint(F.launch(gpu_plugin, blocks, level, caps, work_fill=fill, seed=level + 90), oracle)
    F.check_footprint(F.launch(gpu_plugin, blocks, level, caps, count_fill=0xFFFFFFFF, seed=level + 91), oracle)
    chain = gpu_plugin.profile(level, 131072).chainDepth != 0
    other = 1 if chain else 6
    web = K.weblog(3, 100001)
    big = [web[:s + 30000] for s in sizes]
    L = gpu_plugin.lib
    room = L.qzstd_hip_workspace_bytes(level, len(blocks), 70001) + L.qzstd_hip_workspace_bytes(level, 1, F.BLOCK_MAX)
    first = F.launch(gpu_plugin, big, other, caps, keep=True, work_room=room, seed=level + 92)
    try:
        F.check_footprint(first, oracle)
        F.check_footprint(F.launch(gpu_plugin, blocks, level, caps, work_fill="keep", reuse=first.dev, seed=level + 93), oracle)
    finally:
        first.dev.free()


# ---------------------------------------------------------------------------------------------------------------- the resident service
def run_filled(lane, blk, level, seed, seq_cap=None):
    """one request through a ServiceLane whose whole result area was pre-filled from the seeded stream -> (counts, cap, item bytes,
    the area before, the area after)"""
    import ctypes as C
    nbytes = lane.MAX_ITEMS * lane.ITEM_CAP * 16
    fill = F.stream(seed, nbytes)
    C.memmove(lane.hseq, fill.ctypes.data, nbytes)
    r = lane.run(blk, level, 4096, seq_cap=seq_cap)
    assert r is not None, "not served"
    counts, _, cap, item = r
    after = np.frombuffer((C.c_uint8 * nbytes).from_address(lane.hseq), dtype=np.uint8).copy()
    return counts, cap, item, fill, after


def check_service_area(oracle, lane, blk, level, counts, cap, item, fill, after):
    errors = 0
    for k, got_n in enumerate(counts):
        upto = min(len(blk), (k + 1) * item)
        want_n, want = F.oracle_find(oracle, level, blk[:upto], k * item, cap)
        assert got_n == (B.NSEQ_ERROR if want_n == B.SEQ_ERROR else want_n), "item %d: count %d, oracle %d" % (k, got_n, want_n)
        lo, hi = k * cap * 16, (k + 1) * cap * 16
        if want_n == B.SEQ_ERROR:
            errors += 1
            continue  # (it may have written inside its own region)
        exp = F.expected_entries(want, lane.epoch, 0)
        assert np.array_equal(after[lo:lo + want_n * 16], exp), "item %d: entries differ from the oracle's (with the epoch)" % k
        assert np.array_equal(after[lo + want_n * 16:hi], fill[lo + want_n * 16:hi]), "item %d wrote behind its %d entries" % (k, want_n)
    tail = len(counts) * cap * 16
    assert np.array_equal(after[tail:], fill[tail:]), "the result area behind the last item's region was written"
    return errors


@pytest.mark.parametrize("level", [1, 6, 12])
def test_service_items_keep_to_their_regions(gpu_plugin, oracle, level):
    """the resident service (emit_window behind the parse wave): a block in 4 KiB items into a result area pre-filled with the seeded
    stream — per item nothing behind its count, nothing behind the last item's region; then with seqCapPerItem reduced to 64 and to 4
    (the least the C ABI takes), which the text items exceed (far: a 4 KiB text item has more than 8 x 4 sequences, asserted) and the
    incompressible and zero items do not: those report NSEQ_ERROR, the others equal the oracle, nobody writes outside its region"""
    lane = gpu_plugin.service_lane(slot=11)
    try:
        blk = K.text(8, 65536) + K.incompressible(4, 32768) + bytes(32768)
        counts, cap, item, fill, after = run_filled(lane, blk, level, 31)
        assert check_service_area(oracle, lane, blk, level, counts, cap, item, fill, after) == 0
        assert max(counts) >= 8 * 4, "no item has 8 x 4 sequences any more: the corpus changed"
        for seq_cap in (64, 4):
            counts, cap, item, fill, after = run_filled(lane, blk, level, 32 + seq_cap, seq_cap=seq_cap)
            assert cap == seq_cap
            errors = check_service_area(oracle, lane, blk, level, counts, cap, item, fill, after)
            assert 0 < errors < len(counts), "seqCapPerItem %d: %d of %d items overflow" % (seq_cap, errors, len(counts))
        assert gpu_plugin.lib.qzstd_hip_service_stop(0) == 0
    finally:
        lane.close()
