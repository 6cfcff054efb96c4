"""CPU: the guarded launch and its checker (tools/qz_footprint.py) over the mock device layer — which pins the write footprint of the
oracle and of the mock themselves —, the checker's self-test (a byte altered in every class of location must be noticed), and the
capacity rule at its lower edge: a region of 0, 1, 2 or 3 entries."""
import os

import numpy as np
import pytest

import qz_bind as B
import qz_corpus as K
import qz_footprint as F
from test_host_mock import build_shared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK_SO = os.path.join(ROOT, "tests", "mock", "libqatseqprod_footmock.so")

# one level per parse function of the oracle: table candidates + plain parse, chain candidates + plain parse, table candidates +
# repeat-aware parse, chain candidates + repeat-aware parse
PARSE_LEVELS = [1, 6, 0x101, 12]


@pytest.fixture(scope="module")
def mock(oracle):
    srcs = [os.path.join(B.PKG_DIR, "host", "qatseqprod.c"), os.path.join(B.PKG_DIR, "csrc", "qzstd_profile.c"),
            os.path.join(ROOT, "tests", "mock", "mock_hip.c"), os.path.join(ROOT, "oracle", "qzstd_oracle.c")]
    build_shared(["gcc", "-O2", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-DQZ_TEST_HOOKS", "-shared", "-fPIC", "-pthread",
                  "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"), "-o", MOCK_SO] + srcs, MOCK_SO)
    return B.Plugin(MOCK_SO)


def small_blocks():
    text = K.text(3, 40000)
    return [text[:32768], bytes(32768), K.incompressible(2, 4096), b"ab" * 8192, text[:0], text[:1], text[:5], text[:4095], text[:4097]]


@pytest.mark.parametrize("packed_tag", [0, 0x5A5])
@pytest.mark.parametrize("level", [1, 3, 6, 12, 0x101])
def test_mock_footprint_capacity_rule(mock, oracle, level, packed_tag):
    """every block with seqCap in {n + 2, n + 1, n, n - 1, 100, 16, 4, 3, 2, 1, 0}, regions exactly adjacent, generous neighbours in
    between: counts and entries are the oracle's, nothing else is written"""
    items, pf, caps, far = F.capacity_cases(oracle, level, small_blocks())
    assert far >= 8, "no block overflows its capacity far (n // seqCap = %d)" % far
    for layout in ("adjacent", "gaps", "shuffled"):
        rb = F.launch(mock, items, level, caps, parse_from=pf, packed_tag=packed_tag, layout=layout, seed=level + 3)
        F.check_footprint(rb, oracle)


@pytest.mark.parametrize("level", [1, 6, 12])
def test_mock_footprint_segment_items(mock, oracle, level):
    """segment items (parseFrom) at 4 KiB and 32 KiB granularity, odd and even packed capacities"""
    text = K.text(5, 65536)
    blocks = [text[:4096], text[:8192], text[:32768], text[:65536], text[:40001]]
    froms = [0, 4096, 28672, 32768, 36864]
    items, pf, caps, _ = F.capacity_cases(oracle, level, blocks, froms)
    for tag in (0, 0xABC):
        F.check_footprint(F.launch(mock, items, level, caps, parse_from=pf, packed_tag=tag, seed=9), oracle)


@pytest.mark.parametrize("level,other", [(1, 6), (6, 1)])
def test_mock_footprint_state_left_by_earlier_work(mock, oracle, level, other):
    """the same ragged batch with the scratch zeroed, 0xFF, random, and as an earlier launch at another level left it; counts pre-filled"""
    text = K.text(7, 50000)
    sizes = [0, 1, 5, 4095, 4097, 10000, 20001]
    blocks = [text[:s] for s in sizes]
    caps = [F.generous_cap(30001)] * len(blocks)
    for fill in ("zeros", "ff", "random"):
        F.check_footprint(F.launch(mock, blocks, level, caps, work_fill=fill, seed=11), oracle)
    F.check_footprint(F.launch(mock, blocks, level, caps, count_fill=0xFFFFFFFF, seed=12), oracle)
    big = [K.weblog(3, 30001)[:s + 10000] for s in sizes]
    room = mock.lib.qzstd_hip_workspace_bytes(level, len(blocks), 20001) + mock.lib.qzstd_hip_workspace_bytes(level, 1, F.BLOCK_MAX)
    first = F.launch(mock, big, other, caps, keep=True, work_room=room, seed=13)
    try:
        F.check_footprint(first, oracle)
        F.check_footprint(F.launch(mock, blocks, level, caps, work_fill="keep", reuse=first.dev, seed=14), oracle)
    finally:
        first.dev.free()


# ------------------------------------------------------------------------------------------------------------- the checker's self-test
@pytest.fixture(scope="module")
def passing(mock, oracle):
    text = K.text(3, 20000)
    blocks = [text[:8192], K.incompressible(1, 4096), text[:8192], text[:4097], text[:8192]]
    n = F.oracle_find(oracle, 1, blocks[0], 0, F.generous_cap(8192))[0]
    caps = [n + 40, 16, 10, F.generous_cap(4097), n + 2]  # valid with room behind it, valid, overflowing, valid, valid and nearly full
    rb = F.launch(mock, blocks, 1, caps, layout="gaps", seed=5)
    F.check_footprint(rb, oracle)
    assert [c != B.NSEQ_ERROR for c in rb.counts()] == [True, True, False, True, True]
    return rb


def _altered(rb, name, at):
    after = dict(rb.after)
    after[name] = rb.after[name].copy()
    after[name][at] ^= 0x01
    d = dict(rb.__dict__)
    d["after"] = after
    return F.Readback(**d)


def _locations(rb):
    """(class of location, buffer, byte, what the checker must say) — one altered byte each"""
    nb = len(rb.blocks)
    off0, len0 = rb.regions[0]
    n0 = int(rb.counts()[0])
    order = sorted(range(nb), key=lambda i: rb.regions[i][0])
    first, second = order[0], order[1]
    gap_at = rb.regions[first][0] + rb.regions[first][1]
    assert gap_at < rb.regions[second][0], "the layout has no gap behind its first region"
    return [
        ("an entry inside [0, count)", "seqs", off0 + 16 * (n0 // 2) + 5, r"entry \d+ of \d+ is"),
        ("the mark word of an entry", "seqs", off0 + 16 * (n0 - 1) + 12, r"entry \d+ of \d+ is"),
        ("the first byte behind count", "seqs", off0 + 16 * n0, "behind its"),
        ("the last byte of a region", "seqs", off0 + len0 - 1, "behind its"),
        ("a gap", "seqs", gap_at, "outside every region"),
        ("a byte in front of an overflowing block's region", "seqs", rb.regions[2][0] - 1, "outside every region"),
        ("the first byte of the guard behind the results", "seqs", rb.seq_bytes, "the guard behind the last region"),
        ("the last byte of the guard behind the results", "seqs", rb.after["seqs"].nbytes - 1, "the guard behind the last region"),
        ("a neighbour's count word", "counts", 4 * 3 + 1, r"block 3 .*: count"),
        ("an error block's count word", "counts", 4 * 2, r"block 2 .*: count"),
        ("the count guard", "counts", 4 * nb, "the guard behind the count words"),
        ("a source byte", "src", 100, "the source"),
        ("a descriptor byte", "desc", 32 + 20, "the descriptors"),
        ("the first byte behind the workspace", "work", rb.work_bytes, "the guard behind the workspace"),
        ("the last byte of the workspace guard", "work", rb.after["work"].nbytes - 1, "the guard behind the workspace"),
    ]


def test_checker_notices_one_altered_byte_in_every_class_of_location(passing, oracle):
    for what, name, at, says in _locations(passing):
        with pytest.raises(AssertionError, match=says):
            F.check_footprint(_altered(passing, name, at), oracle)
        # ... and says so for that reason alone: the same byte altered in the `before` image as well is no difference
    F.check_footprint(passing, oracle)


def test_checker_leaves_the_scratch_itself_free(passing, oracle):
    """the scratch is the launch's to use: a byte inside it may change"""
    F.check_footprint(_altered(passing, "work", 0), oracle)


def test_checker_compares_packed_tags(mock, oracle):
    blocks = [K.text(3, 8192)]
    rb = F.launch(mock, blocks, 1, [F.generous_cap(8192)], packed_tag=0x123, seed=2)
    F.check_footprint(rb, oracle)
    with pytest.raises(AssertionError, match=r"entry 0 of \d+ is"):
        F.check_footprint(_altered(rb, "seqs", 7), oracle)  # the top byte of the first packed entry: its tag


def test_checker_holds_a_refused_block_to_an_untouched_region(mock, oracle):
    """`refused` blocks must come back as NSEQ_ERROR with their region as it was: the mock parses them, the checker says so"""
    blocks = [K.text(3, 8192), K.text(4, 4096)]
    rb = F.launch(mock, blocks, 1, [F.generous_cap(8192)] * 2, seed=2)
    F.check_footprint(rb, oracle)
    with pytest.raises(AssertionError, match="refused"):
        F.check_footprint(rb, oracle, refused={0})


# -------------------------------------------------------------------------------------------------------------------- capacity edges
def edge_blocks():
    return [("matches", K.text(9, 32768)), ("incompressible", K.incompressible(9, 32768))]


@pytest.mark.parametrize("level", PARSE_LEVELS)
def test_oracle_capacity_edges(oracle, level):
    """seqCap 0, 1, 2, 3: the count is an error exactly when n >= seqCap - 1 (reference src/qatseqprod.c:1318), computed without the
    subtraction that wraps at 0; nothing is written outside the region, and nothing at all into a region of 0 or 1 entries (asserted
    inside oracle_find).  A block with matches is an error at all four; an incompressible block (n = 1: its delimiter) fits 3 entries."""
    for name, blk in edge_blocks():
        n_full = F.oracle_find(oracle, level, blk, 0, F.generous_cap(len(blk)))[0]
        assert n_full != B.SEQ_ERROR and (n_full > 8 if name == "matches" else n_full == 1)
        for cap in (0, 1, 2, 3):
            n, _ = F.oracle_find(oracle, level, blk, 0, cap)
            want = B.SEQ_ERROR if n_full + 1 >= cap else n_full
            assert n == want, "level %#x, %s, seqCap %d: %d" % (level, name, cap, n)
        assert F.oracle_find(oracle, level, blk, 0, 0)[0] == B.SEQ_ERROR and F.oracle_find(oracle, level, blk, 0, 1)[0] == B.SEQ_ERROR
    assert oracle.find(oracle.profile(level, 32768), edge_blocks()[0][1], cap=0)[0] == B.SEQ_ERROR  # (cap=0 is 0, not the default)


@pytest.mark.parametrize("packed_tag", [0, 1])
@pytest.mark.parametrize("level", PARSE_LEVELS)
def test_mock_capacity_edges(mock, oracle, level, packed_tag):
    blocks, caps = [], []
    for _, blk in edge_blocks():
        for cap in (0, 1, 2, 3, F.generous_cap(len(blk))):
            blocks.append(blk), caps.append(cap)
    rb = F.launch(mock, blocks, level, caps, packed_tag=packed_tag, seed=21)
    F.check_footprint(rb, oracle)
    counts = rb.counts()
    assert all(counts[i] == B.NSEQ_ERROR for i in (0, 1, 2, 3, 5, 6, 7)) and counts[8] == 1 and counts[4] > 8 and counts[9] == 1
    for i in (0, 1, 5, 6):  # a region of 0 or 1 entries: nothing written at all
        off, length = rb.regions[i]
        assert np.array_equal(rb.after["seqs"][off:off + length], rb.before["seqs"][off:off + length])
