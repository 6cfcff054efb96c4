"""GPU: the edge inputs of tools/qz_edges.py through every kernel family — boundary sizes, planted rules, blocks whose neighbour in the
source buffer continues their last match — bit-exact against the CPU oracle: as a launch of blocks that all fit the LDS ring (the NEAR
kernels), as a launch that does not, with packed entries, as work items that parse from a segment start, and through the resident
service.  tests/test_oracle_spec_python.py pins the oracle on the same inputs and shows which rule each of them exercises."""
import numpy as np
import pytest

import qz_bind as B
import qz_edges as E
import test_oracle_spec_python as S
from test_gpu_parity import check_blocks, seqs_to_np
from test_gpu_service import check_request

pytestmark = pytest.mark.gpu

LEVELS = [1, 2, 3, 5, 6, 9, 10, 12, 0x101, 0x102, 0x103, 0x105, 0x106]  # test_gpu_parity.test_levels' list: every kernel family
PACKED_LEVELS = [1, 3, 6, 12, 0x101]
SERVICE_LEVELS = [1, 2, 3, 6, 12, 0x101]
RING = E.kernel_constants()["kRing"]  # a launch whose blocks are all at most this long runs the NEAR kernels


def both_launch_forms(gpu_plugin, oracle, blocks, level, packed_tag=0):
    check_blocks(gpu_plugin, oracle, [b for b in blocks if len(b) <= RING], level, packed_tag)  # maxBlockLen <= the ring: NEAR
    assert max(len(b) for b in blocks) > RING
    check_blocks(gpu_plugin, oracle, blocks, level, packed_tag)                                  # all in one launch: not NEAR


def planted_and_neighbours(pf):
    """the neighbours first and in order: find_batch packs the blocks one behind the other (their lengths are multiples of 16)"""
    return [blk for _, blk in E.neighbours() + E.planted(pf)]


@pytest.mark.parametrize("level", LEVELS)
def test_boundary_sizes(gpu_plugin, oracle, level):
    both_launch_forms(gpu_plugin, oracle, [blk for _, blk in E.edge_blocks(oracle.profile(level, 0))], level)


@pytest.mark.parametrize("level", PACKED_LEVELS)
def test_boundary_sizes_with_packed_entries(gpu_plugin, oracle, level):
    both_launch_forms(gpu_plugin, oracle, [blk for _, blk in E.edge_blocks(oracle.profile(level, 0))], level, packed_tag=0x5A5 if level != 3 else 1)


@pytest.mark.parametrize("level", LEVELS)
def test_planted_rules_and_neighbours(gpu_plugin, oracle, level):
    both_launch_forms(gpu_plugin, oracle, planted_and_neighbours(oracle.profile(level, 0)), level)


@pytest.mark.parametrize("level", LEVELS)
def test_planted_rules_as_segment_work_items(gpu_plugin, oracle, level):
    """every planted block that spans several segments, as items that hold the block up to a segment's end and parse from that segment's start"""
    pf = oracle.profile(level, 0)
    seg = 1 << pf.segLog
    items, froms = [], []
    for _, blk in E.planted(pf):
        for s0 in range(seg, len(blk), seg):
            items.append(blk[:min(len(blk), s0 + seg)])
            froms.append(s0)
    counts, seqs, stride = gpu_plugin.find_batch(items, level, parse_from=froms)
    for i, (blk, s0) in enumerate(zip(items, froms)):
        want_n, want = oracle.find(pf, blk, cap=stride, parse_from=s0)
        assert counts[i] == want_n, "item %d (len %d from %d): %d sequences, oracle %d" % (i, len(blk), s0, counts[i], want_n)
        assert np.array_equal(seqs_to_np(seqs, i * stride, want_n), seqs_to_np(want, 0, want_n)), "item %d (len %d from %d) differs" % (i, len(blk), s0)


@pytest.mark.parametrize("level", SERVICE_LEVELS)
def test_edges_through_the_resident_service(gpu_plugin, oracle, level):
    """the service's in-loop parse (other code than the launch kernels' deferred parse): boundary sizes up to nine segments and the planted
    blocks, as 4 KiB items, every item against qzo_find_sequences_from"""
    pf = oracle.profile(level, 0)
    gpu_plugin.lib.qzstd_hip_service_stop(0)  # (workers of another level that an earlier test left resident)
    lane = gpu_plugin.service_lane(slot=13)
    try:
        for _, blk in E.edge_blocks(pf, RING + (1 << pf.segLog) + 8) + E.planted(pf):
            if len(blk):
                check_request(oracle, lane, blk, level)
        assert gpu_plugin.lib.qzstd_hip_service_stop(0) == 0
    finally:
        lane.close()


SPEC_BLOCKS = {1: ("lazy_by_length", "near_table_tie", "cap_len_decides", "start_at_block_end", "back_ext_stopped_by_anchor"),
               2: ("earlier_sub_tile", "cap_len_decides_with_sub_tiles", "lazy_by_length", "repeat_lengths", "fifth_byte_differs"),
               3: ("second_table_tie", "lazy_by_length", "cap_len", "near_table_tie", "min_len_around_far1"),
               4: ("second_table_tie", "earlier_sub_tile", "cap_len_decides", "back_ext_source_at_0", "start_at_block_end")}


@pytest.mark.parametrize("level", sorted(SPEC_BLOCKS))
def test_kernel_equals_the_python_specification(gpu_plugin, oracle, level):
    """levels 1-4, a handful of small planted blocks: the kernel's sequences against the pure-Python specification directly"""
    pf = oracle.profile(level, 0)
    planted = dict(E.planted(pf))
    blocks = [planted[name] for name in SPEC_BLOCKS[level]]
    counts, seqs, stride = gpu_plugin.find_batch(blocks, level)
    for i, (name, blk) in enumerate(zip(SPEC_BLOCKS[level], blocks)):
        want = S.specification(pf, blk)
        got = [tuple(int(x) for x in row) for row in seqs_to_np(seqs, i * stride, counts[i] if counts[i] != B.NSEQ_ERROR else 0)]
        assert got == want, "level %d, %s: %s" % (level, name, S.first_difference(got, want, "kernel"))
