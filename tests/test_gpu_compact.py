"""GPU: the compaction kernel (qzstd_hip_compact, include/qzstd_hip_device.h) against the plain statement of its contract in
tools/qz_compact_ref.py, on the generator's batches: every byte of the arena and of 4 KiB behind it, the workspace's canary, the inputs
left as they were.  Shapes where the kernel's loops turn: launches of more than one 512-block scan step, blocks of more than one
512-entry emit chunk, the arena's fit boundary next to a scan step, descriptors out of order, aliased and with gaps; and the refusals.

Every buffer is padded (tools/qz_compact_ref.make_batch) so that a kernel missing one of its checks would read garbage inside its
allocations, not past them; no count is above seqCap + 1 except QZSTD_HIP_NSEQ_ERROR."""
import ctypes as C

import numpy as np
import pytest

import qz_device as D  # noqa: F401  (imports torch first: one HIP runtime)
import qz_compact_ref as R

pytestmark = pytest.mark.gpu

SLACK = 4096


def canary(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


class Launch:
    """one batch on the device: source, descriptors, entries, counts, a canary-filled arena of arena_bytes + SLACK and workspace of
    qzstd_hip_compact_workspace_bytes(n) + SLACK"""

    def __init__(self, plug, batch: R.Batch, arena_bytes: int):
        L = self.L = plug.lib
        L.qzstd_hip_compact.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_size_t]
        L.qzstd_hip_compact_workspace_bytes.argtypes = [C.c_uint32]
        L.qzstd_hip_compact_workspace_bytes.restype = C.c_size_t
        self.plug, self.batch, self.arena_bytes = plug, batch, arena_bytes
        n = len(batch.blocks)
        self.work_bytes = L.qzstd_hip_compact_workspace_bytes(n)
        assert self.work_bytes == R.workspace_bytes(n)
        self.host = {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in (
            ("src", batch.src), ("blocks", batch.blocks), ("seqs", batch.seqs), ("counts", batch.counts),
            ("arena", canary(arena_bytes + SLACK, arena_bytes & 0xFFFF)), ("work", canary(self.work_bytes + SLACK, 7)))}
        self.dev = {}
        try:
            for k, h in self.host.items():
                p = L.qzstd_hip_malloc(0, h.nbytes)
                assert p, plug.err()
                self.dev[k] = p
                plug.check(L.qzstd_hip_memcpy_h2d(0, None, p, h.ctypes.data, h.nbytes), "h2d " + k)
            plug.check(L.qzstd_hip_stream_sync(0, None), "sync")
        except Exception:
            self.free()
            raise

    def run(self, n=None, arena_skew=0, work_skew=0, work_bytes=None, arena_bytes=None, null=()):
        d = {k: None if k in null else v for k, v in self.dev.items()}
        r = self.L.qzstd_hip_compact(0, None, d["src"], d["blocks"], len(self.batch.blocks) if n is None else n, d["seqs"], d["counts"],
                                     d["arena"] and d["arena"] + arena_skew, self.arena_bytes if arena_bytes is None else arena_bytes,
                                     d["work"] and d["work"] + work_skew, self.work_bytes if work_bytes is None else work_bytes)
        self.plug.check(self.L.qzstd_hip_stream_sync(0, None), "sync")
        return r

    def read(self, k: str) -> np.ndarray:
        out = np.empty(self.host[k].nbytes, dtype=np.uint8)
        self.plug.check(self.L.qzstd_hip_memcpy_d2h(0, None, out.ctypes.data, self.dev[k], out.nbytes), "d2h " + k)
        self.plug.check(self.L.qzstd_hip_stream_sync(0, None), "sync")
        return out

    def unchanged(self, *keys) -> bool:
        return all(np.array_equal(self.read(k), self.host[k]) for k in keys)

    def free(self):
        for p in self.dev.values():
            self.L.qzstd_hip_free(0, p)
        self.dev = {}


def compact_and_check(plug, batch: R.Batch, arena_bytes: int) -> np.ndarray:
    """the kernel on `batch` -> blocks kept; the whole allocation equals the reference over the canary, nothing else changed"""
    ln = Launch(plug, batch, arena_bytes)
    try:
        plug.check(ln.run(), "qzstd_hip_compact")
        got = ln.read("arena")
        want, used, kept = batch.reference(arena_bytes, ln.host["arena"])
        assert used <= arena_bytes
        bad = np.flatnonzero(got[:arena_bytes] != want)
        assert not len(bad), "arena differs from the contract at %d bytes, the first at %d (headers end %d, used %d of %d)" % (
            len(bad), bad[0], 8 * len(batch.blocks), used, arena_bytes)
        assert np.array_equal(got[arena_bytes:], ln.host["arena"][arena_bytes:]), "written past arenaBytes"
        work = ln.read("work")
        assert np.array_equal(work[ln.work_bytes:], ln.host["work"][ln.work_bytes:]), "written past the workspace"
        assert ln.unchanged("src", "blocks", "seqs", "counts"), "an input changed"
        return kept
    finally:
        ln.free()


@pytest.mark.parametrize("n", [1, 511, 512, 513, 1024, 1537, 4096])
def test_compact_block_counts(gpu_plugin, n):
    """one launch of n blocks: the scan carries its sums across 512-block steps"""
    rng = np.random.default_rng(n)
    batch = R.make_batch(rng, [int(x) for x in rng.integers(1, 2000, n)])
    assert compact_and_check(gpu_plugin, batch, batch.need() + 5).all()


@pytest.mark.parametrize("k,lit_max,zero", [(1, None, None), (511, None, None), (512, None, None), (513, 5, None), (1024, None, None),
                                             (1025, None, (512, 1024)), (4097, 5, None)])
def test_compact_entries_per_block(gpu_plugin, k, lit_max, zero):
    """a block of k entries between two ordinary ones: the emit kernel's 512-entry chunks and their carries; a chunk whose literal lengths
    are all 0; literal runs of 1-5 bytes at every alignment of the source and the destination"""
    rng = np.random.default_rng(k)
    batch = R.make_batch(rng, [3000, 131072, 777], entries=[70, k, 20], lit_max=lit_max, zero_lits=(1,) + zero if zero else None)
    assert compact_and_check(gpu_plugin, batch, batch.need()).all()


def test_compact_mutations(gpu_plugin):
    """one block per rejection rule, each at its boundary: accepted and rejected exactly as the contract says"""
    for seed in range(2):
        batch, where = R.mutation_batch(np.random.default_rng(200 + seed))
        kept = compact_and_check(gpu_plugin, batch, batch.need() + 1)
        for b, name in where.items():
            assert kept[b] == R.MUTATIONS[name], (name, b)


def test_compact_exact_fit(gpu_plugin):
    """an arena of exactly the needed size keeps every block; one byte less drops the last kept one and nothing else; a header-only
    arena keeps nothing"""
    rng = np.random.default_rng(31)
    batch = R.make_batch(rng, [int(x) for x in rng.integers(1, 3000, 700)], mutations={699: "count_zero"})
    need = batch.need()
    assert compact_and_check(gpu_plugin, batch, need)[:699].all()
    kept = compact_and_check(gpu_plugin, batch, need - 1)
    assert kept[:698].all() and not kept[698:].any()
    assert not compact_and_check(gpu_plugin, batch, R.entries_off(700)).any()


@pytest.mark.parametrize("first", [511, 512, 513])
def test_compact_first_block_that_does_not_fit(gpu_plugin, first):
    """the first block that does not fit next to a scan step; a failed block inside the dropped suffix"""
    rng = np.random.default_rng(first)
    batch = R.make_batch(rng, [int(x) for x in rng.integers(1, 1500, 1100)], mutations={first + 200: "count_error"})
    for arena in (batch.need(first), batch.need(first + 1) - 1):
        kept = compact_and_check(gpu_plugin, batch, arena)
        assert kept[:first].all() and not kept[first:].any()


@pytest.mark.parametrize("layout", ["shuffled", "gaps", "aliased"])
def test_compact_descriptor_layouts(gpu_plugin, layout):
    """srcOff / seqOff not in block order, gaps between the blocks' regions, two descriptors on the same source bytes"""
    rng = np.random.default_rng(len(layout))
    lens = [int(x) for x in rng.integers(1, 40000, 600)]
    alias = None
    if layout == "aliased":
        lens[5] = lens[400] = lens[3]
        alias = {5: 3, 400: 3}
    batch = R.make_batch(rng, lens, order="shuffled" if layout == "shuffled" else "block", gap=1000 if layout == "gaps" else 0,
                         alias=alias)
    assert compact_and_check(gpu_plugin, batch, batch.need() + 64).all()


def test_compact_refusals_write_nothing(gpu_plugin):
    """nBlocks 0 returns 0; a misaligned arena or workspace, a short workspace, an arena smaller than its headers and each null pointer
    are refused: the arena and the workspace keep their canaries"""
    batch = R.make_batch(np.random.default_rng(9), [1000, 2000, 3000])
    ln = Launch(gpu_plugin, batch, batch.need())
    try:
        assert ln.run(n=0) == 0
        assert ln.run(arena_skew=8) < 0
        assert ln.run(work_skew=4) < 0
        assert ln.run(work_bytes=ln.work_bytes - 1) < 0
        assert ln.run(arena_bytes=R.entries_off(3) - 1) < 0
        for k in ("src", "blocks", "seqs", "counts", "arena", "work"):
            assert ln.run(null=(k,)) < 0, k
        assert ln.unchanged("arena", "work", "src", "blocks", "seqs", "counts")
    finally:
        ln.free()
