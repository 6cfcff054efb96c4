"""A plain numpy statement of the compaction contract (include/qzstd_hip_device.h, qzstd_hip_compact) and a generator of batches to
check an implementation of it against: the HIP kernel (tests/test_gpu_compact.py) and the CPU mock (tests/test_device_input_mock.py).

compact() returns the whole arena the contract requires, every byte of it: what the call must write (headers, packed entries, literal
bytes) over `base`, the bytes the arena held before the call, which must stay as they were everywhere else — the padding between the
headers and the entries and everything past the last literal byte included.

make_batch() draws valid random parses of random blocks and applies named mutations, one per rejection rule, each at its boundary
(MUTATIONS: name -> whether the block is still accepted).  Every buffer it returns is padded so that an implementation missing one of
its checks reads bytes inside the buffer: the source 256 KiB past the last block, the entries seqCap + 1 past the last region."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NSEQ_ERROR = 0xFFFFFFFF
MARK_COMPACT = 0x80000000
LIMIT = 1 << 17  # offset < LIMIT, litLength <= LIMIT, matchLength < LIMIT: what QZSTD_HIP_PACK holds
SRC_PAD = 256 << 10

# qzstd_hip_block_t (tools/qz_bind.HipBlock), as a numpy record
BLOCK_DTYPE = np.dtype([("srcOff", "<u8"), ("seqOff", "<u8"), ("srcLen", "<u4"), ("seqCap", "<u4"), ("parseFrom", "<u4"),
                        ("mark", "<u4")])


def entries_off(n: int) -> int:
    """QZSTD_HIP_COMPACT_ENTRIES_OFF"""
    return (8 * n + 15) & ~15


def workspace_bytes(n: int) -> int:
    """qzstd_hip_compact_workspace_bytes"""
    return 16 * n + 16


def pack(q: np.ndarray) -> np.ndarray:
    """QZSTD_HIP_PACK(off, lit, ml, 0) of (k, >= 3) entries"""
    q = q.astype(np.uint64)
    return q[:, 0] | (q[:, 1] << np.uint64(17)) | (q[:, 2] << np.uint64(35))


def block_ok(src_len: int, seq_cap: int, mark: int, count: int, seqs: np.ndarray, seq_off: int) -> bool:
    """the per-block rules: the count, the mark, the packed fields, the delimiter, the coverage"""
    if count == NSEQ_ERROR or count == 0 or count > seq_cap or mark & MARK_COMPACT:
        return False
    q = seqs[seq_off:seq_off + count].astype(np.int64)
    if (q[:, 0] >= LIMIT).any() or (q[:, 1] > LIMIT).any() or (q[:, 2] >= LIMIT).any():
        return False
    if q[-1, 0] != 0 or q[-1, 2] != 0:
        return False
    return int(q[:, 1].sum() + q[:, 2].sum()) == src_len


def accounting(blocks: np.ndarray, seqs: np.ndarray, counts: np.ndarray):
    """-> (ok, entries, literal bytes) per block, before the arena's capacity is applied"""
    ok = np.array([block_ok(int(b["srcLen"]), int(b["seqCap"]), int(b["mark"]), int(c), seqs, int(b["seqOff"]))
                   for b, c in zip(blocks, counts)], dtype=bool)
    cnt = np.array([int(c) if k else 0 for c, k in zip(counts, ok)], dtype=np.int64)
    lit = np.array([int(seqs[int(b["seqOff"]):int(b["seqOff"]) + int(c), 1].astype(np.int64).sum()) if k else 0
                    for b, c, k in zip(blocks, counts, ok)], dtype=np.int64)
    return ok, cnt, lit


def compact(src: np.ndarray, blocks: np.ndarray, seqs: np.ndarray, counts: np.ndarray, arena_bytes: int, base: np.ndarray):
    """-> (arena: uint8[arena_bytes], used: the end of the last literal byte, kept: bool per block).  blocks: BLOCK_DTYPE records;
    seqs: (N, 4) uint32 ZSTD_Sequence entries; counts: uint32 per block; base: the arena's bytes before the call"""
    n = len(blocks)
    eo = entries_off(n)
    assert arena_bytes >= eo and len(base) >= arena_bytes
    ok, cnt, lit = accounting(blocks, seqs, counts)
    # the blocks that do not fit are a suffix: from the first one whose end (entries and literals of all blocks so far) passes the arena
    kept = ok & (np.cumsum(8 * cnt + lit) <= arena_bytes - eo)
    cnt, lit = np.where(kept, cnt, 0), np.where(kept, lit, 0)
    arena = np.array(base[:arena_bytes], dtype=np.uint8)
    hdr = np.empty((n, 2), dtype=np.uint32)
    hdr[:, 0] = np.where(kept, cnt, NSEQ_ERROR)
    hdr[:, 1] = lit
    arena[:8 * n] = hdr.reshape(-1).view(np.uint8)
    n_seq, n_lit = int(cnt.sum()), int(lit.sum())
    ent = arena[eo:eo + 8 * n_seq].view(np.uint64)
    lits = arena[eo + 8 * n_seq:eo + 8 * n_seq + n_lit]
    e = d = 0
    for i, b in enumerate(blocks):
        if not kept[i]:
            continue
        q = seqs[int(b["seqOff"]):int(b["seqOff"]) + int(cnt[i])].astype(np.int64)
        ent[e:e + len(q)] = pack(q)
        e += len(q)
        ll, run = q[:, 1], q[:, 1] + q[:, 2]
        start = np.cumsum(run) - run  # each entry's first byte in the block
        idx = np.repeat(start - (np.cumsum(ll) - ll), ll) + np.arange(int(ll.sum()))
        lits[d:d + len(idx)] = src[int(b["srcOff"]) + idx]
        d += len(idx)
    return arena, eo + 8 * n_seq + n_lit, kept


# ---------------------------------------------------------------------------------------------------------------- the generator
# name -> accepted: each mutation puts one field of one block at the boundary of its rule
MUTATIONS = {
    "offset_max": True,         # a match offset of 2^17 - 1
    "offset_over": False,       # 2^17
    "literals_max": True,       # a 128 KiB all-literal block: litLength 2^17
    "literals_over": False,     # srcLen 131 073, one run of 2^17 + 1 literals
    "match_max": True,          # matchLength 2^17 - 1
    "match_over": False,        # matchLength 2^17
    "last_offset": False,       # the last entry has an offset
    "last_match": False,        # the last entry has a match length
    "cover_short": False,       # the entries cover srcLen - 1
    "cover_long": False,        # srcLen + 1
    "count_cap": True,          # count = seqCap
    "count_zero": False,        # 0
    "count_over": False,        # seqCap + 1
    "count_error": False,       # QZSTD_HIP_NSEQ_ERROR, as the matcher writes it
    "mark_compact": False,      # QZSTD_HIP_MARK_COMPACT set
    "mark_epoch": True,         # other bits of the mark set (the service's epoch): no effect
}


def _split(rng: np.random.Generator, total: int, m: int) -> np.ndarray:
    """m + 1 non-negative parts that sum to total"""
    return np.diff(np.concatenate([[0], np.sort(rng.integers(0, total + 1, m)), [total]]))


def random_parse(rng: np.random.Generator, src_len: int, k: int, lit_max: int | None = None) -> np.ndarray:
    """k entries (offset, litLength, matchLength, 0) that cover src_len bytes exactly, the last one a delimiter (offset 0, matchLength
    0).  lit_max: every literal run but the delimiter's is 1 .. lit_max bytes (needs src_len >= (k - 1) * lit_max)"""
    q = np.zeros((k, 4), dtype=np.uint32)
    if k > 1:
        if lit_max:
            ll = rng.integers(1, lit_max + 1, k - 1)
            ml = _split(rng, src_len - int(ll.sum()), k - 1)[:-1]
        else:
            parts = _split(rng, src_len, 2 * k - 2)
            ll, ml = parts[0:-1:2], parts[1::2]
        q[:-1, 0] = rng.integers(1, LIMIT, k - 1)
        q[:-1, 1], q[:-1, 2] = ll, np.minimum(ml, LIMIT - 1)
    q[-1, 1] = src_len - int(q[:-1, 1].astype(np.int64).sum() + q[:-1, 2].astype(np.int64).sum())
    assert 0 <= int(q[-1, 1]) <= LIMIT
    return q


def mutate(rng: np.random.Generator, name: str, src_len: int, q: np.ndarray, seq_cap: int):
    """-> (srcLen, entries, count, seqCap, mark) of a block after mutation `name`"""
    count, mark = len(q), 0
    if name in ("offset_max", "offset_over"):
        src_len = max(src_len, 64)
        q = random_parse(rng, src_len, max(len(q), 2))
        q[0, 0] = LIMIT - 1 if name == "offset_max" else LIMIT
        count = len(q)
    elif name in ("literals_max", "literals_over"):
        src_len = LIMIT if name == "literals_max" else LIMIT + 1
        q = np.array([[0, src_len, 0, 0]], dtype=np.uint32)
        count = 1
    elif name in ("match_max", "match_over"):
        ml = LIMIT - 1 if name == "match_max" else LIMIT
        src_len = LIMIT
        q = np.array([[1, 0, ml, 0], [0, LIMIT - ml, 0, 0]], dtype=np.uint32)
        count = 2
    elif name in ("last_offset", "last_match", "cover_short", "cover_long"):
        q = q.copy()
        if int(q[-1, 1]) == 0:  # give the delimiter a literal byte to trade
            src_len += 1
            q[-1, 1] = 1
        if name == "last_offset":
            q[-1, 0] = 1
        elif name == "last_match":
            q[-1, 1] -= 1
            q[-1, 2] = 1
        else:
            q[-1, 1] = int(q[-1, 1]) + (1 if name == "cover_long" else -1)
    elif name == "count_cap":
        seq_cap = count
    elif name == "count_zero":
        count = 0
    elif name == "count_over":
        if count == 1:
            q = random_parse(rng, src_len, 2)
        seq_cap = len(q) - 1
        count = len(q)
    elif name == "count_error":
        count = NSEQ_ERROR
    elif name == "mark_compact":
        mark = MARK_COMPACT
    elif name == "mark_epoch":
        mark = 0x00ABCDEF
    else:
        raise KeyError(name)
    if name != "count_over":
        seq_cap = max(seq_cap, len(q))
    return src_len, q, count, seq_cap, mark


@dataclass
class Batch:
    src: np.ndarray      # uint8: the launch's source, padded
    blocks: np.ndarray   # BLOCK_DTYPE
    seqs: np.ndarray     # (N, 4) uint32, padded
    counts: np.ndarray   # uint32

    def need(self, upto: int | None = None) -> int:
        """arena bytes that hold every accepted block of blocks [0, upto), headers included"""
        _, cnt, lit = accounting(self.blocks[:upto], self.seqs, self.counts[:upto])
        return entries_off(len(self.blocks)) + int((8 * cnt + lit).sum())

    def reference(self, arena_bytes: int, base: np.ndarray):
        return compact(self.src, self.blocks, self.seqs, self.counts, arena_bytes, base)


def make_batch(rng: np.random.Generator, lens, entries=None, mutations: dict | None = None, order: str = "block", gap: int = 0,
               alias: dict | None = None, lit_max: int | None = None, zero_lits: tuple | None = None) -> Batch:
    """one launch: block i has lens[i] source bytes and entries[i] entries (default: about one per 40 bytes), a random valid parse.
    mutations: {block: MUTATIONS name}.  order "block": srcOff and seqOff ascending; "shuffled": both in a random order of the blocks.
    gap: bytes between source regions (rounded up to 16) and entries between entry regions.  alias: {block: other block} — the
    block reads the other's source bytes (same srcOff and srcLen).  lit_max: literal runs of 1 .. lit_max bytes.  zero_lits: (block,
    first, last) — the block's entries [first, last) have no literals"""
    mutations = mutations or {}
    alias = alias or {}
    n = len(lens)
    spec = []
    for i, ln in enumerate(lens):
        k = entries[i] if entries is not None else max(1, min(int(ln) // 40, 2000))
        q = random_parse(rng, int(ln), int(k), lit_max)
        if zero_lits and zero_lits[0] == i:
            _, a, z = zero_lits
            q[a:z, 2] += q[a:z, 1]  # the literals become match bytes: coverage unchanged
            q[a:z, 1] = 0
            assert (q[:-1, 2] < LIMIT).all()
        count, cap, mark = len(q), len(q) + int(rng.integers(0, 4)), 0
        if i in mutations:
            ln, q, count, cap, mark = mutate(rng, mutations[i], int(ln), q, cap)
        spec.append((int(ln), q, count, cap, mark))
    for i, j in alias.items():
        assert spec[i][0] == spec[j][0]
    place = rng.permutation(n) if order == "shuffled" else np.arange(n)
    blocks = np.zeros(n, dtype=BLOCK_DTYPE)
    so = eo = 0
    for i in place:
        ln, q, count, cap, mark = spec[i]
        if i not in alias:
            blocks[i]["srcOff"] = so
            so += (ln + 15 + gap) & ~15
        blocks[i]["seqOff"], blocks[i]["srcLen"], blocks[i]["seqCap"], blocks[i]["mark"] = eo, ln, cap, mark
        eo += max(cap, len(q)) + gap
    for i, j in alias.items():
        blocks[i]["srcOff"] = blocks[j]["srcOff"]
    max_cap = int(blocks["seqCap"].max())
    src = rng.integers(0, 256, so + SRC_PAD, dtype=np.uint8)
    seqs = rng.integers(0, 1 << 32, (eo + max_cap + 1, 4), dtype=np.uint32)  # what lies past a block's entries: garbage
    counts = np.empty(n, dtype=np.uint32)
    for i, (ln, q, count, cap, mark) in enumerate(spec):
        o = int(blocks[i]["seqOff"])
        seqs[o:o + len(q)] = q
        counts[i] = count
    return Batch(src, blocks, seqs, counts)


def mutation_batch(rng: np.random.Generator, n: int = 48) -> tuple[Batch, dict]:
    """every mutation once, on blocks spread over a batch of n random valid ones -> (batch, {block: name})"""
    lens = [int(x) for x in rng.integers(1, 6000, n)]
    names = list(MUTATIONS)
    where = {int(b): m for b, m in zip(rng.choice(n, len(names), replace=False), names)}
    return make_batch(rng, lens, mutations=where), where
