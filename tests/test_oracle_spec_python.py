"""The oracle's chain levels (>= 5), restated a second time as an executable specification in plain Python and compared
sequence for sequence on small inputs: exact hash chains (4-byte hash, newest first, chainDepth links, best gain),
gain-based lazy rules, greedy parse with bounded extension and 4-byte backward extension, and the window-by-window
repeat-offset aware parse.  Independent of the C code (nothing shared but the profile numbers), so a slip in
oracle/qzstd_oracle.c that still round-trips — a wrong tie rule, an off-by-one in a window edge — shows up here, on CPU.
Pure-Python loops: small cases only.

Levels 1-4 have the same kind of second statement below (fast_candidates, the length-lazy rules of is_start): the tables as
dictionaries from slot to (position, tag), read as they were before the (sub-)tile and updated behind it; the near table as "the first
hashable position of the tile with that slot"; the probe order and the two tie rules as the oracle's header states them.  Both
specifications run on the edge inputs of tools/qz_edges.py (the inputs the GPU tests then run), and
test_edge_inputs_exercise_every_rule shows for every profile field and every named constant below either an edge input whose
sequences change with it, or why none can."""
from os.path import commonprefix

import pytest

import qz_bind as B
import qz_corpus as K
import qz_edges as E
import numpy as np

P1 = 2654435761
P2 = 0x85EBCA77
TAG_BITS = 14            # check tag kept beside a table entry's position
LAZY_WIN = 64            # the lazy rules never look across a window edge:
LAZY_EDGE = (63, 62, 61)   # rule k (k positions ahead) applies at window positions below LAZY_EDGE[k - 1]
LAZY_LEN = (0, 0, 2)     # lazy 1..3 (levels 1-4): position p + k defers p when its candidate is longer by more than LAZY_LEN[k - 1]
LAZY_GAIN = (4, 7)       # lazy 4 (chain levels): ... when it gains more than LAZY_GAIN[k - 1] quarter bytes more
REP_LAZY_GAIN = (4, 11)  # the repeat-aware parse's deferral thresholds
REP_CAP, REP_MIN = 32, 3   # repeat-offset probes compare REP_CAP bytes (a full hit always wins); shorter than REP_MIN is no match


def bitlen(x):  # 31 - clz(x) for x >= 1
    return x.bit_length() - 1


def match_len(src, q, p, cap):
    """common prefix of src[q:] and src[p:], at most cap bytes"""
    return len(commonprefix((src[q:q + cap], src[p:p + cap])))


def seg_end(pf, p, n):
    return min(n, ((p >> pf.segLog) + 1) << pf.segLog) if pf.segLog else n


def candidates(pf, src):
    n = len(src)
    nh = n - 3 if n >= 4 else 0
    tbl = {}
    chain = [0] * (n + 1)
    cand = [(0, 0)] * (n + 1)
    for p in range(nh):
        if p + 4 > seg_end(pf, p, n):  # would hash bytes of the next segment: takes no part
            continue
        v = src[p:p + 4]
        slot = ((int.from_bytes(v, "little") * P1 & 0xFFFFFFFF) * pf.tableSize) >> 32
        link = tbl.get(slot, 0)
        chain[p] = link
        tbl[slot] = p + 1
        cap = min(pf.capLen, seg_end(pf, p, n) - p)
        best, bg = (0, 0), 0
        for _ in range(pf.chainDepth):
            if link == 0:
                break
            q = link - 1
            if src[q:q + 4] == v:
                l = match_len(src, q, p, cap)
                g = 4 * l - bitlen(p - q + 1)
                if l >= 4 and (best[0] == 0 or g > bg):
                    best, bg = (l, p - q), g
            link = chain[q]
        cand[p] = best
    return cand, nh


def min_len(pf, off):
    return pf.minMatch + (1 if off >> pf.farLog1 else 0) + (1 if off >> pf.farLog2 else 0)


def take(pf, c):
    return c[0] != 0 and c[0] >= min_len(pf, c[1])


def extend(pf, src, p, off, L):
    lim = min(seg_end(pf, p, len(src)), ((p >> pf.extLog) + 2) << pf.extLog)
    while p + L < lim and src[p + L - off] == src[p + L]:
        L += 1
    return L


def back(pf, src, q, off, anchor):
    b = 0
    if pf.segLog:
        anchor = max(anchor, (q >> pf.segLog) << pf.segLog)  # never backwards across the start of the segment
    while b < pf.backExt and q - b > anchor and q - off - b > 0 and src[q - b - 1] == src[q - off - b - 1]:
        b += 1
    return b


def is_start(pf, cand, nh, p):
    """a usable candidate that no lazy rule defers: by gain at the chain levels (lazy 4, two rules), by length below them (lazy 1..3 rules)"""
    def gain(c):
        return 4 * c[0] - bitlen(c[1] + 1)

    if not take(pf, cand[p]):
        return False
    for k in range(1, (2 if pf.lazy >= 4 else pf.lazy) + 1):
        if p + k < nh and (p % LAZY_WIN) < LAZY_EDGE[k - 1] and take(pf, cand[p + k]):
            if pf.lazy >= 4 and gain(cand[p + k]) > gain(cand[p]) + LAZY_GAIN[k - 1]:
                return False
            if pf.lazy < 4 and cand[p + k][0] > cand[p][0] + LAZY_LEN[k - 1]:
                return False
    return True


def parse_plain(pf, src, cand, nh):
    out, p, anchor = [], 0, 0
    while p < nh:
        if not cand[p][0] or not is_start(pf, cand, nh, p):
            p += 1
            continue
        L, off = cand[p]
        if L == pf.capLen:
            L = extend(pf, src, p, off, L)
        b = back(pf, src, p, off, anchor)
        out.append((off, p - b - anchor, L + b))
        p += L
        anchor = p
    out.append((0, len(src) - anchor, 0))
    return out


def parse_rep(pf, src, cand, nh):
    n = len(src)
    CAP, MIN = REP_CAP, REP_MIN
    out, cur, anchor, rep, rep_seg = [], 0, 0, [0, 0], 0
    while cur < nh:
        if pf.segLog and (cur >> pf.segLog) != rep_seg:  # a new segment starts without repeat offsets
            rep, rep_seg = [0, 0], cur >> pf.segLog
        start_end = seg_end(pf, cur, n) - pf.hashBytes + 1  # nothing starts in a segment's last positions that cannot be hashed
        if cur >= start_end:
            cur = seg_end(pf, cur, n)
            continue
        lim = min(((cur >> pf.tileLog) + 1) << pf.tileLog, start_end)
        W = min(pf.repWin, lim - cur)
        V = min(W + 2, lim - cur)
        G, opt = [], []
        for k in range(V):
            p = cur + k
            c = cand[p]
            g, o = (4 * c[0] + 32 - bitlen(c[1] + 1), 0) if take(pf, c) else (0, 0)
            for r in range(2):
                if rep[r]:
                    mx, l = min(seg_end(pf, p, n) - p, CAP), 0
                    while l < mx and src[p - rep[r] + l] == src[p + l]:
                        l += 1
                    rg = 0 if l < MIN else (1000 - r if l >= CAP else 4 * l + 36 - r)
                    if rg > g:
                        g, o = rg, 1 + r
            G.append(g)
            opt.append(o)
        pick = None
        for k in range(W):
            if G[k] == 0 or (k + 1 < V and G[k + 1] > G[k] + REP_LAZY_GAIN[0]) or (k + 2 < V and G[k + 2] > G[k] + REP_LAZY_GAIN[1]):
                continue
            pick = k
            break
        if pick is None:
            cur += W
            continue
        q = cur + pick
        if opt[pick]:
            off = rep[opt[pick] - 1]
            mx, L = min(seg_end(pf, q, n) - q, CAP), 0
            while L < mx and src[q - off + L] == src[q + L]:
                L += 1
            if L == CAP:
                L = extend(pf, src, q, off, L)
        else:
            L, off = cand[q]
            if L == pf.capLen:
                L = extend(pf, src, q, off, L)
        b = back(pf, src, q, off, anchor)
        out.append((off, q - b - anchor, L + b))
        if off != rep[0]:
            rep = [off, rep[0]]
        cur = anchor = q + L
    out.append((0, n - anchor, 0))
    return out


# ---- levels 1-4: table probes -----------------------------------------------------------------------------------------------
def mixes(src, hash_bytes):
    """per position the 32-bit mix of its first hash_bytes (4..7) bytes: the first four (little endian) times P1, xor the rest (below 2^24)
    times P2's low 24 bits; hash_bytes 8 (the second table's key): the second four times all of P2"""
    n = len(src) - hash_bytes + 1
    if n <= 0:
        return []
    b = np.frombuffer(src, dtype=np.uint8).astype(np.uint64)
    lo = sum(b[k:n + k] << np.uint64(8 * k) for k in range(4))
    hi = sum(b[k:n + k] << np.uint64(8 * (k - 4)) for k in range(4, hash_bytes)) if hash_bytes > 4 else np.zeros(n, dtype=np.uint64)
    m = (lo * np.uint64(P1)) ^ (hi * np.uint64(P2 if hash_bytes == 8 else P2 & 0xFFFFFF))
    return (m & np.uint64(0xFFFFFFFF)).tolist()


def tag(m):
    return (m >> 3) & ((1 << TAG_BITS) - 1)


def fast_candidates(pf, src):
    """per position the better of up to three sources, in this order: the newest position of the earlier (sub-)tiles in the main table's
    slot; (levels 3-4) the newest one of the earlier (sub-)tiles whose 8 bytes hash alike, if STRICTLY longer; the first position of this
    tile in the near slot, if it lies before p and is AT LEAST as long (on a tie the nearer source wins)"""
    n, hb = len(src), pf.hashBytes
    nh = max(0, n - hb + 1)
    T = 1 << pf.tileLog
    S = 1 << pf.subTileLog if pf.subTileLog else T
    M, M8 = mixes(src, hb), mixes(src, 8) if pf.longSize else []
    main, second = {}, {}  # slot -> (position, tag)
    cand = [(0, 0)] * (n + 1)

    def hashable(p, k):  # the bytes a position hashes lie inside its segment
        return p + k <= seg_end(pf, p, n)

    def near_slot(m):
        return m >> (32 - pf.tileLog) if pf.tileLog else 0

    for t0 in range(0, nh, T):
        tile = [p for p in range(t0, min(t0 + T, nh)) if hashable(p, hb)]
        first = {}
        for p in tile:
            first.setdefault(near_slot(M[p]), (p, tag(M[p])))
        for s0 in range(t0, t0 + T, S):
            sub = [p for p in tile if s0 <= p < s0 + S]
            for p in sub:
                m, cap = M[p], min(pf.capLen, seg_end(pf, p, n) - p)
                probes = []  # (source, tie rule) in probe order
                e = main.get((m * pf.tableSize) >> 32)
                if e and e[1] == tag(m) and (not pf.window or p - e[0] <= pf.window):
                    probes.append((e[0], "first"))
                if pf.longSize and hashable(p, 8):
                    e = second.get((M8[p] * pf.longSize) >> 32)
                    if e and e[1] == tag(M8[p]):
                        probes.append((e[0], ">"))
                if pf.nearTab:
                    q, t = first[near_slot(m)]
                    if t == tag(m) and q < p:
                        probes.append((q, ">="))
                best = (0, 0)
                for q, rule in probes:
                    if src[q:q + 4] == src[p:p + 4]:
                        l = match_len(src, q, p, cap)
                        if rule == "first" or (l > best[0] if rule == ">" else l >= best[0]):
                            best = (l, p - q)
                cand[p] = best
            for p in sub:  # ascending: the largest position stays
                main[(M[p] * pf.tableSize) >> 32] = (p, tag(M[p]))
                if pf.longSize and hashable(p, 8):
                    second[(M8[p] * pf.longSize) >> 32] = (p, tag(M8[p]))
    return cand, nh


CANDIDATE_FIELDS = ("tableSize", "tileLog", "capLen", "nearTab", "window", "hashBytes", "longSize", "chainDepth", "subTileLog", "segLog")
_cand_memo = {}


def specification(pf, src):
    """the sequences of block `src` under profile `pf` by this file's rules (candidates memoised: levels that differ in the parse alone, and
    the parse constants' perturbations, share them)"""
    key = (TAG_BITS, tuple(getattr(pf, f) for f in CANDIDATE_FIELDS), src)
    if key not in _cand_memo:
        _cand_memo[key] = candidates(pf, src) if pf.chainDepth else fast_candidates(pf, src)
    cand, nh = _cand_memo[key]
    return parse_rep(pf, src, cand, nh) if pf.repWin else parse_plain(pf, src, cand, nh)


def oracle_sequences(oracle, pf, blk):
    n, seqs = oracle.find(pf, blk, cap=B.sequence_bound(len(blk)) + 16)  # (room to spare: the capacity rule refuses an empty block at its bound of 2)
    assert n != B.SEQ_ERROR
    return [(seqs[i].offset, seqs[i].litLength, seqs[i].matchLength) for i in range(n)]


def first_difference(got, want, who="oracle"):
    i = next(i for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)
    return "first difference at sequence %d: %s %s, specification %s" % (i, who, (got + [None])[i], (want + [None])[i])


_blocks = []


def blocks():
    if not _blocks:  # (generated once: the text generator builds a vocabulary on every call)
        _blocks.extend(make_blocks())
    return list(_blocks)


def make_blocks():
    yield K.text(21, 2500)
    yield K.weblog(22, 3000)
    yield K.binary_struct(23, 2000)
    yield b"".join(b"record%05d;" % (i % 7) + bytes(53) for i in range(40))  # runs + a 65-byte period: long repeats, capped matches
    yield (b"abcdefgh" * 5 + b"X") * 50
    yield K.text(24, 700) + K.text(24, 700) + K.text(25, 300) + K.text(24, 700)  # far-ish repeats across a tile edge
    yield K.weblog(26, 31000) + K.weblog(26, 4000)  # crosses the 32 KiB segment boundary with repeats on both sides


def small_planted(pf):
    return [(name, blk) for name, blk in E.planted(pf) if len(blk) <= E.CPU_MAX]


@pytest.mark.parametrize("level", [5, 6, 9, 10, 12, 0x106])
def test_chain_levels_equal_the_python_specification(oracle, level):
    for blk in list(blocks()) + [blk for _, blk in small_planted(oracle.profile(level, 0))]:
        pf = oracle.profile(level, len(blk))
        assert pf.chainDepth and pf.hashBytes == 4 and pf.lazy == 4 and not pf.nearTab and not pf.longSize
        want = specification(pf, blk)
        n, seqs = oracle.find(pf, blk)
        got = [(seqs[i].offset, seqs[i].litLength, seqs[i].matchLength) for i in range(n)]
        assert got == want, "level %#x, block of %d: first difference at sequence %d" % (
            level, len(blk), next(i for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b))


def spec_inputs(pf):
    """what the pure-Python specification can afford: every planted block and edge size up to 12.5 KiB (from the segment size on: one
    content kind), and the small blocks of blocks()"""
    return small_planted(pf) + E.edge_blocks(pf, E.CPU_MAX, one_kind_from=(1 << pf.segLog) - 8) + \
        [("blocks()[%d]" % i, blk) for i, blk in enumerate(blocks()) if len(blk) <= E.CPU_MAX]


@pytest.mark.parametrize("level", [1, 2, 3, 4, 0x101, 0x102, 0x103, 0x104])
def test_fast_levels_equal_the_python_specification(oracle, level):
    pf = oracle.profile(level, 0)
    assert not pf.chainDepth and pf.hashBytes == 5 and pf.lazy == 3 and pf.nearTab and pf.tileLog == 9 and pf.segLog == 12
    for name, blk in spec_inputs(pf):
        got, want = oracle_sequences(oracle, pf, blk), specification(pf, blk)
        assert got == want, "level %#x, %s (%d bytes): %s" % (level, name, len(blk), first_difference(got, want))


# ---- which rule does which input exercise ------------------------------------------------------------------------------------
FAMILY_LEVEL = {"fast": 1, "sub-tiles": 2, "second table": 3, "chain": 6, "fast + repeats": 0x101, "chain + repeats": 12}
NO_4_BYTE_MATCH = "below the chain levels a 4-byte candidate needs two 5-byte strings that differ in the fifth byte alone and share a slot: " \
                  "no pair of fifth bytes does (checked below), and only a 4-byte candidate is refused at 2048..4095 back"
EXT_CELL = "with 4 KiB segments the limit ((p >> extLog) + 2) << extLog is never below the segment's end once extLog >= segLog - 1"
REP_PARSE_NO_LAZY = "the repeat-aware parse has its own deferral (REP_LAZY_GAIN) and never reads profile.lazy"
REP_WIN = "a window without an option is skipped and the next one meets the same repeat offsets; the look-ahead of two positions is bounded " \
          "by the tile and the segment, not by the window"
CHAIN_NO_TILES = "the chain levels insert position by position: neither their candidates nor the plain parse read the (sub-)tile size"
CHAIN_SUB_TILE = "the chain levels insert position by position: nothing reads subTileLog (the repeat-aware parse reads tileLog alone)"

# (field, perturbed value, None = some edge input must change | the reason why none can), per family: every field the family's level reads
_COMMON = [("capLen", 47, None), ("minMatch", 5, None), ("farLog2", 15, None), ("backExt", 3, None), ("window", 2048, None),
           ("extLog", 10, None), ("extLog", 12, EXT_CELL), ("segLog", 13, None)]
_FAST = _COMMON + [("tableSize", 4096, None), ("tileLog", 8, None), ("farLog1", 11, NO_4_BYTE_MATCH), ("nearTab", 0, None), ("hashBytes", 6, None)]
_CHAIN = _COMMON + [("tableSize", 2944, None), ("farLog1", 11, None), ("hashBytes", 5, None), ("subTileLog", 5, CHAIN_SUB_TILE)]
PROFILE_ROWS = {
    "fast": _FAST + [("lazy", 2, None)],
    "sub-tiles": _FAST + [("lazy", 2, None), ("subTileLog", 5, None)],
    "second table": _FAST + [("lazy", 2, None), ("longSize", 4096, None)],
    "chain": _CHAIN + [("lazy", 3, None), ("chainDepth", 11, None), ("tileLog", 8, CHAIN_NO_TILES)],
    "fast + repeats": _FAST + [("lazy", 2, REP_PARSE_NO_LAZY), ("repWin", 15, REP_WIN)],
    "chain + repeats": _CHAIN + [("lazy", 3, REP_PARSE_NO_LAZY), ("chainDepth", 39, None), ("tileLog", 8, None), ("repWin", 15, REP_WIN)],
}
# (constant of this file, perturbed value), per family that reads it: through specification(), on the inputs it can afford
TAG_5 = "two 5-byte strings that agree in their first four bytes never share a slot (checked below), and every candidate's first four bytes " \
        "are compared: the tag only spares reading a source that would be refused anyway"
_LAZY_LEN_ROWS = [("LAZY_LEN", (1, 0, 2), None), ("LAZY_LEN", (0, 1, 2), None), ("LAZY_LEN", (0, 0, 3), None), ("LAZY_EDGE", (62, 62, 61), None),
                  ("LAZY_EDGE", (63, 61, 61), None), ("LAZY_EDGE", (63, 62, 60), None)]
_REP_ROWS = [("REP_LAZY_GAIN", (5, 11), None), ("REP_LAZY_GAIN", (4, 12), None), ("REP_CAP", 33, None), ("REP_CAP", 31, None), ("REP_MIN", 4, None),
             ("REP_MIN", 2, None)]
CONSTANT_ROWS = {
    "fast": _LAZY_LEN_ROWS + [("TAG_BITS", 0, TAG_5)], "sub-tiles": _LAZY_LEN_ROWS + [("TAG_BITS", 0, TAG_5)],
    "second table": _LAZY_LEN_ROWS + [("TAG_BITS", 0, None)],  # (two 8-byte strings with equal first halves can share a slot of the second table)
    "chain": [("LAZY_GAIN", (5, 7), None), ("LAZY_GAIN", (4, 8), None), ("LAZY_EDGE", (62, 62, 61), None), ("LAZY_EDGE", (63, 61, 61), None)],
    "fast + repeats": _REP_ROWS + [("TAG_BITS", 0, TAG_5)], "chain + repeats": _REP_ROWS,
}


def test_no_pair_of_fifth_bytes_agrees_in_slot_and_tag():
    """NO_4_BYTE_MATCH, TAG_5: two positions with equal first four bytes mix to values that differ by (b1 * c) ^ (b2 * c), b the fifth
    bytes; a candidate of exactly four bytes needs that difference to vanish in a table's slot bits (near table: the top 9, main table:
    the top 13 or 14) and in the tag's.  It never vanishes even in the top 9: no such pair shares a slot of any table"""
    c = P2 & 0xFFFFFF
    for b1 in range(256):
        for b2 in range(b1):
            assert (((b1 * c) ^ (b2 * c)) & 0xFFFFFFFF) >> (32 - 9), (b1, b2)


NINE_SEGMENTS = 36864 + 8


def all_edge_inputs(pf):
    """the inputs tools/qz_edges.py gives a family, the planted rules first, shortest first (an exercised rule shows early); of the edge sizes those up to nine
    segments (the longer ones are longer prefixes of the same base buffer)"""
    return sorted(E.planted(pf), key=lambda named: len(named[1])) + E.neighbours() + E.edge_blocks(pf, NINE_SEGMENTS)


@pytest.mark.parametrize("family", list(FAMILY_LEVEL))
def test_edge_inputs_exercise_every_rule(oracle, family, monkeypatch):
    """Every profile field the family's level reads, and every named constant of this file's specification, one step off: either at
    least one input of tools/qz_edges.py comes out with other sequences (the input EXERCISES the rule: a kernel that gets it wrong
    differs from the oracle there), or the row says why no input can, and then no input does."""
    import sys
    pf = oracle.profile(FAMILY_LEVEL[family], 0)
    used = {f for f, _ in B.OracleProfile._fields_ if getattr(pf, f)} - {"nearTab", "repWin"} | ({"nearTab"} if pf.nearTab else set()) | ({"repWin"} if pf.repWin else set())
    assert used | {"window"} == {f for f, _, _ in PROFILE_ROWS[family]}, "a profile field this level reads has no row"
    inputs = all_edge_inputs(pf)
    base = {}

    def changed_by(field, value):
        q = B.OracleProfile.from_buffer_copy(pf)
        setattr(q, field, value)
        for i, (name, blk) in enumerate(inputs):
            if i not in base:
                base[i] = oracle_sequences(oracle, pf, blk)
            if oracle_sequences(oracle, q, blk) != base[i]:
                return name
        return None

    report, wrong = [], []
    for field, value, inert in PROFILE_ROWS[family]:
        hit = changed_by(field, value)
        report.append("%s -> %s: %s" % (field, value, hit or "inert"))
        if inert is None and hit is None:
            wrong.append("no edge input exercises profile.%s (%d -> %d changes no sequence)" % (field, getattr(pf, field), value))
        if inert is not None and hit is not None:
            wrong.append("profile.%s -> %d changes %s, but is listed inert: %s" % (field, value, hit, inert))
    small = small_planted(pf)  # (the chain levels' specification takes a second per 4 KiB of text: the planted blocks are what it can afford)
    want = [specification(pf, blk) for _, blk in small]
    for const, value, inert in CONSTANT_ROWS[family]:
        with monkeypatch.context() as mp:
            mp.setattr(sys.modules[__name__], const, value)
            hit = next((name for (name, blk), w in zip(small, want) if specification(pf, blk) != w), None)
        report.append("%s -> %s: %s" % (const, value, hit or "inert"))
        if inert is None and hit is None:
            wrong.append("no edge input exercises %s (-> %s changes no sequence of the specification)" % (const, value))
        if inert is not None and hit is not None:
            wrong.append("%s -> %s changes %s, but is listed inert: %s" % (const, value, hit, inert))
    print("\n".join(report))
    assert not wrong, "%s (level %#x): %s" % (family, FAMILY_LEVEL[family], "; ".join(wrong))
