"""Edge inputs of the match-finder, one generator for the CPU and the GPU tests (deterministic, numpy only, reads nothing but this
repository's own sources).

* ``edge_sizes(pf)`` / ``edge_blocks(pf)`` — the block lengths at which a kernel family can go wrong, derived from the profile (tile,
  segment, bytes hashed) and the kernels' named constants (``kernel_constants()`` reads them out of csrc/qzstd_kernels.hip and
  include/qzstd_hip.h), as prefixes of one base buffer per content kind.
* ``planted(pf)`` — blocks of incompressible bytes with repeats copied in at chosen (dst, src, len); the byte before and the byte
  behind every copy differ from the source's, so the match length is exact.  One block per rule of the definition
  (oracle/qzstd_oracle.c), named after it.
* ``neighbours()`` — consecutive slices of one periodic buffer in lengths that are multiples of 16: packed the way
  ``Plugin.find_batch`` packs its source buffer, every block is followed directly by bytes that continue its last match.
"""
from __future__ import annotations

import os
import re

import qz_corpus as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAZY_WIN = 64  # the lazy rules never look across a 64-position window edge (one wave decides a window)
CPU_MAX = 12800  # blocks up to 12.5 KiB also go through the pure-Python specification

_consts = None


def kernel_constants() -> dict:
    """the kernels' named layout constants, evaluated from their definitions in the sources"""
    global _consts
    if _consts is None:
        with open(os.path.join(ROOT, "include", "qzstd_hip.h")) as f:
            hdr = f.read()
        with open(os.path.join(ROOT, "qat-zstd-plugin_amd", "csrc", "qzstd_kernels.hip")) as f:
            krn = f.read()
        env: dict = {}

        def take(name, text, pat):
            m = re.search(pat % name, text)
            assert m, "no definition of %s" % name
            env[name] = int(eval(re.sub(r"\b(\d+)u\b", r"\1", m.group(1)), {"__builtins__": {}}, dict(env)))

        take("QZ_RING", hdr, r"#define\s+%s\s+(\d+u?)")
        take("QZSTD_HIP_BLOCK_MAX", hdr, r"#define\s+%s\s+(\([^)]*\))")
        for name in ("kMatchWaves", "kTileLog", "kTile", "kRing", "kLook", "kNear", "kRepCap"):
            take(name, krn, r"constexpr\s+\w+\s+(?:[^;]*?,\s*)?%s\s*=\s*([^;,]+)[;,]")
        _consts = env
    return _consts


# ------------------------------------------------------------------------------------------------------------------------ sizes
def edge_sizes(pf, max_len: int | None = None) -> list[int]:
    """block lengths around every boundary of profile `pf`'s kernels, ascending"""
    kc = kernel_constants()
    seg, tile, ring, top = 1 << pf.segLog, 1 << pf.tileLog, kc["kRing"], kc["QZSTD_HIP_BLOCK_MAX"]
    assert tile == kc["kTile"] and pf.segLog and ring % seg == 0
    per_pass = kc["kMatchWaves"]  # segments the launch kernels' deferred parse takes at a time
    assert per_pass * seg == ring
    s = set(range(0, 10)) | {15, 16, 17}
    # the lazy window, the tile, one and two segments; the ring (= the NEAR limit = one pass of segments), one segment more (a second pass),
    # two passes, one more, the longest block
    for b in (LAZY_WIN, tile, seg, 2 * seg, ring, ring + seg, 2 * ring, 2 * ring + seg, top):
        s |= set(range(b - 8, min(b + 8, top) + 1))
    s |= {kc["kLook"] - 1, kc["kLook"], kc["kLook"] + 1}
    return sorted(x for x in s if max_len is None or x <= max_len)


_bases: dict = {}


def base(kind: str) -> bytes:
    """the one base buffer of a content kind (the longest block's length)"""
    if kind not in _bases:
        n = kernel_constants()["QZSTD_HIP_BLOCK_MAX"]
        _bases[kind] = {"text": lambda: K.text(3, n), "weblog": lambda: K.weblog(6, n),
                        "period": lambda: ((b"abcdefgh" * 5 + b"X") * (n // 41 + 1))[:n],
                        "zeros": lambda: bytes(n), "ab": lambda: b"ab" * (n // 2)}[kind]()
    return _bases[kind]


KINDS = ("text", "weblog", "period", "zeros", "ab")


def edge_blocks(pf, max_len: int | None = None, kinds=KINDS, one_kind_from: int | None = None) -> list[tuple[str, bytes]]:
    """(name, block) for every edge size: every content kind below `one_kind_from` (default: the sizes around the ring size), the first
    kind alone from there on"""
    if one_kind_from is None:
        one_kind_from = kernel_constants()["kRing"] - 8
    out = []
    for n in edge_sizes(pf, max_len):
        for kind in (kinds if n < one_kind_from else kinds[:1]):
            out.append(("%s[:%d]" % (kind, n), base(kind)[:n]))
    return out


# ---------------------------------------------------------------------------------------------------------------------- planted
def plant(n: int, copies, seed: int, quiet=(), only=None) -> bytes:
    """n incompressible bytes; the spans `quiet` are zeroed (a filler that occupies one table slot, so that a far source is still in its
    slot when the copy looks it up); then every (dst, src, len) is copied in, in order, and the byte before and the byte behind the copy
    are made to differ from the source's ((dst, src, len, False): the byte before is left alone)"""
    b = bytearray(K.incompressible(seed, n))
    for a, e in quiet:
        b[a:e] = bytes(e - a)
    if only is not None:  # quiet everywhere but in the spans (start, length)
        keep = bytearray(n)
        for a, ln in only:
            keep[a:a + ln] = b[a:a + ln]
        b = keep
    for c in copies:
        dst, src, ln = c[:3]
        assert 0 <= src and src + ln <= dst and dst + ln <= n, (dst, src, ln, n)
        b[dst:dst + ln] = b[src:src + ln]
        if (len(c) < 4 or c[3]) and src > 0 and b[dst - 1] == b[src - 1]:
            b[dst - 1] ^= 0xA5
        if dst + ln < n and b[dst + ln] == b[src + ln]:
            b[dst + ln] ^= 0xA5
    return bytes(b)


def _far_sources(n, first_src, backs, ln, seed, quiet=True):
    """copies of `ln` bytes from sources ln + 60 apart, the i-th exactly backs[i] bytes back"""
    copies = [(first_src + (ln + 60) * i + back, first_src + (ln + 60) * i, ln) for i, back in enumerate(backs)]
    last = first_src + (ln + 60) * len(backs)
    return plant(n, copies, seed, [(last, max(c[0] + c[2] for c in copies) + 16)] if quiet else ())


def _min_len_grid(centre, seed):
    """sources centre - 1 / centre / centre + 1 bytes back, each with match lengths 4, 5, 6 and 7 (qzo_min_len)"""
    copies = []
    for j, back in enumerate((centre - 1, centre, centre + 1)):
        for i, ln in enumerate((4, 5, 6, 7)):
            src = 32 + 24 * (4 * j + i)
            copies.append((src + back, src, ln))
    return plant(centre + 400, copies, seed, [(336, centre + 24)])


def _lazy_pair(copies, a_at, b_at, p, d, la, delta):
    """position p matches the la bytes at a_at, position p + d the la + delta bytes at b_at (which begin with a_at's bytes d..la)"""
    copies.append((b_at, a_at + d, la - d) if a_at < b_at else (a_at + d, b_at, la - d))  # B = A[d:la] + d + delta bytes of its own
    copies.append((p, a_at, la))
    copies.append((p + la, b_at + la - d, d + delta, False))


_planted: dict = {}


def planted(pf) -> list[tuple[str, bytes]]:
    """(name, block) per planted rule, for the kernel family of profile `pf`"""
    key = tuple(getattr(pf, f) for f, _ in pf._fields_)
    if key not in _planted:
        _planted[key] = _plant_all(pf)
    return list(_planted[key])


def _plant_all(pf):
    kc = kernel_constants()
    seg, tile, cap, hb, ring, near, top = 1 << pf.segLog, 1 << pf.tileLog, pf.capLen, pf.hashBytes, kc["kRing"], kc["kNear"], kc["QZSTD_HIP_BLOCK_MAX"]
    rep_cap = kc["kRepCap"]
    out = []

    # sources at the edge between the LDS and the device-memory side of the compare, and at the ring size
    near_backs = (near - 1, near, near + 1)
    out.append(("near_limit_in_32k", _far_sources(ring, 64, near_backs, 40, 101)))
    out.append(("near_limit_and_ring_in_128k", _far_sources(top, 60000, near_backs + (ring - 1, ring, ring + 1), 40, 102)))
    out.append(("near_limit_and_ring_in_128k_busy_tables", _far_sources(top, 60000, near_backs + (ring - 1, ring, ring + 1), 400, 103, quiet=False)))
    # the two offset thresholds of the minimum match length
    out.append(("min_len_around_far1", _min_len_grid(1 << pf.farLog1, 104)))
    out.append(("min_len_around_far2", _min_len_grid(1 << pf.farLog2, 105)))
    # candidate lengths at the cap, and the extension that follows
    out.append(("cap_len", plant(2200, [(1032 + 200 * i, 32 + 200 * i, ln) for i, ln in enumerate((cap - 1, cap, cap + 1, cap + 102))], 106, [(820, 1030)])))

    # repeat offsets: an offset is established by a 10-byte match, three literals on the same offset matches again for `ln` bytes
    copies = []
    for i, ln in enumerate((2, 3, 4, rep_cap - 1, rep_cap, rep_cap + 1)):
        s, d = 32 + 64 * i, 600 + 128 * i
        copies += [(d, s, 10), (d + 13, s + 13, ln)]
    # ... and a repeat of exactly rep_cap - 1 / rep_cap bytes against a hash candidate of cap bytes at the same position ("a full hit always wins")
    for i, ln in enumerate((rep_cap - 1, rep_cap)):
        s, a, d = 1600 + 64 * i, 1800 + 64 * i, 2100 + 128 * i
        copies += [(a, s + 13, ln), (d, s, 10), (d + 13, a, cap)]
    out.append(("repeat_lengths", plant(2500, copies, 107, [(420, 590), (1930, 2090)])))

    # segment ends: a match that ends exactly on a segment's last byte; one that would run across it
    out.append(("match_to_segment_end", plant(2 * seg + 600, [(seg - 20, seg - 720, 20), (2 * seg - 20, 2 * seg - 720, 60)], 108)))
    # starts on the last hashable position of a segment and on the positions behind it (5 bytes hashed below the chain levels, 4 at them, 8 for
    # the second table): copies of 12 bytes that run across the boundary
    out.append(("start_at_last_hashable", plant(3 * seg + 500, [(k * seg - back, k * seg - back - 700, 12) for k, back in ((1, hb), (2, hb - 1), (3, hb + 1))], 109)))
    out.append(("start_at_last_8_hashable", plant(3 * seg + 500, [(k * seg - back, k * seg - back - 700, 12) for k, back in ((1, 8), (2, 7), (3, 3))], 110)))
    # ... and at the end of the block (the last segment's end)
    out.append(("start_at_block_end", plant(1500, [(1500 - 3 * hb, 700, hb), (1500 - hb + 1, 760, hb - 1)], 111)))

    # backward extension of 3 / 4 / 5 equal bytes.  (a) the source's bytes before it are a segment's last, unhashable positions — never
    # inserted, so the match is found at the segment's first byte and grows backwards; (b) stopped by the anchor: a match ends right where the
    # next one starts, whose source also has the bytes before it; (c) stopped by the segment's first byte: the copy starts before the boundary;
    # (d) a source at position 0
    out.append(("back_ext_source_behind_unhashable", plant(3 * seg + 200, [((j + 1) * seg + 100, (j + 1) * seg - k, 30 + k) for j, k in enumerate((3, 4, 5))], 112)))
    copies = []
    for i, k in enumerate((3, 4, 5)):
        s1, s2, d = 32 + 120 * i, 72 + 120 * i, 700 + 100 * i
        copies += [(s2, s1 + 20 - k, k), (d, s1, 20), (d + 20, s2 + k, 20, False)]
    out.append(("back_ext_stopped_by_anchor", plant(1100, copies, 113, [(400, 690)])))
    out.append(("back_ext_stopped_by_segment_start", plant(3 * seg + 200, [((j + 1) * seg - k, (j + 1) * seg - k - 900, 30 + k) for j, k in enumerate((3, 4, 5))], 114)))
    b = bytearray(plant(900, [(600, 0, 30)], 115))
    b[599] = 0  # what lies before a block in a packed source buffer: padding
    out.append(("back_ext_source_at_0", bytes(b)))

    # (e) four equal bytes before a match whose positions found nothing usable: each of their 4-byte strings was planted more often than the
    # deepest chain walks, 4 KiB back (one byte too short to be taken from there), so the chain levels find the real source at the fifth position
    depth, ln, q = max(pf.chainDepth, 64) + 2, 30, 100
    b = bytearray(K.incompressible(116, 200 + 32 * depth + seg + 50 + ln + 100))
    at = 200
    for j in range(4):
        for r in range(depth):
            b[at:at + 4] = b[q - 4 + j:q + j]
            b[at + 4] = b[q + j] ^ (1 + r % 255)
            at += 8
    at += seg + 50
    b[at - 4:at + ln] = b[q - 4:q + ln]
    b[at - 5], b[at + ln] = b[q - 5] ^ 0xA5, b[q + ln] ^ 0xA5
    out.append(("back_ext_behind_exhausted_chains", bytes(b)))
    # one 4-byte string followed by each of the 256 byte values: 5 bytes are hashed below the chain levels, so none may come out as a 4-byte
    # match there (no two of them share a table slot), and every one does at the chain levels
    b = bytearray(K.incompressible(117, 16 + 8 * 256 + 64))
    for v in range(256):
        b[16 + 8 * v:16 + 8 * v + 5] = b[0:4] + bytes([v])
    out.append(("fifth_byte_differs", bytes(b)))

    # the length-lazy rules and their window edges: candidates 1, 2, 3 positions apart whose lengths differ by 0..3, the first at 60..63 of a window
    # (eight cases per pair of tiles: sources in the first, the positions in the second, zeros between them — every incompressible position
    # inserted between a source and its use may take the source's table slot)
    copies, only, i = [], [], 0
    for pos in (60, 61, 62, 63):
        for d in (1, 2, 3):
            for delta in (0, 1, 2, 3):
                pair, w = divmod(i, tile // LAZY_WIN)
                a_at = tile * (1 + 2 * pair) + 40 + 40 * w
                only += [(a_at - 1, 14), (a_at + 19, 14 + delta)]
                _lazy_pair(copies, a_at, a_at + 20, tile * (2 + 2 * pair) + LAZY_WIN * w + pos, d, 12, delta)
                i += 1
    out.append(("lazy_by_length", plant(tile * (1 + 2 * (i // (tile // LAZY_WIN))) + LAZY_WIN, copies, 120, only=only)))
    # the same with gains: (4 per byte) - (bits of the offset); offsets 100 / 200 / 300 / 400 have 6 / 7 / 8 / 8 bits.  Differences of
    # 3, 4, 5 (one position on: thresholds 4 / 4), 6, 7, 8 (two on: 7) and 10, 11, 12 (two on, repeat-aware parse: 11)
    copies, i = [], 0
    cell = 9 * LAZY_WIN
    for d, delta, off_a, off_b in ((1, 1, 100, 200), (1, 1, 400, 300), (1, 1, 200, 100),
                                   (2, 2, 100, 300), (2, 2, 100, 200), (2, 2, 400, 300),
                                   (2, 3, 100, 300), (2, 3, 100, 200), (2, 3, 400, 300)):
        for pos in (63 - d, 64 - d):  # the last position at which the rule looks ahead, and the first at which it does not
            p = 512 + cell * i + 7 * LAZY_WIN + pos
            _lazy_pair(copies, p - off_a, p + d - off_b, p, d, 12, delta)
            i += 1
    out.append(("lazy_by_gain", plant(512 + cell * (i + 1), copies, 121)))

    # the two tie rules.  Near table (>=): the earlier tile's and this tile's source give equal lengths, the nearer one wins
    out.append(("near_table_tie", plant(2 * tile + 200, [(tile + 88, 100, 10), (tile + 288, 100, 10)], 122)))
    # ... and the cap decides a comparison: the earlier tile's source matches cap bytes, the nearer one cap - 1 (the longer one wins; capped one
    # byte earlier they tie and the nearer one wins — at the chain levels by its cheaper offset)
    out.append(("cap_len_decides", plant(2 * tile + 200, [(tile + 88, 100, cap - 1), (tile + 288, 100, cap)], 125)))
    # ... with sub-tiles: the main table offers the newest source of the earlier sub-tiles (cap bytes), the near table the tile's first (cap - 1)
    out.append(("cap_len_decides_with_sub_tiles", plant(2 * tile + 200, [(tile + 24, 100, cap - 1), (tile + 160, 100, cap), (tile + 288, 100, cap)], 126)))
    # second table (strict >): the newest source with the position's 8 bytes sits where 5 bytes are hashable and 8 are not, so the second
    # table still holds the older one; equal lengths, the main table's stays
    out.append(("second_table_tie", plant(seg + 2 * tile, [(seg - 7, 100, 10), (seg + tile + 88, 100, 10)], 123, [(200, seg - 100)])))
    # sub-tiles (level 2): the first occurrence in the tile matches 6 bytes, a later one in an earlier 64-position sub-tile 12: the near table
    # offers the first, the main table, when it is updated per sub-tile, the later one
    b = bytearray(plant(2 * tile, [(tile + 138, tile + 10, 12), (tile + 266, tile + 138, 12)], 124))
    b[tile + 16] ^= 0x5A  # the first occurrence now matches the other two for 6 bytes only
    out.append(("earlier_sub_tile", bytes(b)))
    return out


def neighbours() -> list[tuple[str, bytes]]:
    """consecutive slices of a 41-periodic buffer (lengths: multiples of 16), then zeros of odd length"""
    buf = base("period")
    out, at = [], 0
    for n in (16, 48, 528, 4096, 4112, 1040, 32768, 4080, 16, 36864):
        out.append(("period[%d:+%d]" % (at, n), buf[at:at + n]))
        at += n
    out.append(("zeros[:4099]", bytes(4099)))
    return out
