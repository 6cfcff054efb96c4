/*
 * qzstd_hufblock.h — a zstd Compressed_Block that is Huffman-coded literals and nothing else (no sequences), for blocks whose matches are
 * not worth their sequences: the sign/exponent plane of a byte-grouped frame is i.i.d. draws from some twenty byte values, and a Huffman
 * code is all there is to gain.  Plain C, no GPU header, no libzstd; every function is static inline and compiles for the host and
 * inside a HIP kernel: the kernel (qzstd_hip_huf_code), the CPU suite's mock of it and the tests all use THIS definition, so code lengths,
 * codes and streams are the same bytes wherever they are computed.  libzstd's decoder is the arbiter of the format
 * (tests/test_hufblock_host.py).
 *
 * The pieces, in the order a block is made:
 *   QZSTD_hufLengths       byte histogram -> a complete prefix code of at most QZSTD_HUF_MAX_BITS bits over the bytes that occur
 *   QZSTD_hufCodes         lengths -> canonical codes (zstd's: the longest codes first, symbols ascending within a length)
 *   QZSTD_hufEncodeStreams the 6-byte jump table and the four streams (the sequential definition; the kernel does the same in parallel)
 *   QZSTD_hufWriteTree     lengths -> the tree description (host only: serial and tiny)
 *   QZSTD_hufBlockBody     literals section header, tree description, jump table, streams, and the byte 0x00: no sequences
 *   QZSTD_hufTakes         the rule: is this block written that way
 */
#ifndef QZSTD_HUFBLOCK_H
#define QZSTD_HUFBLOCK_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QZSTD_HUF_FN __host__ __device__ static inline
#else
#define QZSTD_HUF_FN static inline
#endif

#define QZSTD_HUF_MAX_BITS 11u      /* the format's limit for a literals code */
#define QZSTD_HUF_LEN_MIN 1024u     /* shorter blocks are not coded: the single-stream form is never needed */
#define QZSTD_HUF_LEN_MAX 131072u   /* a zstd block */
#define QZSTD_HUF_LENGTHS_BYTES 128u /* 256 code lengths, a nibble each: symbol 2i in the low nibble of byte i, 2i + 1 in the high one */
#define QZSTD_HUF_JUMP_BYTES 6u
#define QZSTD_HUF_TREE_MAX 129u      /* header byte + at most 128 bytes (FSE: below 128; direct: 128 weights in 64 bytes) */
/* what a sequence is priced at by the rule, in eighths of a byte (QZSTD_hufTakes) */
#define QZSTD_HUF_SEQ_EIGHTHS 24u
/* room for any block body: 5 + tree + jump table + streams (below len for a coded block) + 1 */
#define QZSTD_HUF_BODY_BOUND(len) ((size_t)(len) + 5u + QZSTD_HUF_TREE_MAX + 1u)

QZSTD_HUF_FN uint32_t QZSTD_hufHighbit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); } /* x > 0 */

/* ------------------------------------------------------------------------------------------------------------------ code lengths -- */

/* scratch of QZSTD_hufLengthsSorted: the 2n - 1 nodes of the tree, leaves first */
typedef struct {
    uint32_t w[512];    /* a node's count, then its depth */
    uint16_t par[512];  /* its parent */
} QZSTD_hufWksp;

/* keys[0 .. n) = (hist[b] << 8 | b) of the bytes that occur, ascending: by count, then by value.  Returns n.  (Keys are distinct, so any
 * sorting method gives this array; the kernel ranks them in parallel.) */
QZSTD_HUF_FN uint32_t QZSTD_hufSortKeys(const uint32_t hist[256], uint32_t keys[256])
{
    uint32_t n = 0u, b;
    for (b = 0u; b < 256u; b++) {
        uint32_t k, i;
        if (!hist[b]) continue;
        k = (hist[b] << 8) | b;
        for (i = n; i > 0u && keys[i - 1u] > k; i--) keys[i] = keys[i - 1u];
        keys[i] = k;
        n++;
    }
    return n;
}

/* The lengths from the sorted keys of n >= 2 bytes: plain Huffman by the two-queue method (leaves in key order; of a leaf and an inner node
 * of equal count the leaf is taken first), and while the deepest leaf lies deeper than QZSTD_HUF_MAX_BITS every count is halved
 * once more (count >> shift, at least 1: the order of the keys stays a non-decreasing order of the counts) and the tree rebuilt.  All
 * counts 1 give a tree of depth 8, so this ends.  A Huffman tree is full: the code is complete (Kraft sum exactly 1), its longest codes
 * come in pairs.  nbits[] is written for all 256 bytes (0: does not occur); returns the greatest length. */
QZSTD_HUF_FN uint32_t QZSTD_hufLengthsSorted(const uint32_t *keys, uint32_t n, uint8_t nbits[256], QZSTD_hufWksp *ws)
{
    uint32_t shift, i, maxBits = 0u;
    for (i = 0u; i < 256u; i++) nbits[i] = 0u;
    for (shift = 0u;; shift++) {
        uint32_t leaf = 0u, inner = n, next = n, pick[2], j;
        for (i = 0u; i < n; i++) {
            const uint32_t c = (keys[i] >> 8) >> shift;
            ws->w[i] = c ? c : 1u;
        }
        while (next < 2u * n - 1u) {
            for (j = 0u; j < 2u; j++) {
                if (leaf < n && (inner >= next || ws->w[leaf] <= ws->w[inner])) pick[j] = leaf++;
                else pick[j] = inner++;
            }
            ws->w[next] = ws->w[pick[0]] + ws->w[pick[1]];
            ws->par[pick[0]] = (uint16_t)next;
            ws->par[pick[1]] = (uint16_t)next;
            next++;
        }
        ws->w[2u * n - 2u] = 0u; /* the root; a parent is made after its children, so it stands behind them */
        for (i = 2u * n - 2u; i-- > 0u;) ws->w[i] = ws->w[ws->par[i]] + 1u;
        maxBits = 0u;
        for (i = 0u; i < n; i++)
            if (ws->w[i] > maxBits) maxBits = ws->w[i];
        if (maxBits <= QZSTD_HUF_MAX_BITS) break;
    }
    for (i = 0u; i < n; i++) nbits[keys[i] & 0xFFu] = (uint8_t)ws->w[i];
    return maxBits;
}

/* The code lengths of a block of `len` bytes with the byte counts hist[] (they sum to len).  Returns the greatest length, 1 .. 11, or 0:
 * fewer than two distinct bytes, not coded (nbits[] is all 0 then). */
QZSTD_HUF_FN uint32_t QZSTD_hufLengths(const uint32_t hist[256], uint32_t len, uint8_t nbits[256])
{
    uint32_t keys[256], n, i;
    QZSTD_hufWksp ws;
    (void)len;
    n = QZSTD_hufSortKeys(hist, keys);
    if (n < 2u) {
        for (i = 0u; i < 256u; i++) nbits[i] = 0u;
        return 0u;
    }
    return QZSTD_hufLengthsSorted(keys, n, nbits, &ws);
}

QZSTD_HUF_FN uint32_t QZSTD_hufMaxBits(const uint8_t nbits[256])
{
    uint32_t m = 0u, b;
    for (b = 0u; b < 256u; b++)
        if (nbits[b] > m) m = nbits[b];
    return m;
}

/* the Kraft sum of the lengths in units of 2^-11: 2048 for a complete code */
QZSTD_HUF_FN uint32_t QZSTD_hufKraft(const uint8_t nbits[256])
{
    uint32_t s = 0u, b;
    for (b = 0u; b < 256u; b++)
        if (nbits[b]) s += 1u << (QZSTD_HUF_MAX_BITS - nbits[b]);
    return s;
}

QZSTD_HUF_FN void QZSTD_hufPackLengths(const uint8_t nbits[256], uint8_t out[QZSTD_HUF_LENGTHS_BYTES])
{
    uint32_t i;
    for (i = 0u; i < 128u; i++) out[i] = (uint8_t)(nbits[2u * i] | (nbits[2u * i + 1u] << 4));
}

QZSTD_HUF_FN void QZSTD_hufUnpackLengths(const uint8_t in[QZSTD_HUF_LENGTHS_BYTES], uint8_t nbits[256])
{
    uint32_t i;
    for (i = 0u; i < 128u; i++) {
        nbits[2u * i] = in[i] & 15u;
        nbits[2u * i + 1u] = in[i] >> 4;
    }
}

/* ---------------------------------------------------------------------------------------------------------------- canonical codes -- */

/* tab[b] = code | nbits << 16 (0 for a byte that does not occur).  weight = maxBits + 1 - nbits; codes are handed out from the lowest weight
 * (the longest codes, from 0) up, symbols in ascending order within a weight: the first code of a length is half of what follows the last
 * code of the length above it.  This is the order in which zstd's decoder fills its table. */
QZSTD_HUF_FN void QZSTD_hufCodes(const uint8_t nbits[256], uint32_t tab[256])
{
    uint32_t perLen[QZSTD_HUF_MAX_BITS + 2u], val[QZSTD_HUF_MAX_BITS + 2u], b, n, min = 0u;
    for (n = 0u; n < QZSTD_HUF_MAX_BITS + 2u; n++) perLen[n] = 0u;
    for (b = 0u; b < 256u; b++) perLen[nbits[b] <= QZSTD_HUF_MAX_BITS ? nbits[b] : 0u]++;
    for (n = QZSTD_HUF_MAX_BITS; n >= 1u; n--) {
        val[n] = min;
        min = (min + perLen[n]) >> 1;
    }
    val[0] = 0u;
    for (b = 0u; b < 256u; b++) {
        const uint32_t nb = nbits[b];
        tab[b] = (nb && nb <= QZSTD_HUF_MAX_BITS) ? (val[nb]++ | (nb << 16)) : 0u;
    }
}

/* ------------------------------------------------------------------------------------------------------------------------ streams -- */

/* stream k (0 .. 3) covers the bytes [*start, *end) of a block of len >= QZSTD_HUF_LEN_MIN bytes: (len + 3) / 4 each, the fourth the rest */
QZSTD_HUF_FN void QZSTD_hufStreamSpan(uint32_t len, uint32_t k, uint32_t *start, uint32_t *end)
{
    const uint32_t seg = (len + 3u) >> 2;
    *start = k * seg;
    *end = k < 3u ? (k + 1u) * seg : len;
}

/* bytes of a stream of `bits` code bits: the closing 1 bit, then zeros up to the byte */
QZSTD_HUF_FN uint32_t QZSTD_hufStreamBytes(uint32_t bits) { return (bits >> 3) + 1u; }

/* The jump table and the four streams of src[0 .. len) into dst (room for `cap` bytes); the sequential definition.  A stream is written from
 * its last byte to its first, each code as an integer LSB-first into little-endian bytes, closed by a single 1 bit.  Returns the bytes
 * written, 6 + the four streams; 0 when they do not fit in cap, when a byte has no code, or when a stream is too long for the jump table. */
QZSTD_HUF_FN size_t QZSTD_hufEncodeStreams(const uint8_t *src, uint32_t len, const uint32_t tab[256], uint8_t *dst, size_t cap)
{
    size_t pos = QZSTD_HUF_JUMP_BYTES;
    uint32_t k;
    if (len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX || cap < QZSTD_HUF_JUMP_BYTES) return 0u;
    for (k = 0u; k < 4u; k++) {
        const size_t first = pos;
        uint64_t acc = 0u;
        uint32_t fill = 0u, s, e, i;
        QZSTD_hufStreamSpan(len, k, &s, &e);
        for (i = e; i-- > s;) {
            const uint32_t t = tab[src[i]];
            if (!t) return 0u;
            acc |= (uint64_t)(t & 0xFFFFu) << fill;
            fill += t >> 16;
            while (fill >= 8u) {
                if (pos >= cap) return 0u;
                dst[pos++] = (uint8_t)acc;
                acc >>= 8;
                fill -= 8u;
            }
        }
        if (pos >= cap) return 0u;
        dst[pos++] = (uint8_t)(acc | (1u << fill));
        if (k < 3u) {
            if (pos - first > 0xFFFFu) return 0u;
            dst[2u * k] = (uint8_t)(pos - first);
            dst[2u * k + 1u] = (uint8_t)((pos - first) >> 8);
        }
    }
    return pos;
}

/* --------------------------------------------------------------------------------------------------------------- tree description -- */
/* (host only from here on) */

#define QZSTD_HUF_TREE_AUTO 0   /* the smaller form; the direct one when equal */
#define QZSTD_HUF_TREE_DIRECT 1
#define QZSTD_HUF_TREE_FSE 2

typedef struct {
    uint8_t *p;
    size_t cap, pos;
    uint64_t acc;
    uint32_t fill;
    int overflow;
} QZSTD_hufBits;

static inline void QZSTD_hufBitsAdd(QZSTD_hufBits *b, uint32_t v, uint32_t n)
{
    b->acc |= (uint64_t)v << b->fill;
    b->fill += n;
    while (b->fill >= 8u) {
        if (b->pos < b->cap) b->p[b->pos++] = (uint8_t)b->acc;
        else b->overflow = 1;
        b->acc >>= 8;
        b->fill -= 8u;
    }
}

static inline void QZSTD_hufBitsFlush(QZSTD_hufBits *b)
{
    if (b->fill) QZSTD_hufBitsAdd(b, 0u, 8u - b->fill);
}

/* The n >= 2 weights wt[0 .. n) (each 0 .. 11, not all equal) as an FSE stream: the NCount header of a distribution over 64 cells (accuracy
 * log 6; every weight that occurs gets at least one cell, none is a "less than one" cell), then the weights coded backwards with two
 * interleaved states, the states, and the closing 1 bit.  Returns the bytes, or 0 when they do not fit in cap. */
static inline size_t QZSTD_hufFseWeights(const uint8_t *wt, uint32_t n, uint8_t *dst, size_t cap)
{
    enum { LOG = 6, SIZE = 64 };
    uint32_t cnt[16], norm[16], nextState[16], alphabet = 0u, s, u, sum = 0u, i;
    uint8_t sym[SIZE], nb[SIZE], base[SIZE];
    uint32_t st[2];
    QZSTD_hufBits bw;
    for (s = 0u; s < 16u; s++) cnt[s] = 0u;
    for (i = 0u; i < n; i++) {
        if (wt[i] > QZSTD_HUF_MAX_BITS) return 0u;
        cnt[wt[i]]++;
        if (wt[i] + 1u > alphabet) alphabet = wt[i] + 1u;
    }
    for (s = 0u; s < alphabet; s++)
        if (cnt[s] == n) return 0u;
    if (n < 2u) return 0u;
    /* the distribution: cells in proportion, at least one; the difference goes to (or comes off) the weight with the most cells */
    for (s = 0u; s < alphabet; s++) {
        norm[s] = cnt[s] ? (cnt[s] * SIZE / n ? cnt[s] * SIZE / n : 1u) : 0u;
        sum += norm[s];
    }
    while (sum != SIZE) {
        uint32_t big = 0u;
        for (s = 1u; s < alphabet; s++)
            if (norm[s] > norm[big]) big = s;
        if (sum < SIZE) {
            norm[big] += SIZE - sum;
            sum = SIZE;
        } else {
            norm[big]--;
            sum--;
        }
    }
    bw.p = dst; bw.cap = cap; bw.pos = 0u; bw.acc = 0u; bw.fill = 0u; bw.overflow = 0;
    /* NCount */
    {
        uint32_t remaining = SIZE + 1u, threshold = SIZE, nbBits = LOG + 1u, previousIs0 = 0u;
        QZSTD_hufBitsAdd(&bw, LOG - 5u, 4u);
        s = 0u;
        while (s < alphabet && remaining > 1u) {
            if (previousIs0) {
                uint32_t start = s;
                while (s < alphabet && !norm[s]) s++;
                if (s == alphabet) return 0u;
                while (s >= start + 24u) { start += 24u; QZSTD_hufBitsAdd(&bw, 0xFFFFu, 16u); }
                while (s >= start + 3u) { start += 3u; QZSTD_hufBitsAdd(&bw, 3u, 2u); }
                QZSTD_hufBitsAdd(&bw, s - start, 2u);
            }
            {
                uint32_t count = norm[s++];
                const uint32_t max = (2u * threshold - 1u) - remaining;
                remaining -= count;
                count++;
                if (count >= threshold) count += max;
                QZSTD_hufBitsAdd(&bw, count, nbBits - (count < max ? 1u : 0u));
                previousIs0 = count == 1u;
                if (remaining < 1u) return 0u;
                while (remaining < threshold) { nbBits--; threshold >>= 1; }
            }
        }
        if (remaining != 1u) return 0u;
        QZSTD_hufBitsFlush(&bw);
    }
    /* the decoder's table: cell u holds sym[u]; from it the decoder goes to cell base[u] + (nb[u] bits) */
    {
        uint32_t pos = 0u;
        for (s = 0u; s < alphabet; s++) {
            nextState[s] = norm[s];
            for (i = 0u; i < norm[s]; i++) {
                sym[pos] = (uint8_t)s;
                pos = (pos + (SIZE >> 1) + (SIZE >> 3) + 3u) & (SIZE - 1u);
            }
        }
        for (u = 0u; u < SIZE; u++) {
            const uint32_t ns = nextState[sym[u]]++;
            nb[u] = (uint8_t)(LOG - QZSTD_hufHighbit(ns));
            base[u] = (uint8_t)((ns << nb[u]) - SIZE);
        }
    }
    /* the decoder gives wt[i] from state i & 1 and then reads that state's bits; the last two weights are the states the encoder starts
     * from: the first cell of each (the one with the most bits to read, at least one: the decoder notices the end by reading past it) */
    for (i = 0u; i < 2u; i++) {
        const uint32_t w = wt[n - 2u + i];
        for (u = 0u; sym[u] != w; u++) {}
        st[(n - 2u + i) & 1u] = u;
    }
    for (i = n - 2u; i-- > 0u;) {
        const uint32_t x = st[i & 1u];
        for (u = 0u; u < SIZE; u++)
            if (sym[u] == wt[i] && base[u] <= x && x < (uint32_t)base[u] + (1u << nb[u])) break;
        if (u == SIZE) return 0u;
        QZSTD_hufBitsAdd(&bw, x - base[u], nb[u]);
        st[i & 1u] = u;
    }
    QZSTD_hufBitsAdd(&bw, st[1], LOG);
    QZSTD_hufBitsAdd(&bw, st[0], LOG);
    QZSTD_hufBitsAdd(&bw, 1u, 1u);
    QZSTD_hufBitsFlush(&bw);
    return bw.overflow ? 0u : bw.pos;
}

/* The tree description of the lengths: the weights (maxBits + 1 - nbits, 0 for a byte that does not occur) of the bytes 0 .. last - 1, `last`
 * the greatest byte that occurs — its weight is what is missing to a power of two and is never written.
 *   direct: header byte 127 + number of weights (at most 128 of them), then a nibble each, the first in the high one;
 *   FSE:    header byte = size of what follows (below 128), then QZSTD_hufFseWeights.
 * form: QZSTD_HUF_TREE_AUTO picks the smaller (the direct one when equal), the others force one.  Returns the bytes, or 0: this form (or,
 * for AUTO, either) cannot describe these lengths — no code, weights all equal with more than 128 of them, an FSE stream of 128 bytes or more. */
static inline size_t QZSTD_hufWriteTreeForm(const uint8_t nbits[256], uint8_t *dst, size_t cap, int form)
{
    uint8_t wt[256], fse[127];
    uint32_t maxBits = QZSTD_hufMaxBits(nbits), last = 0u, n, i, present = 0u;
    size_t direct = 0u, coded = 0u;
    if (!maxBits || maxBits > QZSTD_HUF_MAX_BITS) return 0u;
    for (i = 0u; i < 256u; i++)
        if (nbits[i]) { last = i; present++; }
    if (present < 2u) return 0u;
    n = last; /* weights of 0 .. last - 1 */
    for (i = 0u; i < n; i++) wt[i] = nbits[i] ? (uint8_t)(maxBits + 1u - nbits[i]) : 0u;
    if (n <= 128u && form != QZSTD_HUF_TREE_FSE) direct = 1u + (n + 1u) / 2u;
    if (n >= 2u && form != QZSTD_HUF_TREE_DIRECT) {
        coded = QZSTD_hufFseWeights(wt, n, fse, sizeof(fse));
        if (coded) coded += 1u;
    }
    if (direct && (!coded || direct <= coded)) {
        if (cap < direct) return 0u;
        dst[0] = (uint8_t)(127u + n);
        for (i = 0u; i < n; i += 2u) dst[1u + i / 2u] = (uint8_t)((wt[i] << 4) | (i + 1u < n ? wt[i + 1u] : 0u));
        return direct;
    }
    if (!coded || cap < coded) return 0u;
    dst[0] = (uint8_t)(coded - 1u);
    for (i = 0u; i + 1u < coded; i++) dst[1u + i] = fse[i];
    return coded;
}

static inline size_t QZSTD_hufWriteTree(const uint8_t nbits[256], uint8_t *dst, size_t cap)
{
    return QZSTD_hufWriteTreeForm(nbits, dst, cap, QZSTD_HUF_TREE_AUTO);
}

/* ---------------------------------------------------------------------------------------------------------------------- block body -- */

/* The content of a Compressed_Block (what follows its 3-byte Block_Header) for `len` bytes whose jump table and streams are
 * streams[0 .. streamBytes) under the lengths nbits[]:
 *   literals section header: Compressed_Literals_Block (type 2), four streams, Size_Format 2 (two 14-bit sizes, 4 bytes) for len <= 16383,
 *       else Size_Format 3 (two 18-bit sizes, 5 bytes); Regenerated_Size = len, Compressed_Size = tree + streamBytes;
 *   the tree description; the jump table and streams; the byte 0x00: no sequences.
 * Returns the bytes, or 0: len outside the limits, no tree description, no room. */
static inline size_t QZSTD_hufBlockBodyForm(const uint8_t nbits[256], uint32_t len, const uint8_t *streams, size_t streamBytes, uint8_t *dst,
                                            size_t cap, int form)
{
    uint8_t tree[QZSTD_HUF_TREE_MAX];
    size_t treeBytes, lit, head, pos, i;
    if (len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX || streamBytes < QZSTD_HUF_JUMP_BYTES + 4u) return 0u;
    treeBytes = QZSTD_hufWriteTreeForm(nbits, tree, sizeof(tree), form);
    if (!treeBytes) return 0u;
    lit = treeBytes + streamBytes;
    head = len <= 16383u ? 4u : 5u;
    if (lit > (head == 4u ? 16383u : 262143u) || cap < head + lit + 1u) return 0u;
    if (head == 4u) {
        const uint32_t h = 2u | (2u << 2) | (len << 4) | ((uint32_t)lit << 18);
        dst[0] = (uint8_t)h; dst[1] = (uint8_t)(h >> 8); dst[2] = (uint8_t)(h >> 16); dst[3] = (uint8_t)(h >> 24);
    } else {
        const uint32_t h = 2u | (3u << 2) | (len << 4) | ((uint32_t)lit << 22);
        dst[0] = (uint8_t)h; dst[1] = (uint8_t)(h >> 8); dst[2] = (uint8_t)(h >> 16); dst[3] = (uint8_t)(h >> 24);
        dst[4] = (uint8_t)(lit >> 10);
    }
    pos = head;
    for (i = 0u; i < treeBytes; i++) dst[pos++] = tree[i];
    for (i = 0u; i < streamBytes; i++) dst[pos++] = streams[i];
    dst[pos++] = 0u;
    return pos;
}

static inline size_t QZSTD_hufBlockBody(const uint8_t nbits[256], uint32_t len, const uint8_t *streams, size_t streamBytes, uint8_t *dst, size_t cap)
{
    return QZSTD_hufBlockBodyForm(nbits, len, streams, streamBytes, dst, cap, QZSTD_HUF_TREE_AUTO);
}

/* the size word of the device layer: the jump table and streams of a row are kept only when they are below len - ((len >> 6) + 2), what
 * libzstd itself demands of a Compressed block, before the tree and the headers are counted */
QZSTD_HUF_FN uint32_t QZSTD_hufSizeWord(uint32_t streamBytes, uint32_t len)
{
    if (len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX) return 0u;
    return streamBytes < len - ((len >> 6) + 2u) ? streamBytes : 0u;
}

/* ------------------------------------------------------------------------------------------------------------------------ the rule -- */

/* 1 when a block of `len` bytes is written as a Huffman-only block: streamBytes its jump table and streams (0: not coded), bodyBytes its
 * QZSTD_hufBlockBody (0: none), litBytes and count the literal bytes and the entries of its compaction header (the sequences and the
 * closing run of literals: count - 1 sequences; litBytes above len, or no entry: the matcher failed the block).  All of:
 *   - the matcher did not fail the block;
 *   - bodyBytes + (len >> 6) + 2 <= len: the gain libzstd demands of a Compressed block;
 *   - (len - litBytes) * streamBytes * 8 <= QZSTD_HUF_SEQ_EIGHTHS * (count - 1) * len: the matched bytes, priced as literals at the
 *     block's own rate, cost no more than their sequences would. */
QZSTD_HUF_FN int QZSTD_hufTakesAt(uint32_t streamBytes, uint32_t bodyBytes, uint32_t len, uint32_t litBytes, uint32_t count, uint32_t seqEighths)
{
    if (litBytes > len || count == 0u) return 0;
    if (!streamBytes || !bodyBytes || len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX) return 0;
    if ((uint64_t)bodyBytes + (len >> 6) + 2u > len) return 0;
    return (uint64_t)(len - litBytes) * streamBytes * 8u <= (uint64_t)seqEighths * (count - 1u) * len;
}

QZSTD_HUF_FN int QZSTD_hufTakes(uint32_t streamBytes, uint32_t bodyBytes, uint32_t len, uint32_t litBytes, uint32_t count)
{
    return QZSTD_hufTakesAt(streamBytes, bodyBytes, len, litBytes, count, QZSTD_HUF_SEQ_EIGHTHS);
}

#endif /* QZSTD_HUFBLOCK_H */
