/*
 * hufblock_check.c — TEST INFRASTRUCTURE ONLY.  include/qzstd_hufblock.h alone.  Built -shared for tests/test_hufblock_host.py (which hands
 * the frames to libzstd's decoder), and as an executable of its own (main below) that runs the same inputs through every function under
 * -fsanitize=address,undefined: lengths at most 11, Kraft sum exact, streams that a decoder built from the canonical codes reads back to
 * the input, both tree forms written into buffers of exactly their size.
 */
#include "qzstd_hufblock.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- exports for the Python test ---- */

unsigned hb_lengths(const unsigned char *src, unsigned len, unsigned char nbits[256])
{
    uint32_t hist[256];
    unsigned i;
    memset(hist, 0, sizeof(hist));
    for (i = 0; i < len; i++) hist[src[i]]++;
    return QZSTD_hufLengths(hist, len, nbits);
}

unsigned hb_kraft(const unsigned char nbits[256]) { return QZSTD_hufKraft(nbits); }

/* jump table + streams -> dst; 0: not coded */
size_t hb_streams(const unsigned char *src, unsigned len, const unsigned char nbits[256], unsigned char *dst, size_t cap)
{
    uint32_t tab[256];
    QZSTD_hufCodes(nbits, tab);
    return QZSTD_hufEncodeStreams(src, len, tab, dst, cap);
}

size_t hb_tree(const unsigned char nbits[256], unsigned char *dst, size_t cap, int form) { return QZSTD_hufWriteTreeForm(nbits, dst, cap, form); }

size_t hb_body(const unsigned char nbits[256], unsigned len, const unsigned char *streams, size_t streamBytes, unsigned char *dst, size_t cap, int form)
{
    return QZSTD_hufBlockBodyForm(nbits, len, streams, streamBytes, dst, cap, form);
}

unsigned hb_size_word(unsigned streamBytes, unsigned len) { return QZSTD_hufSizeWord(streamBytes, len); }

int hb_takes(unsigned streamBytes, unsigned bodyBytes, unsigned len, unsigned litBytes, unsigned count)
{
    return QZSTD_hufTakes(streamBytes, bodyBytes, len, litBytes, count);
}

int hb_takes_at(unsigned streamBytes, unsigned bodyBytes, unsigned len, unsigned litBytes, unsigned count, unsigned seqEighths)
{
    return QZSTD_hufTakesAt(streamBytes, bodyBytes, len, litBytes, count, seqEighths);
}

unsigned hb_seq_eighths(void) { return QZSTD_HUF_SEQ_EIGHTHS; }

/* One zstd frame of one Huffman-only block for src[0 .. len): magic, a single-segment header with a 4-byte content size, the block.  The
 * size word's test is NOT applied (a block that gains nothing is still a valid one): 0 only where the header cannot write the block. */
size_t hb_frame(const unsigned char *src, unsigned len, int form, unsigned char *dst, size_t cap)
{
    unsigned char nbits[256];
    unsigned char *streams;
    size_t s, body;
    if (cap < 12u || !hb_lengths(src, len, nbits)) return 0u;
    streams = (unsigned char *)malloc((size_t)len * 2u + 64u);
    if (!streams) return 0u;
    s = hb_streams(src, len, nbits, streams, (size_t)len * 2u + 64u);
    body = s ? QZSTD_hufBlockBodyForm(nbits, len, streams, s, dst + 12u, cap - 12u, form) : 0u;
    free(streams);
    if (!body || body >= (1u << 21)) return 0u;
    dst[0] = 0x28; dst[1] = 0xB5; dst[2] = 0x2F; dst[3] = 0xFD;
    dst[4] = 0xA0; /* 4-byte Frame_Content_Size, Single_Segment, no checksum, no dictionary */
    dst[5] = (unsigned char)len; dst[6] = (unsigned char)(len >> 8); dst[7] = (unsigned char)(len >> 16); dst[8] = (unsigned char)(len >> 24);
    {
        const uint32_t h = 1u | (2u << 1) | ((uint32_t)body << 3); /* Last_Block, Compressed_Block, Block_Size */
        dst[9] = (unsigned char)h; dst[10] = (unsigned char)(h >> 8); dst[11] = (unsigned char)(h >> 16);
    }
    return 12u + body;
}

/* ---- the stand-alone checker ---- */

static uint32_t rngState = 12345u;
static uint32_t rnd(void)
{
    rngState ^= rngState << 13;
    rngState ^= rngState >> 17;
    rngState ^= rngState << 5;
    return rngState;
}

#define KINDS 8
static const char *kindName[KINDS] = { "two symbols", "256 equal counts", "fibonacci counts", "symbols 200-255", "255 and 0 present",
                                       "129 symbols", "exponent-like", "one symbol" };

static void fill(int kind, unsigned char *p, unsigned n)
{
    unsigned i;
    switch (kind) {
    case 0: for (i = 0; i < n; i++) p[i] = (rnd() & 7u) ? 3u : 250u; break;
    case 1: for (i = 0; i < n; i++) p[i] = (unsigned char)i; break;
    case 2: { /* counts 1, 1, 2, 3, 5, ... : plain Huffman is as deep as there are symbols */
        uint32_t a = 1u, b = 1u, sym = 0u, left;
        i = 0;
        while (i < n) {
            for (left = a; left && i < n; left--) p[i++] = (unsigned char)(10u + sym);
            { const uint32_t c = a + b; a = b; b = c; }
            sym++;
        }
        for (i = n; i-- > 1u;) { /* shuffled */
            const unsigned j = rnd() % (i + 1u);
            const unsigned char t = p[i]; p[i] = p[j]; p[j] = t;
        }
        break;
    }
    case 3: for (i = 0; i < n; i++) { const uint32_t r = rnd(); p[i] = (unsigned char)(200u + ((r & 15u) ? (r >> 8) % 6u : (r >> 8) % 56u)); } break;
    case 4: for (i = 0; i < n; i++) { const uint32_t r = rnd() % 10u; p[i] = r < 5u ? 0u : r < 8u ? 255u : (unsigned char)(r * 7u); } break;
    case 5: for (i = 0; i < n; i++) { const uint32_t r = rnd(); p[i] = (unsigned char)((r & 3u) ? (r >> 8) % 9u : (r >> 8) % 129u); } break;
    case 6: for (i = 0; i < n; i++) { /* a sign bit over a sum of uniform draws */
        const uint32_t r = rnd();
        p[i] = (unsigned char)(((r & 1u) << 7) | (52u + ((r >> 1) & 3u) + ((r >> 3) & 3u) + ((r >> 5) & 3u) + ((r >> 7) & 3u) + ((r >> 9) & 1u)));
    }
    break;
    default: memset(p, 61, n); break;
    }
}

/* reads jump table + streams back with a decoder built from the canonical codes alone */
static int decode_streams(const unsigned char *s, size_t size, const unsigned char nbits[256], unsigned len, unsigned char *out)
{
    uint32_t tab[256], k, b;
    size_t off = QZSTD_HUF_JUMP_BYTES;
    QZSTD_hufCodes(nbits, tab);
    for (k = 0; k < 4u; k++) {
        uint32_t st, en, i;
        size_t bytes = k < 3u ? (size_t)(s[2u * k] | (s[2u * k + 1u] << 8)) : size - off;
        long bit;
        QZSTD_hufStreamSpan(len, k, &st, &en);
        if (off + bytes > size || !bytes || !s[off + bytes - 1u]) return 0;
        bit = (long)(bytes * 8u) - 1;
        while (!((s[off + (size_t)bit / 8u] >> (bit & 7)) & 1u)) bit--;
        for (i = st; i < en; i++) { /* the first byte's code lies just below the closing bit, its first bit uppermost */
            uint32_t code = 0u, nb = 0u;
            for (;;) {
                if (--bit < 0) return 0;
                code = (code << 1) | ((s[off + (size_t)bit / 8u] >> (bit & 7)) & 1u);
                nb++;
                for (b = 0; b < 256u; b++)
                    if (tab[b] == (code | (nb << 16))) break;
                if (b < 256u) break;
                if (nb > QZSTD_HUF_MAX_BITS) return 0;
            }
            out[i] = (unsigned char)b;
        }
        if (bit != 0) return 0;
        off += bytes;
    }
    return off == size;
}

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main(void)
{
    static const unsigned lens[] = { 1024, 1025, 1026, 1027, 16383, 16384, 65536, 131072 };
    unsigned li;
    int kind;
    for (kind = 0; kind < KINDS; kind++)
        for (li = 0; li < sizeof(lens) / sizeof(lens[0]); li++) {
            const unsigned n = lens[li];
            unsigned char *src = (unsigned char *)malloc(n), *out = (unsigned char *)malloc(n), nbits[256], packed[128], again[256];
            unsigned maxBits;
            if (!src || !out) FAIL("no memory");
            fill(kind, src, n);
            maxBits = hb_lengths(src, n, nbits);
            if (kind == 7) {
                if (maxBits || hb_kraft(nbits)) FAIL("%s %u: one symbol got a code", kindName[kind], n);
            } else {
                const size_t bound = (size_t)n * 2u + 64u;
                unsigned char *streams = (unsigned char *)malloc(bound);
                size_t s, exact;
                int form;
                if (!maxBits || maxBits > QZSTD_HUF_MAX_BITS || QZSTD_hufMaxBits(nbits) != maxBits) FAIL("%s %u: depth %u", kindName[kind], n, maxBits);
                if (hb_kraft(nbits) != 2048u) FAIL("%s %u: Kraft sum %u / 2048", kindName[kind], n, hb_kraft(nbits));
                QZSTD_hufPackLengths(nbits, packed);
                QZSTD_hufUnpackLengths(packed, again);
                if (memcmp(nbits, again, 256)) FAIL("%s %u: nibbles", kindName[kind], n);
                s = hb_streams(src, n, nbits, streams, bound);
                if (!s) FAIL("%s %u: no streams", kindName[kind], n);
                /* into a buffer of exactly that size, and one byte less is refused */
                {
                    unsigned char *tight = (unsigned char *)malloc(s);
                    if (hb_streams(src, n, nbits, tight, s) != s || memcmp(tight, streams, s)) FAIL("%s %u: exact-size buffer", kindName[kind], n);
                    if (hb_streams(src, n, nbits, tight, s - 1u)) FAIL("%s %u: wrote past a short buffer", kindName[kind], n);
                    free(tight);
                }
                memset(out, 0xEE, n);
                if (!decode_streams(streams, s, nbits, n, out) || memcmp(out, src, n)) FAIL("%s %u: streams do not read back", kindName[kind], n);
                if (kind == 1 && hb_size_word((unsigned)s, n)) FAIL("%s %u: no gain, yet kept", kindName[kind], n);
                if ((kind == 0 || kind == 6) && hb_size_word((unsigned)s, n) != s) FAIL("%s %u: dropped", kindName[kind], n);
                for (form = 0; form <= 2; form++) {
                    unsigned char tree[QZSTD_HUF_TREE_MAX];
                    const size_t t = hb_tree(nbits, tree, sizeof(tree), form);
                    if (t) {
                        unsigned char *tightTree = (unsigned char *)malloc(t), *body;
                        if (hb_tree(nbits, tightTree, t, form) != t || memcmp(tightTree, tree, t)) FAIL("%s %u: tree form %d, exact-size buffer", kindName[kind], n, form);
                        if (t > 1u && hb_tree(nbits, tightTree, t - 1u, form)) FAIL("%s %u: tree form %d wrote past a short buffer", kindName[kind], n, form);
                        free(tightTree);
                        exact = (n <= 16383u ? 4u : 5u) + t + s + 1u;
                        body = (unsigned char *)malloc(exact);
                        if (hb_body(nbits, n, streams, s, body, exact, form) != exact || body[exact - 1u] != 0u) FAIL("%s %u: body form %d", kindName[kind], n, form);
                        if (hb_body(nbits, n, streams, s, body, exact - 1u, form)) FAIL("%s %u: body form %d wrote past a short buffer", kindName[kind], n, form);
                        free(body);
                    } else if (form == 0 && kind != 1) FAIL("%s %u: no tree description", kindName[kind], n);
                }
                /* symbols 0 .. 128: 128 weights, the most the direct form lists (header byte 255) */
                if (kind == 5 && n >= 16383u && (hb_tree(nbits, packed, sizeof(packed), 1) != 65u || hb_tree(nbits, packed, sizeof(packed), 2) == 0u))
                    FAIL("%s %u: 129 symbols are the direct form's edge", kindName[kind], n);
                free(streams);
            }
            free(src);
            free(out);
        }
    /* the rule's edges */
    if (hb_takes(500, 600, 1024, 0xFFFFFFFFu, 1) || hb_takes(500, 600, 1024, 1024, 0)) FAIL("a failed block is taken");
    if (!hb_takes(500, 1024 - 18, 1024, 1024, 1) || hb_takes(500, 1024 - 17, 1024, 1024, 1)) FAIL("the gain's edge");
    if (!hb_takes(512, 600, 1024, 1024 - 6, 2) || hb_takes(512, 600, 1024, 1024 - 7, 2)) FAIL("the sequence price's edge"); /* 6 * 512 * 8 = 24 * 1 * 1024 */
    if (hb_takes(100, 200, 131072, 100, 3)) FAIL("long matches are taken");
    printf("ok\n");
    return 0;
}
