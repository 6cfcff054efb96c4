/*
 * bytegroup_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program over qat-zstd-plugin_amd/frontend/qzstd_bytegroup.c alone (no HIP, no
 * libzstd), meant to be built with -fsanitize=address,undefined and run as a process of its own (tests/test_bytegroup_host.py):
 *   - QZSTD_byteGroup / QZSTD_byteUngroup round-trip at the edge lengths, in exact-size heap buffers (a byte too far is an ASan report);
 *   - qzbgRebuild reproduces random content from entries generated from that content, block by block of QZSTD_byteGroupBlocks;
 *   - qzbgRebuild returns non-zero, leaving the guard bytes around its output alone, for malformed entries: an offset beyond the block's
 *     start, literals short, a match past L, a missing delimiter (and a delimiter too many, an offset of 0 with a match).
 * Prints "ok" and exits 0, or says what failed and exits 1.
 */
#include "qzstd_bytegroup.h"
#include "qzstd_bytegroup_internal.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13;
    gRng ^= gRng >> 7;
    gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } } while (0)

static void roundtrip(size_t L, unsigned k)
{
    unsigned char *src = (unsigned char *)malloc(L ? L : 1), *g = (unsigned char *)malloc(L ? L : 1), *u = (unsigned char *)malloc(L ? L : 1);
    const size_t n = L / k;
    size_t i;
    for (i = 0; i < L; i++) src[i] = (unsigned char)rnd();
    CHECK(QZSTD_byteGroup(g, src, L, k) == L, "group L=%zu k=%u", L, k);
    for (i = 0; i < n * k; i++) CHECK(g[(i % k) * n + i / k] == src[i], "layout L=%zu k=%u byte %zu", L, k, i);
    for (i = n * k; i < L; i++) CHECK(g[i] == src[i], "tail L=%zu k=%u byte %zu", L, k, i);
    CHECK(QZSTD_byteUngroup(u, g, L, k) == L, "ungroup L=%zu k=%u", L, k);
    CHECK(memcmp(u, src, L) == 0, "round trip L=%zu k=%u", L, k);
    free(src); free(g); free(u);
}

/* entries for content[0, L) with the given block ends: greedy matches against the block's own history (a small hash), delimiters included;
 * literals appended to lit.  Returns the entry count. */
static size_t make_entries(const unsigned char *c, const size_t *ends, size_t nEnds, unsigned *seqs, unsigned char *lit, size_t *nLit)
{
    size_t ns = 0, nl = 0, b, start = 0;
    for (b = 0; b < nEnds; b++) {
        const size_t end = ends[b];
        size_t pos = start, anchor = start;
        static size_t head[4096];
        memset(head, 0xFF, sizeof(head));
        while (pos + 4 <= end) {
            const uint32_t h = ((uint32_t)c[pos] * 2654435761u ^ (uint32_t)c[pos + 1] * 40503u ^ (uint32_t)c[pos + 2] * 97u) & 4095u;
            const size_t cand = head[h];
            head[h] = pos;
            if (cand != (size_t)-1 && cand >= start && memcmp(c + cand, c + pos, 3) == 0) {
                size_t ml = 3;
                while (pos + ml < end && c[cand + ml] == c[pos + ml]) ml++; /* (may run over pos: an overlapping match) */
                seqs[ns * 4 + 0] = (unsigned)(pos - cand);
                seqs[ns * 4 + 1] = (unsigned)(pos - anchor);
                seqs[ns * 4 + 2] = (unsigned)ml;
                seqs[ns * 4 + 3] = 0;
                ns++;
                memcpy(lit + nl, c + anchor, pos - anchor);
                nl += pos - anchor;
                pos += ml;
                anchor = pos;
            } else {
                pos++;
            }
        }
        seqs[ns * 4 + 0] = 0;
        seqs[ns * 4 + 1] = (unsigned)(end - anchor);
        seqs[ns * 4 + 2] = 0;
        seqs[ns * 4 + 3] = 0;
        ns++;
        memcpy(lit + nl, c + anchor, end - anchor);
        nl += end - anchor;
        start = end;
    }
    *nLit = nl;
    return ns;
}

#define GUARD 64u
static unsigned char *guarded(size_t L) /* L bytes between two guards of 0xA5 */
{
    unsigned char *p = (unsigned char *)malloc(L + 2 * GUARD);
    memset(p, 0xA5, L + 2 * GUARD);
    return p;
}
static int guards_intact(const unsigned char *p, size_t L)
{
    size_t i;
    for (i = 0; i < GUARD; i++)
        if (p[i] != 0xA5 || p[GUARD + L + i] != 0xA5) return 0;
    return 1;
}

static void rebuild_cases(size_t L, unsigned k, int compressible)
{
    unsigned char *c = (unsigned char *)malloc(L ? L : 1), *lit = (unsigned char *)malloc(L ? L : 1), *out;
    unsigned *seqs, *bad;
    size_t *ends, nEnds, ns, nl, i;
    for (i = 0; i < L; i++) c[i] = compressible ? (unsigned char)("abcabcabd"[rnd() % 9] + (rnd() % 64 == 0)) : (unsigned char)rnd();
    nEnds = QZSTD_byteGroupBlocks(L, k, NULL, 0);
    CHECK(nEnds != (size_t)-1, "blocks L=%zu k=%u", L, k);
    ends = (size_t *)malloc((nEnds ? nEnds : 1) * sizeof(size_t));
    CHECK(QZSTD_byteGroupBlocks(L, k, ends, nEnds) == nEnds, "blocks twice");
    seqs = (unsigned *)malloc((L + nEnds + 1) * 4 * sizeof(unsigned));
    bad = (unsigned *)malloc((L + nEnds + 2) * 4 * sizeof(unsigned));
    ns = make_entries(c, ends, nEnds, seqs, lit, &nl);

    out = guarded(L);
    CHECK(qzbgRebuild(out + GUARD, L, seqs, ns, lit, nl, ends, nEnds) == 0, "rebuild L=%zu k=%u", L, k);
    CHECK(memcmp(out + GUARD, c, L) == 0 && guards_intact(out, L), "rebuilt content L=%zu k=%u", L, k);
    free(out);
    if (L < 64 || ns < 2) goto done;

#define EXPECT_REFUSED(what, S, NS, NL, NE)                                                           \
    do {                                                                                              \
        out = guarded(L);                                                                             \
        CHECK(qzbgRebuild(out + GUARD, L, S, NS, lit, NL, ends, NE) != 0, "%s accepted (L=%zu k=%u)", what, L, k); \
        CHECK(guards_intact(out, L), "%s: guard bytes written (L=%zu k=%u)", what, L, k);           \
        free(out);                                                                                    \
    } while (0)

    /* literals short */
    if (nl) EXPECT_REFUSED("literals short", seqs, ns, nl - 1, nEnds);
    /* a missing delimiter: the last entry gone; and the first block's delimiter turned into nothing at all */
    EXPECT_REFUSED("last delimiter missing", seqs, ns - 1, nl, nEnds);
    EXPECT_REFUSED("a block end too many", seqs, ns, nl, nEnds - 1);
    /* one delimiter too many */
    memcpy(bad, seqs, ns * 16);
    memset(bad + ns * 4, 0, 16);
    EXPECT_REFUSED("a delimiter too many", bad, ns + 1, nl, nEnds);
    /* an offset beyond the block's start: the first match of a late block reaches one byte in front of it (into the block before, or
     * in front of the buffer for a single block) */
    {
        size_t first = 0, produced = 0, blockStart = 0, pos = 0;
        int found = 0;
        for (i = 0; i < ns; i++) { /* (the first match of the last block that has one) */
            pos += seqs[i * 4 + 1];
            if (seqs[i * 4 + 2] && (!found || pos - produced != blockStart)) { first = i; produced = pos - blockStart; found = 1; }
            pos += seqs[i * 4 + 2];
            if (!seqs[i * 4 + 2]) blockStart = pos;
        }
        if (found) {
            memcpy(bad, seqs, ns * 16);
            bad[first * 4] = (unsigned)produced + 1u;
            EXPECT_REFUSED("an offset beyond the block's start", bad, ns, nl, nEnds);
            bad[first * 4] = 0xFFFFFFFFu;
            EXPECT_REFUSED("a huge offset", bad, ns, nl, nEnds);
            /* a match past L (and past its block): the last match made longer than what is left */
            memcpy(bad, seqs, ns * 16);
            for (i = ns; i-- > 0;)
                if (bad[i * 4 + 2]) { bad[i * 4 + 2] += (unsigned)L; break; }
            EXPECT_REFUSED("a match past L", bad, ns, nl, nEnds);
            memcpy(bad, seqs, ns * 16);
            for (i = ns; i-- > 0;)
                if (bad[i * 4 + 2]) { bad[i * 4 + 2] = 0xFFFFFFFFu; break; }
            EXPECT_REFUSED("a match of 4 GiB", bad, ns, nl, nEnds);
            /* an offset of 0 with a match */
            memcpy(bad, seqs, ns * 16);
            bad[first * 4] = 0;
            EXPECT_REFUSED("offset 0 with a match", bad, ns, nl, nEnds);
        } else {
            CHECK(!compressible, "compressible content without a match (L=%zu k=%u)", L, k);
        }
    }
    /* literals past the block's end: a delimiter that claims more than is left */
    memcpy(bad, seqs, ns * 16);
    bad[(ns - 1) * 4 + 1] += 1u;
    EXPECT_REFUSED("literals past L", bad, ns, nl < L ? nl + 1 : nl, nEnds);
done:
    free(c); free(lit); free(seqs); free(bad); free(ends);
}

int main(void)
{
    static const unsigned ks[] = { 1, 2, 4, 8 };
    unsigned a, b;
    for (a = 0; a < 4; a++) {
        const unsigned k = ks[a];
        const size_t Ls[] = { 0, 1, k - 1, k, k + 1, 15, 16, 17, 4095, 4096, 4097, 131072 + k + 1 };
        for (b = 0; b < sizeof(Ls) / sizeof(Ls[0]); b++) roundtrip(Ls[b], k);
        for (b = 0; b < sizeof(Ls) / sizeof(Ls[0]); b++) {
            rebuild_cases(Ls[b], k, 1);
            rebuild_cases(Ls[b], k, 0);
        }
        rebuild_cases((size_t)4096 * k + 5, k, 1);        /* planes of exactly the cut minimum: k blocks */
        rebuild_cases((size_t)3 * 131072 + 7 * k + 3, k, 1); /* planes cut again at 128 KiB */
    }
    {
        unsigned char x[4] = { 0 }, y[4];
        CHECK(QZSTD_byteGroup(y, x, 4, 3) == (size_t)-1 && QZSTD_byteUngroup(y, x, 4, 0) == (size_t)-1 && QZSTD_byteGroupBlocks(4, 16, NULL, 0) == (size_t)-1,
              "a bad element size accepted");
    }
    puts("ok");
    return 0;
}
