/*
 * ediffcost_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_ediffcost_host.py builds it with
 * -fsanitize=address,undefined, together with frontend/qzstd_elemdiff.c, and runs it as a process of its own) over
 * include/qzstd_ediffcost.h: QZSTD_ediffCostTile / QZSTD_ediffCostChunk against a naive recomputation that shares nothing with them but
 * QZSTD_planeCost — the chunk's differences by QZSTD_elemDiff (include/qzstd_elemdiff.h) over the WHOLE chunk, then per tile and per plane a
 * histogram of the bytes at offset j of every element, of the chunk and of its differences.  A wrong `prev` at a tile border, a tile cut
 * at the wrong element, a tail byte counted or a plane taken from the wrong byte each change a sum.
 *
 * Every k in {1, 2, 4, 8} x every length of kLens x six contents; every input lives in a heap block of EXACTLY its length (a read at or
 * beyond L is the sanitizer's to catch) at an odd address.  All zero: both sums are 0.  x[e] = e + 1 (an arange whose first difference is
 * the step too): the diff sum is 0.  Prints "ok".
 */
#include "qzstd_ediffcost.h"
#include "qzstd_elemdiff.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "ediffcost_check: line %d: %s (k %u, L %zu, content %u)\n", __LINE__, #c, gK, gL, gContent); exit(1); } } while (0)
static unsigned gK, gContent;
static size_t gL;

static uint32_t rnd(uint32_t *s)
{
    *s ^= *s << 13;
    *s ^= *s >> 17;
    *s ^= *s << 5;
    return *s;
}

static void put(unsigned char *p, uint64_t x, unsigned k)
{
    unsigned j;
    for (j = 0; j < k; j++) p[j] = (unsigned char)(x >> (8u * j));
}

enum { ZERO, ARANGE1, NOISE, STEPS_AT_TILES, LARGE_FIRST, DESCENDING, NCONTENT };

/* element e of the content; the tail bytes are noise */
static void fill(unsigned char *p, size_t L, unsigned k, unsigned content)
{
    const size_t n = L / k, T = 16384u / k;
    const uint64_t top = k == 8u ? ~(uint64_t)0 : ((uint64_t)1 << (8u * k)) - 1u;
    uint32_t s = 0x9E3779B9u + (uint32_t)L * 31u + k * 7u + content;
    size_t e, i;
    for (e = 0; e < n; e++) {
        uint64_t x = 0;
        switch (content) {
        case ZERO: x = 0; break;
        case ARANGE1: x = e + 1u; break;
        case NOISE: x = (uint64_t)rnd(&s) << 32 | rnd(&s); break;
        case STEPS_AT_TILES: x = 0x0123456789ABCDEFull * (uint64_t)(e / T + 1u); break; /* constant inside a tile, a jump exactly at its border */
        case LARGE_FIRST: x = e ? 5u + e % 3u : top - 1u; break;
        default: x = 1000u - 7u * (uint64_t)e; break;                                    /* wraps below zero mod 2^(8k) */
        }
        put(p + e * k, x & top, k);
    }
    for (i = n * k; i < L; i++) p[i] = content == ZERO ? 0xFFu : (unsigned char)rnd(&s); /* the tail is in no histogram */
}

static void naive(const unsigned char *p, size_t L, unsigned k, uint64_t sums[2], uint64_t *tiles)
{
    const size_t n = L / k, T = 16384u / k;
    unsigned char *z = (unsigned char *)malloc(L ? L : 1u);
    size_t t0, e;
    unsigned j;
    if (!z || QZSTD_elemDiff(z, p, L, k) != L) { fprintf(stderr, "ediffcost_check: QZSTD_elemDiff failed\n"); exit(1); }
    sums[0] = sums[1] = 0;
    *tiles = 0;
    for (t0 = 0; t0 < n; t0 += T, ++*tiles) {
        const size_t m = n - t0 < T ? n - t0 : T;
        for (j = 0; j < k; j++) {
            unsigned hx[256], hz[256];
            memset(hx, 0, sizeof(hx));
            memset(hz, 0, sizeof(hz));
            for (e = t0; e < t0 + m; e++) {
                hx[p[e * k + j]]++;
                hz[z[e * k + j]]++;
            }
            sums[0] += QZSTD_planeCost(hx, (uint32_t)m);
            sums[1] += QZSTD_planeCost(hz, (uint32_t)m);
        }
    }
    free(z);
}

int main(void)
{
    static const unsigned ks[4] = { 1u, 2u, 4u, 8u };
    unsigned a, b, c;
    for (a = 0; a < 4u; a++) {
        const unsigned k = ks[a];
        const size_t lens[10] = { 0u, k - 1u, k, k + 1u, 16384u - k, 16384u, 16384u + 1u, 16384u + k, 3u * 16384u + 5u, 131072u + 3u };
        for (b = 0; b < 10u; b++) {
            const size_t L = lens[b];
            for (c = 0; c < NCONTENT; c++) {
                unsigned char *block = (unsigned char *)malloc(L + 1u), *p = block + 1; /* odd address; ends exactly at L */
                uint64_t want[2], got[2], byTile[2] = { 0, 0 }, tiles, t;
                const size_t n = L / k, T = 16384u / k;
                gK = k; gL = L; gContent = c;
                CHECK(block);
                fill(p, L, k, c);
                naive(p, L, k, want, &tiles);
                QZSTD_ediffCostChunk(p, L, k, got);
                CHECK(got[0] == want[0] && got[1] == want[1]);
                CHECK(tiles == QZSTD_EDIFF_TILES(L, k) && tiles == QZSTD_HIP_ESUM_TILES(L, k));
                for (t = 0; t < tiles; t++) { /* the tile function with the element in front handed in, as the kernel's workgroups take it */
                    uint32_t w[2];
                    const size_t e0 = (size_t)t * T;
                    QZSTD_ediffCostTile(p + e0 * k, e0 ? QZSTD_ediffElem(p + (e0 - 1u) * k, k) : 0u, (uint32_t)(n - e0 < T ? n - e0 : T), k, w);
                    CHECK(w[0] <= 16384u + k && w[1] <= 16384u + k);
                    byTile[0] += w[0];
                    byTile[1] += w[1];
                }
                CHECK(byTile[0] == got[0] && byTile[1] == got[1]);
                if (c == ZERO) CHECK(got[0] == 0 && got[1] == 0);
                if (c == ARANGE1) CHECK(got[1] == 0 && (n < 2u || got[0] > 0));
                if (c == NOISE && n >= 16384u / k) CHECK(got[0] > n * k * 9u / 10u && got[1] > n * k * 9u / 10u); /* noise stays noise */
                if (c == STEPS_AT_TILES && n) CHECK(got[0] == 0 && (tiles < 2u || got[1] > 0));              /* only the jumps cost */
                if (n == 0) CHECK(got[0] == 0 && got[1] == 0);
                free(block);
            }
        }
    }
    /* a bad k, and an m above the tile: zeros, nothing read */
    {
        uint64_t s[2] = { 7, 7 };
        uint32_t w[2] = { 7, 7 };
        QZSTD_ediffCostChunk(NULL, 100, 3, s);
        QZSTD_ediffCostTile(NULL, 0, 16385u, 1, w);
        if (s[0] || s[1] || w[0] || w[1]) { fprintf(stderr, "ediffcost_check: a bad k or m is not 0\n"); return 1; }
        QZSTD_ediffCostChunk(NULL, 0, 4, s);
        if (s[0] || s[1]) return 1;
    }
    /* the rule: off is the default */
    if (QZSTD_ediffAdvised(0, 0) || QZSTD_ediffAdvised(1000, 1000) || QZSTD_ediffAdvised(1000, 1001) || !QZSTD_ediffAdvised(1000, 0) ||
        QZSTD_ediffAdvised(0, 1) || !QZSTD_ediffAdvised(1, 0)) {
        fprintf(stderr, "ediffcost_check: QZSTD_ediffAdvised\n");
        return 1;
    }
    {
        const uint64_t D = 1u << 20, edge = D + (D >> QZSTD_EDIFF_ADVISE_MARGIN_SHIFT);
        if (QZSTD_ediffAdvised(edge, D) || !QZSTD_ediffAdvised(edge + 1u, D)) { fprintf(stderr, "ediffcost_check: the margin\n"); return 1; }
    }
    puts("ok");
    return 0;
}
