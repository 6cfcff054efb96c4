/*
 * elemdiff_check.c — include/qzstd_elemdiff.h on its own, built with the sanitizers by tests/test_elemdiff_host.py: round trips out of place
 * and in place at every element size, length and start alignment, guard bytes around every buffer, tails untouched, hand-worked vectors,
 * bad element sizes.  Prints "ok".
 */
#include "qzstd_elemdiff.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define GUARD 32u

static unsigned long long rngState = 0x9E3779B97F4A7C15ull;
static unsigned rnd(void)
{
    rngState ^= rngState << 13;
    rngState ^= rngState >> 7;
    rngState ^= rngState << 17;
    return (unsigned)(rngState >> 24);
}

static int fails;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); fails++; }     \
    } while (0)

static int guards_ok(const unsigned char *p, size_t L)
{
    size_t i;
    for (i = 0; i < GUARD; i++)
        if (p[i] != 0xC3 || p[GUARD + L + i] != 0xC3) return 0;
    return 1;
}

static void fill(unsigned char *x, size_t L, unsigned k, int kind)
{
    size_t i;
    for (i = 0; i < L; i++) {
        switch (kind) {
        case 0: x[i] = (unsigned char)rnd(); break;
        case 1: x[i] = 0xFF; break;
        case 2: x[i] = (unsigned char)(i % k == 0 ? 255u - (i / k) % 256u : 0xF0u - (i / k / 256u) % 16u); break; /* descending */
        default: x[i] = (unsigned char)((i / k) % 2 ? 0xFF : 0x00); break;                                      /* 0, max, 0, ... */
        }
    }
}

static void round_trip(size_t L, unsigned k, int kind, unsigned skew)
{
    unsigned char *x = (unsigned char *)malloc(L + 2 * GUARD + 8), *z = (unsigned char *)malloc(L + 2 * GUARD + 8),
                  *y = (unsigned char *)malloc(L + 2 * GUARD + 8);
    unsigned char *xs = x + skew, *zs = z + (skew + 1u) % 8u, *ys = y + (skew + 3u) % 8u;
    const size_t n = L / k;
    if (!x || !z || !y) abort();
    memset(xs, 0xC3, L + 2 * GUARD);
    memset(zs, 0xC3, L + 2 * GUARD);
    memset(ys, 0xC3, L + 2 * GUARD);
    fill(xs + GUARD, L, k, kind);
    CHECK(QZSTD_elemDiff(zs + GUARD, xs + GUARD, L, k) == L);
    CHECK(guards_ok(zs, L));
    CHECK(memcmp(zs + GUARD + n * k, xs + GUARD + n * k, L - n * k) == 0); /* the tail: copied unchanged */
    CHECK(QZSTD_elemSum(ys + GUARD, zs + GUARD, L, k) == L);
    CHECK(guards_ok(ys, L));
    CHECK(memcmp(ys + GUARD, xs + GUARD, L) == 0);
    /* in place, both ways */
    memcpy(ys + GUARD, xs + GUARD, L);
    CHECK(QZSTD_elemDiff(ys + GUARD, ys + GUARD, L, k) == L);
    CHECK(memcmp(ys + GUARD, zs + GUARD, L) == 0);
    CHECK(QZSTD_elemSum(ys + GUARD, ys + GUARD, L, k) == L);
    CHECK(memcmp(ys + GUARD, xs + GUARD, L) == 0 && guards_ok(ys, L));
    free(x);
    free(z);
    free(y);
}

int main(void)
{
    static const unsigned ks[4] = { 1, 2, 4, 8 };
    static const unsigned bad[] = { 0, 3, 5, 6, 7, 9, 16, 0x81 };
    unsigned a, i;
    int kind;
    for (a = 0; a < 4; a++) {
        const unsigned k = ks[a];
        const size_t Ls[] = { 0, 1, k - 1, k, k + 1, 16384 - k, 16384, 16384 + k, 100003 };
        for (i = 0; i < sizeof(Ls) / sizeof(Ls[0]); i++)
            for (kind = 0; kind < 4; kind++) round_trip(Ls[i], k, kind, (unsigned)(i + (unsigned)kind) % 8u);
    }
    { /* k = 2, x = {1, 0, 0xFFFF} -> d = {1, -1, -1} -> z = {2, 1, 1}; one tail byte */
        const unsigned char x[7] = { 1, 0, 0, 0, 0xFF, 0xFF, 0x77 }, want[7] = { 2, 0, 1, 0, 1, 0, 0x77 };
        unsigned char z[7], y[7];
        CHECK(QZSTD_elemDiff(z, x, 7, 2) == 7 && memcmp(z, want, 7) == 0);
        CHECK(QZSTD_elemSum(y, z, 7, 2) == 7 && memcmp(y, x, 7) == 0);
    }
    { /* k = 1, x = {0, 255, 0, 128}: d = {0, -1, +1, -128} -> z = {0, 1, 2, 255} */
        const unsigned char x[4] = { 0, 255, 0, 128 }, want[4] = { 0, 1, 2, 255 };
        unsigned char z[4];
        CHECK(QZSTD_elemDiff(z, x, 4, 1) == 4 && memcmp(z, want, 4) == 0);
    }
    { /* k = 8, x = {2^63, 0}: d = {-2^63, -2^63 (mod 2^64)} -> z = {2^64 - 1, 2^64 - 1} */
        unsigned char x[16] = { 0 }, z[16], y[16];
        x[7] = 0x80;
        CHECK(QZSTD_elemDiff(z, x, 16, 8) == 16);
        for (i = 0; i < 16; i++) CHECK(z[i] == 0xFF);
        CHECK(QZSTD_elemSum(y, z, 16, 8) == 16 && memcmp(y, x, 16) == 0);
    }
    for (i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) {
        unsigned char x[8] = { 1, 2, 3, 4, 5, 6, 7, 8 }, z[8] = { 9, 9, 9, 9, 9, 9, 9, 9 };
        CHECK(QZSTD_elemDiff(z, x, 8, bad[i]) == (size_t)-1 && QZSTD_elemSum(z, x, 8, bad[i]) == (size_t)-1);
        CHECK(z[0] == 9 && z[7] == 9);
    }
    if (fails) return 1;
    puts("ok");
    return 0;
}
