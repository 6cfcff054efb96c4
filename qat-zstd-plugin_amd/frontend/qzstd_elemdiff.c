/*
 * qzstd_elemdiff.c — element differences and their sum (include/qzstd_elemdiff.h).  Plain C: no HIP, no libzstd.
 */
#include "qzstd_elemdiff.h"

#include <string.h>

static int edValid(unsigned k) { return k == 1u || k == 2u || k == 4u || k == 8u; }

static unsigned long long edLoad(const unsigned char *p, unsigned k)
{
    unsigned long long v = 0;
    unsigned j;
    for (j = 0; j < k; j++) v |= (unsigned long long)p[j] << (8u * j);
    return v;
}

static void edStore(unsigned char *p, unsigned k, unsigned long long v)
{
    unsigned j;
    for (j = 0; j < k; j++) p[j] = (unsigned char)(v >> (8u * j));
}

size_t QZSTD_elemDiff(void *dst, const void *src, size_t L, unsigned k)
{
    unsigned char *d = (unsigned char *)dst;
    const unsigned char *s = (const unsigned char *)src;
    unsigned long long mask, prev = 0;
    size_t n, e;
    if (!edValid(k)) return (size_t)-1;
    mask = k == 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
    n = L / k;
    for (e = 0; e < n; e++) {
        const unsigned long long x = edLoad(s + e * k, k), diff = (x - prev) & mask;
        edStore(d + e * k, k, ((diff << 1) ^ (0ull - (diff >> (8u * k - 1u)))) & mask);
        prev = x;
    }
    if (d != s) memcpy(d + n * k, s + n * k, L - n * k);
    return L;
}

size_t QZSTD_elemSum(void *dst, const void *src, size_t L, unsigned k)
{
    unsigned char *d = (unsigned char *)dst;
    const unsigned char *s = (const unsigned char *)src;
    unsigned long long mask, sum = 0;
    size_t n, e;
    if (!edValid(k)) return (size_t)-1;
    mask = k == 8u ? ~0ull : (1ull << (8u * k)) - 1ull;
    n = L / k;
    for (e = 0; e < n; e++) {
        const unsigned long long z = edLoad(s + e * k, k);
        sum = (sum + ((z >> 1) ^ (0ull - (z & 1ull)))) & mask;
        edStore(d + e * k, k, sum);
    }
    if (d != s) memcpy(d + n * k, s + n * k, L - n * k);
    return L;
}
