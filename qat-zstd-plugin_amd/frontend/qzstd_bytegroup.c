/*
 * qzstd_bytegroup.c — the byte-grouped layout and its block rule (include/qzstd_bytegroup.h), and the executor that rebuilds a grouped
 * frame's content from its sequences and literals (qzstd_bytegroup_internal.h).  Plain C: no HIP, no libzstd.
 */
#include "qzstd_bytegroup.h"
#include "qzstd_bytegroup_internal.h"

#include <string.h>

static int bgValid(unsigned k) { return k == 1u || k == 2u || k == 4u || k == 8u; }

size_t QZSTD_byteGroup(void *dst, const void *src, size_t L, unsigned k)
{
    unsigned char *d = (unsigned char *)dst;
    const unsigned char *s = (const unsigned char *)src;
    size_t n, e;
    unsigned j;
    if (!bgValid(k)) return (size_t)-1;
    if (L == 0) return 0;
    if (k == 1u) { memcpy(d, s, L); return L; }
    n = L / k;
    for (j = 0; j < k; j++) {
        unsigned char *plane = d + (size_t)j * n;
        for (e = 0; e < n; e++) plane[e] = s[e * k + j];
    }
    memcpy(d + n * k, s + n * k, L - n * k);
    return L;
}

size_t QZSTD_byteUngroup(void *dst, const void *src, size_t L, unsigned k)
{
    unsigned char *d = (unsigned char *)dst;
    const unsigned char *s = (const unsigned char *)src;
    size_t n, e;
    unsigned j;
    if (!bgValid(k)) return (size_t)-1;
    if (L == 0) return 0;
    if (k == 1u) { memcpy(d, s, L); return L; }
    n = L / k;
    for (j = 0; j < k; j++) {
        const unsigned char *plane = s + (size_t)j * n;
        for (e = 0; e < n; e++) d[e * k + j] = plane[e];
    }
    memcpy(d + n * k, s + n * k, L - n * k);
    return L;
}

void QZSTD_byteXor(void *dst, const void *a, const void *b, size_t n)
{
    unsigned char *d = (unsigned char *)dst;
    const unsigned char *x = (const unsigned char *)a, *y = (const unsigned char *)b;
    size_t i;
    for (i = 0; i < n; i++) d[i] = (unsigned char)(x[i] ^ y[i]);
}

size_t QZSTD_byteGroupBlocks(size_t L, unsigned k, size_t *ends, size_t cap)
{
    const size_t n = bgValid(k) ? L / k : 0;
    const unsigned pieces = k > 1u && n >= QZSTD_BYTEGROUP_CUT_MIN ? k : 1u;
    size_t count = 0, start = 0;
    unsigned j;
    if (!bgValid(k)) return (size_t)-1;
    for (j = 1; j <= pieces; j++) {
        const size_t end = j == pieces ? L : ((size_t)j * n) & ~(size_t)15u;
        while (start < end) {
            start = end - start > QZSTD_BYTEGROUP_BLOCK_MAX ? start + QZSTD_BYTEGROUP_BLOCK_MAX : end;
            if (ends && count < cap) ends[count] = start;
            count++;
        }
    }
    return count;
}

int qzbgRebuild(unsigned char *out, size_t L, const unsigned *seqs, size_t nSeqs, const unsigned char *lit, size_t nLit,
                const size_t *ends, size_t nEnds)
{
    size_t pos = 0, blockStart = 0, litPos = 0, b = 0, i;
    if ((L && !out) || (nSeqs && !seqs) || (nLit && !lit) || (nEnds && !ends)) return -1;
    for (i = 0; i < nSeqs; i++) {
        const unsigned *q = seqs + i * QZBG_ENTRY_WORDS;
        const size_t off = q[0], ll = q[1], ml = q[2];
        size_t end, m;
        if (b >= nEnds) return -1; /* an entry behind the last block */
        end = ends[b];
        if (end > L || end < pos) return -1;
        if (ll > nLit - litPos || ll > end - pos) return -1;
        memcpy(out + pos, lit + litPos, ll);
        pos += ll;
        litPos += ll;
        if (off == 0 && ml == 0) { /* the block's delimiter */
            if (pos != end) return -1;
            b++;
            blockStart = pos;
            continue;
        }
        if (off == 0 || off > pos - blockStart || ml > end - pos) return -1;
        for (m = 0; m < ml; m++, pos++) out[pos] = out[pos - off]; /* (byte by byte: a match may overlap itself) */
    }
    return b == nEnds && pos == L ? 0 : -1;
}
