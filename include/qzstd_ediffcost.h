/*
 * qzstd_ediffcost.h — do element differences (QZSTD_ELEM_DIFF, include/qzstd_elemdiff.h) pay for a buffer?  The order-0 cost
 * (include/qzstd_planecost.h) of every byte plane of the grouped layout, taken twice — over the elements as they are and over their
 * zigzagged differences — and the rule that advises the flag from the two sums (QZSTD_frontAdviseDeviceBatch in qzstd_frontend_device.h).
 * Plain C, no GPU header, no libzstd; every function is static inline and compiles for the host and inside a HIP kernel: the kernel
 * (qzstd_hip_ediff_cost), the CPU suite's mock of it, the front-end and the tests all use THIS definition, so a cost is the same 32-bit
 * word wherever it is computed.
 *
 * For a chunk of L bytes and k in {1, 2, 4, 8}: n = L / k, x[e] and z[e] exactly as include/qzstd_elemdiff.h defines them — x[e] the
 * little-endian unsigned k-byte integer at byte e * k, d[e] = x[e] - x[e-1] mod 2^(8k) with x[-1] = 0, z[e] = zigzag(d[e]) in k bytes;
 * differences are per chunk.  Tiles hold T = 16384 / k elements: tile t covers elements [t T, min(n, (t + 1) T)), m of them;
 * QZSTD_EDIFF_TILES(L, k) tiles, none for a chunk shorter than k; the L - n k tail bytes are in no histogram.
 *     plain(t) = sum over the planes j < k of QZSTD_planeCost(histogram of byte j of x[e] over the tile, m)
 *     diff(t)  = the same sum over byte j of z[e]; z of the tile's first element uses the last element of the tile before it
 * Each plane's cost is rounded up on its own (QZSTD_planeCostOfSum), then the plane costs are added: a tile's word is at most 16384 + k.
 *
 * What the two sums do not see: matches (the low plane of an arange costs its full length here and nearly nothing in a frame), and
 * anything between planes.  They are an estimate of what the entropy stage alone could reach.
 */
#ifndef QZSTD_EDIFFCOST_H
#define QZSTD_EDIFFCOST_H

#include <stddef.h>
#include <stdint.h>

#include "qzstd_planecost.h"

/* bytes of a chunk's elements per tile, for every k */
#define QZSTD_EDIFF_TILE 16384u
/* tiles of a chunk of `len` bytes with elements of `elem` bytes (= QZSTD_HIP_ESUM_TILES of include/qzstd_hip_device.h) */
#define QZSTD_EDIFF_TILES(len, elem) \
    (((uint64_t)(len) / (elem) + QZSTD_EDIFF_TILE / (elem) - 1u) / (QZSTD_EDIFF_TILE / (elem)))
/* Differences are advised when D + (D >> QZSTD_EDIFF_ADVISE_MARGIN_SHIFT) < P.  The largest shift of {4, 3, 2, 1} — the smallest margin —
 * under which, over every input of tests/golden/advise_sizes.json, no input is advised whose differenced frames are not smaller at level 1
 * and at level 6, and the ordered inputs are advised (tools/advise_ratio.py). */
#define QZSTD_EDIFF_ADVISE_MARGIN_SHIFT 4u

/* the little-endian k-byte integer at p, any alignment */
QZSTD_PLANECOST_FN uint64_t QZSTD_ediffElem(const unsigned char *p, uint32_t k)
{
    uint64_t x = 0;
    uint32_t j;
    for (j = 0; j < k; j++) x |= (uint64_t)p[j] << (8u * j);
    return x;
}

/* zigzag(x - prev) in k bytes */
QZSTD_PLANECOST_FN uint64_t QZSTD_ediffZigzag(uint64_t x, uint64_t prev, uint32_t k)
{
    const uint64_t mask = k == 8u ? ~(uint64_t)0 : ((uint64_t)1 << (8u * k)) - 1u;
    const uint64_t d = (x - prev) & mask;
    return ((d << 1) ^ ((uint64_t)0 - (d >> (8u * k - 1u)))) & mask;
}

/* One tile: m <= 16384 / k elements of k bytes at p (any alignment), `prev` the element in front of them (0 at the chunk's start):
 * out[0] = plain, out[1] = diff.  k outside {1, 2, 4, 8} or m above the tile: both 0. */
QZSTD_PLANECOST_FN void QZSTD_ediffCostTile(const unsigned char *p, uint64_t prev, uint32_t m, uint32_t k, uint32_t out[2])
{
    uint32_t j;
    out[0] = out[1] = 0u;
    if ((k != 1u && k != 2u && k != 4u && k != 8u) || m > QZSTD_EDIFF_TILE / k) return;
    for (j = 0; j < k; j++) { /* a plane at a time: two histograms on the stack, not sixteen */
        uint32_t hx[256], hz[256], e, b;
        uint64_t last = prev;
        for (b = 0; b < 256u; b++) hx[b] = hz[b] = 0u;
        for (e = 0; e < m; e++) {
            const uint64_t x = QZSTD_ediffElem(p + (size_t)e * k, k);
            hx[(x >> (8u * j)) & 0xFFu]++;
            hz[(QZSTD_ediffZigzag(x, last, k) >> (8u * j)) & 0xFFu]++;
            last = x;
        }
        out[0] += QZSTD_planeCost(hx, m);
        out[1] += QZSTD_planeCost(hz, m);
    }
}

/* A chunk: sums[0] = the sum of plain(t), sums[1] = the sum of diff(t) over the chunk's tiles; both 0 for a chunk without a tile or a bad k */
QZSTD_PLANECOST_FN void QZSTD_ediffCostChunk(const void *chunk, size_t L, uint32_t k, uint64_t sums[2])
{
    const unsigned char *p = (const unsigned char *)chunk;
    size_t n, T, e0;
    sums[0] = sums[1] = 0u;
    if (k != 1u && k != 2u && k != 4u && k != 8u) return;
    n = L / k;
    T = QZSTD_EDIFF_TILE / k;
    for (e0 = 0; e0 < n; e0 += T) {
        uint32_t w[2];
        QZSTD_ediffCostTile(p + e0 * k, e0 ? QZSTD_ediffElem(p + (e0 - 1u) * k, k) : 0u, (uint32_t)(n - e0 < T ? n - e0 : T), k, w);
        sums[0] += w[0];
        sums[1] += w[1];
    }
}

/* 1 when differences are advised for summed costs P (plain) and D (diff).  P == D, both 0 included, gives 0: off is the default. */
QZSTD_PLANECOST_FN int QZSTD_ediffAdvised(uint64_t P, uint64_t D) { return D + (D >> QZSTD_EDIFF_ADVISE_MARGIN_SHIFT) < P; }

#endif /* QZSTD_EDIFFCOST_H */
