/*
 * qzstd_fingerprint.h — a 64-bit fingerprint of a byte range that is PARALLEL BY CONSTRUCTION: what QZSTD_frontFingerprintDeviceBatch and
 * QZSTD_frontCheckDeviceBatch (qzstd_frontend_device.h) compute per chunk of a device buffer, so that a restore can be checked at load time
 * against 8 bytes kept per frame.  Plain C, no GPU header, no libzstd; every function is static inline and compiles for the host and inside
 * a HIP kernel: the kernel (qzstd_hip_fingerprint), the CPU suite's mock of it, the front-end and the tests all use THIS definition, so a
 * fingerprint is the same 64-bit word wherever it is computed.  It is NOT XXH64 and has no wire format: nothing stores it but the caller.
 *
 * The pieces are XXH64's published ones (the five primes, the round, the merge, the final avalanche); the arrangement is the coalesced access
 * of a 256-lane workgroup instead of four serial chains:
 *
 *   round(acc, in) = rotl(acc + in * P2, 31) * P1          merge(h, v) = (h ^ round(0, v)) * P1 + P4
 *
 * TILE (QZSTD_fpTile): n bytes, 0 < n <= 16384, read as 16-byte little-endian words, bytes at or beyond n read as 0.  256 lanes; lane t
 * starts at acc_t = P5 + t * P1 and takes the words w = t, t + 256, t + 512, t + 768 that start below n, in that order:
 * acc_t = round(round(acc_t, lo64(word w)), hi64(word w)).  The lanes are folded by a fixed binary tree: for s = 1, 2, 4, ..., 128 and every
 * t that is a multiple of 2 s, acc_t = merge(acc_t, acc_{t+s}).  The digest is acc_0.  A lane without a word keeps its start value and is
 * merged all the same, so the tree's shape never depends on n.
 *
 * ROW (QZSTD_fpFold / QZSTD_fingerprint): the row is cut into 16 KiB tiles from its start; h = P5 + len, then h = merge(h, tile_j) for
 * every tile in order, and the fingerprint is avalanche(h).  len == 0: avalanche(P5).
 *
 * Nothing here commutes: the round is a rotate between two odd multiplies (words of one lane), the merge treats its two sides differently
 * (lanes, tiles), every lane starts from another value, and the length is mixed in — so swapped words, swapped lanes, swapped tiles and an
 * appended zero byte all change the value.  It is a check against mistakes (a wrong base, a wrong element size, frames out of order), not
 * against an adversary.
 */
#ifndef QZSTD_FINGERPRINT_H
#define QZSTD_FINGERPRINT_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QZSTD_FP_FN __host__ __device__ static inline
#else
#define QZSTD_FP_FN static inline
#endif

#define QZSTD_FP_TILE_LOG 14u
#define QZSTD_FP_TILE (1u << QZSTD_FP_TILE_LOG) /* bytes of a row per tile digest */
#define QZSTD_FP_LANES 256u                     /* lanes of a tile: a lane takes up to four 16-byte words */
/* tile digests of a row of len bytes */
#define QZSTD_FP_TILES(len) (((uint64_t)(len) + (QZSTD_FP_TILE - 1u)) >> QZSTD_FP_TILE_LOG)

#define QZSTD_FP_P1 0x9E3779B185EBCA87ull
#define QZSTD_FP_P2 0xC2B2AE3D27D4EB4Full
#define QZSTD_FP_P3 0x165667B19E3779F9ull
#define QZSTD_FP_P4 0x85EBCA77C2B2AE63ull
#define QZSTD_FP_P5 0x27D4EB2F165667C5ull

QZSTD_FP_FN uint64_t QZSTD_fpRound(uint64_t acc, uint64_t in)
{
    acc += in * QZSTD_FP_P2;
    acc = (acc << 31) | (acc >> 33);
    return acc * QZSTD_FP_P1;
}

QZSTD_FP_FN uint64_t QZSTD_fpMerge(uint64_t h, uint64_t v) { return (h ^ QZSTD_fpRound(0ull, v)) * QZSTD_FP_P1 + QZSTD_FP_P4; }

QZSTD_FP_FN uint64_t QZSTD_fpAvalanche(uint64_t h)
{
    h ^= h >> 33;
    h *= QZSTD_FP_P2;
    h ^= h >> 29;
    h *= QZSTD_FP_P3;
    h ^= h >> 32;
    return h;
}

/* lane t's start value */
QZSTD_FP_FN uint64_t QZSTD_fpLaneInit(uint32_t t) { return QZSTD_FP_P5 + (uint64_t)t * QZSTD_FP_P1; }

/* one 16-byte word into its lane: the low 8 bytes (little-endian), then the high 8 */
QZSTD_FP_FN uint64_t QZSTD_fpWord(uint64_t acc, uint64_t lo, uint64_t hi) { return QZSTD_fpRound(QZSTD_fpRound(acc, lo), hi); }

/* the 8 bytes at p + at of a range of n bytes, little-endian, bytes at or beyond n read as 0 */
QZSTD_FP_FN uint64_t QZSTD_fpLoad64(const unsigned char *p, uint32_t at, uint32_t n)
{
    uint64_t v = 0ull;
    uint32_t i;
    for (i = 0u; i < 8u && at + i < n; i++) v |= (uint64_t)p[at + i] << (8u * i);
    return v;
}

/* the digest of a tile: n bytes at p, 0 < n <= QZSTD_FP_TILE (the header's definition, lane after lane) */
QZSTD_FP_FN uint64_t QZSTD_fpTile(const void *p, uint32_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t acc[QZSTD_FP_LANES];
    uint32_t t, k, s;
    for (t = 0u; t < QZSTD_FP_LANES; t++) {
        acc[t] = QZSTD_fpLaneInit(t);
        for (k = 0u; k < 4u; k++) {
            const uint32_t w = t + QZSTD_FP_LANES * k;
            if (16u * w < n) acc[t] = QZSTD_fpWord(acc[t], QZSTD_fpLoad64(b, 16u * w, n), QZSTD_fpLoad64(b, 16u * w + 8u, n));
        }
    }
    for (s = 1u; s < QZSTD_FP_LANES; s <<= 1)
        for (t = 0u; t < QZSTD_FP_LANES; t += 2u * s) acc[t] = QZSTD_fpMerge(acc[t], acc[t + s]);
    return acc[0];
}

/* the fingerprint of a row of len bytes from its nTiles = QZSTD_FP_TILES(len) tile digests */
QZSTD_FP_FN uint64_t QZSTD_fpFold(const uint64_t *tiles, size_t nTiles, uint64_t len)
{
    uint64_t h = QZSTD_FP_P5 + len;
    size_t j;
    for (j = 0; j < nTiles; j++) h = QZSTD_fpMerge(h, tiles[j]);
    return QZSTD_fpAvalanche(h);
}

/* the fingerprint of len bytes at p */
QZSTD_FP_FN uint64_t QZSTD_fingerprint(const void *p, size_t len)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = QZSTD_FP_P5 + (uint64_t)len;
    size_t at;
    for (at = 0; at < len; at += QZSTD_FP_TILE)
        h = QZSTD_fpMerge(h, QZSTD_fpTile(b + at, len - at < QZSTD_FP_TILE ? (uint32_t)(len - at) : QZSTD_FP_TILE));
    return QZSTD_fpAvalanche(h);
}

#endif /* QZSTD_FINGERPRINT_H */
