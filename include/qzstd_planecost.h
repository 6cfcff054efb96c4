/*
 * qzstd_planecost.h — which blocks of a byte-grouped frame are noise: the order-0 cost of a block from its byte histogram, and the rule
 * that predicts a Raw_Block from it (QZSTD_frontSetPlaneProbe in qzstd_frontend_device.h).  Plain C, no GPU header, no libzstd; every
 * function is static inline and compiles for the host and inside a HIP kernel: the kernel (qzstd_hip_plane_cost), the CPU suite's mock
 * of it, the front-end and the tests all use THIS definition, so a cost is the same 32-bit word wherever it is computed.
 *
 * The cost of a block of `len` bytes whose byte b occurs hist[b] times is the size no order-0 coder — Huffman included, whatever
 * table it uses — can go below:
 *
 *     cost = ceil( sum over b of hist[b] * (L(len) - L(hist[b])) / (8 * 256) )   bytes,
 *
 * with L(x) an INTEGER approximation of 256 * log2(x) defined by QZSTD_planeLog2 below (a table, shifts, one multiply) — not by libm, so
 * there is nothing that could round differently on another machine.
 */
#ifndef QZSTD_PLANECOST_H
#define QZSTD_PLANECOST_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QZSTD_PLANECOST_FN __host__ __device__ static inline
#else
#define QZSTD_PLANECOST_FN static inline
#endif

/* the longest block a cost is defined for: a zstd block (Block_Maximum_Size) */
#define QZSTD_PLANE_LEN_MAX 131072u
/* A block shorter than this is never raw-predicted: libzstd does not try Huffman on fewer than 64 literal bytes without a table to
 * repeat, and a histogram of so few bytes over 256 bins says little.  Such a block goes the way it goes with the probe off. */
#define QZSTD_PLANE_RAW_MIN 64u
/* matchedBytes of a block the matcher failed (its compaction header has no litBytes): never raw-predicted */
#define QZSTD_PLANE_MATCH_FAILED 0xFFFFFFFFu

/* L(x) for 1 <= x <= 2^17, L(0) = 0:  e = floor(log2 x); the 16 bits below x's leading one, zero-extended, are f = 256 * hi + lo;
 * L = 256 * e + T[hi] + ((T[hi + 1] - T[hi]) * lo + 128 >> 8) with T[i] = round(256 * log2(1 + i / 256)).  For x <= 2^17 no bit of x is
 * dropped (x has at most 16 bits below its leading one, or is 2^17 itself), so |L(x) - 256 log2 x| <= 0.5 (T's rounding) + 0.5 (the
 * interpolation's) + 0.001 (the chord of log2 over 1/256): about one unit.  L is non-decreasing, and L(x << s) = L(x) + 256 s exactly. */
QZSTD_PLANECOST_FN uint32_t QZSTD_planeLog2(uint32_t x)
{
    static const uint16_t T[257] = {
          0,   1,   3,   4,   6,   7,   9,  10,  11,  13,  14,  16,  17,  18,  20,  21,
         22,  24,  25,  26,  28,  29,  30,  32,  33,  34,  36,  37,  38,  40,  41,  42,
         44,  45,  46,  47,  49,  50,  51,  52,  54,  55,  56,  57,  59,  60,  61,  62,
         63,  65,  66,  67,  68,  69,  71,  72,  73,  74,  75,  77,  78,  79,  80,  81,
         82,  84,  85,  86,  87,  88,  89,  90,  92,  93,  94,  95,  96,  97,  98,  99,
        100, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 112, 113, 114, 116, 117,
        118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133,
        134, 135, 136, 137, 138, 139, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
        150, 151, 152, 153, 154, 155, 155, 156, 157, 158, 159, 160, 161, 162, 163, 164,
        165, 166, 167, 168, 169, 169, 170, 171, 172, 173, 174, 175, 176, 177, 178, 178,
        179, 180, 181, 182, 183, 184, 185, 185, 186, 187, 188, 189, 190, 191, 192, 192,
        193, 194, 195, 196, 197, 198, 198, 199, 200, 201, 202, 203, 203, 204, 205, 206,
        207, 208, 208, 209, 210, 211, 212, 212, 213, 214, 215, 216, 216, 217, 218, 219,
        220, 220, 221, 222, 223, 224, 224, 225, 226, 227, 228, 228, 229, 230, 231, 231,
        232, 233, 234, 234, 235, 236, 237, 238, 238, 239, 240, 241, 241, 242, 243, 244,
        244, 245, 246, 247, 247, 248, 249, 249, 250, 251, 252, 252, 253, 254, 255, 255,
        256,
    };
    uint32_t z, norm, hi, lo;
    if (x == 0u) return 0u;
    z = (uint32_t)__builtin_clz(x);
    norm = x << z; /* the leading one at bit 31 */
    hi = (norm >> 23) & 0xFFu;
    lo = (norm >> 15) & 0xFFu;
    return 256u * (31u - z) + T[hi] + ((((uint32_t)T[hi + 1u] - T[hi]) * lo + 128u) >> 8);
}

/* one bin's share of the sum: c * (L(len) - L(c)) for a count 0 <= c <= len <= QZSTD_PLANE_LEN_MAX, Llen = QZSTD_planeLog2(len).
 * Below 2^17 * 4352 < 2^30. */
QZSTD_PLANECOST_FN uint32_t QZSTD_planeTerm(uint32_t c, uint32_t Llen)
{
    return c ? c * (Llen - QZSTD_planeLog2(c)) : 0u;
}

/* the sum of the 256 terms -> bytes, rounded up */
QZSTD_PLANECOST_FN uint32_t QZSTD_planeCostOfSum(uint32_t sum) { return (sum + 2047u) >> 11; }

/* The cost in bytes of a block of len <= QZSTD_PLANE_LEN_MAX bytes with the byte counts hist[] (they sum to len); 0 for len = 0.
 * The accumulator is 32 bits wide: every term is hist[b] * (L(len) - L(hist[b])) <= hist[b] * L(len), the counts sum to len, so the sum is
 * at most len * L(len) <= 131072 * 4352 = 570 425 344 < 2^32 (and stays below 2^32 up to len = 2^19).  Whoever adds the terms in another
 * order (the kernel: a tree over 256 lanes) gets the same word: unsigned addition without overflow.
 * Against the exact order-0 cost: |cost - exact| <= len / 1024 + 1 (two L values per term, about one unit each, over 2048 units a byte,
 * and the final rounding up); 256 equal counts give len exactly. */
QZSTD_PLANECOST_FN uint32_t QZSTD_planeCost(const uint32_t hist[256], uint32_t len)
{
    const uint32_t Llen = QZSTD_planeLog2(len);
    uint32_t sum = 0u, b;
    for (b = 0u; b < 256u; b++) sum += QZSTD_planeTerm(hist[b], Llen);
    return QZSTD_planeCostOfSum(sum);
}

/* 1 when the block is predicted to be a Raw_Block: what entropy coding its bytes could save at the most, (len - cost), plus what its
 * matches could (matchedBytes = len - litBytes of its compaction header; QZSTD_PLANE_MATCH_FAILED for a block the matcher failed), is
 * below the gain libzstd itself demands of a Compressed block, ZSTD_minGain = (len >> 6) + 2.  A flat histogram alone is not enough: the low
 * byte of an arange or a tiled row has one, and long repeats; its matchedBytes keep it out. */
QZSTD_PLANECOST_FN int QZSTD_planeIsRaw(uint32_t cost, uint32_t len, uint32_t matchedBytes)
{
    if (len < QZSTD_PLANE_RAW_MIN || len > QZSTD_PLANE_LEN_MAX || matchedBytes > len) return 0;
    return (len - (cost < len ? cost : len)) + matchedBytes < (len >> 6) + 2u;
}

#endif /* QZSTD_PLANECOST_H */
