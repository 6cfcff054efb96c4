/*
 * planecost_check.c — TEST INFRASTRUCTURE ONLY.  include/qzstd_planecost.h alone: no HIP, no libzstd, no front-end.  Built as an
 * executable (tests/test_planecost_host.py: -fsanitize=address,undefined, run as a process of its own) it checks the header's functions on
 * the cases whose answer is an exact integer; built -shared, the three wrappers below are what the same test compares with numpy.
 */
#include "qzstd_planecost.h"

#include <stdio.h>
#include <string.h>

uint32_t pc_log2(uint32_t x) { return QZSTD_planeLog2(x); }
uint32_t pc_cost(const uint32_t hist[256], uint32_t len) { return QZSTD_planeCost(hist, len); }
int pc_is_raw(uint32_t cost, uint32_t len, uint32_t matchedBytes) { return QZSTD_planeIsRaw(cost, len, matchedBytes); }

static int failures;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main(void)
{
    uint32_t hist[256], len, b, s;
    unsigned char block[4096];
    /* L: exact at powers of two, additive under shifts, non-decreasing */
    for (s = 0; s <= 17u; s++) CHECK(QZSTD_planeLog2(1u << s) == 256u * s);
    for (b = 1; b < 512u; b++)
        for (s = 1; (b << s) <= QZSTD_PLANE_LEN_MAX; s++) CHECK(QZSTD_planeLog2(b << s) == QZSTD_planeLog2(b) + 256u * s);
    for (b = 1; b < QZSTD_PLANE_LEN_MAX; b++) CHECK(QZSTD_planeLog2(b + 1u) >= QZSTD_planeLog2(b));
    CHECK(QZSTD_planeLog2(0) == 0 && QZSTD_planeLog2(3) == 406u); /* 256 * log2(3) = 405.7 */
    /* one value, at any length: nothing to code */
    for (len = 0; len <= QZSTD_PLANE_LEN_MAX; len = len ? len * 2u : 1u) {
        memset(hist, 0, sizeof(hist));
        hist[77] = len;
        CHECK(QZSTD_planeCost(hist, len) == 0);
    }
    /* two values, half each: one bit a byte */
    memset(hist, 0, sizeof(hist));
    hist[0] = hist[255] = 4096;
    CHECK(QZSTD_planeCost(hist, 8192) == 1024);
    /* uniform over 256: eight bits a byte, exactly len — also at the longest block, where the sum is largest (2^28 here; the bound on any
     * histogram, len * L(len) = 570 425 344, is below 2^32) */
    for (len = 256; len <= QZSTD_PLANE_LEN_MAX; len *= 2u) {
        for (b = 0; b < 256u; b++) hist[b] = len / 256u;
        CHECK(QZSTD_planeCost(hist, len) == len);
    }
    /* the rule's two edges at len = 4096: minGain = 66, so a saving of 65 is raw and one of 66 is not — from the cost and from the matches */
    CHECK(QZSTD_planeIsRaw(4096 - 65, 4096, 0) == 1 && QZSTD_planeIsRaw(4096 - 66, 4096, 0) == 0);
    CHECK(QZSTD_planeIsRaw(4096, 4096, 65) == 1 && QZSTD_planeIsRaw(4096, 4096, 66) == 0);
    CHECK(QZSTD_planeIsRaw(4096 - 30, 4096, 35) == 1 && QZSTD_planeIsRaw(4096 - 30, 4096, 36) == 0);
    CHECK(QZSTD_planeIsRaw(5000, 4096, 0) == 1); /* a cost above len counts as len */
    /* never: a block below the minimum length, a failed block, a block above the maximum */
    CHECK(QZSTD_planeIsRaw(63, 63, 0) == 0 && QZSTD_planeIsRaw(64, 64, 0) == 1);
    CHECK(QZSTD_planeIsRaw(4096, 4096, QZSTD_PLANE_MATCH_FAILED) == 0);
    CHECK(QZSTD_planeIsRaw(131073, 131073, 0) == 0 && QZSTD_planeIsRaw(131072, 131072, 0) == 1);
    /* bytes 0..255 tiled: a flat histogram (cost = len), and a matcher that covers all but the first tile — matchedBytes keeps it out */
    for (b = 0; b < sizeof(block); b++) block[b] = (unsigned char)b;
    memset(hist, 0, sizeof(hist));
    for (b = 0; b < sizeof(block); b++) hist[block[b]]++;
    CHECK(QZSTD_planeCost(hist, sizeof(block)) == sizeof(block));
    CHECK(QZSTD_planeIsRaw(QZSTD_planeCost(hist, sizeof(block)), sizeof(block), sizeof(block) - 256u) == 0);
    CHECK(QZSTD_planeIsRaw(QZSTD_planeCost(hist, sizeof(block)), sizeof(block), 0) == 1); /* (the histogram alone would have said raw) */
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
