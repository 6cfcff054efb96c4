/*
 * mock_hip_ungroup_cmp.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ungroup_cmp (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that QZSTD_frontVerifyDeviceBatch runs in the CPU suite: the kernel's definition in plain C,
 * written from the header — with u[e * k + j] = stage byte j * n + e of the row's frame (the tail unchanged; all zeros for a ZERO row, whose
 * stage is never touched), the row matches when u[i] ^ base[i] == ref[i] for every i < len; one word per 16 KiB tile of u[] (the tail with
 * the last tile, a frame shorter than an element one tile, none for an empty row): QZSTD_HIP_CMP_SAME, or the lowest differing row offset of
 * the tile; tile0 filled as the launcher fills it, the same refusals before anything is touched.  Nothing but d_rows and the tile words is
 * written.  A source of its own: a mock built without it is the device layer of an older library, which must refuse the verify call.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gCmpLaunches;
static unsigned long long gCmpRows, gCmpZeroRows, gCmpStageBytes;

/* test hooks */
int qzstd_mock_ungroup_cmp_launches(void) { return gCmpLaunches; }
unsigned long long qzstd_mock_ungroup_cmp_rows(void) { return gCmpRows; }
unsigned long long qzstd_mock_ungroup_cmp_zero_rows(void) { return gCmpZeroRows; }
unsigned long long qzstd_mock_ungroup_cmp_stage_bytes(void) { return gCmpStageBytes; } /* the sum of the launches' stageBytes */

int qzstd_hip_ungroup_cmp(int device, void *stream, qzstd_hip_ungroup_cmp_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_cmp_row_t *d_rows,
                          const void *d_stage, size_t stageBytes, uint32_t *d_tiles)
{
    uint64_t end = 0, total = 0, zeros = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_stage & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_cmp_row_t *r = &rows[i];
        const uint32_t k = r->elem;
        if (k != 1u && k != 2u && k != 4u && k != 8u) return -1;
        if ((r->flags & ~QZSTD_HIP_CMP_ZERO) || r->len > 0xFFFFFFE0u || (r->len && !r->ref)) return -1;
        if (!(r->flags & QZSTD_HIP_CMP_ZERO)) {
            if ((r->srcOff & 15u) || (r->len && !d_stage) || r->srcOff < end) return -1;
            if (r->srcOff > (uint64_t)stageBytes || r->len > (uint64_t)stageBytes - r->srcOff) return -1;
            end = r->srcOff + (((uint64_t)r->len + 15u) & ~(uint64_t)15u);
        } else {
            zeros++;
        }
        total += QZSTD_HIP_CMP_TILES(r->len, k);
    }
    if (total > 0x7FFFFFFFull) return -1;
    if (total == 0) return 0;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_CMP_TILES(rows[i].len, rows[i].elem);
    }
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gCmpLaunches, 1);
    __sync_fetch_and_add(&gCmpRows, (unsigned long long)nRows);
    __sync_fetch_and_add(&gCmpZeroRows, (unsigned long long)zeros);
    __sync_fetch_and_add(&gCmpStageBytes, (unsigned long long)stageBytes);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_cmp_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)d_stage + r->srcOff, *base = (const unsigned char *)(uintptr_t)r->base;
        const unsigned char *ref = (const unsigned char *)(uintptr_t)r->ref;
        const uint32_t k = r->elem, n = r->len / k, tiles = (uint32_t)QZSTD_HIP_CMP_TILES(r->len, k);
        uint32_t t, p;
        for (t = 0; t < tiles; t++) d_tiles[r->tile0 + t] = QZSTD_HIP_CMP_SAME;
        for (p = r->len; p-- > 0;) { /* downwards: the lowest differing offset of a tile is stored last */
            const uint32_t e = p / k, j = p % k;
            const unsigned char u = (r->flags & QZSTD_HIP_CMP_ZERO) ? 0 : from[e < n ? (uint64_t)j * n + e : p];
            if ((unsigned char)(u ^ (base ? base[p] : 0)) != ref[p]) d_tiles[r->tile0 + ((p >> 14) < tiles ? (p >> 14) : tiles - 1u)] = p;
        }
    }
    return 0;
}
