/*
 * mock_hip_ungroup.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ungroup (include/qzstd_hip_device.h) for the CPU stand-in of tests/mock/mock_hip.c
 * and mock_hip_device.c, so that the restore calls run in the CPU suite: the kernel's contract in plain C, written from the header's
 * definition — stage byte j * n + e of a row to byte e * k + j of its destination, the tail behind the planes unchanged, exactly the row's
 * `len` destination bytes written, the stage bytes behind `len` never looked at, the same refusals before anything is touched.  A source of
 * its own: a mock built without it is the device layer of an older library, which must refuse the restore.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gUngroupLaunches;
static unsigned long long gUngroupRows;

/* test hooks */
int qzstd_mock_ungroup_launches(void) { return gUngroupLaunches; }
unsigned long long qzstd_mock_ungroup_rows(void) { return gUngroupRows; }

int qzstd_hip_ungroup(int device, void *stream, const qzstd_hip_ungroup_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_row_t *d_rows,
                      const void *d_stage, size_t stageBytes)
{
    uint64_t end = 0, endTile = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const uint32_t k = rows[i].elem;
        if (k != 1u && k != 2u && k != 4u && k != 8u) return -1;
        if ((rows[i].srcOff & 15u) || (rows[i].len && !rows[i].dst) || rows[i].srcOff < end || rows[i].srcOff > (uint64_t)stageBytes ||
            rows[i].len > (uint64_t)stageBytes - rows[i].srcOff)
            return -1;
        end = rows[i].srcOff + (((uint64_t)rows[i].len + 15u) & ~(uint64_t)15u);
        if (rows[i].len) endTile = (rows[i].srcOff >> 14) + i + ((uint64_t)rows[i].len / k + 16384u / k - 1u) / (16384u / k) + (rows[i].len < k);
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    if (endTile && endTile - (rows[0].srcOff >> 14) > 0x7FFFFFFFull) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gUngroupLaunches, 1);
    __sync_fetch_and_add(&gUngroupRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)d_stage + r->srcOff;
        unsigned char *to = (unsigned char *)(uintptr_t)r->dst;
        const uint32_t k = r->elem, n = r->len / k;
        uint32_t p;
        for (p = 0; p < r->len; p++) {
            const uint32_t e = p / k, j = p % k;
            to[p] = from[e < n ? (uint64_t)j * n + e : p];
        }
    }
    return 0;
}
