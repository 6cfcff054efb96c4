/*
 * mock_hip_ungroup_window.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ungroup_window (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that QZSTD_frontRestoreDeviceSlices runs in the CPU suite: the kernel's contract in plain C,
 * written from the header's definition — with u[e * k + j] = stage byte j * n + e of the row's frame (the tail unchanged), byte winOff + i of
 * u[], XORed with byte i of the row's base, to byte i of its destination; exactly the row's `winLen` destination bytes written, every base
 * byte read before the destination byte of the same offset is written (base == dst: in place), tile0 filled as the launcher fills it, the
 * same refusals before anything is touched.  A source of its own: a mock built without it is the device layer of an older library, which
 * must refuse the slices call.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gUngroupWindowLaunches;
static unsigned long long gUngroupWindowRows;

/* test hooks */
int qzstd_mock_ungroup_window_launches(void) { return gUngroupWindowLaunches; }
unsigned long long qzstd_mock_ungroup_window_rows(void) { return gUngroupWindowRows; }

/* workgroups of a row: the frame's tiles (16 KiB of u[], the tail with the last one) that its window intersects */
static uint64_t rowTiles(const qzstd_hip_ungroup_win_row_t *r)
{
    const uint64_t n = r->len / r->elem, tileMax = 16384u / r->elem, tiles = n ? (n + tileMax - 1u) / tileMax : 1u;
    uint64_t a, b;
    if (!r->winLen) return 0;
    a = r->winOff >> 14;
    b = ((uint64_t)r->winOff + r->winLen - 1u) >> 14;
    if (a > tiles - 1u) a = tiles - 1u;
    if (b > tiles - 1u) b = tiles - 1u;
    return b - a + 1u;
}

int qzstd_hip_ungroup_window(int device, void *stream, qzstd_hip_ungroup_win_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_win_row_t *d_rows,
                             const void *d_stage, size_t stageBytes)
{
    uint64_t end = 0, total = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_win_row_t *r = &rows[i];
        const uint32_t k = r->elem;
        if (k != 1u && k != 2u && k != 4u && k != 8u) return -1;
        if (r->reserved || (r->srcOff & 15u) || r->len > 0xFFFFFFE0u || (uint64_t)r->winOff + r->winLen > r->len || (r->winLen && !r->dst)) return -1;
        if (i && r->srcOff == rows[i - 1].srcOff) {
            if (r->len != rows[i - 1].len || k != rows[i - 1].elem || r->winOff < (uint64_t)rows[i - 1].winOff + rows[i - 1].winLen) return -1;
        } else if (r->srcOff < end) {
            return -1;
        }
        if (r->srcOff > (uint64_t)stageBytes || r->len > (uint64_t)stageBytes - r->srcOff) return -1;
        end = r->srcOff + (((uint64_t)r->len + 15u) & ~(uint64_t)15u);
        total += rowTiles(r);
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    if (total > 0x7FFFFFFFull) return -1;
    if (total == 0) return 0;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += rowTiles(&rows[i]);
    }
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gUngroupWindowLaunches, 1);
    __sync_fetch_and_add(&gUngroupWindowRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_win_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)d_stage + r->srcOff, *base = (const unsigned char *)(uintptr_t)r->base;
        unsigned char *to = (unsigned char *)(uintptr_t)r->dst;
        const uint32_t k = r->elem, n = r->len / k;
        uint32_t w;
        for (w = 0; w < r->winLen; w++) {
            const uint32_t p = r->winOff + w, e = p / k, j = p % k;
            to[w] = (unsigned char)(from[e < n ? (uint64_t)j * n + e : p] ^ (base ? base[w] : 0));
        }
    }
    return 0;
}
