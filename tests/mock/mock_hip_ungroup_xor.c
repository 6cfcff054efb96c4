/*
 * mock_hip_ungroup_xor.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ungroup_xor (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that the delta restore call runs in the CPU suite: the kernel's contract in plain C,
 * written from the header's definition — stage byte j * n + e of a row, XORed with byte e * k + j of the row's base, to byte e * k + j of its
 * destination; a row with base 0 as mock_hip_ungroup.c's; exactly the row's `len` destination bytes written, every base byte read before
 * the destination byte of the same offset is written (base == dst: in place), the same refusals before anything is touched.  A source of
 * its own: a mock built without it is the device layer of an older library, which must refuse a call with a base.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gUngroupXorLaunches;
static unsigned long long gUngroupXorRows;

/* test hooks */
int qzstd_mock_ungroup_xor_launches(void) { return gUngroupXorLaunches; }
unsigned long long qzstd_mock_ungroup_xor_rows(void) { return gUngroupXorRows; }

int qzstd_hip_ungroup_xor(int device, void *stream, const qzstd_hip_ungroup_xor_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_xor_row_t *d_rows,
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
    __sync_fetch_and_add(&gUngroupXorLaunches, 1);
    __sync_fetch_and_add(&gUngroupXorRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_xor_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)d_stage + r->srcOff, *base = (const unsigned char *)(uintptr_t)r->base;
        unsigned char *to = (unsigned char *)(uintptr_t)r->dst;
        const uint32_t k = r->elem, n = r->len / k;
        uint32_t p;
        for (p = 0; p < r->len; p++) {
            const uint32_t e = p / k, j = p % k;
            to[p] = (unsigned char)(from[e < n ? (uint64_t)j * n + e : p] ^ (base ? base[p] : 0));
        }
    }
    return 0;
}
