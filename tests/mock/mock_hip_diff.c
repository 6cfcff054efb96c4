/*
 * mock_hip_diff.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_diff (include/qzstd_hip_device.h) for the CPU stand-in of tests/mock/mock_hip.c and
 * mock_hip_device.c, so that the delta calls' skip of unchanged chunks runs in the CPU suite: the kernel's contract in plain C, written from
 * the header's definition — flag i is 1 when any of the row's `len` bytes at a and b differ and 0 otherwise, an empty row gives 0, only
 * d_flags[0 .. nRows) written, tile0 filled as the launcher fills it, the same refusals before anything is touched.  A source of its own: a
 * mock built without it is the device layer of an older library, which must refuse a delta call with the setting on.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gDiffLaunches;
static unsigned long long gDiffRows;

/* test hooks */
int qzstd_mock_diff_launches(void) { return gDiffLaunches; }
unsigned long long qzstd_mock_diff_rows(void) { return gDiffRows; }

int qzstd_hip_diff(int device, void *stream, qzstd_hip_diff_row_t *rows, uint32_t nRows, qzstd_hip_diff_row_t *d_rows, uint32_t *d_flags)
{
    uint64_t total = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_flags) return -1;
    for (i = 0; i < nRows; i++) {
        if (rows[i].len && (!rows[i].a || !rows[i].b)) return -1;
        if (rows[i].len > 0xFFFFFFE0u) return -1;
        total += ((uint64_t)rows[i].len + 16383u) >> 14;
    }
    if (total > 0x7FFFFFFFull) return -1;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += ((uint64_t)rows[i].len + 16383u) >> 14;
    }
    memset(d_flags, 0, (size_t)nRows * sizeof(uint32_t));
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gDiffLaunches, 1);
    __sync_fetch_and_add(&gDiffRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_diff_row_t *r = &d_rows[i];
        if (r->len && memcmp((const void *)(uintptr_t)r->a, (const void *)(uintptr_t)r->b, r->len) != 0) d_flags[i] = 1u;
    }
    return 0;
}
