/*
 * mock_hip_group_ediff.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_group_ediff (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that the differenced device calls run in the CPU suite: the launcher's checks in plain C —
 * the same refusals before anything is touched — and every row by the headers' own functions: QZSTD_elemDiff (include/qzstd_elemdiff.h)
 * for a row with the flag, then the byte-grouped layout as mock_hip_group.c writes it, the tail and `pad` zero bytes behind the planes,
 * nothing else written.  A source of its own: a mock built without it is the device layer of an older library, which must refuse the flag
 * and serve every other call.  (Built together with qat-zstd-plugin_amd/frontend/qzstd_elemdiff.c.)
 */
#include "qzstd_elemdiff.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int gEdiffLaunches;
static unsigned long long gEdiffRows;

/* test hooks */
int qzstd_mock_group_ediff_launches(void) { return gEdiffLaunches; }
unsigned long long qzstd_mock_group_ediff_rows(void) { return gEdiffRows; }

int qzstd_hip_group_ediff(int device, void *stream, const qzstd_hip_group_ediff_row_t *rows, uint32_t nRows, qzstd_hip_group_ediff_row_t *d_rows,
                          void *d_stage, size_t stageBytes)
{
    uint64_t end = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const uint64_t ext = (uint64_t)rows[i].len + rows[i].pad;
        const uint32_t k = rows[i].elem;
        if ((k != 1u && k != 2u && k != 4u && k != 8u) || (rows[i].flags & ~QZSTD_HIP_EDIFF_DIFF)) return -1;
        if ((rows[i].dstOff & 15u) || (ext & 15u) || (rows[i].len && !rows[i].src) || rows[i].dstOff < end ||
            rows[i].dstOff > (uint64_t)stageBytes || ext > (uint64_t)stageBytes - rows[i].dstOff)
            return -1;
        end = rows[i].dstOff + ext;
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gEdiffLaunches, 1);
    __sync_fetch_and_add(&gEdiffRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_group_ediff_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)(uintptr_t)r->src;
        unsigned char *to = (unsigned char *)d_stage + r->dstOff, *z = NULL;
        const uint32_t k = r->elem, n = r->len / k;
        uint32_t p;
        if ((r->flags & QZSTD_HIP_EDIFF_DIFF) && r->len) {
            if (!(z = (unsigned char *)malloc(r->len)) || QZSTD_elemDiff(z, from, r->len, k) != r->len) { free(z); return -1; }
            from = z;
        }
        for (p = 0; p < r->len; p++) {
            const uint32_t e = p / k, j = p % k;
            to[e < n ? (uint64_t)j * n + e : p] = from[p];
        }
        memset(to + r->len, 0, r->pad);
        free(z);
    }
    return 0;
}
