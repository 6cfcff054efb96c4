/*
 * mock_hip_gather.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_gather (include/qzstd_hip_device.h) for the CPU stand-in of tests/mock/mock_hip.c
 * and mock_hip_device.c, so that QZSTD_frontCompressDeviceBatch runs in the CPU suite: the kernel's contract with memcpy / memset — every
 * row copied to its place in the stage, `pad` zero bytes behind it, nothing else written, the same refusals before anything is touched.
 * A source of its own: a mock built without it is the device layer of an older library, which the batch call must refuse.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gGatherLaunches;
static unsigned long long gGatherRows;

/* test hooks */
int qzstd_mock_gather_launches(void) { return gGatherLaunches; }
unsigned long long qzstd_mock_gather_rows(void) { return gGatherRows; }

int qzstd_hip_gather(int device, void *stream, const qzstd_hip_gather_row_t *rows, uint32_t nRows, qzstd_hip_gather_row_t *d_rows,
                     void *d_stage, size_t stageBytes)
{
    uint64_t end = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const uint64_t ext = (uint64_t)rows[i].len + rows[i].pad;
        if ((rows[i].dstOff & 15u) || (ext & 15u) || (rows[i].len && !rows[i].src) || rows[i].dstOff < end ||
            rows[i].dstOff > (uint64_t)stageBytes || ext > (uint64_t)stageBytes - rows[i].dstOff)
            return -1;
        end = rows[i].dstOff + ext;
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gGatherLaunches, 1);
    __sync_fetch_and_add(&gGatherRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        unsigned char *to = (unsigned char *)d_stage + d_rows[i].dstOff;
        memcpy(to, (const void *)(uintptr_t)d_rows[i].src, d_rows[i].len);
        memset(to + d_rows[i].len, 0, d_rows[i].pad);
    }
    return 0;
}
