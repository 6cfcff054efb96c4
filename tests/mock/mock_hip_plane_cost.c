/*
 * mock_hip_plane_cost.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_plane_cost (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that the plane probe (QZSTD_frontSetPlaneProbe) runs in the CPU suite, and the sequential
 * restatement the GPU test compares the kernel with word for word: per row a histogram of the `len` bytes at d_base + srcOff, one byte at
 * a time and inside the row only, then QZSTD_planeCost of include/qzstd_planecost.h — the kernel's own definition of the cost.  Only
 * d_cost[0 .. nRows) is written; the same refusals before anything is touched.  A source of its own: a mock built without it is the device
 * layer of an older library, which must refuse a grouped or delta call with the setting on.
 */
#include "qzstd_hip_device.h"
#include "qzstd_planecost.h"

#include <stdint.h>
#include <string.h>

static int gPlaneLaunches;
static unsigned long long gPlaneRows;

/* test hooks */
int qzstd_mock_plane_cost_launches(void) { return gPlaneLaunches; }
unsigned long long qzstd_mock_plane_cost_rows(void) { return gPlaneRows; }

int qzstd_hip_plane_cost(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                         qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost)
{
    uint32_t i, b;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_cost || nRows > 0x7FFFFFFFu) return -1;
    for (i = 0; i < nRows; i++)
        if (rows[i].len > QZSTD_PLANE_LEN_MAX || rows[i].reserved || (rows[i].len && !d_base)) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gPlaneLaunches, 1);
    __sync_fetch_and_add(&gPlaneRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const unsigned char *p = (const unsigned char *)d_base + d_rows[i].srcOff;
        uint32_t hist[256];
        memset(hist, 0, sizeof(hist));
        for (b = 0; b < d_rows[i].len; b++) hist[p[b]]++;
        d_cost[i] = QZSTD_planeCost(hist, d_rows[i].len);
    }
    return 0;
}
