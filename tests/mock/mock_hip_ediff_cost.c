/*
 * mock_hip_ediff_cost.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ediff_cost (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that QZSTD_frontAdviseDeviceBatch runs in the CPU suite: the launcher's checks in plain
 * C — the same refusals before anything is touched, tile0 filled as the launcher fills it, only d_tiles[0 .. 2 * total tiles) written —
 * and every tile's two words by the header's own QZSTD_ediffCostTile (include/qzstd_ediffcost.h).  A source of its own: a mock built
 * without it is the device layer of an older library, which must refuse the call and serve every other one.
 */
#include "qzstd_ediffcost.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gEcLaunches;
static unsigned long long gEcRows, gEcTiles;

/* test hooks */
int qzstd_mock_ediff_cost_launches(void) { return gEcLaunches; }
unsigned long long qzstd_mock_ediff_cost_rows(void) { return gEcRows; }
unsigned long long qzstd_mock_ediff_cost_tiles(void) { return gEcTiles; }

int qzstd_hip_ediff_cost(int device, void *stream, qzstd_hip_ediff_cost_row_t *rows, uint32_t nRows, qzstd_hip_ediff_cost_row_t *d_rows,
                         uint32_t *d_tiles)
{
    uint64_t total = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_tiles & 7u)) return -1;
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ediff_cost_row_t *r = &rows[i];
        if ((r->elem != 1u && r->elem != 2u && r->elem != 4u && r->elem != 8u) || r->reserved != 0u) return -1;
        if (r->len > 0xFFFFFFE0u) return -1;
        if (r->len >= r->elem && !r->src) return -1;
        total += QZSTD_HIP_ESUM_TILES(r->len, r->elem);
    }
    if (total > 0x7FFFFFFFull) return -1;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_ESUM_TILES(rows[i].len, rows[i].elem);
    }
    if (total == 0) return 0;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gEcLaunches, 1);
    __sync_fetch_and_add(&gEcRows, (unsigned long long)nRows);
    __sync_fetch_and_add(&gEcTiles, (unsigned long long)total);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ediff_cost_row_t *r = &d_rows[i];
        const unsigned char *p = (const unsigned char *)(uintptr_t)r->src;
        const uint32_t k = r->elem, n = r->len / k, T = QZSTD_EDIFF_TILE / k;
        uint32_t e0, j = 0;
        for (e0 = 0; e0 < n; e0 += T, j++)
            QZSTD_ediffCostTile(p + (size_t)e0 * k, e0 ? QZSTD_ediffElem(p + (size_t)(e0 - 1u) * k, k) : 0u, n - e0 < T ? n - e0 : T, k,
                                &d_tiles[2u * ((size_t)r->tile0 + j)]);
    }
    return 0;
}
