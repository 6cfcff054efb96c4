/*
 * mock_hip_fingerprint.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_fingerprint (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that the fingerprint calls run in the CPU suite: the launcher's checks in plain C — the
 * same refusals before anything is touched, tile0 filled as the launcher fills it, only d_tiles[0 .. total tiles) written — and every tile
 * digest by the header's own QZSTD_fpTile (include/qzstd_fingerprint.h).  A source of its own: a mock built without it is the device layer
 * of an older library, which must refuse the two calls and serve every other one.
 */
#include "qzstd_fingerprint.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gFpLaunches;
static unsigned long long gFpRows, gFpTiles;

/* test hooks */
int qzstd_mock_fingerprint_launches(void) { return gFpLaunches; }
unsigned long long qzstd_mock_fingerprint_rows(void) { return gFpRows; }
unsigned long long qzstd_mock_fingerprint_tiles(void) { return gFpTiles; }

int qzstd_hip_fingerprint(int device, void *stream, qzstd_hip_fp_row_t *rows, uint32_t nRows, qzstd_hip_fp_row_t *d_rows, uint64_t *d_tiles)
{
    uint64_t total = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles) return -1;
    for (i = 0; i < nRows; i++) {
        if (rows[i].len && !rows[i].src) return -1;
        if (rows[i].len > 0xFFFFFFE0u) return -1;
        total += QZSTD_HIP_FP_TILES(rows[i].len);
    }
    if (total > 0x7FFFFFFFull) return -1;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_FP_TILES(rows[i].len);
    }
    if (total == 0) return 0;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gFpLaunches, 1);
    __sync_fetch_and_add(&gFpRows, (unsigned long long)nRows);
    __sync_fetch_and_add(&gFpTiles, (unsigned long long)total);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_fp_row_t *r = &d_rows[i];
        const unsigned char *p = (const unsigned char *)(uintptr_t)r->src;
        uint64_t at, j = 0;
        for (at = 0; at < r->len; at += QZSTD_FP_TILE, j++)
            d_tiles[r->tile0 + j] = QZSTD_fpTile(p + at, r->len - at < QZSTD_FP_TILE ? (uint32_t)(r->len - at) : QZSTD_FP_TILE);
    }
    return 0;
}
