/*
 * mock_hip_esum.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_esum (include/qzstd_hip_device.h) for the CPU stand-in of tests/mock/mock_hip.c and
 * mock_hip_device.c, so that the restore of differenced frames runs in the CPU suite: the launcher's checks in plain C — the same refusals
 * before anything is touched, tile0 filled as the launcher fills it — and every row by the header's own QZSTD_elemSum
 * (include/qzstd_elemdiff.h) in place over exactly [dst, dst + n * k): the tail bytes are never written.  A source of its own: a mock built
 * without it is the device layer of an older library, which must refuse the flag and serve every other call.  (Built together with
 * qat-zstd-plugin_amd/frontend/qzstd_elemdiff.c.)
 */
#include "qzstd_elemdiff.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gEsumLaunches;
static unsigned long long gEsumRows, gEsumTiles;

/* test hooks */
int qzstd_mock_esum_launches(void) { return gEsumLaunches; }
unsigned long long qzstd_mock_esum_rows(void) { return gEsumRows; }
unsigned long long qzstd_mock_esum_tiles(void) { return gEsumTiles; }

int qzstd_hip_esum(int device, void *stream, qzstd_hip_esum_row_t *rows, uint32_t nRows, qzstd_hip_esum_row_t *d_rows, void *d_scratch,
                   size_t scratchBytes)
{
    uint64_t total = 0;
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_scratch || ((uintptr_t)d_scratch & 15u)) return -1;
    for (i = 0; i < nRows; i++) {
        const uint32_t k = rows[i].elem;
        if ((k != 1u && k != 2u && k != 4u && k != 8u) || rows[i].reserved != 0u) return -1;
        if (rows[i].len > 0xFFFFFFE0u) return -1;
        if (rows[i].len >= k && !rows[i].dst) return -1;
        total += QZSTD_HIP_ESUM_TILES(rows[i].len, k);
    }
    if (total > 0x7FFFFFFFull) return -1;
    if (QZSTD_HIP_ESUM_SCRATCH_BYTES(total) > scratchBytes) return -1;
    if (total == 0) return 0;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_ESUM_TILES(rows[i].len, rows[i].elem);
    }
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gEsumLaunches, 1);
    __sync_fetch_and_add(&gEsumRows, (unsigned long long)nRows);
    __sync_fetch_and_add(&gEsumTiles, (unsigned long long)total);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_esum_row_t *r = &d_rows[i];
        unsigned char *p = (unsigned char *)(uintptr_t)r->dst;
        const size_t whole = (size_t)(r->len / r->elem) * r->elem;
        if (whole && QZSTD_elemSum(p, p, whole, r->elem) != whole) return -1;
    }
    return 0;
}
