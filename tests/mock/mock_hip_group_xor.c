/*
 * mock_hip_group_xor.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_group_xor (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that the delta compress call runs in the CPU suite: the kernel's contract in plain C,
 * written from the header's definition — byte j of element e of src ^ base to stage byte j * n + e of the row, the tail and `pad` zero bytes
 * behind the planes, a row with base 0 as mock_hip_group.c's, the base only read, the same refusals before anything is touched.  A source
 * of its own: a mock built without it is the device layer of an older library, which must refuse a call with a base.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

static int gGroupXorLaunches;
static unsigned long long gGroupXorRows;

/* test hooks */
int qzstd_mock_group_xor_launches(void) { return gGroupXorLaunches; }
unsigned long long qzstd_mock_group_xor_rows(void) { return gGroupXorRows; }

int qzstd_hip_group_xor(int device, void *stream, const qzstd_hip_group_xor_row_t *rows, uint32_t nRows, qzstd_hip_group_xor_row_t *d_rows,
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
        if ((k != 1u && k != 2u && k != 4u && k != 8u) || rows[i].reserved != 0u) return -1;
        if ((rows[i].dstOff & 15u) || (ext & 15u) || (rows[i].len && !rows[i].src) || rows[i].dstOff < end ||
            rows[i].dstOff > (uint64_t)stageBytes || ext > (uint64_t)stageBytes - rows[i].dstOff)
            return -1;
        end = rows[i].dstOff + ext;
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gGroupXorLaunches, 1);
    __sync_fetch_and_add(&gGroupXorRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_group_xor_row_t *r = &d_rows[i];
        const unsigned char *from = (const unsigned char *)(uintptr_t)r->src, *base = (const unsigned char *)(uintptr_t)r->base;
        unsigned char *to = (unsigned char *)d_stage + r->dstOff;
        const uint32_t k = r->elem, n = r->len / k;
        uint32_t p;
        for (p = 0; p < r->len; p++) {
            const uint32_t e = p / k, j = p % k;
            to[e < n ? (uint64_t)j * n + e : p] = (unsigned char)(from[p] ^ (base ? base[p] : 0));
        }
        memset(to + r->len, 0, r->pad);
    }
    return 0;
}
