/*
 * mock_hip_huf_code.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_huf_code (include/qzstd_hip_device.h) in plain C over include/qzstd_hufblock.h:
 * the sequential restatement the GPU test compares the kernels with byte for byte, and the device layer's entry for the CPU stand-in of
 * tests/mock/mock_hip.c.  Per row a histogram of the `len` bytes at d_base + srcOff, QZSTD_planeCost, QZSTD_hufLengths, QZSTD_hufCodes,
 * QZSTD_hufEncodeStreams, QZSTD_hufSizeWord; the kept rows packed into d_dense in row order.  Only the outputs the header names are written
 * (d_scratch not at all); the same refusals before anything is touched.  A source of its own: a mock built without it is the device layer
 * of an older library.
 */
#include "qzstd_hip_device.h"
#include "qzstd_hufblock.h"
#include "qzstd_planecost.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int gHufLaunches;
static unsigned long long gHufRows, gHufCoded;

/* test hooks */
int qzstd_mock_huf_code_launches(void) { return gHufLaunches; }
unsigned long long qzstd_mock_huf_code_rows(void) { return gHufRows; }
unsigned long long qzstd_mock_huf_code_coded(void) { return gHufCoded; }

size_t qzstd_hip_huf_code_bytes(const qzstd_hip_plane_row_t *rows, uint32_t nRows)
{
    unsigned long long sum = 0u;
    uint32_t i;
    for (i = 0; i < nRows; i++) sum += QZSTD_HIP_HUF_ROW_BYTES(rows[i].len);
    return sum >= 0xFFFFFFF0ull ? (size_t)-1 : (size_t)sum;
}

int qzstd_hip_huf_code(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                       qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost, uint32_t *d_size, uint32_t *d_off, void *d_dense, size_t denseBytes,
                       void *d_scratch, size_t scratchBytes)
{
    uint32_t i, b, off = 0u;
    size_t need;
    unsigned char *tmp;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_cost || nRows > 0x7FFFFFFFu) return -1;
    for (i = 0; i < nRows; i++)
        if (rows[i].len > QZSTD_PLANE_LEN_MAX || rows[i].reserved || (rows[i].len && !d_base)) return -1;
    if (!d_size || !d_off || !d_dense || !d_scratch || ((uintptr_t)d_dense & 15u) || ((uintptr_t)d_scratch & 15u)) return -1;
    need = qzstd_hip_huf_code_bytes(rows, nRows);
    if (need == (size_t)-1 || denseBytes < need || scratchBytes < QZSTD_HIP_HUF_SCRATCH_BYTES(nRows, need)) return -1;
    tmp = (unsigned char *)malloc(QZSTD_HUF_LEN_MAX);
    if (!tmp) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gHufLaunches, 1);
    __sync_fetch_and_add(&gHufRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const unsigned char *p = (const unsigned char *)d_base + d_rows[i].srcOff;
        const uint32_t len = d_rows[i].len;
        uint32_t hist[256], tab[256], size = 0u;
        uint8_t nbits[256];
        memset(hist, 0, sizeof(hist));
        for (b = 0; b < len; b++) hist[p[b]]++;
        d_cost[i] = QZSTD_planeCost(hist, len);
        d_off[i] = off;
        if (len >= QZSTD_HUF_LEN_MIN && len <= QZSTD_HUF_LEN_MAX && QZSTD_hufLengths(hist, len, nbits)) {
            QZSTD_hufCodes(nbits, tab);
            /* (room for len bytes: streams that do not fit are not below len either) */
            size = QZSTD_hufSizeWord((uint32_t)QZSTD_hufEncodeStreams(p, len, tab, tmp, len), len);
        }
        d_size[i] = size;
        if (size) {
            unsigned char *out = (unsigned char *)d_dense + off;
            const uint32_t padded = (QZSTD_HUF_LENGTHS_BYTES + size + 15u) & ~15u;
            QZSTD_hufPackLengths(nbits, out);
            memcpy(out + QZSTD_HUF_LENGTHS_BYTES, tmp, size);
            memset(out + QZSTD_HUF_LENGTHS_BYTES + size, 0, padded - QZSTD_HUF_LENGTHS_BYTES - size);
            off += padded;
            __sync_fetch_and_add(&gHufCoded, 1ull);
        }
    }
    d_off[nRows] = off;
    free(tmp);
    return 0;
}
