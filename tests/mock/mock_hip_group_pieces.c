/*
 * mock_hip_group_pieces.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_group_pieces (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip.c and mock_hip_device.c, so that QZSTD_frontCompressDeviceSlices runs in the CPU suite, and the reference the GPU
 * test holds the kernel against: the launcher's checks in plain C — the same refusals before anything is touched — and the header's
 * definition with the headers' own functions: a row's pieces concatenated, QZSTD_byteXor with the concatenated bases, QZSTD_byteGroup into
 * the stage, `pad` zero bytes behind.  A source of its own: a mock built without it is the device layer of an older library, which must
 * refuse a call that needs pieces and serve every other one.
 */
#include "qzstd_bytegroup.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int gGroupPiecesLaunches;
static unsigned long long gGroupPiecesRows, gGroupPiecesPieces;

/* test hooks */
int qzstd_mock_group_pieces_launches(void) { return gGroupPiecesLaunches; }
unsigned long long qzstd_mock_group_pieces_rows(void) { return gGroupPiecesRows; }
unsigned long long qzstd_mock_group_pieces_pieces(void) { return gGroupPiecesPieces; }

int qzstd_hip_group_pieces(int device, void *stream, const qzstd_hip_group_pieces_row_t *rows, uint32_t nRows,
                           qzstd_hip_group_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                           qzstd_hip_group_piece_t *d_pieces, void *d_stage, size_t stageBytes)
{
    uint64_t end = 0;
    uint32_t i, p, maxLen = 0;
    unsigned char *c, *b;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return -1;
    if (nPieces && (!pieces || !d_pieces)) return -1;
    for (i = 0; i < nRows; i++) {
        const uint64_t ext = (uint64_t)rows[i].len + rows[i].pad;
        const uint32_t k = rows[i].elem;
        uint64_t at = 0;
        if ((k != 1u && k != 2u && k != 4u && k != 8u) || rows[i].reserved != 0u) return -1;
        if ((rows[i].dstOff & 15u) || (ext & 15u) || rows[i].dstOff < end || rows[i].dstOff > (uint64_t)stageBytes ||
            ext > (uint64_t)stageBytes - rows[i].dstOff)
            return -1;
        if ((uint64_t)rows[i].piece0 + rows[i].nPieces > nPieces) return -1;
        for (p = rows[i].piece0; p < rows[i].piece0 + rows[i].nPieces; p++) {
            if (!pieces[p].len || !pieces[p].src || pieces[p].off != at) return -1;
            at += pieces[p].len;
        }
        if (at != rows[i].len) return -1;
        end = rows[i].dstOff + ext;
        if (rows[i].len > maxLen) maxLen = rows[i].len;
    }
    if ((end >> 4) > 0xFFFFFFFFull - 2048u) return -1;
    if (end == 0) return 0; /* nothing but empty rows */
    c = (unsigned char *)malloc(2u * (size_t)maxLen + 2u);
    if (!c) return -1;
    b = c + maxLen + 1u;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    if (nPieces) memcpy(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces));
    __sync_fetch_and_add(&gGroupPiecesLaunches, 1);
    __sync_fetch_and_add(&gGroupPiecesRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_group_pieces_row_t *r = &d_rows[i];
        unsigned char *to = (unsigned char *)d_stage + r->dstOff;
        memset(b, 0, r->len);
        for (p = r->piece0; p < r->piece0 + r->nPieces; p++) {
            const qzstd_hip_group_piece_t *q = &d_pieces[p];
            memcpy(c + q->off, (const void *)(uintptr_t)q->src, q->len);
            if (q->base) memcpy(b + q->off, (const void *)(uintptr_t)q->base, q->len);
        }
        __sync_fetch_and_add(&gGroupPiecesPieces, (unsigned long long)r->nPieces);
        QZSTD_byteXor(c, c, b, r->len);
        QZSTD_byteGroup(to, c, r->len, r->elem);
        memset(to + r->len, 0, r->pad);
    }
    free(c);
    return 0;
}
