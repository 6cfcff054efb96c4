/*
 * mock_hip_fingerprint_pieces.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_fingerprint_pieces (include/qzstd_hip_device.h) for the CPU stand-in
 * of tests/mock/mock_hip.c and mock_hip_device.c, so that the fingerprint calls with source slices run in the CPU suite, and the reference
 * the GPU test holds the kernel against: the launcher's checks in plain C — the same refusals before anything is touched, tile0 filled as
 * the launcher fills it, only d_tiles[0 .. total tiles) written — and the header's definition: a row's pieces concatenated, every tile
 * digest by the header's own QZSTD_fpTile (include/qzstd_fingerprint.h).  A source of its own: a mock built without it is the device layer
 * of an older library, which must refuse a call with a frame of several pieces and serve every other one.
 */
#include "qzstd_fingerprint.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int gFpPiecesLaunches;
static unsigned long long gFpPiecesRows, gFpPiecesPieces;

/* test hooks */
int qzstd_mock_fingerprint_pieces_launches(void) { return gFpPiecesLaunches; }
unsigned long long qzstd_mock_fingerprint_pieces_rows(void) { return gFpPiecesRows; }
unsigned long long qzstd_mock_fingerprint_pieces_pieces(void) { return gFpPiecesPieces; }

int qzstd_hip_fingerprint_pieces(int device, void *stream, qzstd_hip_fp_pieces_row_t *rows, uint32_t nRows, qzstd_hip_fp_pieces_row_t *d_rows,
                                 const qzstd_hip_group_piece_t *pieces, uint32_t nPieces, qzstd_hip_group_piece_t *d_pieces, uint64_t *d_tiles)
{
    uint64_t total = 0;
    uint32_t i, p, maxLen = 0;
    unsigned char *c;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles) return -1;
    if (nPieces && (!pieces || !d_pieces)) return -1;
    for (i = 0; i < nRows; i++) {
        uint64_t at = 0;
        if (rows[i].len > 0xFFFFFFE0u) return -1;
        if ((uint64_t)rows[i].piece0 + rows[i].nPieces > nPieces) return -1;
        for (p = rows[i].piece0; p < rows[i].piece0 + rows[i].nPieces; p++) {
            if (!pieces[p].len || !pieces[p].src || pieces[p].base || pieces[p].off != at) return -1;
            at += pieces[p].len;
        }
        if (at != rows[i].len) return -1;
        total += QZSTD_HIP_FP_TILES(rows[i].len);
        if (rows[i].len > maxLen) maxLen = rows[i].len;
    }
    if (total > 0x7FFFFFFFull) return -1;
    if (total == 0) return 0;
    c = (unsigned char *)malloc((size_t)maxLen + 1u);
    if (!c) return -1;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_FP_TILES(rows[i].len);
    }
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    memcpy(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces));
    __sync_fetch_and_add(&gFpPiecesLaunches, 1);
    __sync_fetch_and_add(&gFpPiecesRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_fp_pieces_row_t *r = &d_rows[i];
        uint64_t at, j = 0;
        for (p = r->piece0; p < r->piece0 + r->nPieces; p++)
            memcpy(c + d_pieces[p].off, (const void *)(uintptr_t)d_pieces[p].src, d_pieces[p].len);
        __sync_fetch_and_add(&gFpPiecesPieces, (unsigned long long)r->nPieces);
        for (at = 0; at < r->len; at += QZSTD_FP_TILE, j++)
            d_tiles[r->tile0 + j] = QZSTD_fpTile(c + at, r->len - at < QZSTD_FP_TILE ? (uint32_t)(r->len - at) : QZSTD_FP_TILE);
    }
    free(c);
    return 0;
}
