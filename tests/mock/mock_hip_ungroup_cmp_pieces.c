/*
 * mock_hip_ungroup_cmp_pieces.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_ungroup_cmp_pieces (include/qzstd_hip_device.h) for the CPU stand-in
 * of tests/mock/mock_hip.c and mock_hip_device.c, so that QZSTD_frontVerifyDeviceSlices runs in the CPU suite, and the reference the GPU
 * test holds the kernel against: the launcher's checks in plain C — the same refusals before anything is touched, tile0 filled as the
 * launcher fills it — and the header's definition with the headers' own functions: a row's pieces (and their bases) concatenated,
 * QZSTD_byteUngroup of the staged frame (zeros for a ZERO row, whose stage is never touched), QZSTD_byteXor with the bases, and a byte
 * comparison per tile: QZSTD_HIP_CMP_SAME, or the lowest differing row offset of the tile.  Nothing but d_rows, d_pieces and the tile words
 * is written.  A source of its own: a mock built without it is the device layer of an older library.  (Linked with qzstd_bytegroup.c.)
 */
#include "qzstd_bytegroup.h"
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int gCmpPiecesLaunches;
static unsigned long long gCmpPiecesRows, gCmpPiecesZeroRows, gCmpPiecesPieces;

/* test hooks */
int qzstd_mock_ungroup_cmp_pieces_launches(void) { return gCmpPiecesLaunches; }
unsigned long long qzstd_mock_ungroup_cmp_pieces_rows(void) { return gCmpPiecesRows; }
unsigned long long qzstd_mock_ungroup_cmp_pieces_zero_rows(void) { return gCmpPiecesZeroRows; }
unsigned long long qzstd_mock_ungroup_cmp_pieces_pieces(void) { return gCmpPiecesPieces; }

int qzstd_hip_ungroup_cmp_pieces(int device, void *stream, qzstd_hip_ungroup_cmp_pieces_row_t *rows, uint32_t nRows,
                                 qzstd_hip_ungroup_cmp_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                 qzstd_hip_group_piece_t *d_pieces, const void *d_stage, size_t stageBytes, uint32_t *d_tiles)
{
    uint64_t end = 0, total = 0, zeros = 0;
    uint32_t i, p, maxLen = 0;
    unsigned char *u, *ref, *bas;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_stage & 15u)) return -1;
    if (nPieces && (!pieces || !d_pieces)) return -1;
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_cmp_pieces_row_t *r = &rows[i];
        const uint32_t k = r->elem;
        uint64_t at = 0;
        if (k != 1u && k != 2u && k != 4u && k != 8u) return -1;
        if ((r->flags & ~QZSTD_HIP_CMP_ZERO) || r->len > 0xFFFFFFE0u) return -1;
        if ((uint64_t)r->piece0 + r->nPieces > nPieces) return -1;
        for (p = r->piece0; p < r->piece0 + r->nPieces; p++) {
            if (!pieces[p].len || !pieces[p].src || pieces[p].off != at) return -1;
            at += pieces[p].len;
        }
        if (at != r->len) return -1;
        if (!(r->flags & QZSTD_HIP_CMP_ZERO)) {
            if ((r->srcOff & 15u) || (r->len && !d_stage) || r->srcOff < end) return -1;
            if (r->srcOff > (uint64_t)stageBytes || r->len > (uint64_t)stageBytes - r->srcOff) return -1;
            end = r->srcOff + (((uint64_t)r->len + 15u) & ~(uint64_t)15u);
        } else {
            zeros++;
        }
        total += QZSTD_HIP_CMP_TILES(r->len, k);
        if (r->len > maxLen) maxLen = r->len;
    }
    if (total > 0x7FFFFFFFull) return -1;
    if (total == 0) return 0;
    u = (unsigned char *)malloc(3u * ((size_t)maxLen + 1u));
    if (!u) return -1;
    ref = u + maxLen + 1u;
    bas = ref + maxLen + 1u;
    for (i = 0, total = 0; i < nRows; i++) {
        rows[i].tile0 = (uint32_t)total;
        total += QZSTD_HIP_CMP_TILES(rows[i].len, rows[i].elem);
    }
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    memcpy(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces));
    __sync_fetch_and_add(&gCmpPiecesLaunches, 1);
    __sync_fetch_and_add(&gCmpPiecesRows, (unsigned long long)nRows);
    __sync_fetch_and_add(&gCmpPiecesZeroRows, (unsigned long long)zeros);
    for (i = 0; i < nRows; i++) {
        const qzstd_hip_ungroup_cmp_pieces_row_t *r = &d_rows[i];
        const uint32_t tiles = (uint32_t)QZSTD_HIP_CMP_TILES(r->len, r->elem);
        uint32_t t, q;
        memset(bas, 0, r->len);
        for (p = r->piece0; p < r->piece0 + r->nPieces; p++) {
            const qzstd_hip_group_piece_t *pc = &d_pieces[p];
            memcpy(ref + pc->off, (const void *)(uintptr_t)pc->src, pc->len);
            if (pc->base) memcpy(bas + pc->off, (const void *)(uintptr_t)pc->base, pc->len);
        }
        __sync_fetch_and_add(&gCmpPiecesPieces, (unsigned long long)r->nPieces);
        if (r->flags & QZSTD_HIP_CMP_ZERO) memset(u, 0, r->len);
        else QZSTD_byteUngroup(u, (const unsigned char *)d_stage + r->srcOff, r->len, r->elem);
        QZSTD_byteXor(u, u, bas, r->len);
        for (t = 0; t < tiles; t++) d_tiles[r->tile0 + t] = QZSTD_HIP_CMP_SAME;
        for (q = r->len; q-- > 0;) /* downwards: the lowest differing offset of a tile is stored last */
            if (u[q] != ref[q]) d_tiles[r->tile0 + ((q >> 14) < tiles ? (q >> 14) : tiles - 1u)] = q;
    }
    free(u);
    return 0;
}
