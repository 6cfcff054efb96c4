/*
 * qzstd_fingerprint.c — QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch / QZSTD_frontFingerprintStats / QZSTD_fingerprintOf
 * (include/qzstd_frontend_device.h): a 64-bit fingerprint (include/qzstd_fingerprint.h) of every chunk of a list of device buffers, taken on
 * the GPU from the tensors' own bytes, and the check of such buffers against fingerprints kept from an earlier call.  Part of
 * qzstd_frontend.c's translation unit, included behind qzstd_verify.c; it uses the restore's first slot (its stream, and grow-only pinned
 * and device scratch kept there between calls).
 *
 * A call is: the host-side checks of the batch compress call; the scaffold of qzstd_frontend.c (qfCallBegin .. qfCallEnd) with ONE stream;
 * ONE qzstd_hip_fingerprint launch with a row per frame that points INTO the caller's buffers (nothing is staged or copied on the device);
 * one device->host copy of the tile digests (8 bytes per 16 KiB); and QZSTD_fpFold per frame on the calling thread.  Nothing of the producer
 * or the workers is used: a front created with useProducer = 0 serves the calls.
 */

extern int qzstd_hip_fingerprint(int device, void *stream, qzstd_hip_fp_row_t *rows, uint32_t nRows, qzstd_hip_fp_row_t *d_rows,
                                 uint64_t *d_tiles) __attribute__((weak));
extern int qzstd_hip_fingerprint_pieces(int device, void *stream, qzstd_hip_fp_pieces_row_t *rows, uint32_t nRows, qzstd_hip_fp_pieces_row_t *d_rows,
                                        const qzstd_hip_group_piece_t *pieces, uint32_t nPieces, qzstd_hip_group_piece_t *d_pieces,
                                        uint64_t *d_tiles) __attribute__((weak));

unsigned long long QZSTD_fingerprintOf(const void *p, size_t len) { return p || !len ? QZSTD_fingerprint(p, len) : 0ull; }

/* both calls: fp[c] receives the fingerprint of frame c (fp may be NULL when expected is not); with `expected`, differs[c] (or NULL) says
 * whether it is another one, and the return value counts those frames instead of all.  sm: NULL, or the source slices of the calls of
 * qzstd_slicecheck.c (looked up already; bufs holds the sizes): a frame inside one piece is the row it is in a contiguous buffer, and a call
 * with a frame of several pieces is ONE qzstd_hip_fingerprint_pieces launch over all its rows instead */
static size_t qfFingerprintDevice(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, const QF_SrcMap *sm, void *stream, unsigned long long *fp,
                                  size_t *firstFrame, const unsigned long long *expected, int check, size_t nExpected, unsigned char *differs)
{
    const int pieces = sm && sm->multi;
    size_t nPieces = 0, m = 0, multi = 0;
    QF_Call call;
    QF_RestoreSlot *s;
    qzstd_hip_fp_row_t *rows;
    qzstd_hip_fp_pieces_row_t *pieceRows = NULL;
    qzstd_hip_group_piece_t *chk = NULL;
    const uint64_t *tiles;
    size_t i, c = 0, nFrames = 0, nTiles = 0, total = 0, t = 0, nDiff = 0;
    int dev, rc = 0;
    /* host-side checks, the batch compress call's: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufs) || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    for (i = 0; i < nBufs; i++) {
        if (!bufs[i].d_ptr && bufs[i].size) return (size_t)-1;
        nFrames += bufs[i].size / f->p.chunkSize + (bufs[i].size % f->p.chunkSize != 0);
        nTiles += (bufs[i].size / f->p.chunkSize) * (size_t)QZSTD_HIP_FP_TILES(f->p.chunkSize) + (size_t)QZSTD_HIP_FP_TILES(bufs[i].size % f->p.chunkSize);
        total += bufs[i].size;
    }
    if (check) {
        if (nExpected != nFrames || (nFrames && !expected)) return (size_t)-1;
    } else if (nFrames && !fp) {
        return (size_t)-1;
    }
    if (nFrames > 0xFFFFFFFFu || nTiles > 0x7FFFFFFFu || f->p.chunkSize > 0xFFFFFFE0u) return (size_t)-1; /* (one launch: 32-bit rows and tiles) */
    if (!qzstd_hip_fingerprint || !qzstd_hip_pointer_device || !qzstd_hip_event_create || !qzstd_hip_event_record || !qzstd_hip_stream_wait_event ||
        !qzstd_hip_event_destroy)
        return (size_t)-1; /* a device layer without the fingerprint kernel, or without the device-input entry points at all */
    if (pieces && !qzstd_hip_fingerprint_pieces) return (size_t)-1; /* a frame of several pieces and a device layer that cannot read one */
    call.f = f;
    call.restore = 1;
    call.nStreams = 1; /* the restore side's first slot alone: its stream and scratch */
    call.dev = sm ? sm->dev : -1; /* (a call with source slices has looked its memory up: qfSrcMapBuild) */
    if (!sm && qfCallBufs(&call, bufs, NULL, nBufs)) return (size_t)-1;
    /* a call without a frame takes nothing, not even devBusy, as the compress calls */
    if (nFrames == 0) {
        qfFirstFrames(f, bufs, nBufs, firstFrame);
        return 0;
    }
    if (qfCallBegin(&call, stream)) return (size_t)-1; /* (firstFrame is not written by a call that is refused) */
    qfFirstFrames(f, bufs, nBufs, firstFrame);
    dev = call.dev;
    s = f->restoreSlot;

    rows = (qzstd_hip_fp_row_t *)qfBufH(&s->pin.fpRows, nFrames * sizeof(qzstd_hip_fp_row_t)); /* (kept in either launch: the fold below reads a row's len) */
    if (!rows) rc = -1;
    if (rc == 0 && pieces) {
        size_t p, off;
        for (i = 0; i < nBufs; i++)
            for (off = 0, p = sm->first[i]; off < bufs[i].size; off += f->p.chunkSize)
                nPieces += qfSrcFramePieces(sm, &p, off, bufs[i].size - off < f->p.chunkSize ? bufs[i].size - off : f->p.chunkSize);
        if (nPieces > 0xFFFFFFFFu || !(pieceRows = (qzstd_hip_fp_pieces_row_t *)qfBufH(&s->pin.fpPieceRows, nFrames * sizeof(qzstd_hip_fp_pieces_row_t))) ||
            !(chk = (qzstd_hip_group_piece_t *)qfBufH(&s->pin.chkPieces, nPieces * sizeof(qzstd_hip_group_piece_t))) ||
            !qfBufD(dev, &s->dev.fpPieceRows, nFrames * sizeof(qzstd_hip_fp_pieces_row_t)) ||
            !qfBufD(dev, &s->dev.chkPieces, nPieces * sizeof(qzstd_hip_group_piece_t)))
            rc = -1;
    }
    tiles = rc == 0 ? (const uint64_t *)qfBufH(&s->pin.fpTiles, nTiles * sizeof(uint64_t)) : NULL;
    if (!tiles || !qfBufD(dev, &s->dev.fpRows, nFrames * sizeof(qzstd_hip_fp_row_t)) || !qfBufD(dev, &s->dev.fpTiles, nTiles * sizeof(uint64_t))) rc = -1;
    if (rc == 0) {
        for (i = 0, c = 0; i < nBufs; i++) {
            size_t off, p = sm ? sm->first[i] : 0;
            for (off = 0; off < bufs[i].size; off += f->p.chunkSize, c++) {
                qzstd_hip_fp_row_t *r = &rows[c];
                r->src = (uint64_t)(uintptr_t)((const unsigned char *)bufs[i].d_ptr + off);
                r->len = (uint32_t)(bufs[i].size - off < f->p.chunkSize ? bufs[i].size - off : f->p.chunkSize);
                r->tile0 = 0;
                if (sm) {
                    const size_t np = qfSrcFramePieces(sm, &p, off, r->len);
                    r->src = np == 1u ? (uint64_t)(uintptr_t)(sm->pieces[p].src + (off - sm->pieces[p].off)) : 0u;
                    if (pieces) {
                        qzstd_hip_fp_pieces_row_t *q = &pieceRows[c];
                        q->len = r->len;
                        q->tile0 = 0;
                        q->piece0 = (uint32_t)m;
                        q->nPieces = (uint32_t)np;
                        qfSrcFrameTable(sm, p, np, off, r->len, 0, &chk[m]);
                        m += np;
                        if (np > 1u) multi++;
                    }
                }
            }
        }
        if ((pieces ? qzstd_hip_fingerprint_pieces(dev, s->stream, pieceRows, (uint32_t)nFrames, (qzstd_hip_fp_pieces_row_t *)s->dev.fpPieceRows.p, chk,
                                                   (uint32_t)nPieces, (qzstd_hip_group_piece_t *)s->dev.chkPieces.p, (uint64_t *)s->dev.fpTiles.p)
                    : qzstd_hip_fingerprint(dev, s->stream, rows, (uint32_t)nFrames, (qzstd_hip_fp_row_t *)s->dev.fpRows.p, (uint64_t *)s->dev.fpTiles.p)) ||
            qzstd_hip_memcpy_d2h(dev, s->stream, s->pin.fpTiles.p, s->dev.fpTiles.p, nTiles * sizeof(uint64_t)))
            rc = -1;
    }
    if (qfCallWait(&call)) rc = -1;
    for (c = 0; c < nFrames && rc == 0; c++) {
        const size_t n = (size_t)QZSTD_HIP_FP_TILES(rows[c].len);
        const unsigned long long v = QZSTD_fpFold(tiles + t, n, rows[c].len);
        t += n;
        if (fp) fp[c] = v;
        if (check) {
            const int d = v != expected[c];
            if (differs) differs[c] = (unsigned char)d;
            nDiff += (size_t)d;
        }
    }
    if (rc == 0) {
        __atomic_fetch_add(&f->fpStats[0], (unsigned long long)nFrames, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->fpStats[1], (unsigned long long)total, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->fpStats[2], 1ull, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->fpStats[3], (unsigned long long)nDiff, __ATOMIC_RELAXED);
        if (pieces) {
            sm->counts[0] += (unsigned long long)multi; /* (the call adds them to the front's) */
            sm->counts[1] += 1ull;
        }
    }
    qfCallEnd(&call);
    return rc ? (size_t)-1 : (check ? nDiff : nFrames);
}

size_t QZSTD_frontFingerprintDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream, unsigned long long *fp,
                                         size_t *firstFrame)
{
    return qfFingerprintDevice(f, bufs, nBufs, NULL, stream, fp, firstFrame, NULL, 0, 0, NULL);
}

size_t QZSTD_frontCheckDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream, const unsigned long long *expected,
                                   size_t nFrames, unsigned char *differs)
{
    return qfFingerprintDevice(f, bufs, nBufs, NULL, stream, NULL, NULL, expected, 1, nFrames, differs);
}

void QZSTD_frontFingerprintStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->fpStats : NULL, stats, 4); }
