/*
 * qzstd_verify.c — QZSTD_frontVerifyDeviceBatch / QZSTD_frontVerifyStats (include/qzstd_frontend_device.h): do the frames a compress call
 * left reproduce the tensors that are on the device NOW?  The restore with a comparison in the scatter's place: nothing of the caller's is
 * written, no temporary of the buffers' size exists, and the answer says where the first difference of every frame lies.  Part of
 * qzstd_frontend.c's translation unit, included behind qzstd_restore.c, whose slots (QF_RestoreSlot), part type and workers' decode
 * (qfRestoreDecode) it uses; the call's prologue and epilogue are the scaffold's (qfCallBegin .. qfCallEnd, qzstd_frontend.c).
 *
 * The call's frames are cut into parts of whole frames, at most QF_PART_BYTES ($QZSTD_FRONT_DEVICE_PART) of DECODED content each.  Per part,
 * on one of the two restore slots: the workers decode its frames into the pinned buffer; the calling thread queues the host->device copy,
 * ONE qzstd_hip_ungroup_cmp launch (a row per frame: the live chunk, its base chunk, the frame's place in the stage) and the device->host
 * copy of the launch's tile words (4 bytes per 16 KiB), and hands the workers the next part.  A slot's tile words are read when its stream
 * has passed them: before the slot is used again, and behind the last part.  With QZSTD_frontSetDeltaSkip on, a frame of a based buffer
 * that IS the canonical zero frame of its chunk's length (qfIsZeroFrame) is not decoded and takes no room in the pinned buffer or the
 * copy: it is a ZERO row of the part it falls into — live chunk and base chunk are compared directly — and a part may consist of such rows
 * alone (no job, no copy; the launch reads no stage).
 */

extern int qzstd_hip_ungroup_cmp(int device, void *stream, qzstd_hip_ungroup_cmp_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_cmp_row_t *d_rows,
                                 const void *d_stage, size_t stageBytes, uint32_t *d_tiles) __attribute__((weak));
extern int qzstd_hip_ungroup_cmp_pieces(int device, void *stream, qzstd_hip_ungroup_cmp_pieces_row_t *rows, uint32_t nRows,
                                        qzstd_hip_ungroup_cmp_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                        qzstd_hip_group_piece_t *d_pieces, const void *d_stage, size_t stageBytes, uint32_t *d_tiles)
    __attribute__((weak));

/* one frame of the call: the row it becomes */
typedef struct {
    const unsigned char *d_ref;  /* the live chunk; NULL for a frame of several pieces (a call with source slices) */
    const unsigned char *d_base; /* its base chunk, or NULL */
    size_t off, p0, np;          /* a call with source slices: the frame's offset in its buffer and the pieces of the map that hold its bytes */
    size_t len;
    size_t m;                    /* its frame in the decode table; (size_t)-1: a ZERO row, not decoded */
    uint32_t k;
} QF_VerifyRow;

/* frames [c0, c1) of the call, of them decoded [f0, f1) of the table: decoded content bytes, stage bytes, compared bytes (ZERO rows too), tile words */
typedef struct { size_t c0, c1, f0, f1, bytes, stage, compared, tiles, pieces, multi; } QF_VerifyRange; /* (pieces, multi: the frames' pieces, and the frames with more than one) */

/* the tile words of the part a slot last ran (its stream has passed them): per frame the first one that is not "same" */
static void qfVerifyHarvest(QZSTD_Front *f, QF_RestoreSlot *s, const QF_VerifyRange *parts, const QF_VerifyRow *rows, size_t *firstDiff, size_t *nDiff)
{
    const QF_VerifyRange *pr;
    const uint32_t *tiles = (const uint32_t *)s->pin.tiles.p;
    size_t c, t = 0, differing = 0;
    if (!s->pending) return;
    pr = &parts[s->pending - 1u];
    s->pending = 0;
    for (c = pr->c0; c < pr->c1; c++) {
        const size_t n = (size_t)QZSTD_HIP_CMP_TILES(rows[c].len, rows[c].k);
        size_t i, at = QZSTD_VERIFY_SAME;
        for (i = 0; i < n; i++)
            if (tiles[t + i] != QZSTD_HIP_CMP_SAME) { at = tiles[t + i]; break; }
        t += n;
        if (firstDiff) firstDiff[c] = at;
        if (at != QZSTD_VERIFY_SAME) differing++;
    }
    *nDiff += differing;
    __atomic_fetch_add(&f->verifyStats[1], (unsigned long long)differing, __ATOMIC_RELAXED);
}

/* the call's body.  sm: NULL, or the source slices of QZSTD_frontVerifyDeviceSlices (qzstd_slicecheck.c; looked up already, bufs and bases
 * hold the sizes): a frame inside one piece is the row it is in a contiguous buffer, and a part with a frame of several pieces is ONE
 * qzstd_hip_ungroup_cmp_pieces launch over all its rows instead */
static size_t qfVerifyDevice(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                             const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const QF_SrcMap *sm, const unsigned char *elemSizes,
                             size_t nBufs, void *stream, size_t *firstDiff)
{
    QF_RestoreFrame *table = NULL; /* the frames that are decoded */
    size_t *callOf = NULL;         /* their numbers in the call */
    unsigned char *bad = NULL;     /* the ones a worker stopped at */
    QF_VerifyRow *rows = NULL;     /* every frame of the call */
    QF_VerifyRange *parts = NULL;
    unsigned char *scratch = NULL;
    QF_ZeroHash zh;
    QF_Call call;
    QF_RestoreSlot *slot;
    size_t i, c = 0, m = 0, k, nParts = 0, want = 0, partBytes, pos = 0, nDiff = 0, tp;
    int dev, rc = 0, anyBase = 0, skip;
    /* host-side checks, the restore's: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufs) || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    for (i = 0; i < nBufs; i++) {
        const unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : f->group;
        if (!bufs[i].d_ptr && bufs[i].size) return (size_t)-1;
        if (e != 1u && e != 2u && e != 4u && e != 8u) return (size_t)-1;
        want += bufs[i].size / f->p.chunkSize + (bufs[i].size % f->p.chunkSize != 0);
    }
    if (want != nFrames || (nFrames && (!frames || !frameSizes))) return (size_t)-1;
    for (i = 0; bases && i < nBufs; i++) {
        if (!bases[i].d_ptr && !bases[i].size) continue;
        if (!bases[i].d_ptr || bases[i].size != bufs[i].size) return (size_t)-1;
        if (bases[i].size) anyBase = 1;
    }
    if (!anyBase) bases = NULL;
    if (!qzstd_hip_ungroup_cmp || !qzstd_hip_pointer_device || !qzstd_hip_event_create || !qzstd_hip_event_record || !qzstd_hip_stream_wait_event ||
        !qzstd_hip_event_destroy)
        return (size_t)-1; /* a device layer without the ungrouping comparison, or without the device-input entry points at all */
    if (sm && sm->multi && !qzstd_hip_ungroup_cmp_pieces) return (size_t)-1; /* a frame of several pieces and a device layer that cannot read one */
    call.f = f;
    call.restore = 1;
    call.nStreams = 2;
    call.dev = sm ? sm->dev : -1; /* (a call with source slices has looked its memory up: qfSrcMapBuild) */
    if (!sm && qfCallBufs(&call, bufs, bases, nBufs)) return (size_t)-1;
    if (nFrames == 0) return 0;
    if (qfCallBegin(&call, stream)) return (size_t)-1;
    dev = call.dev;
    slot = f->restoreSlot;

    partBytes = qfPartBytes();
    skip = bases && f->deltaSkip;
    memset(&zh, 0, sizeof(zh));
    table = (QF_RestoreFrame *)malloc(nFrames * sizeof(*table));
    callOf = (size_t *)malloc(nFrames * sizeof(*callOf));
    bad = (unsigned char *)calloc(nFrames, 1);
    rows = (QF_VerifyRow *)malloc(nFrames * sizeof(*rows));
    parts = (QF_VerifyRange *)malloc(nFrames * sizeof(*parts));
    if (skip) scratch = (unsigned char *)malloc(qfZeroFrameBound(f->p.chunkSize));
    if (!table || !callOf || !bad || !rows || !parts || (skip && !scratch)) rc = -1;
    for (i = 0; i < nBufs && rc == 0; i++) {
        const unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : f->group;
        const unsigned char *base = bases && bases[i].d_ptr ? (const unsigned char *)bases[i].d_ptr : NULL;
        size_t off, p = sm ? sm->first[i] : 0;
        for (off = 0; off < bufs[i].size; off += f->p.chunkSize, pos += frameSizes[c], c++) {
            const size_t len = bufs[i].size - off < f->p.chunkSize ? bufs[i].size - off : f->p.chunkSize;
            const unsigned char *src = (const unsigned char *)frames + (frameStride ? c * frameStride : pos);
            const int zero = skip && base && qfIsZeroFrame(src, frameSizes[c], len, scratch, &zh, f->p.chunkSize);
            QF_VerifyRange *cur = nParts ? &parts[nParts - 1] : NULL;
            if (len > 0xFFFFFFE0u) { rc = -1; break; } /* (a row's length is 32-bit) */
            /* a part ends where another decoded frame would not fit, where its launch's rows are 32-bit, and where its tile words are */
            if (!cur || (!zero && cur->bytes + len > partBytes) || cur->c1 - cur->c0 >= 0xFFFFFFFFu ||
                cur->tiles + (size_t)QZSTD_HIP_CMP_TILES(len, e) > 0x7FFFFFFFu) {
                cur = &parts[nParts++];
                cur->c0 = c;
                cur->f0 = cur->f1 = m;
                cur->bytes = cur->stage = cur->compared = cur->tiles = cur->pieces = cur->multi = 0;
            }
            rows[c].d_ref = (const unsigned char *)bufs[i].d_ptr + off;
            rows[c].d_base = base ? base + off : NULL;
            rows[c].off = off;
            rows[c].p0 = 0;
            rows[c].np = 1;
            if (sm) {
                const QF_SrcPiece *q;
                rows[c].np = qfSrcFramePieces(sm, &p, off, len);
                rows[c].p0 = p;
                q = &sm->pieces[p];
                rows[c].d_ref = rows[c].np == 1u ? q->src + (off - q->off) : NULL;
                rows[c].d_base = rows[c].np == 1u && q->base ? q->base + (off - q->off) : NULL;
                if (cur->pieces + rows[c].np > 0xFFFFFFFFu) { rc = -1; break; }
            }
            cur->pieces += rows[c].np;
            cur->multi += rows[c].np > 1u;
            rows[c].len = len;
            rows[c].k = e;
            rows[c].m = (size_t)-1;
            if (!zero) {
                table[m].src = src;
                table[m].srcSize = frameSizes[c];
                table[m].d_dst = NULL;
                table[m].d_base = NULL;
                table[m].len = len;
                table[m].at = cur->stage;
                table[m].k = e;
                callOf[m] = c;
                rows[c].m = m;
                cur->f1 = ++m;
                cur->bytes += len;
                cur->stage += qfPad16(len);
            }
            cur->c1 = c + 1u;
            cur->compared += len;
            cur->tiles += (size_t)QZSTD_HIP_CMP_TILES(len, e);
        }
    }
    for (k = 0; k < nParts && rc == 0; k++) {
        const QF_VerifyRange *pr = &parts[k];
        const size_t nf = pr->f1 - pr->f0, nr = pr->c1 - pr->c0;
        QF_RestoreSlot *s = &slot[k % 2];
        unsigned char *hStage;
        qzstd_hip_ungroup_cmp_row_t *cmpRows;
        qzstd_hip_ungroup_cmp_pieces_row_t *pieceRows = NULL;
        qzstd_hip_group_piece_t *chk = NULL;
        /* part k - 2 ran on this slot: its stream must have passed the copy, the launch and the tile words' way back before they are read
         * and the buffers written (or grown) */
        if (qzstd_hip_stream_wait(dev, s->stream, QF_DEV_WAIT_MS) != 0) { rc = -1; break; }
        qfVerifyHarvest(f, s, parts, rows, firstDiff, &nDiff);
        hStage = (unsigned char *)qfBufH(&s->pin.stage, pr->stage);
        cmpRows = hStage ? (qzstd_hip_ungroup_cmp_row_t *)qfBufH(&s->pin.cmpRows, nr * sizeof(qzstd_hip_ungroup_cmp_row_t)) : NULL;
        if (!cmpRows || !qfBufH(&s->pin.tiles, pr->tiles * sizeof(uint32_t)) || !qfBufD(dev, &s->dev.stage, pr->stage) ||
            !qfBufD(dev, &s->dev.cmpRows, nr * sizeof(qzstd_hip_ungroup_cmp_row_t)) || !qfBufD(dev, &s->dev.tiles, pr->tiles * sizeof(uint32_t))) {
            rc = -1;
            break;
        }
        if (pr->multi && (!(pieceRows = (qzstd_hip_ungroup_cmp_pieces_row_t *)qfBufH(&s->pin.cmpPieceRows, nr * sizeof(qzstd_hip_ungroup_cmp_pieces_row_t))) ||
                          !(chk = (qzstd_hip_group_piece_t *)qfBufH(&s->pin.chkPieces, pr->pieces * sizeof(qzstd_hip_group_piece_t))) ||
                          !qfBufD(dev, &s->dev.cmpPieceRows, nr * sizeof(qzstd_hip_ungroup_cmp_pieces_row_t)) ||
                          !qfBufD(dev, &s->dev.chkPieces, pr->pieces * sizeof(qzstd_hip_group_piece_t)))) {
            rc = -1;
            break;
        }
        for (c = 0, tp = 0; pr->multi && c < nr; c++) {
            const QF_VerifyRow *vr = &rows[pr->c0 + c];
            qzstd_hip_ungroup_cmp_pieces_row_t *r = &pieceRows[c];
            r->srcOff = vr->m == (size_t)-1 ? 0u : table[vr->m].at;
            r->len = (uint32_t)vr->len;
            r->elem = vr->k;
            r->flags = vr->m == (size_t)-1 ? QZSTD_HIP_CMP_ZERO : 0u;
            r->tile0 = 0;
            r->piece0 = (uint32_t)tp;
            r->nPieces = (uint32_t)vr->np;
            qfSrcFrameTable(sm, vr->p0, vr->np, vr->off, vr->len, 1, &chk[tp]);
            tp += vr->np;
        }
        for (c = 0; !pr->multi && c < nr; c++) {
            const QF_VerifyRow *vr = &rows[pr->c0 + c];
            qzstd_hip_ungroup_cmp_row_t *r = &cmpRows[c];
            r->ref = (uint64_t)(uintptr_t)vr->d_ref;
            r->base = (uint64_t)(uintptr_t)vr->d_base;
            r->srcOff = vr->m == (size_t)-1 ? 0u : table[vr->m].at;
            r->len = (uint32_t)vr->len;
            r->elem = vr->k;
            r->flags = vr->m == (size_t)-1 ? QZSTD_HIP_CMP_ZERO : 0u;
            r->tile0 = 0;
        }
        if (nf) {
            if (qfRestoreDecode(f, table, pr->f0, nf, hStage, bad)) {
                for (c = pr->f0; firstDiff && c < pr->f1; c++)
                    if (bad[c]) firstDiff[callOf[c]] = QZSTD_VERIFY_UNDECODED;
                rc = -1;
                break;
            }
            if (qzstd_hip_memcpy_h2d(dev, s->stream, s->dev.stage.p, hStage, pr->stage)) { rc = -1; break; }
        }
        if ((pr->multi ? qzstd_hip_ungroup_cmp_pieces(dev, s->stream, pieceRows, (uint32_t)nr, (qzstd_hip_ungroup_cmp_pieces_row_t *)s->dev.cmpPieceRows.p,
                                                      chk, (uint32_t)pr->pieces, (qzstd_hip_group_piece_t *)s->dev.chkPieces.p, s->dev.stage.p,
                                                      pr->stage, (uint32_t *)s->dev.tiles.p)
                       : qzstd_hip_ungroup_cmp(dev, s->stream, cmpRows, (uint32_t)nr, (qzstd_hip_ungroup_cmp_row_t *)s->dev.cmpRows.p, s->dev.stage.p,
                                               pr->stage, (uint32_t *)s->dev.tiles.p)) ||
            qzstd_hip_memcpy_d2h(dev, s->stream, s->pin.tiles.p, s->dev.tiles.p, pr->tiles * sizeof(uint32_t))) {
            rc = -1;
            break;
        }
        s->pending = k + 1u;
        __atomic_fetch_add(&f->verifyStats[0], (unsigned long long)nr, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->verifyStats[2], (unsigned long long)pr->compared, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->verifyStats[3], 1ull, __ATOMIC_RELAXED);
        if (pr->multi) {
            sm->counts[0] += (unsigned long long)pr->multi; /* (the call adds them to the front's) */
            sm->counts[1] += 1ull;
        }
    }
    if (qfCallWait(&call)) rc = -1;
    /* the last parts' tile words, in the parts' order (part nParts - 2 ran on the other slot than the last one) */
    for (k = 0; k < 2; k++) {
        QF_RestoreSlot *s = &slot[(nParts + k) % 2];
        if (rc == 0) qfVerifyHarvest(f, s, parts, rows, firstDiff, &nDiff);
        s->pending = 0;
    }
    free(table);
    free(callOf);
    free(bad);
    free(rows);
    free(parts);
    free(scratch);
    qfCallEnd(&call);
    return rc == 0 ? nDiff : (size_t)-1;
}

size_t QZSTD_frontVerifyDeviceBatch(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                    const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes, size_t nBufs,
                                    void *stream, size_t *firstDiff)
{
    return qfVerifyDevice(f, frames, frameStride, frameSizes, nFrames, bufs, bases, NULL, elemSizes, nBufs, stream, firstDiff);
}

void QZSTD_frontVerifyStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->verifyStats : NULL, stats, 4); }
