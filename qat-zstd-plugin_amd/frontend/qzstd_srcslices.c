/*
 * qzstd_srcslices.c — QZSTD_frontCompressDeviceSlices (include/qzstd_frontend_device.h): the Delta compress call for buffers that are not
 * contiguous in device memory.  Included by qzstd_frontend.c (its types and helpers are used as they are).
 *
 * The call checks its slices, looks their memory up (qfSrcMapBuild, which the calls of qzstd_slicecheck.c use too) and hands qfCompressDevice
 * a map of the non-empty ones (QF_SrcMap: slices that follow each other in memory, bases included, are one piece there) beside a buffer table
 * that holds the sizes.  The per-frame table then says where each frame lies: a frame inside ONE slice has an address, as a frame of a
 * contiguous buffer has, and takes every path such a frame takes — staged by the same launches or read in place; a frame across several
 * slices has none, and the places that would read its bytes from an address read them piece by piece instead:
 *   qfStagePieces      a part with such a frame is staged by ONE qzstd_hip_group_pieces launch over all its rows (the delta parts' rule),
 *                      a piece per (slice x frame) with the slice's base beside it
 *   qfFramePiecesD2H   the raw-bytes path of qfDeviceFrame: one device->host copy per piece into the buffer the single copy fills
 *   qfDiffPass         (qzstd_frontend.c) delta skip: a qzstd_hip_diff row per piece; a frame is equal when none of its rows' flags is set
 * Everything behind the stage never learns where the bytes came from.
 */

/* a row of qzstd_hip_group_pieces and, behind the rows before it, its pieces: with each slice's base beside it */
typedef struct { const QF_SrcMap *sm; qzstd_hip_group_piece_t *pieces; size_t np, multi; } QF_PiecePut;
static void qfPutPieces(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx)
{
    qzstd_hip_group_pieces_row_t *r = (qzstd_hip_group_pieces_row_t *)rows + m;
    QF_PiecePut *x = (QF_PiecePut *)ctx;
    r->dstOff = dstOff;
    r->len = (uint32_t)fm->len;
    r->pad = pad;
    r->elem = fm->k;
    r->piece0 = (uint32_t)x->np;
    r->nPieces = fm->np;
    r->reserved = 0;
    qfSrcFrameTable(x->sm, fm->p0, fm->np, fm->off, fm->len, 1, &x->pieces[x->np]);
    x->np += fm->np;
    if (fm->np > 1u) x->multi++;
}

static int qfStagePieces(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr, size_t stageBytes)
{
    const QF_DevFrame *f0 = &j->frames[pr->f0];
    const size_t nf = pr->f1 - pr->f0;
    QF_PiecePut x;
    size_t c, np = 0;
    if (!qzstd_hip_group_pieces || !j->sm || pr->diff) return -1; /* (the differencing gather knows no pieces: the call has refused them) */
    for (c = 0; c < nf; c++) np += f0[c].np;
    if (np > 0xFFFFFFFFu) return -1;
    x.sm = j->sm;
    x.np = x.multi = 0;
    if (!(x.pieces = (qzstd_hip_group_piece_t *)qfBufH(&s->pin.pieces, np * sizeof(qzstd_hip_group_piece_t))) ||
        !qfBufD(j->dev, &s->dev.pieces, np * sizeof(qzstd_hip_group_piece_t)) ||
        qfStageRows(j, pr, 0, &s->pin.pieceRows, &s->dev.pieceRows, sizeof(qzstd_hip_group_pieces_row_t), qfPutPieces, &x) != nf)
        return -1;
    if (qzstd_hip_group_pieces(j->dev, s->stream, (const qzstd_hip_group_pieces_row_t *)s->pin.pieceRows.p, (uint32_t)nf,
                               (qzstd_hip_group_pieces_row_t *)s->dev.pieceRows.p, x.pieces, (uint32_t)np, (qzstd_hip_group_piece_t *)s->dev.pieces.p,
                               s->dev.stage.p, stageBytes))
        return -1;
    j->sm->counts[0] += (unsigned long long)x.multi; /* (the calling thread stages; the call adds them to the front's when it has succeeded) */
    j->sm->counts[1] += 1ull;
    return 0;
}

/* queues the copies of a frame's pieces (base: of their bases) to to[0 .. len) on `stream`; the caller waits */
static int qfFramePiecesD2H(const QF_DevPart *pt, void *stream, const QF_DevFrame *fm, unsigned char *to, int base)
{
    uint32_t k;
    if (!pt->sm) return -1;
    for (k = 0; k < fm->np; k++) {
        const QF_SrcPiece *q = &pt->sm->pieces[fm->p0 + k];
        size_t lo, hi;
        qfPieceInFrame(q, fm->off, fm->len, &lo, &hi);
        if (qzstd_hip_memcpy_d2h(pt->dev, stream, to + (lo - fm->off), (base ? q->base : q->src) + (lo - q->off), hi - lo)) return -1;
    }
    return 0;
}

/* an allocation known to be memory of the call's device (qzstd_hip_pointer_extent): a column view's 10^5 rows lie in ONE, and a look-up
 * costs some 75 ns — four per slice with a base would be 20 ms of a call that takes 20 */
typedef struct { const unsigned char *lo, *hi; } QF_SrcExtent;

/* is [p, p + n), n > 0, memory of ONE device, and of *dev when that is set (it is set here otherwise)?  Inside the known allocation: yes,
 * without a look-up.  Else the allocation that holds p becomes the known one where the device layer tells it, and a range that leaves it —
 * or a device layer that tells none — is looked up at its first and its last byte, as a buffer of the batch calls is. */
static int qfSrcRangeOnDevice(const unsigned char *p, size_t n, int *dev, QF_SrcExtent *known)
{
    int d;
    if (known->lo && p >= known->lo && p < known->hi && n <= (size_t)(known->hi - p)) return 0;
    if (qzstd_hip_pointer_extent) {
        const void *lo = NULL;
        size_t size = 0;
        d = qzstd_hip_pointer_extent(p, &lo, &size);
        /* the extent is taken only when its LAST byte looks up as memory of the same device too: an address range that is reserved but
         * only partly mapped (a virtual-memory allocation that grows) fails that, and its ranges are then looked up one by one */
        if (d >= 0 && (*dev < 0 || d == *dev) && size && qzstd_hip_pointer_device((const unsigned char *)lo + size - 1u) == d) {
            known->lo = (const unsigned char *)lo;
            known->hi = known->lo + size;
        }
    } else {
        d = qzstd_hip_pointer_device(p);
    }
    if (d < 0 || (*dev >= 0 && d != *dev)) return -1;
    *dev = d;
    if (known->lo && p >= known->lo && p < known->hi && n <= (size_t)(known->hi - p)) return 0;
    return qzstd_hip_pointer_device(p + n - 1) == d ? 0 : -1;
}

/* a call's source slices, checked, looked up and merged into pieces: the map and what it points to (qfSrcMapFree) */
typedef struct {
    QF_SrcMap sm;
    QF_SrcPiece *pieces;
    size_t *first;
    QZSTD_DeviceBuf *bufs, *bases; /* nBufs each: the sizes, and the address of a buffer's first byte (its base's; NULL and 0: none) */
    size_t nSlices;                /* the non-empty ones */
    int anyBase;
    unsigned long long counts[2];  /* sm.counts */
} QF_SrcSlices;

static void qfSrcMapFree(QF_SrcSlices *o)
{
    free(o->pieces);
    free(o->first);
    free(o->bufs);
}

/* the slice list of QZSTD_frontCompressDeviceSlices and of the calls of qzstd_slicecheck.c: the host-side checks (nothing has touched a
 * GPU when one of them fails), the look-ups of the memory, and the map of the non-empty slices — slices that follow each other in memory,
 * bases included, are ONE piece.  withBases 0: d_base is ignored — not checked, not looked up, not part of the merging rule, and no piece
 * has one.  0, or -1 with nothing to free. */
static int qfSrcMapBuild(const QZSTD_Front *f, const size_t *bufSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices, size_t nSlices, int withBases,
                         QF_SrcSlices *o)
{
    QF_SrcPiece *pieces;
    QZSTD_DeviceBuf *bufs, *bases;
    size_t *first;
    size_t i, b = 0, last = 0, at = 0, nPieces = 0, m = 0;
    int mode = -1, anyBase = 0, dev = -1;
    memset(o, 0, sizeof(*o));
    if (!f || (nBufs && !bufSizes) || (nSlices && !slices) || nBufs > 0xFFFFFFFFu) return -1;
    /* the non-empty slices, in order, tile every buffer; a buffer's slices all carry a base or none does */
    for (i = 0; i < nSlices; i++) {
        const QZSTD_DeviceSrcSlice *s = &slices[i];
        if (s->buf >= nBufs || s->buf < last) return -1; /* (empty slices too are in their buffers' order) */
        last = s->buf;
        if (s->offset > bufSizes[s->buf] || s->size > bufSizes[s->buf] - s->offset) return -1;
        if (!s->size) continue;
        for (; b < s->buf; b++, at = 0, mode = -1)
            if (at != bufSizes[b]) return -1; /* the buffer before ends short */
        if (s->offset != at || !s->d_src) return -1; /* a gap, an overlap or out of order */
        if (withBases) {
            if (mode >= 0 && mode != (s->d_base != NULL)) return -1;
            mode = s->d_base != NULL;
            anyBase |= mode;
        }
        at += s->size;
        nPieces++;
    }
    for (; b < nBufs; b++, at = 0)
        if (at != bufSizes[b]) return -1;
    if (!qzstd_hip_pointer_device) return -1; /* a device layer without the device-input entry points */
    {
        /* sources (and bases) that follow each other in memory are ONE range, as in the Slices restore; a range is looked up when it ends */
        const unsigned char *d0 = NULL, *dEnd = NULL, *b0 = NULL, *bEnd = NULL;
        QF_SrcExtent dKnown = { NULL, NULL }, bKnown = { NULL, NULL };
        for (i = 0; i < nSlices; i++) {
            const unsigned char *p = (const unsigned char *)slices[i].d_src, *q = withBases ? (const unsigned char *)slices[i].d_base : NULL;
            if (!slices[i].size) continue;
            if (p != dEnd) {
                if (dEnd && qfSrcRangeOnDevice(d0, (size_t)(dEnd - d0), &dev, &dKnown)) return -1;
                d0 = p;
            }
            dEnd = p + slices[i].size;
            if (q != bEnd || !q) {
                if (bEnd && qfSrcRangeOnDevice(b0, (size_t)(bEnd - b0), &dev, &bKnown)) return -1;
                b0 = q;
            }
            bEnd = q ? q + slices[i].size : NULL;
        }
        if (dEnd && qfSrcRangeOnDevice(d0, (size_t)(dEnd - d0), &dev, &dKnown)) return -1;
        if (bEnd && qfSrcRangeOnDevice(b0, (size_t)(bEnd - b0), &dev, &bKnown)) return -1;
    }
    pieces = (QF_SrcPiece *)malloc((nPieces + 1u) * sizeof(*pieces));
    first = (size_t *)malloc((nBufs + 1u) * sizeof(*first));
    bufs = (QZSTD_DeviceBuf *)calloc(2u * nBufs + 1u, sizeof(*bufs));
    if (!pieces || !first || !bufs) { free(pieces); free(first); free(bufs); return -1; }
    bases = bufs + nBufs;
    for (i = 0, b = 0; b < nBufs; b++) {
        first[b] = m;
        bufs[b].size = bufSizes[b];
        for (; i < nSlices && slices[i].buf == b; i++) {
            const unsigned char *base = withBases ? (const unsigned char *)slices[i].d_base : NULL;
            if (!slices[i].size) continue;
            if (m > first[b] && pieces[m - 1].src + pieces[m - 1].size == (const unsigned char *)slices[i].d_src &&
                (pieces[m - 1].base ? pieces[m - 1].base + pieces[m - 1].size : NULL) == base) {
                pieces[m - 1].size += slices[i].size; /* it follows the slice before in memory, and so does its base: one piece */
                continue;
            }
            pieces[m].off = slices[i].offset;
            pieces[m].size = slices[i].size;
            pieces[m].src = (const unsigned char *)slices[i].d_src;
            pieces[m].base = base;
            m++;
        }
        if (m > first[b]) {
            /* the address of the buffer's first byte: the buffer's own when its slices follow each other in memory */
            bufs[b].d_ptr = pieces[first[b]].src;
            if (pieces[first[b]].base) { bases[b].d_ptr = pieces[first[b]].base; bases[b].size = bufSizes[b]; }
        }
        o->sm.total += bufSizes[b];
    }
    first[nBufs] = m;
    o->pieces = pieces;
    o->first = first;
    o->bufs = bufs;
    o->bases = bases;
    o->nSlices = nPieces;
    o->anyBase = anyBase;
    o->sm.pieces = pieces;
    o->sm.first = first;
    o->sm.dev = dev;
    o->sm.counts = o->counts;
    /* (chunkSize is fixed when the front is created: reading it needs no lock) */
    for (b = 0; b < nBufs && !o->sm.multi; b++) {
        size_t off, p = first[b];
        for (off = 0; off < bufSizes[b] && !o->sm.multi; off += f->p.chunkSize)
            o->sm.multi = qfSrcFramePieces(&o->sm, &p, off, bufSizes[b] - off < f->p.chunkSize ? bufSizes[b] - off : f->p.chunkSize) > 1u;
    }
    return 0;
}

size_t QZSTD_frontCompressDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs,
                                       const QZSTD_DeviceSrcSlice *slices, size_t nSlices, void *stream, void *dst, size_t dstCapacity,
                                       size_t *frameSizes, size_t *firstFrame)
{
    QF_SrcSlices o;
    size_t i, ret;
    /* host-side checks: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufSizes) || (nSlices && !slices) || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    for (i = 0; i < nBufs; i++)
        if (((elemSizes && elemSizes[i] ? elemSizes[i] : f->group) & QZSTD_ELEM_DIFF) != 0u) return (size_t)-1; /* the differencing gather knows no pieces */
    if (qfSrcMapBuild(f, bufSizes, nBufs, slices, nSlices, 1, &o)) return (size_t)-1;
    ret = qfCompressDevice(f, o.bufs, o.anyBase ? o.bases : NULL, &o.sm, elemSizes, nBufs, 1, stream, dst, dstCapacity, frameSizes, firstFrame);
    if (ret != (size_t)-1) {
        __atomic_fetch_add(&f->srcSliceStats[0], (unsigned long long)o.nSlices, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->srcSliceStats[1], (unsigned long long)o.sm.total, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->srcSliceStats[2], o.counts[0], __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->srcSliceStats[3], o.counts[1], __ATOMIC_RELAXED);
    }
    qfSrcMapFree(&o);
    return ret;
}

void QZSTD_frontSrcSliceStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->srcSliceStats : NULL, stats, 4); }
