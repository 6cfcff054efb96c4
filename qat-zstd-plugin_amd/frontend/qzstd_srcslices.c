/*
 * qzstd_srcslices.c — QZSTD_frontCompressDeviceSlices (include/qzstd_frontend_device.h): the Delta compress call for buffers that are not
 * contiguous in device memory.  Included by qzstd_frontend.c (its types and helpers are used as they are).
 *
 * The call checks its slices, looks their memory up (qfSrcMapBuild, which the calls of qzstd_slicecheck.c use too) and hands qfCompressDevice a map of the non-empty ones (QF_SrcMap: slices that follow each
 * other in memory, bases included, are one piece there) beside a buffer table that holds the sizes.  The per-frame table then says where each frame lies: a frame inside ONE slice has an address, as a frame of a contiguous
 * buffer has, and takes every path such a frame takes — staged by the same launches or read in place; a frame across several slices has
 * none, and the three places that would read its bytes from an address read them piece by piece instead:
 *   qfStagePieces      a part with such a frame is staged by ONE qzstd_hip_group_pieces launch over all its rows (the delta parts' rule),
 *                      a piece per (slice x frame) with the slice's base beside it
 *   qfFramePiecesD2H   the raw-bytes path of qfDeviceFrame: one device->host copy per piece into the buffer the single copy fills
 *   qfDiffPassSlices   delta skip: a qzstd_hip_diff row per piece; a frame is equal when none of its rows' flags is set
 * Everything behind the stage never learns where the bytes came from.
 */

/* piece q of the map, cut to the frame: its bytes [*lo, *hi) of the buffer */
static void qfPieceInFrame(const QF_SrcPiece *q, const QF_DevFrame *fm, size_t *lo, size_t *hi)
{
    *lo = q->off > fm->off ? q->off : fm->off;
    *hi = q->off + q->size < fm->off + fm->len ? q->off + q->size : fm->off + fm->len;
}

static int qfStagePieces(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr, size_t stageBytes)
{
    const QF_DevFrame *f0 = &j->frames[pr->f0];
    const size_t nf = pr->f1 - pr->f0;
    size_t c, so = 0, np = 0, m = 0, multi = 0;
    void *h;
    if (!qzstd_hip_group_pieces || !j->sm || nf > 0xFFFFFFFFu) return -1;
    for (c = 0; c < nf; c++) np += f0[c].np;
    if (np > 0xFFFFFFFFu) return -1;
    h = s->hPieceRows;
    if (qfGrowH(&h, &s->hPieceRowsCap, nf * sizeof(qzstd_hip_group_pieces_row_t))) return -1;
    s->hPieceRows = (qzstd_hip_group_pieces_row_t *)h;
    h = s->hPieces;
    if (qfGrowH(&h, &s->hPiecesCap, np * sizeof(qzstd_hip_group_piece_t))) return -1;
    s->hPieces = (qzstd_hip_group_piece_t *)h;
    if (qfGrowD(j->dev, &s->dPieceRows, &s->dPieceRowsCap, nf * sizeof(qzstd_hip_group_pieces_row_t)) ||
        qfGrowD(j->dev, &s->dPieces, &s->dPiecesCap, np * sizeof(qzstd_hip_group_piece_t)))
        return -1;
    for (c = 0; c < nf; so += qfPad16(f0[c].len), c++) {
        qzstd_hip_group_pieces_row_t *r = &s->hPieceRows[c];
        uint32_t k;
        if (f0[c].len > 0xFFFFFFE0u || f0[c].diff) return -1;
        r->dstOff = so;
        r->len = (uint32_t)f0[c].len;
        r->pad = (uint32_t)(qfPad16(f0[c].len) - f0[c].len) + (c + 1 == nf ? 16u : 0u);
        r->elem = f0[c].k;
        r->piece0 = (uint32_t)m;
        r->nPieces = f0[c].np;
        r->reserved = 0;
        for (k = 0; k < f0[c].np; k++, m++) {
            const QF_SrcPiece *q = &j->sm->pieces[f0[c].p0 + k];
            qzstd_hip_group_piece_t *p = &s->hPieces[m];
            size_t lo, hi;
            qfPieceInFrame(q, &f0[c], &lo, &hi);
            p->src = (uint64_t)(uintptr_t)(q->src + (lo - q->off));
            p->base = q->base ? (uint64_t)(uintptr_t)(q->base + (lo - q->off)) : 0u;
            p->off = (uint32_t)(lo - f0[c].off);
            p->len = (uint32_t)(hi - lo);
        }
        if (f0[c].np > 1u) multi++;
    }
    if (qzstd_hip_group_pieces(j->dev, s->stream, s->hPieceRows, (uint32_t)nf, (qzstd_hip_group_pieces_row_t *)s->dPieceRows, s->hPieces, (uint32_t)np,
                               (qzstd_hip_group_piece_t *)s->dPieces, s->dStage, stageBytes))
        return -1;
    j->sm->counts[0] += (unsigned long long)multi; /* (the calling thread stages; the call adds them to the front's when it has succeeded) */
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
        qfPieceInFrame(q, fm, &lo, &hi);
        if (qzstd_hip_memcpy_d2h(pt->dev, stream, to + (lo - fm->off), (base ? q->base : q->src) + (lo - q->off), hi - lo)) return -1;
    }
    return 0;
}

/* qfDiffPass for a call with source slices: the same launch, copy, wait, zero frames and counters; a compared frame has a row per piece
 * (rows of its own, so that a frame's flags are its own), and is equal when none of them is set */
static int qfDiffPassSlices(QZSTD_Front *f, QF_DevSlot *s, int dev, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const QF_SrcMap *sm,
                            size_t nBufs, size_t nFrames, unsigned char *equal, unsigned char *dst, size_t *frameSizes)
{
    const size_t chunk = f->p.chunkSize;
    QF_ZeroHash z;
    size_t i, off, c = 0, rows = 0, frames = 0, r = 0, nEqual = 0, p;
    unsigned long long bytes = 0;
    void *h;
    memset(equal, 0, nFrames);
    memset(&z, 0, sizeof(z));
    for (i = 0; i < nBufs; i++) {
        if (!bases[i].d_ptr) continue;
        for (off = 0, p = sm->first[i]; off < bufs[i].size; off += chunk, frames++)
            rows += qfSrcFramePieces(sm, &p, off, bufs[i].size - off < chunk ? bufs[i].size - off : chunk);
    }
    if (rows == 0) return 0;
    if (rows > 0xFFFFFFFFu || chunk > 0xFFFFFFE0u) return -1;
    if (qfZeroFrameBound(chunk) > f->stride) return -1;
    h = s->hDiffRows;
    if (qfGrowH(&h, &s->hDiffRowsCap, rows * sizeof(qzstd_hip_diff_row_t))) return -1;
    s->hDiffRows = (qzstd_hip_diff_row_t *)h;
    h = s->hDiffFlags;
    if (qfGrowH(&h, &s->hDiffFlagsCap, rows * sizeof(uint32_t))) return -1;
    s->hDiffFlags = (uint32_t *)h;
    if (qfGrowD(dev, &s->dDiffRows, &s->dDiffRowsCap, rows * sizeof(qzstd_hip_diff_row_t)) ||
        qfGrowD(dev, &s->dDiffFlags, &s->dDiffFlagsCap, rows * sizeof(uint32_t)))
        return -1;
    for (i = 0; i < nBufs; i++) {
        if (!bases[i].d_ptr) continue;
        for (off = 0, p = sm->first[i]; off < bufs[i].size; off += chunk) {
            QF_DevFrame fm;
            size_t np, k;
            fm.off = off;
            fm.len = bufs[i].size - off < chunk ? bufs[i].size - off : chunk;
            np = qfSrcFramePieces(sm, &p, off, fm.len);
            for (k = 0; k < np; k++, r++) {
                const QF_SrcPiece *q = &sm->pieces[p + k];
                qzstd_hip_diff_row_t *row = &s->hDiffRows[r];
                size_t lo, hi;
                qfPieceInFrame(q, &fm, &lo, &hi);
                row->a = (uint64_t)(uintptr_t)(q->src + (lo - q->off));
                row->b = (uint64_t)(uintptr_t)(q->base + (lo - q->off));
                row->len = (uint32_t)(hi - lo);
                row->tile0 = 0;
            }
            bytes += fm.len;
        }
    }
    if (qzstd_hip_diff(dev, s->stream, s->hDiffRows, (uint32_t)rows, (qzstd_hip_diff_row_t *)s->dDiffRows, (uint32_t *)s->dDiffFlags) ||
        qzstd_hip_memcpy_d2h(dev, s->stream, s->hDiffFlags, s->dDiffFlags, rows * sizeof(uint32_t)))
        return -1;
    if (qzstd_hip_stream_wait(dev, s->stream, QF_DEV_WAIT_MS) != 0) {
        (void)qzstd_hip_stream_sync(dev, s->stream); /* the launch still reads the caller's slices */
        return -1;
    }
    for (i = 0, r = 0; i < nBufs; i++) {
        const size_t nf = bufs[i].size / chunk + (bufs[i].size % chunk != 0);
        if (bases[i].d_ptr) {
            for (off = 0, p = sm->first[i]; off < nf; off++) {
                const size_t len = bufs[i].size - off * chunk < chunk ? bufs[i].size - off * chunk : chunk;
                size_t np = qfSrcFramePieces(sm, &p, off * chunk, len);
                uint32_t any = 0;
                for (; np; np--, r++) any |= s->hDiffFlags[r];
                if (any) continue;
                equal[c + off] = 1;
                frameSizes[c + off] = qfZeroFrame(dst + (c + off) * f->stride, len, f->checksum, &z, chunk);
                nEqual++;
            }
        }
        c += nf;
    }
    __atomic_fetch_add(&f->skipStats[0], (unsigned long long)frames, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->skipStats[1], (unsigned long long)nEqual, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->skipStats[2], bytes, __ATOMIC_RELAXED);
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

void QZSTD_frontSrcSliceStats(QZSTD_Front *f, unsigned long long stats[4])
{
    int k;
    if (!stats) return;
    for (k = 0; k < 4; k++) stats[k] = f ? __atomic_load_n(&f->srcSliceStats[k], __ATOMIC_RELAXED) : 0ull;
}
