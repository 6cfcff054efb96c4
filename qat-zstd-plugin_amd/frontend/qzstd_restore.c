/*
 * qzstd_restore.c — the way back of the device calls (include/qzstd_frontend_device.h: QZSTD_frontRestoreDeviceBatchTyped,
 * QZSTD_frontRestoreDevice, QZSTD_frontRestoreStats): zstd frames in host memory, decoded by the front's workers and scattered into device
 * buffers, the byte-grouped layout undone on the GPU.  Part of qzstd_frontend.c's translation unit (it is included at that file's end and
 * uses its types and helpers), so that the front-end stays ONE source to whoever builds it.
 *
 * The frames of a call are cut into PARTS of whole frames (at most QF_PART_BYTES of content, $QZSTD_FRONT_DEVICE_PART as on the compress
 * side).  Per part, on one of two restore slots (pinned host buffer + device stage + stream, kept with the front between calls):
 *   - the workers decode the part's frames into the slot's pinned buffer, every frame at a 16-aligned offset, each worker with a ZSTD_DCtx
 *     of its own (created on first use); a frame must decode to exactly its chunk's length;
 *   - the calling thread queues ONE host->device copy of the buffer and ONE qzstd_hip_ungroup launch (a row per frame: its destination in
 *     the caller's buffer, its element size) on the slot's stream — and hands the workers the next part, which goes to the other slot.
 * A slot's pinned buffer and rows are written again only after its stream has passed the copy and the launch that read them.
 * QZSTD_frontRestoreDeviceBatchDelta: a part with a frame whose buffer has a base is scattered by ONE qzstd_hip_ungroup_xor launch instead (base 0
 * for the rows without one): the frames' content is chunk XOR base chunk, and the base — which may be the destination itself — is XORed back
 * in on the way out.  Decoding, the pinned buffers and the copy are the same.  With QZSTD_frontSetDeltaSkip on, a frame of a based buffer that
 * IS the canonical zero frame of its chunk's length (qfIsZeroFrame, qzstd_frontend.c) is left out of the table and the parts: in place
 * nothing happens for it, otherwise a run of such frames is one device->device copy from the base.
 * QZSTD_frontRestoreDeviceSlices (below the whole-buffer calls): byte ranges of the written buffers; only the frames they intersect are decoded,
 * cut into parts the same way, and a part is scattered by ONE qzstd_hip_ungroup_window launch, a row per piece (slice x frame).
 * QZSTD_frontVerifyDeviceBatch (qzstd_verify.c, included behind this file) uses the same slots and the same decode, and compares where these
 * calls scatter.
 * Every call is built on the scaffold of qzstd_frontend.c (qfCallBegin .. qfCallEnd: the look-ups, devBusy, the restore side's two slots, the
 * event pair, the closing waits); the slots' buffers are QF_RestoreSlot's, there too.
 * Nothing of the producer (the match-finder service, the announcements) is used: a front created with useProducer = 0 restores as well.
 */

extern int qzstd_hip_ungroup(int device, void *stream, const qzstd_hip_ungroup_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_row_t *d_rows,
                             const void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_ungroup_xor(int device, void *stream, const qzstd_hip_ungroup_xor_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_xor_row_t *d_rows,
                                 const void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_esum(int device, void *stream, qzstd_hip_esum_row_t *rows, uint32_t nRows, qzstd_hip_esum_row_t *d_rows, void *d_scratch,
                          size_t scratchBytes) __attribute__((weak));
extern int qzstd_hip_ungroup_window(int device, void *stream, qzstd_hip_ungroup_win_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_win_row_t *d_rows,
                                    const void *d_stage, size_t stageBytes) __attribute__((weak));

/* one frame of a restore job (the per-frame table, built once per call) */
typedef struct {
    const unsigned char *src; /* the frame, host memory */
    size_t srcSize;
    unsigned char *d_dst;     /* where its content belongs: device memory */
    const unsigned char *d_base; /* what is XORed into it on the way there: device memory, or NULL */
    size_t len;               /* the chunk's length: what the frame must decode to */
    size_t at;                /* offset in its part's stage, a multiple of 16 */
    uint32_t k;               /* element size of the byte-grouped layout the content is in; 1: the bytes as they are */
    uint32_t diff;            /* QZSTD_ELEM_DIFF: the content is differences, summed on the device after the scatter */
} QF_RestoreFrame;

typedef struct { size_t f0, f1, bytes, stage, based, diffs; } QF_RestoreRange; /* frames [f0, f1): content bytes, stage bytes (16-aligned frames), frames with a base, differenced frames */
typedef struct { unsigned char *d_dst; const unsigned char *d_src; size_t len; } QF_ZeroRun; /* consecutive recognised zero frames of one buffer: base -> destination */

/* the part the workers decode (QZSTD_Front.restore) */
struct QF_RestorePart_s {
    const QF_RestoreFrame *frames; /* the job's table */
    size_t f0;                     /* chunk c of the workers' job is frame f0 + c */
    unsigned char *hStage;
    unsigned char *bad; /* NULL, or a byte per frame of the table: set to 1 for the frame a worker stopped at (QZSTD_frontVerifyDeviceBatch) */
};

/* a worker's share of a part: chunks [c0, c1) of the job are frames of f->restore */
static int qfRestoreSegment(QZSTD_Front *f, QF_Worker *w, const QF_Seg *sg)
{
    const struct QF_RestorePart_s *p = f->restore;
    size_t c;
    if (!w->zd && !(w->zd = ZSTD_createDCtx())) return -1;
    for (c = sg->c0; c < sg->c1; c++) {
        const QF_RestoreFrame *fr = &p->frames[p->f0 + c];
        /* capacity = the chunk's length: a longer content is an error of libzstd's, a shorter one shows in the return value; a frame with a
         * content checksum is verified by the decoder */
        const size_t r = ZSTD_decompressDCtx(w->zd, p->hStage + fr->at, fr->len, fr->src, fr->srcSize);
        if (ZSTD_isError(r) || r != fr->len) {
            if (p->bad) p->bad[p->f0 + c] = 1;
            return -1;
        }
    }
    return 0;
}

/* the workers decode frames [f0, f0 + nf) of the table into hStage; -> 0, or -1: a frame that does not decode, decodes to another length or
 * fails its checksum (bad: NULL, or a byte per frame of the table, set for the frame a worker stopped at) */
static int qfRestoreDecode(QZSTD_Front *f, const QF_RestoreFrame *table, size_t f0, size_t nf, unsigned char *hStage, unsigned char *bad)
{
    struct QF_RestorePart_s part;
    int failed;
    part.frames = table;
    part.f0 = f0;
    part.hStage = hStage;
    part.bad = bad;
    pthread_mutex_lock(&f->mu);
    f->restore = &part;
    f->src = NULL;
    f->srcSize = 0;
    failed = qfRunJobLocked(f, nf);
    f->restore = NULL;
    pthread_mutex_unlock(&f->mu);
    return failed ? -1 : 0;
}

/* what every restore part counts once its copy and scatter are queued */
static void qfRestoreCount(QZSTD_Front *f, size_t nf, size_t bytes, size_t stage, size_t based)
{
    __atomic_fetch_add(&f->restoreStats[0], (unsigned long long)nf, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->restoreStats[1], (unsigned long long)bytes, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->restoreStats[2], (unsigned long long)stage, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->restoreStats[3], 1ull, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->deltaStats[3], (unsigned long long)based, __ATOMIC_RELAXED);
}

static size_t qfRestoreDevice(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                              const QZSTD_DeviceOutBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes, size_t nBufs, void *stream)
{
    QF_RestoreFrame *table = NULL;
    QF_RestoreRange *parts = NULL;
    QF_ZeroRun *runs = NULL; /* delta skip: what the recognised zero frames leave to do, a device->device copy per run */
    unsigned char *scratch = NULL;
    QF_ZeroHash zh;
    QF_Call call;
    QF_RestoreSlot *slot;
    size_t i, c = 0, m = 0, k, nParts = 0, want = 0, partBytes, pos = 0, nRuns = 0, nZero = 0;
    int dev, rc = 0, anyBase = 0, anyDiff = 0, skip;
    /* host-side checks: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufs) || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    for (i = 0; i < nBufs; i++) {
        unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : f->group;
        if (!bufs[i].d_ptr && bufs[i].size) return (size_t)-1;
        if (e & QZSTD_ELEM_DIFF) {
            /* differences: with the buffer's own element size only (0x80 alone is refused), and not against a base */
            if (bases && (bases[i].d_ptr || bases[i].size)) return (size_t)-1;
            anyDiff = 1;
            e &= ~QZSTD_ELEM_DIFF;
        }
        if (e != 1u && e != 2u && e != 4u && e != 8u) return (size_t)-1;
        want += bufs[i].size / f->p.chunkSize + (bufs[i].size % f->p.chunkSize != 0);
    }
    if (want != nFrames || (nFrames && (!frames || !frameSizes))) return (size_t)-1;
    /* a base is none ({NULL, 0}) or as large as its buffer; a call without any is the call without the argument */
    for (i = 0; bases && i < nBufs; i++) {
        if (!bases[i].d_ptr && !bases[i].size) continue;
        if (!bases[i].d_ptr || bases[i].size != bufs[i].size) return (size_t)-1;
        if (bases[i].size) anyBase = 1;
    }
    if (!anyBase) bases = NULL;
    if (!qzstd_hip_ungroup || !qzstd_hip_pointer_device || !qzstd_hip_event_create || !qzstd_hip_event_record || !qzstd_hip_stream_wait_event ||
        !qzstd_hip_event_destroy)
        return (size_t)-1; /* a device layer without the ungrouping scatter, or without the device-input entry points at all */
    if (bases && !qzstd_hip_ungroup_xor) return (size_t)-1; /* a base given and a device layer that cannot XOR one in */
    if (anyDiff && !qzstd_hip_esum) return (size_t)-1;      /* differences to sum and a device layer that cannot */
    call.f = f;
    call.restore = 1;
    call.nStreams = 2;
    call.dev = -1;
    for (i = 0; i < nBufs; i++) /* (qfCallBufs with destinations for buffers) */
        if (qfCallRange(&call, bufs[i].d_ptr, bufs[i].size) || (bases && bases[i].d_ptr && qfCallRange(&call, bases[i].d_ptr, bases[i].size)))
            return (size_t)-1;
    if (nFrames == 0) return 0; /* (an empty call takes nothing, as on the compress side) */
    if (qfCallBegin(&call, stream)) return (size_t)-1;
    dev = call.dev;
    slot = f->restoreSlot;

    partBytes = qfPartBytes();
    table = (QF_RestoreFrame *)malloc(nFrames * sizeof(*table));
    parts = (QF_RestoreRange *)malloc(nFrames * sizeof(*parts));
    if (!table || !parts) rc = -1;
    /* delta skip: a frame of a buffer with a base that IS the canonical zero frame of its chunk's length says "equal to the base" — it is not
     * decoded and gets no place in the table (frame m of the table is the m-th remaining one), in the pinned buffer or in the stage */
    skip = bases && f->deltaSkip && qzstd_hip_memcpy2d_d2d;
    memset(&zh, 0, sizeof(zh));
    if (skip && rc == 0) {
        runs = (QF_ZeroRun *)malloc(nFrames * sizeof(*runs));
        scratch = (unsigned char *)malloc(qfZeroFrameBound(f->p.chunkSize));
        if (!runs || !scratch) rc = -1;
    }
    for (i = 0; i < nBufs && rc == 0; i++) {
        const unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : f->group;
        const unsigned char *base = bases && bases[i].d_ptr ? (const unsigned char *)bases[i].d_ptr : NULL;
        size_t off, lastZero = nFrames; /* the last recognised frame of this buffer (nFrames: none yet) */
        for (off = 0; off < bufs[i].size; off += f->p.chunkSize, pos += frameSizes[c], c++) {
            const size_t len = bufs[i].size - off < f->p.chunkSize ? bufs[i].size - off : f->p.chunkSize;
            const unsigned char *src = (const unsigned char *)frames + (frameStride ? c * frameStride : pos);
            QF_RestoreRange *cur = nParts ? &parts[nParts - 1] : NULL;
            if (skip && base && qfIsZeroFrame(src, frameSizes[c], len, scratch, &zh, f->p.chunkSize)) {
                nZero++;
                if (base == (const unsigned char *)bufs[i].d_ptr) continue; /* in place: the chunk is what it shall be */
                if (lastZero == c - 1u) {
                    runs[nRuns - 1].len += len; /* consecutive chunks: one copy */
                } else {
                    runs[nRuns].d_dst = (unsigned char *)bufs[i].d_ptr + off;
                    runs[nRuns].d_src = base + off;
                    runs[nRuns++].len = len;
                }
                lastZero = c;
                continue;
            }
            if (len > 0xFFFFFFE0u || (cur && cur->f1 - cur->f0 >= 0xFFFFFFFFu)) { rc = -1; break; } /* (a row's length and a launch's rows are 32-bit) */
            if (!cur || cur->bytes + len > partBytes) {
                cur = &parts[nParts++];
                cur->f0 = m;
                cur->bytes = cur->stage = cur->based = cur->diffs = 0;
            }
            table[m].src = src;
            table[m].srcSize = frameSizes[c];
            table[m].d_dst = (unsigned char *)bufs[i].d_ptr + off;
            table[m].d_base = base ? base + off : NULL;
            if (table[m].d_base) cur->based++;
            table[m].len = len;
            table[m].at = cur->stage;
            table[m].k = e & ~QZSTD_ELEM_DIFF;
            table[m].diff = e & QZSTD_ELEM_DIFF;
            if (table[m].diff) cur->diffs++;
            cur->f1 = ++m;
            cur->bytes += len;
            cur->stage += qfPad16(len);
        }
    }
    /* the recognised frames that are not restored in place: base -> destination, one copy per run of consecutive chunks (a wholly frozen
     * tensor: one copy; a run above 1 GiB is cut there, below the 2D copy's largest pitch), on the slots' streams in turn; the destinations
     * are no other frame's */
    for (k = 0; k < nRuns && rc == 0; k++) {
        size_t at;
        for (at = 0; at < runs[k].len && rc == 0; at += (size_t)1 << 30) {
            const size_t n = runs[k].len - at < ((size_t)1 << 30) ? runs[k].len - at : (size_t)1 << 30;
            if (qzstd_hip_memcpy2d_d2d(dev, slot[k % 2].stream, runs[k].d_dst + at, n, runs[k].d_src + at, n, n, 1)) rc = -1;
        }
    }
    for (k = 0; k < nParts && rc == 0; k++) {
        const QF_RestoreRange *pr = &parts[k];
        const size_t nf = pr->f1 - pr->f0;
        QF_RestoreSlot *s = &slot[k % 2];
        unsigned char *hStage;
        qzstd_hip_ungroup_row_t *rows;
        qzstd_hip_ungroup_xor_row_t *xorRows = NULL;
        qzstd_hip_esum_row_t *sumRows = NULL;
        /* part k - 2 was copied and scattered from this slot: its stream must have passed both before the buffers are written (or grown) */
        if (qzstd_hip_stream_wait(dev, s->stream, QF_DEV_WAIT_MS) != 0) { rc = -1; break; }
        hStage = (unsigned char *)qfBufH(&s->pin.stage, pr->stage);
        rows = hStage ? (qzstd_hip_ungroup_row_t *)qfBufH(&s->pin.rows, nf * sizeof(qzstd_hip_ungroup_row_t)) : NULL;
        if (!rows || !qfBufD(dev, &s->dev.stage, pr->stage) || !qfBufD(dev, &s->dev.rows, nf * sizeof(qzstd_hip_ungroup_row_t))) { rc = -1; break; }
        if (pr->based && (!(xorRows = (qzstd_hip_ungroup_xor_row_t *)qfBufH(&s->pin.xorRows, nf * sizeof(qzstd_hip_ungroup_xor_row_t))) ||
                          !qfBufD(dev, &s->dev.xorRows, nf * sizeof(qzstd_hip_ungroup_xor_row_t)))) {
            rc = -1;
            break;
        }
        if (pr->diffs) {
            /* the differenced frames' destinations, summed in place by one launch behind the scatter */
            size_t tiles = 0, r = 0;
            if (!(sumRows = (qzstd_hip_esum_row_t *)qfBufH(&s->pin.sumRows, pr->diffs * sizeof(qzstd_hip_esum_row_t)))) { rc = -1; break; }
            for (c = 0; c < nf; c++) {
                const QF_RestoreFrame *fr = &table[pr->f0 + c];
                if (!fr->diff) continue;
                sumRows[r].dst = (uint64_t)(uintptr_t)fr->d_dst;
                sumRows[r].len = (uint32_t)fr->len;
                sumRows[r].elem = fr->k;
                sumRows[r].tile0 = 0;
                sumRows[r].reserved = 0;
                tiles += (size_t)QZSTD_HIP_ESUM_TILES(fr->len, fr->k);
                r++;
            }
            if (!qfBufD(dev, &s->dev.sumRows, pr->diffs * sizeof(qzstd_hip_esum_row_t)) ||
                !qfBufD(dev, &s->dev.sumScratch, QZSTD_HIP_ESUM_SCRATCH_BYTES(tiles))) {
                rc = -1;
                break;
            }
        }
        for (c = 0; c < nf; c++) {
            const QF_RestoreFrame *fr = &table[pr->f0 + c];
            if (pr->based) {
                xorRows[c].dst = (uint64_t)(uintptr_t)fr->d_dst;
                xorRows[c].base = (uint64_t)(uintptr_t)fr->d_base;
                xorRows[c].srcOff = fr->at;
                xorRows[c].len = (uint32_t)fr->len;
                xorRows[c].elem = fr->k;
                continue;
            }
            rows[c].dst = (uint64_t)(uintptr_t)fr->d_dst;
            rows[c].srcOff = fr->at;
            rows[c].len = (uint32_t)fr->len;
            rows[c].elem = fr->k;
        }
        if (qfRestoreDecode(f, table, pr->f0, nf, hStage, NULL)) { rc = -1; break; }
        if (qzstd_hip_memcpy_h2d(dev, s->stream, s->dev.stage.p, hStage, pr->stage) ||
            (pr->based ? qzstd_hip_ungroup_xor(dev, s->stream, xorRows, (uint32_t)nf, (qzstd_hip_ungroup_xor_row_t *)s->dev.xorRows.p, s->dev.stage.p, pr->stage)
                       : qzstd_hip_ungroup(dev, s->stream, rows, (uint32_t)nf, (qzstd_hip_ungroup_row_t *)s->dev.rows.p, s->dev.stage.p, pr->stage))) {
            rc = -1;
            break;
        }
        qfRestoreCount(f, nf, pr->bytes, pr->stage, pr->based);
        if (pr->diffs) {
            /* behind the scatter on the same stream: the differences lie at their destinations */
            if (qzstd_hip_esum(dev, s->stream, sumRows, (uint32_t)pr->diffs, (qzstd_hip_esum_row_t *)s->dev.sumRows.p, s->dev.sumScratch.p, s->dev.sumScratch.cap)) {
                rc = -1;
                break;
            }
            __atomic_fetch_add(&f->ediffStats[2], (unsigned long long)pr->diffs, __ATOMIC_RELAXED);
            __atomic_fetch_add(&f->ediffStats[3], 1ull, __ATOMIC_RELAXED);
        }
    }
    if (qfCallWait(&call)) rc = -1;
    if (rc == 0) __atomic_fetch_add(&f->skipStats[3], (unsigned long long)nZero, __ATOMIC_RELAXED);
    free(table);
    free(parts);
    free(runs);
    free(scratch);
    qfCallEnd(&call);
    return rc == 0 ? nFrames : (size_t)-1;
}

size_t QZSTD_frontRestoreDeviceBatchTyped(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                          const QZSTD_DeviceOutBuf *bufs, const unsigned char *elemSizes, size_t nBufs, void *stream)
{
    return qfRestoreDevice(f, frames, frameStride, frameSizes, nFrames, bufs, NULL, elemSizes, nBufs, stream);
}

size_t QZSTD_frontRestoreDeviceBatchDelta(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                          const QZSTD_DeviceOutBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes, size_t nBufs,
                                          void *stream)
{
    return qfRestoreDevice(f, frames, frameStride, frameSizes, nFrames, bufs, bases, elemSizes, nBufs, stream);
}

size_t QZSTD_frontRestoreDevice(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames, void *d_dst,
                                size_t dstSize, void *stream)
{
    QZSTD_DeviceOutBuf one;
    one.d_ptr = d_dst;
    one.size = dstSize;
    return qfRestoreDevice(f, frames, frameStride, frameSizes, nFrames, &one, NULL, NULL, 1, stream);
}

/*
 * QZSTD_frontRestoreDeviceSlices: byte ranges of the buffers as they were written, restored from the frames they intersect and from no other.
 * The needed frames get a table of their own (frame m of the job is the m-th needed one), cut into parts as above; a part's rows are its
 * PIECES (slice x frame, in order: all pieces of a frame follow each other, so they lie in its part), scattered by ONE
 * qzstd_hip_ungroup_window launch.  Decode (qfRestoreDecode), copy and counters (qfRestoreCount) are qfRestoreDevice's.
 */
typedef struct {
    size_t m;                    /* the needed frame it is cut from */
    uint32_t winOff, winLen;     /* the window of that frame's content */
    unsigned char *d_dst;
    const unsigned char *d_base; /* or NULL */
} QF_SlicePiece;
typedef struct { size_t f0, f1, p0, p1, bytes, stage, based; } QF_SliceRange; /* needed frames [f0, f1) and pieces [p0, p1) */

size_t QZSTD_frontRestoreDeviceSlices(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                      const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs,
                                      const QZSTD_DeviceSlice *slices, size_t nSlices, void *stream)
{
    QF_RestoreFrame *table = NULL;
    QF_SliceRange *parts = NULL;
    QF_SlicePiece *pieces = NULL;
    size_t *first = NULL;
    QF_Call call;
    QF_RestoreSlot *slot;
    size_t i, c, k, nParts = 0, want = 0, partBytes, nPieces = 0, nNeeded = 0, np = 0, g = 0, pos = 0, lastG = (size_t)-1, chunk;
    unsigned long long nonEmpty = 0, written = 0;
    int dev = -1, rc = 0;
    /* host-side checks: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufSizes) || (nSlices && !slices) || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    chunk = f->p.chunkSize;
    for (i = 0; i < nBufs; i++) {
        const unsigned e = (elemSizes && elemSizes[i] ? elemSizes[i] : f->group) & ~((elemSizes && elemSizes[i]) ? QZSTD_ELEM_DIFF : 0u);
        if (e != 1u && e != 2u && e != 4u && e != 8u) return (size_t)-1; /* (a differenced buffer: refused below when a slice touches it) */
        want += bufSizes[i] / chunk + (bufSizes[i] % chunk != 0);
    }
    if (want != nFrames || (nFrames && (!frames || !frameSizes))) return (size_t)-1;
    for (i = 0; i < nSlices; i++) {
        const QZSTD_DeviceSlice *s = &slices[i];
        if (s->buf >= nBufs || s->offset > bufSizes[s->buf] || s->size > bufSizes[s->buf] - s->offset) return (size_t)-1;
        if (i && (s->buf < slices[i - 1].buf || (s->buf == slices[i - 1].buf && s->offset < slices[i - 1].offset + slices[i - 1].size)))
            return (size_t)-1; /* not in ascending order, or overlapping in the source */
        if (!s->size) continue;
        if (!s->d_dst) return (size_t)-1;
        if (elemSizes && (elemSizes[s->buf] & QZSTD_ELEM_DIFF)) return (size_t)-1; /* a window needs the sum from its frame's start */
        nPieces += (s->offset + s->size - 1u) / chunk - s->offset / chunk + 1u;
    }
    if (!qzstd_hip_ungroup_window || !qzstd_hip_pointer_device || !qzstd_hip_event_create || !qzstd_hip_event_record || !qzstd_hip_stream_wait_event ||
        !qzstd_hip_event_destroy)
        return (size_t)-1; /* a device layer without the windowed scatter, or without the device-input entry points at all */
    {
        /* destinations (and bases) that follow each other without a gap — a column shard's rows in one contiguous tensor — are ONE range, looked
         * up at its first and its last byte as a buffer of the Typed call is: a look-up costs some 75 ns, and a shard has 10^5 slices */
        const unsigned char *dEnd = NULL, *bEnd = NULL;
        for (i = 0; i < nSlices; i++) {
            const unsigned char *p = (const unsigned char *)slices[i].d_dst, *b = (const unsigned char *)slices[i].d_base;
            if (!slices[i].size) continue;
            if (p != dEnd) {
                int d;
                if (dEnd && qzstd_hip_pointer_device(dEnd - 1) != dev) return (size_t)-1;
                d = qzstd_hip_pointer_device(p);
                if (d < 0 || (dev >= 0 && d != dev)) return (size_t)-1;
                dev = d;
            }
            dEnd = p + slices[i].size;
            if (b != bEnd || !b) {
                if (bEnd && qzstd_hip_pointer_device(bEnd - 1) != dev) return (size_t)-1;
                if (b && qzstd_hip_pointer_device(b) != dev) return (size_t)-1;
            }
            bEnd = b ? b + slices[i].size : NULL;
        }
        if (dEnd && qzstd_hip_pointer_device(dEnd - 1) != dev) return (size_t)-1;
        if (bEnd && qzstd_hip_pointer_device(bEnd - 1) != dev) return (size_t)-1;
    }
    if (nPieces == 0) return 0;
    call.f = f;
    call.restore = 1;
    call.nStreams = 2;
    call.dev = dev; /* (looked up above, a range of slices at a time: the scaffold's look-up is per buffer) */
    if (qfCallBegin(&call, stream)) return (size_t)-1;
    slot = f->restoreSlot;

    partBytes = qfPartBytes();
    table = (QF_RestoreFrame *)malloc(nPieces * sizeof(*table)); /* (no more needed frames than pieces) */
    parts = (QF_SliceRange *)malloc(nPieces * sizeof(*parts));
    pieces = (QF_SlicePiece *)malloc(nPieces * sizeof(*pieces));
    first = (size_t *)malloc((nBufs + 1u) * sizeof(*first));
    if (!table || !parts || !pieces || !first) rc = -1;
    for (i = 0, c = 0; i < nBufs && rc == 0; i++) {
        first[i] = c;
        c += bufSizes[i] / chunk + (bufSizes[i] % chunk != 0);
    }
    for (i = 0; i < nSlices && rc == 0; i++) {
        const QZSTD_DeviceSlice *s = &slices[i];
        const unsigned e = elemSizes && elemSizes[s->buf] ? elemSizes[s->buf] : f->group;
        if (!s->size) continue;
        nonEmpty++;
        written += s->size;
        for (c = s->offset / chunk; c * chunk < s->offset + s->size; c++) {
            const size_t fg = first[s->buf] + c, off = c * chunk;
            const size_t len = bufSizes[s->buf] - off < chunk ? bufSizes[s->buf] - off : chunk;
            const size_t lo = s->offset > off ? s->offset : off, hi = s->offset + s->size < off + len ? s->offset + s->size : off + len;
            QF_SliceRange *cur = nParts ? &parts[nParts - 1] : NULL;
            QF_SlicePiece *pc = &pieces[np];
            if (fg != lastG) { /* a frame not seen yet: the next needed one */
                if (len > 0xFFFFFFE0u) { rc = -1; break; } /* (a row's lengths are 32-bit) */
                if (!cur || cur->bytes + len > partBytes) {
                    cur = &parts[nParts++];
                    cur->f0 = nNeeded;
                    cur->p0 = np;
                    cur->bytes = cur->stage = cur->based = 0;
                }
                for (; !frameStride && g < fg; g++) pos += frameSizes[g]; /* only the sizes of the frames in between are read */
                table[nNeeded].src = (const unsigned char *)frames + (frameStride ? fg * frameStride : pos);
                table[nNeeded].srcSize = frameSizes[fg];
                table[nNeeded].d_dst = NULL;
                table[nNeeded].d_base = NULL;
                table[nNeeded].len = len;
                table[nNeeded].at = cur->stage;
                table[nNeeded].k = e;
                cur->f1 = ++nNeeded;
                cur->bytes += len;
                cur->stage += qfPad16(len);
                lastG = fg;
            }
            if (np - cur->p0 >= 0xFFFFFFFFu) { rc = -1; break; } /* (a launch's rows are 32-bit) */
            pc->m = nNeeded - 1u;
            pc->winOff = (uint32_t)(lo - off);
            pc->winLen = (uint32_t)(hi - lo);
            pc->d_dst = (unsigned char *)s->d_dst + (lo - s->offset);
            pc->d_base = s->d_base ? (const unsigned char *)s->d_base + (lo - s->offset) : NULL;
            if (pc->d_base && !table[pc->m].d_base) { /* (d_base of a needed frame: only the mark that a piece of it has one) */
                table[pc->m].d_base = pc->d_base;
                cur->based++;
            }
            cur->p1 = ++np;
        }
    }
    for (k = 0; k < nParts && rc == 0; k++) {
        const QF_SliceRange *pr = &parts[k];
        const size_t nf = pr->f1 - pr->f0, nr = pr->p1 - pr->p0;
        QF_RestoreSlot *s = &slot[k % 2];
        unsigned char *hStage;
        qzstd_hip_ungroup_win_row_t *rows;
        if (qzstd_hip_stream_wait(dev, s->stream, QF_DEV_WAIT_MS) != 0) { rc = -1; break; }
        hStage = (unsigned char *)qfBufH(&s->pin.stage, pr->stage);
        rows = hStage ? (qzstd_hip_ungroup_win_row_t *)qfBufH(&s->pin.winRows, nr * sizeof(qzstd_hip_ungroup_win_row_t)) : NULL;
        if (!rows || !qfBufD(dev, &s->dev.stage, pr->stage) || !qfBufD(dev, &s->dev.winRows, nr * sizeof(qzstd_hip_ungroup_win_row_t))) { rc = -1; break; }
        for (c = 0; c < nr; c++) {
            const QF_SlicePiece *pc = &pieces[pr->p0 + c];
            qzstd_hip_ungroup_win_row_t *r = &rows[c];
            r->dst = (uint64_t)(uintptr_t)pc->d_dst;
            r->base = (uint64_t)(uintptr_t)pc->d_base;
            r->srcOff = table[pc->m].at;
            r->len = (uint32_t)table[pc->m].len;
            r->elem = table[pc->m].k;
            r->winOff = pc->winOff;
            r->winLen = pc->winLen;
            r->tile0 = r->reserved = 0;
        }
        if (qfRestoreDecode(f, table, pr->f0, nf, hStage, NULL)) { rc = -1; break; }
        if (qzstd_hip_memcpy_h2d(dev, s->stream, s->dev.stage.p, hStage, pr->stage) ||
            qzstd_hip_ungroup_window(dev, s->stream, rows, (uint32_t)nr, (qzstd_hip_ungroup_win_row_t *)s->dev.winRows.p, s->dev.stage.p, pr->stage)) {
            rc = -1;
            break;
        }
        qfRestoreCount(f, nf, pr->bytes, pr->stage, pr->based);
        __atomic_fetch_add(&f->sliceStats[2], (unsigned long long)nf, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->sliceStats[3], (unsigned long long)nr, __ATOMIC_RELAXED);
    }
    if (qfCallWait(&call)) rc = -1;
    if (rc == 0) {
        __atomic_fetch_add(&f->sliceStats[0], nonEmpty, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->sliceStats[1], written, __ATOMIC_RELAXED);
    }
    free(table);
    free(parts);
    free(pieces);
    free(first);
    qfCallEnd(&call);
    return rc == 0 ? nNeeded : (size_t)-1;
}

void QZSTD_frontSliceStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->sliceStats : NULL, stats, 4); }

void QZSTD_frontRestoreStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->restoreStats : NULL, stats, 4); }
