/*
 * qzstd_advise.c — QZSTD_frontAdviseDeviceBatch / QZSTD_frontAdviseStats / QZSTD_ediffCostOf / QZSTD_ediffAdvisedOf
 * (include/qzstd_frontend_device.h): for every buffer of a list of device buffers, whether element differences (QZSTD_ELEM_DIFF) pay — from
 * the order-0 costs of the byte planes with and without differences (include/qzstd_ediffcost.h), taken on the GPU from the tensors' own
 * bytes.  Part of qzstd_frontend.c's translation unit, included behind qzstd_elemdiff.c; like the fingerprint calls it uses the restore's
 * first slot (its stream, and grow-only pinned and device scratch kept there between calls).
 *
 * A call is: the host-side checks of the batch compress call; the scaffold of qzstd_frontend.c (qfCallBegin .. qfCallEnd) with ONE stream;
 * ONE qzstd_hip_ediff_cost launch with a row per chunk that points INTO the caller's buffers (nothing is staged or copied on the device);
 * one device->host copy of the tiles' words (8 bytes per 16 KiB); and the sums per buffer on the calling thread.  Nothing of the producer or
 * the workers is used: a front created with useProducer = 0 serves the call.
 */

extern int qzstd_hip_ediff_cost(int device, void *stream, qzstd_hip_ediff_cost_row_t *rows, uint32_t nRows, qzstd_hip_ediff_cost_row_t *d_rows,
                                uint32_t *d_tiles) __attribute__((weak));

void QZSTD_ediffCostOf(const void *chunk, size_t len, unsigned k, unsigned long long sums[2])
{
    uint64_t s[2] = { 0u, 0u };
    if (!sums) return;
    if (chunk || !len) QZSTD_ediffCostChunk(chunk, len, k, s);
    sums[0] = s[0];
    sums[1] = s[1];
}

int QZSTD_ediffAdvisedOf(unsigned long long P, unsigned long long D) { return QZSTD_ediffAdvised(P, D); }

size_t QZSTD_frontAdviseDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const unsigned char *elemSizes, size_t nBufs, void *stream,
                                    unsigned char *advised, unsigned long long *est)
{
    QF_Call call;
    QF_RestoreSlot *s;
    qzstd_hip_ediff_cost_row_t *rows;
    const uint32_t *tiles;
    size_t i, c = 0, nRows = 0, nTiles = 0, t = 0, nFlagged = 0;
    unsigned long long total = 0;
    int dev, rc = 0;
    /* host-side checks, the batch compress call's: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && (!bufs || !advised)) || nBufs > 0xFFFFFFFFu || f->p.chunkSize > 0xFFFFFFE0u) return (size_t)-1;
    for (i = 0; i < nBufs; i++) {
        const unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : f->group; /* (an entry that carries the flag already is none of 1, 2, 4, 8) */
        const size_t whole = bufs[i].size / f->p.chunkSize, rest = bufs[i].size % f->p.chunkSize;
        if (!bufs[i].d_ptr && bufs[i].size) return (size_t)-1;
        if (e != 1u && e != 2u && e != 4u && e != 8u) return (size_t)-1;
        nRows += whole + (rest != 0);
        nTiles += whole * (size_t)QZSTD_HIP_ESUM_TILES(f->p.chunkSize, e) + (size_t)QZSTD_HIP_ESUM_TILES(rest, e);
    }
    if (nRows > 0xFFFFFFFFu || nTiles > 0x7FFFFFFFu) return (size_t)-1; /* (one launch: 32-bit rows and tiles) */
    if (!qzstd_hip_ediff_cost || !qzstd_hip_pointer_device || !qzstd_hip_event_create || !qzstd_hip_event_record || !qzstd_hip_stream_wait_event ||
        !qzstd_hip_event_destroy)
        return (size_t)-1; /* a device layer without the cost kernel, or without the device-input entry points at all */
    call.f = f;
    call.restore = 1;
    call.nStreams = 1; /* the restore side's first slot alone, as the fingerprint calls */
    call.dev = -1;
    if (qfCallBufs(&call, bufs, NULL, nBufs)) return (size_t)-1;
    /* `advised` and `est` are not written by a call that is refused; a call without a buffer that holds an element takes nothing — off is
     * the default, and no GPU is touched — but is counted */
    if (nTiles && qfCallBegin(&call, stream)) return (size_t)-1;
    for (i = 0; i < nBufs; i++) {
        advised[i] = (unsigned char)(elemSizes && elemSizes[i] ? elemSizes[i] : f->group);
        if (est) est[2u * i] = est[2u * i + 1u] = 0ull;
    }
    if (nTiles == 0) {
        __atomic_fetch_add(&f->adviseStats[0], (unsigned long long)nBufs, __ATOMIC_RELAXED);
        return 0;
    }
    dev = call.dev;
    s = f->restoreSlot;

    rows = (qzstd_hip_ediff_cost_row_t *)qfBufH(&s->pin.advRows, nRows * sizeof(qzstd_hip_ediff_cost_row_t));
    tiles = rows ? (const uint32_t *)qfBufH(&s->pin.advTiles, nTiles * 2u * sizeof(uint32_t)) : NULL;
    if (!tiles || !qfBufD(dev, &s->dev.advRows, nRows * sizeof(qzstd_hip_ediff_cost_row_t)) || !qfBufD(dev, &s->dev.advTiles, nTiles * 2u * sizeof(uint32_t)))
        rc = -1;
    if (rc == 0) {
        for (i = 0, c = 0; i < nBufs; i++) {
            size_t off;
            for (off = 0; off < bufs[i].size; off += f->p.chunkSize, c++) { /* chunks as the compress calls cut frames */
                qzstd_hip_ediff_cost_row_t *r = &rows[c];
                r->src = (uint64_t)(uintptr_t)((const unsigned char *)bufs[i].d_ptr + off);
                r->len = (uint32_t)(bufs[i].size - off < f->p.chunkSize ? bufs[i].size - off : f->p.chunkSize);
                r->elem = advised[i];
                r->tile0 = 0;
                r->reserved = 0;
                total += (unsigned long long)(r->len / r->elem) * r->elem;
            }
        }
        if (qzstd_hip_ediff_cost(dev, s->stream, rows, (uint32_t)nRows, (qzstd_hip_ediff_cost_row_t *)s->dev.advRows.p, (uint32_t *)s->dev.advTiles.p) ||
            qzstd_hip_memcpy_d2h(dev, s->stream, s->pin.advTiles.p, s->dev.advTiles.p, nTiles * 2u * sizeof(uint32_t)))
            rc = -1;
    }
    if (qfCallWait(&call)) rc = -1;
    for (i = 0, c = 0; i < nBufs && rc == 0; i++) {
        unsigned long long P = 0, D = 0;
        size_t off;
        for (off = 0; off < bufs[i].size; off += f->p.chunkSize, c++) {
            size_t n = (size_t)QZSTD_HIP_ESUM_TILES(rows[c].len, rows[c].elem);
            for (; n; n--, t++) {
                P += tiles[2u * t];
                D += tiles[2u * t + 1u];
            }
        }
        if (est) { est[2u * i] = P; est[2u * i + 1u] = D; }
        if (QZSTD_ediffAdvised(P, D)) {
            advised[i] |= (unsigned char)QZSTD_ELEM_DIFF;
            nFlagged++;
        }
    }
    if (rc == 0) {
        __atomic_fetch_add(&f->adviseStats[0], (unsigned long long)nBufs, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->adviseStats[1], (unsigned long long)nFlagged, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->adviseStats[2], total, __ATOMIC_RELAXED);
        __atomic_fetch_add(&f->adviseStats[3], 1ull, __ATOMIC_RELAXED);
    }
    qfCallEnd(&call);
    return rc ? (size_t)-1 : nFlagged;
}

void QZSTD_frontAdviseStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->adviseStats : NULL, stats, 4); }
