/*
 * qzstd_slicecheck.c — QZSTD_frontFingerprintDeviceSlices / QZSTD_frontCheckDeviceSlices / QZSTD_frontVerifyDeviceSlices /
 * QZSTD_frontSliceCheckStats (include/qzstd_frontend_device.h): the fingerprint, check and verify calls for buffers that are not contiguous
 * in device memory, given as the source slices QZSTD_frontCompressDeviceSlices takes.  Included by qzstd_frontend.c behind qzstd_srcslices.c.
 *
 * A call checks its slices and looks their memory up with that call's own helper (qfSrcMapBuild) and hands the contiguous call's body —
 * qfFingerprintDevice, qfVerifyDevice — the map beside a buffer table that holds the sizes.  The bodies do the rest: a frame inside ONE
 * piece is the row it is in a contiguous buffer, so a call (a verify part) without a frame of several pieces queues exactly the contiguous
 * call's launches; one with such a frame is ONE launch of the kernel from pieces over all its rows.  The fold, the harvest, the bounded
 * waits, the event pair and the statistics are the bodies' own.
 */

/* the call's counts, added to the front's when it has succeeded */
static void qfSliceCheckCount(QZSTD_Front *f, const QF_SrcSlices *o)
{
    __atomic_fetch_add(&f->sliceCheckStats[0], (unsigned long long)o->nSlices, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->sliceCheckStats[1], (unsigned long long)o->sm.total, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->sliceCheckStats[2], o->counts[0], __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->sliceCheckStats[3], o->counts[1], __ATOMIC_RELAXED);
}

size_t QZSTD_frontFingerprintDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices, size_t nSlices,
                                          void *stream, unsigned long long *fp, size_t *firstFrame)
{
    QF_SrcSlices o;
    size_t ret;
    if (qfSrcMapBuild(f, bufSizes, nBufs, slices, nSlices, 0, &o)) return (size_t)-1;
    ret = qfFingerprintDevice(f, o.bufs, nBufs, &o.sm, stream, fp, firstFrame, NULL, 0, 0, NULL);
    if (ret != (size_t)-1) qfSliceCheckCount(f, &o);
    qfSrcMapFree(&o);
    return ret;
}

size_t QZSTD_frontCheckDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices, size_t nSlices,
                                    void *stream, const unsigned long long *expected, size_t nFrames, unsigned char *differs)
{
    QF_SrcSlices o;
    size_t ret;
    if (qfSrcMapBuild(f, bufSizes, nBufs, slices, nSlices, 0, &o)) return (size_t)-1;
    ret = qfFingerprintDevice(f, o.bufs, nBufs, &o.sm, stream, NULL, NULL, expected, 1, nFrames, differs);
    if (ret != (size_t)-1) qfSliceCheckCount(f, &o);
    qfSrcMapFree(&o);
    return ret;
}

size_t QZSTD_frontVerifyDeviceSlices(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                     const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices,
                                     size_t nSlices, void *stream, size_t *firstDiff)
{
    QF_SrcSlices o;
    size_t ret;
    if (qfSrcMapBuild(f, bufSizes, nBufs, slices, nSlices, 1, &o)) return (size_t)-1;
    ret = qfVerifyDevice(f, frames, frameStride, frameSizes, nFrames, o.bufs, o.anyBase ? o.bases : NULL, &o.sm, elemSizes, nBufs, stream, firstDiff);
    if (ret != (size_t)-1) qfSliceCheckCount(f, &o);
    qfSrcMapFree(&o);
    return ret;
}

void QZSTD_frontSliceCheckStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->sliceCheckStats : NULL, stats, 4); }
