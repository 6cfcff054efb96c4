/*
 * qzstd_frontend.c — batch front-end for the host entropy stage (include/qzstd_frontend.h).
 *
 * A persistent pool of workers, each with its own ZSTD_CCtx + producer state (the reference's threading model:
 * one CCtx per thread, /root/reference/test/benchmark.c:241, :514-516), fed from one shared chunk cursor.  A worker
 * keeps several claims: the one it is entropy-coding and the next two (QZSTD_FRONT_AHEAD), already announced to the GPUs
 * (QZSTD_hintSource), so match-finding always runs ahead of the thread that will consume it.
 */
#define _GNU_SOURCE /* dladdr */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include "qatseqprod.h"
#include "qzstd_bytegroup.h"
#include "qzstd_bytegroup_internal.h"
#include "qzstd_hip_device.h"
#include "qzstd_planecost.h"
#include "qzstd_hufblock.h"
#include "qzstd_fingerprint.h"
#include "qzstd_elemdiff.h"
#include "qzstd_ediffcost.h"

#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

extern int zstdshim_ok(void) __attribute__((weak)); /* tools/zstdshim, when that is the libzstd in the process; else absent */

typedef char qf_seq_layout_is_qzbg[sizeof(ZSTD_Sequence) == QZBG_ENTRY_WORDS * sizeof(unsigned) ? 1 : -1]; /* qzbgRebuild reads the workers' ZSTD_Sequence arrays */

#define QF_NONE ((size_t)-1)
#define QF_HINT_MAX ((size_t)16 << 20)
#define QF_AHEAD_MAX 3u

typedef struct {
    QZSTD_Front *front;
    pthread_t th;
    ZSTD_CCtx *zc;
    void *state;
    int ok;
    /* device-resident input (QZSTD_frontCompressDevice): the frame's sequences unpacked, its raw bytes when they are needed */
    ZSTD_Sequence *seqs;
    size_t seqsCap;
    unsigned char *raw;
    void *rawStream;
    int rawDev;
    int cksum; /* ZSTD_c_checksumFlag as last set on zc (the parameter is sticky: qfCtxChecksum) */
    /* byte-grouped frames: the frame's block ends, and the caller's bytes of a frame that could not be rebuilt (pinned, as raw) */
    size_t *ends;
    size_t endsCap;
    unsigned char *back;
    ZSTD_DCtx *zd; /* the restore calls' decoder, created by the worker's first restore job */
    /* plane probe: the entries and literals of a frame's blocks that are not raw-predicted, and the frame libzstd builds of them */
    ZSTD_Sequence *subSeqs;
    size_t subSeqsCap;
    unsigned char *subLit, *sub;
    size_t subLitCap, subCap;
} QF_Worker;

typedef struct QF_DevPart_s QF_DevPart;
typedef struct QF_DevSlot_s QF_DevSlot;
typedef struct QF_RestoreSlot_s QF_RestoreSlot;
static void qfDevSlotsFree(QZSTD_Front *f);
static void qfRestoreSlotsFree(QZSTD_Front *f);

struct QZSTD_Front_s {
    QZSTD_FrontParams p;
    size_t stride, segChunks;
    QF_Worker *w;
    pthread_mutex_t mu;
    pthread_cond_t cvWork, cvDone;
    /* the job in progress */
    unsigned long gen; /* bumped per job */
    int quit, running, failed;
    const unsigned char *src;
    size_t srcSize, nChunks;
    unsigned char *dst;
    size_t *sizes;
    size_t nextChunk; /* shared claim cursor (atomic) */
    int uniform;      /* every claim a whole segment: the levels whose match-finding, not the entropy stage, sets the pace (see qfClaim) */
    unsigned ahead;   /* claims a worker keeps announced beyond the one it is entropy-coding: $QZSTD_FRONT_AHEAD, 1..3, default 2 */
    unsigned long served[2];
    /* device-resident input: the part the workers entropy-code (NULL: a QZSTD_frontCompress job) and the device jobs' counters */
    const QF_DevPart *part;
    int devBusy;
    unsigned long long devStats[4];
    QF_DevSlot *devSlot; /* two, kept from call to call (device buffers, pinned arenas, streams) for device devSlotDev */
    int devSlotDev;
    /* content checksums (QZSTD_frontSetChecksum): the setting, and frames hashed by the GPU / by libzstd */
    int checksum;
    unsigned long long cksumStats[2];
    /* byte grouping (QZSTD_frontSetByteGroup): the element size of the device calls (1: off), and grouped frames by how they were built */
    unsigned group;
    unsigned long long groupStats[3];
    /* delta frames (the ...Delta calls): frames with a base by how they were built, and frames restored onto a base */
    unsigned long long deltaStats[4];
    unsigned long long ediffStats[4]; /* QZSTD_frontElemDiffStats */
    /* delta skip (QZSTD_frontSetDeltaSkip): the setting, and frames compared / found equal, bytes compared, zero frames a restore recognised */
    int deltaSkip;
    unsigned long long skipStats[4];
    /* plane probe (QZSTD_frontSetPlaneProbe): the setting, and blocks probed / written raw here, frames assembled here / fallen back */
    int planeProbe;
    unsigned long long probeStats[4];
    /* plane code (QZSTD_frontSetPlaneCode): the setting, and rows the kernel coded / blocks taken / frames assembled without libzstd / frames
     * with a taken block that fell back */
    int planeCode;
    unsigned long long codeStats[4];
    /* the restore calls (qzstd_restore.c): the part the workers decode (NULL: a compress job), the counters, and two slots kept from call to
     * call (pinned buffer, device stage, stream) for device restoreSlotDev */
    const struct QF_RestorePart_s *restore;
    unsigned long long restoreStats[4];
    unsigned long long sliceStats[4]; /* QZSTD_frontRestoreDeviceSlices: slices, bytes written, frames decoded, rows launched */
    QF_RestoreSlot *restoreSlot;
    int restoreSlotDev;
    unsigned long long verifyStats[4]; /* QZSTD_frontVerifyDeviceBatch: frames compared, of them differing, bytes compared, launches */
    unsigned long long fpStats[4];     /* the fingerprint calls: frames fingerprinted, bytes read on the device, launches, frames a check found differing */
    unsigned long long adviseStats[4]; /* QZSTD_frontAdviseDeviceBatch: buffers advised on, buffers flagged, bytes read on the device, launches */
    unsigned long long srcSliceStats[4]; /* QZSTD_frontCompressDeviceSlices: slices, their bytes, frames of more than one piece, qzstd_hip_group_pieces launches */
    unsigned long long sliceCheckStats[4]; /* the fingerprint, check and verify calls with source slices: slices, their bytes, frames of more than one piece, launches of the two kernels from pieces */
};

/* A claim: chunks [c0, c1) of the job.  Where the entropy stage sets the pace (levels 1-4: with a libzstd that entropy-codes 1.6 GB/s per core
 * a 512 MiB job is over in 25 ms and its first and last milliseconds count) claims are not all the same size:
 *   - a worker's first claims are small (an eighth, then a quarter, then half of a segment): the GPU's first results are back after
 *     the time one block takes, not after a whole segment was staged and queued, and the pipeline below fills while they are consumed;
 *   - towards the end of the job a claim is at most a (2 x threads)-th of what is left, so the workers finish together;
 *   - never less than QF_MIN_CHUNKS chunks (a launch of fewer than four blocks is not worth its queueing).
 * Where the match-finder sets the pace (the chain levels, 5-12: a 128 KiB block takes a workgroup 4-5 ms at level 6) every claim is a whole
 * segment and three are kept announced: what counts there is how many blocks are on the GPU at any time, and a launch of four blocks
 * takes as long as one of thirty-two (level 6, 18 threads, 4 MiB: 5.8 GB/s with the varying claims, 8.3 with uniform ones; the kernel
 * alone, input resident: 10.5). */
#define QF_MIN_CHUNKS 4u
typedef struct { size_t c0, c1; } QF_Seg;

static int qfClaim(QZSTD_Front *f, unsigned nth, QF_Seg *out)
{
    size_t want = f->segChunks, have, left;
    have = __atomic_load_n(&f->nextChunk, __ATOMIC_RELAXED);
    if (have >= f->nChunks) return 0;
    if (!f->uniform) {
        if (nth < 3 && (f->segChunks >> (3 - nth)) >= QF_MIN_CHUNKS) want = f->segChunks >> (3 - nth);
        left = (f->nChunks - have) / (2u * (size_t)f->p.nThreads);
        if (want > left) want = left;
    }
    if (want < QF_MIN_CHUNKS) want = QF_MIN_CHUNKS;
    if (want > f->segChunks) want = f->segChunks;
    have = __atomic_fetch_add(&f->nextChunk, want, __ATOMIC_RELAXED);
    if (have >= f->nChunks) return 0;
    out->c0 = have;
    out->c1 = have + want < f->nChunks ? have + want : f->nChunks;
    return 1;
}

static void qfAnnounce(QZSTD_Front *f, QF_Worker *w, const QF_Seg *sg)
{
    const size_t off = sg->c0 * f->p.chunkSize;
    size_t len = (sg->c1 - sg->c0) * f->p.chunkSize, grid = f->p.chunkSize;
    if (!f->p.useProducer) return;
    if (len > f->srcSize - off) len = f->srcSize - off;
    /* the block grid of the announcement: the chunk when a chunk is one block; 128 KiB blocks inside bigger frames */
    if (grid > 131072) grid = 131072;
    if ((grid & 15) || len > QF_HINT_MAX) return; /* not announceable: the callbacks take the per-block path */
    /* every chunk is its own frame whose blocks start at the chunk's start: the announcement's grid (anchored at the
     * claim's start) only names those blocks if the chunks are whole grid cells — otherwise every callback would miss
     * and the GPU would match-find everything twice (round-2 ADVICE) */
    if (f->p.chunkSize > grid && f->p.chunkSize % grid != 0) return;
    /* (stable: the source is the const argument of the QZSTD_frontCompress call in progress) */
    (void)QZSTD_hintSourceEx(w->state, f->src + off, len, grid, f->p.level, QZSTD_HINT_STABLE);
}

static int qfDeviceFrame(QZSTD_Front *f, QF_Worker *w, size_t c);
static int qfRestoreSegment(QZSTD_Front *f, QF_Worker *w, const QF_Seg *sg);

/* ZSTD_c_checksumFlag on the worker's context.  The parameter outlives ZSTD_reset_session_only, so every path that builds a frame names
 * the value it needs and no frame inherits the one before it; the context is only touched when the value changes (never, with the
 * setting off).  Parameters cannot be set mid-frame, where a failed call may have left the context: reset first. */
static int qfCtxChecksum(QF_Worker *w, int on)
{
    if (w->cksum == on) return 0;
    (void)ZSTD_CCtx_reset(w->zc, ZSTD_reset_session_only);
    if (ZSTD_isError(ZSTD_CCtx_setParameter(w->zc, ZSTD_c_checksumFlag, on))) return -1;
    w->cksum = on;
    return 0;
}

static int qfCompressSegment(QZSTD_Front *f, QF_Worker *w, const QF_Seg *sg)
{
    size_t c;
    if (f->restore) return qfRestoreSegment(f, w, sg);
    if (f->part) {
        for (c = sg->c0; c < sg->c1; c++)
            if (qfDeviceFrame(f, w, c) != 0) return -1;
        return 0;
    }
    if (qfCtxChecksum(w, f->checksum)) return -1;
    for (c = sg->c0; c < sg->c1; c++) {
        const size_t off = c * f->p.chunkSize;
        const size_t n = f->srcSize - off < f->p.chunkSize ? f->srcSize - off : f->p.chunkSize;
        const size_t r = ZSTD_compress2(w->zc, f->dst + c * f->stride, f->stride, f->src + off, n);
        if (ZSTD_isError(r)) return -1;
        f->sizes[c] = r;
    }
    if (f->checksum) __atomic_fetch_add(&f->cksumStats[1], (unsigned long long)(sg->c1 - sg->c0), __ATOMIC_RELAXED);
    return 0;
}

static void *qfWorker(void *arg)
{
    QF_Worker *w = (QF_Worker *)arg;
    QZSTD_Front *f = w->front;
    unsigned long seen = 0;
    for (;;) {
        QF_Seg q[QF_AHEAD_MAX + 1]; /* claimed and announced, oldest first: q[0] is the one being entropy-coded */
        unsigned n = 0, claims = 0;
        int bad = 0, more = 1;
        pthread_mutex_lock(&f->mu);
        while (!f->quit && f->gen == seen) pthread_cond_wait(&f->cvWork, &f->mu);
        if (f->quit) { pthread_mutex_unlock(&f->mu); break; }
        seen = f->gen;
        pthread_mutex_unlock(&f->mu);

        for (;;) {
            /* keep `ahead` claims announced beyond the current one: the GPUs match-find them while this thread entropy-codes q[0]
             * (a state holds four announcements: three ahead at most) */
            while (more && n < f->ahead + 1u) {
                more = qfClaim(f, claims, &q[n]);
                if (!more) break;
                claims++;
                if (!bad && !f->part && !f->restore) qfAnnounce(f, w, &q[n]);
                n++;
            }
            if (n == 0) break;
            if (!bad && qfCompressSegment(f, w, &q[0]) != 0) bad = 1;
            memmove(&q[0], &q[1], (n - 1) * sizeof(q[0]));
            n--;
        }
        /* the job is over for this worker: whatever it announced ends here.  An announcement otherwise lives until the callback of its
         * last block — which never comes for a last block below 7 bytes (libzstd does not ask the producer), after a failed part, or
         * after `bad` — and a STABLE one would serve the NEXT job by address if the caller used the same buffer again (round-4 ADVICE) */
        if (f->p.useProducer && w->state) QZSTD_dropHints(w->state);
        pthread_mutex_lock(&f->mu);
        if (bad) f->failed = 1;
        if (--f->running == 0) pthread_cond_signal(&f->cvDone);
        pthread_mutex_unlock(&f->mu);
    }
    return NULL;
}

QZSTD_Front *QZSTD_createFront(const QZSTD_FrontParams *p)
{
    QZSTD_Front *f;
    int t, made = 0;
    size_t seg;
    if (!p || p->nThreads < 1 || p->nThreads > 1024 || p->level < 1 || p->level > 12 || p->chunkSize == 0) return NULL;
    /* the libzstd this was linked against must be one that works: when it is tools/zstdshim (tests and bench only) and its look-up of
     * libarrow.so's copy failed, every ZSTD_* call would abort() the process — refuse instead; and the producer API needs >= 1.5.4 */
    if (zstdshim_ok && zstdshim_ok() != 1) return NULL;
    if (ZSTD_versionNumber() < 10504u) return NULL;
    f = (QZSTD_Front *)calloc(1, sizeof(*f));
    if (!f) return NULL;
    f->p = *p;
    f->group = 1u;
    /* measured on MI355X + 16 cores: 2 MiB where the entropy stage sets the pace (levels 1-4), 4 MiB claims of one size where the match-finder does */
    seg = p->segmentBytes ? p->segmentBytes : ((size_t)(p->level >= 5 ? 4 : 2) << 20);
    /* ... and at the chain levels at most 64 chunks per claim (round 5): a claim is one launch, its blocks one workgroup each — level 12 on 32 KiB
     * chunks: 2 MiB claims 8.7 GB/s, 4 MiB 7.7, 8 MiB 6.3 (the kernel alone: 9.8); level 6 on 128 KiB chunks keeps its 4 MiB (32 blocks): 10.3-11.0 */
    if (!p->segmentBytes && p->level >= 5 && seg / p->chunkSize > 64u) seg = 64u * p->chunkSize;
    if (seg > QF_HINT_MAX) seg = QF_HINT_MAX;
    f->segChunks = seg / p->chunkSize ? seg / p->chunkSize : 1;
    f->stride = ZSTD_compressBound(p->chunkSize);
    {
        const char *a = getenv("QZSTD_FRONT_AHEAD");
        const int v = a && *a ? atoi(a) : 2;
        f->ahead = v < 1 ? 1u : (v > (int)QF_AHEAD_MAX ? QF_AHEAD_MAX : (unsigned)v);
        a = getenv("QZSTD_FRONT_UNIFORM");
        f->uniform = a && *a ? atoi(a) != 0 : p->level >= 5;
        if (f->uniform && !(getenv("QZSTD_FRONT_AHEAD") && *getenv("QZSTD_FRONT_AHEAD"))) f->ahead = QF_AHEAD_MAX;
    }
    f->w = (QF_Worker *)calloc((size_t)p->nThreads, sizeof(QF_Worker));
    pthread_mutex_init(&f->mu, NULL);
    pthread_cond_init(&f->cvWork, NULL);
    pthread_cond_init(&f->cvDone, NULL);
    if (!f->w) { QZSTD_freeFront(f); return NULL; }
    if (p->useProducer) (void)QZSTD_startQatDevice(); /* return value ignored, as the reference's callers do: fallback below */
    for (t = 0; t < p->nThreads; t++) {
        QF_Worker *w = &f->w[t];
        const int e = p->extRepcodes == 1 ? ZSTD_ps_enable : (p->extRepcodes == 2 ? ZSTD_ps_disable : ZSTD_ps_auto);
        w->front = f;
        w->zc = ZSTD_createCCtx();
        if (!w->zc) break;
        if (p->useProducer) {
            w->state = QZSTD_createSeqProdState();
            if (!w->state) break;
            ZSTD_registerSequenceProducer(w->zc, w->state, qatSequenceProducer);
            /* any producer error (device down, time-out, dense block) falls back to libzstd's own match-finder */
            (void)ZSTD_CCtx_setParameter(w->zc, ZSTD_c_enableSeqProducerFallback, 1);
        }
        if (ZSTD_isError(ZSTD_CCtx_setParameter(w->zc, ZSTD_c_compressionLevel, p->level)) ||
            ZSTD_isError(ZSTD_CCtx_setParameter(w->zc, ZSTD_c_searchForExternalRepcodes, e)))
            break;
        if (pthread_create(&w->th, NULL, qfWorker, w) != 0) break;
        w->ok = 1;
        made++;
    }
    if (made != p->nThreads) { QZSTD_freeFront(f); return NULL; }
    return f;
}

size_t QZSTD_frontFrameStride(const QZSTD_Front *f) { return f ? f->stride : 0; }

/* hands the workers chunks [0, nChunks) of a job (called with f->mu held) and waits for them */
static int qfRunJobLocked(QZSTD_Front *f, size_t nChunks)
{
    f->nChunks = nChunks;
    f->nextChunk = 0;
    f->failed = 0;
    f->running = f->p.nThreads;
    f->gen++;
    pthread_cond_broadcast(&f->cvWork);
    while (f->running) pthread_cond_wait(&f->cvDone, &f->mu);
    return f->failed;
}

size_t QZSTD_frontCompress(QZSTD_Front *f, const void *src, size_t srcSize, void *dst, size_t dstCapacity, size_t *frameSizes)
{
    size_t nChunks;
    int failed;
    if (!f || (!src && srcSize) || !dst || !frameSizes) return (size_t)-1;
    if (f->group > 1u) return (size_t)-1; /* the host path cannot cut a block per plane: no second layout from one front */
    nChunks = (srcSize + f->p.chunkSize - 1) / f->p.chunkSize;
    if (nChunks == 0) return 0;
    if (dstCapacity / f->stride < nChunks) return (size_t)-1;
    pthread_mutex_lock(&f->mu);
    f->src = (const unsigned char *)src;
    f->srcSize = srcSize;
    f->dst = (unsigned char *)dst;
    f->sizes = frameSizes;
    failed = qfRunJobLocked(f, nChunks);
    pthread_mutex_unlock(&f->mu);
    return failed ? (size_t)-1 : nChunks;
}

size_t QZSTD_frontCompact(const QZSTD_Front *f, void *dst, const size_t *frameSizes, size_t nFrames)
{
    unsigned char *d = (unsigned char *)dst;
    size_t c, pos = 0;
    if (!f || !dst || !frameSizes) return 0;
    for (c = 0; c < nFrames; c++) {
        if (pos != c * f->stride) memmove(d + pos, d + c * f->stride, frameSizes[c]);
        pos += frameSizes[c];
    }
    return pos;
}

void QZSTD_frontStats(QZSTD_Front *f, unsigned long stats[2])
{
    int t;
    if (!stats) return;
    stats[0] = stats[1] = 0;
    if (!f || !f->p.useProducer) return;
    for (t = 0; t < f->p.nThreads; t++) {
        unsigned long s[4] = { 0, 0, 0, 0 };
        if (f->w[t].state) QZSTD_hintStats(f->w[t].state, s);
        stats[0] += s[0];
        stats[1] += s[1];
    }
}

void QZSTD_frontFailStats(QZSTD_Front *f, unsigned long stats[8])
{
    int t, k;
    if (!stats) return;
    for (k = 0; k < 8; k++) stats[k] = 0;
    if (!f || !f->p.useProducer) return;
    for (t = 0; t < f->p.nThreads; t++) {
        unsigned long s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (f->w[t].state) QZSTD_failStats(f->w[t].state, s);
        for (k = 0; k < 8; k++) stats[k] += s[k];
    }
}

void QZSTD_freeFront(QZSTD_Front *f)
{
    int t;
    if (!f) return;
    pthread_mutex_lock(&f->mu);
    f->quit = 1;
    pthread_cond_broadcast(&f->cvWork);
    pthread_mutex_unlock(&f->mu);
    for (t = 0; f->w && t < f->p.nThreads; t++) {
        QF_Worker *w = &f->w[t];
        if (w->ok) pthread_join(w->th, NULL);
        if (w->zc) ZSTD_freeCCtx(w->zc);
        if (w->zd) ZSTD_freeDCtx(w->zd);
        if (w->state) QZSTD_freeSeqProdState(w->state);
        free(w->seqs);
        free(w->ends);
        free(w->subSeqs);
        free(w->subLit);
        free(w->sub);
        if (w->back) qzstd_hip_host_free(w->back);
        if (w->raw) qzstd_hip_host_free(w->raw);
        if (w->rawStream) qzstd_hip_stream_destroy(w->rawDev, w->rawStream);
    }
    qfDevSlotsFree(f);
    qfRestoreSlotsFree(f);
    free(f->w);
    pthread_mutex_destroy(&f->mu);
    pthread_cond_destroy(&f->cvWork);
    pthread_cond_destroy(&f->cvDone);
    free(f);
}

/* ---------------------------------------------------------------- device-resident input -- */
/*
 * QZSTD_frontCompressDevice / QZSTD_frontCompressDeviceBatch: every buffer is cut into frames of chunkSize (the per-frame table, QF_DevFrame) and
 * the frames, across buffer boundaries, into PARTS of whole frames (at most QF_PART_BYTES of input).  A part that is one buffer's 16-aligned
 * chunks is read where it lies; any other is gathered into the slot's stage first (qzstd_hip_gather).  Per part, on one of two device slots:
 * the match-finder (qzstd_hip_find_sequences), the compaction (qzstd_hip_compact: packed entries + literal bytes in one dense arena), the
 * arena's headers and then the arena itself D2H into pinned memory.  The workers entropy-code part k straight from its arena
 * (ZSTD_compressSequencesAndLiterals) while the GPU works on parts k + 1 and k + 2.  The calling thread does the GPU side.
 *
 * What the call does before and behind that — the look-ups, devBusy, the slots, the event pair, the closing waits — is the scaffold's
 * (qfCallBegin .. qfCallEnd below), which every device call of the front-end shares; the slots' memory is QF_Buf's.
 *
 * The new entry points of the device layer are weak references: a device layer without them (an older library, the CPU suite's mock)
 * makes QZSTD_frontCompressDevice fail and leaves the rest of the front-end as it was.
 *
 * Content checksums (QZSTD_frontSetChecksum): the part's frames are hashed where the match-finder reads them (qzstd_hip_xxh64, queued behind
 * the compaction on the slot's stream), 8 bytes per frame come back with the arena's headers, and qfDeviceFrame sets the header's flag and
 * appends the low 32 bits to a frame ZSTD_compressSequencesAndLiterals built (that function refuses ZSTD_c_checksumFlag: it never sees
 * the content).  The raw-bytes paths have the content and let libzstd hash it.
 *
 * Byte grouping (QZSTD_frontSetByteGroup, QZSTD_frontCompressDeviceBatchTyped): a frame with an element size k > 1 is staged by
 * qzstd_hip_group instead — its bytes arrive in the layout of include/qzstd_bytegroup.h — and its blocks are those of QZSTD_byteGroupBlocks:
 * a block per plane, so that the skewed exponent plane and the noisy mantissa plane of float data get entropy tables of their own.
 * Everything behind the staging (match-finder, compaction, hash, arena) sees an ordinary part whose frames have unusual block lengths.
 * A frame that needs its content on the host (a raw block: the common case here) rebuilds it from its own entries and literals.
 *
 * Delta frames (QZSTD_frontCompressDeviceBatchDelta): a part with a frame whose buffer has a base is staged by ONE qzstd_hip_group_xor launch
 * for all its rows (base 0 for the rows without one, elem = 1 rows included) and never read in place; the frame's content is the grouped
 * layout of chunk XOR base chunk, and everything behind the staging — the hash too, which reads the stage — is untouched.  A delta frame that
 * needs its content on the host is treated like a grouped one (qzbgRebuild, also for k = 1); only for a block the matcher failed do the
 * caller's bytes AND the base's come back, to be XORed and grouped here.
 *
 * Delta skip (QZSTD_frontSetDeltaSkip): before the parts are planned, ONE qzstd_hip_diff launch finds the frames of based buffers whose chunk
 * equals its base chunk (qfDiffPass); they get the canonical zero frame, written here, and are left out of the per-frame table — a table
 * entry carries its frame's index in the call — so nothing above ever sees them.  With the setting off, or without a base, nothing changes.
 *
 * Plane probe (QZSTD_frontSetPlaneProbe): a part with a grouped or based frame gets ONE qzstd_hip_plane_cost launch behind its staging — a row per
 * block descriptor over the stage, one word per block back with the compaction headers: the block's order-0 cost (include/qzstd_planecost.h).
 * A frame with a block that QZSTD_planeIsRaw predicts raw is assembled by qfAssembleFrame — the library writes the Raw_Blocks, libzstd codes
 * the remaining blocks once — and never entropy-coded twice.  With the setting off nothing is launched and every frame is what it was.
 *
 * Source slices (QZSTD_frontCompressDeviceSlices, qzstd_srcslices.c): the buffers' bytes lie in pieces anywhere in device memory.  The
 * per-frame table says where every frame lies (src, base): a frame inside one piece is a frame like any other, a frame across several has
 * no address, makes its part one that qzstd_hip_group_pieces stages, and is read piece by piece wherever its bytes are needed on the host.
 */
extern int qzstd_hip_pointer_device(const void *p) __attribute__((weak));
extern int qzstd_hip_pointer_extent(const void *p, const void **lo, size_t *size) __attribute__((weak));
extern void *qzstd_hip_event_create(int device) __attribute__((weak));
extern void qzstd_hip_event_destroy(int device, void *event) __attribute__((weak));
extern int qzstd_hip_event_record(int device, void *event, void *stream) __attribute__((weak));
extern int qzstd_hip_stream_wait_event(int device, void *stream, void *event) __attribute__((weak));
extern int qzstd_hip_memcpy2d_d2d(int device, void *stream, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                                  size_t height) __attribute__((weak));
extern size_t qzstd_hip_compact_workspace_bytes(uint32_t nBlocks) __attribute__((weak));
extern int qzstd_hip_compact(int device, void *stream, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                             const void *d_seqs, const uint32_t *d_nseq, void *d_arena, size_t arenaBytes, void *d_work,
                             size_t workBytes) __attribute__((weak));
extern int qzstd_hip_gather(int device, void *stream, const qzstd_hip_gather_row_t *rows, uint32_t nRows, qzstd_hip_gather_row_t *d_rows,
                            void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_group(int device, void *stream, const qzstd_hip_group_row_t *rows, uint32_t nRows, qzstd_hip_group_row_t *d_rows,
                           void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_group_ediff(int device, void *stream, const qzstd_hip_group_ediff_row_t *rows, uint32_t nRows,
                                 qzstd_hip_group_ediff_row_t *d_rows, void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_group_xor(int device, void *stream, const qzstd_hip_group_xor_row_t *rows, uint32_t nRows, qzstd_hip_group_xor_row_t *d_rows,
                               void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_group_pieces(int device, void *stream, const qzstd_hip_group_pieces_row_t *rows, uint32_t nRows,
                                  qzstd_hip_group_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                  qzstd_hip_group_piece_t *d_pieces, void *d_stage, size_t stageBytes) __attribute__((weak));
extern int qzstd_hip_xxh64(int device, void *stream, const void *d_base, const qzstd_hip_hash_row_t *rows, uint32_t nRows,
                           qzstd_hip_hash_row_t *d_rows, uint64_t *d_out) __attribute__((weak));
extern int qzstd_hip_diff(int device, void *stream, qzstd_hip_diff_row_t *rows, uint32_t nRows, qzstd_hip_diff_row_t *d_rows,
                          uint32_t *d_flags) __attribute__((weak));
extern int qzstd_hip_plane_cost(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                                qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost) __attribute__((weak));
extern size_t qzstd_hip_huf_code_bytes(const qzstd_hip_plane_row_t *rows, uint32_t nRows) __attribute__((weak));
extern int qzstd_hip_huf_code(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                              qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost, uint32_t *d_size, uint32_t *d_off, void *d_dense, size_t denseBytes,
                              void *d_scratch, size_t scratchBytes) __attribute__((weak));

#define QF_PART_BYTES ((size_t)64 << 20)
#define QF_DEV_WAIT_MS 60000u
#define QF_LIT_SLACK 64u /* bytes past the arena's last literal: ZSTD_compressSequencesAndLiterals reads up to 8 past a frame's literals */
#ifndef ZSTD_c_blockDelimiters
#define ZSTD_c_blockDelimiters ((ZSTD_cParameter)1008) /* ZSTD_c_experimentalParam11 */
#endif

typedef size_t (*QF_SeqLitFn)(ZSTD_CCtx *, void *, size_t, const ZSTD_Sequence *, size_t, const void *, size_t, size_t, size_t);
typedef size_t (*QF_SeqFn)(ZSTD_CCtx *, void *, size_t, const ZSTD_Sequence *, size_t, const void *, size_t);
static QF_SeqLitFn qfSeqLit;
static QF_SeqFn qfSeq;
static pthread_once_t qfSeqOnce = PTHREAD_ONCE_INIT;

/* ZSTD_compressSequencesAndLiterals (libzstd >= 1.5.7) and ZSTD_compressSequences, from THE libzstd this library's ZSTD_* calls bind
 * to (with RTLD_DEEPBIND that is not the first one in the process): the object that holds ZSTD_compress2 as bound here */
static void qfResolveSeqApi(void)
{
    Dl_info di;
    void *h;
    if (!dladdr((void *)(uintptr_t)&ZSTD_compress2, &di) || !di.dli_fname) return;
    h = dlopen(di.dli_fname, RTLD_NOW | RTLD_NOLOAD);
    if (!h) return;
    if (!getenv("QZSTD_FRONT_NO_SEQLIT")) qfSeqLit = (QF_SeqLitFn)(uintptr_t)dlsym(h, "ZSTD_compressSequencesAndLiterals");
    qfSeq = (QF_SeqFn)(uintptr_t)dlsym(h, "ZSTD_compressSequences");
    dlclose(h); /* (RTLD_NOLOAD: the library stays, it was loaded before) */
}

/* Grow-only memory of one kind — device memory of the slot's device (qfBufD) or pinned host memory (qfBufH) — kept from call to call.
 * Growing frees and allocates anew: the contents are NOT kept (the one buffer whose contents must move along, the pinned arena, says so
 * where it grows: qfFetchPart).  A need of 0 bytes allocates 16; after a failure the buffer is empty (NULL, capacity 0).  -> the memory,
 * or NULL */
typedef struct { void *p; size_t cap; } QF_Buf;
#define QF_NBUFS(group) (sizeof(group) / sizeof(QF_Buf))

static void *qfBufD(int dev, QF_Buf *b, size_t need)
{
    if (b->cap >= need && b->p) return b->p;
    if (b->p) qzstd_hip_free(dev, b->p);
    b->p = qzstd_hip_malloc(dev, need ? need : 16);
    b->cap = b->p ? need : 0;
    return b->p;
}

static void *qfBufH(QF_Buf *b, size_t need)
{
    if (b->cap >= need && b->p) return b->p;
    if (b->p) qzstd_hip_host_free(b->p);
    b->p = qzstd_hip_host_alloc(need ? need : 16);
    b->cap = b->p ? need : 0;
    return b->p;
}

/* a slot's `dev` or `pin` group: n buffers that follow each other */
static void qfBufsFree(int dev, int pinned, void *group, size_t n)
{
    QF_Buf *b = (QF_Buf *)group;
    for (; n; n--, b++) {
        if (b->p && pinned) qzstd_hip_host_free(b->p);
        else if (b->p) qzstd_hip_free(dev, b->p);
        b->p = NULL;
        b->cap = 0;
    }
}

/* One device slot of the compress calls: a part's buffers.  `dev` (device memory) and `pin` (pinned host memory) hold QF_Buf members and
 * NOTHING ELSE, so that qfDevSlotsFree walks them as arrays: a new buffer is one more member, and it cannot be forgotten there. */
struct QF_DevSlot_s {
    void *stream;
    struct {
        QF_Buf stage;      /* the part copied to 16-aligned frames, when the caller's buffers cannot be read in place */
        QF_Buf rows, groupRows, xorRows, ediffRows, pieceRows, pieces; /* the device copies of the staging launches' rows (pin, below) */
        QF_Buf hashRows, hash;          /* checksums: the rows' device copy, the hashes */
        QF_Buf diffRows, diffFlags;     /* delta skip */
        QF_Buf planeRows, planeCost;    /* plane probe */
        QF_Buf hufWords, hufDense, hufScratch; /* plane code: per block a size word and a dense offset (nb + (nb + 1) words), the dense area of
                                                * code lengths, jump tables and streams, the coder's scratch */
        QF_Buf desc, seqs, count, work, cwork, arena;
    } dev;
    struct {
        QF_Buf desc;       /* qzstd_hip_block_t per block */
        QF_Buf rows;       /* qzstd_hip_gather_row_t: the gather's rows, one per frame */
        QF_Buf groupRows;  /* qzstd_hip_group_row_t: a part with byte-grouped frames */
        QF_Buf xorRows;    /* qzstd_hip_group_xor_row_t: a part with delta frames */
        QF_Buf ediffRows;  /* qzstd_hip_group_ediff_row_t: a part's differenced frames only */
        QF_Buf pieceRows, pieces; /* qzstd_hip_group_pieces_row_t and their piece table: a part with a frame of several pieces */
        QF_Buf hashRows, hash;    /* qzstd_hip_hash_row_t per frame, uint64_t per frame */
        QF_Buf diffRows, diffFlags; /* qzstd_hip_diff_row_t per compared piece, uint32_t per row */
        QF_Buf planeRows, planeCost; /* qzstd_hip_plane_row_t per block, uint32_t per block */
        QF_Buf hufWords, hufDense;   /* uint32_t, bytes */
        QF_Buf arena;      /* the compaction's headers, packed entries and literals */
    } pin;
    size_t *ends; size_t endsCap; /* the block ends of the frame whose descriptors are being written */
    int hashed; /* the part queued on this slot has its frames' hashes in dev.hash; the part fetched from it has them in pin.hash */
    int probed; /* as `hashed`: the queued part's costs are in dev.planeCost; the fetched part's in pin.planeCost */
    int coded;  /* as `probed`: the queued part went through qzstd_hip_huf_code; the fetched part's words and dense area are in pin.hufWords / pin.hufDense */
    size_t *blkSeq, *blkLit; size_t blkCap;   /* per block: first entry, first literal byte (host prefix sums of the headers) */
    const unsigned char *hLit; size_t litTotal; /* the arena's literal bytes, in pin.arena */
};
#define QF_HDR(s) ((const qzstd_hip_compact_hdr_t *)(s)->pin.arena.p)

/* One slot of the restore side (qzstd_restore.c and the calls that use its slots: verify, fingerprint, advise); `dev` and `pin` as above,
 * walked by qfRestoreSlotsFree. */
struct QF_RestoreSlot_s {
    void *stream;
    struct {
        QF_Buf stage;                 /* the device copy of the part's decoded frames */
        QF_Buf rows, xorRows, sumRows, sumScratch, winRows; /* the restore calls' rows, and qzstd_hip_esum's scratch */
        QF_Buf cmpRows, tiles;        /* verify: rows, tile words */
        QF_Buf fpRows, fpTiles;       /* fingerprint (slot 0 only): rows, tile digests */
        QF_Buf advRows, advTiles;     /* adviser (slot 0 only): rows, two cost words per tile */
        QF_Buf fpPieceRows, cmpPieceRows, chkPieces; /* the calls with source slices: the rows of the kernels from pieces, their piece table */
    } dev;
    struct {
        QF_Buf stage;                 /* the part's decoded frames, every frame at a 16-aligned offset */
        QF_Buf rows;                  /* qzstd_hip_ungroup_row_t per frame */
        QF_Buf xorRows;               /* qzstd_hip_ungroup_xor_row_t: a part with a base among its frames */
        QF_Buf sumRows;               /* qzstd_hip_esum_row_t: a part's differenced frames only */
        QF_Buf winRows;               /* qzstd_hip_ungroup_win_row_t per piece (slice x frame) */
        QF_Buf cmpRows, tiles;        /* qzstd_hip_ungroup_cmp_row_t per frame, uint32_t per tile */
        QF_Buf fpRows, fpTiles;       /* qzstd_hip_fp_row_t per frame, uint64_t per tile */
        QF_Buf advRows, advTiles;     /* qzstd_hip_ediff_cost_row_t per chunk, 2 x uint32_t per tile */
        QF_Buf fpPieceRows, cmpPieceRows, chkPieces; /* qzstd_hip_fp_pieces_row_t, qzstd_hip_ungroup_cmp_pieces_row_t, qzstd_hip_group_piece_t */
    } pin;
    size_t pending; /* verify: the part (+ 1) whose tile words are on their way; 0: none */
};

/* the source slices of a QZSTD_frontCompressDeviceSlices call (qzstd_srcslices.c): the non-empty ones, buffer after buffer, ascending and
 * without gaps inside a buffer; NULL in the job of every other call */
typedef struct {
    size_t off, size;               /* bytes [off, off + size) of the buffer */
    const unsigned char *src, *base; /* where they lie; base NULL: the buffer has none */
} QF_SrcPiece;
typedef struct {
    const QF_SrcPiece *pieces;
    const size_t *first; /* nBufs + 1 entries: buffer i owns pieces [first[i], first[i + 1]) */
    size_t total;        /* bytes of all buffers */
    int dev;             /* the device all of them lie on (-1: there are none) */
    int multi;           /* a frame of the call is made of more than one piece */
    unsigned long long *counts; /* the call's own: [0] frames staged (fingerprinted, compared) from more than one piece, [1] launches of the kernel from pieces */
} QF_SrcMap;

/* one frame of a device job (the per-frame table, built once per call): where its bytes lie and which blocks of its part are its own */
typedef struct {
    size_t off, len; /* offset in its buffer, length (chunkSize, or what is left of the buffer) */
    const unsigned char *src, *base; /* the frame's first byte and its base chunk's (NULL: no base); both NULL for a frame of several pieces */
    size_t p0;       /* a call with source slices: the first piece of the map that holds bytes of the frame, */
    uint32_t np;     /* and how many do (1: the frame lies at src as in every other call); 0 in every other call */
    uint32_t based;  /* the frame's buffer has a base: its content is chunk ^ base chunk */
    size_t b0;       /* first block in its part */
    size_t idx;      /* its index in the call: dst + idx * stride, frameSizes[idx] (the table leaves out the frames a delta skip found equal) */
    uint32_t buf;    /* owning buffer */
    uint32_t nb;     /* blocks: QZSTD_byteGroupBlocks(len, k) — ceil(len / 128 KiB) for k = 1 */
    uint32_t k;      /* element size of the byte-grouped layout; 1: the bytes as they are */
    uint32_t diff;   /* QZSTD_ELEM_DIFF: the content is the grouped layout of QZSTD_elemDiff(chunk, k) */
} QF_DevFrame;

/* a part: frames [f0, f1) of the job, matched in one launch */
typedef struct {
    size_t f0, f1, nb, bytes;
    int run; /* the frames are consecutive chunks of ONE buffer: readable in place when aligned, stageable by 2D copies */
    int grouped; /* a frame with k > 1 among them: staged by qzstd_hip_group, never read in place */
    int delta;   /* a frame of a buffer with a base among them: staged by qzstd_hip_group_xor (all its rows), never read in place */
    int diff;    /* a differenced frame among them: those are staged by qzstd_hip_group_ediff, the others by the part's own launch; never read in place */
    int pieces;  /* a frame of several pieces among them: staged by qzstd_hip_group_pieces (all its rows), never read in place */
} QF_DevRange;

struct QF_DevPart_s {
    const QF_SrcMap *sm;         /* the call's source slices, or NULL (the raw-bytes path reads a frame of several pieces piece by piece) */
    const QF_DevFrame *frames;   /* the job's table (the raw-bytes path reads a frame from where its entry says) */
    size_t f0, f1;               /* frames of the job */
    size_t nb;                   /* blocks */
    const QF_DevSlot *slot;
    int dev;
    int hashed; /* checksums on: frame c's content hash is word c - f0 of slot->pin.hash */
    int probed; /* plane probe: block b's order-0 cost is word b of slot->pin.planeCost */
    int coded;  /* plane code: block b's size word is word b of slot->pin.hufWords, its bytes lie in slot->pin.hufDense at word nb + b */
    int failSub; /* test switch ($QZSTD_FRONT_PROBE_FAIL_SUB): the assembled frames' libzstd call counts as failed */
};

/* n counters of the front as a caller reads them (all 0 for no front) */
static void qfStats(const unsigned long long *from, unsigned long long *stats, int n)
{
    int k;
    if (!stats) return;
    for (k = 0; k < n; k++) stats[k] = from ? __atomic_load_n(&from[k], __ATOMIC_RELAXED) : 0ull;
}

static void qfDevSlotsFree(QZSTD_Front *f)
{
    int k;
    for (k = 0; f->devSlot && k < 2; k++) {
        QF_DevSlot *s = &f->devSlot[k];
        qfBufsFree(f->devSlotDev, 0, &s->dev, QF_NBUFS(s->dev));
        qfBufsFree(f->devSlotDev, 1, &s->pin, QF_NBUFS(s->pin));
        if (s->stream) qzstd_hip_stream_destroy(f->devSlotDev, s->stream);
        free(s->ends);
        free(s->blkSeq);
        free(s->blkLit);
    }
    free(f->devSlot);
    f->devSlot = NULL;
}

static void qfRestoreSlotsFree(QZSTD_Front *f)
{
    int k;
    for (k = 0; f->restoreSlot && k < 2; k++) {
        QF_RestoreSlot *s = &f->restoreSlot[k];
        qfBufsFree(f->restoreSlotDev, 0, &s->dev, QF_NBUFS(s->dev));
        qfBufsFree(f->restoreSlotDev, 1, &s->pin, QF_NBUFS(s->pin));
        if (s->stream) qzstd_hip_stream_destroy(f->restoreSlotDev, s->stream);
    }
    free(f->restoreSlot);
    f->restoreSlot = NULL;
}

/* ---- the scaffold of a device call.  Every call is: its own host-side checks (nothing has touched a GPU when one of them fails); the
 * look-up of its buffers (qfCallRange / qfCallBufs: all of them memory of ONE device, or the device a QF_SrcMap already knows in `dev`);
 * qfCallBegin; its planning and launches on the streams of the family's slots; qfCallWait; what it reads of the slots' pinned memory and
 * counts; qfCallEnd.  A call that has nothing to do returns before qfCallBegin and takes nothing. */
typedef struct {
    QZSTD_Front *f;
    int restore;  /* the slot family: the restore side's (f->restoreSlot: restore, verify, fingerprint, advise) or the compress side's (f->devSlot) */
    int nStreams; /* 2, or 1: the call uses slot 0 alone, and only its stream is created, made to wait and waited for */
    int dev;      /* -1 until a look-up (or the caller, from a QF_SrcMap) has set it */
    void *ev;
} QF_Call;

static void **qfCallStream(const QF_Call *c, int k)
{
    if (c->restore) return c->f->restoreSlot ? &c->f->restoreSlot[k].stream : NULL;
    return c->f->devSlot ? &c->f->devSlot[k].stream : NULL;
}

/* [p, p + n) is memory of one device, the call's (the first range looked up sets it); an empty range is not looked up */
static int qfCallRange(QF_Call *c, const void *p, size_t n)
{
    int d;
    if (!n) return 0;
    d = qzstd_hip_pointer_device(p);
    if (d < 0 || qzstd_hip_pointer_device((const unsigned char *)p + n - 1) != d || (c->dev >= 0 && d != c->dev)) return -1;
    c->dev = d;
    return 0;
}

/* every buffer, and behind each its base when the call has bases and the buffer one */
static int qfCallBufs(QF_Call *c, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, size_t nBufs)
{
    size_t i;
    for (i = 0; i < nBufs; i++)
        if (qfCallRange(c, bufs[i].d_ptr, bufs[i].size) || (bases && bases[i].d_ptr && qfCallRange(c, bases[i].d_ptr, bases[i].size))) return -1;
    return 0;
}

/* nothing the library queued may still read or write the caller's buffers when a call returns: a bounded wait on every stream of the call,
 * then an unbounded one.  Also what stands between the launches and the reading of the slots' pinned memory.  -> 0, or -1 after a time-out */
static int qfCallWait(const QF_Call *c)
{
    int k, rc = 0;
    for (k = 0; k < c->nStreams; k++) {
        void **s = qfCallStream(c, k);
        if (!s || !*s) continue;
        if (qzstd_hip_stream_wait(c->dev, *s, QF_DEV_WAIT_MS) != 0) {
            (void)qzstd_hip_stream_sync(c->dev, *s);
            rc = -1;
        }
    }
    return rc;
}

static void qfCallEnd(QF_Call *c)
{
    if (c->ev) qzstd_hip_event_destroy(c->dev, c->ev);
    c->ev = NULL;
    pthread_mutex_lock(&c->f->mu);
    c->f->devBusy = 0;
    pthread_mutex_unlock(&c->f->mu);
}

/* Takes devBusy (refused while another device call or a job is in progress); frees the family's slots when they were another device's and
 * makes two — they stay with the front between calls: allocating and freeing pinned and device memory costs more than a part takes —;
 * creates the streams the call uses; and makes them wait for what the caller queued on `stream` so far: the work that produced (or last
 * used) the buffers.  -> 0; -1: refused or failed, and nothing is held */
static int qfCallBegin(QF_Call *c, void *stream)
{
    QZSTD_Front *f = c->f;
    int k, rc = 0;
    c->ev = NULL;
    pthread_mutex_lock(&f->mu);
    if (f->devBusy || f->running) { pthread_mutex_unlock(&f->mu); return -1; }
    f->devBusy = 1;
    pthread_mutex_unlock(&f->mu);
    if (c->restore) {
        if (f->restoreSlot && f->restoreSlotDev != c->dev) qfRestoreSlotsFree(f);
        if (!f->restoreSlot && !(f->restoreSlot = (QF_RestoreSlot *)calloc(2, sizeof(QF_RestoreSlot)))) rc = -1;
        f->restoreSlotDev = c->dev;
    } else {
        if (f->devSlot && f->devSlotDev != c->dev) qfDevSlotsFree(f);
        if (!f->devSlot && !(f->devSlot = (QF_DevSlot *)calloc(2, sizeof(QF_DevSlot)))) rc = -1;
        f->devSlotDev = c->dev;
    }
    for (k = 0; k < c->nStreams && rc == 0; k++) {
        void **s = qfCallStream(c, k);
        if (!*s && !(*s = qzstd_hip_stream_create(c->dev))) rc = -1;
    }
    if (rc == 0 && !(c->ev = qzstd_hip_event_create(c->dev))) rc = -1;
    if (rc == 0 && qzstd_hip_event_record(c->dev, c->ev, stream)) rc = -1;
    for (k = 0; k < c->nStreams && rc == 0; k++)
        if (qzstd_hip_stream_wait_event(c->dev, *qfCallStream(c, k), c->ev)) rc = -1;
    if (rc) {
        (void)qfCallWait(c);
        qfCallEnd(c);
    }
    return rc;
}

/* firstFrame[i]: the first frame of buffer i in a call's numbering; firstFrame[nBufs]: the frames of the call */
static void qfFirstFrames(const QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, size_t *firstFrame)
{
    size_t i, c = 0;
    if (!firstFrame) return;
    for (i = 0; i < nBufs; i++) {
        firstFrame[i] = c;
        c += bufs[i].size / f->p.chunkSize + (bufs[i].size % f->p.chunkSize != 0);
    }
    firstFrame[nBufs] = c;
}

/* $QZSTD_FRONT_DEVICE_PART: bytes of input (of decoded content) per part — whole frames, at least one —, default 64 MiB */
static size_t qfPartBytes(void)
{
    const char *pb = getenv("QZSTD_FRONT_DEVICE_PART");
    return pb && *pb && atoll(pb) > 0 ? (size_t)atoll(pb) : QF_PART_BYTES;
}

typedef struct {
    QZSTD_Front *f;
    const QF_SrcMap *sm;       /* NULL: the buffers are contiguous (every call but QZSTD_frontCompressDeviceSlices) */
    const QF_DevFrame *frames; /* the per-frame table: frame c of the job */
    const QF_DevRange *parts;
    size_t nParts, blk;        /* blk: the launches' largest block, min(chunkSize, 128 KiB) */
    int dev, level;
    int checksum;              /* the front's setting when the call began */
    int probe;                 /* plane probe: the front's setting when the call began, for a call with a grouped or based frame */
    int code;                  /* plane code: likewise; a call with it has `probe` too */
    int failSub;               /* $QZSTD_FRONT_PROBE_FAIL_SUB (tests) */
} QF_DevJob;

static size_t qfPad16(size_t n) { return (n + 15u) & ~(size_t)15u; }
static int qfStagePieces(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr, size_t stageBytes); /* qzstd_srcslices.c */
static int qfFramePiecesD2H(const QF_DevPart *pt, void *stream, const QF_DevFrame *fm, unsigned char *to, int base);

/* The rows of a staging launch: one per frame of the part that is differenced (diffed 1) or not (0), in the frames' order.  Frame c of
 * the part lies in the stage at the sum of the padded lengths before it, whichever launch stages it; a row's length and padding are
 * 32-bit; a frame is padded to the next multiple of 16 and the part's last one by 16 bytes more (the matcher reads 16-aligned blocks and
 * up to the next multiple of 16 past each).  `put` writes row m of its own type.  Grows the row buffers for nf rows of rowSize bytes.
 * -> the rows written, or (size_t)-1 */
typedef void (*QF_RowPut)(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx);

static size_t qfStageRows(const QF_DevJob *j, const QF_DevRange *pr, int diffed, QF_Buf *pin, QF_Buf *dev, size_t rowSize, QF_RowPut put, void *ctx)
{
    const QF_DevFrame *f0 = &j->frames[pr->f0];
    const size_t nf = pr->f1 - pr->f0;
    size_t c, so = 0, m = 0;
    void *rows;
    if (nf > 0xFFFFFFFFu || !(rows = qfBufH(pin, nf * rowSize)) || !qfBufD(j->dev, dev, nf * rowSize)) return (size_t)-1;
    for (c = 0; c < nf; so += qfPad16(f0[c].len), c++) {
        if ((f0[c].diff != 0u) != (diffed != 0)) continue; /* (staged by the part's other launch) */
        if (f0[c].len > 0xFFFFFFE0u) return (size_t)-1;
        put(rows, m++, &f0[c], so, (uint32_t)(qfPad16(f0[c].len) - f0[c].len) + (c + 1 == nf ? 16u : 0u), ctx);
    }
    return m;
}

static void qfPutGather(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx)
{
    qzstd_hip_gather_row_t *r = (qzstd_hip_gather_row_t *)rows + m;
    (void)ctx;
    r->src = (uint64_t)(uintptr_t)fm->src;
    r->dstOff = dstOff;
    r->len = (uint32_t)fm->len;
    r->pad = pad;
}

/* the gather's rows with each frame's element size: the frames arrive in the byte-grouped layout */
static void qfPutGroup(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx)
{
    qzstd_hip_group_row_t *r = (qzstd_hip_group_row_t *)rows + m;
    (void)ctx;
    r->src = (uint64_t)(uintptr_t)fm->src;
    r->dstOff = dstOff;
    r->len = (uint32_t)fm->len;
    r->pad = pad;
    r->elem = fm->k;
    r->reserved = 0;
}

/* the grouping gather's rows with each frame's base chunk (0: the frame's buffer has none): src ^ base arrives, grouped */
static void qfPutXor(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx)
{
    qzstd_hip_group_xor_row_t *r = (qzstd_hip_group_xor_row_t *)rows + m;
    (void)ctx;
    r->src = (uint64_t)(uintptr_t)fm->src;
    r->base = (uint64_t)(uintptr_t)fm->base;
    r->dstOff = dstOff;
    r->len = (uint32_t)fm->len;
    r->pad = pad;
    r->elem = fm->k;
    r->reserved = 0;
}

static void qfPutEdiff(void *rows, size_t m, const QF_DevFrame *fm, uint64_t dstOff, uint32_t pad, void *ctx)
{
    qzstd_hip_group_ediff_row_t *r = (qzstd_hip_group_ediff_row_t *)rows + m;
    (void)ctx;
    r->src = (uint64_t)(uintptr_t)fm->src;
    r->dstOff = dstOff;
    r->len = (uint32_t)fm->len;
    r->pad = pad;
    r->elem = fm->k;
    r->flags = QZSTD_HIP_EDIFF_DIFF;
}

/* stages a part's frames in the slot's stage (qfStageRows says where).  The differenced frames by a launch of their own, at the frames' own
 * places; the others by ONE launch of the part's kind; without the gather — a run of one buffer's chunks only — a memset and up to two 2D
 * copies (the last chunk alone when it is short) */
static int qfStagePart(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr, size_t stageBytes)
{
    const QF_DevFrame *f0 = &j->frames[pr->f0];
    const size_t nf = pr->f1 - pr->f0;
    const int dev = j->dev;
    size_t m;
    if (!qfBufD(dev, &s->dev.stage, stageBytes)) return -1;
    if (pr->diff) {
        if (!qzstd_hip_group_ediff) return -1;
        m = qfStageRows(j, pr, 1, &s->pin.ediffRows, &s->dev.ediffRows, sizeof(qzstd_hip_group_ediff_row_t), qfPutEdiff, NULL);
        if (m == (size_t)-1 || qzstd_hip_group_ediff(dev, s->stream, (const qzstd_hip_group_ediff_row_t *)s->pin.ediffRows.p, (uint32_t)m,
                                                     (qzstd_hip_group_ediff_row_t *)s->dev.ediffRows.p, s->dev.stage.p, stageBytes))
            return -1;
        __atomic_fetch_add(&j->f->ediffStats[0], (unsigned long long)m, __ATOMIC_RELAXED);
        if (m == nf) return 0;
    }
    if (pr->pieces) return qfStagePieces(j, s, pr, stageBytes);
    if (pr->delta) {
        if (!qzstd_hip_group_xor) return -1;
        m = qfStageRows(j, pr, 0, &s->pin.xorRows, &s->dev.xorRows, sizeof(qzstd_hip_group_xor_row_t), qfPutXor, NULL);
        return m == (size_t)-1 ? -1 : qzstd_hip_group_xor(dev, s->stream, (const qzstd_hip_group_xor_row_t *)s->pin.xorRows.p, (uint32_t)m,
                                                          (qzstd_hip_group_xor_row_t *)s->dev.xorRows.p, s->dev.stage.p, stageBytes);
    }
    if (pr->grouped) {
        if (!qzstd_hip_group) return -1;
        m = qfStageRows(j, pr, 0, &s->pin.groupRows, &s->dev.groupRows, sizeof(qzstd_hip_group_row_t), qfPutGroup, NULL);
        return m == (size_t)-1 ? -1 : qzstd_hip_group(dev, s->stream, (const qzstd_hip_group_row_t *)s->pin.groupRows.p, (uint32_t)m,
                                                      (qzstd_hip_group_row_t *)s->dev.groupRows.p, s->dev.stage.p, stageBytes);
    }
    if (qzstd_hip_gather) {
        m = qfStageRows(j, pr, 0, &s->pin.rows, &s->dev.rows, sizeof(qzstd_hip_gather_row_t), qfPutGather, NULL);
        return m == (size_t)-1 ? -1 : qzstd_hip_gather(dev, s->stream, (const qzstd_hip_gather_row_t *)s->pin.rows.p, (uint32_t)m,
                                                       (qzstd_hip_gather_row_t *)s->dev.rows.p, s->dev.stage.p, stageBytes);
    }
    if (!pr->run || pr->diff) return -1;
    {
        const size_t chunk = j->f->p.chunkSize, pitch = qfPad16(chunk), full = pr->bytes / chunk, tail = pr->bytes - full * chunk;
        const unsigned char *base = f0->src;
        unsigned char *stage = (unsigned char *)s->dev.stage.p;
        if (qzstd_hip_memset(dev, s->stream, stage, 0, stageBytes)) return -1;
        if (full && qzstd_hip_memcpy2d_d2d(dev, s->stream, stage, pitch, base, chunk, chunk, full)) return -1;
        if (tail && qzstd_hip_memcpy2d_d2d(dev, s->stream, stage + full * pitch, tail, base + full * chunk, tail, tail, 1)) return -1;
    }
    return 0;
}

/* queues a part on slot s: staging if needed, match-finder, compaction.  Device side only: the slot's pinned arena may still be read by
 * the workers (the part fetched from it before) */
static int qfQueuePart(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr)
{
    const QF_DevFrame *f0 = &j->frames[pr->f0];
    const size_t nf = pr->f1 - pr->f0, nb = pr->nb, blk = j->blk;
    const size_t cap = qzstd_hip_sequence_bound(blk), capPad = (cap + 1u) & ~(size_t)1u;
    const unsigned char *base = f0->src;
    /* in place: one buffer's chunks, address, chunk and length multiples of 16 (every block then starts 16-aligned and ends inside the buffer) */
    const int inPlace = !pr->grouped && !pr->delta && !pr->diff && !pr->pieces && pr->run && ((uintptr_t)base & 15u) == 0 && (j->f->p.chunkSize & 15u) == 0 && (pr->bytes & 15u) == 0;
    size_t c, b = 0, so = 0, seqCapTotal = 0;
    qzstd_hip_block_t *desc;
    int dev = j->dev;
    if (nb > 0xFFFFFFFFu) return -1;
    if (!(desc = (qzstd_hip_block_t *)qfBufH(&s->pin.desc, nb * sizeof(qzstd_hip_block_t)))) return -1;
    for (c = 0; c < nf; c++) {
        const size_t at = inPlace ? f0[c].off - f0->off : so; /* the frame's first byte from the launch's base */
        size_t o = 0, e;
        if (f0[c].b0 != b) return -1;
        /* one descriptor per block of the frame's rule: every 128 KiB, and for a byte-grouped frame a block per plane first */
        if (s->endsCap < f0[c].nb) {
            free(s->ends);
            s->ends = (size_t *)malloc(f0[c].nb * sizeof(size_t));
            s->endsCap = s->ends ? f0[c].nb : 0;
            if (!s->ends) return -1;
        }
        if (QZSTD_byteGroupBlocks(f0[c].len, f0[c].k, s->ends, s->endsCap) != f0[c].nb) return -1;
        for (e = 0; e < f0[c].nb; o = s->ends[e], e++, b++) {
            qzstd_hip_block_t *d = &desc[b];
            d->srcLen = (uint32_t)(s->ends[e] - o);
            d->srcOff = at + o;
            d->seqOff = b * capPad;
            d->seqCap = (uint32_t)cap;
            d->parseFrom = 0;
            d->mark = 0;
            seqCapTotal += cap;
        }
        so += qfPad16(f0[c].len);
    }
    if (b != nb) return -1;
    {
        const size_t work = qzstd_hip_workspace_bytes(j->level, (uint32_t)nb, (uint32_t)blk);
        const size_t arena = QZSTD_HIP_COMPACT_ENTRIES_OFF(nb) + 8u * seqCapTotal + pr->bytes;
        if (!qfBufD(dev, &s->dev.desc, nb * sizeof(qzstd_hip_block_t)) || !qfBufD(dev, &s->dev.seqs, nb * capPad * 16u) ||
            !qfBufD(dev, &s->dev.count, nb * 4u) || !qfBufD(dev, &s->dev.work, work) ||
            !qfBufD(dev, &s->dev.cwork, qzstd_hip_compact_workspace_bytes((uint32_t)nb)) || !qfBufD(dev, &s->dev.arena, arena))
            return -1;
    }
    if (!inPlace) {
        if (qfStagePart(j, s, pr, so + 16u)) return -1;
        base = (const unsigned char *)s->dev.stage.p;
    }
    if (qzstd_hip_memcpy_h2d(dev, s->stream, s->dev.desc.p, desc, nb * sizeof(qzstd_hip_block_t)) ||
        qzstd_hip_find_sequences(dev, s->stream, j->level, base, (const qzstd_hip_block_t *)s->dev.desc.p, (uint32_t)nb, (uint32_t)blk, s->dev.seqs.p,
                                 (uint32_t *)s->dev.count.p, s->dev.work.p, s->dev.work.cap) ||
        qzstd_hip_compact(dev, s->stream, base, (const qzstd_hip_block_t *)s->dev.desc.p, (uint32_t)nb, s->dev.seqs.p, (const uint32_t *)s->dev.count.p,
                          s->dev.arena.p, s->dev.arena.cap, s->dev.cwork.p, s->dev.cwork.cap))
        return -1;
    s->hashed = 0;
    if (j->checksum) {
        /* the frames' content hashes, from the bytes the match-finder was given: frame c at the offset its first block has */
        qzstd_hip_hash_row_t *rows = (qzstd_hip_hash_row_t *)qfBufH(&s->pin.hashRows, nf * sizeof(qzstd_hip_hash_row_t));
        if (!rows || !qfBufD(dev, &s->dev.hashRows, nf * sizeof(qzstd_hip_hash_row_t)) || !qfBufD(dev, &s->dev.hash, nf * 8u)) return -1;
        for (c = 0; c < nf; c++) {
            rows[c].srcOff = desc[f0[c].b0].srcOff;
            rows[c].len = f0[c].len;
        }
        if (nf > 0xFFFFFFFFu || qzstd_hip_xxh64(dev, s->stream, base, rows, (uint32_t)nf, (qzstd_hip_hash_row_t *)s->dev.hashRows.p, (uint64_t *)s->dev.hash.p))
            return -1;
        s->hashed = 1;
    }
    s->probed = 0;
    s->coded = 0;
    if (j->probe && (pr->grouped || pr->delta)) {
        /* the blocks' byte histograms, reduced to their order-0 cost on the device: a row per descriptor, over the stage (such a part is
         * never read in place) */
        qzstd_hip_plane_row_t *rows = (qzstd_hip_plane_row_t *)qfBufH(&s->pin.planeRows, nb * sizeof(qzstd_hip_plane_row_t));
        if (!rows || !qfBufD(dev, &s->dev.planeRows, nb * sizeof(qzstd_hip_plane_row_t)) || !qfBufD(dev, &s->dev.planeCost, nb * sizeof(uint32_t)))
            return -1;
        for (b = 0; b < nb; b++) {
            rows[b].srcOff = desc[b].srcOff;
            rows[b].len = desc[b].srcLen;
            rows[b].reserved = 0;
        }
        if (j->code) {
            /* plane code: the coder leaves the same cost words, and the blocks worth it Huffman-coded — this launch instead of that one */
            const size_t dense = qzstd_hip_huf_code_bytes(rows, (uint32_t)nb);
            if (dense == (size_t)-1 || !qfBufD(dev, &s->dev.hufWords, (2u * nb + 1u) * sizeof(uint32_t)) || !qfBufD(dev, &s->dev.hufDense, dense + 16u) ||
                !qfBufD(dev, &s->dev.hufScratch, QZSTD_HIP_HUF_SCRATCH_BYTES(nb, dense)))
                return -1;
            if (qzstd_hip_huf_code(dev, s->stream, base, rows, (uint32_t)nb, (qzstd_hip_plane_row_t *)s->dev.planeRows.p, (uint32_t *)s->dev.planeCost.p,
                                   (uint32_t *)s->dev.hufWords.p, (uint32_t *)s->dev.hufWords.p + nb, s->dev.hufDense.p, dense, s->dev.hufScratch.p,
                                   QZSTD_HIP_HUF_SCRATCH_BYTES(nb, dense)))
                return -1;
            s->coded = 1;
        } else if (qzstd_hip_plane_cost(dev, s->stream, base, rows, (uint32_t)nb, (qzstd_hip_plane_row_t *)s->dev.planeRows.p, (uint32_t *)s->dev.planeCost.p)) {
            return -1;
        }
        s->probed = 1;
    }
    return 0;
}

/* waits for a queued part, brings its arena back (one D2H) and fills the per-block offsets; -> the part for the workers */
static int qfFetchPart(const QF_DevJob *j, QF_DevSlot *s, const QF_DevRange *pr, QF_DevPart *out)
{
    const size_t nb = pr->nb, nf = pr->f1 - pr->f0;
    const size_t eo = QZSTD_HIP_COMPACT_ENTRIES_OFF(nb);
    const qzstd_hip_compact_hdr_t *hdr;
    const uint32_t *words = NULL;
    unsigned char *arena;
    size_t b, seqs = 0, lits = 0, bytes, dense = 0;
    if (s->pin.arena.cap < eo && !qfBufH(&s->pin.arena, eo + pr->bytes + (pr->bytes >> 2) + QF_LIT_SLACK)) return -1;
    /* the hashes travel with the headers: one more copy per part, 8 bytes per frame, no wait of its own */
    if (s->hashed && (!qfBufH(&s->pin.hash, nf * 8u) || qzstd_hip_memcpy_d2h(j->dev, s->stream, s->pin.hash.p, s->dev.hash.p, nf * 8u))) return -1;
    /* the blocks' costs travel with the headers as the hashes do: 4 bytes per block */
    if (s->probed && (!qfBufH(&s->pin.planeCost, nb * sizeof(uint32_t)) ||
                      qzstd_hip_memcpy_d2h(j->dev, s->stream, s->pin.planeCost.p, s->dev.planeCost.p, nb * sizeof(uint32_t))))
        return -1;
    /* and so do the size words and the dense offsets: 8 bytes per block and 4 */
    if (s->coded && (!(words = (const uint32_t *)qfBufH(&s->pin.hufWords, (2u * nb + 1u) * sizeof(uint32_t))) ||
                     qzstd_hip_memcpy_d2h(j->dev, s->stream, s->pin.hufWords.p, s->dev.hufWords.p, (2u * nb + 1u) * sizeof(uint32_t))))
        return -1;
    if (qzstd_hip_memcpy_d2h(j->dev, s->stream, s->pin.arena.p, s->dev.arena.p, nb * 8u) || qzstd_hip_stream_wait(j->dev, s->stream, QF_DEV_WAIT_MS) != 0)
        return -1;
    if (s->blkCap < nb) {
        free(s->blkSeq);
        free(s->blkLit);
        s->blkSeq = (size_t *)malloc(nb * sizeof(size_t));
        s->blkLit = (size_t *)malloc(nb * sizeof(size_t));
        s->blkCap = s->blkSeq && s->blkLit ? nb : 0;
        if (!s->blkCap) return -1;
    }
    hdr = QF_HDR(s);
    for (b = 0; b < nb; b++) {
        s->blkSeq[b] = seqs;
        s->blkLit[b] = lits;
        if (hdr[b].count == QZSTD_HIP_NSEQ_ERROR) continue;
        seqs += hdr[b].count;
        lits += hdr[b].litBytes;
    }
    bytes = 8u * seqs + lits;
    if (s->pin.arena.cap < eo + bytes + QF_LIT_SLACK) {
        /* THE buffer that grows and keeps its contents, by hand (an eighth more than this part needs): the headers move along */
        unsigned char *n = (unsigned char *)qzstd_hip_host_alloc(eo + bytes + QF_LIT_SLACK + (bytes >> 3));
        if (!n) return -1;
        memcpy(n, s->pin.arena.p, nb * 8u);
        qzstd_hip_host_free(s->pin.arena.p);
        s->pin.arena.p = n;
        s->pin.arena.cap = eo + bytes + QF_LIT_SLACK + (bytes >> 3);
    }
    arena = (unsigned char *)s->pin.arena.p;
    if (s->coded) {
        /* the dense area: one more copy behind the header wait, as long as the offsets say; it shares the entries' wait */
        dense = words[2u * nb];
        if (dense && (!qfBufH(&s->pin.hufDense, dense) || qzstd_hip_memcpy_d2h(j->dev, s->stream, s->pin.hufDense.p, s->dev.hufDense.p, dense))) return -1;
    }
    if (bytes && qzstd_hip_memcpy_d2h(j->dev, s->stream, arena + eo, (const unsigned char *)s->dev.arena.p + eo, bytes)) return -1;
    if ((bytes || dense) && qzstd_hip_stream_wait(j->dev, s->stream, QF_DEV_WAIT_MS) != 0) return -1;
    memset(arena + eo + bytes, 0, QF_LIT_SLACK);
    s->hLit = arena + eo + 8u * seqs;
    s->litTotal = lits;
    __atomic_fetch_add(&j->f->devStats[2], (unsigned long long)(nb * 8u + bytes + (s->hashed ? nf * 8u : 0u) +
                                                           (s->probed ? nb * 4u : 0u) + (s->coded ? (2u * nb + 1u) * 4u + dense : 0u)),
                       __ATOMIC_RELAXED);
    if (s->probed) __atomic_fetch_add(&j->f->probeStats[0], (unsigned long long)nb, __ATOMIC_RELAXED);
    if (s->coded) {
        unsigned long long coded = 0;
        for (b = 0; b < nb; b++) coded += words[b] != 0u;
        __atomic_fetch_add(&j->f->codeStats[0], coded, __ATOMIC_RELAXED);
    }
    out->hashed = s->hashed;
    out->probed = s->probed;
    out->coded = s->coded;
    out->failSub = j->failSub;
    out->sm = j->sm;
    out->frames = j->frames;
    out->f0 = pr->f0;
    out->f1 = pr->f1;
    out->nb = nb;
    out->slot = s;
    out->dev = j->dev;
    return 0;
}

/* 1 when the frame ZSTD_compressSequencesAndLiterals built holds a Compressed block that libzstd stores raw — that
 * function cannot, ZSTD_compressSequences does when the body does not beat the block's source (ends[k] - ends[k - 1] bytes: the frame's own block lengths) by
 * ZSTD_minGain = (srcSize >> 6) + 2 bytes.  That is the gain of every strategy below btultra; above it the gain is smaller, and a frame
 * this catches without need takes the raw-bytes path and comes out the same.  Walks the frame header (descriptor: single segment,
 * dictionary ID and content size fields) and the 3-byte block headers. */
static int qfStoresRawBlock(const unsigned char *fr, size_t frSize, const size_t *ends, size_t nEnds)
{
    static const unsigned char didBytes[4] = { 0, 1, 2, 4 }, fcsBytes[4] = { 0, 2, 4, 8 };
    const unsigned fhd = fr[4], single = (fhd >> 5) & 1u;
    size_t pos = 5 + !single + didBytes[fhd & 3u] + ((fhd >> 6) == 0 ? single : fcsBytes[fhd >> 6]), k;
    for (k = 0; pos + 3 <= frSize && k < nEnds; k++) {
        const unsigned h = fr[pos] | (unsigned)fr[pos + 1] << 8 | (unsigned)fr[pos + 2] << 16;
        const size_t body = h >> 3, src = ends[k] - (k ? ends[k - 1] : 0);
        if (((h >> 1) & 3u) == 2u && body + (src >> 6) + 2 >= src) return 1;
        pos += 3 + (((h >> 1) & 3u) == 1u ? 1 : body);
        if (h & 1u) break; /* Last_Block */
    }
    return 0;
}

/* Magic and frame header of a frame the library writes itself (the canonical zero frame, a frame assembled around raw-predicted blocks):
 * a frame header descriptor with Single_Segment and the smallest Frame_Content_Size field that holds len (and Content_Checksum_Flag when
 * `checksum`), then that field.  -> bytes written, 6 .. 13 */
static size_t qfFrameHeader(unsigned char *out, size_t len, int checksum)
{
    const unsigned long long L = (unsigned long long)len;
    const unsigned code = L <= 255u ? 0u : (L <= 65791u ? 1u : (L <= 0xFFFFFFFFull ? 2u : 3u)), fcs = code == 0u ? 1u : 1u << code;
    const unsigned long long v = code == 1u ? L - 256u : L;
    size_t pos = 0;
    unsigned i;
    out[pos++] = 0x28; out[pos++] = 0xB5; out[pos++] = 0x2F; out[pos++] = 0xFD;
    out[pos++] = (unsigned char)(code << 6 | 0x20u | (checksum ? 4u : 0u));
    for (i = 0; i < fcs; i++) out[pos++] = (unsigned char)(v >> (8u * i));
    return pos;
}

/* plane probe: 1 when block b of the fetched part (len bytes, its compaction header h) is raw-predicted */
static int qfBlockIsRaw(const QF_DevSlot *s, const qzstd_hip_compact_hdr_t *h, size_t b, size_t len)
{
    return len <= QZSTD_PLANE_LEN_MAX && h->count != QZSTD_HIP_NSEQ_ERROR && h->litBytes <= len &&
           QZSTD_planeIsRaw(((const uint32_t *)s->pin.planeCost.p)[b], (uint32_t)len, (uint32_t)(len - h->litBytes));
}

static int qfGrowBytes(unsigned char **p, size_t *cap, size_t need)
{
    if (*cap >= need && *p) return 0;
    free(*p);
    *p = (unsigned char *)malloc(need ? need : 1u);
    *cap = *p ? need : 0;
    return *p ? 0 : -1;
}

/* Plane probe: frame c of a probed part, whose entries are unpacked in w->seqs and whose block ends are w->ends, assembled by the library
 * when at least one of its blocks is raw-predicted (QZSTD_planeIsRaw over the block's cost from the GPU, its length and its matched bytes).
 *   raw-predicted block -> a 3-byte Raw_Block header and its content: its literals where they lie in the arena when it has no sequences,
 *                          else that block alone executed from its own entries and literals (qzbgRebuild);
 *   the others, in order -> ONE ZSTD_compressSequencesAndLiterals call over their content alone, into the worker's scratch; its blocks
 *                          (header + body) are copied to their places, Last_Block rewritten.
 * The splice is valid because an entry's offset never leaves its block (every block is matched on its own), so no Compressed block refers to
 * bytes of a block that is not in the sub-frame, and because a Raw_Block changes neither the decoder's repeat offsets nor its entropy
 * tables: every Compressed block meets in the spliced frame the decoder state it was coded against.
 * -> 0: dst holds the frame and everything is counted; 1: no raw-predicted block, or the frame must take the setting-off path (counted in
 * [3] then); -1: out of memory. */
static int qfAssembleFrame(QZSTD_Front *f, QF_Worker *w, const QF_DevPart *pt, const QF_DevFrame *fm, size_t c, int maybeRle,
                           unsigned char *dst)
{
    static const unsigned char didBytes[4] = { 0, 1, 2, 4 }, fcsBytes[4] = { 0, 2, 4, 8 };
    const QF_DevSlot *s = pt->slot;
    const qzstd_hip_compact_hdr_t *hdr = QF_HDR(s);
    const size_t n = fm->len, b0 = fm->b0, nb = fm->nb, cap = f->stride;
    size_t e, o, nRaw = 0, subSeqs = 0, subLit = 0, subSize = 0, runs = 0, firstSub = 0, pos, sp = 0, r = 0;
    int prevRaw = 1;
    for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
        const size_t len = w->ends[e] - o, b = b0 + e;
        if (qfBlockIsRaw(s, &hdr[b], b, len)) {
            nRaw++;
            prevRaw = 1;
        } else {
            if (prevRaw && !runs++) firstSub = b;
            prevRaw = 0;
            subSeqs += hdr[b].count;
            subLit += hdr[b].litBytes;
            subSize += len;
        }
    }
    if (nRaw == 0) return 1;
    if (maybeRle || (nRaw < nb && !qfSeqLit)) goto fallback;
    if (nRaw < nb) {
        const unsigned char *lit;
        size_t litCap, k = 0, l = 0;
        if (w->subSeqsCap < subSeqs) {
            free(w->subSeqs);
            w->subSeqs = (ZSTD_Sequence *)malloc(subSeqs * sizeof(ZSTD_Sequence));
            w->subSeqsCap = w->subSeqs ? subSeqs : 0;
            if (!w->subSeqs) return -1;
        }
        if (qfGrowBytes(&w->sub, &w->subCap, cap)) return -1;
        /* one run of such blocks (the common case: the noise planes lie in front): its literals are read where they lie in the arena */
        if (runs > 1 && qfGrowBytes(&w->subLit, &w->subLitCap, subLit + QF_LIT_SLACK)) return -1;
        for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
            const size_t len = w->ends[e] - o, b = b0 + e;
            if (qfBlockIsRaw(s, &hdr[b], b, len))
                continue;
            memcpy(&w->subSeqs[k], &w->seqs[s->blkSeq[b] - s->blkSeq[b0]], hdr[b].count * sizeof(ZSTD_Sequence));
            k += hdr[b].count;
            if (runs > 1) {
                memcpy(w->subLit + l, s->hLit + s->blkLit[b], hdr[b].litBytes);
                l += hdr[b].litBytes;
            }
        }
        if (runs > 1) {
            memset(w->subLit + subLit, 0, QF_LIT_SLACK);
            lit = w->subLit;
            litCap = subLit + QF_LIT_SLACK;
        } else {
            lit = s->hLit + s->blkLit[firstSub];
            litCap = s->litTotal - s->blkLit[firstSub] + QF_LIT_SLACK;
        }
        (void)ZSTD_CCtx_reset(w->zc, ZSTD_reset_session_only);
        if (ZSTD_isError(ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 1)) || qfCtxChecksum(w, 0)) goto fallback;
        r = qfSeqLit(w->zc, w->sub, cap, w->subSeqs, subSeqs, lit, subLit, litCap, subSize);
        if (ZSTD_isError(r) || pt->failSub || r < 6u) goto fallback;
        /* the sub-frame's blocks, one per block handed in: none that libzstd would store raw (qfStoresRawBlock's rule), Last_Block on the
         * final one alone, and nothing behind it */
        {
            const unsigned fhd = w->sub[4], single = (fhd >> 5) & 1u;
            size_t p;
            sp = 5 + !single + didBytes[fhd & 3u] + ((fhd >> 6) == 0 ? single : fcsBytes[fhd >> 6]);
            p = sp;
            k = 0;
            for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
                const size_t len = w->ends[e] - o, b = b0 + e;
                unsigned h, type;
                size_t body;
                if (qfBlockIsRaw(s, &hdr[b], b, len))
                    continue;
                if (p + 3 > r) goto fallback;
                h = w->sub[p] | (unsigned)w->sub[p + 1] << 8 | (unsigned)w->sub[p + 2] << 16;
                type = (h >> 1) & 3u;
                body = type == 1u ? 1u : h >> 3;
                if (type == 3u || (type == 2u && body + (len >> 6) + 2 >= len)) goto fallback;
                if ((type == 2u ? 0u : h >> 3) != (type == 2u ? 0u : len)) goto fallback; /* a Raw or RLE block names its regenerated size */
                k += len;
                if (((h & 1u) != 0u) != (k == subSize)) goto fallback;
                p += 3 + body;
                if (p > r) goto fallback;
            }
            if (p != r) goto fallback;
        }
    }
    /* the frame itself */
    if (13u + 3u * nb + 4u > cap) goto fallback;
    pos = qfFrameHeader(dst, n, pt->hashed);
    for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
        const size_t len = w->ends[e] - o, b = b0 + e;
        const unsigned last = e + 1 == nb ? 1u : 0u;
        if (qfBlockIsRaw(s, &hdr[b], b, len)) {
            const unsigned h = (unsigned)(len << 3) | last; /* Block_Size, Raw_Block, Last_Block */
            if (pos + 3 + len + 4u > cap) goto fallback;
            dst[pos++] = (unsigned char)h; dst[pos++] = (unsigned char)(h >> 8); dst[pos++] = (unsigned char)(h >> 16);
            if (hdr[b].count == 1u && hdr[b].litBytes == len) {
                memcpy(dst + pos, s->hLit + s->blkLit[b], len);
            } else if (qzbgRebuild(dst + pos, len, &w->seqs[s->blkSeq[b] - s->blkSeq[b0]].offset, hdr[b].count, s->hLit + s->blkLit[b],
                                   hdr[b].litBytes, &len, 1) != 0) {
                goto fallback;
            }
            pos += len;
        } else {
            const unsigned h = w->sub[sp] | (unsigned)w->sub[sp + 1] << 8 | (unsigned)w->sub[sp + 2] << 16;
            const size_t whole = 3 + (((h >> 1) & 3u) == 1u ? 1u : h >> 3);
            if (pos + whole + 4u > cap) goto fallback;
            memcpy(dst + pos, w->sub + sp, whole);
            dst[pos] = (unsigned char)((dst[pos] & ~1u) | last);
            pos += whole;
            sp += whole;
        }
    }
    if (nRaw < nb) (void)ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 0);
    if (pt->hashed) {
        const uint64_t h = ((const uint64_t *)s->pin.hash.p)[c];
        dst[pos++] = (unsigned char)h; dst[pos++] = (unsigned char)(h >> 8); dst[pos++] = (unsigned char)(h >> 16); dst[pos++] = (unsigned char)(h >> 24);
        __atomic_fetch_add(&f->cksumStats[0], 1ull, __ATOMIC_RELAXED);
    }
    f->sizes[fm->idx] = pos;
    __atomic_fetch_add(&f->devStats[0], 1ull, __ATOMIC_RELAXED);
    if (fm->k > 1u) __atomic_fetch_add(&f->groupStats[0], 1ull, __ATOMIC_RELAXED);
    if (fm->based) __atomic_fetch_add(&f->deltaStats[0], 1ull, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->probeStats[1], (unsigned long long)nRaw, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->probeStats[2], 1ull, __ATOMIC_RELAXED);
    if (pt->coded && nRaw == nb) __atomic_fetch_add(&f->codeStats[2], 1ull, __ATOMIC_RELAXED); /* (all raw: no libzstd call either) */
    return 0;
fallback:
    __atomic_fetch_add(&f->probeStats[3], 1ull, __ATOMIC_RELAXED);
    return 1;
}

/* plane code: the bytes of block b's QZSTD_hufBlockBody (0: none, or the block is not taken by QZSTD_hufTakes) */
static size_t qfBlockTaken(const QF_DevSlot *s, const qzstd_hip_compact_hdr_t *h, size_t nbPart, size_t b, size_t len)
{
    const uint32_t *words = (const uint32_t *)s->pin.hufWords.p;
    const uint32_t size = words[b];
    const unsigned char *at;
    uint8_t nbits[256], tree[QZSTD_HUF_TREE_MAX];
    size_t t, body;
    if (!size || len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX || h->count == QZSTD_HIP_NSEQ_ERROR) return 0;
    at = (const unsigned char *)s->pin.hufDense.p + words[nbPart + b];
    QZSTD_hufUnpackLengths(at, nbits);
    t = QZSTD_hufWriteTree(nbits, tree, sizeof(tree));
    if (!t) return 0;
    body = (len <= 16383u ? 4u : 5u) + t + size + 1u;
    return QZSTD_hufTakes(size, (uint32_t)body, (uint32_t)len, h->litBytes, h->count) ? body : 0;
}

/* Plane code: frame c of a coded part, assembled WITHOUT any libzstd call when every block of it is raw-predicted (qfBlockIsRaw) or taken
 * (QZSTD_hufTakes) and at least one is taken:
 *   raw-predicted block -> as in qfAssembleFrame;
 *   taken block         -> a 3-byte Compressed_Block header and QZSTD_hufBlockBody over the code lengths and streams from the GPU.
 * All or nothing: a Compressed block of libzstd's sub-frame may repeat the Huffman table of the block before it, and a block coded here in
 * front of it would change that table — a frame with any other block takes exactly the path it takes with the probe on.
 * -> 0: dst holds the frame and everything is counted; 1: not such a frame (counted in [3] when it had a taken block); -1: out of memory. */
static int qfAssembleCoded(QZSTD_Front *f, QF_Worker *w, const QF_DevPart *pt, const QF_DevFrame *fm, size_t c, unsigned char *dst)
{
    const QF_DevSlot *s = pt->slot;
    const qzstd_hip_compact_hdr_t *hdr = QF_HDR(s);
    const size_t n = fm->len, b0 = fm->b0, nb = fm->nb, cap = f->stride;
    size_t e, o, nRaw = 0, nTaken = 0, pos;
    for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
        const size_t len = w->ends[e] - o, b = b0 + e;
        if (qfBlockIsRaw(s, &hdr[b], b, len)) nRaw++;
        else if (qfBlockTaken(s, &hdr[b], pt->nb, b, len)) nTaken++;
    }
    if (!nTaken) return 1;
    if (nRaw + nTaken < nb || 13u + 3u * nb + 4u > cap) goto fallback;
    pos = qfFrameHeader(dst, n, pt->hashed);
    for (e = 0, o = 0; e < nb; o = w->ends[e], e++) {
        const size_t len = w->ends[e] - o, b = b0 + e;
        const unsigned last = e + 1 == nb ? 1u : 0u;
        if (qfBlockIsRaw(s, &hdr[b], b, len)) {
            const unsigned h = (unsigned)(len << 3) | last; /* Block_Size, Raw_Block, Last_Block */
            if (pos + 3 + len + 4u > cap) goto fallback;
            dst[pos++] = (unsigned char)h; dst[pos++] = (unsigned char)(h >> 8); dst[pos++] = (unsigned char)(h >> 16);
            if (hdr[b].count == 1u && hdr[b].litBytes == len) {
                memcpy(dst + pos, s->hLit + s->blkLit[b], len);
            } else if (qzbgRebuild(dst + pos, len, &w->seqs[s->blkSeq[b] - s->blkSeq[b0]].offset, hdr[b].count, s->hLit + s->blkLit[b],
                                   hdr[b].litBytes, &len, 1) != 0) {
                goto fallback;
            }
            pos += len;
        } else {
            const uint32_t *words = (const uint32_t *)s->pin.hufWords.p;
            const unsigned char *at = (const unsigned char *)s->pin.hufDense.p + words[pt->nb + b];
            uint8_t nbits[256];
            size_t body;
            unsigned h;
            if (pos + 3u + len + 4u > cap) goto fallback; /* (a taken body is below len) */
            QZSTD_hufUnpackLengths(at, nbits);
            body = QZSTD_hufBlockBody(nbits, (uint32_t)len, at + QZSTD_HUF_LENGTHS_BYTES, words[b], dst + pos + 3u, len);
            if (!body) goto fallback;
            h = (unsigned)(body << 3) | (2u << 1) | last; /* Block_Size, Compressed_Block, Last_Block */
            dst[pos++] = (unsigned char)h; dst[pos++] = (unsigned char)(h >> 8); dst[pos++] = (unsigned char)(h >> 16);
            pos += body;
        }
    }
    if (pt->hashed) {
        const uint64_t h = ((const uint64_t *)s->pin.hash.p)[c];
        dst[pos++] = (unsigned char)h; dst[pos++] = (unsigned char)(h >> 8); dst[pos++] = (unsigned char)(h >> 16); dst[pos++] = (unsigned char)(h >> 24);
        __atomic_fetch_add(&f->cksumStats[0], 1ull, __ATOMIC_RELAXED);
    }
    f->sizes[fm->idx] = pos;
    __atomic_fetch_add(&f->devStats[0], 1ull, __ATOMIC_RELAXED);
    if (fm->k > 1u) __atomic_fetch_add(&f->groupStats[0], 1ull, __ATOMIC_RELAXED);
    if (fm->based) __atomic_fetch_add(&f->deltaStats[0], 1ull, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->probeStats[1], (unsigned long long)nRaw, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->probeStats[2], 1ull, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->codeStats[1], (unsigned long long)nTaken, __ATOMIC_RELAXED);
    __atomic_fetch_add(&f->codeStats[2], 1ull, __ATOMIC_RELAXED);
    return 0;
fallback:
    __atomic_fetch_add(&f->codeStats[3], 1ull, __ATOMIC_RELAXED);
    return 1;
}

/* frame c of the part in progress -> zstd frame */
static int qfDeviceFrame(QZSTD_Front *f, QF_Worker *w, size_t c)
{
    const QF_DevPart *pt = f->part;
    const QF_DevSlot *s = pt->slot;
    const size_t cg = pt->f0 + c;
    const QF_DevFrame *fm = &pt->frames[cg];
    const size_t n = fm->len, b0 = fm->b0, b1 = b0 + fm->nb;
    const qzstd_hip_compact_hdr_t *hdr = QF_HDR(s);
    const size_t eo = QZSTD_HIP_COMPACT_ENTRIES_OFF(pt->nb);
    const unsigned long long *ent = (const unsigned long long *)(const void *)((const unsigned char *)s->pin.arena.p + eo);
    size_t b, ns = 0, nl = 0, k, r = 0;
    int failedBlock = 0, haveSeqs = 0, maybeRle = 0;
    const int grouped = fm->k > 1u;
    const int dBase = fm->based != 0u; /* the frame's content is chunk ^ base chunk */
    unsigned char *dst = f->dst + fm->idx * f->stride;
    /* the frame's block ends (every 128 KiB; a byte-grouped frame's planes first) */
    if (w->endsCap < fm->nb) {
        free(w->ends);
        w->ends = (size_t *)malloc(fm->nb * sizeof(size_t));
        w->endsCap = w->ends ? fm->nb : 0;
        if (!w->ends) return -1;
    }
    if (QZSTD_byteGroupBlocks(n, fm->k, w->ends, w->endsCap) != fm->nb) return -1;
    for (b = b0; b < b1; b++) {
        if (hdr[b].count == QZSTD_HIP_NSEQ_ERROR) failedBlock = 1;
        else { ns += hdr[b].count; nl += hdr[b].litBytes; }
        /* A plane of one value (the high bytes of small integers) is a block ZSTD_compressSequences may store as RLE — never the frame's
         * first block, and only one of fewer than 4 sequences and fewer than 10 literal bytes (ZSTD_maybeRLE) — which
         * ZSTD_compressSequencesAndLiterals cannot: it has no content to look at.  Such a frame is built from its content, like one with
         * a raw block.  (Byte-grouped frames only: the frames of ungrouped input stay what they were.) */
        if (grouped && b > b0 && hdr[b].count != QZSTD_HIP_NSEQ_ERROR && hdr[b].count < 5u && hdr[b].litBytes < 10u) maybeRle = 1;
    }
    if (!failedBlock) {
        const unsigned long long *q = ent + s->blkSeq[b0];
        if (w->seqsCap < ns) {
            free(w->seqs);
            w->seqs = (ZSTD_Sequence *)malloc(ns * sizeof(ZSTD_Sequence));
            w->seqsCap = w->seqs ? ns : 0;
            if (!w->seqs) return -1;
        }
        for (k = 0; k < ns; k++) {
            const unsigned long long v = q[k];
            w->seqs[k].offset = QZSTD_HIP_PACKED_OFF(v);
            w->seqs[k].litLength = QZSTD_HIP_PACKED_LIT(v);
            w->seqs[k].matchLength = QZSTD_HIP_PACKED_ML(v);
            w->seqs[k].rep = 0;
        }
        haveSeqs = 1;
        if (pt->coded) {
            /* plane code: a frame of raw-predicted and taken blocks alone is assembled here; every other frame goes on as with the probe on */
            const int a = qfAssembleCoded(f, w, pt, fm, c, dst);
            if (a <= 0) return a;
        }
        if (pt->probed) {
            /* plane probe: a frame with a raw-predicted block is assembled here; every other frame goes on as with the setting off */
            const int a = qfAssembleFrame(f, w, pt, fm, c, maybeRle, dst);
            if (a <= 0) return a;
        }
        /* (a session that ended in an error leaves the CCtx mid-frame, where parameters cannot be set: every frame starts afresh) */
        (void)ZSTD_CCtx_reset(w->zc, ZSTD_reset_session_only);
        if (ZSTD_isError(ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 1))) return -1;
        if (qfSeqLit && !maybeRle && qfCtxChecksum(w, 0) == 0) { /* (ZSTD_compressSequencesAndLiterals refuses the checksum flag) */
            /* the frame's literals straight from the arena; everything behind them (later frames' literals, the slack) is readable */
            const unsigned char *lit = s->hLit + s->blkLit[b0];
            const size_t litCap = s->litTotal - s->blkLit[b0] + QF_LIT_SLACK;
            r = qfSeqLit(w->zc, dst, f->stride, w->seqs, ns, lit, nl, litCap, n);
            if (!ZSTD_isError(r) && !qfStoresRawBlock(dst, r, w->ends, fm->nb) && (!pt->hashed || r + 4u <= f->stride)) {
                (void)ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 0);
                if (pt->hashed) {
                    /* Content_Checksum_Flag (bit 2 of the frame header descriptor) and the hash's low 32 bits behind the last block */
                    const uint64_t h = ((const uint64_t *)s->pin.hash.p)[c];
                    dst[4] |= 4u;
                    dst[r] = (unsigned char)h;
                    dst[r + 1] = (unsigned char)(h >> 8);
                    dst[r + 2] = (unsigned char)(h >> 16);
                    dst[r + 3] = (unsigned char)(h >> 24);
                    r += 4u;
                    __atomic_fetch_add(&f->cksumStats[0], 1ull, __ATOMIC_RELAXED);
                }
                f->sizes[fm->idx] = r;
                __atomic_fetch_add(&f->devStats[0], 1ull, __ATOMIC_RELAXED);
                if (grouped) __atomic_fetch_add(&f->groupStats[0], 1ull, __ATOMIC_RELAXED);
                if (dBase) __atomic_fetch_add(&f->deltaStats[0], 1ull, __ATOMIC_RELAXED);
                return 0;
            }
        }
    }
    /* the raw bytes: a block libzstd would store raw (ZSTD_compressSequencesAndLiterals cannot), a block the matcher failed,
     * or a libzstd without the function.  Sequences -> ZSTD_compressSequences, the identical frame; a failed block -> ZSTD_compress2 on
     * this CCtx: its producer fails the same block and libzstd's own match-finder takes it, as on the host path */
    if (!w->raw || w->rawDev != pt->dev) {
        if (w->raw) qzstd_hip_host_free(w->raw);
        if (w->rawStream) qzstd_hip_stream_destroy(w->rawDev, w->rawStream);
        w->raw = (unsigned char *)qzstd_hip_host_alloc(f->p.chunkSize);
        w->rawStream = qzstd_hip_stream_create(pt->dev);
        w->rawDev = pt->dev;
        if (!w->raw || !w->rawStream) return -1;
    }
    /* A byte-grouped frame's content is not what the caller's buffer holds, and in grouped mode this is the common path (a mantissa plane is
     * noise: a raw block).  The arena has everything: the frame's own entries and literals, executed, ARE the grouped content — no second
     * device->host copy, and no look at the stage, which may hold the part after next by now */
    if ((grouped || dBase || fm->diff) && haveSeqs &&
        qzbgRebuild(w->raw, n, ns ? &w->seqs[0].offset : NULL, ns, s->hLit + s->blkLit[b0], nl, w->ends, fm->nb) == 0) {
        if (grouped) __atomic_fetch_add(&f->groupStats[1], 1ull, __ATOMIC_RELAXED);
        if (dBase) __atomic_fetch_add(&f->deltaStats[1], 1ull, __ATOMIC_RELAXED);
    } else {
        unsigned char *to = w->raw;
        if (grouped || dBase || fm->diff) {
            /* a failed block (or entries that do not rebuild): the caller's bytes come back and are grouped here; no sequences are used */
            if (!w->back && !(w->back = (unsigned char *)qzstd_hip_host_alloc(f->p.chunkSize))) return -1;
            to = w->back;
            haveSeqs = 0;
        }
        /* (a frame of several source slices: one copy per piece into the same buffer) */
        if (fm->np > 1u ? qfFramePiecesD2H(pt, w->rawStream, fm, to, 0) : qzstd_hip_memcpy_d2h(pt->dev, w->rawStream, to, fm->src, n)) return -1;
        if (qzstd_hip_stream_wait(pt->dev, w->rawStream, QF_DEV_WAIT_MS) != 0) {
            /* the copy still reads the caller's buffer: the call must not return before it is done */
            (void)qzstd_hip_stream_sync(pt->dev, w->rawStream);
            return -1;
        }
        __atomic_fetch_add(&f->devStats[2], (unsigned long long)n, __ATOMIC_RELAXED);
        if (dBase) {
            /* the base's bytes too (into raw, which the grouping below overwrites), XORed into the caller's */
            if (fm->np > 1u ? qfFramePiecesD2H(pt, w->rawStream, fm, w->raw, 1) : qzstd_hip_memcpy_d2h(pt->dev, w->rawStream, w->raw, fm->base, n)) return -1;
            if (qzstd_hip_stream_wait(pt->dev, w->rawStream, QF_DEV_WAIT_MS) != 0) {
                (void)qzstd_hip_stream_sync(pt->dev, w->rawStream);
                return -1;
            }
            __atomic_fetch_add(&f->devStats[2], (unsigned long long)n, __ATOMIC_RELAXED);
            QZSTD_byteXor(w->back, w->back, w->raw, n);
            __atomic_fetch_add(&f->deltaStats[2], 1ull, __ATOMIC_RELAXED);
        }
        if (fm->diff) {
            /* (a differenced frame's buffer has no base) the differences are taken here, in place, before the grouping */
            if (QZSTD_elemDiff(w->back, w->back, n, fm->k) != n) return -1;
            __atomic_fetch_add(&f->ediffStats[1], 1ull, __ATOMIC_RELAXED);
        }
        if (grouped || dBase || fm->diff) {
            if (QZSTD_byteGroup(w->raw, w->back, n, fm->k) != n) return -1;
            if (grouped) __atomic_fetch_add(&f->groupStats[2], 1ull, __ATOMIC_RELAXED);
        }
    }
    __atomic_fetch_add(&f->devStats[1], 1ull, __ATOMIC_RELAXED);
    /* libzstd has the content here and hashes it itself */
    if (qfCtxChecksum(w, pt->hashed)) return -1;
    if (pt->hashed) __atomic_fetch_add(&f->cksumStats[1], 1ull, __ATOMIC_RELAXED);
    if (haveSeqs && qfSeq) {
        (void)ZSTD_CCtx_reset(w->zc, ZSTD_reset_session_only);
        r = qfSeq(w->zc, dst, f->stride, w->seqs, ns, w->raw, n);
        if (!ZSTD_isError(r)) {
            (void)ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 0);
            f->sizes[fm->idx] = r;
            return 0;
        }
    }
    (void)ZSTD_CCtx_reset(w->zc, ZSTD_reset_session_only);
    (void)ZSTD_CCtx_setParameter(w->zc, ZSTD_c_blockDelimiters, 0);
    r = ZSTD_compress2(w->zc, dst, f->stride, w->raw, n);
    if (ZSTD_isError(r)) return -1;
    f->sizes[fm->idx] = r;
    return 0;
}

size_t QZSTD_frontDeviceBatchFrames(const QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs)
{
    size_t i, n = 0;
    if (!f || (nBufs && !bufs)) return (size_t)-1;
    for (i = 0; i < nBufs; i++) n += bufs[i].size / f->p.chunkSize + (bufs[i].size % f->p.chunkSize != 0);
    return n;
}

/* the per-frame table and the parts of a job.  A part takes whole frames, across buffer boundaries, until the next one would take its input
 * past partBytes or its blocks past four times the blocks of a part of full ones (a block costs the device the same scratch whatever its
 * length); at least one frame.  equal: NULL, or per frame of the call 1 for a frame found equal to its base chunk (QZSTD_frontSetDeltaSkip):
 * it is left out of the table and of the parts, so frame m of the table is frame fr[m].idx of the call, and the frames around it are not
 * consecutive chunks. */
/* source slices: the pieces that hold bytes [off, off + len) of their buffer, len > 0 — *p, the piece a search starts from, moves on to the
 * first of them (frames ascend, so it only moves forward), and their count is returned */
static size_t qfSrcFramePieces(const QF_SrcMap *sm, size_t *p, size_t off, size_t len)
{
    size_t np = 1;
    while (sm->pieces[*p].off + sm->pieces[*p].size <= off) (*p)++;
    while (sm->pieces[*p + np - 1u].off + sm->pieces[*p + np - 1u].size < off + len) np++;
    return np;
}

/* piece q of the map, cut to a frame: its bytes [*lo, *hi) of bytes [off, off + len) of the buffer */
static void qfPieceInFrame(const QF_SrcPiece *q, size_t off, size_t len, size_t *lo, size_t *hi)
{
    *lo = q->off > off ? q->off : off;
    *hi = q->off + q->size < off + len ? q->off + q->size : off + len;
}

/* the piece table of such a frame for the kernels that read pieces: pieces [p, p + np) of the map cut to bytes [off, off + len) of their
 * buffer, offsets counted from the frame's first byte; bases: with the pieces' bases (else 0: none is ever read) */
static void qfSrcFrameTable(const QF_SrcMap *sm, size_t p, size_t np, size_t off, size_t len, int bases, qzstd_hip_group_piece_t *out)
{
    size_t k;
    for (k = 0; k < np; k++) {
        const QF_SrcPiece *q = &sm->pieces[p + k];
        size_t lo, hi;
        qfPieceInFrame(q, off, len, &lo, &hi);
        out[k].src = (uint64_t)(uintptr_t)(q->src + (lo - q->off));
        out[k].base = bases && q->base ? (uint64_t)(uintptr_t)(q->base + (lo - q->off)) : 0u;
        out[k].off = (uint32_t)(lo - off);
        out[k].len = (uint32_t)(hi - lo);
    }
}

static int qfPlanDevice(const QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const QF_SrcMap *sm,
                        const unsigned char *elemSizes, unsigned group, size_t nBufs, const unsigned char *equal,
                        size_t nFrames, size_t partBytes, size_t blk, QF_DevFrame **framesOut, QF_DevRange **partsOut, size_t *nPartsOut)
{
    const size_t chunk = f->p.chunkSize, maxBlocks = 4u * (partBytes / blk ? partBytes / blk : 1u);
    QF_DevFrame *fr = (QF_DevFrame *)malloc(nFrames * sizeof(*fr));
    QF_DevRange *pt = (QF_DevRange *)malloc(nFrames * sizeof(*pt)), *cur = NULL;
    size_t i, c = 0, m = 0, nParts = 0;
    if (!fr || !pt) { free(fr); free(pt); return -1; }
    for (i = 0; i < nBufs; i++) {
        const unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : group, k = e & ~QZSTD_ELEM_DIFF;
        size_t off, p = sm ? sm->first[i] : 0; /* (source slices: the piece that holds the frame's first byte) */
        for (off = 0; off < bufs[i].size; off += chunk, c++) {
            const size_t len = bufs[i].size - off < chunk ? bufs[i].size - off : chunk;
            const size_t nb = QZSTD_byteGroupBlocks(len, k, NULL, 0);
            const unsigned char *src = (const unsigned char *)bufs[i].d_ptr + off, *base = bases && bases[i].d_ptr ? (const unsigned char *)bases[i].d_ptr + off : NULL;
            size_t np = 0;
            if (sm) {
                /* the slices tile the buffer: a frame inside one of them lies at an address like any other frame, one across several has none */
                np = qfSrcFramePieces(sm, &p, off, len);
                src = np == 1u ? sm->pieces[p].src + (off - sm->pieces[p].off) : NULL;
                base = np == 1u && sm->pieces[p].base ? sm->pieces[p].base + (off - sm->pieces[p].off) : NULL;
            }
            if (equal && equal[c]) continue;
            if (!cur || cur->bytes + len > partBytes || cur->nb + nb > maxBlocks) {
                cur = &pt[nParts++];
                cur->f0 = m;
                cur->nb = cur->bytes = 0;
                cur->run = 1;
                cur->grouped = cur->delta = cur->diff = cur->pieces = 0;
            } else if (fr[m - 1].buf != (uint32_t)i || fr[m - 1].off + chunk != off || (sm && (!src || !fr[m - 1].src || fr[m - 1].src + chunk != src))) {
                cur->run = 0;
            }
            if (np > 1u) { cur->pieces = 1; cur->run = 0; }
            if (np > 0xFFFFFFFFu) { free(fr); free(pt); return -1; }
            fr[m].off = off;
            fr[m].len = len;
            fr[m].src = src;
            fr[m].base = base;
            fr[m].p0 = p;
            fr[m].np = (uint32_t)np;
            fr[m].based = bases && bases[i].d_ptr;
            fr[m].b0 = cur->nb;
            fr[m].idx = c;
            fr[m].buf = (uint32_t)i;
            fr[m].nb = (uint32_t)nb;
            fr[m].k = k;
            fr[m].diff = e & QZSTD_ELEM_DIFF;
            if (fr[m].diff) cur->diff = 1;
            if (k > 1u) cur->grouped = 1;
            if (bases && bases[i].d_ptr) cur->delta = 1;
            cur->f1 = ++m;
            cur->nb += nb;
            cur->bytes += len;
        }
    }
    if (c != nFrames) { free(fr); free(pt); return -1; }
    *framesOut = fr;
    *partsOut = pt;
    *nPartsOut = nParts;
    return 0;
}

/* ---- delta skip (QZSTD_frontSetDeltaSkip): chunks equal to their base chunk are found on the GPU before the parts are planned, and the
 * library writes their frames itself */

/* XXH64, seed 0, of len zero bytes: the reference algorithm with every input lane 0 (no buffer of zeros is needed) */
static uint64_t qfRotl64(uint64_t v, unsigned r) { return (v << r) | (v >> (64u - r)); }
static uint64_t qfXxh64Zeros(size_t len)
{
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull,
                   P5 = 0x27D4EB2F165667C5ull;
    size_t n = len;
    uint64_t h = P5;
    if (len >= 32u) {
        uint64_t v[4];
        unsigned i;
        v[0] = P1 + P2; v[1] = P2; v[2] = 0; v[3] = 0ull - P1;
        for (; n >= 32u; n -= 32u)
            for (i = 0; i < 4u; i++) v[i] = qfRotl64(v[i], 31) * P1; /* round(acc, 0) */
        h = qfRotl64(v[0], 1) + qfRotl64(v[1], 7) + qfRotl64(v[2], 12) + qfRotl64(v[3], 18);
        for (i = 0; i < 4u; i++) h = (h ^ (qfRotl64(v[i] * P2, 31) * P1)) * P1 + P4;
    }
    h += (uint64_t)len;
    for (; n >= 8u; n -= 8u) h = qfRotl64(h, 27) * P1 + P4; /* h ^= round(0, 0) = 0 */
    if (n >= 4u) { h = qfRotl64(h, 23) * P2 + P3; n -= 4u; }
    for (; n; n--) h = qfRotl64(h, 11) * P1;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

/* the checksum field of a zero frame: computed once per distinct length while one length follows itself (a buffer's full chunks), and the
 * length of a full chunk is kept apart from the tails' */
typedef struct { size_t len[2]; uint32_t low[2]; } QF_ZeroHash;
static uint32_t qfZeroHash(QF_ZeroHash *z, size_t chunk, size_t len)
{
    const int k = len == chunk ? 0 : 1;
    if (z->len[k] != len) {
        z->low[k] = (uint32_t)qfXxh64Zeros(len);
        z->len[k] = len;
    }
    return z->low[k];
}

/* bytes the canonical zero frame of a chunk of len bytes takes at most (8-byte content size, checksum) */
static size_t qfZeroFrameBound(size_t len) { return 4u + 1u + 8u + 4u * ((len + 131071u) / 131072u) + 4u; }

/* THE CANONICAL ZERO FRAME of a chunk of len > 0 bytes, without its checksum field: magic, a frame header descriptor with Single_Segment and
 * the smallest Frame_Content_Size field that holds len (and Content_Checksum_Flag when `checksum`), RLE_Blocks of the byte 0 cut every
 * 128 KiB from the frame's start, Last_Block on the final one.  -> bytes written (out holds qfZeroFrameBound(len)) */
static size_t qfZeroFrameBody(unsigned char *out, size_t len, int checksum)
{
    size_t pos = qfFrameHeader(out, len, checksum), left = len;
    while (left) {
        const size_t n = left < 131072u ? left : 131072u;
        const unsigned h = (unsigned)(n << 3) | 2u | (left == n ? 1u : 0u); /* Block_Size (the regenerated size), RLE_Block, Last_Block */
        out[pos++] = (unsigned char)h; out[pos++] = (unsigned char)(h >> 8); out[pos++] = (unsigned char)(h >> 16);
        out[pos++] = 0;
        left -= n;
    }
    return pos;
}

/* the whole frame: with `checksum` the low 32 bits of XXH64 of len zero bytes behind the last block */
static size_t qfZeroFrame(unsigned char *out, size_t len, int checksum, QF_ZeroHash *z, size_t chunk)
{
    size_t pos = qfZeroFrameBody(out, len, checksum);
    if (checksum) {
        const uint32_t h = qfZeroHash(z, chunk, len);
        out[pos++] = (unsigned char)h; out[pos++] = (unsigned char)(h >> 8); out[pos++] = (unsigned char)(h >> 16); out[pos++] = (unsigned char)(h >> 24);
    }
    return pos;
}

/* 1 when the frame is byte for byte the canonical zero frame of a chunk of len bytes, with or without the checksum field (the frame's own
 * flag says which); scratch holds qfZeroFrameBound(len) */
static int qfIsZeroFrame(const unsigned char *fr, size_t frSize, size_t len, unsigned char *scratch, QF_ZeroHash *z, size_t chunk)
{
    const int ck = frSize > 4u && (fr[4] & 4u) != 0u;
    size_t body;
    if (frSize < 10u || frSize > qfZeroFrameBound(len)) return 0;
    body = qfZeroFrameBody(scratch, len, ck);
    if (frSize != body + (ck ? 4u : 0u) || memcmp(fr, scratch, body) != 0) return 0;
    if (ck) {
        const uint32_t h = qfZeroHash(z, chunk, len);
        const unsigned char want[4] = { (unsigned char)h, (unsigned char)(h >> 8), (unsigned char)(h >> 16), (unsigned char)(h >> 24) };
        if (memcmp(fr + body, want, 4) != 0) return 0;
    }
    return 1;
}

/* The pre-pass of a delta call with the setting on: ONE qzstd_hip_diff launch on the slot's stream (which already waits for the caller's),
 * the flags back in one copy, a bounded wait.  A frame of a buffer that has a base is compared piece by piece, a row per piece (rows of
 * its own, so that a frame's flags are its own): the pieces of the source map that hold its bytes, or — no map, the buffers are
 * contiguous — ONE piece, bufs[i].d_ptr + off against bases[i].d_ptr + off.  equal[c] (nFrames entries) becomes 1 for a frame none of
 * whose rows differs — its canonical zero frame is written to dst here and its size to frameSizes — and 0 for every other frame, those
 * of buffers without a base included: they are never compared. */
static int qfDiffPass(QZSTD_Front *f, QF_DevSlot *s, int dev, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const QF_SrcMap *sm,
                      size_t nBufs, size_t nFrames, unsigned char *equal, unsigned char *dst, size_t *frameSizes)
{
    const size_t chunk = f->p.chunkSize;
    QF_ZeroHash z;
    size_t i, off, c = 0, rows = 0, frames = 0, r = 0, nEqual = 0, p = 0;
    unsigned long long bytes = 0;
    qzstd_hip_diff_row_t *row;
    const uint32_t *flags;
    memset(equal, 0, nFrames);
    memset(&z, 0, sizeof(z));
    for (i = 0; i < nBufs; i++) {
        if (!bases[i].d_ptr) continue;
        for (off = 0, p = sm ? sm->first[i] : 0; off < bufs[i].size; off += chunk, frames++)
            rows += sm ? qfSrcFramePieces(sm, &p, off, bufs[i].size - off < chunk ? bufs[i].size - off : chunk) : 1u;
    }
    if (rows == 0) return 0;
    if (rows > 0xFFFFFFFFu || chunk > 0xFFFFFFE0u) return -1; /* (a launch's rows and a row's length are 32-bit) */
    if (qfZeroFrameBound(chunk) > f->stride) return -1;
    row = (qzstd_hip_diff_row_t *)qfBufH(&s->pin.diffRows, rows * sizeof(qzstd_hip_diff_row_t));
    flags = (const uint32_t *)qfBufH(&s->pin.diffFlags, rows * sizeof(uint32_t));
    if (!row || !flags || !qfBufD(dev, &s->dev.diffRows, rows * sizeof(qzstd_hip_diff_row_t)) || !qfBufD(dev, &s->dev.diffFlags, rows * sizeof(uint32_t)))
        return -1;
    for (i = 0; i < nBufs; i++) {
        if (!bases[i].d_ptr) continue;
        for (off = 0, p = sm ? sm->first[i] : 0; off < bufs[i].size; off += chunk) {
            const size_t len = bufs[i].size - off < chunk ? bufs[i].size - off : chunk;
            size_t np = sm ? qfSrcFramePieces(sm, &p, off, len) : 1u, k;
            for (k = 0; k < np; k++, row++) {
                size_t lo = off, hi = off + len;
                const unsigned char *a = (const unsigned char *)bufs[i].d_ptr + off, *b = (const unsigned char *)bases[i].d_ptr + off;
                if (sm) {
                    const QF_SrcPiece *q = &sm->pieces[p + k];
                    qfPieceInFrame(q, off, len, &lo, &hi);
                    a = q->src + (lo - q->off);
                    b = q->base + (lo - q->off);
                }
                row->a = (uint64_t)(uintptr_t)a;
                row->b = (uint64_t)(uintptr_t)b;
                row->len = (uint32_t)(hi - lo);
                row->tile0 = 0;
            }
            bytes += len;
        }
    }
    if (qzstd_hip_diff(dev, s->stream, (qzstd_hip_diff_row_t *)s->pin.diffRows.p, (uint32_t)rows, (qzstd_hip_diff_row_t *)s->dev.diffRows.p,
                       (uint32_t *)s->dev.diffFlags.p) ||
        qzstd_hip_memcpy_d2h(dev, s->stream, s->pin.diffFlags.p, s->dev.diffFlags.p, rows * sizeof(uint32_t)))
        return -1;
    if (qzstd_hip_stream_wait(dev, s->stream, QF_DEV_WAIT_MS) != 0) {
        (void)qzstd_hip_stream_sync(dev, s->stream); /* the launch still reads the caller's buffers */
        return -1;
    }
    for (i = 0; i < nBufs; i++) {
        const size_t nf = bufs[i].size / chunk + (bufs[i].size % chunk != 0);
        if (bases[i].d_ptr) {
            for (off = 0, p = sm ? sm->first[i] : 0; off < nf; off++) {
                const size_t len = bufs[i].size - off * chunk < chunk ? bufs[i].size - off * chunk : chunk;
                size_t np = sm ? qfSrcFramePieces(sm, &p, off * chunk, len) : 1u;
                uint32_t any = 0;
                for (; np; np--, r++) any |= flags[r];
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

/* both device entry points.  batch: the call needs the gather (frames of several buffers in one part); the single-buffer call stages a part it
 * cannot read in place with the gather when the device layer has it and with a memset and 2D copies when not.
 * sm: NULL, or (QZSTD_frontCompressDeviceSlices, which has checked the slices and looked their memory up) where the buffers' bytes lie; bufs and
 * bases then hold each buffer's size and the address of its FIRST slice, which is the buffer's own when its slices follow each other in memory */
static size_t qfCompressDevice(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const QF_SrcMap *sm,
                               const unsigned char *elemSizes, size_t nBufs, int batch, void *stream, void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame)
{
    QF_DevJob j;
    QF_Call call;
    QF_DevSlot *slot;
    QF_DevPart part[2];
    QF_DevFrame *frames = NULL;
    QF_DevRange *parts = NULL;
    size_t nFrames, nParts = 0, k, i, total;
    unsigned group;
    unsigned char *equal = NULL;
    int rc = 0, anyGrouped = 0, anyBase = 0, anyDiff = 0, skip, probe, code;
    /* host-side checks: nothing has touched a GPU when one of them fails */
    if (!f || (nBufs && !bufs) || !dst || !frameSizes || !f->p.useProducer || nBufs > 0xFFFFFFFFu) return (size_t)-1;
    for (i = 0; i < nBufs; i++)
        if (!bufs[i].d_ptr && bufs[i].size) return (size_t)-1;
    /* a base is none ({NULL, 0}) or as large as its buffer; a call without any is the call without the argument */
    for (i = 0; bases && i < nBufs; i++) {
        if (!bases[i].d_ptr && !bases[i].size) continue;
        if (!bases[i].d_ptr || bases[i].size != bufs[i].size) return (size_t)-1;
        if (bases[i].size) anyBase = 1;
    }
    if (!anyBase) bases = NULL;
    /* each buffer's element size: its own entry, or (0, or no array) the front's setting */
    group = f->group;
    for (i = 0; i < nBufs; i++) {
        unsigned e = elemSizes && elemSizes[i] ? elemSizes[i] : group;
        if (e & QZSTD_ELEM_DIFF) {
            /* differences: with the buffer's own element size only (0x80 alone is refused), and not against a base */
            if (bases && bases[i].d_ptr) return (size_t)-1;
            anyDiff = 1;
            e &= ~QZSTD_ELEM_DIFF;
        }
        if (e != 1u && e != 2u && e != 4u && e != 8u) return (size_t)-1;
        if (e > 1u) anyGrouped = 1;
    }
    nFrames = QZSTD_frontDeviceBatchFrames(f, bufs, nBufs);
    if (dstCapacity / f->stride < nFrames) return (size_t)-1;
    if (!qzstd_hip_pointer_device || !qzstd_hip_compact || !qzstd_hip_compact_workspace_bytes || !qzstd_hip_event_create ||
        !qzstd_hip_event_record || !qzstd_hip_stream_wait_event || !qzstd_hip_event_destroy || !qzstd_hip_memcpy2d_d2d ||
        (batch && !qzstd_hip_gather))
        return (size_t)-1; /* a device layer without the device-input entry points */
    if (f->checksum && !qzstd_hip_xxh64) return (size_t)-1; /* checksums wanted and a device layer that cannot hash */
    if (anyGrouped && !qzstd_hip_group) return (size_t)-1;  /* byte grouping wanted and a device layer that cannot group */
    if (bases && !qzstd_hip_group_xor) return (size_t)-1;   /* a base given and a device layer that cannot XOR one in */
    if (sm && sm->multi && !qzstd_hip_group_pieces) return (size_t)-1; /* a frame of several pieces and a device layer that cannot assemble one */
    if (anyDiff && !qzstd_hip_group_ediff) return (size_t)-1; /* differences wanted and a device layer that cannot take them */
    skip = bases && f->deltaSkip;
    if (skip && !qzstd_hip_diff) return (size_t)-1;         /* delta skip wanted and a device layer that cannot compare */
    code = f->planeCode && (anyGrouped || bases);
    if (code && (!qzstd_hip_huf_code || !qzstd_hip_huf_code_bytes)) return (size_t)-1; /* plane code wanted and a device layer without the coder */
    probe = code || (f->planeProbe && (anyGrouped || bases));
    if (probe && !code && !qzstd_hip_plane_cost) return (size_t)-1;  /* plane probe wanted and a device layer that cannot take histograms */
    call.f = f;
    call.restore = 0;
    call.nStreams = 2;
    call.dev = sm ? sm->dev : -1; /* (a call with source slices has looked its memory up: qfSrcMapBuild) */
    if (!sm && qfCallBufs(&call, bufs, bases, nBufs)) return (size_t)-1;
    /* a call without a frame takes nothing, not even devBusy: it succeeds while another call is in progress */
    if (nFrames == 0) {
        qfFirstFrames(f, bufs, nBufs, firstFrame);
        return 0;
    }
    if (qfCallBegin(&call, stream)) return (size_t)-1; /* (firstFrame is not written by a call that is refused) */
    qfFirstFrames(f, bufs, nBufs, firstFrame);
    pthread_once(&qfSeqOnce, qfResolveSeqApi);
    for (i = 0, total = 0; i < nBufs; i++) total += bufs[i].size;

    j.f = f;
    j.sm = sm;
    j.dev = call.dev;
    j.checksum = f->checksum; /* (fixed for the call: devBusy keeps QZSTD_frontSetChecksum out) */
    j.probe = probe;
    j.code = code;
    j.failSub = probe && getenv("QZSTD_FRONT_PROBE_FAIL_SUB") != NULL;
    j.blk = f->p.chunkSize < QZSTD_HIP_BLOCK_MAX ? f->p.chunkSize : QZSTD_HIP_BLOCK_MAX;
    {
        const char *rep = getenv("QZSTD_HIP_EXT_REPCODES"); /* the producer path's level flags (QZSTD_startQatDevice) */
        j.level = f->p.level | ((rep && atoi(rep) > 0) ? QZSTD_HIP_LEVEL_REPCODES : 0);
    }
    memset(part, 0, sizeof(part));
    slot = f->devSlot;
    /* delta skip: the chunks equal to their base chunk are found first and get their zero frames; the parts are planned without them */
    if (skip) {
        if (!(equal = (unsigned char *)malloc(nFrames))) rc = -1;
        else rc = qfDiffPass(f, &slot[0], j.dev, bufs, bases, sm, nBufs, nFrames, equal, (unsigned char *)dst, frameSizes);
    }
    if (rc == 0) rc = qfPlanDevice(f, bufs, bases, sm, elemSizes, group, nBufs, equal, nFrames, qfPartBytes(), j.blk, &frames, &parts, &nParts);
    j.frames = frames;
    j.parts = parts;
    j.nParts = nParts;
    /* two parts on the GPU ahead of the one being entropy-coded: part p lives on slot p % 2 from its queueing to its fetch (no part at all
     * when every frame of the call was equal to its base: nothing is staged, matched, copied or handed to the workers) */
    for (k = 0; k < 2 && k < nParts && rc == 0; k++) rc = qfQueuePart(&j, &slot[k], &parts[k]);
    if (rc == 0 && nParts) rc = qfFetchPart(&j, &slot[0], &parts[0], &part[0]);
    for (k = 0; k < nParts && rc == 0; k++) {
        int failed;
        /* slot k % 2 is fetched: its device side takes part k + 2 while the workers read its pinned arena — not the device buffers */
        if (k + 2 < nParts) {
            if ((rc = qfQueuePart(&j, &slot[k % 2], &parts[k + 2])) != 0) break;
        }
        pthread_mutex_lock(&f->mu);
        f->part = &part[k % 2];
        f->src = NULL;
        f->srcSize = 0;
        f->dst = (unsigned char *)dst;
        f->sizes = frameSizes;
        failed = qfRunJobLocked(f, part[k % 2].f1 - part[k % 2].f0);
        f->part = NULL;
        pthread_mutex_unlock(&f->mu);
        if (failed) { rc = -1; break; }
        if (k + 1 < nParts) {
            /* the next part's arena into the other slot (its last reader was the job of part k - 1) */
            rc = qfFetchPart(&j, &slot[(k + 1) % 2], &parts[k + 1], &part[(k + 1) % 2]);
        }
    }
    if (qfCallWait(&call)) rc = -1;
    free(frames);
    free(parts);
    free(equal);
    if (rc == 0) __atomic_fetch_add(&f->devStats[3], (unsigned long long)total, __ATOMIC_RELAXED);
    qfCallEnd(&call);
    return rc == 0 ? nFrames : (size_t)-1;
}

size_t QZSTD_frontCompressDevice(QZSTD_Front *f, const void *d_src, size_t srcSize, void *stream, void *dst, size_t dstCapacity,
                                 size_t *frameSizes)
{
    QZSTD_DeviceBuf one;
    one.d_ptr = d_src;
    one.size = srcSize;
    return qfCompressDevice(f, &one, NULL, NULL, NULL, 1, 0, stream, dst, dstCapacity, frameSizes, NULL);
}

size_t QZSTD_frontCompressDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream, void *dst, size_t dstCapacity,
                                      size_t *frameSizes, size_t *firstFrame)
{
    return qfCompressDevice(f, bufs, NULL, NULL, NULL, nBufs, 1, stream, dst, dstCapacity, frameSizes, firstFrame);
}

size_t QZSTD_frontCompressDeviceBatchTyped(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const unsigned char *elemSizes, size_t nBufs, void *stream,
                                           void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame)
{
    return qfCompressDevice(f, bufs, NULL, NULL, elemSizes, nBufs, 1, stream, dst, dstCapacity, frameSizes, firstFrame);
}

size_t QZSTD_frontCompressDeviceBatchDelta(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes,
                                           size_t nBufs, void *stream, void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame)
{
    return qfCompressDevice(f, bufs, bases, NULL, elemSizes, nBufs, 1, stream, dst, dstCapacity, frameSizes, firstFrame);
}

/* a setting changes only while no device call and no job is in progress; -> 0, or -1: busy */
static int qfSetIdle(QZSTD_Front *f, int *field, int value)
{
    int busy;
    pthread_mutex_lock(&f->mu);
    busy = f->devBusy || f->running;
    if (!busy) *field = value;
    pthread_mutex_unlock(&f->mu);
    return busy ? -1 : 0;
}

void QZSTD_frontDeviceStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->devStats : NULL, stats, 4); }

int QZSTD_frontSetChecksum(QZSTD_Front *f, int on) { return f ? qfSetIdle(f, &f->checksum, on != 0) : -1; }

int QZSTD_frontGetChecksum(const QZSTD_Front *f) { return f ? f->checksum : 0; }

void QZSTD_frontChecksumStats(QZSTD_Front *f, unsigned long long stats[2]) { qfStats(f ? f->cksumStats : NULL, stats, 2); }

int QZSTD_frontSetByteGroup(QZSTD_Front *f, unsigned elemSize)
{
    if (!f || (elemSize != 1u && elemSize != 2u && elemSize != 4u && elemSize != 8u)) return -1;
    return qfSetIdle(f, (int *)&f->group, (int)elemSize); /* (the one setting that is unsigned) */
}

unsigned QZSTD_frontGetByteGroup(const QZSTD_Front *f) { return f ? f->group : 1u; }

void QZSTD_frontByteGroupStats(QZSTD_Front *f, unsigned long long stats[3]) { qfStats(f ? f->groupStats : NULL, stats, 3); }

void QZSTD_frontDeltaStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->deltaStats : NULL, stats, 4); }

void QZSTD_frontElemDiffStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->ediffStats : NULL, stats, 4); }

int QZSTD_frontSetDeltaSkip(QZSTD_Front *f, int on) { return f ? qfSetIdle(f, &f->deltaSkip, on != 0) : -1; }

int QZSTD_frontGetDeltaSkip(const QZSTD_Front *f) { return f ? f->deltaSkip : 0; }

void QZSTD_frontDeltaSkipStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->skipStats : NULL, stats, 4); }

int QZSTD_frontSetPlaneProbe(QZSTD_Front *f, int on) { return f ? qfSetIdle(f, &f->planeProbe, on != 0) : -1; }

int QZSTD_frontGetPlaneProbe(const QZSTD_Front *f) { return f ? f->planeProbe : 0; }

void QZSTD_frontPlaneProbeStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->probeStats : NULL, stats, 4); }

int QZSTD_frontSetPlaneCode(QZSTD_Front *f, int on) { return f ? qfSetIdle(f, &f->planeCode, on != 0) : -1; }

int QZSTD_frontGetPlaneCode(const QZSTD_Front *f) { return f ? f->planeCode : 0; }

void QZSTD_frontPlaneCodeStats(QZSTD_Front *f, unsigned long long stats[4]) { qfStats(f ? f->codeStats : NULL, stats, 4); }

/* include/qzstd_hufblock.h as exported functions (bindings that cannot include the header): the block body (0: none) of `len` bytes from the
 * 128 bytes of code lengths and the jump table + streams that qzstd_hip_huf_code leaves, and the rule */
size_t QZSTD_hufBlockBodyOf(const unsigned char lengths[128], unsigned len, const unsigned char *streams, size_t streamBytes, unsigned char *dst,
                            size_t cap)
{
    uint8_t nbits[256];
    QZSTD_hufUnpackLengths(lengths, nbits);
    return QZSTD_hufBlockBody(nbits, len, streams, streamBytes, dst, cap);
}
int QZSTD_hufTakesOf(unsigned streamBytes, unsigned bodyBytes, unsigned len, unsigned litBytes, unsigned count)
{
    return QZSTD_hufTakes(streamBytes, bodyBytes, len, litBytes, count);
}

unsigned QZSTD_planeCostOf(const unsigned hist[256], unsigned len) { return len <= QZSTD_PLANE_LEN_MAX ? QZSTD_planeCost(hist, len) : len; }
int QZSTD_planeIsRawOf(unsigned cost, unsigned len, unsigned matchedBytes) { return QZSTD_planeIsRaw(cost, len, matchedBytes); }

/* The byte-grouped layout, its block rule and qzbgRebuild: a source of their own, free of HIP and libzstd (the tests build it alone), and
 * part of this translation unit so that the front-end stays ONE source to whoever builds it. */
#include "qzstd_bytegroup.c"

/* The restore calls: a source of their own that uses this file's types and helpers, and part of this translation unit for the same reason. */
#include "qzstd_restore.c"

/* The verify call: the restore's slots and decode with a comparison in the scatter's place; included the same way. */
#include "qzstd_verify.c"

/* The fingerprint calls: one launch over the caller's own buffers, on the restore's first slot; included the same way. */
#include "qzstd_fingerprint.c"

/* Element differences and their sum (include/qzstd_elemdiff.h): free of HIP and libzstd like the byte-grouped layout; included the same way. */
#include "qzstd_elemdiff.c"

/* The adviser: are element differences worth it for a buffer, from plane costs taken on the GPU; on the restore's first slot like the
 * fingerprint calls; included the same way. */
#include "qzstd_advise.c"

/* The compress call whose buffers are lists of source slices: its checks, the staging from pieces and the places that read a frame's bytes
 * piece by piece; included the same way. */
#include "qzstd_srcslices.c"

/* The fingerprint, check and verify calls whose buffers are lists of source slices: the same checks, and the bodies of qzstd_fingerprint.c
 * and qzstd_verify.c with the piece map; included the same way. */
#include "qzstd_slicecheck.c"
