/*
 * qatseqprod.c — host side of the MI355X-native sequence producer, plain C.
 *
 * Mirrors the operator interface of intel/QAT-ZSTD-Plugin for its hot path
 * (/root/reference/src/qatseqprod.c) — same entry points, same guards, same error
 * behaviour — over the thin HIP C ABI of include/qzstd_hip.h:
 *
 *   reference                                      here
 *   ---------------------------------------------  -----------------------------------------
 *   QZSTD_startQatDevice   :948-964                runtime probe + slot table, under a mutex
 *   instance discovery + round-robin shuffle       slots interleaved across GPUs so that
 *     :529-663                                       consecutive slots sit on different devices;
 *                                                    an announced buffer is split across the GPUs
 *   QZSTD_grabInstance / releaseInstance :905-933  test-and-set sweep starting at the hint (hint path,
 *                                                    QZSTD_HIP_COALESCE=0); by default callers are
 *                                                    merged into batches, several in flight per GPU
 *   QZSTD_allocInstMem (lazy)  :685-822            pinned + device buffers, created on first use
 *   input staging memcpy       :1222-1227          memcpy into the pinned staging buffer
 *   cpaDcCompressData2 + poll  :1243-1272          H2D, kernel launch on a stream, bounded wait
 *   poll time-out              :1099-1104,:1261-72 QZSTD_HIP_TIMEOUT_MS (default 2000): error -> libzstd's
 *                                                    fallback; the stream is quarantined until it drains
 *   QZSTD_decLz4s              :1013-1091          (none: the kernel emits ZSTD_Sequence)
 *   result / capacity checks   :1293-1322          count == NSEQ_ERROR or >= cap-1 -> ERROR
 *   device-down counter, retry every 1000 blocks   same (failOffloadCnt)
 *     :88, :1140-1152
 *
 * No QAT / icp_sal / cpa symbol is used or emulated.
 *
 * Sections, each using only what stands above it: types, helpers, take / join, slots, coalescer, service, announcement batcher,
 * announcements, lifecycle, producer (guards -> serve from an announcement -> service -> coalescer -> slot).
 */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE /* SYS_getcpu, sched_getaffinity */
#endif
#include "qatseqprod.h"
#include "qzstd_hip.h"

#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <emmintrin.h>
#include <sys/prctl.h>
#include <sys/syscall.h>
#include <sys/types.h>
#include <time.h>
#include <unistd.h>

#ifndef DEBUGLEVEL
#define DEBUGLEVEL 0
#endif

#define QZ_LEVEL_MIN 1
#define QZ_LEVEL_MAX 12
#define QZ_RETRY_INTERVAL_BLOCKS 1000 /* re-probe a dead device every N failed blocks */
#define QZ_GRAB_SWEEPS 40000 /* 64 yields, then 50 us naps: about two seconds */
#define QZ_MAX_DEVICES 64
#define QZ_MAX_SLOTS 1024
#define QZ_DEFAULT_SLOTS_PER_DEVICE 128
#define QZ_FIRST_COPY_SEQS 16384u /* sequences fetched together with the count */
#define QZ_DEFAULT_TIMEOUT_MS 2000 /* reference: 2 s of polling, src/qatseqprod.c:1099-1104 */

static int qzLogLevel = DEBUGLEVEL; /* 0 silent, 1 errors, 2 events, 3 every sequence */

/* Why a callback returned ZSTD_SEQUENCE_PRODUCER_ERROR (counted per state, QZSTD_failStats; the reference counts only
 * the device-down case: failOffloadCnt, src/qatseqprod.c:122,:1141).  The failing site names the cause in a thread-local;
 * a batch's leader leaves it in the request for the member that waits. */
enum { QZ_CAUSE_NONE = 0, QZ_CAUSE_GUARD, QZ_CAUSE_DEVICE_DOWN, QZ_CAUSE_TIMEOUT, QZ_CAUSE_CAPACITY, QZ_CAUSE_RUNTIME, QZ_CAUSE_N };
static __thread int qzCause = QZ_CAUSE_NONE;
#define QZ_LOG(l, ...)                                       \
    do {                                                     \
        if ((l) <= qzLogLevel) {                             \
            fprintf(stderr, "qatseqprod(hip): " __VA_ARGS__); \
        }                                                    \
    } while (0)

/* One slot = one stream with its staging and device buffers on one GPU (the analogue of a QAT DC instance). */
typedef struct {
    int device;
    volatile int lock;
    int ready; /* buffers + stream exist */
    int stuck; /* a wait on the stream timed out: not reusable until the stream drains */
    void *stream;
    unsigned char *hSrc; /* pinned staging, QZSTD_HIP_BLOCK_MAX + pad */
    unsigned char *dSrc;
    ZSTD_Sequence *hSeqs; /* pinned, seqCap entries */
    ZSTD_Sequence *dSeqs;
    qzstd_hip_block_t *hDesc; /* pinned */
    qzstd_hip_block_t *dDesc;
    unsigned int *hCount; /* pinned */
    unsigned int *dCount;
    size_t seqCap;
    /* launch scratch (hash chains of levels >= 5), grow-only */
    void *dWork; size_t dWorkCap;
    /* buffers of the resident service's requests (qzstd_hip_service_submit), created on first use: the staged block, its
     * device twin, QZ_SVC_ITEMS_MAX result regions and count words — the words are what the caller polls */
    unsigned char *vSrc;   /* pinned */
    unsigned char *vdSrc;  /* device */
    ZSTD_Sequence *vSeqs;  /* pinned, QZ_SVC_ITEMS_MAX x QZ_SVC_ITEM_CAP */
    unsigned int *vCount;  /* pinned, QZ_SVC_ITEMS_MAX */
    void *vdWork;          /* device: chain scratch of a request (levels >= 5: shared by its items), QZSTD_HIP_SVC_WORK_BYTES, on first use */
    unsigned int vEpoch, vItems; /* the last request: its epoch, its item count */
    int vStuck;            /* that request timed out: the slot serves no request before all its count words have arrived */
} QZSTD_Slot_T;
#define QZ_SVC_ITEMS_MAX QZSTD_HIP_SVC_MAX_ITEMS
#define QZ_SVC_ITEM_CAP ((size_t)1371) /* ZSTD_sequenceBound(4096): the smallest item is one 4 KiB segment; 32 of them hold any block's worst case */
#define QZ_NOT_SERVED ((size_t)-2)     /* qzServiceBlock: the resident service does not take this request, use the launch path */

/*
 * Cross-thread request coalescing (one per GPU).  The producer API hands over ONE block per call and waits, and a
 * single block keeps one of 256 CUs busy; many callers (one CCtx per thread, the reference's own scaling model:
 * README.md:138, many DC instances per device: src/qatseqprod.c:905-928) are therefore merged into batches.  A GPU has
 * QZ_BATCHES batches, each with its own stream and staging, so several launches are in flight at once: a caller that
 * finds no batch collecting opens an idle one and leads it — it stages its block, closes the batch and launches, so a
 * lone caller never waits for anybody; callers that arrive while a leader is staging join its batch; when every batch
 * is busy, newcomers wait for the first one to come back and then pile into it together ("group commit": no timers).
 * Every caller copies its own block into the batch's pinned staging area and its own result out of it, so those
 * copies run in parallel on the callers' threads.  Levels may be mixed: one launch per level present in a batch.
 */
#define QZ_BATCH_MAX 128
#define QZ_BATCHES 4
#define QZ_BATCH_PITCH ((size_t)16384) /* sequences per block in the batch's result area; denser blocks are redone alone */
#define QZ_SEGS_MAX 32 /* a batched block goes to the GPU as up to 32 work items, each a run of whole segments (profile.segLog): as many
                        * as keep the launch within one workgroup per CU — 32 per block while at most 8 callers share a batch, 8 up to 32
                        * callers, whole blocks beyond */
#define QZ_DESC_MAX (QZ_BATCH_MAX + QZ_SPLIT_ITEMS_MAX) /* descriptors of a batch: unsplit, or split within QZ_SPLIT_ITEMS_MAX */
#define QZ_SPLIT_ITEMS_MAX 256 /* batches are only cut into segment items while the launch stays within one workgroup per CU */
typedef struct {
    const void *src;
    size_t srcSize, cap, rc;
    int level;
    int nSeg, dense;                /* segments submitted; the batch's result area was too small: redo alone */
    int cause;                      /* QZ_CAUSE_* when rc is the error code (set by the batch's leader) */
    unsigned int segPitch;          /* result entries per segment: QZ_BATCH_PITCH / nSeg */
    unsigned int segCnt[QZ_SEGS_MAX]; /* sequences per segment, each including its delimiter */
} QZSTD_Req_T;

typedef struct {
    int state; /* 0 idle or collecting, 1 closed (running), 2 done (results being copied out) */
    int n, copied, consumed;
    int ready, stuck;
    QZSTD_Req_T req[QZ_BATCH_MAX];
    unsigned char *hSrc;      /* pinned, QZ_BATCH_MAX x QZ_SRC_STRIDE */
    unsigned char *dSrc;      /* device, same size */
    ZSTD_Sequence *hSeqs;     /* pinned, QZ_BATCH_MAX x QZ_BATCH_PITCH */
    qzstd_hip_block_t *hDesc; /* pinned, QZ_BATCH_MAX x QZ_SEGS_MAX */
    unsigned int *hCount;     /* pinned, QZ_BATCH_MAX x QZ_SEGS_MAX */
    void *dvSeqs, *dvDesc, *dvCount; /* device-side addresses of hSeqs / hDesc / hCount */
    void *stream;
    void *dWork; /* launch scratch, grow-only */
    size_t dWorkCap;
    pthread_cond_t cvLead;    /* the batch's leader (its first member) waits here for the members to finish staging */
    pthread_cond_t cvDone;    /* the other members wait here for the results */
} QZSTD_Batch_T;

typedef struct {
    int device;
    int open; /* index of the batch that is collecting, -1 = none */
    pthread_mutex_t mu;
    pthread_cond_t cvOpen; /* callers that found every batch busy wait here */
    QZSTD_Batch_T batch[QZ_BATCHES];
    unsigned long launches, blocks, batches;
} QZSTD_Coalescer_T;
#define QZ_SRC_STRIDE ((size_t)QZSTD_HIP_BLOCK_MAX + 64)
#define QZ_NUMA_NODES_MAX 16

typedef struct {
    int status; /* QZSTD_Status_e */
    int numDevices;
    int numSlots;
    QZSTD_Slot_T *slots;
    QZSTD_Coalescer_T *coal; /* one per device */
    int coalesce;            /* QZSTD_HIP_COALESCE (default 1) */
    int levelFlags;          /* QZSTD_HIP_LEVEL_REPCODES when QZSTD_HIP_EXT_REPCODES=1 */
    int timeoutMs;           /* QZSTD_HIP_TIMEOUT_MS */
    int split;               /* QZSTD_HIP_SPLIT: announced buffers are split across this many GPUs (default: all) */
    int splitBlocks;         /* QZSTD_HIP_SPLIT_BLOCKS (default 1): per-block requests of segmentable levels go as segments */
    int service;             /* QZSTD_HIP_SERVICE (default 1): per-block requests go to the resident service where it serves the level */
    int svcItemBytes;        /* QZSTD_HIP_SERVICE_ITEM (default 4096): bytes per work item of a service request (whole segments) */
    int svcSpinUs;           /* QZSTD_HIP_SERVICE_SPIN_US (default 400; 10 when there are more states than usable cores): busy polling of the count words before napping */
    unsigned long devBlocks[QZ_MAX_DEVICES][3]; /* per GPU: blocks queued from announcements, blocks through batches, blocks through the service */
    pthread_mutex_t mutex;
    /* NUMA (reference: qaeMemAllocNUMA(size, node, 64) for every DMA buffer, src/qatseqprod.c:216-246): the host node every GPU hangs
     * off, so that a slot's / batch's / announcement's pinned memory sits next to its GPU and a state lands on a GPU of the socket
     * its thread runs on */
    int numa;                      /* QZSTD_HIP_NUMA (default 1) */
    int numaThreadNode;            /* QZSTD_HIP_NUMA_NODE: treat every calling thread as running on this node (-1: ask the kernel) */
    int devNode[QZ_MAX_DEVICES];   /* -1 = unknown */
    unsigned int nodeNext[QZ_NUMA_NODES_MAX], anyNext; /* round-robin counters: per node, and the fallback over all GPUs */
    int svcSpinSet;                /* QZSTD_HIP_SERVICE_SPIN_US was given: no adapting */
    int liveStates;                /* producer states alive (one per CCtx, i.e. per calling thread): more of them than usable cores = the callers
                                    * oversubscribe the cores, and a caller that waits for the GPU should give its core away at once */
    struct QZSTD_Batcher_S *hb;    /* announcement batchers, one per device */
    int hintBatches;               /* QZSTD_HIP_HINT_BATCHES (default 4): batch streams per device, i.e. announcement launches in flight */
    unsigned int gen;              /* device layer generation: parts of an earlier start refer to nothing */
    int hintCompact;               /* QZSTD_HIP_HINT_COMPACT (default 1): announcements' result entries are packed — 8 bytes with a 12-bit tag */
    int stageNt;                   /* QZSTD_HIP_STAGE_NT (default 1): announcements are staged with streaming stores (qzStageCopy) */
    int hintDirect;                /* QZSTD_HIP_HINT_DIRECT: 0 (default) a batch's staging copy goes to device memory by a copy kernel on the
                                    * launch's stream; 1 the match-finder reads the pinned staging copy itself; 2 that at the levels without
                                    * chains only; 3 the copy by hipMemcpyAsync (rounds 1-3).  Batch front-end, 16 threads, 2 MiB claims, GB/s
                                    * (one launch per claim, 16 hardware queues): level 1 21.4 / 18.5 / 18.5 / 12-14, level 3 18.6 / 15.7 (the
                                    * kernel takes 0.72 ms per launch out of device memory, 0.96 ms over the bus; hipMemcpyAsync holds the caller
                                    * 0.8-1.1 ms per 4 MiB) */
} QZSTD_Process_T;

static QZSTD_Process_T gProc = { .status = QZSTD_FAIL, .coalesce = 1, .timeoutMs = QZ_DEFAULT_TIMEOUT_MS, .splitBlocks = 1, .service = 1,
                                 .svcItemBytes = 4096, .svcSpinUs = 400, .mutex = PTHREAD_MUTEX_INITIALIZER, .numa = 1, .numaThreadNode = -1,
                                 .hintBatches = 4 };

/* One announced buffer: its blocks are staged into the batch areas of the announcement batcher (below) — split into contiguous
 * block ranges, one per GPU — and match-found there; a callback is served from the area its block went to. */
#define QZ_HINT_MAX_BYTES ((size_t)16 << 20)
#define QZ_HINT_PITCH ((size_t)16384) /* blocks with more sequences take the per-block path */
#define QZ_HINT_PARTS 16 /* block ranges of an announcement: one per GPU, more where a range does not fit one batch area */
#define QZ_COUNT_PENDING 0xFFFFFFFDu /* an announced block's count word until its workgroup publishes it */
#define QZ_HINTS 4 /* announcements a state keeps: a ring (QZSTD_hintSource) */
#define QZ_CONTENT_LOOKUP_BLOCKS 256u /* announcements with more grid blocks are matched by address only */
typedef struct {
    int st;   /* 0 none, 1 in a batch (issued or not), 2 ready, 3 failed */
    int dev, area;       /* the batch area of device dev that holds its blocks */
    unsigned int first;  /* index of block b0 in that area */
    unsigned int gen;    /* gProc.gen when it was staged */
    size_t b0, b1; /* block range [b0, b1) of the announcement */
    size_t seen;   /* every block below this one has published its count */
} QZSTD_Part_T;

typedef struct {
    int st;   /* 0 empty, 1 announced (parts in flight or ready) */
    int touched; /* a callback was served from it */
    int stable;  /* QZSTD_HINT_STABLE: the announcer holds the bytes still until their callbacks have come (no memcmp per callback) */
    unsigned int seq;   /* the state's announcement number (QZSTD_Session_T.hintSeq): callbacks look at the newest announcement first */
    size_t servedUpTo;  /* grid blocks below this one have been served: a STABLE announcement serves every block once, going forward */
    unsigned misses; /* callbacks that found nothing to serve since the announcement was last used */
    int nParts;
    QZSTD_Part_T part[QZ_HINT_PARTS];
    const unsigned char *base;
    size_t size, block, nb;
    int level;
    size_t pitch;             /* result entries per block: min(QZ_HINT_PITCH, ZSTD_sequenceBound(block)) */
    unsigned long long *keys; /* per grid block: size + first / last 8 bytes folded (content look-up for streaming callers) */
    size_t keysCap;
    int noAddr; /* a newer announcement names (some of) these addresses: this one no longer serves by address, only by verified content */
} QZSTD_Hint_T;

/*
 * Announcement batcher (one per GPU): the "group commit" of the coalescer above, applied to announcements.  Announced block ranges of
 * every state of the process go into a few large launches instead of one launch per announcement: launches of different streams that
 * the runtime folds onto one hardware queue run one after the other, so with one launch per 2 MiB claim the GPU held as many claims as
 * there were hardware queues (4 by default: 64 of 512 workgroup slots at level 1).
 *
 * A batch AREA is pinned host memory for up to QZ_HB_BLOCKS blocks: their staged bytes, descriptors, count words and result entries.
 * An announcer reserves room in the OPEN area, stages its bytes and descriptors there itself, and the last one to finish staging issues
 * the area when one of the batcher's QZSTD_HIP_HINT_BATCHES streams is free (its last launch has published every count word): one
 * copy-in of the area's bytes and one launch of its blocks.  While every stream is busy the open area keeps collecting; it is issued
 * by the next announcer or callback that finds a stream free — or, when it is full, holds another level or grid, or a callback or a
 * drop needs one of its blocks, at once, behind the previous launch of a stream.  No timers, no host thread of its own.
 * An area is reused when every part in it has been consumed, dropped or failed; its entries carry a 12-bit tag (24 bits unpacked)
 * that changes with every use, and the area is wiped when the tag starts over.  A wait that times out fails every part of the area;
 * its buffers are parked (QZSTD_Orphan_T) when the last part lets go, its stream is quarantined until it drains.
 */
#define QZ_HB_STREAMS_MAX 32
#define QZ_HB_AREAS 256                                 /* areas per GPU, given buffers on first use (32 MiB of pinned memory each): an area
                                                         * lives until the slowest claim in it is consumed — about 2.4 per announcing thread at
                                                         * level 1 (41 for 17 threads); past the last one a range takes the per-block path */
#define QZ_HB_BLOCKS 256u                               /* blocks per area, i.e. per launch at most (grids finer than 32 KiB) */
#define QZ_HB_SRC_BYTES ((size_t)16 << 20)              /* staged bytes per area: 128 blocks of 128 KiB.  An area fills up when every stream is
                                                         * busy and then goes behind a busy one: 64 blocks per area held 3 hardware queues to
                                                         * 70 workgroups in flight and 17.8 GB/s at level 1 */
#define QZ_HB_ENTRIES ((size_t)128 * QZ_HINT_PITCH)     /* result entries per area: 128 blocks at the widest pitch */
enum { QZ_AREA_FREE = 0, QZ_AREA_OPEN, QZ_AREA_ISSUING, QZ_AREA_ISSUED };
typedef struct {
    int st;
    int level;          /* the level (with flags) and the grid of every block in it: one launch, one profile */
    size_t block;
    unsigned int nBlocks, seen; /* descriptors in use; every block below `seen` has published its count */
    size_t srcUsed, entUsed;    /* staged bytes, result entries reserved */
    int staging;        /* announcers still copying into it */
    int parts;          /* parts that still refer to it */
    int stream;         /* the batch stream it was issued on */
    int stuck;          /* a wait for it timed out */
    int wipe;           /* its tag started over: the opener wipes its result area (qzAreaOpen) */
    int sealed;         /* full, or a range of another level or grid came: it takes no more parts, and goes out as soon as its staging is done */
    unsigned int lap;   /* the tag of its entries */
    unsigned char *hSrc;      /* pinned, QZ_HB_SRC_BYTES */
    qzstd_hip_block_t *hDesc; /* pinned, QZ_HB_BLOCKS */
    unsigned int *hCount;     /* pinned, coherent, QZ_HB_BLOCKS */
    void *hSeqs;              /* pinned, coherent, QZ_HB_ENTRIES packed (8-byte) or sixteen-byte entries */
    size_t seqsCap;           /* bytes */
    void *dvSrc, *dvDesc, *dvCount, *dvSeqs; /* their device-side addresses */
} QZSTD_Area_T;

typedef struct {
    void *stream;
    unsigned char *dSrc;      /* device, QZ_HB_SRC_BYTES: the copy-in's destination */
    void *dWork; size_t dWorkCap; /* launch scratch (levels >= 5), grow-only */
    int last;                 /* area issued last on it, -1 none */
    int issuing;              /* a thread is queueing a launch on it */
    int stuck;                /* a wait timed out: not used before it has drained */
} QZSTD_BStream_T;

typedef struct QZSTD_Batcher_S {
    int device;
    pthread_mutex_t mu;
    pthread_cond_t cv;        /* an area's staging or a stream's issue has finished */
    int open;                 /* the area taking parts, -1 none */
    int pending;              /* the open area holds blocks (read without the lock by callbacks) */
    int nextStream;
    QZSTD_BStream_T str[QZ_HB_STREAMS_MAX];
    QZSTD_Area_T area[QZ_HB_AREAS];
    unsigned long launches, blocks, areas; /* event log / test hook: launches, blocks launched, areas given buffers */
} QZSTD_Batcher_T;

/* Pinned buffers of a batch area that a timed-out kernel may still read (hSrc, hDesc) and write (hSeqs, hCount): the area gets fresh
 * ones, these are parked here — never reused, scrubbed or freed — until the stream it ran on has drained (round-2 ADVICE: a late
 * kernel must not write into the next announcement's results). */
typedef struct QZSTD_Orphan_S {
    struct QZSTD_Orphan_S *next;
    void *buf[4];
    size_t srcCap;
    int device;
    void *stream;
} QZSTD_Orphan_T;
static QZSTD_Orphan_T *qzOrphans;
static unsigned long qzOrphanCount; /* test hook / log: areas whose buffers were parked */
static pthread_mutex_t qzOrphanMu = PTHREAD_MUTEX_INITIALIZER;

/* Per-CCtx state (opaque to the caller). */
typedef struct {
    int slotHint;
    unsigned int failOffloadCnt;
    /* announced batches served to later callbacks (QZSTD_hintSource): so that the GPU can
     * work on the next buffer while libzstd entropy-codes the current one on this thread */
    QZSTD_Hint_T hint[QZ_HINTS]; /* announced by the caller, a ring of four */
    int hintNext;                /* the ring slot the next announcement tries first */
    unsigned int hintSeq;        /* announcements made so far: every one gets the next number (the look-up goes newest first) */
    unsigned int stableSampler;  /* blocks looked up in STABLE announcements: every 16th is compared with the staged copy all the same */
    unsigned long stableBroken;  /* ... and differed (QZSTD_hintBroken) */
    unsigned long servedFromBatch, servedSync, servedService;
    unsigned long fail[QZ_CAUSE_N]; /* callbacks that returned the error code, by cause ([0] = all of them) */
    unsigned long redoneAlone;      /* blocks too dense for a batch's result area, redone on a slot of their own (not errors) */
    unsigned long hintCalls, hintStageNs, hintWaitNs, hintCopyCallNs, hintLaunchCallNs, hintPrepNs, hintDropNs; /* event log only */
} QZSTD_Session_T;

#define QZ_HINT_STALE_MISSES 16u /* an announcement that was used and then missed this often is dropped */

/* ---------------------------------------------------------------- helpers -------- */

/* cheap fingerprint of a block: its size and its first and last 8 bytes (a candidate is always verified with memcmp) */
static unsigned long long qzBlockKey(const unsigned char *p, size_t n)
{
    unsigned long long a, b;
    memcpy(&a, p, 8);
    memcpy(&b, p + n - 8, 8);
    return a ^ (b * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)n << 40);
}

const char *QZSTD_version(void)
{
    return QZSTD_VERSION;
}

static unsigned long qzNowNs(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (unsigned long)ts.tv_sec * 1000000000ul + (unsigned long)ts.tv_nsec;
}

static int qzEnvInt(const char *name, int dflt, int lo, int hi)
{
    const char *v = getenv(name);
    long x;
    if (!v || !*v) return dflt;
    x = strtol(v, NULL, 10);
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return (int)x;
}

/* the cores this process may use: its affinity mask, capped by a cgroup CPU quota (cpu.max) */
static int qzUsableCores(void)
{
    static int cached; /* written once with the same value by whoever gets here first (QZSTD_startQatDevice does, under the process mutex) */
    int n = 0;
    cpu_set_t set;
    FILE *f;
    if ((n = __atomic_load_n(&cached, __ATOMIC_RELAXED)) != 0) return n;
    n = 0;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)sysconf(_SC_NPROCESSORS_ONLN);
    f = fopen("/sys/fs/cgroup/cpu.max", "re");
    if (f) {
        char q[32] = "";
        long per = 0;
        if (fscanf(f, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
            const long quota = (atol(q) + per - 1) / per;
            if (quota > 0 && quota < n) n = (int)quota;
        }
        fclose(f);
    }
    n = n > 0 ? n : 1;
    __atomic_store_n(&cached, n, __ATOMIC_RELAXED);
    return n;
}

/* Bounded wait for a stream (reference: the polling loop with its 2 s limit, src/qatseqprod.c:1261-1285).
 * 0 = everything queued on the stream is done, 1 = timed out (the work is still running: the caller must not touch
 * the buffers involved and marks their owner as stuck), -1 = the runtime reported an error. */
static int qzWait(int dev, void *stream)
{
    const int r = qzstd_hip_stream_wait(dev, stream, (unsigned)gProc.timeoutMs);
    if (r == 1) { qzCause = QZ_CAUSE_TIMEOUT; QZ_LOG(1, "device %d: request timed out after %d ms\n", dev, gProc.timeoutMs); }
    if (r < 0) { qzCause = QZ_CAUSE_RUNTIME; QZ_LOG(1, "device %d: %s\n", dev, qzstd_hip_last_error()); }
    return r;
}

/* the same for a wait whose time-out quarantines the stream's owner: *stuck is set, the owner is not reused until the stream drains */
static int qzWaitOrQuarantine(int dev, void *stream, int *stuck)
{
    const int w = qzWait(dev, stream);
    if (w == 1) *stuck = 1;
    return w;
}

/* A stream that timed out is quarantined; it becomes usable again once a non-blocking query finds it drained. */
static int qzStillStuck(int dev, void *stream, int *stuck)
{
    if (!*stuck) return 0;
    if (qzstd_hip_stream_query(dev, stream) == 0) {
        *stuck = 0;
        QZ_LOG(1, "device %d: a timed-out stream has drained, back in service\n", dev);
        return 0;
    }
    return 1;
}

/* grow-only device buffers: returns the (possibly new) pointer, NULL on failure */
static void *qzGrowDev(int dev, void *old, size_t *cap, size_t need)
{
    void *p;
    if (old && *cap >= need) return old;
    qzstd_hip_free(dev, old);
    p = qzstd_hip_malloc(dev, need);
    *cap = p ? need : 0;
    return p;
}

/* free and forget: a pinned buffer, a device buffer (NULL: nothing to free) */
#define QZ_HOST_FREE(p) do { qzstd_hip_host_free(p); (p) = NULL; } while (0)
#define QZ_DEV_FREE(dev, p) do { qzstd_hip_free(dev, p); (p) = NULL; } while (0)

/* The staging copy of an announcement (reference: the memcpy into DMA memory, :1222-1227): caller's bytes -> pinned buffer the GPU reads over the
 * bus.  For a STABLE announcement nobody on the host reads the copy again soon (a sampled memcmp at most), so it goes out with STREAMING stores: no
 * read-for-ownership of the destination lines and no 2 MiB of a thread's cache spent on bytes only the GPU wants — with 16 threads staging at
 * once the copies share the socket's memory bandwidth, a third of which the ordinary stores' line fills took.  QZSTD_HIP_STAGE_NT=0: memcpy. */
static void qzStageCopy(unsigned char *dst, const unsigned char *src, size_t n)
{
    size_t i = 0;
    if (!gProc.stageNt || n < 4096 || ((uintptr_t)dst & 15u)) { memcpy(dst, src, n); return; }
    for (; i + 64 <= n; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i *)(const void *)(src + i)), b = _mm_loadu_si128((const __m128i *)(const void *)(src + i + 16)),
                      c = _mm_loadu_si128((const __m128i *)(const void *)(src + i + 32)), d = _mm_loadu_si128((const __m128i *)(const void *)(src + i + 48));
        _mm_stream_si128((__m128i *)(void *)(dst + i), a);
        _mm_stream_si128((__m128i *)(void *)(dst + i + 16), b);
        _mm_stream_si128((__m128i *)(void *)(dst + i + 32), c);
        _mm_stream_si128((__m128i *)(void *)(dst + i + 48), d);
    }
    _mm_sfence(); /* streaming stores are weakly ordered: before anything that tells the GPU the bytes are there */
    if (i < n) memcpy(dst + i, src + i, n - i);
}

/* shared by the producer and the hint: is the device usable?  Counts failures and
 * re-probes every QZ_RETRY_INTERVAL_BLOCKS-th block (reference :1140-1152). */
static int qzDeviceUsable(QZSTD_Session_T *s)
{
    if (gProc.status == QZSTD_OK) return 1;
    s->failOffloadCnt++;
    if (s->failOffloadCnt >= QZ_RETRY_INTERVAL_BLOCKS) {
        s->failOffloadCnt = 0;
        if (QZSTD_startQatDevice() == QZSTD_OK) return 1;
        QZ_LOG(1, "tried to restart the device, but failed\n");
        return 0;
    }
    QZ_LOG(1, "the device was not successfully started\n");
    return 0;
}

/* a callback is about to return the error code: count it by cause (QZSTD_failStats) */
static size_t qzFailed(QZSTD_Session_T *s, int cause)
{
    if (s) {
        s->fail[0]++;
        s->fail[cause > 0 && cause < QZ_CAUSE_N ? cause : QZ_CAUSE_RUNTIME]++;
    }
    return ZSTD_SEQUENCE_PRODUCER_ERROR;
}

/* ---- NUMA placement ---- */
/* pinned host memory that device `dev` reads or writes: on the NUMA node the GPU is attached to (reference: qaeMemAllocNUMA on the
 * instance's node, src/qatseqprod.c:216-246).  QZSTD_HIP_NUMA=0 or an unknown node: wherever the calling thread's policy puts it */
static void *qzHostAlloc(size_t bytes, int dev, int coherent)
{
    const int node = (gProc.numa && dev >= 0 && dev < QZ_MAX_DEVICES) ? gProc.devNode[dev] : -1;
    return qzstd_hip_host_alloc_on_node(bytes, node, coherent);
}

/* the NUMA node the calling thread runs on right now (-1 = unknown) */
static int qzThreadNode(void)
{
    unsigned int cpu = 0, node = 0;
    if (gProc.numaThreadNode >= 0) return gProc.numaThreadNode;
#ifdef SYS_getcpu
    if (syscall(SYS_getcpu, &cpu, &node, NULL) == 0) return (int)node;
#endif
    (void)cpu;
    return -1;
}

/* The sticky hint of a state at its first use: hint % numDevices is its GPU, hint / numDevices where its slot sweeps start.  A GPU of
 * the socket the calling thread runs on if there is one (round-robin among those), else round-robin over all GPUs — the reference
 * interleaves its instances across devices (src/qatseqprod.c:601-630) and leaves locality to the instance's node. */
static int qzPickHint(void)
{
    const int nd = gProc.numDevices, node = gProc.numa ? qzThreadNode() : -1;
    if (nd <= 0) return 0;
    if (node >= 0) {
        int local[QZ_MAX_DEVICES], n = 0, d;
        for (d = 0; d < nd && d < QZ_MAX_DEVICES; d++) if (gProc.devNode[d] == node) local[n++] = d;
        if (n > 0 && n < nd) { /* (every GPU on this node = plain round-robin below) */
            const unsigned int k = __sync_fetch_and_add(&gProc.nodeNext[(unsigned)node % QZ_NUMA_NODES_MAX], 1u) & 0xFFFFFu;
            return local[k % (unsigned)n] + nd * (int)(k / (unsigned)n);
        }
    }
    return (int)(__sync_fetch_and_add(&gProc.anyNext, 1u) & 0x3FFFFFFFu);
}

/* ---------------------------------------------------------------- take / join ---- */

/* A result area is completed by count words: the count says how many entries there are, not that they have all arrived — they are stored
 * by other waves than the count and nothing orders them on their ways to host memory (measured in round 3 on the resident service: under
 * load an item's last entries land up to microseconds after its count).  So every entry certifies ITSELF: it is ONE store that carries
 * its request's epoch or its area's tag (qzstd_hip_block_t.mark) and is taken when it shows it, by one of the two takers below.  Their
 * time-out counts from t0 (the service: its submit time) or, t0 == 0, from the first late entry (announcements).  One more round: */
static inline int qzSpinExpired(unsigned *spins, unsigned long t0)
{
    __builtin_ia32_pause();
    __asm__ volatile("" ::: "memory"); /* (a fresh load every time round) */
    return (++*spins & 1023u) == 0u && qzNowNs() - t0 > (unsigned long)gProc.timeoutMs * 1000000ul;
}

/* Takes n 16-byte entries: one aligned load per entry (it arrived as one store), taken when its fourth word shows the epoch; the mark is
 * masked out of the copy (the pinned area keeps it: marks of an earlier lap are wiped when the epoch or tag starts over).  *covered +=
 * the literal and match lengths of the entries taken, added up in the same pass.  0 = taken, 1 = not within the time-out. */
static int qzTakeMarked(ZSTD_Sequence *dst, const ZSTD_Sequence *q, size_t n, unsigned int epoch, unsigned long t0, size_t *covered)
{
    const __m128i keep = _mm_set_epi32(0, -1, -1, -1);
    __m128i acc = _mm_setzero_si128();
    size_t j;
    for (j = 0; j < n; j++) {
        __m128i v;
        unsigned spins = 0;
        while (v = _mm_load_si128((const __m128i *)(const void *)(q + j)), (unsigned int)_mm_cvtsi128_si32(_mm_srli_si128(v, 12)) != epoch) {
            if (!t0) t0 = qzNowNs(); /* not there yet: rare */
            if (qzSpinExpired(&spins, t0)) return 1;
        }
        _mm_storeu_si128((__m128i *)(void *)(dst + j), _mm_and_si128(v, keep));
        acc = _mm_add_epi32(acc, v); /* literal and match lengths add up in lanes 1 and 2 (a block is 128 KiB at most) */
    }
    *covered += (size_t)(unsigned int)_mm_cvtsi128_si32(_mm_srli_si128(acc, 4)) + (unsigned int)_mm_cvtsi128_si32(_mm_srli_si128(acc, 8));
    return 0;
}

/* The same for PACKED entries (qzstd_hip.h: QZSTD_HIP_MARK_COMPACT): one 8-byte load per entry (it arrived as one store), taken when its top 12
 * bits show the tag, unpacked into the caller's ZSTD_Sequence array. */
static int qzTakePacked(ZSTD_Sequence *dst, const unsigned long long *q, size_t n, unsigned int tag, unsigned long t0)
{
    const __m128i m17 = _mm_set_epi32(0, 0x1FFFF, 0, 0x1FFFF), m18 = _mm_set_epi32(0, 0x3FFFF, 0, 0x3FFFF);
    size_t j = 0;
    while (j < n) {
        if (j + 2 <= n && !((uintptr_t)(q + j) & 15u)) { /* two entries per step: the usual case, both there (an ALIGNED 16-byte load: each
                                                           * 8-byte half is one of the kernel's stores, never torn) */
            const __m128i v = _mm_load_si128((const __m128i *)(const void *)(q + j));
            const __m128i t = _mm_srli_epi64(v, 52);
            if ((unsigned int)_mm_cvtsi128_si32(t) == tag && (unsigned int)_mm_cvtsi128_si32(_mm_srli_si128(t, 8)) == tag) {
                const __m128i ol = _mm_or_si128(_mm_and_si128(v, m17), _mm_slli_epi64(_mm_and_si128(_mm_srli_epi64(v, 17), m18), 32)); /* off0 lit0 off1 lit1 */
                const __m128i ml = _mm_and_si128(_mm_srli_epi64(v, 35), m17);                                                          /* ml0  0    ml1  0    */
                _mm_storeu_si128((__m128i *)(void *)(dst + j), _mm_unpacklo_epi64(ol, ml));
                _mm_storeu_si128((__m128i *)(void *)(dst + j + 1), _mm_unpackhi_epi64(ol, ml));
                j += 2;
                continue;
            }
        }
        {
            unsigned long long v;
            unsigned spins = 0;
            while (v = __atomic_load_n(&q[j], __ATOMIC_RELAXED), QZSTD_HIP_PACKED_TAG(v) != tag) {
                if (!t0) t0 = qzNowNs(); /* not there yet: rare */
                if (qzSpinExpired(&spins, t0)) return 1;
            }
            dst[j].offset = QZSTD_HIP_PACKED_OFF(v);
            dst[j].litLength = QZSTD_HIP_PACKED_LIT(v);
            dst[j].matchLength = QZSTD_HIP_PACKED_ML(v);
            dst[j].rep = 0;
            j++;
        }
    }
    return 0;
}

/* Joining independently parsed lists — segments of a batched block, items of a service request, announced grid blocks.  Every piece is
 * count >= 1 entries, the last one its delimiter {0, trailing literals, 0, 0}: all but the delimiter are copied, the pending trailing
 * literals go to the first copied entry, the delimiter's are carried on (a delimiter-only piece only adds to the carry); one delimiter
 * closes the list.  The caller applies its capacity rule BEFORE it appends a piece.  covered: literal + match lengths of the 16-byte
 * entries taken, delimiters included (the service's adds-up check). */
typedef struct { ZSTD_Sequence *dst; size_t out, carry, covered; } QZSTD_Join_T;

/* Appends one piece in the form its descriptor's mark names: 0 = complete in ordinary memory (a launch's results after the stream wait);
 * QZSTD_HIP_MARK_COMPACT | tag = packed entries; else 16-byte entries that show the mark (an epoch or tag of at most 24 bits: bit 31 is
 * never set in one).  Marked and packed entries are taken as they certify themselves, the delimiter too; 1 = not within the time-out. */
static int qzJoinPiece(QZSTD_Join_T *j, const void *q, size_t count, unsigned int mark, unsigned long t0)
{
    ZSTD_Sequence *dst = j->dst + j->out, dl;
    const size_t carry = j->carry;
    if (mark == 0u) {
        memcpy(dst, q, (count - 1) * sizeof(ZSTD_Sequence));
        dl = ((const ZSTD_Sequence *)q)[count - 1];
    } else if (mark & QZSTD_HIP_MARK_COMPACT) {
        const unsigned long long *q8 = (const unsigned long long *)q;
        if (qzTakePacked(dst, q8, count - 1, mark & 0xFFFu, t0) != 0 || qzTakePacked(&dl, q8 + count - 1, 1, mark & 0xFFFu, t0) != 0) return 1;
    } else {
        const ZSTD_Sequence *q16 = (const ZSTD_Sequence *)q;
        if (qzTakeMarked(dst, q16, count - 1, mark, t0, &j->covered) != 0 || qzTakeMarked(&dl, q16 + count - 1, 1, mark, t0, &j->covered) != 0) return 1;
    }
    if (count > 1) {
        dst->litLength += (unsigned int)carry;
        j->out += count - 1;
        j->carry = 0;
    }
    j->carry += dl.litLength;
    return 0;
}

/* closes the joined list with its delimiter; returns the sequence count */
static size_t qzJoinFinish(QZSTD_Join_T *j)
{
    j->dst[j->out].offset = 0; j->dst[j->out].litLength = (unsigned int)j->carry;
    j->dst[j->out].matchLength = 0; j->dst[j->out].rep = 0;
    return ++j->out;
}

/* ---------------------------------------------------------------- slots ---------- */

static void qzFreeSlot(QZSTD_Slot_T *s)
{
    const int dev = s->device;
    if (s->stream) (void)qzstd_hip_stream_wait(dev, s->stream, (unsigned)gProc.timeoutMs);
    if (s->vSrc) memset(s->vSrc, 0, QZSTD_HIP_BLOCK_MAX + 64); /* staged caller data: scrubbed before the pages go back */
    QZ_HOST_FREE(s->hSrc); QZ_HOST_FREE(s->hSeqs); QZ_HOST_FREE(s->hDesc); QZ_HOST_FREE(s->hCount);
    QZ_HOST_FREE(s->vSrc); QZ_HOST_FREE(s->vSeqs); QZ_HOST_FREE(s->vCount);
    QZ_DEV_FREE(dev, s->dSrc); QZ_DEV_FREE(dev, s->dSeqs); QZ_DEV_FREE(dev, s->dDesc); QZ_DEV_FREE(dev, s->dCount); QZ_DEV_FREE(dev, s->dWork);
    QZ_DEV_FREE(dev, s->vdSrc); QZ_DEV_FREE(dev, s->vdWork);
    if (s->stream) qzstd_hip_stream_destroy(dev, s->stream);
    memset(s, 0, sizeof(*s));
    s->device = dev;
}

/* lazy per-slot setup, first use only (reference: QZSTD_allocInstMem, :685-822) */
static int qzSetupSlot(QZSTD_Slot_T *s)
{
    if (!s->stream) {
        s->stream = qzstd_hip_stream_create(s->device);
        if (!s->stream) {
            QZ_LOG(1, "slot setup failed on device %d: %s\n", s->device, qzstd_hip_last_error());
            return QZSTD_FAIL;
        }
    }
    if (s->ready) return QZSTD_OK;
    s->seqCap = qzstd_hip_sequence_bound(QZSTD_HIP_BLOCK_MAX);
    s->hSrc = (unsigned char *)qzHostAlloc(QZSTD_HIP_BLOCK_MAX + 64, s->device, 0);
    s->hSeqs = (ZSTD_Sequence *)qzHostAlloc(s->seqCap * sizeof(ZSTD_Sequence), s->device, 0);
    s->hDesc = (qzstd_hip_block_t *)qzHostAlloc(sizeof(qzstd_hip_block_t), s->device, 0);
    s->hCount = (unsigned int *)qzHostAlloc(64, s->device, 0);
    s->dSrc = (unsigned char *)qzstd_hip_malloc(s->device, QZSTD_HIP_BLOCK_MAX + 64);
    s->dSeqs = (ZSTD_Sequence *)qzstd_hip_malloc(s->device, s->seqCap * sizeof(ZSTD_Sequence));
    s->dDesc = (qzstd_hip_block_t *)qzstd_hip_malloc(s->device, sizeof(qzstd_hip_block_t));
    s->dCount = (unsigned int *)qzstd_hip_malloc(s->device, 64);
    if (!s->hSrc || !s->hSeqs || !s->hDesc || !s->hCount || !s->dSrc || !s->dSeqs || !s->dDesc || !s->dCount) {
        QZ_LOG(1, "slot setup failed on device %d: %s\n", s->device, qzstd_hip_last_error());
        qzFreeSlot(s);
        return QZSTD_FAIL;
    }
    s->ready = 1;
    return QZSTD_OK;
}

/* one quick sweep over the slots (no waiting), starting at the caller's sticky hint; dev >= 0 confines it to the slots of
 * that GPU (slot i sits on device i % numDevices) */
static int qzTryGrabSlot(int hint, int dev)
{
    int k;
    const int n = gProc.numSlots, nd = gProc.numDevices;
    if (n <= 0) return -1;
    if (hint < 0 || hint >= n) hint = 0;
    if (dev >= 0) hint = hint - hint % nd + dev; /* same row, that device's column */
    for (k = 0; k < n; k += dev >= 0 ? nd : 1) {
        const int i = (hint + k) % n;
        if (__sync_lock_test_and_set(&gProc.slots[i].lock, 1) == 0) return i;
    }
    return -1;
}

/* test-and-set sweep over the slots, starting at the caller's sticky hint
 * (reference: QZSTD_grabInstance, :905-928) */
static int qzGrabSlot(int hint, int dev)
{
    int sweep;
    /* The reference sweeps its instances 10 times and then fails the block (src/qatseqprod.c:905-928, :915);
     * here a caller WAITS for a slot: short spins first, then 50 us naps, giving up only after about two seconds
     * (the reference's own time-out for a stuck request, :1261-1285) */
    for (sweep = 0; sweep < QZ_GRAB_SWEEPS; sweep++) {
        const int i = qzTryGrabSlot(hint, dev);
        if (i >= 0 || gProc.numSlots <= 0) return i;
        if (sweep < 64) {
            sched_yield(); /* every slot busy: more threads than slots; let the holders finish */
        } else {
            const struct timespec nap = { 0, 50000 };
            nanosleep(&nap, NULL);
        }
    }
    return -1;
}

static void qzReleaseSlot(int i)
{
    __sync_lock_release(&gProc.slots[i].lock);
}

/* one block, synchronously, on a slot */
static size_t qzRunBlock(QZSTD_Slot_T *sl, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity, const void *src,
                         size_t srcSize, int level)
{
    const size_t cap = outSeqsCapacity < sl->seqCap ? outSeqsCapacity : sl->seqCap;
    size_t first, count;
    memcpy(sl->hSrc, src, srcSize); /* staging copy, reference :1223 */
    sl->hDesc->srcOff = 0;
    sl->hDesc->seqOff = 0;
    sl->hDesc->srcLen = (unsigned int)srcSize;
    sl->hDesc->seqCap = (unsigned int)cap;
    sl->hDesc->parseFrom = 0;
    sl->hDesc->mark = 0;
    {
        const size_t work = qzstd_hip_workspace_bytes(level, 1, (unsigned int)srcSize);
        if (work) sl->dWork = qzGrowDev(sl->device, sl->dWork, &sl->dWorkCap, work);
        if (work && !sl->dWork) goto fail;
    }
    if (qzstd_hip_memcpy_h2d(sl->device, sl->stream, sl->dSrc, sl->hSrc, (srcSize + 15) & ~(size_t)15) ||
        qzstd_hip_memcpy_h2d(sl->device, sl->stream, sl->dDesc, sl->hDesc, sizeof(*sl->hDesc)) ||
        qzstd_hip_find_sequences(sl->device, sl->stream, level, sl->dSrc, sl->dDesc, 1, (unsigned int)srcSize,
                                 sl->dSeqs, sl->dCount, sl->dWork, sl->dWorkCap))
        goto fail;
    first = cap < QZ_FIRST_COPY_SEQS ? cap : QZ_FIRST_COPY_SEQS;
    if (qzstd_hip_memcpy_d2h(sl->device, sl->stream, sl->hCount, sl->dCount, sizeof(unsigned int)) ||
        qzstd_hip_memcpy_d2h(sl->device, sl->stream, sl->hSeqs, sl->dSeqs, first * sizeof(ZSTD_Sequence)))
        goto fail;
    if (qzWaitOrQuarantine(sl->device, sl->stream, &sl->stuck) != 0) goto fail;
    count = *sl->hCount;
    if (count == QZSTD_HIP_NSEQ_ERROR || count == 0 || count >= outSeqsCapacity - 1) {
        QZ_LOG(1, "sequence count %zu does not fit capacity %zu\n", count, outSeqsCapacity);
        qzCause = QZ_CAUSE_CAPACITY;
        return ZSTD_SEQUENCE_PRODUCER_ERROR; /* reference :1318-1322 */
    }
    if (count > first) {
        if (qzstd_hip_memcpy_d2h(sl->device, sl->stream, sl->hSeqs + first, sl->dSeqs + first,
                                 (count - first) * sizeof(ZSTD_Sequence)))
            goto fail;
        if (qzWaitOrQuarantine(sl->device, sl->stream, &sl->stuck) != 0) goto fail;
    }
    memcpy(outSeqs, sl->hSeqs, count * sizeof(ZSTD_Sequence));
    return count;
fail:
    QZ_LOG(1, "device request failed: %s\n", qzstd_hip_last_error());
    return ZSTD_SEQUENCE_PRODUCER_ERROR;
}

/* one block on a slot of its own (QZSTD_HIP_COALESCE=0, and blocks too dense for a batch) */
static size_t qzSlotBlock(QZSTD_Session_T *s, int dev, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity, const void *src,
                          size_t srcSize, int level)
{
    size_t rc = ZSTD_SEQUENCE_PRODUCER_ERROR;
    int tries;
    for (tries = 0; tries < 4; tries++) {
        const int i = qzGrabSlot(s->slotHint + tries * gProc.numDevices, dev);
        QZSTD_Slot_T *sl;
        if (i < 0) {
            QZ_LOG(1, "failed to grab a slot\n");
            return ZSTD_SEQUENCE_PRODUCER_ERROR;
        }
        sl = &gProc.slots[i];
        if (sl->stream && qzStillStuck(sl->device, sl->stream, &sl->stuck)) { /* quarantined: try the next one */
            qzReleaseSlot(i);
            continue;
        }
        if (dev < 0) s->slotHint = i;
        if (qzSetupSlot(sl) == QZSTD_OK) rc = qzRunBlock(sl, outSeqs, outSeqsCapacity, src, srcSize, level);
        QZ_LOG(2, "block %zu B level %d -> %zu sequences (slot %d, device %d)\n", srcSize, level & 0xFF, rc, i, sl->device);
        qzReleaseSlot(i);
        return rc;
    }
    return rc;
}

/* ---------------------------------------------------------------- coalescer ------ */

static void qzFreeBatch(QZSTD_Coalescer_T *c, QZSTD_Batch_T *bt)
{
    if (bt->stream) (void)qzstd_hip_stream_wait(c->device, bt->stream, (unsigned)gProc.timeoutMs);
    QZ_HOST_FREE(bt->hSrc); QZ_HOST_FREE(bt->hSeqs); QZ_HOST_FREE(bt->hDesc); QZ_HOST_FREE(bt->hCount);
    QZ_DEV_FREE(c->device, bt->dSrc); QZ_DEV_FREE(c->device, bt->dWork);
    if (bt->stream) qzstd_hip_stream_destroy(c->device, bt->stream);
    bt->dWorkCap = 0; bt->stream = NULL; bt->dvSeqs = bt->dvDesc = bt->dvCount = NULL; bt->ready = 0;
}

static void qzFreeCoalescer(QZSTD_Coalescer_T *c)
{
    int b;
    for (b = 0; b < QZ_BATCHES; b++) qzFreeBatch(c, &c->batch[b]);
    QZ_LOG(2, "device %d: %lu block(s) in %lu batch(es), %lu launch(es)\n", c->device, c->blocks, c->batches, c->launches);
    pthread_mutex_destroy(&c->mu);
    pthread_cond_destroy(&c->cvOpen);
    for (b = 0; b < QZ_BATCHES; b++) {
        pthread_cond_destroy(&c->batch[b].cvLead);
        pthread_cond_destroy(&c->batch[b].cvDone);
    }
}

/* lazy, per batch, under c->mu; a failure frees what was created (nothing leaks when pinned memory is short) */
static int qzSetupBatch(QZSTD_Coalescer_T *c, QZSTD_Batch_T *bt)
{
    if (bt->ready) return QZSTD_OK;
    bt->stream = qzstd_hip_stream_create(c->device);
    bt->dSrc = (unsigned char *)qzstd_hip_malloc(c->device, QZ_BATCH_MAX * QZ_SRC_STRIDE);
    bt->hSrc = (unsigned char *)qzHostAlloc(QZ_BATCH_MAX * QZ_SRC_STRIDE, c->device, 0);
    bt->hSeqs = (ZSTD_Sequence *)qzHostAlloc(QZ_BATCH_MAX * QZ_BATCH_PITCH * sizeof(ZSTD_Sequence), c->device, 0);
    bt->hDesc = (qzstd_hip_block_t *)qzHostAlloc(QZ_DESC_MAX * sizeof(qzstd_hip_block_t), c->device, 0);
    bt->hCount = (unsigned int *)qzHostAlloc(QZ_DESC_MAX * sizeof(unsigned int), c->device, 0);
    bt->dvSeqs = qzstd_hip_host_device_ptr(bt->hSeqs);
    bt->dvDesc = qzstd_hip_host_device_ptr(bt->hDesc);
    bt->dvCount = qzstd_hip_host_device_ptr(bt->hCount);
    if (!(bt->stream && bt->dSrc && bt->hSrc && bt->hSeqs && bt->hDesc && bt->hCount && bt->dvSeqs && bt->dvDesc && bt->dvCount)) {
        QZ_LOG(1, "batch setup failed on device %d: %s\n", c->device, qzstd_hip_last_error());
        qzFreeBatch(c, bt);
        return QZSTD_FAIL;
    }
    bt->ready = 1;
    return QZSTD_OK;
}

/* How a batch's launch cuts request ri into work items (the service has its own rule, on purpose: qzSvcQueue): r->nSeg descriptors from
 * bt->hDesc[k] on; returns the next free one.  Lone-request latency: at the levels whose profile allows it (segLog: no match crosses a
 * 32 KiB boundary) a block goes as SEGMENT work items — each workgroup inserts the block before its segment into its tables and parses
 * its segment only — which finish in about 40 % of the time of the whole block; the caller joins the segments' sequence lists. */
static int qzPlanSegments(QZSTD_Batch_T *bt, int ri, int k)
{
    QZSTD_Req_T *r = &bt->req[ri];
    const int n = bt->n;
    qzstd_hip_profile_t pf;
    /* a full batch fills the GPU as it is: segment items then only repeat the insert work of the block before them
     * (and, at the chain levels, multiply the scratch); they pay for batches that leave CUs idle */
    size_t seg = 0, segsMax = !gProc.splitBlocks ? 1 : (n * 32 <= QZ_SPLIT_ITEMS_MAX ? 32 : (n * 8 <= QZ_SPLIT_ITEMS_MAX ? 8 : 1));
    int sg;
    r->nSeg = 1;
    r->dense = 0;
    if (segsMax > 1 && qzstd_hip_profile_for_level(r->level, r->srcSize, &pf) == 0 && pf.segLog) {
        /* chain levels: every item of a LAUNCH links the block before it in a scratch of its own (20 B per position of the whole
         * block: the workgroups of a launch do not start in order, so they cannot share one as the service's items do) — 32 items
         * per block would grow the batch's grow-only scratch to 32 x 2.6 MB per caller; eight keep most of the latency gain */
        if (pf.chainDepth && segsMax > 8) segsMax = 8;
        seg = (size_t)1 << pf.segLog;
        while ((r->srcSize + seg - 1) / seg > segsMax) seg *= 2; /* whole segments per item */
        if (r->srcSize > seg) r->nSeg = (int)((r->srcSize + seg - 1) / seg);
    }
    r->segPitch = (unsigned int)(QZ_BATCH_PITCH / (size_t)r->nSeg);
    for (sg = 0; sg < r->nSeg; sg++, k++) {
        qzstd_hip_block_t *d = &bt->hDesc[k];
        d->srcOff = (size_t)ri * QZ_SRC_STRIDE;
        d->mark = 0;
        if (r->nSeg == 1) {
            d->seqOff = (size_t)ri * QZ_BATCH_PITCH;
            d->srcLen = (unsigned int)r->srcSize;
            d->seqCap = (unsigned int)(r->cap < QZ_BATCH_PITCH ? r->cap : QZ_BATCH_PITCH);
            d->parseFrom = 0;
        } else { /* segment sg: the block up to the segment's end, parsed from the segment's start */
            const size_t end = (size_t)(sg + 1) * seg;
            d->seqOff = (size_t)ri * QZ_BATCH_PITCH + (size_t)sg * r->segPitch;
            d->srcLen = (unsigned int)(end < r->srcSize ? end : r->srcSize);
            d->seqCap = r->segPitch;
            d->parseFrom = (unsigned int)((size_t)sg * seg);
        }
    }
    return k;
}

/* the leader's job: one launch per level present in the batch (called WITHOUT c->mu held) */
static void qzRunBatch(QZSTD_Coalescer_T *c, QZSTD_Batch_T *bt)
{
    const int n = bt->n, dev = c->device;
    int order[QZ_BATCH_MAX], first[QZ_BATCH_MAX];
    int i, j, k = 0, g0, failed = 0, launches = 0;
    /* requests grouped by level (insertion sort, stable: the usual batch has one level) */
    for (i = 0; i < n; i++) {
        for (j = i; j > 0 && bt->req[order[j - 1]].level > bt->req[i].level; j--) order[j] = order[j - 1];
        order[j] = i;
    }
    for (j = 0; j < n; j++) {
        first[j] = k;
        k = qzPlanSegments(bt, order[j], k);
    }
    /* one copy in, one launch per level, one wait: the kernel reads the descriptors from and writes the sequences and
     * counts to this batch's pinned host buffers directly (posted PCIe writes while it runs), which takes two
     * copies and one synchronisation off the latency of a request */
    failed = qzstd_hip_memcpy_h2d(dev, bt->stream, bt->dSrc, bt->hSrc, (size_t)n * QZ_SRC_STRIDE);
    for (g0 = 0; g0 < n && !failed; ) {
        const int level = bt->req[order[g0]].level;
        unsigned int maxLen = 0;
        int g1 = g0, k0 = first[g0], k1;
        size_t work;
        while (g1 < n && bt->req[order[g1]].level == level) {
            if (bt->req[order[g1]].srcSize > maxLen) maxLen = (unsigned int)bt->req[order[g1]].srcSize;
            g1++;
        }
        k1 = g1 < n ? first[g1] : k;
        work = qzstd_hip_workspace_bytes(level, (unsigned int)(k1 - k0), maxLen);
        /* the scratch is about to be replaced: what runs on it has to finish first */
        if (work > bt->dWorkCap && launches) failed = qzWaitOrQuarantine(dev, bt->stream, &bt->stuck) != 0;
        if (work && !failed) bt->dWork = qzGrowDev(dev, bt->dWork, &bt->dWorkCap, work);
        failed = failed || (work && !bt->dWork) ||
                 qzstd_hip_find_sequences(dev, bt->stream, level, bt->dSrc, (const qzstd_hip_block_t *)bt->dvDesc + k0,
                                          (unsigned int)(k1 - k0), maxLen, bt->dvSeqs, (unsigned int *)bt->dvCount + k0,
                                          bt->dWork, bt->dWorkCap);
        launches++;
        g0 = g1;
    }
    /* whatever was queued — the copy, the launches of earlier level groups — has to be off the stream before the batch's
     * buffers are handed back, also when a later step failed (round-2 ADVICE); after a time-out the kernel may still write
     * into this batch's buffers: quarantined */
    if (!bt->stuck && qzWaitOrQuarantine(dev, bt->stream, &bt->stuck) != 0) failed = 1;
    {
        const int cause = bt->stuck ? QZ_CAUSE_TIMEOUT : QZ_CAUSE_RUNTIME;
        for (j = 0; j < n; j++) bt->req[j].cause = cause;
    }
    for (j = 0; j < n; j++) {
        QZSTD_Req_T *r = &bt->req[order[j]];
        size_t total = 1;
        int sg, bad = failed;
        for (sg = 0; sg < r->nSeg && !bad; sg++) {
            const unsigned int cnt = bt->hCount[first[j] + sg];
            r->segCnt[sg] = cnt;
            if (cnt == QZSTD_HIP_NSEQ_ERROR || cnt == 0) bad = 1;
            else total += cnt - 1;
        }
        /* capacity rule, reference :1318-1322; a result area of the batch that was too small (not the caller's
         * capacity) means: redo this block alone */
        if (bad) r->dense = !failed && (r->nSeg > 1 || r->cap > QZ_BATCH_PITCH);
        if (!failed) r->cause = QZ_CAUSE_CAPACITY;
        r->rc = (bad || total >= r->cap - 1) ? ZSTD_SEQUENCE_PRODUCER_ERROR : total;
    }
    if (failed) QZ_LOG(1, "device request failed: %s\n", qzstd_hip_last_error());
    c->launches += (unsigned long)launches;
    c->batches++;
    c->blocks += (unsigned long)n;
    __atomic_fetch_add(&gProc.devBlocks[dev][1], (unsigned long)n, __ATOMIC_RELAXED);
}

/* one block through the coalescer of device `dev`; returns the sequence count or the error code */
static size_t qzCoalescedBlock(QZSTD_Session_T *s, int dev, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity, const void *src,
                               size_t srcSize, int level)
{
    QZSTD_Coalescer_T *c = &gProc.coal[dev];
    QZSTD_Batch_T *bt = NULL;
    size_t rc;
    int i, b, dense;

    pthread_mutex_lock(&c->mu);
    for (;;) {
        int usable = 0;
        if (c->open >= 0 && c->batch[c->open].state == 0 && c->batch[c->open].n < QZ_BATCH_MAX) { /* join the collecting batch */
            bt = &c->batch[c->open];
            break;
        }
        if (c->open < 0) { /* nobody is collecting: open an idle batch and lead it */
            for (b = 0; b < QZ_BATCHES && !bt; b++) {
                QZSTD_Batch_T *cand = &c->batch[b];
                if (cand->state != 0 || cand->n != 0) { usable++; continue; } /* busy, but it will come back */
                if (qzStillStuck(dev, cand->stream, &cand->stuck)) continue;
                if (qzSetupBatch(c, cand) != QZSTD_OK) continue;
                bt = cand;
                c->open = b;
            }
            if (bt) break;
            if (!usable) { /* every batch is stuck or cannot be set up: fail the block (libzstd's fallback takes over) */
                pthread_mutex_unlock(&c->mu);
                qzCause = QZ_CAUSE_RUNTIME;
                return ZSTD_SEQUENCE_PRODUCER_ERROR;
            }
        }
        pthread_cond_wait(&c->cvOpen, &c->mu);
    }
    i = bt->n++;
    bt->req[i].src = src;
    bt->req[i].srcSize = srcSize;
    bt->req[i].cap = outSeqsCapacity;
    bt->req[i].rc = ZSTD_SEQUENCE_PRODUCER_ERROR;
    bt->req[i].level = level;
    pthread_mutex_unlock(&c->mu);

    memcpy(bt->hSrc + (size_t)i * QZ_SRC_STRIDE, src, srcSize); /* staging copy (reference :1223), on the caller's thread */

    pthread_mutex_lock(&c->mu);
    bt->copied++;
    if (i == 0) {
        /* the first member leads its batch: whoever arrived while it was staging has joined; close and launch.
         * Every waiter has its own condition variable (no thundering herd when more threads than cores wait here). */
        bt->state = 1;
        c->open = -1; /* newcomers open another batch, or wait for one to come back */
        pthread_cond_broadcast(&c->cvOpen);
        while (bt->copied < bt->n) pthread_cond_wait(&bt->cvLead, &c->mu); /* members still staging */
        pthread_mutex_unlock(&c->mu);
        qzRunBatch(c, bt);
        pthread_mutex_lock(&c->mu);
        bt->state = 2;
        pthread_cond_broadcast(&bt->cvDone);
    } else {
        if (bt->state == 1 && bt->copied == bt->n) pthread_cond_signal(&bt->cvLead);
        while (bt->state != 2) pthread_cond_wait(&bt->cvDone, &c->mu);
    }
    pthread_mutex_unlock(&c->mu);

    rc = bt->req[i].rc;
    if (rc == ZSTD_SEQUENCE_PRODUCER_ERROR) qzCause = bt->req[i].cause;
    if (rc != ZSTD_SEQUENCE_PRODUCER_ERROR) {
        const QZSTD_Req_T *r = &bt->req[i];
        if (r->nSeg == 1) {
            memcpy(outSeqs, bt->hSeqs + (size_t)i * QZ_BATCH_PITCH, rc * sizeof(ZSTD_Sequence));
        } else { /* join the segments: the trailing literals of one flow into the first sequence of the next */
            QZSTD_Join_T jn = { outSeqs, 0, 0, 0 };
            int sg;
            for (sg = 0; sg < r->nSeg; sg++) (void)qzJoinPiece(&jn, bt->hSeqs + (size_t)i * QZ_BATCH_PITCH + (size_t)sg * r->segPitch, r->segCnt[sg], 0u, 0ul);
            (void)qzJoinFinish(&jn); /* (its count is rc: the leader added the segments up for the capacity rule) */
        }
    }
    dense = rc == ZSTD_SEQUENCE_PRODUCER_ERROR && bt->req[i].dense && !bt->stuck;

    pthread_mutex_lock(&c->mu);
    if (++bt->consumed == bt->n) { /* last one out hands the batch back */
        bt->n = bt->copied = bt->consumed = 0;
        bt->state = 0;
        pthread_cond_broadcast(&c->cvOpen);
    }
    pthread_mutex_unlock(&c->mu);
    /* a block with more sequences than the batch's result pitch holds (incompressible-looking data with many
     * short matches) is redone alone with the caller's full capacity */
    if (dense) {
        s->redoneAlone++;
        rc = qzSlotBlock(s, dev, outSeqs, outSeqsCapacity, src, srcSize, level);
    }
    return rc;
}

/* ---------------------------------------------------------------- service -------- */

/* buffers of a slot's service requests, first use only; 0 on success (a failure frees what was created) */
static int qzSetupSlotService(QZSTD_Slot_T *sl)
{
    if (sl->vSrc) return 0;
    sl->vSrc = (unsigned char *)qzHostAlloc(QZSTD_HIP_BLOCK_MAX + 64, sl->device, 1);
    sl->vSeqs = (ZSTD_Sequence *)qzHostAlloc(QZ_SVC_ITEMS_MAX * QZ_SVC_ITEM_CAP * sizeof(ZSTD_Sequence), sl->device, 1);
    if (sl->vSeqs) memset(sl->vSeqs, 0, QZ_SVC_ITEMS_MAX * QZ_SVC_ITEM_CAP * sizeof(ZSTD_Sequence)); /* (fresh pinned pages may hold marked entries of an earlier life) */
    sl->vCount = (unsigned int *)qzHostAlloc(QZ_SVC_ITEMS_MAX * sizeof(unsigned int), sl->device, 1);
    sl->vdSrc = (unsigned char *)qzstd_hip_malloc(sl->device, QZSTD_HIP_BLOCK_MAX + 64);
    if (!sl->vSrc || !sl->vSeqs || !sl->vCount || !sl->vdSrc) {
        QZ_LOG(1, "service buffers of a slot on device %d: %s\n", sl->device, qzstd_hip_last_error());
        QZ_HOST_FREE(sl->vSrc); QZ_HOST_FREE(sl->vSeqs); QZ_HOST_FREE(sl->vCount); QZ_DEV_FREE(sl->device, sl->vdSrc);
        return -1;
    }
    memset(sl->vCount, 0xFF, QZ_SVC_ITEMS_MAX * sizeof(unsigned int)); /* "arrived": nothing is outstanding */
    sl->vItems = 0;
    return 0;
}

/* levels >= 5 (exact hash chains): their service requests carry a chain scratch (a launch's scratch is sized by qzstd_hip_workspace_bytes at every level) */
static int qzIsChainLevel(int level)
{
    qzstd_hip_profile_t p;
    return qzstd_hip_profile_for_level(level, QZSTD_HIP_BLOCK_MAX, &p) == 0 && p.chainDepth != 0;
}

/* one request to the resident service, from the grab of its slot to its answer */
typedef struct {
    QZSTD_Slot_T *sl;
    int slot, level;
    qzstd_hip_svc_req_t rq;
    unsigned long t0, spinNs; /* when the polling began (the time-out counts from here); how long it stays busy before it naps */
} QZSTD_SvcCall_T;
enum { QZ_SVC_DONE = 0, QZ_SVC_TIMED_OUT, QZ_SVC_REJECTED, QZ_SVC_WRONG }; /* how a queued request ended (qzSvcCollect) */

/* Grab a slot of device `dev`, make it ready (buffers, count words, epoch, the request), stage the block and queue the request.
 * 0 = queued, c holds the slot; -1 = not now (no slot free, its last request still outstanding, no memory, the service does not take
 * the request): nothing is held. */
static int qzSvcQueue(QZSTD_SvcCall_T *c, int hint, int dev, const void *src, size_t srcSize, int level)
{
    const size_t pad = ((srcSize + 15) & ~(size_t)15) - srcSize;
    QZSTD_Slot_T *sl;
    qzstd_hip_svc_req_t *rq = &c->rq;
    size_t itemBytes = (size_t)gProc.svcItemBytes, nItems, k;
    int rc, progressive;
    while ((srcSize + itemBytes - 1) / itemBytes > QZ_SVC_ITEMS_MAX) itemBytes *= 2; /* (the launch path's rule differs: qzPlanSegments) */
    nItems = (srcSize + itemBytes - 1) / itemBytes;
    c->level = level;
    c->slot = qzTryGrabSlot(hint, dev);
    if (c->slot < 0) return -1;
    sl = c->sl = &gProc.slots[c->slot];
    if (sl->vStuck) { /* a request of this slot timed out: usable again once every count word of it has arrived */
        for (k = 0; k < sl->vItems; k++)
            if (__atomic_load_n(&sl->vCount[k], __ATOMIC_ACQUIRE) == 0u) goto notNow;
        sl->vStuck = 0;
    }
    if (qzSetupSlotService(sl) != 0) goto notNow;
    /* progressive staging (qzstd_hip.h, round 5): where the workers look at a count word before they read its slice, the request is queued
     * FIRST and the block is copied into the pinned buffer behind it, slice by slice — the staging copy (13 us for 128 KiB) then overlaps
     * the request's way to the first worker (8 us) instead of standing in front of it */
    progressive = qzstd_hip_service_progressive(sl->device) == 1;
    if (!progressive) {
        memcpy(sl->vSrc, src, srcSize); /* staging copy, reference :1223 */
        memset(sl->vSrc + srcSize, 0, pad);
    }
    for (k = 0; k < nItems; k++) sl->vCount[k] = progressive ? QZSTD_HIP_NSEQ_STAGING : 0u;
    sl->vItems = (unsigned int)nItems;
    sl->vEpoch = (sl->vEpoch + 1u) & 0xFFFFFFu;
    if (sl->vEpoch == 0u) {
        /* the 24-bit epoch starts over: an entry that no request of the last 2^24 overwrote would show a mark that is valid again.
         * The slot is ours and its previous request is complete (every count word in): wipe the result area once per lap. */
        memset(sl->vSeqs, 0, QZ_SVC_ITEMS_MAX * QZ_SVC_ITEM_CAP * sizeof(ZSTD_Sequence));
        sl->vEpoch = 1u;
    }
    rq->hSrc = sl->vSrc; rq->dSrc = sl->vdSrc; rq->hSeqs = sl->vSeqs; rq->hCount = sl->vCount;
    rq->srcLen = (uint32_t)srcSize; rq->itemBytes = (uint32_t)itemBytes; rq->nItems = (uint32_t)nItems;
    rq->seqCapPerItem = (uint32_t)(QZ_SVC_ITEMS_MAX * QZ_SVC_ITEM_CAP / nItems); /* the slot's whole result area, shared out */
    rq->slot = (uint32_t)c->slot; rq->epoch = sl->vEpoch;
    rq->dWork = NULL;
    rc = 0;
    if (qzIsChainLevel(level)) { /* every item links the block before it in its own scratch */
        if (!sl->vdWork) sl->vdWork = qzstd_hip_malloc(sl->device, QZSTD_HIP_SVC_WORK_BYTES);
        rq->dWork = sl->vdWork;
        rc = sl->vdWork == NULL; /* (no scratch: as a request the service does not take) */
    }
    if (rc == 0) rc = qzstd_hip_service_submit(sl->device, level, rq);
    if (rc != 0) { /* > 0: the level is not served, the service is down or busy with another level; < 0: an error */
        memset(sl->vCount, 0xFF, nItems * sizeof(unsigned int)); /* nothing outstanding */
        if (rc < 0) QZ_LOG(1, "service request not queued: %s\n", qzstd_hip_last_error());
        goto notNow; /* the launch path may still work */
    }
    for (k = 0; progressive && k < nItems; k++) {
        const size_t from = k * itemBytes, upTo = (k + 1) * itemBytes < srcSize ? (k + 1) * itemBytes : srcSize;
        unsigned int expect = QZSTD_HIP_NSEQ_STAGING;
        memcpy(sl->vSrc + from, (const unsigned char *)src + from, upTo - from);
        if (k + 1 == nItems) memset(sl->vSrc + srcSize, 0, pad);
        /* "slice k is in": only a word that still says STAGING (a request the dispatcher handed back has REJECTED there) */
        (void)__atomic_compare_exchange_n(&sl->vCount[k], &expect, 0u, 0, __ATOMIC_RELEASE, __ATOMIC_RELAXED);
    }
    return 0;
notNow:
    qzReleaseSlot(c->slot);
    return -1;
}

/* Wait for count word k to leave 0; 1 = not within the time-out, or the service has left for good.  `naps`: the policy for an item being
 * worked on — busy for spinNs, then naps, every 1024 polls a poke (the service may have left with this request in its ring: it is
 * launched again; or for good: another request timed out).  Without: busy all the way (words of one wave store). */
static int qzSvcWordWait(const QZSTD_SvcCall_T *c, size_t k, int naps)
{
    const unsigned int *word = &c->sl->vCount[k];
    unsigned polls = 0;
    while (__atomic_load_n(word, __ATOMIC_ACQUIRE) == 0u) {
        __builtin_ia32_pause();
        if ((++polls & (naps ? 63u : 1023u)) == 0u) {
            const unsigned long dt = qzNowNs() - c->t0;
            if (dt > (unsigned long)gProc.timeoutMs * 1000000ul) return 1;
            if (!naps) continue;
            if ((polls & 1023u) == 0u && qzstd_hip_service_poke(c->sl->device, c->level) == 2 && __atomic_load_n(word, __ATOMIC_ACQUIRE) == 0u) return 1;
            if (dt > c->spinNs) { const struct timespec nap = { 0, dt < 20000000ul ? 5000 : 200000 }; nanosleep(&nap, NULL); }
        }
    }
    return 0;
}

/* Poll the count words in item order — the items finish roughly in that order (the later, the more history in front of it) — and JOIN
 * every item's list as it arrives: by the time the last item is in, the rest of the block's list stands.  Returns QZ_SVC_*. */
static int qzSvcCollect(QZSTD_SvcCall_T *c, QZSTD_Join_T *j, size_t outSeqsCapacity)
{
    const QZSTD_Slot_T *sl = c->sl;
    size_t k, m;
    int wrong = 0;
    c->t0 = qzNowNs();
    /* how long a waiting caller polls before it naps: with a core per caller polling is free and a nap costs its wake-up (level 1, 16 threads on
     * 16 cores: 12.7 GB/s polling 400 us, 10.5 napping at once); with more callers than cores a poller keeps another caller's entropy stage
     * off the core (32 threads: 9.5 GB/s polling 400 us, 14.2-14.6 polling 10 us or not at all; 48 threads: 5.6 against 15.1-15.5) */
    c->spinNs = (unsigned long)gProc.svcSpinUs * 1000ul;
    if (!gProc.svcSpinSet && __atomic_load_n(&gProc.liveStates, __ATOMIC_RELAXED) > qzUsableCores()) c->spinNs = 10000ul;
    for (k = 0; k < c->rq.nItems; k++) {
        unsigned int cnt;
        if (qzSvcWordWait(c, k, 1)) return QZ_SVC_TIMED_OUT;
        if (wrong) continue; /* (after a wrong item the rest is only waited for: the slot's buffers are in use until every count is in) */
        cnt = sl->vCount[k];
        if (cnt == QZSTD_HIP_NSEQ_REJECTED) {
            /* handed back whole: nothing of it was queued.  The dispatcher writes all nItems words with one wave store, but stores
             * to pinned host memory can land microseconds apart: the slot is given back only when every word is in — a word
             * landing later would be read by the slot's NEXT request as its own (round-3 ADVICE) */
            for (m = k + 1; m < c->rq.nItems; m++)
                if (qzSvcWordWait(c, m, 0)) return QZ_SVC_TIMED_OUT;
            return QZ_SVC_REJECTED;
        }
        if (cnt == QZSTD_HIP_NSEQ_ERROR || cnt > c->rq.seqCapPerItem || j->out + cnt >= outSeqsCapacity - 1) { wrong = 1; continue; } /* capacity rule, reference :1318-1322 */
        if (qzJoinPiece(j, sl->vSeqs + k * c->rq.seqCapPerItem, cnt, c->rq.epoch, c->t0) != 0) return QZ_SVC_TIMED_OUT; /* (entries later than t0 + the limit) */
    }
    return wrong ? QZ_SVC_WRONG : QZ_SVC_DONE;
}

/* the request was not answered within the time-out: what the service says about itself */
static void qzSvcLogTimeout(const QZSTD_SvcCall_T *c)
{
    unsigned long in[8] = { 0 }, dg[8] = { 0 };
    (void)qzstd_hip_service_info(c->sl->device, in);
    (void)qzstd_hip_service_debug(c->sl->device, dg);
    QZ_LOG(1, "device %d: service request not answered after %lu ms (limit %d; service: %lu launch(es), %lu request(s), state %lu; dispatcher: %lu poll(s), "
              "%lu request(s) taken, %lu item(s) queued; workers: %lu started, %lu item(s) picked up, %lu finished, %lu gave up on a slice; ring: %lu "
              "consumed, %lu reserved, quit %lu, frozen %lu; this request: %zu item(s), level %#x)\n",
           c->sl->device, (qzNowNs() - c->t0) / 1000000ul, gProc.timeoutMs, in[0], in[1], in[4], dg[0], dg[1], dg[2], dg[3], dg[4], dg[5], in[6], dg[6],
           dg[7] & 0x1FFFFFFFFFFFFFFFul, dg[7] >> 62, (dg[7] >> 61) & 1ul, (size_t)c->rq.nItems, (unsigned)c->level);
}

/* the answer does not add up to the block — which item: every item's own list adds up to its range */
static void qzSvcLogSum(const QZSTD_SvcCall_T *c, size_t sum, size_t srcSize)
{
    const QZSTD_Slot_T *sl = c->sl;
    const size_t nItems = c->rq.nItems, itemBytes = c->rq.itemBytes;
    size_t k;
    QZ_LOG(1, "service result does not add up: %zu of %zu bytes\n", sum, srcSize);
    for (k = 0; k < nItems; k++) {
        const ZSTD_Sequence *q = sl->vSeqs + k * c->rq.seqCapPerItem;
        const size_t from = k * itemBytes, upTo = (k + 1) * itemBytes < srcSize ? (k + 1) * itemBytes : srcSize;
        size_t isum = 0, j;
        for (j = 0; j < sl->vCount[k] && j < c->rq.seqCapPerItem; j++) isum += (size_t)q[j].litLength + q[j].matchLength;
        if (isum != upTo - from) QZ_LOG(1, "  item %zu of %zu: %u sequences cover %zu of %zu bytes\n", k, nItems, sl->vCount[k], isum, upTo - from);
    }
}

/* One block through the resident service (qzstd_hip_service_submit): no launch, no stream — one 64-byte request goes into the service's
 * ring, workgroups that are already resident parse the block as up to 32 work items (runs of whole segments) and write sequences and,
 * last, the counts into this slot's pinned memory.  Reference shape: synchronous submit + poll of one request on one DC instance,
 * src/qatseqprod.c:1243-1272.  Returns the count, the error code, or QZ_NOT_SERVED: the caller then takes the launch path. */
static size_t qzServiceBlock(QZSTD_Session_T *s, int dev, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity, const void *src,
                             size_t srcSize, int level)
{
    QZSTD_SvcCall_T c;
    QZSTD_Join_T j = { outSeqs, 0, 0, 0 };
    size_t out;
    int end;
    if (!gProc.service || srcSize == 0 || qzSvcQueue(&c, s->slotHint, dev, src, srcSize, level) != 0) return QZ_NOT_SERVED;
    end = qzSvcCollect(&c, &j, outSeqsCapacity);
    if (end == QZ_SVC_TIMED_OUT) { /* reference: the 2 s poll limit, :1261-1285 */
        qzSvcLogTimeout(&c);
        c.sl->vStuck = 1;
        qzstd_hip_service_mark_broken(c.sl->device);
        qzReleaseSlot(c.slot);
        /* the resident kernels are asked to leave and are not used again; THIS block is not lost: it goes through the batches
         * (whose own wait has the same limit: a device that is really wedged then returns the error, reference :1261-1285) */
        s->redoneAlone++;
        return QZ_NOT_SERVED;
    }
    if (end != QZ_SVC_DONE) {
        qzReleaseSlot(c.slot);
        if (end == QZ_SVC_REJECTED) return QZ_NOT_SERVED;
        qzCause = QZ_CAUSE_CAPACITY; /* QZ_SVC_WRONG */
        return ZSTD_SEQUENCE_PRODUCER_ERROR;
    }
    out = qzJoinFinish(&j);
    qzReleaseSlot(c.slot);
    /* what arrived has to add up to the block (a wrong result must never reach libzstd, which does not validate sequences by
     * default): the lengths were added up on the way */
    if (j.covered != srcSize) {
        qzSvcLogSum(&c, j.covered, srcSize);
        qzstd_hip_service_mark_broken(c.sl->device);
        qzCause = QZ_CAUSE_RUNTIME;
        return ZSTD_SEQUENCE_PRODUCER_ERROR;
    }
    s->servedService++;
    __atomic_fetch_add(&gProc.devBlocks[c.sl->device][2], 1ul, __ATOMIC_RELAXED);
    return out;
}

/* ---------------------------------------------------------------- announcement batcher -- */

/* frees (force) or tries to free the parked buffers whose streams have drained; scrubs the staged caller data first */
static void qzReapOrphans(int force)
{
    QZSTD_Orphan_T **pp;
    pthread_mutex_lock(&qzOrphanMu);
    for (pp = &qzOrphans; *pp; ) {
        QZSTD_Orphan_T *o = *pp;
        int k;
        if (!force && o->stream && qzstd_hip_stream_query(o->device, o->stream) != 0) { pp = &o->next; continue; }
        if (o->buf[0]) memset(o->buf[0], 0, o->srcCap);
        for (k = 0; k < 4; k++) qzstd_hip_host_free(o->buf[k]);
        *pp = o->next;
        free(o);
    }
    pthread_mutex_unlock(&qzOrphanMu);
}

/* the area's buffers may still be in use by a kernel that timed out on `stream`: park them, the area starts afresh at its next use */
static void qzOrphanArea(QZSTD_Area_T *a, int dev, void *stream)
{
    QZSTD_Orphan_T *o = (QZSTD_Orphan_T *)calloc(1, sizeof(*o));
    if (o) { /* (no memory for the list node: the buffers are leaked rather than freed under a running kernel) */
        o->buf[0] = a->hSrc; o->buf[1] = a->hSeqs; o->buf[2] = a->hCount; o->buf[3] = a->hDesc;
        o->srcCap = QZ_HB_SRC_BYTES;
        o->device = dev;
        o->stream = stream;
        pthread_mutex_lock(&qzOrphanMu);
        o->next = qzOrphans;
        qzOrphans = o;
        qzOrphanCount++;
        pthread_mutex_unlock(&qzOrphanMu);
    }
    a->hSrc = NULL; a->hSeqs = NULL; a->hCount = NULL; a->hDesc = NULL;
    a->dvSeqs = a->dvCount = a->dvDesc = a->dvSrc = NULL;
    a->seqsCap = 0;
    QZ_LOG(1, "device %d: a batch area's buffers are parked until a timed-out stream drains\n", dev);
}

/* every block of the area has published its count (called with the batcher's lock held) */
static int qzAreaDone(QZSTD_Area_T *a)
{
    if (!a->hCount) return 1;
    while (a->seen < a->nBlocks && __atomic_load_n(&a->hCount[a->seen], __ATOMIC_ACQUIRE) != QZ_COUNT_PENDING) a->seen++;
    return a->seen >= a->nBlocks;
}

/* a stream a launch may be queued on: nobody is queueing on it and it is not quarantined (a drained one is back in service) */
static int qzStreamUsable(QZSTD_Batcher_T *bt, int k)
{
    QZSTD_BStream_T *q = &bt->str[k];
    if (q->issuing) return 0;
    if (q->stuck) {
        if (qzStillStuck(bt->device, q->stream, &q->stuck)) return 0;
        q->last = -1; /* drained: whatever ran on it is over */
    }
    return 1;
}

/* free = usable, and its last launch has published every count word (not hipStreamQuery: see qzBlocksWait) */
static int qzStreamFree(QZSTD_Batcher_T *bt, int k)
{
    QZSTD_BStream_T *q = &bt->str[k];
    QZSTD_Area_T *a;
    if (!qzStreamUsable(bt, k)) return 0;
    if (q->last < 0) return 1;
    a = &bt->area[q->last];
    if (a->st != QZ_AREA_ISSUED || a->stream != k || qzAreaDone(a)) { q->last = -1; return 1; }
    return 0;
}

/* an area's pinned buffers, allocated WITHOUT the batcher's lock (pinned allocations take milliseconds) into `a`: next to the GPU of
 * the state that needs it first (`home`), as an announcement's own buffers were — the socket of the announcing threads, which stage
 * into it.  0 on success */
static int qzAreaAlloc(QZSTD_Area_T *a, int dev, int home)
{
    const size_t seqs = QZ_HB_ENTRIES * (gProc.hintCompact ? 8u : sizeof(ZSTD_Sequence));
    memset(a, 0, sizeof(*a));
    a->hSrc = (unsigned char *)qzHostAlloc(QZ_HB_SRC_BYTES, home, 0);
    a->hDesc = (qzstd_hip_block_t *)qzHostAlloc(QZ_HB_BLOCKS * sizeof(qzstd_hip_block_t), home, 0);
    a->hCount = (unsigned int *)qzHostAlloc(QZ_HB_BLOCKS * sizeof(unsigned int), home, 1);
    a->hSeqs = qzHostAlloc(seqs, home, 1);
    /* entries certify themselves by the area's tag, and fresh pinned pages may hold anything: tag 0 is never valid, the area starts wiped */
    if (a->hSeqs) memset(a->hSeqs, 0, seqs);
    a->dvSrc = a->hSrc ? qzstd_hip_host_device_ptr(a->hSrc) : NULL;
    a->dvDesc = a->hDesc ? qzstd_hip_host_device_ptr(a->hDesc) : NULL;
    a->dvCount = a->hCount ? qzstd_hip_host_device_ptr(a->hCount) : NULL;
    a->dvSeqs = a->hSeqs ? qzstd_hip_host_device_ptr(a->hSeqs) : NULL;
    if (!a->dvSrc || !a->dvDesc || !a->dvCount || !a->dvSeqs) {
        QZ_LOG(1, "device %d: no pinned memory for a batch area: %s\n", dev, qzstd_hip_last_error());
        QZ_HOST_FREE(a->hSrc); QZ_HOST_FREE(a->hDesc); QZ_HOST_FREE(a->hCount); QZ_HOST_FREE(a->hSeqs);
        memset(a, 0, sizeof(*a));
        return -1;
    }
    a->seqsCap = seqs;
    return 0;
}

/* a free area that has its buffers becomes the open one (lock held); its index, -2 if the free areas have no buffers yet, -1 if there
 * is no free area */
static int qzAreaOpen(QZSTD_Batcher_T *bt, int level, size_t block)
{
    QZSTD_Area_T *a;
    int k, bare = 0;
    for (k = 0; k < QZ_HB_AREAS && !(bt->area[k].st == QZ_AREA_FREE && bt->area[k].hSrc); k++) bare |= bt->area[k].st == QZ_AREA_FREE;
    if (k >= QZ_HB_AREAS) return bare ? -2 : -1;
    a = &bt->area[k];
    a->lap = (a->lap + 1u) & (gProc.hintCompact ? 0xFFFu : 0xFFFFFFu);
    a->staging = a->parts = 0;
    a->wipe = a->sealed = 0;
    if (a->lap == 0u) {
        /* the tag (12 bits packed, 24 unpacked) starts over: an entry no use of the last lap overwrote would show a valid tag again.
         * Nothing runs on the area here (every part of its last use let go): its result area is wiped once per lap — by the opener,
         * outside the lock, counted as one more stager so that the area is not issued before the wipe is done (qzBatchAdd) */
        a->lap = 1u;
        a->wipe = 1;
        a->staging = 1;
    }
    a->st = QZ_AREA_OPEN;
    a->level = level;
    a->block = block;
    a->nBlocks = a->seen = 0;
    a->srcUsed = a->entUsed = 0;
    a->stream = -1;
    a->stuck = 0;
    bt->open = k;
    return k;
}

/* every part of the area has let go (lock held): parked if a wait for it timed out, free again either way */
static void qzAreaRetire(QZSTD_Batcher_T *bt, int ai)
{
    QZSTD_Area_T *a = &bt->area[ai];
    int k;
    if (a->stuck) qzOrphanArea(a, bt->device, a->stream >= 0 ? bt->str[a->stream].stream : NULL);
    for (k = 0; k < QZ_HB_STREAMS_MAX; k++)
        if (bt->str[k].last == ai && !bt->str[k].stuck) bt->str[k].last = -1;
    a->st = QZ_AREA_FREE;
}

/* one copy-in of the area's staged bytes and one launch of its blocks, on stream q (lock NOT held); 0 on success */
static int qzLaunchArea(QZSTD_Session_T *s, QZSTD_Batcher_T *bt, QZSTD_Area_T *a, QZSTD_BStream_T *q)
{
    const int dev = bt->device;
    const size_t work = qzstd_hip_workspace_bytes(a->level, a->nBlocks, (unsigned int)a->block);
    unsigned long t0;
    int direct, rc;
    if (!q->stream && !(q->stream = qzstd_hip_stream_create(dev))) return -1;
    if (work && !(q->dWork = qzGrowDev(dev, q->dWork, &q->dWorkCap, work))) return -1;
    direct = gProc.hintDirect == 1 || (gProc.hintDirect == 2 && work == 0); /* (A/B switch, see hintDirect) */
    if (!direct) {
        if (!q->dSrc && !(q->dSrc = (unsigned char *)qzstd_hip_malloc(dev, QZ_HB_SRC_BYTES))) return -1;
        t0 = qzNowNs();
        /* the staging copy goes to device memory by a copy kernel on the stream (qzstd_hip_copy_in says why not by the runtime's copy) */
        rc = gProc.hintDirect != 3 ? qzstd_hip_copy_in(dev, q->stream, q->dSrc, a->dvSrc, a->srcUsed)
                                   : qzstd_hip_memcpy_h2d(dev, q->stream, q->dSrc, a->hSrc, a->srcUsed);
        if (s) s->hintCopyCallNs += qzNowNs() - t0;
        if (rc) return -1;
    }
    t0 = qzNowNs();
    rc = qzstd_hip_find_sequences(dev, q->stream, a->level, direct ? a->dvSrc : q->dSrc, (const qzstd_hip_block_t *)a->dvDesc, a->nBlocks,
                                  (unsigned int)a->block, a->dvSeqs, (unsigned int *)a->dvCount, q->dWork, q->dWorkCap);
    if (s) s->hintLaunchCallNs += qzNowNs() - t0;
    if (rc) return -1;
    __atomic_fetch_add(&gProc.devBlocks[dev][0], (unsigned long)a->nBlocks, __ATOMIC_RELAXED);
    __atomic_fetch_add(&bt->launches, 1ul, __ATOMIC_RELAXED);
    __atomic_fetch_add(&bt->blocks, (unsigned long)a->nBlocks, __ATOMIC_RELAXED);
    return 0;
}

/* nothing will publish the area's count words (it is not queued): its blocks' callbacks take the per-block path */
static void qzAreaFailCounts(QZSTD_Area_T *a)
{
    memset(a->hCount, 0xFF, a->nBlocks * sizeof(unsigned int)); /* QZSTD_HIP_NSEQ_ERROR, every word */
}

/* Issue a collecting area (lock held; held again on return): area `want`, or the open one when want < 0.  Not forced: only once its
 * staging is done and on a FREE stream, else it keeps collecting.  Forced (a callback or a drop needs its blocks) or sealed (full, or
 * another level or grid came): once its staging is done it is queued behind the launch of a busy stream if no stream is free; forced,
 * the caller waits for that staging. */
static void qzIssueOpen(QZSTD_Session_T *s, QZSTD_Batcher_T *bt, int force, int want)
{
    const int n = gProc.hintBatches;
    for (;;) {
        const int ai = want >= 0 ? want : bt->open;
        QZSTD_Area_T *a;
        int k, pick = -1, busy = 0, rc, go;
        if (ai < 0) return;
        a = &bt->area[ai];
        if (a->st != QZ_AREA_OPEN || a->nBlocks == 0) return; /* (issued meanwhile, or nothing in it yet) */
        if (a->staging > 0) {
            if (!force) return; /* the last announcer to finish staging comes back here */
            pthread_cond_wait(&bt->cv, &bt->mu);
            continue;
        }
        go = force || a->sealed;
        for (k = 0; k < n && pick < 0; k++)
            if (qzStreamFree(bt, (bt->nextStream + k) % n)) pick = (bt->nextStream + k) % n;
        for (k = 0; k < n && pick < 0 && go; k++) {
            const int j = (bt->nextStream + k) % n;
            if (bt->str[j].issuing) busy = 1;
            else if (qzStreamUsable(bt, j)) pick = j;
        }
        if (pick < 0 && !go) return;
        if (pick < 0 && busy) { /* another thread is queueing on the only usable streams: after it */
            pthread_cond_wait(&bt->cv, &bt->mu);
            continue;
        }
        if (bt->open == ai) {
            bt->open = -1;
            __atomic_store_n(&bt->pending, 0, __ATOMIC_RELAXED);
        }
        if (pick < 0) { /* every stream is quarantined: nothing will run these blocks */
            qzAreaFailCounts(a);
            a->st = QZ_AREA_ISSUED;
            QZ_LOG(1, "device %d: every batch stream is quarantined; a batch of %u blocks is not queued\n", bt->device, a->nBlocks);
            if (a->parts == 0) qzAreaRetire(bt, ai);
            return;
        }
        bt->nextStream = (pick + 1) % n;
        a->st = QZ_AREA_ISSUING;
        a->stream = pick;
        bt->str[pick].issuing = 1;
        pthread_mutex_unlock(&bt->mu);
        rc = qzLaunchArea(s, bt, a, &bt->str[pick]);
        pthread_mutex_lock(&bt->mu);
        if (rc) { /* never launched */
            qzAreaFailCounts(a);
            QZ_LOG(1, "device %d: a batch of announced blocks is not queued: %s\n", bt->device, qzstd_hip_last_error());
        }
        a->st = QZ_AREA_ISSUED;
        bt->str[pick].issuing = 0;
        bt->str[pick].last = ai;
        pthread_cond_broadcast(&bt->cv);
        if (a->parts == 0) qzAreaRetire(bt, ai);
        return;
    }
}

/* a caller passing by (a callback, a waiter) issues the open area if a stream has become free */
static void qzBatchPoke(QZSTD_Session_T *s, QZSTD_Batcher_T *bt)
{
    if (!__atomic_load_n(&bt->pending, __ATOMIC_RELAXED) || pthread_mutex_trylock(&bt->mu) != 0) return;
    qzIssueOpen(s, bt, 0, -1);
    pthread_mutex_unlock(&bt->mu);
}

/* blocks of announcement h that fit area a from block b on, at most `want` */
static size_t qzAreaFit(const QZSTD_Area_T *a, const QZSTD_Hint_T *h, size_t want)
{
    size_t n = QZ_HB_BLOCKS - a->nBlocks, bySrc, byEnt;
    bySrc = (QZ_HB_SRC_BYTES - a->srcUsed) / h->block; /* (a range is padded to 64 bytes: both ends of the room are multiples of 64, so n blocks
                                                       * that fit unpadded fit padded) */
    byEnt = (QZ_HB_ENTRIES - a->entUsed) / h->pitch;
    if (n > bySrc) n = bySrc;
    if (n > byEnt) n = byEnt;
    return n < want ? n : want;
}

/* the opener's wipe of an area it staged nothing into (lock NOT held) */
static void qzWipeArea(QZSTD_Session_T *s, QZSTD_Batcher_T *bt, int ai)
{
    QZSTD_Area_T *a = &bt->area[ai];
    memset(a->hSeqs, 0, a->seqsCap);
    pthread_mutex_lock(&bt->mu);
    if (--a->staging == 0) {
        pthread_cond_broadcast(&bt->cv);
        qzIssueOpen(s, bt, 0, ai);
    }
    pthread_mutex_unlock(&bt->mu);
}

/* Stage blocks [b0, b1) of announcement h into device dev's batcher, as one part per area they go to.  Blocks that find no room (no
 * free area, no part left) get a failed part: their callbacks take the per-block path. */
static void qzBatchAdd(QZSTD_Session_T *s, QZSTD_Hint_T *h, int dev, size_t b0, size_t b1, const unsigned char *src, int level, int stable)
{
    QZSTD_Batcher_T *bt = &gProc.hb[dev];
    size_t b = b0;
    while (b < b1 && h->nParts < QZ_HINT_PARTS) {
        QZSTD_Part_T *pt = &h->part[h->nParts];
        QZSTD_Area_T *a;
        size_t n, j, srcOff, entOff, bytes;
        unsigned int first;
        int ai, wipe;
        pthread_mutex_lock(&bt->mu);
        ai = bt->open;
        if (ai >= 0) {
            a = &bt->area[ai];
            if (a->nBlocks > 0 && (a->level != level || a->block != h->block || qzAreaFit(a, h, b1 - b) < b1 - b)) {
                /* another level or grid (one launch = one profile), or too full for this range: it goes as it is — sealed, so that the
                 * last of its stagers issues it, and this range opens the next area without waiting for them */
                a->sealed = 1;
                bt->open = -1;
                __atomic_store_n(&bt->pending, 0, __ATOMIC_RELAXED);
                if (a->staging == 0) qzIssueOpen(s, bt, 0, ai);
                pthread_mutex_unlock(&bt->mu);
                continue;
            }
            a->level = level; /* (an empty open area takes this range's level and grid) */
            a->block = h->block;
        } else if ((ai = qzAreaOpen(bt, level, h->block)) == -2) {
            /* the free areas have no buffers yet: made here, outside the lock, and given to one of them */
            QZSTD_Area_T fresh;
            int k;
            pthread_mutex_unlock(&bt->mu);
            if (qzAreaAlloc(&fresh, dev, s->slotHint % gProc.numDevices) != 0) break;
            pthread_mutex_lock(&bt->mu);
            for (k = 0; k < QZ_HB_AREAS && !(bt->area[k].st == QZ_AREA_FREE && !bt->area[k].hSrc); k++) {}
            if (k < QZ_HB_AREAS) {
                const unsigned int lap = bt->area[k].lap;
                bt->area[k] = fresh;
                bt->area[k].lap = lap;
                bt->areas++;
                fresh.hSrc = NULL;
            }
            pthread_mutex_unlock(&bt->mu);
            if (fresh.hSrc) { /* (another thread filled the last bare one meanwhile) */
                QZ_HOST_FREE(fresh.hSrc); QZ_HOST_FREE(fresh.hDesc); QZ_HOST_FREE(fresh.hCount); QZ_HOST_FREE(fresh.hSeqs);
            }
            continue;
        } else if (ai < 0) {
            pthread_mutex_unlock(&bt->mu);
            QZ_LOG(1, "device %d: no batch area free for an announcement\n", dev);
            break;
        }
        a = &bt->area[ai];
        wipe = a->wipe; /* (this thread opened it at the end of a lap: the wipe is its job) */
        a->wipe = 0;
        n = qzAreaFit(a, h, b1 - b);
        if (n == 0 || (n < b1 - b && h->nParts == QZ_HINT_PARTS - 1)) { /* (the last part: the rest as a failed one) */
            pthread_mutex_unlock(&bt->mu);
            if (wipe) qzWipeArea(s, bt, ai);
            break;
        }
        bytes = ((b + n) * h->block < h->size ? (b + n) * h->block : h->size) - b * h->block;
        first = a->nBlocks;
        srcOff = a->srcUsed;
        entOff = a->entUsed;
        a->nBlocks += (unsigned int)n;
        a->srcUsed += (bytes + 63) & ~(size_t)63;
        a->entUsed += n * h->pitch;
        a->staging++;
        a->parts++;
        __atomic_store_n(&bt->pending, 1, __ATOMIC_RELAXED);
        pthread_mutex_unlock(&bt->mu);

        if (wipe) memset(a->hSeqs, 0, a->seqsCap);
        /* pinned staging (reference: the staging memcpy, :1222-1227).  Streaming stores where the host will not read the copy back: a verified
         * announcement compares every callback's block with it (measured with the copy streamed out: -2 ... -4 %), a STABLE one only samples (+1.5 %) */
        if (stable) qzStageCopy(a->hSrc + srcOff, src + b * h->block, bytes);
        else memcpy(a->hSrc + srcOff, src + b * h->block, bytes);
        /* descriptors: results go straight into the area's pinned result area, h->pitch entries per block; a block with more sequences
         * reports an error and is redone by the per-block path when its callback comes */
        for (j = 0; j < n; j++) {
            const size_t o = (b + j) * h->block, len = h->size - o < h->block ? h->size - o : h->block;
            qzstd_hip_block_t *d = &a->hDesc[first + j];
            const size_t ent = entOff + j * h->pitch;
            d->srcOff = srcOff + j * h->block;
            d->seqOff = gProc.hintCompact ? ent / 2u : ent; /* (sixteen-byte units; the pitch is even) */
            d->srcLen = (unsigned int)len;
            d->seqCap = (unsigned int)h->pitch;
            d->parseFrom = 0;
            d->mark = gProc.hintCompact ? (a->lap | QZSTD_HIP_MARK_COMPACT) : a->lap; /* every entry certifies itself, see qzTakeMarked */
            a->hCount[first + j] = QZ_COUNT_PENDING; /* until its workgroup says otherwise */
            if (h->keys && h->nb <= h->keysCap) h->keys[b + j] = len >= 16 ? qzBlockKey(a->hSrc + d->srcOff, len) : 0ull;
        }
        pt->st = 1;
        pt->dev = dev;
        pt->area = ai;
        pt->first = first;
        pt->gen = gProc.gen;
        pt->b0 = pt->seen = b;
        pt->b1 = b + n;
        h->nParts++;
        b += n;

        pthread_mutex_lock(&bt->mu);
        a->staging -= 1 + wipe;
        if (a->staging == 0) {
            pthread_cond_broadcast(&bt->cv);
            qzIssueOpen(s, bt, 0, ai); /* the last one out issues it if a stream is free */
        }
        pthread_mutex_unlock(&bt->mu);
    }
    if (b < b1 && h->nParts < QZ_HINT_PARTS) {
        QZSTD_Part_T *pt = &h->part[h->nParts++];
        pt->st = 3;
        pt->area = -1;
        pt->b0 = pt->seen = b;
        pt->b1 = b1;
    }
}

/* the area and the index in it of block b of h; NULL when no part holds it (or the device layer has restarted since) */
static QZSTD_Area_T *qzHintBlock(const QZSTD_Hint_T *h, size_t b, unsigned int *idx)
{
    int k;
    for (k = 0; k < h->nParts; k++) {
        const QZSTD_Part_T *pt = &h->part[k];
        if (b < pt->b0 || b >= pt->b1) continue;
        if (pt->area < 0 || pt->gen != gProc.gen || !gProc.hb) return NULL;
        *idx = pt->first + (unsigned int)(b - pt->b0);
        return &gProc.hb[pt->dev].area[pt->area];
    }
    return NULL;
}

/* the staged copy of blocks [b, e) equals p: 1 equal, 0 different, -1 not all of them are staged */
static int qzHintSame(const QZSTD_Hint_T *h, size_t b, size_t e, const unsigned char *p)
{
    size_t bi;
    for (bi = b; bi < e; bi++) {
        unsigned int idx;
        const QZSTD_Area_T *a = qzHintBlock(h, bi, &idx);
        if (!a || !a->hSrc) return -1;
        if (memcmp(a->hSrc + a->hDesc[idx].srcOff, p + (bi - b) * h->block, a->hDesc[idx].srcLen) != 0) return 0;
    }
    return 1;
}

/* Completion of an announced launch WITHOUT the runtime (round 4): every workgroup publishes its block's count word — in the batch
 * area's pinned, coherent result area — with a system-scope release after all of its result stores (csrc/qzstd_kernels.hip,
 * qzstd_find_sequences_kernel), and the words start out as QZ_COUNT_PENDING.  A callback waits for ITS blocks only, by reading memory.
 * (hipStreamQuery on one of 48 streams folded onto 16 hardware queues waits for whatever was queued behind the launch it asks about:
 * with the stream waits a worker of the batch front-end spent 30 % of its time waiting for launches that had long finished.)
 * Count words [i0, i1): 0 = all published, 1 = not within the time-out.  A waiter passing by issues its batcher's open area when a
 * stream has become free. */
static int qzBlocksWait(QZSTD_Session_T *s, QZSTD_Batcher_T *bt, const unsigned int *cnt, size_t i0, size_t i1)
{
    const unsigned long t0 = qzNowNs(), limit = (unsigned long)gProc.timeoutMs * 1000000ul;
    /* 50 us of polling, then naps: a waiting caller does not burn a core others could entropy-code on; with far more callers than
     * cores (states alive > 1.5 x usable cores) no polling at all (front-end, 64 workers on 16 cores: 4.4 GB/s polling).
     * Decided once, at the first miss (round-4 ADVICE: not by how long the first scan happened to take) */
    unsigned long spinNs = 50000ul;
    int decided = 0;
    size_t i = i0;
    for (;;) {
        unsigned long el;
        while (i < i1 && __atomic_load_n(&cnt[i], __ATOMIC_ACQUIRE) != QZ_COUNT_PENDING) i++;
        if (i >= i1) return 0;
        if (!decided) { /* at the first miss, whenever that is */
            decided = 1;
            if (2 * __atomic_load_n(&gProc.liveStates, __ATOMIC_RELAXED) > 3 * qzUsableCores()) spinNs = 0ul;
        }
        el = qzNowNs() - t0;
        if (el > limit) {
            qzCause = QZ_CAUSE_TIMEOUT;
            QZ_LOG(1, "announcement: a block is still not published after %d ms\n", gProc.timeoutMs);
            return 1;
        }
        if (el > spinNs) {
            const struct timespec nap = { 0, el < 20000000ul ? 20000l : 200000l };
            qzBatchPoke(s, bt);
            nanosleep(&nap, NULL);
        }
    }
}

/* Wait for blocks [w0, w1) of part pt (announcement block numbers), issuing its batch first if it is still collecting.  0 = there;
 * -1 = the part failed (3): a wait for its batch timed out — which fails every part of the batch — or the device layer restarted. */
static int qzPartWait(QZSTD_Session_T *s, QZSTD_Part_T *pt, size_t w0, size_t w1)
{
    QZSTD_Batcher_T *bt;
    QZSTD_Area_T *a;
    int stuck;
    if (pt->st != 1) return pt->st == 2 ? 0 : -1;
    if (pt->gen != gProc.gen || !gProc.hb) { pt->st = 3; pt->area = -1; return -1; }
    bt = &gProc.hb[pt->dev];
    a = &bt->area[pt->area];
    if (w0 < pt->seen) w0 = pt->seen;
    pthread_mutex_lock(&bt->mu);
    if (a->st == QZ_AREA_OPEN) qzIssueOpen(s, bt, 1, pt->area); /* (nothing strands in a batch that is still collecting) */
    stuck = a->stuck;
    pthread_mutex_unlock(&bt->mu);
    if (!stuck && (w0 >= w1 || qzBlocksWait(s, bt, a->hCount, pt->first + (w0 - pt->b0), pt->first + (w1 - pt->b0)) == 0)) {
        while (pt->seen < pt->b1 && __atomic_load_n(&a->hCount[pt->first + (pt->seen - pt->b0)], __ATOMIC_ACQUIRE) != QZ_COUNT_PENDING) pt->seen++;
        if (pt->seen >= pt->b1) pt->st = 2;
        return 0;
    }
    pthread_mutex_lock(&bt->mu);
    if (!a->stuck) {
        a->stuck = 1; /* its kernel may still read and write the area: parked when the last part lets go */
        if (a->stream >= 0) bt->str[a->stream].stuck = 1; /* not used before it has drained */
        QZ_LOG(1, "device %d: a batch of %u announced blocks timed out: %s\n", bt->device, a->nBlocks, qzstd_hip_last_error());
    }
    pthread_mutex_unlock(&bt->mu);
    pt->st = 3;
    return -1;
}

/* the part lets go of its area (waited for, or failed) */
static void qzPartRelease(QZSTD_Part_T *pt)
{
    if (pt->st != 0 && pt->area >= 0 && pt->gen == gProc.gen && gProc.hb) {
        QZSTD_Batcher_T *bt = &gProc.hb[pt->dev];
        pthread_mutex_lock(&bt->mu);
        if (--bt->area[pt->area].parts == 0 && bt->area[pt->area].st == QZ_AREA_ISSUED) qzAreaRetire(bt, pt->area);
        pthread_mutex_unlock(&bt->mu);
    }
    pt->area = -1;
    pt->st = 0;
}

/* drop an announcement: wait for what is still in flight (or in a batch still collecting: issued first), then let go of the areas */
static void qzHintDrop(QZSTD_Hint_T *h)
{
    int k;
    for (k = 0; k < h->nParts; k++) {
        if (h->part[k].st == 1) (void)qzPartWait(NULL, &h->part[k], h->part[k].b0, h->part[k].b1);
        qzPartRelease(&h->part[k]);
    }
    h->nParts = 0;
    h->st = 0;
    h->touched = 0;
    h->misses = 0;
}

static void qzFreeBatcher(QZSTD_Batcher_T *bt)
{
    int k;
    QZ_LOG(2, "device %d: %lu announced block(s) in %lu launch(es), %lu batch area(s)\n", bt->device, bt->blocks, bt->launches, bt->areas);
    for (k = 0; k < QZ_HB_STREAMS_MAX; k++) {
        QZSTD_BStream_T *q = &bt->str[k];
        if (q->stream) (void)qzstd_hip_stream_wait(bt->device, q->stream, (unsigned)gProc.timeoutMs);
        QZ_DEV_FREE(bt->device, q->dSrc); QZ_DEV_FREE(bt->device, q->dWork);
    }
    for (k = 0; k < QZ_HB_AREAS; k++) {
        QZSTD_Area_T *a = &bt->area[k];
        if (a->hSrc) memset(a->hSrc, 0, QZ_HB_SRC_BYTES); /* staged caller data: scrubbed before the pages go back */
        QZ_HOST_FREE(a->hSrc); QZ_HOST_FREE(a->hDesc); QZ_HOST_FREE(a->hCount); QZ_HOST_FREE(a->hSeqs);
    }
    for (k = 0; k < QZ_HB_STREAMS_MAX; k++)
        if (bt->str[k].stream) qzstd_hip_stream_destroy(bt->device, bt->str[k].stream);
    pthread_mutex_destroy(&bt->mu);
    pthread_cond_destroy(&bt->cv);
}

/* ---------------------------------------------------------------- announcements -- */

/* Serving a callback from an announcement: (src, srcSize) must start on an announced block grid and cover one or more whole blocks of it
 * (libzstd 1.5.7 cuts multi-block frames into blocks of 32..128 KiB at 32 KiB steps, so a finer grid serves several sizes: neighbours are
 * joined).  Its bytes must still equal the staged copy the sequences were computed from: one memcmp per callback, a mismatch drops the
 * announcement — unless the announcer promised to hold them still (QZSTD_HINT_STABLE): then every block is served ONCE, going forward. */

/* the state's live announcements, newest first (an older one that names the same addresses never shadows a newer one); returns how many */
static int qzHintOrder(const QZSTD_Session_T *s, int order[QZ_HINTS])
{
    int n = 0, k;
    for (k = 0; k < QZ_HINTS; k++) { /* insertion sort of at most four */
        int j = n;
        if (s->hint[k].st == 0) continue;
        while (j > 0 && (int)(s->hint[order[j - 1]].seq - s->hint[k].seq) < 0) { order[j] = order[j - 1]; j--; }
        order[j] = k;
        n++;
    }
    return n;
}

/* the grid blocks [b, e) of announcement h that a callback asks for; rel: its offset in the announced buffer; byAddr: found by address */
typedef struct { QZSTD_Hint_T *h; size_t b, e, rel; int byAddr; } QZSTD_HintHit_T;

/* Does announcement k hold the callback's bytes?  0 = not here (another level, off its grid, unknown content, or dropped here: a STABLE
 * block asked for again, bytes that changed); else *hit says where: 1 = all staged, -1 = not all of them (a part found no room). */
static int qzHintFind(QZSTD_Session_T *s, int k, const unsigned char *p, size_t srcSize, int level, QZSTD_HintHit_T *hit)
{
    QZSTD_Hint_T *h = &s->hint[k];
    size_t b, e, covered = 0;
    int same = 1;
    if (h->st == 0 || h->level != level) return 0;
    hit->h = h;
    hit->byAddr = !h->noAddr && p >= h->base && p + srcSize <= h->base + h->size;
    if (hit->byAddr) { /* by address: the callback names announced memory */
        hit->rel = (size_t)(p - h->base);
        b = hit->rel / h->block;
        if (hit->rel % h->block != 0 || b >= h->nb) return 0; /* off the grid (libzstd 1.5.7 pre-splits multi-block frames at 32 KiB steps): not served from here */
        for (e = b; e < h->nb && covered < srcSize; e++) covered += h->size - e * h->block < h->block ? h->size - e * h->block : h->block;
        if (covered != srcSize || e - b > 8) {
            QZ_LOG(3, "announcement %d: block %zu+%zu does not fit the grid (%zu)\n", k, hit->rel, srcSize, h->block);
            return 0;
        }
        if (h->stable && b < h->servedUpTo) {
            /* a block of a STABLE announcement asked for a second time: the buffer is being used again (a new job over the
             * same memory whose last callbacks never came) — nothing vouches for its bytes any more */
            QZ_LOG(2, "announcement %d: block %zu asked for again; dropped\n", k, b);
            qzHintDrop(h);
            return 0;
        }
        /* verified: every callback; STABLE: every 16th block served, a sampled check of the announcer's promise (QZSTD_hintBroken) */
        if ((!h->stable || (++s->stableSampler & 15u) == 0u) && (same = qzHintSame(h, b, e, p)) == 0) {
            QZ_LOG(h->stable ? 1 : 2, "announcement %d: the buffer changed after it was announced%s; dropped\n", k,
                   h->stable ? " although it was announced with QZSTD_HINT_STABLE" : "");
            if (h->stable) s->stableBroken++;
            qzHintDrop(h);
            return 0;
        }
    } else {
        /* by content: a streaming caller (ZSTD_compressStream2 with small feeds, the zstd CLI) announces the buffer it
         * read into, but libzstd hands the producer blocks out of its OWN window buffer.  An announced grid block with
         * the same size, the same first and last 8 bytes and — verified — the same bytes serves such a callback
         * just as well (the sequences depend on nothing but the block's bytes). */
        unsigned long long key;
        if (srcSize < 16 || h->nb > QZ_CONTENT_LOOKUP_BLOCKS || !h->keys) return 0;
        key = qzBlockKey(p, srcSize);
        for (b = 0; b < h->nb; b++)
            if (h->keys[b] == key && (h->size - b * h->block < h->block ? h->size - b * h->block : h->block) == srcSize &&
                qzHintSame(h, b, b + 1, p) == 1) break;
        if (b >= h->nb) return 0;
        hit->rel = b * h->block;
        e = b + 1;
    }
    hit->b = b; hit->e = e;
    return same < 0 ? -1 : 1;
}

/* Serve the callback from the blocks found (ok: all of them were staged).  Returns the sequence count, 0 when they cannot be served (a
 * failed or timed-out part, a block with too many sequences): the per-block path then takes THIS block. */
static size_t qzHintServe(QZSTD_Session_T *s, const QZSTD_HintHit_T *hit, int ok, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity, size_t srcSize)
{
    QZSTD_Hint_T *h = hit->h;
    const size_t b = hit->b, e = hit->e;
    const int last = hit->byAddr && hit->rel + srcSize >= h->size; /* (a block served by content says nothing about where the announcer is) */
    QZSTD_Join_T j = { outSeqs, 0, 0, 0 };
    size_t held = 0, total = 1, bi;
    int pi;
    for (pi = 0; pi < h->nParts; pi++) { /* the parts that hold these blocks */
        QZSTD_Part_T *pt = &h->part[pi];
        const size_t w0b = b > pt->b0 ? b : pt->b0, w1b = e < pt->b1 ? e : pt->b1;
        if (w0b >= w1b) continue;
        held += w1b - w0b;
        if (pt->st == 1) {
            const unsigned long w0 = qzNowNs();
            (void)qzPartWait(s, pt, w0b, w1b);
            s->hintWaitNs += qzNowNs() - w0;
        }
        if (pt->st != 1 && pt->st != 2) ok = 0;
    }
    if (held != e - b) ok = 0;
    for (bi = b; bi < e && ok; bi++) { /* the capacity rule (reference :1318-1322), before anything is copied */
        unsigned int idx;
        const QZSTD_Area_T *a = qzHintBlock(h, bi, &idx);
        const size_t count = a ? a->hCount[idx] : QZSTD_HIP_NSEQ_ERROR;
        if (count == QZSTD_HIP_NSEQ_ERROR || count == 0 || count > h->pitch) { ok = 0; break; }
        total += count - 1;
    }
    if (total >= outSeqsCapacity - 1) ok = 0;
    for (bi = b; bi < e && ok; bi++) { /* completed by its count word: a block's entries certify themselves one by one */
        unsigned int idx;
        const QZSTD_Area_T *a = qzHintBlock(h, bi, &idx);
        const qzstd_hip_block_t *d = &a->hDesc[idx];
        if (qzJoinPiece(&j, (const unsigned char *)a->hSeqs + d->seqOff * 16u, a->hCount[idx], d->mark, 0ul) != 0) { /* (seqOff: sixteen-byte units) */
            QZ_LOG(1, "announcement: entries of block %zu did not arrive within %d ms of their count\n", bi, gProc.timeoutMs);
            ok = 0;
        }
    }
    if (hit->byAddr && e > h->servedUpTo) h->servedUpTo = e;
    if (!ok) {
        /* announced but not served: the announcement lives on for its other blocks unless this was the last one.  (Round 5 ended a
         * STABLE announcement here, waiting for every launch still in flight: one dense block — more sequences than the result pitch
         * holds — then cost the rest of a 2-4 MiB claim its announcement, a cliff on short-match data (round-5 ADVICE).  Its life is
         * bounded without that: QZSTD_dropHints at the end of the announcer's job, the asked-twice rule, the overlap rule of
         * QZSTD_hintSourceEx.) */
        if (last) qzHintDrop(h);
        return 0;
    }
    s->servedFromBatch++;
    h->touched = 1;
    h->misses = 0;
    if (last) qzHintDrop(h); /* last block consumed */
    return qzJoinFinish(&j);
}

/* announcements the caller has walked away from (used, then missed again and again) are dropped, so that they do not serve stale positions */
static void qzHintReapStale(QZSTD_Session_T *s)
{
    int k;
    for (k = 0; k < QZ_HINTS; k++) {
        QZSTD_Hint_T *h = &s->hint[k];
        if (h->st != 0 && (h->touched || h->noAddr) && ++h->misses > QZ_HINT_STALE_MISSES) {
            QZ_LOG(2, "announcement %d: abandoned by the caller; dropped\n", k);
            qzHintDrop(h);
        }
    }
}

/* Stage a buffer into the announcement batchers and remember it in *h (asynchronous, see QZSTD_hintSource).  The blocks are split
 * into contiguous ranges, one per GPU (reference analogue: instances interleaved across devices, src/qatseqprod.c:601-630), each
 * staged into its GPU's open batch area and launched with whatever else that batch collects; the results land in the area's pinned
 * buffers.  Returns the bytes announced, 0 if none. */
static size_t qzAnnounce(QZSTD_Session_T *s, QZSTD_Hint_T *h, const void *src, size_t srcSize, size_t blockSize,
                         int compressionLevel, int stable)
{
    size_t nb;
    unsigned long tq, tp;
    int parts, k, firstDev;

    tp = qzNowNs();
    qzHintDrop(h); /* an old announcement that was never consumed */
    s->hintDropNs += qzNowNs() - tp;
    if (qzOrphans) qzReapOrphans(0);
    nb = (srcSize + blockSize - 1) / blockSize;
    /* a fine grid means many blocks: the result area is sized by what a block of that size can produce at most */
    h->pitch = qzstd_hip_sequence_bound(blockSize) < QZ_HINT_PITCH ? qzstd_hip_sequence_bound(blockSize) : QZ_HINT_PITCH;
    h->pitch = (h->pitch + 1u) & ~(size_t)1; /* (even: a block's region of packed entries is pitch / 2 sixteen-byte units long) */

    if (s->slotHint < 0) s->slotHint = qzPickHint(); /* the state's own GPU: sticky from its first use */
    firstDev = s->slotHint % gProc.numDevices;
    tp = qzNowNs();
    if (nb <= QZ_CONTENT_LOOKUP_BLOCKS && h->keysCap < nb) {
        free(h->keys);
        h->keys = (unsigned long long *)malloc(nb * sizeof(*h->keys));
        h->keysCap = h->keys ? nb : 0;
    }
    s->hintPrepNs += qzNowNs() - tp;
    tq = qzNowNs();
    h->base = (const unsigned char *)src;
    h->size = srcSize;
    h->block = blockSize;
    h->level = compressionLevel;
    h->nb = nb;
    /* contiguous block ranges, one per GPU, starting at this state's own GPU; a range is worth a launch from 4 blocks */
    parts = gProc.split;
    if ((size_t)parts > nb / 4) parts = nb / 4 ? (int)(nb / 4) : 1;
    h->nParts = 0;
    for (k = 0; k < parts; k++) {
        const size_t b0 = nb * (size_t)k / (size_t)parts, b1 = nb * (size_t)(k + 1) / (size_t)parts;
        const int dev = parts > 1 ? (firstDev + k) % gProc.numDevices : firstDev;
        qzBatchAdd(s, h, dev, b0, b1, (const unsigned char *)src, compressionLevel | gProc.levelFlags, stable);
    }
    h->st = 1;
    h->touched = 0;
    h->misses = 0;
    h->stable = 0;
    h->servedUpTo = 0;
    h->seq = ++s->hintSeq;
    s->hintStageNs += qzNowNs() - tq; /* (staging and queueing are one step now: an announcer stages straight into its batch) */
    return srcSize;
}

/* Lifetime of an announcement (round-4 ADVICE): it ends when the callback of its last block has come, when a callback finds its bytes
 * changed (verified announcements) or asks for a block a second time (STABLE ones), when its LAST block could not be served,
 * when a new announcement names addresses it covers (STABLE: at once; verified: it stops serving by address and lives on for
 * by-content look-ups), after 16 callbacks in a row that it could not serve, at QZSTD_dropHints(), and with its state.  At most
 * four are alive per state. */
int QZSTD_hintSourceEx(void *sequenceProducerState, const void *src, size_t srcSize, size_t blockSize,
                       int compressionLevel, unsigned int flags)
{
    QZSTD_Session_T *s = (QZSTD_Session_T *)sequenceProducerState;
    QZSTD_Hint_T *h = NULL;
    int k, inflight = 0;

    /* the grid: 1 KiB (libzstd's smallest ZSTD_c_maxBlockSize) .. 128 KiB, a multiple of 16 */
    if (!s || !src || srcSize == 0 || srcSize > QZ_HINT_MAX_BYTES || blockSize < 1024 || blockSize > QZSTD_HIP_BLOCK_MAX ||
        (blockSize & 15))
        return -1;
    if (compressionLevel < QZ_LEVEL_MIN || compressionLevel > QZ_LEVEL_MAX || (flags & ~(unsigned int)QZSTD_HINT_STABLE)) return -1;
    if (!qzDeviceUsable(s)) return -1;
    /* an older announcement over (some of) the same addresses is void from here on: whatever it says about them is not what the
     * caller is announcing now */
    for (k = 0; k < QZ_HINTS; k++) {
        QZSTD_Hint_T *o = &s->hint[k];
        if (o->st == 0 || !((const unsigned char *)src < o->base + o->size && o->base < (const unsigned char *)src + srcSize)) continue;
        /* A STABLE one goes (nothing but its announcer's word vouches for its bytes).  A verified one only stops serving BY ADDRESS: a
         * streaming caller that refills and announces the same input buffer again (ZSTD_compressStream2, the zstd CLI) is served by
         * content out of libzstd's window — every such block is compared with the staged copy — and still needs the tail blocks of the
         * older announcement; dropping it also meant a synchronous wait for its launches on every announcement (round-5 ADVICE).  It
         * ends as every announcement does: consumed, stale after 16 misses, pushed out by the fourth newer one, QZSTD_dropHints. */
        if (o->stable || o->nb > QZ_CONTENT_LOOKUP_BLOCKS || !o->keys) qzHintDrop(o);
        else o->noAddr = 1;
    }
    /* an empty place of the ring first (starting where the last announcement left off); only when all four are alive the oldest goes */
    for (k = 0; k < QZ_HINTS && !h; k++)
        if (s->hint[(s->hintNext + k) % QZ_HINTS].st == 0) h = &s->hint[(s->hintNext + k) % QZ_HINTS];
    if (!h) {
        h = &s->hint[0];
        for (k = 1; k < QZ_HINTS; k++)
            if ((int)(s->hint[k].seq - h->seq) < 0) h = &s->hint[k];
    }
    s->hintNext = (int)((h - s->hint) + 1) % QZ_HINTS;
    if (qzAnnounce(s, h, src, srcSize, blockSize, compressionLevel, (flags & QZSTD_HINT_STABLE) != 0) == 0) return -1;
    for (k = 0; k < h->nParts; k++) inflight += h->part[k].st == 1;
    if (!inflight) { /* nothing could be queued */
        qzHintDrop(h);
        return -1;
    }
    h->stable = (flags & QZSTD_HINT_STABLE) != 0;
    h->noAddr = 0;
    s->hintCalls++;
    if (s->hintCalls == 8) /* the event log's timers: steady state only (the first announcements allocate pinned buffers and create streams) */
        s->hintStageNs = s->hintWaitNs = s->hintCopyCallNs = s->hintLaunchCallNs = s->hintPrepNs = s->hintDropNs = 0;
    return 0;
}

int QZSTD_hintSource(void *sequenceProducerState, const void *src, size_t srcSize, size_t blockSize,
                     int compressionLevel)
{
    return QZSTD_hintSourceEx(sequenceProducerState, src, srcSize, blockSize, compressionLevel, 0u);
}

/* the announcer is done with what it announced (end of a job; before it frees or rewrites a buffer it promised to hold still):
 * every announcement of the state ends here — launches in flight are waited for, nothing is served from them afterwards */
void QZSTD_dropHints(void *sequenceProducerState)
{
    QZSTD_Session_T *s = (QZSTD_Session_T *)sequenceProducerState;
    int k;
    if (!s) return;
    for (k = 0; k < QZ_HINTS; k++)
        if (s->hint[k].st != 0) qzHintDrop(&s->hint[k]);
}

/* ---------------------------------------------------------------- lifecycle ------ */

/* Enumerate GPUs and lay the slots out round-robin across them, so that threads whose
 * hints are consecutive land on different devices (reference: the instance shuffle of
 * QZSTD_getAndShuffleInstance, :601-630). */
static int qzBuildSlots(void)
{
    int nDev = qzstd_hip_device_count();
    int perDev, i, b, maxDev;
    if (nDev <= 0) return QZSTD_FAIL;
    maxDev = qzEnvInt("QZSTD_HIP_MAX_DEVICES", QZ_MAX_DEVICES, 1, QZ_MAX_DEVICES);
    if (nDev > maxDev) nDev = maxDev;
    perDev = qzEnvInt("QZSTD_HIP_SLOTS", QZ_DEFAULT_SLOTS_PER_DEVICE, 1, QZ_MAX_SLOTS / nDev);
    gProc.slots = (QZSTD_Slot_T *)calloc((size_t)nDev * perDev, sizeof(QZSTD_Slot_T));
    if (!gProc.slots) return QZSTD_FAIL;
    gProc.numDevices = nDev;
    gProc.numSlots = nDev * perDev;
    memset(gProc.devBlocks, 0, sizeof(gProc.devBlocks));
    for (i = 0; i < gProc.numSlots; i++) gProc.slots[i].device = i % nDev;
    gProc.numa = qzEnvInt("QZSTD_HIP_NUMA", 1, 0, 1);
    gProc.numaThreadNode = qzEnvInt("QZSTD_HIP_NUMA_NODE", -1, -1, 1023);
    memset(gProc.nodeNext, 0, sizeof(gProc.nodeNext));
    gProc.anyNext = 0;
    for (i = 0; i < nDev && i < QZ_MAX_DEVICES; i++) {
        gProc.devNode[i] = qzstd_hip_device_numa_node(i);
        QZ_LOG(2, "device %d: host NUMA node %d\n", i, gProc.devNode[i]);
    }
    gProc.coalesce = qzEnvInt("QZSTD_HIP_COALESCE", 1, 0, 1);
    gProc.split = qzEnvInt("QZSTD_HIP_SPLIT", nDev < QZ_HINT_PARTS ? nDev : QZ_HINT_PARTS, 1, nDev < QZ_HINT_PARTS ? nDev : QZ_HINT_PARTS);
    gProc.coal = (QZSTD_Coalescer_T *)calloc((size_t)nDev, sizeof(QZSTD_Coalescer_T));
    if (!gProc.coal) return QZSTD_FAIL;
    for (i = 0; i < nDev; i++) {
        gProc.coal[i].device = i;
        gProc.coal[i].open = -1;
        pthread_mutex_init(&gProc.coal[i].mu, NULL);
        pthread_cond_init(&gProc.coal[i].cvOpen, NULL);
        for (b = 0; b < QZ_BATCHES; b++) {
            pthread_cond_init(&gProc.coal[i].batch[b].cvLead, NULL);
            pthread_cond_init(&gProc.coal[i].batch[b].cvDone, NULL);
        }
    }
    gProc.hb = (QZSTD_Batcher_T *)calloc((size_t)nDev, sizeof(QZSTD_Batcher_T));
    if (!gProc.hb) return QZSTD_FAIL;
    for (i = 0; i < nDev; i++) {
        gProc.hb[i].device = i;
        gProc.hb[i].open = -1;
        pthread_mutex_init(&gProc.hb[i].mu, NULL);
        pthread_cond_init(&gProc.hb[i].cv, NULL);
        for (b = 0; b < QZ_HB_STREAMS_MAX; b++) gProc.hb[i].str[b].last = -1;
    }
    return QZSTD_OK;
}

int QZSTD_startQatDevice(void)
{
    int status;
    pthread_mutex_lock(&gProc.mutex);
    {
        const char *dbg = getenv("QZSTD_HIP_DEBUG");
        const char *rep = getenv("QZSTD_HIP_EXT_REPCODES");
        if (dbg && *dbg) qzLogLevel = atoi(dbg);
        /* the caller promises ZSTD_c_searchForExternalRepcodes = enable on its CCtx (libzstd's default only
         * from level 10): repeat-offset aware sequences at every level */
        gProc.levelFlags = (rep && atoi(rep) > 0) ? QZSTD_HIP_LEVEL_REPCODES : 0;
        gProc.timeoutMs = qzEnvInt("QZSTD_HIP_TIMEOUT_MS", QZ_DEFAULT_TIMEOUT_MS, 1, 600000);
        gProc.splitBlocks = qzEnvInt("QZSTD_HIP_SPLIT_BLOCKS", 1, 0, 1);
        gProc.service = qzEnvInt("QZSTD_HIP_SERVICE", 1, 0, 1);
        gProc.svcItemBytes = qzEnvInt("QZSTD_HIP_SERVICE_ITEM", 4096, 4096, (int)QZSTD_HIP_BLOCK_MAX) & ~4095;
        gProc.svcSpinUs = qzEnvInt("QZSTD_HIP_SERVICE_SPIN_US", 400, 0, 1000000);
        gProc.svcSpinSet = getenv("QZSTD_HIP_SERVICE_SPIN_US") != NULL;
        /* announcements: PACKED result entries (qzstd_hip.h: QZSTD_HIP_MARK_COMPACT) — 8 bytes per sequence over PCIe instead of 16 (round 6: the
         * level-1 kernel ran at the bus's write rate).  0 = 16-byte entries (A/B) */
        gProc.hintCompact = qzEnvInt("QZSTD_HIP_HINT_COMPACT", 1, 0, 1);
        /* announcement launches in flight per GPU (the batcher's streams): the runtime's default hardware queue count */
        gProc.hintBatches = qzEnvInt("QZSTD_HIP_HINT_BATCHES", 4, 1, QZ_HB_STREAMS_MAX);
        gProc.stageNt = qzEnvInt("QZSTD_HIP_STAGE_NT", 1, 0, 1);
        gProc.hintDirect = qzEnvInt("QZSTD_HIP_HINT_DIRECT", 0, 0, 3);
        (void)qzUsableCores(); /* (read once here, under the process mutex: the waits only load it) */
    }
    if (gProc.status == QZSTD_FAIL) {
        /* runtime up? (reference: QZSTD_salUserStart, :498-527) */
        gProc.status = qzstd_hip_device_count() > 0 ? QZSTD_STARTED : QZSTD_FAIL;
        if (gProc.status == QZSTD_FAIL) QZ_LOG(2, "no usable HIP device: %s\n", qzstd_hip_last_error());
    }
    if (gProc.status == QZSTD_STARTED) {
        gProc.status = qzBuildSlots() == QZSTD_OK ? QZSTD_OK : QZSTD_STARTED;
    }
    QZ_LOG(2, "start: status %d, %d device(s), %d slot(s)\n", gProc.status, gProc.numDevices, gProc.numSlots);
    status = gProc.status;
    pthread_mutex_unlock(&gProc.mutex);
    return status;
}

void QZSTD_stopQatDevice(void)
{
    int i;
    pthread_mutex_lock(&gProc.mutex);
    for (i = 0; i < gProc.numDevices; i++) (void)qzstd_hip_service_stop(i); /* the resident kernels leave before anything is freed */
    if (gProc.slots) {
        for (i = 0; i < gProc.numSlots; i++) qzFreeSlot(&gProc.slots[i]); /* waits (bounded) for each stream */
        free(gProc.slots);
    }
    if (gProc.hb) {
        for (i = 0; i < gProc.numDevices; i++) qzFreeBatcher(&gProc.hb[i]); /* waits (bounded) for each stream */
        free(gProc.hb);
    }
    gProc.hb = NULL;
    qzReapOrphans(1); /* (after the bounded waits for the streams the parked areas' kernels ran on) */
    gProc.gen++; /* parts staged so far refer to nothing any more */
    if (gProc.coal) {
        for (i = 0; i < gProc.numDevices; i++) qzFreeCoalescer(&gProc.coal[i]);
        free(gProc.coal);
    }
    gProc.coal = NULL;
    gProc.slots = NULL;
    gProc.numSlots = 0;
    gProc.numDevices = 0;
    gProc.status = QZSTD_FAIL;
    pthread_mutex_unlock(&gProc.mutex);
}

void *QZSTD_createSeqProdState(void)
{
    QZSTD_Session_T *s = (QZSTD_Session_T *)calloc(1, sizeof(QZSTD_Session_T));
    if (!s) return NULL;
    s->slotHint = -1;
    __atomic_fetch_add(&gProc.liveStates, 1, __ATOMIC_RELAXED);
    return s;
}

void QZSTD_freeSeqProdState(void *sequenceProducerState)
{
    QZSTD_Session_T *s = (QZSTD_Session_T *)sequenceProducerState;
    int k;
    if (!s) return;
    __atomic_fetch_sub(&gProc.liveStates, 1, __ATOMIC_RELAXED);
    QZ_LOG(2, "state %p: %lu block(s) served from announcements, %lu per "
              "block; %lu hint(s), timers from the 9th on: drop %.2f ms, buffers %.2f ms, staging and queueing %.2f ms (%.2f ms in copy calls, %.2f in launch calls), waited %.2f ms for the GPU\n", (void *)s,
           s->servedFromBatch, s->servedSync, s->hintCalls, s->hintDropNs / 1e6, s->hintPrepNs / 1e6, s->hintStageNs / 1e6,
           s->hintCopyCallNs / 1e6, s->hintLaunchCallNs / 1e6, s->hintWaitNs / 1e6);
    for (k = 0; k < QZ_HINTS; k++) {
        qzHintDrop(&s->hint[k]);
        free(s->hint[k].keys);
    }
    free(s);
}

int QZSTD_deviceStats(int device, unsigned long stats[4])
{
    int k;
    if (stats) for (k = 0; k < 4; k++) stats[k] = 0;
    if (stats && device >= 0 && device < gProc.numDevices && device < QZ_MAX_DEVICES)
    {
        for (k = 0; k < 3; k++) stats[k] = __atomic_load_n(&gProc.devBlocks[device][k], __ATOMIC_RELAXED);
        stats[3] = (unsigned long)(gProc.devNode[device] + 1); /* host NUMA node of the GPU + 1 (0 = unknown) */
    }
    return gProc.numDevices;
}

void QZSTD_failStats(void *sequenceProducerState, unsigned long stats[8])
{
    const QZSTD_Session_T *s = (const QZSTD_Session_T *)sequenceProducerState;
    int k;
    if (!stats) return;
    for (k = 0; k < 8; k++) stats[k] = 0;
    if (!s) return;
    stats[0] = s->fail[0];
    stats[1] = s->fail[QZ_CAUSE_GUARD];
    stats[2] = s->fail[QZ_CAUSE_DEVICE_DOWN];
    stats[3] = s->fail[QZ_CAUSE_TIMEOUT];
    stats[4] = s->fail[QZ_CAUSE_CAPACITY];
    stats[5] = s->fail[QZ_CAUSE_RUNTIME];
    stats[6] = s->redoneAlone;
    stats[7] = s->servedService;
}

unsigned long QZSTD_hintBroken(void *sequenceProducerState)
{
    return sequenceProducerState ? ((const QZSTD_Session_T *)sequenceProducerState)->stableBroken : 0ul;
}

void QZSTD_hintStats(void *sequenceProducerState, unsigned long stats[4])
{
    const QZSTD_Session_T *s = (const QZSTD_Session_T *)sequenceProducerState;
    if (!stats) return;
    stats[0] = s ? s->servedFromBatch : 0;
    stats[1] = s ? s->servedSync : 0;
    stats[2] = s ? s->hintCalls : 0;
    stats[3] = s ? s->hintWaitNs / 1000 : 0;
}

#ifdef QZ_TEST_HOOKS /* the mock build of tests/test_host_mock.py only: never in the release library */
unsigned long qzstd_test_orphans(void) { return qzOrphanCount; }
void qzstd_test_set_area_tags(unsigned int e) /* the next use of every batch area, every GPU, gets tag e + 1 (the wrap) */
{
    int d, k;
    for (d = 0; gProc.hb && d < gProc.numDevices; d++) {
        pthread_mutex_lock(&gProc.hb[d].mu);
        for (k = 0; k < QZ_HB_AREAS; k++) gProc.hb[d].area[k].lap = e & 0xFFFFFFu;
        pthread_mutex_unlock(&gProc.hb[d].mu);
    }
}
/* the hook's name from the time announcements kept their own result areas and epochs (tests/test_host_mock.py calls it): the tags now belong to
 * the batch areas, which every state shares, so `state` names nothing and every area's tag moves */
void qzstd_test_set_hint_epochs(void *state, unsigned int e)
{
    (void)state;
    qzstd_test_set_area_tags(e);
}
unsigned long qzstd_test_hint_launches(void) /* announcement launches since the device layer started, every GPU */
{
    unsigned long n = 0;
    int d;
    for (d = 0; gProc.hb && d < gProc.numDevices; d++) n += __atomic_load_n(&gProc.hb[d].launches, __ATOMIC_RELAXED);
    return n;
}
void qzstd_test_set_service_epochs(unsigned int e) /* every slot's next service request gets epoch e + 1 (the 24-bit wrap) */
{
    int i;
    for (i = 0; gProc.slots && i < gProc.numSlots; i++) gProc.slots[i].vEpoch = e & 0xFFFFFFu;
}
#endif

/* ---------------------------------------------------------------- producer ------- */

size_t qatSequenceProducer(void *sequenceProducerState, ZSTD_Sequence *outSeqs, size_t outSeqsCapacity,
                           const void *src, size_t srcSize, const void *dict, size_t dictSize,
                           int compressionLevel, size_t windowSize)
{
    QZSTD_Session_T *s = (QZSTD_Session_T *)sequenceProducerState;
    size_t rc;
    int order[QZ_HINTS], n, oi, dev, found;

    /* guards, reference :1123-1137 */
    if (windowSize < (srcSize < 32 * 1024 ? srcSize : 32 * 1024) || dictSize > 0 || dict) {
        QZ_LOG(2, "window %zu too small for block %zu, or dictionary given (%zu)\n", windowSize, srcSize, dictSize);
        return qzFailed(s, QZ_CAUSE_GUARD);
    }
    if (compressionLevel < QZ_LEVEL_MIN || compressionLevel > QZ_LEVEL_MAX) {
        QZ_LOG(1, "only levels 1-12 can be offloaded, got %d\n", compressionLevel);
        return qzFailed(s, QZ_CAUSE_GUARD);
    }
    if (!s || !outSeqs || !src || srcSize > QZSTD_HIP_BLOCK_MAX || outSeqsCapacity < 3) return qzFailed(s, QZ_CAUSE_GUARD);
    if (!qzDeviceUsable(s)) return qzFailed(s, QZ_CAUSE_DEVICE_DOWN);
    qzCause = QZ_CAUSE_RUNTIME; /* until a failing site below says otherwise */
    /* a batch collecting while every stream was busy goes out with the first caller that finds one free */
    for (dev = 0; gProc.hb && dev < gProc.numDevices; dev++) qzBatchPoke(s, &gProc.hb[dev]);

    /* served from an announcement?  The first one that holds the block decides: what it cannot serve, the per-block path takes */
    n = qzHintOrder(s, order);
    for (oi = 0; oi < n; oi++) {
        QZSTD_HintHit_T hit;
        if ((found = qzHintFind(s, order[oi], (const unsigned char *)src, srcSize, compressionLevel, &hit)) == 0) continue;
        rc = qzHintServe(s, &hit, found > 0, outSeqs, outSeqsCapacity, srcSize);
        if (rc != 0) return rc;
        break;
    }
    qzHintReapStale(s); /* nothing to serve from */

    /* sticky device per state: a GPU of the calling thread's socket if there is one, states spread round-robin (qzPickHint) */
    if (s->slotHint < 0) s->slotHint = qzPickHint();
    dev = s->slotHint % gProc.numDevices;
    rc = qzServiceBlock(s, dev, outSeqs, outSeqsCapacity, src, srcSize, compressionLevel | gProc.levelFlags);
    if (rc != QZ_NOT_SERVED) {
        QZ_LOG(2, "block %zu B level %d -> %zu sequences (service, device %d)\n", srcSize, compressionLevel, rc, dev);
    } else if (gProc.coalesce) {
        rc = qzCoalescedBlock(s, dev, outSeqs, outSeqsCapacity, src, srcSize, compressionLevel | gProc.levelFlags);
        QZ_LOG(2, "block %zu B level %d -> %zu sequences (coalesced, device %d)\n", srcSize, compressionLevel, rc, dev);
    } else {
        rc = qzSlotBlock(s, -1, outSeqs, outSeqsCapacity, src, srcSize, compressionLevel | gProc.levelFlags);
    }
    if (rc != ZSTD_SEQUENCE_PRODUCER_ERROR) s->servedSync++;
    else (void)qzFailed(s, qzCause);
    return rc;
}
