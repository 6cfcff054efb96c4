/*
 * restore_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_restore_host.py builds it with -fsanitize=address,undefined
 * and runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/: what
 * QZSTD_frontCompressDeviceBatchTyped writes is restored by QZSTD_frontRestoreDeviceBatchTyped into buffers at every alignment — several parts,
 * strided and compacted frames, checksums, foreign frames, a front without the producer — and every error path returns (size_t)-1 with the
 * guard bytes around the buffers intact.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_bytegroup.h"
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
int qzstd_mock_ungroup_launches(void);
int qzstd_mock_event_waits(void);

#define CHUNK 32768u
#define NBUF 8u
#define GUARD 64u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "restore_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 7, 8191, CHUNK, CHUNK + 1, 100001, 4 * CHUNK };
static const unsigned char kElems[NBUF] = { 2, 1, 4, 2, 0, 8, 4, 2 }; /* 0: the front's setting */

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

/* bf16-like weights: a skewed high byte, a noisy low one — compressible after grouping, and not all literals before */
static void fill(unsigned char *p, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++) p[i] = (i & 1u) ? (unsigned char)(0x3B + (rnd() & 3u)) : (unsigned char)rnd();
}

/* "device" memory: one registered range, the buffers inside it at place[i], 0xA5 everywhere else */
typedef struct { unsigned char *base; size_t size, place[NBUF]; } Pool;

static void poolMake(Pool *p, int slot, int dev, const unsigned skew[NBUF], int packed)
{
    size_t pos = GUARD, i;
    for (i = 0; i < NBUF; i++) {
        if (!packed) pos = ((pos + 15u) & ~(size_t)15u) + skew[i];
        p->place[i] = pos;
        pos += kSizes[i];
    }
    p->size = pos + GUARD;
    p->base = (unsigned char *)malloc(p->size);
    CHECK(p->base);
    memset(p->base, 0xA5, p->size);
    qzstd_mock_device_range(slot, p->base, p->size, dev);
}

static void poolBufs(const Pool *p, QZSTD_DeviceOutBuf out[NBUF])
{
    size_t i;
    for (i = 0; i < NBUF; i++) { out[i].d_ptr = p->base + p->place[i]; out[i].size = kSizes[i]; }
}

/* the pool holds exactly `datas` inside the buffers (NULL: nothing was written at all) and 0xA5 elsewhere */
static int poolHolds(const Pool *p, unsigned char *const datas[NBUF])
{
    size_t pos = 0, i, b;
    for (i = 0; i <= NBUF; i++) {
        const size_t upTo = i < NBUF ? p->place[i] : p->size;
        for (b = pos; b < upTo; b++) if (p->base[b] != 0xA5) return 0;
        if (i == NBUF) break;
        if (datas ? memcmp(p->base + p->place[i], datas[i], kSizes[i]) != 0 : 0) return 0;
        if (!datas) for (b = 0; b < kSizes[i]; b++) if (p->base[p->place[i] + b] != 0xA5) return 0;
        pos = p->place[i] + kSizes[i];
    }
    return 1;
}

static void poolWipe(Pool *p) { memset(p->base, 0xA5, p->size); }

int main(void)
{
    static const unsigned skewA[NBUF] = { 3, 0, 1, 15, 8, 2, 7, 5 }, skewB[NBUF] = { 0, 1, 2, 3, 4, 5, 6, 9 };
    QZSTD_FrontParams prm;
    QZSTD_Front *f, *plain;
    QZSTD_DeviceBuf in[NBUF];
    QZSTD_DeviceOutBuf out[NBUF], two[NBUF];
    Pool src, dst, packed, other;
    unsigned char *datas[NBUF], *frames, *compact, *foreign, *tmp, *grouped, hostBuf[64];
    size_t sizes[64], first[NBUF + 1], fsizes[64], nFrames, stride, i, c, n, pos;
    unsigned long long st[4], st2[4];
    int checksum, launches, waits;

    CHECK(setenv("QZSTD_FRONT_DEVICE_PART", "98304", 1) == 0); /* three full frames a part: four parts, both slots reused */
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = 1;
    f = QZSTD_createFront(&prm);
    CHECK(f);
    CHECK(QZSTD_frontSetByteGroup(f, 4) == 0);
    stride = QZSTD_frontFrameStride(f);

    poolMake(&src, 0, 0, skewB, 0);
    poolMake(&dst, 1, 0, skewA, 0);
    poolMake(&packed, 2, 0, skewA, 1);
    poolMake(&other, 3, 1, skewB, 0);
    for (i = 0; i < NBUF; i++) {
        datas[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        CHECK(datas[i]);
        fill(datas[i], kSizes[i]);
        memcpy(src.base + src.place[i], datas[i], kSizes[i]);
        in[i].d_ptr = src.base + src.place[i];
        in[i].size = kSizes[i];
    }
    nFrames = QZSTD_frontDeviceBatchFrames(f, in, NBUF);
    CHECK(nFrames == 14 && nFrames <= 64);
    frames = (unsigned char *)malloc(nFrames * stride);
    compact = (unsigned char *)malloc(nFrames * stride);
    foreign = (unsigned char *)malloc(nFrames * stride);
    tmp = (unsigned char *)malloc(stride);
    grouped = (unsigned char *)malloc(CHUNK);
    CHECK(frames && compact && foreign && tmp && grouped);

    for (checksum = 0; checksum < 2; checksum++) {
        CHECK(QZSTD_frontSetChecksum(f, checksum) == 0);
        CHECK(QZSTD_frontCompressDeviceBatchTyped(f, in, kElems, NBUF, NULL, frames, nFrames * stride, sizes, first) == nFrames);
        /* strided, as the compress call left them */
        poolBufs(&dst, out);
        QZSTD_frontRestoreStats(f, st);
        launches = qzstd_mock_ungroup_launches();
        CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames, out, kElems, NBUF, NULL) == nFrames);
        CHECK(poolHolds(&dst, datas));
        QZSTD_frontRestoreStats(f, st2);
        CHECK(st2[0] - st[0] == nFrames && st2[1] - st[1] == 1 + 7 + 8191 + CHUNK + CHUNK + 1 + 100001 + 4 * CHUNK);
        CHECK(st2[3] - st[3] == 4 && qzstd_mock_ungroup_launches() == launches + 4 && st2[2] - st[2] >= st2[1] - st[1]);
        poolWipe(&dst);
        /* compacted, frameStride 0, into buffers packed back to back */
        memcpy(compact, frames, nFrames * stride);
        (void)QZSTD_frontCompact(f, compact, sizes, nFrames);
        poolBufs(&packed, out);
        CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, compact, 0, sizes, nFrames, out, kElems, NBUF, NULL) == nFrames);
        CHECK(poolHolds(&packed, datas));
        poolWipe(&packed);
    }
    CHECK(QZSTD_frontSetChecksum(f, 0) == 0);

    /* foreign frames: ZSTD_compress2 over QZSTD_byteGroup's output, with checksums; restored by a front without the producer */
    {
        ZSTD_CCtx *zc = ZSTD_createCCtx();
        CHECK(zc && !ZSTD_isError(ZSTD_CCtx_setParameter(zc, ZSTD_c_compressionLevel, 3)) &&
              !ZSTD_isError(ZSTD_CCtx_setParameter(zc, ZSTD_c_checksumFlag, 1)));
        for (i = 0, c = 0; i < NBUF; i++) {
            const unsigned k = kElems[i] ? kElems[i] : 4u;
            for (pos = 0; pos < kSizes[i]; pos += CHUNK, c++) {
                n = kSizes[i] - pos < CHUNK ? kSizes[i] - pos : CHUNK;
                CHECK(QZSTD_byteGroup(grouped, datas[i] + pos, n, k) == n);
                fsizes[c] = ZSTD_compress2(zc, foreign + c * stride, stride, grouped, n);
                CHECK(!ZSTD_isError(fsizes[c]));
            }
        }
        CHECK(c == nFrames);
        ZSTD_freeCCtx(zc);
    }
    prm.useProducer = 0;
    plain = QZSTD_createFront(&prm);
    CHECK(plain && QZSTD_frontSetByteGroup(plain, 4) == 0);
    poolBufs(&dst, out);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(plain, foreign, stride, fsizes, nFrames, out, kElems, NBUF, NULL) == nFrames);
    CHECK(poolHolds(&dst, datas));
    poolWipe(&dst);
    /* one buffer, the front's element size (buffer 6: element size 4) */
    CHECK(QZSTD_frontRestoreDevice(plain, foreign + first[6] * stride, stride, fsizes + first[6], first[7] - first[6], dst.base + dst.place[6],
                                   kSizes[6], NULL) == first[7] - first[6]);
    CHECK(memcmp(dst.base + dst.place[6], datas[6], kSizes[6]) == 0);
    memset(dst.base + dst.place[6], 0xA5, kSizes[6]);
    CHECK(poolHolds(&dst, NULL));

    /* refusals before anything is queued: no event wait, no launch, nothing counted, nothing written */
    QZSTD_frontRestoreStats(f, st);
    launches = qzstd_mock_ungroup_launches();
    waits = qzstd_mock_event_waits();
    poolBufs(&dst, out);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames - 1, out, kElems, NBUF, NULL) == ERR);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames + 1, out, kElems, NBUF, NULL) == ERR);
    {
        unsigned char bad[NBUF];
        memcpy(bad, kElems, NBUF);
        bad[5] = 3;
        CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames, out, bad, NBUF, NULL) == ERR);
    }
    memcpy(two, out, sizeof(two));
    two[2].d_ptr = hostBuf; /* a host pointer */
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames, two, kElems, NBUF, NULL) == ERR);
    two[2].d_ptr = NULL;
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames, two, kElems, NBUF, NULL) == ERR);
    memcpy(two, out, sizeof(two));
    two[4].d_ptr = other.base + other.place[4]; /* another device's memory */
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, nFrames, two, kElems, NBUF, NULL) == ERR);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(NULL, frames, stride, sizes, nFrames, out, kElems, NBUF, NULL) == ERR);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, NULL, stride, sizes, nFrames, out, kElems, NBUF, NULL) == ERR);
    CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, frames, stride, sizes, 0, out, kElems, 0, NULL) == 0);
    QZSTD_frontRestoreStats(f, st2);
    CHECK(memcmp(st, st2, sizeof(st)) == 0 && qzstd_mock_ungroup_launches() == launches && qzstd_mock_event_waits() == waits);
    CHECK(poolHolds(&dst, NULL) && poolHolds(&other, NULL));

    /* after work has started: a frame a byte short, a byte long, a damaged checksum — (size_t)-1, the guards intact, the front usable */
    {
        ZSTD_CCtx *zc = ZSTD_createCCtx();
        const size_t victim = first[7] + 2; /* a full chunk of the last buffer, in a later part */
        int mode;
        CHECK(zc);
        for (mode = 0; mode < 3; mode++) {
            unsigned char *at = foreign + victim * stride;
            const size_t keep = fsizes[victim];
            memcpy(tmp, at, keep);
            if (mode < 2) {
                n = mode == 0 ? CHUNK - 1 : CHUNK + 1;
                memset(grouped, 7, CHUNK);
                fsizes[victim] = ZSTD_compress2(zc, at, stride, grouped, mode == 0 ? n : CHUNK);
                if (mode == 1) { /* CHUNK + 1 bytes of content: two frames back to back decode as one content */
                    const size_t more = ZSTD_compress2(zc, at + fsizes[victim], stride - fsizes[victim], grouped, 1);
                    CHECK(!ZSTD_isError(more));
                    fsizes[victim] += more;
                }
                CHECK(!ZSTD_isError(fsizes[victim]));
            } else {
                at[keep - 1] ^= 1u; /* the stored hash */
            }
            poolBufs(&dst, out);
            CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, foreign, stride, fsizes, nFrames, out, kElems, NBUF, NULL) == ERR);
            memcpy(at, tmp, keep);
            fsizes[victim] = keep;
            for (i = 0; i < NBUF; i++) memset(dst.base + dst.place[i], 0xA5, kSizes[i]); /* the buffers' contents are unspecified ... */
            CHECK(poolHolds(&dst, NULL));                                                 /* ... and nothing outside them was written */
            CHECK(QZSTD_frontRestoreDeviceBatchTyped(f, foreign, stride, fsizes, nFrames, out, kElems, NBUF, NULL) == nFrames);
            CHECK(poolHolds(&dst, datas));
            poolWipe(&dst);
        }
        ZSTD_freeCCtx(zc);
    }

    /* the compress call after all that: the frames it built before */
    CHECK(QZSTD_frontSetChecksum(f, 1) == 0);
    CHECK(QZSTD_frontCompressDeviceBatchTyped(f, in, kElems, NBUF, NULL, compact, nFrames * stride, fsizes, NULL) == nFrames);
    for (c = 0; c < nFrames; c++) CHECK(fsizes[c] == sizes[c] && memcmp(compact + c * stride, frames + c * stride, sizes[c]) == 0);

    QZSTD_freeFront(plain);
    QZSTD_freeFront(f);
    for (i = 0; i < NBUF; i++) free(datas[i]);
    free(frames); free(compact); free(foreign); free(tmp); free(grouped);
    free(src.base); free(dst.base); free(packed.base); free(other.base);
    puts("ok");
    return 0;
}
