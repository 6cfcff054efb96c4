/*
 * delta_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_delta_host.py builds it with -fsanitize=address,undefined and
 * runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/ (mock_hip_group_xor.c and
 * mock_hip_ungroup_xor.c included): QZSTD_frontCompressDeviceBatchDelta over ragged sizes and bases at other alignments than their buffers,
 * QZSTD_frontRestoreDeviceBatchDelta into fresh buffers and in place over the bases, the comparison byte for byte, a failed block's
 * copy-back path, and the refusals with the guard bytes intact.  Prints "ok".
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
void qzstd_mock_fail_block(int b);
int qzstd_mock_group_xor_launches(void);
int qzstd_mock_ungroup_xor_launches(void);
int qzstd_mock_event_waits(void);

#define CHUNK 32768u
#define NBUF 10u
#define GUARD 64u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "delta_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 7, 8191, CHUNK, CHUNK + 1, 100001, 4 * CHUNK, 0, 3 * CHUNK + 5 };
static const unsigned char kElems[NBUF] = { 2, 1, 4, 2, 1, 8, 4, 2, 4, 8 };
static int based(size_t i) { return i % 3u != 2u; } /* every third buffer has no base */

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

/* bf16-like weights, and a base a small step away: the high bytes mostly agree, a fifth of the low bytes differ in their low bits */
static void fill(unsigned char *p, unsigned char *b, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++) {
        p[i] = (i & 1u) ? (unsigned char)(0x3B + (rnd() & 3u)) : (unsigned char)rnd();
        b[i] = (unsigned char)(p[i] ^ ((rnd() % 5u == 0 && !(i & 1u)) ? (rnd() & 7u) : 0u));
    }
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

/* the pool holds exactly `datas` inside the buffers (NULL: 0xA5 there too) and 0xA5 elsewhere */
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

static void poolPut(Pool *p, unsigned char *const datas[NBUF])
{
    size_t i;
    memset(p->base, 0xA5, p->size);
    for (i = 0; datas && i < NBUF; i++) memcpy(p->base + p->place[i], datas[i], kSizes[i]);
}

int main(void)
{
    static const unsigned skewA[NBUF] = { 3, 0, 1, 15, 8, 2, 7, 5, 0, 11 }, skewB[NBUF] = { 0, 1, 2, 3, 4, 5, 6, 9, 3, 13 },
                          skewC[NBUF] = { 7, 0, 2, 9, 15, 4, 1, 8, 6, 2 };
    QZSTD_FrontParams prm;
    QZSTD_Front *f;
    QZSTD_DeviceBuf in[NBUF], bs[NBUF], pre[NBUF], bad[NBUF];
    QZSTD_DeviceOutBuf out[NBUF];
    Pool src, bas, xored, dst, packed, other;
    unsigned char *datas[NBUF], *bases[NBUF], *deltas[NBUF], *frames, *typed, *content, *plainBytes, hostBuf[64];
    size_t sizes[64], tsizes[64], first[NBUF + 1], nFrames, stride, i, c, n, pos, nBased = 0;
    unsigned long long st[4], st2[4], dv[4], dv2[4];
    int checksum, gx, ux, waits;
    ZSTD_DCtx *zd = ZSTD_createDCtx();

    CHECK(zd && setenv("QZSTD_FRONT_DEVICE_PART", "98304", 1) == 0); /* three full frames a part: several parts, both slots reused */
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = 1;
    f = QZSTD_createFront(&prm);
    CHECK(f);
    stride = QZSTD_frontFrameStride(f);

    poolMake(&src, 0, 0, skewB, 0);
    poolMake(&bas, 1, 0, skewC, 0); /* the bases at other alignments than their buffers */
    poolMake(&xored, 2, 0, skewA, 0);
    poolMake(&dst, 3, 0, skewA, 0);
    poolMake(&packed, 4, 0, skewA, 1);
    poolMake(&other, 5, 1, skewB, 0);
    for (i = 0; i < NBUF; i++) {
        datas[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        bases[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        deltas[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        CHECK(datas[i] && bases[i] && deltas[i]);
        fill(datas[i], bases[i], kSizes[i]);
        if (based(i)) QZSTD_byteXor(deltas[i], datas[i], bases[i], kSizes[i]); else memcpy(deltas[i], datas[i], kSizes[i]);
        in[i].d_ptr = src.base + src.place[i];
        in[i].size = kSizes[i];
        bs[i].d_ptr = based(i) ? bas.base + bas.place[i] : NULL;
        bs[i].size = based(i) ? kSizes[i] : 0;
        pre[i].d_ptr = xored.base + xored.place[i];
        pre[i].size = kSizes[i];
    }
    poolPut(&src, datas);
    poolPut(&bas, bases);
    poolPut(&xored, deltas);
    nFrames = QZSTD_frontDeviceBatchFrames(f, in, NBUF);
    CHECK(nFrames == 18 && nFrames <= 64);
    for (i = 0; i < NBUF; i++) if (based(i)) nBased += (kSizes[i] + CHUNK - 1) / CHUNK;
    frames = (unsigned char *)malloc(nFrames * stride);
    typed = (unsigned char *)malloc(nFrames * stride);
    content = (unsigned char *)malloc(CHUNK);
    plainBytes = (unsigned char *)malloc(CHUNK);
    CHECK(frames && typed && content && plainBytes);

    for (checksum = 0; checksum < 2; checksum++) {
        CHECK(QZSTD_frontSetChecksum(f, checksum) == 0);
        /* the delta frames are the Typed frames of the pre-XORed buffers */
        CHECK(QZSTD_frontCompressDeviceBatchTyped(f, pre, kElems, NBUF, NULL, typed, nFrames * stride, tsizes, NULL) == nFrames);
        QZSTD_frontDeltaStats(f, dv);
        gx = qzstd_mock_group_xor_launches();
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NBUF, NULL, frames, nFrames * stride, sizes, first) == nFrames);
        QZSTD_frontDeltaStats(f, dv2);
        CHECK(qzstd_mock_group_xor_launches() > gx);
        CHECK(dv2[0] + dv2[1] + dv2[2] - dv[0] - dv[1] - dv[2] == nBased && dv2[2] == dv[2] && dv2[3] == dv[3]);
        for (c = 0; c < nFrames; c++) CHECK(sizes[c] == tsizes[c] && memcmp(frames + c * stride, typed + c * stride, sizes[c]) == 0);
        /* the bases and the buffers were only read */
        for (i = 0; i < NBUF; i++)
            CHECK(memcmp(bas.base + bas.place[i], bases[i], kSizes[i]) == 0 && memcmp(src.base + src.place[i], datas[i], kSizes[i]) == 0);
        /* a reader of its own: decode, ungroup, XOR */
        for (i = 0; i < NBUF; i++)
            for (pos = 0, c = first[i]; pos < kSizes[i]; pos += CHUNK, c++) {
                n = kSizes[i] - pos < CHUNK ? kSizes[i] - pos : CHUNK;
                CHECK(ZSTD_decompressDCtx(zd, content, CHUNK, frames + c * stride, sizes[c]) == n);
                CHECK(QZSTD_byteUngroup(plainBytes, content, n, kElems[i]) == n);
                if (based(i)) QZSTD_byteXor(plainBytes, plainBytes, bases[i] + pos, n);
                CHECK(memcmp(plainBytes, datas[i] + pos, n) == 0);
            }
        /* back: into fresh buffers ... */
        for (i = 0; i < NBUF; i++) { out[i].d_ptr = dst.base + dst.place[i]; out[i].size = kSizes[i]; }
        QZSTD_frontRestoreStats(f, st);
        ux = qzstd_mock_ungroup_xor_launches();
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, sizes, nFrames, out, bs, kElems, NBUF, NULL) == nFrames);
        CHECK(poolHolds(&dst, datas));
        QZSTD_frontRestoreStats(f, st2);
        QZSTD_frontDeltaStats(f, dv);
        CHECK(st2[0] - st[0] == nFrames && qzstd_mock_ungroup_xor_launches() > ux && dv[3] - dv2[3] == nBased);
        poolPut(&dst, NULL);
        /* ... and in place over the bases, packed back to back (neighbours share 16-byte words), from compacted frames */
        poolPut(&packed, NULL);
        for (i = 0; i < NBUF; i++) {
            if (based(i)) memcpy(packed.base + packed.place[i], bases[i], kSizes[i]);
            out[i].d_ptr = packed.base + packed.place[i];
            out[i].size = kSizes[i];
            bad[i].d_ptr = based(i) ? out[i].d_ptr : NULL;
            bad[i].size = based(i) ? kSizes[i] : 0;
        }
        memcpy(typed, frames, nFrames * stride);
        (void)QZSTD_frontCompact(f, typed, sizes, nFrames);
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, typed, 0, sizes, nFrames, out, bad, kElems, NBUF, NULL) == nFrames);
        CHECK(poolHolds(&packed, datas));
    }
    CHECK(QZSTD_frontSetChecksum(f, 0) == 0);

    /* a block the matcher failed: both buffers come back, the frame still decodes to the grouped delta and restores */
    QZSTD_frontDeltaStats(f, dv);
    QZSTD_frontDeviceStats(f, st);
    qzstd_mock_fail_block(0);
    CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NBUF, NULL, frames, nFrames * stride, sizes, first) == nFrames);
    qzstd_mock_fail_block(-1);
    QZSTD_frontDeltaStats(f, dv2);
    QZSTD_frontDeviceStats(f, st2);
    CHECK(dv2[2] > dv[2] && st2[2] > st[2]);
    for (i = 0; i < NBUF; i++) { out[i].d_ptr = dst.base + dst.place[i]; out[i].size = kSizes[i]; }
    CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, sizes, nFrames, out, bs, kElems, NBUF, NULL) == nFrames);
    CHECK(poolHolds(&dst, datas));
    poolPut(&dst, NULL);

    /* refusals before anything is queued: no event wait, no launch, nothing counted, nothing written */
    QZSTD_frontRestoreStats(f, st);
    QZSTD_frontDeltaStats(f, dv);
    gx = qzstd_mock_group_xor_launches();
    ux = qzstd_mock_ungroup_xor_launches();
    waits = qzstd_mock_event_waits();
    for (c = 0; c < 5; c++) {
        memcpy(bad, bs, sizeof(bad));
        if (c == 0) bad[3].size -= 1;                                   /* another size than its buffer */
        if (c == 1) bad[3].d_ptr = NULL;                                /* NULL with a size */
        if (c == 2) { bad[1].d_ptr = hostBuf; }                         /* host memory */
        if (c == 3) bad[4].d_ptr = other.base + other.place[4];         /* another device */
        if (c == 4) bad[7].d_ptr = bas.base - 8;                        /* its first byte in front of the device memory */
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bad, kElems, NBUF, NULL, typed, nFrames * stride, tsizes, NULL) == ERR);
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, sizes, nFrames, out, bad, kElems, NBUF, NULL) == ERR);
    }
    CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, sizes, nFrames - 1, out, bs, kElems, NBUF, NULL) == ERR);
    CHECK(QZSTD_frontCompressDeviceBatchDelta(NULL, in, bs, kElems, NBUF, NULL, typed, nFrames * stride, tsizes, NULL) == ERR);
    CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NBUF, NULL, typed, stride, tsizes, NULL) == ERR); /* dst too small */
    QZSTD_frontRestoreStats(f, st2);
    QZSTD_frontDeltaStats(f, dv2);
    CHECK(memcmp(st, st2, sizeof(st)) == 0 && memcmp(dv, dv2, sizeof(dv)) == 0);
    CHECK(qzstd_mock_group_xor_launches() == gx && qzstd_mock_ungroup_xor_launches() == ux && qzstd_mock_event_waits() == waits);
    CHECK(poolHolds(&dst, NULL) && poolHolds(&other, NULL));

    /* bases NULL: the Typed calls */
    CHECK(QZSTD_frontCompressDeviceBatchTyped(f, in, kElems, NBUF, NULL, typed, nFrames * stride, tsizes, NULL) == nFrames);
    CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, NULL, kElems, NBUF, NULL, frames, nFrames * stride, sizes, NULL) == nFrames);
    for (c = 0; c < nFrames; c++) CHECK(sizes[c] == tsizes[c] && memcmp(frames + c * stride, typed + c * stride, sizes[c]) == 0);
    CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, sizes, nFrames, out, NULL, kElems, NBUF, NULL) == nFrames);
    CHECK(poolHolds(&dst, datas));
    CHECK(qzstd_mock_group_xor_launches() == gx && qzstd_mock_ungroup_xor_launches() == ux);

    ZSTD_freeDCtx(zd);
    QZSTD_freeFront(f);
    for (i = 0; i < NBUF; i++) { free(datas[i]); free(bases[i]); free(deltas[i]); }
    free(frames); free(typed); free(content); free(plainBytes);
    free(src.base); free(bas.base); free(xored.base); free(dst.base); free(packed.base); free(other.base);
    puts("ok");
    return 0;
}
