/*
 * srcslices_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_srcslices_host.py builds it with
 * -fsanitize=address,undefined and runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/:
 * QZSTD_frontCompressDeviceSlices on random cuttings of the buffers — every slice (and its base slice) an allocation of its own size inside
 * one registered pool, so that a read past a piece's end is a read the sanitizer sees as soon as it leaves the pool and a wrong byte as soon
 * as it stays inside — against QZSTD_frontCompressDeviceBatchDelta on the contiguous bytes: equal frame counts, sizes and bytes, with the
 * settings off and on, with a failed block, over several parts; and refusals with nothing counted.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
void qzstd_mock_extent_range(int slot, const void *p, size_t n);
void qzstd_mock_fail_block(int block);
int qzstd_mock_group_pieces_launches(void);

#define CHUNK 16400u
#define NBUF 6u
#define MAXSLICES 60000u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "srcslices_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 7, 16383, 2 * CHUNK + 5, 100001 };
static const unsigned char kElems[NBUF] = { 2, 1, 4, 8, 2, 4 };
static const int kBased[NBUF] = { 1, 1, 0, 1, 1, 1 };

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

int main(void)
{
    QZSTD_FrontParams prm;
    QZSTD_Front *f;
    QZSTD_DeviceBuf in[NBUF], bas[NBUF];
    static QZSTD_DeviceSrcSlice sl[MAXSLICES];
    unsigned char *whole, *pool, *want, *got;
    size_t wsizes[64], gsizes[64], first[NBUF + 1], gfirst[NBUF + 1], nFrames = 0, stride, total = 0, poolSize, i, b, round;
    unsigned long long st[4], st2[4];

    CHECK(setenv("QZSTD_FRONT_DEVICE_PART", "49200", 1) == 0); /* three full frames a part */
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = 1;
    f = QZSTD_createFront(&prm);
    CHECK(f);
    stride = QZSTD_frontFrameStride(f);
    for (b = 0; b < NBUF; b++) { total += kSizes[b]; nFrames += (kSizes[b] + CHUNK - 1u) / CHUNK; }
    CHECK(nFrames <= 64);
    /* the contiguous copies: buffers and bases in one registered range, at odd offsets */
    whole = (unsigned char *)malloc(2 * total + 64 * NBUF);
    CHECK(whole);
    qzstd_mock_device_range(0, whole, 2 * total + 64 * NBUF, 0);
    {
        size_t pos = 0;
        for (b = 0; b < NBUF; b++) {
            unsigned char *d = whole + pos + 1 + b, *s = d + kSizes[b] + 7;
            for (i = 0; i < kSizes[b]; i++) {
                d[i] = (i & 1u) ? (unsigned char)(0x3B + (rnd() & 3u)) : (unsigned char)rnd();
                s[i] = (unsigned char)(d[i] ^ (b == 3 ? 0u : ((rnd() & 7u) == 0 ? (rnd() & 7u) : 0u))); /* buffer 3 equals its base */
            }
            in[b].d_ptr = d; in[b].size = kSizes[b];
            bas[b].d_ptr = kBased[b] ? s : NULL; bas[b].size = kBased[b] ? kSizes[b] : 0;
            pos += 2 * kSizes[b] + 40;
        }
    }
    want = (unsigned char *)malloc(nFrames * stride);
    got = (unsigned char *)malloc(nFrames * stride);
    CHECK(want && got);
    /* the pool of pieces: EXACTLY as large as one round needs, so that the last piece ends on the pool's — the heap block's — last byte */
    for (round = 0; round < 12; round++) {
        const int settings = (round & 1u) != 0, fail = round == 10 || round == 11;
        size_t n = 0, pos = 0, need = 0, multi = 0;
        unsigned char *src[1], *cur;
        (void)src;
        CHECK(QZSTD_frontSetChecksum(f, settings) == 0 && QZSTD_frontSetDeltaSkip(f, settings) == 0);
        /* cut */
        for (b = 0; b < NBUF; b++) {
            size_t at = 0;
            while (at < kSizes[b]) {
                const uint32_t r = rnd();
                size_t len = round == 0 ? kSizes[b] : ((r & 15u) == 0 ? rnd() % 40000u + 1u : ((r & 16u) ? rnd() % 7u + 1u : rnd() % 3000u + 1u));
                if (len > kSizes[b] - at) len = kSizes[b] - at;
                if ((r & 0x700u) == 0 && n + 1 < MAXSLICES) { sl[n].buf = b; sl[n].offset = at; sl[n].size = 0; sl[n].d_src = NULL; sl[n].d_base = NULL; n++; }
                CHECK(n < MAXSLICES);
                sl[n].buf = b; sl[n].offset = at; sl[n].size = len; n++;
                at += len;
                need += 2 * len;
            }
        }
        poolSize = need ? need : 1;
        pool = (unsigned char *)malloc(poolSize);
        CHECK(pool);
        qzstd_mock_device_range(1, pool, poolSize, 0);
        qzstd_mock_extent_range(1, pool, poolSize);
        /* place: back to front, so that memory order is not buffer order; no gaps: a load past a piece reads a neighbour's bytes (wrong frame)
         * or leaves the heap block (the sanitizer) */
        cur = pool + poolSize;
        for (i = 0; i < n; i++) {
            if (!sl[i].size) continue;
            cur -= sl[i].size;
            memcpy(cur, (const unsigned char *)in[sl[i].buf].d_ptr + sl[i].offset, sl[i].size);
            sl[i].d_src = cur;
            cur -= sl[i].size;
            if (kBased[sl[i].buf]) {
                memcpy(cur, (const unsigned char *)bas[sl[i].buf].d_ptr + sl[i].offset, sl[i].size);
                sl[i].d_base = cur;
            } else {
                memset(cur, 0xEE, sl[i].size);
                sl[i].d_base = NULL;
            }
        }
        CHECK(cur == pool || need == 0);
        for (b = 0, pos = 0; b < NBUF; b++) { /* frames of more than one slice (the pieces lie back to front: no two follow each other) */
            size_t c;
            for (c = 0; c * CHUNK < kSizes[b]; c++) {
                const size_t lo = c * CHUNK, hi = lo + CHUNK < kSizes[b] ? lo + CHUNK : kSizes[b];
                for (i = 0; i < n; i++)
                    if (sl[i].buf == b && sl[i].size && sl[i].offset <= lo && lo < sl[i].offset + sl[i].size) break;
                CHECK(i < n);
                if (sl[i].offset + sl[i].size < hi) multi++;
            }
        }
        (void)pos;
        if (fail) qzstd_mock_fail_block(0);
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bas, kElems, NBUF, NULL, want, nFrames * stride, wsizes, first) == nFrames);
        QZSTD_frontSrcSliceStats(f, st);
        i = (size_t)qzstd_mock_group_pieces_launches();
        CHECK(QZSTD_frontCompressDeviceSlices(f, kSizes, kElems, NBUF, sl, n, NULL, got, nFrames * stride, gsizes, gfirst) == nFrames);
        if (fail) qzstd_mock_fail_block(-1);
        QZSTD_frontSrcSliceStats(f, st2);
        CHECK(memcmp(first, gfirst, sizeof(first)) == 0);
        for (i = 0; i < nFrames; i++) {
            CHECK(wsizes[i] == gsizes[i]);
            CHECK(memcmp(want + i * stride, got + i * stride, wsizes[i]) == 0);
        }
        CHECK(st2[1] - st[1] == total && st2[2] - st[2] <= multi && (round == 0 ? st2[2] == st[2] && st2[3] == st[3] : 1));
        if (!settings) CHECK(st2[2] - st[2] == multi);
        /* refusals: nothing counted */
        if (n > 2 && round) {
            QZSTD_DeviceSrcSlice keep = sl[n - 1];
            QZSTD_frontSrcSliceStats(f, st);
            sl[n - 1].size += 1;
            CHECK(QZSTD_frontCompressDeviceSlices(f, kSizes, kElems, NBUF, sl, n, NULL, got, nFrames * stride, gsizes, NULL) == ERR);
            sl[n - 1] = keep;
            CHECK(QZSTD_frontCompressDeviceSlices(f, kSizes, kElems, NBUF, sl, n - 1, NULL, got, nFrames * stride, gsizes, NULL) == ERR);
            sl[n - 1].d_src = (const unsigned char *)sl[n - 1].d_src - 1; /* (the last placed first: it begins one byte in front of the pool) */
            if (sl[n - 1].d_src < (const void *)pool)
                CHECK(QZSTD_frontCompressDeviceSlices(f, kSizes, kElems, NBUF, sl, n, NULL, got, nFrames * stride, gsizes, NULL) == ERR);
            sl[n - 1] = keep;
            QZSTD_frontSrcSliceStats(f, st2);
            CHECK(memcmp(st, st2, sizeof(st)) == 0);
        }
        qzstd_mock_device_range(1, NULL, 0, 0);
        qzstd_mock_extent_range(1, NULL, 0);
        free(pool);
    }
    QZSTD_freeFront(f);
    free(want);
    free(got);
    free(whole);
    printf("ok\n");
    return 0;
}
