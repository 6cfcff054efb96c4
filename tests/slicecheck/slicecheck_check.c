/*
 * slicecheck_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_slicecheck_host.py builds it with
 * -fsanitize=address,undefined and runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/:
 * QZSTD_frontFingerprintDeviceSlices, QZSTD_frontCheckDeviceSlices and QZSTD_frontVerifyDeviceSlices on random cuttings of the buffers —
 * every slice (and its base slice) packed back to front into a heap block of exactly the round's size, so that a read past a piece's end
 * is a read the sanitizer sees as soon as it leaves the block and a wrong answer as soon as it stays inside — against the contiguous calls
 * on the contiguous bytes: equal fingerprints, flags, counts and first differing offsets, with delta skip off and on, unchanged and with a
 * planted byte, over several parts; and refusals with nothing counted.  Prints "ok".
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
int qzstd_mock_fingerprint_pieces_launches(void);
int qzstd_mock_ungroup_cmp_pieces_launches(void);
int qzstd_mock_fingerprint_launches(void);
int qzstd_mock_ungroup_cmp_launches(void);

#define CHUNK 16400u
#define NBUF 6u
#define MAXSLICES 60000u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "slicecheck_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 7, 16383, 2 * CHUNK + 5, 100001 };
static const unsigned char kElems[NBUF] = { 2, 1, 4, 8, 2, 4 };
static const int kBased[NBUF] = { 1, 1, 0, 1, 1, 1 };

static uint64_t gRng = 0xD1B54A32D192ED03ull;
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
    unsigned char *whole, *pool, *frames, wflags[64], gflags[64];
    unsigned long long wfp[64], gfp[64], st[4], st2[4];
    size_t fsizes[64], first[NBUF + 1], gfirst[NBUF + 1], wdiff[64], gdiff[64], nFrames = 0, stride, total = 0, poolSize, i, b, round;

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
    frames = (unsigned char *)malloc(nFrames * stride);
    CHECK(frames);
    for (round = 0; round < 12; round++) {
        const int skip = (round & 1u) != 0, plant = round >= 4 && round != 7; /* (round 9: a planted byte in a recognised zero frame) */
        size_t n = 0, need = 0, multi = 0, wn, gn, planted = 0;
        unsigned char *cur, *plantAt = NULL;
        int l0, l1;
        CHECK(QZSTD_frontSetChecksum(f, skip) == 0 && QZSTD_frontSetDeltaSkip(f, skip) == 0);
        /* the frames and the fingerprints of the contiguous bytes as they are now */
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bas, kElems, NBUF, NULL, frames, nFrames * stride, fsizes, first) == nFrames);
        CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, NBUF, NULL, wfp, NULL) == nFrames);
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
        /* the pool of pieces: EXACTLY as large as the round needs, so that the piece placed first ends on the heap block's last byte */
        poolSize = need ? need : 1;
        pool = (unsigned char *)malloc(poolSize);
        CHECK(pool);
        qzstd_mock_device_range(1, pool, poolSize, 0);
        qzstd_mock_extent_range(1, pool, poolSize);
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
        for (b = 0; b < NBUF; b++) { /* frames of more than one slice (the pieces lie back to front: no two follow each other) */
            size_t c;
            for (c = 0; c * CHUNK < kSizes[b]; c++) {
                const size_t lo = c * CHUNK, hi = lo + CHUNK < kSizes[b] ? lo + CHUNK : kSizes[b];
                for (i = 0; i < n; i++)
                    if (sl[i].buf == b && sl[i].size && sl[i].offset <= lo && lo < sl[i].offset + sl[i].size) break;
                CHECK(i < n);
                if (sl[i].offset + sl[i].size < hi) multi++;
            }
        }
        if (plant) {
            /* ONE byte of the live side changes, in the slices and in the contiguous copy alike: in buffer 3 (all zero frames under the
             * skip), 4 or 5 by turns */
            const size_t pb = 3u + round % 3u, po = rnd() % kSizes[pb];
            for (i = 0; i < n; i++)
                if (sl[i].buf == pb && sl[i].size && sl[i].offset <= po && po < sl[i].offset + sl[i].size) break;
            CHECK(i < n);
            plantAt = (unsigned char *)(uintptr_t)sl[i].d_src + (po - sl[i].offset);
            *plantAt ^= 0x10;
            ((unsigned char *)(uintptr_t)in[pb].d_ptr)[po] ^= 0x10;
            planted = pb * 1000000u + po;
        }
        /* fingerprints and check */
        QZSTD_frontSliceCheckStats(f, st);
        l0 = qzstd_mock_fingerprint_pieces_launches();
        l1 = qzstd_mock_fingerprint_launches();
        CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, NBUF, NULL, gfp, NULL) == nFrames); /* (the oracle of the bytes as they are NOW) */
        CHECK(qzstd_mock_fingerprint_launches() == l1 + 1);
        memset(gfirst, 0xFF, sizeof(gfirst));
        {
            unsigned long long now[64];
            memcpy(now, gfp, sizeof(now));
            memset(gfp, 0, sizeof(gfp));
            CHECK(QZSTD_frontFingerprintDeviceSlices(f, kSizes, NBUF, sl, n, NULL, gfp, gfirst) == nFrames);
            CHECK(memcmp(now, gfp, nFrames * sizeof(now[0])) == 0);
        }
        CHECK(memcmp(first, gfirst, sizeof(first)) == 0);
        CHECK(qzstd_mock_fingerprint_pieces_launches() == l0 + (multi ? 1 : 0) && qzstd_mock_fingerprint_launches() == l1 + 1 + (multi ? 0 : 1));
        wn = QZSTD_frontCheckDeviceBatch(f, in, NBUF, NULL, wfp, nFrames, wflags);
        gn = QZSTD_frontCheckDeviceSlices(f, kSizes, NBUF, sl, n, NULL, wfp, nFrames, gflags);
        CHECK(wn == (plant ? 1u : 0u) && gn == wn && memcmp(wflags, gflags, nFrames) == 0);
        QZSTD_frontSliceCheckStats(f, st2);
        CHECK(st2[1] - st[1] == 2 * total && st2[2] - st[2] == 2 * multi && st2[3] - st[3] == (multi ? 2u : 0u));
        /* verify */
        l0 = qzstd_mock_ungroup_cmp_pieces_launches();
        wn = QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bas, kElems, NBUF, NULL, wdiff);
        gn = QZSTD_frontVerifyDeviceSlices(f, frames, stride, fsizes, nFrames, kSizes, kElems, NBUF, sl, n, NULL, gdiff);
        CHECK(wn == (plant ? 1u : 0u) && gn == wn);
        for (i = 0; i < nFrames; i++) CHECK(wdiff[i] == gdiff[i]);
        if (plant) {
            const size_t pb = planted / 1000000u, po = planted % 1000000u;
            CHECK(gdiff[first[pb] + po / CHUNK] == po % CHUNK);
        }
        CHECK((qzstd_mock_ungroup_cmp_pieces_launches() > l0) == (multi > 0));
        if (round == 0) CHECK(st2[2] == 0 && st2[3] == 0);
        /* refusals: nothing counted */
        if (n > 2 && round) {
            QZSTD_DeviceSrcSlice keep = sl[n - 1];
            QZSTD_frontSliceCheckStats(f, st);
            sl[n - 1].size += 1;
            CHECK(QZSTD_frontFingerprintDeviceSlices(f, kSizes, NBUF, sl, n, NULL, gfp, NULL) == ERR);
            CHECK(QZSTD_frontVerifyDeviceSlices(f, frames, stride, fsizes, nFrames, kSizes, kElems, NBUF, sl, n, NULL, gdiff) == ERR);
            sl[n - 1] = keep;
            CHECK(QZSTD_frontCheckDeviceSlices(f, kSizes, NBUF, sl, n - 1, NULL, wfp, nFrames, gflags) == ERR);
            sl[n - 1].d_src = (const unsigned char *)sl[n - 1].d_src - 1; /* (the last placed first: it begins one byte in front of the pool) */
            if (sl[n - 1].d_src < (const void *)pool) {
                CHECK(QZSTD_frontFingerprintDeviceSlices(f, kSizes, NBUF, sl, n, NULL, gfp, NULL) == ERR);
                CHECK(QZSTD_frontVerifyDeviceSlices(f, frames, stride, fsizes, nFrames, kSizes, kElems, NBUF, sl, n, NULL, gdiff) == ERR);
            }
            sl[n - 1] = keep;
            QZSTD_frontSliceCheckStats(f, st2);
            CHECK(memcmp(st, st2, sizeof(st)) == 0);
        }
        if (plant) { /* the contiguous copy is the next round's again */
            const size_t pb = planted / 1000000u, po = planted % 1000000u;
            ((unsigned char *)(uintptr_t)in[pb].d_ptr)[po] ^= 0x10;
        }
        qzstd_mock_device_range(1, NULL, 0, 0);
        qzstd_mock_extent_range(1, NULL, 0);
        free(pool);
    }
    QZSTD_freeFront(f);
    free(frames);
    free(whole);
    printf("ok\n");
    return 0;
}
