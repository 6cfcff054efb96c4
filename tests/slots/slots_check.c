/*
 * slots_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_slots_host.py builds it with -fsanitize=address,undefined
 * and runs it as a process of its own, leak detection on) over the front-end, qatseqprod.c and the mock device layer of tests/mock/: ONE
 * front used on two devices in turn — device 0, device 1, device 0 again — so that the slots a front keeps between calls (the compress
 * side's and the restore side's: streams, pinned and device buffers) are freed and rebuilt on every change of device, not only by
 * QZSTD_freeFront.  Every round is a Delta compress with checksum, byte grouping, delta skip, plane probe and plane code on, a Delta
 * restore, a verify, a fingerprint + check and an advise over three small buffers; the frames are byte-equal to the first round's, the
 * restored bytes equal the input and the fingerprints are equal.  A buffer that a free forgets is a leak the sanitizer reports.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);

#define CHUNK 16400u
#define NBUF 3u
#define NFRAMES 4u /* 0 + 1 + 3 */
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "slots_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 2 * CHUNK + 5 };
static const unsigned char kElems[NBUF] = { 2, 1, 4 };

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

/* one device's memory: the buffers, their bases and the restore's destinations in ONE registered block, at odd offsets */
typedef struct {
    unsigned char *block;
    QZSTD_DeviceBuf in[NBUF], bas[NBUF], back[NBUF]; /* back: the restore's destinations as a call's input */
    QZSTD_DeviceOutBuf out[NBUF];
} Side;

static void sideMake(Side *s, const Side *like, int range, int dev)
{
    const size_t room = 3 * (kSizes[0] + kSizes[1] + kSizes[2]) + 64 * NBUF;
    size_t pos = 0, b, i;
    s->block = (unsigned char *)malloc(room);
    CHECK(s->block);
    memset(s->block, 0xA5, room);
    qzstd_mock_device_range(range, s->block, room, dev);
    for (b = 0; b < NBUF; b++) {
        unsigned char *d = s->block + pos + 1 + b, *base = d + kSizes[b] + 7, *o = base + kSizes[b] + 3;
        for (i = 0; i < kSizes[b]; i++) {
            if (like) {
                d[i] = ((const unsigned char *)like->in[b].d_ptr)[i];
                base[i] = ((const unsigned char *)like->bas[b].d_ptr)[i];
            } else {
                /* a noisy low byte under quiet high bytes; the last buffer's base equals it in the first chunk and differs in every eighth byte
                 * behind it, the one-byte buffer's differs */
                d[i] = (i & 3u) == 0 ? (unsigned char)rnd() : (unsigned char)(0x3B + (rnd() & 3u));
                base[i] = (unsigned char)(d[i] ^ (b == 1 ? 1u : (i >= CHUNK && i % 8u == 0 ? 1u + (rnd() & 3u) : 0u)));
            }
        }
        s->in[b].d_ptr = d; s->in[b].size = kSizes[b];
        s->bas[b].d_ptr = base; s->bas[b].size = kSizes[b];
        s->out[b].d_ptr = o; s->out[b].size = kSizes[b];
        s->back[b].d_ptr = o; s->back[b].size = kSizes[b];
        pos += 3 * kSizes[b] + 40;
    }
    CHECK(pos <= room);
}

int main(void)
{
    QZSTD_FrontParams prm;
    QZSTD_Front *f;
    Side side[2];
    unsigned char *frames0, *frames, advised0[NBUF], advised[NBUF], differs[NFRAMES];
    unsigned long long fp0[NFRAMES], fp[NFRAMES], st[4];
    size_t sizes0[NFRAMES], sizes[NFRAMES], first[NBUF + 1], firstDiff[NFRAMES], stride, round, b, c;

    CHECK(setenv("QZSTD_FRONT_DEVICE_PART", "16400", 1) == 0); /* a frame a part: both slots of either family are used */
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = 1;
    f = QZSTD_createFront(&prm);
    CHECK(f);
    stride = QZSTD_frontFrameStride(f);
    CHECK(QZSTD_frontSetChecksum(f, 1) == 0 && QZSTD_frontSetByteGroup(f, 2) == 0 && QZSTD_frontSetDeltaSkip(f, 1) == 0 &&
          QZSTD_frontSetPlaneProbe(f, 1) == 0 && QZSTD_frontSetPlaneCode(f, 1) == 0);
    sideMake(&side[0], NULL, 0, 0);
    sideMake(&side[1], &side[0], 1, 1);
    frames0 = (unsigned char *)malloc(NFRAMES * stride);
    frames = (unsigned char *)malloc(NFRAMES * stride);
    CHECK(frames0 && frames);
    for (round = 0; round < 3; round++) {
        const Side *s = &side[round & 1u]; /* device 0, device 1, device 0 again */
        unsigned char *fr = round ? frames : frames0;
        size_t *sz = round ? sizes : sizes0;
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, s->in, s->bas, kElems, NBUF, NULL, fr, NFRAMES * stride, sz, first) == NFRAMES);
        CHECK(first[0] == 0 && first[1] == 0 && first[2] == 1 && first[3] == NFRAMES);
        for (c = 0; round && c < NFRAMES; c++)
            CHECK(sizes[c] == sizes0[c] && memcmp(frames + c * stride, frames0 + c * stride, sizes0[c]) == 0);
        for (b = 0; b < NBUF; b++) memset(s->out[b].d_ptr, 0x5A, kSizes[b]);
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, fr, stride, sz, NFRAMES, s->out, s->bas, kElems, NBUF, NULL) == NFRAMES);
        for (b = 0; b < NBUF; b++) CHECK(memcmp(s->out[b].d_ptr, s->in[b].d_ptr, kSizes[b]) == 0);
        CHECK(QZSTD_frontVerifyDeviceBatch(f, fr, stride, sz, NFRAMES, s->in, s->bas, kElems, NBUF, NULL, firstDiff) == 0);
        for (c = 0; c < NFRAMES; c++) CHECK(firstDiff[c] == QZSTD_VERIFY_SAME);
        CHECK(QZSTD_frontFingerprintDeviceBatch(f, s->in, NBUF, NULL, round ? fp : fp0, first) == NFRAMES);
        CHECK(round == 0 || memcmp(fp, fp0, sizeof(fp0)) == 0);
        CHECK(QZSTD_frontCheckDeviceBatch(f, s->back, NBUF, NULL, fp0, NFRAMES, differs) == 0);
        CHECK(QZSTD_frontAdviseDeviceBatch(f, s->in, kElems, NBUF, NULL, round ? advised : advised0, NULL) != ERR);
        CHECK(round == 0 || memcmp(advised, advised0, sizeof(advised0)) == 0);
    }
    /* the first chunk of the last buffer equals its base: found on the device in every round, recognised by every restore */
    QZSTD_frontDeltaSkipStats(f, st);
    CHECK(st[1] == 3u && st[3] == 3u);
    QZSTD_freeFront(f);
    free(frames0);
    free(frames);
    for (b = 0; b < 2; b++) {
        qzstd_mock_device_range((int)b, NULL, 0, 0);
        free(side[b].block);
    }
    printf("ok\n");
    return 0;
}
