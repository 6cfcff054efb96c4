/*
 * slices_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_slices_host.py builds it with -fsanitize=address,undefined
 * and runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/: what
 * QZSTD_frontCompressDeviceBatchDelta writes is restored by QZSTD_frontRestoreDeviceSlices — a few thousand random sorted disjoint slices per
 * round, packed into one destination at every alignment, onto the bases' matching slices or in place, over several parts, from strided and
 * from compacted frame lists with every frame no slice needs overwritten — and compared with a plain-C reference of the slicing (the bytes
 * of the original, the frames that intersect a slice counted from the sizes); every refusal returns (size_t)-1 with nothing counted and
 * nothing written.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
int qzstd_mock_ungroup_window_launches(void);
unsigned long long qzstd_mock_ungroup_window_rows(void);
int qzstd_mock_ungroup_launches(void);
int qzstd_mock_ungroup_xor_launches(void);
int qzstd_mock_event_waits(void);

#define CHUNK 32768u
#define NBUF 8u
#define GUARD 64u
#define MAXSLICES 8192u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "slices_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static const size_t kSizes[NBUF] = { 0, 1, 7, 8191, CHUNK, CHUNK + 1, 100001, 4 * CHUNK };
static const unsigned char kElems[NBUF] = { 2, 1, 4, 2, 0, 8, 4, 2 }; /* 0: the front's setting */
static const int kBased[NBUF] = { 1, 1, 0, 1, 1, 0, 1, 1 };

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

static void fill(unsigned char *p, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++) p[i] = (i & 1u) ? (unsigned char)(0x3B + (rnd() & 3u)) : (unsigned char)rnd();
}

/* "device" memory: one registered range, 0xA5 everywhere */
typedef struct { unsigned char *base; size_t size; } Pool;

static void poolMake(Pool *p, int slot, int dev, size_t size)
{
    p->size = size;
    p->base = (unsigned char *)malloc(size);
    CHECK(p->base);
    memset(p->base, 0xA5, size);
    qzstd_mock_device_range(slot, p->base, size, dev);
}

/* random slices, sorted and disjoint, over all buffers: mostly short, a few longer than a frame, some empty, some touching their neighbour;
 * `whole`: every buffer in one slice */
static size_t makeSlices(QZSTD_DeviceSlice *s, int whole)
{
    size_t n = 0, b;
    for (b = 0; b < NBUF; b++) {
        size_t pos = 0;
        if (whole) { s[n].buf = b; s[n].offset = 0; s[n].size = kSizes[b]; n++; continue; }
        for (;;) {
            const uint32_t r = rnd();
            size_t gap = (r & 7u) == 0 ? 0 : (r >> 10) % 40u, len = (r & 0x300u) == 0 ? 0 : (rnd() % 400u == 0 ? rnd() % 70000u : rnd() % 96u);
            if (pos + gap > kSizes[b]) break;
            pos += gap;
            if (len > kSizes[b] - pos) len = kSizes[b] - pos;
            CHECK(n < MAXSLICES);
            s[n].buf = b; s[n].offset = pos; s[n].size = len; n++;
            pos += len;
            if (pos == kSizes[b]) break;
        }
    }
    return n;
}

/* the plain-C reference of the slicing: frames (numbered over all buffers) that intersect a non-empty slice, marked in need[]; -> their count,
 * *pieces: the (slice, frame) pairs, *based: the needed frames of buffers with a base */
static size_t reference(const QZSTD_DeviceSlice *s, size_t n, unsigned char *need, size_t nFrames, const size_t first[NBUF + 1], size_t *pieces,
                        size_t *based)
{
    size_t i, c, cnt = 0;
    memset(need, 0, nFrames);
    *pieces = *based = 0;
    for (i = 0; i < n; i++) {
        if (!s[i].size) continue;
        for (c = s[i].offset / CHUNK; c <= (s[i].offset + s[i].size - 1u) / CHUNK; c++) {
            (*pieces)++;
            if (!need[first[s[i].buf] + c]) { need[first[s[i].buf] + c] = 1; cnt++; if (kBased[s[i].buf]) (*based)++; }
        }
    }
    return cnt;
}

int main(void)
{
    QZSTD_FrontParams prm;
    QZSTD_Front *f, *plain;
    QZSTD_DeviceBuf in[NBUF], bas[NBUF];
    static QZSTD_DeviceSlice sl[MAXSLICES], bad[4];
    Pool src, base, dst, other;
    unsigned char *datas[NBUF], *bases[NBUF], *frames, *work, *want, *need, hostBuf[64];
    size_t sizes[64], csizes[64], first[NBUF + 1], nFrames, stride, i, c, n, pos, total = 0, round;
    unsigned long long st[4], st2[4], rs[4], rs2[4], ds[4], ds2[4];

    CHECK(setenv("QZSTD_FRONT_DEVICE_PART", "98304", 1) == 0); /* three full frames a part: several parts, both slots reused */
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = 1;
    f = QZSTD_createFront(&prm);
    CHECK(f);
    CHECK(QZSTD_frontSetByteGroup(f, 4) == 0);
    stride = QZSTD_frontFrameStride(f);

    for (i = 0; i < NBUF; i++) total += kSizes[i] + 32u;
    poolMake(&src, 0, 0, total);
    poolMake(&base, 1, 0, total);
    poolMake(&dst, 2, 0, total + 4u * MAXSLICES + 2u * GUARD);
    poolMake(&other, 3, 1, 4096);
    want = (unsigned char *)malloc(dst.size);
    CHECK(want);
    for (i = 0, pos = 0; i < NBUF; i++) {
        datas[i] = src.base + pos + (i * 5u) % 16u;
        bases[i] = base.base + pos + (i * 11u + 3u) % 16u;
        fill(datas[i], kSizes[i]);
        for (c = 0; c < kSizes[i]; c++) bases[i][c] = (unsigned char)(datas[i][c] ^ (rnd() % 5u == 0 ? rnd() & 7u : 0u));
        in[i].d_ptr = datas[i];
        in[i].size = kSizes[i];
        bas[i].d_ptr = kBased[i] && kSizes[i] ? bases[i] : NULL;
        bas[i].size = kBased[i] ? kSizes[i] : 0;
        pos += kSizes[i] + 32u;
    }
    nFrames = QZSTD_frontDeviceBatchFrames(f, in, NBUF);
    CHECK(nFrames == 14 && nFrames <= 64);
    frames = (unsigned char *)malloc(nFrames * stride);
    work = (unsigned char *)malloc(nFrames * stride);
    need = (unsigned char *)malloc(nFrames);
    CHECK(frames && work && need);
    CHECK(QZSTD_frontSetChecksum(f, 1) == 0);
    CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bas, kElems, NBUF, NULL, frames, nFrames * stride, sizes, first) == nFrames);
    prm.useProducer = 0;
    plain = QZSTD_createFront(&prm);
    CHECK(plain && QZSTD_frontSetByteGroup(plain, 4) == 0);

    /* rounds: 0 strided frames, bases' slices; 1 compacted frames, in place; 2 strided, a front without the producer, in place; 3 every buffer
     * whole, compacted.  In all of them every frame no slice needs is overwritten with noise first. */
    for (round = 0; round < 4; round++) {
        const int inPlace = round == 1 || round == 2, compacted = round == 1 || round == 3;
        QZSTD_Front *use = round == 2 ? plain : f;
        size_t needed, pieces, based, written = 0, nonEmpty = 0;
        int launches = qzstd_mock_ungroup_window_launches(), oldLaunches = qzstd_mock_ungroup_launches() + qzstd_mock_ungroup_xor_launches();
        unsigned long long rows = qzstd_mock_ungroup_window_rows();
        n = makeSlices(sl, round == 3);
        CHECK(round == 3 || n > 2000);
        needed = reference(sl, n, need, nFrames, first, &pieces, &based);
        memset(dst.base, 0xA5, dst.size);
        memset(want, 0xA5, dst.size);
        for (i = 0, pos = GUARD; i < n; i++) {
            const size_t b = sl[i].buf;
            pos += rnd() % 4u; /* neighbours share 16-byte words, or touch */
            sl[i].d_dst = dst.base + pos;
            sl[i].d_base = !kBased[b] ? NULL : (inPlace ? (const void *)(dst.base + pos) : (const void *)(bases[b] + sl[i].offset));
            if (inPlace && kBased[b]) memcpy(dst.base + pos, bases[b] + sl[i].offset, sl[i].size);
            memcpy(want + pos, datas[b] + sl[i].offset, sl[i].size);
            pos += sl[i].size;
            written += sl[i].size;
            nonEmpty += sl[i].size != 0;
        }
        CHECK(pos + GUARD <= dst.size);
        memcpy(work, frames, nFrames * stride);
        memcpy(csizes, sizes, nFrames * sizeof(sizes[0]));
        for (c = 0; c < nFrames; c++)
            if (!need[c]) for (i = 0; i < csizes[c]; i++) work[c * stride + i] = (unsigned char)rnd();
        if (compacted) (void)QZSTD_frontCompact(f, work, csizes, nFrames);
        QZSTD_frontSliceStats(use, st);
        QZSTD_frontRestoreStats(use, rs);
        QZSTD_frontDeltaStats(use, ds);
        CHECK(QZSTD_frontRestoreDeviceSlices(use, work, compacted ? 0 : stride, csizes, nFrames, kSizes, kElems, NBUF, sl, n, NULL) == needed);
        CHECK(memcmp(dst.base, want, dst.size) == 0);
        QZSTD_frontSliceStats(use, st2);
        QZSTD_frontRestoreStats(use, rs2);
        QZSTD_frontDeltaStats(use, ds2);
        CHECK(st2[0] - st[0] == nonEmpty && st2[1] - st[1] == written && st2[2] - st[2] == needed && st2[3] - st[3] == pieces);
        CHECK(rs2[0] - rs[0] == needed && rs2[3] - rs[3] == (unsigned long long)(qzstd_mock_ungroup_window_launches() - launches));
        CHECK(qzstd_mock_ungroup_window_rows() - rows == pieces && ds2[3] - ds[3] == based);
        CHECK(qzstd_mock_ungroup_launches() + qzstd_mock_ungroup_xor_launches() == oldLaunches);
        CHECK(round != 3 || (needed == nFrames && qzstd_mock_ungroup_window_launches() - launches >= 4));
    }

    /* refusals before anything is queued: no event wait, no launch, nothing counted, nothing written */
    {
        const int launches = qzstd_mock_ungroup_window_launches(), waits = qzstd_mock_event_waits();
        unsigned char elems[NBUF];
        memset(dst.base, 0xA5, dst.size);
        QZSTD_frontSliceStats(f, st);
        QZSTD_frontRestoreStats(f, rs);
        memset(bad, 0, sizeof(bad));
        bad[0].buf = 6; bad[0].offset = 10; bad[0].size = 1000; bad[0].d_dst = dst.base + GUARD; bad[0].d_base = bases[6] + 10;
        bad[1].buf = 6; bad[1].offset = 40000; bad[1].size = 3000; bad[1].d_dst = dst.base + GUARD + 1003; bad[1].d_base = bases[6] + 40000;
#define REFUSED(nf, bs, es, nb, s, ns) CHECK(QZSTD_frontRestoreDeviceSlices(f, frames, stride, sizes, nf, bs, es, nb, s, ns, NULL) == ERR)
        REFUSED(nFrames - 1, kSizes, kElems, NBUF, bad, 2);
        REFUSED(nFrames, kSizes, kElems, NBUF - 1, bad, 2);
        REFUSED(nFrames, NULL, kElems, NBUF, bad, 2);
        REFUSED(nFrames, kSizes, kElems, NBUF, NULL, 2);
        memcpy(elems, kElems, NBUF);
        elems[0] = 3; /* (of a buffer no slice touches: refused all the same, as the Typed call does) */
        REFUSED(nFrames, kSizes, elems, NBUF, bad, 2);
        bad[2] = bad[0]; bad[3] = bad[1];
        bad[0] = bad[3]; bad[1] = bad[2]; /* out of order */
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[0] = bad[2]; bad[1] = bad[3];
        bad[1].offset = 1009; /* overlapping */
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].buf = NBUF;
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].offset = kSizes[6] - 2999; /* ends a byte past its buffer */
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].d_dst = NULL;
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1].d_dst = hostBuf; bad[1].size = 64;
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].d_dst = other.base; /* another device's memory */
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].d_base = other.base;
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        bad[1].d_base = hostBuf; bad[1].size = 64;
        REFUSED(nFrames, kSizes, kElems, NBUF, bad, 2);
        bad[1] = bad[3];
        CHECK(QZSTD_frontRestoreDeviceSlices(NULL, frames, stride, sizes, nFrames, kSizes, kElems, NBUF, bad, 2, NULL) == ERR);
        CHECK(QZSTD_frontRestoreDeviceSlices(f, NULL, stride, sizes, nFrames, kSizes, kElems, NBUF, bad, 2, NULL) == ERR);
        /* nothing to do: 0, and still nothing queued */
        CHECK(QZSTD_frontRestoreDeviceSlices(f, frames, stride, sizes, nFrames, kSizes, kElems, NBUF, NULL, 0, NULL) == 0);
        bad[0].size = bad[1].size = 0;
        CHECK(QZSTD_frontRestoreDeviceSlices(f, frames, stride, sizes, nFrames, kSizes, kElems, NBUF, bad, 2, NULL) == 0);
        bad[0] = bad[2]; bad[1] = bad[3];
        QZSTD_frontSliceStats(f, st2);
        QZSTD_frontRestoreStats(f, rs2);
        CHECK(memcmp(st, st2, sizeof(st)) == 0 && memcmp(rs, rs2, sizeof(rs)) == 0);
        CHECK(qzstd_mock_ungroup_window_launches() == launches && qzstd_mock_event_waits() == waits);
        for (i = 0; i < dst.size; i++) CHECK(dst.base[i] == 0xA5);
        for (i = 0; i < other.size; i++) CHECK(other.base[i] == 0xA5);
        /* after work has started: a needed frame cut short — (size_t)-1, nothing outside the destinations written, the front usable */
        memcpy(csizes, sizes, nFrames * sizeof(sizes[0]));
        csizes[first[6] + 1] -= 3;
        CHECK(QZSTD_frontRestoreDeviceSlices(f, frames, stride, csizes, nFrames, kSizes, kElems, NBUF, bad, 2, NULL) == ERR);
        memset(dst.base + GUARD, 0xA5, 1000);
        memset(dst.base + GUARD + 1003, 0xA5, 3000);
        for (i = 0; i < dst.size; i++) CHECK(dst.base[i] == 0xA5);
        CHECK(QZSTD_frontRestoreDeviceSlices(f, frames, stride, sizes, nFrames, kSizes, kElems, NBUF, bad, 2, NULL) == 2);
        CHECK(memcmp(dst.base + GUARD, datas[6] + 10, 1000) == 0 && memcmp(dst.base + GUARD + 1003, datas[6] + 40000, 3000) == 0);
        CHECK(dst.base[GUARD - 1] == 0xA5 && dst.base[GUARD + 1000] == 0xA5 && dst.base[GUARD + 1002] == 0xA5 && dst.base[GUARD + 4003] == 0xA5);
    }

    QZSTD_freeFront(plain);
    QZSTD_freeFront(f);
    free(frames); free(work); free(need); free(want);
    free(src.base); free(base.base); free(dst.base); free(other.base);
    puts("ok");
    return 0;
}
