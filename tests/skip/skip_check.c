/*
 * skip_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_skip_host.py builds it with -fsanitize=address,undefined and
 * runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/ (mock_hip_diff.c included):
 * delta skip (QZSTD_frontSetDeltaSkip).  The canonical zero frame's writer and recogniser at the edge lengths, with and without checksums
 * (every written frame has the size the layout gives, decodes with libzstd to zeros, and is recognised again by the restore); the compacted
 * frame tables on both sides (equal and changed frames mixed, buffers without a base between them, several parts, fresh buffers and in
 * place, strided and compacted frames); the all-equal call and the none-equal call.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
int qzstd_mock_diff_launches(void);
int qzstd_mock_launches(void);
int qzstd_mock_group_xor_launches(void);
int qzstd_mock_ungroup_xor_launches(void);

#define GUARD 64u
#define MAXBUF 16u
#define MAXFRAMES 64u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "skip_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

/* "device" memory: one registered range, buffer i of size[i] bytes at place[i] (16-aligned + skew), 0xA5 everywhere else */
typedef struct { unsigned char *base; size_t size, place[MAXBUF], n; const size_t *sizes; } Pool;

static void poolMake(Pool *p, int slot, const size_t *sizes, size_t n, unsigned skew)
{
    size_t pos = GUARD, i;
    for (i = 0; i < n; i++) {
        pos = ((pos + 15u) & ~(size_t)15u) + (skew + 3u * i) % 16u;
        p->place[i] = pos;
        pos += sizes[i];
    }
    p->n = n;
    p->sizes = sizes;
    p->size = pos + GUARD;
    p->base = (unsigned char *)malloc(p->size);
    CHECK(p->base);
    memset(p->base, 0xA5, p->size);
    qzstd_mock_device_range(slot, p->base, p->size, 0);
}

static void poolPut(Pool *p, unsigned char *const *datas)
{
    size_t i;
    memset(p->base, 0xA5, p->size);
    for (i = 0; datas && i < p->n; i++) memcpy(p->base + p->place[i], datas[i], p->sizes[i]);
}

/* the pool holds exactly `datas` inside the buffers and 0xA5 elsewhere */
static int poolHolds(const Pool *p, unsigned char *const *datas)
{
    size_t pos = 0, i, b;
    for (i = 0; i <= p->n; i++) {
        const size_t upTo = i < p->n ? p->place[i] : p->size;
        for (b = pos; b < upTo; b++) if (p->base[b] != 0xA5) return 0;
        if (i == p->n) break;
        if (memcmp(p->base + p->place[i], datas[i], p->sizes[i]) != 0) return 0;
        pos = p->place[i] + p->sizes[i];
    }
    return 1;
}

/* the size the canonical zero frame of len bytes has */
static size_t zeroFrameSize(size_t len, int checksum)
{
    return 4u + 1u + (len <= 255u ? 1u : (len <= 65791u ? 2u : 4u)) + 4u * ((len + 131071u) / 131072u) + (checksum ? 4u : 0u);
}

static QZSTD_Front *makeFront(size_t chunk)
{
    QZSTD_FrontParams prm;
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = chunk;
    prm.useProducer = 1;
    return QZSTD_createFront(&prm);
}

/* every buffer equal to its base: the writer and the recogniser at the lengths the sizes give */
static void edgeLengths(size_t chunk, const size_t *sizes, size_t nb, ZSTD_DCtx *zd)
{
    QZSTD_Front *f = makeFront(chunk);
    QZSTD_DeviceBuf in[MAXBUF], bs[MAXBUF];
    QZSTD_DeviceOutBuf out[MAXBUF];
    Pool src, bas, dst;
    unsigned char *datas[MAXBUF], *frames, *content;
    size_t fsizes[MAXFRAMES], first[MAXBUF + 1], nFrames, stride, i, c, b, pos, total = 0;
    unsigned long long sk[4], sk2[4], rs[4], rs2[4];
    int checksum, finds, xors;
    CHECK(f && nb <= MAXBUF);
    stride = QZSTD_frontFrameStride(f);
    poolMake(&src, 0, sizes, nb, 1);
    poolMake(&bas, 1, sizes, nb, 8);
    poolMake(&dst, 2, sizes, nb, 5);
    for (i = 0; i < nb; i++) {
        datas[i] = (unsigned char *)malloc(sizes[i] ? sizes[i] : 1);
        CHECK(datas[i]);
        for (b = 0; b < sizes[i]; b++) datas[i][b] = (unsigned char)rnd();
        in[i].d_ptr = src.base + src.place[i];
        bs[i].d_ptr = bas.base + bas.place[i];
        out[i].d_ptr = dst.base + dst.place[i];
        in[i].size = bs[i].size = out[i].size = sizes[i];
        total += sizes[i];
    }
    poolPut(&src, datas);
    poolPut(&bas, datas);
    nFrames = QZSTD_frontDeviceBatchFrames(f, in, nb);
    CHECK(nFrames && nFrames <= MAXFRAMES);
    frames = (unsigned char *)malloc(nFrames * stride);
    content = (unsigned char *)malloc(chunk);
    CHECK(frames && content);
    CHECK(QZSTD_frontGetDeltaSkip(f) == 0 && QZSTD_frontSetDeltaSkip(f, 1) == 0 && QZSTD_frontGetDeltaSkip(f) == 1);
    for (checksum = 0; checksum < 2; checksum++) {
        CHECK(QZSTD_frontSetChecksum(f, checksum) == 0);
        QZSTD_frontDeltaSkipStats(f, sk);
        finds = qzstd_mock_launches();
        xors = qzstd_mock_group_xor_launches();
        memset(frames, 0xEE, nFrames * stride);
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, NULL, nb, NULL, frames, nFrames * stride, fsizes, first) == nFrames);
        QZSTD_frontDeltaSkipStats(f, sk2);
        /* all equal: nothing staged, nothing matched */
        CHECK(qzstd_mock_launches() == finds && qzstd_mock_group_xor_launches() == xors);
        CHECK(sk2[0] - sk[0] == nFrames && sk2[1] - sk[1] == nFrames && sk2[2] - sk[2] == total);
        for (i = 0; i < nb; i++)
            for (pos = 0, c = first[i]; pos < sizes[i]; pos += chunk, c++) {
                const size_t n = sizes[i] - pos < chunk ? sizes[i] - pos : chunk;
                const unsigned char *fr = frames + c * stride;
                CHECK(fsizes[c] == zeroFrameSize(n, checksum));
                CHECK(fr[fsizes[c]] == 0xEE); /* (nothing written behind the frame) */
                CHECK(((fr[4] >> 2) & 1) == checksum && (fr[4] & 0x20));
                CHECK(ZSTD_decompressDCtx(zd, content, chunk, fr, fsizes[c]) == n); /* (libzstd verifies the checksum) */
                for (b = 0; b < n; b++) CHECK(content[b] == 0);
            }
        /* the recogniser: no frame is decoded; fresh buffers get the base's bytes, in place nothing happens */
        QZSTD_frontRestoreStats(f, rs);
        poolPut(&dst, NULL);
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, fsizes, nFrames, out, bs, NULL, nb, NULL) == nFrames);
        CHECK(poolHolds(&dst, datas));
        for (i = 0; i < nb; i++) out[i].d_ptr = bas.base + bas.place[i];
        CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, fsizes, nFrames, out, bs, NULL, nb, NULL) == nFrames);
        CHECK(poolHolds(&bas, datas));
        for (i = 0; i < nb; i++) out[i].d_ptr = dst.base + dst.place[i];
        QZSTD_frontRestoreStats(f, rs2);
        QZSTD_frontDeltaSkipStats(f, sk);
        CHECK(memcmp(rs, rs2, sizeof(rs)) == 0 && sk[3] - sk2[3] == 2u * nFrames);
        /* a zero frame damaged in its last byte is no zero frame: it is decoded (and, with a checksum, fails) */
        frames[fsizes[0] - 1] ^= 0x40;
        poolPut(&dst, NULL);
        if (checksum) {
            CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, fsizes, nFrames, out, bs, NULL, nb, NULL) == ERR);
        } else {
            /* (the RLE byte is now 0x40: a valid frame of another content) */
            const size_t n0 = sizes[0] < chunk ? sizes[0] : chunk;
            CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, fsizes, nFrames, out, bs, NULL, nb, NULL) == nFrames);
            QZSTD_frontRestoreStats(f, rs);
            CHECK(rs[0] - rs2[0] == 1);
            if (n0 <= 131072u) for (b = 0; b < n0; b++) CHECK(dst.base[dst.place[0] + b] == (datas[0][b] ^ 0x40));
        }
        frames[fsizes[0] - 1] ^= 0x40;
    }
    /* the setting off: the same frames are decoded like any other, to the same bytes */
    CHECK(QZSTD_frontSetDeltaSkip(f, 0) == 0);
    QZSTD_frontRestoreStats(f, rs);
    poolPut(&dst, NULL);
    CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, frames, stride, fsizes, nFrames, out, bs, NULL, nb, NULL) == nFrames);
    QZSTD_frontRestoreStats(f, rs2);
    CHECK(poolHolds(&dst, datas) && rs2[0] - rs[0] == nFrames);
    QZSTD_freeFront(f);
    for (i = 0; i < nb; i++) free(datas[i]);
    free(frames); free(content);
    free(src.base); free(bas.base); free(dst.base);
}

/* equal and changed frames mixed: the tables of both sides leave frames out */
#define CHUNK 32768u
#define NMIX 9u
static const size_t kMix[NMIX] = { 4 * CHUNK + 5, 100, 3 * CHUNK, 0, CHUNK + 1, 2 * CHUNK + 77, 5 * CHUNK + 9, 7, 2 * CHUNK };
static const unsigned char kElems[NMIX] = { 2, 1, 4, 2, 8, 2, 4, 1, 2 };
/* per buffer: bit c set = frame c differs from the base */
static const unsigned kChanged[NMIX] = { 0x0A, 0, 0x7, 0, 0x2, 0, 0x11, 1, 0 };
static int mixBased(size_t i) { return i != 5u; } /* buffer 5: zeros without a base */

static void mixed(ZSTD_DCtx *zd)
{
    QZSTD_Front *f;
    QZSTD_DeviceBuf in[NMIX], bs[NMIX], inPlace[NMIX];
    QZSTD_DeviceOutBuf out[NMIX];
    Pool src, bas, dst, place;
    unsigned char *datas[NMIX], *bases[NMIX], *off, *on, *compacted, *content;
    size_t offSizes[MAXFRAMES], onSizes[MAXFRAMES], first[NMIX + 1], nFrames, stride, i, c, b, pos, nBased = 0, nEqual = 0, total = 0;
    unsigned long long sk[4], sk2[4], rs[4], rs2[4], dv[4], dv2[4], ds[4], ds2[4];
    int checksum, part, diffs;
    for (part = 0; part < 2; part++) {
        CHECK(setenv("QZSTD_FRONT_DEVICE_PART", part ? "98304" : "1000000000", 1) == 0); /* three frames a part, or one part */
        f = makeFront(CHUNK);
        CHECK(f);
        stride = QZSTD_frontFrameStride(f);
        poolMake(&src, 0, kMix, NMIX, 2);
        poolMake(&bas, 1, kMix, NMIX, 11);
        poolMake(&dst, 2, kMix, NMIX, 7);
        poolMake(&place, 3, kMix, NMIX, 4);
        nBased = nEqual = total = 0;
        for (i = 0; i < NMIX; i++) {
            datas[i] = (unsigned char *)malloc(kMix[i] ? kMix[i] : 1);
            bases[i] = (unsigned char *)malloc(kMix[i] ? kMix[i] : 1);
            CHECK(datas[i] && bases[i]);
            for (b = 0; b < kMix[i]; b++) datas[i][b] = mixBased(i) ? ((b & 1u) ? (unsigned char)(0x3B + (rnd() & 3u)) : (unsigned char)rnd()) : 0;
            memcpy(bases[i], datas[i], kMix[i]);
            for (pos = 0, c = 0; pos < kMix[i]; pos += CHUNK, c++) {
                const size_t n = kMix[i] - pos < CHUNK ? kMix[i] - pos : CHUNK;
                if (!mixBased(i)) continue;
                nBased++;
                if (kChanged[i] >> c & 1u) bases[i][pos + (c & 1u ? n - 1u : n / 2u)] ^= 0x04; /* one bit: the frame's last byte, or its middle */
                else nEqual++;
            }
            in[i].d_ptr = src.base + src.place[i];
            bs[i].d_ptr = mixBased(i) ? bas.base + bas.place[i] : NULL;
            out[i].d_ptr = dst.base + dst.place[i];
            inPlace[i].d_ptr = mixBased(i) ? place.base + place.place[i] : NULL;
            in[i].size = out[i].size = kMix[i];
            bs[i].size = inPlace[i].size = mixBased(i) ? kMix[i] : 0;
            total += kMix[i];
        }
        poolPut(&src, datas);
        poolPut(&bas, bases);
        nFrames = QZSTD_frontDeviceBatchFrames(f, in, NMIX);
        CHECK(nFrames && nFrames <= MAXFRAMES && nEqual && nEqual < nBased);
        off = (unsigned char *)malloc(nFrames * stride);
        on = (unsigned char *)malloc(nFrames * stride);
        compacted = (unsigned char *)malloc(nFrames * stride);
        content = (unsigned char *)malloc(CHUNK);
        CHECK(off && on && compacted && content);
        for (checksum = 0; checksum < 2; checksum++) {
            CHECK(QZSTD_frontSetChecksum(f, checksum) == 0);
            /* off: no comparison */
            CHECK(QZSTD_frontSetDeltaSkip(f, 0) == 0);
            diffs = qzstd_mock_diff_launches();
            QZSTD_frontDeltaSkipStats(f, sk);
            CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NMIX, NULL, off, nFrames * stride, offSizes, NULL) == nFrames);
            QZSTD_frontDeltaSkipStats(f, sk2);
            CHECK(qzstd_mock_diff_launches() == diffs && memcmp(sk, sk2, sizeof(sk)) == 0);
            /* on: the changed frames are the setting-off frames, the equal ones zero frames */
            CHECK(QZSTD_frontSetDeltaSkip(f, 1) == 0);
            QZSTD_frontDeltaStats(f, dv);
            QZSTD_frontDeviceStats(f, ds);
            memset(on, 0xEE, nFrames * stride);
            CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NMIX, NULL, on, nFrames * stride, onSizes, first) == nFrames);
            QZSTD_frontDeltaSkipStats(f, sk);
            QZSTD_frontDeltaStats(f, dv2);
            QZSTD_frontDeviceStats(f, ds2);
            CHECK(qzstd_mock_diff_launches() == diffs + 1);
            CHECK(sk[0] - sk2[0] == nBased && sk[1] - sk2[1] == nEqual && sk[3] == sk2[3]);
            CHECK(dv2[0] + dv2[1] + dv2[2] - dv[0] - dv[1] - dv[2] == nBased - nEqual);
            CHECK(ds2[0] + ds2[1] - ds[0] - ds[1] == nFrames - nEqual && ds2[3] - ds[3] == total);
            for (i = 0; i < NMIX; i++)
                for (pos = 0, c = 0; pos < kMix[i]; pos += CHUNK, c++) {
                    const size_t n = kMix[i] - pos < CHUNK ? kMix[i] - pos : CHUNK, g = first[i] + c;
                    if (mixBased(i) && !(kChanged[i] >> c & 1u)) {
                        CHECK(onSizes[g] == zeroFrameSize(n, checksum));
                        CHECK(ZSTD_decompressDCtx(zd, content, CHUNK, on + g * stride, onSizes[g]) == n);
                        for (b = 0; b < n; b++) CHECK(content[b] == 0);
                    } else {
                        /* (buffer 5 too: zeros without a base are never compared and never skipped) */
                        CHECK(onSizes[g] == offSizes[g] && memcmp(on + g * stride, off + g * stride, onSizes[g]) == 0);
                    }
                }
            for (i = 0; i < NMIX; i++)
                CHECK(memcmp(src.base + src.place[i], datas[i], kMix[i]) == 0 && (!mixBased(i) || memcmp(bas.base + bas.place[i], bases[i], kMix[i]) == 0));
            /* back, into fresh buffers: only the other frames are decoded */
            QZSTD_frontRestoreStats(f, rs);
            QZSTD_frontDeltaStats(f, dv);
            poolPut(&dst, NULL);
            CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, on, stride, onSizes, nFrames, out, bs, kElems, NMIX, NULL) == nFrames);
            CHECK(poolHolds(&dst, datas));
            QZSTD_frontRestoreStats(f, rs2);
            QZSTD_frontDeltaStats(f, dv2);
            QZSTD_frontDeltaSkipStats(f, sk2);
            CHECK(rs2[0] - rs[0] == nFrames - nEqual && dv2[3] - dv[3] == nBased - nEqual && sk2[3] - sk[3] == nEqual);
            /* in place over the bases, from compacted frames */
            poolPut(&place, datas);
            for (i = 0; i < NMIX; i++) {
                if (mixBased(i)) memcpy(place.base + place.place[i], bases[i], kMix[i]);
                out[i].d_ptr = place.base + place.place[i];
            }
            memcpy(compacted, on, nFrames * stride);
            (void)QZSTD_frontCompact(f, compacted, onSizes, nFrames);
            CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, compacted, 0, onSizes, nFrames, out, inPlace, kElems, NMIX, NULL) == nFrames);
            CHECK(poolHolds(&place, datas));
            QZSTD_frontRestoreStats(f, rs);
            CHECK(rs[0] - rs2[0] == nFrames - nEqual);
            /* the setting off on the way back: every frame decoded, the same bytes */
            CHECK(QZSTD_frontSetDeltaSkip(f, 0) == 0);
            for (i = 0; i < NMIX; i++) out[i].d_ptr = dst.base + dst.place[i];
            poolPut(&dst, NULL);
            CHECK(QZSTD_frontRestoreDeviceBatchDelta(f, on, stride, onSizes, nFrames, out, bs, kElems, NMIX, NULL) == nFrames);
            QZSTD_frontRestoreStats(f, rs2);
            CHECK(poolHolds(&dst, datas) && rs2[0] - rs[0] == nFrames);
        }
        /* none equal: every frame of a based buffer changed — the comparison runs, nothing is skipped, the frames are the setting-off frames */
        for (i = 0; i < NMIX; i++) {
            if (!mixBased(i)) continue;
            for (pos = 0; pos < kMix[i]; pos += CHUNK) bas.base[bas.place[i] + pos] = (unsigned char)(datas[i][pos] ^ 0x80);
        }
        CHECK(QZSTD_frontSetDeltaSkip(f, 0) == 0);
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NMIX, NULL, off, nFrames * stride, offSizes, NULL) == nFrames);
        CHECK(QZSTD_frontSetDeltaSkip(f, 1) == 0);
        QZSTD_frontDeltaSkipStats(f, sk);
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NMIX, NULL, on, nFrames * stride, onSizes, NULL) == nFrames);
        QZSTD_frontDeltaSkipStats(f, sk2);
        CHECK(sk2[0] - sk[0] == nBased && sk2[1] == sk[1]);
        for (c = 0; c < nFrames; c++) CHECK(onSizes[c] == offSizes[c] && memcmp(on + c * stride, off + c * stride, onSizes[c]) == 0);
        /* a call without any base is not compared at all */
        diffs = qzstd_mock_diff_launches();
        CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, NULL, kElems, NMIX, NULL, on, nFrames * stride, onSizes, NULL) == nFrames);
        CHECK(qzstd_mock_diff_launches() == diffs);
        CHECK(QZSTD_frontSetDeltaSkip(NULL, 1) == -1 && QZSTD_frontGetDeltaSkip(NULL) == 0);
        QZSTD_freeFront(f);
        for (i = 0; i < NMIX; i++) { free(datas[i]); free(bases[i]); }
        free(off); free(on); free(compacted); free(content);
        free(src.base); free(bas.base); free(dst.base); free(place.base);
    }
}

int main(void)
{
    static const size_t edgeA[] = { 1, 15, 255, 256, 4095, 65791, 65792, 131071, 131072, 131073, 2 * 131072 + 16 };
    static const size_t edgeB[] = { 131073, 262144, 262147, 262147 + 131072 };
    ZSTD_DCtx *zd = ZSTD_createDCtx();
    CHECK(zd);
    edgeLengths(131072, edgeA, sizeof(edgeA) / sizeof(edgeA[0]), zd);
    edgeLengths(262147, edgeB, sizeof(edgeB) / sizeof(edgeB[0]), zd); /* chunks of two blocks and a tail */
    mixed(zd);
    ZSTD_freeDCtx(zd);
    puts("ok");
    return 0;
}
