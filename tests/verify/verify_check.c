/*
 * verify_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_verify_host.py builds it with -fsanitize=address,undefined and
 * runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/ (mock_hip_ungroup_cmp.c included):
 * QZSTD_frontVerifyDeviceBatch.  The frame table and the part planning (buffers with a base and without, element sizes 1 / 2 / 4, tails of one
 * byte, parts of one to three frames so that both slots are reused, strided and compacted frames, with and without firstDiff), ZERO rows
 * (delta skip on: frozen buffers between changed ones, a call of zero frames alone), the all-same call, the all-different call (every frame
 * of every buffer changed, the offsets exact), and the undecodable frame (QZSTD_VERIFY_UNDECODED, the front usable again).  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
int qzstd_mock_ungroup_cmp_launches(void);
unsigned long long qzstd_mock_ungroup_cmp_zero_rows(void);
unsigned long long qzstd_mock_ungroup_cmp_stage_bytes(void);

#define GUARD 64u
#define NB 8u
#define MAXFRAMES 64u
#define CHUNK 32768u
#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "verify_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static uint64_t gRng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    gRng ^= gRng << 13; gRng ^= gRng >> 7; gRng ^= gRng << 17;
    return (uint32_t)(gRng >> 16);
}

/* per buffer: size, element size, has a base, frozen (equal to its base) */
static const size_t kSizes[NB] = { 2u * CHUNK + 1u, CHUNK + 255u, 0u, 3u * CHUNK, 1u, CHUNK + 16385u, 2u * CHUNK + 7u, 300u };
static const unsigned char kElems[NB] = { 2, 1, 4, 4, 2, 1, 2, 4 };
static const int kBased[NB] = { 1, 1, 1, 0, 1, 1, 1, 0 };
static const int kFrozen[NB] = { 1, 0, 0, 0, 1, 0, 1, 0 };

/* "device" memory: one registered range, buffer i at place[i] (16-aligned + skew), 0xA5 everywhere else */
typedef struct { unsigned char *base; size_t size, place[NB]; } Pool;

static void poolMake(Pool *p, int slot, unsigned skew, unsigned char *const *datas)
{
    size_t pos = GUARD, i;
    for (i = 0; i < NB; i++) {
        pos = ((pos + 15u) & ~(size_t)15u) + (skew + 3u * i) % 16u;
        p->place[i] = pos;
        pos += kSizes[i];
    }
    p->size = pos + GUARD;
    p->base = (unsigned char *)malloc(p->size);
    CHECK(p->base);
    memset(p->base, 0xA5, p->size);
    for (i = 0; i < NB; i++) memcpy(p->base + p->place[i], datas[i], kSizes[i]);
    qzstd_mock_device_range(slot, p->base, p->size, 0);
}

static QZSTD_Front *makeFront(int useProducer)
{
    QZSTD_FrontParams prm;
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 3;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = useProducer;
    return QZSTD_createFront(&prm);
}

int main(void)
{
    QZSTD_Front *f, *g;
    QZSTD_DeviceBuf in[NB], bs[NB];
    Pool src, bas;
    unsigned char *datas[NB], *bases[NB], *frames, *packed, *snapSrc, *snapBas;
    size_t fsizes[MAXFRAMES], first[NB + 1], diff[MAXFRAMES], lens[MAXFRAMES], bufOf[MAXFRAMES], offOf[MAXFRAMES];
    size_t nFrames, stride, i, c, b, total = 0, nZero = 0, packedSize;
    unsigned long long st[4], st2[4], rs[4], rs2[4], sk[4], sk2[4];
    int skip, part, launches;
    for (i = 0; i < NB; i++) {
        datas[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        bases[i] = (unsigned char *)malloc(kSizes[i] ? kSizes[i] : 1);
        CHECK(datas[i] && bases[i]);
        for (b = 0; b < kSizes[i]; b++) {
            bases[i][b] = (unsigned char)(rnd() & 0x3Fu);
            datas[i][b] = (unsigned char)(bases[i][b] ^ (kFrozen[i] || rnd() % 5u ? 0u : 1u << (rnd() % 7u)));
        }
        if (!kFrozen[i])
            for (b = 0; b < kSizes[i]; b += CHUNK) datas[i][b] ^= 0x80u; /* every frame of a changed buffer differs from its base chunk */
        total += kSizes[i];
    }
    poolMake(&src, 0, 1, datas);
    poolMake(&bas, 1, 8, bases);
    for (i = 0; i < NB; i++) {
        in[i].d_ptr = src.base + src.place[i];
        bs[i].d_ptr = kBased[i] ? bas.base + bas.place[i] : NULL;
        in[i].size = kSizes[i];
        bs[i].size = kBased[i] ? kSizes[i] : 0;
    }
    snapSrc = (unsigned char *)malloc(src.size);
    snapBas = (unsigned char *)malloc(bas.size);
    CHECK(snapSrc && snapBas);
    memcpy(snapSrc, src.base, src.size);
    memcpy(snapBas, bas.base, bas.size);

    for (skip = 0; skip < 2; skip++) {
        for (part = 1; part <= 3; part++) {
            char env[32];
            snprintf(env, sizeof(env), "%u", (unsigned)part * CHUNK);
            CHECK(setenv("QZSTD_FRONT_DEVICE_PART", env, 1) == 0);
            f = makeFront(1);
            g = makeFront(0); /* the verify needs nothing of the producer */
            CHECK(f && g);
            stride = QZSTD_frontFrameStride(f);
            nFrames = QZSTD_frontDeviceBatchFrames(f, in, NB);
            CHECK(nFrames && nFrames <= MAXFRAMES);
            frames = (unsigned char *)malloc(nFrames * stride);
            CHECK(frames);
            CHECK(QZSTD_frontSetDeltaSkip(f, skip) == 0 && QZSTD_frontSetDeltaSkip(g, skip) == 0 && QZSTD_frontSetChecksum(f, part & 1) == 0);
            CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in, bs, kElems, NB, NULL, frames, nFrames * stride, fsizes, first) == nFrames);
            for (i = 0, c = 0, nZero = 0; i < NB; i++)
                for (b = 0; b < kSizes[i]; b += CHUNK, c++) {
                    lens[c] = kSizes[i] - b < CHUNK ? kSizes[i] - b : CHUNK;
                    bufOf[c] = i;
                    offOf[c] = b;
                    if (skip && kBased[i] && kFrozen[i]) nZero++;
                }
            CHECK(c == nFrames);

            /* ---- all the same, on both fronts; the counters; nothing of the caller's written */
            QZSTD_frontVerifyStats(f, st);
            QZSTD_frontRestoreStats(f, rs);
            QZSTD_frontDeltaSkipStats(f, sk);
            launches = qzstd_mock_ungroup_cmp_launches();
            {
                const unsigned long long z0 = qzstd_mock_ungroup_cmp_zero_rows(), s0 = qzstd_mock_ungroup_cmp_stage_bytes();
                unsigned long long stage = 0;
                memset(diff, 0x77, sizeof(diff));
                CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == 0);
                for (c = 0; c < nFrames; c++) {
                    CHECK(diff[c] == QZSTD_VERIFY_SAME);
                    if (!(skip && kBased[bufOf[c]] && kFrozen[bufOf[c]])) stage += (lens[c] + 15u) & ~(size_t)15u;
                }
                CHECK(qzstd_mock_ungroup_cmp_zero_rows() - z0 == nZero && qzstd_mock_ungroup_cmp_stage_bytes() - s0 == stage);
            }
            QZSTD_frontVerifyStats(f, st2);
            QZSTD_frontRestoreStats(f, rs2);
            QZSTD_frontDeltaSkipStats(f, sk2);
            CHECK(st2[0] - st[0] == nFrames && st2[1] == st[1] && st2[2] - st[2] == total);
            {   /* the parts: whole frames, at most part x CHUNK bytes of decoded content; a zero frame joins the part it falls into */
                size_t nParts = 0, bytes = 0;
                for (c = 0; c < nFrames; c++) {
                    const int zero = skip && kBased[bufOf[c]] && kFrozen[bufOf[c]];
                    if (!nParts || (!zero && bytes + lens[c] > (size_t)part * CHUNK)) { nParts++; bytes = 0; }
                    if (!zero) bytes += lens[c];
                }
                CHECK(st2[3] - st[3] == nParts && qzstd_mock_ungroup_cmp_launches() - launches == (int)nParts && nParts > 2u);
            }
            CHECK(memcmp(rs, rs2, sizeof(rs)) == 0 && memcmp(sk, sk2, sizeof(sk)) == 0);
            CHECK(QZSTD_frontVerifyDeviceBatch(g, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, NULL) == 0);
            CHECK(memcmp(snapSrc, src.base, src.size) == 0 && memcmp(snapBas, bas.base, bas.size) == 0);
            /* compacted frames */
            packedSize = 0;
            for (c = 0; c < nFrames; c++) packedSize += fsizes[c];
            packed = (unsigned char *)malloc(packedSize);
            CHECK(packed);
            for (c = 0, b = 0; c < nFrames; b += fsizes[c], c++) memcpy(packed + b, frames + c * stride, fsizes[c]);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, packed, 0, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == 0);

            /* ---- all different: the last byte of every frame's chunk changed on the device, then the first one too */
            for (c = 0; c < nFrames; c++) src.base[src.place[bufOf[c]] + offOf[c] + lens[c] - 1u] ^= 0x10u;
            memset(diff, 0x77, sizeof(diff));
            CHECK(QZSTD_frontVerifyDeviceBatch(f, packed, 0, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == nFrames);
            for (c = 0; c < nFrames; c++) CHECK(diff[c] == lens[c] - 1u);
            for (c = 0; c < nFrames; c += 2) src.base[src.place[bufOf[c]] + offOf[c]] ^= 0x01u;
            CHECK(QZSTD_frontVerifyDeviceBatch(g, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == nFrames);
            for (c = 0; c < nFrames; c++) CHECK(diff[c] == (c % 2u ? lens[c] - 1u : 0u));
            QZSTD_frontVerifyStats(f, st);
            CHECK(st[1] - st2[1] == nFrames);
            memcpy(src.base, snapSrc, src.size);
            /* one bit of a base, at offset 16384 of the frame it falls into (buffer 5, frame 1) */
            bas.base[bas.place[5] + CHUNK + 16384u] ^= 0x02u;
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == 1);
            for (c = 0; c < nFrames; c++) CHECK(diff[c] == (bufOf[c] == 5u && offOf[c] == CHUNK ? 16384u : QZSTD_VERIFY_SAME));
            memcpy(bas.base, snapBas, bas.size);

            /* ---- the undecodable frame: the second frame of buffer 3 (no base, never a zero frame) cut short, then with a bad magic */
            c = first[3] + 1u;
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, NULL) == 0);
            fsizes[c] -= 3u;
            memset(diff, 0x77, sizeof(diff));
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(diff[c] == QZSTD_VERIFY_UNDECODED);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, NULL) == ERR);
            fsizes[c] += 3u;
            frames[c * stride] ^= 0xFFu;
            CHECK(QZSTD_frontVerifyDeviceBatch(g, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(diff[c] == QZSTD_VERIFY_UNDECODED);
            frames[c * stride] ^= 0xFFu;
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == 0);
            CHECK(memcmp(snapSrc, src.base, src.size) == 0 && memcmp(snapBas, bas.base, bas.size) == 0);

            /* ---- refusals before anything is queued */
            launches = qzstd_mock_ungroup_cmp_launches();
            CHECK(QZSTD_frontVerifyDeviceBatch(NULL, frames, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames + 1u, in, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, NULL, stride, fsizes, nFrames, in, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, nFrames, NULL, bs, kElems, NB, NULL, diff) == ERR);
            CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fsizes, 0, in, bs, kElems, 0, NULL, diff) == 0);
            CHECK(qzstd_mock_ungroup_cmp_launches() == launches);

            /* ---- a call of frozen buffers alone (skip on: nothing but ZERO rows, one launch, no stage) */
            if (skip) {
                QZSTD_DeviceBuf in2[2], bs2[2];
                const unsigned char el2[2] = { kElems[0], kElems[6] };
                const unsigned long long s0 = qzstd_mock_ungroup_cmp_stage_bytes();
                size_t n2, fs2[8];
                in2[0] = in[0]; in2[1] = in[6];
                bs2[0] = bs[0]; bs2[1] = bs[6];
                n2 = QZSTD_frontDeviceBatchFrames(f, in2, 2);
                CHECK(n2 == 6u);
                CHECK(QZSTD_frontCompressDeviceBatchDelta(f, in2, bs2, el2, 2, NULL, frames, nFrames * stride, fs2, NULL) == n2);
                launches = qzstd_mock_ungroup_cmp_launches();
                CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fs2, n2, in2, bs2, el2, 2, NULL, diff) == 0);
                CHECK(qzstd_mock_ungroup_cmp_launches() == launches + 1 && qzstd_mock_ungroup_cmp_stage_bytes() == s0);
                src.base[src.place[6] + 2u * CHUNK + 6u] ^= 0x40u;
                CHECK(QZSTD_frontVerifyDeviceBatch(f, frames, stride, fs2, n2, in2, bs2, el2, 2, NULL, diff) == 1 && diff[5] == 6u && diff[4] == QZSTD_VERIFY_SAME);
                memcpy(src.base, snapSrc, src.size);
            }
            free(packed);
            free(frames);
            QZSTD_freeFront(f);
            QZSTD_freeFront(g);
        }
    }
    for (i = 0; i < NB; i++) { free(datas[i]); free(bases[i]); }
    free(src.base);
    free(bas.base);
    free(snapSrc);
    free(snapBas);
    puts("ok");
    return 0;
}
