/*
 * fingerprint_check.c — TEST INFRASTRUCTURE ONLY.  A stand-alone program (tests/test_fingerprint_host.py builds it with
 * -fsanitize=address,undefined and runs it as a process of its own) over the front-end, qatseqprod.c and the mock device layer of tests/mock/
 * (mock_hip_fingerprint.c included): the fingerprint of include/qzstd_fingerprint.h and the two calls that take it on device buffers
 * (QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch).
 *
 * The definition: at the edge lengths every input lives in a heap block of EXACTLY its length (a read at or beyond n is the sanitizer's to
 * catch), QZSTD_fingerprint is the fold of its tiles' digests, and the properties hold ON THE INPUTS GIVEN, not statistically — one bit
 * flipped in the first byte, the last byte and on either side of the 4096 and 16384 boundaries, two words of one lane swapped (w and
 * w + 256), two neighbouring words swapped (neighbouring lanes), two tiles swapped, a zero byte appended: each changes the value.  The GPU
 * tests assert the same pairs (tools/qz_device.py: fp_corpus is fill() below), so a "differs" that fails there is a kernel that is not the
 * definition, never bad luck.  The calls: a mixed batch at odd alignments, fingerprints equal to the function's, firstFrame, Check's count
 * and flags after one bit, a whole frame and the order of two frames change, the refusals, a front without the producer.  Prints "ok".
 */
#include "qatseqprod.h" /* (the libzstd declarations the library itself builds with) */
#include "qzstd_fingerprint.h"
#include "qzstd_frontend.h"
#include "qzstd_frontend_device.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev);
int qzstd_mock_fingerprint_launches(void);
unsigned long long qzstd_mock_fingerprint_rows(void);
unsigned long long qzstd_mock_fingerprint_tiles(void);

#define ERR ((size_t)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "fingerprint_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

/* byte i of the input with this seed (tools/qz_device.py: fp_corpus) */
static void fill(unsigned char *p, size_t n, uint32_t seed)
{
    size_t i;
    for (i = 0; i < n; i++) {
        uint32_t x = (uint32_t)i * 2654435761u + seed * 2246822519u;
        x ^= x >> 15;
        x *= 2246822519u;
        x ^= x >> 13;
        p[i] = (unsigned char)x;
    }
}

/* a heap block of exactly n bytes (n = 0: one byte that is never passed on as content) */
static unsigned char *exact(size_t n, uint32_t seed)
{
    unsigned char *p = (unsigned char *)malloc(n ? n : 1);
    CHECK(p);
    fill(p, n, seed);
    return p;
}

static void swapBytes(unsigned char *a, unsigned char *b, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++) { const unsigned char t = a[i]; a[i] = b[i]; b[i] = t; }
}

#define NLEN 12u
static const size_t kLens[NLEN] = { 0, 1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 5 };

static void definition(void)
{
    static const size_t flipAt[] = { 4095, 4096, 16383, 16384 };
    uint64_t seen[NLEN];
    size_t k, j;
    for (k = 0; k < NLEN; k++) {
        const size_t n = kLens[k], nt = (size_t)QZSTD_FP_TILES(n);
        unsigned char *p = exact(n, 11u + (uint32_t)k), *q;
        uint64_t tiles[4], v, w;
        CHECK(nt <= 4u && nt == (n + 16383u) / 16384u);
        for (j = 0; j < nt; j++) tiles[j] = QZSTD_fpTile(p + j * 16384u, n - j * 16384u < 16384u ? (uint32_t)(n - j * 16384u) : 16384u);
        v = QZSTD_fingerprint(p, n);
        CHECK(v == QZSTD_fpFold(tiles, nt, n) && v == QZSTD_fingerprintOf(p, n));
        if (n == 0) CHECK(v == QZSTD_fpAvalanche(QZSTD_FP_P5) && QZSTD_fingerprintOf(NULL, 0) == v);
        for (j = 0; j < k; j++) CHECK(seen[j] != v);
        seen[k] = v;
        /* the same bytes at another address and alignment: the same value */
        q = (unsigned char *)malloc(n + 3u);
        CHECK(q);
        if (n) memcpy(q + 3, p, n);
        CHECK(QZSTD_fingerprint(q + 3, n) == v);
        free(q);
        /* one bit: the first byte, the last byte, either side of the boundaries */
        if (n) {
            p[0] ^= 0x01; CHECK(QZSTD_fingerprint(p, n) != v); p[0] ^= 0x01;
            p[n - 1] ^= 0x80; CHECK(QZSTD_fingerprint(p, n) != v); p[n - 1] ^= 0x80;
        }
        for (j = 0; j < sizeof(flipAt) / sizeof(flipAt[0]); j++) {
            if (flipAt[j] >= n) continue;
            p[flipAt[j]] ^= 0x10; CHECK(QZSTD_fingerprint(p, n) != v); p[flipAt[j]] ^= 0x10;
        }
        CHECK(QZSTD_fingerprint(p, n) == v);
        /* a zero byte appended (in a block of exactly n + 1 bytes) */
        q = (unsigned char *)malloc(n + 1u);
        CHECK(q);
        if (n) memcpy(q, p, n);
        q[n] = 0;
        w = QZSTD_fingerprint(q, n + 1u);
        CHECK(w != v);
        free(q);
        /* words of one lane (w and w + 256), neighbouring words (neighbouring lanes) */
        if (n >= 16u * 260u) {
            CHECK(memcmp(p + 16u * 3u, p + 16u * 259u, 16) != 0 && memcmp(p + 16u * 3u, p + 16u * 4u, 16) != 0);
            swapBytes(p + 16u * 3u, p + 16u * 259u, 16); CHECK(QZSTD_fingerprint(p, n) != v); swapBytes(p + 16u * 3u, p + 16u * 259u, 16);
            swapBytes(p + 16u * 3u, p + 16u * 4u, 16); CHECK(QZSTD_fingerprint(p, n) != v); swapBytes(p + 16u * 3u, p + 16u * 4u, 16);
        }
        /* two tiles */
        if (n >= 2u * 16384u) {
            CHECK(memcmp(p, p + 16384u, 16384u) != 0);
            swapBytes(p, p + 16384u, 16384u); CHECK(QZSTD_fingerprint(p, n) != v); swapBytes(p, p + 16384u, 16384u);
        }
        CHECK(QZSTD_fingerprint(p, n) == v);
        free(p);
    }
    /* the lanes without a word are merged all the same: one byte and sixteen zero-extended bytes are not the same input */
    {
        unsigned char one[1] = { 0x5A }, wide[16] = { 0x5A };
        CHECK(QZSTD_fingerprint(one, 1) != QZSTD_fingerprint(wide, 16));
        CHECK(QZSTD_fpTile(one, 1) == QZSTD_fpTile(wide, 16)); /* (the tile digest does not know the length: the fold does) */
    }
}

/* "device" memory: one registered range, buffer i at a 16-aligned place + skew, 0xA5 everywhere else */
#define CHUNK 131072u
#define NB 6u
#define GUARD 64u
static const size_t kSizes[NB] = { 0, 256, 65791, CHUNK + 255u, 2u * CHUNK + 1u, 3u * CHUNK + 9u };
#define NFRAMES (0u + 1u + 1u + 2u + 3u + 4u)

typedef struct { unsigned char *base; size_t size, place[NB]; } Pool;

static void poolMake(Pool *p, int slot, unsigned skew)
{
    size_t pos = GUARD, i;
    for (i = 0; i < NB; i++) {
        pos = ((pos + 15u) & ~(size_t)15u) + (skew + 5u * i) % 16u;
        p->place[i] = pos;
        pos += kSizes[i];
    }
    p->size = pos + GUARD;
    p->base = (unsigned char *)malloc(p->size);
    CHECK(p->base);
    memset(p->base, 0xA5, p->size);
    for (i = 0; i < NB; i++) fill(p->base + p->place[i], kSizes[i], 40u + (uint32_t)i);
    qzstd_mock_device_range(slot, p->base, p->size, 0);
}

static QZSTD_Front *makeFront(int useProducer)
{
    QZSTD_FrontParams prm;
    memset(&prm, 0, sizeof(prm));
    prm.nThreads = 2;
    prm.level = 1;
    prm.chunkSize = CHUNK;
    prm.useProducer = useProducer;
    return QZSTD_createFront(&prm);
}

static void calls(int useProducer)
{
    QZSTD_Front *f = makeFront(useProducer);
    QZSTD_DeviceBuf in[NB], bad[NB];
    Pool pool;
    unsigned char *copy, differs[NFRAMES], host[64];
    unsigned long long fp[NFRAMES + 1], want[NFRAMES], st[4], st2[4], t;
    size_t first[NB + 1], i, c, pos, total = 0, tiles = 0;
    int launches;
    CHECK(f);
    poolMake(&pool, 0, 3);
    copy = (unsigned char *)malloc(pool.size);
    CHECK(copy);
    memcpy(copy, pool.base, pool.size);
    for (i = 0, c = 0; i < NB; i++) {
        in[i].d_ptr = kSizes[i] ? pool.base + pool.place[i] : NULL;
        in[i].size = kSizes[i];
        total += kSizes[i];
        for (pos = 0; pos < kSizes[i]; pos += CHUNK, c++) {
            const size_t n = kSizes[i] - pos < CHUNK ? kSizes[i] - pos : CHUNK;
            want[c] = QZSTD_fingerprintOf(copy + pool.place[i] + pos, n);
            tiles += (n + 16383u) / 16384u;
        }
    }
    CHECK(c == NFRAMES && QZSTD_frontDeviceBatchFrames(f, in, NB) == NFRAMES);
    QZSTD_frontFingerprintStats(f, st);
    CHECK(st[0] == 0 && st[1] == 0 && st[2] == 0 && st[3] == 0);
    launches = qzstd_mock_fingerprint_launches();
    t = qzstd_mock_fingerprint_tiles();
    memset(fp, 0xEE, sizeof(fp));
    memset(first, 0xEE, sizeof(first));
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, NB, NULL, fp, first) == NFRAMES);
    CHECK(memcmp(fp, want, sizeof(want)) == 0 && fp[NFRAMES] == 0xEEEEEEEEEEEEEEEEull);
    CHECK(first[0] == 0 && first[1] == 0 && first[2] == 1 && first[3] == 2 && first[4] == 4 && first[5] == 7 && first[6] == NFRAMES);
    CHECK(qzstd_mock_fingerprint_launches() == launches + 1 && qzstd_mock_fingerprint_tiles() - t == tiles);
    CHECK(memcmp(copy, pool.base, pool.size) == 0); /* the buffers are only read */
    QZSTD_frontFingerprintStats(f, st);
    CHECK(st[0] == NFRAMES && st[1] == total && st[2] == 1 && st[3] == 0);
    /* Check: the same buffers, then one bit, a whole frame, and two frames' fingerprints in the wrong order */
    memset(differs, 7, sizeof(differs));
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES, differs) == 0);
    for (c = 0; c < NFRAMES; c++) CHECK(differs[c] == 0);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES, NULL) == 0);
    pool.base[pool.place[4] + CHUNK + 77u] ^= 0x04; /* buffer 4, frame 1: call frame 5 */
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES, differs) == 1);
    for (c = 0; c < NFRAMES; c++) CHECK(differs[c] == (c == 5u));
    memset(pool.base + pool.place[5] + 3u * CHUNK, 0, 9); /* buffer 5's tail of 9 bytes: call frame 10 */
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES, differs) == 2);
    for (c = 0; c < NFRAMES; c++) CHECK(differs[c] == (c == 5u || c == 10u));
    memcpy(pool.base, copy, pool.size);
    t = fp[7]; fp[7] = fp[8]; fp[8] = t; /* buffer 5's first two frames, kept in the wrong order */
    CHECK(want[7] != want[8]);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES, differs) == 2);
    for (c = 0; c < NFRAMES; c++) CHECK(differs[c] == (c == 7u || c == 8u));
    t = fp[7]; fp[7] = fp[8]; fp[8] = t;
    QZSTD_frontFingerprintStats(f, st2);
    CHECK(st2[0] == 6u * NFRAMES && st2[1] == 6u * total && st2[2] == 6 && st2[3] == 5);
    /* a slice of whole chunks is a list of buffers like any other: buffer 5's frames 1 and 2 alone */
    {
        QZSTD_DeviceBuf part;
        part.d_ptr = pool.base + pool.place[5] + CHUNK;
        part.size = 2u * CHUNK;
        CHECK(QZSTD_frontCheckDeviceBatch(f, &part, 1, NULL, fp + 8, 2, differs) == 0 && differs[0] == 0 && differs[1] == 0);
    }
    /* refusals: nothing is launched, counted or written */
    launches = qzstd_mock_fingerprint_launches();
    QZSTD_frontFingerprintStats(f, st);
    memset(differs, 7, sizeof(differs));
    CHECK(QZSTD_frontFingerprintDeviceBatch(NULL, in, NB, NULL, fp, NULL) == ERR);
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, NULL, NB, NULL, fp, NULL) == ERR);
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, NB, NULL, NULL, NULL) == ERR);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, NULL, NFRAMES, differs) == ERR);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES - 1u, differs) == ERR);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, NB, NULL, fp, NFRAMES + 1u, differs) == ERR);
    memcpy(bad, in, sizeof(in));
    bad[2].d_ptr = NULL; /* a null pointer with a size */
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, bad, NB, NULL, fp, NULL) == ERR);
    bad[2].d_ptr = host; /* host memory */
    bad[2].size = sizeof(host);
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, bad, NB, NULL, fp, NULL) == ERR);
    CHECK(QZSTD_frontCheckDeviceBatch(f, bad, NB, NULL, fp, NFRAMES, differs) == ERR);
    memcpy(bad, in, sizeof(in));
    bad[5].size = pool.size; /* a buffer that ends outside device memory */
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, bad, NB, NULL, fp, NULL) == ERR);
    for (c = 0; c < NFRAMES; c++) CHECK(differs[c] == 7 && fp[c] == want[c]);
    /* no buffers, or only empty ones: 0, nothing launched */
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, 0, NULL, NULL, first) == 0 && first[0] == 0);
    CHECK(QZSTD_frontFingerprintDeviceBatch(f, in, 1, NULL, NULL, first) == 0 && first[0] == 0 && first[1] == 0);
    CHECK(QZSTD_frontCheckDeviceBatch(f, in, 1, NULL, NULL, 0, NULL) == 0);
    CHECK(QZSTD_frontCheckDeviceBatch(f, NULL, 0, NULL, NULL, 0, NULL) == 0);
    QZSTD_frontFingerprintStats(f, st2);
    CHECK(qzstd_mock_fingerprint_launches() == launches && memcmp(st, st2, sizeof(st)) == 0);
    QZSTD_frontFingerprintStats(NULL, st2);
    CHECK(st2[0] == 0 && st2[3] == 0);
    QZSTD_frontFingerprintStats(f, NULL);
    CHECK(memcmp(copy, pool.base, pool.size) == 0);
    QZSTD_freeFront(f);
    free(copy);
    free(pool.base);
}

int main(void)
{
    definition();
    calls(1);
    calls(0); /* a front without the producer serves the calls, like the restore */
    puts("ok");
    return 0;
}
