/*
 * mock_hip_xxh64.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_xxh64 (include/qzstd_hip_device.h) for the CPU stand-in of tests/mock/mock_hip.c,
 * mock_hip_device.c and mock_hip_gather.c, so that the device calls run with content checksums on (QZSTD_frontSetChecksum) in the CPU suite.
 * XXH64 written from its published specification (xxHash, "XXH64 algorithm description": four accumulators over 32-byte stripes, their
 * merge, the 8-, 4- and 1-byte tail steps, the avalanche), seed 0; bytes are read one at a time, inside [srcOff, srcOff + len) only.
 * A source of its own: a mock built without it is a device layer that cannot hash, which the device calls must refuse with checksums on.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <string.h>

#define P1 0x9E3779B185EBCA87ull
#define P2 0xC2B2AE3D27D4EB4Full
#define P3 0x165667B19E3779F9ull
#define P4 0x85EBCA77C2B2AE63ull
#define P5 0x27D4EB2F165667C5ull

static int gHashLaunches;
static unsigned long long gHashRows;

/* test hooks */
int qzstd_mock_xxh64_launches(void) { return gHashLaunches; }
unsigned long long qzstd_mock_xxh64_rows(void) { return gHashRows; }

static uint64_t rotl(uint64_t v, unsigned r) { return (v << r) | (v >> (64u - r)); }
static uint64_t le(const unsigned char *p, unsigned n)
{
    uint64_t v = 0;
    unsigned i;
    for (i = 0; i < n; i++) v |= (uint64_t)p[i] << (8u * i);
    return v;
}
static uint64_t round64(uint64_t acc, uint64_t lane) { return rotl(acc + lane * P2, 31) * P1; }
static uint64_t merge(uint64_t h, uint64_t acc) { return (h ^ round64(0, acc)) * P1 + P4; }

uint64_t qzstd_mock_xxh64(const void *data, uint64_t len)
{
    const unsigned char *p = (const unsigned char *)data, *end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t a1 = P1 + P2, a2 = P2, a3 = 0, a4 = 0 - P1;
        for (; (uint64_t)(end - p) >= 32; p += 32) {
            a1 = round64(a1, le(p, 8));
            a2 = round64(a2, le(p + 8, 8));
            a3 = round64(a3, le(p + 16, 8));
            a4 = round64(a4, le(p + 24, 8));
        }
        h = rotl(a1, 1) + rotl(a2, 7) + rotl(a3, 12) + rotl(a4, 18);
        h = merge(merge(merge(merge(h, a1), a2), a3), a4);
    } else {
        h = P5;
    }
    h += len;
    for (; end - p >= 8; p += 8) h = rotl(h ^ round64(0, le(p, 8)), 27) * P1 + P4;
    if (end - p >= 4) { h = rotl(h ^ le(p, 4) * P1, 23) * P2 + P3; p += 4; }
    for (; p < end; p++) h = rotl(h ^ *p * P5, 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

int qzstd_hip_xxh64(int device, void *stream, const void *d_base, const qzstd_hip_hash_row_t *rows, uint32_t nRows,
                    qzstd_hip_hash_row_t *d_rows, uint64_t *d_out)
{
    uint32_t i;
    (void)device; (void)stream;
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_out || ((uintptr_t)d_base & 15u)) return -1;
    for (i = 0; i < nRows; i++)
        if ((rows[i].srcOff & 15u) || (rows[i].len && !d_base)) return -1;
    memcpy(d_rows, rows, (size_t)nRows * sizeof(*rows));
    __sync_fetch_and_add(&gHashLaunches, 1);
    __sync_fetch_and_add(&gHashRows, (unsigned long long)nRows);
    for (i = 0; i < nRows; i++) d_out[i] = qzstd_mock_xxh64((const unsigned char *)d_base + d_rows[i].srcOff, d_rows[i].len);
    return 0;
}
