/*
 * mock_hip_device.c — TEST INFRASTRUCTURE ONLY.  The device-input entry points of include/qzstd_hip.h (pointer look-up, events,
 * the 2D device copy, the compaction) for the CPU stand-in of tests/mock/mock_hip.c, so that QZSTD_frontCompressDevice runs in the
 * CPU suite: "device" memory is plain host memory the test registers with qzstd_mock_device_range(); every other address is host
 * memory.  The compaction follows the kernel's contract (headers, packed entries, literals; a block whose entries do not cover it
 * exactly, and every block from the first one that does not fit the arena, contributes nothing; the same refusals) —
 * tools/qz_compact_ref.py states it and the CPU suite holds the two together.
 */
#include "qzstd_hip_device.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MOCK_RANGES 16
static struct { const unsigned char *p; size_t n; int dev; } gRanges[MOCK_RANGES];
static int gCompactLaunches, gEventWaits;

/* test hooks */
void qzstd_mock_device_range(int slot, const void *p, size_t n, int dev)
{
    if (slot < 0 || slot >= MOCK_RANGES) return;
    gRanges[slot].p = (const unsigned char *)p;
    gRanges[slot].n = n;
    gRanges[slot].dev = dev;
}
int qzstd_mock_compact_launches(void) { return gCompactLaunches; }
int qzstd_mock_event_waits(void) { return gEventWaits; }

int qzstd_hip_pointer_device(const void *p)
{
    int k;
    for (k = 0; k < MOCK_RANGES; k++)
        if (gRanges[k].p && (const unsigned char *)p >= gRanges[k].p && (const unsigned char *)p < gRanges[k].p + gRanges[k].n) return gRanges[k].dev;
    return -1;
}
void *qzstd_hip_event_create(int device) { (void)device; return malloc(1); }
void qzstd_hip_event_destroy(int device, void *e) { (void)device; free(e); }
int qzstd_hip_event_record(int device, void *e, void *s) { (void)device; (void)e; (void)s; return 0; }
int qzstd_hip_stream_wait_event(int device, void *s, void *e) { (void)device; (void)s; (void)e; __sync_fetch_and_add(&gEventWaits, 1); return 0; }
int qzstd_hip_memcpy2d_d2d(int device, void *s, void *dst, size_t dp, const void *src, size_t sp, size_t w, size_t h)
{
    size_t r;
    (void)device; (void)s;
    for (r = 0; r < h; r++) memcpy((char *)dst + r * dp, (const char *)src + r * sp, w);
    return 0;
}
size_t qzstd_hip_compact_workspace_bytes(uint32_t nBlocks) { return (size_t)nBlocks * 16u + 16u; }

int qzstd_hip_compact(int device, void *stream, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                      const void *d_seqs, const uint32_t *d_nseq, void *d_arena, size_t arenaBytes, void *d_work, size_t workBytes)
{
    qzstd_hip_compact_hdr_t *hdr = (qzstd_hip_compact_hdr_t *)d_arena;
    const size_t eo = QZSTD_HIP_COMPACT_ENTRIES_OFF(nBlocks);
    const uint32_t *seqs = (const uint32_t *)d_seqs;
    unsigned long long all = 0, nSeq = 0, nLit = 0;
    uint32_t b, i;
    (void)device; (void)stream;
    if (nBlocks == 0) return 0;
    if (!d_src || !d_blocks || !d_seqs || !d_nseq || !d_arena || !d_work || workBytes < qzstd_hip_compact_workspace_bytes(nBlocks) ||
        ((uintptr_t)d_work & 7u) || ((uintptr_t)d_arena & 15u) || arenaBytes < eo)
        return -1;
    __sync_fetch_and_add(&gCompactLaunches, 1);
    for (b = 0; b < nBlocks; b++) { /* count */
        const qzstd_hip_block_t *k = &d_blocks[b];
        const uint32_t n = d_nseq[b];
        unsigned long long lit = 0, cover = 0;
        int ok = n != QZSTD_HIP_NSEQ_ERROR && n >= 1u && n <= k->seqCap && !(k->mark & QZSTD_HIP_MARK_COMPACT);
        for (i = 0; ok && i < n; i++) {
            const uint32_t *s = seqs + (k->seqOff + i) * 4u;
            lit += s[1];
            cover += (unsigned long long)s[1] + s[2];
            if (s[0] >= (1u << 17) || s[1] > (1u << 17) || s[2] >= (1u << 17) || (i + 1u == n && (s[0] | s[2]) != 0u)) ok = 0;
        }
        ok = ok && cover == k->srcLen;
        hdr[b].count = ok ? n : QZSTD_HIP_NSEQ_ERROR;
        hdr[b].litBytes = ok ? (uint32_t)lit : 0u;
    }
    for (b = 0; b < nBlocks; b++) { /* scan + capacity */
        const unsigned long long c = hdr[b].count == QZSTD_HIP_NSEQ_ERROR ? 0 : hdr[b].count;
        all += 8u * c + hdr[b].litBytes;
        if (all > arenaBytes - eo) { hdr[b].count = QZSTD_HIP_NSEQ_ERROR; hdr[b].litBytes = 0; continue; }
        nSeq += c;
        nLit += hdr[b].litBytes;
    }
    {
        uint64_t *ent = (uint64_t *)((unsigned char *)d_arena + eo);
        unsigned char *lits = (unsigned char *)d_arena + eo + 8u * nSeq;
        for (b = 0; b < nBlocks; b++) { /* emit */
            const qzstd_hip_block_t *k = &d_blocks[b];
            const unsigned char *in = (const unsigned char *)d_src + k->srcOff;
            size_t pos = 0;
            if (hdr[b].count == QZSTD_HIP_NSEQ_ERROR) continue;
            for (i = 0; i < hdr[b].count; i++) {
                const uint32_t *s = seqs + (k->seqOff + i) * 4u;
                *ent++ = QZSTD_HIP_PACK(s[0], s[1], s[2], 0u);
                memcpy(lits, in + pos, s[1]);
                lits += s[1];
                pos += (size_t)s[1] + s[2];
            }
        }
    }
    return 0;
}
