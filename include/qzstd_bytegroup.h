/*
 * qzstd_bytegroup.h — the byte-grouped layout of typed data (bf16 / fp16 / fp32 weights, integer columns) and the block rule that goes with
 * it: plain C, no GPU, no libzstd.  Exported by libqzstdfront; the device calls of qzstd_frontend_device.h build frames of this layout
 * (QZSTD_frontSetByteGroup), and a reader undoes it with QZSTD_byteUngroup after decoding the frame.
 *
 * For a frame of L content bytes and element size k in {2, 4, 8}: n = L / k (rounded down); plane j holds byte j of elements 0 .. n-1 at
 * [j * n, (j + 1) * n); the L - n * k tail bytes follow, unchanged.  k = 1 is the identity.  The layout is per frame, never across frames,
 * and follows from L and k alone: the element size is not stored in the frame.
 */
#ifndef QZSTD_BYTEGROUP_H
#define QZSTD_BYTEGROUP_H

#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

/* planes shorter than this are not given blocks of their own (measured: profiles/device_group_ratio.json) */
#define QZSTD_BYTEGROUP_CUT_MIN 4096u
#define QZSTD_BYTEGROUP_BLOCK_MAX 131072u

/* src (L bytes, elements of k bytes) -> dst in the grouped layout, and back.  dst and src do not overlap.  Return L, or (size_t)-1 for a
 * k outside {1, 2, 4, 8}. */
size_t QZSTD_byteGroup(void *dst, const void *src, size_t L, unsigned k);
size_t QZSTD_byteUngroup(void *dst, const void *src, size_t L, unsigned k);
/* dst[i] = a[i] ^ b[i] for i < n; dst may be a or b.  The delta frames of qzstd_frontend_device.h (QZSTD_frontCompressDeviceBatchDelta) hold the
 * grouped layout of chunk XOR base chunk: a reader who decodes such a frame itself calls QZSTD_byteUngroup, then this with the base's bytes. */
void QZSTD_byteXor(void *dst, const void *a, const void *b, size_t n);

/* The block ends of a grouped frame of L bytes, ascending, the last one L; returns their count (ends may be NULL with cap 0 to size the
 * array; at most cap entries are written), 0 for L = 0, (size_t)-1 for a k outside {1, 2, 4, 8}.
 * With k > 1 and n >= QZSTD_BYTEGROUP_CUT_MIN the frame is cut at (j * n) & ~15 for j = 1 .. k-1 — a block per plane, so that every plane
 * gets entropy tables of its own; block starts stay multiples of 16, a few bytes of the neighbouring plane in a block are harmless — and
 * every piece is then cut every 128 KiB from its own start.  Otherwise the blocks are every 128 KiB from the frame's start. */
size_t QZSTD_byteGroupBlocks(size_t L, unsigned k, size_t *ends, size_t cap);

#if defined(__cplusplus)
}
#endif
#endif /* QZSTD_BYTEGROUP_H */
