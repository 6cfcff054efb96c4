/*
 * qzstd_elemdiff.h — element differences of integer columns (row ids, offsets, timestamps, sorted keys, sampled signals) and the sum that
 * undoes them: plain C, no GPU, no libzstd.  Exported by libqzstdfront.  The second of the two standard column filters: a differenced
 * frame's content is QZSTD_byteGroup(QZSTD_elemDiff(chunk), k) of include/qzstd_bytegroup.h, and a reader undoes it with QZSTD_byteUngroup,
 * then QZSTD_elemSum, after decoding the frame.
 *
 * For a chunk of L bytes and element size k in {1, 2, 4, 8}: n = L / k (rounded down); x[e] is the little-endian unsigned k-byte integer at
 * byte e * k of the chunk, whatever the chunk's address is.
 *   d[0] = x[0];  d[e] = x[e] - x[e-1] mod 2^(8k) for e >= 1
 *   z[e] = (d[e] << 1) ^ (0 - (d[e] >> (8k - 1))), in k bytes (zigzag: small differences of either sign become small numbers)
 * z[] is stored little-endian at the same places; the L - n * k tail bytes are copied unchanged.  The transform is per chunk, never across
 * chunks, and follows from L and k alone: neither k nor the fact that differences were taken is stored in a frame.  Addition mod 2^(8k) is
 * associative, so a sum taken in any parallel order gives the same bits.  Data without order GROWS under this transform.
 */
#ifndef QZSTD_ELEMDIFF_H
#define QZSTD_ELEMDIFF_H

#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

/* src (L bytes, elements of k bytes) -> dst = the zigzagged differences, and back (un-zigzag, then an inclusive prefix sum mod 2^(8k)).
 * dst == src is allowed; any other overlap is not.  Return L, or (size_t)-1 for a k outside {1, 2, 4, 8}. */
size_t QZSTD_elemDiff(void *dst, const void *src, size_t L, unsigned k);
size_t QZSTD_elemSum(void *dst, const void *src, size_t L, unsigned k);

#if defined(__cplusplus)
}
#endif
#endif /* QZSTD_ELEMDIFF_H */
