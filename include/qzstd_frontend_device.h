/*
 * qzstd_frontend_device.h — the batch front-end's way in for DEVICE-RESIDENT input (a GPU tensor, any HIP allocation): the input is
 * never copied to the host; exported by libqzstdfront next to the calls of qzstd_frontend.h, which includes this header (its own
 * declarations stay what they were).
 */
#ifndef QZSTD_FRONTEND_DEVICE_H
#define QZSTD_FRONTEND_DEVICE_H

#include "qzstd_frontend.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Device-resident input.  Compresses srcSize bytes at the DEVICE address d_src as ceil(srcSize / chunkSize) independent frames,
 * exactly as QZSTD_frontCompress would frame them (dst at QZSTD_frontFrameStride() strides, sizes in frameSizes[]).  The device is
 * the one d_src belongs to.  stream = the hipStream_t that orders the producer of d_src (NULL = the default stream): nothing is
 * read before the work queued on it so far completes.  Returns the frame count or (size_t)-1.  Blocks until done; d_src must stay
 * valid and unchanged until then.
 *
 * The GPU match-finds the input in parts of whole chunks (at most 64 MiB) and packs each part's sequences and literal bytes into one
 * dense arena (qzstd_hip_compact) that comes back in one copy; the workers build the frames from it with
 * ZSTD_compressSequencesAndLiterals (explicit block delimiters, one 128 KiB block per delimiter) while the GPU works on the next
 * parts.  A frame with a block libzstd would store raw, or a failed block, is built from its raw bytes, copied back.  Errors that return before
 * anything is queued: dst too small, a front created with useProducer = 0, an address that is not device memory, a call while
 * another one runs on this front. */
size_t QZSTD_frontCompressDevice(QZSTD_Front *f, const void *d_src, size_t srcSize, void *stream,
                                 void *dst, size_t dstCapacity, size_t *frameSizes);
/* since creation: [0] frames from sequences + literals, [1] frames whose raw bytes were copied back (a block libzstd would store raw,
 * a matcher error, or a libzstd without ZSTD_compressSequencesAndLiterals), [2] bytes copied device->host, [3] bytes of input of the calls
 * that succeeded */
void QZSTD_frontDeviceStats(QZSTD_Front *f, unsigned long long stats[4]);

#if defined(__cplusplus)
}
#endif
#endif /* QZSTD_FRONTEND_DEVICE_H */
