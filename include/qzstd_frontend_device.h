/*
 * qzstd_frontend_device.h — the batch front-end's way in for DEVICE-RESIDENT input (a GPU tensor, any HIP allocation): the input is
 * never copied to the host — and the way back, frames restored into device buffers; exported by libqzstdfront next to the calls of qzstd_frontend.h, which includes this header (its own
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
 * The GPU match-finds the input in parts of whole chunks (at most 64 MiB; a part that is not 16-byte aligned throughout is copied to
 * library memory first) and packs each part's sequences and literal bytes into one
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

/* A batch of device buffers of any sizes and alignments, wherever the allocator put them (a checkpoint's tensors, column buffers), in ONE
 * call.  Buffer i becomes frames firstFrame[i] .. firstFrame[i + 1] - 1, cut every chunkSize bytes OF THAT BUFFER (an empty buffer yields
 * none): byte for byte the frames QZSTD_frontCompressDevice(f, bufs[i].d_ptr, bufs[i].size, ...) produces, whatever its neighbours are.
 * Frame c at dst + c * QZSTD_frontFrameStride(), its size in frameSizes[c]; firstFrame (nBufs + 1 entries) may be NULL.  The GPU's parts are
 * filled across buffer boundaries (at most 64 MiB of input each, whole frames): thousands of small buffers share one descriptor upload,
 * one gather launch (qzstd_hip_gather: the part's frames copied to 16-aligned places of library memory), one match-finder launch, one
 * compaction, one arena copy and one job of the workers.  `stream`, blocking and the validity of the buffers: as QZSTD_frontCompressDevice.
 * Returns the frame count (0 for no buffers or empty ones: no GPU is touched) or (size_t)-1.  Errors that return before anything is
 * queued: dst below frames x stride, a front created with useProducer = 0, bufs NULL with nBufs > 0, a NULL buffer of a size above 0, a
 * buffer whose first or last byte is not device memory, buffers of different devices, a call while another one runs on this front, a
 * device layer without qzstd_hip_gather.  QZSTD_frontDeviceStats counts a batch as the single calls: [3] grows by the sum of the sizes. */
typedef struct {
    const void *d_ptr; /* device address, any alignment */
    size_t size;       /* bytes, may be 0 */
} QZSTD_DeviceBuf;
/* frames the batch yields: the sum over i of ceil(size_i / chunkSize) — what dst (x QZSTD_frontFrameStride()) and frameSizes must hold;
 * (size_t)-1 for f NULL or bufs NULL with nBufs > 0 */
size_t QZSTD_frontDeviceBatchFrames(const QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs);
size_t QZSTD_frontCompressDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream,
                                      void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame);

/* Content checksums (RFC 8878: Content_Checksum_Flag, the low 32 bits of XXH64 of the frame's content behind its last block): off by
 * default.  On: every frame of every call on this front carries one, and all calls still agree byte for byte — QZSTD_frontCompress runs its
 * contexts with ZSTD_c_checksumFlag = 1; the device calls hash each part's frames ON THE GPU (qzstd_hip_xxh64, one launch per part, 8 bytes
 * per frame device->host), set the header's flag and append the four bytes themselves, since the input never reaches the host; a frame
 * built from its raw bytes (QZSTD_frontDeviceStats [1]) is hashed by libzstd like a host frame.  A decoder sees an ordinary frame and
 * verifies it.  The GPU hashes a frame as one serial chain: frames far longer than 128 KiB in a part of few frames take it
 * correspondingly long (64 MiB: 2 M steps).  With the setting on and a device layer without qzstd_hip_xxh64 the device calls return
 * (size_t)-1 before anything is queued; QZSTD_frontCompress is not affected.
 * Set: 0, or -1 for f NULL or while a call runs on the front.  Get: 0 / 1 (0 for f NULL). */
int QZSTD_frontSetChecksum(QZSTD_Front *f, int on);
int QZSTD_frontGetChecksum(const QZSTD_Front *f);
/* since creation, frames whose checksum [0] the GPU computed, [1] libzstd computed (host calls, and device frames built from raw bytes) */
void QZSTD_frontChecksumStats(QZSTD_Front *f, unsigned long long stats[2]);

/* Byte grouping for typed data (include/qzstd_bytegroup.h): elemSize 2, 4 or 8 makes every device call on this front build its frames from
 * the BYTE-GROUPED content of each chunk — byte 0 of every element, then byte 1 of every element, ... (per frame: n = frame length /
 * elemSize elements, the remainder behind the planes, unchanged) — with a block per plane from 4096 elements on
 * (QZSTD_byteGroupBlocks): the sign/exponent bytes of bf16 / fp16 / fp32 weights are skewed and the mantissa bytes noise, and a block of
 * their own gives each its own entropy tables.  1 (the default): off, every frame byte for byte what it was.  The grouping happens on the
 * GPU while a part is staged (qzstd_hip_group): no extra pass, no host copy.  A frame is an ordinary zstd frame OF THE GROUPED CONTENT: the
 * element size is not stored in it — the caller keeps it — and the layout follows from the frame's content size and elemSize alone; a
 * reader either hands the frames to QZSTD_frontRestoreDeviceBatchTyped with the same element sizes (below: decoded by the front's workers,
 * ungrouped on the GPU), or decodes a frame itself and calls QZSTD_byteUngroup on the host.  Checksums (QZSTD_frontSetChecksum) cover the grouped content, which is what a decoder
 * verifies.  Frame counts, strides and QZSTD_frontDeviceBatchFrames are unchanged.
 * A grouped frame whose content libzstd needs (a block it stores raw — a mantissa plane — is the rule here) gets it rebuilt on the host
 * from the frame's own sequences and literals, already in the arena: no second device->host copy.  Only a frame with a block the matcher
 * failed has the caller's bytes copied back and grouped on the host; that frame is built by ZSTD_compress2 and is any valid frame of the
 * grouped content.  QZSTD_frontDeviceStats [1] counts rebuilt frames too (frames that were not built from sequences + literals).
 * With a setting above 1 QZSTD_frontCompress returns (size_t)-1 (the host path cannot cut blocks per plane, and one front does not
 * produce two layouts), and with a device layer without qzstd_hip_group the device calls return (size_t)-1 before anything is queued.
 * Set: 0, or -1 for f NULL, an elemSize other than 1, 2, 4, 8, or while a call runs on the front.  Get: the setting (1 for f NULL). */
int QZSTD_frontSetByteGroup(QZSTD_Front *f, unsigned elemSize);
unsigned QZSTD_frontGetByteGroup(const QZSTD_Front *f);
/* QZSTD_frontCompressDeviceBatch with an element size per buffer (a checkpoint mixes bf16 weights and fp32 norms): elemSizes[i] is 1, 2, 4
 * or 8, or 0 for the front's setting; NULL means all 0.  Any other value: (size_t)-1 before anything is queued. */
size_t QZSTD_frontCompressDeviceBatchTyped(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const unsigned char *elemSizes, size_t nBufs,
                                           void *stream, void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame);
/* since creation, byte-grouped frames (element size above 1) built from [0] sequences + literals, [1] content rebuilt from the arena,
 * [2] content copied back from the device and grouped on the host */
void QZSTD_frontByteGroupStats(QZSTD_Front *f, unsigned long long stats[3]);

/* The way back: frames in HOST memory restored into device buffers, in ONE call.  Frame c lies at frames + c * frameStride, its size in
 * frameSizes[c] — what the compress calls leave with frameStride = QZSTD_frontFrameStride(); with frameStride == 0 it lies at the sum of the
 * sizes before it, which is what QZSTD_frontCompact leaves.  Buffer i receives frames firstFrame[i] .. firstFrame[i + 1] - 1 under the compress
 * calls' own rule (ceil(size_i / chunkSize) frames, none for an empty buffer); nFrames must equal QZSTD_frontDeviceBatchFrames of the same
 * sizes.  elemSizes: as QZSTD_frontCompressDeviceBatchTyped's (1, 2, 4, 8, or 0 for the front's setting; NULL: all 0; anything else is refused) —
 * the values the frames were written with, which the caller keeps.
 *
 * A frame is ANY valid zstd frame whose content is the (byte-grouped) chunk: one of this library's, or one built by ZSTD_compress2 over
 * QZSTD_byteGroup's output.  Every frame is decoded with capacity = the chunk's expected length and must yield exactly that; the header's
 * content-size field is not relied on.  libzstd verifies a content checksum where a frame carries one, whatever QZSTD_frontSetChecksum says.
 *
 * The call is cut into parts of whole frames (at most 64 MiB of content, $QZSTD_FRONT_DEVICE_PART as on the compress side).  The front's
 * workers, each with a ZSTD_DCtx of its own, decode a part into one of two pinned buffers kept with the front, every frame at a 16-aligned
 * offset; one host->device copy and one qzstd_hip_ungroup launch (the frames scattered to their buffers at any alignment, the grouped layout
 * undone on the way, exactly the buffers' bytes written) follow on a stream of the library's, while the workers decode the next part into the
 * other buffer.  `stream`: the hipStream_t that orders the last user of the buffers (NULL = the default stream): nothing is written before
 * the work queued on it so far completes.  Blocks until done.
 *
 * Returns nFrames (0 for no buffers or empty ones: no GPU is touched) or (size_t)-1.  Before anything is queued: f NULL, bufs NULL with
 * nBufs > 0, a NULL buffer of a size above 0, a bad elemSizes entry, a wrong nFrames, frames or frameSizes NULL with nFrames > 0, a buffer
 * whose first or last byte is not device memory, buffers of different devices, a call while another one runs on this front, a device layer
 * without qzstd_hip_ungroup.  After work has started: a frame that does not decode, decodes to another length than its chunk's or fails its
 * checksum — the buffers' contents are then unspecified, but nothing outside them was written, and nothing of the library's is still running
 * on the GPU when the call returns.
 * The restore needs nothing of the producer: a front created with useProducer = 0 (no match-finder service is started) is accepted.
 * The compress calls, their frames and their stats are not affected. */
typedef struct {
    void *d_ptr; /* device address, any alignment */
    size_t size; /* bytes, may be 0 */
} QZSTD_DeviceOutBuf;
size_t QZSTD_frontRestoreDeviceBatchTyped(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                          const QZSTD_DeviceOutBuf *bufs, const unsigned char *elemSizes, size_t nBufs, void *stream);
/* one buffer, the front's element size (QZSTD_frontSetByteGroup) */
size_t QZSTD_frontRestoreDevice(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                void *d_dst, size_t dstSize, void *stream);
/* since creation, of the parts that were queued: [0] frames decoded, [1] bytes of content, [2] bytes copied host->device (the frames at
 * 16-aligned offsets), [3] qzstd_hip_ungroup launches (one per part) */
void QZSTD_frontRestoreStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Delta frames: the Typed calls with a BASE per buffer — the previous checkpoint's tensor, still on the device.  bases[i] is {NULL, 0} for a
 * buffer without one, else a device address of exactly bufs[i].size bytes on the buffers' device, at any alignment; bases == NULL makes each
 * call exactly its ...Typed counterpart.  A frame of a buffer with a base is an ordinary zstd frame whose content is the byte-grouped layout,
 * for that buffer's element size (1 included), of chunk XOR base chunk: where the step between two checkpoints is small, that is mostly zero
 * bytes in exactly the mantissa planes grouping cannot help.  NEITHER THE BASE NOR THE FACT THAT THERE WAS ONE IS STORED IN THE FRAME: the
 * caller keeps both with the frames, as it keeps the element size.  A reader hands the frames to QZSTD_frontRestoreDeviceBatchDelta with the
 * same element sizes and bases, or decodes a frame itself: decode, QZSTD_byteUngroup, QZSTD_byteXor with the base's bytes.
 *
 * Compress: the XOR happens while a part is staged (qzstd_hip_group_xor: one launch for all rows of a part that holds a frame with a base —
 * such a part is always staged, never read in place): no temporary of the buffers' size, no pass of its own.  Framing, strides,
 * QZSTD_frontDeviceBatchFrames, the per-plane block rule and checksums are the Typed call's; a checksum covers the content a decoder
 * verifies, the delta.  Frames of buffers without a base are byte for byte what the Typed call yields, whatever their neighbours are, and a
 * call in which no buffer has a base is the Typed call, launch for launch.  A delta frame that needs its content on the host gets it rebuilt
 * from its own sequences and literals, like a grouped one; only a frame with a block the matcher failed has the caller's bytes AND the base's
 * copied back (both count in QZSTD_frontDeviceStats [2]), XORed and grouped on the host, and is built by ZSTD_compress2.  The bases are only
 * read; `stream` must order their last writer too.
 *
 * Restore: decoding, the pinned buffers and the host->device copy are the Typed call's; a part with a base among its rows is scattered by
 * one qzstd_hip_ungroup_xor launch, which XORs the base back in on the way out.  bases[i].d_ptr == bufs[i].d_ptr restores IN PLACE over the
 * previous checkpoint (every byte is read by its only writer, before it is written); a base that overlaps its buffer in any other way is
 * the caller's error.  `stream` must order the last writer of the bases too.
 *
 * Both return (size_t)-1 before anything is queued for everything the Typed calls refuse, a base of another size than its buffer (a NULL one
 * of a size above 0 included), a base whose first or last byte is not device memory or lies on another device than the buffers, and — when a
 * base is given — a device layer without qzstd_hip_group_xor / qzstd_hip_ungroup_xor (the Typed and older calls are not affected). */
size_t QZSTD_frontCompressDeviceBatchDelta(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes,
                                           size_t nBufs, void *stream, void *dst, size_t dstCapacity, size_t *frameSizes, size_t *firstFrame);
size_t QZSTD_frontRestoreDeviceBatchDelta(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                          const QZSTD_DeviceOutBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes, size_t nBufs,
                                          void *stream);
/* since creation: frames with a base built from [0] sequences + literals, [1] content rebuilt from the arena, [2] both buffers copied back,
 * XORed (and grouped) on the host; [3] frames restored onto a base */
void QZSTD_frontDeltaStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Element differences for integer columns (include/qzstd_elemdiff.h): QZSTD_ELEM_DIFF OR-ed into an elemSizes[i] entry — 0x81, 0x82, 0x84 or
 * 0x88; 0x80 alone ("the front's setting, with differences") stays refused, and QZSTD_frontSetByteGroup takes no flag.  Off unless the caller
 * asks for it, per buffer: row ids, offsets, timestamps, sorted keys and sampled signals shrink, data without order GROWS.  A frame of a flagged
 * buffer is an ordinary zstd frame whose content is QZSTD_byteGroup(QZSTD_elemDiff(chunk, k), k), the block-per-plane rule unchanged; the
 * differences are per chunk, so every frame decodes on its own.  NEITHER k NOR THE FACT THAT DIFFERENCES WERE TAKEN IS STORED IN THE FRAME: the
 * caller keeps both, as it keeps element sizes.  A reader hands the frames to a restore call with the same entries, or decodes a frame itself:
 * decode, QZSTD_byteUngroup, QZSTD_elemSum.
 *
 * QZSTD_frontCompressDeviceBatchTyped, and QZSTD_frontCompressDeviceBatchDelta for a buffer without a base: a flagged buffer's frames are always
 * staged, never read in place — by one qzstd_hip_group_ediff launch over the flagged frames of a part, beside the launch the part's other
 * frames get as before.  Checksums cover the transformed content; the plane probe sees the staged blocks as before; a frame whose content is
 * rebuilt from the arena needs nothing new; a frame with a block the matcher failed has the caller's bytes copied back, QZSTD_elemDiff and
 * QZSTD_byteGroup applied on the host, and is built by ZSTD_compress2.  Frames of unflagged buffers are byte for byte what they are without
 * any flag in the call, whatever their neighbours are, and a call without any flag is launch for launch what it was.
 * QZSTD_frontRestoreDeviceBatchTyped / ...Delta for a buffer without a base: after a part's ungroup launch ONE qzstd_hip_esum launch over the
 * flagged frames' destinations follows on the same stream and sums them in place.
 *
 * (size_t)-1 before anything is queued: a flagged buffer that also has a base, in either direction; a flagged buffer in
 * QZSTD_frontVerifyDeviceBatch; a flagged buffer that a non-empty slice of QZSTD_frontRestoreDeviceSlices touches (a window needs the sum from
 * the frame's start); a flagged buffer with a device layer without qzstd_hip_group_ediff (compress) or qzstd_hip_esum (restore).
 * QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch work on the tensors' own bytes and are THE end-to-end check for flagged buffers. */
#define QZSTD_ELEM_DIFF 0x80u
/* since creation: [0] frames whose differences were taken on the GPU (every flagged frame of a staged part), [1] of those, frames whose
 * content was taken again on the host (a failed block), [2] frames summed by a restore, [3] qzstd_hip_esum launches */
void QZSTD_frontElemDiffStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Delta skip: chunks EQUAL to their base chunk — a frozen backbone, frozen embeddings, buffers, an evaluation-only interval — found on the GPU
 * and skipped.  Off by default; with the setting off every call is launch for launch and byte for byte what it was.
 *
 * Compress (QZSTD_frontCompressDeviceBatchDelta with a base given; a call without any base and every other call are not affected): after
 * the host-side checks and the wait for `stream`, ONE qzstd_hip_diff launch compares every frame of every buffer that has a base with its
 * base chunk (2 bytes read per content byte), the flags come back in one copy (4 bytes per compared frame, not counted in
 * QZSTD_frontDeviceStats [2]) and a bounded wait follows.  A frame found equal is left out of the parts — it is not staged, matched,
 * compacted, copied back or entropy-coded, and a part of 64 MiB holds 64 MiB of changed input; when every frame of the call is equal no part
 * is queued at all.  Its frame is written by the library itself, THE CANONICAL ZERO FRAME of the chunk's length L: magic, a frame header
 * descriptor with Single_Segment and the smallest Frame_Content_Size field that holds L, RLE_Blocks of the byte 0 cut every 128 KiB from the
 * frame's start (the per-plane block rule does not apply: the content is zeros whatever the element size), Last_Block on the final one, and
 * with QZSTD_frontSetChecksum on the Content_Checksum_Flag and the low 32 bits of XXH64 (seed 0) of L zero bytes, computed on the host:
 * 10 - 13 bytes and 4 per further 128 KiB.  It is an ordinary zstd frame whose content is L zero bytes, the delta of an unchanged chunk:
 * the caller keeps nothing new, and any decoder reads it.  Frames of changed chunks are byte for byte the frames the setting-off call yields;
 * frames of buffers without a base are never compared and never skipped, zeros or not; frameSizes, firstFrame, strides and the return value
 * are unchanged.  QZSTD_frontDeviceStats [3] counts skipped input too; its [0] and [1], QZSTD_frontDeltaStats and QZSTD_frontByteGroupStats
 * do not count skipped frames.  With the setting on, a base given and a device layer without qzstd_hip_diff the call returns (size_t)-1
 * before anything is queued.
 *
 * Restore (QZSTD_frontRestoreDeviceBatchDelta): a frame of a buffer with a base whose bytes equal the canonical zero frame of its chunk's
 * length (with or without the checksum field) is recognised: it is not decoded and takes no room in the pinned buffer, the copy or the
 * stage.  In place (bases[i].d_ptr == bufs[i].d_ptr) nothing at all happens for it; otherwise consecutive recognised frames of one buffer
 * become ONE device->device copy from base to destination (a wholly frozen tensor: a single copy).  The parts are packed from the remaining
 * frames; when none remains no part is queued.  QZSTD_frontRestoreStats counts only what was decoded and copied, QZSTD_frontDeltaStats [3]
 * only frames scattered onto a base.  With the setting off such a frame is decoded like any other — it is a valid frame.
 * QZSTD_frontRestoreDeviceSlices and QZSTD_frontRestoreDeviceBatchTyped do not look for zero frames: they decode one as the ordinary frame it is.
 *
 * Set: 0, or -1 for f NULL or while a call runs on the front.  Get: 0 / 1 (0 for f NULL). */
int QZSTD_frontSetDeltaSkip(QZSTD_Front *f, int on);
int QZSTD_frontGetDeltaSkip(const QZSTD_Front *f);
/* since creation: [0] frames compared with their base chunk, [1] of them found equal and written as zero frames (nothing staged, matched or
 * entropy-coded), [2] bytes compared, [3] zero frames recognised by a restore (not decoded, nothing copied host->device) */
void QZSTD_frontDeltaSkipStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Plane probe, OFF by default: the noise planes of byte-grouped and delta frames are found on the GPU before a worker touches the frame, and
 * the library writes them as Raw_Blocks itself.  With the setting off every call is launch for launch and byte for byte what it was.
 *
 * With it on, a part that holds a frame with an element size above 1 or with a base gets ONE more launch behind its staging
 * (qzstd_hip_plane_cost: a byte histogram per block of the part, reduced on the device to one 32-bit word, the block's order-0 cost in
 * bytes — include/qzstd_planecost.h), and the words come back with the part's compaction headers: 4 bytes per block, no wait of their own.
 * A block is RAW-PREDICTED when QZSTD_planeIsRaw(cost, length, length - litBytes) holds: neither entropy coding its bytes nor its matches
 * could save libzstd's own minimum gain.  A frame with at least one such block (and no failed block, and no plane of one value) is ASSEMBLED
 * BY THE LIBRARY: magic and a frame header with Single_Segment and the smallest Frame_Content_Size field that holds the frame's length; per
 * raw-predicted block a 3-byte Raw_Block header and the block's content (its literals in the arena when it has no sequences, else that block
 * alone rebuilt from its entries); the remaining blocks, in order, from ONE ZSTD_compressSequencesAndLiterals call over their content alone,
 * copied to their places with Last_Block set on the frame's final block only; with checksums on, the header's flag and the GPU's hash.
 * When that call fails or yields a block libzstd would store raw, the frame takes the path it takes with the setting off.  A frame without
 * a raw-predicted block is byte for byte the frame of the setting off.  An assembled frame is an ordinary zstd frame of the same content:
 * the restore, slices and verify calls and any zstd decoder read it as before; it may be larger than the setting-off frame by at most
 * (length >> 6) + 2 bytes per raw-predicted block.  Parts without a grouped or based frame are untouched whatever the setting.
 *
 * With the setting on, a call with such a frame and a device layer without qzstd_hip_plane_cost returns (size_t)-1 before anything is queued.
 * QZSTD_frontDeviceStats counts an assembled frame in [0] (built from sequences and literals, nothing copied back) and the probe's words in [2];
 * QZSTD_frontByteGroupStats [0] and QZSTD_frontDeltaStats [0] count it as they count a frame built from the arena.
 *
 * Set: 0, or -1 for f NULL or while a call runs on the front.  Get: 0 / 1 (0 for f NULL). */
int QZSTD_frontSetPlaneProbe(QZSTD_Front *f, int on);
int QZSTD_frontGetPlaneProbe(const QZSTD_Front *f);
/* since creation: [0] blocks probed, [1] blocks written raw by the library, [2] frames assembled by the library, [3] frames with a
 * raw-predicted block that fell back to the setting-off path */
void QZSTD_frontPlaneProbeStats(QZSTD_Front *f, unsigned long long stats[4]);
/* QZSTD_planeCost / QZSTD_planeIsRaw of include/qzstd_planecost.h as exported functions (bindings that cannot include the header) */
unsigned QZSTD_planeCostOf(const unsigned hist[256], unsigned len);
int QZSTD_planeIsRawOf(unsigned cost, unsigned len, unsigned matchedBytes);

/* Plane code, OFF by default: blocks whose matches are not worth their sequences — the sign/exponent plane of float weights — are written as
 * Huffman-only Compressed blocks whose streams the GPU codes (include/qzstd_hufblock.h).  With the setting off every call is launch for launch
 * and byte for byte what it was.
 *
 * With it on, the front behaves as with the plane probe on (whatever that setting says), and a part that would be probed gets
 * qzstd_hip_huf_code INSTEAD of qzstd_hip_plane_cost: the same cost word per block, a size word and a dense offset per block (they travel
 * with the compaction headers and the costs: no wait of their own), and for the blocks of 1 KiB and more that a Huffman code shrinks, 128
 * bytes of code lengths, the jump table and the four streams, packed densely: one more copy behind the header wait.  A block is TAKEN when
 * QZSTD_hufTakes holds over its size word, the bytes of its QZSTD_hufBlockBody, its length and its compaction header.  A frame whose every
 * block is raw-predicted or taken is assembled WITHOUT ANY libzstd CALL: the header of an assembled frame, per raw-predicted block what the
 * probe writes, per taken block a 3-byte Compressed_Block header and QZSTD_hufBlockBody — literals section header, tree description (written
 * on the host from the code lengths), jump table and streams as the GPU left them, and one 0x00: no sequences.  All or nothing per frame: a
 * frame with any other block takes exactly the path it takes with the probe on.  Checksums are those of assembled frames;
 * the zero frames of a delta skip and frames with a failed block are untouched.  The frames are ordinary zstd frames: the restore, slices and
 * verify calls and any zstd decoder read them as before.
 *
 * Not done: a taken block's literals and entries still come back in the arena, so device-to-host bytes per input byte go up,
 * not down; the matcher is not skipped for taken blocks; no sequences are coded and nothing is decoded on the GPU; blocks under 1 KiB are
 * never taken.
 *
 * With the setting on, a call with a grouped or based frame and a device layer without qzstd_hip_huf_code returns (size_t)-1 before anything
 * is queued.  QZSTD_frontDeviceStats [2] counts the words and the dense area; QZSTD_frontPlaneProbeStats counts as with the probe on (a frame
 * assembled here in [2], its raw blocks in [1]).
 *
 * Set: 0, or -1 for f NULL or while a call runs on the front.  Get: 0 / 1 (0 for f NULL). */
int QZSTD_frontSetPlaneCode(QZSTD_Front *f, int on);
int QZSTD_frontGetPlaneCode(const QZSTD_Front *f);
/* since creation: [0] rows (blocks) the kernel coded, [1] blocks taken, [2] frames assembled without a libzstd call (all their blocks
 * raw-predicted or taken), [3] frames with a taken block that fell back to the probe's path */
void QZSTD_frontPlaneCodeStats(QZSTD_Front *f, unsigned long long stats[4]);
/* QZSTD_hufBlockBody (over the 128 bytes of code lengths as qzstd_hip_huf_code leaves them) and QZSTD_hufTakes of include/qzstd_hufblock.h as
 * exported functions (bindings that cannot include the header) */
size_t QZSTD_hufBlockBodyOf(const unsigned char lengths[128], unsigned len, const unsigned char *streams, size_t streamBytes, unsigned char *dst,
                            size_t cap);
int QZSTD_hufTakesOf(unsigned streamBytes, unsigned bodyBytes, unsigned len, unsigned litBytes, unsigned count);

/* Slices: byte ranges of the buffers AS THEY WERE WRITTEN restored into device memory — a checkpoint written by one rank layout and loaded
 * by another (a row shard: one contiguous slice per tensor; a column shard of an [R, C] matrix: R slices of one buffer) — without a
 * temporary of the buffers' size and without decoding the frames no slice touches.  frames / frameStride / frameSizes / nFrames are the WHOLE
 * frame list the compress call left for bufSizes (nFrames must equal the sum of ceil(bufSizes[i] / chunkSize)); elemSizes as in the Typed
 * call; the caller keeps the written sizes, the element sizes and which base each buffer was written against.  Slices are in ascending order
 * and disjoint in the source: (buf, offset) must not decrease, and within one buffer offset[i] >= offset[i-1] + size[i-1].  d_base: NULL, or
 * the SAME slice of the base the buffer was written against (`size` bytes), which may be d_dst itself: in place.
 *
 * Only frames that intersect a non-empty slice are decoded; the bytes of every other frame are never read (with frameStride == 0 the sizes
 * of the other frames still are, to place the frames).  The needed frames are cut into parts of whole frames (at most
 * $QZSTD_FRONT_DEVICE_PART bytes of content); the two restore slots, the workers' decode into the pinned buffer, the one host->device copy
 * per part, the event pair with `stream` and the closing waits are the Typed call's; the launch is ONE qzstd_hip_ungroup_window per part,
 * a row per piece (slice x frame): windows of the frames' content, at any byte, also inside an element of a grouped frame.
 * QZSTD_frontRestoreStats counts the parts as before (frames decoded, their content bytes, host->device bytes, launches), and
 * QZSTD_frontDeltaStats [3] grows by the frames restored onto a base.
 *
 * Returns the number of frames decoded (0 for no slices or only empty ones: no GPU is touched) or (size_t)-1.  Before anything is queued:
 * everything the Typed call refuses that applies here, a wrong nFrames, bufSizes or slices NULL with a count above 0, a slice with
 * buf >= nBufs or that ends past its buffer, slices out of order or overlapping, a NULL d_dst with size > 0, a destination or base whose first
 * or last byte is not device memory or that lies on another device than the rest (destinations — or bases — of consecutive slices that follow
 * each other in memory without a gap, a column shard's rows in one contiguous tensor, are looked up as ONE range, at its first and its last
 * byte: what the Typed call does for a buffer), a call while another one runs on this front, a device layer without qzstd_hip_ungroup_window.  After work has started: a needed frame that does not decode, decodes to another length or fails its
 * checksum — the rule is the Typed call's: the destinations' contents are unspecified, nothing outside them was written, and nothing of the
 * library's is still running on the GPU when the call returns.  A front created with useProducer = 0 is accepted; the other calls do not change. */
typedef struct {
    size_t buf;          /* index into bufSizes: the buffer, as it was WRITTEN, that the slice is cut from */
    size_t offset, size; /* bytes [offset, offset + size) of that buffer; any values inside it; size may be 0 */
    void *d_dst;         /* device address that receives them, any alignment */
    const void *d_base;  /* NULL, or the device address of `size` bytes XORed in: the SAME slice of the base the
                            buffer was written against; may equal d_dst */
} QZSTD_DeviceSlice;
size_t QZSTD_frontRestoreDeviceSlices(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                      const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs,
                                      const QZSTD_DeviceSlice *slices, size_t nSlices, void *stream);
/* since creation: [0] non-empty slices restored, [1] bytes written to destinations, [2] frames decoded for them, [3] rows launched */
void QZSTD_frontSliceStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Source slices: QZSTD_frontCompressDeviceBatchDelta for buffers that are NOT contiguous in device memory — a column view W[:, a:b] of a fused
 * matrix, a pitched allocation, a parameter kept in another order than the checkpoint stores, scattered cache pages, a tensor loaded as slices
 * by QZSTD_frontRestoreDeviceSlices and saved again — without the `.contiguous()` copy, a temporary of the buffers' size.  Logical buffer i has
 * bufSizes[i] bytes; the non-empty slices of a buffer, in order, tile [0, bufSizes[i]) exactly, each with the device address of its bytes.
 * A buffer has a base when its slices carry d_base (the same slice of the base, which may be d_src itself); all of them do, or none.
 *
 * Everything about the result is QZSTD_frontCompressDeviceBatchDelta's for the same bytes held contiguously: frames are cut every chunkSize
 * bytes of the LOGICAL buffer, the frame count, firstFrame, strides and QZSTD_frontDeviceBatchFrames of the sizes are the same, and EVERY
 * FRAME IS BYTE FOR BYTE the frame that call returns with the same elemSizes, bases and front settings (byte group, checksum, plane probe,
 * delta skip); `stream` (it orders the last writer of every slice and base) and blocking are as there.  The frame format knows nothing of
 * where a chunk's bytes came from, so restore, slices, verify and fingerprints read these frames as before and the caller keeps nothing new;
 * the TENSORS the frames are checked against may stay slices too: QZSTD_frontVerifyDeviceSlices, ...FingerprintDeviceSlices, ...CheckDeviceSlices.
 *
 * A frame that lies inside one slice is handled as a frame of a contiguous buffer is, so a call in which every frame does — one slice per
 * buffer in particular — queues the launches of the Delta call.  A part that holds a frame made of several slices is always staged, by ONE
 * qzstd_hip_group_pieces launch over all its rows: the frame is assembled in the stage from its pieces, XORed with their bases and grouped
 * in the same pass.  Where such a frame's bytes are needed on the host (a block the matcher failed) they come back with one copy per piece,
 * the base's likewise; delta skip compares such a frame piece by piece in the same single launch.  QZSTD_frontDeviceStats,
 * ...ByteGroupStats, ...DeltaStats, ...DeltaSkipStats, ...ChecksumStats and ...PlaneProbeStats count this call as they count the Delta call.
 *
 * (size_t)-1 before anything is queued: everything the Delta call refuses that applies here; bufSizes or slices NULL with a count above 0; a
 * slice with buf >= nBufs; slices out of order; a gap, an overlap, or an end past its buffer; a buffer with based and unbased slices; a NULL
 * d_src with size > 0; a source or base whose first or last byte is not device memory, or that lies on another device than the rest
 * (consecutive slices that follow each other in memory are looked up as ONE range, as in QZSTD_frontRestoreDeviceSlices); an element size
 * with QZSTD_ELEM_DIFF — the differencing gather does not assemble pieces: out of scope here, make such a buffer contiguous and use the
 * Typed call; and, for a call with a frame made of several slices, a device layer without qzstd_hip_group_pieces (such a layer serves a
 * call without such a frame, and every other call, as before).
 * Look-ups: where the device layer tells the extent of the allocation that holds an address (qzstd_hip_pointer_extent) and the extent's own
 * last byte looks up as memory of the same device, a range that lies inside the allocation looked up last is accepted without a look-up of
 * its own — a view's 10^5 rows cost one — so "first or last byte" becomes "inside an allocation of the device" for such ranges.  That
 * is as good as the runtime's answer: an address range that is reserved and only partly mapped fails the last-byte test and is looked up
 * range by range, but a reservation with an unmapped hole in its MIDDLE would pass, and has not been tested. */
typedef struct {
    size_t buf;          /* index into bufSizes: the logical buffer this slice belongs to */
    size_t offset, size; /* bytes [offset, offset + size) of that buffer; size may be 0 */
    const void *d_src;   /* device address of those bytes, any alignment */
    const void *d_base;  /* NULL, or the device address of the same slice of the buffer's base; may equal d_src */
} QZSTD_DeviceSrcSlice;
size_t QZSTD_frontCompressDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs,
                                       const QZSTD_DeviceSrcSlice *slices, size_t nSlices, void *stream, void *dst, size_t dstCapacity,
                                       size_t *frameSizes, size_t *firstFrame);
/* since creation, of the calls that succeeded: [0] non-empty slices, [1] their bytes, [2] frames assembled from more than one piece,
 * [3] qzstd_hip_group_pieces launches (one per part that holds such a frame) */
void QZSTD_frontSrcSliceStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Verify: do the frames just written reproduce the tensors that are on the device NOW — asked before the previous checkpoint is dropped?  A
 * delta frame is only as good as the base it is applied to and the element size it is ungrouped with, and neither is in the frame; a content
 * checksum covers the grouped delta, not the tensor.  A mistake in the caller's bookkeeping (another base, another element size, frames in
 * another order) and a tensor that changed while the compress call ran both pass libzstd's check and fail this one.
 *
 * The arguments are QZSTD_frontRestoreDeviceBatchDelta's, with bufs CONST: the live tensors, compared and never written.  bases == NULL (or no
 * base among them) makes the call the Typed counterpart.  Per part the restore's slots and the workers' decode are used as they are; then ONE
 * host->device copy, ONE qzstd_hip_ungroup_cmp launch (the frames ungrouped, XORed with their base chunks and compared with the live chunks in
 * registers: nothing is stored but one word per 16 KiB) and one device->host copy of those words.  No temporary of the buffers' size exists,
 * and nothing on the device but the library's own stage and result buffers is written.  bases[i].d_ptr == bufs[i].d_ptr is accepted and
 * compares the frames' content with zero.  With QZSTD_frontSetDeltaSkip on, a frame of a based buffer that is the canonical zero frame of its
 * chunk's length is not decoded and takes no room in the pinned buffer or the copy: its live chunk is compared with its base chunk directly,
 * by the same launch (a call whose frames are all such frames still launches); with the setting off it is decoded like any other frame.
 *
 * Returns the NUMBER OF FRAMES THAT DIFFER — 0: the checkpoint reproduces the tensors — or (size_t)-1.  firstDiff (nFrames entries, or NULL):
 * firstDiff[c] is QZSTD_VERIFY_SAME, or the lowest byte offset inside frame c's chunk at which the restored value differs from the live one.
 * Blocks until done.  `stream` must order the last writer of the tensors and of the bases.
 * (size_t)-1 before anything is queued: everything QZSTD_frontRestoreDeviceBatchDelta refuses (the nFrames rule, element sizes, pointers that
 * are not device memory of one device, a call while another one runs on this front; a front created with useProducer = 0 is accepted), and a
 * device layer without qzstd_hip_ungroup_cmp — every other call is served by such a layer as before.  After work has started: a frame that
 * does not decode, decodes to another length or fails its checksum; with firstDiff given at least the frame a worker stopped at then holds
 * QZSTD_VERIFY_UNDECODED, the other entries are unspecified, and nothing of the library's is still running on the GPU when the call returns.
 * QZSTD_frontRestoreStats, QZSTD_frontDeltaStats and QZSTD_frontDeltaSkipStats do not count this call. */
#define QZSTD_VERIFY_SAME      ((size_t)-1)
#define QZSTD_VERIFY_UNDECODED ((size_t)-2)
size_t QZSTD_frontVerifyDeviceBatch(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                    const QZSTD_DeviceBuf *bufs, const QZSTD_DeviceBuf *bases, const unsigned char *elemSizes, size_t nBufs,
                                    void *stream, size_t *firstDiff /* nFrames entries, or NULL */);
/* since creation, of the parts that were queued: [0] frames compared, [1] of them differing, [2] content bytes compared, [3] qzstd_hip_ungroup_cmp
 * launches (one per part) */
void QZSTD_frontVerifyStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Fingerprints: are the tensors that a restore brought back the tensors that were written — asked at LOAD time, weeks later, when the live
 * tensors Verify needs are gone?  A 64-bit fingerprint (include/qzstd_fingerprint.h: parallel by construction, not XXH64, no wire format) of
 * every chunk is taken on the GPU from the tensor's OWN bytes; the caller keeps it with the frames, 8 bytes per frame, as it keeps element
 * sizes and bases; after any restore one call recomputes it and says which frames differ.  The fingerprint depends on the chunk's bytes and
 * length alone — not on element size, base, level, grouping, probe or checksum settings — so a load against another base, with a swapped
 * element size or with frames in another order, which passes every other check, fails this one.
 *
 * QZSTD_frontFingerprintDeviceBatch: fp[c] = QZSTD_fingerprintOf(chunk c) for the chunks as the compress calls cut frames —
 * QZSTD_frontDeviceBatchFrames entries, the same rule per buffer, none for an empty buffer; firstFrame as in QZSTD_frontCompressDeviceBatch.
 * Returns the frame count.  QZSTD_frontCheckDeviceBatch: the same pass, compared with expected[0 .. nFrames): returns HOW MANY FRAMES
 * DIFFER — 0: the buffers are what was fingerprinted — and differs[c] (nFrames entries, or NULL) is 1 for those and 0 for the others.
 *
 * Both: the host-side pointer and device checks of QZSTD_frontCompressDeviceBatch, the library's stream waits for `stream`, ONE
 * qzstd_hip_fingerprint launch with a row per frame pointing INTO the caller's buffers (nothing is staged, the buffers are only read: one
 * byte read per content byte), one device->host copy of the tile digests (8 bytes per 16 KiB), a bounded wait, and the fold per frame on
 * the calling thread.  Rows and digests live in grow-only pinned and device scratch kept with the front.  Blocks until done.  The calls work
 * on live, restored or never-compressed tensors alike, and on any list of buffers whose chunks are the chunks that were fingerprinted.
 * (size_t)-1 before anything is queued: everything the batch compress call refuses about bufs (a null array, a null pointer with a size,
 * memory that is not device memory of one device), fp — or expected — NULL with frames to write or read, nFrames that is not the buffers'
 * frame count (Check), a call while another one runs on this front, more than 2^32 - 1 frames or 2^31 - 1 tiles (32 TiB) in one call, and a
 * device layer without qzstd_hip_fingerprint (as in the compress calls: also for a call without frames) — every other call is served by such
 * a layer as before.  A front created with useProducer = 0 is accepted.  No buffers, or only empty ones: 0, and no GPU is touched. */
unsigned long long QZSTD_fingerprintOf(const void *p, size_t len); /* QZSTD_fingerprint of include/qzstd_fingerprint.h, exported for bindings */
size_t QZSTD_frontFingerprintDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream, unsigned long long *fp,
                                         size_t *firstFrame /* nBufs + 1, or NULL */);
size_t QZSTD_frontCheckDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, size_t nBufs, void *stream, const unsigned long long *expected,
                                   size_t nFrames, unsigned char *differs /* nFrames entries, or NULL */);
/* since creation, of the calls that succeeded: [0] frames fingerprinted, [1] bytes read on the device, [2] qzstd_hip_fingerprint launches,
 * [3] frames a check found differing */
void QZSTD_frontFingerprintStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Fingerprint, check and verify with SOURCE SLICES: the three calls above for buffers that are not contiguous in device memory, given as
 * QZSTD_frontCompressDeviceSlices takes them — so that a view saved from slices is verified and fingerprinted, and a view restored by
 * QZSTD_frontRestoreDeviceSlices is checked, without the `.contiguous()` copy either.  The slice list obeys that call's rules: the non-empty
 * slices of a buffer, in order, tile [0, bufSizes[i]) exactly; d_src is the live (or restored) bytes of the slice.  In the verify call d_base
 * is the same slice of the base the buffer was written against, or NULL: all slices of a buffer carry one, or none does; it may equal d_src.
 * In the two fingerprint calls d_base is IGNORED — never read, never looked up, mixed based and unbased slices are no error — so the list
 * given to the compress call serves unchanged.
 *
 * Frames are cut every chunkSize bytes of the LOGICAL buffer, and every answer is the contiguous call's for the same bytes held
 * contiguously: fp[c], differs[], the return values and firstDiff[c] (the lowest differing offset inside frame c's chunk, QZSTD_VERIFY_SAME,
 * QZSTD_VERIFY_UNDECODED), with QZSTD_frontSetDeltaSkip on and off — a recognised zero frame made of several slices is compared live
 * against base piece by piece, and is not decoded — and for every element size.
 *
 * A frame that lies inside one piece (slices that follow each other in memory, bases included, are one piece) is handled as a frame of a
 * contiguous buffer is: a call, or a verify part, in which every frame does — one slice per buffer in particular — queues exactly the
 * launches of the contiguous call.  A fingerprint call with at least one frame made of several pieces takes ONE
 * qzstd_hip_fingerprint_pieces launch over all its rows, a verify part that holds such a frame ONE qzstd_hip_ungroup_cmp_pieces launch
 * over all its rows, in the contiguous launch's place.  Rows and the piece table live in grow-only pinned and device scratch kept with the
 * front.  QZSTD_frontFingerprintStats and QZSTD_frontVerifyStats count these calls as they count the contiguous ones.
 *
 * (size_t)-1 before anything is queued: everything the contiguous counterpart refuses that applies (QZSTD_ELEM_DIFF in the verify call
 * among it; the fingerprint calls take no element sizes); everything QZSTD_frontCompressDeviceSlices refuses about bufSizes and slices,
 * with that call's look-ups (consecutive ranges count as one, qzstd_hip_pointer_extent where the layer tells it); in the verify call a
 * buffer with based and unbased slices; and, for a call with a frame made of several pieces, a device layer without the kernel from
 * pieces — such a layer serves a call without such a frame, and every other call, as before.  A front created with useProducer = 0 is
 * accepted.  No slices, or only empty ones: 0, and no GPU is touched. */
size_t QZSTD_frontFingerprintDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices, size_t nSlices,
                                          void *stream, unsigned long long *fp, size_t *firstFrame /* nBufs + 1, or NULL */);
size_t QZSTD_frontCheckDeviceSlices(QZSTD_Front *f, const size_t *bufSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices, size_t nSlices,
                                    void *stream, const unsigned long long *expected, size_t nFrames, unsigned char *differs /* or NULL */);
size_t QZSTD_frontVerifyDeviceSlices(QZSTD_Front *f, const void *frames, size_t frameStride, const size_t *frameSizes, size_t nFrames,
                                     const size_t *bufSizes, const unsigned char *elemSizes, size_t nBufs, const QZSTD_DeviceSrcSlice *slices,
                                     size_t nSlices, void *stream, size_t *firstDiff /* nFrames entries, or NULL */);
/* since creation, of the three calls that succeeded: [0] non-empty slices, [1] their bytes, [2] frames assembled from more than one piece,
 * [3] launches of qzstd_hip_fingerprint_pieces and qzstd_hip_ungroup_cmp_pieces */
void QZSTD_frontSliceCheckStats(QZSTD_Front *f, unsigned long long stats[4]);

/* Advice: which buffers of a list should carry QZSTD_ELEM_DIFF?  Differences shrink columns with order and GROW data without, so the flag is
 * per buffer and the caller's decision; this call makes it from statistics instead of compressing every buffer twice.  Per chunk — cut as the
 * compress calls cut frames — and per 16 KiB tile of its elements the GPU takes the byte histograms of every plane of the grouped layout
 * twice, once for the elements as they are and once for their zigzagged differences, and reduces them to two order-0 cost words
 * (include/qzstd_ediffcost.h over include/qzstd_planecost.h: exact 32-bit words, the same on the device and in plain C).  The host sums them per
 * buffer: P (as they are) and D (differenced), in bytes, and flags the buffer where QZSTD_ediffAdvised(P, D) holds:
 * D + (D >> QZSTD_EDIFF_ADVISE_MARGIN_SHIFT) < P.  P == D, both 0 included, is not flagged: off is the default.
 *
 * elemSizes: as QZSTD_frontCompressDeviceBatchTyped's (1, 2, 4, 8, or 0 for the front's setting; NULL: all 0); an entry that ALREADY carries
 * QZSTD_ELEM_DIFF is refused like any other bad entry.  advised[i] receives the buffer's resolved element size — never 0 — with
 * QZSTD_ELEM_DIFF OR-ed in where differences are advised: the array can be passed as it is to QZSTD_frontCompressDeviceBatchTyped and
 * QZSTD_frontRestoreDeviceBatchTyped, and is kept with the frames as element sizes are.  est (2 * nBufs entries, or NULL): est[2 i] = P and
 * est[2 i + 1] = D of buffer i.  Returns how many buffers are flagged.
 *
 * THE ADVICE IS AN ESTIMATE of what the entropy stage alone can reach.  It does not see matches: the low plane of a sawtooth or an arange
 * costs its full length in P and next to nothing in a frame, so P is overestimated for such columns (D, whose planes are near-noise or
 * constant, is within a few points of the differenced frames' size).  It does not see bases: a buffer is judged as if it had none, and the
 * compress calls refuse a flagged buffer with a base anyway.  It says nothing on whether to byte-group at all.  A caller that knows more may
 * apply its own rule to est and build the array itself.
 *
 * The calling sequence is the fingerprint calls': the host-side pointer and device checks of QZSTD_frontCompressDeviceBatch, the library's stream
 * waits for `stream`, ONE qzstd_hip_ediff_cost launch with a row per chunk pointing INTO the caller's buffers (nothing is staged, the buffers
 * are only read: one byte read per content byte), one device->host copy (8 bytes per 16 KiB), a bounded wait, and the sums on the calling
 * thread.  Rows and words live in grow-only pinned and device scratch kept with the front.  Blocks until done.
 * (size_t)-1 before anything is queued: everything the batch compress call refuses about bufs (a null array, a null pointer with a size,
 * memory that is not device memory of one device), a bad or flagged elemSizes entry, advised NULL with nBufs > 0, a call while another one
 * runs on this front, more than 2^32 - 1 chunks or 2^31 - 1 tiles in one call, and a device layer without qzstd_hip_ediff_cost — every other
 * call is served by such a layer as before.  A front created with useProducer = 0 is accepted.  No buffers, or only buffers shorter than
 * their element: advised[] is filled with the resolved sizes, est with zeros, 0 is returned and no GPU is touched. */
size_t QZSTD_frontAdviseDeviceBatch(QZSTD_Front *f, const QZSTD_DeviceBuf *bufs, const unsigned char *elemSizes, size_t nBufs,
                                    void *stream, unsigned char *advised /* nBufs */, unsigned long long *est /* 2 * nBufs, or NULL */);
/* since creation, of the calls that succeeded: [0] buffers advised on, [1] of them flagged, [2] bytes read on the device (whole elements),
 * [3] qzstd_hip_ediff_cost launches */
void QZSTD_frontAdviseStats(QZSTD_Front *f, unsigned long long stats[4]);
/* QZSTD_ediffCostChunk / QZSTD_ediffAdvised of include/qzstd_ediffcost.h as exported functions (bindings that cannot include the header):
 * sums[0] = P and sums[1] = D of one chunk of len bytes with elements of k bytes; both 0 for a k outside {1, 2, 4, 8} */
void QZSTD_ediffCostOf(const void *chunk, size_t len, unsigned k, unsigned long long sums[2]);
int QZSTD_ediffAdvisedOf(unsigned long long P, unsigned long long D);

#if defined(__cplusplus)
}
#endif
#endif /* QZSTD_FRONTEND_DEVICE_H */
