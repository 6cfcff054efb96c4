/*
 * qzstd_hip_device.h — the device layer's entry points for DEVICE-RESIDENT input (QZSTD_frontCompressDevice in
 * qzstd_frontend_device.h): pointer look-up, events on a caller's stream, a strided device copy, the compaction kernel and the gather kernel
 * (QZSTD_frontCompressDeviceBatch), the byte-grouping gather and its inverse, the ungrouping scatter (QZSTD_frontRestoreDeviceBatchTyped),
 * both also with a base XORed in (the ...Delta calls), the gather also for rows assembled from pieces (QZSTD_frontCompressDeviceSlices), the
 * scatter also for windows of the staged frames (QZSTD_frontRestoreDeviceSlices),
 * the comparison of staged frames with live bytes (QZSTD_frontVerifyDeviceBatch), the comparison of rows with their bases (QZSTD_frontSetDeltaSkip),
 * the content-checksum kernel (QZSTD_frontSetChecksum), the byte histograms' cost per block (QZSTD_frontSetPlaneProbe), the tile
 * digests of the tensor fingerprints (QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch), and the grouping gather with element
 * differences and the element sum that undoes them (QZSTD_ELEM_DIFF in an elemSizes entry of the Typed calls), and the plane costs with and
 * without element differences that advise that flag (QZSTD_frontAdviseDeviceBatch).
 * Additive to qzstd_hip.h (same conventions: 0 on success, < 0 on failure, qzstd_hip_last_error()), which includes this header;
 * exported by the same library (libqatseqprod).
 */
#ifndef QZSTD_HIP_DEVICE_H
#define QZSTD_HIP_DEVICE_H

#include "qzstd_hip.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* the library's device index of a pointer into DEVICE memory (hipPointerGetAttributes); < 0 for host, pinned-host, managed or
 * unknown memory and for a device the library does not use.  Starts no work on any GPU. */
int qzstd_hip_pointer_device(const void *p);
/* qzstd_hip_pointer_device, and the ALLOCATION that holds p: every byte of [*lo, *lo + *size) is memory of the returned device.  *size is 0
 * (and *lo NULL) where p is no device memory or the runtime does not tell: the caller then looks addresses up one by one.  A caller with
 * 10^5 ranges inside one tensor looks the tensor up once (QZSTD_frontCompressDeviceSlices).  The extent is the runtime's answer
 * (hipMemGetAddressRange): for an address range that is reserved and mapped piece by piece it may name more than is mapped — a caller
 * checks the extent's last byte with qzstd_hip_pointer_device before it relies on it.  Starts no work on any GPU. */
int qzstd_hip_pointer_extent(const void *p, const void **lo, size_t *size);
/* events, so that the library's streams wait for work a caller queued on a stream of its own (NULL = the default stream) */
void *qzstd_hip_event_create(int device);
void qzstd_hip_event_destroy(int device, void *event);
int qzstd_hip_event_record(int device, void *event, void *stream);
int qzstd_hip_stream_wait_event(int device, void *stream, void *event);
/* strided device->device copy (qzstd_hip_memcpy2d_d2h's layout): reads exactly `width` bytes of every source row */
int qzstd_hip_memcpy2d_d2d(int device, void *stream, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height);

/*
 * Compaction: one launch's match-finder results (d_src, d_blocks, d_seqs, d_nseq exactly as qzstd_hip_find_sequences left them,
 * 16-byte entries: no QZSTD_HIP_MARK_COMPACT items) packed densely into ONE device arena, so that a single D2H copy brings back
 * what libzstd needs to build the frames (ZSTD_compressSequencesAndLiterals):
 *
 *   [0, 8 * nBlocks)                  per block a header {count, litBytes}: entries including the delimiter, literal bytes;
 *                                     count = QZSTD_HIP_NSEQ_ERROR (litBytes 0) for a block the matcher failed, a block whose
 *                                     entries do not cover exactly [srcOff, srcOff + srcLen), and every block from the first one
 *                                     that would not fit arenaBytes on: such a block contributes nothing below
 *   QZSTD_HIP_COMPACT_ENTRIES_OFF(n)  every block's entries, block after block, QZSTD_HIP_PACK(off, lit, ml, 0), delimiters included
 *   ... + 8 * (sum of counts)         every block's literal bytes, block after block
 *
 * The literals are copied out of d_src inside [srcOff, srcOff + srcLen) of each block and nowhere else.  d_work: scratch of
 * qzstd_hip_compact_workspace_bytes(nBlocks) bytes, private to the launch until it completes.  Asynchronous on `stream`.
 */
#define QZSTD_HIP_COMPACT_ENTRIES_OFF(nBlocks) ((((size_t)(nBlocks) * 8u) + 15u) & ~(size_t)15u)
typedef struct {
    uint32_t count;    /* entries of the block, delimiter included, or QZSTD_HIP_NSEQ_ERROR */
    uint32_t litBytes; /* literal bytes of the block */
} qzstd_hip_compact_hdr_t;
size_t qzstd_hip_compact_workspace_bytes(uint32_t nBlocks);
int qzstd_hip_compact(int device, void *stream, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                      const void *d_seqs, const uint32_t *d_nseq, void *d_arena, size_t arenaBytes, void *d_work, size_t workBytes);

/*
 * Gather: ONE launch copies every row — nRows byte ranges anywhere in device memory, at any alignment — to its place in a staging buffer
 * and writes `pad` zero bytes behind it, so that a part made of many buffers lies in 16-aligned pieces as the match-finder reads them.
 * Work is divided by bytes of the stage (16 KiB per workgroup, the row of every 16-byte word found by a binary search over dstOff), not by
 * rows: rows of one byte and rows of a MiB in one launch keep the device equally busy.  Stores are aligned 16-byte stores; loads are aligned
 * 16-byte loads of the words that overlap [src, src + len) and of no other word, shifted into place in registers.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous) and must stay unchanged until the stream has passed the call; the
 * launcher checks it and uploads it to d_rows, device scratch of nRows entries.  Refused (< 0) before anything is queued: a null
 * rows, d_rows or d_stage, d_stage not 16-aligned, a dstOff or a len + pad that is no multiple of 16, a null src with len > 0, a row
 * that ends past stageBytes, rows that are not in ascending stage order or overlap there (dstOff[i] >= dstOff[i-1] + len[i-1] + pad[i-1]),
 * a stage span of 64 GiB or more (the kernel counts 16-byte words in 32 bits).  Stage bytes between rows are left as they are.
 * No row may overlap the stage in memory.  nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t src;    /* device address of the row's first byte, any alignment */
    uint64_t dstOff; /* byte offset in d_stage, a multiple of 16 */
    uint32_t len;    /* bytes to copy, may be 0 */
    uint32_t pad;    /* zero bytes written behind them; len + pad is a multiple of 16 */
} qzstd_hip_gather_row_t;
int qzstd_hip_gather(int device, void *stream, const qzstd_hip_gather_row_t *rows, uint32_t nRows, qzstd_hip_gather_row_t *d_rows,
                     void *d_stage, size_t stageBytes);

/*
 * Byte-grouping gather: the gather with a per-row element size.  A row's `len` bytes land in the stage in the byte-grouped layout of
 * include/qzstd_bytegroup.h for k = elem — n = len / elem; byte j of elements 0 .. n-1 at [j * n, (j + 1) * n) of the row; the len - n * elem
 * tail bytes behind them, unchanged — and `pad` zero bytes follow.  elem = 1 rows give exactly what qzstd_hip_gather gives.
 *
 * A workgroup takes 16 KiB of ONE row's source (an element range) across all `elem` planes: the source is read once (aligned 16-byte loads
 * of the words that overlap [src, src + len) and of no other word, shifted into place in registers), split into the planes in LDS, and every
 * stage word — a 16-byte word of the stage belongs to the plane and element range of its FIRST byte — leaves with one aligned 16-byte
 * store by one lane.  The owner of a word that reaches into the next element range, the next plane, the tail or the padding fetches those
 * few bytes itself.  No atomics, no read-modify-write of the stage; stage bytes between rows are left as they are.  Rows of one byte and
 * rows of many MiB go in one launch.
 *
 * `rows`, d_rows, the refusals before anything is queued, nRows == 0 and asynchrony: as qzstd_hip_gather, plus an `elem` outside
 * {1, 2, 4, 8} and a `reserved` that is not 0.
 */
typedef struct {
    uint64_t src;      /* device address of the row's first byte, any alignment */
    uint64_t dstOff;   /* byte offset in d_stage, a multiple of 16 */
    uint32_t len;      /* bytes to copy, may be 0 */
    uint32_t pad;      /* zero bytes written behind them; len + pad is a multiple of 16 */
    uint32_t elem;     /* element size: 1, 2, 4 or 8 */
    uint32_t reserved; /* 0 */
} qzstd_hip_group_row_t;
int qzstd_hip_group(int device, void *stream, const qzstd_hip_group_row_t *rows, uint32_t nRows, qzstd_hip_group_row_t *d_rows,
                    void *d_stage, size_t stageBytes);

/*
 * Ungrouping scatter, the inverse of qzstd_hip_group: ONE launch copies every row out of a 16-aligned staging buffer to its destination
 * anywhere in device memory and undoes the byte-grouped layout of include/qzstd_bytegroup.h on the way — for k = elem and n = len / k,
 * dst[e * k + j] = stage[srcOff + j * n + e] for e < n, and the len - n * k tail bytes are copied unchanged.  elem = 1 rows are a plain scatter.
 *
 * EXACTLY the bytes [dst, dst + len) of every row are written, each once, and no other byte of device memory: the 16-byte words that lie
 * wholly inside a row leave as aligned 16-byte stores, the up to 15 bytes in front of the first such word and behind the last as single
 * bytes, and the destination is never read — two rows of one launch may be neighbours in memory and share a 16-byte word (tensor views
 * packed back to back) without a race between their workgroups.  dst may have ANY alignment, also one that is no multiple of elem.
 *
 * A workgroup takes 16 KiB of ONE row's destination (an element range) across all `elem` planes: the plane strips of that range come from the
 * stage into LDS (aligned 16-byte loads inside [srcOff, srcOff + pad16(len)) of the row and nowhere else; the bytes between len and
 * pad16(len) may be loaded and are never looked at), and every destination word — it belongs to the element range of its FIRST byte — is
 * assembled from the strips by one lane; the owner of a word that reaches into the next element range or the tail fetches those few bytes
 * itself.  No atomics.  Rows of one byte and rows of many MiB go in one launch.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous) and must stay unchanged until the stream has passed the call; the
 * launcher checks it and uploads it to d_rows, device scratch of nRows entries.  Refused (< 0) before anything is queued: a null rows,
 * d_rows or d_stage, d_stage not 16-aligned, a srcOff that is no multiple of 16, an elem outside {1, 2, 4, 8}, a null dst with len > 0, a row
 * that ends past stageBytes, rows that are not in ascending stage order or overlap there (srcOff[i] >= srcOff[i-1] + pad16(len[i-1])), a
 * stage span of 64 GiB or more, more than 2^31 - 1 tiles between the first row's and the last row's.  Destinations that overlap each other
 * or the stage are the caller's error and are not checked.  nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t dst;    /* device address of the row's first byte, any alignment */
    uint64_t srcOff; /* byte offset of the row in d_stage, a multiple of 16 */
    uint32_t len;    /* bytes, may be 0 */
    uint32_t elem;   /* element size: 1, 2, 4 or 8; the row lies in the stage in the grouped layout for k = elem */
} qzstd_hip_ungroup_row_t;
int qzstd_hip_ungroup(int device, void *stream, const qzstd_hip_ungroup_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_row_t *d_rows,
                      const void *d_stage, size_t stageBytes);

/*
 * The two above with a BASE XORed in on the way (delta frames: QZSTD_frontCompressDeviceBatchDelta / QZSTD_frontRestoreDeviceBatchDelta) — no
 * temporary of the rows' size, no pass of its own.  A row's `base` is a device address of `len` bytes, at any alignment, also one that
 * differs from the row's src / dst mod 16; 0 = the row has no base and is handled exactly as qzstd_hip_group / qzstd_hip_ungroup handle it.
 *
 * qzstd_hip_group_xor: the stage receives the byte-grouped layout of src[i] ^ base[i], i < len; the padding stays zero.  The base is read
 * under the source's own rule — aligned 16-byte loads of the words that overlap [base, base + len) and of no other word — and XORed with the
 * source's bytes in registers before they are split into the planes; the few bytes a stage word's owner fetches singly have their base byte
 * fetched the same way.  The base is never written; src == base is allowed (a row of zeros).  Everything else — one aligned 16-byte store
 * per stage word, no atomics, stage bytes between rows left alone — is qzstd_hip_group's.
 *
 * qzstd_hip_ungroup_xor: dst[i] = ungrouped[i] ^ base[i], under every write guarantee of qzstd_hip_ungroup (exactly [dst, dst + len) written,
 * each byte once, whole words as aligned 16-byte stores, the up to 15 bytes in front and behind singly).  The base bytes of a destination
 * word are loaded by the lane that stores the word (one aligned load when base and dst agree mod 16, else two and a shift: the word lies
 * inside the row, so both overlap [base, base + len)), those of a head or tail byte as single bytes by the lane that stores the byte.
 * base == dst is therefore allowed — the update in place over a previous checkpoint: every byte is read by its only writer before it is
 * written, and neighbours that share a 16-byte word stay free of races.  A base that overlaps its destination in any other way, or the
 * stage, is the caller's error and is not checked.
 *
 * `rows`, d_rows, nRows == 0, asynchrony and the refusals before anything is queued: those of qzstd_hip_group / qzstd_hip_ungroup; no value
 * of `base` is refused.
 */
typedef struct {
    uint64_t src;      /* device address of the row's first byte, any alignment */
    uint64_t base;     /* device address of the base's first byte, any alignment; 0 = no base */
    uint64_t dstOff;   /* byte offset in d_stage, a multiple of 16 */
    uint32_t len;      /* bytes, may be 0 */
    uint32_t pad;      /* zero bytes written behind them; len + pad is a multiple of 16 */
    uint32_t elem;     /* element size: 1, 2, 4 or 8 */
    uint32_t reserved; /* 0 */
} qzstd_hip_group_xor_row_t;
int qzstd_hip_group_xor(int device, void *stream, const qzstd_hip_group_xor_row_t *rows, uint32_t nRows, qzstd_hip_group_xor_row_t *d_rows,
                        void *d_stage, size_t stageBytes);
typedef struct {
    uint64_t dst;    /* device address of the row's first byte, any alignment */
    uint64_t base;   /* device address of the base's first byte, any alignment; 0 = no base; base == dst: update in place */
    uint64_t srcOff; /* byte offset of the row in d_stage, a multiple of 16 */
    uint32_t len;    /* bytes, may be 0 */
    uint32_t elem;   /* element size: 1, 2, 4 or 8 */
} qzstd_hip_ungroup_xor_row_t;
int qzstd_hip_ungroup_xor(int device, void *stream, const qzstd_hip_ungroup_xor_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_xor_row_t *d_rows,
                          const void *d_stage, size_t stageBytes);

/*
 * Byte-grouping gather from PIECES (QZSTD_frontCompressDeviceSlices): qzstd_hip_group_xor for rows whose content is assembled from pieces that
 * lie anywhere in device memory — a column view, a pitched allocation, scattered pages.  A row owns pieces[piece0 .. piece0 + nPieces); for
 * piece p of the row and i < p.len, c[p.off + i] = src_p[i] ^ base_p[i] (no XOR when base == 0); the stage receives the byte-grouped layout
 * of c[0 .. len) for k = elem at dstOff, and `pad` zero bytes follow.  A row with one piece lands exactly as qzstd_hip_group_xor lands it.
 *
 * The guarantees are qzstd_hip_group's, for pieces: one aligned 16-byte store per stage word, by one lane; no atomics and no
 * read-modify-write of the stage; stage bytes between rows are left alone.  src and base are read only with aligned 16-byte loads of words
 * that overlap THAT PIECE's [src, src + len) or [base, base + len), and of no other word — a piece may end at the last byte of an allocation,
 * and no load is justified by the neighbouring piece.  src == base is allowed; pieces may be one byte long, may begin and end inside an
 * element, and sixteen of them may feed one lane's 16 bytes.  Neither sources nor bases are written.
 *
 * Work is divided as in qzstd_hip_group: a workgroup per 16 KiB tile of one row's content across all planes, the row found by a binary search.
 * One lane then narrows the row's pieces to those that hold the tile's first and last byte (two binary searches over `off`); a lane whose 16
 * content bytes lie inside one piece takes them with one fetch per side, a lane whose bytes straddle pieces assembles them piece by piece,
 * every sub-fetch under the read rule above, and the single bytes that a stage word's owner fetches itself (the next element range, the next
 * plane, the tail) go through the same lookup over all of the row's pieces.  The table is read from device memory, not cached in LDS.
 *
 * `rows` and `pieces` are HOST memory (pinned, for the uploads to be asynchronous) and must stay unchanged until the stream has passed the
 * call; the launcher checks them and uploads them to d_rows and d_pieces, device scratch of nRows and nPieces entries.  Refused (< 0) before
 * anything is queued: everything qzstd_hip_group_xor refuses (the null source is a piece's), a null pieces or d_pieces with nPieces > 0, a
 * piece0 + nPieces past the table, a piece with len == 0 or a null src, pieces of a row that do not tile [0, len) exactly in ascending
 * order (so nPieces == 0 only for len == 0).  No value of a piece's `base` is refused.  nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t src;  /* device address of the piece's first byte, any alignment */
    uint64_t base; /* device address of `len` bytes XORed in, any alignment, also another one mod 16 than src; 0 = none */
    uint32_t off;  /* the piece's first byte in its row's content c[] */
    uint32_t len;  /* bytes, > 0 */
} qzstd_hip_group_piece_t;
typedef struct {
    uint64_t dstOff;   /* byte offset in d_stage, a multiple of 16 */
    uint32_t len;      /* content bytes, may be 0 */
    uint32_t pad;      /* zero bytes written behind them; len + pad is a multiple of 16 */
    uint32_t elem;     /* 1, 2, 4 or 8 */
    uint32_t piece0;   /* the row's first piece */
    uint32_t nPieces;  /* its pieces tile [0, len) exactly, ascending, none empty; 0 only for len == 0 */
    uint32_t reserved; /* 0 */
} qzstd_hip_group_pieces_row_t;
int qzstd_hip_group_pieces(int device, void *stream, const qzstd_hip_group_pieces_row_t *rows, uint32_t nRows,
                           qzstd_hip_group_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                           qzstd_hip_group_piece_t *d_pieces, void *d_stage, size_t stageBytes);

/*
 * Windowed ungrouping scatter (QZSTD_frontRestoreDeviceSlices): qzstd_hip_ungroup_xor for a WINDOW of a staged frame.  The frame lies at
 * srcOff in the byte-grouped layout for k = elem (n = len / k elements, plane j at [j * n, (j + 1) * n), the len - n * k tail bytes behind
 * the planes); with u[] its ungrouped content — u[e * k + j] = stage[srcOff + j * n + e], the tail unchanged — a row writes
 * dst[i] = u[winOff + i] ^ base[i] for i < winLen.  Several rows may be windows of ONE frame (equal srcOff, len and elem): a column shard's
 * pieces.  winOff and winLen are any bytes inside the frame, also mid-element.
 *
 * The guarantees are qzstd_hip_ungroup_xor's, for the window: EXACTLY [dst, dst + winLen) of every row is written, each byte once, and no
 * other byte of device memory; the 16-byte destination words wholly inside the window leave as aligned 16-byte stores, the up to 15 bytes in
 * front of the first and behind the last as single bytes; the destination is never read except as a base; two rows of one launch — two
 * windows of the same frame included — may share a 16-byte destination word without a race; base bytes are loaded by the lane that stores
 * them (base == dst: in place); stage loads are aligned 16-byte loads inside [srcOff, srcOff + pad16(len)) of the row's frame; no atomics.
 *
 * Work is divided by the FRAME's tiles (16 KiB of u[], the tail with the last tile, a frame shorter than k one tile): a row gets a workgroup
 * per tile its window intersects, none for winLen == 0, and a destination word belongs to the tile of its first byte.  A workgroup brings into
 * LDS only the part of each plane strip that covers its share of the window — a 2 KiB window of a 128 KiB fp32 frame fetches about 2 KiB and
 * a word per strip, not 16 KiB.  The launcher writes tile0 (the running sum of the rows' workgroups) into the caller's rows before the upload;
 * a workgroup finds its row by a binary search over it.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_stage, d_stage not 16-aligned, a srcOff that is no multiple of 16, an elem outside
 * {1, 2, 4, 8}, a reserved that is not 0, winOff + winLen > len, a null dst with winLen > 0, a frame that ends past stageBytes,
 * len > 0xFFFFFFE0, a stage span of 64 GiB or more, more than 2^31 - 1 workgroups, rows out of order: srcOff must not decrease; equal srcOff
 * is the same frame — len and elem equal and winOff[i] >= winOff[i-1] + winLen[i-1]; a larger one must be >= srcOff[i-1] + pad16(len[i-1]).
 * No value of `base` is refused.  nRows == 0, or every row with winLen == 0: nothing is queued, 0.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t dst;      /* device address that receives u[winOff]; any alignment */
    uint64_t base;     /* device address of winLen bytes XORed in, any alignment; 0 = none; base == dst: in place */
    uint64_t srcOff;   /* the FRAME's offset in d_stage, a multiple of 16 */
    uint32_t len;      /* the FRAME's content length: fixes n and the tail */
    uint32_t elem;     /* 1, 2, 4 or 8 */
    uint32_t winOff;   /* first byte of u[] wanted; ANY value, also mid-element */
    uint32_t winLen;   /* bytes written; winOff + winLen <= len; may be 0 */
    uint32_t tile0;    /* written by the launcher: workgroups of the rows before this one */
    uint32_t reserved; /* 0 */
} qzstd_hip_ungroup_win_row_t;
int qzstd_hip_ungroup_window(int device, void *stream, qzstd_hip_ungroup_win_row_t *rows, uint32_t nRows,
                             qzstd_hip_ungroup_win_row_t *d_rows, const void *d_stage, size_t stageBytes);

/*
 * Ungrouping comparison (QZSTD_frontVerifyDeviceBatch): qzstd_hip_ungroup_xor with its store replaced by a comparison — does a staged frame,
 * ungrouped and XORed with its base, reproduce the LIVE bytes at `ref`?  With u[] the frame's ungrouped content exactly as qzstd_hip_ungroup
 * defines it (u[e * k + j] = stage[srcOff + j * n + e] for k = elem, n = len / k; the len - n * k tail bytes unchanged), and u[] all zeros for a
 * ZERO row (flags bit 0: a recognised canonical zero frame — the stage is not read and srcOff not looked at), a row MATCHES when
 * u[i] ^ base[i] == ref[i] for every i < len; base 0 means no XOR.  ref == base is allowed (u[] is compared with zero).
 *
 * Work is divided as in the window and diff kernels: a workgroup per 16 KiB tile of u[] — QZSTD_HIP_CMP_TILES(len, elem) of them: the tail
 * goes with the last tile, a frame shorter than elem is one tile, an empty row has none.  The launcher writes tile0 (the running sum of the
 * rows' workgroups) into the caller's rows before the upload; a workgroup finds its row by a binary search over it.  Every workgroup stores
 * ONE word: d_tiles[tile0 + t] = QZSTD_HIP_CMP_SAME when its share of the row matches, else the lowest differing row offset i it saw; the
 * host takes the first entry of a row that is not QZSTD_HIP_CMP_SAME.  d_tiles holds the sum of the rows' QZSTD_HIP_CMP_TILES words.
 *
 * No atomics, no memset; nothing but d_tiles[0 .. total tiles) is written — ref, base and the stage are only read.  ref and base are read
 * with aligned 16-byte loads of the words that overlap [p, p + len) and of no other word, each shifted into place by its own misalignment;
 * stage loads are aligned 16-byte loads inside [srcOff, srcOff + pad16(len)) of the row; the bytes of a first or last word that lie outside
 * the row never influence the result; every byte of [0, len) is compared by some lane.  The lowest differing offset of a tile is found with
 * a wave min and one LDS step across the four waves.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_tiles, a null d_stage with a row that is neither ZERO nor empty, d_stage not 16-aligned, an
 * elem outside {1, 2, 4, 8}, a flags bit other than bit 0, a null ref with len > 0, len > 0xFFFFFFE0, more than 2^31 - 1 workgroups, and for
 * the rows that are not ZERO: a srcOff that is no multiple of 16, a frame that ends past stageBytes, frames out of ascending stage order or
 * overlapping (srcOff >= the previous such row's srcOff + pad16(len)).  No value of `base` is refused.  nRows == 0, or only empty rows:
 * nothing is queued, 0.  Asynchronous on `stream`.
 */
#define QZSTD_HIP_CMP_SAME 0xFFFFFFFFu
#define QZSTD_HIP_CMP_ZERO 1u /* flags bit 0 */
/* workgroups of a row = its words in d_tiles */
#define QZSTD_HIP_CMP_TILES(len, elem)                                                                                    \
    ((uint64_t)(len) / (elem) ? ((uint64_t)(len) / (elem) + 16384u / (elem) - 1u) / (16384u / (elem)) : (uint64_t)((len) ? 1u : 0u))
typedef struct {
    uint64_t ref;    /* device address of the `len` live bytes to compare with, any alignment */
    uint64_t base;   /* device address of `len` bytes XORed in first, any alignment, also another one mod 16 than ref; 0 = none */
    uint64_t srcOff; /* the frame's offset in d_stage, a multiple of 16 (not looked at for a ZERO row) */
    uint32_t len;    /* content bytes, may be 0 */
    uint32_t elem;   /* 1, 2, 4 or 8: the grouped layout the frame lies in */
    uint32_t flags;  /* QZSTD_HIP_CMP_ZERO: the frame's content is `len` zero bytes and the stage is not read; other bits 0 */
    uint32_t tile0;  /* written by the launcher: workgroups of the rows before this one */
} qzstd_hip_ungroup_cmp_row_t;
int qzstd_hip_ungroup_cmp(int device, void *stream, qzstd_hip_ungroup_cmp_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_cmp_row_t *d_rows,
                          const void *d_stage, size_t stageBytes, uint32_t *d_tiles);

/*
 * Comparison with a base (QZSTD_frontSetDeltaSkip): ONE launch compares every row's two byte ranges — d_flags[i] = 1 when any of the `len`
 * bytes at a and b differ, 0 when none does; an empty row gives 0.  a and b have any alignment, also different ones mod 16; a == b is allowed.
 *
 * Work is divided by bytes: a workgroup per 16 KiB tile of a row, none for an empty row, so rows of one byte and rows of 64 MiB in one launch
 * keep the device equally busy.  The launcher writes tile0 (the running sum of the rows' workgroups) into the caller's rows before the upload;
 * a workgroup finds its row by a binary search over it.  Loads are aligned 16-byte loads of the words that overlap [a, a + len) and
 * [b, b + len) and of no other word, each side shifted into place in registers by its own misalignment; the bytes of a row's first and last
 * words that lie outside the range never influence the flag.  The lanes OR their XORs, a wave votes, and one lane of a wave that saw a
 * difference stores the value 1 to d_flags[row] — an ordinary store; several waves may store the same 1.  The launcher zeroes
 * d_flags[0 .. nRows) first (a memset on the same stream).  No atomics, no read-modify-write; nothing but d_flags[0 .. nRows) is written.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_flags, a null a or b with len > 0, len > 0xFFFFFFE0, more than 2^31 - 1 workgroups.
 * nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t a, b;  /* device addresses of `len` bytes each, any alignment, also different mod 16; a == b allowed */
    uint32_t len;   /* may be 0 */
    uint32_t tile0; /* written by the launcher: workgroups of the rows before this one */
} qzstd_hip_diff_row_t;
int qzstd_hip_diff(int device, void *stream, qzstd_hip_diff_row_t *rows, uint32_t nRows, qzstd_hip_diff_row_t *d_rows, uint32_t *d_flags);

/*
 * Content checksum: ONE launch hashes every row — d_out[i] = XXH64, seed 0, of the `len` bytes at d_base + srcOff (the full 64-bit value; a
 * zstd frame stores its low 32 bits).  The rows are a part's frames where the match-finder reads them (the stage, or the caller's buffer
 * for a part read in place): both start every frame 16-aligned, hence the alignment rule.  XXH64's four accumulators are serial chains
 * (the rotation breaks linearity), so the parallelism is ACROSS rows: a wave takes 16 rows, four lanes per row, one lane per accumulator;
 * rows of different lengths in a wave finish independently.  A row much longer than its neighbours is one long chain (64 MiB: 2 M steps).
 * Loads are aligned 16-byte loads of the words that overlap [srcOff, srcOff + len) and of no other word; the bytes behind `len` in a row's
 * last word are loaded and never looked at.  Only d_out[0 .. nRows) is written.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous) and must stay unchanged until the stream has passed the call; the
 * launcher checks it and uploads it to d_rows, device scratch of nRows entries.  Refused (< 0) before anything is queued: a null rows,
 * d_rows or d_out, a null d_base with a row that is not empty, a d_base that is not 16-aligned, a srcOff that is no multiple of 16.
 * nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
#define QZSTD_HIP_XXH64_TILE 1024u /* bytes of a row the kernel fetches at a time (tests place lengths around its multiples) */
typedef struct {
    uint64_t srcOff; /* bytes from d_base, a multiple of 16 */
    uint64_t len;    /* bytes to hash, may be 0 */
} qzstd_hip_hash_row_t;
int qzstd_hip_xxh64(int device, void *stream, const void *d_base, const qzstd_hip_hash_row_t *rows, uint32_t nRows,
                    qzstd_hip_hash_row_t *d_rows, uint64_t *d_out);

/*
 * Plane cost (QZSTD_frontSetPlaneProbe): ONE launch takes the byte histogram of every row — the `len` bytes at d_base + srcOff, at ANY byte
 * offset — and leaves ONE word per row: d_cost[i] = QZSTD_planeCost(histogram, len) of include/qzstd_planecost.h, the order-0 cost of the row in
 * bytes, computed on the device with that header's own functions.  The rows are a part's block descriptors over the launch's base (the
 * stage, or the caller's buffer for a part read in place); the front-end predicts Raw_Blocks from the words (QZSTD_planeIsRaw).
 *
 * One workgroup of 256 threads per row.  Loads are aligned 16-byte loads of the words that overlap [srcOff, srcOff + len) and of no other
 * word; the bytes of the first and last word outside the row are never counted.  The histogram lives in LDS, in 16 copies (a lane's copy is
 * its index mod 16, bin b of copy c at word 16 b + c) that LDS atomics fill, so that a plane of a handful of values does not serialise on
 * one word; a reduction over the workgroup follows and one ordinary store.  No global atomics, no memset; nothing but d_cost[0 .. nRows)
 * is written.  An empty row costs 0 and loads nothing.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous) and must stay unchanged until the stream has passed the call; the
 * launcher checks it and uploads it to d_rows, device scratch of nRows entries.  Refused (< 0) before anything is queued: a null rows,
 * d_rows or d_cost, a null d_base with a row that is not empty, a len above 131072 (QZSTD_PLANE_LEN_MAX), a reserved that is not 0, more
 * than 2^31 - 1 rows.  nRows == 0: nothing happens.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t srcOff;   /* bytes from d_base, any value */
    uint32_t len;      /* bytes, 0 .. 131072 */
    uint32_t reserved; /* 0 */
} qzstd_hip_plane_row_t;
int qzstd_hip_plane_cost(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                         qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost);

/*
 * Huffman literals coder (include/qzstd_hufblock.h): the rows of qzstd_hip_plane_cost, and per row the SAME cost word in d_cost — a caller
 * queues this launch instead of that one — plus, for the rows worth it, the jump table and the four Huffman streams of a zstd
 * Compressed_Literals_Block, computed on the device with that header's own definitions.
 *
 * Per row (one workgroup of 256 threads): the byte histogram in LDS as in the cost kernel (aligned 16-byte loads of the words that overlap
 * the row and of no other word), the cost word, the code lengths (the bytes that occur are ranked by the workgroup, then
 * QZSTD_hufLengthsSorted on one lane), the canonical codes; then one wave per stream, a lane per run of consecutive bytes: the lanes sum
 * their runs' code lengths, a scan per stream in the stream's reversed order gives every run its bit offset, and the lanes pack — whole 32-bit
 * words straight to memory, the words a lane shares with its neighbours merged in LDS and stored once.
 *
 *   d_size[i]   the row's size word: bytes of jump table + streams, or 0 — len outside QZSTD_HUF_LEN_MIN .. QZSTD_HUF_LEN_MAX, fewer than two
 *               distinct bytes, or jump table + streams not below len - ((len >> 6) + 2) (QZSTD_hufSizeWord)
 *   d_off[i]    where row i's bytes start in d_dense, i = 0 .. nRows; d_off[nRows] is the bytes used.  A multiple of 16 each.
 *   d_dense     for every row with a size word, in row order: QZSTD_HUF_LENGTHS_BYTES (128) of code lengths, a nibble each
 *               (QZSTD_hufPackLengths), the d_size[i] bytes, and zeros up to the next multiple of 16.  Other rows take no room.
 *
 * Four launches on `stream`: a scan of the rows' scratch needs, the coder (into d_scratch, a row's bytes at a place of its own), a scan of
 * the size words into d_off, and a copy into d_dense; no workgroup waits for another.  No global atomics, no memset; nothing is written
 * but d_rows, d_cost, d_size, d_off[0 .. nRows], d_dense[0 .. d_off[nRows]) and d_scratch.
 *
 * qzstd_hip_huf_code_bytes(rows, nRows): the bytes of d_dense that every outcome fits in — the sum of QZSTD_HIP_HUF_ROW_BYTES(len) — or
 * (size_t)-1 when that is 4 GiB or more.  d_scratch needs QZSTD_HIP_HUF_SCRATCH_BYTES(nRows, that).  Both 16-byte aligned.
 *
 * `rows` is HOST memory as for qzstd_hip_plane_cost.  Refused (< 0) before anything is queued: what qzstd_hip_plane_cost refuses, a null
 * d_size, d_off, d_dense or d_scratch, a d_dense or d_scratch that is not 16-byte aligned or too small.  nRows == 0: nothing happens.
 */
#define QZSTD_HIP_HUF_ROW_BYTES(len) ((len) >= 1024u && (len) <= 131072u ? (((size_t)(len) + 15u) & ~(size_t)15u) + 128u : (size_t)0)
#define QZSTD_HIP_HUF_SCRATCH_BYTES(nRows, denseBytes) (((((size_t)(nRows) + 1u) * 4u + 15u) & ~(size_t)15u) + (size_t)(denseBytes))
size_t qzstd_hip_huf_code_bytes(const qzstd_hip_plane_row_t *rows, uint32_t nRows);
int qzstd_hip_huf_code(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                       qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost, uint32_t *d_size, uint32_t *d_off, void *d_dense, size_t denseBytes,
                       void *d_scratch, size_t scratchBytes);

/*
 * Fingerprint (QZSTD_frontFingerprintDeviceBatch / QZSTD_frontCheckDeviceBatch): ONE launch digests every row — `len` bytes anywhere in device
 * memory, at any alignment — tile by tile: d_tiles[tile0 + j] = QZSTD_fpTile of include/qzstd_fingerprint.h over the row's j-th 16 KiB (the
 * last tile: what is left), computed on the device with that header's own functions.  The host folds a row's tile digests into its
 * fingerprint (QZSTD_fpFold): 8 bytes per 16 KiB come back.
 *
 * Work is divided as in qzstd_hip_diff: a workgroup of 256 threads per 16 KiB tile of a row — QZSTD_HIP_FP_TILES(len) of them, none for an
 * empty row — so rows of one byte and rows of 64 MiB in one launch keep the device equally busy.  The launcher writes tile0 (the running sum
 * of the rows' workgroups) into the caller's rows before the upload; a workgroup finds its row by a binary search over it.  Loads are aligned
 * 16-byte loads of the words that overlap [src, src + len) and of no other word, shifted into place in registers by the row's own
 * misalignment; the bytes behind the row's last one are set to 0 before they are looked at, those in front of the first never arrive.  The
 * lanes are folded across each wave (shuffles) and across the four waves (one LDS step), and one lane stores the tile's ONE word with an
 * ordinary 8-byte store.  No atomics, no memset, no read-modify-write; nothing but d_tiles[0 .. sum of the rows' QZSTD_HIP_FP_TILES) is
 * written — the rows' bytes are only read.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_tiles, a null src with len > 0, len > 0xFFFFFFE0, more than 2^31 - 1 workgroups.
 * nRows == 0, or only empty rows: nothing is queued, 0.  Asynchronous on `stream`.
 */
#define QZSTD_HIP_FP_TILES(len) (((uint64_t)(len) + 16383u) >> 14)
typedef struct {
    uint64_t src;   /* device address of the row's first byte, any alignment */
    uint32_t len;   /* bytes, may be 0 */
    uint32_t tile0; /* written by the launcher: workgroups of the rows before this one */
} qzstd_hip_fp_row_t;
int qzstd_hip_fingerprint(int device, void *stream, qzstd_hip_fp_row_t *rows, uint32_t nRows, qzstd_hip_fp_row_t *d_rows, uint64_t *d_tiles);

/*
 * Fingerprint from PIECES (QZSTD_frontFingerprintDeviceSlices / QZSTD_frontCheckDeviceSlices): qzstd_hip_fingerprint for rows whose content
 * is the concatenation of pieces that lie anywhere in device memory (the piece table of qzstd_hip_group_pieces: a row owns
 * pieces[piece0 .. piece0 + nPieces), c[p.off + i] = src_p[i]).  d_tiles[tile0 + j] = QZSTD_fpTile over the j-th 16 KiB of c[] (the last
 * tile: what is left), by the header's own functions: exactly what qzstd_hip_fingerprint leaves for the same bytes held contiguously.
 *
 * Work is divided as in qzstd_hip_fingerprint: a workgroup of 256 threads per 16 KiB tile of a row, the row found by a binary search over
 * tile0 (written by the launcher).  One lane narrows the row's pieces to those that hold the tile's first and last byte; every lane takes
 * its four words (t, t + 256, t + 512, t + 768) through the lookup of qzstd_hip_group_pieces — one fetch for a word inside a piece, piece
 * by piece for a word that straddles pieces, up to sixteen one-byte pieces per word — and the rounds, the tree and the single 8-byte
 * store are qzstd_hip_fingerprint's.  No atomics, no memset, no read-modify-write; nothing but d_tiles[0 .. sum of the rows'
 * QZSTD_HIP_FP_TILES) is written.  Sources are read only with aligned 16-byte loads of words that overlap THAT PIECE's [src, src + len),
 * and of no other word — a piece may end on an allocation's last byte; a base is never read.  No workgroup waits for another.  The piece
 * table is read from device memory, not cached in LDS.
 *
 * `rows` and `pieces` are HOST memory (pinned, for the uploads to be asynchronous); `rows` is WRITTEN by the launcher (tile0 only, and only
 * by a launch that is not refused); both must stay unchanged until the stream has passed the call; d_rows and d_pieces: device scratch of
 * nRows and nPieces entries.  Refused (< 0) before anything is queued: what qzstd_hip_fingerprint refuses (the null source is a piece's),
 * what qzstd_hip_group_pieces refuses about the table (a null pieces or d_pieces with nPieces > 0, a piece0 + nPieces past the table, a
 * piece with len == 0 or a null src, pieces of a row that do not tile [0, len) exactly in ascending order), and a piece whose `base` is
 * not 0.  nRows == 0, or only empty rows: nothing is queued, 0.  Asynchronous on `stream`.
 */
typedef struct {
    uint32_t len;     /* content bytes, may be 0 */
    uint32_t tile0;   /* written by the launcher: workgroups of the rows before this one */
    uint32_t piece0;  /* the row's first piece */
    uint32_t nPieces; /* its pieces tile [0, len) exactly, ascending, none empty; 0 only for len == 0 */
} qzstd_hip_fp_pieces_row_t;
int qzstd_hip_fingerprint_pieces(int device, void *stream, qzstd_hip_fp_pieces_row_t *rows, uint32_t nRows, qzstd_hip_fp_pieces_row_t *d_rows,
                                 const qzstd_hip_group_piece_t *pieces, uint32_t nPieces, qzstd_hip_group_piece_t *d_pieces, uint64_t *d_tiles);

/*
 * Ungrouping comparison with PIECES (QZSTD_frontVerifyDeviceSlices): qzstd_hip_ungroup_cmp for rows whose live bytes (and base) are pieces
 * that lie anywhere in device memory.  With u[] as qzstd_hip_ungroup_cmp defines it (all zeros for a ZERO row, whose stage is never read),
 * a row MATCHES when u[p.off + i] ^ base_p[i] == src_p[i] for every piece p of the row and every i < p.len; base 0 means no XOR;
 * src == base is allowed.  Tiles, the tail with the last tile, QZSTD_HIP_CMP_TILES, the ONE word per tile (QZSTD_HIP_CMP_SAME, or the
 * lowest differing row offset) and the wave-min / LDS reduction are qzstd_hip_ungroup_cmp's; one lane narrows the row's pieces to those
 * that hold the tile's first and last byte, and a lane fetches src ^ base of its 16 bytes through the lookup of qzstd_hip_group_pieces.
 *
 * No atomics, no memset, no read-modify-write; nothing but d_tiles[0 .. total tiles) is written.  Sources and bases are read only with
 * aligned 16-byte loads of words that overlap THAT PIECE's [src, src + len) or [base, base + len), and of no other word — a piece may end
 * on an allocation's last byte; stage loads are qzstd_hip_ungroup_cmp's.  No workgroup waits for another.  The piece table is read from
 * device memory, not cached in LDS.
 *
 * `rows` and `pieces` are HOST memory (pinned); `rows` is WRITTEN by the launcher (tile0 only, and only by a launch that is not refused);
 * both must stay unchanged until the stream has passed the call.  Refused (< 0) before anything is queued: what qzstd_hip_ungroup_cmp
 * refuses (the null ref is a piece's null src) and what qzstd_hip_group_pieces refuses about the table.  No value of a piece's `base` is
 * refused.  nRows == 0, or only empty rows: nothing is queued, 0.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t srcOff;  /* the frame's offset in d_stage, a multiple of 16 (not looked at for a ZERO row) */
    uint32_t len;     /* content bytes, may be 0 */
    uint32_t elem;    /* 1, 2, 4 or 8: the grouped layout the frame lies in */
    uint32_t flags;   /* QZSTD_HIP_CMP_ZERO; other bits 0 */
    uint32_t tile0;   /* written by the launcher: workgroups of the rows before this one */
    uint32_t piece0;  /* the row's first piece */
    uint32_t nPieces; /* its pieces tile [0, len) exactly, ascending, none empty; 0 only for len == 0 */
} qzstd_hip_ungroup_cmp_pieces_row_t;
int qzstd_hip_ungroup_cmp_pieces(int device, void *stream, qzstd_hip_ungroup_cmp_pieces_row_t *rows, uint32_t nRows,
                                 qzstd_hip_ungroup_cmp_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                 qzstd_hip_group_piece_t *d_pieces, const void *d_stage, size_t stageBytes, uint32_t *d_tiles);

/*
 * Byte-grouping gather with element differences (include/qzstd_elemdiff.h): qzstd_hip_group with a `flags` word in place of `reserved`.
 * A row without QZSTD_HIP_EDIFF_DIFF lands exactly as qzstd_hip_group lands it; a row with it lands as the grouped layout of
 * QZSTD_elemDiff(row, len, elem) — z[e] = zigzag(x[e] - x[e-1]), x[-1] = 0, the tail bytes unchanged — and `pad` zero bytes follow.
 * Elements count from the row's first byte, not from memory alignment: src may have any alignment, also one that is no multiple of elem.
 *
 * The tile is qzstd_hip_group's: 16 KiB of ONE row's source across all planes.  The differences are taken in registers between the fetch
 * and the split into planes: a lane's 16 source bytes hold whole elements, the element in front of them comes from the lane before by a
 * shuffle, and the first lane of a wave — so also the first of a tile — fetches that one element itself (elem bytes at any alignment, under
 * the source-read rule: aligned 16-byte loads of words that overlap [src, src + len) only).  The bytes a stage word's owner fetches singly
 * are computed from the two elements they depend on, fetched the same way.  Everything else — one aligned 16-byte store per stage word, no
 * atomics, no read-modify-write, stage bytes between rows left alone, `rows` / d_rows, nRows == 0, asynchrony and the refusals before
 * anything is queued — is qzstd_hip_group's, with "a flags bit other than bit 0" in place of "a reserved that is not 0".  Two launches over
 * disjoint ascending subsets of a part's rows (this one for the rows with differences, qzstd_hip_group for the rest) do not disturb each other.
 */
#define QZSTD_HIP_EDIFF_DIFF 1u /* flags bit 0 */
typedef struct {
    uint64_t src;    /* device address of the row's first byte, any alignment */
    uint64_t dstOff; /* byte offset in d_stage, a multiple of 16 */
    uint32_t len;    /* bytes, may be 0 */
    uint32_t pad;    /* zero bytes written behind them; len + pad is a multiple of 16 */
    uint32_t elem;   /* element size: 1, 2, 4 or 8 */
    uint32_t flags;  /* QZSTD_HIP_EDIFF_DIFF: differences are taken; other bits 0 */
} qzstd_hip_group_ediff_row_t;
int qzstd_hip_group_ediff(int device, void *stream, const qzstd_hip_group_ediff_row_t *rows, uint32_t nRows,
                          qzstd_hip_group_ediff_row_t *d_rows, void *d_stage, size_t stageBytes);

/*
 * Element sum, the inverse of the differences, IN PLACE on the destinations: with k = elem, n = len / k and z[e] the little-endian k-byte
 * integer at dst + e * k, every row becomes x[e] = sum over i <= e of unzigzag(z[i]) mod 2^(8k) — QZSTD_elemSum(dst, dst, len, k).
 * dst has ANY alignment, also one that is no multiple of elem; a row may be far longer than a frame (len up to 0xFFFFFFE0).
 *
 * EXACTLY the bytes [dst, dst + n * k) of every row are written, each once: the 16-byte words that lie wholly inside that range leave as
 * aligned 16-byte stores, the up to 15 bytes in front of the first such word and behind the last as single bytes — two rows of one launch
 * may be neighbours in memory and share a 16-byte word.  The len - n * k tail bytes are never written.  Loads are aligned 16-byte loads
 * of the words that overlap [dst, dst + n * k) and of no other word.
 *
 * Work is divided by 16 KiB tiles of a row (QZSTD_HIP_ESUM_TILES; a row shorter than elem has none): the launcher writes tile0 (the running
 * sum of the rows' tiles) into the caller's rows before the upload; a workgroup finds its row by a binary search over it.  No workgroup
 * waits for another; three launches, ordered by the stream:
 *   1  a workgroup per tile stores the tile's 64-bit sum and a copy of the tile's first 16 bytes into d_scratch
 *   2  ONE workgroup turns the sums into their exclusive prefix sums (over all tiles of the launch; a row's carry into tile t is the
 *      difference between the prefix at t and the prefix at the row's first tile: addition mod 2^64 is exact for every k)
 *   3  a workgroup per tile un-zigzags in registers, scans its tile (shuffles inside a wave, one LDS step across the four waves), adds the
 *      carry, and stores through LDS, where the sums are realigned from element to memory alignment.  A destination word belongs to the
 *      tile of its first byte in the row; the owner of a word that reaches into the next tile sums that tile's first elements itself, from
 *      the copy of pass 1 — the next tile's workgroup may have replaced them already — and every tile reads its own first 16 bytes there too.
 * d_scratch: device memory of QZSTD_HIP_ESUM_SCRATCH_BYTES(total tiles) bytes, 16-aligned, private to the launch until it completes.
 * No atomics.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_scratch, a d_scratch that is not 16-aligned or smaller than the tiles need, an elem outside
 * {1, 2, 4, 8}, a reserved that is not 0, a null dst with len >= elem, len > 0xFFFFFFE0, more than 2^31 - 1 tiles.  Destinations that
 * overlap each other are the caller's error and are not checked.  nRows == 0, or no row with an element: nothing is queued, 0.
 * Asynchronous on `stream`.
 */
#define QZSTD_HIP_ESUM_TILES(len, elem) (((uint64_t)(len) / (elem) + 16384u / (elem) - 1u) / (16384u / (elem)))
#define QZSTD_HIP_ESUM_SCRATCH_BYTES(tiles) ((size_t)(tiles) * 24u) /* 16 bytes of every tile's head, then 8 of its sum */
typedef struct {
    uint64_t dst;      /* device address of the row's first byte, any alignment */
    uint32_t len;      /* bytes; n = len / elem elements are summed, the rest is left alone */
    uint32_t elem;     /* element size: 1, 2, 4 or 8 */
    uint32_t tile0;    /* written by the launcher: tiles of the rows before this one */
    uint32_t reserved; /* 0 */
} qzstd_hip_esum_row_t;
int qzstd_hip_esum(int device, void *stream, qzstd_hip_esum_row_t *rows, uint32_t nRows, qzstd_hip_esum_row_t *d_rows, void *d_scratch,
                   size_t scratchBytes);

/*
 * Element-difference cost (QZSTD_frontAdviseDeviceBatch): ONE launch reads every row — `len` bytes anywhere in device memory, at any
 * alignment, also one that is no multiple of elem; one byte read per content byte — and leaves TWO words per 16 KiB tile of its elements:
 * d_tiles[2 (tile0 + j)] = plain and d_tiles[2 (tile0 + j) + 1] = diff of include/qzstd_ediffcost.h (QZSTD_ediffCostTile: the order-0 cost of
 * every byte plane of the tile's elements as they are, and of their zigzagged differences), computed on the device with that header's and
 * qzstd_planecost.h's own functions.  Tiles are qzstd_hip_esum's (QZSTD_HIP_ESUM_TILES; a row shorter than elem has none, the len - n * elem
 * tail bytes are in no histogram); differences are per row, x[-1] = 0.  The host sums a row's words.
 *
 * One workgroup of 256 threads per tile; its row is found by a binary search over tile0, which the launcher writes (the running sum of the
 * rows' tiles).  Loads are aligned 16-byte loads of the words that overlap [src, src + n * elem) and of no other word, shifted into place by
 * the row's own misalignment; a lane's 16 bytes are whole elements counted from the row's first byte, the element in front of them comes
 * from the lane before by a shuffle that every lane executes, and the first lane of a wave fetches it itself (0 at the row's start) — what
 * qzstd_hip_group_ediff does.  The 2 * elem histograms live in LDS, each in 16 / elem copies (a lane's copy is its index mod 16 / elem;
 * 32 KiB for every elem); a plane on which all of a wave's bytes agree — the zero planes of small differences, the constant upper bytes of
 * timestamps — gets ONE add of the wave's element count by one lane.  A reduction with QZSTD_planeTerm and QZSTD_planeCostOfSum follows, and
 * one lane stores the tile's two words as one 8-byte store.  No global atomics, no memset, no workgroup waits for another; nothing but
 * d_tiles[0 .. 2 * total tiles) is written — the rows' bytes are only read.
 *
 * `rows` is HOST memory (pinned, for the upload to be asynchronous), is WRITTEN by the launcher (tile0 only, and only by a launch that is
 * not refused) and must stay unchanged until the stream has passed the call; d_rows: device scratch of nRows entries.  Refused (< 0) before
 * anything is queued: a null rows, d_rows or d_tiles, a d_tiles that is not 8-byte aligned, a null src with len >= elem, an elem outside
 * {1, 2, 4, 8}, a reserved that is not 0, len > 0xFFFFFFE0, more than 2^31 - 1 tiles.  nRows == 0, or no row with an element: nothing is
 * queued, 0.  Asynchronous on `stream`.
 */
typedef struct {
    uint64_t src;      /* device address of the row's first byte, any alignment */
    uint32_t len;      /* bytes; n = len / elem elements are counted, the rest is left out */
    uint32_t elem;     /* element size: 1, 2, 4 or 8 */
    uint32_t tile0;    /* written by the launcher: tiles of the rows before this one */
    uint32_t reserved; /* 0 */
} qzstd_hip_ediff_cost_row_t;
int qzstd_hip_ediff_cost(int device, void *stream, qzstd_hip_ediff_cost_row_t *rows, uint32_t nRows, qzstd_hip_ediff_cost_row_t *d_rows,
                         uint32_t *d_tiles);

#if defined(__cplusplus)
}
#endif
#endif /* QZSTD_HIP_DEVICE_H */
