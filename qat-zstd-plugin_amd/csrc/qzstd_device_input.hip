/*
 * qzstd_device_input.hip — the kernels for input that already lives in device memory, and the part of include/qzstd_hip_device.h that
 * launches them: compaction of a launch's sequences and literals into one arena, the gather of rows into a stage, the byte-grouping
 * gather for typed rows and the ungrouping scatter that undoes it, both also with a base XORed in on the way (delta frames), the gather also for
 * rows assembled from pieces (source slices), the scatter also for
 * windows of the staged frames (slices), the comparison of staged frames with live bytes (verify), the comparison of rows with their bases (delta skip), the XXH64 content checksum, the plane cost (plane probe), the tile digests of the tensor fingerprints, and the grouping gather with element differences and the element sum (integer columns).  They use nothing of the match-finder
 * (qzstd_kernels.hip).  What the launchers of row tables and their kernels share — the checks, the refusals' text, the workgroup's search
 * for its row — stands once, in the section "row tables" behind the plain gather's kernel.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "qzstd_hip.h"
#include "qzstd_hip_device.h"
#include "qzstd_hip_internal.h"

/* ---------------------------------------------------------------- device-resident input: compaction ---------- */
/*
 * qzstd_hip_compact (include/qzstd_hip_device.h): a launch's ZSTD_Sequence entries (16 B each, in device memory) and the literal bytes they
 * name, packed densely into one arena — 8-byte entries (QZSTD_HIP_PACK, tag 0) and the literals back to back — so that one D2H copy of
 * about 0.64 B per input byte (level 1, text) gives libzstd everything ZSTD_compressSequencesAndLiterals needs.  Three kernels:
 *   count  one workgroup per block: checks the block's entries and sums their literal bytes -> header {count, litBytes}
 *   scan   one workgroup: exclusive prefix sums of entries and literal bytes over the blocks, the arena's capacity check
 *   emit   one workgroup per block: packs the entries and copies the literal runs, a chunk of kCompactT entries at a time (the
 *          destination and source offsets of the runs are a scan of litLength and litLength + matchLength over the chunk in LDS)
 * A block is emitted only when its entries cover exactly [0, srcLen): every literal read lies inside [srcOff, srcOff + srcLen).
 */
namespace {
constexpr uint32_t kCompactT = 512u; /* threads per workgroup of the count and emit kernels, entries per chunk of the emit kernel */

/* block-wide inclusive scan of one 64-bit value per thread (kCompactT threads); `red` holds kCompactT / 64 partials */
__device__ inline unsigned long long compact_scan(unsigned long long v, unsigned long long *red, unsigned long long *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == 63u) red[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t w = 0; w < kCompactT / 64u; w++) {
        const unsigned long long r = red[w];
        if (w < wave) before += r;
        all += r;
    }
    __syncthreads(); /* red is reused by the next call */
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(kCompactT) void qzstd_compact_count_kernel(const qzstd_hip_block_t *__restrict__ blocks, const uint4 *__restrict__ seqs,
                                                                        const uint32_t *__restrict__ nseq, qzstd_hip_compact_hdr_t *__restrict__ hdr)
{
    __shared__ unsigned long long red[kCompactT / 64u];
    const qzstd_hip_block_t bk = blocks[blockIdx.x];
    const uint32_t count = nseq[blockIdx.x];
    bool ok = count != QZSTD_HIP_NSEQ_ERROR && count >= 1u && count <= bk.seqCap && (bk.mark & QZSTD_HIP_MARK_COMPACT) == 0u;
    unsigned long long lit = 0, cover = 0, bad = 0;
    if (ok) {
        const uint4 *q = seqs + bk.seqOff;
        for (uint32_t i = threadIdx.x; i < count; i += kCompactT) {
            const uint4 s = q[i]; /* x offset, y litLength, z matchLength */
            lit += s.y;
            cover += (unsigned long long)s.y + s.z;
            /* the packed fields: offset 17 bits, litLength 18, matchLength 17; the last entry is the delimiter */
            if (s.x >= (1u << 17) || s.y > (1u << 17) || s.z >= (1u << 17) || (i + 1u == count && (s.x | s.z) != 0u)) bad++;
        }
    }
    unsigned long long t;
    (void)compact_scan(lit, red, &lit);
    (void)compact_scan(cover, red, &cover);
    (void)compact_scan(bad, red, &t);
    if (threadIdx.x == 0) {
        ok = ok && t == 0 && cover == bk.srcLen;
        hdr[blockIdx.x].count = ok ? count : QZSTD_HIP_NSEQ_ERROR;
        hdr[blockIdx.x].litBytes = ok ? (uint32_t)lit : 0u;
    }
}

/* work: [0, 8n) first entry of each block, [8n, 16n) first literal byte of each block, then {entries, literal bytes} in total */
__global__ __launch_bounds__(kCompactT) void qzstd_compact_scan_kernel(qzstd_hip_compact_hdr_t *__restrict__ hdr, uint32_t n,
                                                                       unsigned long long *__restrict__ work, unsigned long long cap)
{
    __shared__ unsigned long long red[kCompactT / 64u];
    unsigned long long *seqBase = work, *litBase = work + n, *totals = work + 2u * (size_t)n;
    unsigned long long carryAll = 0, carrySeq = 0, carryLit = 0;
    for (uint32_t c = 0; c < n; c += kCompactT) {
        const uint32_t b = c + threadIdx.x;
        qzstd_hip_compact_hdr_t h = { QZSTD_HIP_NSEQ_ERROR, 0u };
        if (b < n) h = hdr[b];
        const unsigned long long cnt = h.count == QZSTD_HIP_NSEQ_ERROR ? 0ull : h.count;
        unsigned long long tAll, tSeq, tLit;
        /* the arena's bytes up to the end of this block (entries and literals both counted): the blocks that do not fit are a suffix */
        const unsigned long long endAll = carryAll + compact_scan(8ull * cnt + h.litBytes, red, &tAll);
        const bool fits = endAll <= cap;
        const unsigned long long keepCnt = fits ? cnt : 0ull, keepLit = fits ? h.litBytes : 0ull;
        const unsigned long long inSeq = compact_scan(keepCnt, red, &tSeq), inLit = compact_scan(keepLit, red, &tLit);
        if (b < n) {
            seqBase[b] = carrySeq + inSeq - keepCnt;
            litBase[b] = carryLit + inLit - keepLit;
            if (!fits && h.count != QZSTD_HIP_NSEQ_ERROR) { h.count = QZSTD_HIP_NSEQ_ERROR; h.litBytes = 0u; hdr[b] = h; }
        }
        carryAll += tAll;
        carrySeq += tSeq;
        carryLit += tLit;
    }
    if (threadIdx.x == 0) { totals[0] = carrySeq; totals[1] = carryLit; }
}

__global__ __launch_bounds__(kCompactT) void qzstd_compact_emit_kernel(const uint8_t *__restrict__ src, const qzstd_hip_block_t *__restrict__ blocks,
                                                                       const uint4 *__restrict__ seqs, const qzstd_hip_compact_hdr_t *__restrict__ hdr,
                                                                       const unsigned long long *__restrict__ work, uint32_t n, uint8_t *__restrict__ arena)
{
    __shared__ unsigned long long red[kCompactT / 64u];
    __shared__ uint32_t dStart[kCompactT + 1u], sStart[kCompactT];
    const qzstd_hip_compact_hdr_t h = hdr[blockIdx.x];
    if (h.count == QZSTD_HIP_NSEQ_ERROR) return;
    const qzstd_hip_block_t bk = blocks[blockIdx.x];
    const unsigned long long seqBase = work[blockIdx.x], litBase = work[n + blockIdx.x], totalSeq = work[2u * (size_t)n];
    const size_t entriesOff = QZSTD_HIP_COMPACT_ENTRIES_OFF(n);
    unsigned long long *outSeq = reinterpret_cast<unsigned long long *>(arena + entriesOff) + seqBase;
    uint8_t *outLit = arena + entriesOff + 8ull * totalSeq + litBase;
    const uint8_t *in = src + bk.srcOff;
    const uint4 *q = seqs + bk.seqOff;
    uint32_t dCarry = 0, sCarry = 0; /* literal bytes and covered bytes of the chunks before */
    for (uint32_t c = 0; c < h.count; c += kCompactT) {
        const uint32_t i = c + threadIdx.x;
        uint4 s = make_uint4(0u, 0u, 0u, 0u);
        if (i < h.count) {
            s = q[i];
            outSeq[i] = QZSTD_HIP_PACK(s.x, s.y, s.z, 0u);
        }
        unsigned long long tLit, tCov;
        const uint32_t dEnd = (uint32_t)compact_scan(s.y, red, &tLit), sEnd = (uint32_t)compact_scan((unsigned long long)s.y + s.z, red, &tCov);
        dStart[threadIdx.x] = dEnd - s.y;
        sStart[threadIdx.x] = sCarry + sEnd - s.y - s.z;
        if (threadIdx.x == 0) dStart[kCompactT] = (uint32_t)tLit;
        __syncthreads();
        /* the chunk's literal bytes [0, tLit): four consecutive bytes per lane, the run found by a binary search over dStart.  Byte stores:
         * the runs start anywhere in the source and the destination.  Measured at level 1 (ms per GiB, the emit kernel): bytes 2.17 - 2.39; aligned
         * dword stores of gathered bytes 2.50; aligned 16-byte stores 4.65 — a chunk's ~1.7 KiB of literals then keeps a quarter of the lanes
         * busy, each with sixteen dependent byte loads.  Wider stores do not make it faster */
        const uint32_t lits = (uint32_t)tLit;
        for (uint32_t j = threadIdx.x * 4u; j < lits; j += kCompactT * 4u) {
            uint32_t lo = 0, hi = kCompactT; /* the last run e with dStart[e] <= j */
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (dStart[mid] <= j) lo = mid; else hi = mid;
            }
            uint32_t e = lo;
            for (uint32_t k = 0; k < 4u && j + k < lits; k++) {
                while (j + k >= dStart[e + 1u]) e++;
                outLit[dCarry + j + k] = in[sStart[e] + (j + k - dStart[e])];
            }
        }
        dCarry += lits;
        sCarry += (uint32_t)tCov;
        __syncthreads(); /* dStart / sStart are rewritten by the next chunk */
    }
}
} // namespace

extern "C" {

size_t qzstd_hip_compact_workspace_bytes(uint32_t nBlocks) { return (size_t)nBlocks * 16u + 16u; }

int qzstd_hip_compact(int device, void *stream, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                      const void *d_seqs, const uint32_t *d_nseq, void *d_arena, size_t arenaBytes, void *d_work, size_t workBytes)
{
    if (nBlocks == 0) return 0;
    if (!d_src || !d_blocks || !d_seqs || !d_nseq || !d_arena || !d_work) return fail_msg("qzstd_hip_compact: null pointer");
    if (workBytes < qzstd_hip_compact_workspace_bytes(nBlocks) || ((uintptr_t)d_work & 7u) || ((uintptr_t)d_arena & 15u))
        return fail_msg("qzstd_hip_compact: workspace too small, or workspace / arena not aligned");
    if (arenaBytes < QZSTD_HIP_COMPACT_ENTRIES_OFF(nBlocks)) return fail_msg("qzstd_hip_compact: arena smaller than its headers");
    QZ_SET_DEVICE(device);
    const hipStream_t s = (hipStream_t)stream;
    auto *hdr = static_cast<qzstd_hip_compact_hdr_t *>(d_arena);
    auto *work = static_cast<unsigned long long *>(d_work);
    const auto *seqs = static_cast<const uint4 *>(d_seqs);
    hipLaunchKernelGGL(qzstd_compact_count_kernel, dim3(nBlocks), dim3(kCompactT), 0, s, d_blocks, seqs, d_nseq, hdr);
    QZ_CHECK(hipGetLastError(), "launch qzstd_compact_count_kernel");
    hipLaunchKernelGGL(qzstd_compact_scan_kernel, dim3(1), dim3(kCompactT), 0, s, hdr, nBlocks, work,
                       (unsigned long long)(arenaBytes - QZSTD_HIP_COMPACT_ENTRIES_OFF(nBlocks)));
    QZ_CHECK(hipGetLastError(), "launch qzstd_compact_scan_kernel");
    hipLaunchKernelGGL(qzstd_compact_emit_kernel, dim3(nBlocks), dim3(kCompactT), 0, s, static_cast<const uint8_t *>(d_src), d_blocks, seqs, hdr,
                       work, nBlocks, static_cast<uint8_t *>(d_arena));
    QZ_CHECK(hipGetLastError(), "launch qzstd_compact_emit_kernel");
    return 0;
}

} /* extern "C" */

/* ---------------------------------------------------------------- gather (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kGatherT = 256u;               /* threads per workgroup */
constexpr uint32_t kGatherWords = 4u * kGatherT;  /* 16-byte words of the stage per workgroup: 16 KiB */

/* the last row of [lo, hi] whose first word is at or before word w (lo when there is none) */
__device__ inline uint32_t gather_row_of(const qzstd_hip_gather_row_t *__restrict__ rows, uint32_t lo, uint32_t hi, uint32_t w)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if ((uint32_t)(rows[mid].dstOff >> 4) <= w) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

/* one workgroup per 16 KiB of the stage between the first row's start and the last row's end; a lane takes every 256th word.  The rows that
 * reach into the workgroup's piece are found once (two searches over all rows), a word's own row by a search among those: no step at all
 * inside a long row, at most ten where 1024 one-word rows share the piece */
__global__ __launch_bounds__(kGatherT) void qzstd_gather_kernel(const qzstd_hip_gather_row_t *__restrict__ rows, uint32_t nRows, uint32_t firstWord,
                                                                uint32_t endWord, uint4 *__restrict__ stage)
{
    __shared__ uint32_t span[2];
    const uint32_t w0 = firstWord + blockIdx.x * kGatherWords;
    const uint32_t wEnd = endWord - w0 < kGatherWords ? endWord : w0 + kGatherWords;
    if (threadIdx.x == 0) {
        span[0] = gather_row_of(rows, 0u, nRows - 1u, w0);
        span[1] = gather_row_of(rows, span[0], nRows - 1u, wEnd - 1u);
    }
    __syncthreads();
    const uint32_t rLo = span[0], rHi = span[1];
    for (uint32_t w = w0 + threadIdx.x; w < wEnd; w += kGatherT) {
        const qzstd_hip_gather_row_t row = rows[gather_row_of(rows, rLo, rHi, w)];
        const uint64_t o = ((uint64_t)w << 4) - row.dstOff; /* the word's first byte in its row (wraps to a huge value in front of row 0) */
        if (o >= (uint64_t)row.len + row.pad) continue;     /* between two rows: not ours to write */
        uint64_t o0 = 0, o1 = 0;
        if (o < row.len) {
            const uint64_t a = row.src + o;
            const uint32_t sh = (uint32_t)a & 15u;
            const uint32_t valid = row.len - o < 16u ? (uint32_t)(row.len - o) : 16u; /* payload bytes of this word */
            const uint4 *p = reinterpret_cast<const uint4 *>(a - sh);
            /* the aligned word that holds byte a, and the next one only when payload of this word lies in it */
            const uint4 l = p[0];
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh + valid > 16u) h = p[1];
            const uint64_t l0 = l.x | (uint64_t)l.y << 32, l1 = l.z | (uint64_t)l.w << 32, h0 = h.x | (uint64_t)h.y << 32, h1 = h.z | (uint64_t)h.w << 32;
            /* {h1 h0 l1 l0} >> 8 * sh: whole 64-bit halves first, then the bytes */
            const bool half = (sh & 8u) != 0u;
            const uint32_t bits = (sh & 7u) * 8u;
            const uint64_t a0 = half ? l1 : l0, a1 = half ? h0 : l1, a2 = half ? h1 : h0;
            o0 = bits ? (a0 >> bits) | (a1 << (64u - bits)) : a0;
            o1 = bits ? (a1 >> bits) | (a2 << (64u - bits)) : a1;
            if (valid < 16u) { /* the row's last word: zero behind the payload (what the shift brought in lies inside the aligned words read) */
                o1 = valid > 8u ? o1 & ((1ull << ((valid - 8u) * 8u)) - 1ull) : 0ull;
                if (valid < 8u) o0 &= (1ull << (valid * 8u)) - 1ull;
            }
        }
        stage[w] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
    }
}
} // namespace

/* ---------------------------------------------------------------- row tables: what their launchers and their kernels share -- */
/* Every launcher below takes a table of rows, checks it, copies it to the device and starts one workgroup per tile of a row; a workgroup
 * finds its row by a search over the table.  There are two ways of numbering the workgroups, and each has ONE check on the host and ONE
 * search on the device, here:
 *   stage numbering  (group, group_xor, group_pieces, group_ediff by dstOff; ungroup, ungroup_xor by srcOff)  workgroup v is tile
 *                    v - start(r) of row r, start(r) = (off >> 14) + r: strictly ascending in r, and a row's tiles (at most
 *                    ceil(extent / 16 KiB)) end before the next row's start, so the launcher needs no prefix sums over the rows.  A
 *                    workgroup whose number falls behind its row's last tile has nothing to do.  stage_rows_check / stage_row_of
 *   tile0 numbering  (ungroup_window, ungroup_cmp, diff, fingerprint, esum, ediff_cost and those from pieces)  the launcher writes every
 *                    row's first workgroup into the row, tile0: rows without a tile share the tile0 of the row behind them and are never
 *                    the one a search finds.  tile0_rows / tile0_row_of
 * A refusal reads "<launcher>: <reason>", returns < 0, queues nothing and writes nothing, the caller's rows included. */
namespace {
constexpr uint32_t kGroupTileLog = 14u; /* bytes of one row per workgroup, under both numberings: 16 KiB, 16 KiB / elem elements */
constexpr uint32_t kGroupTile = 1u << kGroupTileLog;

inline int refuse(const char *who, const char *why)
{
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return fail_msg(msg);
}

/* the rules that hold for every table: each returns nullptr, or the reason it is broken */
inline const char *elem_check(uint32_t elem) { return elem != 1u && elem != 2u && elem != 4u && elem != 8u ? "elem not 1, 2, 4 or 8" : nullptr; }
inline const char *len_check(uint32_t len) { return len > 0xFFFFFFE0u ? "a row longer than 0xFFFFFFE0 bytes" : nullptr; }
/* (one grid dimension, and tile numbers that stay positive as int) */
inline const char *tiles_check(uint64_t tiles) { return tiles > 0x7FFFFFFFull ? "too many tiles" : nullptr; }
/* (the stage's 16-byte words in 32 bits, with room for a workgroup's last step) */
inline const char *stage_span_check(uint64_t end) { return (end >> 4) > 0xFFFFFFFFull - 2u * kGatherWords ? "stage span too large" : nullptr; }

inline uint64_t round16(uint64_t len) { return (len + 15u) & ~(uint64_t)15u; }

/* A row's place in the stage: behind the row before it — `again`: AT the row before it, the next window of the same frame — and its `fit`
 * bytes from `off` on inside stageBytes.  Moves *end behind the row's extent. */
inline const char *stage_place(uint64_t off, uint64_t ext, uint64_t fit, size_t stageBytes, bool again, uint64_t *end)
{
    if (!again && off < *end) return "rows overlap in the stage or are not in ascending order";
    if (off > (uint64_t)stageBytes || fit > (uint64_t)stageBytes - off) return "a row ends past stageBytes";
    *end = off + ext;
    return nullptr;
}

/* the place of a staged frame that a comparison reads */
inline const char *frame_place(uint64_t srcOff, uint32_t len, const void *d_stage, size_t stageBytes, uint64_t *end)
{
    if (srcOff & 15u) return "srcOff not a multiple of 16";
    if (len && !d_stage) return "null stage";
    return stage_place(srcOff, round16(len), len, stageBytes, false, end);
}

/* a row assembled from pieces: its pieces [piece0, piece0 + count) of the table tile [0, len); noBase: a base is refused too */
inline const char *pieces_check(const qzstd_hip_group_piece_t *pieces, uint32_t nPieces, uint32_t piece0, uint32_t count, uint32_t len, bool noBase)
{
    if ((uint64_t)piece0 + count > nPieces) return "a row's pieces end past the table";
    uint64_t at = 0;
    for (uint32_t p = piece0; p < piece0 + count; p++) {
        if (!pieces[p].len || !pieces[p].src) return "an empty piece or a null source";
        if (noBase && pieces[p].base) return "a piece with a base";
        if (pieces[p].off != at) return "a row's pieces do not tile its content in ascending order";
        at += pieces[p].len;
    }
    return at == len ? nullptr : "a row's pieces do not tile its content in ascending order";
}

/* ---- stage numbering, host side */
struct stage_row_t { uint64_t off, ext, fit; uint32_t len, elem; }; /* what the check looks at: stage offset, extent, the bytes that must lie inside
                                                                       stageBytes, content length, element size */
struct row_own_t { const char *early, *mid, *late; };               /* a launcher's own refusals for a row (nullptr: none), at their places in the order */
struct stage_launch_t { uint64_t end, firstTile; uint32_t tiles; }; /* end of the last row; the launch: tiles == 0, nothing to do */

/* Row by row, the first offending row decides: elem, own.early, offset and extent multiples of 16, own.mid, the place (stage_place),
 * own.late; then the stage's span, and for typed rows the launch's tiles.  Typed == false: rows without elem (the plain gather's), no tiles. */
template <bool Typed = true, class Row, class Place, class Own>
int stage_rows_check(const char *who, const Row *rows, uint32_t nRows, size_t stageBytes, Place place, Own own, stage_launch_t *go)
{
    uint64_t end = 0, endTile = 0;
    for (uint32_t i = 0; i < nRows; i++) {
        const stage_row_t p = place(rows[i]);
        const row_own_t mine = own(rows[i]);
        const char *why = Typed ? elem_check(p.elem) : nullptr;
        if (!why) why = mine.early;
        if (!why && ((p.off & 15u) || (p.ext & 15u))) why = "the row's stage offset or its extent (len + pad) not a multiple of 16";
        if (!why) why = mine.mid;
        if (!why) why = stage_place(p.off, p.ext, p.fit, stageBytes, false, &end);
        if (!why) why = mine.late;
        if (why) return refuse(who, why);
        if (Typed && p.ext) { /* the row's tiles in the launch's numbering */
            const uint64_t n = p.len / p.elem, tileMax = kGroupTile / p.elem;
            endTile = (p.off >> kGroupTileLog) + i + (n ? (n + tileMax - 1u) / tileMax : 1u);
        }
    }
    if (const char *why = stage_span_check(end)) return refuse(who, why);
    *go = { end, place(rows[0]).off >> kGroupTileLog, 0u };
    if (endTile == 0) return 0; /* nothing but empty rows */
    if (const char *why = tiles_check(endTile - go->firstTile)) return refuse(who, why);
    go->tiles = (uint32_t)(endTile - go->firstTile);
    return 0;
}

/* the gathers' rows (dstOff; len + pad bytes, all of them inside the stage) and the scatters' (srcOff; len bytes of a 16-byte multiple) */
template <class Row, class Own> int group_rows_check(const char *who, const Row *rows, uint32_t nRows, size_t stageBytes, Own own, stage_launch_t *go)
{
    return stage_rows_check(who, rows, nRows, stageBytes,
                            [](const Row &r) { return stage_row_t{ r.dstOff, (uint64_t)r.len + r.pad, (uint64_t)r.len + r.pad, r.len, r.elem }; }, own, go);
}
template <class Row, class Own> int ungroup_rows_check(const char *who, const Row *rows, uint32_t nRows, size_t stageBytes, Own own, stage_launch_t *go)
{
    return stage_rows_check(who, rows, nRows, stageBytes, [](const Row &r) { return stage_row_t{ r.srcOff, round16(r.len), r.len, r.len, r.elem }; },
                            own, go);
}
const auto kGatherOwn = [](const auto &r) { return row_own_t{ nullptr, r.len && !r.src ? "null source" : nullptr, nullptr }; };
const auto kGroupOwn = [](const auto &r) { return row_own_t{ r.reserved ? "reserved not 0" : nullptr, r.len && !r.src ? "null source" : nullptr, nullptr }; };
const auto kUngroupOwn = [](const auto &r) { return row_own_t{ nullptr, r.len && !r.dst ? "null destination" : nullptr, nullptr }; };

/* ---- tile0 numbering, host side: every row is checked and its tiles are counted, the count is held against the limit, and ONLY THEN is
 * tile0 written.  check(row, i): nullptr or the reason; tiles(row): the row's workgroups. */
template <class Row, class Check, class Tiles>
int tile0_count(const char *who, const Row *rows, uint32_t nRows, Check check, Tiles tiles, uint32_t *total)
{
    uint64_t sum = 0;
    for (uint32_t i = 0; i < nRows; i++) {
        if (const char *why = check(rows[i], i)) return refuse(who, why);
        sum += tiles(rows[i]);
    }
    if (const char *why = tiles_check(sum)) return refuse(who, why);
    *total = (uint32_t)sum;
    return 0;
}

template <class Row, class Tiles> void tile0_write(Row *rows, uint32_t nRows, Tiles tiles)
{
    uint32_t at = 0;
    for (uint32_t i = 0; i < nRows; i++) {
        rows[i].tile0 = at;
        at += (uint32_t)tiles(rows[i]);
    }
}

/* `always`: tile0 is written even when no row has a tile (the caller's rows then say so); else such a table is left as it came */
template <class Row, class Check, class Tiles>
int tile0_rows(const char *who, Row *rows, uint32_t nRows, Check check, Tiles tiles, bool always, uint32_t *total)
{
    if (tile0_count(who, rows, nRows, check, tiles, total)) return -1;
    if (*total || always) tile0_write(rows, nRows, tiles);
    return 0;
}

/* ---- the workgroup's row, device side (one lane runs it; the kernels keep the result in LDS) */
/* stage numbering: the last row whose first tile is at or before v */
template <class Row>
__device__ __forceinline__ uint32_t stage_row_of(const Row *__restrict__ rows, uint32_t nRows, uint64_t Row::*off, uint64_t v)
{
    uint32_t lo = 0, hi = nRows - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if ((rows[mid].*off >> kGroupTileLog) + mid <= v) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

/* tile0 numbering: the last row whose first workgroup is this one or one before it */
template <class Row> __device__ __forceinline__ uint32_t tile0_row_of(const Row *__restrict__ rows, uint32_t nRows)
{
    uint32_t lo = 0, hi = nRows - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (rows[mid].tile0 <= blockIdx.x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}
} // namespace

extern "C" int qzstd_hip_gather(int device, void *stream, const qzstd_hip_gather_row_t *rows, uint32_t nRows, qzstd_hip_gather_row_t *d_rows,
                                void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_gather";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    stage_launch_t go;
    if (stage_rows_check<false>(who, rows, nRows, stageBytes,
                                [](const qzstd_hip_gather_row_t &r) { return stage_row_t{ r.dstOff, (uint64_t)r.len + r.pad, (uint64_t)r.len + r.pad, r.len, 0u }; },
                                kGatherOwn, &go))
        return -1;
    const uint32_t firstWord = (uint32_t)(rows[0].dstOff >> 4), endWord = (uint32_t)(go.end >> 4);
    if (endWord == firstWord) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (gather rows)");
    const uint32_t groups = (endWord - firstWord + kGatherWords - 1u) / kGatherWords;
    hipLaunchKernelGGL(qzstd_gather_kernel, dim3(groups), dim3(kGatherT), 0, (hipStream_t)stream, d_rows, nRows, firstWord, endWord,
                       static_cast<uint4 *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_gather_kernel");
    return 0;
}

/* ---------------------------------------------------------------- byte-grouping gather (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kGroupT = 256u;                    /* threads per workgroup; a workgroup takes kGroupTile source bytes of one row */
constexpr uint32_t kGroupSlack = 32u;                 /* bytes behind each plane in LDS: a stage word's two aligned 16-byte reads stay inside */
constexpr uint32_t kGroupLds = kGroupTile + 8u * kGroupSlack;

/* byte p of the row's grouped layout (0 from len on), by one aligned 16-byte load of the word that holds its source byte */
__device__ inline uint64_t group_byte(const qzstd_hip_group_row_t &row, uint32_t n, uint32_t kLog, uint64_t p)
{
    if (p >= row.len) return 0ull;
    uint64_t s = p;
    if (p < ((uint64_t)n << kLog)) {
        const uint32_t j = (uint32_t)p / n; /* (p < len: 32 bits) */
        s = ((uint64_t)((uint32_t)p - j * n) << kLog) + j;
    }
    const uint64_t a = row.src + s;
    const uint32_t sh = (uint32_t)a & 15u;
    const uint4 v = *reinterpret_cast<const uint4 *>(a - sh);
    const uint32_t d = sh < 8u ? (sh < 4u ? v.x : v.y) : (sh < 12u ? v.z : v.w);
    return (d >> ((sh & 3u) * 8u)) & 0xFFu;
}

/* {h, l} >> 8 * sh, its low 16 bytes: whole 64-bit halves first, then the bytes (the gather's shift) */
__device__ inline void group_shift(const uint4 l, const uint4 h, uint32_t sh, uint64_t *o0, uint64_t *o1)
{
    const uint64_t l0 = l.x | (uint64_t)l.y << 32, l1 = l.z | (uint64_t)l.w << 32, h0 = h.x | (uint64_t)h.y << 32, h1 = h.z | (uint64_t)h.w << 32;
    const bool half = (sh & 8u) != 0u;
    const uint32_t bits = (sh & 7u) * 8u;
    const uint64_t a0 = half ? l1 : l0, a1 = half ? h0 : l1, a2 = half ? h1 : h0;
    *o0 = bits ? (a0 >> bits) | (a1 << (64u - bits)) : a0;
    *o1 = bits ? (a1 >> bits) | (a2 << (64u - bits)) : a1;
}

/* bytes [from, 16) of the stage word at row offset o, fetched one by one: the few bytes of a word that lie outside its owner's tile */
__device__ inline void group_patch(const qzstd_hip_group_row_t &row, uint32_t n, uint32_t kLog, uint64_t o, uint32_t from, uint64_t *o0, uint64_t *o1)
{
    *o1 = from > 8u ? *o1 & ((1ull << ((from - 8u) * 8u)) - 1ull) : 0ull;
    if (from < 8u) *o0 = from ? *o0 & ((1ull << (from * 8u)) - 1ull) : 0ull;
    if (o + from >= row.len) return; /* padding only */
    for (uint32_t i = from; i < 16u; i++) {
        const uint64_t b = group_byte(row, n, kLog, o + i);
        if (i < 8u) *o0 |= b << (i * 8u); else *o1 |= b << ((i - 8u) * 8u);
    }
}

/* the 16 source bytes {o1, o0} = 16 / K elements: byte j of each into plane j of the tile in LDS, at the elements' place (word w of the tile) */
template <uint32_t K> __device__ inline void group_split(uint64_t o0, uint64_t o1, uint8_t *lds, uint32_t w)
{
    constexpr uint32_t per = 16u / K, pitch = kGroupTile / K + kGroupSlack;
    if constexpr (K == 1u) {
        *reinterpret_cast<uint4 *>(lds + w * 16u) = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
            uint64_t v = 0;
#pragma unroll
            for (uint32_t e = 0; e < per; e++) {
                const uint32_t i = e * K + j;
                v |= (((i < 8u ? o0 >> (i * 8u) : o1 >> ((i - 8u) * 8u))) & 0xFFull) << (e * 8u);
            }
            uint8_t *at = lds + j * pitch + w * per;
            if constexpr (per == 8u) *reinterpret_cast<uint64_t *>(at) = v;
            else if constexpr (per == 4u) *reinterpret_cast<uint32_t *>(at) = (uint32_t)v;
            else *reinterpret_cast<uint16_t *>(at) = (uint16_t)v;
        }
    }
}

/* One workgroup per tile: elements [e0, e0 + tileElems) of one row, 16 KiB of its source.
 *   A  every lane takes the tile's source 16 bytes at a time (aligned loads shifted into place, as the gather's), splits them by byte
 *      position and writes the pieces to the tile's planes in LDS: the source crosses the memory system once for all planes
 *   B  per plane, every stage word whose first byte is one of the tile's elements is read back from LDS (two aligned 16-byte reads shifted
 *      by the plane's offset in its stage word), completed with single bytes where it reaches past the tile, and stored
 *   and the row's last tile writes the words that start in the tail or the padding. */
__global__ __launch_bounds__(kGroupT) void qzstd_group_kernel(const qzstd_hip_group_row_t *__restrict__ rows, uint32_t nRows, uint64_t firstTile,
                                                               uint4 *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kGroupLds];
    __shared__ uint32_t which;
    const uint64_t v = firstTile + blockIdx.x;
    if (threadIdx.x == 0) which = stage_row_of(rows, nRows, &qzstd_hip_group_row_t::dstOff, v);
    __syncthreads();
    const uint32_t r = which;
    const qzstd_hip_group_row_t row = rows[r];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kGroupTile >> kLog;
    const uint64_t ext = (uint64_t)row.len + row.pad;
    const uint64_t tiles = n ? ((uint64_t)n + tileMax - 1u) / tileMax : (ext ? 1ull : 0ull);
    const uint64_t t = v - ((row.dstOff >> kGroupTileLog) + r);
    if (t >= tiles) return; /* (the whole workgroup) */
    const uint32_t e0 = (uint32_t)t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint32_t tileBytes = tileElems << kLog;
    const uint64_t srcTile = row.src + ((uint64_t)e0 << kLog);

    for (uint32_t w = threadIdx.x; w * 16u < tileBytes; w += kGroupT) {
        const uint64_t a = srcTile + w * 16u;
        const uint32_t sh = (uint32_t)a & 15u;
        const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
        const uint4 *p = reinterpret_cast<const uint4 *>(a - sh);
        /* the aligned word that holds byte a, and the next one only when bytes of the tile lie in it */
        const uint4 l = p[0];
        uint4 h = make_uint4(0u, 0u, 0u, 0u);
        if (sh + valid > 16u) h = p[1];
        uint64_t o0, o1;
        group_shift(l, h, sh, &o0, &o1);
        switch (kLog) {
        case 0u: group_split<1u>(o0, o1, lds, w); break;
        case 1u: group_split<2u>(o0, o1, lds, w); break;
        case 2u: group_split<4u>(o0, o1, lds, w); break;
        default: group_split<8u>(o0, o1, lds, w); break;
        }
    }
    __syncthreads();

    uint4 *out = stage + (row.dstOff >> 4);
    for (uint32_t j = 0; j < (1u << kLog); j++) {
        const uint64_t planeAt = (uint64_t)j * n + e0; /* row offset of the tile's first element in plane j */
        const uint32_t aj = (uint32_t)planeAt & 15u;
        const uint8_t *base = lds + j * (tileMax + kGroupSlack);
        /* c: offset from the stage word that holds planeAt; that word itself belongs here only when it starts at planeAt */
        for (uint32_t c = (aj ? 16u : 0u) + threadIdx.x * 16u; c < aj + tileElems; c += kGroupT * 16u) {
            const uint32_t x0 = c - aj, q = x0 & ~15u, sh = x0 & 15u;
            const uint32_t valid = tileElems - x0 < 16u ? tileElems - x0 : 16u;
            const uint64_t o = planeAt + x0;
            const uint4 l = *reinterpret_cast<const uint4 *>(base + q);
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh) h = *reinterpret_cast<const uint4 *>(base + q + 16u);
            uint64_t o0, o1;
            group_shift(l, h, sh, &o0, &o1);
            if (valid < 16u) group_patch(row, n, kLog, o, valid, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
    if (t + 1u == tiles) {
        const uint64_t tailAt = ((((uint64_t)n << kLog) + 15u) & ~(uint64_t)15u);
        for (uint64_t o = tailAt + threadIdx.x * 16u; o < ext; o += kGroupT * 16u) {
            uint64_t o0 = 0, o1 = 0;
            group_patch(row, n, kLog, o, 0u, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
}

/* ---- the same with a base XORed in (qzstd_hip_group_xor).  A kernel of its own: written as one template with qzstd_group_kernel, that
 * kernel's register allocation and instruction mix changed (profiles/device_delta_kernels.txt), and it is to stay what it was.  group_shift
 * and group_split are shared; what looks at a row is written again for a row with a base. */

/* the byte at address a, by one aligned 16-byte load of the word that holds it */
__device__ inline uint64_t group_byte_at(uint64_t a)
{
    const uint32_t sh = (uint32_t)a & 15u;
    const uint4 v = *reinterpret_cast<const uint4 *>(a - sh);
    const uint32_t d = sh < 8u ? (sh < 4u ? v.x : v.y) : (sh < 12u ? v.z : v.w);
    return (d >> ((sh & 3u) * 8u)) & 0xFFu;
}

/* group_byte for a row with a base: the source byte and, when the row has one, the base byte of the same row offset, each by one aligned
 * 16-byte load, XORed */
__device__ inline uint64_t group_xor_byte(const qzstd_hip_group_xor_row_t &row, uint32_t n, uint32_t kLog, uint64_t p)
{
    if (p >= row.len) return 0ull;
    uint64_t s = p;
    if (p < ((uint64_t)n << kLog)) {
        const uint32_t j = (uint32_t)p / n; /* (p < len: 32 bits) */
        s = ((uint64_t)((uint32_t)p - j * n) << kLog) + j;
    }
    const uint64_t b = group_byte_at(row.src + s);
    return row.base ? b ^ group_byte_at(row.base + s) : b;
}

/* group_patch over group_xor_byte */
__device__ inline void group_xor_patch(const qzstd_hip_group_xor_row_t &row, uint32_t n, uint32_t kLog, uint64_t o, uint32_t from, uint64_t *o0,
                                       uint64_t *o1)
{
    *o1 = from > 8u ? *o1 & ((1ull << ((from - 8u) * 8u)) - 1ull) : 0ull;
    if (from < 8u) *o0 = from ? *o0 & ((1ull << (from * 8u)) - 1ull) : 0ull;
    if (o + from >= row.len) return; /* padding only */
    for (uint32_t i = from; i < 16u; i++) {
        const uint64_t b = group_xor_byte(row, n, kLog, o + i);
        if (i < 8u) *o0 |= b << (i * 8u); else *o1 |= b << ((i - 8u) * 8u);
    }
}

/* the 16 bytes from address a on, of which the first `valid` are wanted: the aligned word that holds byte a, and the next one only when
 * wanted bytes lie in it, shifted into place */
__device__ inline void group_fetch(uint64_t a, uint32_t valid, uint64_t *o0, uint64_t *o1)
{
    const uint32_t sh = (uint32_t)a & 15u;
    const uint4 *p = reinterpret_cast<const uint4 *>(a - sh);
    const uint4 l = p[0];
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    if (sh + valid > 16u) h = p[1];
    group_shift(l, h, sh, o0, o1);
}

/* qzstd_group_kernel's tiles and phases.  In A the base's 16 bytes are fetched like the source's — aligned loads of the words that overlap
 * [base, base + len) only, shifted by the base's OWN misalignment — and XORed in before the split: B sees a tile of src ^ base. */
__global__ __launch_bounds__(kGroupT) void qzstd_group_xor_kernel(const qzstd_hip_group_xor_row_t *__restrict__ rows, uint32_t nRows,
                                                                   uint64_t firstTile, uint4 *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kGroupLds];
    __shared__ uint32_t which;
    const uint64_t v = firstTile + blockIdx.x;
    if (threadIdx.x == 0) which = stage_row_of(rows, nRows, &qzstd_hip_group_xor_row_t::dstOff, v);
    __syncthreads();
    const uint32_t r = which;
    const qzstd_hip_group_xor_row_t row = rows[r];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kGroupTile >> kLog;
    const uint64_t ext = (uint64_t)row.len + row.pad;
    const uint64_t tiles = n ? ((uint64_t)n + tileMax - 1u) / tileMax : (ext ? 1ull : 0ull);
    const uint64_t t = v - ((row.dstOff >> kGroupTileLog) + r);
    if (t >= tiles) return; /* (the whole workgroup) */
    const uint32_t e0 = (uint32_t)t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint32_t tileBytes = tileElems << kLog;
    const uint64_t srcTile = row.src + ((uint64_t)e0 << kLog), baseTile = row.base + ((uint64_t)e0 << kLog);

    for (uint32_t w = threadIdx.x; w * 16u < tileBytes; w += kGroupT) {
        const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
        uint64_t o0, o1;
        group_fetch(srcTile + w * 16u, valid, &o0, &o1);
        if (row.base) {
            uint64_t b0, b1;
            group_fetch(baseTile + w * 16u, valid, &b0, &b1);
            o0 ^= b0;
            o1 ^= b1;
        }
        switch (kLog) {
        case 0u: group_split<1u>(o0, o1, lds, w); break;
        case 1u: group_split<2u>(o0, o1, lds, w); break;
        case 2u: group_split<4u>(o0, o1, lds, w); break;
        default: group_split<8u>(o0, o1, lds, w); break;
        }
    }
    __syncthreads();

    uint4 *out = stage + (row.dstOff >> 4);
    for (uint32_t j = 0; j < (1u << kLog); j++) {
        const uint64_t planeAt = (uint64_t)j * n + e0; /* row offset of the tile's first element in plane j */
        const uint32_t aj = (uint32_t)planeAt & 15u;
        const uint8_t *plane = lds + j * (tileMax + kGroupSlack);
        /* c: offset from the stage word that holds planeAt; that word itself belongs here only when it starts at planeAt */
        for (uint32_t c = (aj ? 16u : 0u) + threadIdx.x * 16u; c < aj + tileElems; c += kGroupT * 16u) {
            const uint32_t x0 = c - aj, q = x0 & ~15u, sh = x0 & 15u;
            const uint32_t valid = tileElems - x0 < 16u ? tileElems - x0 : 16u;
            const uint64_t o = planeAt + x0;
            const uint4 l = *reinterpret_cast<const uint4 *>(plane + q);
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh) h = *reinterpret_cast<const uint4 *>(plane + q + 16u);
            uint64_t o0, o1;
            group_shift(l, h, sh, &o0, &o1);
            if (valid < 16u) group_xor_patch(row, n, kLog, o, valid, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
    if (t + 1u == tiles) {
        const uint64_t tailAt = ((((uint64_t)n << kLog) + 15u) & ~(uint64_t)15u);
        for (uint64_t o = tailAt + threadIdx.x * 16u; o < ext; o += kGroupT * 16u) {
            uint64_t o0 = 0, o1 = 0;
            group_xor_patch(row, n, kLog, o, 0u, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
}
} // namespace

extern "C" int qzstd_hip_group(int device, void *stream, const qzstd_hip_group_row_t *rows, uint32_t nRows, qzstd_hip_group_row_t *d_rows,
                               void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_group";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    stage_launch_t go;
    if (group_rows_check(who, rows, nRows, stageBytes, kGroupOwn, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (group rows)");
    hipLaunchKernelGGL(qzstd_group_kernel, dim3(go.tiles), dim3(kGroupT), 0, (hipStream_t)stream, d_rows, nRows, go.firstTile,
                       static_cast<uint4 *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_group_kernel");
    return 0;
}

/* (a row's base may be anything, 0 included) */
extern "C" int qzstd_hip_group_xor(int device, void *stream, const qzstd_hip_group_xor_row_t *rows, uint32_t nRows,
                                   qzstd_hip_group_xor_row_t *d_rows, void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_group_xor";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    stage_launch_t go;
    if (group_rows_check(who, rows, nRows, stageBytes, kGroupOwn, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (group xor rows)");
    hipLaunchKernelGGL(qzstd_group_xor_kernel, dim3(go.tiles), dim3(kGroupT), 0, (hipStream_t)stream, d_rows, nRows, go.firstTile,
                       static_cast<uint4 *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_group_xor_kernel");
    return 0;
}

/* ---- the same for rows whose content is assembled from pieces (qzstd_hip_group_pieces).  A kernel of its own, as qzstd_group_xor_kernel is:
 * the two above stay what they were.  group_shift, group_split, group_fetch and group_byte_at are shared; what is new is the way from a
 * content offset to a piece and an address.  The piece table is not cached in LDS: a tile of one-byte pieces has 16384 of them (384 KiB),
 * so a cache could only hold a prefix and would need a second path behind it; instead the workgroup narrows the table to the tile's pieces
 * once, and a lane's search runs over that range — no step at all for a tile inside one piece, one or two for 8 KiB pieces, and the
 * entries it touches are the same few lines for the whole wave. */
namespace {
/* the last piece of [lo, hi] whose off is at or before c (pieces ascend and tile the row: pieces[lo].off <= c) */
__device__ inline uint32_t pieces_find(const qzstd_hip_group_piece_t *__restrict__ pieces, uint32_t lo, uint32_t hi, uint32_t c)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (pieces[mid].off <= c) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

/* bytes [0, m) of {t1, t0} to bytes [at, at + m) of {o1, o0}; at + m <= 16, m >= 1; what lies behind byte m of t is dropped */
__device__ inline void pieces_place(uint64_t t0, uint64_t t1, uint32_t m, uint32_t at, uint64_t *o0, uint64_t *o1)
{
    if (m < 8u) { t0 &= (1ull << (m * 8u)) - 1ull; t1 = 0ull; }
    else if (m < 16u) t1 = m > 8u ? t1 & ((1ull << ((m - 8u) * 8u)) - 1ull) : 0ull;
    const uint32_t bits = (at & 7u) * 8u;
    if (at & 8u) { *o1 |= t0 << bits; }
    else {
        *o0 |= t0 << bits;
        *o1 |= bits ? (t1 << bits) | (t0 >> (64u - bits)) : t1;
    }
}

/* the `valid` content bytes from content offset c on (src ^ base), p the piece that holds c: one group_fetch per side when they lie inside
 * p, else piece by piece — every sub-fetch asks for exactly the bytes of ITS piece, so group_fetch loads only words that overlap that
 * piece's [src, src + len) and [base, base + len) */
__device__ inline void pieces_fetch(const qzstd_hip_group_piece_t *__restrict__ pieces, uint32_t p, uint32_t c, uint32_t valid, uint64_t *o0,
                                    uint64_t *o1)
{
    qzstd_hip_group_piece_t pc = pieces[p];
    uint32_t in = c - pc.off;
    if (valid <= pc.len - in) {
        group_fetch(pc.src + in, valid, o0, o1);
        if (pc.base) {
            uint64_t b0, b1;
            group_fetch(pc.base + in, valid, &b0, &b1);
            *o0 ^= b0;
            *o1 ^= b1;
        }
        return;
    }
    *o0 = 0ull;
    *o1 = 0ull;
    for (uint32_t at = 0;;) {
        const uint32_t m = valid - at < pc.len - in ? valid - at : pc.len - in;
        uint64_t t0, t1;
        group_fetch(pc.src + in, m, &t0, &t1);
        if (pc.base) {
            uint64_t b0, b1;
            group_fetch(pc.base + in, m, &b0, &b1);
            t0 ^= b0;
            t1 ^= b1;
        }
        pieces_place(t0, t1, m, at, o0, o1);
        at += m;
        if (at >= valid) break;
        pc = pieces[++p]; /* (the pieces tile the row: the next one begins where this one ends) */
        in = 0u;
    }
}

/* group_xor_byte through the lookup: byte p of the row's grouped layout (0 from len on); the search runs over all of the row's pieces,
 * for the byte may lie in another tile */
__device__ inline uint64_t pieces_byte(const qzstd_hip_group_pieces_row_t &row, const qzstd_hip_group_piece_t *__restrict__ pieces, uint32_t n,
                                       uint32_t kLog, uint64_t p)
{
    if (p >= row.len) return 0ull;
    uint32_t s = (uint32_t)p; /* (p < len: 32 bits) */
    if (p < ((uint64_t)n << kLog)) {
        const uint32_t j = (uint32_t)p / n;
        s = (((uint32_t)p - j * n) << kLog) + j;
    }
    const qzstd_hip_group_piece_t pc = pieces[pieces_find(pieces, row.piece0, row.piece0 + row.nPieces - 1u, s)];
    const uint64_t b = group_byte_at(pc.src + (s - pc.off));
    return pc.base ? b ^ group_byte_at(pc.base + (s - pc.off)) : b;
}

/* group_patch over pieces_byte */
__device__ inline void pieces_patch(const qzstd_hip_group_pieces_row_t &row, const qzstd_hip_group_piece_t *__restrict__ pieces, uint32_t n,
                                    uint32_t kLog, uint64_t o, uint32_t from, uint64_t *o0, uint64_t *o1)
{
    *o1 = from > 8u ? *o1 & ((1ull << ((from - 8u) * 8u)) - 1ull) : 0ull;
    if (from < 8u) *o0 = from ? *o0 & ((1ull << (from * 8u)) - 1ull) : 0ull;
    if (o + from >= row.len) return; /* padding only */
    for (uint32_t i = from; i < 16u; i++) {
        const uint64_t b = pieces_byte(row, pieces, n, kLog, o + i);
        if (i < 8u) *o0 |= b << (i * 8u); else *o1 |= b << ((i - 8u) * 8u);
    }
}

/* qzstd_group_xor_kernel's tiles and phases.  Before A, one lane finds the pieces that hold the tile's first and last content byte; in A a
 * lane finds the piece of its first byte among them and fetches through pieces_fetch: B sees a tile of the assembled src ^ base. */
__global__ __launch_bounds__(kGroupT) void qzstd_group_pieces_kernel(const qzstd_hip_group_pieces_row_t *__restrict__ rows, uint32_t nRows,
                                                                      const qzstd_hip_group_piece_t *__restrict__ pieces, uint64_t firstTile,
                                                                      uint4 *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kGroupLds];
    __shared__ uint32_t which, pieceLo, pieceHi;
    const uint64_t v = firstTile + blockIdx.x;
    if (threadIdx.x == 0) {
        const uint32_t lo = stage_row_of(rows, nRows, &qzstd_hip_group_pieces_row_t::dstOff, v);
        which = lo;
        const qzstd_hip_group_pieces_row_t &rw = rows[lo];
        const uint64_t t = v - ((rw.dstOff >> kGroupTileLog) + lo);
        const uint32_t whole = rw.len & ~(rw.elem - 1u); /* the content bytes that are elements: tiles cover [0, whole) */
        pieceLo = pieceHi = rw.piece0;
        if ((t << kGroupTileLog) < whole) {
            const uint32_t c0 = (uint32_t)t << kGroupTileLog, c1 = whole - c0 < kGroupTile ? whole - 1u : c0 + kGroupTile - 1u;
            pieceLo = pieces_find(pieces, rw.piece0, rw.piece0 + rw.nPieces - 1u, c0);
            pieceHi = pieces_find(pieces, pieceLo, rw.piece0 + rw.nPieces - 1u, c1);
        }
    }
    __syncthreads();
    const uint32_t r = which;
    const qzstd_hip_group_pieces_row_t row = rows[r];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kGroupTile >> kLog;
    const uint64_t ext = (uint64_t)row.len + row.pad;
    const uint64_t tiles = n ? ((uint64_t)n + tileMax - 1u) / tileMax : (ext ? 1ull : 0ull);
    const uint64_t t = v - ((row.dstOff >> kGroupTileLog) + r);
    if (t >= tiles) return; /* (the whole workgroup) */
    const uint32_t e0 = (uint32_t)t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint32_t tileBytes = tileElems << kLog;
    const uint32_t cTile = e0 << kLog; /* the tile's first content byte */
    const uint32_t pLo = pieceLo, pHi = pieceHi;

    for (uint32_t w = threadIdx.x; w * 16u < tileBytes; w += kGroupT) {
        const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
        const uint32_t c = cTile + w * 16u;
        uint64_t o0, o1;
        pieces_fetch(pieces, pLo == pHi ? pLo : pieces_find(pieces, pLo, pHi, c), c, valid, &o0, &o1);
        switch (kLog) {
        case 0u: group_split<1u>(o0, o1, lds, w); break;
        case 1u: group_split<2u>(o0, o1, lds, w); break;
        case 2u: group_split<4u>(o0, o1, lds, w); break;
        default: group_split<8u>(o0, o1, lds, w); break;
        }
    }
    __syncthreads();

    uint4 *out = stage + (row.dstOff >> 4);
    for (uint32_t j = 0; j < (1u << kLog); j++) {
        const uint64_t planeAt = (uint64_t)j * n + e0; /* row offset of the tile's first element in plane j */
        const uint32_t aj = (uint32_t)planeAt & 15u;
        const uint8_t *plane = lds + j * (tileMax + kGroupSlack);
        /* c: offset from the stage word that holds planeAt; that word itself belongs here only when it starts at planeAt */
        for (uint32_t c = (aj ? 16u : 0u) + threadIdx.x * 16u; c < aj + tileElems; c += kGroupT * 16u) {
            const uint32_t x0 = c - aj, q = x0 & ~15u, sh = x0 & 15u;
            const uint32_t valid = tileElems - x0 < 16u ? tileElems - x0 : 16u;
            const uint64_t o = planeAt + x0;
            const uint4 l = *reinterpret_cast<const uint4 *>(plane + q);
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh) h = *reinterpret_cast<const uint4 *>(plane + q + 16u);
            uint64_t o0, o1;
            group_shift(l, h, sh, &o0, &o1);
            if (valid < 16u) pieces_patch(row, pieces, n, kLog, o, valid, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
    if (t + 1u == tiles) {
        const uint64_t tailAt = ((((uint64_t)n << kLog) + 15u) & ~(uint64_t)15u);
        for (uint64_t o = tailAt + threadIdx.x * 16u; o < ext; o += kGroupT * 16u) {
            uint64_t o0 = 0, o1 = 0;
            pieces_patch(row, pieces, n, kLog, o, 0u, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
}
} // namespace

/* (the content has no address of its own: in the place of the null source test, every row's pieces tile its content) */
extern "C" int qzstd_hip_group_pieces(int device, void *stream, const qzstd_hip_group_pieces_row_t *rows, uint32_t nRows,
                                      qzstd_hip_group_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                      qzstd_hip_group_piece_t *d_pieces, void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_group_pieces";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    if (nPieces && (!pieces || !d_pieces)) return refuse(who, "null piece table");
    const auto own = [&](const qzstd_hip_group_pieces_row_t &r) {
        return row_own_t{ r.reserved ? "reserved not 0" : nullptr, nullptr, pieces_check(pieces, nPieces, r.piece0, r.nPieces, r.len, false) };
    };
    stage_launch_t go;
    if (group_rows_check(who, rows, nRows, stageBytes, own, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (group pieces rows)");
    if (nPieces)
        QZ_CHECK(hipMemcpyAsync(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces), hipMemcpyHostToDevice, (hipStream_t)stream),
                 "hipMemcpyAsync H2D (group pieces table)");
    hipLaunchKernelGGL(qzstd_group_pieces_kernel, dim3(go.tiles), dim3(kGroupT), 0, (hipStream_t)stream, d_rows, nRows, d_pieces, go.firstTile,
                       static_cast<uint4 *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_group_pieces_kernel");
    return 0;
}

/* ---------------------------------------------------------------- ungrouping scatter (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kUngroupT = 256u;                 /* threads per workgroup */
constexpr uint32_t kUngroupTileLog = kGroupTileLog;  /* destination bytes of one row per workgroup: 16 KiB, 16 KiB / elem elements */
constexpr uint32_t kUngroupTile = 1u << kUngroupTileLog;
constexpr uint32_t kUngroupSlack = 48u;              /* bytes behind each plane strip in LDS: the strip's one extra stage word (a strip starts anywhere
                                                        in its first word) and the aligned reads of a destination word's last elements */
constexpr uint32_t kUngroupLds = kUngroupTile + 8u * kUngroupSlack;

/* byte p (< len) of the row as the destination holds it, by one aligned 16-byte load of the stage word that holds it in the grouped layout:
 * the bytes a destination word needs from outside its owner's tile, and the bytes in front of and behind a row's whole words */
__device__ inline uint32_t ungroup_byte(const uint8_t *__restrict__ stageRow, uint32_t n, uint32_t kLog, uint32_t p)
{
    uint64_t s = p;
    if (p < ((uint64_t)n << kLog)) s = (uint64_t)(p & ((1u << kLog) - 1u)) * n + (p >> kLog);
    const uint32_t sh = (uint32_t)s & 15u;
    const uint4 v = *reinterpret_cast<const uint4 *>(stageRow + (s - sh));
    const uint32_t d = sh < 8u ? (sh < 4u ? v.x : v.y) : (sh < 12u ? v.z : v.w);
    return (d >> ((sh & 3u) * 8u)) & 0xFFu;
}

/* 16 / K bytes of a plane strip in LDS from byte `at` on (any alignment), in the low bytes of the result: aligned reads, shifted.  K = 8: the
 * two bytes wanted and two more that nobody looks at */
template <uint32_t K> __device__ inline uint64_t ungroup_strip(const uint8_t *strip, uint32_t at)
{
    if constexpr (K == 2u) {
        const uint32_t q = at & ~7u, bits = (at & 7u) * 8u;
        const uint64_t lo = *reinterpret_cast<const uint64_t *>(strip + q), hi = *reinterpret_cast<const uint64_t *>(strip + q + 8u);
        return bits ? (lo >> bits) | (hi << (64u - bits)) : lo;
    } else {
        const uint32_t q = at & ~3u;
        const uint64_t both = *reinterpret_cast<const uint32_t *>(strip + q) | (uint64_t)*reinterpret_cast<const uint32_t *>(strip + q + 4u) << 32;
        return (uint32_t)(both >> ((at & 3u) * 8u));
    }
}

/* The 16 destination bytes at row offset o (any phase inside an element), from the tile's plane strips in LDS.  Byte i of the word is byte
 * (ph + i) % K of element o / K + (ph + i) / K, ph = o % K: plane j = (jj + ph) % K gives the word's bytes jj, jj + K, jj + 2 K, ..., which lie
 * side by side in its strip from element o / K (+ 1 for the planes below ph) on.  Every plane is read once, 16 / K bytes wide, and the bytes are
 * interleaved by v_perm_b32 (byte selects 0-3: the second operand, 4-7: the first), not one by one.  Plane j's strip lies at strip 0 +
 * j * pitch and starts (j * n + e0) & 15 bytes into its first word, as it does in the stage. */
template <uint32_t K> __device__ inline uint4 ungroup_word(const uint8_t *lds, uint32_t n, uint32_t e0, uint32_t o)
{
    constexpr uint32_t pitch = kUngroupTile / K + kUngroupSlack;
    const uint32_t ph = o & (K - 1u), e = o / K - e0;
    uint64_t q[K];
#pragma unroll
    for (uint32_t jj = 0; jj < K; jj++) {
        const uint32_t j = (jj + ph) & (K - 1u);
        const uint32_t at = (uint32_t)(((uint64_t)j * n + e0) & 15u) + e + (j < ph ? 1u : 0u);
        q[jj] = ungroup_strip<K>(lds + j * pitch, at);
    }
    constexpr uint32_t lo01 = 0x05010400u, hi01 = 0x07030602u; /* {b0 a0 b1 a1}, {b2 a2 b3 a3} of perm(a, b) */
    constexpr uint32_t lo16 = 0x05040100u, hi16 = 0x07060302u; /* {b0 b1 a0 a1}, {b2 b3 a2 a3} */
    if constexpr (K == 2u) {
        const uint32_t a0 = (uint32_t)q[0], a1 = (uint32_t)(q[0] >> 32), b0 = (uint32_t)q[1], b1 = (uint32_t)(q[1] >> 32);
        return make_uint4(__builtin_amdgcn_perm(b0, a0, lo01), __builtin_amdgcn_perm(b0, a0, hi01), __builtin_amdgcn_perm(b1, a1, lo01),
                          __builtin_amdgcn_perm(b1, a1, hi01));
    } else if constexpr (K == 4u) {
        const uint32_t t0 = __builtin_amdgcn_perm((uint32_t)q[1], (uint32_t)q[0], lo01), t1 = __builtin_amdgcn_perm((uint32_t)q[1], (uint32_t)q[0], hi01);
        const uint32_t u0 = __builtin_amdgcn_perm((uint32_t)q[3], (uint32_t)q[2], lo01), u1 = __builtin_amdgcn_perm((uint32_t)q[3], (uint32_t)q[2], hi01);
        return make_uint4(__builtin_amdgcn_perm(u0, t0, lo16), __builtin_amdgcn_perm(u0, t0, hi16), __builtin_amdgcn_perm(u1, t1, lo16),
                          __builtin_amdgcn_perm(u1, t1, hi16));
    } else {
        const uint32_t a01 = __builtin_amdgcn_perm((uint32_t)q[1], (uint32_t)q[0], lo01), a23 = __builtin_amdgcn_perm((uint32_t)q[3], (uint32_t)q[2], lo01);
        const uint32_t a45 = __builtin_amdgcn_perm((uint32_t)q[5], (uint32_t)q[4], lo01), a67 = __builtin_amdgcn_perm((uint32_t)q[7], (uint32_t)q[6], lo01);
        return make_uint4(__builtin_amdgcn_perm(a23, a01, lo16), __builtin_amdgcn_perm(a67, a45, lo16), __builtin_amdgcn_perm(a23, a01, hi16),
                          __builtin_amdgcn_perm(a67, a45, hi16));
    }
}

/* K = 1: the strip is the row; two aligned 16-byte reads shifted, as the group kernel's */
template <> __device__ inline uint4 ungroup_word<1u>(const uint8_t *lds, uint32_t n, uint32_t e0, uint32_t o)
{
    const uint32_t at = (e0 & 15u) + (o - e0), q = at & ~15u, sh = at & 15u;
    const uint4 l = *reinterpret_cast<const uint4 *>(lds + q);
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    if (sh) h = *reinterpret_cast<const uint4 *>(lds + q + 16u);
    uint64_t o0, o1;
    group_shift(l, h, sh, &o0, &o1);
    (void)n;
    return make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
}

/* A: the tile's K plane strips, stage words (aligned 16-byte loads) to LDS as they lie in the stage; B, behind the barrier: the tile's
 * destination words, assembled and stored.  One function of the thread's index for both, so that the kernel's body reads as its two phases. */
__device__ inline void ungroup_load(const uint8_t *__restrict__ stageRow, uint32_t n, uint32_t kLog, uint32_t e0, uint32_t tileElems, uint8_t *lds,
                                    uint32_t tid)
{
    const uint32_t stripLog = kUngroupTileLog - 4u - kLog, stripWords = 1u << stripLog; /* a strip without its extra word */
    const uint32_t pitch = (kUngroupTile >> kLog) + kUngroupSlack;
    if (!tileElems) return;
#pragma unroll
    for (uint32_t u = 0; u < kUngroupTile / 16u / kUngroupT; u++) {
        const uint32_t idx = tid + u * kUngroupT, j = idx >> stripLog, i = idx & (stripWords - 1u);
        const uint64_t s0 = (uint64_t)j * n + e0;
        if (i < (((uint32_t)s0 & 15u) + tileElems + 15u) >> 4)
            *reinterpret_cast<uint4 *>(lds + j * pitch + i * 16u) = *reinterpret_cast<const uint4 *>(stageRow + ((s0 >> 4) + i) * 16u);
    }
    if (tid < (1u << kLog)) { /* the extra word of a full strip that does not start on a word */
        const uint64_t s0 = (uint64_t)tid * n + e0;
        if ((((uint32_t)s0 & 15u) + tileElems + 15u) >> 4 > stripWords)
            *reinterpret_cast<uint4 *>(lds + tid * pitch + stripWords * 16u) = *reinterpret_cast<const uint4 *>(stageRow + ((s0 >> 4) + stripWords) * 16u);
    }
}

/* qzstd_hip_ungroup_xor's rows carry a base address (0: none); the store phase and the kernel's body are written once for both row types
 * (the instantiation without a base compiles to the kernel it was: profiles/device_delta_kernels.txt) */
template <class Row> inline constexpr bool kRowHasBase = false;
template <> inline constexpr bool kRowHasBase<qzstd_hip_ungroup_xor_row_t> = true;

/* A row with a base (the XOR variant's rows): every byte leaves XORed with the base's byte of the same row offset.  The base bytes of a
 * destination word are fetched by the lane that stores the word — one aligned 16-byte load when base and dst agree mod 16, else two and a
 * shift; the word lies inside the row, so both loads overlap [base, base + len) — and those of a head or tail byte singly, by the lane
 * that stores the byte: with base == dst every byte is read by its only writer, before it writes. */
template <class Row>
__device__ inline void ungroup_store(const Row &row, const uint8_t *__restrict__ stageRow, uint32_t n, uint32_t kLog, uint32_t e0,
                                     uint32_t tileElems, bool first, bool last, const uint8_t *lds, uint32_t tid)
{
    uint8_t *dst = reinterpret_cast<uint8_t *>(row.dst);
    /* the row's whole destination words: `words` of them from row offset `head` on; in front of them and behind them single bytes */
    const uint32_t lead = (uint32_t)(0u - row.dst) & 15u, head = lead < row.len ? lead : row.len;
    const uint32_t words = (row.len - head) >> 4;
    const uint64_t t0 = (uint64_t)e0 << kLog, lim = (uint64_t)(e0 + tileElems) << kLog; /* the tile's bytes of the row: what its strips hold */
    const uint64_t t1 = last ? row.len : lim; /* a word belongs to the tile of its FIRST byte; the tail behind the elements to the last tile */
    for (uint64_t i = (t0 <= head ? 0u : (t0 - head + 15u) >> 4) + tid; i < words && head + i * 16u < t1; i += kUngroupT) {
        const uint32_t o = head + (uint32_t)i * 16u;
        uint4 v;
        switch (kLog) {
        case 0u: v = ungroup_word<1u>(lds, n, e0, o); break;
        case 1u: v = ungroup_word<2u>(lds, n, e0, o); break;
        case 2u: v = ungroup_word<4u>(lds, n, e0, o); break;
        default: v = ungroup_word<8u>(lds, n, e0, o); break;
        }
        if (lim - o < 16u) { /* the word reaches into the next tile or the tail: those bytes one by one, from the stage */
            uint32_t d[4] = { v.x, v.y, v.z, v.w };
            for (uint32_t b = (uint32_t)(lim - o); b < 16u; b++)
                d[b >> 2] = (d[b >> 2] & ~(0xFFu << ((b & 3u) * 8u))) | ungroup_byte(stageRow, n, kLog, o + b) << ((b & 3u) * 8u);
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        if constexpr (kRowHasBase<Row>) {
            if (row.base) {
                const uint64_t b = row.base + o;
                const uint32_t bsh = (uint32_t)b & 15u;
                const uint4 *bp = reinterpret_cast<const uint4 *>(b - bsh);
                const uint4 bl = bp[0];
                uint4 bh = make_uint4(0u, 0u, 0u, 0u);
                if (bsh) bh = bp[1];
                uint64_t b0, b1;
                group_shift(bl, bh, bsh, &b0, &b1);
                v = make_uint4(v.x ^ (uint32_t)b0, v.y ^ (uint32_t)(b0 >> 32), v.z ^ (uint32_t)b1, v.w ^ (uint32_t)(b1 >> 32));
            }
        }
        *reinterpret_cast<uint4 *>(dst + o) = v;
    }
    if (first && tid < head) {
        uint32_t b = ungroup_byte(stageRow, n, kLog, tid);
        if constexpr (kRowHasBase<Row>) {
            if (row.base) b ^= reinterpret_cast<const uint8_t *>(row.base)[tid];
        }
        dst[tid] = (uint8_t)b;
    }
    if (last) {
        const uint32_t from = head + words * 16u;
        if (tid < row.len - from) {
            uint32_t b = ungroup_byte(stageRow, n, kLog, from + tid);
            if constexpr (kRowHasBase<Row>) {
                if (row.base) b ^= reinterpret_cast<const uint8_t *>(row.base)[from + tid];
            }
            dst[from + tid] = (uint8_t)b;
        }
    }
}

/* One workgroup per tile: elements [e0, e0 + tileElems) of one row — 16 KiB of its destination — in the stage numbering by srcOff (stage_row_of).
 * No destination byte is read, none is written twice, none outside [dst, dst + len). */
template <class Row>
__device__ __forceinline__ void ungroup_tile(const Row *__restrict__ rows, uint32_t nRows, uint64_t firstTile, const uint8_t *__restrict__ stage,
                                             uint8_t *lds, uint32_t *which)
{
    const uint64_t v = firstTile + blockIdx.x;
    if (threadIdx.x == 0) *which = stage_row_of(rows, nRows, &Row::srcOff, v);
    __syncthreads();
    const uint32_t r = *which;
    const Row row = rows[r];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kUngroupTile >> kLog;
    const uint64_t tiles = n ? ((uint64_t)n + tileMax - 1u) / tileMax : (row.len ? 1ull : 0ull);
    const uint64_t t = v - ((row.srcOff >> kUngroupTileLog) + r);
    if (t >= tiles) return; /* (the whole workgroup) */
    const uint32_t e0 = (uint32_t)t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint8_t *stageRow = stage + row.srcOff;
    ungroup_load(stageRow, n, kLog, e0, tileElems, lds, threadIdx.x);
    __syncthreads();
    ungroup_store(row, stageRow, n, kLog, e0, tileElems, t == 0, t + 1u == tiles, lds, threadIdx.x);
}

__global__ __launch_bounds__(kUngroupT) void qzstd_ungroup_kernel(const qzstd_hip_ungroup_row_t *__restrict__ rows, uint32_t nRows, uint64_t firstTile,
                                                                   const uint8_t *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kUngroupLds];
    __shared__ uint32_t which;
    ungroup_tile(rows, nRows, firstTile, stage, lds, &which);
}

/* the destination IS read here when a row's base is its destination: see ungroup_store */
__global__ __launch_bounds__(kUngroupT) void qzstd_ungroup_xor_kernel(const qzstd_hip_ungroup_xor_row_t *__restrict__ rows, uint32_t nRows,
                                                                       uint64_t firstTile, const uint8_t *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kUngroupLds];
    __shared__ uint32_t which;
    ungroup_tile(rows, nRows, firstTile, stage, lds, &which);
}
} // namespace

extern "C" int qzstd_hip_ungroup(int device, void *stream, const qzstd_hip_ungroup_row_t *rows, uint32_t nRows, qzstd_hip_ungroup_row_t *d_rows,
                                 const void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_ungroup";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    stage_launch_t go;
    if (ungroup_rows_check(who, rows, nRows, stageBytes, kUngroupOwn, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ungroup rows)");
    hipLaunchKernelGGL(qzstd_ungroup_kernel, dim3(go.tiles), dim3(kUngroupT), 0, (hipStream_t)stream, d_rows, nRows, go.firstTile,
                       static_cast<const uint8_t *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_ungroup_kernel");
    return 0;
}

/* (a row's base may be anything, 0 and the row's dst included) */
extern "C" int qzstd_hip_ungroup_xor(int device, void *stream, const qzstd_hip_ungroup_xor_row_t *rows, uint32_t nRows,
                                     qzstd_hip_ungroup_xor_row_t *d_rows, const void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_ungroup_xor";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    stage_launch_t go;
    if (ungroup_rows_check(who, rows, nRows, stageBytes, kUngroupOwn, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ungroup xor rows)");
    hipLaunchKernelGGL(qzstd_ungroup_xor_kernel, dim3(go.tiles), dim3(kUngroupT), 0, (hipStream_t)stream, d_rows, nRows, go.firstTile,
                       static_cast<const uint8_t *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_ungroup_xor_kernel");
    return 0;
}

/* ---------------------------------------------------------------- windowed ungrouping scatter (include/qzstd_hip_device.h) -- */
namespace {
/* the frame tile that owns byte p (< len) of a frame's ungrouped content: 16 KiB of the elements each, the tail with the last one */
__host__ __device__ inline uint32_t window_tile(uint32_t p, uint32_t tiles) { return (p >> kUngroupTileLog) < tiles ? (p >> kUngroupTileLog) : tiles - 1u; }

/* One workgroup per frame tile that a row's window intersects, in the tile0 numbering (tile0_row_of).  Its body is written on its own and not through ungroup_tile /
 * ungroup_store: a window has its own origin (winOff), its own clipping of the tile and its own strips, and the two whole-row kernels stay the
 * code they were.  The pieces are shared: ungroup_load and ungroup_word take any element origin, here the first element of the workgroup's
 * share [lo, hi) of the window instead of the tile's, so only that share's part of each plane strip comes into LDS. */
__global__ __launch_bounds__(kUngroupT) void qzstd_ungroup_window_kernel(const qzstd_hip_ungroup_win_row_t *__restrict__ rows, uint32_t nRows,
                                                                          const uint8_t *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kUngroupLds];
    __shared__ uint32_t which;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) which = tile0_row_of(rows, nRows);
    __syncthreads();
    const qzstd_hip_ungroup_win_row_t row = rows[which];
    if (!row.winLen) return; /* (never: rows without a workgroup are not found, tile0_row_of) */
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kUngroupTile >> kLog;
    const uint32_t tiles = n ? (uint32_t)(((uint64_t)n + tileMax - 1u) / tileMax) : 1u;
    const uint32_t winEnd = row.winOff + row.winLen; /* <= len */
    const uint32_t tFirst = window_tile(row.winOff, tiles), tLast = window_tile(winEnd - 1u, tiles);
    const uint32_t t = tFirst + (blockIdx.x - row.tile0);
    if (t > tLast) return; /* (the whole workgroup) */
    /* [lo, hi): the window clipped to the tile, in bytes of the frame's content; the words whose first byte lies in it are this workgroup's */
    const uint32_t tileLo = t << kUngroupTileLog, tileHi = t + 1u == tiles ? row.len : (t + 1u) << kUngroupTileLog;
    const uint32_t lo = row.winOff > tileLo ? row.winOff : tileLo, hi = winEnd < tileHi ? winEnd : tileHi;
    /* its share of the elements, [eLo, eHi): what the strips in LDS hold; none when the share lies in the tail */
    const uint32_t eLo = (lo >> kLog) < n ? lo >> kLog : n;
    const uint32_t eEnd = (uint32_t)(((uint64_t)hi + (1u << kLog) - 1u) >> kLog), eHi = eEnd < n ? eEnd : n;
    const uint8_t *stageRow = stage + row.srcOff;
    ungroup_load(stageRow, n, kLog, eLo, eHi - eLo, lds, tid);
    __syncthreads();

    uint8_t *dst = reinterpret_cast<uint8_t *>(row.dst);
    /* the window's whole destination words: `words` of them from window offset `head` on; in front of them and behind them single bytes */
    const uint32_t lead = (uint32_t)(0u - row.dst) & 15u, head = lead < row.winLen ? lead : row.winLen;
    const uint32_t words = (row.winLen - head) >> 4;
    const uint64_t lim = (uint64_t)eHi << kLog; /* the strips' end: a word that reaches past it takes those bytes from the stage, one by one */
    const uint32_t w0 = row.winOff + head;      /* the first word's place in the frame's content */
    for (uint64_t i = (lo <= w0 ? 0u : ((uint64_t)(lo - w0) + 15u) >> 4) + tid; i < words && (uint64_t)w0 + i * 16u < hi; i += kUngroupT) {
        const uint32_t w = head + (uint32_t)i * 16u, o = row.winOff + w;
        uint4 v;
        switch (kLog) {
        case 0u: v = ungroup_word<1u>(lds, n, eLo, o); break;
        case 1u: v = ungroup_word<2u>(lds, n, eLo, o); break;
        case 2u: v = ungroup_word<4u>(lds, n, eLo, o); break;
        default: v = ungroup_word<8u>(lds, n, eLo, o); break;
        }
        if (lim - o < 16u) {
            uint32_t d[4] = { v.x, v.y, v.z, v.w };
            for (uint32_t b = (uint32_t)(lim - o); b < 16u; b++)
                d[b >> 2] = (d[b >> 2] & ~(0xFFu << ((b & 3u) * 8u))) | ungroup_byte(stageRow, n, kLog, o + b) << ((b & 3u) * 8u);
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        if (row.base) { /* the word lies inside the window, so both loads overlap [base, base + winLen) */
            const uint64_t b = row.base + w;
            const uint32_t bsh = (uint32_t)b & 15u;
            const uint4 *bp = reinterpret_cast<const uint4 *>(b - bsh);
            const uint4 bl = bp[0];
            uint4 bh = make_uint4(0u, 0u, 0u, 0u);
            if (bsh) bh = bp[1];
            uint64_t b0, b1;
            group_shift(bl, bh, bsh, &b0, &b1);
            v = make_uint4(v.x ^ (uint32_t)b0, v.y ^ (uint32_t)(b0 >> 32), v.z ^ (uint32_t)b1, v.w ^ (uint32_t)(b1 >> 32));
        }
        *reinterpret_cast<uint4 *>(dst + w) = v;
    }
    if (t == tFirst && tid < head) {
        uint32_t b = ungroup_byte(stageRow, n, kLog, row.winOff + tid);
        if (row.base) b ^= reinterpret_cast<const uint8_t *>(row.base)[tid];
        dst[tid] = (uint8_t)b;
    }
    if (t == tLast) {
        const uint32_t from = head + words * 16u;
        if (tid < row.winLen - from) {
            uint32_t b = ungroup_byte(stageRow, n, kLog, row.winOff + from + tid);
            if (row.base) b ^= reinterpret_cast<const uint8_t *>(row.base)[from + tid];
            dst[from + tid] = (uint8_t)b;
        }
    }
}
} // namespace

extern "C" int qzstd_hip_ungroup_window(int device, void *stream, qzstd_hip_ungroup_win_row_t *rows, uint32_t nRows,
                                        qzstd_hip_ungroup_win_row_t *d_rows, const void *d_stage, size_t stageBytes)
{
    using row_t = qzstd_hip_ungroup_win_row_t;
    constexpr const char *who = "qzstd_hip_ungroup_window";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    uint64_t end = 0;
    const auto check = [&](const row_t &r, uint32_t i) -> const char * {
        if (const char *why = elem_check(r.elem)) return why;
        if (r.reserved) return "reserved not 0";
        if (r.srcOff & 15u) return "srcOff not a multiple of 16";
        if (const char *why = len_check(r.len)) return why;
        if ((uint64_t)r.winOff + r.winLen > r.len) return "a window ends past its frame";
        if (r.winLen && !r.dst) return "null destination";
        const bool again = i && r.srcOff == rows[i - 1].srcOff; /* the same frame again: the next window of it */
        if (again && (r.len != rows[i - 1].len || r.elem != rows[i - 1].elem || r.winOff < (uint64_t)rows[i - 1].winOff + rows[i - 1].winLen))
            return "windows of one frame differ in len or elem, overlap or are not in ascending order";
        if (const char *why = stage_place(r.srcOff, round16(r.len), r.len, stageBytes, again, &end)) return why;
        return i + 1u == nRows ? stage_span_check(end) : nullptr; /* (of the whole table: behind the last row's own checks) */
    };
    const auto tiles = [](const row_t &r) -> uint32_t { /* the frame tiles that the window intersects */
        if (!r.winLen) return 0u;
        const uint64_t n = r.len / r.elem, tileMax = kUngroupTile / r.elem;
        const uint32_t frameTiles = n ? (uint32_t)((n + tileMax - 1u) / tileMax) : 1u;
        return window_tile(r.winOff + r.winLen - 1u, frameTiles) - window_tile(r.winOff, frameTiles) + 1u;
    };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, tiles, false, &total)) return -1;
    if (total == 0) return 0; /* nothing but empty windows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ungroup window rows)");
    hipLaunchKernelGGL(qzstd_ungroup_window_kernel, dim3(total), dim3(kUngroupT), 0, (hipStream_t)stream, d_rows, nRows,
                       static_cast<const uint8_t *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_ungroup_window_kernel");
    return 0;
}

/* ---------------------------------------------------------------- ungrouping comparison (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kCmpSame = 0xFFFFFFFFu; /* a tile word: nothing differs */

/* the first `valid` (1 .. 16) of the 16 bytes {o1, o0}; the others become 0 */
__device__ inline void cmp_mask(uint32_t valid, uint64_t *o0, uint64_t *o1)
{
    if (valid >= 16u) return;
    *o1 = valid > 8u ? *o1 & ((1ull << ((valid - 8u) * 8u)) - 1ull) : 0ull;
    if (valid < 8u) *o0 &= (1ull << (valid * 8u)) - 1ull;
}

/* qzstd_ungroup_xor_kernel with its store replaced by a comparison.  One workgroup per 16 KiB tile of a frame's ungrouped content u[] (the tail
 * with the last tile, a frame shorter than an element one tile), in the tile0 numbering (tile0_row_of).
 * Phase A is ungroup_load: the tile's plane strips, stage to LDS — nothing for a ZERO row, whose u[] is zeros and whose stage is
 * never read.  Phase B walks the tile's bytes [t0, t1) of u[] in 16-byte steps FROM THE TILE'S START (nothing is stored, so no side's
 * alignment has to be met): a lane assembles u's 16 bytes with ungroup_word, takes the few bytes behind the strips' end — the tail — singly
 * from the stage (ungroup_byte), fetches base and ref as the comparison with a base fetches its sides (group_fetch: the aligned words that
 * overlap the wanted bytes only, each shifted by its OWN misalignment), masks what lies behind the row's last byte, and keeps the lowest
 * row offset whose byte differs.  A wave min (xor shuffles), one LDS step across the four waves, and thread 0 stores the tile's ONE word. */
__global__ __launch_bounds__(kUngroupT) void qzstd_ungroup_cmp_kernel(const qzstd_hip_ungroup_cmp_row_t *__restrict__ rows, uint32_t nRows,
                                                                       const uint8_t *__restrict__ stage, uint32_t *__restrict__ tilesOut)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kUngroupLds];
    __shared__ uint32_t which;
    __shared__ uint32_t red[kUngroupT / 64u];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) which = tile0_row_of(rows, nRows);
    __syncthreads();
    const qzstd_hip_ungroup_cmp_row_t row = rows[which];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kUngroupTile >> kLog;
    const uint32_t tiles = n ? (uint32_t)(((uint64_t)n + tileMax - 1u) / tileMax) : (row.len ? 1u : 0u);
    const uint32_t t = blockIdx.x - row.tile0;
    if (t >= tiles) return; /* (the whole workgroup; never: rows without a tile share the tile0 of the row behind them) */
    const bool zero = (row.flags & 1u) != 0u;
    const uint32_t e0 = t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint8_t *stageRow = stage + row.srcOff;
    if (!zero) ungroup_load(stageRow, n, kLog, e0, tileElems, lds, tid); /* (row is the workgroup's: the branch is uniform) */
    __syncthreads();

    const uint32_t t0 = e0 << kLog, lim = (e0 + tileElems) << kLog; /* the tile's bytes of u[]: what its strips hold (len <= 0xFFFFFFE0) */
    const uint32_t t1 = t + 1u == tiles ? row.len : lim;           /* the tail behind the elements goes with the last tile */
    uint32_t first = kCmpSame;
    for (uint32_t rel = tid * 16u; rel < t1 - t0; rel += kUngroupT * 16u) { /* (t1 - t0 <= 16 KiB + 7: no wrap near 4 GiB) */
        const uint32_t o = t0 + rel, valid = t1 - o < 16u ? t1 - o : 16u;
        uint64_t u0 = 0ull, u1 = 0ull;
        if (!zero) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (o < lim) {
                switch (kLog) {
                case 0u: v = ungroup_word<1u>(lds, n, e0, o); break;
                case 1u: v = ungroup_word<2u>(lds, n, e0, o); break;
                case 2u: v = ungroup_word<4u>(lds, n, e0, o); break;
                default: v = ungroup_word<8u>(lds, n, e0, o); break;
                }
            }
            if (lim - o < valid || o >= lim) { /* the word reaches into the tail: those bytes one by one, from the stage */
                uint32_t d[4] = { v.x, v.y, v.z, v.w };
                for (uint32_t b = o < lim ? lim - o : 0u; b < valid; b++)
                    d[b >> 2] = (d[b >> 2] & ~(0xFFu << ((b & 3u) * 8u))) | ungroup_byte(stageRow, n, kLog, o + b) << ((b & 3u) * 8u);
                v = make_uint4(d[0], d[1], d[2], d[3]);
            }
            u0 = v.x | (uint64_t)v.y << 32;
            u1 = v.z | (uint64_t)v.w << 32;
        }
        uint64_t r0, r1;
        group_fetch(row.ref + o, valid, &r0, &r1);
        u0 ^= r0;
        u1 ^= r1;
        if (row.base) {
            uint64_t b0, b1;
            group_fetch(row.base + o, valid, &b0, &b1);
            u0 ^= b0;
            u1 ^= b1;
        }
        cmp_mask(valid, &u0, &u1); /* the row's last word: what lies behind the row, in the strips' slack and in memory, does not count */
        if (u0 | u1) {
            const uint32_t at = o + (u0 ? (uint32_t)__builtin_ctzll(u0) >> 3 : 8u + ((uint32_t)__builtin_ctzll(u1) >> 3));
            first = at < first ? at : first; /* (a lane's offsets ascend: only its first one is kept) */
        }
    }
#pragma unroll
    for (uint32_t d = 32u; d; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)first, (int)d, 64);
        first = other < first ? other : first;
    }
    if ((tid & 63u) == 0u) red[tid >> 6] = first;
    __syncthreads();
    if (tid == 0) {
        uint32_t m = red[0];
#pragma unroll
        for (uint32_t w = 1; w < kUngroupT / 64u; w++) m = red[w] < m ? red[w] : m;
        tilesOut[blockIdx.x] = m;
    }
}
} // namespace

extern "C" int qzstd_hip_ungroup_cmp(int device, void *stream, qzstd_hip_ungroup_cmp_row_t *rows, uint32_t nRows,
                                     qzstd_hip_ungroup_cmp_row_t *d_rows, const void *d_stage, size_t stageBytes, uint32_t *d_tiles)
{
    using row_t = qzstd_hip_ungroup_cmp_row_t;
    constexpr const char *who = "qzstd_hip_ungroup_cmp";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    uint64_t end = 0;
    const auto check = [&](const row_t &r, uint32_t) -> const char * {
        if (const char *why = elem_check(r.elem)) return why;
        if (r.flags & ~QZSTD_HIP_CMP_ZERO) return "unknown flags";
        if (const char *why = len_check(r.len)) return why;
        if (r.len && !r.ref) return "null ref";
        if (r.flags & QZSTD_HIP_CMP_ZERO) return nullptr; /* a ZERO row's srcOff is not looked at */
        return frame_place(r.srcOff, r.len, d_stage, stageBytes, &end);
    };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, [](const row_t &r) { return QZSTD_HIP_CMP_TILES(r.len, r.elem); }, false, &total)) return -1;
    if (total == 0) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ungroup cmp rows)");
    hipLaunchKernelGGL(qzstd_ungroup_cmp_kernel, dim3(total), dim3(kUngroupT), 0, (hipStream_t)stream, d_rows, nRows,
                       static_cast<const uint8_t *>(d_stage), d_tiles);
    QZ_CHECK(hipGetLastError(), "launch qzstd_ungroup_cmp_kernel");
    return 0;
}

/* ---------------------------------------------------------------- comparison with a base (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kDiffT = 256u;               /* threads per workgroup */
constexpr uint32_t kDiffTileLog = kGroupTileLog; /* bytes of one row per workgroup: 16 KiB, four 16-byte words per lane */

/* One workgroup per 16 KiB tile of a row, in the tile0 numbering (tile0_row_of).  Both sides are fetched as the grouping gather fetches
 * its source — group_fetch: the aligned word that holds the first wanted byte and the next one only when wanted bytes lie in it, shifted
 * by that side's OWN misalignment, so the bytes in front of a and b never arrive — and the bytes behind the row's last one are masked
 * before the lane's OR.  A wave that saw a difference stores the 1 from one lane: no atomics, the flag is never read. */
__global__ __launch_bounds__(kDiffT) void qzstd_diff_kernel(const qzstd_hip_diff_row_t *__restrict__ rows, uint32_t nRows, uint32_t *__restrict__ flags)
{
    __shared__ uint32_t which;
    if (threadIdx.x == 0) which = tile0_row_of(rows, nRows);
    __syncthreads();
    const uint32_t r = which;
    const qzstd_hip_diff_row_t row = rows[r];
    const uint64_t at = (uint64_t)(blockIdx.x - row.tile0) << kDiffTileLog; /* the tile's first byte in its row */
    if (at >= row.len) return; /* (never: rows without a tile are not found, tile0_row_of) */
    const uint32_t tileBytes = row.len - at < (1u << kDiffTileLog) ? (uint32_t)(row.len - at) : 1u << kDiffTileLog;
    uint64_t acc = 0;
    for (uint32_t w = threadIdx.x; w * 16u < tileBytes; w += kDiffT) {
        const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
        uint64_t a0, a1, b0, b1;
        group_fetch(row.a + at + w * 16u, valid, &a0, &a1);
        group_fetch(row.b + at + w * 16u, valid, &b0, &b1);
        a0 ^= b0;
        a1 ^= b1;
        if (valid < 16u) { /* the row's last word: what lies behind the row does not count */
            a1 = valid > 8u ? a1 & ((1ull << ((valid - 8u) * 8u)) - 1ull) : 0ull;
            if (valid < 8u) a0 &= (1ull << (valid * 8u)) - 1ull;
        }
        acc |= a0 | a1;
    }
    if (__any(acc != 0ull) && (threadIdx.x & 63u) == 0u) flags[r] = 1u;
}
} // namespace

extern "C" int qzstd_hip_diff(int device, void *stream, qzstd_hip_diff_row_t *rows, uint32_t nRows, qzstd_hip_diff_row_t *d_rows, uint32_t *d_flags)
{
    using row_t = qzstd_hip_diff_row_t;
    constexpr const char *who = "qzstd_hip_diff";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_flags) return refuse(who, "null pointer");
    const auto check = [](const row_t &r, uint32_t) -> const char * { return r.len && (!r.a || !r.b) ? "null row" : len_check(r.len); };
    const auto tiles = [](const row_t &r) { return ((uint64_t)r.len + (1u << kDiffTileLog) - 1u) >> kDiffTileLog; };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, tiles, true, &total)) return -1;
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemsetAsync(d_flags, 0, (size_t)nRows * sizeof(uint32_t), (hipStream_t)stream), "hipMemsetAsync (diff flags)");
    if (total == 0) return 0; /* nothing but empty rows: their flags are 0 */
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (diff rows)");
    hipLaunchKernelGGL(qzstd_diff_kernel, dim3(total), dim3(kDiffT), 0, (hipStream_t)stream, d_rows, nRows, d_flags);
    QZ_CHECK(hipGetLastError(), "launch qzstd_diff_kernel");
    return 0;
}

/* ---------------------------------------------------------------- content checksum (include/qzstd_hip_device.h) -- */
namespace {
constexpr uint32_t kHashRows = 16u;                /* rows per wave: four lanes each, one per XXH64 accumulator */
constexpr uint32_t kHashTile = QZSTD_HIP_XXH64_TILE; /* bytes of a row per fetch: one whole-wave 16-byte load */
constexpr uint32_t kHashPitch = kHashTile + 32u;    /* a row's tile in LDS: 32 bytes of padding put the eight rows of a 32-lane group on
                                                       the 64 banks once (8 B per lane, 32 B per row and stripe) */
constexpr uint64_t kXP1 = 0x9E3779B185EBCA87ull, kXP2 = 0xC2B2AE3D27D4EB4Full, kXP3 = 0x165667B19E3779F9ull, kXP4 = 0x85EBCA77C2B2AE63ull,
                   kXP5 = 0x27D4EB2F165667C5ull;

typedef uint32_t hash_word_t __attribute__((ext_vector_type(4))); /* one aligned 16-byte word */

__device__ inline uint64_t xxh_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
__device__ inline uint64_t xxh_round(uint64_t acc, uint64_t in) { return xxh_rotl(acc + in * kXP2, 31u) * kXP1; }
__device__ inline uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0ull, v)) * kXP1 + kXP4; }

/* One wave per workgroup, rows [16 * blockIdx.x, + 16).  Per step every row's next 1 KiB tile is fetched with one 16-byte load per lane
 * (the words that overlap the row only) into registers while the tile before it, in LDS, is consumed: lane 4 r + a runs accumulator a
 * of row r over the tile's 32-byte stripes.  The multiply chain (two 64-bit multiplies per 8 bytes and lane) sets the pace; the fetch of
 * the next tile has a whole tile's chain to arrive.  A row ends in the step that holds byte (len & ~31): its first lane collects the
 * four accumulators, walks the tail (8-, 4- and 1-byte steps over bytes below len only) and stores the hash.  The loop runs to the longest
 * row of the wave; lanes of rows that are done idle. */
__global__ __launch_bounds__(64) void qzstd_xxh64_kernel(const uint8_t *__restrict__ base, const qzstd_hip_hash_row_t *__restrict__ rows,
                                                         uint32_t nRows, unsigned long long *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[kHashRows * kHashPitch];
    const uint32_t lane = threadIdx.x, r = lane >> 2, a = lane & 3u;
    const uint32_t row0 = blockIdx.x * kHashRows;
    /* the wave's rows, by uniform addresses: their offsets and 16-byte word counts are the same in every lane (scalar registers) */
#define QZ_HASH_EACH_ROW(X, t) X(0, t) X(1, t) X(2, t) X(3, t) X(4, t) X(5, t) X(6, t) X(7, t) X(8, t) X(9, t) X(10, t) X(11, t) X(12, t) X(13, t) X(14, t) X(15, t)
#define QZ_HASH_ROW(j, t)                                                                   \
    const uint64_t off##j = row0 + j < nRows ? rows[row0 + j].srcOff : 0ull;               \
    const uint64_t words##j = row0 + j < nRows ? (rows[row0 + j].len + 15u) >> 4 : 0ull;   \
    hash_word_t next##j = { 0u, 0u, 0u, 0u };                                              \
    nTiles = (words##j >> 6) + 1u > nTiles ? (words##j >> 6) + 1u : nTiles;
    uint64_t nTiles = 0; /* steps of the wave: past the longest row's tail (a row of k whole tiles ends in step k, which fetches nothing) */
    QZ_HASH_EACH_ROW(QZ_HASH_ROW, 0)
    const uint64_t len = row0 + r < nRows ? rows[row0 + r].len : 0ull;
    const uint64_t endTile = len / kHashTile; /* the tile that holds the row's tail; every stripe of the row lies at or before it */
    uint64_t acc = a == 0u ? kXP1 + kXP2 : (a == 1u ? kXP2 : (a == 2u ? 0ull : 0ull - kXP1));
    uint64_t stripesLeft = len >> 5;
    /* tile t of row j: word t * 64 + lane of the row, when the row has it.  Sixteen named registers, not an array: the fetches must stay
     * in flight in VGPRs across the chain below */
#define QZ_HASH_FETCH1(j, t) \
    if ((t) * (kHashTile / 16u) + lane < words##j) next##j = reinterpret_cast<const hash_word_t *>(base + off##j)[(t) * (kHashTile / 16u) + lane];
#define QZ_HASH_STAGE1(j, t) \
    if ((t) * (kHashTile / 16u) + lane < words##j) *reinterpret_cast<hash_word_t *>(&tile[j * kHashPitch + lane * 16u]) = next##j;
#define QZ_HASH_FETCH(t) QZ_HASH_EACH_ROW(QZ_HASH_FETCH1, t)
#define QZ_HASH_STAGE(t) QZ_HASH_EACH_ROW(QZ_HASH_STAGE1, t)
    QZ_HASH_FETCH(0ull)
    QZ_HASH_STAGE(0ull)
    __syncthreads();
    for (uint64_t t = 0; t < nTiles; t++) {
        const bool more = t + 1u < nTiles;
        if (more) { QZ_HASH_FETCH(t + 1u) }
        const uint8_t *mine = &tile[r * kHashPitch];
        const uint32_t n = stripesLeft < kHashTile / 32u ? (uint32_t)stripesLeft : kHashTile / 32u;
        for (uint32_t s = 0; s < n; s++) acc = xxh_round(acc, *reinterpret_cast<const uint64_t *>(mine + s * 32u + a * 8u));
        stripesLeft -= n;
        /* (all lanes: the row's accumulators to each of its lanes) */
        const uint64_t v1 = __shfl(acc, (int)(lane & ~3u)), v2 = __shfl(acc, (int)(lane & ~3u) + 1), v3 = __shfl(acc, (int)(lane & ~3u) + 2),
                       v4 = __shfl(acc, (int)(lane & ~3u) + 3);
        if (t == endTile && a == 0u && row0 + r < nRows) {
            uint64_t h;
            if (len >= 32u) {
                h = xxh_rotl(v1, 1u) + xxh_rotl(v2, 7u) + xxh_rotl(v3, 12u) + xxh_rotl(v4, 18u);
                h = xxh_merge(xxh_merge(xxh_merge(xxh_merge(h, v1), v2), v3), v4);
            } else {
                h = kXP5;
            }
            h += len;
            uint32_t p = (uint32_t)((len & ~(uint64_t)31u) - t * kHashTile), left = (uint32_t)len & 31u;
            for (; left >= 8u; left -= 8u, p += 8u)
                h = xxh_rotl(h ^ xxh_round(0ull, *reinterpret_cast<const uint64_t *>(mine + p)), 27u) * kXP1 + kXP4;
            if (left >= 4u) {
                h = xxh_rotl(h ^ (uint64_t)*reinterpret_cast<const uint32_t *>(mine + p) * kXP1, 23u) * kXP2 + kXP3;
                p += 4u;
                left -= 4u;
            }
            for (; left; left--, p++) h = xxh_rotl(h ^ (uint64_t)mine[p] * kXP5, 11u) * kXP1;
            h ^= h >> 33;
            h *= kXP2;
            h ^= h >> 29;
            h *= kXP3;
            h ^= h >> 32;
            out[row0 + r] = h;
        }
        __syncthreads(); /* the tile is consumed: the next one may take its place */
        if (more) { QZ_HASH_STAGE(t + 1u) }
        __syncthreads();
    }
#undef QZ_HASH_EACH_ROW
#undef QZ_HASH_ROW
#undef QZ_HASH_FETCH1
#undef QZ_HASH_STAGE1
#undef QZ_HASH_FETCH
#undef QZ_HASH_STAGE
}
} // namespace

extern "C" int qzstd_hip_xxh64(int device, void *stream, const void *d_base, const qzstd_hip_hash_row_t *rows, uint32_t nRows,
                               qzstd_hip_hash_row_t *d_rows, uint64_t *d_out)
{
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_out) return fail_msg("qzstd_hip_xxh64: null pointer");
    if ((uintptr_t)d_base & 15u) return fail_msg("qzstd_hip_xxh64: base not 16-byte aligned");
    for (uint32_t i = 0; i < nRows; i++) {
        if (rows[i].srcOff & 15u) return fail_msg("qzstd_hip_xxh64: srcOff not a multiple of 16");
        if (rows[i].len && !d_base) return fail_msg("qzstd_hip_xxh64: null base");
    }
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (hash rows)");
    hipLaunchKernelGGL(qzstd_xxh64_kernel, dim3((nRows + kHashRows - 1u) / kHashRows), dim3(64), 0, (hipStream_t)stream,
                       static_cast<const uint8_t *>(d_base), d_rows, nRows, reinterpret_cast<unsigned long long *>(d_out));
    QZ_CHECK(hipGetLastError(), "launch qzstd_xxh64_kernel");
    return 0;
}

/* ---------------------------------------------------------------- plane cost (include/qzstd_hip_device.h, qzstd_planecost.h) -- */
#include "qzstd_planecost.h"

namespace {
constexpr uint32_t kPlaneT = 256u;      /* threads per workgroup: one per bin in the reduction, four waves to hide the loads' latency */
constexpr uint32_t kPlaneCopies = 16u;  /* sub-histograms: bin b of copy c at word b * 16 + c — the 64 lanes of a wave that all meet ONE
                                           bin (an exponent plane) land on 16 banks, four lanes per word, not 64 on one; the lanes of
                                           a noise plane spread over all 64 banks.  16 KiB of LDS: eight workgroups a CU, all 32 waves */

/* One workgroup per row (a block of at most 128 KiB).  The aligned 16-byte words that overlap [base + srcOff, + len) — and no other — are
 * loaded once each, lane after lane; the bytes of the first and last word that lie outside the row are skipped, every other byte is one
 * LDS atomic add on the lane's sub-histogram.  Then thread b sums bin b over the copies, takes its term of the cost
 * (QZSTD_planeTerm), the terms are added across the wave (xor shuffles) and the four waves (one LDS step), and thread 0 stores the row's
 * ONE word.  No global atomics; the output is never read. */
__global__ __launch_bounds__(kPlaneT) void qzstd_plane_cost_kernel(const uint8_t *__restrict__ base, const qzstd_hip_plane_row_t *__restrict__ rows,
                                                                    uint32_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[256u * kPlaneCopies];
    __shared__ uint32_t red[kPlaneT / 64u];
    const uint32_t tid = threadIdx.x;
    const qzstd_hip_plane_row_t row = rows[blockIdx.x];
    for (uint32_t i = tid; i < 256u * kPlaneCopies; i += kPlaneT) hist[i] = 0u;
    __syncthreads();
    const uint64_t a = (uint64_t)(uintptr_t)base + row.srcOff;
    const uint32_t head = (uint32_t)a & 15u;
    const uint4 *words = reinterpret_cast<const uint4 *>(a - head);
    const uint32_t span = head + row.len;                          /* (len <= 128 KiB) */
    const uint32_t nWords = row.len ? (span + 15u) >> 4 : 0u;      /* the last one holds byte len - 1; an empty row loads nothing */
    uint32_t *mine = &hist[tid & (kPlaneCopies - 1u)];
    for (uint32_t w = tid; w < nWords; w += kPlaneT) {
        const uint4 v = words[w];
        const uint32_t d[4] = { v.x, v.y, v.z, v.w };
        const uint32_t lo = w ? 0u : head, hi = span - w * 16u < 16u ? span - w * 16u : 16u;
        if (lo == 0u && hi == 16u) {
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++) atomicAdd(&mine[((d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu) * kPlaneCopies], 1u);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++)
                if (b >= lo && b < hi) atomicAdd(&mine[((d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu) * kPlaneCopies], 1u);
        }
    }
    __syncthreads();
    uint32_t c = 0u;
    {
        const uint4 *h = reinterpret_cast<const uint4 *>(&hist[tid * kPlaneCopies]);
#pragma unroll
        for (uint32_t j = 0; j < kPlaneCopies / 4u; j++) {
            const uint4 q = h[j];
            c += q.x + q.y + q.z + q.w;
        }
    }
    uint32_t sum = QZSTD_planeTerm(c, QZSTD_planeLog2(row.len)); /* (at most len * L(len) < 2^30 in all: 32 bits hold every partial sum) */
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)s, 64);
    if ((tid & 63u) == 0u) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = red[0];
#pragma unroll
        for (uint32_t w = 1; w < kPlaneT / 64u; w++) total += red[w];
        out[blockIdx.x] = QZSTD_planeCostOfSum(total);
    }
}
} // namespace

extern "C" int qzstd_hip_plane_cost(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                                    qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost)
{
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_cost) return fail_msg("qzstd_hip_plane_cost: null pointer");
    if (nRows > 0x7FFFFFFFu) return fail_msg("qzstd_hip_plane_cost: too many rows");
    for (uint32_t i = 0; i < nRows; i++) {
        if (rows[i].len > QZSTD_PLANE_LEN_MAX) return fail_msg("qzstd_hip_plane_cost: a row longer than 128 KiB");
        if (rows[i].reserved) return fail_msg("qzstd_hip_plane_cost: reserved not 0");
        if (rows[i].len && !d_base) return fail_msg("qzstd_hip_plane_cost: null base");
    }
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (plane cost rows)");
    hipLaunchKernelGGL(qzstd_plane_cost_kernel, dim3(nRows), dim3(kPlaneT), 0, (hipStream_t)stream, static_cast<const uint8_t *>(d_base), d_rows, d_cost);
    QZ_CHECK(hipGetLastError(), "launch qzstd_plane_cost_kernel");
    return 0;
}

/* ---------------------------------------------------------------- Huffman literals coder (include/qzstd_hip_device.h, qzstd_hufblock.h) -- */
#include "qzstd_hufblock.h"

namespace {
constexpr uint32_t kHufT = kPlaneT; /* four waves: one per stream */

__device__ inline uint32_t huf_round16(uint32_t x) { return (x + 15u) & ~15u; }

/* off[i] <- f(0) + .. + f(i - 1) for i = 0 .. n, by ONE workgroup, kHufT rows a step.  sizes == nullptr: f(i) = QZSTD_HIP_HUF_ROW_BYTES of row
 * i's len (a row's place in the scratch); else f(i) = the bytes row i takes in the dense area, 0 without a size word.  The launcher has
 * checked that the sums stay below 2^32. */
__global__ __launch_bounds__(kHufT) void qzstd_huf_scan_kernel(const qzstd_hip_plane_row_t *__restrict__ rows, const uint32_t *__restrict__ sizes,
                                                               uint32_t n, uint32_t *__restrict__ off)
{
    __shared__ uint32_t red[kHufT / 64u];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t carry = 0u;
    for (uint32_t c = 0; c < n; c += kHufT) {
        const uint32_t i = c + threadIdx.x;
        uint32_t mine = 0u;
        if (i < n) {
            if (sizes) mine = sizes[i] ? huf_round16(QZSTD_HUF_LENGTHS_BYTES + sizes[i]) : 0u;
            else mine = (uint32_t)QZSTD_HIP_HUF_ROW_BYTES(rows[i].len);
        }
        uint32_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63u) red[wave] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kHufT / 64u; w++) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        __syncthreads(); /* red is rewritten by the next step */
        if (i < n) off[i] = before + incl - mine;
        carry += all;
    }
    if (threadIdx.x == 0) off[n] = carry;
}

/* One workgroup per row; see include/qzstd_hip_device.h.  A row's bytes go to stage + stageOff[row]: 128 bytes of lengths, then the jump table
 * and the streams, as 32-bit words (the place is 16-byte aligned; the last word may reach up to 3 bytes past the streams, inside the row's
 * QZSTD_HIP_HUF_ROW_BYTES).
 *
 * The bits of jump table + streams are one string of 8 * size bits, cut among the 256 threads in the order q = 64 * stream + (63 - lane):
 * thread q writes the bits [S[q], S[q + 1]) — its run's codes from the run's last byte to its first; the stream's first lane also the closing
 * 1 bit and the zeros up to the byte; q = 0 also the jump table in front.  A word that lies wholly inside a thread's bits is stored by it.
 * A word shared by several threads is put together in edge[q], q the thread that holds the word's FIRST bit (found by a search over S; for a
 * thread's last, unfinished word that is the thread itself), with LDS atomic ORs, and stored by that thread after the barrier. */
__global__ __launch_bounds__(kHufT) void qzstd_huf_code_kernel(const uint8_t *__restrict__ base, const qzstd_hip_plane_row_t *__restrict__ rows,
                                                               const uint32_t *__restrict__ stageOff, uint32_t *__restrict__ cost,
                                                               uint32_t *__restrict__ size, uint8_t *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[256u * kPlaneCopies];
    __shared__ uint32_t cnt[256], keys[256], tab[256], S[kHufT + 1u], edge[kHufT], red[kHufT / 64u], streamBits[4];
    __shared__ uint8_t nbits[256];
    __shared__ QZSTD_hufWksp ws;
    const uint32_t tid = threadIdx.x;
    const qzstd_hip_plane_row_t row = rows[blockIdx.x];
    const uint32_t len = row.len;
    for (uint32_t i = tid; i < 256u * kPlaneCopies; i += kHufT) hist[i] = 0u;
    edge[tid] = 0u;
    __syncthreads();
    const uint64_t a = (uint64_t)(uintptr_t)base + row.srcOff;
    {   /* the histogram and the cost word: qzstd_plane_cost_kernel's */
        const uint32_t head = (uint32_t)a & 15u;
        const uint4 *words = reinterpret_cast<const uint4 *>(a - head);
        const uint32_t span = head + len;
        const uint32_t nWords = len ? (span + 15u) >> 4 : 0u;
        uint32_t *mine = &hist[tid & (kPlaneCopies - 1u)];
        for (uint32_t w = tid; w < nWords; w += kHufT) {
            const uint4 v = words[w];
            const uint32_t d[4] = { v.x, v.y, v.z, v.w };
            const uint32_t lo = w ? 0u : head, hi = span - w * 16u < 16u ? span - w * 16u : 16u;
            if (lo == 0u && hi == 16u) {
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++) atomicAdd(&mine[((d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu) * kPlaneCopies], 1u);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 16u; b++)
                    if (b >= lo && b < hi) atomicAdd(&mine[((d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu) * kPlaneCopies], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t c = 0u;
    {
        const uint4 *h = reinterpret_cast<const uint4 *>(&hist[tid * kPlaneCopies]);
#pragma unroll
        for (uint32_t j = 0; j < kPlaneCopies / 4u; j++) {
            const uint4 q = h[j];
            c += q.x + q.y + q.z + q.w;
        }
    }
    cnt[tid] = c;
    uint32_t sum = QZSTD_planeTerm(c, QZSTD_planeLog2(len));
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)s, 64);
    if ((tid & 63u) == 0u) red[tid >> 6] = sum;
    const uint32_t present = (uint32_t)__syncthreads_count(c != 0u);
    if (tid == 0) {
        uint32_t total = red[0];
#pragma unroll
        for (uint32_t w = 1; w < kHufT / 64u; w++) total += red[w];
        cost[blockIdx.x] = QZSTD_planeCostOfSum(total);
    }
    if (len < QZSTD_HUF_LEN_MIN || len > QZSTD_HUF_LEN_MAX || present < 2u) { /* (the same for every thread) */
        if (tid == 0) size[blockIdx.x] = 0u;
        return;
    }
    /* the bytes that occur, ascending by (count, value): every thread ranks its own */
    if (c) {
        const uint32_t key = (c << 8) | tid;
        uint32_t rank = 0u;
        for (uint32_t u = 0; u < 256u; u++) {
            const uint32_t cu = cnt[u];
            rank += (cu != 0u && ((cu << 8) | u) < key) ? 1u : 0u;
        }
        keys[rank] = key;
    }
    __syncthreads();
    if (tid == 0) {
        (void)QZSTD_hufLengthsSorted(keys, present, nbits, &ws);
        QZSTD_hufCodes(nbits, tab);
    }
    __syncthreads();
    /* one wave per stream, a lane per run of consecutive bytes */
    const uint32_t k = tid >> 6, lane = tid & 63u, q = k * 64u + (63u - lane);
    uint32_t segStart, segEnd;
    QZSTD_hufStreamSpan(len, k, &segStart, &segEnd);
    const uint32_t segLen = segEnd - segStart, run = (segLen + 63u) >> 6;
    const uint32_t rs = segStart + (lane * run < segLen ? lane * run : segLen);
    const uint32_t re = segStart + ((lane + 1u) * run < segLen ? (lane + 1u) * run : segLen);
    const uint64_t A0 = a + rs, A1 = a + re; /* the run's bytes; A0 == A1: none */
    uint32_t bits = 0u;
    if (A1 > A0) {
        for (uint64_t wa = A0 & ~15ull; wa < A1; wa += 16u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(wa);
            const uint32_t d[4] = { v.x, v.y, v.z, v.w };
            const uint32_t lo = wa < A0 ? (uint32_t)(A0 - wa) : 0u, hi = A1 - wa < 16u ? (uint32_t)(A1 - wa) : 16u;
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++)
                if (b >= lo && b < hi) bits += tab[(d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu] >> 16;
        }
    }
    /* the run's bit offset in its stream: the bits of the runs behind it (the stream is written from its last byte) */
    uint32_t incl = bits;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)incl, d, 64);
        if (lane + d < 64u) incl += o;
    }
    if (lane == 0u) streamBits[k] = incl;
    __syncthreads();
    uint32_t byteOff[5];
    byteOff[0] = QZSTD_HUF_JUMP_BYTES;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) byteOff[j + 1u] = byteOff[j] + QZSTD_hufStreamBytes(streamBits[j]);
    const uint32_t sizeWord = QZSTD_hufSizeWord(byteOff[4], len);
    if (!sizeWord) { /* (the same for every thread) */
        if (tid == 0) size[blockIdx.x] = 0u;
        return;
    }
    S[q] = q ? 8u * byteOff[k] + (incl - bits) : 0u;
    if (tid == 0) S[kHufT] = 8u * sizeWord;
    __syncthreads();
    uint8_t *mine = stage + stageOff[blockIdx.x];
    uint32_t *out = reinterpret_cast<uint32_t *>(mine + QZSTD_HUF_LENGTHS_BYTES);
    const uint32_t myStart = S[q], myNext = S[q + 1u];
    if (myNext > myStart) {
        uint32_t wordIdx = myStart >> 5, fill = myStart & 31u, owner = q;
        bool headShared = fill != 0u;
        uint64_t acc = 0ull;
        if (headShared) { /* the last thread whose bits begin at or before the word's first bit */
            const uint32_t x = myStart & ~31u;
            uint32_t lo = 0u, hi = q; /* S[lo] <= x < S[hi] */
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (S[mid] <= x) lo = mid;
                else hi = mid;
            }
            owner = lo;
        }
        auto emit = [&](uint32_t v, uint32_t nb) {
            acc |= (uint64_t)v << fill;
            fill += nb;
            if (fill >= 32u) {
                if (headShared) {
                    atomicOr(&edge[owner], (uint32_t)acc);
                    headShared = false;
                } else {
                    out[wordIdx] = (uint32_t)acc;
                }
                acc >>= 32;
                fill -= 32u;
                wordIdx++;
            }
        };
        if (q == 0u) {
#pragma unroll
            for (uint32_t j = 0; j < 3u; j++) emit(byteOff[j + 1u] - byteOff[j], 16u);
        }
        if (A1 > A0) {
            for (uint64_t wa = (A1 - 1u) & ~15ull;; wa -= 16u) {
                const uint4 v = *reinterpret_cast<const uint4 *>(wa);
                const uint32_t d[4] = { v.x, v.y, v.z, v.w };
                const uint32_t lo = wa < A0 ? (uint32_t)(A0 - wa) : 0u, hi = A1 - wa < 16u ? (uint32_t)(A1 - wa) : 16u;
#pragma unroll
                for (uint32_t b = 16u; b-- > 0u;) {
                    if (b >= lo && b < hi) {
                        const uint32_t t = tab[(d[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu];
                        emit(t & 0xFFFFu, t >> 16);
                    }
                }
                if (wa <= (A0 & ~15ull)) break;
            }
        }
        if (lane == 0u) {
            emit(1u, 1u);
            emit(0u, 7u - (streamBits[k] & 7u));
        }
        if (fill) atomicOr(&edge[headShared ? owner : q], (uint32_t)acc);
    }
    __syncthreads();
    if (myNext > myStart && (myNext & 31u) && myStart <= (myNext & ~31u)) out[myNext >> 5] = edge[q];
    if (tid < QZSTD_HUF_LENGTHS_BYTES / 4u) {
        uint32_t w = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) w |= (uint32_t)(nbits[8u * tid + 2u * j] | (nbits[8u * tid + 2u * j + 1u] << 4)) << (8u * j);
        reinterpret_cast<uint32_t *>(mine)[tid] = w;
    }
    if (tid == 0) size[blockIdx.x] = sizeWord;
}

/* the kept rows' bytes from their places in the scratch to the dense area, 16 bytes a thread; what lies behind lengths + size in the last 16 is
 * written as zeros */
__global__ __launch_bounds__(kHufT) void qzstd_huf_pack_kernel(const uint32_t *__restrict__ size, const uint32_t *__restrict__ stageOff,
                                                               const uint32_t *__restrict__ off, const uint8_t *__restrict__ stage,
                                                               uint8_t *__restrict__ dense)
{
    const uint32_t sz = size[blockIdx.x];
    if (!sz) return;
    const uint32_t bytes = QZSTD_HUF_LENGTHS_BYTES + sz, nWords = (bytes + 15u) >> 4;
    const uint4 *src = reinterpret_cast<const uint4 *>(stage + stageOff[blockIdx.x]);
    uint4 *dst = reinterpret_cast<uint4 *>(dense + off[blockIdx.x]);
    for (uint32_t w = threadIdx.x; w < nWords; w += kHufT) {
        uint4 v = src[w];
        const uint32_t valid = bytes - w * 16u;
        if (valid < 16u) {
            uint32_t d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t nv = valid > 4u * j ? (valid - 4u * j < 4u ? valid - 4u * j : 4u) : 0u;
                d[j] &= nv >= 4u ? 0xFFFFFFFFu : (1u << (8u * nv)) - 1u;
            }
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        dst[w] = v;
    }
}
} // namespace

extern "C" size_t qzstd_hip_huf_code_bytes(const qzstd_hip_plane_row_t *rows, uint32_t nRows)
{
    unsigned long long sum = 0u;
    for (uint32_t i = 0; i < nRows; i++) sum += QZSTD_HIP_HUF_ROW_BYTES(rows[i].len);
    return sum >= 0xFFFFFFF0ull ? (size_t)-1 : (size_t)sum;
}

extern "C" int qzstd_hip_huf_code(int device, void *stream, const void *d_base, const qzstd_hip_plane_row_t *rows, uint32_t nRows,
                                  qzstd_hip_plane_row_t *d_rows, uint32_t *d_cost, uint32_t *d_size, uint32_t *d_off, void *d_dense,
                                  size_t denseBytes, void *d_scratch, size_t scratchBytes)
{
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_cost) return fail_msg("qzstd_hip_huf_code: null pointer");
    if (nRows > 0x7FFFFFFFu) return fail_msg("qzstd_hip_huf_code: too many rows");
    for (uint32_t i = 0; i < nRows; i++) {
        if (rows[i].len > QZSTD_PLANE_LEN_MAX) return fail_msg("qzstd_hip_huf_code: a row longer than 128 KiB");
        if (rows[i].reserved) return fail_msg("qzstd_hip_huf_code: reserved not 0");
        if (rows[i].len && !d_base) return fail_msg("qzstd_hip_huf_code: null base");
    }
    if (!d_size || !d_off || !d_dense || !d_scratch) return fail_msg("qzstd_hip_huf_code: null output");
    if (((uintptr_t)d_dense & 15u) || ((uintptr_t)d_scratch & 15u)) return fail_msg("qzstd_hip_huf_code: dense area or scratch not 16-byte aligned");
    const size_t need = qzstd_hip_huf_code_bytes(rows, nRows);
    if (need == (size_t)-1) return fail_msg("qzstd_hip_huf_code: 4 GiB of rows or more");
    if (denseBytes < need || scratchBytes < QZSTD_HIP_HUF_SCRATCH_BYTES(nRows, need)) return fail_msg("qzstd_hip_huf_code: dense area or scratch too small");
    QZ_SET_DEVICE(device);
    hipStream_t s = (hipStream_t)stream;
    uint32_t *stageOff = static_cast<uint32_t *>(d_scratch);
    uint8_t *stage = static_cast<uint8_t *>(d_scratch) + QZSTD_HIP_HUF_SCRATCH_BYTES(nRows, 0u);
    uint8_t *dense = static_cast<uint8_t *>(d_dense);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D (huf rows)");
    hipLaunchKernelGGL(qzstd_huf_scan_kernel, dim3(1), dim3(kHufT), 0, s, d_rows, static_cast<const uint32_t *>(nullptr), nRows, stageOff);
    QZ_CHECK(hipGetLastError(), "launch qzstd_huf_scan_kernel");
    hipLaunchKernelGGL(qzstd_huf_code_kernel, dim3(nRows), dim3(kHufT), 0, s, static_cast<const uint8_t *>(d_base), d_rows, stageOff, d_cost, d_size, stage);
    QZ_CHECK(hipGetLastError(), "launch qzstd_huf_code_kernel");
    hipLaunchKernelGGL(qzstd_huf_scan_kernel, dim3(1), dim3(kHufT), 0, s, d_rows, d_size, nRows, d_off);
    QZ_CHECK(hipGetLastError(), "launch qzstd_huf_scan_kernel");
    hipLaunchKernelGGL(qzstd_huf_pack_kernel, dim3(nRows), dim3(kHufT), 0, s, d_size, stageOff, d_off, stage, dense);
    QZ_CHECK(hipGetLastError(), "launch qzstd_huf_pack_kernel");
    return 0;
}

/* ---------------------------------------------------------------- fingerprint (include/qzstd_hip_device.h, qzstd_fingerprint.h) -- */
#include "qzstd_fingerprint.h"

namespace {
constexpr uint32_t kFpT = QZSTD_FP_LANES;       /* threads per workgroup: the definition's lanes */
constexpr uint32_t kFpTileLog = QZSTD_FP_TILE_LOG; /* bytes of one row per workgroup: 16 KiB, four 16-byte words per lane */
constexpr uint32_t kFpWords = (1u << kFpTileLog) / 16u / kFpT;
static_assert(kFpT == 256u && kFpWords == 4u && kFpTileLog == kDiffTileLog, "the definition's tile: 256 lanes, four words each");

/* One workgroup per 16 KiB tile of a row, in the tile0 numbering (tile0_row_of).  Lane t fetches
 * the tile's words t, t + 256, t + 512, t + 768 as the comparison fetches its sides — group_fetch: the aligned words that overlap the wanted
 * bytes only, shifted by the row's OWN misalignment — all four before the first round, so that the loads are in flight together; the bytes
 * behind the row's last one are masked to 0 (cmp_mask) before they enter a round.  Then the definition's tree: six steps inside the wave
 * (lane t takes lane t + s by a shuffle; the lanes that are no multiple of 2 s compute a value nobody reads), one word per wave through
 * LDS, and thread 0 does the last two steps and stores the tile's ONE word.  No atomics, nothing is read back. */
__global__ __launch_bounds__(kFpT) void qzstd_fingerprint_kernel(const qzstd_hip_fp_row_t *__restrict__ rows, uint32_t nRows,
                                                                 unsigned long long *__restrict__ tilesOut)
{
    __shared__ uint32_t which;
    __shared__ uint64_t red[kFpT / 64u];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) which = tile0_row_of(rows, nRows);
    __syncthreads();
    const qzstd_hip_fp_row_t row = rows[which];
    const uint64_t at = (uint64_t)(blockIdx.x - row.tile0) << kFpTileLog; /* the tile's first byte in its row */
    if (at >= row.len) return; /* (the whole workgroup; never: rows without a tile share the tile0 of the row behind them) */
    const uint32_t tileBytes = row.len - at < (1u << kFpTileLog) ? (uint32_t)(row.len - at) : 1u << kFpTileLog;
    uint64_t w0[kFpWords], w1[kFpWords];
#pragma unroll
    for (uint32_t k = 0; k < kFpWords; k++) {
        const uint32_t w = tid + k * kFpT;
        w0[k] = w1[k] = 0ull;
        if (w * 16u < tileBytes) {
            const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
            group_fetch(row.src + at + w * 16u, valid, &w0[k], &w1[k]);
            cmp_mask(valid, &w0[k], &w1[k]); /* the row's last word: what lies behind the row reads as 0 */
        }
    }
    uint64_t acc = QZSTD_fpLaneInit(tid);
#pragma unroll
    for (uint32_t k = 0; k < kFpWords; k++)
        if ((tid + k * kFpT) * 16u < tileBytes) acc = QZSTD_fpWord(acc, w0[k], w1[k]);
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint64_t other = __shfl_down(acc, s, 64);
        acc = QZSTD_fpMerge(acc, other);
    }
    if ((tid & 63u) == 0u) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const uint64_t a = QZSTD_fpMerge(red[0], red[1]), b = QZSTD_fpMerge(red[2], red[3]); /* s = 64 */
        tilesOut[blockIdx.x] = QZSTD_fpMerge(a, b);                                          /* s = 128 */
    }
}
} // namespace

extern "C" int qzstd_hip_fingerprint(int device, void *stream, qzstd_hip_fp_row_t *rows, uint32_t nRows, qzstd_hip_fp_row_t *d_rows, uint64_t *d_tiles)
{
    using row_t = qzstd_hip_fp_row_t;
    constexpr const char *who = "qzstd_hip_fingerprint";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles) return refuse(who, "null pointer");
    const auto check = [](const row_t &r, uint32_t) -> const char * { return r.len && !r.src ? "null row" : len_check(r.len); };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, [](const row_t &r) { return QZSTD_HIP_FP_TILES(r.len); }, true, &total)) return -1;
    if (total == 0) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (fingerprint rows)");
    hipLaunchKernelGGL(qzstd_fingerprint_kernel, dim3(total), dim3(kFpT), 0, (hipStream_t)stream, d_rows, nRows,
                       reinterpret_cast<unsigned long long *>(d_tiles));
    QZ_CHECK(hipGetLastError(), "launch qzstd_fingerprint_kernel");
    return 0;
}

/* ---------------------------------------------------------------- fingerprint and comparison from pieces (include/qzstd_hip_device.h) -- */
/* Kernels of their own, as qzstd_group_pieces_kernel is: qzstd_fingerprint_kernel and qzstd_ungroup_cmp_kernel stay what they were.  The
 * way from a content offset to a piece and an address is qzstd_group_pieces_kernel's (pieces_find, pieces_fetch), and so is the reason the
 * piece table stays in device memory: a tile of one-byte pieces has 16384 entries. */
namespace {
/* the pieces of [first, first + count) that hold content bytes c0 and c1 (c0 <= c1, both inside the row) */
__device__ inline void pieces_narrow(const qzstd_hip_group_piece_t *__restrict__ pieces, uint32_t first, uint32_t count, uint32_t c0, uint32_t c1,
                                     uint32_t *lo, uint32_t *hi)
{
    *lo = pieces_find(pieces, first, first + count - 1u, c0);
    *hi = pieces_find(pieces, *lo, first + count - 1u, c1);
}

/* qzstd_fingerprint_kernel over a row's pieces: the search for the row, then one lane narrows the row's pieces to the tile's; a lane's four
 * words come through pieces_fetch (no piece of a launch has a base: the launcher refuses one), all four before the first round; masking,
 * rounds, tree and the store are the neighbour's. */
__global__ __launch_bounds__(kFpT) void qzstd_fingerprint_pieces_kernel(const qzstd_hip_fp_pieces_row_t *__restrict__ rows, uint32_t nRows,
                                                                        const qzstd_hip_group_piece_t *__restrict__ pieces,
                                                                        unsigned long long *__restrict__ tilesOut)
{
    __shared__ uint32_t which, pieceLo, pieceHi;
    __shared__ uint64_t red[kFpT / 64u];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        const uint32_t lo = tile0_row_of(rows, nRows);
        which = lo;
        const qzstd_hip_fp_pieces_row_t rw = rows[lo];
        const uint64_t a = (uint64_t)(blockIdx.x - rw.tile0) << kFpTileLog;
        pieceLo = pieceHi = rw.piece0;
        if (a < rw.len) {
            const uint32_t c0 = (uint32_t)a, c1 = rw.len - c0 < (1u << kFpTileLog) ? rw.len - 1u : c0 + (1u << kFpTileLog) - 1u;
            pieces_narrow(pieces, rw.piece0, rw.nPieces, c0, c1, &pieceLo, &pieceHi);
        }
    }
    __syncthreads();
    const qzstd_hip_fp_pieces_row_t row = rows[which];
    const uint64_t at64 = (uint64_t)(blockIdx.x - row.tile0) << kFpTileLog; /* the tile's first byte in its row */
    if (at64 >= row.len) return; /* (the whole workgroup; never: rows without a tile share the tile0 of the row behind them) */
    const uint32_t at = (uint32_t)at64;
    const uint32_t tileBytes = row.len - at < (1u << kFpTileLog) ? row.len - at : 1u << kFpTileLog;
    const uint32_t pLo = pieceLo, pHi = pieceHi;
    uint64_t w0[kFpWords], w1[kFpWords];
#pragma unroll
    for (uint32_t k = 0; k < kFpWords; k++) {
        const uint32_t w = tid + k * kFpT;
        w0[k] = w1[k] = 0ull;
        if (w * 16u < tileBytes) {
            const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
            const uint32_t c = at + w * 16u;
            pieces_fetch(pieces, pLo == pHi ? pLo : pieces_find(pieces, pLo, pHi, c), c, valid, &w0[k], &w1[k]);
            cmp_mask(valid, &w0[k], &w1[k]); /* the row's last word: what lies behind the row reads as 0 */
        }
    }
    uint64_t acc = QZSTD_fpLaneInit(tid);
#pragma unroll
    for (uint32_t k = 0; k < kFpWords; k++)
        if ((tid + k * kFpT) * 16u < tileBytes) acc = QZSTD_fpWord(acc, w0[k], w1[k]);
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint64_t other = __shfl_down(acc, s, 64);
        acc = QZSTD_fpMerge(acc, other);
    }
    if ((tid & 63u) == 0u) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const uint64_t a = QZSTD_fpMerge(red[0], red[1]), b = QZSTD_fpMerge(red[2], red[3]); /* s = 64 */
        tilesOut[blockIdx.x] = QZSTD_fpMerge(a, b);                                          /* s = 128 */
    }
}

/* qzstd_ungroup_cmp_kernel over a row's pieces: phase A is the neighbour's; before it, one lane narrows the row's pieces to those of the
 * tile's bytes [t0, t1) of u[]; in phase B the two group_fetch of ref and base are ONE pieces_fetch of src ^ base at the content offset. */
__global__ __launch_bounds__(kUngroupT) void qzstd_ungroup_cmp_pieces_kernel(const qzstd_hip_ungroup_cmp_pieces_row_t *__restrict__ rows, uint32_t nRows,
                                                                              const qzstd_hip_group_piece_t *__restrict__ pieces,
                                                                              const uint8_t *__restrict__ stage, uint32_t *__restrict__ tilesOut)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kUngroupLds];
    __shared__ uint32_t which, pieceLo, pieceHi;
    __shared__ uint32_t red[kUngroupT / 64u];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        const uint32_t lo = tile0_row_of(rows, nRows);
        which = lo;
        const qzstd_hip_ungroup_cmp_pieces_row_t rw = rows[lo];
        const uint32_t kl = rw.elem == 8u ? 3u : (rw.elem == 4u ? 2u : (rw.elem == 2u ? 1u : 0u));
        const uint32_t nn = rw.len >> kl, tm = kUngroupTile >> kl;
        const uint32_t nt = nn ? (uint32_t)(((uint64_t)nn + tm - 1u) / tm) : (rw.len ? 1u : 0u);
        const uint32_t tt = blockIdx.x - rw.tile0;
        pieceLo = pieceHi = rw.piece0;
        if (tt < nt) {
            const uint32_t first = tt * tm, elems = nn - first < tm ? nn - first : tm;
            const uint32_t c0 = first << kl, c1 = tt + 1u == nt ? rw.len : (first + elems) << kl; /* (c0 < c1: a tile holds bytes) */
            pieces_narrow(pieces, rw.piece0, rw.nPieces, c0, c1 - 1u, &pieceLo, &pieceHi);
        }
    }
    __syncthreads();
    const qzstd_hip_ungroup_cmp_pieces_row_t row = rows[which];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kUngroupTile >> kLog;
    const uint32_t tiles = n ? (uint32_t)(((uint64_t)n + tileMax - 1u) / tileMax) : (row.len ? 1u : 0u);
    const uint32_t t = blockIdx.x - row.tile0;
    if (t >= tiles) return; /* (the whole workgroup; never: rows without a tile share the tile0 of the row behind them) */
    const bool zero = (row.flags & 1u) != 0u;
    const uint32_t e0 = t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint8_t *stageRow = stage + row.srcOff;
    const uint32_t pLo = pieceLo, pHi = pieceHi;
    if (!zero) ungroup_load(stageRow, n, kLog, e0, tileElems, lds, tid); /* (row is the workgroup's: the branch is uniform) */
    __syncthreads();

    const uint32_t t0 = e0 << kLog, lim = (e0 + tileElems) << kLog; /* the tile's bytes of u[]: what its strips hold (len <= 0xFFFFFFE0) */
    const uint32_t t1 = t + 1u == tiles ? row.len : lim;           /* the tail behind the elements goes with the last tile */
    uint32_t first = kCmpSame;
    for (uint32_t rel = tid * 16u; rel < t1 - t0; rel += kUngroupT * 16u) { /* (t1 - t0 <= 16 KiB + 7: no wrap near 4 GiB) */
        const uint32_t o = t0 + rel, valid = t1 - o < 16u ? t1 - o : 16u;
        uint64_t u0 = 0ull, u1 = 0ull;
        if (!zero) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (o < lim) {
                switch (kLog) {
                case 0u: v = ungroup_word<1u>(lds, n, e0, o); break;
                case 1u: v = ungroup_word<2u>(lds, n, e0, o); break;
                case 2u: v = ungroup_word<4u>(lds, n, e0, o); break;
                default: v = ungroup_word<8u>(lds, n, e0, o); break;
                }
            }
            if (lim - o < valid || o >= lim) { /* the word reaches into the tail: those bytes one by one, from the stage */
                uint32_t d[4] = { v.x, v.y, v.z, v.w };
                for (uint32_t b = o < lim ? lim - o : 0u; b < valid; b++)
                    d[b >> 2] = (d[b >> 2] & ~(0xFFu << ((b & 3u) * 8u))) | ungroup_byte(stageRow, n, kLog, o + b) << ((b & 3u) * 8u);
                v = make_uint4(d[0], d[1], d[2], d[3]);
            }
            u0 = v.x | (uint64_t)v.y << 32;
            u1 = v.z | (uint64_t)v.w << 32;
        }
        uint64_t r0, r1;
        pieces_fetch(pieces, pLo == pHi ? pLo : pieces_find(pieces, pLo, pHi, o), o, valid, &r0, &r1); /* src ^ base */
        u0 ^= r0;
        u1 ^= r1;
        cmp_mask(valid, &u0, &u1); /* the row's last word: what lies behind the row, in the strips' slack and in memory, does not count */
        if (u0 | u1) {
            const uint32_t at = o + (u0 ? (uint32_t)__builtin_ctzll(u0) >> 3 : 8u + ((uint32_t)__builtin_ctzll(u1) >> 3));
            first = at < first ? at : first; /* (a lane's offsets ascend: only its first one is kept) */
        }
    }
#pragma unroll
    for (uint32_t d = 32u; d; d >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)first, (int)d, 64);
        first = other < first ? other : first;
    }
    if ((tid & 63u) == 0u) red[tid >> 6] = first;
    __syncthreads();
    if (tid == 0) {
        uint32_t m = red[0];
#pragma unroll
        for (uint32_t w = 1; w < kUngroupT / 64u; w++) m = red[w] < m ? red[w] : m;
        tilesOut[blockIdx.x] = m;
    }
}
} // namespace

extern "C" int qzstd_hip_fingerprint_pieces(int device, void *stream, qzstd_hip_fp_pieces_row_t *rows, uint32_t nRows, qzstd_hip_fp_pieces_row_t *d_rows,
                                            const qzstd_hip_group_piece_t *pieces, uint32_t nPieces, qzstd_hip_group_piece_t *d_pieces,
                                            uint64_t *d_tiles)
{
    using row_t = qzstd_hip_fp_pieces_row_t;
    constexpr const char *who = "qzstd_hip_fingerprint_pieces";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles) return refuse(who, "null pointer");
    if (nPieces && (!pieces || !d_pieces)) return refuse(who, "null piece table");
    const auto check = [&](const row_t &r, uint32_t) -> const char * {
        if (const char *why = len_check(r.len)) return why;
        return pieces_check(pieces, nPieces, r.piece0, r.nPieces, r.len, true);
    };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, [](const row_t &r) { return QZSTD_HIP_FP_TILES(r.len); }, false, &total)) return -1;
    if (total == 0) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (fingerprint pieces rows)");
    QZ_CHECK(hipMemcpyAsync(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces), hipMemcpyHostToDevice, (hipStream_t)stream),
             "hipMemcpyAsync H2D (fingerprint pieces table)");
    hipLaunchKernelGGL(qzstd_fingerprint_pieces_kernel, dim3(total), dim3(kFpT), 0, (hipStream_t)stream, d_rows, nRows, d_pieces,
                       reinterpret_cast<unsigned long long *>(d_tiles));
    QZ_CHECK(hipGetLastError(), "launch qzstd_fingerprint_pieces_kernel");
    return 0;
}

extern "C" int qzstd_hip_ungroup_cmp_pieces(int device, void *stream, qzstd_hip_ungroup_cmp_pieces_row_t *rows, uint32_t nRows,
                                            qzstd_hip_ungroup_cmp_pieces_row_t *d_rows, const qzstd_hip_group_piece_t *pieces, uint32_t nPieces,
                                            qzstd_hip_group_piece_t *d_pieces, const void *d_stage, size_t stageBytes, uint32_t *d_tiles)
{
    using row_t = qzstd_hip_ungroup_cmp_pieces_row_t;
    constexpr const char *who = "qzstd_hip_ungroup_cmp_pieces";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    if (nPieces && (!pieces || !d_pieces)) return refuse(who, "null piece table");
    uint64_t end = 0;
    const auto check = [&](const row_t &r, uint32_t) -> const char * {
        if (const char *why = elem_check(r.elem)) return why;
        if (r.flags & ~QZSTD_HIP_CMP_ZERO) return "unknown flags";
        if (const char *why = len_check(r.len)) return why;
        if (const char *why = pieces_check(pieces, nPieces, r.piece0, r.nPieces, r.len, false)) return why;
        if (r.flags & QZSTD_HIP_CMP_ZERO) return nullptr; /* a ZERO row's srcOff is not looked at */
        return frame_place(r.srcOff, r.len, d_stage, stageBytes, &end);
    };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, [](const row_t &r) { return QZSTD_HIP_CMP_TILES(r.len, r.elem); }, false, &total)) return -1;
    if (total == 0) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ungroup cmp pieces rows)");
    QZ_CHECK(hipMemcpyAsync(d_pieces, pieces, (size_t)nPieces * sizeof(*pieces), hipMemcpyHostToDevice, (hipStream_t)stream),
             "hipMemcpyAsync H2D (ungroup cmp pieces table)");
    hipLaunchKernelGGL(qzstd_ungroup_cmp_pieces_kernel, dim3(total), dim3(kUngroupT), 0, (hipStream_t)stream, d_rows, nRows, d_pieces,
                       static_cast<const uint8_t *>(d_stage), d_tiles);
    QZ_CHECK(hipGetLastError(), "launch qzstd_ungroup_cmp_pieces_kernel");
    return 0;
}

/* ---------------------------------------------------------------- element differences and their sum (include/qzstd_hip_device.h, qzstd_elemdiff.h) -- */
namespace {
/* the element of K bytes at address a, any alignment: group_fetch's aligned words, the ones that overlap [a, a + K) */
template <uint32_t K> __device__ inline uint64_t ediff_elem_at(uint64_t a)
{
    uint64_t o0, o1;
    group_fetch(a, K, &o0, &o1);
    return K == 8u ? o0 : o0 & ((1ull << (8u * (K & 7u))) - 1ull);
}

/* the 16 source bytes {o1, o0} = 16 / K elements, the element in front of them: each becomes zigzag(x[e] - x[e-1]) in K bytes */
template <uint32_t K> __device__ inline void ediff_word(uint64_t *o0, uint64_t *o1, uint64_t prev)
{
    if constexpr (K == 8u) {
        const uint64_t d0 = *o0 - prev, d1 = *o1 - *o0;
        *o0 = (d0 << 1) ^ (0ull - (d0 >> 63));
        *o1 = (d1 << 1) ^ (0ull - (d1 >> 63));
    } else {
        constexpr uint64_t mask = (1ull << (8u * K)) - 1ull;
        uint64_t in[2] = { *o0, *o1 }, out[2] = { 0ull, 0ull };
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
#pragma unroll
            for (uint32_t e = 0; e < 8u / K; e++) {
                const uint64_t x = (in[h] >> (e * 8u * K)) & mask, d = (x - prev) & mask;
                out[h] |= (((d << 1) ^ (0ull - (d >> (8u * K - 1u)))) & mask) << (e * 8u * K);
                prev = x;
            }
        }
        *o0 = out[0];
        *o1 = out[1];
    }
}

/* the element that ends the 16 bytes {o1, o0}: what the lane behind needs */
template <uint32_t K> __device__ inline uint64_t ediff_last(uint64_t o1) { return K == 8u ? o1 : o1 >> (64u - 8u * K); }

/* phase A of a tile with differences: group_fetch, the differences, group_split.  Every lane runs every round (the shuffle is not under a
 * lane's own condition); a lane without a word in a round fetches nothing.  Lane l of a round holds the word behind lane l - 1's, so the
 * element in front of its own comes from there; the first lane of a wave fetches it (x[-1] = 0 for the row's first word). */
template <uint32_t K> __device__ inline void ediff_phase_a(uint64_t srcTile, uint32_t tileBytes, bool rowStart, uint8_t *lds)
{
    for (uint32_t w0 = 0; w0 * 16u < tileBytes; w0 += kGroupT) {
        const uint32_t w = w0 + threadIdx.x;
        const bool mine = w * 16u < tileBytes;
        uint64_t o0 = 0, o1 = 0;
        if (mine) group_fetch(srcTile + w * 16u, tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u, &o0, &o1);
        uint64_t prev = __shfl_up(ediff_last<K>(o1), 1u, 64);
        if (mine) {
            if ((threadIdx.x & 63u) == 0u) prev = (w == 0u && rowStart) ? 0ull : ediff_elem_at<K>(srcTile + w * 16u - K);
            ediff_word<K>(&o0, &o1, prev);
            group_split<K>(o0, o1, lds, w);
        }
    }
}

/* group_byte for a row of the differencing gather: byte p of the row's grouped layout, of its differences when `diff` */
__device__ inline uint64_t ediff_byte(const qzstd_hip_group_ediff_row_t &row, uint32_t n, uint32_t kLog, bool diff, uint64_t p)
{
    if (p >= row.len) return 0ull;
    if (p >= ((uint64_t)n << kLog)) return group_byte_at(row.src + p); /* the tail */
    const uint32_t j = (uint32_t)p / n, e = (uint32_t)p - j * n;       /* (p < len: 32 bits) */
    const uint64_t at = row.src + ((uint64_t)e << kLog);
    if (!diff) return group_byte_at(at + j);
    uint64_t o0 = 0, o1 = 0;
    switch (kLog) { /* the element alone in a word: the rest of the word's differences are not looked at */
    case 0u: o0 = ediff_elem_at<1u>(at); ediff_word<1u>(&o0, &o1, e ? ediff_elem_at<1u>(at - 1u) : 0ull); break;
    case 1u: o0 = ediff_elem_at<2u>(at); ediff_word<2u>(&o0, &o1, e ? ediff_elem_at<2u>(at - 2u) : 0ull); break;
    case 2u: o0 = ediff_elem_at<4u>(at); ediff_word<4u>(&o0, &o1, e ? ediff_elem_at<4u>(at - 4u) : 0ull); break;
    default: o0 = ediff_elem_at<8u>(at); ediff_word<8u>(&o0, &o1, e ? ediff_elem_at<8u>(at - 8u) : 0ull); break;
    }
    return (o0 >> (j * 8u)) & 0xFFull;
}

/* group_patch over ediff_byte */
__device__ inline void ediff_patch(const qzstd_hip_group_ediff_row_t &row, uint32_t n, uint32_t kLog, bool diff, uint64_t o, uint32_t from,
                                   uint64_t *o0, uint64_t *o1)
{
    *o1 = from > 8u ? *o1 & ((1ull << ((from - 8u) * 8u)) - 1ull) : 0ull;
    if (from < 8u) *o0 = from ? *o0 & ((1ull << (from * 8u)) - 1ull) : 0ull;
    if (o + from >= row.len) return; /* padding only */
    for (uint32_t i = from; i < 16u; i++) {
        const uint64_t b = ediff_byte(row, n, kLog, diff, o + i);
        if (i < 8u) *o0 |= b << (i * 8u); else *o1 |= b << ((i - 8u) * 8u);
    }
}

/* qzstd_group_kernel's tiles and phases — a kernel of its own, as qzstd_group_xor_kernel is, so that qzstd_group_kernel stays what it was.
 * A row without the flag goes through that kernel's phase A; a row with it through ediff_phase_a: B sees a tile of zigzagged differences. */
__global__ __launch_bounds__(kGroupT) void qzstd_group_ediff_kernel(const qzstd_hip_group_ediff_row_t *__restrict__ rows, uint32_t nRows,
                                                                     uint64_t firstTile, uint4 *__restrict__ stage)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kGroupLds];
    __shared__ uint32_t which;
    const uint64_t v = firstTile + blockIdx.x;
    if (threadIdx.x == 0) which = stage_row_of(rows, nRows, &qzstd_hip_group_ediff_row_t::dstOff, v);
    __syncthreads();
    const uint32_t r = which;
    const qzstd_hip_group_ediff_row_t row = rows[r];
    const bool diff = (row.flags & QZSTD_HIP_EDIFF_DIFF) != 0u;
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kGroupTile >> kLog;
    const uint64_t ext = (uint64_t)row.len + row.pad;
    const uint64_t tiles = n ? ((uint64_t)n + tileMax - 1u) / tileMax : (ext ? 1ull : 0ull);
    const uint64_t t = v - ((row.dstOff >> kGroupTileLog) + r);
    if (t >= tiles) return; /* (the whole workgroup) */
    const uint32_t e0 = (uint32_t)t * tileMax;
    const uint32_t tileElems = n - e0 < tileMax ? n - e0 : tileMax;
    const uint32_t tileBytes = tileElems << kLog;
    const uint64_t srcTile = row.src + ((uint64_t)e0 << kLog);

    if (diff) {
        switch (kLog) {
        case 0u: ediff_phase_a<1u>(srcTile, tileBytes, e0 == 0u, lds); break;
        case 1u: ediff_phase_a<2u>(srcTile, tileBytes, e0 == 0u, lds); break;
        case 2u: ediff_phase_a<4u>(srcTile, tileBytes, e0 == 0u, lds); break;
        default: ediff_phase_a<8u>(srcTile, tileBytes, e0 == 0u, lds); break;
        }
    } else {
        for (uint32_t w = threadIdx.x; w * 16u < tileBytes; w += kGroupT) {
            uint64_t o0, o1;
            group_fetch(srcTile + w * 16u, tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u, &o0, &o1);
            switch (kLog) {
            case 0u: group_split<1u>(o0, o1, lds, w); break;
            case 1u: group_split<2u>(o0, o1, lds, w); break;
            case 2u: group_split<4u>(o0, o1, lds, w); break;
            default: group_split<8u>(o0, o1, lds, w); break;
            }
        }
    }
    __syncthreads();

    uint4 *out = stage + (row.dstOff >> 4);
    for (uint32_t j = 0; j < (1u << kLog); j++) {
        const uint64_t planeAt = (uint64_t)j * n + e0; /* row offset of the tile's first element in plane j */
        const uint32_t aj = (uint32_t)planeAt & 15u;
        const uint8_t *plane = lds + j * (tileMax + kGroupSlack);
        /* c: offset from the stage word that holds planeAt; that word itself belongs here only when it starts at planeAt */
        for (uint32_t c = (aj ? 16u : 0u) + threadIdx.x * 16u; c < aj + tileElems; c += kGroupT * 16u) {
            const uint32_t x0 = c - aj, q = x0 & ~15u, sh = x0 & 15u;
            const uint32_t valid = tileElems - x0 < 16u ? tileElems - x0 : 16u;
            const uint64_t o = planeAt + x0;
            const uint4 l = *reinterpret_cast<const uint4 *>(plane + q);
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh) h = *reinterpret_cast<const uint4 *>(plane + q + 16u);
            uint64_t o0, o1;
            group_shift(l, h, sh, &o0, &o1);
            if (valid < 16u) ediff_patch(row, n, kLog, diff, o, valid, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
    if (t + 1u == tiles) {
        const uint64_t tailAt = ((((uint64_t)n << kLog) + 15u) & ~(uint64_t)15u);
        for (uint64_t o = tailAt + threadIdx.x * 16u; o < ext; o += kGroupT * 16u) {
            uint64_t o0 = 0, o1 = 0;
            ediff_patch(row, n, kLog, diff, o, 0u, &o0, &o1);
            out[o >> 4] = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        }
    }
}

/* ---- the sum.  A tile is 16 KiB of a row's elements: 1024 words of 16 bytes, wave v of the four takes words [256 v, 256 v + 256) in
 * four rounds of 64 (round q, lane l: word 256 v + 64 q + l — a wave's load is 1 KiB in a row).  A word holds whole elements: the tile
 * starts at an element, 16 is a multiple of every k. */
constexpr uint32_t kEsumT = 256u;
constexpr uint32_t kEsumTileLog = kGroupTileLog;
constexpr uint32_t kEsumTile = 1u << kEsumTileLog;
constexpr uint32_t kEsumRounds = kEsumTile / 16u / kEsumT;
constexpr uint32_t kEsumScanPer = 8u; /* sums per thread and step of the scan kernel */
static_assert(kEsumRounds == 4u, "four words per lane");

/* the words {o1, o0} = 16 / K zigzagged differences -> their running sums from `sum` on, each in K bytes; returns the sum behind the last
 * (in 64 bits: 2^(8K) divides 2^64, so the low K bytes of every partial sum are exact whatever the order) */
template <uint32_t K> __device__ inline uint64_t esum_word(uint64_t *o0, uint64_t *o1, uint64_t sum)
{
    if constexpr (K == 8u) {
        sum += (*o0 >> 1) ^ (0ull - (*o0 & 1ull));
        *o0 = sum;
        sum += (*o1 >> 1) ^ (0ull - (*o1 & 1ull));
        *o1 = sum;
    } else {
        constexpr uint64_t mask = (1ull << (8u * K)) - 1ull;
        uint64_t in[2] = { *o0, *o1 }, out[2] = { 0ull, 0ull };
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) {
#pragma unroll
            for (uint32_t e = 0; e < 8u / K; e++) {
                const uint64_t z = (in[h] >> (e * 8u * K)) & mask;
                sum += ((z >> 1) ^ (0ull - (z & 1ull))) & mask;
                out[h] |= (sum & mask) << (e * 8u * K);
            }
        }
        *o0 = out[0];
        *o1 = out[1];
    }
    return sum;
}

__device__ inline uint64_t esum_word_k(uint32_t kLog, uint64_t *o0, uint64_t *o1, uint64_t sum)
{
    switch (kLog) {
    case 0u: return esum_word<1u>(o0, o1, sum);
    case 1u: return esum_word<2u>(o0, o1, sum);
    case 2u: return esum_word<4u>(o0, o1, sum);
    default: return esum_word<8u>(o0, o1, sum);
    }
}

/* what both tile kernels start with: the workgroup's row and tile, and the lane's four words of zigzagged differences (0 where the tile
 * has none: unzigzag(0) = 0).  With `heads` the tile's word 0 comes from the copy of pass 1, not from memory. */
struct esum_tile_t {
    qzstd_hip_esum_row_t row;
    uint32_t kLog, tileBytes;
    uint64_t at, rowBytes; /* the tile's first byte in its row; n * k */
    uint64_t z0[kEsumRounds], z1[kEsumRounds];
};

__device__ inline bool esum_tile_load(const qzstd_hip_esum_row_t *__restrict__ rows, uint32_t nRows, const uint4 *__restrict__ heads, uint32_t *which,
                                      esum_tile_t *t)
{
    if (threadIdx.x == 0) *which = tile0_row_of(rows, nRows);
    __syncthreads();
    t->row = rows[*which];
    t->kLog = t->row.elem == 8u ? 3u : (t->row.elem == 4u ? 2u : (t->row.elem == 2u ? 1u : 0u));
    t->rowBytes = (uint64_t)(t->row.len >> t->kLog) << t->kLog;
    t->at = (uint64_t)(blockIdx.x - t->row.tile0) << kEsumTileLog;
    if (t->at >= t->rowBytes) return false; /* (the whole workgroup; never: rows without a tile share the tile0 of the row behind them) */
    t->tileBytes = t->rowBytes - t->at < kEsumTile ? (uint32_t)(t->rowBytes - t->at) : kEsumTile;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t q = 0; q < kEsumRounds; q++) {
        const uint32_t w = wave * (kEsumT * kEsumRounds / 4u) + q * 64u + lane;
        t->z0[q] = t->z1[q] = 0ull;
        if (w * 16u < t->tileBytes) {
            const uint32_t valid = t->tileBytes - w * 16u < 16u ? t->tileBytes - w * 16u : 16u;
            if (heads && w == 0u) {
                const uint4 h = heads[blockIdx.x];
                t->z0[q] = h.x | (uint64_t)h.y << 32;
                t->z1[q] = h.z | (uint64_t)h.w << 32;
            } else {
                group_fetch(t->row.dst + t->at + w * 16u, valid, &t->z0[q], &t->z1[q]);
            }
            cmp_mask(valid, &t->z0[q], &t->z1[q]); /* what lies behind the row's last element reads as 0 */
        }
    }
    return true;
}

/* pass 1: the tile's sum, and its first 16 bytes as they are before anything is summed */
__global__ __launch_bounds__(kEsumT) void qzstd_esum_tile_kernel(const qzstd_hip_esum_row_t *__restrict__ rows, uint32_t nRows, uint4 *__restrict__ heads,
                                                                 unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t which;
    __shared__ uint64_t red[kEsumT / 64u];
    esum_tile_t t;
    if (!esum_tile_load(rows, nRows, nullptr, &which, &t)) return;
    if (threadIdx.x == 0) heads[blockIdx.x] = make_uint4((uint32_t)t.z0[0], (uint32_t)(t.z0[0] >> 32), (uint32_t)t.z1[0], (uint32_t)(t.z1[0] >> 32));
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kEsumRounds; q++) {
        uint64_t a = t.z0[q], b = t.z1[q];
        sum = esum_word_k(t.kLog, &a, &b, sum);
    }
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) sum += __shfl_xor(sum, (int)s, 64);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

/* pass 2: sums[i] <- sums[0] + .. + sums[i-1], in place, by ONE workgroup: kEsumT * kEsumScanPer of them a step */
__global__ __launch_bounds__(kEsumT) void qzstd_esum_scan_kernel(unsigned long long *__restrict__ sums, uint32_t total)
{
    __shared__ uint64_t red[kEsumT / 64u];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t carry = 0;
    for (uint32_t c = 0; c < total; c += kEsumT * kEsumScanPer) {
        const uint32_t i0 = c + threadIdx.x * kEsumScanPer;
        uint64_t v[kEsumScanPer], mine = 0;
#pragma unroll
        for (uint32_t i = 0; i < kEsumScanPer; i++) {
            v[i] = i0 + i < total ? sums[i0 + i] : 0ull;
            mine += v[i];
        }
        uint64_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63u) red[wave] = incl;
        __syncthreads();
        uint64_t before = carry, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kEsumT / 64u; w++) {
            if (w < wave) before += red[w];
            all += red[w];
        }
        __syncthreads(); /* red is rewritten by the next step */
        uint64_t run = before + incl - mine;
#pragma unroll
        for (uint32_t i = 0; i < kEsumScanPer; i++) {
            if (i0 + i < total) sums[i0 + i] = run;
            run += v[i];
        }
        carry += all;
    }
}

/* pass 3: see include/qzstd_hip_device.h.  `sums` holds the exclusive prefix sums of pass 2. */
__global__ __launch_bounds__(kEsumT) void qzstd_esum_apply_kernel(const qzstd_hip_esum_row_t *__restrict__ rows, uint32_t nRows, const uint4 *__restrict__ heads,
                                                                  const unsigned long long *__restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kEsumTile + 32u];
    __shared__ uint32_t which;
    __shared__ uint64_t red[kEsumT / 64u];
    esum_tile_t t;
    if (!esum_tile_load(rows, nRows, heads, &which, &t)) return;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    /* the lane's words' sums, a wave scan of them per round, the rounds chained through lane 63 */
    uint64_t excl[kEsumRounds], waveSum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kEsumRounds; q++) {
        uint64_t a = t.z0[q], b = t.z1[q];
        const uint64_t mine = esum_word_k(t.kLog, &a, &b, 0ull);
        uint64_t incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        excl[q] = waveSum + incl - mine;
        waveSum += __shfl(incl, 63, 64);
    }
    if (lane == 0u) red[wave] = waveSum;
    __syncthreads();
    uint64_t carry = sums[blockIdx.x] - sums[t.row.tile0], tileSum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kEsumT / 64u; w++) {
        if (w < wave) carry += red[w];
        tileSum += red[w];
    }
#pragma unroll
    for (uint32_t q = 0; q < kEsumRounds; q++) {
        const uint32_t w = wave * (kEsumT * kEsumRounds / 4u) + q * 64u + lane;
        if (w * 16u < t.tileBytes) {
            (void)esum_word_k(t.kLog, &t.z0[q], &t.z1[q], carry + excl[q]);
            *reinterpret_cast<uint4 *>(lds + w * 16u) = make_uint4((uint32_t)t.z0[q], (uint32_t)(t.z0[q] >> 32), (uint32_t)t.z1[q], (uint32_t)(t.z1[q] >> 32));
        }
    }
    /* the elements of the next tile that complete this tile's last destination word: up to 16 bytes, whole elements, from pass 1's copy */
    if (threadIdx.x == 0 && t.at + t.tileBytes < t.rowBytes) { /* (the tile is a whole one: tileBytes = 16 KiB) */
        const uint64_t left = t.rowBytes - t.at - t.tileBytes;
        const uint4 h = heads[blockIdx.x + 1u];
        uint64_t a = h.x | (uint64_t)h.y << 32, b = h.z | (uint64_t)h.w << 32;
        cmp_mask(left < 16u ? (uint32_t)left : 16u, &a, &b);
        (void)esum_word_k(t.kLog, &a, &b, sums[blockIdx.x] - sums[t.row.tile0] + tileSum);
        *reinterpret_cast<uint4 *>(lds + kEsumTile) = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
    __syncthreads();
    /* the destination's 16-byte slots whose first byte inside the row lies in this tile */
    const uint64_t rowEnd = t.row.dst + t.rowBytes, tileAt = t.row.dst + t.at, tileEnd = tileAt + t.tileBytes;
    const uint64_t first = t.at ? (tileAt + 15u) & ~(uint64_t)15u : tileAt & ~(uint64_t)15u;
    for (uint64_t s = first + threadIdx.x * 16u; s < tileEnd; s += kEsumT * 16u) {
        const uint64_t lo = s < t.row.dst ? t.row.dst : s, hi = s + 16u > rowEnd ? rowEnd : s + 16u;
        if (lo == s && hi == s + 16u) {
            const uint32_t off = (uint32_t)(s - tileAt), q = off & ~15u, sh = off & 15u;
            const uint4 l = *reinterpret_cast<const uint4 *>(lds + q);
            uint4 h = make_uint4(0u, 0u, 0u, 0u);
            if (sh) h = *reinterpret_cast<const uint4 *>(lds + q + 16u);
            uint64_t o0, o1;
            group_shift(l, h, sh, &o0, &o1);
            *reinterpret_cast<uint4 *>(s) = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
        } else {
            for (uint64_t b = lo; b < hi; b++) *reinterpret_cast<uint8_t *>(b) = lds[b - tileAt];
        }
    }
}
} // namespace

extern "C" int qzstd_hip_group_ediff(int device, void *stream, const qzstd_hip_group_ediff_row_t *rows, uint32_t nRows,
                                     qzstd_hip_group_ediff_row_t *d_rows, void *d_stage, size_t stageBytes)
{
    constexpr const char *who = "qzstd_hip_group_ediff";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_stage || ((uintptr_t)d_stage & 15u)) return refuse(who, "null pointer or stage not 16-byte aligned");
    const auto own = [](const qzstd_hip_group_ediff_row_t &r) {
        return row_own_t{ r.flags & ~QZSTD_HIP_EDIFF_DIFF ? "unknown flags" : nullptr, r.len && !r.src ? "null source" : nullptr, nullptr };
    };
    stage_launch_t go;
    if (group_rows_check(who, rows, nRows, stageBytes, own, &go)) return -1;
    if (!go.tiles) return 0; /* nothing but empty rows */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (group ediff rows)");
    hipLaunchKernelGGL(qzstd_group_ediff_kernel, dim3(go.tiles), dim3(kGroupT), 0, (hipStream_t)stream, d_rows, nRows, go.firstTile,
                       static_cast<uint4 *>(d_stage));
    QZ_CHECK(hipGetLastError(), "launch qzstd_group_ediff_kernel");
    return 0;
}

namespace {
/* the element sum's and the element-difference cost's rows: `mem` is the row's address, needed when the row has an element */
inline const char *elems_row_check(uint32_t elem, uint32_t reserved, uint32_t len, uint64_t mem)
{
    if (const char *why = elem_check(elem)) return why;
    if (reserved) return "reserved not 0";
    if (const char *why = len_check(len)) return why;
    return len >= elem && !mem ? "null row" : nullptr;
}
} // namespace

extern "C" int qzstd_hip_esum(int device, void *stream, qzstd_hip_esum_row_t *rows, uint32_t nRows, qzstd_hip_esum_row_t *d_rows, void *d_scratch,
                              size_t scratchBytes)
{
    using row_t = qzstd_hip_esum_row_t;
    constexpr const char *who = "qzstd_hip_esum";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_scratch || ((uintptr_t)d_scratch & 15u)) return refuse(who, "null pointer or scratch not 16-byte aligned");
    const auto check = [](const row_t &r, uint32_t) { return elems_row_check(r.elem, r.reserved, r.len, r.dst); };
    const auto tilesOf = [](const row_t &r) { return QZSTD_HIP_ESUM_TILES(r.len, r.elem); };
    uint32_t tiles;
    /* (tile0_rows's steps, with the scratch held against the count before anything is written) */
    if (tile0_count(who, rows, nRows, check, tilesOf, &tiles)) return -1;
    if (QZSTD_HIP_ESUM_SCRATCH_BYTES(tiles) > scratchBytes) return refuse(who, "scratch too small");
    if (tiles == 0) return 0; /* no row with an element */
    tile0_write(rows, nRows, tilesOf);
    QZ_SET_DEVICE(device);
    const hipStream_t s = (hipStream_t)stream;
    auto *heads = static_cast<uint4 *>(d_scratch);
    auto *sums = reinterpret_cast<unsigned long long *>(heads + tiles);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D (esum rows)");
    hipLaunchKernelGGL(qzstd_esum_tile_kernel, dim3(tiles), dim3(kEsumT), 0, s, d_rows, nRows, heads, sums);
    QZ_CHECK(hipGetLastError(), "launch qzstd_esum_tile_kernel");
    hipLaunchKernelGGL(qzstd_esum_scan_kernel, dim3(1), dim3(kEsumT), 0, s, sums, tiles);
    QZ_CHECK(hipGetLastError(), "launch qzstd_esum_scan_kernel");
    hipLaunchKernelGGL(qzstd_esum_apply_kernel, dim3(tiles), dim3(kEsumT), 0, s, d_rows, nRows, heads, sums);
    QZ_CHECK(hipGetLastError(), "launch qzstd_esum_apply_kernel");
    return 0;
}

/* ---------------------------------------------------------------- element-difference cost (include/qzstd_hip_device.h, qzstd_ediffcost.h) -- */
#include "qzstd_ediffcost.h"

namespace {
constexpr uint32_t kEcT = 256u;                          /* threads per workgroup: one per bin in the reduction */
constexpr uint32_t kEcTile = 1u << kGroupTileLog;        /* bytes of a row's elements per workgroup: 16 KiB, four 16-byte words per lane */
constexpr uint32_t kEcRounds = kEcTile / 16u / kEcT;
constexpr uint32_t kEcWords = 2u * 256u * 16u;           /* LDS words: 2 K histograms of 256 bins in 16 / K copies each — 32 KiB for every K:
                                                            four workgroups a CU. Bin b of histogram h, copy c: word (h * 256 + b) * (16 / K) + c */
static_assert(kEcTile == QZSTD_EDIFF_TILE && kEcRounds == 4u, "the definition's tile: 256 lanes, four words each");
static_assert(QZSTD_EDIFF_TILES(16385u, 2u) == QZSTD_HIP_ESUM_TILES(16385u, 2u) && QZSTD_EDIFF_TILES(7u, 8u) == QZSTD_HIP_ESUM_TILES(7u, 8u),
              "one tile rule");

/* the K low bytes of x, repeated over 8 bytes */
template <uint32_t K> __device__ inline uint64_t ec_repeat(uint64_t x)
{
    if constexpr (K == 8u) return x;
    else if constexpr (K == 4u) return (x & 0xFFFFFFFFull) * 0x0000000100000001ull;
    else if constexpr (K == 2u) return (x & 0xFFFFull) * 0x0001000100010001ull;
    else return (x & 0xFFull) * 0x0101010101010101ull;
}

/* One side's 16 bytes {o1, o0} = 16 / K elements into that side's K histograms (`mine`: the side's first word plus the lane's copy).
 * Every lane of the wave calls it.  Per plane the wave first asks whether ALL its bytes of the plane equal the first lane's (an XOR with
 * that lane's first element repeated, OR-ed down to K bytes, one vote): then lane 0 adds the wave's element count to that one bin — the
 * zero planes of small differences and the constant upper bytes of a column would otherwise put 64 lanes on one word, four times a round
 * for K = 4.  Otherwise every lane adds its own bytes, on its copy.  `valid`: the lane's bytes that count (a multiple of K; 0 for a lane
 * without a word, whose o0 and o1 are 0); the bytes behind them are 0 and are not counted. */
template <uint32_t K> __device__ inline void ec_count(uint32_t *mine, uint64_t o0, uint64_t o1, uint32_t valid, uint32_t waveElems)
{
    constexpr uint32_t C = 16u / K;
    const uint64_t first = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o0) |
                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o0 >> 32)) << 32;
    const uint64_t R = ec_repeat<K>(first);
    uint64_t t = valid ? (o0 ^ R) | (o1 ^ R) : 0ull;
    if constexpr (K <= 4u) t |= t >> 32;
    if constexpr (K <= 2u) t |= t >> 16;
    if constexpr (K == 1u) t |= t >> 8;
#pragma unroll
    for (uint32_t j = 0; j < K; j++) {
        if (!__any((int)((uint32_t)(t >> (8u * j)) & 0xFFu))) { /* (the same answer in every lane) */
            if ((threadIdx.x & 63u) == 0u && waveElems) atomicAdd(&mine[(j * 256u + ((uint32_t)(R >> (8u * j)) & 0xFFu)) * C], waveElems);
        } else if (valid == 16u) {
#pragma unroll
            for (uint32_t e = 0; e < C; e++) {
                const uint32_t i = e * K + j;
                atomicAdd(&mine[(j * 256u + ((uint32_t)(i < 8u ? o0 >> (i * 8u) : o1 >> ((i - 8u) * 8u)) & 0xFFu)) * C], 1u);
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < C; e++) {
                const uint32_t i = e * K + j;
                if (i < valid) atomicAdd(&mine[(j * 256u + ((uint32_t)(i < 8u ? o0 >> (i * 8u) : o1 >> ((i - 8u) * 8u)) & 0xFFu)) * C], 1u);
            }
        }
    }
}

/* A tile of `tileBytes` bytes (whole elements) at srcTile -> its two words.  Lane t takes the tile's words t, t + 256, t + 512, t + 768,
 * fetched as the differencing gather fetches its source (group_fetch: the aligned words that overlap the wanted bytes only, shifted by the
 * row's OWN misalignment), all four before the first is counted, so that the loads are in flight together; the bytes behind the tile's
 * last element are masked to 0 (cmp_mask) and never counted.  The element in front of a lane's word comes from the lane before it by a
 * shuffle that every lane executes; a wave's first lane fetches it (ediff_elem_at), or takes 0 at the row's start — ediff_phase_a's rule.
 * Then bin t of every histogram: its copies summed, QZSTD_planeTerm, a sum over the wave (xor shuffles) and the four waves (one LDS step),
 * QZSTD_planeCostOfSum per plane, and thread 0 stores the two words with one 8-byte store. */
template <uint32_t K> __device__ inline void ec_tile(uint64_t srcTile, uint32_t tileBytes, bool rowStart, uint32_t *hist, uint32_t (*red)[kEcT / 64u],
                                                     uint2 *out)
{
    constexpr uint32_t C = 16u / K;
    const uint32_t tid = threadIdx.x;
    uint64_t x0[kEcRounds], x1[kEcRounds], front[kEcRounds];
#pragma unroll
    for (uint32_t q = 0; q < kEcRounds; q++) {
        const uint32_t w = q * kEcT + tid;
        x0[q] = x1[q] = front[q] = 0ull;
        if (w * 16u < tileBytes) {
            const uint32_t valid = tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u;
            group_fetch(srcTile + w * 16u, valid, &x0[q], &x1[q]);
            cmp_mask(valid, &x0[q], &x1[q]);
            if ((tid & 63u) == 0u && !(w == 0u && rowStart)) front[q] = ediff_elem_at<K>(srcTile + w * 16u - K);
        }
    }
    uint32_t *mineX = hist + (tid & (C - 1u)), *mineZ = mineX + K * 256u * C;
#pragma unroll
    for (uint32_t q = 0; q < kEcRounds; q++) {
        const uint32_t w = q * kEcT + tid, wave0 = w & ~63u;
        const uint32_t valid = w * 16u < tileBytes ? (tileBytes - w * 16u < 16u ? tileBytes - w * 16u : 16u) : 0u;
        const uint32_t waveBytes = wave0 * 16u < tileBytes ? (tileBytes - wave0 * 16u < 1024u ? tileBytes - wave0 * 16u : 1024u) : 0u;
        uint64_t prev = __shfl_up(ediff_last<K>(x1[q]), 1u, 64);
        if ((tid & 63u) == 0u) prev = front[q];
        uint64_t z0 = x0[q], z1 = x1[q];
        ediff_word<K>(&z0, &z1, prev);
        cmp_mask(valid, &z0, &z1);
        if (valid == 0u) z0 = z1 = 0ull;
        ec_count<K>(mineX, x0[q], x1[q], valid, waveBytes / K);
        ec_count<K>(mineZ, z0, z1, valid, waveBytes / K);
    }
    __syncthreads();
    const uint32_t Lm = QZSTD_planeLog2(tileBytes / K);
#pragma unroll
    for (uint32_t h = 0; h < 2u * K; h++) {
        const uint32_t *bin = &hist[(h * 256u + tid) * C];
        uint32_t c = 0u;
        if constexpr (C == 2u) {
            const uint2 v = *reinterpret_cast<const uint2 *>(bin);
            c = v.x + v.y;
        } else {
#pragma unroll
            for (uint32_t v4 = 0; v4 < C / 4u; v4++) {
                const uint4 v = reinterpret_cast<const uint4 *>(bin)[v4];
                c += v.x + v.y + v.z + v.w;
            }
        }
        uint32_t sum = QZSTD_planeTerm(c, Lm); /* (a plane's terms: at most m * L(m) < 2^26) */
#pragma unroll
        for (uint32_t s = 32u; s; s >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)s, 64);
        if ((tid & 63u) == 0u) red[h][tid >> 6] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t cost[2] = { 0u, 0u };
#pragma unroll
        for (uint32_t h = 0; h < 2u * K; h++) cost[h / K] += QZSTD_planeCostOfSum(red[h][0] + red[h][1] + red[h][2] + red[h][3]);
        *out = make_uint2(cost[0], cost[1]);
    }
}

/* One workgroup per tile of a row's elements, in the tile0 numbering (tile0_row_of).  No atomics but the LDS ones; nothing is read back. */
__global__ __launch_bounds__(kEcT) void qzstd_ediff_cost_kernel(const qzstd_hip_ediff_cost_row_t *__restrict__ rows, uint32_t nRows,
                                                                uint2 *__restrict__ tilesOut)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[kEcWords];
    __shared__ uint32_t red[16][kEcT / 64u];
    __shared__ uint32_t which;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) which = tile0_row_of(rows, nRows);
    for (uint32_t i = tid; i < kEcWords / 4u; i += kEcT) reinterpret_cast<uint4 *>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const qzstd_hip_ediff_cost_row_t row = rows[which];
    const uint32_t kLog = row.elem == 8u ? 3u : (row.elem == 4u ? 2u : (row.elem == 2u ? 1u : 0u));
    const uint32_t n = row.len >> kLog, tileMax = kEcTile >> kLog;
    const uint64_t e0 = (uint64_t)(blockIdx.x - row.tile0) * tileMax; /* the tile's first element in its row */
    if (e0 >= n) return; /* (the whole workgroup; never: rows without a tile are not found, tile0_row_of) */
    const uint32_t tileBytes = (n - (uint32_t)e0 < tileMax ? n - (uint32_t)e0 : tileMax) << kLog;
    const uint64_t srcTile = row.src + (e0 << kLog);
    uint2 *out = tilesOut + blockIdx.x;
    switch (kLog) {
    case 0u: ec_tile<1u>(srcTile, tileBytes, e0 == 0u, hist, red, out); break;
    case 1u: ec_tile<2u>(srcTile, tileBytes, e0 == 0u, hist, red, out); break;
    case 2u: ec_tile<4u>(srcTile, tileBytes, e0 == 0u, hist, red, out); break;
    default: ec_tile<8u>(srcTile, tileBytes, e0 == 0u, hist, red, out); break;
    }
}
} // namespace

extern "C" int qzstd_hip_ediff_cost(int device, void *stream, qzstd_hip_ediff_cost_row_t *rows, uint32_t nRows, qzstd_hip_ediff_cost_row_t *d_rows,
                                    uint32_t *d_tiles)
{
    using row_t = qzstd_hip_ediff_cost_row_t;
    constexpr const char *who = "qzstd_hip_ediff_cost";
    if (nRows == 0) return 0;
    if (!rows || !d_rows || !d_tiles || ((uintptr_t)d_tiles & 7u)) return refuse(who, "null pointer or tiles not 8-byte aligned");
    const auto check = [](const row_t &r, uint32_t) { return elems_row_check(r.elem, r.reserved, r.len, r.src); };
    uint32_t total;
    if (tile0_rows(who, rows, nRows, check, [](const row_t &r) { return QZSTD_HIP_ESUM_TILES(r.len, r.elem); }, true, &total)) return -1;
    if (total == 0) return 0; /* no row with an element */
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(d_rows, rows, (size_t)nRows * sizeof(*rows), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D (ediff cost rows)");
    hipLaunchKernelGGL(qzstd_ediff_cost_kernel, dim3(total), dim3(kEcT), 0, (hipStream_t)stream, d_rows, nRows,
                       reinterpret_cast<uint2 *>(d_tiles));
    QZ_CHECK(hipGetLastError(), "launch qzstd_ediff_cost_kernel");
    return 0;
}
