/*
 * mock_fail_block.c — TEST INFRASTRUCTURE ONLY.  A matcher error on demand for the CPU stand-in of tests/mock/mock_hip.c: this file provides
 * qzstd_hip_find_sequences for the whole mock library — the host path and the front-end alike — as mock_hip.c's own, followed by the block
 * that qzstd_mock_fail_block() names, if any, reported as failed (its count QZSTD_HIP_NSEQ_ERROR).  A mock that wants it compiles mock_hip.c
 * ALONE with -Dqzstd_hip_find_sequences=qzstd_mock_find_sequences_inner, so that its match-finder carries that name, and links this file in;
 * no other source is built with the define.
 */
#include "qzstd_hip.h"

#include <stdint.h>

int qzstd_mock_find_sequences_inner(int device, void *stream, int level, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                                    uint32_t maxBlockLen, void *d_seqs, uint32_t *d_nseq, void *d_work, size_t workBytes);

static int gFailBlock = -1;
/* test hook: block `b` of every launch from now on comes back failed (-1: none) */
void qzstd_mock_fail_block(int b) { gFailBlock = b; }

int qzstd_hip_find_sequences(int device, void *stream, int level, const void *d_src, const qzstd_hip_block_t *d_blocks, uint32_t nBlocks,
                             uint32_t maxBlockLen, void *d_seqs, uint32_t *d_nseq, void *d_work, size_t workBytes)
{
    const int rc = qzstd_mock_find_sequences_inner(device, stream, level, d_src, d_blocks, nBlocks, maxBlockLen, d_seqs, d_nseq, d_work, workBytes);
    if (rc == 0 && gFailBlock >= 0 && (uint32_t)gFailBlock < nBlocks) d_nseq[gFailBlock] = QZSTD_HIP_NSEQ_ERROR;
    return rc;
}
