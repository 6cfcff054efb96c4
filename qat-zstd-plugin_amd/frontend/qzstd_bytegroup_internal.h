/* qzstd_bytegroup_internal.h — what qzstd_frontend.c and the tests' stand-alone driver share with qzstd_bytegroup.c; not installed */
#ifndef QZSTD_BYTEGROUP_INTERNAL_H
#define QZSTD_BYTEGROUP_INTERNAL_H

#include <stddef.h>

/* one unpacked entry: four unsigned values — offset, litLength, matchLength, rep (not looked at) — which is ZSTD_Sequence's layout, without
 * its header.  offset 0 and matchLength 0: a block delimiter, litLength the block's last literals */
#define QZBG_ENTRY_WORDS 4u

/* Executes one frame's entries (delimiters included) and literal bytes into out[0, L): the frame's content, block after block, each block
 * matched on its own (an offset never reaches in front of its block).  ends[0 .. nEnds): the block ends (QZSTD_byteGroupBlocks).
 * Returns 0, or non-zero — having written nothing outside out[0, L) and read nothing outside lit[0, nLit) — when the entries need more
 * literals than there are, produce a byte past a block's end or past L, hold an offset of 0 with a match or one beyond the bytes produced
 * in its block, or when a block does not end exactly on its delimiter (one missing, one too many, one early). */
int qzbgRebuild(unsigned char *out, size_t L, const unsigned *seqs, size_t nSeqs, const unsigned char *lit, size_t nLit,
                const size_t *ends, size_t nEnds);

#endif /* QZSTD_BYTEGROUP_INTERNAL_H */
