/* ape_lz4f_placed.h -- LZ4 frames whose blocks may be short: the decoded size of a block without
 * decoding it, and a framed decode that sizes every block first and then decodes each where it
 * belongs.  A stand-alone part of the batched GPU API: it includes ape_lz4f.h, is included by
 * nothing, and keeps that header's conventions -- device pointers, asynchronous on `stream`, no
 * allocation, no synchronisation, graph-capturable, a number of launches fixed on the host,
 * APE_LZ4_GPU_OK or a negative APE_LZ4_GPU_E* code.  Every call checks its arguments
 * (APE_LZ4_GPU_EINVAL) before it looks for a device, and a batch of 0 launches nothing and may
 * pass null arrays and a null scratch.
 *
 * Why: APE_LZ4_lz4f_decompress_batch_dev places block q at q x block maximum, which holds for
 * LZ4F_compressFrame and the lz4 tool but not for a streaming producer that flushes
 * (LZ4F_compressUpdate + LZ4F_flush, python-lz4's and lz4-java's flush(), Kafka's record
 * batches): those frames are well-formed and have short blocks in the middle.
 * tests/lz4fplacedmodel.py defines the codes; DESIGN.md 3.24 has the launch list. */
#pragma once
#include <stddef.h>

#include "ape_lz4f.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* d_result[i] = the value APE_LZ4_decompress_safe(d_src[i], dst, d_srcSize[i], d_dstCap[i])
 * returns -- the decoded size, or the reference's -(ip)-1 -- and, with d_dictSize, the value
 * APE_LZ4_decompress_safe_usingDict returns with a dictionary of d_dictSize[i] bytes (the
 * dictionary's bytes do not matter to it, only how far back an offset may reach).  A dry run
 * of the decoder's parse: there is no destination, and nothing but d_result is written.  Of
 * d_src[i] the bytes [0, d_srcSize[i]) are read (byte 0 also where the size is not positive,
 * as the reference does).  One launch, one wave per block.
 * EINVAL: a null d_src, d_srcSize, d_dstCap or d_result with n > 0, n < 0. */
int APE_LZ4_decompress_safe_size_batch_dev(const char *const *d_src, const int *d_srcSize,
                                           const int *d_dstCap,
                                           const int *d_dictSize /* may be null */,
                                           int *d_result, int n, void *stream);

/* ---- decode, blocks of any size ----
 * The arguments and flags of APE_LZ4_lz4f_decompress_batch_dev (1 = do not verify checksums,
 * 2 = the batch has no block-linked frame), and the frames it accepts WITHOUT the full-block
 * rule: a block may decode to any size from 0 to the block maximum.
 * d_result[f]: the decoded size, or the first of these that applies:
 *   -1, -3, -2, APE_LZ4_GPU_ERANGE   the header stage, as in ape_lz4f.h
 *   -4  a block has no decoded size (a dry run with the block maximum as capacity fails)
 *   -9  d_dstCap[f] below the sum of the blocks' decoded sizes
 *   -8  content size mismatch
 *   -6  block checksum
 *   -4  a block fails to decode into exactly its decoded size, or a match of a linked block
 *       reaches back before the frame's start
 *   -7  content checksum
 * -9 is judged against what the blocks decode to, not against blocks x maximum: a flushed
 * frame of 1000 small blocks needs a destination of its content's size.  The first -4, -9 and
 * -8 are decided before a byte of d_dst[f] is written, and such a frame writes nothing.  -5
 * does not occur.  A frame's trouble never touches another frame; nothing outside
 * d_dst[f][0, d_dstCap[f]) is written.
 * placed_scratch_size: bytes of d_scratch (16-byte aligned) for nframes frames of up to
 *   maxBlocks (>= 1) blocks: 96 bytes per block, 36 per frame; 0 for arguments out of range,
 *   (size_t)-1 from 2^24 blocks on.  What the scratch held is never read.  maxBlocks sets the
 *   scratch and also the length of the chained launch, in which one wave per frame walks
 *   maxBlocks slots in order.
 * Launches: plan, size, place, stored copies, decode, chained decode (without flag 2), hash
 * (without flag 1), finish.
 * EINVAL: a null array or scratch with nframes > 0, nframes < 0, maxBlocks < 1, flags outside
 * 0..3, 2^24 blocks or more, a scratch that is too small or not 16-byte aligned. */
size_t APE_LZ4_lz4f_decompress_placed_scratch_size(int nframes, int maxBlocks);
int APE_LZ4_lz4f_decompress_placed_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nframes, int maxBlocks, int flags,
                                             void *d_scratch, size_t scratch_bytes, void *stream);

#if defined(__cplusplus)
}
#endif
