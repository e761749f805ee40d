/* ape_lz4f.h -- the LZ4 frame format on the GPU: XXH32 over a batch of streams, framed
 * compress and framed decode.  A stand-alone part of the batched GPU API: it includes
 * ape_lz4_gpu.h for the return codes and keeps its conventions -- device pointers, asynchronous
 * on `stream`, no allocation, no synchronisation, graph-capturable, a number of launches fixed
 * on the host, APE_LZ4_GPU_OK or a negative APE_LZ4_GPU_E* code.  Every call checks its
 * arguments (APE_LZ4_GPU_EINVAL) before it looks for a device, and a batch of 0 launches
 * nothing and may pass null arrays and a null scratch.
 *
 * The frame: magic 0x184D2204, FLG (version 01, block independence, block checksums, content
 * size, content checksum, dictionary ID), BD (block-size ID 4..7 = 64 KiB, 256 KiB, 1 MiB,
 * 4 MiB), the optional fields, a header checksum ((XXH32 of the descriptor >> 8) & 255), then
 * blocks [le32 size, bit 31 = stored][bytes][XXH32 of those bytes, with block checksums], an
 * end mark of four zero bytes and, with a content checksum, XXH32 of the content.  That is what
 * liblz4's LZ4F_*, the lz4 tool and python-lz4 read and write.  tests/lz4fmodel.py defines the
 * bytes these calls write and the codes they return; DESIGN.md 3.23 has the launch lists. */
#pragma once
#include <stddef.h>

#include "ape_lz4_gpu.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* d_hash[i] = XXH32, with `seed`, of the max(d_size[i], 0) bytes at d_src[i]: any alignment, any
 * size up to 2^31 - 1, nothing read outside those bytes (d_src[i] may be null where the size is
 * not positive).  One launch, 16 streams per wave; a stream is a serial chain, so one long
 * stream runs at one lane's rate however many there are.
 * EINVAL: a null array with n > 0, n < 0. */
int APE_LZ4_xxh32_batch_dev(const char *const *d_src, const int *d_size, unsigned seed,
                            unsigned *d_hash, int n, void *stream);

/* ---- compress ----
 * flags: 1 = content checksum, 2 = block checksums, 4 = write the content size.
 * Frame f holds d_src[f][0, d_srcSize[f]) as ceil(n / 65536) block-independent blocks of 65536
 * bytes (the last shorter) at block-size ID 4, version 01, no dictionary ID.  A block is
 * APE_LZ4_compress_batch_dev's bytes when they take at most blockBytes - 1 (liblz4's rule),
 * else it is stored.  The frame is a pure function of (input, flags).
 * d_result[f]: the frame's bytes; 0 when that exceeds d_dstCap[f] (nothing of d_dst[f] is
 * written then: the size is known before the first byte goes out) or d_srcSize[f] < 0;
 * APE_LZ4_GPU_ERANGE when d_srcSize[f] > maxSrcSize.  Nothing outside d_dst[f][0, d_dstCap[f])
 * is written.
 * compress_bound: host only, the exact worst case (every block stored); 0 for srcSize outside
 *   0..0x7E000000 or flags outside 0..7.
 * compress_scratch_size: bytes of d_scratch (16-byte aligned) for nframes frames of up to
 *   maxSrcSize (0..0x7E000000) bytes: a 64 KiB slot and 36 bytes of arrays per block, 8 bytes
 *   per frame; 0 for arguments out of range, (size_t)-1 from 2^24 blocks on.  What the scratch
 *   held is never read.
 * Launches: plan, encode, layout, hash (with flags & 3), pack.
 * EINVAL: a null array or scratch with nframes > 0, nframes < 0, maxSrcSize or flags out of
 * range, 2^24 blocks or more, a scratch that is too small or not 16-byte aligned. */
size_t APE_LZ4_lz4f_compress_bound(int srcSize, int flags);
size_t APE_LZ4_lz4f_compress_scratch_size(int nframes, int maxSrcSize);
int APE_LZ4_lz4f_compress_batch_dev(const char *const *d_src, const int *d_srcSize,
                                    char *const *d_dst, const int *d_dstCap, int *d_result,
                                    int nframes, int maxSrcSize, int flags, void *d_scratch,
                                    size_t scratch_bytes, void *stream);

/* ---- what a frame is, without decoding it ----
 * d_info[8 f .. 8 f + 7]: [0] 0 or the decoder's code of the header stage (-1, -3, -2 below;
 * the other seven are then 0, 0, 0, 0, 0, -1, -1), [1] FLG, [2] the block maximum, [3] blocks,
 * [4] the frame's bytes including a trailing checksum, [5] the decoded bound (the content size
 * when the frame carries it, else blocks x maximum), [6] [7] the content size's low and high
 * word, or -1 -1.  One launch.  EINVAL: a null array with nframes > 0, nframes < 0. */
int APE_LZ4_lz4f_info_batch_dev(const char *const *d_src, const int *d_srcSize, int *d_info,
                                int nframes, void *stream);

/* ---- decode ----
 * flags: 1 = do not verify checksums, 2 = the batch has no block-linked frame (the chained
 * launch is omitted, and a linked frame gets -3).
 * Accepted: block-size IDs 4..7, independent and linked blocks, stored blocks, block checksums,
 * content size, content checksum; bytes after the frame's end are ignored.  EVERY BLOCK BUT THE
 * LAST MUST DECODE TO EXACTLY THE BLOCK MAXIMUM -- what LZ4F_compressFrame, the lz4 tool and the
 * compressor above write -- so block q's output starts at q x maximum.
 * d_result[f]: the decoded size, or the first of these that applies:
 *   -1  bad magic, version, reserved bit, block-size ID or header checksum
 *   -3  unsupported: dictionary ID, skippable or legacy magic, a linked frame with flag 2, a
 *       decoded bound of 2^31 or more
 *   -2  truncated, or a block reaches past d_srcSize[f] or exceeds the block maximum
 *   APE_LZ4_GPU_ERANGE  more than maxBlocks blocks
 *   -9  d_dstCap[f] below the decoded bound (info [5])
 *   -6  block checksum      -4  a block fails to decode      -5  a short block before the last
 *   -8  content size mismatch      -7  content checksum
 * (the header is judged field by field, a truncation ending that: see tests/lz4fmodel.py).
 * A frame's trouble never touches another frame; nothing outside d_dst[f][0, d_dstCap[f]) is
 * written; with a code below -9's row in the list, bytes inside it may have been.
 * decompress_scratch_size: bytes of d_scratch (16-byte aligned) for nframes frames of up to
 *   maxBlocks (>= 1) blocks: 88 bytes per block, 32 per frame; 0 for arguments out of range,
 *   (size_t)-1 from 2^24 blocks on.  What the scratch held is never read.
 * Launches: plan, stored copies, decode, chained decode (without flag 2), hash (without flag 1),
 * finish.
 * EINVAL: a null array or scratch with nframes > 0, nframes < 0, maxBlocks < 1, flags outside
 * 0..3, 2^24 blocks or more, a scratch that is too small or not 16-byte aligned. */
size_t APE_LZ4_lz4f_decompress_scratch_size(int nframes, int maxBlocks);
int APE_LZ4_lz4f_decompress_batch_dev(const char *const *d_src, const int *d_srcSize,
                                      char *const *d_dst, const int *d_dstCap, int *d_result,
                                      int nframes, int maxBlocks, int flags, void *d_scratch,
                                      size_t scratch_bytes, void *stream);

#if defined(__cplusplus)
}
#endif
