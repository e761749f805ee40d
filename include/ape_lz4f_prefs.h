/* ape_lz4f_prefs.h -- framed compress with preferences: the block-size ID and the encoder, what
 * liblz4 takes as LZ4F_preferences_t's blockSizeID and compressionLevel (`lz4 -9 -B7`).  A
 * stand-alone part of the frame layer: it includes ape_lz4f.h and keeps its conventions -- device
 * pointers, asynchronous on `stream`, no allocation, no synchronisation, graph-capturable, a
 * number of launches fixed on the host, APE_LZ4_GPU_EINVAL before any device call, and a batch
 * of 0 launches nothing and may pass null arrays and a null scratch.
 *
 * blockSizeID: 4..7, blocks of B = 64 KiB, 256 KiB, 1 MiB, 4 MiB.
 * mode: 0 the fast encoder, 1 the high-ratio lazy parse, 2 the cost-minimising parse (as for
 *   frames with a dictionary).  depth: 0..256, 0 = 64; it must be 0 with mode 0.
 * flags: those of APE_LZ4_lz4f_compress_batch_dev -- 1 content checksum, 2 block checksums,
 *   4 content size.
 *
 * Frame f holds d_src[f][0, n) as ceil(n / B) block-independent blocks of B bytes (the last
 * shorter): version 01, no dictionary ID, BD = blockSizeID << 4.  Block q is byte for byte what
 * the large-input call of the mode writes for d_src[f][q B, min(n, (q + 1) B)) with capacity
 * len - 1 -- mode 0: APE_LZ4_compress_large_batch_dev at acceleration 1; mode 1:
 * APE_LZ4_compress_large_hc_batch_dev; mode 2: APE_LZ4_compress_large_hc_opt_batch_dev, the last
 * two with restartBytes 0 and no index -- and where that call answers 0 the block is stored.
 * With blockSizeID 4 and mode 0 the frame is APE_LZ4_lz4f_compress_batch_dev's, byte for byte.
 * The frame is a pure function of (input, blockSizeID, mode, depth, flags): the same for any
 * accepted scratch size, any batch composition and any alignment.  tests/lz4fprefsmodel.py
 * defines the bytes; DESIGN.md 3.27 has the launch list and figures.
 *
 * d_result[f]: the frame's bytes; 0 when that exceeds d_dstCap[f] (nothing of d_dst[f] is
 * written then: the size is known before the first byte goes out) or d_srcSize[f] < 0;
 * APE_LZ4_GPU_ERANGE when d_srcSize[f] > maxSrcSize.  A frame's trouble never touches another
 * frame; nothing outside d_dst[f][0, d_dstCap[f]) is written.
 *
 * Choosing the ID.  Larger blocks carry the matches beyond 64 KiB and so compress better, but a
 * block is one unit of work for what reads the frame: APE_LZ4_lz4f_decompress_batch_dev decodes
 * one block per wave, so a batch at ID 7 has 64 times fewer waves than the same bytes at ID 4
 * and decodes far slower (profiles/lz4f_prefs.json).  A block checksum (flag 2)
 * is one XXH32 chain over the block -- 4 MiB of serial steps at ID 7, about 0.23 GiB/s per
 * stream.  That is a property of XXH32, not of this call; only many blocks in
 * flight hide it.
 *
 * compress_prefs_bound: host only, the exact worst case (every block stored); 0 for srcSize
 *   outside 0..0x7E000000, blockSizeID outside 4..7 or flags outside 0..7.
 * compress_prefs_scratch_size: bytes of d_scratch (16-byte aligned) for nframes frames of up to
 *   maxSrcSize (0..0x7E000000) bytes: a slot of B bytes and 36 bytes of arrays for each of
 *   nframes x ceil(maxSrcSize / B) blocks, 8 bytes per frame, then the whole scratch of the
 *   mode's large-input call for that many inputs of up to B bytes.  passSlices has the meaning it
 *   has in APE_LZ4_compress_large_hc_scratch_size (slices searched per pass, 0 = all at once)
 *   and is ignored for mode 0.  0 for arguments out of range, (size_t)-1 from 2^24 block slots
 *   or 2^24 slices on.  The call accepts any scratch from scratch_size(.., 1) on; one below
 *   scratch_size(.., 0) gives more passes and the same bytes.  What the scratch held is never
 *   read.
 * Launches: plan, the mode's large-input launches over the block slots, layout, hash (with
 *   flags & 3), pack (one wave per 64 KiB piece of a block).
 * EINVAL: a null array or scratch with nframes > 0, nframes < 0, maxSrcSize, blockSizeID, mode,
 * depth or flags out of range, depth not 0 with mode 0, 2^24 blocks or slices or more, a scratch
 * that is too small or not 16-byte aligned. */
#pragma once
#include <stddef.h>

#include "ape_lz4f.h"

#if defined(__cplusplus)
extern "C" {
#endif

size_t APE_LZ4_lz4f_compress_prefs_bound(int srcSize, int blockSizeID, int flags);
size_t APE_LZ4_lz4f_compress_prefs_scratch_size(int nframes, int maxSrcSize, int blockSizeID,
                                                int mode, int passSlices);
int APE_LZ4_lz4f_compress_prefs_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          char *const *d_dst, const int *d_dstCap, int *d_result,
                                          int nframes, int maxSrcSize, int blockSizeID, int mode,
                                          int depth, int flags, void *d_scratch,
                                          size_t scratch_bytes, void *stream);

#if defined(__cplusplus)
}
#endif
