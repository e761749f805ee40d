/* ape_lz4f_dict.h -- LZ4 frames with a dictionary: framed compress against a prepared dictionary
 * per frame, frame info that accepts a dictionary ID, and a framed decode that picks each frame's
 * dictionary from a table by the ID the frame names.  What liblz4 calls
 * LZ4F_compressFrame_usingCDict and LZ4F_decompress_usingDict, and the lz4 tool -D.  A stand-alone
 * part of the batched GPU API: it includes ape_lz4f.h, is included by nothing, and keeps that
 * header's conventions -- device pointers, asynchronous on `stream`, no allocation, no
 * synchronisation, graph-capturable, a number of launches fixed on the host, APE_LZ4_GPU_OK or a
 * negative APE_LZ4_GPU_E* code.  Every call checks its arguments (APE_LZ4_GPU_EINVAL) before it
 * looks for a device, and a batch of 0 launches nothing and may pass null arrays and a null
 * scratch.  What the scratch held is never read.
 *
 * The format: FLG bit 0 announces a le32 dictionary ID after the optional content size and before
 * the header checksum, which covers it.  liblz4 writes the field exactly when the ID is not 0;
 * the dictionary is used either way.  In a block-independent frame EVERY block is compressed
 * against the dictionary and decoded with it as its only history; in a linked frame the history
 * of a block is the last 64 KiB of (dictionary ++ content so far).  An offset counts back from
 * the dictionary's end: of a longer dictionary only the last 64 KiB count.
 * tests/lz4fdictmodel.py defines the bytes and the codes; DESIGN.md 3.26 has the launch lists. */
#pragma once
#include <stddef.h>

#include "ape_lz4f.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* ---- what a frame is, without decoding it ----
 * d_info[10 f .. 10 f + 9]: [0..7] are the eight ints of APE_LZ4_lz4f_info_batch_dev, except that
 * a dictionary ID is no reason for -3; [8] 1 if the frame carries the field, else 0; [9] the ID
 * (its 32 bits), or 0.  With a header-stage code in [0], [8] and [9] are 0.  On every frame
 * without the field [0..7] equal the existing call's.  One launch.
 * EINVAL: a null array with nframes > 0, nframes < 0. */
int APE_LZ4_lz4f_info_dict_batch_dev(const char *const *d_src, const int *d_srcSize, int *d_info,
                                     int nframes, void *stream);

/* ---- compress, a prepared dictionary per frame ----
 * Frame f holds d_src[f][0, d_srcSize[f]) as ONE block-independent block (none for a size of 0),
 * block-size ID 4, version 01; flags as APE_LZ4_lz4f_compress_batch_dev (1 = content checksum,
 * 2 = block checksums, 4 = content size).  The dictionary-ID field is written exactly when
 * d_dictID is not null and d_dictID[f] != 0 (liblz4's rule).  One block per frame is the limit of
 * the prepared objects, whose window shares 64 KiB with the message: of the dictionary the last
 * D = min(dictSize, 65536 - maxSrcSize) bytes are used (fast objects round D down to 64), and a
 * receiver may hand the whole dictionary to any LZ4 frame decoder.
 * mode 0: the fast encoder, objects of APE_LZ4_cdict_prepare*, depth 0.  mode 1: the high-ratio
 * lazy parse, mode 2: the cost-minimising parse; objects of APE_LZ4_hc_cdict_prepare* for this
 * maxSrcSize, depth as in APE_LZ4_compress_hc_usingCDicts_batch_dev (0 = the default).
 * The block is byte for byte what APE_LZ4_compress_usingCDicts_batch_dev (_hc_, _hc_opt_) gives
 * message f against d_cdict[f] with capacity srcSize - 1; when that is 0 the block is stored.
 * There is no new byte rule for blocks (tests/encmodel.py encode_cdict, tests/hcdictmodel.py,
 * tests/hcoptdictmodel.py).
 * A BAD OBJECT -- null, misaligned, of the other kind, never prepared, prepared for another
 * maxSrcSize -- GIVES A VALID FRAME WITH A STORED BLOCK: the block encoders cannot tell a bad
 * object from "does not fit", so it costs the message its ratio and never its correctness.
 * d_result[f]: the frame's bytes; 0 when that exceeds d_dstCap[f] (nothing of d_dst[f] is written
 * then) or d_srcSize[f] < 0; APE_LZ4_GPU_ERANGE when the message exceeds maxSrcSize or, mode 0,
 * the maxSrcSize its (good) object was prepared for.  A frame's trouble never touches another
 * frame; nothing outside d_dst[f][0, d_dstCap[f]) is written.  The frame is a pure function of
 * (message, the object's window bytes, ID, mode, depth, flags).
 * usingCDicts_bound: host only, the exact worst case (a stored block, an ID field); 0 for
 *   srcSize outside 0..65536 or flags outside 0..7.
 * usingCDicts_scratch_size: bytes of d_scratch (16-byte aligned): per frame a slot of maxSrcSize
 *   bytes rounded up to 16 and 44 bytes of arrays, and for modes 1 and 2 the whole scratch of
 *   APE_LZ4_compress_hc_usingCDict_scratch_size (_hc_opt_) for nframes messages; 0 for arguments
 *   out of range, (size_t)-1 from 2^24 frames on.
 * Launches: plan, the mode's encoder (one; three per pass of the high-ratio scratch), layout,
 * hash (with flags & 3), pack.
 * EINVAL: a null array (d_cdict included; d_dictID may be null) or scratch with nframes > 0,
 * nframes < 0, maxSrcSize outside 1..65536, mode outside 0..2, depth outside 0..256 or not 0
 * with mode 0, flags outside 0..7, 2^24 frames or more, a scratch that is too small or not
 * 16-byte aligned. */
size_t APE_LZ4_lz4f_compress_usingCDicts_bound(int srcSize, int flags);
size_t APE_LZ4_lz4f_compress_usingCDicts_scratch_size(int nframes, int maxSrcSize, int mode);
int APE_LZ4_lz4f_compress_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                char *const *d_dst, const int *d_dstCap,
                                                int *d_result, int nframes,
                                                const void *const *d_cdict,
                                                const unsigned *d_dictID /* may be null */,
                                                int maxSrcSize, int mode, int depth, int flags,
                                                void *d_scratch, size_t scratch_bytes,
                                                void *stream);

/* ---- decode, each frame's dictionary from a table ----
 * flags: 1 and 2 as in ape_lz4f.h (do not verify checksums; no linked frame in the batch);
 * 4 = blocks of any size: every block is sized first and decoded where it belongs, with the
 * codes, their order and the scratch of the short-block decode.  Without 4 the
 * full-block rule, codes and scratch of APE_LZ4_lz4f_decompress_batch_dev hold.
 * The table: device arrays of ntable >= 0 entries, key d_tableID[k] -> the dictionary
 * d_tableDict[k] of d_tableDictSize[k] bytes.  A frame's key is its dictionary ID, or 0 when it
 * carries no field; the FIRST entry with that key is the frame's dictionary (a wave-wide search
 * on the device, 64 entries per step, any ntable).  Without a matching entry a frame WITH the
 * field gets -10 and a frame without it is decoded with no dictionary, exactly as the existing
 * calls do.  A matching entry with a negative size, or a null pointer and a positive size, is
 * unusable: -10 for the frames that name it, and nothing is read through it.  Size 0 is a legal,
 * empty dictionary.  A dictionary longer than 64 KiB counts from its end.
 *   -10 belongs to the header stage: after -1, -3, -2 and APE_LZ4_GPU_ERANGE, before -9; nothing
 *   of the destination has been written.  A dictionary ID is no reason for -3 here.
 * In an independent frame every compressed block is decoded with the dictionary as external
 * dictionary, all blocks in parallel; with flag 4 each is sized with the dictionary's size, so an
 * offset past the dictionary's start fails at sizing (-4, nothing written).  In a linked frame
 * block 0 gets the dictionary, and a later block that starts at 65536 or beyond the output
 * before it.
 * THE ONE UNSUPPORTED SHAPE: a later compressed block of a linked frame with a (non-empty)
 * dictionary that starts below 65536 -- possible with flag 4 only -- would need the
 * dictionary's tail and the output as one history.  The frame gets -3, decided before a byte is
 * written: after the sizing's -4, before -9 and -8.
 * With ntable == 0 the call equals the existing call of the same placement on every frame but
 * one with an ID field, which gets -10 where they give -3.
 * usingDicts_scratch_size: the scratch size of the call this one is with these flags; 0 for
 *   arguments out of range (flags outside 0..7 too), (size_t)-1 from 2^24 blocks on.
 * Launches: those of the underlying call; the lookup is part of the plan.
 * EINVAL: the underlying call's list, ntable < 0, a null table array with ntable > 0, flags
 * outside 0..7. */
size_t APE_LZ4_lz4f_decompress_usingDicts_scratch_size(int nframes, int maxBlocks, int flags);
int APE_LZ4_lz4f_decompress_usingDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 char *const *d_dst, const int *d_dstCap,
                                                 int *d_result, int nframes, int maxBlocks,
                                                 const unsigned *d_tableID,
                                                 const char *const *d_tableDict,
                                                 const int *d_tableDictSize, int ntable, int flags,
                                                 void *d_scratch, size_t scratch_bytes,
                                                 void *stream);

#if defined(__cplusplus)
}
#endif
