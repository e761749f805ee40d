/* ape_lz4_cdicts.h -- a prepared dictionary per message: the part of the batched GPU API
 * (ape_lz4_gpu.h, which includes this file and defines the return codes) that compresses a
 * mixed batch -- messages of several classes, each class with its own dictionary -- in one
 * call, and prepares the classes' objects in one launch.  Same conventions: device pointers,
 * asynchronous on `stream`, APE_LZ4_GPU_OK or a negative APE_LZ4_GPU_E* code. */
#pragma once
#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

/* ---- compress, a prepared object per message (lz4_encode.hip, lz4_hc_cdict.hip) ----
 * The three calls that read a prepared dictionary -- APE_LZ4_compress_usingCDict_batch_dev,
 * APE_LZ4_compress_hc_usingCDict_batch_dev and APE_LZ4_compress_hc_opt_usingCDict_batch_dev, "the
 * twins" below -- take one object for the whole batch.  These take d_cdict[i], a device array of
 * device pointers, one per message, as APE_LZ4_decompress_safe_usingDict_batch_dev takes
 * d_dict[i]; a caller who holds a table of objects and a class per message builds the array with
 * one gather.
 *
 * THE RULE: d_result[i] and d_dst[i][0, d_result[i]) are what the twin gives message i in a call
 * on the object d_cdict[i] -- whatever the other messages of the call name.  There is no new byte
 * rule: the bytes are a pure function of (message, that object's window bytes, depth), and
 * tests/encmodel.py encode_cdict, tests/hcdictmodel.py and tests/hcoptdictmodel.py define them
 * as before.  They do not depend on the batch's composition or order, on the number of passes,
 * on what the scratch held or on any alignment.  The window size D may differ from object to
 * object in one call; for the hc calls maxSrcSize may not (every object must have been prepared
 * for the call's maxSrcSize).
 *
 * PER MESSAGE, not per call: message i gets d_result[i] = 0, and nothing of d_dst[i] is
 * written, when d_cdict[i] is null or not 16-byte aligned (nothing is read through it), when the
 * object's header is not one the twin accepts -- a wrong magic (the other kind's object
 * included), memory that was never prepared, for the hc calls an object prepared for another
 * maxSrcSize -- and the header is the first thing read of an object, in every kernel.  EVERY
 * OTHER MESSAGE OF THE CALL IS UNAFFECTED.  (The twins give the whole batch 0 for a bad object;
 * here a bad object costs only the messages that name it.)  APE_LZ4_GPU_ERANGE for a message
 * larger than its object's (hc: the call's) maxSrcSize, 0 for a negative size or a block that
 * does not fit d_dstCap[i], and nothing written outside d_dst[i][0, d_dstCap[i]): as the twins.
 *
 * scratch (hc calls): exactly the twins' -- the slot layout depends on maxSrcSize only, so
 *   APE_LZ4_compress_hc_usingCDict_scratch_size and ..._hc_opt_usingCDict_scratch_size serve
 *   these calls unchanged, a smaller scratch of at least one slot runs more passes with
 *   identical bytes, and every scratch byte a call reads it has written before.
 * Asynchronous, no allocation, no sync, graph-capturable; the twins' launch counts (one; three
 * per pass).  The objects are only read: any number of calls on any streams may share them.
 * APE_LZ4_GPU_EINVAL before any device call: the twins' list, with "a null d_cdict array when
 * nblocks > 0" in place of the checks of the one object.  nblocks == 0 launches nothing. */
int APE_LZ4_compress_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                           char *const *d_dst, const int *d_dstCap, int *d_result,
                                           int nblocks, const void *const *d_cdict, void *stream);
int APE_LZ4_compress_hc_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                              char *const *d_dst, const int *d_dstCap,
                                              int *d_result, int nblocks,
                                              const void *const *d_cdict, int maxSrcSize, int depth,
                                              void *d_scratch, size_t scratch_bytes, void *stream);
int APE_LZ4_compress_hc_opt_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                  char *const *d_dst, const int *d_dstCap,
                                                  int *d_result, int nblocks,
                                                  const void *const *d_cdict, int maxSrcSize,
                                                  int depth, void *d_scratch, size_t scratch_bytes,
                                                  void *stream);

/* ---- prepare, ndicts objects in one launch (lz4_cdict.hip, lz4_hc_cdict.hip) ----
 * Object k, at (char *)d_cdicts + k * cdict_stride, is BYTE FOR BYTE what APE_LZ4_cdict_prepare_dev
 * (APE_LZ4_hc_cdict_prepare_dev) writes for (d_dict[k], d_dictSize[k], maxSrcSize): all
 * cdict_size() (hc_cdict_size()) bytes.  d_dict and d_dictSize are device arrays.
 * d_dictSize[k] == 0 with a null d_dict[k] is legal, as in the single call.
 * The sizes live on the device, so a bad entry -- a negative size, or a null pointer with a
 * positive size -- cannot be EINVAL: the kernel writes sixteen zero bytes as that object's
 * header and nothing else of it, every other object is intact, and every compress against that
 * object gives 0.  Bytes between objects (cdict_stride larger than the object) are never written.
 * One asynchronous launch of ndicts workgroups; ndicts == 0 launches nothing.
 * APE_LZ4_GPU_EINVAL before any device call for a null array or a null d_cdicts with ndicts > 0,
 * ndicts < 0, maxSrcSize outside 1..65536, a d_cdicts that is not 16-byte aligned, a cdict_stride
 * below the object's size or no multiple of 16. */
int APE_LZ4_cdict_prepare_batch_dev(const char *const *d_dict, const int *d_dictSize,
                                    int maxSrcSize, void *d_cdicts, size_t cdict_stride,
                                    int ndicts, void *stream);
int APE_LZ4_hc_cdict_prepare_batch_dev(const char *const *d_dict, const int *d_dictSize,
                                       int maxSrcSize, void *d_cdicts, size_t cdict_stride,
                                       int ndicts, void *stream);

#if defined(__cplusplus)
}
#endif
