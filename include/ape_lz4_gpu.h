/*
 * ape_lz4_gpu.h -- batched MI355X LZ4 block codec: the performance path.
 *
 * Each entry point runs N *independent* LZ4 blocks on the calling thread's
 * current HIP device, one workgroup per block.  Per-block results use exactly
 * the conventions of the single-block calls they batch:
 *
 *   APE_LZ4_compress_batch_dev       == N x APE_LZ4_compress_default
 *                                        (ref src/ape_lz4.c:811-815)
 *   APE_LZ4_decompress_safe_batch_dev == N x APE_LZ4_decompress_safe
 *                                        (ref src/ape_lz4.c:1472-1478)
 *   ..._partial_batch_dev            == N x APE_LZ4_decompress_safe_partial
 *                                        (ref src/ape_lz4.c:1480-1487)
 *
 * Compression emits a valid LZ4 v1.7.1 block (decodable by the reference
 * decompress_safe with cap = srcSize) but not the reference's byte stream:
 * the GPU parse is its own.  Decompression is bit-exact
 * with the reference: same return value, same dst[0:ret].
 *
 * Pointers named d_* are device pointers (hipMalloc / torch CUDA tensors).
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 * launchers are asynchronous and graph-capturable (no allocation, no sync), except
 * APE_LZ4_compress_destSize_batch_dev (stream-ordered scratch; see its _scratch form).
 * Return value of a launcher: 0 on success, otherwise a negative
 * APE_LZ4_GPU_E* code (nothing was launched); per-block status is in d_result.
 *
 * GPU limits: one encoder workgroup takes at most APE_LZ4_GPU_MAX_BLOCK (65536) bytes
 * (the LZ4 window; the benchmark's 64 KiB block), and the compress_*_batch_dev entry
 * points give a larger input d_result = APE_LZ4_GPU_ERANGE.  Larger inputs, up to
 * 0x7E000000 bytes, go through APE_LZ4_compress_large_batch_dev, which compresses slices
 * in parallel and stitches them into one block.  The decoder has no block-size limit.
 *
 * History: compress_withPrefix takes it from the bytes before each input (chained streams);
 * compress_usingCDict takes it from one prepared dictionary shared by the whole batch
 * (independent messages); decompress_safe_usingDict decodes both.
 */
#pragma once
#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

#define APE_LZ4_GPU_MAX_BLOCK 65536
#define APE_LZ4_GPU_ERANGE (-2147483647 - 1) /* per-block: size outside GPU limits */

enum {
    APE_LZ4_GPU_OK = 0,
    APE_LZ4_GPU_ENODEV = -1,   /* no usable MI355X / HIP runtime          */
    APE_LZ4_GPU_EINVAL = -2,   /* bad argument (N < 0, null pointer ...)  */
    APE_LZ4_GPU_ELAUNCH = -3,  /* kernel launch / HIP runtime error        */
    APE_LZ4_GPU_ENOMEM = -4    /* staging allocation failed                */
};

/* Runtime. */
int APE_LZ4_gpu_init(void);                 /* 0 if a gfx950 device is usable */
int APE_LZ4_gpu_device_count(void);
const char *APE_LZ4_gpu_last_error(void);   /* thread-local message */
const char *APE_LZ4_gpu_arch(void);         /* "gfx950" */

/* ---- batched, device-resident, pointer-array form ----
 * d_src[i]  : block i input (device)     d_srcSize[i] : its size (0..65536)
 * d_dst[i]  : block i output (device)    d_dstCap[i]  : its capacity
 * d_result[i] <- compressed size, or 0 if it does not fit d_dstCap[i].
 *
 * DETERMINISM (APE_LZ4_compress_batch_dev, _compress_fast_batch_dev and
 *   _compress_withPrefix_batch_dev): the output bytes are a pure function of (input bytes, the
 *   used prefix, acceleration) -- the same on every call, stream, batch composition, capacity
 *   that holds the block, and alignment of source and destination; tests/encmodel.py defines
 *   that function on the CPU.  The strided and host-buffer forms, compress_destSize with a
 *   target the block fits and the large-input path up to 65536 bytes write the same bytes.  The
 *   bytes differ from the reference's. */
int APE_LZ4_compress_batch_dev(const char *const *d_src, const int *d_srcSize,
                               char *const *d_dst, const int *d_dstCap, int *d_result,
                               int nblocks, void *stream);

/* == N x APE_LZ4_compress_fast (ref src/ape_lz4.c:789-808): acceleration > 1 probes the
 * reference's positions -- the match end, the next two, then steps of acceleration growing
 * by one every 64 misses (:591-600) -- with the reference's unbounded catch-up, so the ratio
 * follows the reference's (within 1 % at 2, 4, 8 on the benchmark data); <= 1 is
 * compress_default. */
int APE_LZ4_compress_fast_batch_dev(const char *const *d_src, const int *d_srcSize,
                                    char *const *d_dst, const int *d_dstCap, int *d_result,
                                    int nblocks, int acceleration, void *stream);

/* Greedy-exact mode (slow, for debugging): == N x APE_LZ4_compress_fast
 * (ref src/ape_lz4.c:789-808 -> LZ4_compress_generic :530-755, byU16), BYTE FOR BYTE -- the
 * reference's sequential parse run by one wave per block, limitedOutput's early exits (0)
 * included; acceleration <= 1 is compress_default.  Deviation: a negative d_dstCap[i] gives 0
 * (the reference treats it as a huge unsigned capacity in its last-literals check). */
int APE_LZ4_compress_exact_batch_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int acceleration, void *stream);

/* d_result[i] <- decoded size, or -(consumed)-1, as APE_LZ4_decompress_safe. */
int APE_LZ4_decompress_safe_batch_dev(const char *const *d_src, const int *d_compressedSize,
                                      char *const *d_dst, const int *d_maxDecompressedSize,
                                      int *d_result, int nblocks, void *stream);

/* As APE_LZ4_decompress_safe_partial with per-block targetOutputSize. */
int APE_LZ4_decompress_safe_partial_batch_dev(const char *const *d_src,
                                              const int *d_compressedSize,
                                              char *const *d_dst, const int *d_targetOutputSize,
                                              const int *d_maxDecompressedSize,
                                              int *d_result, int nblocks, void *stream);

/* ---- chained streams (socket path with the reference wire format) ----
 * The reference socket compresses each chunk with compress_fast_continue against the
 * previous <= 64 KiB of its stream and the receiver decodes it with
 * decompress_safe_continue against its saved dictionary (ref src/ape_lz4.c:1160-1220,
 * :1555-1584; src/ape_socket.c:832-857, :1386-1421).  Batched across connections:
 *
 * compress_withPrefix : d_prefixSize[i] bytes immediately before d_src[i] are the
 *   stream's history; matches may reach into it (the last min(prefix, 65536 - size)
 *   bytes, rounded down to a multiple of 64, are used).  d_result[i] as
 *   APE_LZ4_compress_batch_dev.  The block decodes with decompress_safe_continue /
 *   decompress_safe_usingDict given that history (bytes differ from the reference's,
 *   as for every GPU-compressed block).
 * decompress_safe_usingDict : == N x APE_LZ4_decompress_safe_usingDict(src, dst,
 *   csize, cap, dict, dictSize) (ref src/ape_lz4.c:1625-1655), bit-exact, any
 *   placement of the dictionary (adjacent to dst or not). */
int APE_LZ4_compress_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          const int *d_prefixSize, char *const *d_dst,
                                          const int *d_dstCap, int *d_result, int nblocks,
                                          void *stream);
int APE_LZ4_decompress_safe_usingDict_batch_dev(const char *const *d_src,
                                                const int *d_compressedSize, char *const *d_dst,
                                                const int *d_maxDecompressedSize,
                                                const char *const *d_dict, const int *d_dictSize,
                                                int *d_result, int nblocks, void *stream);

/* ---- prepared dictionaries: many independent messages against one shared dictionary ----
 * compress_withPrefix needs the history to be the bytes right before each input, which fits
 * a chained stream.  The other classic use -- small independent messages (JSON frames, RPC
 * replies) compressed against one shared dictionary, loadDict + compress_fast_continue on a
 * fresh stream per message (ref src/ape_lz4.c:1101-1133, :1160-1220) -- goes through a
 * PREPARED dictionary (in the sense of zstd's CDict): one kernel turns the dictionary into a
 * device object holding a padded copy of the dictionary's tail and a prebuilt image of the
 * encoder's hash table, and any number of later batched calls encode against it without a
 * per-message copy or a per-message hashing pass.
 *
 * cdict_size    : bytes of device memory one prepared dictionary takes (a compile-time
 *   constant, a multiple of 16).
 * cdict_window  : bytes D of the dictionary's tail a prepared dictionary uses: D =
 *   min(dictSize, 65536 - maxSrcSize) rounded down to a multiple of 64, below 64 -> 0.
 *   Host-only arithmetic; -1 for arguments out of range.
 * cdict_prepare : d_dict[dictSize - D, dictSize) -> the object at d_cdict (16-byte aligned,
 *   cdict_bytes >= cdict_size()).  maxSrcSize (1..65536) trades dictionary for message size:
 *   window and message share the encoder's one 64 KiB window.  dictSize may exceed 65536
 *   (only the tail counts); dictSize 0 (d_dict may then be NULL), or a D that rounds to 0, is
 *   legal and gives an object that encodes like APE_LZ4_compress_batch_dev, without history.
 *   One asynchronous launch, no allocation, no sync, graph-capturable.  It writes EVERY byte
 *   of d_cdict[0, cdict_size()), so two prepares of the same input give identical bytes.
 * compress_usingCDict : == N x (loadDict(dict) ; compress_fast_continue(src, acceleration
 *   1)) on fresh streams.  d_result[i] <- compressed size, or 0 if it does not fit
 *   d_dstCap[i] or the size is negative; APE_LZ4_GPU_ERANGE when d_srcSize[i] exceeds the
 *   maxSrcSize the object was prepared for.  The other blocks of the call are unaffected.
 *   The output is a valid LZ4 block that decompress_safe_usingDict(src, dst, csize, cap,
 *   dict, dictSize) decodes with the CALLER'S ORIGINAL dictionary (offsets count back from
 *   its end, so any placement works); bytes differ from the reference's, as for every
 *   GPU-compressed block.  A match taken from the dictionary ends at the dictionary's end
 *   (the reference lets it run on into the message; a few bytes of ratio).
 *   The object is only read: any number of calls, on any streams, may share it.  It starts
 *   with a header (magic, D, maxSrcSize) that the kernel checks before it uses anything else
 *   of it: every block of a call on an object that was never prepared gets result 0.  One
 *   dictionary per call (a dictionary per message: ape_lz4_cdicts.h); no acceleration
 *   parameter (as compress_withPrefix has none).
 * Both launchers return APE_LZ4_GPU_EINVAL before any device call for a null pointer,
 * nblocks < 0, dictSize < 0, maxSrcSize out of range, cdict_bytes too small or d_cdict not
 * 16-byte aligned; 0 otherwise. */
size_t APE_LZ4_cdict_size(void);
int APE_LZ4_cdict_window(int dictSize, int maxSrcSize);
int APE_LZ4_cdict_prepare_dev(const char *d_dict, int dictSize, int maxSrcSize, void *d_cdict,
                              size_t cdict_bytes, void *stream);
int APE_LZ4_compress_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          char *const *d_dst, const int *d_dstCap, int *d_result,
                                          int nblocks, const void *d_cdict, void *stream);

/* == N x APE_LZ4_decompress_fast(src, dst, originalSize) (ref src/ape_lz4.c:1489):
 * d_result[i] <- compressed bytes consumed, or -(consumed)-1.  The reference reads its
 * input without a bound; the batch needs d_srcBound[i] = the readable bytes at d_src[i]
 * (e.g. compressBound(originalSize)), and rejects an offset reaching before d_dst[i]
 * (the reference reads memory before dst there). */
int APE_LZ4_decompress_fast_batch_dev(const char *const *d_src, const int *d_srcBound,
                                      char *const *d_dst, const int *d_originalSize,
                                      int *d_result, int nblocks, void *stream);

/* == N x APE_LZ4_compress_destSize(src, dst, &srcSize, targetDstSize) (ref
 * src/ape_lz4.c:1048-1067, :843-1021): d_srcSize[i] is in/out -- on entry the input size,
 * on return the input bytes the block encodes; d_result[i] <- bytes written to d_dst[i]
 * (<= d_targetDstSize[i]; 0 if the target is < 1 or the size negative).  The output is a
 * valid LZ4 block of src[0, consumed) (decodes with cap = consumed); when the whole block
 * fits the target it is compress_default's output.  Bytes and consumed size differ from
 * the reference's greedy cut (the GPU parse is chunk-parallel; the cut is at a sequence
 * boundary followed by as many literals as fit).  The one launcher that allocates:
 * stream-ordered scratch (hipMallocAsync/hipFreeAsync on `stream`) of ~65.8 KB per
 * block, at most 16384 blocks at a time -- not for graph capture; the _scratch form
 * below takes caller-owned scratch instead and allocates nothing. */
int APE_LZ4_compress_destSize_batch_dev(const char *const *d_src, int *d_srcSize,
                                        char *const *d_dst, const int *d_targetDstSize,
                                        int *d_result, int nblocks, void *stream);
/* Scratch bytes for destSize of nblocks in one pass (a smaller 16-aligned scratch, at
 * least scratch_size(1), makes the call run several passes). */
size_t APE_LZ4_compress_destSize_scratch_size(int nblocks);
int APE_LZ4_compress_destSize_batch_scratch_dev(const char *const *d_src, int *d_srcSize,
                                                char *const *d_dst, const int *d_targetDstSize,
                                                int *d_result, int nblocks, void *d_scratch,
                                                size_t scratch_bytes, void *stream);

/* ---- high-ratio mode: spend time, get ratio (lz4_encode_hc.hip) ----
 * d_result[i] <- size of one valid LZ4 v1.7.1 block of d_src[i][0, d_srcSize[i]) (decodes with
 * decompress_safe, cap = srcSize; never above compressBound(srcSize)), found by a deep search:
 * every position tries the first `depth` earlier positions that share the hash of its 4 bytes,
 * nearest first, keeps the strictly longest match, and a sequential parse takes the match at
 * the first position whose successor's match is not longer (a one-step lazy parse).  Per block
 * the call behaves as APE_LZ4_compress_batch_dev: 0 if the block does not fit d_dstCap[i]
 * (checked before every sequence is written) or the size is negative, APE_LZ4_GPU_ERANGE for
 * d_srcSize[i] > 65536; the other blocks of the call are unaffected; nothing outside
 * d_dst[i][0, cap) is written and nothing outside d_src[i][0, size) is read.
 *
 * depth : chain candidates tried per position, 1..256; 0 means the default, 64.  The ratio
 *   grows and the speed falls with it (README, "high-ratio mode").
 * DETERMINISM: the output bytes are a pure function of (input bytes, depth) -- the same on
 *   every call, stream, batch composition, scratch size and alignment; tests/hcmodel.py
 *   defines that function on the CPU.  The bytes differ from the reference's and from
 *   APE_LZ4_compress_batch_dev's.
 * scratch : the caller's, 16-byte aligned device memory.  scratch_size(nblocks) is what one
 *   pass over nblocks takes -- a chain table and one (length, source) record per position,
 *   393216 bytes per block, at most 1024 blocks at a time; 0 for nblocks <= 0.  A smaller
 *   scratch, at least scratch_size(1), makes the call run several passes with identical
 *   output.  Every scratch byte the call reads it has written before, in the same call.
 * Asynchronous, no allocation, no sync, graph-capturable: three stream-ordered launches per
 * pass, their number decided on the host.  APE_LZ4_GPU_EINVAL before any device call for
 * nblocks < 0, a null array (nblocks > 0), depth outside 0..256, a null or misaligned
 * scratch or one below scratch_size(1); with nblocks == 0 it returns 0 and launches
 * nothing. */
size_t APE_LZ4_compress_hc_scratch_size(int nblocks);
int APE_LZ4_compress_hc_batch_dev(const char *const *d_src, const int *d_srcSize,
                                  char *const *d_dst, const int *d_dstCap, int *d_result,
                                  int nblocks, int depth, void *d_scratch, size_t scratch_bytes,
                                  void *stream);
/* The high-ratio mode with history: block i is compressed with the bytes just before d_src[i]
 * as its history, and decodes with decompress_safe_usingDict given that history (or in place
 * behind it).  USED HISTORY: the last min(d_prefixSize[i], 65536 - d_srcSize[i]) bytes before
 * the block -- not rounded to a multiple of 64 as the fast encoder's prefix is; a negative
 * prefix counts as 0, a null d_prefixSize means no history for any block, and the call then
 * writes APE_LZ4_compress_hc_batch_dev's bytes.  The chains run over history + block, so a
 * candidate may lie in the history; only the block's positions are searched and parsed.  A
 * block shorter than 13 bytes is one literal run.  Nothing outside [d_src[i] - used history,
 * d_src[i] + size) is read.  Scratch, passes, depth, results and errors are as above.
 * DETERMINISM: the bytes are a pure function of (input bytes, used history, depth);
 * tests/hclargemodel.py compress_prefix() defines that function on the CPU. */
int APE_LZ4_compress_hc_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             const int *d_prefixSize, char *const *d_dst,
                                             const int *d_dstCap, int *d_result, int nblocks,
                                             int depth, void *d_scratch, size_t scratch_bytes,
                                             void *stream);

/* ---- high-ratio mode, cost-minimising parse (lz4_encode_hc.hip) ----
 * APE_LZ4_compress_hc_opt_batch_dev and APE_LZ4_compress_hc_opt_withPrefix_batch_dev are the two
 * calls above with another parse over the same search: arguments, used history, depth (0..256,
 * 0 = 64), per-block results, what is read and written, passes and errors are theirs.  THE RULE:
 * every offset of an LZ4 block costs two bytes, so the longest match the search found at a
 * position prices every shorter length of it too.  A backward pass over the block gives each
 * position the bytes the rest of the block takes from there -- a literal (with the length byte
 * it adds to the literal run it leads), or a match of any length from 4 up to the match's FULL
 * length (the common prefix of source and position up to the block's end less 5, also past the
 * search's cap of 272) -- and keeps the cheapest; a tie goes to the match, and among equally
 * cheap lengths to the longest.  A forward pass emits the choices; there is no lazy step and no
 * backward extension.  The parse is cost-minimising, not optimal: a literal is priced against
 * the run of the chosen continuation only.  The block's size is known before its first byte is
 * written, so a block that does not fit d_dstCap[i] writes nothing.
 * DETERMINISM: the output bytes are a pure function of (input bytes, used history, depth) -- the
 *   same on every call, stream, batch composition, scratch size and alignment;
 *   tests/hcoptmodel.py defines that function on the CPU (compress(), compress_prefix()).  On
 *   the test inputs no block is larger than the lazy parse's; the bytes differ from it.
 * scratch : the caller's, 16-byte aligned.  scratch_size(nblocks) is what one pass over nblocks
 *   takes -- the chain table, the match records and one cost per position, 393216 + 262144 =
 *   655360 bytes per block, at most 1024 blocks at a time; 0 for nblocks <= 0.  A smaller
 *   scratch, at least scratch_size(1), makes the call run several passes with identical output.
 *   Every scratch byte the call reads it has written before, in the same call.
 * Asynchronous, no allocation, no sync, graph-capturable: three stream-ordered launches per pass
 * (chain build and search as above, then one kernel that prices and emits), their number
 * decided on the host.  APE_LZ4_GPU_EINVAL before any device call as above, with this
 * scratch_size(1). */
size_t APE_LZ4_compress_hc_opt_scratch_size(int nblocks);
int APE_LZ4_compress_hc_opt_batch_dev(const char *const *d_src, const int *d_srcSize,
                                      char *const *d_dst, const int *d_dstCap, int *d_result,
                                      int nblocks, int depth, void *d_scratch,
                                      size_t scratch_bytes, void *stream);
int APE_LZ4_compress_hc_opt_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 const int *d_prefixSize, char *const *d_dst,
                                                 const int *d_dstCap, int *d_result, int nblocks,
                                                 int depth, void *d_scratch, size_t scratch_bytes,
                                                 void *stream);

/* ---- the high-ratio mode against a prepared dictionary (lz4_hc_cdict.hip) ----
 * Many independent messages, one shared dictionary, the deep search: message i is compressed
 * with the dictionary's tail as its history, without a per-message copy of the dictionary and
 * without a per-message chain build over it.  A PREPARED HIGH-RATIO DICTIONARY is a device
 * object of its own kind (not the fast encoder's, above): a padded copy of the dictionary's
 * tail, and the hash chains and the head table of that tail as the chain build leaves them.
 *
 * hc_cdict_size    : bytes of device memory one such object takes (a compile-time constant, a
 *   multiple of 16).
 * hc_cdict_window  : bytes D of the dictionary's tail the object uses: D = min(dictSize,
 *   65536 - maxSrcSize), NOT rounded to a multiple of 64 (the rule of compress_hc_withPrefix,
 *   not of cdict_window); 0 is legal.  Host-only arithmetic; -1 for arguments out of range.
 * hc_cdict_prepare : d_dict[dictSize - D, dictSize) -> the object at d_cdict (16-byte aligned,
 *   cdict_bytes >= hc_cdict_size()).  maxSrcSize (1..65536) trades dictionary for message size.
 *   dictSize may exceed 65536 (only the tail counts); dictSize 0 (d_dict may then be NULL) is
 *   legal.  One asynchronous launch, no allocation, no sync, graph-capturable.  It writes EVERY
 *   byte of d_cdict[0, hc_cdict_size()), so two prepares of the same input give identical bytes.
 * compress_hc_usingCDict : d_result[i] <- size of one valid LZ4 block of d_src[i][0,
 *   d_srcSize[i]) that decompress_safe_usingDict decodes with the CALLER'S ORIGINAL dictionary
 *   (any size, any placement).  THE BYTES are exactly those APE_LZ4_compress_hc_withPrefix_
 *   batch_dev writes for the staged window [dictionary's last D bytes | message] with prefix D:
 *   a pure function of (message, those D bytes, depth), tests/hcdictmodel.py on the CPU.  So,
 *   unlike compress_usingCDict, a match that starts in the dictionary runs on into the message,
 *   and the three positions before the message are chain members; a message shorter than 13
 *   bytes is one literal run.  With D = 0 the bytes are APE_LZ4_compress_hc_batch_dev's.
 *   maxSrcSize is the host-side bound that sizes the grid and the scratch; the kernels compare
 *   it with the object's header BEFORE anything else of the object is used, and a mismatch, a
 *   wrong magic (the fast encoder's object, say) or an object that was never prepared gives
 *   EVERY block of the call result 0.  depth is 0..256, 0 meaning 64.  Per block: 0 for a
 *   negative size or a block that does not fit d_dstCap[i] (checked before each sequence is
 *   written), APE_LZ4_GPU_ERANGE above maxSrcSize; the other blocks are unaffected.  Nothing
 *   outside d_src[i][0, size), the object and d_dst[i][0, cap) is touched.  The object is only
 *   read: any number of calls, on any streams, may share it.
 * scratch : the caller's, 16-byte aligned.  scratch_size(nblocks, maxSrcSize) is what one pass
 *   takes: per message a u16 chain entry for each window position from D - 3 on (maxSrcSize +
 *   3 of them) and a u32 match record per message position, each rounded to 16 bytes -- about
 *   6 x maxSrcSize bytes -- for at most 262144 / ceil(maxSrcSize / 256) messages at a time; 0
 *   for nblocks <= 0 or maxSrcSize out of range.  A smaller scratch, at least scratch_size(1,
 *   maxSrcSize), makes the call run several passes (their number decided on the host) with
 *   identical bytes.  Every scratch byte the call reads it has written before, in the same
 *   call.  No allocation, no sync: three stream-ordered launches per pass, graph-capturable.
 * APE_LZ4_GPU_EINVAL before any device call for a null array (nblocks > 0), nblocks < 0,
 * dictSize < 0, depth or maxSrcSize out of range, a null, misaligned or too small object
 * (prepare; compress cannot see its size) or scratch; 0 otherwise. */
size_t APE_LZ4_hc_cdict_size(void);
int APE_LZ4_hc_cdict_window(int dictSize, int maxSrcSize);
int APE_LZ4_hc_cdict_prepare_dev(const char *d_dict, int dictSize, int maxSrcSize, void *d_cdict,
                                 size_t cdict_bytes, void *stream);
size_t APE_LZ4_compress_hc_usingCDict_scratch_size(int nblocks, int maxSrcSize);
int APE_LZ4_compress_hc_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nblocks, const void *d_cdict,
                                             int maxSrcSize, int depth, void *d_scratch,
                                             size_t scratch_bytes, void *stream);

/* ---- the cost-minimising parse against a prepared high-ratio dictionary (lz4_hc_cdict.hip) ----
 * APE_LZ4_compress_hc_usingCDict_batch_dev with the parse of APE_LZ4_compress_hc_opt_batch_dev:
 * the same object (APE_LZ4_hc_cdict_prepare_dev; there is no other kind and no other prepare),
 * the same chains and search, then every message position priced backward and the choices
 * emitted forward.  THE BYTES are exactly those APE_LZ4_compress_hc_opt_withPrefix_batch_dev
 * writes for the staged window [dictionary's last D bytes | message] with prefix D: a pure
 * function of (message, those D bytes, depth), tests/hcoptdictmodel.py on the CPU.  Each block
 * decodes with decompress_safe_usingDict given the CALLER'S ORIGINAL dictionary; with D = 0 the
 * bytes are APE_LZ4_compress_hc_opt_batch_dev's; a message shorter than 13 bytes is one literal
 * run.  Arguments, the header check, per-block results and APE_LZ4_GPU_EINVAL are
 * compress_hc_usingCDict's, with one difference: the block's size is known before its first
 * byte is written, so a block that does not fit d_dstCap[i] gets result 0 and NOTHING is written
 * to d_dst[i].
 * scratch : compress_hc_usingCDict's slot plus a u32 cost per message position, rounded to 16
 *   bytes -- about 10 x maxSrcSize bytes per message -- for the same number of messages per
 *   pass; 0 for nblocks <= 0 or maxSrcSize out of range.  A scratch of at least scratch_size(1,
 *   maxSrcSize) runs as many passes as it needs with identical bytes.  Every scratch byte the
 *   call reads it has written before, in the same call.  No allocation, no sync: three
 *   stream-ordered launches per pass, graph-capturable. */
size_t APE_LZ4_compress_hc_opt_usingCDict_scratch_size(int nblocks, int maxSrcSize);
int APE_LZ4_compress_hc_opt_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 char *const *d_dst, const int *d_dstCap,
                                                 int *d_result, int nblocks, const void *d_cdict,
                                                 int maxSrcSize, int depth, void *d_scratch,
                                                 size_t scratch_bytes, void *stream);

/* ---- dictionary training (lz4_dict_train.hip) ----
 * The step before cdict_prepare / hc_cdict_prepare: APE_LZ4_dict_train_scratch_size and
 * APE_LZ4_dict_train_dev build a dictionary from a batch of device-resident sample messages.
 * They are a family of their own -- they compress and decompress nothing -- and are declared,
 * with the rule and the reading and writing bounds, in ape_lz4_dict_train.h, which the end of
 * this header includes. */

/* ---- a prepared dictionary per message (lz4_encode.hip, lz4_hc_cdict.hip, lz4_cdict.hip) ----
 * The three compress calls above that read a prepared dictionary take one object per call.  Their
 * usingCDicts forms take a device array with one object pointer per message, so a batch of mixed
 * message classes is one call, and the two prepare_batch calls prepare the classes' objects in
 * one launch.  They add no byte rule: message i gets what the call above writes for it against
 * its own object, and a bad object costs only the messages that name it.  They are declared,
 * with those rules, in ape_lz4_cdicts.h, which the end of this header includes. */

/* ---- inputs larger than one encoder block, as ONE LZ4 block (lz4_large.hip) ----
 * == N x APE_LZ4_compress_fast on inputs of any size up to maxSrcSize: d_result[i] <-
 * size of ONE valid LZ4 block of d_src[i][0, d_srcSize[i]) (decodes with decompress_safe,
 * cap = srcSize), or 0 if it does not fit d_dstCap[i] (nothing is written then).  The
 * output never exceeds compressBound(srcSize).
 *
 * maxSrcSize (1 .. 0x7E000000) is a host-side upper bound on every d_srcSize[i]: it sizes
 * the grid and the scratch, since the sizes themselves live on the device.  A block with
 * d_srcSize[i] > maxSrcSize gets APE_LZ4_GPU_ERANGE, a negative size 0; the other blocks of
 * the call are unaffected.  The scratch is the caller's: 16-byte aligned device memory of
 * at least APE_LZ4_compress_large_scratch_size(nblocks, maxSrcSize) bytes (about the batch's
 * maxSrcSize x nblocks again), otherwise the call returns APE_LZ4_GPU_EINVAL and
 * APE_LZ4_gpu_last_error names the size needed.  There are no internal passes: a batch that
 * needs too much scratch is split by the caller (scratch_size returns (size_t)-1 for a batch
 * of 2^24 or more slices, 0 for arguments out of range).  Asynchronous, no
 * allocation, no sync, graph-capturable: four stream-ordered launches.
 *
 * Slicing.  An input of at most 65536 bytes is one slice and its output is byte-identical
 * to APE_LZ4_compress_fast_batch_dev at the same acceleration.  A larger input is cut at
 * multiples of S = APE_LZ4_compress_large_slice_size() (a compile-time constant, a multiple
 * of 64, <= 65536 - 64); slice k is compressed with the preceding min(k*S, 65536 - len_k)
 * bytes as history, exactly as APE_LZ4_compress_withPrefix_batch_dev does with prefix = k*S
 * (all slices in parallel).  The block is the slices' sequences STITCHED: where slice k-1
 * ends in a final literal run of t bytes and slice k begins with l literals, the output has
 * one sequence of t + l literals that keeps slice k's match; a slice with no match at all
 * only lengthens the run carried into the next slice; the block ends with one final literal
 * run.  Every other byte is the slices' own.
 *
 * Decoding such a block with APE_LZ4_decompress_safe_batch_dev is one workgroup per block.
 * A block written with restart points and a seek index
 * (APE_LZ4_compress_large_indexed_batch_dev, below) decodes one wave per segment. */
int APE_LZ4_compress_large_slice_size(void);
size_t APE_LZ4_compress_large_scratch_size(int nblocks, int maxSrcSize);
int APE_LZ4_compress_large_batch_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int maxSrcSize, int acceleration,
                                     void *d_scratch, size_t scratch_bytes, void *stream);
/* Diagnostic (tools/large_bench.py): the same call with HIP events around its four launches;
 * waits for them and returns ms4[0..4) = plan, encode, offsets, stitch in milliseconds.
 * Synchronous, creates events: not for graph capture. */
int APE_LZ4_compress_large_timed_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int maxSrcSize, int acceleration,
                                     void *d_scratch, size_t scratch_bytes, void *stream,
                                     float *ms4);

/* ---- large blocks with restart points and a seek index (lz4_large.hip, lz4_decode.hip) ----
 * A plain LZ4 block decodes serially: token positions are known only by walking it, and a
 * match may copy bytes that are themselves copies.  Here the compressor cooperates.  With
 * restartBytes = R > 0 (a positive multiple of the slice size S), every slice that starts at
 * a multiple of R is encoded with NO history, and slice k at k*S otherwise with the bytes
 * back to the last multiple of R (at most 65536 - len_k of them).  The block is still one
 * ordinary LZ4 block (the stitch is unchanged: a literal run may merge across a restart
 * point), but no match of the bytes [j R, (j + 1) R) reaches before j R, so the block falls
 * into segments that decode independently once their positions are known.  The index says
 * where they are.  restartBytes = 0 places no restart points: the block is byte-identical to
 * APE_LZ4_compress_large_batch_dev's, which is this call with restartBytes 0 and no index.
 *
 * Index format: one per block at d_index + i * index_stride (16-byte aligned, the stride a
 * multiple of 16), little-endian uint32 words
 *     w[0] 0x3158494C ("LIX1")   w[1] nseg   w[2] n (decoded size)   w[3] c (block size)
 *     w[4 + 2j], w[5 + 2j] = ip_j, op_j    for j = 0 .. nseg
 * A valid index satisfies, and a decoder relies on nothing else:
 *   - (ip_0, op_0) = (0, 0) and (ip_nseg, op_nseg) = (c, n); both columns are non-decreasing;
 *   - for j < nseg, ip_j is the position of a token and op_j the output position at which
 *     that sequence's literals start;
 *   - every sequence that starts in [ip_j, ip_{j+1}) takes its match from output positions
 *     >= op_j;
 *   - segment nseg - 1 ends with the block's final literal run;
 *   - a segment may be empty (ip_j == ip_{j+1}, then op_j == op_{j+1});
 *   - when no block was produced (d_result[i] <= 0), w[1] = 0.
 * The compressor writes nseg = ceil(n / R) segments for an input of n > 65536 and n > R bytes
 * and one segment otherwise; entry j is the first sequence whose match lies at or after j R
 * (op_j <= j R: its literals may begin before), so a stretch without any match gives empty
 * segments and an incompressible input has its whole block in the last one.
 *
 * APE_LZ4_large_index_segments(maxSrcSize, restartBytes) = the most segments an input of up to
 * maxSrcSize bytes gets (1 when maxSrcSize <= 65536 or restartBytes == 0);
 * APE_LZ4_large_index_size = 16 + 8 (segments + 1) rounded up to 16, the least index_stride.
 * Both are host-only and return 0 for arguments out of range (maxSrcSize outside
 * [1, 0x7E000000], restartBytes negative or no multiple of S).
 *
 * APE_LZ4_compress_large_indexed_batch_dev: the arguments of APE_LZ4_compress_large_batch_dev
 * with restartBytes, d_index, index_stride before the stream.  d_index == NULL places the
 * restart points only.  APE_LZ4_GPU_EINVAL for a restartBytes that is neither 0 nor a positive
 * multiple of S, a misaligned d_index, or a stride that is no multiple of 16 or below
 * APE_LZ4_large_index_size(maxSrcSize, restartBytes).  Asynchronous, no allocation, no sync,
 * graph-capturable; one more launch than the plain call when there is an index.
 *
 * APE_LZ4_decompress_safe_indexed_batch_dev: two stream-ordered launches, no scratch, no
 * allocation, no sync, graph-capturable.  The index is never trusted.  The first launch
 * judges each header: wrong magic, nseg == 0, w[3] != d_compressedSize[i],
 * n > d_maxDecompressedSize[i] or a wrong first or last pair give d_result[i] = -1,
 * nseg > maxSegments gives APE_LZ4_GPU_ERANGE, otherwise d_result[i] = n.  The second is
 * nblocks x maxSegments waves (fewer than 2^31, index_stride >= 16 + 8 (maxSegments + 1),
 * else APE_LZ4_GPU_EINVAL); wave (i, j) decodes src + ip_j into dst + op_j with the block's true
 * end and capacity (the reference's end-of-block tests apply as in a serial decode), with
 * op_j as the floor of every match, and for j < nseg - 1 up to the SEGMENT STOP: it
 * succeeds when the parse reaches token position ip_{j+1} exactly with output position
 * op_{j+1} exactly.  Stepping over the stop, reaching it at another output position or
 * meeting the final sequence first fails; the last segment is an ordinary decode to the end,
 * of n - op_j bytes.  A failing segment records -(p)-1, p counted from the block's start
 * (index inconsistencies: p = ip_j); d_result[i] ends as the code with the smallest p,
 * whatever the order the waves ran in.
 *   - d_result[i] = r > 0: r and dst[0, r) are what APE_LZ4_decompress_safe gives.
 *   - A negative result need not be the reference's code: a stream that a serial decoder
 *     accepts but that breaks the index's invariants is rejected.  With nseg = 1 the call is
 *     bit-exact with APE_LZ4_decompress_safe_batch_dev, codes included.
 *   - Nothing outside src[0, c) and the index is read, nothing outside dst[0, cap) written.
 * A block that is one literal run (incompressible input) is one segment: one wave. */
int APE_LZ4_large_index_segments(int maxSrcSize, int restartBytes);
size_t APE_LZ4_large_index_size(int maxSrcSize, int restartBytes);
int APE_LZ4_compress_large_indexed_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nblocks, int maxSrcSize,
                                             int acceleration, void *d_scratch,
                                             size_t scratch_bytes, int restartBytes, void *d_index,
                                             size_t index_stride, void *stream);
int APE_LZ4_decompress_safe_indexed_batch_dev(const char *const *d_src,
                                              const int *d_compressedSize, char *const *d_dst,
                                              const int *d_maxDecompressedSize,
                                              const void *d_index, size_t index_stride,
                                              int maxSegments, int *d_result, int nblocks,
                                              void *stream);

/* ---- large and indexed blocks in the high-ratio mode (lz4_large.hip, lz4_encode_hc.hip) ----
 * APE_LZ4_compress_large_hc_batch_dev is APE_LZ4_compress_large_indexed_batch_dev with the
 * high-ratio encoder on the slices: the same slicing at multiples of S, the same restart
 * points (restartBytes) and seek index (d_index, nullable), the same stitch, the same per-block
 * results (0 for a negative size or a block that does not fit -- nothing is written then for
 * an input above 65536 bytes, a smaller one is encoded in place -- and APE_LZ4_GPU_ERANGE above
 * maxSrcSize), and blocks that every decoder above reads.  Slice k is
 * compressed as APE_LZ4_compress_hc_withPrefix_batch_dev does with the bytes back to the
 * input's start or the last restart point as its prefix, so its used history is the last
 * min(that, 65536 - len_k) bytes.  An input of at most 65536 bytes is one slice and gets
 * exactly APE_LZ4_compress_hc_batch_dev's bytes.  depth is as there (0..256, 0 = 64).
 * DETERMINISM: the bytes are a pure function of (input bytes, used history, depth,
 *   restartBytes) -- the same on every call, stream, batch composition, scratch size and
 *   alignment; tests/hclargemodel.py is that function (compress_large()).
 * scratch : the caller's, 16-byte aligned.  APE_LZ4_compress_large_hc_scratch_size(nblocks,
 *   maxSrcSize, passSlices) is the large path's layout plus the high-ratio tables (393216
 *   bytes each) of passSlices slices; passSlices = 0 means as many as the batch has, at most
 *   1024.  It returns 0 for arguments out of range and (size_t)-1 for 2^24 slices or more, as
 *   APE_LZ4_compress_large_scratch_size does.  The call accepts any scratch of at least
 *   scratch_size(nblocks, maxSrcSize, 1) bytes and runs the high-ratio kernels in passes of as
 *   many slices as it holds: a smaller scratch means more passes and the same bytes.
 * Asynchronous, no allocation, no sync, graph-capturable: plan, three launches per pass, offsets,
 * stitch and (with an index) one more, their number decided on the host.  APE_LZ4_GPU_EINVAL
 * before any device call for a null array or nblocks < 0, depth outside 0..256, maxSrcSize
 * outside [1, 0x7E000000], a restartBytes that is neither 0 nor a positive multiple of S, a
 * misaligned d_index or a bad index_stride, and a null, misaligned or too small scratch
 * (APE_LZ4_gpu_last_error names the size needed); nblocks == 0 returns 0 and launches nothing. */
size_t APE_LZ4_compress_large_hc_scratch_size(int nblocks, int maxSrcSize, int passSlices);
int APE_LZ4_compress_large_hc_batch_dev(const char *const *d_src, const int *d_srcSize,
                                        char *const *d_dst, const int *d_dstCap, int *d_result,
                                        int nblocks, int maxSrcSize, int depth, void *d_scratch,
                                        size_t scratch_bytes, int restartBytes, void *d_index,
                                        size_t index_stride, void *stream);
/* Diagnostic (tools/hc_bench.py --large): the same call without an index and with HIP events
 * around its launches; waits for them and returns ms6[0..6) = plan, chain, search, parse
 * (each summed over the passes), offsets, stitch in milliseconds.  Synchronous, creates events:
 * not for graph capture. */
int APE_LZ4_compress_large_hc_timed_dev(const char *const *d_src, const int *d_srcSize,
                                        char *const *d_dst, const int *d_dstCap, int *d_result,
                                        int nblocks, int maxSrcSize, int depth, void *d_scratch,
                                        size_t scratch_bytes, int restartBytes, void *stream,
                                        float *ms6);
/* APE_LZ4_compress_large_hc_opt_batch_dev is APE_LZ4_compress_large_hc_batch_dev with the
 * cost-minimising parse (above) on the slices: slice k gets the bytes of
 * APE_LZ4_compress_hc_opt_withPrefix_batch_dev, an input of at most 65536 bytes those of
 * APE_LZ4_compress_hc_opt_batch_dev.  Slicing, restart points, the seek index, the stitch, the
 * results, the errors and the decoders that read the blocks are unchanged.
 * DETERMINISM: a pure function of (input bytes, used history, depth, restartBytes);
 *   tests/hcoptmodel.py compress_large() is that function.
 * scratch : as above with 655360 bytes of tables per slice of a pass instead of 393216
 *   (APE_LZ4_compress_large_hc_opt_scratch_size).  Plan, three launches per pass, offsets,
 *   stitch and (with an index) one more. */
size_t APE_LZ4_compress_large_hc_opt_scratch_size(int nblocks, int maxSrcSize, int passSlices);
int APE_LZ4_compress_large_hc_opt_batch_dev(const char *const *d_src, const int *d_srcSize,
                                            char *const *d_dst, const int *d_dstCap,
                                            int *d_result, int nblocks, int maxSrcSize, int depth,
                                            void *d_scratch, size_t scratch_bytes,
                                            int restartBytes, void *d_index, size_t index_stride,
                                            void *stream);

/* ---- byte ranges of indexed blocks (lz4_decode.hip) ----
 * APE_LZ4_decompress_range_indexed_batch_dev decodes, for each REQUEST, the bytes
 * [rangeStart, rangeStart + rangeLen) of an indexed block without decoding the block: only the
 * segments that cover the range are parsed.  The batch dimension is the request; d_src,
 * d_compressedSize and d_index describe nblocks blocks as in the whole-block call, every
 * other array has nreq entries, and d_blockOf[r] names request r's block (NULL: request r
 * reads block r, and nreq == nblocks).  Many requests may name one block; each has its own
 * d_dst[r].  Two stream-ordered launches, no scratch, no allocation, no sync,
 * graph-capturable.  The index is never trusted.
 *
 * For request r on block i, with n and c from the index, a = d_rangeStart[r] and
 * m = min(d_rangeLen[r], n - a):
 *   - d_result[r] = -1 for d_blockOf[r] outside [0, nblocks), a < 0, d_rangeLen[r] < 0, a > n,
 *     or a header the whole-block call rejects (there is no capacity to compare n with; an
 *     n >= 2^31 is rejected); APE_LZ4_GPU_ERANGE for nseg > maxSegments; both leave
 *     d_window = {0, 0};
 *   - m == 0: d_result[r] = 0, nothing is written, d_window = {0, 0}.
 * Otherwise the covering segments j0 (of a) and j1 (of a + m - 1) come from this binary search
 * of the op column, for x = a and x = a + m - 1: lo = 0, hi = nseg; while hi - lo > 1:
 * mid = (lo + hi) / 2, lo = mid if op_mid <= x, else hi = mid; j = lo.  The request is -1
 * unless op_j0 <= a < op_{j0+1}, op_j1 <= a + m - 1 < op_{j1+1} and j0 <= j1 (a column that
 * is not sorted can fail this).
 *
 * Final run.  Segment nseg - 1 is ONE FINAL LITERAL RUN when, with L = n - op_last,
 * c - ip_last == 1 + lenbytes(L) + L (lenbytes(L) = 0 for L < 15, else (L - 15) / 255 + 1) and
 * the bytes say so: the token's high nibble is min(L, 15), every length byte but the last is
 * 255 and the last is (L - 15) % 255.  (The closed form alone is met by a segment of
 * 15-literal, 4-byte-match sequences too.)  When j1 = nseg - 1 is such a run, only its bytes
 * [max(a, op_last), a + m) are copied: a read from an incompressible block costs its own size.
 *
 * Window.  lo = a if j0 is the verified final run, else op_j0.  E = a + m if j1 is the
 * verified final run, else op_{j1+1}.  hi = min(E + 16, n): the 16 covers the 12 bytes that the
 * reference's end-of-output tests want after a sequence, so every sequence that ends at or
 * before E is judged as in mid-block; but hi = E when j0 is the verified final run, where
 * nothing is decoded and the range is copied (need = m: a 4 KiB read from an incompressible
 * block takes a 4 KiB destination).  need = hi - lo bytes of d_dst[r] are used:
 * d_window[2r] = a - lo (where the range begins in d_dst[r]), d_window[2r + 1] = need.
 * d_dstCap[r] < need gives APE_LZ4_GPU_ERANGE with nothing written: read need from d_window and
 * retry.  Otherwise the first launch writes d_result[r] = m.
 *
 * The second launch is nreq x wavesPerRequest waves (fewer than 2^31): wave k of request r
 * decodes segments j0 + k, j0 + k + wavesPerRequest, ... up to j1, so wavesPerRequest is a
 * parallelism knob only.  Segment j is decoded as by the whole-block call -- src + ip_j, the
 * block's true end, floor op_j, the stop at ip_{j+1}, the same pair checks and success rule --
 * into d_dst[r] + (op_j - lo) with the output room hi - op_j, whatever d_dstCap[r] is, so a
 * result never depends on spare capacity.  An op_j outside [lo, hi] fails like a wrong pair
 * (p = ip_j).  Failures record -(p)-1 with the smallest p, as in the whole-block call.
 *   - Nothing outside src[0, c), the index and dst[0, need) is accessed, whatever the input.
 *   - d_result[r] = m > 0: dst[d_window[2r], +m) is what this segment decode of the covering
 *     segments gives; bytes of dst[0, need) outside it are unspecified.
 *   - For every (block, index) the whole-block call accepts, that is APE_LZ4_decompress_safe's
 *     bytes [a, a + m).
 *   - Segments before j0 are not parsed: a forged index over a valid block can select other
 *     bytes.  It cannot reach out of bounds.
 * The decode does not stop inside segment j1 once a + m is reached (that needs another flag
 * in the decoder's hot loop): a request costs its covering segments, and restartBytes is the
 * granularity knob.
 * APE_LZ4_GPU_EINVAL before any device call: a null array (d_blockOf may be NULL only when
 * nreq == nblocks), a negative count, wavesPerRequest < 1, nreq x wavesPerRequest >= 2^31,
 * maxSegments < 1, a misaligned index, a stride below 16 + 8 (maxSegments + 1) or no multiple
 * of 16. */
int APE_LZ4_decompress_range_indexed_batch_dev(const char *const *d_src,
                                               const int *d_compressedSize, const void *d_index,
                                               size_t index_stride, int maxSegments, int nblocks,
                                               const int *d_blockOf, const int *d_rangeStart,
                                               const int *d_rangeLen, char *const *d_dst,
                                               const int *d_dstCap, int *d_window, int *d_result,
                                               int nreq, int wavesPerRequest, void *stream);

/* One-shot routing: ape_lz4.h one-shot calls on blocks smaller than
 * `bytes` (compress: input size; decompress_safe/_partial: capacity) run the host codec,
 * which is byte-identical to the reference; larger ones run on the GPU.  The default is
 * 0x7FFFFFFF -- every one-shot call on the host, because one GPU call costs 40-850 us
 * against 2-47 us on one host core for 1-64 KiB -- or the value of
 * the APE_LZ4_ONESHOT_HOST_BELOW environment variable; 0 puts every one-shot call on the
 * GPU.  The batch entry points below always run on the GPU.  Returns the previous
 * threshold. */
int APE_LZ4_gpu_set_oneshot_host_below(int bytes);

/* ---- batched, device-resident, strided form (block i at base + i*stride) ----
 * The layout the benchmark uses: uncompressed slots of `src_stride` bytes,
 * compressed slots of `dst_stride` bytes; a NULL cap array means
 * "capacity = compressBound(srcSize)" / "= dst_stride". */
int APE_LZ4_compress_batch_strided_dev(const char *d_src, size_t src_stride,
                                       const int *d_srcSize, char *d_dst, size_t dst_stride,
                                       const int *d_dstCap, int *d_result, int nblocks,
                                       void *stream);
int APE_LZ4_decompress_safe_batch_strided_dev(const char *d_src, size_t src_stride,
                                              const int *d_compressedSize, char *d_dst,
                                              size_t dst_stride,
                                              const int *d_maxDecompressedSize,
                                              int *d_result, int nblocks, void *stream);

/* ---- framed stream of independent blocks (socket path) ----
 * The reference socket stream frames each LZ4 block as [int32 size][block]
 * (ref src/ape_socket.c:813-850) with chained blocks; this batched form keeps
 * the frame layout (little-endian size) with independent blocks, back to back.
 *   frame_offsets : d_off[i] = sum_{j<i} (4 + d_compressedSize[j]) for i <= N
 *                   (d_off has N + 1 entries, d_off[N] = stream length);
 *                   d_scratch = APE_LZ4_frame_scratch_size(N) bytes of device memory
 *   frame_pack    : compressed slots (block i at d_comp + i*comp_stride) -> frames
 *   decompress_safe_frames : block i read from d_frames + d_off[i] (size from its
 *                   header), decoded to d_dst + i*dst_stride; results as
 *                   APE_LZ4_decompress_safe. */
size_t APE_LZ4_frame_scratch_size(int nblocks);
int APE_LZ4_frame_offsets_dev(const int *d_compressedSize, long long *d_off, void *d_scratch,
                              int nblocks, void *stream);
int APE_LZ4_frame_pack_strided_dev(const char *d_comp, size_t comp_stride,
                                   const int *d_compressedSize, const long long *d_off,
                                   char *d_frames, int nblocks, void *stream);
int APE_LZ4_decompress_safe_frames_dev(const char *d_frames, const long long *d_off,
                                       char *d_dst, size_t dst_stride,
                                       const int *d_maxDecompressedSize, int *d_result,
                                       int nblocks, void *stream);

/* ---- host-buffer batch (socket / ape_buffer path): pinned staging, H2D,
 * kernel, D2H on an internal stream; synchronous.  h_result as above. */
int APE_LZ4_compress_batch_host(const char *const *h_src, const int *h_srcSize,
                                char *const *h_dst, const int *h_dstCap, int *h_result,
                                int nblocks);
int APE_LZ4_decompress_safe_batch_host(const char *const *h_src, const int *h_compressedSize,
                                       char *const *h_dst, const int *h_maxDecompressedSize,
                                       int *h_result, int nblocks);

/* ---- socket path (BASELINE config 5; lz4_sock.hip) ----
 * APE_LZ4_rxbuf: the receive buffer of ape_socket (`buffer`, ref src/ape_buffer.c:210-228)
 * as a growable host buffer registered with hipHostRegister, plus a frame parser for the
 * [le32 size][block] stream that is correct across any read boundaries (the reference's
 * parser desyncs, src/ape_socket.c:1372-1379).
 *   rxbuf_prepare(b, n) : >= n free bytes after `used` (realloc + re-register); 0 / -1
 *   rxbuf_append        : copy bytes in (what a read() into data + used does)
 *   rxbuf_frames        : off[0..n) = complete frames' header positions, off[n] = their end;
 *                         returns n (<= max_frames), or -1 for a size < 0 or > max_block
 *   rxbuf_consume(b, k) : drop the first k bytes
 * socket_send_blocks : nblocks host blocks -> GPU encode -> frames -> write(fd); returns the
 *                      bytes written or an APE_LZ4_GPU_E* code.
 * socket_recv_blocks : read(fd) -> rxbuf -> GPU decode from the frames -> host blocks;
 *                      h_result[i] as decompress_safe; returns the blocks received, or an
 *                      APE_LZ4_GPU_E* code (EINVAL also for a malformed stream / early EOF).
 * Both are blocking calls for one connection; each overlaps socket I/O with GPU work. */
typedef struct APE_LZ4_rxbuf APE_LZ4_rxbuf;
APE_LZ4_rxbuf *APE_LZ4_rxbuf_new(size_t initial);
int APE_LZ4_rxbuf_prepare(APE_LZ4_rxbuf *b, size_t more);
int APE_LZ4_rxbuf_append(APE_LZ4_rxbuf *b, const char *data, size_t len);
int APE_LZ4_rxbuf_frames(const APE_LZ4_rxbuf *b, long long *off, int max_frames, int max_block);
void APE_LZ4_rxbuf_consume(APE_LZ4_rxbuf *b, size_t n);
char *APE_LZ4_rxbuf_data(APE_LZ4_rxbuf *b);
size_t APE_LZ4_rxbuf_used(const APE_LZ4_rxbuf *b);
size_t APE_LZ4_rxbuf_room(const APE_LZ4_rxbuf *b);
int APE_LZ4_rxbuf_pinned(const APE_LZ4_rxbuf *b);
void APE_LZ4_rxbuf_free(APE_LZ4_rxbuf *b);
long long APE_LZ4_socket_send_blocks(int fd, const char *h_src, size_t src_stride, int block_size,
                                     int nblocks, int batch);
long long APE_LZ4_socket_recv_blocks(int fd, char *h_dst, size_t dst_stride, int block_size,
                                     int nblocks, int batch, int *h_result);

/* ---- chained socket streams: the reference wire format through the GPU (lz4_sock.hip) ----
 * nconn connections, each a stream exactly as the reference socket writes and reads it:
 * every message cut into 8 KiB chunks, each compressed against the previous <= 64 KiB of
 * its stream and framed [int32 size][block] (ref src/ape_socket.c:811-871); the receiver
 * decodes each frame against the previous 64 KiB it decoded (:1333-1467).  An unmodified
 * reference peer reads what chain_send writes and writes what chain_recv reads.
 *   chain_new(nconn, msg_len) : device history windows for nconn send and nconn receive
 *                        streams, msg_len bytes per message (NULL on failure)
 *   chain_send         : nmsg rounds; round m compresses message m of every connection
 *                        (at h_msgs + (m * nconn + i) * msg_stride) in one GPU launch (a
 *                        chunk's history is plaintext the sender has) and writes connection
 *                        i's frames to fds[i].  Returns the bytes written or APE_LZ4_GPU_E*.
 *   chain_recv         : nmsg rounds; reads every fd (poll), parses each connection's frames
 *                        split-safe, decodes round m's message of every connection with one
 *                        usingDict launch per 8 KiB chunk (the connections are the batch) into
 *                        h_out + (m * nconn + i) * out_stride.  h_status[i] = 0 or the first
 *                        bad result of connection i.  Returns the payload bytes or
 *                        APE_LZ4_GPU_E* (EINVAL: malformed frame, early EOF, failed decode).
 * One thread may send while another receives on the same chain.  Errors are sticky per
 * direction: a failed call has consumed frames / advanced the streams it ran, so every later
 * call in that direction returns APE_LZ4_GPU_EINVAL (h_status[i] = -1); free the chain. */
typedef struct APE_LZ4_chain APE_LZ4_chain;
APE_LZ4_chain *APE_LZ4_chain_new(int nconn, int msg_len);
void APE_LZ4_chain_free(APE_LZ4_chain *c);
long long APE_LZ4_chain_send(APE_LZ4_chain *c, const int *fds, const char *h_msgs,
                             size_t msg_stride, int nmsg);
long long APE_LZ4_chain_recv(APE_LZ4_chain *c, const int *fds, char *h_out, size_t out_stride,
                             int nmsg, int *h_status);

/* Time split of the socket calls since the last reset, out[16] in ms: TX [0] H2D, [1] encode
 * + frame offsets + pack (GPU), [2] D2H, [3] write(), [4] host waiting for the GPU, [5]
 * batches (count), [6] the whole send call; RX [7] the whole receive loop, [8] read(), [9]
 * frame parse + leftover copy, [10] H2D, [11] decode (GPU), [12] D2H, [13] host waiting for
 * the GPU, [14] batches (count), [15] receive-buffer growth.  GPU phases are timing events
 * around each batch's stages.  reset != 0 zeroes the counters. */
int APE_LZ4_socket_stats(double *out16, int reset);

/* ---- synthetic benchmark data, device-side ----
 * kind 0 = random bytes, 1 = compressible; block b is seeded with first_block+b. */
int APE_LZ4_synth_blocks_dev(char *d_out, size_t stride, int blockSize,
                             long long first_block, int nblocks, int kind, void *stream);

#if defined(__cplusplus)
}
#endif

#include "ape_lz4_dict_train.h"
#include "ape_lz4_cdicts.h"
