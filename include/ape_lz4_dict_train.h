/* ape_lz4_dict_train.h -- dictionary training on the MI355X: the part of the batched GPU API
 * (ape_lz4_gpu.h, which includes this file and defines the return codes) that builds the
 * dictionary the prepared-dictionary calls start from.  Same conventions: device pointers,
 * asynchronous on `stream`, APE_LZ4_GPU_OK or a negative APE_LZ4_GPU_E* code. */
#pragma once
#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

/* ---- dictionary training (lz4_dict_train.hip) ----
 * The step before cdict_prepare / hc_cdict_prepare: a dictionary of dictCapacity bytes built
 * from a batch of device-resident sample messages (in the sense of zstd's
 * ZDICT_trainFromBuffer).  d_dict can go straight into either prepare call on the same stream.
 *
 * THE RULE is tests/dicttrainmodel.py's, byte for byte.  With k = segmentSize, st = k / 4 and
 * J = ceil(maxSampleSize / st):
 *   counts : freq[idx] = the number of positions p, p + 8 <= size_i, over all samples, whose 8
 *     bytes have table index idx = (the bytes as a little-endian u64 * 0x9E3779B185EBCA87 mod
 *     2^64) >> 44 (a table of 2^20 entries).  No counted substring crosses into another sample.
 *     A negative size counts as 0.  A sample larger than maxSampleSize is IGNORED: not counted,
 *     no candidates, nothing of it is read; d_info counts such samples.
 *   slots  : slot c = i * J + j (0 <= j < J) is the segment [j * st, j * st + n) of sample i, n =
 *     min(k, size_i - j * st); it is empty when n < 8.  Its score is the sum of freq[idx] over
 *     the DISTINCT indices of its n - 7 substrings.
 *   rounds : E = dictCapacity / k rounds; round e looks at the slots [e * M / E, (e + 1) * M / E),
 *     M = nsamples * J, and picks the one with the highest score, the lowest slot on a tie, none
 *     when every score is 0.  A pick then sets freq[idx] = 0 for every substring of its segment,
 *     so later rounds are paid for new material only.  There is one cycle over the rounds.
 *   layout : pick 0 is the dictionary's LAST bytes (prepare keeps the tail when it has to cut),
 *     pick r ends where pick r - 1 begins, and the dictionary starts with dictCapacity - u zero
 *     bytes, u the picks' total: u < dictCapacity when rounds come up empty or segments are cut
 *     by their sample's end.
 *   d_info[0..4) = {u, number of picks, samples ignored, 0}.
 * Deterministic: the counts are integer adds, which commute, and every choice is the rule's, so
 * two calls on the same samples give identical bytes whatever the scratch held.
 *
 * Arguments: segmentSize a multiple of 16 in [16, 1024]; dictCapacity in [segmentSize, 65536];
 * maxSampleSize in [8, 0x7E000000], a host-side bound that sizes the slot grid;
 * nsamples * maxSampleSize <= 2^31 - 1, so that no count wraps.  nsamples == 0 is legal (the
 * arrays may then be NULL): an all-zero dictionary and d_info = {0, 0, 0, 0}.
 * Reads d_sampleSize[0, nsamples) and, of a sample with 8 <= size <= maxSampleSize, d_samples[i]
 * and d_samples[i][0, size) at any alignment, nothing else.  Writes EVERY byte of d_dict[0,
 * dictCapacity) and of d_info[0, 4), and nothing else outside the scratch.
 * scratch : the caller's, 16-byte aligned, at least scratch_size(nsamples, maxSampleSize,
 *   segmentSize) bytes: the count table (4 MiB), the state and one partial result per score
 *   workgroup; a multiple of 16, 0 for arguments out of range.  Every scratch byte the call reads
 *   it has written before, in the same call.
 * Asynchronous, no allocation, no sync, graph-capturable: 3 + 2 * E stream-ordered launches at
 * most, their number decided on the host.
 * APE_LZ4_GPU_EINVAL before any device call for a null array (nsamples > 0), a null d_dict or
 * d_info, nsamples < 0, any parameter out of range, the product bound, a null, misaligned or too
 * small scratch. */
size_t APE_LZ4_dict_train_scratch_size(int nsamples, int maxSampleSize, int segmentSize);
int APE_LZ4_dict_train_dev(const char *const *d_samples, const int *d_sampleSize, int nsamples,
                           int maxSampleSize, char *d_dict, int dictCapacity, int segmentSize,
                           void *d_scratch, size_t scratch_bytes, int *d_info, void *stream);

#if defined(__cplusplus)
}
#endif
