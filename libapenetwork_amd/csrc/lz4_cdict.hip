// lz4_cdict.hip -- MI355X (gfx950): the prepare kernel of a prepared dictionary.
//
// APE_LZ4_compress_usingCDict_batch_dev is N x (loadDict ; compress_fast_continue) (ref
// src/ape_lz4.c:1101-1133, :1160-1220) with one dictionary shared by every block.  loadDict's
// work -- hashing the dictionary into the table -- is done here once, not per block: this
// kernel writes the device object the encoder's EXT instantiation (lz4_encode.hip) starts
// from.  Layout and constants: lz4_gpu_internal.h.
//
// One workgroup of four waves.  Wave 0 builds the table in LDS exactly as the encoder's
// prefix_history does for positions of the dictionary alone: every third window position v
// with v + 8 <= D, oldest first, the value v itself.  One wave, so its LDS writes land in
// program order and the newest position of a slot wins deterministically.  The other three
// waves meanwhile write the header, the window copy and every pad byte; then all four store
// the table image.  Every byte of the object is written, so two prepares of the same input
// give identical objects.
//
// APE_LZ4_cdict_prepare_batch_dev is the same body, one workgroup per object of a
// batch: lz4_cdict_prepare.inc, included into both kernels.
#include "lz4_gpu_internal.h"

namespace apelz4 {

namespace {

constexpr int kPrepThreads = 256;

__global__ void __launch_bounds__(kPrepThreads)
lz4_cdict_prepare_kernel(const char *dict, int dict_size, int max_src, uint8_t *cd) {
#include "lz4_cdict_prepare.inc"
}

// Object blockIdx.x of a batch (APE_LZ4_cdict_prepare_batch_dev), from the
// device arrays' entry.  The sizes were never on the host: an entry no single prepare would take
// (a negative size, a null pointer with a positive one) gets sixteen zero bytes as its header,
// which every compress rejects, and nothing else of its object is written.
__global__ void __launch_bounds__(kPrepThreads)
lz4_cdict_prepare_batch_kernel(const char *const *dicts, const int *dict_sizes, int max_src,
                               uint8_t *cds, size_t stride) {
    const char *dict = wave_uniform(dicts[blockIdx.x]);
    const int dict_size = (int)wave_first((uint32_t)dict_sizes[blockIdx.x]);
    uint8_t *cd = cds + (size_t)blockIdx.x * stride;
    if (dict_size < 0 || (dict_size > 0 && !dict)) {
        if (threadIdx.x == 0) gstore16((gu8 *)cd, make_uint4(0, 0, 0, 0));
        return;
    }
#include "lz4_cdict_prepare.inc"
}

}  // namespace

hipError_t launch_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                hipStream_t s) {
    hipLaunchKernelGGL(lz4_cdict_prepare_kernel, dim3(1), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdict);
    return hipGetLastError();
}

hipError_t launch_cdict_prepare_batch(const char *const *dict, const int *dict_size, int max_src,
                                      void *cdicts, size_t stride, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lz4_cdict_prepare_batch_kernel, dim3(n), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdicts, stride);
    return hipGetLastError();
}

}  // namespace apelz4
