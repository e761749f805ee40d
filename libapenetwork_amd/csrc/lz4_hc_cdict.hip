// lz4_hc_cdict.hip -- the high-ratio mode against a prepared dictionary shared by a batch
// (APE_LZ4_hc_cdict_prepare_dev, APE_LZ4_compress_hc_usingCDict_batch_dev, DESIGN.md 3.15;
// APE_LZ4_compress_hc_opt_usingCDict_batch_dev, 3.17).
//
// The block of message m is compress_hc_withPrefix's for the window [dictionary tail | m]
// (tests/hcdictmodel.py is the definition), without staging that window: window position w is
// the object's byte w when w < D and the message's byte w - D otherwise.  The chain build over
// the positions whose 4 bytes lie in the dictionary is done once, by the prepare kernel; a
// message's chain kernel starts from that head table and inserts only the positions D - 3 on
// (the first three straddle dictionary and message).  A chain walk follows the object's
// chain[] below D - 3 and the message's scratch from there on.  The stages are
// lz4_hc_common.h's, over SplitView; match[] and cost[] are indexed by message position.
//
// Every kernel checks the object's header before it uses anything else of it.
//
// Two forms of every kernel: one object for the batch, and (the usingCDicts calls,
// APE_LZ4_hc_cdict_prepare_batch_dev) one per message or per workgroup, from a device array.  The
// bodies are the same text, included into both (lz4_hc_cdict_stages.inc,
// lz4_hc_cdict_prepare.inc); the one-object kernels are instruction for instruction what they
// were before the second form existed (profiles/cdicts_asm_diff.txt).
#include "lz4_hc_common.h"

namespace apelz4 {
namespace {

constexpr int kPrepThreads = 256;

// The window of one message: positions [0, D) in the object, [D, D + n) in the message.
typedef __attribute__((address_space(1))) const uint16_t gcu16;
struct SplitView {
    gcu8 *dict, *msg;
    int origin;               // D
    gcu16 *shared;            // chain[w] of w < D - 3: the object's ...
    uint16_t *own;            // ... and from there on the message's scratch, entry w - D + 3
    __device__ __forceinline__ uint32_t byte(int w) const {
        return w < origin ? dict[w] : msg[w - origin];
    }
    __device__ __forceinline__ gcu8 *at(int w) const {
        return w < origin ? dict + w : msg + (w - origin);
    }
    // [w, w + len) lies wholly on one side
    __device__ __forceinline__ bool one_side(int w, int len) const {
        return w + len <= origin || w >= origin;
    }
    // at D - 3 .. D - 1 the 4 bytes come from both sides (the object's load runs into its back
    // pad, and those bytes are masked off; n >= 4)
    __device__ __forceinline__ uint32_t load4(int w) const {
        if (w >= origin) return gload4(msg + (w - origin));
        const uint32_t lo = gload4(dict + w);
        const int in = origin - w;
        if (in >= 4) return lo;
        return (lo & ((1u << (8 * in)) - 1u)) | gload4(msg) << (8 * in);
    }
    __device__ __forceinline__ gcu8 *block() const { return msg; }
    __device__ __forceinline__ uint32_t next(int w) const {
        return w < origin - 3 ? shared[w] : own[w - origin + 3];
    }
    __device__ __forceinline__ void set_next(int w, uint32_t v) const {
        own[w - origin + 3] = (uint16_t)v;
    }
};

// The header, before anything else of the object: true when it was prepared for a.max_src.
// PER: the call has an object per message, per[b] in place of a.cdict; a null
// or misaligned entry fails without a read.  A template flag and no runtime branch: the
// one-object kernels carry nothing of the other form.
template <bool PER = false>
__device__ __forceinline__ bool open_object(const HcDictArgs &a, SplitView *w, int b,
                                            const uint8_t *const *per = nullptr) {
    gcu8 *cd;
    if constexpr (PER) {
        cd = (gcu8 *)message_object(per, b);
        if (!cd) return false;
    } else {
        cd = (gcu8 *)a.cdict;
    }
    const CDictHdr H = object_header<PER>(cd);
    if (H.magic != kHdMagic || H.max_src != (uint32_t)a.max_src || H.zero != 0u ||
        H.D > (uint32_t)(kMaxBlock - a.max_src))
        return false;
    w->dict = cd + (kHdWin + kCdFront);
    w->msg = (gcu8 *)a.src[b];
    w->origin = (int)H.D;
    w->shared = (gcu16 *)(cd + kHdChain);
    w->own = a.chain + (size_t)b * a.chain_stride;
    return true;
}

// a message the parse kernels read nothing of; *n and *cap otherwise
template <bool PER = false>
__device__ __forceinline__ bool open_parse(const HcDictArgs &a, SplitView *w, int b, int lane, int *n,
                                           int *cap, const uint8_t *const *per = nullptr) {
    *n = a.src_size[b];
    *cap = a.dst_cap[b];
    const bool ok = open_object<PER>(a, w, b, per);
    if (ok && *n >= 0 && *n <= a.max_src && *cap > 0) return true;
    if (lane == 0) a.result[b] = ok && *n > a.max_src ? kErange : 0;
    return false;
}

// ---- prepare ----
// One workgroup of four waves.  Wave 0 runs the chain build over the dictionary's positions
// 0 .. D - 4 alone, 64 per step (one wave: the order is deterministic); the other three
// meanwhile write the header, the window with its pads and the zero rest of chain[].  Then all
// four store the head table.  Every byte of the object is written.
__global__ void __launch_bounds__(kPrepThreads)
lz4_hc_cdict_prepare_kernel(const char *dict, int dict_size, int max_src, uint8_t *cd) {
#include "lz4_hc_cdict_prepare.inc"
}

// Object blockIdx.x of a batch (APE_LZ4_hc_cdict_prepare_batch_dev); a bad entry gets a zero
// header and nothing else, as in lz4_cdict_prepare_batch_kernel (lz4_cdict.hip).
__global__ void __launch_bounds__(kPrepThreads)
lz4_hc_cdict_prepare_batch_kernel(const char *const *dicts, const int *dict_sizes, int max_src,
                                  uint8_t *cds, size_t stride) {
    const char *dict = wave_uniform(dicts[blockIdx.x]);
    const int dict_size = (int)wave_first((uint32_t)dict_sizes[blockIdx.x]);
    uint8_t *cd = cds + (size_t)blockIdx.x * stride;
    if (dict_size < 0 || (dict_size > 0 && !dict)) {
        if (threadIdx.x == 0) gstore16((gu8 *)cd, make_uint4(0, 0, 0, 0));
        return;
    }
#include "lz4_hc_cdict_prepare.inc"
}

// ---- the stages of one message ----
// one object for the batch ...
#define HCD_KERNEL(stage) lz4_hc_cdict_##stage##_kernel
#define HCD_PER false
#define HCD_PARAM
#define HCD_ARG
#define HCD_OBJECT a.cdict
#include "lz4_hc_cdict_stages.inc"
#undef HCD_KERNEL
#undef HCD_PER
#undef HCD_PARAM
#undef HCD_ARG
#undef HCD_OBJECT
// ... and one per message: a message whose entry or object fails reads nothing of the object in
// any stage, gets result 0 from the parse, and costs the other messages nothing
#define HCD_KERNEL(stage) lz4_hc_cdicts_##stage##_kernel
#define HCD_PER true
#define HCD_PARAM , const uint8_t *const *cdicts
#define HCD_ARG , cdicts
#define HCD_OBJECT (W.dict - (kHdWin + kCdFront))
#include "lz4_hc_cdict_stages.inc"
#undef HCD_KERNEL
#undef HCD_PER
#undef HCD_PARAM
#undef HCD_ARG
#undef HCD_OBJECT

template <class Parse, class Args>
hipError_t launch_stages(const HcDictArgs &a, Parse parse, const Args &pa, hipStream_t s) {
    if (a.nblocks <= 0) return hipSuccess;
    const int groups = hc_cdict_groups(a.max_src);
    hipLaunchKernelGGL(lz4_hc_cdict_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    hipLaunchKernelGGL(lz4_hc_cdict_search_kernel, dim3((unsigned)a.nblocks * groups),
                       dim3(kHcdThreads), 0, s, a, groups);
    hipLaunchKernelGGL(parse, dim3(a.nblocks), dim3(64), 0, s, pa);
    return hipGetLastError();
}

template <class Parse, class Args>
hipError_t launch_stages_per(const HcDictArgs &a, Parse parse, const Args &pa,
                             const uint8_t *const *cdicts, hipStream_t s) {
    if (a.nblocks <= 0) return hipSuccess;
    const int groups = hc_cdict_groups(a.max_src);
    hipLaunchKernelGGL(lz4_hc_cdicts_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a, cdicts);
    hipLaunchKernelGGL(lz4_hc_cdicts_search_kernel, dim3((unsigned)a.nblocks * groups),
                       dim3(kHcdThreads), 0, s, a, groups, cdicts);
    hipLaunchKernelGGL(parse, dim3(a.nblocks), dim3(64), 0, s, pa, cdicts);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_hc_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                   hipStream_t s) {
    hipLaunchKernelGGL(lz4_hc_cdict_prepare_kernel, dim3(1), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdict);
    return hipGetLastError();
}

hipError_t launch_hc_cdict_prepare_batch(const char *const *dict, const int *dict_size,
                                         int max_src, void *cdicts, size_t stride, int n,
                                         hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lz4_hc_cdict_prepare_batch_kernel, dim3(n), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdicts, stride);
    return hipGetLastError();
}

hipError_t launch_encode_hc_cdict(const HcDictArgs &a, hipStream_t s,
                                  const uint8_t *const *cdicts) {
    if (cdicts) return launch_stages_per(a, lz4_hc_cdicts_parse_kernel, a, cdicts, s);
    return launch_stages(a, lz4_hc_cdict_parse_kernel, a, s);
}

hipError_t launch_encode_hc_cdict_opt(const HcDictOptArgs &o, hipStream_t s,
                                      const uint8_t *const *cdicts) {
    if (cdicts) return launch_stages_per(o.a, lz4_hc_cdicts_opt_parse_kernel, o, cdicts, s);
    return launch_stages(o.a, lz4_hc_cdict_opt_parse_kernel, o, s);
}

}  // namespace apelz4
