// lz4_encode_hc.hip -- the high-ratio encoder on a contiguous window
// (APE_LZ4_compress_hc_batch_dev; APE_LZ4_compress_hc_opt_batch_dev, 3.16).
//
// Three launches per pass over caller-owned scratch (lz4_gpu_internal.h, HcArgs / HcOptArgs):
// chain build (one wave per block), search (one lane per position), then the lazy parse or the
// cost-minimising parse (one wave per block).  The stages are lz4_hc_common.h's, over FlatView.
//
// With history (HcArgs::prefix) the window is [src - h, src + n), h =
// min(prefix, 65536 - n) bytes of history and the block: chain[], match[] and cost[] are
// indexed by window position (h + n <= 65536, so position + 1 stays inside u16), the chains run
// over the whole window, and only the block's positions are searched and parsed.
#include "lz4_hc_common.h"

namespace apelz4 {
namespace {

constexpr int kHcSearchThreads = 256;
constexpr int kHcGroups = kMaxBlock / kHcSearchThreads;   // search workgroups per block

// The window of block b (of 0 <= n <= kMaxBlock bytes).  Its history: what the caller offers,
// as far as one window of u16 positions holds it; not rounded, a negative prefix counts as none.
__device__ __forceinline__ FlatView open_window(const HcArgs &a, int b, int n) {
    const int hist = a.prefix ? max(0, min(a.prefix[b], kMaxBlock - n)) : 0;
    return FlatView{(gcu8 *)a.src[b] - hist, hist, a.chain + (size_t)b * kMaxBlock};
}

// a block the parse kernels read nothing more of (a slot of size -1 not even its tail)
__device__ __forceinline__ bool rejected(const HcArgs &a, int b, int n, int cap, int lane) {
    if (n >= 0 && n <= kMaxBlock && cap > 0) return false;
    if (lane == 0) {
        a.result[b] = n > kMaxBlock ? kErange : 0;
        if (a.tail && n >= 0) a.tail[b] = 0;
    }
    return true;
}

// the large path (lz4_large.hip) stitches slices at their final literal runs
__device__ __forceinline__ void report(const HcArgs &a, int b, int lane, int result, uint32_t tail) {
    if (lane == 0) {
        a.result[b] = result;
        if (a.tail) a.tail[b] = (int)tail;
    }
}

}  // namespace

__global__ void __launch_bounds__(64) lz4_hc_chain_kernel(HcArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b];
    if (n < kMinLength || n > kMaxBlock) return;   // no position can match: nothing is read
    const FlatView W = open_window(a, b, n);
    for (int i = lane; i < kHcTable / 8; i += 64) ((uint4 *)head)[i] = make_uint4(0u, 0u, 0u, 0u);
    wave_sync();
    hc_chain_build(W, head, 0, W.origin + n - kMinMatch, lane);
}

__global__ void __launch_bounds__(kHcSearchThreads) lz4_hc_search_kernel(HcArgs a) {
    const int b = blockIdx.x / kHcGroups;
    const int n = a.src_size[b];
    if (n < kMinLength || n > kMaxBlock) return;
    // (a workgroup past the block's last searchable position leaves here)
    const int i = (int)(blockIdx.x % kHcGroups) * kHcSearchThreads + (int)threadIdx.x;
    if (i > n - kMFLimit) return;
    const FlatView W = open_window(a, b, n);
    a.match[(size_t)b * kMaxBlock + W.origin + i] = hc_search(W, n, i, a.depth);
}

__global__ void __launch_bounds__(64) lz4_hc_parse_kernel(HcArgs a) {
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b], cap = a.dst_cap[b];
    if (rejected(a, b, n, cap, lane)) return;
    const FlatView W = open_window(a, b, n);
    Emitter em{(gu8 *)a.dst[b], W.block(), (uint32_t)cap, 0u, lane};
    uint32_t tail;
    const int result = hc_lazy_parse(W, n, a.match + (size_t)b * kMaxBlock + W.origin, em, &tail);
    report(a, b, lane, result, tail);
}

__global__ void __launch_bounds__(64) lz4_hc_opt_parse_kernel(HcOptArgs o) {
    const HcArgs &a = o.a;
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b], cap = a.dst_cap[b];
    if (rejected(a, b, n, cap, lane)) return;
    const FlatView W = open_window(a, b, n);
    Emitter em{(gu8 *)a.dst[b], W.block(), (uint32_t)cap, 0u, lane};
    const size_t first = (size_t)b * kMaxBlock + W.origin;
    uint32_t tail;
    const int result = hc_opt_parse(W, n, a.match + first, o.cost + first, em, a.tail != nullptr, &tail);
    report(a, b, lane, result, tail);
}

namespace {

// ev (nullable): three events, recorded after the chain, the search and the parse launch
template <class Parse, class Args>
hipError_t launch_stages(const HcArgs &a, Parse parse, const Args &pa, hipStream_t s, hipEvent_t *ev) {
    if (a.nblocks <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(lz4_hc_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    if (ev) e = hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(lz4_hc_search_kernel, dim3((unsigned)a.nblocks * kHcGroups),
                       dim3(kHcSearchThreads), 0, s, a);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(parse, dim3(a.nblocks), dim3(64), 0, s, pa);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[2], s);
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : e;
}

}  // namespace

hipError_t launch_encode_hc(const HcArgs &a, hipStream_t s, hipEvent_t *ev) {
    return launch_stages(a, lz4_hc_parse_kernel, a, s, ev);
}

hipError_t launch_encode_hc_opt(const HcOptArgs &o, hipStream_t s, hipEvent_t *ev) {
    return launch_stages(o.a, lz4_hc_opt_parse_kernel, o, s, ev);
}

}  // namespace apelz4
