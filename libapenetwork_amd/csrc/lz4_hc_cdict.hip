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
#include "lz4_hc_common.h"

namespace apelz4 {
namespace {

constexpr int kPrepThreads = 256;

// The window of one message: positions [0, D) in the object, [D, D + n) in the message.
struct SplitView {
    gcu8 *dict, *msg;
    int origin;               // D
    const uint16_t *shared;   // chain[w] of w < D - 3: the object's ...
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
__device__ __forceinline__ bool open_object(const HcDictArgs &a, SplitView *w, int b) {
    const CDictHdr H = *(const CDictHdr *)a.cdict;
    if (H.magic != kHdMagic || H.max_src != (uint32_t)a.max_src || H.zero != 0u ||
        H.D > (uint32_t)(kMaxBlock - a.max_src))
        return false;
    w->dict = (gcu8 *)a.cdict + (kHdWin + kCdFront);
    w->msg = (gcu8 *)a.src[b];
    w->origin = (int)H.D;
    w->shared = (const uint16_t *)(a.cdict + kHdChain);
    w->own = a.chain + (size_t)b * a.chain_stride;
    return true;
}

// a message the parse kernels read nothing of; *n and *cap otherwise
__device__ __forceinline__ bool open_parse(const HcDictArgs &a, SplitView *w, int b, int lane, int *n,
                                           int *cap) {
    *n = a.src_size[b];
    *cap = a.dst_cap[b];
    const bool ok = open_object(a, w, b);
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
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = hc_cdict_window(dict_size, max_src);
    gcu8 *src = (gcu8 *)dict + (dict_size - D);   // window position v = src[v]
    const int nchain = max(D - 3, 0);             // chain entries the build writes

    for (int i = tid; i < kHcTable / 8; i += kPrepThreads) ((uint4 *)head)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    if (wave == 0) {
        hc_chain_build(FlatView{src, 0, (uint16_t *)(cd + kHdChain)}, head, 0, nchain - 1, lane);
    } else {
        const uint32_t t = (uint32_t)tid - 64u, nt = kPrepThreads - 64;
        if (t == 0) {
            CDictHdr H;
            H.magic = kHdMagic;
            H.D = (uint32_t)D;
            H.max_src = (uint32_t)max_src;
            H.zero = 0u;
            *(CDictHdr *)cd = H;
        }
        // chain[nchain, 65536) = 0: whole 16-byte pieces, and the entries of the piece that
        // wave 0 shares one by one
        gu8 *cz = (gu8 *)cd + kHdChain;
        for (uint32_t i = t; i < (uint32_t)kMaxBlock / 8u; i += nt) {
            const uint32_t e = 8u * i;   // first entry of the piece
            if (e >= (uint32_t)nchain) {
                gstore16(cz + 16u * i, make_uint4(0, 0, 0, 0));
            } else if (e + 8u > (uint32_t)nchain) {
                for (uint32_t j = (uint32_t)nchain; j < e + 8u; j++) ((uint16_t *)(cd + kHdChain))[j] = 0;
            }
        }
        // [kHdWin, kHdSize) in 16-byte pieces: pad, window, pad (the window's last piece byte
        // by byte: nothing past the dictionary's end is read)
        gu8 *w = (gu8 *)cd + kHdWin;
        constexpr uint32_t kPieces = (kHdSize - kHdWin) / 16u;
        for (uint32_t i = t; i < kPieces; i += nt) {
            const uint32_t at = 16u * i;          // byte of the region; window byte at - kCdFront
            uint4 v = make_uint4(0, 0, 0, 0);
            if (at >= kCdFront && at - kCdFront < (uint32_t)D) {
                const uint32_t v0 = at - kCdFront;
                if (v0 + 16u <= (uint32_t)D) {
                    v = gload16(src + v0);
                } else {
                    uint32_t x[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t j = 0; v0 + j < (uint32_t)D; j++)
                        x[j >> 2] |= (uint32_t)src[v0 + j] << (8u * (j & 3u));
                    v = make_uint4(x[0], x[1], x[2], x[3]);
                }
            }
            gstore16(w + at, v);
        }
    }
    __syncthreads();
    uint4 *img = (uint4 *)(cd + kHdHead);
    for (int i = tid; i < kHcTable / 8; i += kPrepThreads) img[i] = ((const uint4 *)head)[i];
}

// ---- the stages of one message ----
__global__ void __launch_bounds__(64) lz4_hc_cdict_chain_kernel(HcDictArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    if (!open_object(a, &W, b)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;   // no position can match: nothing is read
    const uint4 *img = (const uint4 *)(a.cdict + kHdHead);
    for (int i = lane; i < kHcTable / 8; i += 64) ((uint4 *)head)[i] = img[i];
    wave_sync();
    // positions D - 3 .. D + n - 4 (from 0 when the dictionary is shorter than 3 bytes)
    hc_chain_build(W, head, max(W.origin - 3, 0), W.origin + n - kMinMatch, lane);
}

__global__ void __launch_bounds__(kHcdThreads) lz4_hc_cdict_search_kernel(HcDictArgs a, int groups) {
    const int b = blockIdx.x / groups;
    SplitView W;
    if (!open_object(a, &W, b)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;
    // (a workgroup past the last searchable position leaves here)
    const int i = (int)(blockIdx.x % groups) * kHcdThreads + (int)threadIdx.x;
    if (i > n - kMFLimit) return;
    a.match[(size_t)b * a.match_stride + i] = hc_search(W, n, i, a.depth);
}

__global__ void __launch_bounds__(64) lz4_hc_cdict_parse_kernel(HcDictArgs a) {
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    int n, cap;
    if (!open_parse(a, &W, b, lane, &n, &cap)) return;
    Emitter em{(gu8 *)a.dst[b], W.msg, (uint32_t)cap, 0u, lane};
    uint32_t tail;
    const int result = hc_lazy_parse(W, n, a.match + (size_t)b * a.match_stride, em, &tail);
    if (lane == 0) a.result[b] = result;
}

__global__ void __launch_bounds__(64) lz4_hc_cdict_opt_parse_kernel(HcDictOptArgs o) {
    const HcDictArgs &a = o.a;
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    int n, cap;
    if (!open_parse(a, &W, b, lane, &n, &cap)) return;
    Emitter em{(gu8 *)a.dst[b], W.msg, (uint32_t)cap, 0u, lane};
    uint32_t tail;
    const int result = hc_opt_parse(W, n, a.match + (size_t)b * a.match_stride,
                                    o.cost + (size_t)b * o.cost_stride, em, false, &tail);
    if (lane == 0) a.result[b] = result;
}

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

}  // namespace

hipError_t launch_hc_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                   hipStream_t s) {
    hipLaunchKernelGGL(lz4_hc_cdict_prepare_kernel, dim3(1), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdict);
    return hipGetLastError();
}

hipError_t launch_encode_hc_cdict(const HcDictArgs &a, hipStream_t s) {
    return launch_stages(a, lz4_hc_cdict_parse_kernel, a, s);
}

hipError_t launch_encode_hc_cdict_opt(const HcDictOptArgs &o, hipStream_t s) {
    return launch_stages(o.a, lz4_hc_cdict_opt_parse_kernel, o, s);
}

}  // namespace apelz4
