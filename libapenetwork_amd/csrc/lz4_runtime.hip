// lz4_runtime.hip -- the thin C-ABI shim between the C host code and the HIP
// kernels: device checks, the batched launchers of include/ape_lz4_gpu.h, and
// the pinned-staging host path used by the one-shot ape_lz4.h calls.
//
// No CPU fallback anywhere: without a usable gfx950 device every entry point
// returns APE_LZ4_GPU_ENODEV (and the one-shot API reports failure).
//
// Every launcher reads: fill the kernel's argument struct, check the arguments, check the
// device, launch.  The argument checks come before the device check, so a bad call fails the
// same way on any machine (the few places that keep another order say so).
#include <initializer_list>
#include <mutex>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../include/ape_lz4_gpu.h"
#include "../../include/ape_lz4f.h"
#include "../../include/ape_lz4f_placed.h"
#include "../../include/ape_lz4f_dict.h"
#include "../../include/ape_lz4f_prefs.h"
#include "lz4_gpu_internal.h"
#include "lz4_gpu_shim.h"

using namespace apelz4;

namespace {

thread_local char g_err[256] = "";

void set_err(const char *what, hipError_t e) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, e == hipSuccess ? "ok" : hipGetErrorString(e));
}

// The one way to reject a call.  Every message starts with the entry point's name (its symbol
// without the APE_LZ4_ prefix), so APE_LZ4_gpu_last_error() never shows an earlier call's text.
__attribute__((format(printf, 1, 2))) int einval(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return APE_LZ4_GPU_EINVAL;
}

// a negative count, or a null array in a batch that has entries
bool bad_arrays(int n, std::initializer_list<const void *> arrays) {
    bool bad = n < 0;
    if (n > 0)
        for (const void *p : arrays) bad |= !p;
    return bad;
}

int check_arrays(const char *who, int n, std::initializer_list<const void *> arrays) {
    if (!bad_arrays(n, arrays)) return APE_LZ4_GPU_OK;
    return einval("%s: invalid argument (a null array or a negative count, nblocks %d)", who, n);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int g_ndev = -1;
std::vector<int> g_dev_ok;  // per device: 1 = gfx950
std::once_flag g_once;

void probe() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    g_ndev = n;
    g_dev_ok.assign(n > 0 ? n : 0, 0);
    for (int d = 0; d < n; d++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0)
            g_dev_ok[d] = 1;
    }
}

int check_device() {
    std::call_once(g_once, probe);
    if (g_ndev <= 0) {
        snprintf(g_err, sizeof g_err, "no HIP device visible (libape_lz4_amd needs an MI355X)");
        return APE_LZ4_GPU_ENODEV;
    }
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= g_ndev || !g_dev_ok[d]) {
        snprintf(g_err, sizeof g_err, "current HIP device %d is not gfx950 (MI355X)", d);
        return APE_LZ4_GPU_ENODEV;
    }
    return APE_LZ4_GPU_OK;
}

int finish_launch(hipError_t e, const char *what) {
    if (e != hipSuccess) {
        set_err(what, e);
        return APE_LZ4_GPU_ELAUNCH;
    }
    return APE_LZ4_GPU_OK;
}

// The events of a timed call: all created or the call fails, all destroyed on every way out.
struct Events {
    std::vector<hipEvent_t> ev;
    explicit Events(int n) : ev((size_t)n, nullptr) {}
    Events(const Events &) = delete;
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        hipError_t e = hipSuccess;
        for (size_t q = 0; q < ev.size() && e == hipSuccess; q++) e = hipEventCreate(&ev[q]);
        return finish_launch(e, "hipEventCreate");
    }
};

// ---- pinned staging for the host-buffer path: a process-wide pool ----
// A call borrows one context (stream + pinned + device staging) for its duration and
// returns it, so concurrent callers never share staging, and a thread that exits holds
// nothing (no thread-local HIP resources to leak).  Contexts whose staging grew past
// kKeepBytes are freed on return instead of pooled.
struct HostCtx {
    int dev = -1;
    hipStream_t stream = nullptr;
    char *h = nullptr;  // pinned
    size_t hcap = 0;
    char *d = nullptr;  // device
    size_t dcap = 0;
    void release() {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        if (stream) (void)hipStreamDestroy(stream);
        *this = HostCtx();
    }
};
constexpr size_t kKeepBytes = 64u << 20;
std::mutex g_pool_mu;
std::vector<HostCtx *> g_pool;   // idle contexts (any device)

HostCtx *ctx_acquire() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); i++) {
            if (g_pool[i]->dev == dev) {
                HostCtx *c = g_pool[i];
                g_pool.erase(g_pool.begin() + (long)i);
                return c;
            }
        }
    }
    HostCtx *c = new HostCtx();
    c->dev = dev;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err("hipStreamCreate", e);
        delete c;
        return nullptr;
    }
    return c;
}

void ctx_return(HostCtx *c) {
    if (!c) return;
    if (c->hcap > kKeepBytes || c->dcap > kKeepBytes) {
        c->release();
        delete c;
        return;
    }
    std::lock_guard<std::mutex> g(g_pool_mu);
    g_pool.push_back(c);
}

int host_reserve(HostCtx &c, size_t bytes) {
    if (c.hcap < bytes) {
        if (c.h) (void)hipHostFree(c.h);
        c.h = nullptr;
        size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;
        hipError_t e = hipHostMalloc((void **)&c.h, cap, hipHostMallocDefault);
        if (e != hipSuccess) { c.hcap = 0; set_err("hipHostMalloc", e); return APE_LZ4_GPU_ENOMEM; }
        c.hcap = cap;
    }
    if (c.dcap < bytes) {
        if (c.d) (void)hipFree(c.d);
        c.d = nullptr;
        size_t cap = bytes < (1u << 20) ? (1u << 20) : bytes;
        hipError_t e = hipMalloc((void **)&c.d, cap);
        if (e != hipSuccess) { c.dcap = 0; set_err("hipMalloc", e); return APE_LZ4_GPU_ENOMEM; }
        c.dcap = cap;
    }
    return APE_LZ4_GPU_OK;
}

// Staging layout (same offsets on host and device):
//   [ptr arrays: src, dst][int arrays: in_size, cap, target, result][inputs][outputs]
// mode: 0 = compress, 1 = decompress_safe, 2 = decompress_safe_partial
int host_batch_run(HostCtx &ctx, int mode, int accel, const char *const *h_src, const int *h_in,
                   char *const *h_dst, const int *h_cap, const int *h_target, int *h_res, int nb,
                   const std::vector<size_t> &in_off, const std::vector<size_t> &out_off,
                   const std::vector<size_t> &out_len, size_t total) {
    char *H = ctx.h, *D = ctx.d;
    const char **hp_src = (const char **)H;
    char **hp_dst = (char **)(H + (size_t)nb * sizeof(void *));
    int *hi = (int *)(H + up16((size_t)nb * 2 * sizeof(void *)));
    int *h_size = hi, *h_capd = hi + nb, *h_tgt = hi + 2 * nb;
    const size_t ioff = up16((size_t)nb * 2 * sizeof(void *));
    for (int i = 0; i < nb; i++) {
        hp_src[i] = D + in_off[i];
        hp_dst[i] = D + out_off[i];
        h_size[i] = h_in[i];
        h_capd[i] = h_cap[i];
        h_tgt[i] = h_target ? h_target[i] : 0;
        if (h_in[i] > 0) memcpy(H + in_off[i], h_src[i], (size_t)h_in[i]);
        else H[in_off[i]] = h_src[i] ? h_src[i][0] : 0;
    }
    hipStream_t s = ctx.stream;
    hipError_t e = hipMemcpyAsync(D, H, out_off[0], hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return finish_launch(e, "hipMemcpyAsync H2D");
    BlockArgs a{};
    a.accel = accel;
    a.src = (const char *const *)D;
    a.dst = (char *const *)(D + (size_t)nb * sizeof(void *));
    a.src_size = (const int *)(D + ioff);
    a.dst_cap = (const int *)(D + ioff) + nb;
    a.target = (const int *)(D + ioff) + 2 * nb;
    a.result = (int *)(D + ioff) + 3 * nb;
    a.nblocks = nb;
    e = (mode == 0) ? launch_encode(a, s) : launch_decode(a, mode == 2, s);
    if (e != hipSuccess) return finish_launch(e, "kernel launch");
    e = hipMemcpyAsync(H + ioff + 3 * nb * sizeof(int), (const char *)a.result, nb * sizeof(int),
                       hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(H + out_off[0], D + out_off[0], total - out_off[0],
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return finish_launch(e, "D2H / synchronize");
    const int *hres = (const int *)(H + ioff) + 3 * nb;
    for (int i = 0; i < nb; i++) {
        h_res[i] = hres[i];
        if (hres[i] > 0 && (size_t)hres[i] <= out_len[i]) memcpy(h_dst[i], H + out_off[i], hres[i]);
    }
    return APE_LZ4_GPU_OK;
}

int host_batch(const char *who, int mode, int accel, const char *const *h_src, const int *h_in,
               char *const *h_dst, const int *h_cap, const int *h_target, int *h_res, int nb) {
    if (int rc = check_arrays(who, nb, {h_src, h_in, h_dst, h_cap, h_res})) return rc;
    int rc = check_device();
    if (rc) return rc;
    if (nb == 0) return APE_LZ4_GPU_OK;
    std::vector<size_t> in_off(nb), out_off(nb), out_len(nb);
    size_t meta = up16((size_t)nb * 2 * sizeof(void *)) + up16((size_t)nb * 4 * sizeof(int));
    size_t pos = meta;
    for (int i = 0; i < nb; i++) {
        in_off[i] = pos;
        size_t len = h_in[i] > 0 ? (size_t)h_in[i] : 1;  // size <= 0 still reads src[0]
        pos += up16(len);
    }
    for (int i = 0; i < nb; i++) {
        out_off[i] = pos;
        size_t lim;
        if (mode == 0) {
            int n = h_in[i] > 0 ? h_in[i] : 0;
            size_t bound = (size_t)n + n / 255 + 16;
            lim = h_cap[i] <= 0 ? 0 : ((size_t)h_cap[i] < bound ? (size_t)h_cap[i] : bound);
        } else {
            // the decoder writes only decoded bytes, and LZ4 expands at most 255x (a
            // 255 length byte per 255 output bytes): a huge cap needs no huge staging
            const size_t cs = h_in[i] > 0 ? (size_t)h_in[i] : 0;
            const size_t most = 255 * cs + 64;
            lim = h_cap[i] <= 0 ? 0 : ((size_t)h_cap[i] < most ? (size_t)h_cap[i] : most);
        }
        out_len[i] = lim;
        pos += up16(lim ? lim : 1);
    }
    const size_t total = pos;
    HostCtx *ctx = ctx_acquire();
    if (!ctx) return APE_LZ4_GPU_ENOMEM;
    rc = host_reserve(*ctx, total);
    if (rc) { ctx_return(ctx); return rc; }
    rc = host_batch_run(*ctx, mode, accel, h_src, h_in, h_dst, h_cap, h_target, h_res, nb,
                        in_off, out_off, out_len, total);
    // a failed run may have left copies or the kernel queued on the context's stream:
    // drain them before another caller can borrow its pinned buffer
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    ctx_return(ctx);
    return rc;
}

// ---- the kernels' argument structs from the caller's arguments, and the checks on them ----
// the pointer-array form: block i at src[i], written to dst[i]
BlockArgs ptr_args(const char *const *src, const int *in, char *const *dst, const int *cap,
                   const int *tgt, int *res, int nb) {
    BlockArgs a{};
    a.src = src;
    a.dst = dst;
    a.src_size = in;
    a.dst_cap = cap;
    a.target = tgt;
    a.result = res;
    a.nblocks = nb;
    return a;
}

// arguments, then device; `more`: the arrays an entry point takes beyond the standard five
int ready_ptr(const char *who, const BlockArgs &a, std::initializer_list<const void *> more = {}) {
    if (int rc = check_arrays(who, a.nblocks, {a.src, a.src_size, a.dst, a.dst_cap, a.result}))
        return rc;
    if (int rc = check_arrays(who, a.nblocks, more)) return rc;
    return check_device();
}

// the strided form: block i at src + i * src_stride, written to dst + i * dst_stride
BlockArgs strided_args(const char *src, size_t src_stride, const int *in, char *dst,
                       size_t dst_stride, const int *cap, int *res, int nb) {
    BlockArgs a{};
    a.src_base = src;
    a.dst_base = dst;
    a.src_stride = src_stride;
    a.dst_stride = dst_stride;
    a.src_size = in;
    a.dst_cap = cap;
    a.result = res;
    a.nblocks = nb;
    return a;
}

// arguments, then device; the blocks' places come from their sizes or, in a framed stream, from
// the offsets, and without capacities the capacity is the stride, which then has to fit an int
int ready_strided(const char *who, const BlockArgs &a) {
    const void *places = a.frame_off ? (const void *)a.frame_off : a.src_size;
    if (int rc = check_arrays(who, a.nblocks, {a.src_base, places, a.dst_base, a.result}))
        return rc;
    if (!a.dst_cap && a.dst_stride > 0x7FFFFFFF)
        return einval("%s: dst stride %zu needs explicit capacities", who, a.dst_stride);
    return check_device();
}

// both kinds of prepared dictionary: an object of `size` bytes for messages up to maxSrcSize
int ready_prepare(const char *who, const char *d_dict, int dictSize, int maxSrcSize,
                  const void *d_cdict, size_t cdict_bytes, uint32_t size) {
    if (dictSize < 0 || (dictSize > 0 && !d_dict) || maxSrcSize < 1 || maxSrcSize > kMaxBlock ||
        !d_cdict || cdict_bytes < (size_t)size || !aligned16(d_cdict))
        return einval("%s: dictSize %d, maxSrcSize %d (1..%d), object of %zu bytes at %p (need "
                      "%u bytes, 16-byte aligned)", who, dictSize, maxSrcSize, kMaxBlock,
                      cdict_bytes, d_cdict, size);
    return check_device();
}

// ndicts objects of `size` bytes each, object k at d_cdicts + k * stride; the dictionaries' sizes
// are device memory, so a bad entry is the kernel's to mark (a zero header)
int ready_prepare_batch(const char *who, const char *const *d_dict, const int *d_dictSize,
                        int maxSrcSize, const void *d_cdicts, size_t stride, int ndicts,
                        uint32_t size) {
    if (bad_arrays(ndicts, {d_dict, d_dictSize, d_cdicts}) || maxSrcSize < 1 ||
        maxSrcSize > kMaxBlock || !aligned16(d_cdicts) || stride < (size_t)size || stride % 16)
        return einval("%s: ndicts %d, maxSrcSize %d (1..%d), objects at %p with stride %zu (need "
                      "16-byte alignment and a stride that is a multiple of 16, at least %u), or "
                      "a null array", who, ndicts, maxSrcSize, kMaxBlock, d_cdicts, stride, size);
    return check_device();
}

// blocks per pass: as many as the scratch holds of `slot` bytes each, at most `most` and no
// more than the batch has
int pass_blocks(size_t scratch_bytes, size_t slot, int most, int nblocks) {
    const size_t fit = scratch_bytes / slot;
    const int sub = fit < (size_t)most ? (int)fit : most;
    return sub > nblocks ? nblocks : sub;
}

// ---- compress_destSize (lz4_destsize.hip) ----
constexpr int kDsSub = 16384;   // blocks per scratch pass
inline size_t ds_stride() { return up16((size_t)kMaxBlock + kMaxBlock / 255 + 16); }
inline size_t ds_scratch(int sub) { return (size_t)sub * ds_stride() + (size_t)sub * sizeof(int); }

// encode into the scratch (full-size output, every block fits), then cut each block to
// its target; `sub` blocks per pass (the scratch holds ds_scratch(sub) bytes)
hipError_t destsize_passes(const char *const *d_src, int *d_srcSize, char *const *d_dst,
                           const int *d_targetDstSize, int *d_result, int nblocks, char *scr,
                           int sub, hipStream_t s) {
    const size_t stride = ds_stride();
    int *sres = (int *)(scr + (size_t)sub * stride);
    hipError_t e = hipSuccess;
    for (int off = 0; off < nblocks && e == hipSuccess; off += sub) {
        const int m = nblocks - off < sub ? nblocks - off : sub;
        BlockArgs a{};
        a.src = d_src + off;
        a.dst_base = scr;
        a.dst_stride = stride;  // cap = stride >= compressBound: every block fits
        a.src_size = d_srcSize + off;
        a.result = sres;
        a.nblocks = m;
        e = launch_encode(a, s);
        if (e == hipSuccess)
            e = launch_destsize(d_src + off, d_srcSize + off, d_dst + off, d_targetDstSize + off,
                                d_result + off, scr, stride, sres, m, s);
    }
    return e;
}

// ---- the high-ratio mode (lz4_encode_hc.hip, lz4_hc_cdict.hip) ----
constexpr int kHcSub = 1024;   // blocks per scratch pass: 262144 search workgroups

// d_prefixSize (nullable): per-block bytes of history before d_src[i]; opt: the cost-minimising
// parse, whose cost tables follow the match tables in the scratch.  The scratch has to hold one
// block whatever nblocks is.
int hc_batch(const char *who, bool opt, const char *const *d_src, const int *d_srcSize,
             const int *d_prefixSize, char *const *d_dst, const int *d_dstCap, int *d_result,
             int nblocks, int depth, void *d_scratch, size_t scratch_bytes, void *stream) {
    const size_t slot = opt ? kHcOptSlotBytes : kHcSlotBytes;
    if (depth < 0 || depth > kHcMaxDepth || !d_scratch || !aligned16(d_scratch) ||
        scratch_bytes < slot || bad_arrays(nblocks, {d_src, d_srcSize, d_dst, d_dstCap, d_result}))
        return einval("%s: nblocks %d, depth %d (0..%d), scratch of %zu bytes at %p (need %zu "
                      "bytes, 16-byte aligned)", who, nblocks, depth, kHcMaxDepth, scratch_bytes,
                      d_scratch, slot);
    if (int rc = check_device()) return rc;
    const int sub = pass_blocks(scratch_bytes, slot, kHcSub, nblocks);
    hipError_t e = hipSuccess;
    for (int off = 0; off < nblocks && e == hipSuccess; off += sub) {
        HcOptArgs o{};
        HcArgs &a = o.a;
        a.src = d_src + off;
        a.src_size = d_srcSize + off;
        a.dst = d_dst + off;
        a.dst_cap = d_dstCap + off;
        a.result = d_result + off;
        a.prefix = d_prefixSize ? d_prefixSize + off : nullptr;
        a.nblocks = nblocks - off < sub ? nblocks - off : sub;
        a.depth = depth ? depth : kHcDefaultDepth;
        a.chain = (uint16_t *)d_scratch;
        a.match = (uint32_t *)((char *)d_scratch + (size_t)sub * kHcChainBytes);
        o.cost = (uint32_t *)((char *)d_scratch + (size_t)sub * kHcSlotBytes);
        e = opt ? launch_encode_hc_opt(o, (hipStream_t)stream)
                : launch_encode_hc(a, (hipStream_t)stream);
    }
    return finish_launch(e, opt ? "lz4_hc_chain_kernel + lz4_hc_search_kernel + "
                                  "lz4_hc_opt_parse_kernel"
                                : "lz4_hc_chain_kernel + lz4_hc_search_kernel + "
                                  "lz4_hc_parse_kernel");
}

// messages per scratch pass against a prepared dictionary: as many as make kHcSub x 256 search
// workgroups
inline int hc_cdict_sub(int maxSrcSize) {
    return kHcSub * (kMaxBlock / kHcdThreads) / hc_cdict_groups(maxSrcSize);
}

size_t hc_cdict_scratch(int nblocks, int maxSrcSize, bool opt) {
    if (nblocks <= 0 || maxSrcSize < 1 || maxSrcSize > kMaxBlock) return 0;
    const int sub = hc_cdict_sub(maxSrcSize);
    return (size_t)(nblocks < sub ? nblocks : sub) *
           (opt ? hc_cdict_opt_slot_bytes(maxSrcSize) : hc_cdict_slot_bytes(maxSrcSize));
}

// opt, and the scratch at nblocks == 0: as hc_batch.  The object is d_cdict for every message
// or, with d_cdicts (the usingCDicts calls: d_cdict is then null), d_cdicts[i] for message i,
// which only the kernels can check.
int hc_cdict_batch(const char *who, bool opt, const char *const *d_src, const int *d_srcSize,
                   char *const *d_dst, const int *d_dstCap, int *d_result, int nblocks,
                   const void *d_cdict, int maxSrcSize, int depth, void *d_scratch,
                   size_t scratch_bytes, void *stream, const void *const *d_cdicts = nullptr,
                   bool per = false) {
    const bool range = maxSrcSize >= 1 && maxSrcSize <= kMaxBlock;
    const size_t slot = !range ? 0 : opt ? hc_cdict_opt_slot_bytes(maxSrcSize)
                                         : hc_cdict_slot_bytes(maxSrcSize);
    const bool object = per ? !bad_arrays(nblocks, {d_cdicts}) : d_cdict && aligned16(d_cdict);
    if (!range || depth < 0 || depth > kHcMaxDepth || !object ||
        !d_scratch || !aligned16(d_scratch) || scratch_bytes < slot ||
        bad_arrays(nblocks, {d_src, d_srcSize, d_dst, d_dstCap, d_result}))
        return einval("%s: nblocks %d, maxSrcSize %d (1..%d), depth %d (0..%d), object%s at %p, "
                      "scratch of %zu bytes at %p (need %zu bytes; both 16-byte aligned)", who,
                      nblocks, maxSrcSize, kMaxBlock, depth, kHcMaxDepth, per ? " array" : "",
                      per ? (const void *)d_cdicts : d_cdict, scratch_bytes, d_scratch, slot);
    if (int rc = check_device()) return rc;
    const int sub = pass_blocks(scratch_bytes, slot, hc_cdict_sub(maxSrcSize), nblocks);
    hipError_t e = hipSuccess;
    for (int off = 0; off < nblocks && e == hipSuccess; off += sub) {
        HcDictOptArgs o{};
        HcDictArgs &a = o.a;
        a.src = d_src + off;
        a.src_size = d_srcSize + off;
        a.dst = d_dst + off;
        a.dst_cap = d_dstCap + off;
        a.result = d_result + off;
        a.nblocks = nblocks - off < sub ? nblocks - off : sub;
        a.depth = depth ? depth : kHcDefaultDepth;
        a.max_src = maxSrcSize;
        a.cdict = (const uint8_t *)d_cdict;
        a.chain_stride = (uint32_t)hc_cdict_chain_entries(maxSrcSize);
        a.match_stride = (uint32_t)hc_cdict_match_entries(maxSrcSize);
        a.chain = (uint16_t *)d_scratch;
        a.match = (uint32_t *)((char *)d_scratch + (size_t)sub * a.chain_stride * sizeof(uint16_t));
        o.cost_stride = (uint32_t)hc_cdict_cost_entries(maxSrcSize);
        o.cost = (uint32_t *)((char *)d_scratch + (size_t)sub * hc_cdict_slot_bytes(maxSrcSize));
        const uint8_t *const *objs = per ? (const uint8_t *const *)d_cdicts + off : nullptr;
        e = opt ? launch_encode_hc_cdict_opt(o, (hipStream_t)stream, objs)
                : launch_encode_hc_cdict(a, (hipStream_t)stream, objs);
    }
    if (per)
        return finish_launch(e, opt ? "lz4_hc_cdicts_chain_kernel + lz4_hc_cdicts_search_kernel + "
                                      "lz4_hc_cdicts_opt_parse_kernel"
                                    : "lz4_hc_cdicts_chain_kernel + lz4_hc_cdicts_search_kernel + "
                                      "lz4_hc_cdicts_parse_kernel");
    return finish_launch(e, opt ? "lz4_hc_cdict_chain_kernel + lz4_hc_cdict_search_kernel + "
                                  "lz4_hc_cdict_opt_parse_kernel"
                                : "lz4_hc_cdict_chain_kernel + lz4_hc_cdict_search_kernel + "
                                  "lz4_hc_cdict_parse_kernel");
}

// The framed dictionary call's high-ratio passes (include/ape_lz4f_dict.h): hc_cdict_batch's
// loop on arguments that are already checked -- three launches per pass, as many messages per
// pass as the scratch holds slots.  d_cdicts (nullable): an object per message.
hipError_t hc_cdict_passes(bool opt, const char *const *d_src, const int *d_srcSize,
                           char *const *d_dst, const int *d_dstCap, int *d_result, int nblocks,
                           const void *d_cdict, const void *const *d_cdicts, int maxSrcSize,
                           int depth, void *d_scratch, size_t scratch_bytes, hipStream_t stream) {
    const size_t slot = opt ? hc_cdict_opt_slot_bytes(maxSrcSize) : hc_cdict_slot_bytes(maxSrcSize);
    const int sub = pass_blocks(scratch_bytes, slot, hc_cdict_sub(maxSrcSize), nblocks);
    hipError_t e = hipSuccess;
    for (int off = 0; off < nblocks && e == hipSuccess; off += sub) {
        HcDictOptArgs o{};
        HcDictArgs &a = o.a;
        a.src = d_src + off;
        a.src_size = d_srcSize + off;
        a.dst = d_dst + off;
        a.dst_cap = d_dstCap + off;
        a.result = d_result + off;
        a.nblocks = nblocks - off < sub ? nblocks - off : sub;
        a.depth = depth ? depth : kHcDefaultDepth;
        a.max_src = maxSrcSize;
        a.cdict = (const uint8_t *)d_cdict;
        a.chain_stride = (uint32_t)hc_cdict_chain_entries(maxSrcSize);
        a.match_stride = (uint32_t)hc_cdict_match_entries(maxSrcSize);
        a.chain = (uint16_t *)d_scratch;
        a.match = (uint32_t *)((char *)d_scratch + (size_t)sub * a.chain_stride * sizeof(uint16_t));
        o.cost_stride = (uint32_t)hc_cdict_cost_entries(maxSrcSize);
        o.cost = (uint32_t *)((char *)d_scratch + (size_t)sub * hc_cdict_slot_bytes(maxSrcSize));
        const uint8_t *const *objs = d_cdicts ? (const uint8_t *const *)d_cdicts + off : nullptr;
        e = opt ? launch_encode_hc_cdict_opt(o, stream, objs)
                : launch_encode_hc_cdict(a, stream, objs);
    }
    return e;
}

// ---- inputs of any size as one block (lz4_large.hip) ----
constexpr int kLargeMaxSrc = 0x7E000000;   // LZ4_MAX_INPUT_SIZE (ref src/ape_lz4.h)

bool large_src_ok(int maxSrcSize) { return maxSrcSize >= 1 && maxSrcSize <= kLargeMaxSrc; }
// restartBytes: 0 or a positive multiple of the slice size
bool restart_ok(int restartBytes) {
    return restartBytes >= 0 && restartBytes % large_slice_size() == 0;
}

// the caller's side of LargeArgs; buf is the whole scratch until large_layout cuts it up
LargeArgs large_in(const char *const *d_src, const int *d_srcSize, char *const *d_dst,
                   const int *d_dstCap, int *d_result, int nblocks, int maxSrcSize,
                   void *d_scratch, int restartBytes = 0, void *d_index = nullptr,
                   size_t index_stride = 0) {
    LargeArgs a{};
    a.restart = restartBytes;
    a.index = (char *)d_index;
    a.index_stride = index_stride;
    a.src = d_src;
    a.src_size = d_srcSize;
    a.dst = d_dst;
    a.dst_cap = d_dstCap;
    a.result = d_result;
    a.nblocks = nblocks;
    a.max_src = maxSrcSize;
    a.buf = (char *)d_scratch;
    return a;
}

int check_large_arrays(const char *who, const LargeArgs &a) {
    return check_arrays(who, a.nblocks, {a.src, a.src_size, a.dst, a.dst_cap, a.result, a.buf});
}

// what compress_large and compress_large_hc ask of maxSrcSize, restartBytes and the index
int check_large(const char *who, const LargeArgs &a) {
    if (!large_src_ok(a.max_src))
        return einval("%s: maxSrcSize %d outside [1, %d]", who, a.max_src, kLargeMaxSrc);
    if (!restart_ok(a.restart))
        return einval("%s: restartBytes %d is neither 0 nor a positive multiple of the slice size "
                      "%d", who, a.restart, large_slice_size());
    const size_t least = large_index_size(a.max_src, a.restart);
    if (a.index && (!aligned16(a.index) || a.index_stride % 16u || a.index_stride < least))
        return einval("%s: index at %p with stride %zu, need 16-byte alignment and a stride that "
                      "is a multiple of 16 and >= %zu", who, a.index, a.index_stride, least);
    return APE_LZ4_GPU_OK;
}

// cut the scratch of a batch that has blocks into the slot arrays; it has to hold them and
// `tables` more bytes, which then begin at *base
int large_layout(const char *who, LargeArgs &a, size_t scratch_bytes, size_t tables,
                 size_t *base) {
    const char *scratch = a.buf;
    *base = up16(large_scratch_layout(a.nblocks, a.max_src, &a));
    if (*base == 0)
        return einval("%s: %d inputs of up to %d bytes are more slices than one call takes; "
                      "split the batch", who, a.nblocks, a.max_src);
    if (scratch_bytes < *base + tables || !aligned16(scratch))
        return einval("%s: scratch of %zu bytes at %p, need %zu bytes 16-byte aligned", who,
                      scratch_bytes, scratch, *base + tables);
    return APE_LZ4_GPU_OK;
}

// The scratch is looked at only once there is work to do, so after the device check: an empty
// batch is OK with any scratch.
int large_batch(const char *who, LargeArgs a, int acceleration, size_t scratch_bytes,
                void *stream, hipEvent_t *ev) {
    if (int rc = check_large_arrays(who, a)) return rc;
    if (int rc = check_large(who, a)) return rc;
    if (int rc = check_device()) return rc;
    if (a.nblocks == 0) return APE_LZ4_GPU_OK;
    size_t need = 0;
    if (int rc = large_layout(who, a, scratch_bytes, 0, &need)) return rc;
    return finish_launch(launch_large(a, acceleration, (hipStream_t)stream, ev),
                         "large plan + lz4_encode_kernel + offsets + stitch");
}

// ---- the high-ratio mode on inputs of any size (lz4_large.hip launch_large_hc) ----
// Scratch: the large path's layout, then the chain and match tables of one pass of slices.
// slices per pass out of `want` (0 = all): 1 .. min(slots, kHcSub)
int large_hc_pass(long long nslots, long long want) {
    long long most = nslots < kHcSub ? nslots : kHcSub;
    if (most < 1) most = 1;
    if (want <= 0 || want > most) want = most;
    return (int)want;
}

size_t large_hc_scratch(int nblocks, int maxSrcSize, int passSlices, size_t slot) {
    if (nblocks < 0 || !large_src_ok(maxSrcSize) || passSlices < 0) return 0;
    const size_t base = large_scratch_layout(nblocks, maxSrcSize, nullptr);
    if (!base) return (size_t)-1;   // more slice slots than one call takes: split the batch
    const long long S = large_slice_size();
    const long long nsl = maxSrcSize <= kMaxBlock ? 1 : ((long long)maxSrcSize + S - 1) / S;
    return up16(base) + (size_t)large_hc_pass(nblocks * nsl, passSlices) * slot;
}

// Unlike large_batch, the scratch of a batch that has blocks is checked before the device.
// ms6 (nullable): the timed form.
int large_hc_batch(const char *who, bool opt, LargeArgs a, int depth, size_t scratch_bytes,
                   void *stream, float *ms6) {
    const size_t slot = opt ? kHcOptSlotBytes : kHcSlotBytes;
    char *const scratch = a.buf;
    if (int rc = check_large_arrays(who, a)) return rc;
    if (depth < 0 || depth > kHcMaxDepth)
        return einval("%s: depth %d outside 0..%d", who, depth, kHcMaxDepth);
    if (int rc = check_large(who, a)) return rc;
    size_t base = 0;
    if (a.nblocks > 0)
        if (int rc = large_layout(who, a, scratch_bytes, slot, &base)) return rc;
    if (int rc = check_device()) return rc;
    if (a.nblocks == 0) return APE_LZ4_GPU_OK;
    // as many slices per pass as the caller's scratch holds
    const int pass = large_hc_pass(a.nslots, (long long)((scratch_bytes - base) / slot));
    const char *what = "large plan + lz4_hc kernels + offsets + stitch";
    const hipStream_t s = (hipStream_t)stream;
    const int d = depth ? depth : kHcDefaultDepth;
    if (!ms6)
        return finish_launch(launch_large_hc(a, d, scratch + base, pass, s, nullptr, opt), what);
    // the timed form: events around every launch, the passes' times summed per kernel
    const int passes = large_hc_passes(a.nslots, pass);
    Events t(5 + 3 * passes);
    int rc = t.create();
    if (rc == APE_LZ4_GPU_OK)
        rc = finish_launch(launch_large_hc(a, d, scratch + base, pass, s, t.ev.data(), opt), what);
    for (int q = 0; q < 6; q++) ms6[q] = 0.f;
    if (rc == APE_LZ4_GPU_OK) {
        hipError_t e = hipEventSynchronize(t.ev.back());
        auto span = [&](int slot, int from) {
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, t.ev[from], t.ev[from + 1]);
            ms6[slot] += ms;
        };
        span(0, 0);
        for (int p = 0; p < passes; p++)
            for (int k = 0; k < 3; k++) span(1 + k, 1 + 3 * p + k);
        span(4, 1 + 3 * passes);
        span(5, 2 + 3 * passes);   // (the index launch, after it, is not in any figure)
        rc = finish_launch(e, "compress_large_hc stage events");
    }
    return rc;
}

// ---- indexed blocks (lz4_decode.hip) ----
// the stride holds the header and maxSegments + 1 pairs, so a block's index is never read past
bool index_ok(const void *d_index, size_t index_stride, int maxSegments) {
    return maxSegments >= 1 && aligned16(d_index) && index_stride % 16u == 0 &&
           index_stride >= 16u + 8u * ((size_t)maxSegments + 1u);
}

// ---- dictionary training (lz4_dict_train.hip) ----
// what sizes the slot grid and the scratch; the product bound keeps every u32 count from wrapping
bool dt_shape_ok(int nsamples, int maxSampleSize, int segmentSize) {
    return nsamples >= 0 && maxSampleSize >= kDtMinSample && maxSampleSize <= kDtMaxSample &&
           segmentSize >= kDtMinSeg && segmentSize <= kDtMaxSeg && segmentSize % 16 == 0 &&
           (long long)nsamples * maxSampleSize <= 0x7FFFFFFFll;
}

// ---- the framed decodes (lz4_lz4f.hip): the call of include/ape_lz4f.h and, with `placed`,
// the one of include/ape_lz4f_placed.h ----
size_t lz4f_decode_scratch(int nframes, int maxBlocks, bool placed) {
    if (nframes < 0 || maxBlocks < 1) return 0;
    return lz4f_decode_layout(nframes, maxBlocks, placed, nullptr);
}

// The table of the dictionary call (include/ape_lz4f_dict.h); a null `table` is the other two.
struct LfTable {
    const unsigned *id;
    const char *const *dict;
    const int *size;
    int n;
};

int lz4f_decode_batch(const char *who, bool placed, const char *const *d_src,
                      const int *d_srcSize, char *const *d_dst, const int *d_dstCap,
                      int *d_result, int nframes, int maxBlocks, int flags, void *d_scratch,
                      size_t scratch_bytes, void *stream, const LfTable *table = nullptr) {
    if (int rc = check_arrays(who, nframes, {d_src, d_srcSize, d_dst, d_dstCap, d_result}))
        return rc;
    if (table && bad_arrays(table->n, {table->id, table->dict, table->size}))
        return einval("%s: ntable %d with a null table array, or negative", who, table->n);
    const size_t need = lz4f_decode_scratch(nframes, maxBlocks, placed);
    if (maxBlocks < 1 || (flags & ~3) || need == (size_t)-1 ||
        (nframes > 0 && (!d_scratch || scratch_bytes < need || !aligned16(d_scratch))))
        return einval("%s: nframes %d, maxBlocks %d (from 1), flags %d (0..3), scratch of %zu "
                      "bytes at %p (need %zu bytes 16-byte aligned, fewer than 2^24 blocks)", who,
                      nframes, maxBlocks, flags, scratch_bytes, d_scratch, need);
    if (int rc = check_device()) return rc;
    LfDecode d{};
    d.src = d_src;
    d.src_size = d_srcSize;
    d.dst = d_dst;
    d.dst_cap = d_dstCap;
    d.result = d_result;
    d.nframes = nframes;
    d.max_blocks = maxBlocks;
    d.verify = !(flags & 1);
    d.no_linked = (flags & 2) != 0;
    d.zero = (const char *)d_scratch;
    lz4f_decode_layout(nframes, maxBlocks, placed, &d);
    if (table) {
        d.dicts = true;
        d.t_id = table->id;
        d.t_dict = table->dict;
        d.t_size = table->size;
        d.ntable = table->n;
    }
    return finish_launch(launch_lz4f_decode(d, (hipStream_t)stream),
                         table ? "lz4f_decompress_usingDicts"
                               : placed ? "lz4f_decompress_placed" : "lz4f_decompress");
}

// ---- framed compress with preferences (include/ape_lz4f_prefs.h, lz4_lz4f.hip) ----
bool lf_prefs_ok(int blockSizeID, int mode) {
    return blockSizeID >= 4 && blockSizeID <= 7 && mode >= 0 && mode <= 2;
}
// the scratch's three parts: the frame layer's, the large call's for the block slots as inputs
// of up to one block, and for the high-ratio modes the tables of `want` slices per pass (0: all).
// 0 out of range, (size_t)-1 from 2^24 block slots or slices on.
size_t lf_prefs_scratch(int nframes, int maxSrcSize, int blockSizeID, int mode, int want,
                        size_t *frame, size_t *large) {
    if (nframes < 0 || maxSrcSize < 0 || maxSrcSize > kLfMaxSrc || !lf_prefs_ok(blockSizeID, mode) ||
        want < 0)
        return 0;
    const int B = (int)lf_block_bytes(blockSizeID);
    const size_t f = lz4f_compress_layout(nframes, maxSrcSize, blockSizeID, nullptr);
    if (f == (size_t)-1) return f;
    const long long bpf = maxSrcSize > 0 ? ((long long)maxSrcSize + B - 1) / B : 1;
    const int nslots = (int)(nframes * bpf);
    const size_t l = large_scratch_layout(nslots, B, nullptr);
    if (!l) return (size_t)-1;
    if (frame) *frame = f;
    if (large) *large = up16(l);
    if (mode == 0) return f + up16(l);
    const long long S = large_slice_size(), nsl = B <= kMaxBlock ? 1 : (B + S - 1) / S;
    return f + up16(l) + (size_t)large_hc_pass(nslots * nsl, want) *
                             (mode == 2 ? kHcOptSlotBytes : kHcSlotBytes);
}

}  // namespace

extern "C" {

int APE_LZ4_gpu_init(void) { return check_device(); }

int APE_LZ4_gpu_device_count(void) {
    std::call_once(g_once, probe);
    return g_ndev < 0 ? 0 : g_ndev;
}

const char *APE_LZ4_gpu_last_error(void) { return g_err; }
const char *APE_LZ4_gpu_arch(void) { return "gfx950"; }

int APE_LZ4_compress_batch_dev(const char *const *d_src, const int *d_srcSize,
                               char *const *d_dst, const int *d_dstCap, int *d_result,
                               int nblocks, void *stream) {
    BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    if (int rc = ready_ptr("compress_batch_dev", a)) return rc;
    return finish_launch(launch_encode(a, (hipStream_t)stream), "lz4_encode_kernel");
}

int APE_LZ4_compress_fast_batch_dev(const char *const *d_src, const int *d_srcSize,
                                    char *const *d_dst, const int *d_dstCap, int *d_result,
                                    int nblocks, int acceleration, void *stream) {
    BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    a.accel = acceleration;
    if (int rc = ready_ptr("compress_fast_batch_dev", a)) return rc;
    return finish_launch(launch_encode(a, (hipStream_t)stream), "lz4_encode_kernel");
}

int APE_LZ4_compress_exact_batch_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int acceleration, void *stream) {
    BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    a.accel = acceleration;
    if (int rc = ready_ptr("compress_exact_batch_dev", a)) return rc;
    return finish_launch(launch_encode_exact(a, (hipStream_t)stream), "lz4_encode_exact_kernel");
}

int APE_LZ4_decompress_safe_batch_dev(const char *const *d_src, const int *d_compressedSize,
                                      char *const *d_dst, const int *d_maxDecompressedSize,
                                      int *d_result, int nblocks, void *stream) {
    BlockArgs a = ptr_args(d_src, d_compressedSize, d_dst, d_maxDecompressedSize, nullptr,
                           d_result, nblocks);
    if (int rc = ready_ptr("decompress_safe_batch_dev", a)) return rc;
    return finish_launch(launch_decode(a, false, (hipStream_t)stream), "lz4_decode_kernel");
}

int APE_LZ4_decompress_safe_partial_batch_dev(const char *const *d_src,
                                              const int *d_compressedSize, char *const *d_dst,
                                              const int *d_targetOutputSize,
                                              const int *d_maxDecompressedSize, int *d_result,
                                              int nblocks, void *stream) {
    BlockArgs a = ptr_args(d_src, d_compressedSize, d_dst, d_maxDecompressedSize,
                           d_targetOutputSize, d_result, nblocks);
    if (int rc = ready_ptr("decompress_safe_partial_batch_dev", a, {d_targetOutputSize}))
        return rc;
    return finish_launch(launch_decode(a, true, (hipStream_t)stream),
                         "lz4_decode_kernel<partial>");
}

int APE_LZ4_decompress_safe_usingDict_batch_dev(const char *const *d_src,
                                                const int *d_compressedSize, char *const *d_dst,
                                                const int *d_maxDecompressedSize,
                                                const char *const *d_dict, const int *d_dictSize,
                                                int *d_result, int nblocks, void *stream) {
    BlockArgs a = ptr_args(d_src, d_compressedSize, d_dst, d_maxDecompressedSize, nullptr,
                           d_result, nblocks);
    a.dict = d_dict;
    a.dict_size = d_dictSize;
    if (int rc = ready_ptr("decompress_safe_usingDict_batch_dev", a, {d_dict, d_dictSize}))
        return rc;
    return finish_launch(launch_decode(a, false, (hipStream_t)stream),
                         "lz4_decode_kernel<usingDict>");
}

int APE_LZ4_decompress_fast_batch_dev(const char *const *d_src, const int *d_srcBound,
                                      char *const *d_dst, const int *d_originalSize,
                                      int *d_result, int nblocks, void *stream) {
    BlockArgs a = ptr_args(d_src, d_srcBound, d_dst, d_originalSize, nullptr, d_result, nblocks);
    a.fast = 1;
    if (int rc = ready_ptr("decompress_fast_batch_dev", a)) return rc;
    return finish_launch(launch_decode(a, false, (hipStream_t)stream), "lz4_decode_kernel<fast>");
}

int APE_LZ4_compress_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          const int *d_prefixSize, char *const *d_dst,
                                          const int *d_dstCap, int *d_result, int nblocks,
                                          void *stream) {
    BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    a.dict_size = d_prefixSize;
    if (int rc = ready_ptr("compress_withPrefix_batch_dev", a, {d_prefixSize})) return rc;
    return finish_launch(launch_encode(a, (hipStream_t)stream), "lz4_encode_kernel<prefix>");
}

// ---- prepared dictionaries (lz4_cdict.hip, the encoder's EXT instantiation) ----
size_t APE_LZ4_cdict_size(void) { return (size_t)kCdSize; }

int APE_LZ4_cdict_window(int dictSize, int maxSrcSize) {
    if (dictSize < 0 || maxSrcSize < 1 || maxSrcSize > kMaxBlock) return -1;
    const int D = cdict_window(dictSize, maxSrcSize);
    return D < 64 ? 0 : D;
}

int APE_LZ4_cdict_prepare_dev(const char *d_dict, int dictSize, int maxSrcSize, void *d_cdict,
                              size_t cdict_bytes, void *stream) {
    if (int rc = ready_prepare("cdict_prepare_dev", d_dict, dictSize, maxSrcSize, d_cdict,
                               cdict_bytes, kCdSize))
        return rc;
    return finish_launch(launch_cdict_prepare(d_dict, dictSize, maxSrcSize, d_cdict,
                                              (hipStream_t)stream),
                         "lz4_cdict_prepare_kernel");
}

// (the object is needed for an empty batch too)
int APE_LZ4_compress_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          char *const *d_dst, const int *d_dstCap, int *d_result,
                                          int nblocks, const void *d_cdict, void *stream) {
    if (!d_cdict || !aligned16(d_cdict))
        return einval("compress_usingCDict_batch_dev: object at %p, need one 16-byte aligned",
                      d_cdict);
    BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    if (int rc = ready_ptr("compress_usingCDict_batch_dev", a)) return rc;
    return finish_launch(launch_encode_cdict(a, d_cdict, (hipStream_t)stream),
                         "lz4_encode_cdict_kernel");
}

// ---- compress_destSize (lz4_destsize.hip) ----
size_t APE_LZ4_compress_destSize_scratch_size(int nblocks) {
    const int sub = nblocks < 1 ? 1 : (nblocks < kDsSub ? nblocks : kDsSub);
    return ds_scratch(sub);
}

// (the scratch's size and alignment are looked at only once there is work to do, so after the
// device check: an empty batch is OK with any scratch)
int APE_LZ4_compress_destSize_batch_scratch_dev(const char *const *d_src, int *d_srcSize,
                                                char *const *d_dst, const int *d_targetDstSize,
                                                int *d_result, int nblocks, void *d_scratch,
                                                size_t scratch_bytes, void *stream) {
    const char *who = "compress_destSize_batch_scratch_dev";
    if (int rc = check_arrays(who, nblocks,
                              {d_src, d_srcSize, d_dst, d_targetDstSize, d_result, d_scratch}))
        return rc;
    if (int rc = check_device()) return rc;
    if (nblocks == 0) return APE_LZ4_GPU_OK;
    if (scratch_bytes < ds_scratch(1))
        return einval("%s: destSize scratch of %zu bytes < %zu (one block)", who, scratch_bytes,
                      ds_scratch(1));
    if (!aligned16(d_scratch))
        return einval("%s: scratch at %p is not 16-byte aligned", who, d_scratch);
    const int sub = pass_blocks(scratch_bytes, ds_scratch(1), nblocks, nblocks);
    return finish_launch(destsize_passes(d_src, d_srcSize, d_dst, d_targetDstSize, d_result,
                                         nblocks, (char *)d_scratch, sub, (hipStream_t)stream),
                         "lz4_encode_kernel + lz4_destsize_kernel");
}

int APE_LZ4_compress_destSize_batch_dev(const char *const *d_src, int *d_srcSize,
                                        char *const *d_dst, const int *d_targetDstSize,
                                        int *d_result, int nblocks, void *stream) {
    if (int rc = check_arrays("compress_destSize_batch_dev", nblocks,
                              {d_src, d_srcSize, d_dst, d_targetDstSize, d_result}))
        return rc;
    if (int rc = check_device()) return rc;
    if (nblocks == 0) return APE_LZ4_GPU_OK;
    // The one launcher that allocates: stream-ordered scratch (hipMallocAsync / hipFreeAsync
    // on the caller's stream, so concurrent calls never share it).  Under graph capture
    // use APE_LZ4_compress_destSize_batch_scratch_dev with caller-owned scratch.
    const int sub = nblocks < kDsSub ? nblocks : kDsSub;
    hipStream_t s = (hipStream_t)stream;
    char *scr = nullptr;
    hipError_t e = hipMallocAsync((void **)&scr, ds_scratch(sub), s);
    if (e != hipSuccess) {
        set_err("hipMallocAsync (destSize scratch)", e);
        return APE_LZ4_GPU_ENOMEM;
    }
    e = destsize_passes(d_src, d_srcSize, d_dst, d_targetDstSize, d_result, nblocks, scr, sub, s);
    hipError_t ef = hipFreeAsync(scr, s);
    if (e == hipSuccess) e = ef;
    return finish_launch(e, "lz4_encode_kernel + lz4_destsize_kernel");
}

// ---- the high-ratio mode (lz4_encode_hc.hip) ----
size_t APE_LZ4_compress_hc_scratch_size(int nblocks) {
    if (nblocks <= 0) return 0;
    return (size_t)(nblocks < kHcSub ? nblocks : kHcSub) * kHcSlotBytes;
}

size_t APE_LZ4_compress_hc_opt_scratch_size(int nblocks) {
    if (nblocks <= 0) return 0;
    return (size_t)(nblocks < kHcSub ? nblocks : kHcSub) * kHcOptSlotBytes;
}

int APE_LZ4_compress_hc_opt_batch_dev(const char *const *d_src, const int *d_srcSize,
                                      char *const *d_dst, const int *d_dstCap, int *d_result,
                                      int nblocks, int depth, void *d_scratch,
                                      size_t scratch_bytes, void *stream) {
    return hc_batch("compress_hc_opt_batch_dev", true, d_src, d_srcSize, nullptr, d_dst, d_dstCap,
                    d_result, nblocks, depth, d_scratch, scratch_bytes, stream);
}

int APE_LZ4_compress_hc_opt_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 const int *d_prefixSize, char *const *d_dst,
                                                 const int *d_dstCap, int *d_result, int nblocks,
                                                 int depth, void *d_scratch, size_t scratch_bytes,
                                                 void *stream) {
    return hc_batch("compress_hc_opt_withPrefix_batch_dev", true, d_src, d_srcSize, d_prefixSize,
                    d_dst, d_dstCap, d_result, nblocks, depth, d_scratch, scratch_bytes, stream);
}

int APE_LZ4_compress_hc_batch_dev(const char *const *d_src, const int *d_srcSize,
                                  char *const *d_dst, const int *d_dstCap, int *d_result,
                                  int nblocks, int depth, void *d_scratch, size_t scratch_bytes,
                                  void *stream) {
    return hc_batch("compress_hc_batch_dev", false, d_src, d_srcSize, nullptr, d_dst, d_dstCap,
                    d_result, nblocks, depth, d_scratch, scratch_bytes, stream);
}

int APE_LZ4_compress_hc_withPrefix_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             const int *d_prefixSize, char *const *d_dst,
                                             const int *d_dstCap, int *d_result, int nblocks,
                                             int depth, void *d_scratch, size_t scratch_bytes,
                                             void *stream) {
    return hc_batch("compress_hc_withPrefix_batch_dev", false, d_src, d_srcSize, d_prefixSize,
                    d_dst, d_dstCap, d_result, nblocks, depth, d_scratch, scratch_bytes, stream);
}

// ---- the high-ratio mode against a prepared dictionary (lz4_hc_cdict.hip) ----
size_t APE_LZ4_hc_cdict_size(void) { return (size_t)kHdSize; }

int APE_LZ4_hc_cdict_window(int dictSize, int maxSrcSize) {
    if (dictSize < 0 || maxSrcSize < 1 || maxSrcSize > kMaxBlock) return -1;
    return hc_cdict_window(dictSize, maxSrcSize);
}

int APE_LZ4_hc_cdict_prepare_dev(const char *d_dict, int dictSize, int maxSrcSize, void *d_cdict,
                                 size_t cdict_bytes, void *stream) {
    if (int rc = ready_prepare("hc_cdict_prepare_dev", d_dict, dictSize, maxSrcSize, d_cdict,
                               cdict_bytes, kHdSize))
        return rc;
    return finish_launch(launch_hc_cdict_prepare(d_dict, dictSize, maxSrcSize, d_cdict,
                                                 (hipStream_t)stream),
                         "lz4_hc_cdict_prepare_kernel");
}

size_t APE_LZ4_compress_hc_usingCDict_scratch_size(int nblocks, int maxSrcSize) {
    return hc_cdict_scratch(nblocks, maxSrcSize, false);
}

size_t APE_LZ4_compress_hc_opt_usingCDict_scratch_size(int nblocks, int maxSrcSize) {
    return hc_cdict_scratch(nblocks, maxSrcSize, true);
}

int APE_LZ4_compress_hc_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nblocks, const void *d_cdict,
                                             int maxSrcSize, int depth, void *d_scratch,
                                             size_t scratch_bytes, void *stream) {
    return hc_cdict_batch("compress_hc_usingCDict_batch_dev", false, d_src, d_srcSize, d_dst,
                          d_dstCap, d_result, nblocks, d_cdict, maxSrcSize, depth, d_scratch,
                          scratch_bytes, stream);
}

int APE_LZ4_compress_hc_opt_usingCDict_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 char *const *d_dst, const int *d_dstCap,
                                                 int *d_result, int nblocks, const void *d_cdict,
                                                 int maxSrcSize, int depth, void *d_scratch,
                                                 size_t scratch_bytes, void *stream) {
    return hc_cdict_batch("compress_hc_opt_usingCDict_batch_dev", true, d_src, d_srcSize, d_dst,
                          d_dstCap, d_result, nblocks, d_cdict, maxSrcSize, depth, d_scratch,
                          scratch_bytes, stream);
}

// ---- dictionary training (lz4_dict_train.hip) ----
// ---- a prepared dictionary per message (ape_lz4_cdicts.h) ----
int APE_LZ4_cdict_prepare_batch_dev(const char *const *d_dict, const int *d_dictSize,
                                    int maxSrcSize, void *d_cdicts, size_t cdict_stride,
                                    int ndicts, void *stream) {
    if (int rc = ready_prepare_batch("cdict_prepare_batch_dev", d_dict, d_dictSize, maxSrcSize,
                                     d_cdicts, cdict_stride, ndicts, kCdSize))
        return rc;
    return finish_launch(launch_cdict_prepare_batch(d_dict, d_dictSize, maxSrcSize, d_cdicts,
                                                    cdict_stride, ndicts, (hipStream_t)stream),
                         "lz4_cdict_prepare_batch_kernel");
}

int APE_LZ4_hc_cdict_prepare_batch_dev(const char *const *d_dict, const int *d_dictSize,
                                       int maxSrcSize, void *d_cdicts, size_t cdict_stride,
                                       int ndicts, void *stream) {
    if (int rc = ready_prepare_batch("hc_cdict_prepare_batch_dev", d_dict, d_dictSize, maxSrcSize,
                                     d_cdicts, cdict_stride, ndicts, kHdSize))
        return rc;
    return finish_launch(launch_hc_cdict_prepare_batch(d_dict, d_dictSize, maxSrcSize, d_cdicts,
                                                       cdict_stride, ndicts, (hipStream_t)stream),
                         "lz4_hc_cdict_prepare_batch_kernel");
}

int APE_LZ4_compress_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                           char *const *d_dst, const int *d_dstCap, int *d_result,
                                           int nblocks, const void *const *d_cdict, void *stream) {
    const BlockArgs a = ptr_args(d_src, d_srcSize, d_dst, d_dstCap, nullptr, d_result, nblocks);
    if (int rc = ready_ptr("compress_usingCDicts_batch_dev", a, {d_cdict})) return rc;
    return finish_launch(launch_encode_cdicts(a, d_cdict, (hipStream_t)stream),
                         "lz4_encode_cdicts_kernel");
}

int APE_LZ4_compress_hc_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                              char *const *d_dst, const int *d_dstCap,
                                              int *d_result, int nblocks,
                                              const void *const *d_cdict, int maxSrcSize, int depth,
                                              void *d_scratch, size_t scratch_bytes, void *stream) {
    return hc_cdict_batch("compress_hc_usingCDicts_batch_dev", false, d_src, d_srcSize, d_dst,
                          d_dstCap, d_result, nblocks, nullptr, maxSrcSize, depth, d_scratch,
                          scratch_bytes, stream, d_cdict, true);
}

int APE_LZ4_compress_hc_opt_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                  char *const *d_dst, const int *d_dstCap,
                                                  int *d_result, int nblocks,
                                                  const void *const *d_cdict, int maxSrcSize,
                                                  int depth, void *d_scratch, size_t scratch_bytes,
                                                  void *stream) {
    return hc_cdict_batch("compress_hc_opt_usingCDicts_batch_dev", true, d_src, d_srcSize, d_dst,
                          d_dstCap, d_result, nblocks, nullptr, maxSrcSize, depth, d_scratch,
                          scratch_bytes, stream, d_cdict, true);
}

size_t APE_LZ4_dict_train_scratch_size(int nsamples, int maxSampleSize, int segmentSize) {
    if (!dt_shape_ok(nsamples, maxSampleSize, segmentSize)) return 0;
    return dt_scratch_bytes(nsamples, maxSampleSize, segmentSize);
}

int APE_LZ4_dict_train_dev(const char *const *d_samples, const int *d_sampleSize, int nsamples,
                           int maxSampleSize, char *d_dict, int dictCapacity, int segmentSize,
                           void *d_scratch, size_t scratch_bytes, int *d_info, void *stream) {
    const char *who = "dict_train_dev";
    if (int rc = check_arrays(who, nsamples, {d_samples, d_sampleSize})) return rc;
    if (!dt_shape_ok(nsamples, maxSampleSize, segmentSize))
        return einval("%s: nsamples %d x maxSampleSize %d (%d..%d, product below 2^31), "
                      "segmentSize %d (a multiple of 16 in %d..%d)", who, nsamples, maxSampleSize,
                      kDtMinSample, kDtMaxSample, segmentSize, kDtMinSeg, kDtMaxSeg);
    const size_t need = dt_scratch_bytes(nsamples, maxSampleSize, segmentSize);
    if (!d_dict || !d_info || dictCapacity < segmentSize || dictCapacity > kDtMaxDict ||
        !d_scratch || !aligned16(d_scratch) || scratch_bytes < need)
        return einval("%s: dictionary at %p, dictCapacity %d (%d..%d), info at %p, scratch of %zu "
                      "bytes at %p (need %zu bytes, 16-byte aligned)", who, (void *)d_dict,
                      dictCapacity, segmentSize, kDtMaxDict, (void *)d_info, scratch_bytes,
                      d_scratch, need);
    if (int rc = check_device()) return rc;
    DtArgs a{};
    a.samples = d_samples;
    a.size = d_sampleSize;
    a.nsamples = nsamples;
    a.max_sample = maxSampleSize;
    a.dict = d_dict;
    a.capacity = dictCapacity;
    a.segment = segmentSize;
    a.freq = (uint32_t *)d_scratch;
    a.state = (DtState *)((char *)d_scratch + kDtStateAt);
    a.partial = (DtPartial *)((char *)d_scratch + kDtPartialAt);
    a.info = d_info;
    return finish_launch(launch_dict_train(a, (hipStream_t)stream),
                         "lz4_dict_train zero + count + score + pick + finish kernels");
}

// ---- inputs of any size as one block (lz4_large.hip) ----
int APE_LZ4_compress_large_slice_size(void) { return large_slice_size(); }

size_t APE_LZ4_compress_large_scratch_size(int nblocks, int maxSrcSize) {
    if (nblocks < 0 || !large_src_ok(maxSrcSize)) return 0;
    const size_t need = large_scratch_layout(nblocks, maxSrcSize, nullptr);
    return need ? need : (size_t)-1;   // more slice slots than one call takes: split the batch
}

int APE_LZ4_large_index_segments(int maxSrcSize, int restartBytes) {
    if (!large_src_ok(maxSrcSize) || !restart_ok(restartBytes)) return 0;
    return (int)large_index_segments(maxSrcSize, restartBytes);
}

size_t APE_LZ4_large_index_size(int maxSrcSize, int restartBytes) {
    if (!large_src_ok(maxSrcSize) || !restart_ok(restartBytes)) return 0;
    return large_index_size(maxSrcSize, restartBytes);
}

int APE_LZ4_compress_large_batch_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int maxSrcSize, int acceleration,
                                     void *d_scratch, size_t scratch_bytes, void *stream) {
    return large_batch("compress_large_batch_dev",
                       large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks, maxSrcSize,
                                d_scratch),
                       acceleration, scratch_bytes, stream, nullptr);
}

int APE_LZ4_compress_large_indexed_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nblocks, int maxSrcSize,
                                             int acceleration, void *d_scratch,
                                             size_t scratch_bytes, int restartBytes, void *d_index,
                                             size_t index_stride, void *stream) {
    return large_batch("compress_large_indexed_batch_dev",
                       large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks, maxSrcSize,
                                d_scratch, restartBytes, d_index, index_stride),
                       acceleration, scratch_bytes, stream, nullptr);
}

// (the events are made before the arguments are looked at, so without a device the call fails
// there)
int APE_LZ4_compress_large_timed_dev(const char *const *d_src, const int *d_srcSize,
                                     char *const *d_dst, const int *d_dstCap, int *d_result,
                                     int nblocks, int maxSrcSize, int acceleration,
                                     void *d_scratch, size_t scratch_bytes, void *stream,
                                     float *ms4) {
    if (!ms4) return einval("compress_large_timed_dev: ms4 is null");
    Events t(5);
    int rc = t.create();
    if (rc == APE_LZ4_GPU_OK)
        rc = large_batch("compress_large_timed_dev",
                         large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks, maxSrcSize,
                                  d_scratch),
                         acceleration, scratch_bytes, stream, t.ev.data());
    for (int q = 0; q < 4; q++) ms4[q] = 0.f;
    if (rc == APE_LZ4_GPU_OK && nblocks > 0) {
        hipError_t e = hipEventSynchronize(t.ev[4]);
        for (int q = 0; q < 4 && e == hipSuccess; q++)
            e = hipEventElapsedTime(&ms4[q], t.ev[q], t.ev[q + 1]);
        rc = finish_launch(e, "compress_large stage events");
    }
    return rc;
}

int APE_LZ4_decompress_safe_indexed_batch_dev(const char *const *d_src,
                                              const int *d_compressedSize, char *const *d_dst,
                                              const int *d_maxDecompressedSize,
                                              const void *d_index, size_t index_stride,
                                              int maxSegments, int *d_result, int nblocks,
                                              void *stream) {
    const char *who = "decompress_safe_indexed_batch_dev";
    if (int rc = check_arrays(who, nblocks, {d_src, d_compressedSize, d_dst,
                                             d_maxDecompressedSize, d_index, d_result}))
        return rc;
    // one wave per (block, segment) in a one-dimensional grid
    if (!index_ok(d_index, index_stride, maxSegments) ||
        (long long)nblocks * maxSegments > 0x7FFFFFFFll)
        return einval("%s: maxSegments %d x %d blocks, index at %p with stride %zu (need 16-byte "
                      "alignment, a stride that is a multiple of 16 and >= 16 + 8 (maxSegments + "
                      "1), and fewer than 2^31 segments in all)", who, maxSegments, nblocks,
                      d_index, index_stride);
    if (int rc = check_device()) return rc;
    IndexedArgs a{};
    a.src = d_src;
    a.src_size = d_compressedSize;
    a.dst = d_dst;
    a.dst_cap = d_maxDecompressedSize;
    a.index = (const char *)d_index;
    a.index_stride = index_stride;
    a.max_seg = maxSegments;
    a.result = d_result;
    a.nblocks = nblocks;
    return finish_launch(launch_decode_indexed(a, (hipStream_t)stream),
                         "lz4_index_check_kernel + lz4_decode_indexed_kernel");
}

int APE_LZ4_decompress_range_indexed_batch_dev(const char *const *d_src,
                                               const int *d_compressedSize, const void *d_index,
                                               size_t index_stride, int maxSegments, int nblocks,
                                               const int *d_blockOf, const int *d_rangeStart,
                                               const int *d_rangeLen, char *const *d_dst,
                                               const int *d_dstCap, int *d_window, int *d_result,
                                               int nreq, int wavesPerRequest, void *stream) {
    const char *who = "decompress_range_indexed_batch_dev";
    if ((!d_blockOf && nreq != nblocks) ||
        bad_arrays(nblocks, {d_src, d_compressedSize, d_index}) ||
        bad_arrays(nreq, {d_rangeStart, d_rangeLen, d_dst, d_dstCap, d_window, d_result}))
        return einval("%s: invalid argument (a null array, a negative count, or no d_blockOf "
                      "with nreq %d != nblocks %d)", who, nreq, nblocks);
    // nreq x wavesPerRequest waves in a one-dimensional grid
    if (wavesPerRequest < 1 || (long long)nreq * wavesPerRequest > 0x7FFFFFFFll ||
        !index_ok(d_index, index_stride, maxSegments))
        return einval("%s: %d requests x %d waves, maxSegments %d, index at %p with stride %zu "
                      "(need wavesPerRequest >= 1, fewer than 2^31 waves in all, maxSegments >= 1, "
                      "16-byte alignment and a stride that is a multiple of 16 and >= 16 + 8 "
                      "(maxSegments + 1))", who, nreq, wavesPerRequest, maxSegments, d_index,
                      index_stride);
    if (int rc = check_device()) return rc;
    RangeArgs a{};
    a.src = d_src;
    a.src_size = d_compressedSize;
    a.index = (const char *)d_index;
    a.index_stride = index_stride;
    a.max_seg = maxSegments;
    a.nblocks = nblocks;
    a.block_of = d_blockOf;
    a.start = d_rangeStart;
    a.len = d_rangeLen;
    a.dst = d_dst;
    a.dst_cap = d_dstCap;
    a.window = d_window;
    a.result = d_result;
    a.nreq = nreq;
    a.waves = wavesPerRequest;
    return finish_launch(launch_decode_range(a, (hipStream_t)stream),
                         "lz4_range_plan_kernel + lz4_decode_range_kernel");
}

// ---- the high-ratio mode on inputs of any size (lz4_large.hip launch_large_hc) ----
size_t APE_LZ4_compress_large_hc_scratch_size(int nblocks, int maxSrcSize, int passSlices) {
    return large_hc_scratch(nblocks, maxSrcSize, passSlices, kHcSlotBytes);
}

size_t APE_LZ4_compress_large_hc_opt_scratch_size(int nblocks, int maxSrcSize, int passSlices) {
    return large_hc_scratch(nblocks, maxSrcSize, passSlices, kHcOptSlotBytes);
}

int APE_LZ4_compress_large_hc_opt_batch_dev(const char *const *d_src, const int *d_srcSize,
                                            char *const *d_dst, const int *d_dstCap,
                                            int *d_result, int nblocks, int maxSrcSize, int depth,
                                            void *d_scratch, size_t scratch_bytes,
                                            int restartBytes, void *d_index, size_t index_stride,
                                            void *stream) {
    return large_hc_batch("compress_large_hc_opt_batch_dev", true,
                          large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks,
                                   maxSrcSize, d_scratch, restartBytes, d_index, index_stride),
                          depth, scratch_bytes, stream, nullptr);
}

int APE_LZ4_compress_large_hc_batch_dev(const char *const *d_src, const int *d_srcSize,
                                        char *const *d_dst, const int *d_dstCap, int *d_result,
                                        int nblocks, int maxSrcSize, int depth, void *d_scratch,
                                        size_t scratch_bytes, int restartBytes, void *d_index,
                                        size_t index_stride, void *stream) {
    return large_hc_batch("compress_large_hc_batch_dev", false,
                          large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks,
                                   maxSrcSize, d_scratch, restartBytes, d_index, index_stride),
                          depth, scratch_bytes, stream, nullptr);
}

int APE_LZ4_compress_large_hc_timed_dev(const char *const *d_src, const int *d_srcSize,
                                        char *const *d_dst, const int *d_dstCap, int *d_result,
                                        int nblocks, int maxSrcSize, int depth, void *d_scratch,
                                        size_t scratch_bytes, int restartBytes, void *stream,
                                        float *ms6) {
    if (!ms6) return einval("compress_large_hc_timed_dev: ms6 is null");
    return large_hc_batch("compress_large_hc_timed_dev", false,
                          large_in(d_src, d_srcSize, d_dst, d_dstCap, d_result, nblocks,
                                   maxSrcSize, d_scratch, restartBytes),
                          depth, scratch_bytes, stream, ms6);
}

// ---- the strided form, and the framed stream of independent blocks (lz4_frame.hip) ----
int APE_LZ4_compress_batch_strided_dev(const char *d_src, size_t src_stride, const int *d_srcSize,
                                       char *d_dst, size_t dst_stride, const int *d_dstCap,
                                       int *d_result, int nblocks, void *stream) {
    BlockArgs a = strided_args(d_src, src_stride, d_srcSize, d_dst, dst_stride, d_dstCap,
                               d_result, nblocks);
    if (int rc = ready_strided("compress_batch_strided_dev", a)) return rc;
    return finish_launch(launch_encode(a, (hipStream_t)stream), "lz4_encode_kernel");
}

int APE_LZ4_decompress_safe_batch_strided_dev(const char *d_src, size_t src_stride,
                                              const int *d_compressedSize, char *d_dst,
                                              size_t dst_stride, const int *d_maxDecompressedSize,
                                              int *d_result, int nblocks, void *stream) {
    BlockArgs a = strided_args(d_src, src_stride, d_compressedSize, d_dst, dst_stride,
                               d_maxDecompressedSize, d_result, nblocks);
    if (int rc = ready_strided("decompress_safe_batch_strided_dev", a)) return rc;
    return finish_launch(launch_decode(a, false, (hipStream_t)stream), "lz4_decode_kernel");
}

size_t APE_LZ4_frame_scratch_size(int nblocks) {
    return nblocks < 0 ? 0 : (size_t)frame_scratch_elems(nblocks) * sizeof(long long);
}

// (the offsets have nblocks + 1 entries: the arrays are needed for an empty batch too)
int APE_LZ4_frame_offsets_dev(const int *d_compressedSize, long long *d_off,
                              void *d_scratch, int nblocks, void *stream) {
    if (nblocks < 0 || !d_compressedSize || !d_off || !d_scratch)
        return einval("frame_offsets_dev: invalid argument (a null array or a negative count, "
                      "nblocks %d)", nblocks);
    if (int rc = check_device()) return rc;
    return finish_launch(launch_frame_offsets(d_compressedSize, d_off, (long long *)d_scratch,
                                              nblocks, (hipStream_t)stream),
                         "frame offsets");
}

int APE_LZ4_frame_pack_strided_dev(const char *d_comp, size_t comp_stride,
                                   const int *d_compressedSize, const long long *d_off,
                                   char *d_frames, int nblocks, void *stream) {
    if (int rc = check_arrays("frame_pack_strided_dev", nblocks,
                              {d_comp, d_compressedSize, d_off, d_frames}))
        return rc;
    if (int rc = check_device()) return rc;
    return finish_launch(launch_frame_pack(d_comp, comp_stride, d_compressedSize, d_off,
                                           d_frames, nblocks, (hipStream_t)stream),
                         "frame pack");
}

int APE_LZ4_decompress_safe_frames_dev(const char *d_frames, const long long *d_off,
                                       char *d_dst, size_t dst_stride,
                                       const int *d_maxDecompressedSize, int *d_result,
                                       int nblocks, void *stream) {
    BlockArgs a = strided_args(d_frames, 0, nullptr, d_dst, dst_stride, d_maxDecompressedSize,
                               d_result, nblocks);
    a.frame_off = d_off;
    if (int rc = ready_strided("decompress_safe_frames_dev", a)) return rc;
    return finish_launch(launch_decode(a, false, (hipStream_t)stream), "lz4_decode_kernel");
}

int APE_LZ4_compress_batch_host(const char *const *h_src, const int *h_srcSize,
                                char *const *h_dst, const int *h_dstCap, int *h_result,
                                int nblocks) {
    return host_batch("compress_batch_host", 0, 1, h_src, h_srcSize, h_dst, h_dstCap, nullptr,
                      h_result, nblocks);
}

int APE_LZ4_decompress_safe_batch_host(const char *const *h_src, const int *h_compressedSize,
                                       char *const *h_dst, const int *h_maxDecompressedSize,
                                       int *h_result, int nblocks) {
    return host_batch("decompress_safe_batch_host", 1, 1, h_src, h_compressedSize, h_dst,
                      h_maxDecompressedSize, nullptr, h_result, nblocks);
}

int APE_LZ4_synth_blocks_dev(char *d_out, size_t stride, int blockSize, long long first_block,
                             int nblocks, int kind, void *stream) {
    if (nblocks < 0 || blockSize < 0 || blockSize > kMaxBlock || (nblocks > 0 && !d_out) ||
        stride < (size_t)blockSize)
        return einval("synth_blocks_dev: nblocks %d of %d bytes (0..%d) at %p with stride %zu",
                      nblocks, blockSize, kMaxBlock, d_out, stride);
    if (int rc = check_device()) return rc;
    return finish_launch(launch_synth(d_out, stride, blockSize, first_block, nblocks, kind,
                                      (hipStream_t)stream),
                         "lz4_synth_kernel");
}

// ---- the LZ4 frame format (include/ape_lz4f.h, lz4_lz4f.hip) ----
int APE_LZ4_xxh32_batch_dev(const char *const *d_src, const int *d_size, unsigned seed,
                            unsigned *d_hash, int n, void *stream) {
    if (int rc = check_arrays("xxh32_batch_dev", n, {d_src, d_size, d_hash})) return rc;
    if (int rc = check_device()) return rc;
    return finish_launch(launch_xxh32(d_src, d_size, seed, d_hash, n, (hipStream_t)stream),
                         "xxh32_batch_kernel");
}

size_t APE_LZ4_lz4f_compress_bound(int srcSize, int flags) {
    if (srcSize < 0 || srcSize > kLfMaxSrc || (flags & ~7)) return 0;
    const size_t nb = ((size_t)srcSize + kMaxBlock - 1) / kMaxBlock;
    return (size_t)((flags & 4) ? kLfHeaderMax : kLfHeaderMin) + (size_t)srcSize +
           nb * ((flags & 2) ? 8 : 4) + ((flags & 1) ? 8 : 4);
}

size_t APE_LZ4_lz4f_compress_scratch_size(int nframes, int maxSrcSize) {
    if (nframes < 0 || maxSrcSize < 0 || maxSrcSize > kLfMaxSrc) return 0;
    return lz4f_compress_layout(nframes, maxSrcSize, 4, nullptr);
}

int APE_LZ4_lz4f_compress_batch_dev(const char *const *d_src, const int *d_srcSize,
                                    char *const *d_dst, const int *d_dstCap, int *d_result,
                                    int nframes, int maxSrcSize, int flags, void *d_scratch,
                                    size_t scratch_bytes, void *stream) {
    const char *who = "lz4f_compress_batch_dev";
    if (int rc = check_arrays(who, nframes, {d_src, d_srcSize, d_dst, d_dstCap, d_result}))
        return rc;
    const size_t need = APE_LZ4_lz4f_compress_scratch_size(nframes, maxSrcSize);
    if (maxSrcSize < 0 || maxSrcSize > kLfMaxSrc || (flags & ~7) || need == (size_t)-1 ||
        (nframes > 0 && (!d_scratch || scratch_bytes < need || !aligned16(d_scratch))))
        return einval("%s: nframes %d, maxSrcSize %d (0..%d), flags %d (0..7), scratch of %zu "
                      "bytes at %p (need %zu bytes 16-byte aligned, fewer than 2^24 blocks)", who,
                      nframes, maxSrcSize, kLfMaxSrc, flags, scratch_bytes, d_scratch, need);
    if (int rc = check_device()) return rc;
    LfCompress c{};
    c.src = d_src;
    c.src_size = d_srcSize;
    c.dst = d_dst;
    c.dst_cap = d_dstCap;
    c.result = d_result;
    c.nframes = nframes;
    c.max_src = maxSrcSize;
    c.flags = flags;
    c.buf = (char *)d_scratch;
    lz4f_compress_layout(nframes, maxSrcSize, 4, &c);
    return finish_launch(launch_lz4f_compress(c, (hipStream_t)stream), "lz4f_compress");
}

// ---- framed compress with preferences (include/ape_lz4f_prefs.h, lz4_lz4f.hip) ----
size_t APE_LZ4_lz4f_compress_prefs_bound(int srcSize, int blockSizeID, int flags) {
    if (srcSize < 0 || srcSize > kLfMaxSrc || blockSizeID < 4 || blockSizeID > 7 || (flags & ~7))
        return 0;
    const size_t B = lf_block_bytes(blockSizeID), nb = ((size_t)srcSize + B - 1) / B;
    return (size_t)((flags & 4) ? kLfHeaderMax : kLfHeaderMin) + (size_t)srcSize +
           nb * ((flags & 2) ? 8 : 4) + ((flags & 1) ? 8 : 4);
}

size_t APE_LZ4_lz4f_compress_prefs_scratch_size(int nframes, int maxSrcSize, int blockSizeID,
                                                int mode, int passSlices) {
    return lf_prefs_scratch(nframes, maxSrcSize, blockSizeID, mode, passSlices, nullptr, nullptr);
}

int APE_LZ4_lz4f_compress_prefs_batch_dev(const char *const *d_src, const int *d_srcSize,
                                          char *const *d_dst, const int *d_dstCap, int *d_result,
                                          int nframes, int maxSrcSize, int blockSizeID, int mode,
                                          int depth, int flags, void *d_scratch,
                                          size_t scratch_bytes, void *stream) {
    const char *who = "lz4f_compress_prefs_batch_dev";
    if (int rc = check_arrays(who, nframes, {d_src, d_srcSize, d_dst, d_dstCap, d_result}))
        return rc;
    // the least scratch: one slice per pass
    size_t frame = 0, large = 0;
    const size_t need = lf_prefs_scratch(nframes, maxSrcSize, blockSizeID, mode, 1, &frame, &large);
    if (maxSrcSize < 0 || maxSrcSize > kLfMaxSrc || !lf_prefs_ok(blockSizeID, mode) || depth < 0 ||
        depth > (mode ? kHcMaxDepth : 0) || (flags & ~7) || need == (size_t)-1 ||
        (nframes > 0 && (!d_scratch || scratch_bytes < need || !aligned16(d_scratch))))
        return einval("%s: nframes %d, maxSrcSize %d (0..%d), blockSizeID %d (4..7), mode %d "
                      "(0..2), depth %d (0..%d; 0 with mode 0), flags %d (0..7), scratch of %zu "
                      "bytes at %p (need %zu bytes 16-byte aligned, fewer than 2^24 blocks and "
                      "slices)", who, nframes, maxSrcSize, kLfMaxSrc, blockSizeID, mode, depth,
                      kHcMaxDepth, flags, scratch_bytes, d_scratch, need);
    if (int rc = check_device()) return rc;
    if (nframes == 0) return APE_LZ4_GPU_OK;
    LfCompress c{};
    c.src = d_src;
    c.src_size = d_srcSize;
    c.dst = d_dst;
    c.dst_cap = d_dstCap;
    c.result = d_result;
    c.nframes = nframes;
    c.max_src = maxSrcSize;
    c.flags = flags;
    c.buf = (char *)d_scratch;
    lz4f_compress_layout(nframes, maxSrcSize, blockSizeID, &c);
    LargeArgs a{};
    a.src = c.s_src;
    a.src_size = c.s_size;
    a.dst = c.s_dst;
    a.dst_cap = c.s_cap;
    a.result = c.s_res;
    a.nblocks = c.nslots;
    a.max_src = (int)lf_block_bytes(blockSizeID);
    a.buf = (char *)d_scratch + frame;
    large_scratch_layout(a.nblocks, a.max_src, &a);
    // as many slices per pass as the caller's scratch holds
    const size_t slot = mode == 2 ? kHcOptSlotBytes : kHcSlotBytes;
    const int pass = mode ? large_hc_pass(a.nslots, (long long)((scratch_bytes - frame - large) / slot))
                          : 0;
    return finish_launch(launch_lz4f_prefs_compress(c, a, mode, depth ? depth : kHcDefaultDepth,
                                                    (char *)d_scratch + frame + large, pass,
                                                    (hipStream_t)stream),
                         "lz4f_compress_prefs");
}

int APE_LZ4_lz4f_info_batch_dev(const char *const *d_src, const int *d_srcSize, int *d_info,
                                int nframes, void *stream) {
    if (int rc = check_arrays("lz4f_info_batch_dev", nframes, {d_src, d_srcSize, d_info}))
        return rc;
    if (int rc = check_device()) return rc;
    return finish_launch(launch_lz4f_info(d_src, d_srcSize, d_info, nframes, (hipStream_t)stream),
                         "lz4f_info_kernel");
}

size_t APE_LZ4_lz4f_decompress_scratch_size(int nframes, int maxBlocks) {
    return lz4f_decode_scratch(nframes, maxBlocks, false);
}

int APE_LZ4_lz4f_decompress_batch_dev(const char *const *d_src, const int *d_srcSize,
                                      char *const *d_dst, const int *d_dstCap, int *d_result,
                                      int nframes, int maxBlocks, int flags, void *d_scratch,
                                      size_t scratch_bytes, void *stream) {
    return lz4f_decode_batch("lz4f_decompress_batch_dev", false, d_src, d_srcSize, d_dst, d_dstCap,
                             d_result, nframes, maxBlocks, flags, d_scratch, scratch_bytes, stream);
}

// ---- frames with short blocks (include/ape_lz4f_placed.h, lz4_decode.hip, lz4_lz4f.hip) ----
int APE_LZ4_decompress_safe_size_batch_dev(const char *const *d_src, const int *d_srcSize,
                                           const int *d_dstCap, const int *d_dictSize,
                                           int *d_result, int n, void *stream) {
    if (int rc = check_arrays("decompress_safe_size_batch_dev", n,
                              {d_src, d_srcSize, d_dstCap, d_result}))
        return rc;
    if (int rc = check_device()) return rc;
    BlockArgs a{};
    a.src = d_src;
    a.src_size = d_srcSize;
    a.dst_cap = d_dstCap;
    a.dict_size = d_dictSize;
    a.result = d_result;
    a.nblocks = n;
    return finish_launch(launch_decode_size(a, (hipStream_t)stream), "lz4_decode_size_kernel");
}

size_t APE_LZ4_lz4f_decompress_placed_scratch_size(int nframes, int maxBlocks) {
    return lz4f_decode_scratch(nframes, maxBlocks, true);
}

int APE_LZ4_lz4f_decompress_placed_batch_dev(const char *const *d_src, const int *d_srcSize,
                                             char *const *d_dst, const int *d_dstCap,
                                             int *d_result, int nframes, int maxBlocks, int flags,
                                             void *d_scratch, size_t scratch_bytes, void *stream) {
    return lz4f_decode_batch("lz4f_decompress_placed_batch_dev", true, d_src, d_srcSize, d_dst,
                             d_dstCap, d_result, nframes, maxBlocks, flags, d_scratch,
                             scratch_bytes, stream);
}

// ---- frames with a dictionary (include/ape_lz4f_dict.h, lz4_lz4f.hip) ----
int APE_LZ4_lz4f_info_dict_batch_dev(const char *const *d_src, const int *d_srcSize, int *d_info,
                                     int nframes, void *stream) {
    if (int rc = check_arrays("lz4f_info_dict_batch_dev", nframes, {d_src, d_srcSize, d_info}))
        return rc;
    if (int rc = check_device()) return rc;
    return finish_launch(launch_lz4f_info_dict(d_src, d_srcSize, d_info, nframes,
                                               (hipStream_t)stream),
                         "lz4f_info_kernel");
}

size_t APE_LZ4_lz4f_compress_usingCDicts_bound(int srcSize, int flags) {
    if (srcSize < 0 || srcSize > kMaxBlock || (flags & ~7)) return 0;
    return (size_t)((flags & 4) ? kLfHeaderMax : kLfHeaderMin) + 4 + (size_t)srcSize +
           (srcSize ? ((flags & 2) ? 8 : 4) : 0) + ((flags & 1) ? 8 : 4);
}

size_t APE_LZ4_lz4f_compress_usingCDicts_scratch_size(int nframes, int maxSrcSize, int mode) {
    if (nframes < 0 || maxSrcSize < 1 || maxSrcSize > kMaxBlock || mode < 0 || mode > 2) return 0;
    const size_t frame = lz4f_dict_compress_layout(nframes, maxSrcSize, nullptr);
    if (frame == (size_t)-1) return frame;
    return frame + (mode ? up16(hc_cdict_scratch(nframes, maxSrcSize, mode == 2)) : 0);
}

int APE_LZ4_lz4f_compress_usingCDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                char *const *d_dst, const int *d_dstCap,
                                                int *d_result, int nframes,
                                                const void *const *d_cdict,
                                                const unsigned *d_dictID, int maxSrcSize, int mode,
                                                int depth, int flags, void *d_scratch,
                                                size_t scratch_bytes, void *stream) {
    const char *who = "lz4f_compress_usingCDicts_batch_dev";
    if (int rc = check_arrays(who, nframes, {d_src, d_srcSize, d_dst, d_dstCap, d_result, d_cdict}))
        return rc;
    const size_t need = APE_LZ4_lz4f_compress_usingCDicts_scratch_size(nframes, maxSrcSize, mode);
    if (maxSrcSize < 1 || maxSrcSize > kMaxBlock || mode < 0 || mode > 2 || depth < 0 ||
        depth > (mode ? kHcMaxDepth : 0) || (flags & ~7) || need == (size_t)-1 ||
        (nframes > 0 && (!d_scratch || scratch_bytes < need || !aligned16(d_scratch))))
        return einval("%s: nframes %d, maxSrcSize %d (1..%d), mode %d (0..2), depth %d (0..%d; 0 "
                      "with mode 0), flags %d (0..7), scratch of %zu bytes at %p (need %zu bytes "
                      "16-byte aligned, fewer than 2^24 frames)", who, nframes, maxSrcSize,
                      kMaxBlock, mode, depth, kHcMaxDepth, flags, scratch_bytes, d_scratch, need);
    if (int rc = check_device()) return rc;
    if (nframes == 0) return APE_LZ4_GPU_OK;
    const hipStream_t s = (hipStream_t)stream;
    LfCompress c{};
    c.src = d_src;
    c.src_size = d_srcSize;
    c.dst = d_dst;
    c.dst_cap = d_dstCap;
    c.result = d_result;
    c.nframes = nframes;
    c.max_src = maxSrcSize;
    c.flags = flags;
    c.dict_id = d_dictID;
    c.buf = (char *)d_scratch;
    const size_t frame = lz4f_dict_compress_layout(nframes, maxSrcSize, &c);
    hipError_t e = launch_lz4f_dict_compress_plan(c, s);
    if (e == hipSuccess && mode == 0) {
        BlockArgs a{};
        a.src = c.s_src;
        a.dst = c.s_dst;
        a.src_size = c.s_size;
        a.dst_cap = c.s_cap;
        a.result = c.s_res;
        a.nblocks = nframes;
        e = launch_encode_cdicts(a, d_cdict, s);
    } else if (e == hipSuccess) {
        e = hc_cdict_passes(mode == 2, c.s_src, c.s_size, c.s_dst, c.s_cap, c.s_res, nframes,
                            nullptr, d_cdict, maxSrcSize, depth, (char *)d_scratch + frame,
                            need - frame, s);
    }
    if (e == hipSuccess) e = launch_lz4f_dict_compress_rest(c, s);
    return finish_launch(e, "lz4f_compress_usingCDicts");
}

size_t APE_LZ4_lz4f_decompress_usingDicts_scratch_size(int nframes, int maxBlocks, int flags) {
    if (flags & ~7) return 0;
    return lz4f_decode_scratch(nframes, maxBlocks, (flags & 4) != 0);
}

int APE_LZ4_lz4f_decompress_usingDicts_batch_dev(const char *const *d_src, const int *d_srcSize,
                                                 char *const *d_dst, const int *d_dstCap,
                                                 int *d_result, int nframes, int maxBlocks,
                                                 const unsigned *d_tableID,
                                                 const char *const *d_tableDict,
                                                 const int *d_tableDictSize, int ntable, int flags,
                                                 void *d_scratch, size_t scratch_bytes,
                                                 void *stream) {
    const char *who = "lz4f_decompress_usingDicts_batch_dev";
    if (flags & ~7) return einval("%s: flags %d (0..7)", who, flags);
    const LfTable table{d_tableID, d_tableDict, d_tableDictSize, ntable};
    return lz4f_decode_batch(who, (flags & 4) != 0, d_src, d_srcSize, d_dst, d_dstCap, d_result,
                             nframes, maxBlocks, flags & 3, d_scratch, scratch_bytes, stream,
                             &table);
}

#ifdef APE_LZ4_STATS
}  // extern "C"
namespace apelz4 {
hipError_t dec_stats_read(unsigned long long *out, int reset);
hipError_t enc_stats_read(unsigned long long *out, int reset);
}
extern "C" {
// Diagnostic build only: per-phase cycle sums (which: 0 = decode, 1 = encode).
int APE_LZ4_debug_stats(int which, unsigned long long *out16, int reset) {
    hipError_t e = which ? apelz4::enc_stats_read(out16, reset) : apelz4::dec_stats_read(out16, reset);
    return e == hipSuccess ? 0 : -1;
}
#endif

// ---- internal shim for the one-shot C API (ape_lz4_api.c) ----
int ape_lz4_gpu_compress_one(const char *src, char *dst, int n, int cap, int accel, int *rt) {
    int res = 0;
    *rt = host_batch("compress_one", 0, accel, &src, &n, &dst, &cap, nullptr, &res, 1);
    return res;
}

int ape_lz4_gpu_decompress_one(const char *src, char *dst, int csize, int cap, int partial,
                               int target, int *rt) {
    int res = 0;
    *rt = host_batch("decompress_one", partial ? 2 : 1, 1, &src, &csize, &dst, &cap,
                     partial ? &target : nullptr, &res, 1);
    return res;
}

}  // extern "C"
