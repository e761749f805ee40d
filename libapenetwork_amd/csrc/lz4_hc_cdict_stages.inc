// lz4_hc_cdict_stages.inc -- the four stage kernels of lz4_hc_cdict.hip, included once per form
// of the call: one object for the batch (HCD_PER false: APE_LZ4_compress_hc[_opt]_usingCDict_
// batch_dev) and one per message (HCD_PER true, with the device array `cdicts` as a further
// parameter: ..._usingCDicts_batch_dev, DESIGN.md 3.22).  HCD_KERNEL names a form's kernels,
// HCD_PARAM and HCD_ARG are its further parameter and argument, HCD_OBJECT is the opened
// object.  (As text and not as functions called from thin kernels: see lz4_cdict_prepare.inc.)
__global__ void __launch_bounds__(64) HCD_KERNEL(chain)(HcDictArgs a HCD_PARAM) {
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    if (!open_object<HCD_PER>(a, &W, b HCD_ARG)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;   // no position can match: nothing is read
    const uint4 *img = (const uint4 *)(HCD_OBJECT + kHdHead);
    for (int i = lane; i < kHcTable / 8; i += 64) ((uint4 *)head)[i] = img[i];
    wave_sync();
    // positions D - 3 .. D + n - 4 (from 0 when the dictionary is shorter than 3 bytes)
    hc_chain_build(W, head, max(W.origin - 3, 0), W.origin + n - kMinMatch, lane);
}

__global__ void __launch_bounds__(kHcdThreads) HCD_KERNEL(search)(HcDictArgs a, int groups HCD_PARAM) {
    const int b = blockIdx.x / groups;
    SplitView W;
    if (!open_object<HCD_PER>(a, &W, b HCD_ARG)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;
    // (a workgroup past the last searchable position leaves here)
    const int i = (int)(blockIdx.x % groups) * kHcdThreads + (int)threadIdx.x;
    if (i > n - kMFLimit) return;
    a.match[(size_t)b * a.match_stride + i] = hc_search(W, n, i, a.depth);
}

__global__ void __launch_bounds__(64) HCD_KERNEL(parse)(HcDictArgs a HCD_PARAM) {
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    int n, cap;
    if (!open_parse<HCD_PER>(a, &W, b, lane, &n, &cap HCD_ARG)) return;
    Emitter em{(gu8 *)a.dst[b], W.msg, (uint32_t)cap, 0u, lane};
    uint32_t tail;
    const int result = hc_lazy_parse(W, n, a.match + (size_t)b * a.match_stride, em, &tail);
    if (lane == 0) a.result[b] = result;
}

__global__ void __launch_bounds__(64) HCD_KERNEL(opt_parse)(HcDictOptArgs o HCD_PARAM) {
    const HcDictArgs &a = o.a;
    const int b = blockIdx.x, lane = lane_id();
    SplitView W;
    int n, cap;
    if (!open_parse<HCD_PER>(a, &W, b, lane, &n, &cap HCD_ARG)) return;
    Emitter em{(gu8 *)a.dst[b], W.msg, (uint32_t)cap, 0u, lane};
    uint32_t tail;
    const int result = hc_opt_parse(W, n, a.match + (size_t)b * a.match_stride,
                                    o.cost + (size_t)b * o.cost_stride, em, false, &tail);
    if (lane == 0) a.result[b] = result;
}
