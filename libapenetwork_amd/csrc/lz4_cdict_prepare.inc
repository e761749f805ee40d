// lz4_cdict_prepare.inc -- the body of lz4_cdict.hip's two prepare kernels, included into each:
// one object at `cd` from dict[dict_size - D, dict_size) for messages of up to max_src bytes.
// (As text and not as a function: a body inlined from a function is optimised on its own first,
// without the kernel's launch bounds and argument kinds, and the single kernel's code then
// differs from what it was; profiles/cdicts_asm_diff.txt.)
    __shared__ __attribute__((aligned(16))) uint16_t tab[kHSize];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int Di = cdict_window(dict_size, max_src);
    if (Di < 64) Di = 0;
    const uint32_t D = (uint32_t)Di;
    gcu8 *src = (gcu8 *)dict + (dict_size - Di);   // window position v = src[v]

    for (int i = tid; i < kHSize / 8; i += kPrepThreads) ((uint4 *)tab)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    if (wave == 0) {
        constexpr int kU = 8;   // loads in flight per trip (the loop is latency bound)
        for (uint32_t v0 = 0; v0 < D; v0 += 192u * kU) {
            uint2 x[kU];
            bool ok[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const uint32_t v = v0 + 192u * u + 3u * (uint32_t)lane;
                ok[u] = v + 8u <= D;
                x[u] = ok[u] ? gload8(src + v) : make_uint2(0, 0);
            }
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const uint32_t v = v0 + 192u * u + 3u * (uint32_t)lane;
                if (ok[u]) tab[hashk(x[u].x, x[u].y)] = (uint16_t)v;
            }
        }
    } else {
        const int t = tid - 64, nt = kPrepThreads - 64;
        if (t == 0) {
            CDictHdr H;
            H.magic = kCdMagic;
            H.D = D;
            H.max_src = (uint32_t)max_src;
            H.zero = 0u;
            *(CDictHdr *)cd = H;
        }
        // [kCdWin, kCdSize) in 16-byte pieces: pad, window, pad (D is a multiple of 64)
        gu8 *w = (gu8 *)cd + kCdWin;
        constexpr uint32_t kPieces = (kCdSize - kCdWin) / 16u;
        for (uint32_t i = (uint32_t)t; i < kPieces; i += (uint32_t)nt) {
            const uint32_t at = 16u * i;          // byte of the region; window byte at - kCdFront
            uint4 v = make_uint4(0, 0, 0, 0);
            if (at >= kCdFront && at - kCdFront < D) v = gload16(src + (at - kCdFront));
            gstore16(w + at, v);
        }
    }
    __syncthreads();
    uint4 *img = (uint4 *)(cd + kCdTab);
    for (int i = tid; i < kHSize / 8; i += kPrepThreads) img[i] = ((const uint4 *)tab)[i];
