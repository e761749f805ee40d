// lz4_hc_cdict_prepare.inc -- the body of lz4_hc_cdict.hip's two prepare kernels, included into
// each: one object at `cd` from dict[dict_size - D, dict_size) for messages of up to max_src
// bytes.  (As text and not as a function: see lz4_cdict_prepare.inc.)
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
