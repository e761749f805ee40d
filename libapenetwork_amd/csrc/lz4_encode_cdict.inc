// lz4_encode_cdict.inc -- one block against the prepared dictionary at `cd` whose header is H:
// the body of lz4_encode.hip's two EXT kernels from the header check on, included into each
// (S, a, b, tid, lane and wave are the kernel's).  (As text and not as a function: see
// lz4_cdict_prepare.inc.)
    if (H.magic != kCdMagic || H.D > kCdMaxWin || (H.D & 63u) != 0u || H.max_src < 1u ||
        H.max_src > (uint32_t)kMaxBlock || H.D + H.max_src > (uint32_t)kMaxBlock) {
        if (tid == 0) a.result[b] = 0;
        return;
    }
    const int nr = a.src_size[b];
    const int icap = a.dst_cap[b];
    if (nr < 0 || nr > (int)H.max_src || icap < 0) {
        if (tid == 0) a.result[b] = (nr > (int)H.max_src) ? kErange : 0;
        return;
    }
    const int D = (int)H.D;
    Blk B;
    B.win = (gcu8 *)(cd + kCdWin + kCdFront);
    B.D = (uint32_t)D;
    B.in = (gcu8 *)a.src[b] - D;     // (an address only: nothing below position D is read from it)
    B.dst = (gu8 *)a.dst[b];
    B.n = D + nr;
    B.nr = (uint32_t)nr;
    B.k0 = D / 64;
    B.stride = 1u;
    B.cap = (uint32_t)icap;
    B.un = (uint32_t)B.n;
    B.mstart = B.un >= 12 ? B.un - 12 : 0;
    B.mlimit = B.un >= 5 ? B.un - 5 : 0;
    B.nch = (B.n + 63) / 64;

    // table = the prepared image (all zero for D = 0: the state of a block without history)
    const uint4 *img = (const uint4 *)(cd + kCdTab);
    for (int i = tid; i < kHSize / 8; i += 192) ((uint4 *)S.tab)[i] = img[i];
    for (int i = tid; i < (int)(kRingE / 16 + 4); i += 192) ((uint4 *)S.ring)[i] = make_uint4(0, 0, 0, 0);
    if (tid == 0) S.qn[0] = S.qn[1] = 0u;
    __syncthreads();
    if (B.n < kSmall) encode_block<true, false, true>(S, B, wave, lane, &a.result[b], nullptr);
    else encode_block<false, false, true>(S, B, wave, lane, &a.result[b], nullptr);
