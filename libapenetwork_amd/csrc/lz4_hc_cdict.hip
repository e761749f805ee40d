// lz4_hc_cdict.hip -- the high-ratio mode against a prepared dictionary shared by a batch
// (APE_LZ4_hc_cdict_prepare_dev, APE_LZ4_compress_hc_usingCDict_batch_dev).
//
// The block of message m is compress_hc_withPrefix's for the window [dictionary tail | m]
// (tests/hcdictmodel.py is the definition), without staging that window: window position w is
// the object's byte w when w < D and the message's byte w - D otherwise.  The chain build over
// the positions whose 4 bytes lie in the dictionary is done once, by the prepare kernel; a
// message's chain kernel starts from that head table and inserts only the positions D - 3 on
// (the first three straddle dictionary and message).  A chain walk follows the object's
// chain[] below D - 3 and the message's scratch from there on.  The search and the parse are
// lz4_encode_hc.hip's, rule for rule, with loads that pick their side of the boundary.
// APE_LZ4_compress_hc_opt_usingCDict_batch_dev runs the same chain build and
// search and then lz4_encode_hc_opt.hip's cost-minimising parse, in message positions.
//
// Every kernel checks the object's header before it uses anything else of it.  Every load of a
// message stays inside src[0, n), every load of the object inside it, every store inside
// dst[0, cap).
#include "lz4_gpu_internal.h"

namespace apelz4 {
namespace {

constexpr int kPrepThreads = 256;

// One wave's LDS stores, made visible to its own later loads (the chain build runs on a single
// wave, so no workgroup barrier is needed -- and the prepare kernel's other waves must not
// meet one).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// One step of lz4_hc_chain_kernel's rule: 64 positions base + lane with hashes h (an invalid
// lane brings a hash no other lane has) enter the head table; returns chain[base + lane].
__device__ __forceinline__ uint32_t chain_step(volatile uint16_t *vhead, int base, int lane,
                                               bool valid, uint32_t h) {
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t me = (uint32_t)(base + lane) + 1u;
    const uint32_t prev = valid ? vhead[h] : 0u;
    if (valid) vhead[h] = (uint16_t)me;
    wave_sync();
    const bool lost = valid && vhead[h] != me;
    uint64_t rem = wave_ballot(lost);
    int pred = -1;
    bool owner = false;
    while (rem) {
        const uint32_t hl = lane_val(h, __builtin_ctzll(rem));
        const uint64_t grp = wave_ballot(h == hl);
        if (h == hl) {
            const uint64_t lo = grp & below;
            pred = lo ? 63 - __builtin_clzll(lo) : -1;
            owner = (grp >> lane) == 1ull;
        }
        rem &= ~grp;
    }
    wave_sync();
    if (owner) vhead[h] = (uint16_t)me;
    wave_sync();
    return pred >= 0 ? (uint32_t)(base + pred) + 1u : prev;
}

// The window of one message: positions [0, D) in the object, [D, D + n) in the message.
struct Window {
    gcu8 *dict, *msg;
    int D;
    __device__ __forceinline__ uint32_t byte(int w) const { return w < D ? dict[w] : msg[w - D]; }
    __device__ __forceinline__ gcu8 *at(int w) const { return w < D ? dict + w : msg + (w - D); }
    // [w, w + len) lies wholly on one side
    __device__ __forceinline__ bool one_side(int w, int len) const { return w + len <= D || w >= D; }
    // the 4 bytes at w <= D + n - 4 (n >= 4); at D - 3 .. D - 1 they come from both sides (the
    // object's load runs into its back pad, and those bytes are masked off)
    __device__ __forceinline__ uint32_t load4(int w) const {
        if (w >= D) return gload4(msg + (w - D));
        const uint32_t lo = gload4(dict + w);
        const int in = D - w;
        if (in >= 4) return lo;
        return (lo & ((1u << (8 * in)) - 1u)) | gload4(msg) << (8 * in);
    }
};

// The header, before anything else of the object: true when it was prepared for a.max_src.
__device__ __forceinline__ bool open_object(const HcDictArgs &a, Window *w, int b) {
    const CDictHdr H = *(const CDictHdr *)a.cdict;
    if (H.magic != kHdMagic || H.max_src != (uint32_t)a.max_src || H.zero != 0u ||
        H.D > (uint32_t)(kMaxBlock - a.max_src))
        return false;
    w->dict = (gcu8 *)a.cdict + (kHdWin + kCdFront);
    w->msg = (gcu8 *)a.src[b];
    w->D = (int)H.D;
    return true;
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
        uint16_t *chain = (uint16_t *)(cd + kHdChain);
        for (int base = 0; base < nchain; base += 64) {
            const int p = base + lane;
            const bool valid = p < nchain;
            const uint32_t h = valid ? hc_hash(gload4(src + p)) : (uint32_t)(kHcTable + lane);
            const uint32_t c = chain_step(head, base, lane, valid, h);
            if (valid) chain[p] = (uint16_t)c;
        }
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

// ---- chain build of one message ----
__global__ void __launch_bounds__(64) lz4_hc_cdict_chain_kernel(HcDictArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];
    const int b = blockIdx.x, lane = lane_id();
    Window W;
    if (!open_object(a, &W, b)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;   // no position can match: nothing is read
    const uint4 *img = (const uint4 *)(a.cdict + kHdHead);
    for (int i = lane; i < kHcTable / 8; i += 64) ((uint4 *)head)[i] = img[i];
    wave_sync();
    // positions D - 3 .. D + n - 4 (from 0 when the dictionary is shorter than 3 bytes)
    uint16_t *chain = a.chain + (size_t)b * a.chain_stride;   // position w at entry w - D + 3
    const int last = W.D + n - kMinMatch;
    for (int base = max(W.D - 3, 0); base <= last; base += 64) {
        const int p = base + lane;
        const bool valid = p <= last;
        const uint32_t h = valid ? hc_hash(W.load4(p)) : (uint32_t)(kHcTable + lane);
        const uint32_t c = chain_step(head, base, lane, valid, h);
        if (valid) chain[p - W.D + 3] = (uint16_t)c;
    }
}

// ---- search ----
__global__ void __launch_bounds__(kHcdThreads) lz4_hc_cdict_search_kernel(HcDictArgs a, int groups) {
    const int b = blockIdx.x / groups;
    Window W;
    if (!open_object(a, &W, b)) return;
    const int n = a.src_size[b];
    if (n < kMinLength || n > a.max_src) return;
    // message position i is window position D + i (a workgroup past the last searchable
    // position leaves here)
    const int i = (int)(blockIdx.x % groups) * kHcdThreads + (int)threadIdx.x;
    if (i > n - kMFLimit) return;
    const int D = W.D;
    // chain[] of window position w: the message's own from D - 3 on (entry w - D + 3)
    const uint16_t *own = a.chain + (size_t)b * a.chain_stride;
    const uint16_t *shared = (const uint16_t *)(a.cdict + kHdChain);   // ... the object's below
    const int mx = min(kHcCap, n - kLastLiterals - i);   // >= 7
    const uint32_t x = gload4(W.msg + i);
    uint32_t cur = own[i + 3], best = 0u, best_q = 0u;
    for (int d = 0; d < a.depth && cur; d++) {
        const int q = (int)cur - 1;
        cur = q < D - 3 ? shared[q] : own[q - D + 3];
        if (W.load4(q) != x) continue;        // a collision, or fewer than 4 bytes: depth spent
        int k = kMinMatch;
        while (k < mx) {
            if (i + k + 16 <= n && W.one_side(q + k, 16)) {
                const uint4 u = gload16(W.msg + i + k), v = gload16(W.at(q + k));
                const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y, d2 = u.z ^ v.z, d3 = u.w ^ v.w;
                if (d0 | d1 | d2 | d3) {
                    k += d0 ? first_diff(d0) : d1 ? 4 + first_diff(d1) : d2 ? 8 + first_diff(d2)
                                                                            : 12 + first_diff(d3);
                    break;
                }
                k += 16;
            } else {                          // across the boundary and at the message's end
                if (W.byte(q + k) != W.msg[i + k]) break;
                k++;
            }
        }
        const uint32_t L = (uint32_t)min(k, mx);
        if (L > best) {                       // strictly longer: a tie stays with the nearer
            best = L;
            best_q = (uint32_t)q;
        }
        if (L == (uint32_t)mx) break;
    }
    a.match[(size_t)b * a.match_stride + i] = best << 16 | best_q;
}

// ---- parse + emit ----
// lz4_hc_parse_kernel's walk in message positions: literals come from the message, a match's
// source is a window position, and only the forward extension of a capped match reads its
// source across the boundary.
__global__ void __launch_bounds__(64) lz4_hc_cdict_parse_kernel(HcDictArgs a) {
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b], cap = a.dst_cap[b];
    Window W;
    const bool ok = open_object(a, &W, b);
    if (!ok || n < 0 || n > a.max_src || cap <= 0) {
        if (lane == 0) a.result[b] = ok && n > a.max_src ? kErange : 0;
        return;
    }
    gcu8 *src = W.msg;
    gu8 *dst = (gu8 *)a.dst[b];
    const uint32_t *M = a.match + (size_t)b * a.match_stride;
    const uint32_t un = (uint32_t)n, ucap = (uint32_t)cap, uD = (uint32_t)W.D;

    auto put = [&](uint32_t o, uint32_t v) {   // one output byte
        if (lane == 0) dst[o] = (uint8_t)v;
    };
    auto put_len = [&](uint32_t o, uint32_t v, uint32_t nb) {   // a length field's nb bytes
        for (uint32_t j = (uint32_t)lane; j < nb; j += 64u)
            dst[o + j] = (uint8_t)(j + 1u == nb ? (v - 15u) % 255u : 255u);
    };
    auto copy = [&](uint32_t o, uint32_t s, uint32_t len) {     // literals
        for (uint32_t j = 16u * (uint32_t)lane; j + 16u <= len; j += 1024u)
            gstore16(dst + o + j, gload16(src + s + j));
        const uint32_t r = len & ~15u;
        if ((uint32_t)lane < len - r) dst[o + r + lane] = src[s + r + lane];
    };

    uint32_t op = 0u, anchor = 0u;
    bool fail = false;
    if (n >= kMinLength) {
        const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;
        uint32_t p = 0u;
        while (p <= last) {
            // 64 positions from p: this one's match and the next one's
            const uint32_t pos = p + (uint32_t)lane;
            const uint32_t m = pos <= last ? M[pos] : 0u;
            const uint32_t len = m >> 16, next_len = pos + 1u <= last ? M[pos + 1u] >> 16 : 0u;
            const uint64_t has = wave_ballot(len > 0u);
            if (!has) {
                p += 64u;
                continue;
            }
            // the lazy step, as lz4_hc_parse_kernel's
            const int first = __builtin_ctzll(has);
            const uint64_t stop = wave_ballot(lane >= first && !(next_len > len));
            if (!stop) {
                p += 63u;
                continue;
            }
            const int sl = __builtin_ctzll(stop);
            const uint32_t sp = p + (uint32_t)sl, mm = lane_val(m, sl);
            const uint32_t q = mm & 0xFFFFu, lim = end - sp;   // q: a window position
            uint32_t L = mm >> 16;
            if (L == umin((uint32_t)kHcCap, lim)) {
                // capped by the search: extend forward to at most the end - 5, 8 bytes per lane
                while (L < lim) {
                    const uint32_t o = L + 8u * (uint32_t)lane;
                    const int qo = (int)(q + o);
                    uint32_t cnt = 0u;
                    if (o + 8u <= lim && W.one_side(qo, 8)) {
                        const uint2 u = gload8(src + sp + o), v = gload8(W.at(qo));
                        const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y;
                        cnt = d0 ? first_diff(d0) : d1 ? 4u + first_diff(d1) : 8u;
                    } else {
                        while (cnt < 8u && o + cnt < lim && src[sp + o + cnt] == W.byte(qo + (int)cnt))
                            cnt++;
                    }
                    const uint64_t part = wave_ballot(cnt < 8u);
                    if (!part) {
                        L += 512u;
                        continue;
                    }
                    const int fl = __builtin_ctzll(part);
                    L += 8u * (uint32_t)fl + lane_val(cnt, fl);
                    break;
                }
            }
            // the sequence, if all of it fits
            const uint32_t lits = sp - anchor, ml = L - (uint32_t)kMinMatch, off = uD + sp - q;
            const uint32_t nlb = len_bytes(lits), nmb = len_bytes(ml);
            if (op + 1u + nlb + lits + 2u + nmb > ucap) {
                fail = true;
                break;
            }
            put(op, umin(lits, 15u) << 4 | umin(ml, 15u));
            op += 1u;
            put_len(op, lits, nlb);
            op += nlb;
            copy(op, anchor, lits);
            op += lits;
            put(op, off & 255u);
            put(op + 1u, off >> 8);
            op += 2u;
            put_len(op, ml, nmb);
            op += nmb;
            p = sp + L;
            anchor = p;
        }
    }
    int result = 0;
    if (!fail) {
        const uint32_t run = un - anchor, nlb = len_bytes(run);
        if (op + 1u + nlb + run <= ucap) {
            put(op, umin(run, 15u) << 4);
            op += 1u;
            put_len(op, run, nlb);
            op += nlb;
            copy(op, anchor, run);
            result = (int)(op + run);
        }
    }
    if (lane == 0) a.result[b] = result;
}

// ---- price + emit (the cost-minimising parse) ----
// lz4_hc_opt_parse_kernel's rule in message positions (lz4_encode_hc_opt.hip describes the
// registers and the run shortcut; tests/hcoptdictmodel.py is the definition): cost[] and match[]
// are indexed by message position, a match's source is a window position, and only the
// extension of a capped match reads its source, on whichever side of the boundary it lies.

// what this wave's lanes stored to global memory so far is what any of its lanes loads from here
// on (lz4_encode_hc_opt.hip's)
__device__ __forceinline__ void own_stores_visible() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// len_bytes() for this kernel alone.  The compiler derives value ranges for a shared helper from
// all of its call sites, so calling len_bytes() here would change the instructions it emits for
// lz4_hc_cdict_parse_kernel, which stays exactly as it was (profiles/hc_opt_cdict_asm_diff.txt).
__device__ __forceinline__ uint32_t opt_len_bytes(uint32_t v) {
    return v >= 15u ? (v - 15u) / 255u + 1u : 0u;
}

// the common prefix of the message from sp on and the window from q on, from L on and at most
// lim (sp + lim <= n - 5): 8 bytes per lane while the source's 8 lie on one side, byte by byte
// across the boundary and at the end
__device__ __forceinline__ uint32_t extend(const Window &W, uint32_t sp, uint32_t q, uint32_t L,
                                           uint32_t lim, int lane) {
    while (L < lim) {
        const uint32_t o = L + 8u * (uint32_t)lane;
        const int qo = (int)(q + o);
        uint32_t cnt = 0u;
        if (o + 8u <= lim && W.one_side(qo, 8)) {
            const uint2 u = gload8(W.msg + sp + o), v = gload8(W.at(qo));
            const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y;
            cnt = d0 ? first_diff(d0) : d1 ? 4u + first_diff(d1) : 8u;
        } else {
            while (cnt < 8u && o + cnt < lim && W.msg[sp + o + cnt] == W.byte(qo + (int)cnt)) cnt++;
        }
        const uint64_t part = wave_ballot(cnt < 8u);
        if (!part) {
            L += 512u;
            continue;
        }
        const int fl = __builtin_ctzll(part);
        L += 8u * (uint32_t)fl + lane_val(cnt, fl);
        break;
    }
    return umin(L, lim);
}

__global__ void __launch_bounds__(64) lz4_hc_cdict_opt_parse_kernel(HcDictOptArgs o) {
    const HcDictArgs &a = o.a;
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b], cap = a.dst_cap[b];
    Window W;
    const bool ok = open_object(a, &W, b);
    if (!ok || n < 0 || n > a.max_src || cap <= 0) {
        if (lane == 0) a.result[b] = ok && n > a.max_src ? kErange : 0;
        return;
    }
    gcu8 *src = W.msg;
    gu8 *dst = (gu8 *)a.dst[b];
    uint32_t *M = a.match + (size_t)b * a.match_stride;
    uint32_t *A = o.cost + (size_t)b * o.cost_stride;
    const uint32_t un = (uint32_t)n, ucap = (uint32_t)cap, uD = (uint32_t)W.D;
    const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;

    // ---- backward: the cost of every message position, and its choice ----
    uint32_t total = 1u + un + opt_len_bytes(un);   // one literal run
    if (n >= kMinLength) {
        uint32_t a1 = 1u, r1 = 0u;   // cost[p + 1] (cost[n] = 1: the final run's token), and the
                                     // literals that lead it
        // the capped match last extended past the cap: its offset, position, end and cost[end]
        uint32_t run_off = 0u, run_p = 0u, run_end = 0u, run_a = 0u;
        // near0 lane i holds cost[hi - i] (as far as priced), near<c> lane i cost[hi + 64 c - i]
        uint32_t near1 = 0u, near2 = 0u, near3 = 0u, near4 = 0u, near5 = 0u;
        for (int hi = n - 1; hi >= 0; hi -= 64) {
            const int pos = hi - lane;
            const bool valid = pos >= 0;
            const uint32_t m = valid && (uint32_t)pos <= last ? M[pos] : 0u;
            const int cnt = min(64, hi + 1);
            uint32_t near0 = 0u, my_c = 0u;
            for (int j = 0; j < cnt; j++) {
                const uint32_t p = (uint32_t)(hi - j);
                const uint32_t mm = lane_val(m, j);
                const uint32_t L = mm >> 16, q = mm & 0xFFFFu;   // q: a window position
                const uint32_t r2 = r1 + 1u;
                // a literal: its byte, and the length byte it adds to the run it leads
                const uint32_t lit = 1u + a1 + (r2 >= 15u && (r2 - 15u) % 255u == 0u ? 1u : 0u);
                uint32_t choice = 0u, cost = lit;
                if (L >= (uint32_t)kMinMatch) {
                    const uint32_t lim = end - p;
                    uint32_t E = L, far = 0u;
                    if (L == (uint32_t)kHcCap && lim > (uint32_t)kHcCap) {
                        // capped by the search: the full length, from the run this match
                        // continues (whichever side its source lies on) or by extension
                        const uint32_t off = uD + p - q;
                        if (off == run_off && run_p <= p + L) {
                            E = run_end - p;
                            far = run_a;
                            run_p = p;
                        } else {
                            E = extend(W, p, q, L, lim, lane);
                            run_off = 0u;   // (an extension that ends at the cap starts no run)
                            if (E > (uint32_t)kHcCap) {
                                own_stores_visible();
                                far = __hip_atomic_load(A + p + E, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
                                run_off = off;
                                run_p = p;
                                run_end = p + E;
                                run_a = far;
                            }
                        }
                    }
                    // lengths 4 .. L: the least cost, then the longest (the key and its
                    // reduction are lz4_hc_opt_parse_kernel's)
                    const uint32_t uj = (uint32_t)j;
                    auto cand = [&](uint32_t c, uint32_t base) {
                        const uint32_t l = base - (uint32_t)lane;   // (wraps for an unpriced lane)
                        const uint32_t inv = 0xFFFFF800u - ((c + (l >= 19u ? 1u : 0u)) << 9) + l;
                        return l - (uint32_t)kMinMatch <= L - (uint32_t)kMinMatch ? inv : 0u;
                    };
                    uint32_t best = cand(near0, uj);
                    if (uj + 1u <= L) {
                        best = umax(best, cand(near1, uj + 64u));
                        if (uj + 65u <= L) {
                            best = umax(best, cand(near2, uj + 128u));
                            if (uj + 129u <= L) {
                                best = umax(best, cand(near3, uj + 192u));
                                if (uj + 193u <= L) {
                                    best = umax(best, cand(near4, uj + 256u));
                                    if (uj + 257u <= L) best = umax(best, cand(near5, uj + 320u));
                                }
                            }
                        }
                    }
                    const uint32_t key = ~lane_val(wave_incl_max(best), 63);
                    uint32_t mc = key >> 9, ml = 511u - (key & 511u);
                    if (E > (uint32_t)kHcCap) {   // the one far candidate
                        const uint32_t fc = 3u + opt_len_bytes(E - (uint32_t)kMinMatch) + far;
                        if (fc <= mc) {
                            mc = fc;
                            ml = E;
                        }
                    }
                    if (mc <= lit) {   // a tie goes to the match
                        choice = ml;
                        cost = mc;
                    }
                }
                a1 = cost;
                r1 = choice ? 0u : r2;
                if (lane == j) {
                    near0 = cost;
                    my_c = choice ? choice << 16 | q : 0u;
                }
            }
            if (valid) {
                A[pos] = near0;
                if ((uint32_t)pos <= last) M[pos] = my_c;
            }
            near5 = near4;
            near4 = near3;
            near3 = near2;
            near2 = near1;
            near1 = near0;
        }
        total = a1;
        own_stores_visible();
    }

    // ---- forward: the sequences, if the block fits ----
    auto put = [&](uint32_t at, uint32_t v) {   // one output byte
        if (lane == 0) dst[at] = (uint8_t)v;
    };
    auto put_len = [&](uint32_t at, uint32_t v, uint32_t nb) {   // a length field's nb bytes
        for (uint32_t j = (uint32_t)lane; j < nb; j += 64u)
            dst[at + j] = (uint8_t)(j + 1u == nb ? (v - 15u) % 255u : 255u);
    };
    auto copy = [&](uint32_t at, uint32_t s, uint32_t len) {     // literals
        for (uint32_t j = 16u * (uint32_t)lane; j + 16u <= len; j += 1024u)
            gstore16(dst + at + j, gload16(src + s + j));
        const uint32_t r = len & ~15u;
        if ((uint32_t)lane < len - r) dst[at + r + lane] = src[s + r + lane];
    };

    const bool fit = total <= ucap;   // decided before anything is written
    uint32_t op = 0u, anchor = 0u;
    bool fail = !fit;
    if (fit && n >= kMinLength) {
        uint32_t p = 0u;
        while (p <= last) {
            // 64 positions from p: the first one with a choice (below 4: none, so p advances)
            const uint32_t pos = p + (uint32_t)lane;
            const uint32_t c = pos <= last ? M[pos] : 0u;
            const uint64_t has = wave_ballot((c >> 16) >= (uint32_t)kMinMatch);
            if (!has) {
                p += 64u;
                continue;
            }
            const int fl = __builtin_ctzll(has);
            const uint32_t sp = p + (uint32_t)fl, mm = lane_val(c, fl);
            const uint32_t q = mm & 0xFFFFu, L = umin(mm >> 16, end - sp);
            const uint32_t lits = sp - anchor, ml = L - (uint32_t)kMinMatch, off = uD + sp - q;
            const uint32_t nlb = opt_len_bytes(lits), nmb = opt_len_bytes(ml);
            if (op + 1u + nlb + lits + 2u + nmb > ucap) {   // (the sequences sum to cost[0])
                fail = true;
                break;
            }
            put(op, umin(lits, 15u) << 4 | umin(ml, 15u));
            op += 1u;
            put_len(op, lits, nlb);
            op += nlb;
            copy(op, anchor, lits);
            op += lits;
            put(op, off & 255u);
            put(op + 1u, off >> 8);
            op += 2u;
            put_len(op, ml, nmb);
            op += nmb;
            p = sp + L;
            anchor = p;
        }
    }
    int result = 0;
    if (!fail) {
        const uint32_t run = un - anchor, nlb = opt_len_bytes(run);
        if (op + 1u + nlb + run <= ucap) {
            put(op, umin(run, 15u) << 4);
            op += 1u;
            put_len(op, run, nlb);
            op += nlb;
            copy(op, anchor, run);
            result = (int)(op + run);
        }
    }
    if (lane == 0) a.result[b] = result;
}

}  // namespace

hipError_t launch_hc_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                   hipStream_t s) {
    hipLaunchKernelGGL(lz4_hc_cdict_prepare_kernel, dim3(1), dim3(kPrepThreads), 0, s, dict,
                       dict_size, max_src, (uint8_t *)cdict);
    return hipGetLastError();
}

hipError_t launch_encode_hc_cdict(const HcDictArgs &a, hipStream_t s) {
    if (a.nblocks <= 0) return hipSuccess;
    const int groups = hc_cdict_groups(a.max_src);
    hipLaunchKernelGGL(lz4_hc_cdict_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    hipLaunchKernelGGL(lz4_hc_cdict_search_kernel, dim3((unsigned)a.nblocks * groups),
                       dim3(kHcdThreads), 0, s, a, groups);
    hipLaunchKernelGGL(lz4_hc_cdict_parse_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_encode_hc_cdict_opt(const HcDictOptArgs &o, hipStream_t s) {
    const HcDictArgs &a = o.a;
    if (a.nblocks <= 0) return hipSuccess;
    const int groups = hc_cdict_groups(a.max_src);
    hipLaunchKernelGGL(lz4_hc_cdict_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    hipLaunchKernelGGL(lz4_hc_cdict_search_kernel, dim3((unsigned)a.nblocks * groups),
                       dim3(kHcdThreads), 0, s, a, groups);
    hipLaunchKernelGGL(lz4_hc_cdict_opt_parse_kernel, dim3(a.nblocks), dim3(64), 0, s, o);
    return hipGetLastError();
}

}  // namespace apelz4
