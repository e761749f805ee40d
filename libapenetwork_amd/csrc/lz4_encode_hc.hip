// lz4_encode_hc.hip -- the high-ratio encoder (APE_LZ4_compress_hc_batch_dev).
//
// Three launches per pass over caller-owned scratch (lz4_gpu_internal.h, HcArgs):
//   chain   one wave per block: chain[p] = the nearest earlier position with the hash of the 4
//           bytes at p, through a u16 head table in LDS, 64 positions per step;
//   search  one lane per position p <= n - 12: the first `depth` members of p's chain, the
//           strictly longest common prefix (>= 4, capped at min(kHcCap, n - 5 - p)) -> match[p];
//   parse   one wave per block: the sequential walk over match[] with the one-step lazy rule,
//           capped matches extended forward, sequences written with the whole wave.
// The output is a pure function of (input bytes, depth): tests/hcmodel.py is its definition,
// and the rules below are that model's, line for line.  Every load of the input stays inside
// src[0, n) and every store inside dst[0, cap).
//
// With history (HcArgs::prefix; tests/hclargemodel.py is the definition) the
// three kernels work on the WINDOW [src - h, src + n), h = min(prefix, 65536 - n) bytes of
// history and the block: chain[] and match[] are indexed by window position (h + n <= 65536,
// so position + 1 stays inside u16), the chains run over the whole window, and only the block's
// positions h .. h + n - 12 are searched and parsed.  Every load stays inside the window.
#include "lz4_gpu_internal.h"

namespace apelz4 {
namespace {

constexpr int kHcSearchThreads = 256;
constexpr int kHcGroups = kMaxBlock / kHcSearchThreads;   // search workgroups per block

// bytes of history block b (of 0 <= n <= kMaxBlock bytes) uses: what the caller offers, as far
// as one window of u16 positions holds it; not rounded, a negative prefix counts as none
__device__ __forceinline__ int hc_history(const HcArgs &a, int b, int n) {
    return a.prefix ? max(0, min(a.prefix[b], kMaxBlock - n)) : 0;
}

}  // namespace

// ---- chain build ----
__global__ void __launch_bounds__(64) lz4_hc_chain_kernel(HcArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t head[kHcTable];   // position + 1, 0 = empty
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b];
    if (n < kMinLength || n > kMaxBlock) return;   // no position can match: nothing is read
    const int hist = hc_history(a, b, n);
    gcu8 *src = (gcu8 *)a.src[b] - hist;           // the window's base
    uint16_t *chain = a.chain + (size_t)b * kMaxBlock;
    for (int i = lane; i < kHcTable / 8; i += 64) ((uint4 *)head)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    volatile uint16_t *vhead = head;
    const uint64_t below = (1ull << lane) - 1ull;
    const int last = hist + n - kMinMatch;
    for (int base = 0; base <= last; base += 64) {
        const int p = base + lane;
        const bool valid = p <= last;
        // (a lane past the end gets a hash no other lane has)
        const uint32_t h = valid ? hc_hash(gload4(src + p)) : (uint32_t)(kHcTable + lane);
        const uint32_t me = (uint32_t)p + 1u;
        const uint32_t prev = valid ? vhead[h] : 0u;
        // Lanes with equal hashes: each needs the highest lower lane of its group, and the
        // group's highest lane owns the table entry.  Every lane stores; a lane that reads
        // another's value back is in a group of two or more, and only such groups are walked
        // (an all-zero block is one group per step, distinct hashes are none).
        if (valid) vhead[h] = (uint16_t)me;
        __syncthreads();
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
        __syncthreads();
        if (owner) vhead[h] = (uint16_t)me;
        if (valid) chain[p] = (uint16_t)(pred >= 0 ? (uint32_t)(base + pred) + 1u : prev);
        __syncthreads();
    }
}

// ---- search ----
__global__ void __launch_bounds__(kHcSearchThreads) lz4_hc_search_kernel(HcArgs a) {
    const int b = blockIdx.x / kHcGroups;
    const int n = a.src_size[b];
    if (n < kMinLength || n > kMaxBlock) return;
    // window positions: the block's own start at hist, the window ends at wn (a workgroup past
    // the block's last searchable position leaves here)
    const int hist = hc_history(a, b, n), wn = hist + n;
    const int p = hist + (int)(blockIdx.x % kHcGroups) * kHcSearchThreads + (int)threadIdx.x;
    if (p > wn - kMFLimit) return;
    gcu8 *src = (gcu8 *)a.src[b] - hist;
    const uint16_t *chain = a.chain + (size_t)b * kMaxBlock;
    const int mx = min(kHcCap, wn - kLastLiterals - p);   // >= 7
    const uint32_t x = gload4(src + p);
    uint32_t cur = chain[p], best = 0u, best_q = 0u;
    for (int d = 0; d < a.depth && cur; d++) {
        const int q = (int)cur - 1;
        cur = chain[q];
        if (gload4(src + q) != x) continue;   // a collision, or fewer than 4 bytes: depth spent
        int k = kMinMatch;
        while (k < mx) {
            if (p + k + 16 <= wn) {           // q < p: both loads end inside the window
                const uint4 u = gload16(src + p + k), v = gload16(src + q + k);
                const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y, d2 = u.z ^ v.z, d3 = u.w ^ v.w;
                if (d0 | d1 | d2 | d3) {
                    k += d0 ? first_diff(d0) : d1 ? 4 + first_diff(d1) : d2 ? 8 + first_diff(d2)
                                                                            : 12 + first_diff(d3);
                    break;
                }
                k += 16;
            } else {                          // the window's last bytes, one at a time
                while (k < mx && src[p + k] == src[q + k]) k++;
                break;
            }
        }
        const uint32_t L = (uint32_t)min(k, mx);
        if (L > best) {                       // strictly longer: a tie stays with the nearer
            best = L;
            best_q = (uint32_t)q;
        }
        if (L == (uint32_t)mx) break;
    }
    a.match[(size_t)b * kMaxBlock + p] = best << 16 | best_q;
}

// ---- parse + emit ----
__global__ void __launch_bounds__(64) lz4_hc_parse_kernel(HcArgs a) {
    const int b = blockIdx.x, lane = lane_id();
    const int n = a.src_size[b], cap = a.dst_cap[b];
    if (n < 0 || n > kMaxBlock || cap <= 0) {   // (a slot of size -1 reads nothing more)
        if (lane == 0) {
            a.result[b] = n > kMaxBlock ? kErange : 0;
            if (a.tail && n >= 0) a.tail[b] = 0;
        }
        return;
    }
    // src, un and every position below are the window's: the block starts at hist
    const int hist = hc_history(a, b, n);
    gcu8 *src = (gcu8 *)a.src[b] - hist;
    gu8 *dst = (gu8 *)a.dst[b];
    const uint32_t *M = a.match + (size_t)b * kMaxBlock;
    const uint32_t un = (uint32_t)(hist + n), ucap = (uint32_t)cap;

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

    uint32_t op = 0u, anchor = (uint32_t)hist;
    bool fail = false;
    if (n >= kMinLength) {
        const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;
        uint32_t p = (uint32_t)hist;
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
            // the lazy step: from the first match on, the first position whose successor's
            // match is not longer (the rule has no memory, so a run that leaves the window
            // resumes at its last lane)
            const int first = __builtin_ctzll(has);
            const uint64_t stop = wave_ballot(lane >= first && !(next_len > len));
            if (!stop) {
                p += 63u;
                continue;
            }
            const int sl = __builtin_ctzll(stop);
            const uint32_t sp = p + (uint32_t)sl, mm = lane_val(m, sl);
            const uint32_t q = mm & 0xFFFFu, lim = end - sp;
            uint32_t L = mm >> 16;
            if (L == umin((uint32_t)kHcCap, lim)) {
                // capped by the search: extend forward to at most the end - 5, 8 bytes per lane
                while (L < lim) {
                    const uint32_t o = L + 8u * (uint32_t)lane;
                    uint32_t cnt = 0u;
                    if (o + 8u <= lim) {
                        const uint2 u = gload8(src + sp + o), v = gload8(src + q + o);
                        const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y;
                        cnt = d0 ? first_diff(d0) : d1 ? 4u + first_diff(d1) : 8u;
                    } else {
                        while (o + cnt < lim && src[sp + o + cnt] == src[q + o + cnt]) cnt++;
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
            const uint32_t lits = sp - anchor, ml = L - (uint32_t)kMinMatch, off = sp - q;
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
    if (lane == 0) {
        a.result[b] = result;
        // the large path (lz4_large.hip) stitches slices at their final literal runs: the run
        // of a finished walk, also when it did not fit; 0 when the walk broke off
        if (a.tail) a.tail[b] = fail ? 0 : (int)(un - anchor);
    }
}

// ev (nullable): three events, recorded after the chain, the search and the parse launch
hipError_t launch_encode_hc(const HcArgs &a, hipStream_t s, hipEvent_t *ev) {
    if (a.nblocks <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(lz4_hc_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    if (ev) e = hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(lz4_hc_search_kernel, dim3((unsigned)a.nblocks * kHcGroups),
                       dim3(kHcSearchThreads), 0, s, a);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(lz4_hc_parse_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[2], s);
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : e;
}

}  // namespace apelz4
