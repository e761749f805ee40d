// lz4_encode_hc_opt.hip -- the high-ratio encoder's cost-minimising parse
// (APE_LZ4_compress_hc_opt_batch_dev).
//
// Three launches per pass over caller-owned scratch (lz4_gpu_internal.h, HcOptArgs): the chain
// build and the search of lz4_encode_hc.hip exactly as they are, then
//   price + emit  one wave per block, two passes over match[] in ONE kernel:
//     backward  p = W - 1 .. h: cost[p] = the bytes window[p:] takes -- a literal, or a match of
//               any length l from 4 to the match's full length E (every offset costs two bytes,
//               so the longest match of a position prices all its prefixes); the least cost
//               wins, a tie goes to the match and to the longer l.  match[p] becomes
//               chosen length << 16 | source.
//     forward   the walk over the choices, sequences written with the whole wave.
// The output is a pure function of (input bytes, used history, depth): tests/hcoptmodel.py is its
// definition.  The parse is cost-minimising, not optimal: a literal's length byte is priced
// against the run of the chosen continuation only.  cost[h] is the block's size, so a block that
// does not fit its capacity writes nothing.  Every load of the input stays inside the window
// [src - h, src + n) and every store inside dst[0, cap).
//
// The near costs cost[p + 4 .. p + 272] stay in registers (six per lane, the last 384 positions
// priced); all of cost[] is in scratch for the one far candidate cost[p + E] of a match longer
// than the search's cap.  Along a run of such matches at one offset (zeros, periodic data, a
// repeated half) p + E is constant: E and the far cost are carried in registers, so a run costs
// one extension and one far load.  The wave reads back what its own lanes stored earlier in the
// kernel (the far cost, and match[] in the forward pass): each such read follows an agent-scope
// release, a drained store counter and an acquire.  Both loops run at most n steps; none waits
// on data.
#include "lz4_gpu_internal.h"

namespace apelz4 {

// lz4_encode_hc.hip's kernels, launched from here as they are
__global__ void lz4_hc_chain_kernel(HcArgs a);
__global__ void lz4_hc_search_kernel(HcArgs a);

namespace {

constexpr int kSearchThreads = 256;                      // lz4_hc_search_kernel's workgroup ...
constexpr int kSearchGroups = kMaxBlock / kSearchThreads;   // ... and its workgroups per block
static_assert(kHcCap <= 5 * 64 && kHcCap < 511, "near costs: five registers behind the current "
                                                "64 positions, lengths in 9 bits");

// bytes of history block b uses (lz4_encode_hc.hip's rule)
__device__ __forceinline__ int opt_history(const HcArgs &a, int b, int n) {
    return a.prefix ? max(0, min(a.prefix[b], kMaxBlock - n)) : 0;
}

// what this wave's lanes stored to global memory so far is what any of its lanes loads from here on
__device__ __forceinline__ void own_stores_visible() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// the common prefix of src[sp..] and src[q..] from L on, at most lim: 8 bytes per lane, 512 a step
__device__ __forceinline__ uint32_t extend(gcu8 *src, uint32_t sp, uint32_t q, uint32_t L,
                                           uint32_t lim, int lane) {
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
    return umin(L, lim);
}

}  // namespace

// ---- price + emit ----
__global__ void __launch_bounds__(64) lz4_hc_opt_parse_kernel(HcOptArgs o) {
    const HcArgs &a = o.a;
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
    const int hist = opt_history(a, b, n);
    gcu8 *src = (gcu8 *)a.src[b] - hist;
    gu8 *dst = (gu8 *)a.dst[b];
    uint32_t *M = a.match + (size_t)b * kMaxBlock;
    uint32_t *A = o.cost + (size_t)b * kMaxBlock;
    const uint32_t un = (uint32_t)(hist + n), ucap = (uint32_t)cap;
    const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;

    // ---- backward: the cost of every position, and its choice ----
    uint32_t total = 1u + (uint32_t)n + len_bytes((uint32_t)n);   // one literal run
    if (n >= kMinLength) {
        uint32_t a1 = 1u, r1 = 0u;   // cost[p + 1] (cost[W] = 1: the final run's token), and
                                     // the literals that lead it
        // the capped match last extended past the cap: its offset, position, end and cost[end]
        uint32_t run_off = 0u, run_p = 0u, run_end = 0u, run_a = 0u;
        // The near costs, in registers: positions are priced 64 at a time down from hi, lane j
        // the j-th, so near0 lane i holds cost[hi - i] (as far as priced) and near<c> lane i
        // cost[hi + 64 c - i]: the candidate of length l = j + 64 c - i for position hi - j.
        uint32_t near1 = 0u, near2 = 0u, near3 = 0u, near4 = 0u, near5 = 0u;
        for (int hi = (int)un - 1; hi >= hist; hi -= 64) {
            const int pos = hi - lane;
            const bool valid = pos >= hist;
            const uint32_t m = valid && (uint32_t)pos <= last ? M[pos] : 0u;
            const int cnt = min(64, hi - hist + 1);
            uint32_t near0 = 0u, my_c = 0u;
            for (int j = 0; j < cnt; j++) {
                const uint32_t p = (uint32_t)(hi - j);
                const uint32_t mm = lane_val(m, j);
                const uint32_t L = mm >> 16, q = mm & 0xFFFFu;
                const uint32_t r2 = r1 + 1u;
                // a literal: its byte, and the length byte it adds to the run it leads
                const uint32_t lit = 1u + a1 + (r2 >= 15u && (r2 - 15u) % 255u == 0u ? 1u : 0u);
                uint32_t choice = 0u, cost = lit;
                if (L >= (uint32_t)kMinMatch) {
                    const uint32_t lim = end - p;
                    uint32_t E = L, far = 0u;
                    if (L == (uint32_t)kHcCap && lim > (uint32_t)kHcCap) {
                        // capped by the search: the full length, from the run this match
                        // continues or by extension
                        const uint32_t off = p - q;
                        if (off == run_off && run_p <= p + L) {
                            E = run_end - p;
                            far = run_a;
                            run_p = p;
                        } else {
                            E = extend(src, p, q, L, lim, lane);
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
                    // lengths 4 .. L: the least cost, then the longest.  The key is cost << 9 |
                    // (511 - l); a lane holds ~key, or 0 without a candidate, and the maximum
                    // finds the least key.  A register whose lengths all exceed L is skipped.
                    const uint32_t uj = (uint32_t)j;
                    auto cand = [&](uint32_t a, uint32_t base) {
                        const uint32_t l = base - (uint32_t)lane;   // (wraps for an unpriced lane)
                        const uint32_t inv = 0xFFFFF800u - ((a + (l >= 19u ? 1u : 0u)) << 9) + l;
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
                        const uint32_t fc = 3u + len_bytes(E - (uint32_t)kMinMatch) + far;
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

    const bool fit = total <= ucap;   // decided before anything is written
    uint32_t op = 0u, anchor = (uint32_t)hist;
    bool fail = false;
    if (n >= kMinLength) {
        uint32_t p = (uint32_t)hist;
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
            const uint32_t lits = sp - anchor, ml = L - (uint32_t)kMinMatch, off = sp - q;
            if (fit) {
                const uint32_t nlb = len_bytes(lits), nmb = len_bytes(ml);
                if (op + 1u + nlb + lits + 2u + nmb > ucap) {   // (the sequences sum to cost[h])
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
            }
            p = sp + L;
            anchor = p;
        }
    }
    int result = 0;
    if (fit && !fail) {
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
        // as lz4_hc_parse_kernel: the final run of a finished walk, also when it did not fit
        if (a.tail) a.tail[b] = fail ? 0 : (int)(un - anchor);
    }
}

// ev (nullable): three events, recorded after the chain, the search and the parse launch
hipError_t launch_encode_hc_opt(const HcOptArgs &o, hipStream_t s, hipEvent_t *ev) {
    const HcArgs &a = o.a;
    if (a.nblocks <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(lz4_hc_chain_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    if (ev) e = hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(lz4_hc_search_kernel, dim3((unsigned)a.nblocks * kSearchGroups),
                       dim3(kSearchThreads), 0, s, a);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(lz4_hc_opt_parse_kernel, dim3(a.nblocks), dim3(64), 0, s, o);
    if (ev && e == hipSuccess) e = hipEventRecord(ev[2], s);
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : e;
}

}  // namespace apelz4
