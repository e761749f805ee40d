// lz4_hc_common.h -- the high-ratio mode's stages, written once over a window view
// (DESIGN.md 3.18).  lz4_encode_hc.hip instantiates them for the contiguous window
// [history | block] (FlatView, below), lz4_hc_cdict.hip for the split window [prepared dictionary
// | message] (its SplitView); its prepare kernel builds the dictionary's chains over a FlatView.
//
//   chain   one wave: chain[w] = the nearest earlier window position with the hash of the 4 bytes
//           at w, through a u16 head table in LDS, 64 positions per step;
//   search  one lane per block position i <= n - 12: the first `depth` members of its chain, the
//           strictly longest common prefix (>= 4, capped at min(kHcCap, n - 5 - i));
//   lazy    one wave: the sequential walk over match[] with the one-step lazy rule, capped
//           matches extended forward, sequences written with the whole wave;
//   opt     one wave, two passes over match[]: backward, cost[i] = the bytes block[i:] takes -- a
//           literal, or a match of any length l from 4 to the match's full length E (every offset
//           costs two bytes, so the longest match of a position prices all its prefixes); the
//           least cost wins, a tie goes to the match and to the longer l; match[i] becomes chosen
//           length << 16 | source.  Forward, the walk over the choices.  Cost-minimising, not
//           optimal: a literal's length byte is priced against the run of the chosen
//           continuation only.  cost[0] is the block's size, so a block that does not fit its
//           capacity writes nothing.
// The output is a pure function of (window bytes, depth): tests/hcmodel.py, hclargemodel.py and
// hcoptmodel.py define it, and hcdictmodel.py / hcoptdictmodel.py call those on the split window.
//
// A view V names window positions w in [0, origin + n), the block being [origin, origin + n):
//   byte(w), at(w), load4(w)   the byte, its address, the 4 bytes at w <= origin + n - 4
//   one_side(w, len)           [w, w + len) can be read through at(w) in one load
//   block()                    the block's first byte; origin: its window position
//   next(w), set_next(w, v)    chain[w]
// The rules run in block positions: position i is window position origin + i, match[] and cost[]
// arrive as pointers to the block's first entry, literals are read from block(), a match's source
// q stays a window position (the offset is origin + i - q), and only the match comparison and the
// extension go through the view.
//
// Bounds.  Every load through block() stays inside block[0, n).  Every load through the view
// stays inside the window -- for the split view inside the message or the object with its pads:
// a wide load at a source position is taken only where one_side() holds and the block's own load
// of the same width ends inside the block (the source lies below it), everything else goes byte
// by byte; the split view's load4 at D - 3 .. D - 1 runs into the object's back pad and masks,
// a path the contiguous view does not have.  Every store of the emitter stays inside dst[0, cap):
// a sequence is written only after all of it was found to fit.  Both passes of a parse run at
// most n steps; no loop waits on data.
#pragma once
#include "lz4_gpu_internal.h"

namespace apelz4 {

static_assert(kHcCap <= 5 * 64 && kHcCap < 511, "near costs: five registers behind the current "
                                                "64 positions, lengths in 9 bits");

// The contiguous window: position w is base[w], one chain table indexed by window position.
struct FlatView {
    gcu8 *base;
    int origin;
    uint16_t *chain;
    __device__ __forceinline__ uint32_t byte(int w) const { return base[w]; }
    __device__ __forceinline__ gcu8 *at(int w) const { return base + w; }
    __device__ __forceinline__ uint32_t load4(int w) const { return gload4(base + w); }
    __device__ static constexpr bool one_side(int, int) { return true; }
    __device__ __forceinline__ gcu8 *block() const { return base + origin; }
    __device__ __forceinline__ uint32_t next(int w) const { return chain[w]; }
    __device__ __forceinline__ void set_next(int w, uint32_t v) const { chain[w] = (uint16_t)v; }
};

// One wave's LDS stores, made visible to its own later loads (a chain build runs on a single
// wave, so no workgroup barrier is needed -- and the prepare kernel's other waves must not
// meet one).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// what this wave's lanes stored to global memory so far is what any of its lanes loads from here on
__device__ __forceinline__ void own_stores_visible() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// ---- chain build ----
// One step: 64 positions base + lane with hashes h (an invalid lane brings a hash no other lane
// has) enter the head table (position + 1, 0 = empty); returns chain[base + lane].
__device__ __forceinline__ uint32_t chain_step(volatile uint16_t *vhead, int base, int lane,
                                               bool valid, uint32_t h) {
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t me = (uint32_t)(base + lane) + 1u;
    const uint32_t prev = valid ? vhead[h] : 0u;
    // Lanes with equal hashes: each needs the highest lower lane of its group, and the group's
    // highest lane owns the table entry.  Every lane stores; a lane that reads another's value
    // back is in a group of two or more, and only such groups are walked (an all-zero block is
    // one group per step, distinct hashes are none).
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

// window positions first .. last enter the head table in order (chain[] is not read here)
template <class V>
__device__ __forceinline__ void hc_chain_build(const V &W, uint16_t *head, int first, int last,
                                               int lane) {
    for (int base = first; base <= last; base += 64) {
        const int p = base + lane;
        const bool valid = p <= last;
        const uint32_t h = valid ? hc_hash(W.load4(p)) : (uint32_t)(kHcTable + lane);
        const uint32_t c = chain_step(head, base, lane, valid, h);
        if (valid) W.set_next(p, c);
    }
}

// ---- search ----
// match[i] of block position i <= n - 12 (n >= 13): length << 16 | source, 0 = none
template <class V>
__device__ __forceinline__ uint32_t hc_search(const V &W, int n, int i, int depth) {
    gcu8 *blk = W.block();
    const int mx = min(kHcCap, n - kLastLiterals - i);   // >= 7
    const uint32_t x = gload4(blk + i);
    uint32_t cur = W.next(W.origin + i), best = 0u, best_q = 0u;
    for (int d = 0; d < depth && cur; d++) {
        const int q = (int)cur - 1;
        cur = W.next(q);
        if (W.load4(q) != x) continue;        // a collision, or fewer than 4 bytes: depth spent
        int k = kMinMatch;
        while (k < mx) {
            if (i + k + 16 <= n && W.one_side(q + k, 16)) {
                const uint4 u = gload16(blk + i + k), v = gload16(W.at(q + k));
                const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y, d2 = u.z ^ v.z, d3 = u.w ^ v.w;
                if (d0 | d1 | d2 | d3) {
                    k += d0 ? first_diff(d0) : d1 ? 4 + first_diff(d1) : d2 ? 8 + first_diff(d2)
                                                                            : 12 + first_diff(d3);
                    break;
                }
                k += 16;
            } else {                          // across a boundary and at the block's end
                if (W.byte(q + k) != blk[i + k]) break;
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
    return best << 16 | best_q;
}

// the common prefix of the block from sp on and the window from q on, from L on and at most lim
// (sp + lim <= n - 5): 8 bytes per lane and 512 a step where the source's 8 can be loaded at
// once, byte by byte across a boundary and at the end
template <class V>
__device__ __forceinline__ uint32_t hc_extend(const V &W, uint32_t sp, uint32_t q, uint32_t L,
                                              uint32_t lim, int lane) {
    gcu8 *blk = W.block();
    while (L < lim) {
        const uint32_t o = L + 8u * (uint32_t)lane;
        const int qo = (int)(q + o);
        uint32_t cnt = 0u;
        if (o + 8u <= lim && W.one_side(qo, 8)) {
            const uint2 u = gload8(blk + sp + o), v = gload8(W.at(qo));
            const uint32_t d0 = u.x ^ v.x, d1 = u.y ^ v.y;
            cnt = d0 ? first_diff(d0) : d1 ? 4u + first_diff(d1) : 8u;
        } else {
            while (cnt < 8u && o + cnt < lim && blk[sp + o + cnt] == W.byte(qo + (int)cnt)) cnt++;
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

// ---- the sequence emitter: one wave writes dst[0, cap) from the block's bytes ----
struct Emitter {
    gu8 *dst;
    gcu8 *blk;
    uint32_t cap, op;
    int lane;
    __device__ __forceinline__ void put(uint32_t o, uint32_t v) const {   // one output byte
        if (lane == 0) dst[o] = (uint8_t)v;
    }
    // a length field's nb bytes
    __device__ __forceinline__ void put_len(uint32_t o, uint32_t v, uint32_t nb) const {
        for (uint32_t j = (uint32_t)lane; j < nb; j += 64u)
            dst[o + j] = (uint8_t)(j + 1u == nb ? (v - 15u) % 255u : 255u);
    }
    __device__ __forceinline__ void copy(uint32_t o, uint32_t s, uint32_t len) const {   // literals
        for (uint32_t j = 16u * (uint32_t)lane; j + 16u <= len; j += 1024u)
            gstore16(dst + o + j, gload16(blk + s + j));
        const uint32_t r = len & ~15u;
        if ((uint32_t)lane < len - r) dst[o + r + lane] = blk[s + r + lane];
    }
    // the literals blk[anchor, sp) and a match of L bytes at offset off, if all of it fits
    __device__ __forceinline__ bool sequence(uint32_t anchor, uint32_t sp, uint32_t L, uint32_t off) {
        const uint32_t lits = sp - anchor, ml = L - (uint32_t)kMinMatch;
        const uint32_t nlb = len_bytes(lits), nmb = len_bytes(ml);
        if (op + 1u + nlb + lits + 2u + nmb > cap) return false;
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
        return true;
    }
    // the final run blk[anchor, n): the block's size, 0 when the run does not fit
    __device__ __forceinline__ int final_run(uint32_t anchor, uint32_t n) {
        const uint32_t run = n - anchor, nlb = len_bytes(run);
        if (op + 1u + nlb + run > cap) return 0;
        put(op, umin(run, 15u) << 4);
        op += 1u;
        put_len(op, run, nlb);
        op += nlb;
        copy(op, anchor, run);
        return (int)(op + run);
    }
};

// ---- the lazy parse ----
// Returns the block's size (0: it does not fit).  *tail: the final literal run of a finished
// walk, also when that run did not fit; 0 when the walk broke off.
// (A sequence that does not fit leaves the loop through `fail`, not by a return from inside it:
// with the return the contiguous kernel measured 2 % slower, profiles/hc_unify_parent_ab.txt.)
template <class V>
__device__ __forceinline__ int hc_lazy_parse(const V &W, int n, const uint32_t *M, Emitter &em,
                                             uint32_t *tail) {
    const int lane = em.lane;
    const uint32_t un = (uint32_t)n;
    bool fail = false;
    uint32_t anchor = 0u;
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
            // the lazy step: from the first match on, the first position whose successor's
            // match is not longer (the rule has no memory, so a run that leaves the 64
            // positions resumes at its last lane)
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
            // capped by the search: extend forward to at most the end - 5
            if (L == umin((uint32_t)kHcCap, lim)) L = hc_extend(W, sp, q, L, lim, lane);
            if (!em.sequence(anchor, sp, L, (uint32_t)W.origin + sp - q)) {
                fail = true;
                break;
            }
            p = sp + L;
            anchor = p;
        }
    }
    *tail = fail ? 0u : un - anchor;
    return fail ? 0 : em.final_run(anchor, un);
}

// ---- the cost-minimising parse ----
// Backward: cost[] and the choices of block positions n - 1 .. 0; returns cost[0], the block's
// size.
//
// The near costs cost[p + 4 .. p + 272] stay in registers (six per lane, the last 384 positions
// priced); all of cost[] is in scratch for the one far candidate cost[p + E] of a match longer
// than the search's cap.  Along a run of such matches at one offset (zeros, periodic data, a
// repeated half) p + E is constant: E and the far cost are carried in registers, so a run costs
// one extension and one far load.  The wave reads back what its own lanes stored earlier in the
// kernel (the far cost, and match[] in the forward pass): each such read follows
// own_stores_visible().
template <class V>
__device__ __forceinline__ uint32_t hc_price(const V &W, int n, uint32_t *M, uint32_t *A, int lane) {
    const uint32_t un = (uint32_t)n, origin = (uint32_t)W.origin;
    if (n < kMinLength) return 1u + un + len_bytes(un);   // one literal run
    const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;
    uint32_t a1 = 1u, r1 = 0u;   // cost[p + 1] (cost[n] = 1: the final run's token), and the
                                 // literals that lead it
    // the capped match last extended past the cap: its offset, position, end and cost[end]
    uint32_t run_off = 0u, run_p = 0u, run_end = 0u, run_a = 0u;
    // Positions are priced 64 at a time down from hi, lane j the j-th, so near0 lane i holds
    // cost[hi - i] (as far as priced) and near<c> lane i cost[hi + 64 c - i]: the candidate of
    // length l = j + 64 c - i for position hi - j.
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
                    // capped by the search: the full length, from the run this match continues
                    // or by extension
                    const uint32_t off = origin + p - q;
                    if (off == run_off && run_p <= p + L) {
                        E = run_end - p;
                        far = run_a;
                        run_p = p;
                    } else {
                        E = hc_extend(W, p, q, L, lim, lane);
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
                // (511 - l); a lane holds ~key, or 0 without a candidate, and the maximum finds
                // the least key.  A register whose lengths all exceed L is skipped.
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
    own_stores_visible();
    return a1;
}

// Forward: the walk over the choices.  A block that does not fit (decided before anything is
// written) writes nothing; it is still walked when the caller wants its tail.  Result and *tail
// as hc_lazy_parse's.
__device__ __forceinline__ int hc_forward(int n, uint32_t origin, const uint32_t *M, Emitter &em,
                                          bool fit, bool want_tail, uint32_t *tail) {
    const int lane = em.lane;
    const uint32_t un = (uint32_t)n;
    uint32_t anchor = 0u;
    if (n >= kMinLength && (fit || want_tail)) {
        const uint32_t last = un - (uint32_t)kMFLimit, end = un - (uint32_t)kLastLiterals;
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
            // (the sequences sum to cost[0], so one that does not fit is not met)
            if (fit && !em.sequence(anchor, sp, L, origin + sp - q)) {
                *tail = 0u;
                return 0;
            }
            p = sp + L;
            anchor = p;
        }
    }
    *tail = un - anchor;
    return fit ? em.final_run(anchor, un) : 0;
}

template <class V>
__device__ __forceinline__ int hc_opt_parse(const V &W, int n, uint32_t *M, uint32_t *A, Emitter &em,
                                            bool want_tail, uint32_t *tail) {
    const uint32_t total = hc_price(W, n, M, A, em.lane);
    return hc_forward(n, (uint32_t)W.origin, M, em, total <= em.cap, want_tail, tail);
}

}  // namespace apelz4
