// lz4_large.hip -- inputs larger than the 64 KiB encoder block, compressed on the GPU as ONE
// LZ4 block (APE_LZ4_compress_large_batch_dev, include/ape_lz4_gpu.h).
//
// A sender always has the plaintext before a slice, so all slices of a large input are
// encoded in parallel by the regular encoder (lz4_encode.hip, the withPrefix form: slice k at
// k * S with the bytes before it as history).  Each slice's output is a sequence stream that
// ends in a literal-only sequence; the block is those streams STITCHED: the final literal
// run of slice k-1 (t bytes) and the leading literals of slice k (l bytes) become one
// sequence of t + l literals with slice k's match.  A slice without a match ("no body")
// only lengthens the run carried into the next slice; the block ends with one final run.
//
// Four stream-ordered launches (the kernel boundaries are the only synchronisation):
//   1. large_plan_kernel     one thread per slice slot: the encoder's argument arrays
//   2. lz4_encode_kernel     unchanged; BlockArgs::tail reports each slice's final run
//   3. large_offsets_kernel  one wave per input: a scan over its slices (carried across
//                            trips of 64) gives every piece's output offset and the total
//   4. large_stitch_kernel   one workgroup per slice: merged token + length bytes, the
//                            slice's own literals from the source, the rest of its
//                            sequences from scratch
// With restart points (LargeArgs::restart = R > 0) the plan gives a slice only the history back
// to the last multiple of R, so no match of [j R, (j + 1) R) reaches before j R; a fifth launch,
// large_index_kernel, then writes each input's seek index from what the offsets kernel left
// (APE_LZ4_compress_large_indexed_batch_dev; the decoder of such blocks is in lz4_decode.hip).
// Work per stitch workgroup is O(S): a slice copies its OWN trailing literals to their place
// in the run they belong to (the run's position comes from the next slice with a body), so
// an incompressible input of any size never gathers onto one workgroup.
#include "lz4_gpu_internal.h"

#ifndef APE_LZ4_LARGE_SLICE
#define APE_LZ4_LARGE_SLICE 32768   // S: chosen by measurement, DESIGN.md "Large inputs"
#endif

namespace apelz4 {

static_assert(APE_LZ4_LARGE_SLICE % 64 == 0 && APE_LZ4_LARGE_SLICE >= 64 &&
              APE_LZ4_LARGE_SLICE <= kMaxBlock - 64, "slice size: a multiple of 64, <= 65536 - 64");

namespace {

constexpr uint32_t kS = APE_LZ4_LARGE_SLICE;
constexpr uint32_t kNoBodyEnc = 0x7FFFFFFFu;   // next-body scan: index j travels as this - j

__device__ __forceinline__ uint32_t ext_len(uint32_t L) { return L >= 15u ? (L - 15u) / 255u + 1u : 0u; }

__global__ void __launch_bounds__(256)
large_plan_kernel(LargeArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nslots) return;
    const int i = (int)(t / a.nsl);
    const uint32_t k = (uint32_t)(t % a.nsl);
    const int n = a.src_size[i];
    const char *src = a.src[i];
    char *dst = a.buf + (size_t)t * a.stride;
    // absent slot (past the input's end, or an input outside the limits): size -1 ends the
    // encoder's workgroup before it touches anything (result 0)
    int size = -1, prefix = 0, cap = 0;
    if (n >= 0 && n <= a.max_src) {
        if (n <= kMaxBlock) {
            if (k == 0) {   // one slice, encoded straight into the caller's buffer: no stitch
                size = n;
                dst = a.dst[i];
                cap = a.dst_cap[i];
            }
        } else if ((uint64_t)k * kS < (uint32_t)n) {
            const uint32_t start = k * kS;
            src += start;
            size = (int)umin(kS, (uint32_t)n - start);
            // history back to the last restart point at or before the slice (a slice AT one
            // is encoded with none: no match of its group reaches before the group's start)
            prefix = (int)(a.restart > 0 ? start % (uint32_t)a.restart : start);
            cap = (int)a.stride;   // >= compressBound(S): every slice fits
        }
    }
    a.s_src[t] = src;
    a.s_dst[t] = dst;
    a.s_size[t] = size;
    a.s_prefix[t] = prefix;
    a.s_cap[t] = cap;
}

// Literal length of the first sequence of a slice's stream (token + length bytes), read 16
// bytes at a time; `r` = the stream's size (the slot has 16 bytes of slack after it).
__device__ __forceinline__ uint32_t lead_literals(gcu8 *p, uint32_t r) {
    uint32_t l = (uint32_t)p[0] >> 4;
    if (l < 15u) return l;
    for (uint32_t pos = 1; pos < r; pos += 16) {
        const uint4 v = gload16(p + pos);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint32_t b = (w[q >> 2] >> (8 * (q & 3))) & 255u;
            l += b;
            if (b != 255u) return l;
        }
    }
    return l;
}

// One wave per input.  Slice j = [j S, j S + len_j) ends in tail_j literals; it has a body
// when tail_j < len_j.  A_j = end of the last match before slice j (the running maximum of
// j' S + len_j' - tail_j' over earlier slices with a body, 0 without one), carry c_j =
// j S - A_j.  The piece of a slice with a body is its stream with the first sequence's
// literal length raised by c_j and the final run cut off; a slice without one has no piece.
__global__ void __launch_bounds__(64)
large_offsets_kernel(LargeArgs a) {
    const int i = blockIdx.x;
    const int lane = lane_id();
    const int n = a.src_size[i];
    const size_t t0 = (size_t)i * a.nsl;
    if (n < 0 || n > a.max_src) {
        if (lane == 0) a.result[i] = n < 0 ? 0 : kErange;
        return;
    }
    if (n <= kMaxBlock) {   // encoded in place by its one slice
        if (lane == 0) a.result[i] = a.s_res[t0];
        return;
    }
    const uint32_t un = (uint32_t)n;
    const uint32_t K = (un + kS - 1u) / kS;
    uint32_t *runR = a.run_pos + (size_t)i * (a.nsl + 1), *runA = a.run_anchor + (size_t)i * (a.nsl + 1);
    uint32_t cA = 0, cO = 0;
    for (uint32_t base = 0; base < K; base += 64) {
        const uint32_t j = base + (uint32_t)lane;
        const bool live = j < K;
        const size_t t = t0 + j;
        const uint32_t start = live ? j * kS : 0u;
        const uint32_t len = live ? umin(kS, un - start) : 0u;
        const uint32_t r = live ? (uint32_t)a.s_res[t] : 0u;
        const uint32_t tl = live ? umin((uint32_t)a.s_tail[t], len) : 0u;
        const bool body = tl < len;
        const uint32_t inclA = wave_incl_max(body ? start + len - tl : 0u);
        const uint32_t A = umax(cA, wave_shr1(inclA, 0u));
        const uint32_t c = start - A;
        uint32_t l = 0, P = 0;
        if (body) {
            l = lead_literals((gcu8 *)(a.buf + t * a.stride), r);
            const uint32_t seqs = r - (1u + ext_len(tl) + tl);   // the stream less its final run
            P = 1u + ext_len(c + l) + c + l + (seqs - (1u + ext_len(l) + l));
        }
        const uint32_t inclP = wave_incl_sum(P);
        const uint32_t O = cO + wave_shr1(inclP, 0u);
        if (live) {
            a.s_off[t] = O;
            a.s_carry[t] = c;
            a.s_lead[t] = l;
        }
        if (body) {   // where the literals of this piece's run start, and the input position
            runR[j] = O + 1u + ext_len(c + l);
            runA[j] = A;
        }
        cA = umax(cA, lane_val(inclA, 63));
        cO += lane_val(inclP, 63);
    }
    const uint32_t fin = un - cA, fhdr = 1u + ext_len(fin);
    const uint32_t total = cO + fhdr + fin;   // < 2^31: <= compressBound(n), n <= 0x7E000000
    if (lane == 0) {
        runR[K] = cO + fhdr;
        runA[K] = cA;
        const int cap = a.dst_cap[i];
        a.result[i] = (cap > 0 && total <= (uint32_t)cap) ? (int)total : 0;
    }
    // next slice with a body after each slice (K = the final run), scanned from the end
    uint32_t ce = kNoBodyEnc - K;
    for (uint32_t hi = K; hi > 0; hi = hi > 64u ? hi - 64u : 0u) {
        const bool live = (uint32_t)lane < hi;
        const uint32_t j = live ? hi - 1u - (uint32_t)lane : 0u;
        const size_t t = t0 + j;
        const uint32_t len = umin(kS, un - j * kS);
        const bool body = live && (uint32_t)a.s_tail[t] < len;
        const uint32_t incl = wave_incl_max(body ? kNoBodyEnc - j : 0u);
        const uint32_t e = umax(ce, wave_shr1(incl, 0u));
        if (live) a.s_next[t] = kNoBodyEnc - e;
        ce = umax(ce, lane_val(incl, 63));
    }
}

// The seek index of every input (a.index != nullptr), one wave per input, after the offsets
// kernel.  Group j = the slices of [j R, (j + 1) R).  Entry j is the token position and the
// run anchor of the first slice at or after slice j R / S that has a body (its piece starts
// with the sequence whose literals begin at the anchor, and the anchor is at or before the
// group's start: no earlier slice of the group has a match); without such a slice it is the
// final run's.  A group without any body therefore becomes an empty segment.
__global__ void __launch_bounds__(64)
large_index_kernel(LargeArgs a) {
    const int i = blockIdx.x;
    const int lane = lane_id();
    uint32_t *w = (uint32_t *)(a.index + (size_t)i * a.index_stride);
    const int n = a.src_size[i], r = a.result[i];
    const bool one = n <= kMaxBlock || a.restart <= 0 || n <= a.restart;
    if (r <= 0 || one) {   // no block: nseg = 0; one segment: the whole block
        if (lane == 0) {
            w[0] = kIxMagic;
            w[1] = r > 0 ? 1u : 0u;
            w[2] = r > 0 ? (uint32_t)n : 0u;
            w[3] = r > 0 ? (uint32_t)r : 0u;
            if (r > 0) {
                w[4] = 0u;
                w[5] = 0u;
                w[6] = (uint32_t)r;
                w[7] = (uint32_t)n;
            }
        }
        return;
    }
    const uint32_t un = (uint32_t)n, R = (uint32_t)a.restart;
    const uint32_t K = (un + kS - 1u) / kS, nseg = (un + R - 1u) / R, per = R / kS;
    const size_t t0 = (size_t)i * a.nsl;
    const uint32_t *runR = a.run_pos + (size_t)i * (a.nsl + 1), *runA = a.run_anchor + (size_t)i * (a.nsl + 1);
    const uint32_t fin = un - runA[K], ftok = runR[K] - (1u + ext_len(fin));   // the final run's token
    if (lane == 0) {
        w[0] = kIxMagic;
        w[1] = nseg;
        w[2] = un;
        w[3] = (uint32_t)r;
        w[4 + 2 * nseg] = (uint32_t)r;
        w[5 + 2 * nseg] = un;
    }
    for (uint32_t j = (uint32_t)lane; j < nseg; j += 64u) {
        const uint32_t g = j * per;   // < K
        const uint32_t len = umin(kS, un - g * kS);
        const uint32_t m = (uint32_t)a.s_tail[t0 + g] < len ? g : a.s_next[t0 + g];
        w[4 + 2 * j] = m < K ? a.s_off[t0 + m] : ftok;
        w[5 + 2 * j] = runA[m];
    }
}

// workgroup-wide copy of len bytes: 16-byte stores on dst's alignment, unaligned 16-byte
// loads (all inside [s, s + len)), single bytes at the two ends
__device__ __forceinline__ void block_copy(gu8 *d, gcu8 *s, uint32_t len, uint32_t tid, uint32_t nt) {
    const uint32_t head = umin(len, (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u);
    const uint32_t nvec = (len - head) / 16u;
    for (uint32_t v = tid; v < nvec; v += nt) gstore16(d + head + 16u * v, gload16(s + head + 16u * v));
    for (uint32_t b = tid; b < head; b += nt) d[b] = s[b];
    for (uint32_t b = head + 16u * nvec + tid; b < len; b += nt) d[b] = s[b];
}

// token (literal length L, match nibble ml) and L's length bytes at p
__device__ __forceinline__ void put_header(gu8 *p, uint32_t L, uint32_t ml, uint32_t tid, uint32_t nt) {
    if (tid == 0) p[0] = (uint8_t)(((L < 15u ? L : 15u) << 4) | ml);
    if (L < 15u) return;
    const uint32_t ne = ext_len(L);   // ne - 1 bytes of 255, then the remainder
    if (tid == 0) p[ne] = (uint8_t)((L - 15u) % 255u);
    gu8 *f = p + 1;
    const uint32_t nf = ne - 1u;
    const uint32_t head = umin(nf, (16u - (uint32_t)((uintptr_t)f & 15u)) & 15u);
    const uint32_t nvec = (nf - head) / 16u;
    for (uint32_t v = tid; v < nvec; v += nt)
        gstore16(f + head + 16u * v, make_uint4(~0u, ~0u, ~0u, ~0u));
    for (uint32_t b = tid; b < head; b += nt) f[b] = 255;
    for (uint32_t b = head + 16u * nvec + tid; b < nf; b += nt) f[b] = 255;
}

__global__ void __launch_bounds__(256)
large_stitch_kernel(LargeArgs a) {
    const size_t t = blockIdx.x;
    const int i = (int)(t / a.nsl);
    const uint32_t k = (uint32_t)(t % a.nsl);
    const uint32_t tid = threadIdx.x;
    const int n = a.src_size[i];
    if (n <= kMaxBlock || n > a.max_src) return;
    const uint32_t un = (uint32_t)n;
    const uint32_t K = (un + kS - 1u) / kS;
    if (k >= K || a.result[i] <= 0) return;   // (a block that did not fit writes nothing)
    const uint32_t start = k * kS, len = umin(kS, un - start);
    const uint32_t r = (uint32_t)a.s_res[t], tl = umin((uint32_t)a.s_tail[t], len);
    gcu8 *in = (gcu8 *)a.src[i];
    gu8 *out = (gu8 *)a.dst[i];
    gcu8 *buf = (gcu8 *)(a.buf + t * a.stride);
    const uint32_t *runR = a.run_pos + (size_t)i * (a.nsl + 1), *runA = a.run_anchor + (size_t)i * (a.nsl + 1);
    if (tl < len) {   // the piece: merged header, own leading literals, the other sequences
        const uint32_t O = a.s_off[t], c = a.s_carry[t], l = a.s_lead[t];
        const uint32_t L = c + l, hdr = 1u + ext_len(L), h = 1u + ext_len(l);
        const uint32_t seqs = r - (1u + ext_len(tl) + tl);
        put_header(out + O, L, (uint32_t)buf[0] & 15u, tid, 256);
        block_copy(out + O + hdr + c, in + start, l, tid, 256);
        block_copy(out + O + hdr + L, buf + h + l, seqs - h - l, tid, 256);
    }
    {   // own trailing literals, into the run of the next slice with a body (or the final run)
        const uint32_t m = a.s_next[t], ts = start + len - tl;
        block_copy(out + runR[m] + (ts - runA[m]), in + ts, tl, tid, 256);
    }
    if (k == K - 1u) {
        const uint32_t fin = un - runA[K], fhdr = 1u + ext_len(fin);
        put_header(out + runR[K] - fhdr, fin, 0u, tid, 256);
    }
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

int large_slice_size() { return (int)kS; }

// slots per input: one when every input fits the encoder's block
static long long large_nsl(int max_src) {
    return max_src <= kMaxBlock ? 1 : ((long long)max_src + kS - 1) / kS;
}

// Layout: [src, dst pointers][9 int arrays per slot][2 run arrays of nsl + 1 per input][slot
// buffers of `stride` bytes]; every region 16-aligned.  Returns 0 for 2^24 slots or
// more (the caller splits the batch).
size_t large_scratch_layout(int nblocks, int max_src, LargeArgs *out) {
    const long long nsl = large_nsl(max_src);
    const long long nslots = (long long)nblocks * nsl;
    if (nslots >= (1 << 24)) return 0;   // (grid x 256 threads stays below 2^32)
    const size_t ns = (size_t)nslots, nrun = (size_t)nblocks * (size_t)(nsl + 1);
    // a slice's stream (<= compressBound(S)) + 16 bytes of slack for lead_literals' loads
    const size_t stride = max_src <= kMaxBlock ? 0 : up16((size_t)kS + kS / 255 + 16) + 16;
    size_t pos = 0;
    const size_t o_src = pos; pos += up16(ns * sizeof(void *));
    const size_t o_dst = pos; pos += up16(ns * sizeof(void *));
    size_t o_int[9];
    for (int q = 0; q < 9; q++) { o_int[q] = pos; pos += up16(ns * sizeof(int)); }
    const size_t o_rp = pos; pos += up16(nrun * sizeof(uint32_t));
    const size_t o_ra = pos; pos += up16(nrun * sizeof(uint32_t));
    const size_t o_buf = pos; pos += ns * stride;
    if (out) {
        char *b = out->buf;   // (the scratch base on entry)
        out->nsl = (int)nsl;
        out->nslots = (int)nslots;
        out->stride = stride;
        out->s_src = (const char **)(b + o_src);
        out->s_dst = (char **)(b + o_dst);
        out->s_size = (int *)(b + o_int[0]);
        out->s_prefix = (int *)(b + o_int[1]);
        out->s_cap = (int *)(b + o_int[2]);
        out->s_res = (int *)(b + o_int[3]);
        out->s_tail = (int *)(b + o_int[4]);
        out->s_off = (uint32_t *)(b + o_int[5]);
        out->s_carry = (uint32_t *)(b + o_int[6]);
        out->s_lead = (uint32_t *)(b + o_int[7]);
        out->s_next = (uint32_t *)(b + o_int[8]);
        out->run_pos = (uint32_t *)(b + o_rp);
        out->run_anchor = (uint32_t *)(b + o_ra);
        out->buf = b + o_buf;
    }
    return pos > 16 ? pos : 16;
}

// ev (nullable): five events recorded before, between and after the four launches
hipError_t launch_large(const LargeArgs &a, int accel, hipStream_t s, hipEvent_t *ev) {
    if (a.nblocks <= 0) return hipSuccess;
    auto mark = [&](int q) { return ev ? hipEventRecord(ev[q], s) : hipSuccess; };
    hipError_t e = mark(0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(large_plan_kernel, dim3((unsigned)((a.nslots + 255) / 256)), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = mark(1);
    if (e != hipSuccess) return e;
    BlockArgs b{};
    b.src = a.s_src;
    b.dst = a.s_dst;
    b.src_size = a.s_size;
    b.dict_size = a.s_prefix;
    b.dst_cap = a.s_cap;
    b.result = a.s_res;
    b.tail = a.s_tail;
    b.accel = accel;
    b.nblocks = a.nslots;
    e = launch_encode(b, s);
    if (e == hipSuccess) e = mark(2);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(large_offsets_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = mark(3);
    if (e != hipSuccess) return e;
    if (a.max_src > kMaxBlock) {   // (otherwise every input is one slice: nothing to stitch)
        hipLaunchKernelGGL(large_stitch_kernel, dim3(a.nslots), dim3(256), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mark(4);
    if (e == hipSuccess && a.index) {
        hipLaunchKernelGGL(large_index_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        e = hipGetLastError();
    }
    return e;
}

// The high-ratio encoder on the slices.  Plan, offsets, stitch and index are
// the launches above, unchanged: they need a slice's stream, its size and the length of its
// final run, whichever encoder wrote them.  The plan's s_prefix is the history OFFERED (back to
// the input's start or the last restart point); the high-ratio kernels use min(that, 65536 -
// size) of it.  An absent slot has size -1: its parse wave writes result 0 and reads nothing.
// opt picks the slices' parse: the lazy one, or the cost-minimising one, whose
// cost tables follow the match tables at `hc`.
hipError_t launch_large_hc(const LargeArgs &a, int depth, void *hc, int pass, hipStream_t s,
                           hipEvent_t *ev, bool opt) {
    if (a.nblocks <= 0) return hipSuccess;
    int q = 0;
    auto mark = [&]() { return ev ? hipEventRecord(ev[q++], s) : hipSuccess; };
    hipError_t e = mark();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(large_plan_kernel, dim3((unsigned)((a.nslots + 255) / 256)), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = mark();
    for (int off = 0; off < a.nslots && e == hipSuccess; off += pass) {
        HcArgs h{};
        h.src = a.s_src + off;
        h.src_size = a.s_size + off;
        h.dst = a.s_dst + off;
        h.dst_cap = a.s_cap + off;
        h.result = a.s_res + off;
        h.prefix = a.s_prefix + off;
        h.tail = a.s_tail + off;
        h.nblocks = a.nslots - off < pass ? a.nslots - off : pass;
        h.depth = depth;
        h.chain = (uint16_t *)hc;
        h.match = (uint32_t *)((char *)hc + (size_t)pass * kHcChainBytes);
        if (opt) {
            HcOptArgs o{};
            o.a = h;
            o.cost = (uint32_t *)((char *)hc + (size_t)pass * kHcSlotBytes);
            e = launch_encode_hc_opt(o, s, ev ? ev + q : nullptr);
        } else {
            e = launch_encode_hc(h, s, ev ? ev + q : nullptr);
        }
        if (ev) q += 3;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(large_offsets_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = mark();
    if (e != hipSuccess) return e;
    if (a.max_src > kMaxBlock) {   // (otherwise every input is one slice: nothing to stitch)
        hipLaunchKernelGGL(large_stitch_kernel, dim3(a.nslots), dim3(256), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mark();
    if (e == hipSuccess && a.index) {
        hipLaunchKernelGGL(large_index_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mark();
    return e;
}

}  // namespace apelz4
