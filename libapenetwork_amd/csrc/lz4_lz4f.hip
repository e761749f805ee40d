// lz4_lz4f.hip -- the LZ4 frame format (include/ape_lz4f.h): xxHash32 over a
// batch of streams, framed compress and framed decode.  The block codecs are the existing
// launchers (launch_encode, launch_decode, launch_decode_chain); this file plans their
// pointer arrays in the caller's scratch, hashes, and packs or judges the frames.
// tests/lz4fmodel.py is the definition of the frame bytes and of the decoder's codes.
// The placed decode (include/ape_lz4f_placed.h; tests/lz4fplacedmodel.py) sizes
// every block with launch_decode_size before it places and decodes them.  Frames with a dictionary
// (include/ape_lz4f_dict.h; tests/lz4fdictmodel.py) are the same kernels with a
// dictionary stage: an ID field in header and info, one block per frame against a prepared
// dictionary on the compress side, a table lookup in the decode plan.  The call with preferences
// (include/ape_lz4f_prefs.h; tests/lz4fprefsmodel.py) is the compress side with the
// block size as a field, the large-input launchers as its block encoders, and a pack that cuts a
// block into pieces.
#include "lz4_gpu_internal.h"

namespace apelz4 {

namespace {

// ---- xxHash32 ----
constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u,
                   kP5 = 374761393u;

__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return __builtin_rotateleft32(x, r); }
__device__ __forceinline__ uint32_t xxh_round(uint32_t acc, uint32_t x) {
    return rotl(acc + x * kP2, 13) * kP1;
}
__device__ __forceinline__ uint32_t xxh_word(uint32_t h, uint32_t x) { return rotl(h + x * kP3, 17) * kP4; }
__device__ __forceinline__ uint32_t xxh_byte(uint32_t h, uint32_t x) { return rotl(h + x * kP5, 11) * kP1; }
__device__ __forceinline__ uint32_t xxh_avalanche(uint32_t h) {
    h ^= h >> 15;
    h *= kP2;
    h ^= h >> 13;
    h *= kP3;
    return h ^ (h >> 16);
}

// XXH32 of fewer than 16 bytes held by the calling lane (a frame descriptor)
__device__ __forceinline__ uint32_t xxh32_short(const uint8_t *b, uint32_t n, uint32_t seed) {
    uint32_t h = seed + kP5 + n, i = 0;
    for (; i + 4 <= n; i += 4)
        h = xxh_word(h, (uint32_t)b[i] | (uint32_t)b[i + 1] << 8 | (uint32_t)b[i + 2] << 16 |
                            (uint32_t)b[i + 3] << 24);
    for (; i < n; i++) h = xxh_byte(h, b[i]);
    return xxh_avalanche(h);
}

// One stream of a hash launch: n bytes at p, the hash to *out; a null out is no stream.
struct XStream {
    gcu8 *p;
    uint32_t n;
    uint32_t *out;
};

// A wave hashes kXhStreams streams at once: lane 4 s + a owns accumulator a of the wave's
// stream s.  The four accumulators of a stream are independent chains of n / 16 steps each
// (acc = rotl(acc + x * P2, 13) * P1 on every fourth word), so the 64 lanes run 64 chains.  The
// bytes come in 1 KiB per stream and round: all 64 lanes load 16 bytes of stream t (one
// coalesced global_load_dwordx4 per stream, any alignment), park them in LDS, and each lane
// then reads its accumulator's word of each 16-byte stripe back (ds_read_b32).  The row pitch
// of 1040 bytes puts the 32 lanes of a read group on 32 banks: (260 s + 4 k + a) mod 32 =
// 4 s + a + 4 k.  The loads of round r + 1 are issued before the steps of round r and wait in
// registers.  Only whole stripes inside [p, p + n) are loaded; the lane with a = 0 merges the
// accumulators and takes the last n mod 16 bytes by 4-byte and 1-byte loads.
constexpr int kXhStreams = 16;
constexpr int kXhRound = 1024;            // bytes per stream and round: 64 stripes
constexpr int kXhPitch = kXhRound + 16;
constexpr int kXhLds = kXhStreams * kXhPitch;

// (stream_of, by this file's convention: one XStream that starts as "no stream" and is filled in
// on the way to a single return, so that every path that skips a stream leaves `out` null.)
template <class F>
__device__ __forceinline__ void xxh32_group(uint8_t *lds, F stream_of, uint32_t first,
                                            uint32_t nstreams, uint32_t seed) {
    const int lane = lane_id();
    const uint32_t s = (uint32_t)lane >> 2, a = (uint32_t)lane & 3u;
    const uint32_t i = first + s;
    XStream st{nullptr, 0u, nullptr};
    if (i < nstreams) st = stream_of(i);
    if (!st.out) st.n = 0u;
    const uint32_t stripes = st.n >> 4;
    const uint32_t most = lane_val(wave_incl_max(stripes), 63);
    const uint32_t rounds = (most + 63u) >> 6;
    const uint32_t plo = (uint32_t)(uint64_t)st.p, phi = (uint32_t)((uint64_t)st.p >> 32);

    uint4 pre[kXhStreams];
#pragma unroll
    for (int t = 0; t < kXhStreams; t++) pre[t] = make_uint4(0u, 0u, 0u, 0u);
    auto fetch = [&](uint32_t r) {
#pragma unroll
        for (int t = 0; t < kXhStreams; t++) {
            gcu8 *base = (gcu8 *)((uint64_t)lane_val(phi, 4 * t) << 32 | lane_val(plo, 4 * t));
            const uint32_t k = r * 64u + (uint32_t)lane;
            if (k < lane_val(stripes, 4 * t)) pre[t] = gload16(base + (size_t)k * 16u);
        }
    };

    uint32_t acc = a == 0u ? seed + kP1 + kP2 : a == 1u ? seed + kP2 : a == 2u ? seed : seed - kP1;
    if (rounds) fetch(0u);
    for (uint32_t r = 0; r < rounds; r++) {
#pragma unroll
        for (int t = 0; t < kXhStreams; t++)
            if (r * 64u + (uint32_t)lane < lane_val(stripes, 4 * t))
                *(uint4 *)(lds + t * kXhPitch + lane * 16) = pre[t];
        __syncthreads();
        if (r + 1u < rounds) fetch(r + 1u);
        const uint32_t done = r * 64u;
        const uint32_t mine = stripes > done ? umin(stripes - done, 64u) : 0u;
        const uint32_t top = umin(most - done, 64u);
        const uint8_t *row = lds + s * kXhPitch + a * 4u;
#pragma unroll 8
        for (uint32_t k = 0; k < top; k++) {
            const uint32_t x = *(const uint32_t *)(row + k * 16u);
            if (k < mine) acc = xxh_round(acc, x);
        }
        __syncthreads();
    }

    const int q = lane & ~3;
    const uint32_t v1 = (uint32_t)__shfl((int)acc, q), v2 = (uint32_t)__shfl((int)acc, q + 1),
                   v3 = (uint32_t)__shfl((int)acc, q + 2), v4 = (uint32_t)__shfl((int)acc, q + 3);
    if (a == 0u && st.out) {
        uint32_t h = st.n >= 16u ? rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18)
                                 : seed + kP5;
        h += st.n;
        gcu8 *p = st.p + (size_t)(st.n & ~15u);
        uint32_t rem = st.n & 15u;
        for (; rem >= 4u; rem -= 4u, p += 4) h = xxh_word(h, gload4(p));
        for (; rem; rem--, p++) h = xxh_byte(h, *p);
        *st.out = xxh_avalanche(h);
    }
}

__global__ void __launch_bounds__(64)
xxh32_batch_kernel(const char *const *src, const int *size, uint32_t seed, uint32_t *hash, int n) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXhLds];
    xxh32_group(lds, [&](uint32_t i) {
        const int sz = size[i];
        return XStream{(gcu8 *)src[i], sz > 0 ? (uint32_t)sz : 0u, hash + i};
    }, blockIdx.x * (uint32_t)kXhStreams, (uint32_t)n, seed);
}

// ---- helpers of both directions ----
constexpr uint32_t kLfMagic = 0x184D2204u, kLfSkipMagic = 0x184D2A50u, kLfLegacyMagic = 0x184C2102u;
constexpr uint32_t kFlgLinkedOff = 0x20u, kFlgBlockSum = 0x10u, kFlgSize = 0x08u,
                   kFlgContentSum = 0x04u, kFlgReserved = 0x02u, kFlgDictId = 0x01u;

// n bytes from s to d, any alignment of either, by the calling wave
__device__ __forceinline__ void wave_copy(gu8 *d, gcu8 *s, uint32_t n) {
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t i = lane * 16u; i + 16u <= n; i += 1024u) gstore16(d + i, gload16(s + i));
    const uint32_t base = n & ~15u;
    if (lane < (n & 15u)) d[base + lane] = s[base + lane];
}

__device__ __forceinline__ void put_le32(gu8 *d, uint32_t v) {
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
    d[2] = (uint8_t)(v >> 16);
    d[3] = (uint8_t)(v >> 24);
}

// ---- compress ----
// the block size is 2^blog bytes: block-size ID 4..7 = 64 KiB .. 4 MiB
__device__ __forceinline__ uint32_t lfc_blog(const LfCompress &c) { return 8u + 2u * (uint32_t)c.bsid; }
__device__ __forceinline__ uint32_t lfc_blocks(int n, uint32_t blog) {
    return (uint32_t)(((uint64_t)(uint32_t)n + ((1u << blog) - 1u)) >> blog);
}
__device__ __forceinline__ uint32_t lfc_header_bytes(int flags) { return (flags & 4) ? 15u : 7u; }

// one lane per slot (frame f, block q at f * bpf + q): the encoder's arguments; a slot
// without a block gets size -1, which the encoder answers with 0 before it reads anything (the
// large-input launchers, whose "inputs" the slots are above ID 4, do the same)
__global__ void __launch_bounds__(256)
lz4f_compress_plan_kernel(LfCompress c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)c.nslots) return;
    const uint32_t f = i / (uint32_t)c.bpf, q = i % (uint32_t)c.bpf;
    const int n = c.src_size[f];
    const uint32_t blog = lfc_blog(c);
    const bool real = n > 0 && n <= c.max_src && ((uint64_t)q << blog) < (uint64_t)n;
    const int bsz = real ? (int)umin((uint32_t)n - (q << blog), 1u << blog) : -1;
    c.s_src[i] = real ? c.src[f] + ((size_t)q << blog) : c.buf;
    c.s_dst[i] = c.buf + ((size_t)i << blog);
    c.s_size[i] = bsz;
    c.s_cap[i] = real ? bsz - 1 : 0;
}

// The dictionary call (include/ape_lz4f_dict.h): one lane per frame, which is one
// slot.  The encoders read the object's header before the size, so a frame without a block
// (size -1) costs a header read and gets 0.
__global__ void __launch_bounds__(256)
lz4f_dict_compress_plan_kernel(LfCompress c) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= (uint32_t)c.nframes) return;
    const int n = c.src_size[f];
    const bool real = n > 0 && n <= c.max_src;
    c.s_src[f] = real ? c.src[f] : c.buf;
    c.s_dst[f] = c.buf + (size_t)f * (size_t)c.slot;
    c.s_size[f] = real ? n : -1;
    c.s_cap[f] = real ? n - 1 : 0;
}

// the frame's dictionary ID, 0 = no field (kDict: the dictionary call)
template <bool kDict>
__device__ __forceinline__ uint32_t lfc_dict_id(const LfCompress &c, uint32_t f) {
    if constexpr (kDict) return c.dict_id ? c.dict_id[f] : 0u;
    return 0u;
}

// one wave per frame: where every block goes, what the frame takes, whether it fits.  kDict: a
// message above its object's maxSrcSize, which only the encoder can know, is its ERANGE.
template <bool kDict>
__global__ void __launch_bounds__(64)
lz4f_compress_layout_kernel(LfCompress c) {
    const uint32_t f = blockIdx.x, lane = (uint32_t)lane_id();
    const int n = c.src_size[f], cap = c.dst_cap[f];
    bool over = n > c.max_src;
    if constexpr (kDict) over = over || (n > 0 && c.s_res[f] == kErange);
    if (n < 0 || over) {
        if (lane == 0) {
            c.f_total[f] = 0;
            c.result[f] = n < 0 ? 0 : kErange;
        }
        return;
    }
    const uint32_t nb = lfc_blocks(n, lfc_blog(c)), per = 4u + ((c.flags & 2) ? 4u : 0u);
    uint32_t at = lfc_header_bytes(c.flags) + (lfc_dict_id<kDict>(c, f) ? 4u : 0u);
    for (uint32_t q0 = 0; q0 < nb; q0 += 64u) {
        const uint32_t q = q0 + lane, i = f * (uint32_t)c.bpf + q;
        uint32_t bytes = 0u;
        if (q < nb) {
            const int r = c.s_res[i];
            bytes = per + (uint32_t)(r > 0 ? r : c.s_size[i]);
        }
        const uint32_t incl = wave_incl_sum(bytes);
        if (q < nb) c.s_off[i] = at + incl - bytes;
        at += lane_val(incl, 63);
    }
    const uint32_t total = at + 4u + ((c.flags & 1) ? 4u : 0u);
    if (lane == 0) {
        const bool fits = cap >= 0 && total <= (uint32_t)cap;
        c.f_total[f] = fits ? (int)total : 0;
        c.result[f] = fits ? (int)total : 0;
    }
}

__global__ void __launch_bounds__(64)
lz4f_compress_hash_kernel(LfCompress c, uint32_t first, uint32_t end) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXhLds];
    xxh32_group(lds, [&](uint32_t i) {
        const bool block = i < (uint32_t)c.nslots;
        const uint32_t f = block ? i / (uint32_t)c.bpf : i - (uint32_t)c.nslots;
        XStream st{nullptr, 0u, nullptr};
        if (c.f_total[f] <= 0) {
            // nothing of a frame that is not written is hashed
        } else if (!block) {   // a frame's input
            st.p = (gcu8 *)c.src[f];
            st.n = (uint32_t)c.src_size[f];
            st.out = c.f_hash + f;
        } else if (c.s_size[i] > 0) {   // a block, as it will sit in the frame
            const int r = c.s_res[i];
            st.p = (gcu8 *)(r > 0 ? (const char *)c.s_dst[i] : c.s_src[i]);
            st.n = (uint32_t)(r > 0 ? r : c.s_size[i]);
            st.out = c.s_hash + i;
        }
        return st;
    }, first + blockIdx.x * (uint32_t)kXhStreams, end, 0u);
}

// Pack.  One wave per (slot, piece): piece p of a slot is bytes [p, p + 1) x 64 KiB of the block as
// it sits in the frame -- the encoder's output in the slot buffer, or the source when the block
// is stored -- so a 4 MiB block is moved by 64 waves of 64 trips each, not by one wave of 4096
// dependent trips.  A piece starts at a multiple of 64 KiB of the block, so whole 16-byte
// vectors of one piece never meet another's and only the block's last piece has a scalar tail:
// every byte of the frame is written exactly once, and nothing is read outside the slot's
// result or the source block.  The wave of a block's piece 0 writes the size word and the
// checksum; that of a frame's slot 0 also the header and the trailer.  A wave whose piece starts
// at or beyond the block's bytes leaves once it has read the slot's result.  With one piece per
// slot (ID 4, and the dictionary call) this is one wave per block.
constexpr uint32_t kLfPiece = 65536u;

template <bool kDict>
__global__ void __launch_bounds__(64)
lz4f_compress_pack_kernel(LfCompress c) {
    const uint32_t i = blockIdx.x / (uint32_t)c.ppb, p = blockIdx.x % (uint32_t)c.ppb;
    const uint32_t f = i / (uint32_t)c.bpf, q = i % (uint32_t)c.bpf;
    const int total = c.f_total[f];
    if (total <= 0) return;
    gu8 *out = (gu8 *)wave_uniform(c.dst[f]);
    const uint32_t lane = (uint32_t)lane_id();
    if (q == 0u && p == 0u && lane == 0u) {
        const int n = c.src_size[f];
        const uint32_t id = lfc_dict_id<kDict>(c, f);
        uint8_t d[kDict ? 14 : 10];
        d[0] = (uint8_t)(0x40u | kFlgLinkedOff | ((c.flags & 2) ? kFlgBlockSum : 0u) |
                         ((c.flags & 4) ? kFlgSize : 0u) | ((c.flags & 1) ? kFlgContentSum : 0u) |
                         (id ? kFlgDictId : 0u));
        d[1] = (uint8_t)((uint32_t)c.bsid << 4);
        uint32_t dn = 2u;
        if (c.flags & 4) {
            for (int k = 0; k < 8; k++) d[2 + k] = k < 4 ? (uint8_t)((uint32_t)n >> (8 * k)) : 0u;
            dn = 10u;
        }
        if constexpr (kDict) {
            if (id) {
                for (int k = 0; k < 4; k++) d[dn + k] = (uint8_t)(id >> (8 * k));
                dn += 4u;
            }
        }
        put_le32(out, kLfMagic);
        for (uint32_t k = 0; k < dn; k++) out[4u + k] = d[k];
        out[4u + dn] = (uint8_t)(xxh32_short(d, dn, 0u) >> 8);
        gu8 *end = out + (uint32_t)total - ((c.flags & 1) ? 8u : 4u);
        put_le32(end, 0u);
        if (c.flags & 1) put_le32(end + 4, c.f_hash[f]);
    }
    const int bsz = c.s_size[i];
    if (bsz <= 0) return;
    const int r = c.s_res[i];
    const uint32_t bytes = (uint32_t)(r > 0 ? r : bsz), from = p * kLfPiece;
    if (from >= bytes) return;
    gu8 *at = out + c.s_off[i];
    if (p == 0u && lane == 0u) {
        put_le32(at, r > 0 ? bytes : bytes | 0x80000000u);
        if (c.flags & 2) put_le32(at + 4u + bytes, c.s_hash[i]);
    }
    gcu8 *body = (gcu8 *)wave_uniform(r > 0 ? (const char *)c.s_dst[i] : c.s_src[i]);
    wave_copy(at + 4u + from, body + from, umin(bytes - from, kLfPiece));
}

// ---- decode ----
struct LfHead {
    int code;            // 0, -1, -3, -2
    uint32_t flg, bmax, bytes;
    uint32_t cs_lo, cs_hi;   // the content size, when flg has kFlgSize
    uint32_t dict_id;        // the dictionary ID, when flg has kFlgDictId (kDictOk alone)
};

// The header of frame s[0, n), in the order of tests/lz4fmodel.py: each check on the bytes it
// needs, a truncation ending the walk.  kDictOk: the calls of include/ape_lz4f_dict.h, for which
// a dictionary ID is a field and no reason for -3.
template <bool kDictOk = false>
__device__ __forceinline__ LfHead lf_header(gcu8 *s, int n, bool no_linked) {
    LfHead h{0, 0u, 0u, 0u, 0u, 0u, 0u};
    if (n < 4) return h.code = -2, h;
    const uint32_t magic = gload4(s);
    if ((magic & 0xFFFFFFF0u) == kLfSkipMagic || magic == kLfLegacyMagic) return h.code = -3, h;
    if (magic != kLfMagic) return h.code = -1, h;
    if (n < 6) return h.code = -2, h;
    uint8_t d[14];
    d[0] = s[4];
    d[1] = s[5];
    const uint32_t flg = d[0], bd = d[1], id = (bd >> 4) & 7u;
    if ((flg >> 6) != 1u || (flg & kFlgReserved) || (bd & 0x8Fu) || id < 4u) return h.code = -1, h;
    const uint32_t dn = 2u + ((flg & kFlgSize) ? 8u : 0u) + ((flg & kFlgDictId) ? 4u : 0u);
    if ((uint32_t)n < 4u + dn + 1u) return h.code = -2, h;
    for (uint32_t k = 2; k < dn; k++) d[k] = s[4u + k];
    if (s[4u + dn] != (uint8_t)(xxh32_short(d, dn, 0u) >> 8)) return h.code = -1, h;
    h.flg = flg;
    h.bmax = 1u << (8u + 2u * id);
    h.bytes = 4u + dn + 1u;
    if (flg & kFlgSize) {
        h.cs_lo = (uint32_t)d[2] | (uint32_t)d[3] << 8 | (uint32_t)d[4] << 16 | (uint32_t)d[5] << 24;
        h.cs_hi = (uint32_t)d[6] | (uint32_t)d[7] << 8 | (uint32_t)d[8] << 16 | (uint32_t)d[9] << 24;
    }
    if constexpr (kDictOk) {
        if (flg & kFlgDictId) {
            const uint32_t k = dn - 4u;
            h.dict_id = (uint32_t)d[k] | (uint32_t)d[k + 1u] << 8 | (uint32_t)d[k + 2u] << 16 |
                        (uint32_t)d[k + 3u] << 24;
        }
    }
    if ((!kDictOk && (flg & kFlgDictId)) || (no_linked && !(flg & kFlgLinkedOff)) ||
        ((flg & kFlgSize) && (h.cs_hi || h.cs_lo >= 0x80000000u)))
        return h.code = -3, h;
    return h;
}

// The block headers from the frame header to the end mark and the trailer: 0 or -2.  put(q,
// position of the data, size word) sees every block in order.
template <class Put>
__device__ __forceinline__ int lf_walk(gcu8 *s, int n, const LfHead &h, Put put, uint32_t *nb,
                                       uint32_t *bytes) {
    const uint32_t un = (uint32_t)n, sum = (h.flg & kFlgBlockSum) ? 4u : 0u;
    uint32_t p = h.bytes, q = 0u;
    for (;; q++) {
        if (un - p < 4u) return -2;
        const uint32_t w = gload4(s + p), sz = w & 0x7FFFFFFFu;
        p += 4u;
        if (sz == 0u) break;
        if (sz > h.bmax || un - p < sz + sum) return -2;   // (p <= un, sz + sum < 2^31)
        put(q, p, w);
        p += sz + sum;
    }
    if (h.flg & kFlgContentSum) {
        if (un - p < 4u) return -2;
        p += 4u;
    }
    *nb = q;
    *bytes = p;
    return 0;
}

// header, walk, bound: the code of the header stage, and the decoded bound when it is 0
__device__ __forceinline__ int lf_bound(const LfHead &h, int walk, uint32_t nb, uint32_t *bound) {
    if (h.code) return h.code;
    if (walk) return walk;
    const uint64_t b = (h.flg & kFlgSize) ? (uint64_t)h.cs_lo : (uint64_t)nb * h.bmax;
    if (b >= 0x80000000ull) return -3;
    *bound = (uint32_t)b;
    return 0;
}

template <bool kDict>
__global__ void __launch_bounds__(64)
lz4f_info_kernel(const char *const *src, const int *src_size, int *info, int nframes) {
    const int f = (int)(blockIdx.x * 64u + threadIdx.x);
    if (f >= nframes) return;
    gcu8 *s = (gcu8 *)src[f];
    const int n = src_size[f];
    const LfHead h = lf_header<kDict>(s, n, false);
    uint32_t nb = 0u, bytes = 0u, bound = 0u;
    const int walk = h.code ? 0 : lf_walk(s, n, h, [](uint32_t, uint32_t, uint32_t) {}, &nb, &bytes);
    const int code = lf_bound(h, walk, nb, &bound);
    int *o = info + (kDict ? 10 : 8) * (size_t)f;
    const bool sized = !code && (h.flg & kFlgSize);
    o[0] = code;
    o[1] = code ? 0 : (int)h.flg;
    o[2] = code ? 0 : (int)h.bmax;
    o[3] = code ? 0 : (int)nb;
    o[4] = code ? 0 : (int)bytes;
    o[5] = code ? 0 : (int)bound;
    o[6] = sized ? (int)h.cs_lo : -1;
    o[7] = sized ? (int)h.cs_hi : -1;
    if constexpr (kDict) {
        const bool field = !code && (h.flg & kFlgDictId);
        o[8] = field ? 1 : 0;
        o[9] = field ? (int)h.dict_id : 0;
    }
}

enum : int { kLfAbsent = 0, kLfIndep = 1, kLfLinked = 2, kLfStored = 3 };

// Both framed decodes run the kernels below: kPlaced is the call of
// include/ape_lz4f_placed.h (tests/lz4fplacedmodel.py defines its codes), which
// sizes every block before it places it.

// slot i of the three decode launches: nothing to do.  The one-byte block 00 with capacity 0
// decodes to 0 (the reference's rule) and touches the scratch's first byte alone.
template <bool kPlaced>
__device__ __forceinline__ void lfd_absent(const LfDecode &d, uint32_t i) {
    d.src_a[i] = d.zero;
    d.src_b[i] = d.zero;
    d.dict[i] = d.zero;
    d.out[i] = (char *)d.zero;
    d.data[i] = d.zero;
    d.size_a[i] = 1;
    d.size_b[i] = 1;
    d.cap_a[i] = 0;
    d.cap_b[i] = 0;
    d.dict_size[i] = 0;
    d.size[i] = 0;
    d.kind[i] = kLfAbsent;
    d.cap[i] = 0;
    if constexpr (kPlaced) d.cap_s[i] = 0;
}

// What the frame says of a block, into the absent slot i: its bytes at s + p, its size word w,
// its checksum, and its kind with that kind's decoder input.  then(kind) is what the caller
// adds, called in the kind's own branch, where the kind is a constant.
template <class Then>
__device__ __forceinline__ void lfd_fill(const LfDecode &d, uint32_t i, gcu8 *s, uint32_t p,
                                         uint32_t w, uint32_t flg, Then then) {
    const uint32_t sz = w & 0x7FFFFFFFu;
    d.data[i] = (const char *)s + p;
    d.size[i] = (int)sz;
    if (flg & kFlgBlockSum) d.want[i] = gload4(s + p + sz);
    if (w >> 31) {
        d.kind[i] = kLfStored;
        then(kLfStored);
    } else if (flg & kFlgLinkedOff) {
        d.kind[i] = kLfIndep;
        d.src_a[i] = (const char *)s + p;
        d.size_a[i] = (int)sz;
        then(kLfIndep);
    } else {
        d.kind[i] = kLfLinked;
        d.src_b[i] = (const char *)s + p;
        d.size_b[i] = (int)sz;
        then(kLfLinked);
    }
}

// Slot i goes to `at` = out + pos with `room` bytes.  In two parts, so that the grid plan keeps
// the parent's order of stores (the position, the fill, then the kind's own fields in the
// kind's branch) and with it its instructions: where the block goes ...
__device__ __forceinline__ void lfd_place(const LfDecode &d, uint32_t i, char *at, int room) {
    d.out[i] = at;
    d.cap[i] = room;
}
// ... and its decoder's capacity, with the output before a linked block as its dictionary
template <class Pos>
__device__ __forceinline__ void lfd_place_kind(const LfDecode &d, uint32_t i, int kind, char *out,
                                               Pos pos, int room) {
    if (kind == kLfIndep) {
        d.cap_a[i] = room;
    } else if (kind == kLfLinked) {
        const uint32_t back = (uint32_t)(pos < 65536u ? pos : 65536u);
        d.cap_b[i] = room;
        d.dict[i] = out + pos - back;
        d.dict_size[i] = (int)back;
    }
}

// One wave per frame: lane 0 judges the header and walks the blocks, filling slot q * nframes
// + f for block q; the wave then marks the frame's other slots absent -- all of them when the
// frame has a code.  The grid call knows where block q goes, q * bmax, because every block but
// the last is full.  The placed call does not yet: a compressed block gets its sizer arguments
// instead, the block maximum as capacity and for a linked frame 65536 bytes of assumed history
// (the decoded size does not depend on the offsets; the real decode applies the true test).
// kDict (include/ape_lz4f_dict.h): between the header and the walk the whole wave
// looks the frame's key up in the caller's table -- the dictionary ID, 0 without the field --
// 64 entries per step, the first match winning.  The frame's dictionary then is the history of
// every compressed block of an independent frame and of block 0 of a linked one, for the sizer
// too (the true test, not the assumed 64 KiB).  A named ID without a usable entry is -10.
template <bool kPlaced, bool kDict>
__global__ void __launch_bounds__(64)
lz4f_decode_plan_kernel(LfDecode d) {
    const uint32_t f = blockIdx.x, lane = (uint32_t)lane_id(), nf = (uint32_t)d.nframes;
    uint32_t filled = 0u;
    LfHead hd{0, 0u, 0u, 0u, 0u, 0u, 0u};
    const char *dict = nullptr;   // the frame's dictionary, wave-uniform
    int dsize = 0;
    bool missing = false;
    if constexpr (kDict) {
        uint32_t live = 0u, key = 0u, named = 0u;
        if (lane == 0u) {
            hd = lf_header<true>((gcu8 *)d.src[f], d.src_size[f], d.no_linked);
            live = hd.code ? 0u : 1u;
            key = hd.dict_id;
            named = hd.flg & kFlgDictId;
        }
        live = wave_first(live);
        key = wave_first(key);
        named = wave_first(named);
        if (live) {
            int found = -1;
            const uint32_t nt = (uint32_t)d.ntable;
            for (uint32_t base = 0u; base < nt; base += 64u) {
                const uint32_t k = base + lane;
                const uint64_t hits = wave_ballot(k < nt && d.t_id[k] == key);
                if (hits) {
                    found = (int)(base + (uint32_t)__builtin_ctzll(hits));
                    break;
                }
            }
            if (found >= 0) {
                const int sz = d.t_size[found];
                const char *p = d.t_dict[found];
                // an unusable entry: nothing is read through it
                if (sz < 0 || (sz > 0 && !p)) missing = true;
                else if (sz > 0) dict = p, dsize = sz;
            } else {
                missing = named != 0u;
            }
        }
    }
    if (lane == 0u) {
        // the absent slots' block, 00: every frame's wave writes the same byte, and the
        // decoders that read it are later launches
        *(uint8_t *)d.zero = 0u;
        gcu8 *s = (gcu8 *)d.src[f];
        const int n = d.src_size[f], cap = kPlaced ? 0 : d.dst_cap[f];
        char *const out = kPlaced ? nullptr : d.dst[f];
        const LfHead h = kDict ? hd : lf_header(s, n, d.no_linked);
        // the dictionary as the history of a block that has nothing else before it
        auto with_dict = [&](uint32_t i, uint32_t q, int kind) {
            if constexpr (kDict) {
                if (dsize > 0 && (kind == kLfIndep || (kind == kLfLinked && q == 0u))) {
                    d.dict[i] = dict;
                    d.dict_size[i] = dsize;
                }
            }
        };
        uint32_t nb = 0u, bytes = 0u, bound = 0u;
        int walk = 0;
        if (!h.code)
            walk = lf_walk(s, n, h, [&](uint32_t q, uint32_t p, uint32_t w) {
                if (q >= (uint32_t)d.max_blocks) return;
                const uint32_t i = q * nf + f;
                if constexpr (kPlaced) {
                    lfd_absent<true>(d, i);
                    lfd_fill(d, i, s, p, w, h.flg, [&](int kind) {
                        if (kind == kLfLinked) d.dict_size[i] = 65536;
                        if (kind != kLfStored) d.cap_s[i] = (int)h.bmax;
                        with_dict(i, q, kind);
                    });
                } else {
                    const uint64_t pos = (uint64_t)q * h.bmax;
                    const int room = cap > 0 && (uint64_t)cap > pos
                                         ? (int)umin((uint32_t)((uint64_t)cap - pos), h.bmax) : 0;
                    lfd_absent<false>(d, i);
                    lfd_place(d, i, out + pos, room);
                    lfd_fill(d, i, s, p, w, h.flg,
                             [&](int kind) {
                                 lfd_place_kind(d, i, kind, out, pos, room);
                                 with_dict(i, q, kind);
                             });
                }
            }, &nb, &bytes);
        int code = lf_bound(h, walk, nb, &bound);
        if (!code && nb > (uint32_t)d.max_blocks) code = kErange;
        if (kDict && !code && missing) code = -10;
        if (!kPlaced && !code && (cap < 0 || (uint32_t)cap < bound)) code = -9;
        LfFrame &r = d.frame[f];
        r.code = code;
        r.nb = (int)nb;
        r.bmax = h.bmax;
        r.flg = h.flg;
        r.content = h.cs_lo;
        r.want = (h.flg & kFlgContentSum) && !code ? gload4(s + bytes - 4u) : 0u;
        r.got = 0u;
        if constexpr (kDict) r.dsize = dsize;
        if constexpr (kPlaced) d.total[f] = 0;
        filled = code ? 0u : nb;
    }
    filled = wave_first(filled);
    for (uint32_t q = filled + lane; q < (uint32_t)d.max_blocks; q += 64u)
        lfd_absent<kPlaced>(d, q * nf + f);
}

// the bytes block i decodes to, or -1: a stored block's size when it fits its room
__device__ __forceinline__ int lfd_block_result(const LfDecode &d, uint32_t i) {
    const int kind = d.kind[i];
    if (kind == kLfStored) return d.size[i] <= d.cap[i] ? d.size[i] : -1;
    return kind == kLfIndep ? d.res_a[i] : d.res_b[i];
}

// one wave per slot: a stored block goes to its place
__global__ void __launch_bounds__(64)
lz4f_decode_stored_kernel(LfDecode d) {
    const uint32_t i = blockIdx.x;
    if (d.kind[i] != kLfStored) return;
    const int sz = d.size[i];
    if (sz > d.cap[i]) return;
    wave_copy((gu8 *)wave_uniform(d.out[i]), (gcu8 *)wave_uniform(d.data[i]), (uint32_t)sz);
}

template <bool kPlaced>
__global__ void __launch_bounds__(64)
lz4f_decode_hash_kernel(LfDecode d) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXhLds];
    const uint32_t nslots = (uint32_t)d.nframes * (uint32_t)d.max_blocks;
    xxh32_group(lds, [&](uint32_t i) {
        const uint32_t f = i < nslots ? i % (uint32_t)d.nframes : i - nslots;
        LfFrame *const r = d.frame + f;
        XStream st{nullptr, 0u, nullptr};
        if (r->code) {
            // nothing of a frame with a code is hashed
        } else if (i < nslots) {   // a block, as it sits in the frame
            if ((r->flg & kFlgBlockSum) && d.kind[i] != kLfAbsent) {
                st.p = (gcu8 *)d.data[i];
                st.n = (uint32_t)d.size[i];
                st.out = d.got + i;
            }
        } else if (r->flg & kFlgContentSum) {
            if constexpr (kPlaced) {   // the content: [0, total), inside the capacity
                st.p = (gcu8 *)d.dst[f];
                st.n = (uint32_t)d.total[f];
                st.out = &r->got;
            } else {
                // The decoded bytes: full blocks, then what the last one gave.  The frame is
                // untrusted: with a declared content size the capacity may be far below blocks x
                // maximum, and a last block 00 "decodes" to 0 in no room at all, so the length is
                // taken in 64 bits and nothing is hashed unless it lies inside the destination
                // (finish then reports the block that did not fit: -4 or -5).
                const uint32_t nb = (uint32_t)r->nb;
                const int last = nb ? lfd_block_result(d, (nb - 1u) * (uint32_t)d.nframes + f) : 0;
                const uint64_t n = (nb ? (uint64_t)(nb - 1u) * r->bmax : 0u) + (uint64_t)(last > 0 ? last : 0);
                const int cap = d.dst_cap[f];
                if (last >= 0 && cap >= 0 && n <= (uint64_t)cap) {
                    st.p = (gcu8 *)d.dst[f];
                    st.n = (uint32_t)n;
                    st.out = &r->got;
                }
            }
        }
        return st;
    }, blockIdx.x * (uint32_t)kXhStreams, nslots + (uint32_t)d.nframes, 0u);
}

// one wave per frame: the first code of the table that applies, or the decoded size
__global__ void __launch_bounds__(64)
lz4f_decode_finish_kernel(LfDecode d) {
    const uint32_t f = blockIdx.x, lane = (uint32_t)lane_id(), nf = (uint32_t)d.nframes;
    const LfFrame r = d.frame[f];
    int code = r.code;
    if (!code) {
        const uint32_t nb = (uint32_t)r.nb;
        const bool sums = d.verify && (r.flg & kFlgBlockSum);
        bool bad_sum = false, bad_block = false, is_short = false;
        uint32_t tail = 0u;   // what the last block gave (one lane's)
        for (uint32_t q = lane; q < nb; q += 64u) {
            const uint32_t i = q * nf + f;
            const int got = lfd_block_result(d, i);
            bad_sum |= sums && d.got[i] != d.want[i];
            bad_block |= got < 0;
            is_short |= q + 1u < nb && got >= 0 && (uint32_t)got != r.bmax;
            if (q + 1u == nb && got >= 0) tail = (uint32_t)got;
        }
        tail = lane_val(wave_incl_max(tail), 63);
        // In 64 bits: with a declared content size nothing bounds blocks x maximum.  A size
        // above the capacity (so above 2^31 too) means a block before the last had less room
        // than the maximum, which is -4 or -5 before this is looked at; the check is kept.
        const uint64_t size = (nb ? (uint64_t)(nb - 1u) * r.bmax : 0u) + tail;
        const int cap = d.dst_cap[f];
        if (wave_any(bad_sum)) code = -6;
        else if (wave_any(bad_block)) code = -4;
        else if (wave_any(is_short)) code = -5;
        else if (cap < 0 || size > (uint64_t)cap) code = -4;
        else if ((r.flg & kFlgSize) && (uint64_t)r.content != size) code = -8;
        else if (d.verify && (r.flg & kFlgContentSum) && r.got != r.want) code = -7;
        else code = (int)size;
    }
    if (lane == 0u) d.result[f] = code;
}

// ---- the placed call's own launches: place and finish (the sizer is lz4_decode.hip's) ----
// `cap` becomes the block's measured size, which is also the room its decoder gets.
// the bytes block i of a planned frame decodes to, or -1: a stored block's length, else what
// the sizer found
__device__ __forceinline__ int lfp_measured(const LfDecode &d, uint32_t i) {
    return d.kind[i] == kLfStored ? d.size[i] : d.res_s[i];
}

// One wave per frame: the sizes scanned into positions and the total.  What can be decided is
// decided here, before a byte of the destination is written: a block without a size (-4), a
// total above the capacity (-9), a declared content size that is not the total (-8).  Such a
// frame's slots become absent; the others get their place, out = dst + pos, a room of exactly
// the measured size, and for a linked block the output before it as dictionary.
// kDict: block 0 of a linked frame keeps the frame's dictionary, which the plan gave it.  A later
// compressed block of such a frame that starts below 65536 would need the dictionary's tail and
// the output before it as one history, which the block decoder does not have: the frame is -3,
// after the sizing's -4 and before -9 and -8.
template <bool kDict>
__global__ void __launch_bounds__(64)
lz4f_placed_place_kernel(LfDecode d) {
    const uint32_t f = blockIdx.x, lane = (uint32_t)lane_id(), nf = (uint32_t)d.nframes;
    LfFrame &r = d.frame[f];
    if (r.code) return;   // (its slots are absent since the plan)
    const uint32_t nb = (uint32_t)r.nb;
    const int cap = d.dst_cap[f];
    // (a chunk of 64 blocks sums to at most 2^28; the total is kept in 64 bits)
    uint64_t total = 0u;
    bool unsized = false, two_part = false;
    const bool linked_dict = kDict && r.dsize > 0 && !(r.flg & kFlgLinkedOff);
    for (uint32_t q0 = 0; q0 < nb; q0 += 64u) {
        const uint32_t q = q0 + lane;
        const int m = q < nb ? lfp_measured(d, q * nf + f) : 0;
        unsized |= m < 0;
        const uint32_t mine = m > 0 ? (uint32_t)m : 0u, incl = wave_incl_sum(mine);
        if constexpr (kDict)
            two_part |= linked_dict && q >= 1u && q < nb && d.kind[q * nf + f] == kLfLinked &&
                        total + (incl - mine) < 65536u;
        total += lane_val(incl, 63);
    }
    int code = 0;
    if (wave_any(unsized)) code = -4;
    else if (kDict && wave_any(two_part)) code = -3;
    else if (cap < 0 || total > (uint64_t)cap) code = -9;
    else if ((r.flg & kFlgSize) && (uint64_t)r.content != total) code = -8;
    if (code) {
        for (uint32_t q = lane; q < nb; q += 64u) lfd_absent<true>(d, q * nf + f);
        if (lane == 0u) r.code = code;
        return;
    }
    char *const out = wave_uniform(d.dst[f]);
    uint32_t at = 0u;   // (total <= cap < 2^31)
    for (uint32_t q0 = 0; q0 < nb; q0 += 64u) {
        const uint32_t q = q0 + lane, i = q * nf + f;
        const uint32_t m = q < nb ? (uint32_t)lfp_measured(d, i) : 0u;
        const uint32_t incl = wave_incl_sum(m);
        if (q < nb) {
            const uint32_t pos = at + incl - m;
            const int kind = d.kind[i];
            lfd_place(d, i, out + pos, (int)m);
            // (block 0 of a linked frame with a dictionary keeps it)
            if (linked_dict && q == 0u && kind == kLfLinked) d.cap_b[i] = (int)m;
            else lfd_place_kind(d, i, kind, out, pos, (int)m);
        }
        at += lane_val(incl, 63);
    }
    if (lane == 0u) d.total[f] = (int)total;
}

// one wave per frame: the place launch's code, else the first of -6, -4, -7, else the total
__global__ void __launch_bounds__(64)
lz4f_placed_finish_kernel(LfDecode d) {
    const uint32_t f = blockIdx.x, lane = (uint32_t)lane_id(), nf = (uint32_t)d.nframes;
    const LfFrame r = d.frame[f];
    int code = r.code;
    if (!code) {
        const uint32_t nb = (uint32_t)r.nb;
        const bool sums = d.verify && (r.flg & kFlgBlockSum);
        bool bad_sum = false, bad_block = false;
        for (uint32_t q = lane; q < nb; q += 64u) {
            const uint32_t i = q * nf + f;
            bad_sum |= sums && d.got[i] != d.want[i];
            bad_block |= lfd_block_result(d, i) != d.cap[i];   // (not what was measured)
        }
        if (wave_any(bad_sum)) code = -6;
        else if (wave_any(bad_block)) code = -4;
        else if (d.verify && (r.flg & kFlgContentSum) && r.got != r.want) code = -7;
        else code = d.total[f];
    }
    if (lane == 0u) d.result[f] = code;
}

// ---- host side ----
// a scratch cut into regions that start 16-byte aligned: take() is the next region's offset,
// `at` the bytes taken so far
struct Cutter {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t was = at;
        at += (bytes + 15) & ~(size_t)15;
        return was;
    }
};

}  // namespace

// ---- launchers ----
hipError_t launch_xxh32(const char *const *src, const int *size, uint32_t seed, uint32_t *hash,
                        int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const unsigned groups = ((unsigned)n + kXhStreams - 1u) / kXhStreams;
    hipLaunchKernelGGL(xxh32_batch_kernel, dim3(groups), dim3(64), 0, s, src, size, seed, hash, n);
    return hipGetLastError();
}

size_t lz4f_compress_layout(int nframes, int max_src, int bsid, LfCompress *out) {
    const size_t block = lf_block_bytes(bsid);
    const size_t bpf = max_src > 0 ? ((size_t)max_src + block - 1) / block : 1;
    const size_t nslots = (size_t)nframes * bpf;
    if (nslots >= ((size_t)1 << 24)) return (size_t)-1;
    Cutter c;
    const size_t buf = c.take(nslots * block), src = c.take(nslots * 8), dst = c.take(nslots * 8);
    const size_t size = c.take(nslots * 4), cap = c.take(nslots * 4), res = c.take(nslots * 4);
    const size_t off = c.take(nslots * 4), hash = c.take(nslots * 4);
    const size_t total = c.take((size_t)nframes * 4), fhash = c.take((size_t)nframes * 4);
    if (out) {
        char *b = out->buf;
        out->bpf = (int)bpf;
        out->nslots = (int)nslots;
        out->bsid = bsid;
        out->ppb = (int)(block / kLfPiece);
        out->buf = b + buf;
        out->s_src = (const char **)(b + src);
        out->s_dst = (char **)(b + dst);
        out->s_size = (int *)(b + size);
        out->s_cap = (int *)(b + cap);
        out->s_res = (int *)(b + res);
        out->s_off = (uint32_t *)(b + off);
        out->s_hash = (uint32_t *)(b + hash);
        out->f_total = (int *)(b + total);
        out->f_hash = (uint32_t *)(b + fhash);
    }
    return c.at;
}

// layout, hash (with a checksum flag), pack: what follows the encoder in both compress calls
template <bool kDict>
static hipError_t lz4f_compress_rest(const LfCompress &c, hipStream_t s) {
    hipError_t e;
    hipLaunchKernelGGL(lz4f_compress_layout_kernel<kDict>, dim3((unsigned)c.nframes), dim3(64), 0,
                       s, c);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (c.flags & 3) {   // block checksums are streams [0, nslots), content checksums follow
        const uint32_t first = (c.flags & 2) ? 0u : (uint32_t)c.nslots;
        const uint32_t end = (c.flags & 1) ? (uint32_t)c.nslots + (uint32_t)c.nframes
                                           : (uint32_t)c.nslots;
        hipLaunchKernelGGL(lz4f_compress_hash_kernel,
                           dim3((end - first + kXhStreams - 1u) / kXhStreams), dim3(64), 0, s, c,
                           first, end);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lz4f_compress_pack_kernel<kDict>, dim3((unsigned)c.nslots * (unsigned)c.ppb),
                       dim3(64), 0, s, c);
    return hipGetLastError();
}

hipError_t launch_lz4f_compress(const LfCompress &c, hipStream_t s) {
    if (c.nframes <= 0) return hipSuccess;
    hipError_t e;
    hipLaunchKernelGGL(lz4f_compress_plan_kernel, dim3(((unsigned)c.nslots + 255u) / 256u),
                       dim3(256), 0, s, c);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    BlockArgs a{};
    a.src = c.s_src;
    a.dst = c.s_dst;
    a.src_size = c.s_size;
    a.dst_cap = c.s_cap;
    a.result = c.s_res;
    a.nblocks = c.nslots;
    if ((e = launch_encode(a, s)) != hipSuccess) return e;
    return lz4f_compress_rest<false>(c, s);
}

// The call with preferences (include/ape_lz4f_prefs.h): the slots are the
// "inputs" of the mode's large-input launcher, `a` its arguments over the slot arrays.
hipError_t launch_lz4f_prefs_compress(const LfCompress &c, const LargeArgs &a, int mode, int depth,
                                      void *hc, int pass, hipStream_t s) {
    if (c.nframes <= 0) return hipSuccess;
    hipError_t e;
    hipLaunchKernelGGL(lz4f_compress_plan_kernel, dim3(((unsigned)c.nslots + 255u) / 256u),
                       dim3(256), 0, s, c);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = mode == 0 ? launch_large(a, 1, s) : launch_large_hc(a, depth, hc, pass, s, nullptr, mode == 2);
    if (e != hipSuccess) return e;
    return lz4f_compress_rest<false>(c, s);
}

hipError_t launch_lz4f_dict_compress_plan(const LfCompress &c, hipStream_t s) {
    if (c.nframes <= 0) return hipSuccess;
    hipLaunchKernelGGL(lz4f_dict_compress_plan_kernel, dim3(((unsigned)c.nframes + 255u) / 256u),
                       dim3(256), 0, s, c);
    return hipGetLastError();
}

hipError_t launch_lz4f_dict_compress_rest(const LfCompress &c, hipStream_t s) {
    if (c.nframes <= 0) return hipSuccess;
    return lz4f_compress_rest<true>(c, s);
}


size_t lz4f_dict_compress_layout(int nframes, int max_src, LfCompress *out) {
    const size_t n = (size_t)nframes, slot = ((size_t)max_src + 15) & ~(size_t)15;
    if (n >= ((size_t)1 << 24)) return (size_t)-1;
    Cutter c;
    const size_t buf = c.take(n * slot), src = c.take(n * 8), dst = c.take(n * 8);
    size_t ints[7];   // s_size, s_cap, s_res, s_off, s_hash, f_total, f_hash
    for (int k = 0; k < 7; k++) ints[k] = c.take(n * 4);
    if (out) {
        char *b = out->buf;
        out->bpf = 1;
        out->nslots = nframes;
        out->bsid = 4;
        out->ppb = 1;   // (a slot holds at most 65536 bytes)
        out->slot = (int)slot;
        out->buf = b + buf;
        out->s_src = (const char **)(b + src);
        out->s_dst = (char **)(b + dst);
        out->s_size = (int *)(b + ints[0]);
        out->s_cap = (int *)(b + ints[1]);
        out->s_res = (int *)(b + ints[2]);
        out->s_off = (uint32_t *)(b + ints[3]);
        out->s_hash = (uint32_t *)(b + ints[4]);
        out->f_total = (int *)(b + ints[5]);
        out->f_hash = (uint32_t *)(b + ints[6]);
    }
    return c.at;
}

hipError_t launch_lz4f_info(const char *const *src, const int *src_size, int *info, int nframes,
                            hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    hipLaunchKernelGGL(lz4f_info_kernel<false>, dim3(((unsigned)nframes + 63u) / 64u), dim3(64),
                       0, s, src, src_size, info, nframes);
    return hipGetLastError();
}

hipError_t launch_lz4f_info_dict(const char *const *src, const int *src_size, int *info,
                                 int nframes, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    hipLaunchKernelGGL(lz4f_info_kernel<true>, dim3(((unsigned)nframes + 63u) / 64u), dim3(64), 0,
                       s, src, src_size, info, nframes);
    return hipGetLastError();
}

size_t lz4f_decode_layout(int nframes, int max_blocks, bool placed, LfDecode *out) {
    const size_t nslots = (size_t)nframes * (size_t)max_blocks;
    if (nslots >= ((size_t)1 << 24)) return (size_t)-1;
    Cutter c;
    const size_t zero = c.take(16), frame = c.take((size_t)nframes * sizeof(LfFrame));
    size_t ptrs[5], ints[12], sizer[3] = {0, 0, 0};
    for (size_t &p : ptrs) p = c.take(nslots * 8);
    for (size_t &p : ints) p = c.take(nslots * 4);
    if (placed) {   // after the grid call's regions
        sizer[0] = c.take(nslots * 4);
        sizer[1] = c.take(nslots * 4);
        sizer[2] = c.take((size_t)nframes * 4);
    }
    if (out) {
        char *b = (char *)out->zero;
        out->zero = b + zero;
        out->frame = (LfFrame *)(b + frame);
        out->src_a = (const char **)(b + ptrs[0]);
        out->src_b = (const char **)(b + ptrs[1]);
        out->dict = (const char **)(b + ptrs[2]);
        out->out = (char **)(b + ptrs[3]);
        out->data = (const char **)(b + ptrs[4]);
        int **const arrays[12] = {&out->size_a, &out->cap_a, &out->res_a, &out->size_b,
                                  &out->cap_b, &out->res_b, &out->dict_size, &out->size,
                                  &out->kind, &out->cap, (int **)&out->want, (int **)&out->got};
        for (int k = 0; k < 12; k++) *arrays[k] = (int *)(b + ints[k]);
        out->placed = placed;
        out->cap_s = placed ? (int *)(b + sizer[0]) : nullptr;
        out->res_s = placed ? (int *)(b + sizer[1]) : nullptr;
        out->total = placed ? (int *)(b + sizer[2]) : nullptr;
    }
    return c.at;
}

hipError_t launch_lz4f_decode(const LfDecode &d, hipStream_t s) {
    if (d.nframes <= 0) return hipSuccess;
    hipError_t e;
    const int nslots = d.nframes * d.max_blocks;
    const dim3 frames((unsigned)d.nframes), slots((unsigned)nslots), wave(64);
    void (*const plan)(LfDecode) = d.dicts ? d.placed ? lz4f_decode_plan_kernel<true, true>
                                                      : lz4f_decode_plan_kernel<false, true>
                                           : d.placed ? lz4f_decode_plan_kernel<true, false>
                                                      : lz4f_decode_plan_kernel<false, false>;
    hipLaunchKernelGGL(plan, frames, wave, 0, s, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (d.placed) {
        BlockArgs z{};   // every slot: a stored or absent one has capacity 0 and ends at once
        z.src = d.data;
        z.src_size = d.size;
        z.dst_cap = d.cap_s;
        z.dict_size = d.dict_size;
        z.result = d.res_s;
        z.nblocks = nslots;
        if ((e = launch_decode_size(z, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(d.dicts ? lz4f_placed_place_kernel<true>
                                   : lz4f_placed_place_kernel<false>, frames, wave, 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lz4f_decode_stored_kernel, slots, wave, 0, s, d);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    BlockArgs a{};
    a.src = d.src_a;
    a.dst = d.out;
    a.src_size = d.size_a;
    a.dst_cap = d.cap_a;
    a.result = d.res_a;
    a.nblocks = nslots;
    if (d.dicts && d.ntable > 0) {   // the blocks of independent frames against their dictionaries
        a.dict = d.dict;
        a.dict_size = d.dict_size;
    }
    if ((e = launch_decode(a, false, s)) != hipSuccess) return e;
    if (!d.no_linked) {
        BlockArgs b{};
        b.src = d.src_b;
        b.dst = d.out;
        b.src_size = d.size_b;
        b.dst_cap = d.cap_b;
        b.dict = d.dict;
        b.dict_size = d.dict_size;
        b.result = d.res_b;
        b.nblocks = nslots;
        if ((e = launch_decode_chain(b, d.nframes, d.max_blocks, s)) != hipSuccess) return e;
    }
    if (d.verify) {
        const unsigned streams = (unsigned)nslots + (unsigned)d.nframes;
        hipLaunchKernelGGL(d.placed ? lz4f_decode_hash_kernel<true> : lz4f_decode_hash_kernel<false>,
                           dim3((streams + kXhStreams - 1u) / kXhStreams), wave, 0, s, d);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(d.placed ? lz4f_placed_finish_kernel : lz4f_decode_finish_kernel, frames,
                       wave, 0, s, d);
    return hipGetLastError();
}

}  // namespace apelz4
