// lz4_gpu_internal.h -- shared device helpers and launcher prototypes for the
// MI355X LZ4 kernels (gfx950 / CDNA4, wave64).  Internal to libape_lz4_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace apelz4 {

// Format constants of LZ4 v1.7.1 (ref src/ape_lz4.c:237-254).
constexpr int kMinMatch = 4;
constexpr int kLastLiterals = 5;
constexpr int kMFLimit = 12;
constexpr int kMinLength = 13;
constexpr int kMaxBlock = 65536;  // GPU block limit (LZ4 window, benchmark block)
constexpr int kErange = -2147483647 - 1;

// Global-address-space byte pointers: global_load/store with an SGPR base and a
// 32-bit offset instead of flat accesses (which also tie up lgkmcnt).
typedef __attribute__((address_space(1))) const uint8_t gcu8;
typedef __attribute__((address_space(1))) uint8_t gu8;
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));

// unaligned 16 / 8 / 4-byte global accesses (the hardware handles any alignment)
__device__ __forceinline__ uint4 gload16(gcu8 *p) {
    const u32x4_u v = *(__attribute__((address_space(1))) const u32x4_u *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint2 gload8(gcu8 *p) {
    const u32x2_u v = *(__attribute__((address_space(1))) const u32x2_u *)p;
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint32_t gload4(gcu8 *p) {
    return *(__attribute__((address_space(1))) const u32_u *)p;
}
__device__ __forceinline__ void gstore16(gu8 *p, uint4 v) {
    u32x4_u w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    *(__attribute__((address_space(1))) u32x4_u *)p = w;
}
__device__ __forceinline__ void gstore4(gu8 *p, uint32_t v) {
    *(__attribute__((address_space(1))) u32_u *)p = v;
}

// ---- wave64 helpers ----
__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// Wave votes on a bool: HIP's __ballot / __any take an int, and the int round trip
// costs a v_cndmask + v_cmp per vote where the condition already is a lane mask.
__device__ __forceinline__ uint64_t wave_ballot(bool c) { return __builtin_amdgcn_ballot_w64(c); }
__device__ __forceinline__ bool wave_any(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }
// This lane's bit of a wave-uniform mask as a lane predicate: the mask itself becomes the
// condition register (no shift / and / 64-bit compare per lane).
__device__ __forceinline__ bool lane_in(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// DPP lane moves (GFX9-family controls, available on gfx950): lanes whose
// source is outside the row / masked off keep `old`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, false);
}
// ... with every row and bank enabled and bound_ctrl set: a lane whose source is outside
// reads 0, and no `old` register is needed (no v_mov 0 before the move)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_z(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114,
              kDppRowShr8 = 0x118, kDppBcast15 = 0x142, kDppBcast31 = 0x143,
              kDppWaveShr1 = 0x138, kDppWaveShl1 = 0x130;

// Inclusive scans over the 64 lanes (Hillis-Steele inside 16-lane rows, then
// row broadcasts) -- VALU latency instead of LDS-crossbar shuffles.
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x) {
    x += dpp<kDppRowShr1>(0u, x);
    x += dpp<kDppRowShr2>(0u, x);
    x += dpp<kDppRowShr4>(0u, x);
    x += dpp<kDppRowShr8>(0u, x);
    x += dpp<kDppBcast15, 0xA>(0u, x);
    x += dpp<kDppBcast31, 0xC>(0u, x);
    return x;
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x) {
    x = umax(x, dpp<kDppRowShr1>(0u, x));
    x = umax(x, dpp<kDppRowShr2>(0u, x));
    x = umax(x, dpp<kDppRowShr4>(0u, x));
    x = umax(x, dpp<kDppRowShr8>(0u, x));
    x = umax(x, dpp<kDppBcast15, 0xA>(0u, x));
    x = umax(x, dpp<kDppBcast31, 0xC>(0u, x));
    return x;
}

// value of the previous lane (lane 0 gets `first`)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x, uint32_t first) {
    return dpp<kDppWaveShr1>(first, x);
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v) {
    return wave_shr1(wave_incl_sum(v), 0u);
}

__device__ __forceinline__ uint32_t lane_val(uint32_t v, int l) {  // l wave-uniform
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

// A value every lane of the wave holds alike, moved into a scalar register; a pointer likewise
// (one loaded from an array entry that the workgroup indexes by blockIdx): what is read through
// it keeps an SGPR base.
__device__ __forceinline__ uint32_t wave_first(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
template <class T>
__device__ __forceinline__ T *wave_uniform(T *p) {
    const uint64_t v = (uint64_t)p;
    return (T *)((uint64_t)wave_first((uint32_t)(v >> 32)) << 32 | wave_first((uint32_t)v));
}

// ---- the encoder's hash table (lz4_encode.hip; lz4_cdict.hip prebuilds an image of it) ----
// Table entries, the hash scaled onto [0, kHSize).  7328 entries make the block's LDS 17904
// bytes, inside the 35 x 512-byte granules that fit 9 blocks = 27 waves per CU (7 per SIMD:
// <= 72 VGPRs); the reference's 8192 entries fit 8 blocks, +4.6 % encode time for +0.6 % ratio
// (measured; tools/enc_model.c models the ratio per table size).
constexpr int kHSize = 7328;
static_assert(kHSize < 8192 && kHSize % 8 == 0, "table size");
// Bytes the table hash covers (the reference: 5, :456-473).  7 keeps short chance matches from
// pre-empting longer ones: ratio up, 23 % fewer sequences (tools/enc_model.c key study,
// DESIGN.md 3.1).
constexpr int kKey = 7;

// Hash of the kKey bytes at p (x0 = in[p..p+3], x1 = in[p+4..p+7]) onto [0, kHSize).  The
// reference multiplies the 40-bit sequence by 889523592379 (:456-473), which needs
// quarter-rate 32-bit multiplies here; any hash gives a valid stream, so this one uses
// full-rate 24 x 24-bit multiplies (v_mul_u32_u24 / v_mad_u32_u24, which read only the low
// 24 bits of their operands) of bytes 0-2, 3-5 and 6.
__device__ __forceinline__ uint32_t hashk(uint32_t x0, uint32_t x1) {
    static_assert(kKey == 7, "hashk covers bytes 0..6");
    const uint32_t hi = __builtin_amdgcn_alignbyte(x1, x0, 3u);   // bytes 3..6 (the multiply takes 3..5)
    // (__umul24 returns int: do the sums unsigned)
    const uint32_t v = (uint32_t)__umul24(x0, 0x9E3779u) + (uint32_t)__umul24(hi, 0xC2B2AEu) +
                       (uint32_t)__umul24((x1 >> 16) & 0xFFu, 0x27D4EBu);
    return __umulhi(v, (uint32_t)kHSize);   // v scaled onto [0, kHSize): one v_mul_hi_u32
}

// ---- prepared dictionary (lz4_cdict.hip writes it, lz4_encode_kernel<.., EXT> reads it) ----
// One device object, every region 16-byte aligned:
//   [0, 16)                      header: magic, D (window bytes), maxSrcSize, 0
//   [kCdTab, kCdTab + 2 kHSize)  the table prefix_history would build for window positions
//                                [0, D) alone (u16 positions, 0 = empty)
//   [kCdWin, kCdSize)            kCdFront bytes of pad, the window (the dictionary's last D
//                                bytes, window position v at kCdWin + kCdFront + v), then pad to
//                                the object's end (>= kCdBack bytes): a 16-byte load at any
//                                window position, or up to 4 bytes before it, stays inside
// D + maxSrcSize <= 65536 (one window of u16 positions), D a multiple of 64.
constexpr uint32_t kCdMagic = 0x44435A4Cu;   // "LZCD"
constexpr uint32_t kCdTab = 16u, kCdWin = kCdTab + 2u * (uint32_t)kHSize;
constexpr uint32_t kCdFront = 16u, kCdBack = 256u;
constexpr uint32_t kCdMaxWin = (uint32_t)kMaxBlock - 64u;   // maxSrcSize >= 1 leaves 65472
constexpr uint32_t kCdSize = kCdWin + kCdFront + (uint32_t)kMaxBlock + kCdBack;
static_assert(kCdWin % 16u == 0u && kCdSize % 16u == 0u, "prepared dictionary regions");
struct CDictHdr {
    uint32_t magic, D, max_src, zero;
};
// The prepared object a message names in a per-message array: null for a null
// or not 16-byte aligned entry, of which nothing is read.
__device__ __forceinline__ const uint8_t *message_object(const uint8_t *const *objs, int b) {
    const uint8_t *cd = wave_uniform(objs[b]);
    return ((uint64_t)cd & 15u) ? nullptr : cd;
}
// The header of either kind of object.  PER: of message_object's, into scalar registers.
template <bool PER, class P>
__device__ __forceinline__ CDictHdr object_header(P *cd) {
    if constexpr (!PER) {
        return *(const CDictHdr *)cd;
    } else {
        const uint4 v = gload16((gcu8 *)cd);
        return CDictHdr{wave_first(v.x), wave_first(v.y), wave_first(v.z), wave_first(v.w)};
    }
}
// D of a prepared dictionary: min(dict_size, 65536 - max_src) rounded down to 64 (host and device)
__host__ __device__ inline int cdict_window(int dict_size, int max_src) {
    const int room = kMaxBlock - max_src;
    return (dict_size < room ? dict_size : room) & ~63;
}

// ---- diagnostic phase timers (built only into libape_lz4_amd_stats.so) ----
// Thread 0 of every workgroup accumulates s_memtime cycles per phase and adds them
// to a per-kernel __device__ array at exit.  Never compiled into the product.
#ifdef APE_LZ4_STATS
#define STATS_DECL uint64_t st_t_ = clock64(); uint64_t st_acc_[16] = {0};
#define STAT(i) do { uint64_t t_ = clock64(); st_acc_[i] += t_ - st_t_; st_t_ = t_; } while (0)
#define STAT_ADD(i, v) (st_acc_[i] += (uint64_t)(v))
#define STATS_FLUSH(arr) STATS_FLUSH_TID(arr, 0)
#define STATS_FLUSH_TID(arr, t) do { if (threadIdx.x == (t)) { _Pragma("unroll") for (int i_ = 0; i_ < 16; i_++) if (st_acc_[i_]) atomicAdd(&(arr)[i_], (unsigned long long)st_acc_[i_]); } } while (0)
#else
#define STATS_DECL
#define STAT(i) do {} while (0)
#define STAT_ADD(i, v) do {} while (0)
#define STATS_FLUSH(arr) do {} while (0)
#define STATS_FLUSH_TID(arr, t) do {} while (0)
#endif
hipError_t stats_read(int which, unsigned long long *out, int reset);

// Launchers (lz4_decode.hip / lz4_encode.hip / lz4_synth.hip).
struct BlockArgs {
    const char *const *src;   // pointer-array form (nullptr when strided)
    char *const *dst;
    const char *src_base;     // strided form
    char *dst_base;
    size_t src_stride, dst_stride;
    const int *src_size;      // per-block input size
    const int *dst_cap;       // per-block capacity (nullable -> default)
    const int *target;        // partial decode target (nullable)
    const long long *frame_off;  // decoder: blocks read from a framed stream at src_base
                                 // (frame i = [le32 size][block] at src_base + frame_off[i])
    const char *const *dict;  // decoder: per-block external dictionary (nullable) ...
    const int *dict_size;     // ... and its size (usingDict, ref src/ape_lz4.c:1625-1647)
    int fast;                 // decoder: decompress_fast (src_size = readable bound of src)
    int accel;                // encoder: acceleration (compress_fast, :789); > 1 drops the
                              // in-chunk candidate (faster, lower ratio)
    int *result;
    int nblocks;
    int *tail;                // encoder: per-block length of the final literal run (nullable;
                              // the large-input path stitches slices there, lz4_large.hip)
};

hipError_t launch_decode(const BlockArgs &a, bool partial, hipStream_t s);
// usingDict decodes of nq chunk positions x nconn connections (block q * nconn + i), one
// workgroup per connection looping over its chunks in order (lz4_decode.hip)
hipError_t launch_decode_chain(const BlockArgs &a, int nconn, int nq, hipStream_t s);
hipError_t launch_encode(const BlockArgs &a, hipStream_t s);
// against a prepared dictionary (layout above): the history is the object's window and table
// image, not the bytes before each block (lz4_encode.hip, its EXT instantiation)
hipError_t launch_encode_cdict(const BlockArgs &a, const void *cdict, hipStream_t s);
// ... message i against the object cdicts[i] (a device array of device pointers)
hipError_t launch_encode_cdicts(const BlockArgs &a, const void *const *cdicts, hipStream_t s);
// dict[dict_size - D, dict_size) -> the prepared dictionary at cdict (lz4_cdict.hip)
hipError_t launch_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                hipStream_t s);
// n objects in one launch, object k at cdicts + k * stride from dict[k], dict_size[k] (device
// arrays); a negative size, or a null pointer with a positive one, leaves a zero header
hipError_t launch_cdict_prepare_batch(const char *const *dict, const int *dict_size, int max_src,
                                      void *cdicts, size_t stride, int n, hipStream_t s);
// the greedy-exact mode (lz4_encode_exact.hip): the reference's sequential parse, byte for byte
hipError_t launch_encode_exact(const BlockArgs &a, hipStream_t s);
// The high-ratio mode (lz4_encode_hc.hip; tests/hcmodel.py restates the two constants): hash
// chains over the block, the first `depth` chain members of every position searched for the
// longest match, then a sequential parse with a one-step lazy rule.  With HcArgs::prefix the
// block is the end of a window of history + block (tests/hclargemodel.py).
constexpr int kHcCap = 272;       // longest match the search reports (the parse extends it)
constexpr int kHcHashBits = 14;   // chain hash; the u16 head table is 32 KiB of LDS
constexpr int kHcMaxDepth = 256, kHcDefaultDepth = 64;
constexpr int kHcTable = 1 << kHcHashBits;
__device__ __forceinline__ uint32_t hc_hash(uint32_t x) {
    return (x * 2654435761u) >> (32 - kHcHashBits);
}
// bytes of a length field after the token (value v >= 15: 255s, then the remainder)
__device__ __forceinline__ uint32_t len_bytes(uint32_t v) { return v >= 15u ? (v - 15u) / 255u + 1u : 0u; }
// leading equal bytes of two little-endian words whose xor is x (x != 0)
__device__ __forceinline__ uint32_t first_diff(uint32_t x) { return (uint32_t)__builtin_ctz(x) >> 3; }
// scratch of one block: chain[p] (u16: nearest earlier position with p's hash, + 1; 0 = none)
// and match[p] (u32: length << 16 | source; 0 = none) for every position
constexpr size_t kHcChainBytes = (size_t)kMaxBlock * sizeof(uint16_t);
constexpr size_t kHcSlotBytes = kHcChainBytes + (size_t)kMaxBlock * sizeof(uint32_t);
struct HcArgs {
    const char *const *src;   // caller's arrays, one entry per block of this pass
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    int *result;
    int nblocks, depth;
    uint16_t *chain;          // block i's at chain + i * kMaxBlock ...
    uint32_t *match;          // ... and match + i * kMaxBlock
    const int *prefix;        // per-block bytes of history before src[i] (nullable: none); the
                              // last min(prefix, 65536 - size) of them are used, and chain[] and
                              // match[] are then indexed by position in history + block
    int *tail;                // per-block length of the final literal run, as BlockArgs::tail
                              // (nullable)
};
// chain build (one wave per block), search (one lane per position), parse + emit (one wave per
// block)
hipError_t launch_encode_hc(const HcArgs &a, hipStream_t s, hipEvent_t *ev = nullptr);
// The cost-minimising parse (lz4_encode_hc.hip; tests/hcoptmodel.py is the
// definition): the chain build and the search above as they are, then a parse that prices
// every position backward and emits forward.  It needs one more table per block, cost[p] (u32:
// the bytes the rest of the block takes from p on), so the scratch of one block is
// kHcOptSlotBytes.  HcArgs keeps its layout: the extra pointer travels beside it.
constexpr size_t kHcOptSlotBytes = kHcSlotBytes + (size_t)kMaxBlock * sizeof(uint32_t);
struct HcOptArgs {
    HcArgs a;
    uint32_t *cost;           // block i's at cost + i * kMaxBlock
};
// chain build, search, price + emit (one wave per block): three launches
hipError_t launch_encode_hc_opt(const HcOptArgs &o, hipStream_t s, hipEvent_t *ev = nullptr);

// ---- prepared high-ratio dictionary (lz4_hc_cdict.hip) ----
// The window of message m is [the dictionary's last D bytes | m], D = min(dictSize, 65536 -
// maxSrcSize), not rounded; the bytes are compress_hc_withPrefix's for that window
// (tests/hcdictmodel.py).  One device object, every region 16-byte aligned:
//   [0, 16)              header: magic, D, maxSrcSize, 0
//   [kHdHead, kHdChain)  the u16 head table (position + 1, 0 = empty) as the chain build leaves
//                        it after window positions 0 .. D - 4, the ones whose 4 bytes lie in
//                        the dictionary
//   [kHdChain, kHdWin)   chain[0 .. D - 4] of those positions (u16), zero up to entry 65535
//   [kHdWin, kHdSize)    kCdFront bytes of pad, the window's D dictionary bytes, then zero to
//                        the object's end (>= kCdBack bytes): a 16-byte load at any of the D
//                        positions stays inside
constexpr uint32_t kHdMagic = 0x44485A4Cu;   // "LZHD"
constexpr uint32_t kHdHead = 16u, kHdChain = kHdHead + 2u * (1u << kHcHashBits);
constexpr uint32_t kHdWin = kHdChain + 2u * (uint32_t)kMaxBlock;
constexpr uint32_t kHdSize = kHdWin + kCdFront + (uint32_t)kMaxBlock + kCdBack;
static_assert(kHdChain % 16u == 0u && kHdWin % 16u == 0u && kHdSize % 16u == 0u,
              "prepared high-ratio dictionary regions");
// D of a prepared high-ratio dictionary (host and device; 1 <= max_src <= 65536)
__host__ __device__ inline int hc_cdict_window(int dict_size, int max_src) {
    const int room = kMaxBlock - max_src;
    return dict_size < room ? dict_size : room;
}
// scratch of one message: chain[] of the window positions from D - 3 on (entry w - D + 3) and
// one match record per message position
inline size_t hc_cdict_chain_entries(int max_src) { return ((size_t)max_src + 3 + 7) & ~(size_t)7; }
inline size_t hc_cdict_match_entries(int max_src) { return ((size_t)max_src + 3) & ~(size_t)3; }
inline size_t hc_cdict_slot_bytes(int max_src) {
    return hc_cdict_chain_entries(max_src) * sizeof(uint16_t) +
           hc_cdict_match_entries(max_src) * sizeof(uint32_t);
}
constexpr int kHcdThreads = 256;   // search lanes per workgroup
inline int hc_cdict_groups(int max_src) { return (max_src + kHcdThreads - 1) / kHcdThreads; }
struct HcDictArgs {
    const char *const *src;   // caller's arrays, one entry per message of this pass
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    int *result;
    int nblocks, depth;
    int max_src;              // the caller's bound; the kernels compare it with the header's
    const uint8_t *cdict;
    uint16_t *chain;          // message i's at chain + i * chain_stride ...
    uint32_t *match;          // ... and match + i * match_stride (entries)
    uint32_t chain_stride, match_stride;
};
hipError_t launch_hc_cdict_prepare(const char *dict, int dict_size, int max_src, void *cdict,
                                   hipStream_t s);
// as launch_cdict_prepare_batch
hipError_t launch_hc_cdict_prepare_batch(const char *const *dict, const int *dict_size,
                                         int max_src, void *cdicts, size_t stride, int n,
                                         hipStream_t s);
// chain build (one wave per message), search (one lane per message position), parse + emit
// (one wave per message).  cdicts (nullable): message i's object is cdicts[i], not a.cdict.
hipError_t launch_encode_hc_cdict(const HcDictArgs &a, hipStream_t s,
                                  const uint8_t *const *cdicts = nullptr);
// The cost-minimising parse against the same object (tests/hcoptdictmodel.py is
// the definition): the chain build and the search above as they are, then a parse that prices
// every message position backward and emits forward.  One more table per message, cost[p] (u32:
// the bytes the rest of the message takes from position p on).  HcDictArgs keeps its layout.
inline size_t hc_cdict_cost_entries(int max_src) { return ((size_t)max_src + 3) & ~(size_t)3; }
inline size_t hc_cdict_opt_slot_bytes(int max_src) {
    return hc_cdict_slot_bytes(max_src) + hc_cdict_cost_entries(max_src) * sizeof(uint32_t);
}
struct HcDictOptArgs {
    HcDictArgs a;
    uint32_t *cost;           // message i's at cost + i * cost_stride (entries)
    uint32_t cost_stride;
};
// chain build, search, price + emit (one wave per message): three launches
hipError_t launch_encode_hc_cdict_opt(const HcDictOptArgs &o, hipStream_t s,
                                      const uint8_t *const *cdicts = nullptr);
// ---- dictionary training (lz4_dict_train.hip) ----
// tests/dicttrainmodel.py is the definition and restates these constants: 8-byte substrings of
// the samples are counted in a table of 2^kDtBits u32 entries, and rounds of scored segments
// ("slots": every segment / 4 bytes of every sample) pick the dictionary's pieces.
constexpr int kDtSub = 8;                                // d: bytes of a counted substring
constexpr int kDtBits = 20;                              // F: the table has 2^F entries
constexpr uint64_t kDtPrime = 0x9E3779B185EBCA87ull;     // index = (u64 LE * prime) >> (64 - F)
constexpr uint32_t kDtTable = 1u << kDtBits;
constexpr int kDtMinSeg = 16, kDtMaxSeg = 1024, kDtMaxDict = 65536;
constexpr int kDtMinSample = kDtSub, kDtMaxSample = 0x7E000000;
constexpr int kDtMaxGroups = 1024;   // score workgroups of a round, one partial each
// Scratch: the table, the state, then one partial per score workgroup.
struct DtState {
    uint32_t used, picks, ignored, zero;   // bytes and segments picked so far; samples ignored
};
struct DtPartial {
    unsigned long long score;   // a workgroup's best: highest score, then lowest slot
    uint32_t slot, zero;
};
constexpr size_t kDtStateAt = (size_t)kDtTable * sizeof(uint32_t);
constexpr size_t kDtPartialAt = kDtStateAt + sizeof(DtState);
static_assert(sizeof(DtState) == 16 && sizeof(DtPartial) == 16, "scratch regions");
// slots per sample (J), slots in all (M; < 2^31 given nsamples * max_sample < 2^31), and the
// score workgroups a round of `slots` slots gets (four waves each, one slot per wave and trip)
inline long long dt_slots_per_sample(int max_sample, int segment) {
    const int st = segment / 4;
    return ((long long)max_sample + st - 1) / st;
}
inline long long dt_slots(int nsamples, int max_sample, int segment) {
    return (long long)nsamples * dt_slots_per_sample(max_sample, segment);
}
inline int dt_groups(long long slots) {
    const long long g = (slots + 3) / 4;
    return g < 1 ? 1 : g > kDtMaxGroups ? kDtMaxGroups : (int)g;
}
inline size_t dt_scratch_bytes(int nsamples, int max_sample, int segment) {
    return kDtPartialAt +
           (size_t)dt_groups(dt_slots(nsamples, max_sample, segment)) * sizeof(DtPartial);
}
struct DtArgs {
    const char *const *samples;   // caller's arrays, one entry per sample
    const int *size;
    int nsamples, max_sample;
    char *dict;
    int capacity, segment;
    uint32_t *freq;               // the scratch's three regions
    DtState *state;
    DtPartial *partial;
    int *info;
};
// zero, count, per round with slots: score + pick, finish: 3 + 2 * rounds launches at most
hipError_t launch_dict_train(const DtArgs &a, hipStream_t s);

// compress_destSize pass 2 (lz4_destsize.hip): scratch slot i (at scratch + i*stride, encoder
// result sres[i]) -> dst[i] cut to target[i]; src_size[i] <- consumed input
hipError_t launch_destsize(const char *const *src, int *src_size, char *const *dst,
                           const int *target, int *result, const char *scratch, size_t stride,
                           const int *sres, int n, hipStream_t s);
hipError_t launch_frame_offsets(const int *csize, long long *off, long long *scratch, int n,
                                hipStream_t s);
int frame_scratch_elems(int n);
hipError_t launch_frame_pack(const char *comp, size_t stride, const int *csize,
                             const long long *off, char *frames, int n, hipStream_t s);
// Large inputs as one block (lz4_large.hip): the caller's arrays, and the scratch cut into
// per-slot arrays (slot = input i, slice k at i * nsl + k) by large_scratch_layout.
struct LargeArgs {
    const char *const *src;   // caller's arrays, one entry per input
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    int *result;
    int nblocks, max_src;
    int nsl, nslots;          // slots per input, slots in all
    size_t stride;            // bytes per slot buffer
    const char **s_src;       // the encoder's arguments, one entry per slot ...
    char **s_dst;
    int *s_size, *s_prefix, *s_cap, *s_res, *s_tail;   // ... and its results
    uint32_t *s_off, *s_carry, *s_lead, *s_next;       // offsets kernel -> stitch kernel
    uint32_t *run_pos, *run_anchor;                    // per input, nsl + 1 entries
    char *buf;                // slot buffers (the scratch base before large_scratch_layout)
    int restart;              // R: every R bytes a slice starts without history (0 = never)
    char *index;              // seek index per input at index + i * index_stride (nullable)
    size_t index_stride;
};
int large_slice_size();
// Seek index of an indexed block (layout in include/ape_lz4_gpu.h): little-endian uint32 words
// {magic, nseg, n, c}, then nseg + 1 pairs (ip_j, op_j).
constexpr uint32_t kIxMagic = 0x3158494Cu;   // "LIX1"
// segments of an input of up to max_src bytes with restart points every `restart` bytes
inline long long large_index_segments(int max_src, int restart) {
    if (max_src <= kMaxBlock || restart <= 0) return 1;
    return ((long long)max_src + restart - 1) / restart;
}
inline size_t large_index_size(int max_src, int restart) {
    return ((size_t)(16 + 8 * (large_index_segments(max_src, restart) + 1)) + 15) & ~(size_t)15;
}
struct IndexedArgs {
    const char *const *src;   // caller's arrays, one entry per block
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    const char *index;        // block i's index at index + i * index_stride
    size_t index_stride;
    int max_seg;              // waves per block; a block with more segments gets kErange
    int *result;
    int nblocks;
};
// check launch + one wave per (block, segment) (lz4_decode.hip)
hipError_t launch_decode_indexed(const IndexedArgs &a, hipStream_t s);
// Byte ranges of indexed blocks: the batch dimension is the request.
struct RangeArgs {
    const char *const *src;   // caller's arrays, one entry per block
    const int *src_size;
    const char *index;        // block i's index at index + i * index_stride
    size_t index_stride;
    int max_seg;              // a block with more segments gets kErange
    int nblocks;
    const int *block_of;      // per request from here on; null: request r reads block r
    const int *start, *len;
    char *const *dst;
    const int *dst_cap;
    int *window;              // two ints per request: {where the range begins in dst, need}
    int *result;
    int nreq, waves;          // waves per request
};
// plan launch (one wave per request) + nreq x waves waves over the covering segments
hipError_t launch_decode_range(const RangeArgs &a, hipStream_t s);
size_t large_scratch_layout(int nblocks, int max_src, LargeArgs *out);
hipError_t launch_large(const LargeArgs &a, int accel, hipStream_t s, hipEvent_t *ev = nullptr);
// The same with the high-ratio encoder on the slices: its three kernels run
// over the slot arrays in passes of `pass` slots (1..1024) on the chain and match tables at
// `hc` (pass * kHcSlotBytes bytes).  ev (nullable): 5 + 3 * passes events, recorded before the
// plan, after it, after each pass's chain, search and parse, and after offsets, stitch, index.
// opt: the cost-minimising parse on the slices; `hc` then holds the cost tables
// after the chain and match tables (pass * kHcOptSlotBytes bytes).
inline int large_hc_passes(int nslots, int pass) { return (nslots + pass - 1) / pass; }
hipError_t launch_large_hc(const LargeArgs &a, int depth, void *hc, int pass, hipStream_t s,
                           hipEvent_t *ev = nullptr, bool opt = false);
hipError_t launch_synth(char *out, size_t stride, int n, long long first, int nblocks,
                        int kind, hipStream_t s);

// ---- the LZ4 frame format (lz4_lz4f.hip, include/ape_lz4f.h) ----
// hash[i] = XXH32(src[i][0, max(size[i], 0)), seed): one launch, 16 streams per wave
hipError_t launch_xxh32(const char *const *src, const int *size, uint32_t seed, uint32_t *hash,
                        int n, hipStream_t s);
constexpr int kLfMaxSrc = 0x7E000000;
constexpr int kLfHeaderMax = 15, kLfHeaderMin = 7;   // with and without the content size
// Framed compress: the caller's arrays, and the scratch cut into per-slot arrays (slot = frame
// f, block q at f * bpf + q) by lz4f_compress_layout.
struct LfCompress {
    const char *const *src;   // caller's arrays, one entry per frame
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    int *result;
    int nframes, max_src, flags;
    int bpf, nslots;          // slots per frame, slots in all
    int bsid, ppb;            // block-size ID 4..7; pack pieces per slot (the layouts set both)
    char *buf;                // slot buffers of one block (the scratch base before the layout)
    const char **s_src;       // the encoder's arguments, one entry per slot ...
    char **s_dst;
    int *s_size, *s_cap, *s_res;   // ... and its results
    uint32_t *s_off, *s_hash;      // the block's place in its frame; its checksum
    int *f_total;             // per frame: the frame's bytes, 0 when nothing is to be written
    uint32_t *f_hash;         // per frame: the content checksum
    // the dictionary call alone (include/ape_lz4f_dict.h): one slot per frame
    const unsigned *dict_id;  // per frame (nullable): the ID field is written where it is not 0
    int slot;                 // bytes of a slot buffer: maxSrcSize rounded up to 16
};
constexpr size_t lf_block_bytes(int bsid) { return (size_t)1 << (8 + 2 * bsid); }
// fills out's scratch fields from out->buf (out nullable) for blocks of lf_block_bytes(bsid);
// (size_t)-1 from 2^24 slots on
size_t lz4f_compress_layout(int nframes, int max_src, int bsid, LfCompress *out);
// plan, encode, layout, hash (with a checksum flag), pack: 4 or 5 launches
hipError_t launch_lz4f_compress(const LfCompress &c, hipStream_t s);
// The call with preferences (include/ape_lz4f_prefs.h): plan, the mode's large
// launcher (0: launch_large at acceleration 1; 1, 2: launch_large_hc, lazy or opt, with `depth`,
// the tables at `hc` and `pass` slices per pass) over `a`, whose five arrays are c's slot arrays
// with nblocks = c.nslots and max_src = the block size, then layout, hash, pack.
hipError_t launch_lz4f_prefs_compress(const LfCompress &c, const LargeArgs &a, int mode, int depth,
                                      void *hc, int pass, hipStream_t s);
// One block per frame against a prepared dictionary per frame: the same
// arrays with bpf = 1 and slots of c.slot bytes.  The caller runs the plan, then the mode's
// encoder on the s_ arrays with the frames' objects, then the rest: layout, hash, pack.
size_t lz4f_dict_compress_layout(int nframes, int max_src, LfCompress *out);
hipError_t launch_lz4f_dict_compress_plan(const LfCompress &c, hipStream_t s);
hipError_t launch_lz4f_dict_compress_rest(const LfCompress &c, hipStream_t s);
hipError_t launch_lz4f_info(const char *const *src, const int *src_size, int *info, int nframes,
                            hipStream_t s);
// ten ints per frame: a dictionary ID is no code, [8] whether the frame has the field, [9] the ID
hipError_t launch_lz4f_info_dict(const char *const *src, const int *src_size, int *info,
                                 int nframes, hipStream_t s);
// Framed decode: what the plan launch found out about a frame ...
struct LfFrame {
    int code, nb;             // the header stage's code (0: go on); blocks
    uint32_t bmax, flg;       // block maximum; FLG
    uint32_t content;         // content size, with that bit in flg
    uint32_t want, got;       // content checksum: the frame's, and the output's
    int dsize;                // the dictionary call alone: bytes of the frame's dictionary, 0 =
                              // none (the other calls never write or read it)
};
static_assert(sizeof(LfFrame) % 16 == 0, "scratch regions");
// ... and the per-slot arrays (slot = block q of frame f at q * nframes + f): the arguments of
// launch_decode (_a: blocks of block-independent frames) and launch_decode_chain (_b: blocks of
// linked frames, with the output before them as dictionary), and what the other launches need.
// One struct for both framed decodes.  `placed` is the call of
// include/ape_lz4f_placed.h: `cap` then holds a block's measured size once the
// place launch has run, and the last three members are what the sizer needs besides; the call
// of include/ape_lz4f.h leaves them null.
struct LfDecode {
    const char *const *src;   // caller's arrays, one entry per frame
    const int *src_size;
    char *const *dst;
    const int *dst_cap;
    int *result;
    int nframes, max_blocks;
    bool verify, no_linked;   // decompress flags bit 0 clear; bit 1 set
    const char *zero;         // 16 bytes, the first 0 (the scratch base before the layout)
    LfFrame *frame;
    const char **src_a, **src_b, **dict, **data;   // data: the block's bytes in the frame
    char **out;               // where the block's output goes
    int *size_a, *cap_a, *res_a, *size_b, *cap_b, *res_b, *dict_size;
    int *size, *kind, *cap;   // the block's bytes in the frame; kLf...; its room in dst
    uint32_t *want, *got;     // block checksum: the frame's, and the bytes'
    bool placed;              // (the host's choice of kernels; no kernel reads it)
    int *cap_s, *res_s;       // the sizer's capacity (the block maximum; 0: not sized) and result
    int *total;               // per frame: the sum of the measured sizes, once the frame is placed
    // the dictionary call alone (include/ape_lz4f_dict.h): the caller's table,
    // key t_id[k] -> dictionary t_dict[k] of t_size[k] bytes
    bool dicts;               // (the host's choice of kernels; no kernel reads it)
    const unsigned *t_id;
    const char *const *t_dict;
    const int *t_size;
    int ntable;
};
// result[i] = what decompress_safe (with a.dict_size: _usingDict) would return for block i, by
// a dry run of the decoder's parse: a.src, a.src_size, a.dst_cap, a.dict_size (nullable) and
// a.result are used, and nothing but a.result is written (lz4_decode.hip)
hipError_t launch_decode_size(const BlockArgs &a, hipStream_t s);
// fills out's scratch fields from out->zero (out nullable); (size_t)-1 from 2^24 slots on.
// placed: the same regions, then the sizer's two arrays per slot and the totals per frame
size_t lz4f_decode_layout(int nframes, int max_blocks, bool placed, LfDecode *out);
// plan, [placed: size, place,] stored copies, decode, chained decode (unless no_linked), hash
// (when verify), finish: 4 to 6 launches, 6 to 8 when placed; with d.dicts the same launches, the
// plan looking each frame's dictionary up in the table
hipError_t launch_lz4f_decode(const LfDecode &d, hipStream_t s);

}  // namespace apelz4
