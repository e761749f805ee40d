// lz4_dict_train.hip -- MI355X (gfx950): train a dictionary from a batch of sample messages.
//
// APE_LZ4_dict_train_dev builds the dictionary the prepared-dictionary calls start from.  The
// rule is tests/dicttrainmodel.py's, byte for byte (constants and the scratch
// layout in lz4_gpu_internal.h): count the table index of every 8-byte substring of the
// samples, then in E = capacity / segment rounds score a share of the candidate segments
// ("slots") by the counts of their DISTINCT indices, take the best of the round, lay it before
// the earlier picks and zero the counts it covers, so that later rounds pay for new material.
//
// Launches, all stream-ordered and decided on the host:
//   zero    the table and the state
//   count   one wave per (sample, 1024 positions): a u32 no-return global add per position.
//           Integer adds commute, so the table does not depend on the order of arrival.
//   score   per round: one wave per slot, grid-stride over the round's range, substrings across
//           lanes.  The set of distinct indices is an open-addressed table in LDS, one per wave
//           (at most half full); a sum over a set does not depend on the insertion order.  Each
//           workgroup leaves its best (highest score, then lowest slot) as one partial.
//   pick    per round, one workgroup: the best of the partials, its bytes copied, its counts
//           zeroed with plain stores, the state advanced.
//   finish  the zero fill before the picks, and d_info.
// A round without slots (fewer slots than rounds) has no launches.
//
// Reads: d_sampleSize[0, nsamples), d_samples[i] and d_samples[i][0, size) of every sample with
// 0 < size <= max_sample -- every 8-byte window is one load that lies inside the sample, at any
// alignment.  Writes: d_dict[0, capacity), d_info[0, 4), the scratch.  Every scratch byte that
// is read was written before in the same call.
#include "lz4_gpu_internal.h"

namespace apelz4 {

namespace {

constexpr int kDtThreads = 256, kDtWaves = kDtThreads / 64;
constexpr int kDtChunk = 1024;            // positions per wave of the count pass
constexpr int kDtCountGroups = 4096;      // count workgroups at most (grid-stride): 16 per CU
constexpr int kDtSetMax = 2048;           // set entries per wave: >= 2 x (kDtMaxSeg - 7)
constexpr uint32_t kDtEmpty = 0xFFFFFFFFu;   // (no index: they are below 2^kDtBits)
constexpr uint32_t kDtNoSlot = 0xFFFFFFFFu;
static_assert(kDtSetMax >= 2 * (kDtMaxSeg - kDtSub + 1), "the set stays at most half full");
static_assert(kDtSub == 8, "one 8-byte load per substring");

__device__ __forceinline__ uint32_t dt_index(uint2 x) {
    const uint64_t v = (uint64_t)x.x | ((uint64_t)x.y << 32);
    return (uint32_t)((v * kDtPrime) >> (64 - kDtBits));
}

// bytes of sample i that count: 0 for a negative size, -1 for a sample that is ignored
__device__ __forceinline__ int dt_size(const int *size, int i, int max_sample) {
    const int z = size[i];
    return z > max_sample ? -1 : z < 0 ? 0 : z;
}

__device__ __forceinline__ bool dt_better(unsigned long long score, uint32_t slot,
                                          unsigned long long best, uint32_t best_slot) {
    return score > best || (score == best && score != 0 && slot < best_slot);
}

__global__ void __launch_bounds__(kDtThreads)
lz4_dict_train_zero_kernel(uint32_t *freq, DtState *state) {
    const uint32_t g = blockIdx.x * kDtThreads + threadIdx.x;   // one 16-byte piece each
    ((uint4 *)freq)[g] = make_uint4(0, 0, 0, 0);
    if (g == 0) *(uint4 *)state = make_uint4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(kDtThreads)
lz4_dict_train_count_kernel(const char *const *samples, const int *size, int max_sample,
                            int chunks, long long units, uint32_t *freq, DtState *state) {
    const int lane = lane_id();
    const long long nwaves = (long long)gridDim.x * kDtWaves;
    for (long long u = (long long)blockIdx.x * kDtWaves + (threadIdx.x >> 6); u < units;
         u += nwaves) {
        const int i = (int)(u / chunks), ch = (int)(u % chunks);
        const int z = dt_size(size, i, max_sample);
        if (z < 0 && ch == 0 && lane == 0) atomicAdd(&state->ignored, 1u);
        const long long first = (long long)ch * kDtChunk;
        const long long npos = (long long)z - (kDtSub - 1);     // positions p with p + 8 <= z
        if (first >= npos) continue;
        const uint32_t end = (uint32_t)(npos - first < kDtChunk ? npos : first + kDtChunk);
        gcu8 *s = (gcu8 *)samples[i];
        for (uint32_t p = (uint32_t)first + (uint32_t)lane; p < end; p += 64u)
            atomicAdd(&freq[dt_index(gload8(s + p))], 1u);
    }
}

// the segment of slot c: sample, first byte, bytes (n < kDtSub: an empty slot)
struct DtSeg {
    int i, at, n;
};
__device__ __forceinline__ DtSeg dt_segment(uint32_t c, const int *size, int max_sample,
                                            int segment, int per_sample) {
    DtSeg g;
    g.i = (int)(c / (uint32_t)per_sample);
    g.at = (int)(c % (uint32_t)per_sample) * (segment / 4);   // < max_sample + segment / 4
    const long long left = (long long)dt_size(size, g.i, max_sample) - g.at;
    g.n = (int)(left < 0 ? 0 : left < segment ? left : segment);
    return g;
}

__global__ void __launch_bounds__(kDtThreads)
lz4_dict_train_score_kernel(const char *const *samples, const int *size, int max_sample,
                            int segment, int per_sample, uint32_t lo, uint32_t hi,
                            uint32_t set_size, const uint32_t *freq, DtPartial *partial) {
    __shared__ uint32_t set[kDtWaves][kDtSetMax];
    __shared__ unsigned long long w_score[kDtWaves];
    __shared__ uint32_t w_slot[kDtWaves];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t *mine = set[wave];
    const uint32_t mask = set_size - 1u;
    const int shift = 32 - (31 - __builtin_clz(set_size));
    unsigned long long best = 0;
    uint32_t best_slot = kDtNoSlot;
    const uint64_t nwaves = (uint64_t)gridDim.x * kDtWaves;
    for (uint64_t c64 = (uint64_t)lo + blockIdx.x * kDtWaves + wave; c64 < hi; c64 += nwaves) {
        const uint32_t c = (uint32_t)c64;
        const DtSeg g = dt_segment(c, size, max_sample, segment, per_sample);
        if (g.n < kDtSub) continue;   // (wave-uniform)
        for (uint32_t t = (uint32_t)lane; t < set_size; t += 64u) mine[t] = kDtEmpty;
        __builtin_amdgcn_wave_barrier();
        gcu8 *s = (gcu8 *)samples[g.i] + g.at;
        unsigned long long sum = 0;
        for (int q = lane; q < g.n - (kDtSub - 1); q += 64) {
            const uint32_t idx = dt_index(gload8(s + q));
            uint32_t h = (idx * 2654435761u) >> shift;
            for (;;) {
                const uint32_t old = atomicCAS(&mine[h], kDtEmpty, idx);
                if (old == kDtEmpty) sum += freq[idx];   // the first of its index
                if (old == kDtEmpty || old == idx) break;
                h = (h + 1u) & mask;
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (dt_better(sum, c, best, best_slot)) {
            best = sum;
            best_slot = c;
        }
    }
    if (lane == 0) {
        w_score[wave] = best;
        w_slot[wave] = best_slot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kDtWaves; w++)
            if (dt_better(w_score[w], w_slot[w], best, best_slot)) {
                best = w_score[w];
                best_slot = w_slot[w];
            }
        DtPartial p;
        p.score = best;
        p.slot = best_slot;
        p.zero = 0u;
        partial[blockIdx.x] = p;
    }
}

__global__ void __launch_bounds__(kDtThreads)
lz4_dict_train_pick_kernel(const char *const *samples, const int *size, int max_sample,
                           int segment, int per_sample, const DtPartial *partial, int groups,
                           char *dict, int capacity, uint32_t *freq, DtState *state) {
    __shared__ unsigned long long r_score[kDtThreads];
    __shared__ uint32_t r_slot[kDtThreads];
    const int tid = threadIdx.x;
    unsigned long long best = 0;
    uint32_t best_slot = kDtNoSlot;
    for (int g = tid; g < groups; g += kDtThreads) {
        const DtPartial p = partial[g];
        if (dt_better(p.score, p.slot, best, best_slot)) {
            best = p.score;
            best_slot = p.slot;
        }
    }
    r_score[tid] = best;
    r_slot[tid] = best_slot;
    __syncthreads();
    for (int half = kDtThreads / 2; half >= 1; half >>= 1) {
        if (tid < half && dt_better(r_score[tid + half], r_slot[tid + half], r_score[tid],
                                    r_slot[tid])) {
            r_score[tid] = r_score[tid + half];
            r_slot[tid] = r_slot[tid + half];
        }
        __syncthreads();
    }
    if (r_score[0] == 0) return;   // nothing left to gain in this round's range
    const DtSeg g = dt_segment(r_slot[0], size, max_sample, segment, per_sample);
    const uint32_t used = state->used;
    // (state and partials lie in the caller's scratch: should two calls be made to share one,
    // the copy still stays inside d_dict)
    if (g.n < kDtSub || used + (uint32_t)g.n > (uint32_t)capacity) return;
    __syncthreads();               // every thread has read the state
    gcu8 *s = (gcu8 *)samples[g.i] + g.at;
    gu8 *d = (gu8 *)dict + ((uint32_t)capacity - used - (uint32_t)g.n);
    for (int b = tid; b < g.n; b += kDtThreads) d[b] = s[b];
    for (int q = tid; q < g.n - (kDtSub - 1); q += kDtThreads) freq[dt_index(gload8(s + q))] = 0u;
    if (tid == 0) {
        state->used = used + (uint32_t)g.n;
        state->picks += 1u;
    }
}

__global__ void __launch_bounds__(kDtThreads)
lz4_dict_train_finish_kernel(char *dict, int capacity, const DtState *state, int *info) {
    const DtState st = *state;
    const uint32_t fill = st.used <= (uint32_t)capacity ? (uint32_t)capacity - st.used : 0u;
    const uint32_t g = blockIdx.x * kDtThreads + threadIdx.x;
    for (uint32_t b = g; b < fill; b += gridDim.x * kDtThreads) ((gu8 *)dict)[b] = 0;
    if (g == 0) {
        info[0] = (int)st.used;
        info[1] = (int)st.picks;
        info[2] = (int)st.ignored;
        info[3] = 0;
    }
}

}  // namespace

hipError_t launch_dict_train(const DtArgs &a, hipStream_t s) {
    constexpr uint32_t kPieces = kDtTable * sizeof(uint32_t) / 16u;
    static_assert(kPieces % kDtThreads == 0, "the zero launch covers the table exactly");
    hipLaunchKernelGGL(lz4_dict_train_zero_kernel, dim3(kPieces / kDtThreads), dim3(kDtThreads), 0,
                       s, a.freq, a.state);
    const int per_sample = (int)dt_slots_per_sample(a.max_sample, a.segment);
    const long long M = dt_slots(a.nsamples, a.max_sample, a.segment);
    if (a.nsamples > 0) {
        const int chunks = (a.max_sample - (kDtSub - 1) + kDtChunk - 1) / kDtChunk;
        const long long units = (long long)a.nsamples * chunks;
        const long long groups = (units + kDtWaves - 1) / kDtWaves;
        hipLaunchKernelGGL(lz4_dict_train_count_kernel,
                           dim3((unsigned)(groups < kDtCountGroups ? groups : kDtCountGroups)),
                           dim3(kDtThreads), 0, s, a.samples, a.size, a.max_sample, chunks, units,
                           a.freq, a.state);
    }
    // the set of a slot: a power of two, at least twice the segment's substrings
    uint32_t set_size = 64;
    while (set_size < 2u * (uint32_t)(a.segment - (kDtSub - 1))) set_size *= 2;
    const int rounds = a.capacity / a.segment;
    for (long long e = 0; e < rounds; e++) {
        const long long lo = e * M / rounds, hi = (e + 1) * M / rounds;
        if (hi <= lo) continue;
        const int groups = dt_groups(hi - lo);
        hipLaunchKernelGGL(lz4_dict_train_score_kernel, dim3(groups), dim3(kDtThreads), 0, s,
                           a.samples, a.size, a.max_sample, a.segment, per_sample, (uint32_t)lo,
                           (uint32_t)hi, set_size, a.freq, a.partial);
        hipLaunchKernelGGL(lz4_dict_train_pick_kernel, dim3(1), dim3(kDtThreads), 0, s, a.samples,
                           a.size, a.max_sample, a.segment, per_sample, a.partial, groups, a.dict,
                           a.capacity, a.freq, a.state);
    }
    hipLaunchKernelGGL(lz4_dict_train_finish_kernel, dim3(4), dim3(kDtThreads), 0, s, a.dict,
                       a.capacity, a.state, a.info);
    return hipGetLastError();
}

}  // namespace apelz4
