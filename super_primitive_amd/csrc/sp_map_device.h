// Device-side pieces shared by the map kernels (sp_views.hip, sp_results.hip, sp_fuse.hip): each idiom has its one definition here.
#pragma once
#include "sp_device.h"

// ---- depth-buffer keys ---------------------------------------------------------------------------------------------------------------
// One pixel of a depth buffer is one 64-bit word, 0 while nothing landed, decided by atomicMax (integer maxima commute: two runs give
// the same bits); id + 1 keeps every key above 0 (ids stay below 2^31 - 1).
//   nearest     ~bits(float32 z) << 32 | (id + 1), for z > 0 only: a positive float has sign bit 0 and its exponent above its mantissa,
//               so its bits order as unsigned integers exactly as the floats do; the complement turns the smallest z into the largest
//               key, and equal float32 z goes to the highest id
//   highest id  (id + 1) << 32 | bits(float32 z): NumPy's repeated-index assignment; z only rides along, any value may be stored
__device__ __forceinline__ unsigned long long key_nearest(float z, uint32_t id) {
    return ((unsigned long long)(~__float_as_uint(z)) << 32) | (unsigned long long)(id + 1u);
}
__device__ __forceinline__ unsigned long long key_highest_id(float z, uint32_t id) {
    return ((unsigned long long)(id + 1u) << 32) | (unsigned long long)__float_as_uint(z);
}
// the winner of a pixel: its id, or -1 for the empty word (0 - 1 wraps), and its float32 z, or 0
__device__ __forceinline__ int key_nearest_id(unsigned long long k) { return (int)((uint32_t)(k & 0xffffffffull) - 1u); }
__device__ __forceinline__ float key_nearest_z(unsigned long long k) { return k ? __uint_as_float(~(uint32_t)(k >> 32)) : 0.f; }
__device__ __forceinline__ int key_highest_id_id(unsigned long long k) { return (int)((uint32_t)(k >> 32) - 1u); }
__device__ __forceinline__ float key_highest_id_z(unsigned long long k) { return __uint_as_float((uint32_t)(k & 0xffffffffull)); }

// one 64-bit atomicMax, no return value; a relaxed load first skips a key that already loses (the race is benign: the atomic decides)
__device__ __forceinline__ void key_offer(unsigned long long* slot, unsigned long long key) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) return;
    atomicMax(slot, key);
}

// ---- ordered compaction: ballot per 256-row block, one workgroup scans the block counts, every block writes at block offset + rank ---
struct BlockRank { int rank, count; };                     // the kept lanes before this one in its workgroup; all of the workgroup's
// EVERY thread of the block must call it (there is a barrier inside), once per kernel; wc: SP_WAVES ints of LDS
__device__ __forceinline__ BlockRank block_rank(bool keep, int* wc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wc[wave] = __popcll(ballot);
    __syncthreads();
    BlockRank r = {(int)__popcll(ballot & ((1ull << lane) - 1ull)), (wc[0] + wc[1]) + (wc[2] + wc[3])};
    for (int w = 0; w < wave; ++w) r.rank += wc[w];
    return r;
}

// One workgroup of SP_BLOCK threads, all of which must call it: bc[n] becomes its exclusive prefix sum (running sums in int64, stored
// as int32) and every thread gets the total.  Thread t takes the blocks t per .. t per + per - 1; at_block(j, prefix) is called once
// for every block j, by the thread that owns it, with the prefix stored there.  part: SP_BLOCK long longs of LDS.
template <class AtBlock>
__device__ __forceinline__ long long block_count_scan(int32_t* __restrict__ bc, int n, long long* part, AtBlock at_block) {
    const int tid = threadIdx.x;
    const int per = (n + SP_BLOCK - 1) / SP_BLOCK;
    const long long j0 = (long long)tid * per;
    const long long j1 = j0 + per < n ? j0 + per : n;
    long long s = 0;
    for (long long j = j0; j < j1; ++j) s += bc[j];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < SP_BLOCK; ++t) { run += part[t]; part[t] = run; }    // inclusive over the threads' ranges
    }
    __syncthreads();
    long long run = part[tid] - s;
    for (long long j = j0; j < j1; ++j) {
        const int c = bc[j];
        bc[j] = (int32_t)run;
        at_block(j, run);
        run += c;
    }
    return part[SP_BLOCK - 1];
}

// ---- the keyframe walk: a workgroup belongs to ONE keyframe, the last record whose first_block is at or before it (uniform: scalar loads)
__device__ __forceinline__ int keyframe_of_block(const SpMapKeyframe* __restrict__ kfs, int n_kf, int block) {
    int lo = 0, hi = n_kf;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (kfs[mid].first_block <= block) lo = mid; else hi = mid; }
    return lo;
}
