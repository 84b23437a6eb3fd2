// Map fusion: one averaged point per occupied voxel (sp_map_fuse; the contract is in include/sp_hip.h).
//
// A hash table in the caller's scratch: S slots of 64 bytes, S the smallest power of two >= 2 Q, open addressing with linear probing from
// a splitmix64 finaliser of the voxel's key (the keys of one surface are neighbours: the identity would cluster).  One slot = the key,
// the lowest member row, the member count and the six integer sums: everything a point adds to lies in ONE 64-byte line.
//   k_fuse_init    the table: key = all ones (no key: keys use 63 bits), first = INT_MAX, everything else 0; 8-byte stores, coalesced
//   k_fuse_insert  one lane per point: its key in float64 (every operation rounded on its own: contraction is off for this file), its
//                  slot found or claimed by a 64-bit atomicCAS after a relaxed load (most points find their key already there); the slot
//                  number is remembered per point (-1: dropped).  Then the wave merges: a run of neighbouring lanes with one slot sums
//                  its seven integers over the lanes (a segmented scan by lane swaps, skipped when no lane continues a run) and only
//                  its last lane adds -- atomicMin of the run's first row into `first` (skipped when a load shows a lower row: the
//                  atomic decides) and integer atomicAdd into n, S[3], C[3].  Every lane of a wave hits another 64-byte line, the slow
//                  shape for atomics, so their number is what the call costs: with 16 points per voxel the merge halves the call's
//                  time, with 64 it takes it to 0.28, and a map without runs pays nothing measurable (profiles/map_fuse_wave_merge_ab.txt)
//   k_fuse_count   a point is its voxel's representative iff its row is the slot's `first`; per 256-row block their number (block_rank)
//   k_fuse_scan    one workgroup: the exclusive prefix sum of the block counts, in place (block_count_scan); the total is n_fused
//   k_fuse_emit    representative i writes fused row rank(i) = block prefix + its place in the block from its slot, and the rank back
//                  into the slot (over n, which only the representative reads)
//   k_fuse_label   label[i] = the rank in point i's slot
// The ordered compaction of sp_depth_lift, from the same pieces (sp_map_device.h): no workgroup waits on another, no flags, nothing
// spins.  Every loop is bounded: a probe visits at most S slots and cannot exhaust them (at most Q < S keys are ever claimed); should it
// ever, the point is dropped, not looped on.
// All sums are integers: any order gives the same bits.
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

struct FuseSlot {
    unsigned long long key;            // FUSE_EMPTY until claimed
    int32_t first;                     // lowest member row
    int32_t n;                         // member count; after k_fuse_emit the voxel's fused row
    unsigned long long S[3];           // sums of the sub-voxel positions (<= 2^28 x 65535 < 2^44)
    unsigned long long C[3];           // sums of the 8-bit colours
};
static_assert(sizeof(FuseSlot) == 64, "one slot is one 64-byte line");

// (the empty key, the hash, the key of three cells and the probe loop are sp_map_device.h's: sp_nearest.hip builds its table from them too)

// one axis of a point: false = dropped; else the biased voxel index (0 .. 2^21 - 1) and the sub-voxel position (0 .. 65535)
__device__ __forceinline__ bool fuse_axis(float p, double o, double voxel, unsigned long long& cell, unsigned long long& sub) {
    const double q = ((double)p - o) / voxel;
    const double g = floor(q);
    if (!(g >= -FUSE_HALF_RANGE && g <= FUSE_HALF_RANGE - 1.0)) return false;        // NaN and +-inf fail; tested before the conversion
    const double f = q - g;
    const int s = (int)(f * 65536.0);
    cell = (unsigned long long)((long long)g + 1048576LL);
    sub = (unsigned long long)(s < 65535 ? s : 65535);
    return true;
}

// grid ceil(8 S / 256): word w of the table; words 0 and 1 of a slot are the key and (first, n)
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_init(unsigned long long* __restrict__ words, long long n_words) {
    const long long w = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    const int part = (int)(w & 7);
    words[w] = part == 0 ? FUSE_EMPTY : (part == 1 ? 0x000000007fffffffull : 0ull);
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_insert(const float* __restrict__ points, const float* __restrict__ colours, int Q,
                                                          float voxel, float ox, float oy, float oz, FuseSlot* __restrict__ table,
                                                          unsigned int mask, int32_t* __restrict__ slot_of) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const bool in = i < Q;
    const long long at_i = in ? i : 0;                     // (lanes beyond Q stay for the wave's exchanges; they read row 0 and add nothing)
    const double vx = (double)voxel;
    unsigned long long cx = 0, cy = 0, cz = 0, s[3] = {0, 0, 0};
    const bool kept = in && fuse_axis(points[3 * at_i], (double)ox, vx, cx, s[0]) && fuse_axis(points[3 * at_i + 1], (double)oy, vx, cy, s[1]) &&
                      fuse_axis(points[3 * at_i + 2], (double)oz, vx, cz, s[2]);
    int32_t slot = -1;
    if (kept) slot = fuse_claim(table, mask, fuse_key(cx, cy, cz));
    if (in) slot_of[i] = slot;
    // what this point adds: 1, its three sub-voxel positions, its three 8-bit colours
    uint32_t v[7] = {1u, (uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[2], 0u, 0u, 0u};
    if (colours && slot >= 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[4 + ch] = colour_u8(colours[3 * at_i + ch]);
    }
    int32_t row = (int32_t)i;
    // Map points arrive in table order, so neighbouring lanes often share a voxel: a run of lanes with one slot adds its integer total
    // once, from its last lane (at most 64 x 65535 per sum: 32 bits), with the row of its first lane.  Integers: no bit changes.
    const int lane = threadIdx.x & 63;
    const int32_t before = __shfl_up(slot, 1, 64);
    const bool head = lane == 0 || slot < 0 || before != slot;
    const unsigned long long heads = __ballot(head);
    if (~heads) {                                          // (wave-uniform: some lane continues a run)
        const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));              // the head at or below this lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const bool take = lane - off >= start;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const uint32_t up = (uint32_t)__shfl_up((int)v[k], off, 64);
                if (take) v[k] += up;
            }
        }
        row -= lane - start;
        if (lane < 63 && !((heads >> (lane + 1)) & 1ull)) slot = -1;                 // not the last lane of its run: adds nothing
    }
    if (slot < 0) return;
    FuseSlot* t = table + slot;
    if (__hip_atomic_load(&t->first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(&t->first, row);
    atomicAdd(&t->n, (int32_t)v[0]);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&t->S[a], (unsigned long long)v[1 + a]);
    if (colours) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) atomicAdd(&t->C[ch], (unsigned long long)v[4 + ch]);
    }
}

__device__ __forceinline__ bool fuse_is_first(const FuseSlot* __restrict__ table, const int32_t* __restrict__ slot_of, long long i, int Q,
                                              int32_t& slot) {
    slot = i < Q ? slot_of[i] : -1;
    return slot >= 0 && table[slot].first == (int32_t)i;
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_count(const FuseSlot* __restrict__ table, const int32_t* __restrict__ slot_of, int Q,
                                                         int32_t* __restrict__ block_counts) {
    __shared__ int wc[SP_WAVES];
    int32_t slot;
    const bool rep = fuse_is_first(table, slot_of, (long long)blockIdx.x * SP_BLOCK + threadIdx.x, Q, slot);
    const int count = block_rank(rep, wc).count;
    if (threadIdx.x == 0) block_counts[blockIdx.x] = count;
}

// one workgroup: bc[n] becomes its exclusive prefix sum, n_fused[0] the total
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_scan(int32_t* __restrict__ bc, int n, long long* __restrict__ n_fused) {
    __shared__ long long part[SP_BLOCK];
    const long long total = block_count_scan(bc, n, part, [](long long, long long) {});
    if (threadIdx.x == 0) n_fused[0] = total;
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_emit(FuseSlot* __restrict__ table, const int32_t* __restrict__ slot_of, int Q,
                                                        const int32_t* __restrict__ block_offsets, float voxel, float ox, float oy, float oz,
                                                        float* __restrict__ out_points, float* __restrict__ out_colours,
                                                        int32_t* __restrict__ count, int32_t* __restrict__ first) {
    __shared__ int wc[SP_WAVES];
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    int32_t slot;
    const bool rep = fuse_is_first(table, slot_of, i, Q, slot);
    const int rank = block_rank(rep, wc).rank;
    if (!rep) return;
    const int32_t row = block_offsets[blockIdx.x] + rank;
    FuseSlot* t = table + slot;
    const unsigned long long key = t->key;
    const int32_t n = t->n;
    const double nd = (double)n, vx = (double)voxel;
    const double o[3] = {(double)ox, (double)oy, (double)oz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double g = (double)((long long)((key >> (42 - 21 * a)) & 0x1fffffull) - 1048576LL);
        const double m = (double)t->S[a] / nd;
        const double c = (m + 0.5) / 65536.0;
        out_points[3 * (size_t)row + a] = (float)((g + c) * vx + o[a]);
    }
    if (out_colours) {
        const double den = 255.0 * nd;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out_colours[3 * (size_t)row + ch] = (float)((double)t->C[ch] / den);
    }
    count[row] = n;
    first[row] = (int32_t)i;
    t->n = row;                                            // (read by k_fuse_label; nobody else reads n in this launch)
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_fuse_label(const FuseSlot* __restrict__ table, const int32_t* __restrict__ slot_of, int Q,
                                                         int32_t* __restrict__ label) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= Q) return;
    const int32_t slot = slot_of[i];
    label[i] = slot < 0 ? -1 : table[slot].n;
}

struct FuseLayout { long long slots, slot_units, row_units, block_units, blocks; };

// Q in 1 .. SP_MAP_FUSE_MAX_POINTS
FuseLayout fuse_layout(long long Q) {
    FuseLayout l;
    l.slots = 2;
    while (l.slots < 2 * Q) l.slots <<= 1;
    l.blocks = (Q + SP_BLOCK - 1) / SP_BLOCK;
    l.slot_units = l.slots;                                // 64 bytes each
    l.row_units = (Q + 15) / 16;                           // Q int32
    l.block_units = (l.blocks + 15) / 16;                  // ceil(Q / 256) int32
    return l;
}

}  // namespace

extern "C" {

int sp_map_fuse_scratch_units(long long Q) {
    if (Q <= 0) return SP_EINVAL;
    if (Q > SP_MAP_FUSE_MAX_POINTS) return SP_ELIMIT;
    const FuseLayout l = fuse_layout(Q);
    return (int)(l.slot_units + l.row_units + l.block_units);                        // <= 2^29 + 2^24 + 2^16
}

int sp_map_fuse(const float* points, const float* colours, long long Q, float voxel, float ox, float oy, float oz, void* scratch,
                float* out_points, float* out_colours, int32_t* count, int32_t* first, int32_t* label, long long* n_fused, void* stream) {
    if (!points || !scratch || !out_points || !count || !first || !label || !n_fused || ((colours == nullptr) != (out_colours == nullptr)))
        return SP_EINVAL;
    if (Q <= 0 || !(voxel > 0.f && voxel < HUGE_VALF)) return SP_EINVAL;
    if (!(fabsf(ox) < HUGE_VALF && fabsf(oy) < HUGE_VALF && fabsf(oz) < HUGE_VALF)) return SP_EINVAL;
    if (Q > SP_MAP_FUSE_MAX_POINTS) return SP_ELIMIT;
    const FuseLayout l = fuse_layout(Q);
    FuseSlot* table = static_cast<FuseSlot*>(scratch);
    int32_t* slot_of = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + 64 * (size_t)l.slot_units);
    int32_t* block_counts = slot_of + 16 * (size_t)l.row_units;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)l.blocks;
    const long long n_words = 8 * l.slots;
    hipLaunchKernelGGL(k_fuse_init, dim3((unsigned)((n_words + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s,
                       reinterpret_cast<unsigned long long*>(scratch), n_words);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_insert, dim3(grid), dim3(SP_BLOCK), 0, s, points, colours, (int)Q, voxel, ox, oy, oz, table,
                       (unsigned int)(l.slots - 1), slot_of);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_count, dim3(grid), dim3(SP_BLOCK), 0, s, table, slot_of, (int)Q, block_counts);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_scan, dim3(1), dim3(SP_BLOCK), 0, s, block_counts, (int)l.blocks, n_fused);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_emit, dim3(grid), dim3(SP_BLOCK), 0, s, table, slot_of, (int)Q, block_counts, voxel, ox, oy, oz, out_points,
                       out_colours, count, first);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fuse_label, dim3(grid), dim3(SP_BLOCK), 0, s, table, slot_of, (int)Q, label);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
