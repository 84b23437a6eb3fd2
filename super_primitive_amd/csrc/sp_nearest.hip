// Map distances: for every point of one cloud its nearest point of another within a radius, and the number of points within it
// (sp_cloud_grid_build, sp_cloud_grid_nearest; the contract is in include/sp_hip.h).
//
// A grid of cells of side r (1 + 2^-10) over the reference cloud, hashed: S slots of 16 bytes (the cell's key, where its members start
// and how many there are), S the smallest power of two >= 2 Q, open addressing with linear probing -- the table of sp_fuse.hip, from
// the same pieces (sp_map_device.h: the key of three cells, the hash, the claiming probe loop).  The members of one cell lie side by
// side: one 16-byte record {x, y, z, row} each, so a query fetches a member with ONE dwordx4 load and never touches the cloud itself.
//   k_grid_init     the header (r2, cell, origin, mask, Q: what the query reads its parameters from) and the table: key = all ones,
//                   start = count = 0
//   k_grid_count    one lane per point: its cell in float64 (every operation rounded on its own: contraction is off for this file),
//                   its slot found or claimed, the slot's count raised by one; the slot number is remembered per point (-1: out of range)
//   k_grid_sums     per 256 slots the sum of their counts
//   k_grid_scan     one workgroup: the exclusive prefix sum of those sums, in place (block_count_scan)
//   k_grid_starts   slot s gets start = the sum of its block + the counts before it in its block (a scan by lane swaps)
//   k_grid_scatter  one lane per point: its place is what an atomic add of 1 to its slot's start returns; it writes its record there.
//                   `start` is the cursor, so AFTER this pass it holds the cell's END: the members are end - count .. end - 1
//   k_grid_nearest  one lane per query: the 27 cells around its own, each looked up (a 16-byte load per probe, until the key or an
//                   empty slot), each cell's records walked; the decision is made in float64 exactly as the contract writes it
//                   (grid_nearest_walk in sp_map_device.h, with the layout of the scratch: sp_register.hip walks the same way)
// The order in which the scatter stores a cell's members differs from run to run; a minimum over (d2, row) and a count do not depend
// on it.  No workgroup waits on another, no flags, nothing spins.  Every loop is bounded: a probe visits at most S slots, a walk at
// most `count` records.
// A float32 pre-test of the distance is NOT made: per member it would cost eight float32 operations, a compare and a branch to skip
// eleven float64 operations, and the walk waits for its 16-byte loads either way (profiles/map_nearest.txt has the bytes per query).
// Two forms with more loads in flight per lane were measured and not kept (DESIGN.md section 4 "Map distances"): two records per step
// of the walk is 9 - 14 % faster at 64 neighbours per query and 7 - 9 % slower at 16 (profiles/map_nearest_walk_ab.txt); the first
// probes of the three cells of a column issued together is 16 - 18 % slower where the lookups bind.
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

struct BlockScan { int before, total; };                   // the sum over the threads before this one in its workgroup; over all of them
// EVERY thread of the block must call it (there is a barrier inside), once per kernel; wc: SP_WAVES ints of LDS
__device__ __forceinline__ BlockScan block_scan(int v, int* wc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wc[wave] = inc;
    __syncthreads();
    BlockScan r = {inc - v, (wc[0] + wc[1]) + (wc[2] + wc[3])};
    for (int w = 0; w < wave; ++w) r.before += wc[w];
    return r;
}

// grid ceil(2 S / 256): word w of the table (word 0 of a slot is the key, word 1 start and count); thread 0 writes the header
__global__ __launch_bounds__(SP_BLOCK) void k_grid_init(GridHeader* __restrict__ header, unsigned long long* __restrict__ words, long long n_words,
                                                        double r2, double cell, double ox, double oy, double oz, unsigned int mask, int Q) {
    const long long w = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (w == 0) {
        header->r2 = r2; header->cell = cell; header->o[0] = ox; header->o[1] = oy; header->o[2] = oz;
        header->mask = mask; header->Q = Q; header->pad_[0] = header->pad_[1] = 0;
    }
    if (w < n_words) words[w] = (w & 1) ? 0ull : FUSE_EMPTY;
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_grid_count(const float* __restrict__ points, int Q, double cell, double ox, double oy, double oz,
                                                         GridSlot* __restrict__ table, unsigned int mask, int32_t* __restrict__ slot_of) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= Q) return;
    unsigned long long cx = 0, cy = 0, cz = 0;
    int32_t slot = -1;
    if (grid_axis(points[3 * i], ox, cell, cx) && grid_axis(points[3 * i + 1], oy, cell, cy) && grid_axis(points[3 * i + 2], oz, cell, cz))
        slot = fuse_claim(table, mask, fuse_key(cx, cy, cz));
    slot_of[i] = slot;
    if (slot >= 0) atomicAdd(&table[slot].count, 1);
}

// grid ceil(S / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_grid_sums(const GridSlot* __restrict__ table, long long S, int32_t* __restrict__ block_sums) {
    __shared__ int wc[SP_WAVES];
    const long long s = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const int total = block_scan(s < S ? table[s].count : 0, wc).total;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: bs[n] becomes its exclusive prefix sum
__global__ __launch_bounds__(SP_BLOCK) void k_grid_scan(int32_t* __restrict__ bs, int n) {
    __shared__ long long part[SP_BLOCK];
    block_count_scan(bs, n, part, [](long long, long long) {});
}

// grid ceil(S / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_grid_starts(GridSlot* __restrict__ table, long long S, const int32_t* __restrict__ block_offsets) {
    __shared__ int wc[SP_WAVES];
    const long long s = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const int before = block_scan(s < S ? table[s].count : 0, wc).before;
    if (s < S) table[s].start = block_offsets[blockIdx.x] + before;
}

// grid ceil(Q / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_grid_scatter(const float* __restrict__ points, int Q, GridSlot* __restrict__ table,
                                                           const int32_t* __restrict__ slot_of, GridRecord* __restrict__ records) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= Q) return;
    const int32_t slot = slot_of[i];
    if (slot < 0) return;
    const int32_t place = atomicAdd(&table[slot].start, 1);
    if (place < 0 || place >= Q) return;                   // (cannot happen: the starts partition 0 .. the number of points in range)
    GridRecord r = {points[3 * i], points[3 * i + 1], points[3 * i + 2], (int32_t)i};
    records[place] = r;
}

// grid ceil(Qa / 256): one lane per query
__global__ __launch_bounds__(SP_BLOCK) void k_grid_nearest(const float* __restrict__ queries, long long Qa, const GridHeader* __restrict__ header,
                                                           const GridSlot* __restrict__ table, const GridRecord* __restrict__ records,
                                                           unsigned int mask, int Q, int skip_self, int32_t* __restrict__ index,
                                                           float* __restrict__ dist, int32_t* __restrict__ count) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= Qa) return;
    const float ax = queries[3 * (size_t)i], ay = queries[3 * (size_t)i + 1], az = queries[3 * (size_t)i + 2];
    const GridNearest f = grid_nearest_walk((double)ax, (double)ay, (double)az, header, table, records, mask, Q, skip_self ? (int32_t)i : -1);
    index[i] = f.row;
    dist[i] = f.row < 0 ? GRID_INF : (float)sqrt(f.d2);
    count[i] = f.count;
}

}  // namespace

extern "C" {

int sp_cloud_grid_scratch_units(long long Q) {
    if (Q <= 0) return SP_EINVAL;
    if (Q > SP_CLOUD_GRID_MAX_POINTS) return SP_ELIMIT;
    const GridLayout l = grid_layout(Q);
    return (int)(1 + l.table_units + l.record_units + l.row_units + l.block_units);  // <= 1 + 2^27 + 2^26 + 2^24 + 2^17
}

int sp_cloud_grid_build(const float* points, long long Q, float radius, float ox, float oy, float oz, void* scratch, void* stream) {
    if (!points || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 15u)) return SP_EINVAL;
    if (Q <= 0 || !(radius > 0.f && radius < HUGE_VALF)) return SP_EINVAL;
    if (!(fabsf(ox) < HUGE_VALF && fabsf(oy) < HUGE_VALF && fabsf(oz) < HUGE_VALF)) return SP_EINVAL;
    if (Q > SP_CLOUD_GRID_MAX_POINTS) return SP_ELIMIT;
    const GridLayout l = grid_layout(Q);
    const double r = (double)radius;
    const double r2 = r * r, cell = r * 1.0009765625;
    char* base = static_cast<char*>(scratch);
    GridHeader* header = reinterpret_cast<GridHeader*>(base);
    GridSlot* table = reinterpret_cast<GridSlot*>(base + 64);
    GridRecord* records = reinterpret_cast<GridRecord*>(base + 64 * (size_t)(1 + l.table_units));
    int32_t* slot_of = reinterpret_cast<int32_t*>(base + 64 * (size_t)(1 + l.table_units + l.record_units));
    int32_t* block_sums = slot_of + 16 * (size_t)l.row_units;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((Q + SP_BLOCK - 1) / SP_BLOCK), slot_grid = (unsigned)l.blocks;
    const unsigned int mask = (unsigned int)(l.slots - 1);
    const long long n_words = 2 * l.slots;
    hipLaunchKernelGGL(k_grid_init, dim3((unsigned)((n_words + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s, header,
                       reinterpret_cast<unsigned long long*>(table), n_words, r2, cell, (double)ox, (double)oy, (double)oz, mask, (int)Q);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_count, dim3(grid), dim3(SP_BLOCK), 0, s, points, (int)Q, cell, (double)ox, (double)oy, (double)oz, table, mask, slot_of);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_sums, dim3(slot_grid), dim3(SP_BLOCK), 0, s, table, l.slots, block_sums);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_scan, dim3(1), dim3(SP_BLOCK), 0, s, block_sums, (int)l.blocks);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_starts, dim3(slot_grid), dim3(SP_BLOCK), 0, s, table, l.slots, block_sums);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_grid_scatter, dim3(grid), dim3(SP_BLOCK), 0, s, points, (int)Q, table, slot_of, records);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_cloud_grid_nearest(const float* queries, long long Qa, long long Q, const void* scratch, int skip_self, int32_t* index, float* dist,
                          int32_t* count, void* stream) {
    if (!queries || !scratch || !index || !dist || !count || (reinterpret_cast<uintptr_t>(scratch) & 15u)) return SP_EINVAL;
    if (Qa <= 0 || Q <= 0 || (skip_self != 0 && skip_self != 1) || (skip_self == 1 && Qa != Q)) return SP_EINVAL;
    if (Q > SP_CLOUD_GRID_MAX_POINTS || Qa > 2147483646LL) return SP_ELIMIT;
    const GridLayout l = grid_layout(Q);
    const char* base = static_cast<const char*>(scratch);
    hipLaunchKernelGGL(k_grid_nearest, dim3((unsigned)((Qa + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream),
                       queries, Qa, reinterpret_cast<const GridHeader*>(base), reinterpret_cast<const GridSlot*>(base + 64),
                       reinterpret_cast<const GridRecord*>(base + 64 * (size_t)(1 + l.table_units)), (unsigned int)(l.slots - 1), (int)Q, skip_self,
                       index, dist, count);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
