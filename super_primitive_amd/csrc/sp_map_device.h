// Device-side pieces shared by the map kernels (sp_views.hip, sp_results.hip, sp_fuse.hip, sp_surfel.hip, sp_nearest.hip, sp_register.hip, sp_tsdf.hip, sp_raycast.hip, sp_mesh.hip, sp_mesh_render.hip) and the host side of a view set (its limits, a depth buffer's launch tail): each idiom has its one definition here.
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

// block_rank for lanes that keep `count` >= 0 rows each (sp_tsdf.hip: the crossing edges of a node, the faces of a cell): rank = the rows
// kept before this lane in its workgroup (a wave's inclusive scan by lane swaps, then the waves before it), count = all of the
// workgroup's.  The same conditions: every thread calls it, once per kernel; wc: SP_WAVES ints of LDS
__device__ __forceinline__ BlockRank block_prefix(int count, int* wc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wc[wave] = incl;
    __syncthreads();
    BlockRank r = {incl - count, (wc[0] + wc[1]) + (wc[2] + wc[3])};
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

// The int64 forms of the two (sp_mesh.hip: one face may keep 2^31 rows, a block of faces 2^39): the same shapes and the same
// conditions, counts and prefixes carried in 64 bits throughout.  wc: SP_WAVES long longs of LDS
struct BlockRank64 { long long rank, count; };
__device__ __forceinline__ BlockRank64 block_prefix64(long long count, long long* wc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wc[wave] = incl;
    __syncthreads();
    BlockRank64 r = {incl - count, (wc[0] + wc[1]) + (wc[2] + wc[3])};
    for (int w = 0; w < wave; ++w) r.rank += wc[w];
    return r;
}

// bc[n] (int64) becomes its exclusive prefix sum, in place; every thread gets the total.  part: SP_BLOCK long longs of LDS
__device__ __forceinline__ long long block_count_scan64(long long* __restrict__ bc, long long n, long long* part) {
    const int tid = threadIdx.x;
    const long long per = (n + SP_BLOCK - 1) / SP_BLOCK;
    const long long j0 = (long long)tid * per < n ? (long long)tid * per : n;
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
        const long long c = bc[j];
        bc[j] = run;
        run += c;
    }
    return part[SP_BLOCK - 1];
}

// ---- hashed cell tables (sp_fuse.hip, sp_nearest.hip): 64-bit keys of three biased 21-bit cell indices, open addressing with linear
// probing from a splitmix64 finaliser of the key (the cells of one surface are neighbours: the identity would cluster) ---------------
constexpr unsigned long long FUSE_EMPTY = ~0ull;           // no key: keys use 63 bits
constexpr double FUSE_HALF_RANGE = 1048576.0;              // 2^20 cells to either side of the origin

__device__ __forceinline__ unsigned long long fuse_mix(unsigned long long x) {       // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long fuse_key(unsigned long long cx, unsigned long long cy, unsigned long long cz) {
    return (cx << 42) | (cy << 21) | cz;
}

// The slot of `key` in a table of mask + 1 slots whose first member is the 64-bit key (FUSE_EMPTY until claimed): found, or claimed by
// a 64-bit atomicCAS after a relaxed load (most points find their key already there).  At most mask + 1 probes; a table that holds
// fewer keys than slots cannot exhaust them -- should it ever, the answer is -1, not a loop.
template <class Slot>
__device__ __forceinline__ int32_t fuse_claim(Slot* __restrict__ table, unsigned int mask, unsigned long long key) {
    unsigned int h = (unsigned int)fuse_mix(key) & mask;
    for (unsigned int probe = 0; probe <= mask; ++probe) {                           // at most S slots
        unsigned long long* at = &table[h].key;
        unsigned long long cur = __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == FUSE_EMPTY) cur = atomicCAS(at, FUSE_EMPTY, key);                 // (returns what it found: empty = claimed now)
        if (cur == FUSE_EMPTY || cur == key) return (int32_t)h;
        h = (h + 1u) & mask;
    }
    return -1;
}

// ---- the prepared cloud of sp_cloud_grid_build (sp_nearest.hip builds and queries it, sp_register.hip queries it): its layout, the
// cell of a point, and THE neighbour walk -- one definition, so a registration pass finds exactly the row sp_cloud_grid_nearest finds.
// The arithmetic carries its own contraction pragma: every operation is rounded on its own whatever the including file allows. -------
struct GridHeader {
    double r2, cell, o[3];
    unsigned int mask;                 // S - 1
    int32_t Q;
    long long pad_[2];
};
static_assert(sizeof(GridHeader) == 64, "the header is one 64-byte unit");

struct alignas(16) GridSlot {
    unsigned long long key;            // FUSE_EMPTY until claimed
    int32_t start;                     // the scatter's cursor: the cell's first record before it, its end after it
    int32_t count;
};
static_assert(sizeof(GridSlot) == 16, "one slot is one 16-byte load");

struct alignas(16) GridRecord { float x, y, z; int32_t row; };
static_assert(sizeof(GridRecord) == 16, "one member is one 16-byte load");

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr float GRID_INF = __builtin_huge_valf();

struct GridLayout { long long slots, blocks, table_units, record_units, row_units, block_units; };

// Q in 1 .. SP_CLOUD_GRID_MAX_POINTS.  The scratch: header | table | records | slot numbers | block sums, each a whole number of units
inline GridLayout grid_layout(long long Q) {
    GridLayout l;
    l.slots = 2;
    while (l.slots < 2 * Q) l.slots <<= 1;
    l.blocks = (l.slots + SP_BLOCK - 1) / SP_BLOCK;
    l.table_units = (l.slots + 3) / 4;                     // 16 bytes each
    l.record_units = (Q + 3) / 4;                          // 16 bytes each
    l.row_units = (Q + 15) / 16;                           // Q int32
    l.block_units = (l.blocks + 15) / 16;                  // ceil(S / 256) int32
    return l;
}

// one axis of a point (a float32 coordinate converted exactly, or a float64 one): false = out of range; else the biased cell index
// (1 .. 2^21 - 2: the cells to either side have one too)
__device__ __forceinline__ bool grid_axis(double p, double o, double cell, unsigned long long& c) {
#pragma clang fp contract(off)
    const double q = (p - o) / cell;
    const double g = floor(q);
    if (!(g >= 1.0 - FUSE_HALF_RANGE && g <= FUSE_HALF_RANGE - 2.0)) return false;  // NaN and +-inf fail; tested before the conversion
    c = (unsigned long long)((long long)g + 1048576LL);
    return true;
}

// The walk of one query (x, y, z) over the prepared cloud: the 27 cells around its own, each looked up (a 16-byte load per probe, until
// the key or an empty slot), each cell's records walked; d2 is computed in float64 exactly as the contract of sp_cloud_grid_nearest
// writes it, and visit(d2, row, place) is called for every NEIGHBOUR (d2 <= r2, row != self), in the order the records lie in.
// `self`: a row that is not a neighbour (-1: none).  A scratch built for another Q, or a query out of range, has no neighbours.
// Every loop is bounded: a probe visits at most S slots, a walk at most `count` records, clamped to the record array.
template <class Visit>
__device__ __forceinline__ void grid_walk(double x, double y, double z, const GridHeader* __restrict__ header,
                                          const GridSlot* __restrict__ table, const GridRecord* __restrict__ records,
                                          unsigned int mask, int Q, int32_t self, Visit visit) {
#pragma clang fp contract(off)
    const double r2 = header->r2, cell = header->cell;     // (uniform: scalar loads)
    const bool built = header->mask == mask && header->Q == Q;
    unsigned long long cx = 0, cy = 0, cz = 0;
    const bool in = built && grid_axis(x, header->o[0], cell, cx) && grid_axis(y, header->o[1], cell, cy) && grid_axis(z, header->o[2], cell, cz);
    if (in) {
#pragma unroll 1
        for (int c = 0; c < 27; ++c) {
            const int c9 = c / 9, c3 = (c / 3) % 3, c1 = c % 3;
            const unsigned long long key = fuse_key(cx + (unsigned long long)c9 - 1ull, cy + (unsigned long long)c3 - 1ull, cz + (unsigned long long)c1 - 1ull);
            unsigned int h = (unsigned int)fuse_mix(key) & mask;
            int32_t end = 0, members = 0;
            for (unsigned int probe = 0; probe <= mask; ++probe) {                   // at most S slots
                const i32x4 s = *reinterpret_cast<const i32x4*>(table + h);
                const unsigned long long cur = ((unsigned long long)(uint32_t)s.y << 32) | (unsigned long long)(uint32_t)s.x;
                if (cur == key) { end = s.z; members = s.w; break; }
                if (cur == FUSE_EMPTY) break;
                h = (h + 1u) & mask;
            }
            if (members > end) members = end;              // (cannot happen after a build: keeps the walk inside the records)
            if (end > Q) members = 0;
            for (int32_t m = end - members; m < end; ++m) {
                const i32x4 raw = *reinterpret_cast<const i32x4*>(records + m);
                const double dx = x - (double)__int_as_float(raw.x), dy = y - (double)__int_as_float(raw.y), dz = z - (double)__int_as_float(raw.z);
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const int32_t row = raw.w;
                if (d2 <= r2 && row != self) visit(d2, row, m);
            }
        }
    }
}

// what one query finds: d2 and row of the neighbour with the smallest (d2, row) (HUGE_VAL and -1: none), where its record lies, and
// the number of neighbours
struct GridNearest { double d2; int32_t row, place, count; };

// grid_walk keeping the minimum over (d2, row) and the count: what sp_cloud_grid_nearest answers and sp_cloud_register pairs with
__device__ __forceinline__ GridNearest grid_nearest_walk(double x, double y, double z, const GridHeader* __restrict__ header,
                                                         const GridSlot* __restrict__ table, const GridRecord* __restrict__ records,
                                                         unsigned int mask, int Q, int32_t self) {
    GridNearest f = {HUGE_VAL, -1, -1, 0};
    grid_walk(x, y, z, header, table, records, mask, Q, self, [&f](double d2, int32_t row, int32_t m) {
        ++f.count;
        if (d2 < f.d2 || (d2 == f.d2 && row < f.row)) { f.d2 = d2; f.row = row; f.place = m; }
    });
    return f;
}

// ---- the keyframe walk: a workgroup belongs to ONE keyframe, the last record whose first_block is at or before it (uniform: scalar loads)
__device__ __forceinline__ int keyframe_of_block(const SpMapKeyframe* __restrict__ kfs, int n_kf, int block) {
    int lo = 0, hi = n_kf;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (kfs[mid].first_block <= block) lo = mid; else hi = mid; }
    return lo;
}

// the segment of table point i of a keyframe
__device__ __forceinline__ int map_point_segment(const SpMapKeyframe& kf, int i) { return segment_of(kf.seg_off, kf.N, i); }

// ---- views: one record per view in float64, the projection, a footprint's half-width (every kernel that projects; the arithmetic
// carries its own contraction pragma: every operation is rounded on its own whatever the including file allows) ----------------------
constexpr int VIEW_CHUNK = 16;

struct ViewD {
    double Rt[9], t[3];                // R^T row major, t: p_c = R^T (p - t)
    double fx, fy, cx, cy;
    int ident, pad_;
};

__device__ __forceinline__ void view_setup(const SpView& v, ViewD& o) {
    bool ident = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = v.pose[4 * c + r];
            o.Rt[3 * r + c] = (double)e;
            ident = ident && e == (r == c ? 1.f : 0.f);
        }
        const float t = v.pose[4 * r + 3];
        o.t[r] = (double)t;
        ident = ident && t == 0.f;
    }
    o.fx = (double)v.K[0]; o.fy = (double)v.K[4]; o.cx = (double)v.K[2]; o.cy = (double)v.K[5];
    o.ident = ident ? 1 : 0;
    o.pad_ = 0;
}

// The projection of one point into one view, shared by every kernel that projects (the contract of sp_render_views in include/sp_hip.h):
// p_c = R^T (p - t), the three-term sums as (a + b) + c; an exact identity pose leaves the point untouched.
__device__ __forceinline__ void camera_point(const ViewD& w, double px, double py, double pz, double& x, double& y, double& z) {
#pragma clang fp contract(off)
    x = px; y = py; z = pz;
    if (!w.ident) {
        const double d0 = px - w.t[0], d1 = py - w.t[1], d2 = pz - w.t[2];
        x = (w.Rt[0] * d0 + w.Rt[1] * d1) + w.Rt[2] * d2;
        y = (w.Rt[3] * d0 + w.Rt[4] * d1) + w.Rt[5] * d2;
        z = (w.Rt[6] * d0 + w.Rt[7] * d1) + w.Rt[8] * d2;
    }
}

// camera_point's inverse along the ray of one pixel (the contract of sp_tsdf_raycast in include/sp_hip.h): the ray is parameterised by
// camera z, q = (xr z, yr z, z), and p = R q + t, every row as ((a + b) + c) + t.  R is Rt read transposed (R_ab = Rt[3 b + a]); an exact
// identity pose leaves p = q.
__device__ __forceinline__ void world_point(const ViewD& w, double xr, double yr, double z, double& px, double& py, double& pz) {
#pragma clang fp contract(off)
    const double q0 = xr * z, q1 = yr * z;
    px = q0; py = q1; pz = z;
    if (!w.ident) {
        px = ((w.Rt[0] * q0 + w.Rt[3] * q1) + w.Rt[6] * z) + w.t[0];
        py = ((w.Rt[1] * q0 + w.Rt[4] * q1) + w.Rt[7] * z) + w.t[1];
        pz = ((w.Rt[2] * q0 + w.Rt[5] * q1) + w.Rt[8] * z) + w.t[2];
    }
}

// u = x fx / z + cx, v = y fy / z + cy: two IEEE divisions
__device__ __forceinline__ void pixel_of(const ViewD& w, double x, double y, double z, double& u, double& v) {
#pragma clang fp contract(off)
    u = (x * w.fx) / z + w.cx;
    v = (y * w.fy) / z + w.cy;
}

// the half-width of a footprint in pixels: anything that is not >= 0 (a negative or NaN radius, inf / inf) is a point
__device__ __forceinline__ double half_width(double h, double cap) { return !(h >= 0.0) ? 0.0 : (h < cap ? h : cap); }

// ---- signed-distance volumes (sp_tsdf.hip, sp_raycast.hip): where a node sits, when it counts, its cell's corners, the sizes allowed ----
// the centre of node i of one axis: ((float64(i) + 0.5) * voxel) + o
__device__ __forceinline__ double node_centre(int i, double voxel, double o) {
#pragma clang fp contract(off)
    return ((double)i + 0.5) * voxel + o;
}
// a node is VALID iff its weight is >= min_weight and its tsdf is finite
__device__ __forceinline__ bool node_valid(float f, float w, float min_weight) { return w >= min_weight && fabsf(f) < HUGE_VALF; }
// the linear offset of corner / edge type c from a node (offset bits x = 1, y = 2, z = 4)
__device__ __forceinline__ int corner_offset(int c, int nx, int nxy) { return (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nxy; }

// nx ny nz without overflow: 0 if any is < 1, -1 beyond the limit
inline long long volume_nodes(int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    const long long xy = (long long)nx * ny;
    if (xy > SP_TSDF_MAX_NODES || xy * nz > SP_TSDF_MAX_NODES) return -1;
    return xy * nz;
}

// neither NaN nor +-inf: finite_f on the host (the entry points' arguments), finite_d on either side
inline bool finite_f(float x) { return fabsf(x) < HUGE_VALF; }
__host__ __device__ __forceinline__ bool finite_d(double x) { return fabs(x) < HUGE_VAL; }

// ---- the host side of a view set: its limits, a depth buffer's empty keys and pixel grid -------------------------------------------
// ids and pixels are 32-bit, a grid dimension 16-bit: 0, or SP_ELIMIT beyond 65535 views, 2^31 - 1 pixels in all or 2^31 - 2 points
inline int view_limits(int V, int H, int W, long long Q = 0) {
    const long long HW = (long long)H * W;
    return Q > 0x7ffffffeLL || V > 65535 || HW >= 0x80000000LL || (long long)V * HW >= 0x80000000LL ? SP_ELIMIT : 0;
}
// every key word 0: nothing landed
inline hipError_t keys_clear(unsigned long long* keys, long long n_pix, hipStream_t s) {
    return hipMemsetAsync(keys, 0, sizeof(unsigned long long) * (size_t)n_pix, s);
}
// one thread per pixel
inline dim3 pixel_grid(long long n_pix) { return dim3((unsigned)((n_pix + SP_BLOCK - 1) / SP_BLOCK)); }

// ---- the resolve pass and the launch tail of every depth buffer of keys (sp_render_views, sp_render_splats, sp_render_surfels): one
// definition here, one static copy in every file that launches it and says so by defining SP_MAP_DEVICE_RESOLVE before this header --
#ifdef SP_MAP_DEVICE_RESOLVE
// grid ceil(V H W / 256), block SP_BLOCK
static __global__ __launch_bounds__(SP_BLOCK) void k_render_resolve(const unsigned long long* __restrict__ keys, const float* __restrict__ colours,
                                                             int n_pix, int mode, uint8_t* __restrict__ image, float* __restrict__ depth,
                                                             int32_t* __restrict__ index) {
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (at >= n_pix) return;
    const unsigned long long k = keys[at];
    const int idx = mode == 1 ? key_nearest_id(k) : key_highest_id_id(k);
    const float d = mode == 1 ? key_nearest_z(k) : key_highest_id_z(k);
    if (index) index[at] = idx;
    if (depth) depth[at] = d;
    if (image) {
        uint8_t rgb[3] = {0, 0, 0};
        if (idx >= 0) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) rgb[ch] = colour_u8(colours[3 * (size_t)idx + ch]);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) image[3 * (size_t)at + ch] = rgb[ch];
    }
}

// The launch tail of a depth buffer of n_pix keys: empty keys, the caller's key pass -- key_pass() launches it -- and, if any output is
// asked for, the resolve pass
template <class KeyPass>
int depth_buffer_launch(unsigned long long* keys, const float* colours, long long n_pix, int mode, uint8_t* image, float* depth, int32_t* index,
                        hipStream_t s, KeyPass key_pass) {
    const hipError_t e = keys_clear(keys, n_pix, s);
    if (e != hipSuccess) return (int)e;
    key_pass();
    SP_CHECK_LAUNCH();
    if (image || depth || index) {
        hipLaunchKernelGGL(k_render_resolve, pixel_grid(n_pix), dim3(SP_BLOCK), 0, s, keys, colours, (int)n_pix, mode, image, depth, index);
        SP_CHECK_LAUNCH();
    }
    return 0;
}
#endif
