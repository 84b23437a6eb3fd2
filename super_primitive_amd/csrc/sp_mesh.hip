// Mesh surfaces: one record per face of a triangle list (sp_mesh_faces) and an area-uniform, seeded cloud sampled from those records
// (sp_mesh_sample); the contracts are in include/sp_hip.h.  Float64 from the float32 inputs, every operation rounded on its own: the
// arithmetic of the rule is written with __dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn, and the file carries the
// contraction pragma on top.
//
// sp_mesh_faces.  One launch, one thread per face: three indices, a gather of nine floats, the record.  The summary is six 64-bit words
// zeroed by a memset node in front of the launch: a wave counts its faces per state by ballots and takes the maximum of its areas' bit
// patterns by lane swaps, the workgroup adds its four waves in LDS, and threads 0 .. 5 send one integer atomic each (atomicAdd, atomicMax
// on the bits) -- only for a word the block changes, so a mesh of valid faces costs two atomics per 256 faces.  Integer sums and maxima
// commute: two runs give the same bits.
//
// sp_mesh_sample.  Ordered expansion from the pieces of sp_map_device.h in their int64 forms (block_prefix64, block_count_scan64): a
// face may keep 2^31 rows.  No workgroup waits on another, nothing spins, no atomics, no sort, no float prefix sum:
//   k_sample_count   one thread per face: its number of rows n_i (stochastic rounding of area density by the face's own hash) and the
//                    rows before it in its 256-face block -> one int64 per face; per block its rows
//   k_sample_scan    one workgroup: the exclusive prefix sum of the block array, in place; n_out = the total
//   k_sample_rows    ONE THREAD PER OUTPUT ROW: the last block whose offset is <= the row, then the last face of that block whose
//                    prefix is <= what is left (two binary searches over integers: at most 20 + 8 steps), k = the rest; the row is a
//                    function of (seed, face, k) alone.  A face of 10^6 rows is 10^6 threads; a wave stores 768 contiguous bytes
// The last is launched only with a capacity, over ceil(capacity / 256) workgroups (the host does not know the total), and writes nothing
// when the total is beyond 2^31 - 1.
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

constexpr unsigned long long MESH_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long MESH_ONE = 1ull << 53;        // A(x) < 2^53; u = A * 2^-53
constexpr double MESH_ROWS_MAX = 2147483648.0;             // 2^31

__device__ __forceinline__ unsigned long long mesh_a(unsigned long long x) { return fuse_mix(x) >> 11; }
__device__ __forceinline__ double mesh_u(unsigned long long a) { return __dmul_rn((double)a, 0x1p-53); }   // (a <= 2^53: both steps exact)
__device__ __forceinline__ unsigned long long mesh_hash(unsigned long long seed, long long face) {
    return seed + MESH_GOLDEN * ((unsigned long long)face + 1ull);
}
__device__ __forceinline__ bool mesh_index_ok(int i0, int i1, int i2, int M) {
    return (unsigned)i0 < (unsigned)M && (unsigned)i1 < (unsigned)M && (unsigned)i2 < (unsigned)M;
}

// ---- faces -------------------------------------------------------------------------------------------------------------------------------
// grid ceil(F / 256), block SP_BLOCK.  summary: six words, zero before the launch
__global__ __launch_bounds__(SP_BLOCK) void k_mesh_faces(const float* __restrict__ vertices, int M, const int32_t* __restrict__ faces, int F,
                                                         double* __restrict__ area, float* __restrict__ normals, uint8_t* __restrict__ state,
                                                         double* __restrict__ cross, unsigned long long* __restrict__ summary) {
    __shared__ unsigned long long acc[SP_WAVES][SP_MESH_SUMMARY_WORDS];
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const bool in = at < F;
    int st = -1;                                            // (a lane beyond the mesh counts nowhere)
    double a = 0.0, c[3] = {0.0, 0.0, 0.0};
    float n[3] = {0.f, 0.f, 0.f};
    if (in) {
        const int i0 = faces[3 * (size_t)at], i1 = faces[3 * (size_t)at + 1], i2 = faces[3 * (size_t)at + 2];
        if (!mesh_index_ok(i0, i1, i2, M)) {
            st = 1;
        } else if (i0 == i1 || i1 == i2 || i0 == i2) {
            st = 2;
        } else {
            float p[3][3];
            bool finite = true;
            const int idx[3] = {i0, i1, i2};
#pragma unroll
            for (int v = 0; v < 3; ++v)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    p[v][ax] = vertices[3 * (size_t)idx[v] + ax];
                    finite = finite && fabsf(p[v][ax]) < HUGE_VALF;
                }
            if (!finite) {
                st = 3;
            } else {
                double e1[3], e2[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    e1[ax] = __dsub_rn((double)p[1][ax], (double)p[0][ax]);
                    e2[ax] = __dsub_rn((double)p[2][ax], (double)p[0][ax]);
                }
                const double cx = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));
                const double cy = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
                const double cz = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
                const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz)));
                const double ar = __dmul_rn(0.5, l);
                if (!(ar > 0.0 && ar < HUGE_VAL)) {
                    st = 4;
                } else {
                    st = 0;
                    a = ar;
                    c[0] = cx; c[1] = cy; c[2] = cz;
                    n[0] = (float)__ddiv_rn(cx, l); n[1] = (float)__ddiv_rn(cy, l); n[2] = (float)__ddiv_rn(cz, l);
                }
            }
        }
        if (area) area[at] = a;
        if (state) state[at] = (uint8_t)st;
        if (normals) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) normals[3 * (size_t)at + ax] = n[ax];
        }
        if (cross) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) cross[3 * (size_t)at + ax] = c[ax];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long top = (unsigned long long)__double_as_longlong(a);            // a >= 0: the bits order as the doubles do
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(top, off, 64);
        top = other > top ? other : top;
    }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const unsigned long long b = __ballot(st == s);
        if (lane == 0) acc[wave][s] = (unsigned long long)__popcll(b);
    }
    if (lane == 0) acc[wave][5] = top;
    __syncthreads();
    if (threadIdx.x < SP_MESH_SUMMARY_WORDS) {
        const int s = threadIdx.x;
        if (s < 5) {
            const unsigned long long sum = (acc[0][s] + acc[1][s]) + (acc[2][s] + acc[3][s]);
            if (sum) atomicAdd(summary + s, sum);
        } else {
            unsigned long long m = acc[0][5];
#pragma unroll
            for (int w = 1; w < SP_WAVES; ++w) m = acc[w][5] > m ? acc[w][5] : m;
            if (m) atomicMax(summary + 5, m);
        }
    }
}

// ---- sample ------------------------------------------------------------------------------------------------------------------------------
// grid ceil(F / 256): n_i, its prefix in the block, the block's rows
__global__ __launch_bounds__(SP_BLOCK) void k_sample_count(const int32_t* __restrict__ faces, int F, int M, const double* __restrict__ area,
                                                         const uint8_t* __restrict__ state, double density, unsigned long long seed,
                                                         long long* __restrict__ prefix, long long* __restrict__ block_counts) {
    __shared__ long long wc[SP_WAVES];
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    long long n = 0;
    if (at < F && state[at] == 0 && mesh_index_ok(faces[3 * (size_t)at], faces[3 * (size_t)at + 1], faces[3 * (size_t)at + 2], M)) {
        double t = __dmul_rn(area[at], density);
        if (!(t < MESH_ROWS_MAX)) t = MESH_ROWS_MAX;
        const double v = floor(__dadd_rn(t, mesh_u(mesh_a(mesh_hash(seed, at)))));  // <= 2^31
        n = v > 0.0 ? (long long)v : 0;
    }
    const BlockRank64 r = block_prefix64(n, wc);
    if (at < F) prefix[at] = r.rank;
    if (threadIdx.x == 0) block_counts[blockIdx.x] = r.count;
}

// grid 1
__global__ __launch_bounds__(SP_BLOCK) void k_sample_scan(long long* __restrict__ block_counts, long long n_blocks, long long* __restrict__ n_out) {
    __shared__ long long part[SP_BLOCK];
    const long long total = block_count_scan64(block_counts, n_blocks, part);
    if (threadIdx.x == 0) n_out[0] = total;
}

// one axis of a row: (p0 + u1 (p1 - p0)) + u2 (p2 - p0)
__device__ __forceinline__ float mesh_blend(float p0, float p1, float p2, double u1, double u2) {
    const double q0 = (double)p0;
    return (float)__dadd_rn(__dadd_rn(q0, __dmul_rn(u1, __dsub_rn((double)p1, q0))), __dmul_rn(u2, __dsub_rn((double)p2, q0)));
}

// grid ceil(capacity / 256): one thread per row
__global__ __launch_bounds__(SP_BLOCK) void k_sample_rows(const float* __restrict__ vertices, const float* __restrict__ vertex_colours,
                                                        const int32_t* __restrict__ faces, int F, const float* __restrict__ face_normals,
                                                        unsigned long long seed, const long long* __restrict__ prefix,
                                                        const long long* __restrict__ block_offsets, int n_blocks,
                                                        const long long* __restrict__ n_out, long long capacity, float* __restrict__ points,
                                                        float* __restrict__ normals, float* __restrict__ colours, int32_t* __restrict__ face) {
    const long long row = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const long long total = n_out[0];
    if (row >= capacity || row >= total || total > 0x7fffffffLL) return;
    int lo = 0, hi = n_blocks;                              // block_offsets[0] = 0 <= row: the last block at or before the row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (block_offsets[mid] <= row) lo = mid; else hi = mid;
    }
    const long long local = row - block_offsets[lo];
    int flo = lo * SP_BLOCK, fhi = flo + SP_BLOCK < F ? flo + SP_BLOCK : F;          // prefix[flo] = 0 <= local
    while (fhi - flo > 1) {
        const int mid = (flo + fhi) >> 1;
        if (prefix[mid] <= local) flo = mid; else fhi = mid;
    }
    // the last face whose first row is at or before this one owns it: its rows end where the next face's begin, beyond this row, so it
    // has n > 0 -- and k_sample_count gave rows only to faces whose indices are inside the vertices
    const int i = flo;
    const unsigned long long k = (unsigned long long)(local - prefix[i]);
    const unsigned long long h = mesh_hash(seed, i);
    unsigned long long a1 = mesh_a(h + 1ull + 2ull * k), a2 = mesh_a(h + 2ull + 2ull * k);
    if (a1 + a2 > MESH_ONE) { a1 = MESH_ONE - a1; a2 = MESH_ONE - a2; }
    const double u1 = mesh_u(a1), u2 = mesh_u(a2);
    const size_t i0 = 3 * (size_t)faces[3 * (size_t)i], i1 = 3 * (size_t)faces[3 * (size_t)i + 1], i2 = 3 * (size_t)faces[3 * (size_t)i + 2];
    const size_t out = 3 * (size_t)row;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) points[out + ax] = mesh_blend(vertices[i0 + ax], vertices[i1 + ax], vertices[i2 + ax], u1, u2);
    if (colours) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) colours[out + ch] = mesh_blend(vertex_colours[i0 + ch], vertex_colours[i1 + ch], vertex_colours[i2 + ch], u1, u2);
    }
    if (normals) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) normals[out + ax] = face_normals[3 * (size_t)i + ax];
    }
    if (face) face[row] = i;
}

struct SampleLayout { long long blocks, prefix_units, block_units; };

// F in 1 .. SP_MESH_MAX_FACES.  The scratch: one int64 per face | one per 256 faces, each a whole number of 64-byte units
SampleLayout sample_layout(long long F) {
    SampleLayout l;
    l.blocks = (F + SP_BLOCK - 1) / SP_BLOCK;
    l.prefix_units = (F + 7) / 8;
    l.block_units = (l.blocks + 7) / 8;
    return l;
}

inline bool finite_d(double x) { return fabs(x) < HUGE_VAL; }

}  // namespace

extern "C" {

int sp_mesh_faces(const float* vertices, long long M, const int32_t* faces, long long F, double* area, float* normals, uint8_t* state,
                  double* cross, long long* summary, void* stream) {
    if (!vertices || !faces || !summary || F < 1 || M < 1) return SP_EINVAL;
    if (F > SP_MESH_MAX_FACES || M > SP_MESH_MAX_FACES) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(summary, 0, sizeof(long long) * SP_MESH_SUMMARY_WORDS, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_mesh_faces, dim3((unsigned)((F + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s, vertices, (int)M, faces, (int)F, area,
                       normals, state, cross, reinterpret_cast<unsigned long long*>(summary));
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_mesh_sample_scratch_units(long long F) {
    if (F < 1) return SP_EINVAL;
    if (F > SP_MESH_MAX_FACES) return SP_ELIMIT;
    const SampleLayout l = sample_layout(F);
    return (int)(l.prefix_units + l.block_units);           // 2^25 + 2^17 at the limit
}

int sp_mesh_sample(const float* vertices, const float* vertex_colours, long long M, const int32_t* faces, long long F, const double* area,
                   const float* face_normals, const uint8_t* state, double density, long long seed, void* scratch, long long capacity,
                   float* points, float* normals, float* colours, int32_t* face, long long* n_out, void* stream) {
    if (!vertices || !faces || !area || !state || !scratch || !n_out || ((uintptr_t)scratch & 7)) return SP_EINVAL;
    if (F < 1 || M < 1 || capacity < 0 || !(density > 0.0 && finite_d(density))) return SP_EINVAL;
    if ((points != nullptr) != (capacity > 0)) return SP_EINVAL;
    if (capacity == 0 && (normals || colours || face)) return SP_EINVAL;
    if ((normals && !face_normals) || (colours && !vertex_colours)) return SP_EINVAL;
    if (F > SP_MESH_MAX_FACES || M > SP_MESH_MAX_FACES || capacity > 0x7fffffffLL) return SP_ELIMIT;
    const SampleLayout l = sample_layout(F);
    long long* prefix = static_cast<long long*>(scratch);
    long long* blocks = prefix + 8 * (size_t)l.prefix_units;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_sample_count, dim3((unsigned)l.blocks), dim3(SP_BLOCK), 0, s, faces, (int)F, (int)M, area, state, density,
                       (unsigned long long)seed, prefix, blocks);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(SP_BLOCK), 0, s, blocks, l.blocks, n_out);
    SP_CHECK_LAUNCH();
    if (capacity > 0) {
        hipLaunchKernelGGL(k_sample_rows, dim3((unsigned)((capacity + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s, vertices, vertex_colours, faces,
                           (int)F, face_normals, (unsigned long long)seed, prefix, blocks, (int)l.blocks, n_out, capacity, points, normals, colours,
                           face);
        SP_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
