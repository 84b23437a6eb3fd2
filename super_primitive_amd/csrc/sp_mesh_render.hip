// Mesh views: a triangle mesh rasterised into depth, normal, colour and face-index images of V cameras (sp_mesh_render; the rule is in
// include/sp_hip.h).  Float64 from the float32 inputs, every operation rounded on its own: the file carries the contraction pragma, as
// sp_mesh.hip does, and camera_point / pixel_of (sp_map_device.h) carry their own.
//
// The unit of work is an ITEM: one (face, view, tile) -- a tile is 64 pixels of the image's own tile grid, SP_MESH_RENDER_TILE_W wide
// (a compile-time macro the results cannot depend on: the rule fixes the rectangle, the tiles only cut it up).  One wave per item, one
// lane per pixel: a wall triangle that covers the image is ceil(H / th) ceil(W / tw) waves next to a million faces of one wave each, never
// one lane's loop.  Views go through in chunks of SP_MESH_RENDER_VIEW_CHUNK; the scratch holds one chunk.  Per chunk three launches, none
// of which waits on the host (the number of items stays on the device):
//   k_mr_count    one thread per (face, view of the chunk): the rule's rectangle, the tiles it touches (0 for a dropped face) and -- by
//                 block_prefix64 -- the items before it in its 256-entry block -> one int64 per entry; per block its items
//   k_mr_scan     one workgroup: the exclusive prefix sum of the block array in place (block_count_scan64); the total -> scratch word 0
//   k_mr_raster   a fixed grid whose waves stride over the items, 8 consecutive ones at a time: the entry by k_sample_rows' two binary
//                 searches (all wave-uniform; skipped, with the set-up, while the next item is a tile of the same entry), the tile from
//                 the remainder, the set-up again in float64, the rule's test on the wave's 64 pixels, key_offer for the covered ones
//                 (mode 1's "nearest" key: 64-bit integer maxima, two runs give the same bits)
// and at the end ONE k_mr_resolve over every pixel: index and depth from the key, the normal from the face's record, the colour from the
// rule's weights formed again for (face, view, pixel) -- so every output is a function of the winner alone.
// No floating-point atomics, no scratch (private) memory, no workgroup waits on another.
#include "sp_map_device.h"

#pragma clang fp contract(off)

#ifndef SP_MESH_RENDER_TILE_W
#define SP_MESH_RENDER_TILE_W 8
#endif

namespace {

constexpr int MR_TW = SP_MESH_RENDER_TILE_W;
constexpr int MR_TH = 64 / MR_TW;
static_assert(MR_TW >= 1 && MR_TW <= 64 && MR_TW * MR_TH == 64, "a tile is the 64 pixels of one wave: its width divides 64");
constexpr int MR_GRID = 2048;                              // workgroups of the raster pass: 8 per CU, 32 waves
constexpr int MR_CHUNK = SP_MESH_RENDER_VIEW_CHUNK;
constexpr int MR_RUN = 8;                                  // consecutive items per wave and trip: the tiles of one large face share a set-up

// One (face, view): the edge planes, det, and the rule's rectangle (face_setup answers false for a face that covers nothing in the view)
struct FaceSetup {
    double n[3][3];                    // n_0 = q_1 x q_2, n_1 = q_2 x q_0, n_2 = q_0 x q_1
    double det;
    int c0, c1, r0, r1;                // the rectangle, inclusive, inside the image
};

__device__ __forceinline__ void mr_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// the range of one axis: lo = the smallest of the three pixel coordinates, hi the largest, n the image's size there
__device__ __forceinline__ bool mr_range(double lo, double hi, int n, int& first, int& last) {
    const double a = fmax(floor(lo), 0.0), b = fmin(ceil(hi), (double)n - 1.0);     // clamped in float64, then converted
    if (!(a <= b)) return false;
    first = (int)a; last = (int)b;
    return true;
}

__device__ __forceinline__ bool face_setup(const float* __restrict__ vertices, int M, const int32_t* __restrict__ faces, int f, const ViewD& w,
                                           int H, int W, double zmin, int cull, FaceSetup& s) {
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if (!((unsigned)i0 < (unsigned)M && (unsigned)i1 < (unsigned)M && (unsigned)i2 < (unsigned)M)) return false;
    if (i0 == i1 || i1 == i2 || i0 == i2) return false;
    const float* p0 = vertices + 3 * (size_t)i0;
    const float* p1 = vertices + 3 * (size_t)i1;
    const float* p2 = vertices + 3 * (size_t)i2;
    const float a0 = p0[0], a1 = p0[1], a2 = p0[2], b0 = p1[0], b1 = p1[1], b2 = p1[2], c0 = p2[0], c1 = p2[1], c2 = p2[2];
    const bool finite = fabsf(a0) < HUGE_VALF && fabsf(a1) < HUGE_VALF && fabsf(a2) < HUGE_VALF && fabsf(b0) < HUGE_VALF && fabsf(b1) < HUGE_VALF &&
                        fabsf(b2) < HUGE_VALF && fabsf(c0) < HUGE_VALF && fabsf(c1) < HUGE_VALF && fabsf(c2) < HUGE_VALF;
    if (!finite) return false;
    double q0[3], q1[3], q2[3];
    camera_point(w, (double)a0, (double)a1, (double)a2, q0[0], q0[1], q0[2]);
    camera_point(w, (double)b0, (double)b1, (double)b2, q1[0], q1[1], q1[2]);
    camera_point(w, (double)c0, (double)c1, (double)c2, q2[0], q2[1], q2[2]);
    mr_cross(q1, q2, s.n[0]);
    mr_cross(q2, q0, s.n[1]);
    mr_cross(q0, q1, s.n[2]);
    s.det = (q0[0] * s.n[0][0] + q0[1] * s.n[0][1]) + q0[2] * s.n[0][2];
    if (s.det == 0.0 || !finite_d(s.det)) return false;
    if (cull && !(s.det < 0.0)) return false;
    const bool f0 = q0[2] > zmin, f1 = q1[2] > zmin, f2 = q2[2] > zmin;
    if (!f0 && !f1 && !f2) return false;                   // every point of it lies at or behind the plane
    s.c0 = 0; s.c1 = W - 1; s.r0 = 0; s.r1 = H - 1;        // a face that crosses the plane: the whole image
    if (f0 && f1 && f2) {
        double u0, v0, u1, v1, u2, v2;
        pixel_of(w, q0[0], q0[1], q0[2], u0, v0);
        pixel_of(w, q1[0], q1[1], q1[2], u1, v1);
        pixel_of(w, q2[0], q2[1], q2[2], u2, v2);
        if (finite_d(u0) && finite_d(u1) && finite_d(u2) && finite_d(v0) && finite_d(v1) && finite_d(v2)) {
            if (!mr_range(fmin(fmin(u0, u1), u2), fmax(fmax(u0, u1), u2), W, s.c0, s.c1)) return false;
            if (!mr_range(fmin(fmin(v0, v1), v2), fmax(fmax(v0, v1), v2), H, s.r0, s.r1)) return false;
        }
    }
    return true;
}

// The rule's test of one pixel: covered or not, and E_k, S, z for the caller
__device__ __forceinline__ bool pixel_test(const FaceSetup& s, const ViewD& w, int row, int col, double zmin, double* E, double& S, double& z) {
    const double a = ((double)col - w.cx) / w.fx, b = ((double)row - w.cy) / w.fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) E[k] = (s.n[k][0] * a + s.n[k][1] * b) + s.n[k][2];
    S = (E[0] + E[1]) + E[2];
    z = s.det / S;
    const bool inside = s.det < 0.0 ? (E[0] <= 0.0 && E[1] <= 0.0 && E[2] <= 0.0 && S < 0.0) : (E[0] >= 0.0 && E[1] >= 0.0 && E[2] >= 0.0 && S > 0.0);
    return inside && z > zmin && z < HUGE_VAL;
}

// the tiles of the image's tile grid that a rectangle touches
__device__ __forceinline__ long long rect_tiles(const FaceSetup& s) {
    return (long long)(s.c1 / MR_TW - s.c0 / MR_TW + 1) * (long long)(s.r1 / MR_TH - s.r0 / MR_TH + 1);
}

// ---- count ----------------------------------------------------------------------------------------------------------------------------
// grid (ceil(F / 256), views of the chunk), block SP_BLOCK: entry block blockIdx.y * gridDim.x + blockIdx.x, entry tid of it
__global__ __launch_bounds__(SP_BLOCK) void k_mr_count(const float* __restrict__ vertices, int M, const int32_t* __restrict__ faces, int F,
                                                       const SpView* __restrict__ views, int H, int W, float z_min, int cull,
                                                       long long* __restrict__ prefix, long long* __restrict__ block_counts) {
    __shared__ long long wc[SP_WAVES];
    __shared__ ViewD vd;
    if (threadIdx.x == 0) view_setup(views[blockIdx.y], vd);
    __syncthreads();
    const long long f = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    long long n = 0;
    if (f < F) {
        FaceSetup s;
        if (face_setup(vertices, M, faces, (int)f, vd, H, W, (double)z_min, cull, s)) n = rect_tiles(s);
    }
    const BlockRank64 r = block_prefix64(n, wc);
    const size_t block = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    prefix[block * SP_BLOCK + threadIdx.x] = r.rank;
    if (threadIdx.x == 0) block_counts[block] = r.count;
}

// grid 1
__global__ __launch_bounds__(SP_BLOCK) void k_mr_scan(long long* __restrict__ block_counts, long long n_blocks, long long* __restrict__ total) {
    __shared__ long long part[SP_BLOCK];
    const long long t = block_count_scan64(block_counts, n_blocks, part);
    if (threadIdx.x == 0) total[0] = t;
}

// ---- raster ---------------------------------------------------------------------------------------------------------------------------
// a fixed grid, block SP_BLOCK: wave j takes the items 8 j .. 8 j + 7, then those 8 waves further on, ...; consecutive items of one entry
// (the tiles of a face larger than a tile) reuse its search and its set-up.  keys: the chunk's first view
__global__ __launch_bounds__(SP_BLOCK) void k_mr_raster(const float* __restrict__ vertices, int M, const int32_t* __restrict__ faces, int F,
                                                        const SpView* __restrict__ views, int nv, int H, int W, float z_min, int cull,
                                                        const long long* __restrict__ prefix, const long long* __restrict__ block_offsets,
                                                        int blocks_per_view, const long long* __restrict__ total_at,
                                                        unsigned long long* __restrict__ keys) {
    __shared__ ViewD vd[MR_CHUNK];
    if ((int)threadIdx.x < nv) view_setup(views[threadIdx.x], vd[threadIdx.x]);
    __syncthreads();
    const long long total = total_at[0];
    const int n_blocks = blocks_per_view * nv;
    const int lane = threadIdx.x & 63;
    const int lx = lane % MR_TW, ly = lane / MR_TW;
    const long long waves = (long long)gridDim.x * SP_WAVES;
    const size_t HW = (size_t)H * W;
    const double zmin = (double)z_min;
    // the items of the entry whose set-up the wave holds, [own_first, own_end): none yet
    long long own_first = 0, own_end = 0, f = 0;
    int k = 0;
    FaceSetup s = {};
    const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SP_WAVES + (threadIdx.x >> 6)));
    for (long long base = wave * MR_RUN; base < total; base += waves * MR_RUN)
    for (int j = 0; j < MR_RUN; ++j) {
        const long long item = base + j;
        if (item >= total) break;
        if (item < own_first || item >= own_end) {         // another entry's: find it and set it up
            int lo = 0, hi = n_blocks;                     // block_offsets[0] = 0 <= item: the last block at or before the item
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (block_offsets[mid] <= item) lo = mid; else hi = mid;
            }
            const long long local = item - block_offsets[lo];
            const long long* in_block = prefix + (size_t)lo * SP_BLOCK;
            int e = 0, eh = SP_BLOCK;                      // in_block[0] = 0 <= local
            while (eh - e > 1) {
                const int mid = (e + eh) >> 1;
                if (in_block[mid] <= local) e = mid; else eh = mid;
            }
            // the last entry whose first item is at or before this one owns it: its items end where the next entry's begin, beyond
            // this item, so it has tiles -- and k_mr_count gave tiles only to faces below F whose indices are inside the vertices
            own_first = block_offsets[lo] + in_block[e];
            own_end = own_first;                           // (empty until the set-up stands)
            k = lo / blocks_per_view;
            f = (long long)(lo - k * blocks_per_view) * SP_BLOCK + e;
            if (f >= F || !face_setup(vertices, M, faces, (int)f, vd[k], H, W, zmin, cull, s)) continue;
            own_end = own_first + rect_tiles(s);
        }
        const ViewD& w = vd[k];
        const long long tile = item - own_first;
        const int tx0 = s.c0 / MR_TW, across = s.c1 / MR_TW - tx0 + 1;
        const long long ty = tile / across;
        const int col = (tx0 + (int)(tile - ty * across)) * MR_TW + lx;
        const long long row = (long long)(s.r0 / MR_TH + ty) * MR_TH + ly;
        const bool in_rect = col >= s.c0 && col <= s.c1 && row >= s.r0 && row <= s.r1;
        double E[3], S, z;
        const bool covered = pixel_test(s, w, (int)row, col, zmin, E, S, z) && in_rect;       // (lanes beside the rectangle test and discard)
        unsigned long long* slot = keys + (size_t)k * HW + (size_t)(in_rect ? row * W + col : 0);
        const unsigned long long key = key_nearest((float)z, (uint32_t)f);
#ifdef SP_MESH_RENDER_COUNTERS
        // the measuring build (tools/mesh_render_bench.py --lib): key_offer spelled out, the keys offered and the atomics issued counted
        // per wave into words 1 and 2 of the scratch's first unit, which the call zeroes
        const bool issued = covered && __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key;
        if (issued) atomicMax(slot, key);
        const unsigned long long offered_mask = __ballot(covered), issued_mask = __ballot(issued);
        if (lane == 0 && offered_mask) {
            atomicAdd(const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(total_at)) + 1, (unsigned long long)__popcll(offered_mask));
            atomicAdd(const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(total_at)) + 2, (unsigned long long)__popcll(issued_mask));
        }
#else
        if (covered) key_offer(slot, key);
#endif
    }
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------------
// grid ceil(V H W / 256), block SP_BLOCK: one thread per pixel
__global__ __launch_bounds__(SP_BLOCK) void k_mr_resolve(const float* __restrict__ vertices, const float* __restrict__ vertex_colours, int M,
                                                         const int32_t* __restrict__ faces, const float* __restrict__ face_normals,
                                                         const SpView* __restrict__ views, int H, int W, float z_min,
                                                         const unsigned long long* __restrict__ keys, long long n_pix, float* __restrict__ depth,
                                                         float* __restrict__ normals, uint8_t* __restrict__ image, int32_t* __restrict__ index) {
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (at >= n_pix) return;
    const unsigned long long key = keys[at];
    const int f = key_nearest_id(key);
    if (index) index[at] = f;
    if (depth) depth[at] = key_nearest_z(key);             // the winner's float32(z): the rule's own value, carried by the key
    if (normals) {
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) normals[3 * (size_t)at + ax] = f >= 0 ? face_normals[3 * (size_t)f + ax] : nan;
    }
    if (image) {
        uint8_t rgb[3] = {0, 0, 0};
        if (f >= 0) {
            const long long HW = (long long)H * W;
            const long long v = at / HW, pix = at - v * HW;
            const int row = (int)(pix / W), col = (int)(pix - (long long)row * W);
            ViewD w;
            view_setup(views[v], w);
            FaceSetup s;
            double E[3], S, z;
            // (the winner passed both in the raster pass: the same arithmetic passes again; cull = 0 leaves det's sign to pixel_test)
            if (face_setup(vertices, M, faces, f, w, H, W, (double)z_min, 0, s) && pixel_test(s, w, row, col, (double)z_min, E, S, z)) {
                const double l0 = E[0] / S, l1 = E[1] / S, l2 = E[2] / S;
                const size_t i0 = 3 * (size_t)faces[3 * (size_t)f], i1 = 3 * (size_t)faces[3 * (size_t)f + 1], i2 = 3 * (size_t)faces[3 * (size_t)f + 2];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double c = (l0 * (double)vertex_colours[i0 + ch] + l1 * (double)vertex_colours[i1 + ch]) + l2 * (double)vertex_colours[i2 + ch];
                    rgb[ch] = colour_u8((float)c);
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) image[3 * (size_t)at + ch] = rgb[ch];
    }
}

struct RenderLayout { long long blocks_per_view, block_units, prefix_units; };

// F in 1 .. SP_MESH_MAX_FACES.  The scratch: one unit for the total | one int64 per entry block | one int64 per entry, for one chunk of views
RenderLayout render_layout(long long F) {
    RenderLayout l;
    l.blocks_per_view = (F + SP_BLOCK - 1) / SP_BLOCK;
    l.block_units = (l.blocks_per_view * MR_CHUNK + 7) / 8;
    l.prefix_units = l.blocks_per_view * MR_CHUNK * (SP_BLOCK / 8);
    return l;
}

}  // namespace

extern "C" {

int sp_mesh_render_scratch_units(long long F) {
    if (F < 1) return SP_EINVAL;
    if (F > SP_MESH_MAX_FACES) return SP_ELIMIT;
    const RenderLayout l = render_layout(F);
    return (int)(1 + l.block_units + l.prefix_units);      // 1 + 2^21 + 2^29 at the limit
}

int sp_mesh_render(const float* vertices, const float* vertex_colours, long long M, const int32_t* faces, long long F,
                   const float* face_normals, const SpView* views, int V, int H, int W, float z_min, int cull, void* scratch,
                   unsigned long long* keys, float* depth, float* normals, uint8_t* image, int32_t* index, void* stream) {
    if (!vertices || !faces || !views || !scratch || !keys || ((uintptr_t)scratch & 7) || ((uintptr_t)keys & 7)) return SP_EINVAL;
    if (!depth && !normals && !image && !index) return SP_EINVAL;
    if ((image && !vertex_colours) || (normals && !face_normals)) return SP_EINVAL;
    if (((uintptr_t)vertices & 3) || ((uintptr_t)faces & 3) || ((uintptr_t)views & 3) || ((uintptr_t)vertex_colours & 3) ||
        ((uintptr_t)face_normals & 3) || ((uintptr_t)depth & 3) || ((uintptr_t)normals & 3) || ((uintptr_t)index & 3))
        return SP_EINVAL;
    if (F < 1 || M < 1 || V < 1 || H < 1 || W < 1 || !(z_min >= 0.f) || (cull != 0 && cull != 1)) return SP_EINVAL;
    if (F > SP_MESH_MAX_FACES || M > SP_MESH_MAX_FACES || view_limits(V, H, W)) return SP_ELIMIT;
    const RenderLayout l = render_layout(F);
    long long* total = static_cast<long long*>(scratch);
    long long* blocks = total + 8;
    long long* prefix = blocks + 8 * (size_t)l.block_units;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W, n_pix = (long long)V * HW;
    const hipError_t e = keys_clear(keys, n_pix, s);
    if (e != hipSuccess) return (int)e;
    const long long tiles = (long long)((W + MR_TW - 1) / MR_TW) * ((H + MR_TH - 1) / MR_TH);      // of a whole image
#ifdef SP_MESH_RENDER_COUNTERS
    if (hipMemsetAsync(scratch, 0, 64, s) != hipSuccess) return SP_EINVAL;
#endif
    for (int v0 = 0; v0 < V; v0 += MR_CHUNK) {
        const int nv = V - v0 < MR_CHUNK ? V - v0 : MR_CHUNK;
        const long long n_blocks = l.blocks_per_view * nv;
        hipLaunchKernelGGL(k_mr_count, dim3((unsigned)l.blocks_per_view, (unsigned)nv), dim3(SP_BLOCK), 0, s, vertices, (int)M, faces, (int)F,
                           views + v0, H, W, z_min, cull, prefix, blocks);
        SP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mr_scan, dim3(1), dim3(SP_BLOCK), 0, s, blocks, n_blocks, total);
        SP_CHECK_LAUNCH();
        // the host does not know the number of items, only that it is at most every entry on every tile: a small call takes a small grid
        const long long entries = n_blocks * SP_BLOCK, full = (long long)MR_GRID * SP_WAVES;
        const long long most = entries >= full || tiles >= full ? full : entries * tiles;
        const long long grid = (most + SP_WAVES - 1) / SP_WAVES;
        hipLaunchKernelGGL(k_mr_raster, dim3((unsigned)(grid < MR_GRID ? grid : MR_GRID)), dim3(SP_BLOCK), 0, s, vertices, (int)M, faces, (int)F,
                           views + v0, nv, H, W, z_min, cull, prefix, blocks, (int)l.blocks_per_view, total, keys + (size_t)v0 * HW);
        SP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_mr_resolve, pixel_grid(n_pix), dim3(SP_BLOCK), 0, s, vertices, vertex_colours, (int)M, faces, face_normals, views, H, W,
                       z_min, keys, n_pix, depth, normals, image, index);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
