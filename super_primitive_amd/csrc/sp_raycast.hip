// Surface views: the signed-distance volume of sp_tsdf.hip ray-cast into depth, normal, colour and cell-index images of V cameras
// (sp_tsdf_raycast); the contract -- THE RULE every pixel follows -- is in include/sp_hip.h.
//
// One launch, one thread per pixel, nothing shared between threads but the view's float64 record (formed once per workgroup into LDS by
// view_setup, read as wave-uniform broadcasts), no atomics, no scratch: two runs give the same bits.
//
// Tiles.  A workgroup owns a 16 x 16 pixel tile of ONE view and each of its four waves an 8 x 8 quarter of it (lane = 8 row + col), not a
// 64-pixel row: the 64 rays of a wave stay within a few cells of each other as they walk through the volume, so the 16 dword gathers of
// a sample (8 tsdf, 8 weight) fall on few cache lines.  Tiles are numbered view after view, row-major.  The hardware deals consecutive
// workgroups to different XCDs, whose L2s are separate, so every XCD gets one contiguous run of the tile list (xcd_chunked_tile of
// sp_device.h; the grid is rounded up to 8 and the surplus workgroups leave at once): neighbouring tiles, whose rays cross the same cells,
// share an L2.  Speed only -- the pixels computed are the same; SP_RAYCAST_XCD_CHUNKS = 0 builds the plain order for the A/B of
// tools/tsdf_raycast_bench.py (profiles/tsdf_raycast.txt: the chunks take 6 % less time at 256^3 nodes and 16 views of 480 x 640).
//
// The clip.  The rule is stated over all k = 0 .. n_steps-1, and a sample outside the box of node centres is INVALID by the rule.  The
// kernel therefore skips every k it can prove invalid (clip_steps below) and runs the rule exactly over the remaining range; what it
// skips could neither end the ray nor serve as the valid sample before a hit, so no bit of the result changes.
//
// Rays of a wave end at different k and the loop runs until the wave's last lane ends; the state carried from step to step is the
// previous sample's value and validity and k.  Colour, cell index and normal are formed once per ray, after the march.
#include "sp_map_device.h"

#pragma clang fp contract(off)

#ifndef SP_RAYCAST_XCD_CHUNKS
#define SP_RAYCAST_XCD_CHUNKS 1
#endif

namespace {

constexpr int RAY_TILE = 8;                                // a wave's tile: 8 x 8 pixels
constexpr int RAY_BLOCK_TILE = 2 * RAY_TILE;               // a workgroup's: 2 x 2 of them
static_assert(RAY_TILE * RAY_TILE == 64 && SP_WAVES == 4, "one wave per 8 x 8 tile, four to a workgroup");

struct RayVolume {
    const float* tsdf;
    const float* weight;
    const float* colour;
    int nx, ny, nz;
    float voxel, ox, oy, oz, min_weight;
};

// the cell of a world point: its lower node and the point's position inside it, each in 0 .. 1
struct RayCell { int node; double fx, fy, fz; };

// g_a = (p_a - o_a) / voxel - 0.5, i_a = floor(g_a), f_a = g_a - i_a; false unless 0 <= i_a <= n_a - 2 on every axis (NaN and +-inf fail
// the comparisons, which are made on the float64 value before any conversion to an integer)
__device__ __forceinline__ bool ray_cell(const RayVolume& v, double px, double py, double pz, RayCell& c) {
    const double vx = (double)v.voxel;
    const double gx = (px - (double)v.ox) / vx - 0.5, gy = (py - (double)v.oy) / vx - 0.5, gz = (pz - (double)v.oz) / vx - 0.5;
    const double ix = floor(gx), iy = floor(gy), iz = floor(gz);
    if (!(ix >= 0.0 && ix <= (double)(v.nx - 2) && iy >= 0.0 && iy <= (double)(v.ny - 2) && iz >= 0.0 && iz <= (double)(v.nz - 2))) return false;
    c.node = ((int)iz * v.ny + (int)iy) * v.nx + (int)ix;  // < nx ny nz <= 2^30
    c.fx = gx - ix;
    c.fy = gy - iy;
    c.fz = gz - iz;
    return true;
}

// trilinear interpolation of the eight corner values (corner c has offset bits x = 1, y = 2, z = 4), lerps a + f (b - a): along x, then y,
// then z
__device__ __forceinline__ double ray_lerp(const float (&f)[8], const RayCell& c) {
    double x[4], y[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = (double)f[2 * k], b = (double)f[2 * k + 1];
        x[k] = a + c.fx * (b - a);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) y[k] = x[2 * k] + c.fy * (x[2 * k + 1] - x[2 * k]);
    return y[0] + c.fz * (y[1] - y[0]);
}

// the field in a cell: false unless all eight nodes are valid
__device__ __forceinline__ bool ray_field(const RayVolume& v, const RayCell& c, double& F) {
    const int nxy = v.nx * v.ny;
    float f[8];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = c.node + corner_offset(k, v.nx, nxy);
        f[k] = v.tsdf[j];
        ok = ok && node_valid(f[k], v.weight[j], v.min_weight);
    }
    F = ray_lerp(f, c);
    return ok;
}

// S(p): the sample of the rule
__device__ __forceinline__ bool ray_sample(const RayVolume& v, double px, double py, double pz, double& F) {
    RayCell c = {0, 0.0, 0.0, 0.0};
    F = 0.0;
    return ray_cell(v, px, py, pz, c) && ray_field(v, c, F);
}

// one colour channel in a cell (the cell is valid: the caller's sample was)
__device__ __forceinline__ double ray_colour(const RayVolume& v, const RayCell& c, int ch) {
    const int nxy = v.nx * v.ny;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = v.colour[3 * (size_t)(c.node + corner_offset(k, v.nx, nxy)) + ch];
    return ray_lerp(f, c);
}

// The range k0 <= k < k1 outside which every sample of the ray is INVALID by the rule, so that the march may leave it out.
// In exact arithmetic the ray is p_a(z) = d_a z + t_a with d_a = R_a0 xr + R_a1 yr + R_a2, and a valid sample has every p_a inside
// [centre of node 0, centre of node n_a - 1].  Everything rounded on the way -- d_a as computed here against the three products of
// world_point, z_k, the sample's own g_a, the slab arithmetic below -- moves a world coordinate by a few 2^-53 of
// |t_a| + |o_a| + A_a z_end + voxel n_a  (A_a = |R_a0 xr| + |R_a1 yr| + |R_a2|, z_end the last z of the march), and a quotient by a slope
// moves its z by that much over the slope: in world units the same again.  The box is widened by e_a = 2^-20 voxel + 2^-40 of that sum
// on either side -- thousands of times any of it --, so a z outside the widened slab of some axis has its sample outside the true box.
// On top comes one whole step on either side.  A slope of exactly 0 decides by t_a alone; a NaN bound constrains nothing; with a
// non-finite pose, ray or bound every sample is invalid anyway (p_a is not finite), so any range is right.
__device__ __forceinline__ void clip_steps(const ViewD& cam, const RayVolume& v, double xr, double yr, double z_start, double step, int n_steps,
                                           int& k0, int& k1) {
    const double z_end = z_start + (double)(n_steps - 1) * step, vx = (double)v.voxel;
    const double o[3] = {(double)v.ox, (double)v.oy, (double)v.oz};
    const int n[3] = {v.nx, v.ny, v.nz};
    double za = -HUGE_VAL, zb = HUGE_VAL;
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r0 = cam.Rt[a] * xr, r1 = cam.Rt[3 + a] * yr, r2 = cam.Rt[6 + a], t = cam.t[a];
        const double d = (r0 + r1) + r2, A = (fabs(r0) + fabs(r1)) + fabs(r2);
        const double e = vx * 0x1p-20 + 0x1p-40 * ((fabs(t) + fabs(o[a])) + (A * z_end + vx * (double)n[a]));
        const double lo = node_centre(0, vx, o[a]) - e, hi = node_centre(n[a] - 1, vx, o[a]) + e;
        if (d == 0.0) {
            if (!(t >= lo && t <= hi)) empty = true;
            continue;
        }
        const double z1 = (lo - t) / d, z2 = (hi - t) / d;
        if (!(z1 == z1 && z2 == z2)) continue;
        const double near = z1 < z2 ? z1 : z2, far = z1 < z2 ? z2 : z1;
        if (near > za) za = near;
        if (far < zb) zb = far;
    }
    k0 = 0;
    k1 = n_steps;
    if (empty || za > zb) {
        k1 = 0;
        return;
    }
    const double first = floor((za - z_start) / step) - 1.0, end = ceil((zb - z_start) / step) + 2.0;      // one step of margin either side
    if (first > 0.0) k0 = first >= (double)n_steps ? n_steps : (int)first;
    if (end < (double)n_steps) k1 = end > 0.0 ? (int)end : 0;
}

// grid: the tiles of all views (rounded up to 8 for the chunks), block SP_BLOCK
__global__ __launch_bounds__(SP_BLOCK) void k_tsdf_raycast(RayVolume vol, const SpView* __restrict__ views, int H, int W, int tiles_x, int tiles_per_view,
                                                           int n_tiles, float z_start, float step, int n_steps, float* __restrict__ depth,
                                                           float* __restrict__ normals, uint8_t* __restrict__ image, int32_t* __restrict__ index) {
    __shared__ ViewD cam_lds;
    const int tile = SP_RAYCAST_XCD_CHUNKS ? xcd_chunked_tile((int)blockIdx.x, n_tiles) : (int)blockIdx.x;
    if (tile >= n_tiles) return;                           // (uniform: the whole workgroup leaves)
    const int view = tile / tiles_per_view, in_view = tile - view * tiles_per_view;
    const int ty = in_view / tiles_x, tx = in_view - ty * tiles_x;
    if (threadIdx.x == 0) view_setup(views[view], cam_lds);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = ty * RAY_BLOCK_TILE + (wave >> 1) * RAY_TILE + (lane >> 3), col = tx * RAY_BLOCK_TILE + (wave & 1) * RAY_TILE + (lane & 7);
    if (row >= H || col >= W) return;
    const ViewD& cam = cam_lds;
    const double xr = ((double)col - cam.cx) / cam.fx, yr = ((double)row - cam.cy) / cam.fy;
    const double z0 = (double)z_start, st = (double)step;
    int k0, k1;
    clip_steps(cam, vol, xr, yr, z0, st, n_steps, k0, k1);
    // ---- the march: the first valid negative sample ends the ray
    double F_prev = 0.0, F_end = 0.0;
    bool valid_prev = false;                               // (sample k0 - 1 is invalid, or k0 = 0 and there is none)
    int k_end = -1;
    for (int k = k0; k < k1; ++k) {
        double px, py, pz, F;
        world_point(cam, xr, yr, z0 + (double)k * st, px, py, pz);
        const bool ok = ray_sample(vol, px, py, pz, F);
        if (ok && F < 0.0) {
            k_end = k;
            F_end = F;
            break;
        }
        valid_prev = ok;
        F_prev = F;
    }
    const bool hit = k_end >= 1 && valid_prev && F_prev >= 0.0;
    const size_t pix = ((size_t)view * H + row) * W + col;
    const float nan = __builtin_nanf("");
    float d_out = 0.f, n_out[3] = {nan, nan, nan};
    int32_t i_out = -1;
    uint8_t rgb[3] = {0, 0, 0};
    if (hit) {
        const double t = F_prev / (F_prev - F_end), z_before = z0 + (double)(k_end - 1) * st;
        const double zs = t * st + z_before;
        d_out = (float)zs;
        double px, py, pz;
        RayCell at_end = {0, 0.0, 0.0, 0.0};
        world_point(cam, xr, yr, z0 + (double)k_end * st, px, py, pz);
        ray_cell(vol, px, py, pz, at_end);                 // (valid: it ended the ray)
        i_out = at_end.node;
        if (image) {
            RayCell before = {0, 0.0, 0.0, 0.0};
            world_point(cam, xr, yr, z_before, px, py, pz);
            ray_cell(vol, px, py, pz, before);             // (valid: the hit asks for it)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double ca = ray_colour(vol, before, ch), cb = ray_colour(vol, at_end, ch);
                rgb[ch] = colour_u8((float)(ca + t * (cb - ca)));
            }
        }
        if (normals) {
            world_point(cam, xr, yr, zs, px, py, pz);
            const double h = (double)vol.voxel;
            double fp, fm, g[3];
            bool all = ray_sample(vol, px + h, py, pz, fp);
            all = ray_sample(vol, px - h, py, pz, fm) && all;
            g[0] = fp - fm;
            all = ray_sample(vol, px, py + h, pz, fp) && all;
            all = ray_sample(vol, px, py - h, pz, fm) && all;
            g[1] = fp - fm;
            all = ray_sample(vol, px, py, pz + h, fp) && all;
            all = ray_sample(vol, px, py, pz - h, fm) && all;
            g[2] = fp - fm;
            const double len = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
            if (all && len > 0.0 && len < HUGE_VAL) {
#pragma unroll
                for (int a = 0; a < 3; ++a) n_out[a] = (float)(g[a] / len);
            }
        }
    }
    if (depth) depth[pix] = d_out;
    if (index) index[pix] = i_out;
    if (normals) {
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[3 * pix + a] = n_out[a];
    }
    if (image) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) image[3 * pix + ch] = rgb[ch];
    }
}

}  // namespace

extern "C" {

int sp_tsdf_raycast(const float* tsdf, const float* weight, const float* colour, int nx, int ny, int nz, float voxel, float ox, float oy, float oz,
                    float min_weight, const SpView* views, int V, int H, int W, float z_start, float step, int n_steps, float* depth, float* normals,
                    uint8_t* image, int32_t* index, void* stream) {
    if (!tsdf || !weight || !views || (!depth && !normals && !image && !index) || (image && !colour)) return SP_EINVAL;
    if (nx < 2 || ny < 2 || nz < 2 || V < 1 || H < 1 || W < 1 || n_steps < 2) return SP_EINVAL;
    if (!(voxel > 0.f && finite_f(voxel)) || !(step > 0.f && finite_f(step)) || !(finite_f(ox) && finite_f(oy) && finite_f(oz))) return SP_EINVAL;
    if (min_weight != min_weight || !(z_start >= 0.f && finite_f(z_start))) return SP_EINVAL;
    if (view_limits(V, H, W) || volume_nodes(nx, ny, nz) < 0 || n_steps > SP_TSDF_RAYCAST_MAX_STEPS) return SP_ELIMIT;
    const int tiles_x = (W + RAY_BLOCK_TILE - 1) / RAY_BLOCK_TILE, tiles_y = (H + RAY_BLOCK_TILE - 1) / RAY_BLOCK_TILE;
    const long long n_tiles = (long long)V * tiles_x * tiles_y;                        // <= V H W < 2^31
    const long long grid = SP_RAYCAST_XCD_CHUNKS ? 8 * ((n_tiles + 7) / 8) : n_tiles;
    const RayVolume vol = {tsdf, weight, colour, nx, ny, nz, voxel, ox, oy, oz, min_weight};
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)grid), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), vol, views, H, W, tiles_x,
                       tiles_x * tiles_y, (int)n_tiles, z_start, step, n_steps, depth, normals, image, index);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
