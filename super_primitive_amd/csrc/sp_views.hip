// Map views: a point set rendered into camera views (tool/viz.py:163-190 project_points_np / render_pcd, as gui/sfm_gui.py:460-468 uses
// it, plus a depth-buffer mode the reference does not have) and depth images lifted into a point cloud (tool/viz.py:30-51
// depth_image_lift, i.e. Open3D's PointCloud.create_from_depth_image with depth_scale 1, stride 1, then transform).
//
// sp_render_views, sp_render_splats and sp_render_surfels check their own arguments and share everything after that (render_launch): the
// limits and the launch tail of sp_map_device.h -- the empty keys, ONE key pass, and the resolve pass.  The key pass is k_view_keys, a
// template on "a point is a pixel" / "a point is a footprint" / "a point is an oriented footprint".
//
// Key pass, common part: one thread per point, its three floats staged through LDS (one coalesced read of the workgroup's 3 x 256
// floats), then a loop over the views.  Every 16 views the workgroup forms their float64 numbers once into LDS -- R^T (9), t (3), fx, fy,
// cx, cy and an "identity pose" flag -- so the per-view operands are wave-uniform LDS broadcasts.  Arithmetic in float64 from the float32
// inputs, every operation rounded on its own (contraction is switched off for this file: the reference is NumPy in float64):
//     d = p - t;   p_c = ((Rt0 d0 + Rt1 d1) + Rt2 d2) per row   (an exact identity pose skips both: p_c = p, as render_pcd has it --
//     0 x inf would otherwise turn a point at z = inf, which the reference keeps, into NaN);   u = x fx / z + cx;   v = y fy / z + cy.
// A kept (point, view) offers its key to its pixels (key_offer; the two key forms, their decoders and why float32 z orders as an
// integer are in sp_map_device.h).
//     pixel, mode 0  kept iff 0 <= u < W and 0 <= v < H (NaN and +-inf fail), pixel (trunc v, trunc u); the "highest id" key: NumPy's
//                    repeated-index assignment; no test on z at all
//     pixel, mode 1  the same test, then z > z_min >= 0; the "nearest" key
//     footprint      (sp_render_splats; the radius staged through LDS beside the coordinates, in this instantiation only) z > z_min and
//                    finite u, v; the half-widths ru = (r fx) / z, rv = (r fy) / z in float64, not >= 0 -> 0, capped at max_px; the
//                    thread loops over the pixels whose cell meets [u - ru, u + ru] x [v - rv, v + rv], clipped to the image (bounds
//                    clamped in float64 before the conversion: at most 33 x 33) with the point's one "nearest" key: a splat is flat
//     surfel         (sp_render_surfels; normals staged beside coordinates and radii, in this instantiation only) the footprint's test
//                    and rectangle, so coverage is identical.  Per (point, view) the normal is turned into the view once and
//                    s = n_c . p_c formed once; the row's b sits in the outer loop, the inner loop has one float64 division, one key
//                    and one offer per pixel.  A point without a usable normal takes the footprint's flat loop
// Resolve pass: one thread per pixel decodes the winner: index (or -1), depth = float32 z (or 0), image = trunc(c * 255) from the exact
// float64 product, clamped to 0 .. 255, NaN -> 0 (or 0, 0, 0).  Integer maxima commute: two runs give the same bits.
//
// sp_map_consistency.  The same projection (camera_point / pixel_of of sp_map_device.h, one pair of functions for every kernel), no keys: one
// lane per point, 32 views per workgroup in LDS, and per seen (point, view) a gather of the (2 window + 1)^2 depths around its pixel
// from the V depth images, which every workgroup re-reads (they stay in L2 / the Infinity Cache).  Each pair is one of agree, in front,
// behind or unseen; three integer counters per point in registers, stored plainly when V fits one chunk, else added by integer
// atomicAdd onto zeroed counts.  Integers: two runs give the same bits.
//
// sp_image_metrics.  One launch, grid (ceil(H W / 1024), V): per counted pixel (index >= 0) and channel d = |rendered - u8(target)| with
// the resolve pass's conversion; n, sum d and sum d^2 as 32-bit integers per thread, wave (lane swaps) and workgroup (LDS), then one 64-bit
// integer atomicAdd per workgroup and quantity.  Integers: exact, whatever the order.
//
// sp_depth_lift.  Ordered compaction (block_rank / block_count_scan of sp_map_device.h), three plain passes, no workgroup waits on
// another: (1) per 256-pixel block of one image the number of valid pixels (0 < d <= depth_trunc; NaN invalid); (2) one workgroup scans
// the block counts in place (exclusive) and writes offsets and counts; (3) every block recomputes its ranks and writes its valid pixels
// at block offset + rank: row-major order, image after image.  Point arithmetic in float64, every operation rounded on its own, rounded
// to float32 once at the end:
//     x = ((c - cx) d) / fx;   y = ((r - cy) d) / fy;   z = d;   world = ((T0 x + T1 y) + T2 z) + T3 per row (no pose: the point itself).
#include <type_traits>
#define SP_MAP_DEVICE_RESOLVE                       // this file launches k_render_resolve
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

enum KeyKind { KEY_PIXEL, KEY_FOOTPRINT, KEY_SURFEL };     // what a point is to k_view_keys

// the radii and the normals of a workgroup's points: LDS that only the instantiations of k_view_keys that read them have
template <bool HAS>
__device__ __forceinline__ float* radius_stage() {
    if constexpr (!HAS) return nullptr;
    else { __shared__ float sr[SP_BLOCK]; return sr; }
}
template <bool HAS>
__device__ __forceinline__ float* normal_stage() {
    if constexpr (!HAS) return nullptr;
    else { __shared__ float sn[3 * SP_BLOCK]; return sn; }
}

// k_view_keys' last argument: `mode` for the pixel and the footprint kind, what the surfel kind alone reads for that one
struct SurfelArgs { int cull; const float* normals; };
template <KeyKind KIND> using KeyLast = std::conditional_t<KIND == KEY_SURFEL, SurfelArgs, int>;

// grid ceil(Q / 256), block SP_BLOCK: the key pass of sp_render_views (KEY_PIXEL: one pixel per kept (point, view), mode 0 or 1), of
// sp_render_splats (KEY_FOOTPRINT: mode 1 with a rectangle of pixels per kept (point, view), at most 33 x 33; `mode` is not read) and of
// sp_render_surfels (KEY_SURFEL: that rectangle -- the same lines, so coverage is identical --, the depth of every covered pixel taken
// on the point's tangent plane; a point without a usable normal takes the footprint's flat loop).  `last` comes after the arguments the
// footprint pass had before the passes became one, and is `mode` for the first two kinds: their instantiations are then those passes
// instruction for instruction, pixel loops at the same offsets.  Those short loops (load, compare, atomic) are sensitive to where they
// fall: the same instructions 16 bytes earlier cost 2 - 4 % at large footprints (profiles/map_kernels_refactor.txt)
template <KeyKind KIND>
__global__ __launch_bounds__(SP_BLOCK) void k_view_keys(const float* __restrict__ points, const float* __restrict__ radii, int Q,
                                                        const SpView* __restrict__ views, int V, int H, int W, float z_min,
                                                        int max_px, unsigned long long* __restrict__ keys, KeyLast<KIND> last) {
    __shared__ float sp[3 * SP_BLOCK];
    __shared__ ViewD vd[VIEW_CHUNK];
    float* sr = radius_stage<KIND != KEY_PIXEL>();
    float* sn = normal_stage<KIND == KEY_SURFEL>();
    const int tid = threadIdx.x;
    // the workgroups take the points from the END of the set: in mode 0 the highest index wins, so the early workgroups set keys that
    // most later points lose against, and the load before the atomic skips them (ascending, every point would beat what it finds);
    // in mode 1 equal float32 z goes to the highest index
    const long long first = (long long)(gridDim.x - 1 - blockIdx.x) * SP_BLOCK;
    const int n = (int)((long long)Q - first < SP_BLOCK ? (long long)Q - first : SP_BLOCK);
    for (int j = tid; j < 3 * n; j += SP_BLOCK) {
        sp[j] = points[3 * first + j];
        if constexpr (KIND == KEY_SURFEL) sn[j] = last.normals[3 * first + j];
    }
    if (KIND != KEY_PIXEL && tid < n) sr[tid] = radii[first + tid];
    const size_t HW = (size_t)H * W;
    const double Wd = (double)W, Hd = (double)H, zmin = (double)z_min;
    const uint32_t id = (uint32_t)(first + tid);           // (Q <= 2^31 - 2)
    for (int v0 = 0; v0 < V; v0 += VIEW_CHUNK) {
        const int nv = V - v0 < VIEW_CHUNK ? V - v0 : VIEW_CHUNK;
        __syncthreads();                                   // (sp, sr, sn are written; the previous chunk has been read)
        if (tid < nv) view_setup(views[v0 + tid], vd[tid]);
        __syncthreads();
        if (tid >= n) continue;
        const double px = (double)sp[3 * tid], py = (double)sp[3 * tid + 1], pz = (double)sp[3 * tid + 2];
        const double rad = KIND != KEY_PIXEL ? (double)sr[tid] : 0.0, cap = (double)max_px;       // (footprints and surfels only)
        double n0 = 0.0, n1 = 0.0, n2 = 0.0, h = 0.0;      // (surfels only: the normal, usable or not, and the reach of the clamp)
        bool usable = false;
        if constexpr (KIND == KEY_SURFEL) {
            const float nf0 = sn[3 * tid], nf1 = sn[3 * tid + 1], nf2 = sn[3 * tid + 2];
            usable = fabsf(nf0) < HUGE_VALF && fabsf(nf1) < HUGE_VALF && fabsf(nf2) < HUGE_VALF && (nf0 != 0.f || nf1 != 0.f || nf2 != 0.f);
            n0 = (double)nf0; n1 = (double)nf1; n2 = (double)nf2;
            h = 2.0 * (rad >= 0.0 ? rad : 0.0);            // a disc reaching the square's corners stays within z -+ 2 rad however it is tilted
        }
        for (int k = 0; k < nv; ++k) {
            const ViewD& w = vd[k];
            double x, y, z, u, v;
            camera_point(w, px, py, pz, x, y, z);
            pixel_of(w, x, y, z, u, v);
            unsigned long long* view_keys = keys + (size_t)(v0 + k) * HW;
            if constexpr (KIND == KEY_PIXEL) {
                if (!(u >= 0.0 && u < Wd && v >= 0.0 && v < Hd)) continue;
                if (last == 1 && !(z > zmin)) continue;
                key_offer(view_keys + (size_t)(int)v * W + (size_t)(int)u, last == 1 ? key_nearest((float)z, id) : key_highest_id((float)z, id));
            } else {
                if (!(z > zmin) || !(fabs(u) < HUGE_VAL) || !(fabs(v) < HUGE_VAL)) continue;
                const double ru = half_width((rad * w.fx) / z, cap), rv = half_width((rad * w.fy) / z, cap);
                const double ul = u - ru, uh = u + ru, vl = v - rv, vh = v + rv;
                if (!(uh >= 0.0 && ul < Wd && vh >= 0.0 && vl < Hd)) continue;
                // clamped in float64, then converted: 0 <= c0 <= c1 <= W - 1 and 0 <= r0 <= r1 <= H - 1
                const int c0 = (int)fmax(floor(ul), 0.0), c1 = (int)fmin(floor(uh), Wd - 1.0);
                const int r0 = (int)fmax(floor(vl), 0.0), r1 = (int)fmin(floor(vh), Hd - 1.0);
                if constexpr (KIND == KEY_SURFEL) {
                    if (usable) {                          // a depth per pixel, on the tangent plane
                        double nc0 = n0, nc1 = n1, nc2 = n2;                             // n_c = R^T n; an exact identity pose leaves it untouched
                        if (!w.ident) {
                            nc0 = (w.Rt[0] * n0 + w.Rt[1] * n1) + w.Rt[2] * n2;
                            nc1 = (w.Rt[3] * n0 + w.Rt[4] * n1) + w.Rt[5] * n2;
                            nc2 = (w.Rt[6] * n0 + w.Rt[7] * n1) + w.Rt[8] * n2;
                        }
                        const double s = (nc0 * x + nc1 * y) + nc2 * z;
                        if (last.cull && s >= 0.0) continue;                             // the surface seen from behind
                        const double tl = z - h, th = z + h;
                        for (int r = r0; r <= r1; ++r) {
                            const double b = (((double)r + 0.5) - w.cy) / w.fy;
                            unsigned long long* row_keys = view_keys + (size_t)r * W;
                            for (int c = c0; c <= c1; ++c) {
                                const double a = (((double)c + 0.5) - w.cx) / w.fx;
                                const double den = (nc0 * a + nc1 * b) + nc2;
                                double t = s / den;
                                if (t != t) t = z;
                                if (t < tl) t = tl;
                                if (t > th) t = th;
                                if (t > zmin && t < HUGE_VAL) key_offer(row_keys + c, key_nearest((float)t, id));
                            }
                        }
                        continue;
                    }
                }
                const unsigned long long key = key_nearest((float)z, id);                // a splat is flat: the point's one key
                for (int r = r0; r <= r1; ++r)
                    for (int c = c0; c <= c1; ++c) key_offer(view_keys + (size_t)r * W + c, key);
            }
        }
    }
}

constexpr int CONS_CHUNK = 32;                            // views per workgroup of k_map_consistency

// grid (ceil(Q / 256), ceil(V / CONS_CHUNK)), block SP_BLOCK: one lane per point, the chunk's views in LDS (wave-uniform broadcasts),
// the three counters in registers.  The test on z comes before the two divisions, so a point behind the camera pays for neither.
// The window is a template argument (0, 1, 2): its 1, 9 or 25 loads are unrolled and in flight together.
// add = 0: the one chunk stores its counters; add = 1: counts is zeroed and every chunk adds what it found (integers: any order).
template <int WIN>
__global__ __launch_bounds__(SP_BLOCK) void k_map_consistency(const float* __restrict__ points, const int32_t* __restrict__ owner, int Q,
                                                              const SpView* __restrict__ views, const int32_t* __restrict__ view_owner, int V,
                                                              const float* __restrict__ depth, int H, int W, float tol, float z_min,
                                                              int32_t* __restrict__ counts, int add) {
    __shared__ ViewD vd[CONS_CHUNK];
    __shared__ int32_t vown[CONS_CHUNK];
    const int tid = threadIdx.x;
    const int v0 = blockIdx.y * CONS_CHUNK;
    const int nv = V - v0 < CONS_CHUNK ? V - v0 : CONS_CHUNK;
    if (tid < nv) {
        view_setup(views[v0 + tid], vd[tid]);
        vown[tid] = view_owner ? view_owner[v0 + tid] : -1;
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * SP_BLOCK + tid;
    if (i >= Q) return;
    const double px = (double)points[3 * i], py = (double)points[3 * i + 1], pz = (double)points[3 * i + 2];
    const int own = owner ? owner[i] : -1;
    const size_t HW = (size_t)H * W;
    const double Wd = (double)W, Hd = (double)H, zmin = (double)z_min, tol64 = (double)tol;
    int n_agree = 0, n_front = 0, n_behind = 0;
    for (int k = 0; k < nv; ++k) {
        if (own >= 0 && own == vown[k]) continue;          // the point's own keyframe: skipped
        const ViewD& w = vd[k];
        double x, y, z, u, v;
        camera_point(w, px, py, pz, x, y, z);
        if (!(z > zmin)) continue;
        pixel_of(w, x, y, z, u, v);
        if (!(u >= 0.0 && u < Wd && v >= 0.0 && v < Hd)) continue;
        const int r = (int)v, c = (int)u;                  // 0 <= r < H, 0 <= c < W
        const double zf = (double)(float)z;
        const float* img = depth + (size_t)(v0 + k) * HW;
        // the window's depths first (all loads in flight together; a pixel outside the image reads as 0: no surface), then the rule
        constexpr int SIDE = 2 * WIN + 1;
        float d[SIDE * SIDE];
#pragma unroll
        for (int dr = -WIN; dr <= WIN; ++dr) {
            const int rr = r + dr, rc = rr < 0 ? 0 : (rr > H - 1 ? H - 1 : rr);
#pragma unroll
            for (int dc = -WIN; dc <= WIN; ++dc) {
                const int cc = c + dc, ccl = cc < 0 ? 0 : (cc > W - 1 ? W - 1 : cc);
                const float val = img[(size_t)rc * W + ccl];
                d[(dr + WIN) * SIDE + dc + WIN] = rr == rc && cc == ccl ? val : 0.f;
            }
        }
        bool any = false, agree = false, all_front = true;
#pragma unroll
        for (int j = 0; j < SIDE * SIDE; ++j) {
            const bool valid = d[j] > 0.f && d[j] < HUGE_VALF;             // 0, negative, NaN, inf: no surface (float32 to float64 is exact)
            const double D = (double)d[j], b = tol64 * D;
            any = any || valid;
            agree = agree || (valid && fabs(zf - D) <= b);
            all_front = all_front && (!valid || zf < D - b);
        }
        if (!any) continue;
        if (agree) ++n_agree;
        else if (all_front) ++n_front;
        else ++n_behind;
    }
    int32_t* out = counts + 3 * i;
    if (!add) {
        out[0] = n_agree; out[1] = n_front; out[2] = n_behind;
    } else {
        if (n_agree) atomicAdd(out, n_agree);
        if (n_front) atomicAdd(out + 1, n_front);
        if (n_behind) atomicAdd(out + 2, n_behind);
    }
}

constexpr int METRIC_PIX = 4;                              // pixels per thread of k_image_metrics

// grid (ceil(H W / 1024), V), block SP_BLOCK: n, sum |a - b| and sum (a - b)^2 over the counted pixels of one view, three channels each.
// A thread's 4 pixels give at most 4 x 3 x 255^2 < 2^20, a workgroup's 256 threads < 2^28: 32-bit sums until the one 64-bit atomic
__global__ __launch_bounds__(SP_BLOCK) void k_image_metrics(const uint8_t* __restrict__ rendered, const float* __restrict__ target,
                                                            const int32_t* __restrict__ index, int HW, unsigned long long* __restrict__ out) {
    __shared__ uint32_t part[SP_WAVES][3];
    const int view = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)view * HW;
    uint32_t s[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < METRIC_PIX; ++j) {
        const long long p = ((long long)blockIdx.x * METRIC_PIX + j) * SP_BLOCK + tid;
        if (p >= HW || index[base + p] < 0) continue;
        s[0] += 1u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int a = (int)rendered[3 * (base + p) + ch];
            const int b = (int)colour_u8(target[(3 * (size_t)view + ch) * HW + p]);
            const int d = a > b ? a - b : b - a;
            s[1] += (uint32_t)d;
            s[2] += (uint32_t)(d * d);
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s[q] += (uint32_t)__shfl_xor((int)s[q], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) part[tid >> 6][q] = s[q];
    }
    __syncthreads();
    if (tid < 3) {
        const uint32_t sum = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        if (sum) atomicAdd(out + 3 * (size_t)view + tid, (unsigned long long)sum);
    }
}

// ---- depth lift ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lift_valid(float d, float depth_trunc) { return d > 0.f && d <= depth_trunc; }

// grid (ceil(H W / 256), B)
__global__ __launch_bounds__(SP_BLOCK) void k_lift_count(const float* __restrict__ depth, int HW, float depth_trunc,
                                                         int32_t* __restrict__ block_counts) {
    __shared__ int wc[SP_WAVES];
    const int p = blockIdx.x * SP_BLOCK + threadIdx.x;
    const bool ok = p < HW && lift_valid(depth[(size_t)blockIdx.y * HW + p], depth_trunc);
    const int count = block_rank(ok, wc).count;
    if (threadIdx.x == 0) block_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = count;
}

// one workgroup: bc[n] (n = B nblk) becomes its exclusive prefix sum; offsets[b] = the prefix at image b's first block, offsets[B] the
// total, counts[b] = offsets[b + 1] - offsets[b]
__global__ __launch_bounds__(SP_BLOCK) void k_lift_scan(int32_t* __restrict__ bc, int n, int nblk, int B, int32_t* __restrict__ counts,
                                                        long long* __restrict__ offsets) {
    __shared__ long long part[SP_BLOCK];
    const long long total = block_count_scan(bc, n, part, [=](long long j, long long prefix) {
        if (j % nblk == 0) offsets[j / nblk] = prefix;
    });
    if (threadIdx.x == 0) offsets[B] = total;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += SP_BLOCK) counts[b] = (int32_t)(offsets[b + 1] - offsets[b]);
}

// grid (ceil(H W / 256), B)
__global__ __launch_bounds__(SP_BLOCK) void k_lift_write(const float* __restrict__ depth, const float* __restrict__ K,
                                                         const float* __restrict__ pose, const float* __restrict__ image, int HW, int W,
                                                         float depth_trunc, const int32_t* __restrict__ block_offsets,
                                                         float* __restrict__ points, float* __restrict__ colours,
                                                         int32_t* __restrict__ pixel) {
    __shared__ int wc[SP_WAVES];
    const int b = blockIdx.y;
    const int p = blockIdx.x * SP_BLOCK + threadIdx.x;
    const float df = p < HW ? depth[(size_t)b * HW + p] : 0.f;
    const bool ok = p < HW && lift_valid(df, depth_trunc);
    const int rank = block_rank(ok, wc).rank;
    if (!ok) return;
    const size_t row = (size_t)block_offsets[(size_t)b * gridDim.x + blockIdx.x] + (size_t)rank;
    const float* Kb = K + 9 * (size_t)b;
    const double fx = (double)Kb[0], fy = (double)Kb[4], cx = (double)Kb[2], cy = (double)Kb[5];
    const int r = p / W, c = p - r * W;
    const double d = (double)df;
    double x = (((double)c - cx) * d) / fx;
    double y = (((double)r - cy) * d) / fy;
    double z = d;
    if (pose) {
        const float* T = pose + 16 * (size_t)b;
        const double wx = (((double)T[0] * x + (double)T[1] * y) + (double)T[2] * z) + (double)T[3];
        const double wy = (((double)T[4] * x + (double)T[5] * y) + (double)T[6] * z) + (double)T[7];
        const double wz = (((double)T[8] * x + (double)T[9] * y) + (double)T[10] * z) + (double)T[11];
        x = wx; y = wy; z = wz;
    }
    points[3 * row] = (float)x;
    points[3 * row + 1] = (float)y;
    points[3 * row + 2] = (float)z;
    if (colours) {
        const float* img = image + 3 * (size_t)b * HW + p;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) colours[3 * row + ch] = img[(size_t)ch * HW];
    }
    pixel[row] = p;
}

// what sp_render_views (radii = NULL), sp_render_splats (normals = NULL) and sp_render_surfels launch once their own arguments are
// checked: the limits, then the depth buffer's launch tail around the key pass of their kind.  The kind is told by two argument pairs:
// (radii, max_px) is (NULL, 0) for pixels, (normals, cull) is (NULL, 0) for pixels and footprints; a pair given makes the kind
int render_launch(const float* points, const float* colours, long long Q, const SpView* views, int V, int H, int W, int mode, float z_min,
                  const float* radii, int max_px, const float* normals, int cull, unsigned long long* keys, uint8_t* image, float* depth,
                  int32_t* index, void* stream) {
    if (view_limits(V, H, W, Q)) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return depth_buffer_launch(keys, colours, (long long)V * H * W, mode, image, depth, index, s, [&] {
        const dim3 grid((unsigned)((Q + SP_BLOCK - 1) / SP_BLOCK)), block(SP_BLOCK);
        if (normals)
            hipLaunchKernelGGL(k_view_keys<KEY_SURFEL>, grid, block, 0, s, points, radii, (int)Q, views, V, H, W, z_min, max_px, keys,
                               SurfelArgs{cull, normals});
        else
            hipLaunchKernelGGL(radii ? k_view_keys<KEY_FOOTPRINT> : k_view_keys<KEY_PIXEL>, grid, block, 0, s, points, radii, (int)Q, views, V, H,
                               W, z_min, max_px, keys, mode);
    });
}

}  // namespace

extern "C" {

int sp_render_views(const float* points, const float* colours, long long Q, const SpView* views, int V, int H, int W, int mode, float z_min,
                    unsigned long long* keys, uint8_t* image, float* depth, int32_t* index, void* stream) {
    if (!points || !views || !keys || (image && !colours)) return SP_EINVAL;
    if (Q <= 0 || V <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1) || !(z_min >= 0.f)) return SP_EINVAL;
    return render_launch(points, colours, Q, views, V, H, W, mode, z_min, nullptr, 0, nullptr, 0, keys, image, depth, index, stream);
}

int sp_render_splats(const float* points, const float* colours, long long Q, const SpView* views, int V, int H, int W, float z_min,
                     const float* radii, int max_px, unsigned long long* keys, uint8_t* image, float* depth, int32_t* index, void* stream) {
    if (!points || !views || !keys || !radii || (image && !colours)) return SP_EINVAL;
    if (Q <= 0 || V <= 0 || H <= 0 || W <= 0 || !(z_min >= 0.f) || max_px < 0 || max_px > 16) return SP_EINVAL;
    return render_launch(points, colours, Q, views, V, H, W, 1, z_min, radii, max_px, nullptr, 0, keys, image, depth, index, stream);
}

int sp_render_surfels(const float* points, const float* colours, const float* normals, long long Q, const SpView* views, int V, int H, int W,
                      float z_min, const float* radii, int max_px, int cull, unsigned long long* keys, uint8_t* image, float* depth,
                      int32_t* index, void* stream) {
    if (!points || !views || !keys || !radii || !normals || (image && !colours)) return SP_EINVAL;
    if (Q <= 0 || V <= 0 || H <= 0 || W <= 0 || !(z_min >= 0.f) || max_px < 0 || max_px > 16 || (cull != 0 && cull != 1)) return SP_EINVAL;
    return render_launch(points, colours, Q, views, V, H, W, 1, z_min, radii, max_px, normals, cull, keys, image, depth, index, stream);
}

int sp_map_consistency(const float* points, const int32_t* owner, long long Q, const SpView* views, const int32_t* view_owner, int V,
                       const float* depth, int H, int W, float tol, int window, float z_min, int32_t* counts, void* stream) {
    if (!points || !views || !depth || !counts || Q <= 0 || V <= 0 || H <= 0 || W <= 0) return SP_EINVAL;
    if (!(tol >= 0.f && tol < 1.f) || window < 0 || window > 2 || !(z_min >= 0.f)) return SP_EINVAL;
    if (view_limits(V, H, W, Q)) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (V + CONS_CHUNK - 1) / CONS_CHUNK;
    if (chunks > 1) {
        hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 3 * (size_t)Q, s);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((Q + SP_BLOCK - 1) / SP_BLOCK), (unsigned)chunks);
    const int add = chunks > 1 ? 1 : 0;
    if (window == 0)
        hipLaunchKernelGGL(k_map_consistency<0>, grid, dim3(SP_BLOCK), 0, s, points, owner, (int)Q, views, view_owner, V, depth, H, W, tol, z_min, counts, add);
    else if (window == 1)
        hipLaunchKernelGGL(k_map_consistency<1>, grid, dim3(SP_BLOCK), 0, s, points, owner, (int)Q, views, view_owner, V, depth, H, W, tol, z_min, counts, add);
    else
        hipLaunchKernelGGL(k_map_consistency<2>, grid, dim3(SP_BLOCK), 0, s, points, owner, (int)Q, views, view_owner, V, depth, H, W, tol, z_min, counts, add);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_image_metrics(const uint8_t* rendered, const float* target, const int32_t* index, int V, int H, int W, long long* out, void* stream) {
    if (!rendered || !target || !index || !out || V <= 0 || H <= 0 || W <= 0) return SP_EINVAL;
    if (view_limits(V, H, W)) return SP_ELIMIT;
    const long long HW = (long long)H * W;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(out, 0, sizeof(long long) * 3 * (size_t)V, s);
    if (e != hipSuccess) return (int)e;
    const long long per_block = (long long)METRIC_PIX * SP_BLOCK;
    hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)((HW + per_block - 1) / per_block), (unsigned)V), dim3(SP_BLOCK), 0, s, rendered, target,
                       index, (int)HW, reinterpret_cast<unsigned long long*>(out));
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_depth_lift_blocks(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return SP_EINVAL;
    if (view_limits(B, H, W)) return SP_ELIMIT;
    return (int)((long long)B * (((long long)H * W + SP_BLOCK - 1) / SP_BLOCK));
}

int sp_depth_lift(const float* depth, const float* K, const float* pose, const float* image, int B, int H, int W, float depth_trunc,
                  int32_t* block_counts, float* points, float* colours, int32_t* pixel, int32_t* counts, long long* offsets, void* stream) {
    if (!depth || !K || !block_counts || !points || !pixel || !counts || !offsets || ((image == nullptr) != (colours == nullptr)))
        return SP_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || !(depth_trunc > 0.f)) return SP_EINVAL;
    const int n = sp_depth_lift_blocks(B, H, W);
    if (n < 0) return n;
    const int HW = H * W, nblk = n / B;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_lift_count, dim3(nblk, B), dim3(SP_BLOCK), 0, s, depth, HW, depth_trunc, block_counts);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lift_scan, dim3(1), dim3(SP_BLOCK), 0, s, block_counts, n, nblk, B, counts, offsets);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lift_write, dim3(nblk, B), dim3(SP_BLOCK), 0, s, depth, K, pose, image, HW, W, depth_trunc, block_counts, points,
                       colours, pixel);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
