// Map normals and oriented surfels (the contracts of sp_map_normals and sp_render_surfels in include/sp_hip.h).  All arithmetic is float64
// from the float32 inputs, every operation rounded on its own (contraction is switched off for this file: the reference is NumPy in
// float64), rounded to float32 once.
//
// sp_map_normals.  sp_map_points' walk (keyframe_of_block: sp_map_device.h; segment_of: sp_device.h), one thread per output row, a workgroup
// belongs to ONE keyframe.  The rotation -- composed with the alignment's rot_reanchor where there is one -- goes through LDS as 9 float64;
// the (row, 3) outputs are staged in LDS and written as runs of consecutive floats.  A row's neighbours are looked up at stride 1 in the
// row's own segment: left and right are the adjacent table points, up and down two binary searches of the segment's range (pix is
// strictly increasing there), the only divergent part, bounded by log2 of the segment's size.  No atomics, no workgroup waits on another.
//
// sp_render_surfels.  The footprint instantiation of k_view_keys (sp_views.hip) with a depth per covered pixel: the same staging of 256
// points and of 16-view chunks through LDS, normals staged beside coordinates and radii; camera_point / pixel_of / half_width and the
// rectangle are that kernel's, so coverage is identical.  Per (point, view) the normal is turned into the view once and s = n_c . p_c
// formed once; the row's b sits in the outer loop, the inner loop has one float64 division, one key and one offer per pixel.  The keys are
// sp_map_device.h's "nearest" keys and the resolve pass is the one of every depth buffer.
#include <math.h>
#define SP_MAP_DEVICE_RESOLVE                       // this file launches k_render_resolve
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

// the first table point of [lo, hi) whose pixel word (validity bit masked off) is at or beyond `want`: hi if there is none
__device__ __forceinline__ int pix_lower_bound(const uint32_t* __restrict__ pix, int lo, int hi, uint32_t want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((pix[mid] & 0x7fffffffu) < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// central difference with both neighbours (b = behind: left / up, a = ahead: right / down), one-sided with one, 0 with none
__device__ __forceinline__ double table_difference(const float* __restrict__ baseL, int i, int b, int a) {
    if (b >= 0 && a >= 0) return ((double)baseL[a] - (double)baseL[b]) / 2.0;
    if (a >= 0) return (double)baseL[a] - (double)baseL[i];
    if (b >= 0) return (double)baseL[i] - (double)baseL[b];
    return 0.0;
}

// grid total_blocks, block SP_BLOCK: k_map_points' walk
__global__ __launch_bounds__(SP_BLOCK) void k_map_normals(const SpMapKeyframe* __restrict__ kfs, int n_kf, int stride,
                                                          const SpTrajAlign* __restrict__ align, int n_align, float* __restrict__ normals,
                                                          long long total_rows) {
    __shared__ double Rm[9];                               // R' (row major)
    __shared__ float stage[3 * SP_BLOCK];
    const int tid = threadIdx.x, block = blockIdx.x;
    const int lo = keyframe_of_block(kfs, n_kf, block);
    const SpMapKeyframe kf = kfs[lo];
    const int Q = (int)(((long long)kf.P + stride - 1) / stride);
    const long long local0 = (long long)(block - kf.first_block) * SP_BLOCK;
    const long long row0 = kf.out_offset + local0;
    // rows of this workgroup that exist: inside the keyframe and inside the output
    long long n_rows = (long long)Q - local0;
    if (total_rows - row0 < n_rows) n_rows = total_rows - row0;
    if (n_rows > SP_BLOCK) n_rows = SP_BLOCK;
    if (n_rows < 0 || local0 < 0 || row0 < 0) n_rows = 0;
    if (tid < 9) {
        const int r = tid / 3, c = tid % 3;
        const float* T = kf.pose;
        double v = (double)T[4 * r + c];
        if (align && kf.align >= 0 && kf.align < n_align) {
            const SpTrajAlign& a = align[kf.align];
            v = (a.rot_reanchor[3 * r] * (double)T[c] + a.rot_reanchor[3 * r + 1] * (double)T[4 + c]) + a.rot_reanchor[3 * r + 2] * (double)T[8 + c];
        }
        Rm[tid] = v;
    }
    __syncthreads();
    if (tid < n_rows) {
        const int i = (int)(local0 + tid) * stride;        // table point (< P: the row is below Q)
        const int n = map_point_segment(kf, i);
        const int s0 = kf.seg_off[n], s1 = n + 1 < kf.N ? kf.seg_off[n + 1] : kf.P;      // the segment's table range, s0 <= i < s1
        const uint32_t w = kf.pix[i] & 0x7fffffffu;
        const int r = (int)(w >> 16), c = (int)(w & 0xffffu);
        // neighbours at stride 1, in this segment only: -1 where there is none
        int left = -1, right = -1, up = -1, down = -1;
        if (c > 0 && i - 1 >= s0 && (kf.pix[i - 1] & 0x7fffffffu) == w - 1u) left = i - 1;
        if (c < 0xffff && i + 1 < s1 && (kf.pix[i + 1] & 0x7fffffffu) == w + 1u) right = i + 1;
        if (r > 0) {
            const uint32_t want = w - 0x10000u;
            const int k = pix_lower_bound(kf.pix, s0, i, want);
            if (k < i && (kf.pix[k] & 0x7fffffffu) == want) up = k;
        }
        if (r < 0x7fff) {
            const uint32_t want = w + 0x10000u;
            const int k = pix_lower_bound(kf.pix, i + 1, s1, want);
            if (k < s1 && (kf.pix[k] & 0x7fffffffu) == want) down = k;
        }
        const double Lu = table_difference(kf.baseL, i, left, right), Lv = table_difference(kf.baseL, i, up, down);
        const double fx = (double)kf.K[0], fy = (double)kf.K[4], cx = (double)kf.K[2], cy = (double)kf.K[5];
        const double m0 = -(fx * Lu), m1 = -(fy * Lv), m2 = (1.0 + ((double)c - cx) * Lu) + ((double)r - cy) * Lv;
        double nw[3] = {0.0, 0.0, 0.0};                    // a non-finite m: no normal
        if (fabs(m0) < HUGE_VAL && fabs(m1) < HUGE_VAL && fabs(m2) < HUGE_VAL) {
            const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            const double n0 = -m0 / len, n1 = -m1 / len, n2 = -m2 / len;               // faces the keyframe's camera: m . ray = 1
#pragma unroll
            for (int q = 0; q < 3; ++q) nw[q] = (Rm[3 * q] * n0 + Rm[3 * q + 1] * n1) + Rm[3 * q + 2] * n2;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) stage[3 * tid + q] = (float)nw[q];
    }
    __syncthreads();
    for (int j = tid; j < 3 * (int)n_rows; j += SP_BLOCK) normals[3 * row0 + j] = stage[j];
}

// grid ceil(Q / 256), block SP_BLOCK: k_view_keys<true> (sp_views.hip) with the depth of every covered pixel taken on the point's
// tangent plane; the workgroups take the points from the END of the set, as there
__global__ __launch_bounds__(SP_BLOCK) void k_surfel_keys(const float* __restrict__ points, const float* __restrict__ radii,
                                                          const float* __restrict__ normals, int Q, const SpView* __restrict__ views, int V,
                                                          int H, int W, float z_min, int max_px, int cull,
                                                          unsigned long long* __restrict__ keys) {
    __shared__ float sp[3 * SP_BLOCK];
    __shared__ float sn[3 * SP_BLOCK];
    __shared__ float sr[SP_BLOCK];
    __shared__ ViewD vd[VIEW_CHUNK];
    const int tid = threadIdx.x;
    const long long first = (long long)(gridDim.x - 1 - blockIdx.x) * SP_BLOCK;
    const int n = (int)((long long)Q - first < SP_BLOCK ? (long long)Q - first : SP_BLOCK);
    for (int j = tid; j < 3 * n; j += SP_BLOCK) { sp[j] = points[3 * first + j]; sn[j] = normals[3 * first + j]; }
    if (tid < n) sr[tid] = radii[first + tid];
    const size_t HW = (size_t)H * W;
    const double Wd = (double)W, Hd = (double)H, zmin = (double)z_min;
    const uint32_t id = (uint32_t)(first + tid);           // (Q <= 2^31 - 2)
    for (int v0 = 0; v0 < V; v0 += VIEW_CHUNK) {
        const int nv = V - v0 < VIEW_CHUNK ? V - v0 : VIEW_CHUNK;
        __syncthreads();                                   // (sp, sn, sr are written; the previous chunk has been read)
        if (tid < nv) view_setup(views[v0 + tid], vd[tid]);
        __syncthreads();
        if (tid >= n) continue;
        const double px = (double)sp[3 * tid], py = (double)sp[3 * tid + 1], pz = (double)sp[3 * tid + 2];
        const float nf0 = sn[3 * tid], nf1 = sn[3 * tid + 1], nf2 = sn[3 * tid + 2];
        const bool usable = fabsf(nf0) < HUGE_VALF && fabsf(nf1) < HUGE_VALF && fabsf(nf2) < HUGE_VALF && (nf0 != 0.f || nf1 != 0.f || nf2 != 0.f);
        const double n0 = (double)nf0, n1 = (double)nf1, n2 = (double)nf2;
        const double rad = (double)sr[tid], cap = (double)max_px;
        const double h = 2.0 * (rad >= 0.0 ? rad : 0.0);   // a disc reaching the square's corners stays within z -+ 2 rad however it is tilted
        for (int k = 0; k < nv; ++k) {
            const ViewD& w = vd[k];
            double x, y, z, u, v;
            camera_point(w, px, py, pz, x, y, z);
            pixel_of(w, x, y, z, u, v);
            unsigned long long* view_keys = keys + (size_t)(v0 + k) * HW;
            if (!(z > zmin) || !(fabs(u) < HUGE_VAL) || !(fabs(v) < HUGE_VAL)) continue;
            const double ru = half_width((rad * w.fx) / z, cap), rv = half_width((rad * w.fy) / z, cap);
            const double ul = u - ru, uh = u + ru, vl = v - rv, vh = v + rv;
            if (!(uh >= 0.0 && ul < Wd && vh >= 0.0 && vl < Hd)) continue;
            // clamped in float64, then converted: 0 <= c0 <= c1 <= W - 1 and 0 <= r0 <= r1 <= H - 1
            const int c0 = (int)fmax(floor(ul), 0.0), c1 = (int)fmin(floor(uh), Wd - 1.0);
            const int r0 = (int)fmax(floor(vl), 0.0), r1 = (int)fmin(floor(vh), Hd - 1.0);
            if (!usable) {                                 // no normal: sp_render_splats' flat splat, the point's one key
                const unsigned long long key = key_nearest((float)z, id);
                for (int r = r0; r <= r1; ++r)
                    for (int c = c0; c <= c1; ++c) key_offer(view_keys + (size_t)r * W + c, key);
                continue;
            }
            double nc0 = n0, nc1 = n1, nc2 = n2;           // n_c = R^T n; an exact identity pose leaves it untouched
            if (!w.ident) {
                nc0 = (w.Rt[0] * n0 + w.Rt[1] * n1) + w.Rt[2] * n2;
                nc1 = (w.Rt[3] * n0 + w.Rt[4] * n1) + w.Rt[5] * n2;
                nc2 = (w.Rt[6] * n0 + w.Rt[7] * n1) + w.Rt[8] * n2;
            }
            const double s = (nc0 * x + nc1 * y) + nc2 * z;
            if (cull && s >= 0.0) continue;                // the surface seen from behind
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
        }
    }
}

}  // namespace

extern "C" {

int sp_map_normals(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int stride, const SpTrajAlign* align, int n_align, float* normals,
                   long long total_rows, void* stream) {
    if (!kfs || !normals) return SP_EINVAL;
    if (n_kf <= 0 || n_kf > 65535 || stride < 1 || total_blocks < 1 || n_align < 0 || (align == nullptr) != (n_align == 0)) return SP_EINVAL;
    if (total_rows < 1 || total_rows > (long long)total_blocks * SP_BLOCK) return SP_EINVAL;
    hipLaunchKernelGGL(k_map_normals, dim3(total_blocks), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), kfs, n_kf, stride, align,
                       n_align, normals, total_rows);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_render_surfels(const float* points, const float* colours, const float* normals, long long Q, const SpView* views, int V, int H, int W,
                      float z_min, const float* radii, int max_px, int cull, unsigned long long* keys, uint8_t* image, float* depth,
                      int32_t* index, void* stream) {
    if (!points || !views || !keys || !radii || !normals || (image && !colours)) return SP_EINVAL;
    if (Q <= 0 || V <= 0 || H <= 0 || W <= 0 || !(z_min >= 0.f) || max_px < 0 || max_px > 16 || (cull != 0 && cull != 1)) return SP_EINVAL;
    const long long HW = (long long)H * W;
    if (Q > 0x7ffffffeLL || V > 65535 || HW >= 0x80000000LL || (long long)V * HW >= 0x80000000LL) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long n_pix = (long long)V * HW;
    hipError_t e = hipMemsetAsync(keys, 0, sizeof(unsigned long long) * (size_t)n_pix, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_surfel_keys, dim3((unsigned)((Q + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s, points, radii, normals, (int)Q,
                       views, V, H, W, z_min, max_px, cull, keys);
    SP_CHECK_LAUNCH();
    if (image || depth || index) {
        hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((n_pix + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, s, keys, colours,
                           (int)n_pix, 1, image, depth, index);
        SP_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
