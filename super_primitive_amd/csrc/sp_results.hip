// Sequence results: what the reference reports once a sequence ran -- the similarity alignment of the keyframe trajectory against the
// ground truth (tool/pose_utils.py:16-133 align / transfer_scale / apply_scale) and the coloured world points of the window keyframes
// (gui/odometery_gui.py:569-575,665-686 get_dense_pcd).
//
// sp_traj_align.  One workgroup per trajectory, three strided passes over its translations (means; cross-covariance and the model's
// spread; the per-pose errors), every sum in float64 in a fixed order: per thread, then over the wave by lane swaps, then over the four
// waves through LDS.  Thread 0 decomposes the 3x3 cross-covariance by one-sided Jacobi rotations (float64, registers).  The rotation is
// U diag(1, 1, det(U) det(Vh)) Vh; with the third left vector taken as u1 x u2 this is u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T, whatever
// sign a library would give u3 -- and well defined when the third singular value is exactly 0 (a planar trajectory).
//
// sp_map_points.  One thread per output row; a workgroup belongs to ONE keyframe (keyframe_of_block, sp_map_device.h).  Its pose --
// composed with the alignment in float64 where there is one -- goes through LDS as 12 floats; the (row, 3) outputs are staged in LDS and
// written as runs of consecutive floats.
//
// sp_keyframe_depths.  What each keyframe claims to see, straight from its table (the renderer's x fx / z + cx does not give back the
// integer column exactly): sp_map_points' walk at stride 1, the depth by the same device function, the pixel from decode_pix, the
// nearest point of a pixel by a 64-bit atomicMax; a second pass decodes depth and segment.  Integer maxima: two runs give the same bits.
#include <math.h>
#include "sp_map_device.h"

namespace {

// every thread ends up with the block's totals of its NV accumulators; red: SP_WAVES * NV doubles of LDS
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&acc)[NV], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = wave_sum(acc[k]);
    __syncthreads();                                       // (the previous totals have been read)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = (red[k] + red[NV + k]) + (red[2 * NV + k] + red[3 * NV + k]);
}

// one-sided Jacobi on the columns of a (3x3, a[r][c]); v accumulates the rotations: a_in v = a_out with orthogonal columns
__device__ __forceinline__ void jacobi_pair(double (&a)[3][3], double (&v)[3][3], const int p, const int q, bool& rotated) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) { alpha += a[r][p] * a[r][p]; beta += a[r][q] * a[r][q]; gamma += a[r][p] * a[r][q]; }
    if (gamma == 0.0 || fabs(gamma) <= 2.3e-16 * sqrt(alpha * beta)) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = a[r][p], aq = a[r][q], vp = v[r][p], vq = v[r][q];
        a[r][p] = c * ap - s * aq; a[r][q] = s * ap + c * aq;
        v[r][p] = c * vp - s * vq; v[r][q] = s * vp + c * vq;
    }
    rotated = true;
}

// rot = U diag(1, 1, det(U) det(Vh)) Vh of the singular value decomposition of A (row major), sigma descending
__device__ void svd3_rotation(const double* A, double* rot, double* sigma) {
    double a[3][3], v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[r][c] = A[3 * r + c]; v[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        jacobi_pair(a, v, 0, 1, rotated);
        jacobi_pair(a, v, 0, 2, rotated);
        jacobi_pair(a, v, 1, 2, rotated);
        if (!rotated) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sg[c] = sqrt(a[0][c] * a[0][c] + a[1][c] * a[1][c] + a[2][c] * a[2][c]);
    // columns by descending singular value (swaps of whole columns of a and v)
#define SP_SWAP_COLS(i, j)                                                                      \
    if (sg[i] < sg[j]) {                                                                        \
        double t_ = sg[i]; sg[i] = sg[j]; sg[j] = t_;                                           \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                         \
            t_ = a[r][i]; a[r][i] = a[r][j]; a[r][j] = t_;                                      \
            t_ = v[r][i]; v[r][i] = v[r][j]; v[r][j] = t_;                                      \
        }                                                                                       \
    }
    SP_SWAP_COLS(0, 1)
    SP_SWAP_COLS(1, 2)
    SP_SWAP_COLS(0, 1)
#undef SP_SWAP_COLS
    double u1[3], u2[3], u3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] = a[r][0] / sg[0]; u2[r] = a[r][1] / sg[1]; }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double n3 = sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
    const double det_v = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                         v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double f3 = (det_v < 0.0 ? -1.0 : 1.0) / n3;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) rot[3 * r + c] = u1[r] * v[c][0] + u2[r] * v[c][1] + f3 * u3[r] * v[c][2];
    sigma[0] = sg[0]; sigma[1] = sg[1]; sigma[2] = sg[2];
}

__device__ __forceinline__ void load_translation(const float* __restrict__ T16, double (&t)[3]) {
    t[0] = (double)T16[3]; t[1] = (double)T16[7]; t[2] = (double)T16[11];
}

// grid S, block SP_BLOCK
__global__ __launch_bounds__(SP_BLOCK) void k_traj_align(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const int32_t* __restrict__ lengths, int n_max, int anchor_rotation,
                                                         SpTrajAlign* __restrict__ out, double* __restrict__ err_scaled,
                                                         double* __restrict__ err) {
    __shared__ double red[SP_WAVES * 10];
    __shared__ double fit[16];                             // rot (9), s, trans_scaled (3), trans (3)
    const int traj = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(lengths[traj], 0), n_max);
    const float* P = pred + (size_t)traj * n_max * 16;
    const float* G = gt + (size_t)traj * n_max * 16;
    SpTrajAlign& rec = out[traj];
    double m[3], d[3];
    // ---- means
    double mean[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += SP_BLOCK) {
        load_translation(P + 16 * (size_t)i, m);
        load_translation(G + 16 * (size_t)i, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) { mean[k] += m[k]; mean[3 + k] += d[k]; }
    }
    block_sum_d<6>(mean, red);
    const double nd = (double)n;
#pragma unroll
    for (int k = 0; k < 6; ++k) mean[k] /= nd;
    // ---- cross-covariance of the zero-centred translations, W[j][k] = sum mz[j] dz[k], and the model's spread
    double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += SP_BLOCK) {
        load_translation(P + 16 * (size_t)i, m);
        load_translation(G + 16 * (size_t)i, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) { m[k] -= mean[k]; d[k] -= mean[3 + k]; }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[3 * j + k] += m[j] * d[k];
        acc[9] += m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
    }
    block_sum_d<10>(acc, red);
    if (tid == 0) {
        double A[9], rot[9], sigma[3];                     // A = W^T
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) A[3 * j + k] = acc[3 * k + j];
        svd3_rotation(A, rot, sigma);
        double dots = 0.0;                                 // sum dz . (rot mz) = sum_jk rot[j][k] A[j][k]
#pragma unroll
        for (int k = 0; k < 9; ++k) dots += rot[k] * A[k];
        const double s = dots / acc[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double rm = rot[3 * r] * mean[0] + rot[3 * r + 1] * mean[1] + rot[3 * r + 2] * mean[2];
            fit[10 + r] = mean[3 + r] - s * rm;
            fit[13 + r] = mean[3 + r] - rm;
            rec.trans_scaled[r] = fit[10 + r];
            rec.trans[r] = fit[13 + r];
            rec.sigma[r] = sigma[r];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) { fit[k] = rot[k]; rec.rot[k] = rot[k]; }
        fit[9] = s;
        rec.s = s; rec.dots = dots; rec.norms = acc[9];
        // rot_reanchor = R_gt[0] R_pred[0]^T
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double v = r == c ? 1.0 : 0.0;
                if (anchor_rotation && n > 0)
                    v = (double)G[4 * r] * (double)P[4 * c] + (double)G[4 * r + 1] * (double)P[4 * c + 1] + (double)G[4 * r + 2] * (double)P[4 * c + 2];
                rec.rot_reanchor[3 * r + c] = v;
            }
    }
    __syncthreads();
    // ---- per-pose errors and their mean squares
    double sq[2] = {0.0, 0.0};
    const double s = fit[9];
    for (int i = tid; i < n; i += SP_BLOCK) {
        load_translation(P + 16 * (size_t)i, m);
        load_translation(G + 16 * (size_t)i, d);
        double es = 0.0, e = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double rm = fit[3 * r] * m[0] + fit[3 * r + 1] * m[1] + fit[3 * r + 2] * m[2];
            const double a = s * rm + fit[10 + r] - d[r], b = rm + fit[13 + r] - d[r];
            es += a * a; e += b * b;
        }
        sq[0] += es; sq[1] += e;
        err_scaled[(size_t)traj * n_max + i] = sqrt(es);
        err[(size_t)traj * n_max + i] = sqrt(e);
    }
    for (int i = n + tid; i < n_max; i += SP_BLOCK) {
        err_scaled[(size_t)traj * n_max + i] = 0.0;
        err[(size_t)traj * n_max + i] = 0.0;
    }
    block_sum_d<2>(sq, red);
    if (tid == 0) { rec.ate_scaled = sqrt(sq[0] / nd); rec.ate = sqrt(sq[1] / nd); }
}

// grid total_blocks, block SP_BLOCK
__global__ __launch_bounds__(SP_BLOCK) void k_map_points(const SpMapKeyframe* __restrict__ kfs, int n_kf, int stride,
                                                         const SpTrajAlign* __restrict__ align, int n_align, float* __restrict__ points,
                                                         float* __restrict__ colours, int32_t* __restrict__ kf_index,
                                                         int32_t* __restrict__ seg_ids, long long total_rows) {
    __shared__ float M[13];                                // R' (9, row major), t' (3), s
    __shared__ float stage[2][3 * SP_BLOCK];
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
    if (tid < 13) {
        const bool aligned = align && kf.align >= 0 && kf.align < n_align;
        const float* T = kf.pose;
        float v;
        if (!aligned) {
            v = tid < 9 ? T[4 * (tid / 3) + tid % 3] : (tid < 12 ? T[4 * (tid - 9) + 3] : 1.f);
        } else {
            const SpTrajAlign& a = align[kf.align];
            if (tid < 9) {
                const int r = tid / 3, c = tid % 3;
                v = (float)(a.rot_reanchor[3 * r] * (double)T[c] + a.rot_reanchor[3 * r + 1] * (double)T[4 + c] + a.rot_reanchor[3 * r + 2] * (double)T[8 + c]);
            } else if (tid < 12) {
                const int r = tid - 9;
                v = (float)(a.s * (a.rot[3 * r] * (double)T[3] + a.rot[3 * r + 1] * (double)T[7] + a.rot[3 * r + 2] * (double)T[11]) + a.trans_scaled[r]);
            } else {
                v = (float)a.s;
            }
        }
        M[tid] = v;
    }
    __syncthreads();
    if (tid < n_rows) {
        const int i = (int)(local0 + tid) * stride;        // table point (< P: the row is below Q)
        const int n = map_point_segment(kf, i);
        float col, row; bool src_ok;
        decode_pix(kf.pix[i], col, row, src_ok);
        const float d = table_point_depth(kf.baseL, kf.kld, kf.kp_L, i, n);
        Cam Ks;
        load_cam(kf.K, Ks);
        float x, y;
        backproject(col, row, d, Ks, 1.f / Ks.fx, 1.f / Ks.fy, x, y);
        const float sc = M[12];
        const float px = sc * x, py = sc * y, pz = sc * d;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            stage[0][3 * tid + r] = fmaf(M[3 * r], px, fmaf(M[3 * r + 1], py, fmaf(M[3 * r + 2], pz, M[9 + r])));
        const int pr = min((int)row, kf.H - 1), pc = min((int)col, kf.W - 1);
        const size_t plane = (size_t)kf.H * kf.W, at = (size_t)pr * kf.W + pc;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) stage[1][3 * tid + ch] = kf.image[ch * plane + at];
        kf_index[row0 + tid] = lo;
        seg_ids[row0 + tid] = n;
    }
    __syncthreads();
    for (int j = tid; j < 3 * (int)n_rows; j += SP_BLOCK) {
        points[3 * row0 + j] = stage[0][j];
        colours[3 * row0 + j] = stage[1][j];
    }
}

// grid total_blocks, block SP_BLOCK: sp_map_points' walk at stride 1; the nearest point of a pixel by the "nearest" key of
// sp_map_device.h, sp_render_views mode 1's: the smallest z wins, equal z goes to the highest table index
__global__ __launch_bounds__(SP_BLOCK) void k_keyframe_depth_keys(const SpMapKeyframe* __restrict__ kfs, int n_kf, int H, int W,
                                                                  unsigned long long* __restrict__ keys) {
    const int tid = threadIdx.x, block = blockIdx.x;
    const int lo = keyframe_of_block(kfs, n_kf, block);
    const SpMapKeyframe kf = kfs[lo];
    const long long at = (long long)(block - kf.first_block) * SP_BLOCK + tid;
    if (at < 0 || at >= kf.P) return;
    const int i = (int)at;
    const int n = map_point_segment(kf, i);
    float col, row; bool src_ok;
    decode_pix(kf.pix[i], col, row, src_ok);
    const float z = table_point_depth(kf.baseL, kf.kld, kf.kp_L, i, n);
    if (!(z > 0.f && z < HUGE_VALF)) return;               // NaN, 0 (underflow), inf: no surface
    const int r = (int)row, c = (int)col;
    if (r >= H || c >= W) return;                          // (a table of another size: never written beyond the image)
    key_offer(keys + ((size_t)lo * H + r) * W + c, key_nearest(z, (uint32_t)i));
}

// grid ceil(n_kf H W / 256), block SP_BLOCK
__global__ __launch_bounds__(SP_BLOCK) void k_keyframe_depth_resolve(const unsigned long long* __restrict__ keys,
                                                                     const SpMapKeyframe* __restrict__ kfs, int HW, int n_pix,
                                                                     float* __restrict__ depth, int32_t* __restrict__ seg) {
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (at >= n_pix) return;
    const unsigned long long k = keys[at];
    depth[at] = key_nearest_z(k);
    if (seg) seg[at] = k ? map_point_segment(kfs[at / HW], key_nearest_id(k)) : -1;
}

}  // namespace

extern "C" {

int sp_traj_align(const float* pred, const float* gt, const int32_t* lengths, int S, int n_max, int anchor_rotation, SpTrajAlign* out,
                  double* err_scaled, double* err, void* stream) {
    if (!pred || !gt || !lengths || !out || !err_scaled || !err) return SP_EINVAL;
    if (S <= 0 || S > 65535 || n_max < 3) return SP_EINVAL;
    if ((long long)S * n_max * 16 > 0x7fffffffLL) return SP_ELIMIT;
    hipLaunchKernelGGL(k_traj_align, dim3(S), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), pred, gt, lengths, n_max,
                       anchor_rotation != 0, out, err_scaled, err);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_map_points(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int stride, const SpTrajAlign* align, int n_align, float* points,
                  float* colours, int32_t* kf_index, int32_t* seg_ids, long long total_rows, void* stream) {
    if (!kfs || !points || !colours || !kf_index || !seg_ids) return SP_EINVAL;
    if (n_kf <= 0 || n_kf > 65535 || stride < 1 || total_blocks < 1 || n_align < 0 || (align == nullptr) != (n_align == 0)) return SP_EINVAL;
    if (total_rows < 1 || total_rows > (long long)total_blocks * SP_BLOCK) return SP_EINVAL;
    hipLaunchKernelGGL(k_map_points, dim3(total_blocks), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), kfs, n_kf, stride, align,
                       n_align, points, colours, kf_index, seg_ids, total_rows);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_keyframe_depths(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int H, int W, unsigned long long* keys, float* depth,
                       int32_t* seg, void* stream) {
    if (!kfs || !keys || !depth || n_kf <= 0 || n_kf > 65535 || total_blocks < 1 || H <= 0 || W <= 0) return SP_EINVAL;
    if (view_limits(n_kf, H, W)) return SP_ELIMIT;         // (n_kf <= 65535 stands: the keyframes are the views)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long HW = (long long)H * W, n_pix = (long long)n_kf * HW;
    hipError_t e = keys_clear(keys, n_pix, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_keyframe_depth_keys, dim3(total_blocks), dim3(SP_BLOCK), 0, s, kfs, n_kf, H, W, keys);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_keyframe_depth_resolve, pixel_grid(n_pix), dim3(SP_BLOCK), 0, s, keys, kfs, (int)HW, (int)n_pix, depth, seg);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
