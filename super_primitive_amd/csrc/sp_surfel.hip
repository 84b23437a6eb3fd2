// Map normals (the contract of sp_map_normals in include/sp_hip.h; the surfels that carry them are rendered by sp_views.hip, as one kind
// of its key pass).  All arithmetic is float64 from the float32 inputs, every operation rounded on its own (contraction is switched off
// for this file: the reference is NumPy in float64), rounded to float32 once.
//
// sp_map_normals.  sp_map_points' walk (keyframe_of_block: sp_map_device.h; segment_of: sp_device.h), one thread per output row, a workgroup
// belongs to ONE keyframe.  The rotation -- composed with the alignment's rot_reanchor where there is one -- goes through LDS as 9 float64;
// the (row, 3) outputs are staged in LDS and written as runs of consecutive floats.  A row's neighbours are looked up at stride 1 in the
// row's own segment: left and right are the adjacent table points, up and down two binary searches of the segment's range (pix is
// strictly increasing there), the only divergent part, bounded by log2 of the segment's size.  No atomics, no workgroup waits on another.
#include <math.h>
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

}  // extern "C"
