// Depth completion, the last stage (BASELINE config 4): fill every uncovered pixel from its nearest covered one and score
// depth maps -- depth_completion/fill_in_tools.py:5-7 fill_depth, depth_completion/void.py:7-65 ErrorMetrics /
// ErrorMetricsDeltas, as evaluate_void.py:122-146 uses them.
//
// Fill.  scipy's distance_transform_edt(invalid, return_indices=True) gives every invalid pixel (r, c) the valid pixel
// (r', c') that minimises ((r - r')^2 + (c - c')^2, c', r') lexicographically (DESIGN.md §4 "Depth fill").  Two passes,
// integers only:
//   1. columns: off[r][c] = r' - r of the nearest valid row of column c (ties: the smaller row), OFF_NONE when the column
//      has none; a column is walked as 16 runs of rows side by side.  Within one column the distance and the tie are both
//      decided by the row alone, so one candidate per column is all pass 2 ever needs.
//   2. rows: a workgroup stages its row of offsets in LDS; every invalid pixel walks the columns c, c-1, c+1, c-2, c+2, ...
//      and stops once dc^2 exceeds its best d^2.  Columns to the left are met in falling order, so a left candidate wins
//      on d^2 <= best; columns to the right in rising order, so a right candidate wins on d^2 < best only.
// Pass 1 is bound by the latency of its column walks (16 B W threads of H / 16 rows, three times), pass 2 by LDS reads:
// about 2 sqrt(d^2) per invalid pixel.
//
// Metrics.  Every per-pixel term is formed in fp32 with each operation rounded on its own (numpy's arithmetic on float32
// arrays; the Makefile's -ffp-contract=on must not fuse them), widened and summed in fp64 in a fixed order: a thread's
// pixels in index order, the wave by butterfly, the waves 0..3, then the workgroups' partials the same way.  No atomics.
#include "sp_device.h"

namespace {

constexpr int16_t OFF_NONE = -32768;
constexpr int MT_VALUES = 12;
constexpr int MT_PIXELS = 8 * SP_BLOCK;       // pixels of one image per workgroup of the first stage

// ---- fill ---------------------------------------------------------------------------------------------------------
// grid (ceil(W / FC_COLS), B), block (FC_COLS, FC_SEGS): thread = one of FC_SEGS runs of rows of one column of one image.  A run first
// finds its own first and last valid row; the nearest valid row above (below) the run is then the last (first) one of the nearest run
// above (below) that has any, and the two walks of the run start from those.
constexpr int FC_COLS = 64, FC_SEGS = 16;

__global__ __launch_bounds__(FC_COLS * FC_SEGS) void k_fill_columns(const uint8_t* __restrict__ invalid, int H, int W, int16_t* __restrict__ off,
                                                                     int32_t* __restrict__ counts) {
    __shared__ int first_valid[FC_SEGS][FC_COLS], last_valid[FC_SEGS][FC_COLS], n_valid_of[FC_SEGS];
    const int lane = threadIdx.x, seg = threadIdx.y;
    const int c = blockIdx.x * FC_COLS + lane, b = blockIdx.y;
    const int rows = (H + FC_SEGS - 1) / FC_SEGS, r0 = min(seg * rows, H), r1 = min(r0 + rows, H);
    const size_t base = (size_t)b * H * W + c;
    int first = -1, last = -1, n_valid = 0;
    if (c < W) {
        for (int r = r0; r < r1; ++r) {
            if (!invalid[base + (size_t)r * W]) {
                if (first < 0) first = r;
                last = r;
                ++n_valid;
            }
        }
    }
    first_valid[seg][lane] = first;
    last_valid[seg][lane] = last;
    n_valid = wave_sum(n_valid);                                  // a wave is one run of the block's 64 columns
    if (lane == 0) n_valid_of[seg] = n_valid;
    __syncthreads();
    if (c < W) {
        last = -1;                                                // nearest valid row at or above r
        for (int s = seg - 1; s >= 0 && last < 0; --s) last = last_valid[s][lane];
        int next = -1;                                            // nearest valid row at or below r
        for (int s = seg + 1; s < FC_SEGS && next < 0; ++s) next = first_valid[s][lane];
        for (int r = r0; r < r1; ++r) {
            const size_t i = base + (size_t)r * W;
            if (!invalid[i]) last = r;
            off[i] = last < 0 ? OFF_NONE : (int16_t)(last - r);
        }
        for (int r = r1 - 1; r >= r0; --r) {
            const size_t i = base + (size_t)r * W;
            if (!invalid[i]) next = r;
            const int up = off[i];
            if (next >= 0 && (up == OFF_NONE || next - r < -up)) off[i] = (int16_t)(next - r);      // a tie keeps the smaller row
        }
    }
    if (seg == 0 && lane == 0) {
        int n = 0;
        for (int s = 0; s < FC_SEGS; ++s) n += n_valid_of[s];
        if (n) atomicAdd(counts + 2 * b, n);
    }
}

// grid (H, B): workgroup = one row of one image; row[] = W int16 of dynamic LDS
__global__ __launch_bounds__(SP_BLOCK) void k_fill_rows(const float* __restrict__ depth, const uint8_t* __restrict__ invalid,
                                                         const int16_t* __restrict__ off, int H, int W, float* __restrict__ filled,
                                                         int32_t* __restrict__ index, int32_t* __restrict__ counts) {
    extern __shared__ int16_t row[];
    const int r = blockIdx.x, b = blockIdx.y;
    const size_t image = (size_t)b * H * W, base = image + (size_t)r * W;
    const int n_valid = counts[2 * b];                            // complete: written by the launch before this one
    if (r == 0 && threadIdx.x == 0) counts[2 * b + 1] = n_valid ? H * W - n_valid : 0;
    if (n_valid) {
        for (int c = threadIdx.x; c < W; c += SP_BLOCK) row[c] = off[base + c];
        __syncthreads();
    }
    for (int c = threadIdx.x; c < W; c += SP_BLOCK) {
        int src_r = r, src_c = c;
        if (n_valid && invalid[base + c]) {
            uint32_t best = 0xffffffffu;
            int o = row[c];
            if (o != OFF_NONE) { best = (uint32_t)(o * o); src_r = r + o; }
            const int k_max = max(c, W - 1 - c);
            for (int k = 1; k <= k_max && (uint32_t)(k * k) <= best; ++k) {
                const uint32_t kk = (uint32_t)(k * k);
                if (c - k >= 0 && (o = row[c - k]) != OFF_NONE) {
                    const uint32_t d = kk + (uint32_t)(o * o);
                    if (d <= best) { best = d; src_r = r + o; src_c = c - k; }
                }
                if (c + k < W && (o = row[c + k]) != OFF_NONE) {
                    const uint32_t d = kk + (uint32_t)(o * o);
                    if (d < best) { best = d; src_r = r + o; src_c = c + k; }
                }
            }
        }
        const int src = src_r * W + src_c;
        filled[base + c] = depth[image + src];
        if (index) index[base + c] = src;
    }
}

// ---- metrics ------------------------------------------------------------------------------------------------------
// Sum of each of the MT_VALUES accumulators over the workgroup, left in tot[] of thread 0 (fixed order)
__device__ __forceinline__ void mt_block_sum(double (&acc)[MT_VALUES], double (*red)[MT_VALUES], double (&tot)[MT_VALUES]) {
#pragma unroll
    for (int k = 0; k < MT_VALUES; ++k) {
#pragma unroll
        for (int o = 32; o; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < MT_VALUES; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MT_VALUES; ++k) {
            double s = red[0][k];
            for (int w = 1; w < SP_WAVES; ++w) s += red[w][k];
            tot[k] = s;
        }
    }
}

// np.maximum: a NaN on either side stays a NaN
__device__ __forceinline__ float mt_max(float a, float b) { return (a > b || a != a) ? a : b; }

// grid (ceil(H W / MT_PIXELS), B): sums of one chunk of one image -> partials[b][chunk][MT_VALUES]
__global__ __launch_bounds__(SP_BLOCK) void k_metrics_partial(const float* __restrict__ estimate, const float* __restrict__ target,
                                                               const uint8_t* __restrict__ valid, int HW, double* __restrict__ partials) {
    __shared__ double red[SP_WAVES][MT_VALUES];
    const int b = blockIdx.y;
    const size_t image = (size_t)b * HW;
    const int first = blockIdx.x * MT_PIXELS, end = min(first + MT_PIXELS, HW);
    double acc[MT_VALUES] = {};
    for (int p = first + threadIdx.x; p < end; p += SP_BLOCK) {
        const size_t i = image + p;
        if (!valid[i]) continue;                                  // selected away: its target may be inf (evaluate_void.py:116)
        const float e = estimate[i], t = target[i];
        const float d = __fsub_rn(__fmul_rn(1000.f, e), __fmul_rn(1000.f, t)), ad = fabsf(d);          // void.py:58-60, mm
        const float it = __fdiv_rn(1.f, __fmul_rn(0.001f, t));
        const float id = __fsub_rn(__fdiv_rn(1.f, __fmul_rn(0.001f, e)), it), aid = fabsf(id);         // void.py:63-65, 1/km
        const float ratio = mt_max(__fdiv_rn(t, e), __fdiv_rn(e, t));                                   // void.py:27-28
        acc[0] += 1.0;
        acc[1] += (double)__fmul_rn(d, d);
        acc[2] += (double)ad;
        acc[3] += (double)__fdiv_rn(ad, __fmul_rn(1000.f, t));
        acc[4] += (double)__fmul_rn(id, id);
        acc[5] += (double)aid;
        acc[6] += (double)__fdiv_rn(aid, it);
        acc[7] += ratio < 1.05f ? 1.0 : 0.0;
        acc[8] += ratio < 1.10f ? 1.0 : 0.0;
        acc[9] += ratio < 1.25f ? 1.0 : 0.0;
        acc[10] += ratio < 1.5625f ? 1.0 : 0.0;
        acc[11] += ratio < 1.953125f ? 1.0 : 0.0;
    }
    double tot[MT_VALUES];
    mt_block_sum(acc, red, tot);
    if (threadIdx.x == 0) {
        double* out = partials + ((size_t)b * gridDim.x + blockIdx.x) * MT_VALUES;
#pragma unroll
        for (int k = 0; k < MT_VALUES; ++k) out[k] = tot[k];
    }
}

// grid (B): the chunks of one image -> {n, rmse, mae, absrel, inv_rmse, inv_mae, inv_absrel, five fractions}
__global__ __launch_bounds__(SP_BLOCK) void k_metrics_finish(const double* __restrict__ partials, int n_chunks, double* __restrict__ out) {
    __shared__ double red[SP_WAVES][MT_VALUES];
    const int b = blockIdx.x;
    double acc[MT_VALUES] = {};
    for (int j = threadIdx.x; j < n_chunks; j += SP_BLOCK) {
        const double* p = partials + ((size_t)b * n_chunks + j) * MT_VALUES;
#pragma unroll
        for (int k = 0; k < MT_VALUES; ++k) acc[k] += p[k];
    }
    double tot[MT_VALUES];
    mt_block_sum(acc, red, tot);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)b * MT_VALUES;
        const double n = tot[0];                                  // n = 0: 0 / 0 = NaN everywhere, the reference's empty mean
        o[0] = n;
        o[1] = sqrt(tot[1] / n);
        o[2] = tot[2] / n;
        o[3] = tot[3] / n;
        o[4] = sqrt(tot[4] / n);
        o[5] = tot[5] / n;
        o[6] = tot[6] / n;
#pragma unroll
        for (int k = 7; k < MT_VALUES; ++k) o[k] = tot[k] / n;
    }
}

int image_sizes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return SP_EINVAL;
    if (B > 65535 || H > 32767 || W > 32767 || (long long)B * H * W > 0x3fffffffLL) return SP_ELIMIT;
    return 0;
}

int metric_chunks(int H, int W) { return (int)(((long long)H * W + MT_PIXELS - 1) / MT_PIXELS); }

}  // namespace

extern "C" {

int sp_depth_fill_workspace_bytes(int B, int H, int W) {
    const int rc = image_sizes(B, H, W);
    return rc ? rc : (int)(((long long)B * H * W * 2 + 15) & ~15LL);
}

int sp_depth_fill_nearest(const float* depth, const uint8_t* invalid, int B, int H, int W, void* workspace, float* filled,
                          int32_t* index_or_null, int32_t* counts, void* stream) {
    if (!depth || !invalid || !workspace || !filled || !counts || filled == depth) return SP_EINVAL;
    const int rc = image_sizes(B, H, W);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int16_t* off = static_cast<int16_t*>(workspace);
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * B, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_fill_columns, dim3((W + FC_COLS - 1) / FC_COLS, B), dim3(FC_COLS, FC_SEGS), 0, s, invalid, H, W, off, counts);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fill_rows, dim3(H, B), dim3(SP_BLOCK), (size_t)((2 * W + 15) & ~15), s, depth, invalid, off, H, W, filled,
                       index_or_null, counts);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_depth_metrics_workspace_doubles(int B, int H, int W) {
    const int rc = image_sizes(B, H, W);
    return rc ? rc : B * metric_chunks(H, W) * MT_VALUES;
}

int sp_depth_metrics(const float* estimate, const float* target, const uint8_t* valid, int B, int H, int W, double* workspace,
                     double* out, void* stream) {
    if (!estimate || !target || !valid || !workspace || !out) return SP_EINVAL;
    const int rc = image_sizes(B, H, W);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = metric_chunks(H, W);
    hipLaunchKernelGGL(k_metrics_partial, dim3(chunks, B), dim3(SP_BLOCK), 0, s, estimate, target, valid, H * W, workspace);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_metrics_finish, dim3(B), dim3(SP_BLOCK), 0, s, workspace, chunks, out);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
