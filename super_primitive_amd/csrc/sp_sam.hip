// From SAM's raw output to the (masks, keypoints) of a keyframe: the tensor code behind frontend/segment/mask_generation.py
// (:13-95 smallest_good_mask_batch, :143-288 infer_masks, :291-313 masks_to_edges / infer_edge_probs) and the helpers it calls
// (calculate_stability_score, batched_mask_to_box, batched_nms with one category).  DESIGN.md §4 "SAM mask selection".
//
//   sp_sam_candidate_stats  one read of the M = 3n logit maps -> per candidate {#(x > t+o), #(x > t-o), #(x > t), box of x > t}.
//                           A candidate is a flat run of H W floats, cut into chunks of SS_CHUNK pixels, one workgroup each; 16-byte
//                           loads from the first 16-byte boundary on, the pixels before it and the last (H W - head) % 4 one by one.
//                           Lanes -> wave (shuffles) -> workgroup (LDS) -> integer atomics: any order gives the same integers.
//   sp_box_nms              one workgroup: rank by (score, index), boxes in rank order in LDS, greedy sweep.
//   sp_sam_build_masks      pixel-major: a lane owns 4 pixels and walks the K chosen candidates; their OR is the coverage.
//   sp_mask_edges           output-pixel-major: Scharr/32 magnitude of every mask, maximum over masks.  On 0/1 inputs
//                           32 gx and 32 gy are integers, so the maximum is taken over the integer 1024 (gx^2 + gy^2) and one
//                           correctly rounded square root ends it: the map is bitwise the reference's in any order.
//   sp_sam_cut_masks        keep[k] from the one pixel under keypoint k, then the kept masks ANDed with edge_probs > thr,
//                           compacted in order, with their OR.
#include "sp_device.h"

namespace {

constexpr int SS_VEC_ITERS = 8, SS_UNROLL = 4;              // 16-byte loads per lane and workgroup; of them in flight at once
constexpr int SS_CHUNK = SP_BLOCK * 4 * SS_VEC_ITERS;     // pixels of one candidate per workgroup
constexpr int SS_STATS = 8;                               // int32 per candidate: n_hi, n_lo, n_pos, left, top, right, bottom, 0
constexpr int NMS_MAX = 2048, NMS_BLOCK = 1024;
constexpr int INT_BIG = 0x7fffffff;

struct Acc {
    int n_hi, n_lo, n_pos, left, top, right, bottom;
};

__device__ __forceinline__ void acc_pixel(Acc& a, float x, float t, float t_hi, float t_lo, int r, int c) {
    a.n_hi += x > t_hi ? 1 : 0;                           // strict; NaN is false, +inf true
    a.n_lo += x > t_lo ? 1 : 0;
    if (x > t) {
        ++a.n_pos;
        a.left = min(a.left, c);
        a.right = max(a.right, c);
        a.top = min(a.top, r);
        a.bottom = max(a.bottom, r);
    }
}

__global__ void k_stats_init(int32_t* __restrict__ stats, int M) {
    const int m = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (m >= M) return;
    int32_t* s = stats + (size_t)m * SS_STATS;
    s[0] = s[1] = s[2] = 0;
    s[3] = s[4] = INT_BIG;
    s[5] = s[6] = -1;
    s[7] = 0;
}

// an empty mask's box is zeros (batched_mask_to_box)
__global__ void k_stats_finish(int32_t* __restrict__ stats, int M) {
    const int m = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (m >= M) return;
    int32_t* s = stats + (size_t)m * SS_STATS;
    if (s[2] == 0) s[3] = s[4] = s[5] = s[6] = 0;
}

// grid (chunks, M).  head = pixels of the candidate in front of its first 16-byte boundary (the same for every candidate when
// H W % 4 == 0; computed per candidate otherwise).
__global__ __launch_bounds__(SP_BLOCK) void k_candidate_stats(const float* __restrict__ logits, int HW, int W, float t, float t_hi, float t_lo,
                                                               int32_t* __restrict__ stats) {
    __shared__ int red[SP_WAVES][7];
    const int m = blockIdx.y;
    const float* cand = logits + (size_t)m * HW;
    const int head = min((int)((4u - (uint32_t)(((uintptr_t)cand >> 2) & 3u)) & 3u), HW);
    const int n_vec = (HW - head) >> 2;                   // whole 16-byte groups after the head
    Acc a = {0, 0, 0, INT_BIG, INT_BIG, -1, -1};
    {
        const int v_end = min(n_vec, (int)(blockIdx.x + 1) * (SS_CHUNK / 4));
        int v = blockIdx.x * (SS_CHUNK / 4) + threadIdx.x;
        if (v < v_end) {
            const int p0 = head + 4 * v;
            int r = p0 / W, c = p0 - r * W;
            const int step_r = (4 * SP_BLOCK) / W, step_c = (4 * SP_BLOCK) - step_r * W;
            gptr_f4 src = (gptr_f4)(cand + p0);
            for (; v < v_end; v += SS_UNROLL * SP_BLOCK, src += SS_UNROLL * SP_BLOCK) {
                float4 x[SS_UNROLL] = {};                 // the trip's loads are issued before the first is used
#pragma unroll
                for (int u = 0; u < SS_UNROLL; ++u)
                    if (v + u * SP_BLOCK < v_end) x[u] = ntload4(src + u * SP_BLOCK);
#pragma unroll
                for (int u = 0; u < SS_UNROLL; ++u) {
                    if (v + u * SP_BLOCK >= v_end) break;
                    const float xs[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
                    int rr = r, cc = c;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc_pixel(a, xs[j], t, t_hi, t_lo, rr, cc);
                        if (++cc == W) { cc = 0; ++rr; }
                    }
                    r += step_r;
                    c += step_c;
                    if (c >= W) { c -= W; ++r; }
                }
            }
        }
    }
    if (blockIdx.x == 0) {                                // the pixels no 16-byte load covers: at most 3 in front, 3 behind
        const int tail0 = head + 4 * n_vec;
        int p = -1;
        if ((int)threadIdx.x < head) p = threadIdx.x;
        else if (threadIdx.x >= 4 && tail0 + (int)threadIdx.x - 4 < HW) p = tail0 + (int)threadIdx.x - 4;
        if (p >= 0) acc_pixel(a, cand[p], t, t_hi, t_lo, p / W, p % W);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        a.n_hi += __shfl_xor(a.n_hi, o, 64);
        a.n_lo += __shfl_xor(a.n_lo, o, 64);
        a.n_pos += __shfl_xor(a.n_pos, o, 64);
        a.left = min(a.left, __shfl_xor(a.left, o, 64));
        a.top = min(a.top, __shfl_xor(a.top, o, 64));
        a.right = max(a.right, __shfl_xor(a.right, o, 64));
        a.bottom = max(a.bottom, __shfl_xor(a.bottom, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = a.n_hi; red[wave][1] = a.n_lo; red[wave][2] = a.n_pos;
        red[wave][3] = a.left; red[wave][4] = a.top; red[wave][5] = a.right; red[wave][6] = a.bottom;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        int v = red[0][k];
        for (int w = 1; w < SP_WAVES; ++w) v = k < 3 ? v + red[w][k] : (k < 5 ? min(v, red[w][k]) : max(v, red[w][k]));
        int32_t* out = stats + (size_t)m * SS_STATS + k;
        if (k < 3) { if (v) atomicAdd(out, v); }
        else if (k < 5) { if (v != INT_BIG) atomicMin(out, v); }
        else if (v >= 0) atomicMax(out, v);
    }
}

// ---- NMS ----------------------------------------------------------------------------------------------------------
// a score as an unsigned key: larger key = visited earlier.  NaN sorts first (torch.sort descending), -0 equals +0.
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0xffffffffu;
    if (s == 0.f) return 0x80000000u;
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(NMS_BLOCK) void k_box_nms(const float* __restrict__ boxes, const float* __restrict__ scores, int K, float thr,
                                                        int64_t* __restrict__ keep, int32_t* __restrict__ n_keep) {
    __shared__ uint32_t key[NMS_MAX];
    __shared__ float4 sbox[NMS_MAX];                      // in visiting order
    __shared__ float sarea[NMS_MAX];
    __shared__ int16_t order[NMS_MAX];
    __shared__ uint8_t dead[NMS_MAX];
    const int tid = threadIdx.x;
    for (int i = tid; i < K; i += NMS_BLOCK) key[i] = score_key(scores[i]);
    __syncthreads();
    for (int i = tid; i < K; i += NMS_BLOCK) {
        const uint32_t ki = key[i];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const uint32_t kj = key[j];
            rank += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
        }
        const float4 b = make_float4(boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]);
        sbox[rank] = b;                                   // (key, index) is a total order: rank is a permutation of 0 .. K-1
        sarea[rank] = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
        order[rank] = (int16_t)i;
        dead[rank] = 0;
    }
    __syncthreads();
    int n = 0;
    for (int a = 0; a < K; ++a) {
        if (dead[a]) continue;                            // uniform: written before the last barrier
        if (tid == 0) keep[n] = order[a];
        ++n;
        const float4 bi = sbox[a];
        const float ai = sarea[a];
        for (int b = a + 1 + tid; b < K; b += NMS_BLOCK) {
            if (dead[b]) continue;
            const float4 bj = sbox[b];
            const float w = fmaxf(__fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)), 0.f);
            const float h = fmaxf(__fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)), 0.f);
            const float inter = __fmul_rn(w, h);
            const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, sarea[b]), inter));
            if (iou > thr) dead[b] = 1;                   // 0/0 = NaN: false
        }
        __syncthreads();
    }
    if (tid == 0) *n_keep = n;
}

// ---- masks of the chosen candidates -------------------------------------------------------------------------------
// VEC: H W % 4 == 0 and both arrays 16- / 4-byte aligned, so every lane's 4 pixels are one 16-byte load and one 4-byte store
template <bool VEC>
__global__ __launch_bounds__(SP_BLOCK) void k_build_masks(const float* __restrict__ logits, const int32_t* __restrict__ cand, int K, int M, int HW,
                                                           float t, uint8_t* __restrict__ masks, uint8_t* __restrict__ coverage) {
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (VEC) {
        const int p = 4 * i;
        if (p >= HW) return;
        uint32_t any = 0;
        for (int k = 0; k < K; ++k) {
            const int m = cand[k];
            uint32_t bits = 0;
            if ((uint32_t)m < (uint32_t)M) {
                const float4 x = ntload4((gptr_f4)(logits + (size_t)m * HW + p));
                bits = (x.x > t ? 1u : 0u) | (x.y > t ? 0x100u : 0u) | (x.z > t ? 0x10000u : 0u) | (x.w > t ? 0x1000000u : 0u);
            }
            *reinterpret_cast<uint32_t*>(masks + (size_t)k * HW + p) = bits;
            any |= bits;
        }
        if (coverage) *reinterpret_cast<uint32_t*>(coverage + p) = any;
    } else {
        if (i >= HW) return;
        uint8_t any = 0;
        for (int k = 0; k < K; ++k) {
            const int m = cand[k];
            const uint8_t bit = ((uint32_t)m < (uint32_t)M && logits[(size_t)m * HW + i] > t) ? 1 : 0;
            masks[(size_t)k * HW + i] = bit;
            any |= bit;
        }
        if (coverage) coverage[i] = any;
    }
}

// ---- edges --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// 1024 (gx^2 + gy^2) of mask m at coarse pixel (r, c): Scharr {3, 10, 3} x {-1, 0, 1}, reflect at the coarse border
__device__ __forceinline__ int scharr_sq(const uint8_t* __restrict__ m, int r, int c, int He, int We, int H, int W, const int32_t* __restrict__ row_map,
                                         const int32_t* __restrict__ col_map) {
    int rows[3], cols[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        int rr = reflect_index(r + d - 1, He), cc = reflect_index(c + d - 1, We);
        if (row_map) rr = row_map[rr];
        if (col_map) cc = col_map[cc];
        rows[d] = min(max(rr, 0), H - 1);
        cols[d] = min(max(cc, 0), W - 1);
    }
    int v[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint8_t* row = m + (size_t)rows[a] * W;
#pragma unroll
        for (int b = 0; b < 3; ++b) v[a][b] = row[cols[b]] ? 1 : 0;
    }
    const int gx = 3 * (v[0][2] - v[0][0]) + 10 * (v[1][2] - v[1][0]) + 3 * (v[2][2] - v[2][0]);
    const int gy = 3 * (v[2][0] - v[0][0]) + 10 * (v[2][1] - v[0][1]) + 3 * (v[2][2] - v[0][2]);
    return gx * gx + gy * gy;
}

__global__ __launch_bounds__(SP_BLOCK) void k_mask_edges(const uint8_t* __restrict__ masks, int K, int H, int W, const int32_t* __restrict__ row_map,
                                                          const int32_t* __restrict__ col_map, int He, int We, float* __restrict__ edges,
                                                          float* __restrict__ edge_probs, int pool) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * SP_WAVES + (threadIdx.x >> 6);
    if (c >= We || r >= He) return;
    const size_t HW = (size_t)H * W;
    int best = 0;
    if (!pool) {
        for (int k = 0; k < K; ++k) best = max(best, scharr_sq(masks + k * HW, r, c, He, We, H, W, row_map, col_map));
    } else {                                              // max_pool2d(3, 1, 1): the in-bounds neighbours only
        const int r0 = max(r - 1, 0), r1 = min(r + 1, He - 1), c0 = max(c - 1, 0), c1 = min(c + 1, We - 1);
        for (int k = 0; k < K; ++k)
            for (int rr = r0; rr <= r1; ++rr)
                for (int cc = c0; cc <= c1; ++cc) best = max(best, scharr_sq(masks + k * HW, rr, cc, He, We, H, W, row_map, col_map));
    }
    const float e = __fsqrt_rn((float)best * (1.f / 1024.f));
    const size_t o = (size_t)r * We + c;
    edges[o] = e;
    edge_probs[o] = fminf(fmaxf(__fsub_rn(1.f, __fmul_rn(2.f, e)), 0.f), 1.f);
}

// ---- cut and compact ----------------------------------------------------------------------------------------------
// one workgroup: slot[k] = position of mask k among the kept ones, or -1
__global__ __launch_bounds__(SP_BLOCK) void k_cut_keep(const uint8_t* __restrict__ masks, int K, int H, int W, const float* __restrict__ edge_probs,
                                                        float thr, const int32_t* __restrict__ kp_rc, int32_t* __restrict__ slot) {
    __shared__ int wave_total[SP_WAVES];
    __shared__ int base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += SP_BLOCK) {
        const int k = k0 + threadIdx.x;
        int kept = 0;
        if (k < K) {
            kept = 1;
            if (kp_rc) {
                const int r = kp_rc[2 * k], c = kp_rc[2 * k + 1];
                kept = 0;
                if ((uint32_t)r < (uint32_t)H && (uint32_t)c < (uint32_t)W) {
                    const size_t p = (size_t)r * W + c;
                    kept = masks[(size_t)k * H * W + p] && (!edge_probs || edge_probs[p] > thr) ? 1 : 0;
                }
            }
        }
        int incl = kept;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        if (k < K) slot[k] = kept ? before + incl - 1 : -1;
        __syncthreads();
        if (threadIdx.x == SP_BLOCK - 1) base = before + incl;
        __syncthreads();
    }
}

template <bool VEC>
__global__ __launch_bounds__(SP_BLOCK) void k_cut_masks(const uint8_t* __restrict__ masks, int K, int HW, const float* __restrict__ edge_probs, float thr,
                                                         const int32_t* __restrict__ slot, uint8_t* __restrict__ out, uint8_t* __restrict__ coverage) {
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (VEC) {
        const int p = 4 * i;
        if (p >= HW) return;
        uint32_t valid = 0x01010101u;
        if (edge_probs) {
            const float4 e = *reinterpret_cast<const float4*>(edge_probs + p);
            valid = (e.x > thr ? 1u : 0u) | (e.y > thr ? 0x100u : 0u) | (e.z > thr ? 0x10000u : 0u) | (e.w > thr ? 0x1000000u : 0u);
        }
        uint32_t any = 0;
        for (int k = 0; k < K; ++k) {
            const int s = slot[k];
            if (s < 0) continue;
            const uint32_t bits = *reinterpret_cast<const uint32_t*>(masks + (size_t)k * HW + p) & valid;
            if (out) *reinterpret_cast<uint32_t*>(out + (size_t)s * HW + p) = bits;
            any |= bits;
        }
        *reinterpret_cast<uint32_t*>(coverage + p) = any;
    } else {
        if (i >= HW) return;
        const uint8_t valid = (!edge_probs || edge_probs[i] > thr) ? 1 : 0;
        uint8_t any = 0;
        for (int k = 0; k < K; ++k) {
            const int s = slot[k];
            if (s < 0) continue;
            const uint8_t bit = (masks[(size_t)k * HW + i] ? 1 : 0) & valid;
            if (out) out[(size_t)s * HW + i] = bit;
            any |= bit;
        }
        coverage[i] = any;
    }
}

int map_sizes(int H, int W) {
    if (H <= 0 || W <= 0) return SP_EINVAL;
    if (W > 32767 || (long long)H * W > 0x7fffffffLL) return SP_ELIMIT;
    return 0;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int sp_sam_candidate_stats(const float* logits, int M, int H, int W, float thresh, float offset, int32_t* stats, void* stream) {
    if (!logits || !stats || (const void*)logits == (const void*)stats || M <= 0 || !aligned(logits, 4) || !aligned(stats, 4)) return SP_EINVAL;
    const int rc = map_sizes(H, W);
    if (rc) return rc;
    if (M > 65535) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    const int chunks = (HW + SS_CHUNK - 1) / SS_CHUNK;    // the head shifts the groups by at most 3 pixels: never one chunk more than this
    hipLaunchKernelGGL(k_stats_init, dim3((M + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, stats, M);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_candidate_stats, dim3(chunks, M), dim3(SP_BLOCK), 0, s, logits, HW, W, thresh, thresh + offset, thresh - offset, stats);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stats_finish, dim3((M + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, stats, M);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_box_nms(const float* boxes, const float* scores, int K, float thr, int64_t* keep, int32_t* n_keep, void* stream) {
    if (!boxes || !scores || !keep || !n_keep || K <= 0 || (const void*)keep == (const void*)boxes || (const void*)keep == (const void*)scores ||
        (const void*)n_keep == (const void*)keep)
        return SP_EINVAL;
    if (K > NMS_MAX) return SP_ELIMIT;
    hipLaunchKernelGGL(k_box_nms, dim3(1), dim3(NMS_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, scores, K, thr, keep, n_keep);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_sam_build_masks(const float* logits, const int32_t* cand, int K, int M, int H, int W, float thresh, uint8_t* masks,
                       uint8_t* coverage_or_null, void* stream) {
    if (!logits || !cand || !masks || K <= 0 || M <= 0 || (const void*)masks == (const void*)logits || masks == coverage_or_null ||
        !aligned(logits, 4))
        return SP_EINVAL;
    const int rc = map_sizes(H, W);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    if (HW % 4 == 0 && aligned(logits, 16) && aligned(masks, 4) && aligned(coverage_or_null, 4))
        hipLaunchKernelGGL(k_build_masks<true>, dim3((HW / 4 + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, logits, cand, K, M, HW, thresh, masks,
                           coverage_or_null);
    else
        hipLaunchKernelGGL(k_build_masks<false>, dim3((HW + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, logits, cand, K, M, HW, thresh, masks,
                           coverage_or_null);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_mask_edges(const uint8_t* masks, int K, int H, int W, const int32_t* row_map_or_null, const int32_t* col_map_or_null, int He, int We,
                  float* edges, float* edge_probs, int pool, void* stream) {
    if (!masks || !edges || !edge_probs || edges == edge_probs || K <= 0 || He <= 0 || We <= 0) return SP_EINVAL;
    const int rc = map_sizes(H, W);
    if (rc) return rc;
    if ((!row_map_or_null && He != H) || (!col_map_or_null && We != W)) return SP_EINVAL;
    if (He < 2 || We < 2 || He > 32767 || We > 32767) return SP_ELIMIT;              // reflect padding needs two pixels
    hipLaunchKernelGGL(k_mask_edges, dim3((We + 63) / 64, (He + SP_WAVES - 1) / SP_WAVES), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), masks, K,
                       H, W, row_map_or_null, col_map_or_null, He, We, edges, edge_probs, pool);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_sam_cut_masks(const uint8_t* masks, int K, int H, int W, const float* edge_probs_or_null, float prob_thresh, const int32_t* kp_rc_or_null,
                     int32_t* keep, uint8_t* out_masks_or_null, uint8_t* final_coverage, void* stream) {
    uint8_t* out_masks = out_masks_or_null;
    if (!masks || !keep || !final_coverage || K <= 0 || out_masks == masks || final_coverage == masks || final_coverage == out_masks)
        return SP_EINVAL;
    const int rc = map_sizes(H, W);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    hipLaunchKernelGGL(k_cut_keep, dim3(1), dim3(SP_BLOCK), 0, s, masks, K, H, W, edge_probs_or_null, prob_thresh, kp_rc_or_null, keep);
    SP_CHECK_LAUNCH();
    if (HW % 4 == 0 && aligned(masks, 4) && aligned(out_masks, 4) && aligned(final_coverage, 4) && aligned(edge_probs_or_null, 16))
        hipLaunchKernelGGL(k_cut_masks<true>, dim3((HW / 4 + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, masks, K, HW, edge_probs_or_null,
                           prob_thresh, keep, out_masks, final_coverage);
    else
        hipLaunchKernelGGL(k_cut_masks<false>, dim3((HW + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, masks, K, HW, edge_probs_or_null,
                           prob_thresh, keep, out_masks, final_coverage);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
