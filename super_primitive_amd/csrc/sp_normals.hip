// Normal integration: per-segment log-depth from surface normals (the stage before N2) -- what the
// reference's frontend/normals/normals_integration.py:7-28 hands to a batched conjugate-gradient solver of an
// un-vendored cupy submodule.  The arithmetic is the definition in DESIGN.md §4 "Normal integration":
//   ax = nx (c - cx) + ny (r - cy) fx / fy + nz fx,   ay = nx (c - cx) fy / fx + ny (r - cy) + nz fy,
//   edge (p, q) to the right / downward neighbour inside the mask: w = (a_p^2 + a_q^2) / 2, t = -(a_p n_p + a_q n_q) / 2,
//   (L u)_p = sum_e w_e (u_p - u_other), b_q += t, b_p -= t, plain CG on L u = b from u = 0, depth = exp(u).
//
// Layout: every vector of a segment is DENSE INSIDE THE SEGMENT'S TIGHT BOX, row stride S = box width rounded up to
// 16 floats, with a guard of S zeros in front and behind.  A pixel that is not in the mask (or a padding column) has
// zero weights on all four sides and b = 0, so it stays at u = r = p = 0 for ever: the solve needs no index arrays, no
// bounds tests and no (row, col) arithmetic -- the stencil of element i reads i +- 1 and i +- S, and the weight of a
// missing edge is 0.  One workgroup owns a segment for its whole solve; a group of four elements belongs to the same thread in every
// pass, so only p (whose neighbours a thread reads) has to cross threads, at one __syncthreads() per iteration next to
// the two of the dot products.  By its own size a segment keeps p, q and r, p and q, or p alone in LDS (DESIGN.md §4:
// measured 2 x on a keyframe's largest segment); the weights and u stay in scratch, served by L1 / L2.
#include "sp_device.h"

namespace {

constexpr int NI_THREADS = 1024;
constexpr int NI_WAVES = NI_THREADS / 64;
constexpr int NI_VECS = 6;            // wR, wD, u, r, p, q
constexpr int NI_PLAN_HEAD = 4;       // int32 words in front of the segment records: the total floats of the vector area (one int64), two spare
constexpr int NI_SEG_WORDS = 8;
constexpr int NI_LDS_FLOATS = 38912;  // 152 KiB of the CU's 160 KiB for the vectors a segment keeps in LDS
constexpr float NI_U_CLAMP = 15.f;    // exp(-15) = 3.1e-7 stays above process_frame.py:234's `> 1e-7` mask test

struct NiSeg {                        // 32 bytes, NI_SEG_WORDS int32
    int32_t r0, c0, bh, bw;           // tight box: first row / column, height, width (bh = 0: empty mask)
    long long off;                    // first float of the segment's NI_VECS vectors, relative to the vector area
    int32_t S, len;                   // row stride; floats per vector (guards included, multiple of 16)
};
static_assert(sizeof(NiSeg) == NI_SEG_WORDS * 4, "NiSeg layout");

__host__ __device__ inline int ni_stride(int bw) { return (bw + 15) & ~15; }
__host__ __device__ inline long long ni_len(int bh, int bw) {
    const long long S = ni_stride(bw);
    return bh > 0 ? ((bh * S + 2 * S + 15) & ~15LL) : 0;
}

// Sum over the workgroup, the same bits in every thread (fixed order: lanes by butterfly, then waves 0..15).  `red` is
// one of two LDS rows used alternately: the barrier of call k+1 separates the reads of call k from the writes of k+2.
__device__ __forceinline__ float ni_block_sum(float v, float* red) {
    v = wave_sum(v);                                          // x + y == y + x: every lane ends with the same bits
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NI_WAVES; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ f32x4& ni_v4(float* v, int i) { return *reinterpret_cast<f32x4*>(v + i); }   // i a multiple of 4

__device__ __forceinline__ int ni_wave_min(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// ---- plan: tight boxes, vector lengths, offsets, largest-first order ---------------------------------------------
__global__ __launch_bounds__(SP_BLOCK) void k_ni_box(const uint8_t* __restrict__ masks, const int32_t* __restrict__ boxes, int H,
                                                      int W, NiSeg* __restrict__ segs) {
    const int n = blockIdx.x;
    int R0 = 0, C0 = 0, R1 = H, C1 = W;
    if (boxes) {                                              // the hint only narrows the scan; the box used is always the tight one
        R0 = max(boxes[4 * n], 0); C0 = max(boxes[4 * n + 1], 0);
        R1 = min(boxes[4 * n + 2], H); C1 = min(boxes[4 * n + 3], W);
    }
    const int bw = max(C1 - C0, 0), total = max(R1 - R0, 0) * bw;
    const uint8_t* m = masks + (size_t)n * H * W;
    int rmin = H, cmin = W, rmax = -1, cmax = -1;
    for (int i = threadIdx.x; i < total; i += SP_BLOCK) {
        const int r = R0 + i / bw, c = C0 + i % bw;
        if (m[(size_t)r * W + c]) { rmin = min(rmin, r); cmin = min(cmin, c); rmax = max(rmax, r); cmax = max(cmax, c); }
    }
    __shared__ int red[4][SP_WAVES];
    rmin = ni_wave_min(rmin); cmin = ni_wave_min(cmin); rmax = -ni_wave_min(-rmax); cmax = -ni_wave_min(-cmax);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = rmin; red[1][w] = cmin; red[2][w] = rmax; red[3][w] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SP_WAVES; ++w) {
            rmin = min(rmin, red[0][w]); cmin = min(cmin, red[1][w]); rmax = max(rmax, red[2][w]); cmax = max(cmax, red[3][w]);
        }
        NiSeg s;
        const bool any = rmax >= 0;
        s.r0 = any ? rmin : 0; s.c0 = any ? cmin : 0;
        s.bh = any ? rmax - rmin + 1 : 0; s.bw = any ? cmax - cmin + 1 : 0;
        s.S = ni_stride(s.bw); s.len = (int32_t)ni_len(s.bh, s.bw); s.off = 0;
        segs[n] = s;
    }
}

// block n: its offset (sum of the vectors of the segments before it) and its rank by box size, largest first, ties by index
__global__ __launch_bounds__(SP_BLOCK) void k_ni_layout(NiSeg* __restrict__ segs, int N, int32_t* __restrict__ order,
                                                         long long* __restrict__ total) {
    const int n = blockIdx.x;
    const int mine = segs[n].len;
    long long before = 0;
    int rank = 0;
    for (int j = threadIdx.x; j < N; j += SP_BLOCK) {
        const int lj = segs[j].len;
        if (j < n) before += lj;
        rank += (lj > mine) || (lj == mine && j < n);
    }
    __shared__ long long sb[SP_BLOCK];
    __shared__ int sr[SP_BLOCK];
    sb[threadIdx.x] = before; sr[threadIdx.x] = rank;
    __syncthreads();
    for (int o = SP_BLOCK / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) { sb[threadIdx.x] += sb[threadIdx.x + o]; sr[threadIdx.x] += sr[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // (off is written by its own block only and read by nobody else in this launch: the loop above reads len)
        segs[n].off = sb[0] * NI_VECS;
        order[sr[0]] = n;
        if (n == N - 1) *total = (sb[0] + mine) * NI_VECS;
    }
}

// ---- the solve ---------------------------------------------------------------------------------------------------
struct NiCam { float fx, fy, cx, cy; };

// {ax, ay, nx, ny} of pixel (r, c)
__device__ __forceinline__ float4 ni_pixel(const float* __restrict__ normals, int W, int r, int c, const NiCam k) {
    const float* nrm = normals + ((size_t)r * W + c) * 3;
    const float nx = nrm[0], ny = nrm[1], nz = nrm[2];
    const float x = (float)c - k.cx, y = (float)r - k.cy;
    const float ax = nx * x + ny * y * (k.fx / k.fy) + nz * k.fx;
    const float ay = nx * x * (k.fy / k.fx) + ny * y + nz * k.fy;
    return make_float4(ax, ay, nx, ny);
}

// One segment from set-up to depth.  TIER = how many of the vectors p, q, r live in LDS for the whole solve (chosen by the
// segment's own size, so a segment's result never depends on the rest of the batch); the others, wR, wD and u stay in the
// segment's scratch.  `lds` holds TIER vectors of `len` floats, laid out like the global ones.
template <int TIER>
__device__ __forceinline__ void ni_segment(const float* __restrict__ normals, const NiCam cam, const uint8_t* __restrict__ m,
                                           const NiSeg sg, int H, int W, int max_iter, float tol, float* base, float* lds,
                                           float (*red)[NI_WAVES], float* __restrict__ out, float* __restrict__ info2) {
    const int tid = threadIdx.x;
    const int S = sg.S, len = sg.len, cells = sg.bh * S;
    for (int i = 4 * tid; i < NI_VECS * len; i += 4 * NI_THREADS) ni_v4(base, i) = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 4 * tid; i < TIER * len; i += 4 * NI_THREADS) ni_v4(lds, i) = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    // interior element i of a vector sits at [S + i]: the guards make i - S and i + S addressable for every i
    float* wR = base + S;
    float* wD = wR + len;
    float* u = wD + len;
    float* r = TIER >= 3 ? lds + 2 * len + S : u + len;
    float* p = TIER >= 1 ? lds + S : u + 2 * len;
    float* q = TIER >= 2 ? lds + len + S : u + 3 * len;

    // set-up: edge weights to the right and downward neighbour and b, gathered per pixel (no atomics: b_p collects
    // -t of its right / down edge and +t of its left / up edge in a fixed order)
    float acc = 0.f;
    for (int i = tid; i < cells; i += NI_THREADS) {
        const int rr_ = i / S, cc = i - rr_ * S;
        if (cc >= sg.bw) continue;
        const int row = sg.r0 + rr_, col = sg.c0 + cc;
        if (!m[(size_t)row * W + col]) continue;
        const float4 me = ni_pixel(normals, W, row, col, cam);
        float b = 0.f;
        if (cc + 1 < sg.bw && m[(size_t)row * W + col + 1]) {
            const float4 o = ni_pixel(normals, W, row, col + 1, cam);
            wR[i] = 0.5f * (me.x * me.x + o.x * o.x);
            b += 0.5f * (me.x * me.z + o.x * o.z);
        }
        if (rr_ + 1 < sg.bh && m[(size_t)(row + 1) * W + col]) {
            const float4 o = ni_pixel(normals, W, row + 1, col, cam);
            wD[i] = 0.5f * (me.y * me.y + o.y * o.y);
            b += 0.5f * (me.y * me.w + o.y * o.w);
        }
        if (cc > 0 && m[(size_t)row * W + col - 1]) {
            const float4 o = ni_pixel(normals, W, row, col - 1, cam);
            b -= 0.5f * (me.x * me.z + o.x * o.z);
        }
        if (rr_ > 0 && m[(size_t)(row - 1) * W + col]) {
            const float4 o = ni_pixel(normals, W, row - 1, col, cam);
            b -= 0.5f * (me.y * me.w + o.y * o.w);
        }
        r[i] = b;
        p[i] = b;
        acc += b * b;
    }
    int par = 0;
    const float bb = ni_block_sum(acc, red[par]);            // (its barrier also publishes wR, wD and p)
    par ^= 1;
    float rr = bb;
    const float stop = tol * sqrtf(bb);
    int k = 0;
    if (bb > 0.f) {
        while (k < max_iter && sqrtf(rr) > stop) {
            // four consecutive cells per thread and trip (S is a multiple of 16: every vector access is a 16-byte one; only the two
            // neighbours across the ends of the group are single loads)
            acc = 0.f;
            for (int i = 4 * tid; i < cells; i += 4 * NI_THREADS) {
                const f32x4 pc = ni_v4(p, i), pu = ni_v4(p, i - S), pd = ni_v4(p, i + S);
                const f32x4 wr = ni_v4(wR, i), wd = ni_v4(wD, i), wu = ni_v4(wD, i - S);
                const float pl = p[i - 1], pr = p[i + 4], wl = wR[i - 1];
                const f32x4 pL = {pl, pc.x, pc.y, pc.z}, pR = {pc.y, pc.z, pc.w, pr}, wL = {wl, wr.x, wr.y, wr.z};
                const f32x4 v = wr * (pc - pR) + wd * (pc - pd) + wL * (pc - pL) + wu * (pc - pu);
                ni_v4(q, i) = v;
                acc += pc.x * v.x;
                acc += pc.y * v.y;
                acc += pc.z * v.z;
                acc += pc.w * v.w;
            }
            const float pq = ni_block_sum(acc, red[par]);
            par ^= 1;
            if (!(pq > 0.f)) break;
            const float alpha = rr / pq;
            acc = 0.f;
            for (int i = 4 * tid; i < cells; i += 4 * NI_THREADS) {
                ni_v4(u, i) += alpha * ni_v4(p, i);
                const f32x4 v = ni_v4(r, i) - alpha * ni_v4(q, i);
                ni_v4(r, i) = v;
                acc += v.x * v.x;
                acc += v.y * v.y;
                acc += v.z * v.z;
                acc += v.w * v.w;
            }
            const float rr_new = ni_block_sum(acc, red[par]);
            par ^= 1;
            const float beta = rr_new / rr;
            rr = rr_new;
            ++k;
            for (int i = 4 * tid; i < cells; i += 4 * NI_THREADS) ni_v4(p, i) = ni_v4(r, i) + beta * ni_v4(p, i);
            __syncthreads();                                  // p of the neighbours, for the next stencil
        }
    }
    if (tid == 0) { info2[0] = (float)k; info2[1] = bb > 0.f ? sqrtf(rr) / sqrtf(bb) : 0.f; }

    // depth = exp(u) on the mask, 0 elsewhere (normals_integration.py:25-26 `expanded`).  Every write of u is followed by
    // the barrier of the dot product after it, so reading it here in image order (another thread's element) is safe
    const int r1 = sg.r0 + sg.bh, c1 = sg.c0 + sg.bw, HW = H * W;
    for (int i = tid; i < HW; i += NI_THREADS) {
        const int row = i / W, col = i - row * W;
        float d = 0.f;
        if (row >= sg.r0 && row < r1 && col >= sg.c0 && col < c1 && m[i]) {
            const float v = u[(row - sg.r0) * S + (col - sg.c0)];
            d = fast_exp(fminf(fmaxf(v, -NI_U_CLAMP), NI_U_CLAMP));
        }
        out[i] = d;
    }
}

__global__ __launch_bounds__(NI_THREADS) void k_ni_solve(const float* __restrict__ normals, const float* __restrict__ Kmat,
                                                          const uint8_t* __restrict__ masks, const NiSeg* __restrict__ segs,
                                                          const int32_t* __restrict__ order, int H, int W, int max_iter, float tol,
                                                          float* vectors, long long capacity, float* __restrict__ depth,
                                                          float* __restrict__ info) {
    __shared__ float red[2][NI_WAVES];
    __shared__ __attribute__((aligned(16))) float lds[NI_LDS_FLOATS];
    const int n = order[blockIdx.x];
    const NiSeg sg = segs[n];
    const int tid = threadIdx.x;
    const uint8_t* m = masks + (size_t)n * H * W;
    float* out = depth + (size_t)n * H * W;

    if (sg.bh <= 0 || sg.off + (long long)NI_VECS * sg.len > capacity) {     // empty mask, or a scratch smaller than the plan asks for
        for (int i = tid; i < H * W; i += NI_THREADS) out[i] = 0.f;
        if (tid == 0) { info[2 * n] = sg.bh <= 0 ? 0.f : -1.f; info[2 * n + 1] = 0.f; }
        return;
    }
    const NiCam cam = {Kmat[0], Kmat[4], Kmat[2], Kmat[5]};
    float* base = vectors + sg.off;
    // (uniform over the workgroup: one segment, one tier)
    if (3 * sg.len <= NI_LDS_FLOATS) ni_segment<3>(normals, cam, m, sg, H, W, max_iter, tol, base, lds, red, out, info + 2 * n);
    else if (2 * sg.len <= NI_LDS_FLOATS) ni_segment<2>(normals, cam, m, sg, H, W, max_iter, tol, base, lds, red, out, info + 2 * n);
    else if (sg.len <= NI_LDS_FLOATS) ni_segment<1>(normals, cam, m, sg, H, W, max_iter, tol, base, lds, red, out, info + 2 * n);
    else ni_segment<0>(normals, cam, m, sg, H, W, max_iter, tol, base, lds, red, out, info + 2 * n);
}

int ni_check_sizes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return SP_EINVAL;
    if (N > 65535 || H > 32767 || W > 32767 || (long long)NI_VECS * ni_len(H, W) > 0x7fffffffLL) return SP_ELIMIT;
    return 0;
}

int ni_plan_words(int N) { return (NI_PLAN_HEAD + (NI_SEG_WORDS + 1) * N + 15) & ~15; }

int ni_plan(const uint8_t* masks, const int32_t* boxes, int N, int H, int W, int32_t* plan, hipStream_t s) {
    NiSeg* segs = reinterpret_cast<NiSeg*>(plan + NI_PLAN_HEAD);
    hipLaunchKernelGGL(k_ni_box, dim3(N), dim3(SP_BLOCK), 0, s, masks, boxes, H, W, segs);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ni_layout, dim3(N), dim3(SP_BLOCK), 0, s, segs, N, plan + NI_PLAN_HEAD + NI_SEG_WORDS * N,
                       reinterpret_cast<long long*>(plan));
    SP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int sp_normal_integration_plan_words(int N) {
    if (N <= 0) return SP_EINVAL;
    if (N > 65535) return SP_ELIMIT;
    return ni_plan_words(N);
}

int sp_normal_integration_segment_floats(int H, int W) {
    const int rc = ni_check_sizes(1, H, W);
    return rc ? rc : (int)(NI_VECS * ni_len(H, W));
}

int sp_normal_integration_plan(const uint8_t* masks, const int32_t* boxes_or_null, int N, int H, int W, int32_t* plan, void* stream) {
    if (!masks || !plan) return SP_EINVAL;
    const int rc = ni_check_sizes(N, H, W);
    if (rc) return rc;
    return ni_plan(masks, boxes_or_null, N, H, W, plan, static_cast<hipStream_t>(stream));
}

int sp_normal_integration(const float* normals, const float* K, const uint8_t* masks, const int32_t* boxes_or_null, int N, int H,
                          int W, int cg_max_iter, float cg_tol, int flags, float* scratch, long long scratch_floats, float* depth,
                          float* info, void* stream) {
    if (!normals || !K || !masks || !scratch || !depth || !info || cg_max_iter < 0 || !(cg_tol >= 0.f) || flags != 0) return SP_EINVAL;
    int rc = ni_check_sizes(N, H, W);
    if (rc) return rc;
    const int words = ni_plan_words(N);
    if (scratch_floats < words) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* plan = reinterpret_cast<int32_t*>(scratch);
    rc = ni_plan(masks, boxes_or_null, N, H, W, plan, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ni_solve, dim3(N), dim3(NI_THREADS), 0, s, normals, K, masks,
                       reinterpret_cast<const NiSeg*>(plan + NI_PLAN_HEAD), plan + NI_PLAN_HEAD + NI_SEG_WORDS * N, H, W, cg_max_iter,
                       cg_tol, scratch + words, scratch_floats - words, depth, info);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
