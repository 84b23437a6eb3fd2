// Map neighbourhoods: for every query its k nearest points of a prepared cloud within the radius (sp_cloud_grid_knn), and a surface
// normal from such a list by the principal axes of its points (sp_cloud_normals); the contracts are in include/sp_hip.h.
//
//   k_grid_knn<CAP, BLOCK>  one lane per query.  THE walk of sp_cloud_grid_nearest (grid_walk in sp_map_device.h: the range test, the
//                   27 cells, their records, d2 in float64, d2 <= r2, row != self) with another visitor: the lane keeps the k smallest
//                   (d2, row) it has met, sorted, in LDS -- a structure of arrays with the lane as the fastest index (d2[j][lane],
//                   row[j][lane]: a wave's access to entry j touches consecutive banks, and nothing is indexed at run time in private
//                   memory: scratch bytes are 0) --, and the current worst of a full list and the fill level in registers.  A neighbour
//                   that does not make the list costs one float64 compare and no LDS traffic; one that does is inserted by shifting,
//                   so the list stays sorted and the output pass is a plain copy (padded with -1 and +inf).  The k smallest of a set
//                   under a total order do not depend on the order its members are met in.
//                   Three capacities, 8, 16 and 32 entries, chosen by k; an entry is 12 bytes, so a lane owns 96, 192 or 384 bytes of
//                   LDS and a CU's 160 KiB hold 26, 13 or 6 waves' lists.  The workgroup size per capacity is SP_KNN_BLOCK_* below
//                   (DESIGN.md section 4 "Map neighbourhoods" has what was timed).
//   k_cloud_normals one lane per query: the listed points relative to the query summed in float64 in list order (S1, the six S2), the
//                   covariance, its eigenvalues and the eigenvector of the smallest by cyclic Jacobi with a fixed number of sweeps
//                   (no trigonometric function: a rotation is t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
//                   s = t c; it branches on nothing but "this off-diagonal entry is zero"), the sign by the largest component and then
//                   by the viewpoint.  Everything in named registers: no array is indexed at run time.
// Measured and not kept: an insertion that finds the place from four entries loaded together and moves the run four entries
// a step is 6 % faster at k = 32 with 64 neighbours per query and 1 - 6 % slower everywhere else.
// No atomics, no workgroup waits on another, nothing spins, every loop is bounded (the walk as in sp_nearest.hip; an insertion shifts
// at most k - 1 entries; a list has k entries; the sweeps are counted).
#include "sp_map_device.h"

#pragma clang fp contract(off)

// lanes per workgroup of the list kernel at capacity 8 / 16 / 32 (a multiple of 64; CAP * BLOCK * 12 bytes of LDS per workgroup).
// One wave per workgroup at every capacity: timed against 128 and 256 lanes in alternating rounds (profiles/cloud_knn.txt), 64 lanes
// are 0 - 5 % faster at capacity 8, 3 - 6 % at 16 and 2 - 6 % (128) or 36 - 53 % (256) at 32 -- the CU's LDS is handed out in
// finer pieces and a workgroup ends when its slowest wave does.  Macros, so that another build can be timed beside this one.
#ifndef SP_KNN_BLOCK_8
#define SP_KNN_BLOCK_8 64
#endif
#ifndef SP_KNN_BLOCK_16
#define SP_KNN_BLOCK_16 64
#endif
#ifndef SP_KNN_BLOCK_32
#define SP_KNN_BLOCK_32 64
#endif

namespace {

// grid ceil(Qa / BLOCK): one lane per query; k in 1 .. CAP
template <int CAP, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_grid_knn(const float* __restrict__ queries, long long Qa, const GridHeader* __restrict__ header,
                                                    const GridSlot* __restrict__ table, const GridRecord* __restrict__ records,
                                                    unsigned int mask, int Q, int skip_self, int k, int32_t* __restrict__ index,
                                                    float* __restrict__ dist, int32_t* __restrict__ count) {
    static_assert(BLOCK % 64 == 0 && CAP * BLOCK * 12 <= 160 * 1024, "whole waves, and the lists fit a CU's LDS");
    __shared__ double list_d2[CAP][BLOCK];
    __shared__ int32_t list_row[CAP][BLOCK];
    const int t = threadIdx.x;
    const long long i = (long long)blockIdx.x * BLOCK + t;
    if (i >= Qa) return;                                   // (no barrier below: a lane reads and writes its own column only)
    const float ax = queries[3 * (size_t)i], ay = queries[3 * (size_t)i + 1], az = queries[3 * (size_t)i + 2];
    int fill = 0, n = 0;
    double worst_d2 = HUGE_VAL;                            // until the list is full every neighbour makes it: d2 <= r2 < inf
    int32_t worst_row = 0x7fffffff;
    grid_walk((double)ax, (double)ay, (double)az, header, table, records, mask, Q, skip_self ? (int32_t)i : -1,
              [&](double d2, int32_t row, int32_t) {
                  ++n;
                  if (!(d2 < worst_d2 || (d2 == worst_d2 && row < worst_row))) return;
                  int j = fill < k ? fill : k - 1;         // the free entry, or the worst's, which drops out
                  for (; j > 0; --j) {                     // at most k - 1 shifts
                      const double pd = list_d2[j - 1][t];
                      const int32_t pr = list_row[j - 1][t];
                      if (!(d2 < pd || (d2 == pd && row < pr))) break;
                      list_d2[j][t] = pd;
                      list_row[j][t] = pr;
                  }
                  list_d2[j][t] = d2;
                  list_row[j][t] = row;
                  if (fill < k) ++fill;
                  if (fill == k) { worst_d2 = list_d2[k - 1][t]; worst_row = list_row[k - 1][t]; }
              });
    count[i] = n;
    const size_t base = (size_t)i * (size_t)k;
    for (int j = 0; j < k; ++j) {
        const bool have = j < fill;
        index[base + j] = have ? list_row[j][t] : -1;
        dist[base + j] = have ? (float)sqrt(list_d2[j][t]) : GRID_INF;
    }
}

// one Jacobi rotation in the plane (p, q) of a symmetric 3 x 3 matrix, r the third axis: app, aqq, apq, arp, arq are its entries, vp and
// vq the columns p and q of the accumulated eigenvectors
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& vp0, double& vp1,
                                              double& vp2, double& vq0, double& vq1, double& vq2) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);        // (+-inf for a tiny apq: t = 0 then)
    const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double tn = theta < 0.0 ? -tt : tt;
    const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
    app = app - tn * apq;
    aqq = aqq + tn * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double p0 = c * vp0 - s * vq0, q0 = s * vp0 + c * vq0;
    const double p1 = c * vp1 - s * vq1, q1 = s * vp1 + c * vq1;
    const double p2 = c * vp2 - s * vq2, q2 = s * vp2 + c * vq2;
    vp0 = p0; vq0 = q0; vp1 = p1; vq1 = q1; vp2 = p2; vq2 = q2;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < GRID_INF && fabsf(y) < GRID_INF && fabsf(z) < GRID_INF; }

// grid ceil(Qa / 256): one lane per query
__global__ __launch_bounds__(SP_BLOCK) void k_cloud_normals(const float* __restrict__ points, int Q, const float* __restrict__ queries,
                                                            const int32_t* __restrict__ index, long long Qa, int k,
                                                            const float* __restrict__ toward, int V, const int32_t* __restrict__ owner,
                                                            float* __restrict__ normals, float* __restrict__ curvature,
                                                            int32_t* __restrict__ used) {
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= Qa) return;
    const double qx = (double)queries[3 * (size_t)i], qy = (double)queries[3 * (size_t)i + 1], qz = (double)queries[3 * (size_t)i + 2];
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    int n = 0;
    const size_t base = (size_t)i * (size_t)k;
    for (int j = 0; j < k; ++j) {
        const int32_t r = index[base + j];
        if (r < 0 || r >= Q) continue;                     // -1 padding, and a caller's list stays inside the cloud
        const float px = points[3 * (size_t)r], py = points[3 * (size_t)r + 1], pz = points[3 * (size_t)r + 2];
        if (!finite3(px, py, pz)) continue;
        const double dx = (double)px - qx, dy = (double)py - qy, dz = (double)pz - qz;
        s1x += dx; s1y += dy; s1z += dz;
        sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
        ++n;
    }
    used[i] = n;
    const float nan = __builtin_nanf("");
    float ox = nan, oy = nan, oz = nan, oc = nan;
    if (n >= 3) {
        const double N = (double)n;
        const double mx = s1x / N, my = s1y / N, mz = s1z / N;
        double a00 = sxx / N - mx * mx, a01 = sxy / N - mx * my, a02 = sxz / N - mx * mz;
        double a11 = syy / N - my * my, a12 = syz / N - my * mz, a22 = szz / N - mz * mz;
        double v00 = 1.0, v10 = 0.0, v20 = 0.0, v01 = 0.0, v11 = 1.0, v21 = 0.0, v02 = 0.0, v12 = 0.0, v22 = 1.0;   // v<row><column>
#pragma unroll 1
        for (int sweep = 0; sweep < SP_CLOUD_NORMALS_SWEEPS; ++sweep) {
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);          // (0, 1), third axis 2
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);          // (0, 2), third axis 1
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);          // (1, 2), third axis 0
        }
        // the smallest eigenvalue and its column (on a tie the lowest column), the middle and the largest.  Selects of values: written
        // as two ifs that each assign a column, the compiler stores V to private memory and loads the column by index (80 bytes a lane)
        const bool one = a11 < a00;
        const double l01 = one ? a11 : a00;
        const bool two = a22 < l01;
        const double l0 = two ? a22 : l01;
        double ex = two ? v02 : (one ? v01 : v00), ey = two ? v12 : (one ? v11 : v10), ez = two ? v22 : (one ? v21 : v20);
        const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
        const double l2 = hi01 < a22 ? a22 : hi01;
        const double mid = hi01 < a22 ? hi01 : a22;
        const double l1 = lo01 < mid ? mid : lo01;
        if (l1 > 9.31322574615478515625e-10 * l2) {        // 2^-30; false for coincident or collinear points, l2 = 0 and NaN
            const double len = sqrt((ex * ex + ey * ey) + ez * ez);
            ex = ex / len; ey = ey / len; ez = ez / len;
            // the component of largest magnitude positive (on a tie the lowest axis) ...
            const double mx_ = fabs(ex), my_ = fabs(ey), mz_ = fabs(ez);
            double lead = ex;
            double big = mx_;
            if (my_ > big) { big = my_; lead = ey; }
            if (mz_ > big) { big = mz_; lead = ez; }
            bool flip = lead < 0.0;
            // ... unless a viewpoint says otherwise: towards it
            if (toward) {
                const int o = owner ? owner[i] : 0;
                if (o >= 0 && o < V) {
                    const double cx = (double)toward[3 * (size_t)o] - qx, cy = (double)toward[3 * (size_t)o + 1] - qy, cz = (double)toward[3 * (size_t)o + 2] - qz;
                    const double dot = (ex * cx + ey * cy) + ez * cz;
                    if (dot < 0.0) flip = true;
                    if (dot > 0.0) flip = false;           // (a zero or NaN product keeps the rule above)
                }
            }
            if (flip) { ex = -ex; ey = -ey; ez = -ez; }
            ox = (float)ex; oy = (float)ey; oz = (float)ez;
            const double pos = l0 > 0.0 ? l0 : 0.0;
            oc = (float)(pos / ((l0 + l1) + l2));
        }
    }
    normals[3 * (size_t)i] = ox; normals[3 * (size_t)i + 1] = oy; normals[3 * (size_t)i + 2] = oz;
    curvature[i] = oc;
}

template <int CAP, int BLOCK>
void launch_knn(const float* queries, long long Qa, long long Q, const void* scratch, int skip_self, int k, int32_t* index, float* dist,
                int32_t* count, hipStream_t s) {
    const GridLayout l = grid_layout(Q);
    const char* base = static_cast<const char*>(scratch);
    hipLaunchKernelGGL((k_grid_knn<CAP, BLOCK>), dim3((unsigned)((Qa + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, queries, Qa,
                       reinterpret_cast<const GridHeader*>(base), reinterpret_cast<const GridSlot*>(base + 64),
                       reinterpret_cast<const GridRecord*>(base + 64 * (size_t)(1 + l.table_units)), (unsigned int)(l.slots - 1), (int)Q, skip_self, k,
                       index, dist, count);
}

}  // namespace

extern "C" {

int sp_cloud_grid_knn(const float* queries, long long Qa, long long Q, const void* scratch, int skip_self, int k, int32_t* index, float* dist,
                      int32_t* count, void* stream) {
    if (!queries || !scratch || !index || !dist || !count || (reinterpret_cast<uintptr_t>(scratch) & 15u)) return SP_EINVAL;
    if (Qa <= 0 || Q <= 0 || k < 1 || (skip_self != 0 && skip_self != 1) || (skip_self == 1 && Qa != Q)) return SP_EINVAL;
    if (k > SP_CLOUD_KNN_MAX || Q > SP_CLOUD_GRID_MAX_POINTS || Qa > 2147483646LL || Qa * k > 2147483646LL) return SP_ELIMIT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (k <= 8) launch_knn<8, SP_KNN_BLOCK_8>(queries, Qa, Q, scratch, skip_self, k, index, dist, count, s);
    else if (k <= 16) launch_knn<16, SP_KNN_BLOCK_16>(queries, Qa, Q, scratch, skip_self, k, index, dist, count, s);
    else launch_knn<32, SP_KNN_BLOCK_32>(queries, Qa, Q, scratch, skip_self, k, index, dist, count, s);
    SP_CHECK_LAUNCH();
    return 0;
}

int sp_cloud_normals(const float* points, long long Q, const float* queries, const int32_t* index, long long Qa, int k, const float* toward,
                     int V, const int32_t* owner, float* normals, float* curvature, int32_t* used, void* stream) {
    if (!points || !queries || !index || !normals || !curvature || !used) return SP_EINVAL;
    if (Q <= 0 || Qa <= 0 || k < 1 || (toward && (V < 1 || (!owner && V != 1)))) return SP_EINVAL;
    if (k > SP_CLOUD_KNN_MAX || Q > SP_CLOUD_GRID_MAX_POINTS || Qa > 2147483646LL || Qa * k > 2147483646LL) return SP_ELIMIT;
    hipLaunchKernelGGL(k_cloud_normals, dim3((unsigned)((Qa + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream),
                       points, (int)Q, queries, index, Qa, k, toward, toward ? V : 0, toward ? owner : nullptr, normals, curvature, used);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
