// Map registration: the similarity x -> s R x + t that moves a query cloud onto a cloud prepared by sp_cloud_grid_build, by Gauss-Newton
// ICP (sp_cloud_register; the contract is in include/sp_hip.h).  One iteration is two launches:
//   k_register_pairs   one lane per query row: the row is moved by the state's transform (float64, every operation rounded on its own:
//                      contraction is off for this file), its neighbour found by THE walk of sp_cloud_grid_nearest (grid_nearest_walk in
//                      sp_map_device.h: one definition, so the correspondences are that kernel's), the rows of its residual and
//                      Jacobian formed, and w J^T J, w J^T r, w r^2 and the pair count reduced over the workgroup in a fixed order --
//                      a butterfly of lane swaps per wave, the four waves through LDS -- into ONE record of 40 float64 per workgroup.
//                      A template per residual kind: the point-to-point kind has three rows per pair, the two plane kinds one.
//   k_register_solve   one workgroup of 512 threads: the records summed in a fixed order (25 groups of 20 lanes; group g takes the records
//                      g, g + 25, ..., its lanes one 16-byte pair of a record each, eight loads in flight; then the 25 running sums in
//                      order -- a 256-thread form with 8-byte loads took 203 us for the 4096 records of 2^20 queries, more than half
//                      a pass over the cloud: profiles/cloud_register.txt), thread 0 solves H delta = -g by LDL^T
//                      (ldlt_solve<6> / ldlt_solve<7> of sp_solve_device.h), moves the transform on the left, decides the status and writes
//                      the state and the iteration's row of the history.
// The stop is decided on the device: both kernels begin with one uniform load of state->status and return when it is not RUNNING (the
// solve kernel then still writes its history row).  No floating-point atomics, no workgroup waits on another, every loop is bounded.
#include <stddef.h>

#include "sp_map_device.h"
#include "sp_solve_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int REG_H = 28, REG_G = 7, REG_SUMS = REG_H + REG_G + 1;            // 36 float64 sums; the count is an integer beside them
constexpr int REG_SOLVE_BLOCK = 512;                                           // the solve pass: one workgroup of 8 waves (1024 threads would cap a thread at 128 registers and spill the solve)
constexpr int REG_PAIRS = SP_CLOUD_REG_WORK_DOUBLES / 2;                       // a record is 20 pairs of float64: one 16-byte load each
constexpr int REG_GROUPS = REG_SOLVE_BLOCK / REG_PAIRS;                        // 25 strided sums per entry in the solve
static_assert(REG_SUMS + 1 <= SP_CLOUD_REG_WORK_DOUBLES && REG_SUMS % 2 == 0 && REG_GROUPS * REG_PAIRS <= REG_SOLVE_BLOCK,
              "a record holds the sums and the count, the count first in its pair; the solve has a thread per (group, pair)");
static_assert(sizeof(long long) == sizeof(double), "the count lies in a float64 slot of the record");

typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool finite3(double x, double y, double z) { return fabs(x) < HUGE_VAL && fabs(y) < HUGE_VAL && fabs(z) < HUGE_VAL; }

// grid ceil(Qa / 256): one lane per query row
template <int KIND>
__global__ __launch_bounds__(SP_BLOCK) void k_register_pairs(const float* __restrict__ queries, const float* __restrict__ normals, long long Qa,
                                                             const GridHeader* __restrict__ header, const GridSlot* __restrict__ table,
                                                             const GridRecord* __restrict__ records, unsigned int mask, int Q, int with_scale,
                                                             double huber, const SpCloudReg* __restrict__ state, int32_t* __restrict__ index,
                                                             double* __restrict__ work) {
    if (state->status != SP_CLOUD_REG_RUNNING) return;     // (uniform: one scalar load)
    constexpr int NR = KIND == 0 ? 3 : 1;                  // rows of the residual per pair
    __shared__ double part[SP_WAVES][REG_SUMS];
    __shared__ int pairs[SP_WAVES];
    const long long i = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    double J[NR][7], r[NR], w = 1.0;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        r[k] = 0.0;
#pragma unroll
        for (int a = 0; a < 7; ++a) J[k][a] = 0.0;
    }
    bool use = false;
    if (i < Qa) {
        double R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = state->rot[k];  // (uniform: scalar loads)
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = state->trans[k];
        const double s = state->s;
        const double ax = (double)queries[3 * (size_t)i], ay = (double)queries[3 * (size_t)i + 1], az = (double)queries[3 * (size_t)i + 2];
        const double px = s * ((R[0] * ax + R[1] * ay) + R[2] * az) + t[0];
        const double py = s * ((R[3] * ax + R[4] * ay) + R[5] * az) + t[1];
        const double pz = s * ((R[6] * ax + R[7] * ay) + R[8] * az) + t[2];
        const GridNearest f = grid_nearest_walk(px, py, pz, header, table, records, mask, Q, -1);
        int32_t row = -1;
        if (f.row >= 0) {
            const i32x4 raw = *reinterpret_cast<const i32x4*>(records + f.place);
            const double bx = (double)__int_as_float(raw.x), by = (double)__int_as_float(raw.y), bz = (double)__int_as_float(raw.z);
            const double dx = px - bx, dy = py - by, dz = pz - bz;
            bool ok = true;                                // (a' is finite: it passed the range test of the walk)
            double rho;
            if constexpr (KIND == 0) {
                rho = sqrt((dx * dx + dy * dy) + dz * dz);
                r[0] = dx; r[1] = dy; r[2] = dz;
                J[0][1] = pz;  J[0][2] = -py; J[0][3] = 1.0; J[0][6] = px;
                J[1][0] = -pz; J[1][2] = px;  J[1][4] = 1.0; J[1][6] = py;
                J[2][0] = py;  J[2][1] = -px; J[2][5] = 1.0; J[2][6] = pz;
            } else {
                double nx, ny, nz;
                if (KIND == 1) {
                    nx = (double)normals[3 * (size_t)f.row]; ny = (double)normals[3 * (size_t)f.row + 1]; nz = (double)normals[3 * (size_t)f.row + 2];
                } else {
                    const double mx = (double)normals[3 * (size_t)i], my = (double)normals[3 * (size_t)i + 1], mz = (double)normals[3 * (size_t)i + 2];
                    ok = ok && finite3(mx, my, mz);
                    nx = (R[0] * mx + R[1] * my) + R[2] * mz;
                    ny = (R[3] * mx + R[4] * my) + R[5] * mz;
                    nz = (R[6] * mx + R[7] * my) + R[8] * mz;
                }
                ok = ok && finite3(nx, ny, nz);
                const double ux = KIND == 1 ? px : bx, uy = KIND == 1 ? py : by, uz = KIND == 1 ? pz : bz;
                r[0] = (nx * dx + ny * dy) + nz * dz;
                rho = fabs(r[0]);
                J[0][0] = uy * nz - uz * ny;
                J[0][1] = uz * nx - ux * nz;
                J[0][2] = ux * ny - uy * nx;
                J[0][3] = nx; J[0][4] = ny; J[0][5] = nz;
                J[0][6] = (nx * px + ny * py) + nz * pz;
            }
            if (huber > 0.0 && rho > 0.0) w = fmin(1.0, huber / rho);
            if (ok) { use = true; row = f.row; }
        }
        index[i] = row;
    }
    // the pair's own terms; a lane without a pair adds exact zeros, and so does the scale's column when the scale is not an unknown
    if (!use) w = 1.0;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        if (!use) r[k] = 0.0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
            if (!use || (a == 6 && !with_scale)) J[k][a] = 0.0;
    }
    double acc[REG_SUMS];
#pragma unroll
    for (int k = 0; k < REG_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        double wJ[7];
#pragma unroll
        for (int a = 0; a < 7; ++a) wJ[a] = w * J[k][a];
        int e = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
#pragma unroll
            for (int b = a; b < 7; ++b) {
                acc[e] = acc[e] + wJ[a] * J[k][b];
                ++e;
            }
        }
#pragma unroll
        for (int a = 0; a < 7; ++a) acc[REG_H + a] = acc[REG_H + a] + wJ[a] * r[k];
        acc[REG_H + REG_G] = acc[REG_H + REG_G] + (w * r[k]) * r[k];
    }
    // the workgroup's record: a butterfly over the wave (every lane ends with the same bits), then the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < REG_SUMS; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) part[wave][k] = v;
    }
    const int in_wave = (int)__popcll(__ballot(use));
    if (lane == 0) pairs[wave] = in_wave;
    __syncthreads();
    double* record = work + (size_t)blockIdx.x * SP_CLOUD_REG_WORK_DOUBLES;
    if (threadIdx.x < REG_SUMS) record[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (threadIdx.x == REG_SUMS) reinterpret_cast<long long*>(record)[REG_SUMS] = (long long)((pairs[0] + pairs[1]) + (pairs[2] + pairs[3]));
}

// one workgroup of REG_SOLVE_BLOCK threads
__global__ __launch_bounds__(REG_SOLVE_BLOCK) void k_register_solve(const double* __restrict__ work, int n_records, int with_scale, double tol,
                                                                    long long min_pairs, int iter, int max_iters, SpCloudReg* __restrict__ state,
                                                                    double* __restrict__ history) {
    const int status0 = state->status;                     // (uniform; every thread has it before thread 0 stores a new one: barriers below)
    if (status0 != SP_CLOUD_REG_RUNNING) {
        if (threadIdx.x < 4) history[4 * (size_t)iter + threadIdx.x] = threadIdx.x == 3 ? (double)status0 : 0.0;
        return;
    }
    __shared__ double part[REG_GROUPS][SP_CLOUD_REG_WORK_DOUBLES];
    __shared__ long long part_n[REG_GROUPS];
    __shared__ double sums[REG_SUMS];
    // thread (g, c) sums the float64 pair c of the records g, g + REG_GROUPS, ...: the lanes of a group read one record side by side, 16
    // bytes each; eight loads in flight per trip, added in record order
    const int g = threadIdx.x / REG_PAIRS, c = threadIdx.x - g * REG_PAIRS;
    if (g < REG_GROUPS) {
        const f64x2* pairs = reinterpret_cast<const f64x2*>(work);
        double s0 = 0.0, s1 = 0.0;
        long long sn = 0;                                  // (means something in the pair that holds the count only)
        for (int p = g; p < n_records; p += 8 * REG_GROUPS) {
            f64x2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int pp = p + u * REG_GROUPS;
                const f64x2 x = pairs[(size_t)min(pp, n_records - 1) * REG_PAIRS + c];         // unconditional load (clamped address)
                v[u].x = pp < n_records ? x.x : 0.0;
                v[u].y = pp < n_records ? x.y : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s0 = s0 + v[u].x;
                s1 = s1 + v[u].y;
                sn += __double_as_longlong(v[u].x);
            }
        }
        part[g][2 * c] = s0;
        part[g][2 * c + 1] = s1;
        if (2 * c == REG_SUMS) part_n[g] = sn;
    }
    __syncthreads();
    if (threadIdx.x < REG_SUMS) {
        double s = part[0][threadIdx.x];
        for (int k = 1; k < REG_GROUPS; ++k) s = s + part[k][threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long n = 0;
    for (int k = 0; k < REG_GROUPS; ++k) n += part_n[k];
    bool finite = true;
    for (int k = 0; k < REG_SUMS; ++k) finite = finite && fabs(sums[k]) < HUGE_VAL;
    const int nu = with_scale ? 7 : 6;
    double delta[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int status = SP_CLOUD_REG_RUNNING;
    if (n < min_pairs) status = SP_CLOUD_REG_FEW;
    else if (!finite) status = SP_CLOUD_REG_DEGENERATE;
    else {
        bool ok;
        if (with_scale) {
            double S[49], rhs[7];
            int e = 0;
            for (int a = 0; a < 7; ++a)
                for (int b = a; b < 7; ++b) { S[7 * a + b] = sums[e]; S[7 * b + a] = sums[e]; ++e; }
            for (int a = 0; a < 7; ++a) rhs[a] = -sums[REG_H + a];
            ok = ldlt_solve<7>(S, rhs);
            for (int a = 0; a < 7; ++a) delta[a] = ok ? rhs[a] : 0.0;
        } else {
            double S[36], rhs[6];
            int e = 0;
            for (int a = 0; a < 7; ++a)
                for (int b = a; b < 7; ++b) {
                    if (b < 6) { S[6 * a + b] = sums[e]; S[6 * b + a] = sums[e]; }
                    ++e;
                }
            for (int a = 0; a < 6; ++a) rhs[a] = -sums[REG_H + a];
            ok = ldlt_solve<6>(S, rhs);
            for (int a = 0; a < 6; ++a) delta[a] = ok ? rhs[a] : 0.0;
        }
        if (!ok) status = SP_CLOUD_REG_DEGENERATE;
    }
    double step = 0.0;
    if (status == SP_CLOUD_REG_RUNNING) {
        for (int a = 0; a < nu; ++a) step = step + delta[a] * delta[a];
        step = sqrt(step);
        if (!(fabs(step) < HUGE_VAL)) {                    // (a solve that overflowed: nothing moves)
            status = SP_CLOUD_REG_DEGENERATE;
            step = 0.0;
            for (int a = 0; a < 7; ++a) delta[a] = 0.0;
        }
    }
    if (status == SP_CLOUD_REG_RUNNING) {
        const double wx = delta[0], wy = delta[1], wz = delta[2];
        const double th2 = (wx * wx + wy * wy) + wz * wz;
        double A, B;
        if (th2 < SP_CLOUD_REG_SMALL_ANGLE2) {
            A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0;
        } else {
            const double th = sqrt(th2), half = th / 2.0;
            const double h = sin(half) / half;
            A = sin(th) / th; B = 0.5 * h * h;
        }
        const double wv[3] = {wx, wy, wz};
        const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
        double E[9], R[9], t[3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double I = a == b ? 1.0 : 0.0;
                E[3 * a + b] = (I + A * W[3 * a + b]) + B * (wv[a] * wv[b] - I * th2);
            }
        for (int k = 0; k < 9; ++k) R[k] = state->rot[k];
        for (int k = 0; k < 3; ++k) t[k] = state->trans[k];
        const double e = exp(delta[6]);                    // (sigma = 0 without scale: e = 1 exactly)
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) state->rot[3 * a + b] = (E[3 * a] * R[b] + E[3 * a + 1] * R[3 + b]) + E[3 * a + 2] * R[6 + b];
            state->trans[a] = e * ((E[3 * a] * t[0] + E[3 * a + 1] * t[1]) + E[3 * a + 2] * t[2]) + delta[3 + a];
        }
        state->s = state->s * e;
        if (step <= tol) status = SP_CLOUD_REG_CONVERGED;
        else if (iter + 1 >= max_iters) status = SP_CLOUD_REG_MAX_ITERS;
    }
    for (int k = 0; k < REG_H; ++k) state->H[k] = sums[k];
    for (int a = 0; a < 7; ++a) { state->g[a] = sums[REG_H + a]; state->delta[a] = delta[a]; }
    const double cost = sums[REG_H + REG_G];
    state->cost = cost;
    state->step = step;
    state->n = n;
    state->iterations = iter + 1;
    state->status = status;
    history[4 * (size_t)iter] = (double)n;
    history[4 * (size_t)iter + 1] = cost;
    history[4 * (size_t)iter + 2] = step;
    history[4 * (size_t)iter + 3] = (double)status;
}

}  // namespace

extern "C" {

int sp_cloud_register_work_doubles(long long Qa) {
    if (Qa <= 0) return SP_EINVAL;
    if (Qa > 2147483646LL) return SP_ELIMIT;
    return (int)(SP_CLOUD_REG_WORK_DOUBLES * ((Qa + SP_BLOCK - 1) / SP_BLOCK));    // <= 40 * 2^23
}

int sp_cloud_register(const float* queries, const float* normals, long long Qa, long long Q, const void* grid_scratch, int residual, int with_scale,
                      double huber, double tol, long long min_pairs, int max_iters, SpCloudReg* state, double* history, int32_t* index, double* work,
                      void* stream) {
    if (!queries || !grid_scratch || !state || !history || !index || !work) return SP_EINVAL;
    if (residual < 0 || residual > 2 || (residual != 0 && !normals) || (with_scale != 0 && with_scale != 1)) return SP_EINVAL;
    if (!(huber >= 0.0 && huber < HUGE_VAL) || !(tol >= 0.0 && tol < HUGE_VAL)) return SP_EINVAL;
    if (min_pairs < (with_scale ? 7 : 6) || max_iters < 1 || Q <= 0 || Qa <= 0) return SP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(grid_scratch) & 15u) || (reinterpret_cast<uintptr_t>(state) & 7u) || (reinterpret_cast<uintptr_t>(history) & 7u) ||
        (reinterpret_cast<uintptr_t>(work) & 15u))
        return SP_EINVAL;
    if (Q > SP_CLOUD_GRID_MAX_POINTS || Qa > 2147483646LL || max_iters > SP_CLOUD_REG_ITERS_LIMIT) return SP_ELIMIT;
    const GridLayout l = grid_layout(Q);
    const char* base = static_cast<const char*>(grid_scratch);
    const GridHeader* header = reinterpret_cast<const GridHeader*>(base);
    const GridSlot* table = reinterpret_cast<const GridSlot*>(base + 64);
    const GridRecord* records = reinterpret_cast<const GridRecord*>(base + 64 * (size_t)(1 + l.table_units));
    const unsigned int mask = (unsigned int)(l.slots - 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((Qa + SP_BLOCK - 1) / SP_BLOCK);
    // everything after the start: H, g, delta, cost, step, n, status (RUNNING), iterations
    const hipError_t e = hipMemsetAsync(reinterpret_cast<char*>(state) + offsetof(SpCloudReg, H), 0, sizeof(SpCloudReg) - offsetof(SpCloudReg, H), s);
    if (e != hipSuccess) return (int)e;
    for (int iter = 0; iter < max_iters; ++iter) {
        if (residual == 0)
            hipLaunchKernelGGL(k_register_pairs<0>, dim3(grid), dim3(SP_BLOCK), 0, s, queries, normals, Qa, header, table, records, mask, (int)Q, with_scale,
                               huber, state, index, work);
        else if (residual == 1)
            hipLaunchKernelGGL(k_register_pairs<1>, dim3(grid), dim3(SP_BLOCK), 0, s, queries, normals, Qa, header, table, records, mask, (int)Q, with_scale,
                               huber, state, index, work);
        else
            hipLaunchKernelGGL(k_register_pairs<2>, dim3(grid), dim3(SP_BLOCK), 0, s, queries, normals, Qa, header, table, records, mask, (int)Q, with_scale,
                               huber, state, index, work);
        SP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_register_solve, dim3(1), dim3(REG_SOLVE_BLOCK), 0, s, work, (int)grid, with_scale, tol, min_pairs, iter, max_iters, state, history);
        SP_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
