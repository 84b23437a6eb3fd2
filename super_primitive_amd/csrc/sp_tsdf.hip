// Map surfaces: V depth images fused into a dense signed-distance volume (sp_tsdf_integrate) and its zero level set cut into an indexed
// triangle mesh by marching tetrahedra on the Kuhn split of every cell (sp_tsdf_mesh); the contracts are in include/sp_hip.h.
//
// sp_tsdf_integrate.  One launch, one thread per node, x fastest: the lanes of a wave read and write 256 contiguous bytes of tsdf,
// weight and (768 of) colour.  A node's state lives in registers while the thread walks the views in order; every 16 views the workgroup
// forms their float64 records once into LDS (view_setup), so the per-view operands are wave-uniform LDS broadcasts.  The projection is
// camera_point / pixel_of of sp_map_device.h, the one pair every map kernel projects with; the test on z comes before the two divisions.
// The update is float32 with every operation rounded on its own.  No atomics, nothing shared between threads: two runs give the same bits,
// and a call over views 0 .. V-1 leaves the bits of two calls over 0 .. k-1 and k .. V-1.  No workgroup skips a view by a frustum test:
// every node tests every view.  (A per-node test that finds a miss of more than a pixel by four products in place of the two divisions
// gave the same bits and 5 % at 256^3 nodes and 16 views, inside the spread of the runs: the waves that straddle an image's border still
// divide.  It is not kept.)
//
// sp_tsdf_mesh.  Ordered compaction twice, from the pieces of sp_map_device.h (block_prefix, block_count_scan); no workgroup waits on
// another, nothing spins, no atomics, no sort:
//   k_mesh_nodes     one thread per node: the 7-bit mask of its crossing lattice edges (towards node + offset, offsets 1 .. 7) and the
//                    number of crossing edges before it in its 256-node block -> one int32 per node (mask | prefix << 8; the prefix is
//                    at most 255 x 7); per block the number of crossing edges
//   k_mesh_cells<0>  one thread per cell: its number of faces (six tetrahedra, 0, 1 or 2 each); per 256-cell block their number
//   k_mesh_scan      two workgroups: the exclusive prefix sums of the two block arrays, in place; n_out[0] and n_out[1] are the totals
//   k_mesh_vertices  a node writes the vertices of its crossing edges at block offset + prefix + rank in the mask: ascending edge id
//   k_mesh_cells<1>  a cell recomputes its faces and writes them at block offset + prefix: ascending (cell, tetrahedron, triangle); the
//                    vertex of an edge is found from its lower node's word and block offset
// The last two are launched only when a capacity is > 0, and write nothing when a total is beyond 2^31 - 1 (the block offsets and the
// face indices are int32; n_out still holds the true totals).
// The cycle of every (tetrahedron, sign case) is a table of 6 x 16 words built at compile time from the rule itself (mesh_case below).
#include "sp_map_device.h"

#pragma clang fp contract(off)

namespace {

// ---- integrate ------------------------------------------------------------------------------------------------------------------------
// new = (old * weight + sample) / (weight + 1), float32, every operation rounded on its own
__device__ __forceinline__ float running_mean(float old, float weight, float sample, float wn) {
    return __fdiv_rn(__fadd_rn(__fmul_rn(old, weight), sample), wn);
}

// grid ceil(nx ny nz / 256), block SP_BLOCK
__global__ __launch_bounds__(SP_BLOCK) void k_tsdf_integrate(const float* __restrict__ depth, const float* __restrict__ images,
                                                             const SpView* __restrict__ views, int V, int H, int W, int nx, int ny, int n_nodes,
                                                             float voxel, float ox, float oy, float oz, float trunc, float z_min,
                                                             float depth_max, float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ colour) {
    __shared__ ViewD vd[VIEW_CHUNK];
    const int tid = threadIdx.x;
    const long long at = (long long)blockIdx.x * SP_BLOCK + tid;
    const bool in = at < n_nodes;
    const int i = in ? (int)at : 0;                        // (lanes beyond the volume stay for the barriers; they store nothing)
    const int ix = i % nx, iyz = i / nx, iy = iyz % ny, iz = iyz / ny;
    const double vx = (double)voxel;
    const double px = node_centre(ix, vx, (double)ox), py = node_centre(iy, vx, (double)oy), pz = node_centre(iz, vx, (double)oz);
    const size_t HW = (size_t)H * W;
    const double Wd = (double)W, Hd = (double)H, zmin = (double)z_min, tr = (double)trunc;
    float f = 0.f, w = 0.f, c[3] = {0.f, 0.f, 0.f};
    if (in) {
        f = tsdf[i];
        w = weight[i];
        if (colour) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = colour[3 * (size_t)i + ch];
        }
    }
    for (int v0 = 0; v0 < V; v0 += VIEW_CHUNK) {
        const int nv = V - v0 < VIEW_CHUNK ? V - v0 : VIEW_CHUNK;
        __syncthreads();                                   // (the previous chunk has been read)
        if (tid < nv) view_setup(views[v0 + tid], vd[tid]);
        __syncthreads();
        if (!in) continue;
        for (int k = 0; k < nv; ++k) {
            const ViewD& cam = vd[k];
            double x, y, z, u, v;
            camera_point(cam, px, py, pz, x, y, z);
            if (!(z > zmin)) continue;
            pixel_of(cam, x, y, z, u, v);
            const double cu = floor(u + 0.5), cv = floor(v + 0.5);
            if (!(cu >= 0.0 && cu < Wd && cv >= 0.0 && cv < Hd)) continue;           // NaN and +-inf fail
            const size_t pix = (size_t)(int)cv * W + (size_t)(int)cu;               // 0 <= row < H, 0 <= col < W
            const float D = depth[(size_t)(v0 + k) * HW + pix];
            if (!(D > 0.f && D <= depth_max && D < HUGE_VALF)) continue;             // NaN, 0, negative, inf, beyond depth_max
            const double sdf = (double)D - z;
            if (sdf < -tr) continue;
            const double q = sdf / tr;
            const float s = (float)(q < 1.0 ? q : 1.0);
            const float wn = __fadd_rn(w, 1.f);
            f = running_mean(f, w, s, wn);
            if (colour) {
                const float* img = images + 3 * (size_t)(v0 + k) * HW + pix;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float e = img[(size_t)ch * HW];
                    c[ch] = running_mean(c[ch], w, e == e ? e : 0.f, wn);
                }
            }
            w = wn;
        }
    }
    if (!in) return;
    tsdf[i] = f;
    weight[i] = w;
    if (colour) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) colour[3 * (size_t)i + ch] = c[ch];
    }
}

// ---- mesh: the table -------------------------------------------------------------------------------------------------------------------
// the six tetrahedra of a cell by corner (corner c has offset bits x = 1, y = 2, z = 4); all share the diagonal 0 - 7, and along each the
// corners' bits grow: 0 < c1 < c2 < 7 as sets.  So every edge (ci, cj), i < j, is the lattice edge of type cj - ci at the node of ci, and
// the node of ci lies before the node of cj in linear order: within a tetrahedron edge ids ascend with (i, cj - ci).
constexpr int TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

struct TetEdge { int i, j; };                              // local corners, i < j

constexpr int edge_key(int tet, TetEdge e) { return 8 * e.i + (TET[tet][e.j] - TET[tet][e.i] - 1); }
// an edge as the face kernel wants it: its lower corner (3 bits) and its type - 1 (3 bits)
constexpr uint32_t edge_field(int tet, TetEdge e) { return (uint32_t)TET[tet][e.i] | ((uint32_t)(TET[tet][e.j] - TET[tet][e.i] - 1) << 3); }
constexpr int corner_axis(int c, int a) { return (c >> a) & 1; }

// The rule of include/sp_hip.h for tetrahedron `tet` with the local corners of `neg` (4 bits) negative: the crossing edges as a cycle
// from the smallest edge id, oriented so that with every vertex at its edge's midpoint (doubled: exact integers) (v1 - v0) x (v2 - v0)
// has a positive dot product with centroid(positive corners) - centroid(negative corners) (times npos nneg: exact integers too).
// The word: the number of edges (0, 3 or 4) | field of q0 << 3 | q1 << 9 | q2 << 15 | q3 << 21; `dot_out`: the dot product, never 0.
constexpr uint32_t mesh_case(int tet, int neg, long long* dot_out = nullptr) {
    int nneg = 0;
    for (int k = 0; k < 4; ++k) nneg += (neg >> k) & 1;
    if (dot_out) *dot_out = 1;
    if (nneg == 0 || nneg == 4) return 0u;
    TetEdge cyc[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    int m = 0;
    if (nneg == 2) {                                       // a quad: A, B negative, C, D positive -> AC, AD, BD, BC (neighbours share a corner)
        int n2[2] = {0, 0}, p2[2] = {0, 0}, a = 0, b = 0;
        for (int k = 0; k < 4; ++k) {
            if ((neg >> k) & 1) n2[a++] = k; else p2[b++] = k;
        }
        const int order[4][2] = {{n2[0], p2[0]}, {n2[0], p2[1]}, {n2[1], p2[1]}, {n2[1], p2[0]}};
        for (int k = 0; k < 4; ++k) cyc[k] = order[k][0] < order[k][1] ? TetEdge{order[k][0], order[k][1]} : TetEdge{order[k][1], order[k][0]};
        m = 4;
    } else {                                               // a triangle: the three edges at the lone corner
        int lone = 0;
        for (int k = 0; k < 4; ++k) if ((((neg >> k) & 1) == 1) == (nneg == 1)) lone = k;
        for (int k = 0; k < 4; ++k) if (k != lone) cyc[m++] = k < lone ? TetEdge{k, lone} : TetEdge{lone, k};
    }
    int start = 0;
    for (int k = 1; k < m; ++k) if (edge_key(tet, cyc[k]) < edge_key(tet, cyc[start])) start = k;
    TetEdge fwd[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, bwd[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int k = 0; k < m; ++k) { fwd[k] = cyc[(start + k) % m]; bwd[k] = cyc[(start + m - k) % m]; }
    // doubled midpoints of the first three vertices, the normal, the direction
    long long p[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, dir[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q)
        for (int a = 0; a < 3; ++a) p[q][a] = corner_axis(TET[tet][fwd[q].i], a) + corner_axis(TET[tet][fwd[q].j], a);
    const long long e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const long long nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) dir[a] += ((neg >> k) & 1) ? -(long long)(4 - nneg) * corner_axis(TET[tet][k], a) : (long long)nneg * corner_axis(TET[tet][k], a);
    const long long dot = nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2];
    if (dot_out) *dot_out = dot;
    const TetEdge* use = dot > 0 ? fwd : bwd;
    uint32_t word = (uint32_t)m;
    for (int k = 0; k < m; ++k) word |= edge_field(tet, use[k]) << (3 + 6 * k);
    return word;
}

struct MeshTable { uint32_t word[96]; bool decided; };
constexpr MeshTable mesh_table() {
    MeshTable t = {{0}, true};
    for (int tet = 0; tet < 6; ++tet)
        for (int neg = 0; neg < 16; ++neg) {
            long long dot = 0;
            t.word[16 * tet + neg] = mesh_case(tet, neg, &dot);
            t.decided = t.decided && dot != 0;
        }
    return t;
}
constexpr MeshTable MESH_TABLE_HOST = mesh_table();
static_assert(MESH_TABLE_HOST.decided, "the midpoint test decides every case");
__constant__ MeshTable MESH_TABLE = MESH_TABLE_HOST;

// ---- mesh: kernels ----------------------------------------------------------------------------------------------------------------------
struct MeshDims { int nx, ny, nz; };

// grid ceil(nx ny nz / 256)
__global__ __launch_bounds__(SP_BLOCK) void k_mesh_nodes(const float* __restrict__ tsdf, const float* __restrict__ weight, MeshDims d, int n_nodes,
                                                         float min_weight, int32_t* __restrict__ words, int32_t* __restrict__ block_counts) {
    __shared__ int wc[SP_WAVES];
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    int mask = 0;
    if (at < n_nodes) {
        const int i = (int)at, nxy = d.nx * d.ny;
        const int ix = i % d.nx, iyz = i / d.nx, iy = iyz % d.ny, iz = iyz / d.ny;
        const float fa = tsdf[i];
        if (node_valid(fa, weight[i], min_weight)) {
#pragma unroll
            for (int e = 1; e < 8; ++e) {
                if (ix + (e & 1) >= d.nx || iy + ((e >> 1) & 1) >= d.ny || iz + (e >> 2) >= d.nz) continue;
                const int j = i + corner_offset(e, d.nx, nxy);
                const float fb = tsdf[j];
                if (node_valid(fb, weight[j], min_weight) && (fa < 0.f) != (fb < 0.f)) mask |= 1 << (e - 1);
            }
        }
    }
    const BlockRank r = block_prefix(__popc(mask), wc);
    if (at < n_nodes) words[at] = mask | (r.rank << 8);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = r.count;
}

// the vertex of the edge of type t + 1 at `node`: its block's offset + the crossing edges before the node in its block + those before it in the node
__device__ __forceinline__ int32_t edge_vertex(const int32_t* __restrict__ words, const int32_t* __restrict__ block_offsets, int node, int t) {
    const int32_t word = words[node];
    return block_offsets[node >> 8] + (word >> 8) + __popc(word & ((1 << t) - 1));
}

// grid ceil(cells / 256).  EMIT = false: block_counts[block] = the block's faces.  EMIT = true: the faces, at block_offsets[block] + the
// faces before the cell in its block
template <bool EMIT>
__global__ __launch_bounds__(SP_BLOCK) void k_mesh_cells(const float* __restrict__ tsdf, const float* __restrict__ weight, MeshDims d, int n_cells,
                                                         float min_weight, int32_t* __restrict__ block_counts, const int32_t* __restrict__ words,
                                                         const int32_t* __restrict__ node_offsets, const long long* __restrict__ n_out,
                                                         long long max_faces, int32_t* __restrict__ faces) {
    __shared__ int wc[SP_WAVES];
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    const int nxy = d.nx * d.ny;
    int valid = 0, neg = 0, node = 0, count = 0;
    if (at < n_cells) {
        const int i = (int)at, cx = d.nx - 1, cy = d.ny - 1;
        const int ix = i % cx, iyz = i / cx, iy = iyz % cy, iz = iyz / cy;
        node = (iz * d.ny + iy) * d.nx + ix;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int j = node + corner_offset(c, d.nx, nxy);
            const float f = tsdf[j];
            if (node_valid(f, weight[j], min_weight)) valid |= 1 << c;
            if (f < 0.f) neg |= 1 << c;
        }
    }
    uint32_t entry[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        int all = 1, sign = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            all &= valid >> TET[t][k];
            sign |= ((neg >> TET[t][k]) & 1) << k;
        }
        entry[t] = (all & 1) ? MESH_TABLE.word[16 * t + sign] : 0u;   // (a cell beyond the volume has valid = 0)
        count += (int)(entry[t] & 7u) - ((entry[t] & 7u) ? 2 : 0);    // 3 edges: one face, 4: two
    }
    const BlockRank r = block_prefix(count, wc);
    if constexpr (!EMIT) {
        if (threadIdx.x == 0) block_counts[blockIdx.x] = r.count;
    } else {
        if (count == 0 || n_out[0] > 0x7fffffffLL || n_out[1] > 0x7fffffffLL) return;
        long long row = (long long)block_counts[blockIdx.x] + r.rank;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int m = (int)(entry[t] & 7u);
            if (m == 0) continue;
            int32_t q[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= m) continue;
                const int field = (int)(entry[t] >> (3 + 6 * k)) & 63;
                q[k] = edge_vertex(words, node_offsets, node + corner_offset(field & 7, d.nx, nxy), field >> 3);
            }
            if (row < max_faces) { faces[3 * row] = q[0]; faces[3 * row + 1] = q[1]; faces[3 * row + 2] = q[2]; }
            ++row;
            if (m == 4) {
                if (row < max_faces) { faces[3 * row] = q[0]; faces[3 * row + 1] = q[2]; faces[3 * row + 2] = q[3]; }
                ++row;
            }
        }
    }
}

// grid 2: workgroup 0 scans the nodes' block counts, workgroup 1 the cells'; n_out[b] = the total
__global__ __launch_bounds__(SP_BLOCK) void k_mesh_scan(int32_t* __restrict__ node_blocks, int n_node_blocks, int32_t* __restrict__ cell_blocks,
                                                        int n_cell_blocks, long long* __restrict__ n_out) {
    __shared__ long long part[SP_BLOCK];
    const bool cells = blockIdx.x == 1;
    const long long total = block_count_scan(cells ? cell_blocks : node_blocks, cells ? n_cell_blocks : n_node_blocks, part, [](long long, long long) {});
    if (threadIdx.x == 0) n_out[blockIdx.x] = total;
}

// grid ceil(nx ny nz / 256): one vertex per crossing edge, float64 from the float32 values, rounded to float32 once
__global__ __launch_bounds__(SP_BLOCK) void k_mesh_vertices(const float* __restrict__ tsdf, const float* __restrict__ colour, MeshDims d, int n_nodes,
                                                            float voxel, float ox, float oy, float oz, const int32_t* __restrict__ words,
                                                            const int32_t* __restrict__ block_offsets, const long long* __restrict__ n_out,
                                                            long long max_vertices, float* __restrict__ vertices, float* __restrict__ vertex_colours) {
    const long long at = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (at >= n_nodes || n_out[0] > 0x7fffffffLL) return;
    const int i = (int)at, nxy = d.nx * d.ny;
    const int32_t word = words[i];
    const int mask = word & 127;
    if (!mask) return;
    long long row = (long long)block_offsets[blockIdx.x] + (word >> 8);
    const int ix = i % d.nx, iyz = i / d.nx, iy = iyz % d.ny, iz = iyz / d.ny;
    const int at_axis[3] = {ix, iy, iz};
    const double vx = (double)voxel, o[3] = {(double)ox, (double)oy, (double)oz};
    const double fa = (double)tsdf[i];
    for (int e = 1; e < 8; ++e) {
        if (!((mask >> (e - 1)) & 1)) continue;
        if (row < max_vertices) {
            const int j = i + corner_offset(e, d.nx, nxy);
            const double fb = (double)tsdf[j];
            const double t = fa / (fa - fb);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double pa = node_centre(at_axis[a], vx, o[a]), pb = node_centre(at_axis[a] + ((e >> a) & 1), vx, o[a]);
                vertices[3 * row + a] = (float)(pa + t * (pb - pa));
            }
            if (vertex_colours) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double ca = (double)colour[3 * (size_t)i + ch], cb = (double)colour[3 * (size_t)j + ch];
                    vertex_colours[3 * row + ch] = (float)(ca + t * (cb - ca));
                }
            }
        }
        ++row;
    }
}

struct MeshLayout { long long nodes, cells, node_blocks, cell_blocks, word_units, node_block_units, cell_block_units; };

// nx, ny, nz >= 2 and nx ny nz <= 2^30.  The scratch: words | the nodes' block counts | the cells' block counts, each a whole number
// of 64-byte units
MeshLayout mesh_layout(int nx, int ny, int nz) {
    MeshLayout l;
    l.nodes = (long long)nx * ny * nz;
    l.cells = (long long)(nx - 1) * (ny - 1) * (nz - 1);
    l.node_blocks = (l.nodes + SP_BLOCK - 1) / SP_BLOCK;
    l.cell_blocks = (l.cells + SP_BLOCK - 1) / SP_BLOCK;
    l.word_units = (l.nodes + 15) / 16;
    l.node_block_units = (l.node_blocks + 15) / 16;
    l.cell_block_units = (l.cell_blocks + 15) / 16;
    return l;
}

}  // namespace

extern "C" {

int sp_tsdf_integrate(const float* depth, const float* images, const SpView* views, int V, int H, int W, int nx, int ny, int nz, float voxel,
                      float ox, float oy, float oz, float trunc, float z_min, float depth_max, float* tsdf, float* weight, float* colour,
                      void* stream) {
    if (!depth || !views || !tsdf || !weight || ((images == nullptr) != (colour == nullptr))) return SP_EINVAL;
    const long long nodes = volume_nodes(nx, ny, nz);
    if (V <= 0 || H <= 0 || W <= 0 || nodes == 0) return SP_EINVAL;
    if (!(voxel > 0.f && finite_f(voxel)) || !(trunc > 0.f && finite_f(trunc)) || !(z_min >= 0.f) || !(depth_max > 0.f)) return SP_EINVAL;
    if (!(finite_f(ox) && finite_f(oy) && finite_f(oz))) return SP_EINVAL;
    if (view_limits(V, H, W) || nodes < 0) return SP_ELIMIT;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((nodes + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream),
                       depth, images, views, V, H, W, nx, ny, (int)nodes, voxel, ox, oy, oz, trunc, z_min, depth_max, tsdf, weight, colour);
    SP_CHECK_LAUNCH();
    return 0;
}

long long sp_tsdf_mesh_scratch_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return SP_EINVAL;
    if (volume_nodes(nx, ny, nz) < 0) return SP_ELIMIT;
    const MeshLayout l = mesh_layout(nx, ny, nz);
    return 64 * (l.word_units + l.node_block_units + l.cell_block_units);            // <= 4 (2^30 + 2^23) + 128 bytes
}

int sp_tsdf_mesh(const float* tsdf, const float* weight, const float* colour, int nx, int ny, int nz, float voxel, float ox, float oy, float oz,
                 float min_weight, void* scratch, long long max_vertices, long long max_faces, float* vertices, float* vertex_colours,
                 int32_t* faces, long long* n_out, void* stream) {
    if (!tsdf || !weight || !scratch || !n_out || ((uintptr_t)scratch & 3)) return SP_EINVAL;
    if (nx < 2 || ny < 2 || nz < 2 || max_vertices < 0 || max_faces < 0) return SP_EINVAL;
    if ((vertices != nullptr) != (max_vertices > 0) || (faces != nullptr) != (max_faces > 0)) return SP_EINVAL;
    if ((vertex_colours != nullptr) != (max_vertices > 0 && colour != nullptr)) return SP_EINVAL;
    if (!(voxel > 0.f && finite_f(voxel)) || !(finite_f(ox) && finite_f(oy) && finite_f(oz)) || min_weight != min_weight) return SP_EINVAL;
    if (volume_nodes(nx, ny, nz) < 0 || max_vertices > 0x7fffffffLL || max_faces > 0x7fffffffLL) return SP_ELIMIT;
    const MeshLayout l = mesh_layout(nx, ny, nz);
    int32_t* words = static_cast<int32_t*>(scratch);
    int32_t* node_blocks = words + 16 * (size_t)l.word_units;
    int32_t* cell_blocks = node_blocks + 16 * (size_t)l.node_block_units;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MeshDims d = {nx, ny, nz};
    const dim3 node_grid((unsigned)l.node_blocks), cell_grid((unsigned)l.cell_blocks);
    hipLaunchKernelGGL(k_mesh_nodes, node_grid, dim3(SP_BLOCK), 0, s, tsdf, weight, d, (int)l.nodes, min_weight, words, node_blocks);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mesh_cells<false>, cell_grid, dim3(SP_BLOCK), 0, s, tsdf, weight, d, (int)l.cells, min_weight, cell_blocks, nullptr, nullptr,
                       nullptr, 0LL, nullptr);
    SP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mesh_scan, dim3(2), dim3(SP_BLOCK), 0, s, node_blocks, (int)l.node_blocks, cell_blocks, (int)l.cell_blocks, n_out);
    SP_CHECK_LAUNCH();
    if (max_vertices > 0) {
        hipLaunchKernelGGL(k_mesh_vertices, node_grid, dim3(SP_BLOCK), 0, s, tsdf, colour, d, (int)l.nodes, voxel, ox, oy, oz, words, node_blocks, n_out,
                           max_vertices, vertices, vertex_colours);
        SP_CHECK_LAUNCH();
    }
    if (max_faces > 0) {
        hipLaunchKernelGGL(k_mesh_cells<true>, cell_grid, dim3(SP_BLOCK), 0, s, tsdf, weight, d, (int)l.cells, min_weight, cell_blocks, words,
                           node_blocks, n_out, max_faces, faces);
        SP_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
