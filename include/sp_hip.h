/*
 * sp_hip.h -- C ABI of libsp_hip.so: the MI355X (gfx950) implementation of SuperPrimitive's
 * per-segment photometric pose-and-depth optimisation hot path.
 *
 * The reference (makezur/super_primitive) is 100 % Python: the interface this library sits behind is a set
 * of module-level Python functions, not an FFI.  Each entry point below names the reference function(s)
 * whose arithmetic it replaces (paths relative to the reference tree); the Python wrappers in
 * super_primitive_amd/ keep those functions' names and signatures and call these symbols through ctypes.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); nothing here synchronises the host;
 *   - every function returns 0 on success, a hipError_t (>0) from the runtime, or a negative SP_E* code;
 *   - all arithmetic is fp32 (fp64 only inside the small per-pair finalise / solve kernels);
 *   - the library allocates nothing: workspaces are caller-owned (sizes via sp_*_workspace_floats()).
 *
 * Data layout of a compacted source keyframe ("segment table", built once per keyframe):
 *   pix[P]      uint32  bit31 = source-pixel validity, bits 30..16 = row, bits 15..0 = col; points ordered
 *                       (segment, row, col) exactly like torch.where(keypoint_regions) in
 *                       core/dense_optim.py:103
 *   seg_off[N+1] int32  CSR offsets of the segments into pix / src4
 *   src4[P]     float4  {I_src.r, I_src.g, I_src.b, L}: the source image of ONE pyramid level sampled at the
 *                       point's own pixel (core/dense_optim.py:315-317) and the base log-depth
 *                       logdepth_perseg[n,row,col]
 *   kp_L[N]     float   logdepth_perseg[n, kp_row, kp_col] (core/dense_optim.py:51-64)
 *   tiles[T]    int32x4 {pair, segment, first point, point count}; a tile never straddles two segments
 *   seg_tile_off[N+1]   CSR offsets of the segments into tiles
 * Target images are packed HWC3 (r,g,b adjacent, 12 bytes per texel) per pyramid level so one bilinear tap is one
 * 12-byte load and a level costs exactly the algorithmic 12 B per pixel of HBM traffic.
 */
#ifndef SP_HIP_H
#define SP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_ABI_VERSION 20

/* Every record of this ABI states its size once, right after its definition: checked by every C++ and C11 translation unit that
 * includes this header (and, field by field, by tests/test_abi_mirror.py against the ctypes mirror).  Uses take no semicolon. */
#if defined(__cplusplus)
#define SP_ABI_ASSERT(cond, msg) static_assert(cond, msg);
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define SP_ABI_ASSERT(cond, msg) _Static_assert(cond, msg);
#else
#define SP_ABI_ASSERT(cond, msg)
#endif
#define SP_ABI_SIZE(T, n) SP_ABI_ASSERT(sizeof(T) == (n), #T " is part of the ABI: " #n " bytes")

#define SP_EINVAL (-1)   /* bad argument (null pointer, non-positive size, ...) */
#define SP_ELIMIT (-2)   /* size outside what the kernels support (H or W > 32767, N > 65535, ...) */

/* floats per partial record: mode 0 -- one tile of sp_photo_cost_grad (workspace = n_tiles * B * 16) or one span of
 * sp_pairs_cost; mode 1 -- one span of sp_pairs_cost */
#define SP_GRAD_PARTIAL_FLOATS 16
#define SP_GN_PARTIAL_FLOATS   32
#define SP_GNA_PARTIAL_FLOATS  48   /* mode 2: Gauss-Newton with the affine brightness pair among the unknowns */

int sp_abi_version(void);

/* ------------------------------------------------------------------------------------------------------
 * Segment table construction (replaces the per-iteration torch.where / dense (N,H,W) passes of
 * core/dense_optim.py:38-114 by a once-per-keyframe compaction).
 * ---------------------------------------------------------------------------------------------------- */

/* Pass 1: row_counts[N*H] = exclusive per-segment scan of the per-row mask counts (scratch kept for pass 2),
 * counts[N] = pixels per segment, seg_off[N+1] = exclusive scan of counts (seg_off[N] = P, which the host
 * reads once to size the table).  masks: N*H*W bytes (torch.bool). */
int sp_mask_count(const uint8_t* masks, int N, int H, int W, int32_t* row_counts, int32_t* counts,
                  int32_t* seg_off, void* stream);

/* Pass 2: fill pix (row/col, validity bit cleared), base log-depth baseL[P] and kp_L[N].  row_off = the
 * row_counts array produced by sp_mask_count.  keypoints: (N,2) normalised (row,col) as in
 * image/keyframe.py:20-75; the keypoint pixel is round_half_even(0.5*(dim-1)*(kp+1))
 * (tool/point_utils.py:37-40).  Order inside a segment is row-major, like torch.where. */
int sp_table_fill(const uint8_t* masks, const float* logdepth, const float* keypoints, int N, int H, int W,
                  const int32_t* seg_off, const int32_t* row_off, uint32_t* pix, float* baseL, float* kp_L,
                  void* stream);

/* Sample one source pyramid level at every table point and pack {rgb, L}.  set_validity != 0: also compute the
 * source validity bit of pix with the reference's formula (core/dense_optim.py:143-162 applied to the source
 * frame, :315-317); it depends on the geometry grid only (not on the level), so it is set by the first sampling
 * after the table is built and pix is read-only afterwards.  img: planar (3,Hl,Wl) f32.  K: 9 floats row-major.
 * The formula, per point, in this operation order: d = exp(L + (kld[n] - kp_L[n])); x = (col - cx) d / fx;
 * zinv = 1 / d where |d| > 1e-6, else the CONSTANT 1e-6 (core/ops.py:19-40: such a point re-projects onto the
 * principal point, not onto its own pixel); u = x fx zinv + cx; xn = 2 u (1 / (W - 1)) - 1 (rows alike with H);
 * valid = |xn| <= 0.99 and |yn| <= 0.99 and d > 1e-7 (false for a NaN log-depth).  The colour is the bilinear
 * sample (align-corners: ix = (xn + 1) 0.5 (Wl - 1)) at that position for EVERY point, valid or not -- the points
 * of the border band and of the zinv branch included; taps outside the level read as zero.  src4.w is L itself. */
int sp_table_sample_source(uint32_t* pix, const float* baseL, const int32_t* seg_off, const float* kp_L,
                           const float* kld, int N, int P, int H, int W, const float* img, int Hl, int Wl,
                           const float* K, float* src4, int set_validity, void* stream);

/* planar (B,3,H,W) f32 -> packed (B,H,W,3) f32 */
int sp_pack_rgb(const float* chw, int B, int H, int W, float* hwc3, void* stream);

/* One pyramid step of image/gaussian_pyramid.py:53-85: reflect-pad 1, 3x3 binomial /16, keep even rows and
 * columns.  in: planar (C,H,W); out: planar (C,ceil(H/2),ceil(W/2)).  A dimension of ONE pixel has nothing to
 * reflect onto (torch refuses that padding): the pixel itself is taken, so a 1 x 1 level blurs to itself --
 * here and in the batched pass (sp_prepare_blur_pack). */
int sp_blur_decimate(const float* in, int C, int H, int W, float* out, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Batched preparation: the table / pyramid / sampling passes above for MANY keyframes per launch (job records in DEVICE
 * memory, one grid row per record).  PairBatch builds hundreds of frame pairs with ~12 launches and ONE host
 * synchronisation (the per-segment counts, which size the tables) instead of ~15 launches and a synchronisation per pair.
 * A "table" is the compacted point set of one keyframe on a pixel lattice: stride 1 = every mask pixel (the tables above),
 * stride s > 1 = the mask pixels whose row and column are multiples of s (coarse levels of per-pair schedules).
 *   sp_prepare_count : row_counts (scratch, N*H) and counts[N] of every lattice of every keyframe, and the masks as packed bit
 *                      words (SpPrepTable.bits)                                                     [masks read once]
 *   -- host: reads counts, lays the segments out (runs padded to multiples of 256), allocates pix / baseL, uploads seg_off --
 *   sp_prepare_fill  : pix / baseL at seg_off[n] + rank inside the segment; kp_L[N] where kp_L != NULL
 *   sp_prepare_pack  : planar (3,H,W) -> HWC3 of every job image
 *   sp_prepare_blur_pack: one pyramid step (sp_blur_decimate) of every three-channel job image (the target frames) and the packing at once
 *   sp_prepare_gather: n small float vectors, one DEVICE pointer each (src[i], off[i + 1] - off[i] floats), into one flat array
 *                      (out + off[i]); src and off are device arrays.  What the host side otherwise does with one torch.cat /
 *                      torch.stack over hundreds of per-pair tensors (the intrinsics and initial log-depths of a batch: 0.7 us of
 *                      interpreter time per tensor); no counterpart in the reference, which optimises one pair per call
 *   sp_prepare_sample: sp_table_sample_source of every job at all its levels, and the source-validity bit of pix.  Every
 *                      segment's run must start at a multiple of 256 (the padded layout of the many-pairs work list; of 64 when
 *                      SpPrepSample.granule is 64);
 *                      positions beyond counts[n] of a run are padding and are written as {pix 0, src4 0} = invalid points,
 *                      so pix / src4 need no prior clearing
 * ---------------------------------------------------------------------------------------------------- */
#define SP_PREP_MAX_STRIDES 4
#define SP_PREP_MAX_LEVELS 4
typedef struct SpPrepTable {     /* one keyframe: its masks are read once per pass for all its lattices */
    const uint8_t* masks;        /* (N,H,W) bool */
    const float* logdepth;       /* (N,H,W) */
    const float* keypoints;      /* (N,2), used when kp_L != NULL */
    float* kp_L;                 /* N or NULL, out of sp_prepare_fill */
    int32_t* row_counts[SP_PREP_MAX_STRIDES];   /* N*H scratch each: written by sp_prepare_count, read by sp_prepare_fill */
    int32_t* counts[SP_PREP_MAX_STRIDES];       /* N each, out of sp_prepare_count */
    const int32_t* seg_off[SP_PREP_MAX_STRIDES];/* N each: first table position of every segment (host-made, padded layout) */
    uint32_t* pix[SP_PREP_MAX_STRIDES];         /* out of sp_prepare_fill */
    float* baseL[SP_PREP_MAX_STRIDES];          /* out of sp_prepare_fill: the log-depth of every table point -- or all NULL (ABI 13): no copy is made, the
                                                   sampling pass reads the keyframe's dense array instead (SP_PREP_DENSE_L): 8 bytes per lattice point of
                                                   writes and re-reads less, and the fill pass loses its log-depth loads */
    int32_t stride[SP_PREP_MAX_STRIDES];
    int32_t N, H, W, n_strides;
    uint32_t* bits;              /* N*H*(W/16) words or NULL: the masks as one bit word per 16 pixels, written by sp_prepare_count on
                                    its fast path (W a multiple of 16 up to 1024, masks 16-byte aligned, strides in {1,2,4,8,16}) and
                                    read by sp_prepare_fill INSTEAD of the masks (4 instead of 16 bytes per 16 pixels); NULL, or a
                                    keyframe off the fast path: the fill pass reads the masks.  logdepth must be 16-byte aligned
                                    when bits is given.  The words of rows WITHOUT a set pixel are left unwritten when stride[0] is 1
                                    (the fill pass finds such rows empty through their counts and never reads their words): scratch
                                    between the two passes, not an output */
    const int32_t* boxes;        /* NULL, or N x {row0, col0, row1, col1} (half open, pixels): a HINT from whoever made the masks -- SAM's
                                    frontend computes and NMS-filters exactly these (frontend/segment/mask_generation.py:93,155-180) --
                                    that segment n has no set pixel outside its box.  The count pass then reads the masks inside
                                    the boxes only (the 16-pixel pieces that meet them), ~1 MB of a 640x480x64 keyframe's 19.7 MB;
                                    boxes are clamped to the image, an empty or inverted box is an empty segment.  A mask pixel that
                                    breaks the contract is not seen when its ROW is outside the box or its 16-pixel piece does not
                                    meet the box columns, and seen otherwise (deterministic either way).  Fast path only (see
                                    bits); ignored on the general path, which scans everything */
} SpPrepTable;
SP_ABI_SIZE(SpPrepTable, 240)
typedef struct SpPrepSample {    /* one table, sampled at up to SP_PREP_MAX_LEVELS pyramid levels in one pass; sets pix bit 31 */
    uint32_t* pix;
    const float* baseL;          /* [P] the table's own log-depths; under SP_PREP_DENSE_L: the keyframe's dense (N,H,W) array (N H W < 2^32) */
    const int32_t* seg_off;      /* N, relative to pix */
    const int32_t* counts;       /* N: real points of every segment */
    const float* kp_L;
    const float* kld;
    const float* K;              /* 9 floats, full-resolution intrinsics */
    const float* image[SP_PREP_MAX_LEVELS];     /* planar (3,Hl,Wl) source image of each level */
    float* src4[SP_PREP_MAX_LEVELS];            /* (P,4) out, one per level */
    int32_t Hl[SP_PREP_MAX_LEVELS], Wl[SP_PREP_MAX_LEVELS];
    int32_t N, P, H, W, n_levels;
    int32_t granule;             /* low 16 bits: padding granule of the runs: 0 / 256, or 64 for wave-span tables (SP_COST_WAVE_SPANS);
                                    | SP_PREP_DEPTH_TABLE: write exp(L) instead of L into src4.w (SP_COST_DEPTH_TABLE)
                                    | SP_PREP_DENSE_L: baseL is the dense (N,H,W) array, a point's log-depth sits at (its segment, row, column) */
} SpPrepSample;
SP_ABI_SIZE(SpPrepSample, 176)
#define SP_PREP_DEPTH_TABLE 0x10000
#define SP_PREP_DENSE_L 0x20000
typedef struct SpPrepImage {
    const float* in;             /* (C,H,W) planar */
    float* out;                  /* (H,W,3) */
    int32_t H, W;
} SpPrepImage;
SP_ABI_SIZE(SpPrepImage, 24)
int sp_prepare_count(const SpPrepTable* tables, int n_tables, int max_rows, int max_N, void* stream);
/* (ABI 15) sp_prepare_count for batches whose keyframes ALL carry the segment-box hint (SpPrepTable.boxes; mask_generation.py:93,155-180 computes
 * the boxes of SAM's masks): same outputs, bit for bit; a workgroup tests 64 blocks of 64 rows against the boxes at once and only walks those
 * that meet one (the pass is otherwise bound by the latency of 184 k two-load chains per 384 keyframes).  Keyframes without boxes are handled
 * too, correctly but slowly. */
int sp_prepare_count_boxed(const SpPrepTable* tables, int n_tables, int max_rows, int max_N, void* stream);
int sp_prepare_fill(const SpPrepTable* tables, int n_tables, int max_rows, int max_N, void* stream);
int sp_prepare_sample(const SpPrepSample* jobs, int n_jobs, int max_P, void* stream);
/* (ABI 15) sp_prepare_sample for TWO tables of every keyframe in one launch: jobs_a[i] and jobs_b[i] (i < n_jobs) belong to the same keyframe and
 * take consecutive workgroups, so that a source image both tables gather from (the all-points table and the stride-2 lattice, both sampled at
 * level 0) is fetched from memory once.  Same outputs as two sp_prepare_sample calls, bit for bit. */
int sp_prepare_sample_pairs(const SpPrepSample* jobs_a, int max_P_a, const SpPrepSample* jobs_b, int max_P_b, int n_jobs, void* stream);
/* (ABI 20) retired: sp_prepare_blur, the planar-only pyramid step of a batch -- the set-up uses sp_prepare_blur_pack. */
int sp_prepare_pack(const SpPrepImage* jobs, int n_jobs, int max_pixels, void* stream);
/* One pyramid step of THREE-CHANNEL images together with their packed forms (ABI 14): what sp_blur_decimate followed by sp_pack_rgb
 * computes, bit for bit, without the packing pass's re-read of the planar levels.  out (planar level l + 1), packed_out (level l + 1 as
 * HWC3) and packed_in (level l as HWC3) may each be NULL. */
typedef struct SpPrepImagePack {
    const float* in;             /* (3,H,W) planar, level l */
    float* out;
    float* packed_in;
    float* packed_out;
    int32_t H, W;
} SpPrepImagePack;
SP_ABI_SIZE(SpPrepImagePack, 40)
int sp_prepare_blur_pack(const SpPrepImagePack* jobs, int n_jobs, int max_out_pixels, void* stream);
int sp_prepare_gather(const float* const* src, const long long* off, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * The cost: one source keyframe against B target frames (B = 1: core/dense_optim.py:265-363
 * photomeric_cost and :365-403 photomeric_cost_precomputed; B >= 1: core/dense_optim_batch.py:50-147).
 * One fused pass computes residual[b] = mean_{ch,pt} |(I_src - I_trg')*mask| AND its first-order information.
 *
 *   mode 0 (gradient): d residual[b] / d {kld (N), pose rows 0..2 (3x4), affine (a_s,b_s,a_t,b_t)}
 *                      -- what autograd produces in the reference's Adam loops;
 *   mode 1 (Gauss-Newton): IRLS-weighted normal equations of the same residuals over the left SE(3) tangent
 *                      [tau,phi] and the per-segment log-depths (arrow structure); see sp_gn_* below.
 *
 * K_src: 9 floats. K_trg: B*9. pose: B*16 row-major (target <- source). aff_src: 2 floats or NULL,
 * aff_trg: B*2 or NULL (both or neither).  zmin: 1e-7 for the single-target functions, 1e-6 for the batch
 * function (dense_optim.py:146 vs dense_optim_batch.py:15).
 * Outputs (mode 0): residual[B], g_kld[B*N], g_pose[B*16] (row 3 = 0), g_aff[B*4].
 * ---------------------------------------------------------------------------------------------------- */
int sp_photo_cost_grad(const uint32_t* pix, const float* src4, const int32_t* seg_off, const float* kp_L,
                       const int32_t* tiles, const int32_t* seg_tile_off, int n_tiles, int N, int P, int H, int W,
                       const float* K_src, const float* kld, const float* trg3, int Hl, int Wl,
                       const float* K_trg, const float* pose, int B, const float* aff_src, const float* aff_trg,
                       float zmin, float* workspace, float* residual, float* g_kld, float* g_pose, float* g_aff,
                       void* stream);

/* The same cost for an EXPLICIT list of source points -- core/dense_optim.py:365-403 photomeric_cost_precomputed fed
 * with a dict that did not come from this library's table (built by hand, filtered, or round-tripped through
 * tool/etc.py dict_cpu / a queue / a checkpoint): xyz (n,3) = src_pts and rgb (n,3) = src_pixels^T of the points whose
 * src_valid_mask is set (the caller compacts; invalid source points contribute exact zeros in the reference), 24 bytes
 * per point (tracking variant).  P_total = the ORIGINAL number of points: the residual is a mean
 * over 3 * P_total values (core/dense_optim.py:249-253).  No log-depth unknowns: outputs residual[B], g_pose[B*16],
 * g_aff[B*4].  workspace: sp_points_workspace_floats(n_points, B) floats. */
int sp_points_workspace_floats(int n_points, int B);
int sp_points_cost_grad(const float* xyz, const float* rgb, int n_points, int P_total, int H, int W, const float* trg3,
                        int Hl, int Wl, const float* K_trg, const float* pose, int B, const float* aff_src,
                        const float* aff_trg, float zmin, float* workspace, float* residual, float* g_pose, float* g_aff,
                        void* stream);

/* Per-point diagnostics of the same pass (collect_stats > 0 in the reference, core/dense_optim.py:347-361).
 * Any output pointer may be NULL.  Only every stride-th table point is reported (stride 1 = the reference's
 * tensors; > 1 = the down-sampled channel for a visualiser): with Q = ceil(P / stride) rows the
 * shapes are src_pts (Q,3); trg_pts (B,Q,3); src_rgb (3,Q); trg_rgb (B,3,Q) after brightness compensation;
 * raw (B,3,Q) = (I_src - I_trg')*mask; src_valid (Q) u8; trg_valid (B,Q) u8; seg_ids (Q) int64. */
int sp_photo_stats(const uint32_t* pix, const float* src4, const int32_t* seg_off, const float* kp_L, int N, int P,
                   int H, int W, const float* K_src, const float* kld, const float* trg3, int Hl, int Wl,
                   const float* K_trg, const float* pose, int B, const float* aff_src, const float* aff_trg,
                   float zmin, float* src_pts, float* trg_pts, float* src_rgb, float* trg_rgb, float* raw,
                   uint8_t* src_valid, uint8_t* trg_valid, int64_t* seg_ids, int stride, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Many independent frame pairs per launch (BASELINE.json configs 2 and 5; the throughput path).  Each pair
 * has its own segment table, target image, intrinsics, pose and log-depths, described by one SpPair record
 * in device memory.  No host synchronisation anywhere: one optimiser iteration is sp_pairs_cost + one
 * sp_pairs_*_step launch and can be captured in a hipGraph.
 *
 * Work list.  The tables of this path are PADDED: every segment's run of points in pix / src4 is extended to a
 * multiple of 256 with invalid points (pix word 0, src4 zeros; they contribute exact zeros).
 *   chunks[C] int32x4 {pair, segment, start, count}: a run of `count` (multiple of 256) points of one segment,
 *             `start` = index of its first point in the pair's padded arrays; chunks of a pair are consecutive
 *             and contiguous in memory (segment-major, like the table);
 *   spans[S]  int32x4 {first chunk, number of chunks, points, pair}: what one workgroup processes -- a run of
 *             consecutive chunks of one pair; pair-level sums are reduced once per span, segment-level sums once
 *             per chunk and wave.
 * Partials, two arrays:
 *   span_partials[S]      one record of (SP_GRAD_PARTIAL_FLOATS | SP_GN_PARTIAL_FLOATS) floats per span: the sums that
 *                         belong to the PAIR (mode 0: as sp_photo_cost_grad's tile record with column 13 unused;
 *                         mode 1: [0] sum|r|, [1..21] H_pp upper triangle, [22..27] b_p, [28] valid points);
 *   seg_partials[4 * C]   one record of (SP_GRAD_SEG_FLOATS | SP_GN_SEG_FLOATS) floats per (chunk, wave), record
 *                         4 * chunk + wave: the sums that belong to the SEGMENT (mode 0: d/dkld; mode 1: h_pd(6), D, b_d, and -- ABI 13 --
 *                         [8] the record's own sum |r|, [9] its valid points: the cost PER SEGMENT, what the verdict's within-pair
 *                         test reads; [10], [11] unused).
 * The solvers sum records in index order.  Per pair they need its span range (SpPair.tile0, n_tiles), the index of
 * its first segment record (rec0) and, per segment, the record range of its chunks (seg_tile_off, relative to rec0).
 * ---------------------------------------------------------------------------------------------------- */
#define SP_GRAD_SEG_FLOATS 1
#define SP_GN_SEG_FLOATS 12
#define SP_GNA_SEG_FLOATS 12
typedef struct SpPair {
    const uint32_t* pix;      /* [P_padded] */
    const float*    src4;     /* [P_padded*4] for the level being optimised */
    const float*    kp_L;     /* [N] */
    const float*    trg3;     /* [Hl*Wl*3] packed HWC3, for the level being optimised */
    float*          kld;      /* [N]  optimisation variable */
    float*          pose;     /* [16] optimisation variable (target <- source) */
    float*          aff;      /* [4]  {a_s,b_s,a_t,b_t} or NULL */
    const int32_t*  seg_tile_off; /* [N+1] offsets into this pair's segment records, relative to rec0 */
    float K_src[4];           /* fx fy cx cy */
    float K_trg[4];
    int32_t N, P, H, W, Hl, Wl;   /* P = number of REAL points (the cost is a mean over 3 P values) */
    int32_t tile0;            /* first span of this pair */
    int32_t n_tiles;          /* number of spans (workgroups) of this pair */
    float zmin;
    int32_t rec0;             /* first segment record of this pair (= 4 * its first chunk) */
} SpPair;
SP_ABI_SIZE(SpPair, 136)

/* HOST helpers (no device work): the work list above for a whole batch.  pc[s] / seg_pos[s]: padded run length and pair-relative
 * position of every segment (all pairs concatenated), n_off[m]: first segment of pair m (n_pairs + 1 entries).  Chunks: pieces of at
 * most tile_points points (granule-aligned, nearly equal) of every segment; spans: greedy runs of consecutive chunks of one pair up
 * to span_points points.  sp_host_work_list_chunks returns the number of chunks (sizes the arrays: chunks and spans 4 int32 per
 * entry, spans at most as many as chunks); sp_host_work_list fills chunks, spans, seg_tile_off (per pair N + 1 record offsets, 4
 * records per chunk; sum N + n_pairs entries, pair m at sto_off[m]), c_off / s_off (first chunk / span of every pair) and returns
 * the number of spans. */
int sp_host_work_list_chunks(const long long* pc, int n_segs, int tile_points, int granule);
/* The padded layout of every lattice of a batch from the per-segment point counts (counts[l * n_segs + s], as sp_prepare_count leaves
 * them): pc = the count rounded up to the granule, seg_pos = the segment's first point relative to its pair's table, p_off[l * (n_pairs +
 * 1) + m] = first point of pair m in the lattice's flat arrays, seg_off[l * 2 n_segs ...] = the segment positions as int32, first inside
 * the flat array (sp_prepare_fill), then relative to the pair (sp_prepare_sample, SpPair.seg_tile_off's companion), points[l * n_pairs +
 * m] = real points of pair m.  One pass where the numpy form takes a dozen array operations per lattice. */
int sp_host_layout(const int32_t* counts, int n_lattices, int n_segs, const long long* n_off, int n_pairs, int granule,
                   long long* pc, long long* seg_pos, long long* p_off, int32_t* seg_off, long long* points);
int sp_host_work_list(const long long* pc, const long long* seg_pos, const long long* n_off, int n_pairs, int span_points,
                      int tile_points, int granule /* 256, or 64 for wave spans */, int records_per_chunk /* 4, or 1 for wave spans */,
                      int32_t* chunks, int32_t* spans, int32_t* seg_tile_off, long long* sto_off, long long* c_off, long long* s_off);

/* WAVE SPANS (mode | SP_COST_WAVE_SPANS, modes 0 and 1): a work list whose spans belong to single WAVES instead of workgroups -- the
 * tables are padded to multiples of 64 points instead of 256, chunk counts are multiples of 64, and there is ONE segment record per
 * chunk (record index = chunk index) instead of four.  For batches of many small ragged segments (SAM-like masks): at 1200
 * segments of ~280 pixels the 256-point granule pads 40 %, the 64-point granule 11 %.  Four consecutive spans share a workgroup. */
#define SP_COST_WAVE_SPANS 0x100
/* DEPTH TABLES (mode | SP_COST_DEPTH_TABLE, modes 0 and 1, with or without wave spans): src4.w of the tables holds exp(L) -- the
 * source depth at the segment's seed -- instead of L, and a point's depth is src4.w * exp(kld - kp_L): the exponential is taken once
 * per chunk (a scalar) instead of once per point (v_exp_f32 is a quarter-rate transcendental; -1.8 % kernel time on the headline
 * workload, profiles/r04_kernel_experiments.txt).  Same value up to 2 ulp of the product.  sp_prepare_sample writes such tables with
 * SP_PREP_DEPTH_TABLE. */
#define SP_COST_DEPTH_TABLE 0x200

/* mode 0 / 1 as above.  mode 2 = mode 1 plus the affine brightness pair of the TARGET frame as two more unknowns (a_t, b_t; the
 * source frame's pair enters with the opposite sign): residual columns j_a = gain * I_trg(sample), j_b = -1.  Span record
 * (SP_GNA_PARTIAL_FLOATS): [0..28] as mode 1, [29..31] H_aa = {aa, ab, bb}, [32,33] b_a, [34..39] H_{a,pose}, [40..45] H_{b,pose};
 * segment record (SP_GNA_SEG_FLOATS): [0..7] as mode 1, [8] H_{a,depth}, [9] H_{b,depth}.  Consumed by sp_window_gn_step.
 * mode 2 takes neither flag; any other value of mode is SP_EINVAL (checked before any device work).
 *
 * WHAT EVERY RECORD SUMS (tests/cost_pass_ref.py restates one launch in float64 from this paragraph; tests/test_gpu_cost_pass.py holds every
 * column of every record of every variant to it).  Per table point, with col / row / src_ok from its pixel word:
 *     d = exp(src4.w + kld[seg] - kp_L[seg])   (depth tables: src4.w * exp(kld[seg] - kp_L[seg]));   p = ((col - cx_s) d / fx_s, (row - cy_s) d / fy_s, d)
 *     q = R p + t;   zi = 1 / qz where |qz| > 1e-6, else 1e-6;   u = fx_t qx zi + cx_t;   xn = 2 u / (W - 1) - 1;   ix = (xn + 1) (Wl - 1) / 2   (v, yn, iy alike)
 *     m = src_ok and d > 1e-7 and |xn| <= 0.99 and |yn| <= 0.99 and qz > zmin:  a point whose m is false -- every padding point -- adds ZERO to every column
 *     I, Ix, Iy per channel: bilinear value and slopes (level pixels) from the four taps at floor(ix), floor(iy);   gain = exp(-(a_t - a_s)), bias = b_t - b_s
 *     r = I_src - (gain I + bias);   w = 1 / max(|r|, irls_eps);   J = -gain (Ix ax fx_t zi Ahat0 + Iy ay fy_t zi Ahat1),  ax = (Wl - 1) / (W - 1), ay = (Hl - 1) / (H - 1)
 *     Ahat0 = [1, 0, -ux, -ux qy, qz + ux qx, -qy, ex - ux ez],  Ahat1 = [0, 1, -vy, -(qz + vy qy), vy qx, qx, ey - vy ez],  ux = qx / qz, vy = qy / qz, e = q - t
 *   over the unknowns [tau(3), phi(3)] of the left perturbation Exp(xi) T and the segment's log-depth (column 6).  Modes 1, 2 sum over channels and points
 *   m w J_i J_j (H_pp: i <= j < 6, row-major; h_pd: j = 6; D: i = j = 6), m w r J_i (b_p, b_d), m |r| and m; mode 2 the same with j_a = gain I, j_b = -1 for
 *   [29..45] / segment [8], [9] ([30] = sum w j_a j_b, [33] = sum w r j_b).  Mode 0 sums, with s = sign(r) and g = -gain (ax fx_t zi sum s Ix, ay fy_t zi
 *   sum s Iy, .) whose third component is -(g_x qx + g_y qy) / qz:  [0] m |r|, [1..3] g, [4..12] g p^T (row-major), [14] gain sum s I, [15] -sum s; segment: g . (q - t).
 *   WHICH POINTS:  span record s sums the points of the chunks spans[s].first .. + spans[s].n.  Segment record 4 q + w of chunk q sums the points
 *   chunk.start + 256 j + 64 w + lane (j < count / 256, lane < 64) -- those wave w handles -- and under SP_COST_WAVE_SPANS record q sums all points of chunk q.
 *   [8] / [9] of a mode-1 segment record are sum |r| and the valid points of exactly those points.
 *   UNUSED COLUMNS:  every float of a span record is written, the columns without a meaning as 0 (mode 0: [13]; mode 1: [29..31]; mode 2: [46], [47]).
 *   Of a segment record modes 1 and 2 write [0..9] and NEVER [10], [11], which keep what the buffer held.  Nothing is written past record n_spans - 1 /
 *   4 C - 1 (C - 1 under wave spans), nor to the records of a span skipped through `done`; a segment without points has no chunk and no record.
 *
 * sp_pairs_cost_opt is sp_pairs_cost with three optional arguments; sp_pairs_cost passes NULL for each.
 *   done (n_pairs int32, see sp_pairs_gn_step_conv): workgroups return at once for spans of marked pairs, so that an iteration
 *     costs time only for the pairs still moving.
 *   pix_base, desc (both or neither; mode 0 or 1 | SP_COST_WAVE_SPANS | SP_COST_DEPTH_TABLE, anything else is SP_EINVAL): the pixel
 *     words come from RUN DESCRIPTORS (SpRunDesc below) instead of pix.  pix_base = the flat pix array every pair's SpPair.pix
 *     points into (pair tables start at multiples of 64 points from it), desc = sp_run_desc_build of that array, without groups of
 *     more than two runs.  Bitwise the same partials as without them. */
int sp_pairs_cost(const SpPair* pairs, const int32_t* chunks, const int32_t* spans, int n_spans, int mode, float irls_eps,
                  float* span_partials, float* seg_partials, void* stream);
struct SpRunDesc;
int sp_pairs_cost_opt(const SpPair* pairs, const int32_t* chunks, const int32_t* spans, int n_spans, int mode, float irls_eps,
                      float* span_partials, float* seg_partials, const int32_t* done, const uint32_t* pix_base,
                      const struct SpRunDesc* desc, void* stream);

/* Adam step on {kld, left SE(3) tangent, affine} of every pair from the mode-0 partials: reduces the tile
 * partials (fixed order, fp64), loss = |residual| like odometery/two_frame_sfm.py:201-206, maps d/dpose to the
 * tangent of Exp(a)*T, applies torch.optim.Adam semantics (betas 0.9/0.999, eps 1e-8, bias correction) with
 * per-group learning rates, retracts pose <- Exp(step)*pose.  state: per pair (2*(N+6+2)+2) floats, zeroed
 * by the caller before the first step.  losses: [n_pairs] written every step.
 * Pinned call by call (pair_adam_step_ref in tests/window_adam_step_ref.py, tests/test_gpu_pairs_adam_step.py): the sign is taken of the
 * FLOAT32 residual (0 -> every gradient is zero and the moments still decay); state per pair = {step count, unused, m_kld[max_N],
 * v_kld[max_N], m_xi[6], v_xi[6], m_aff[2], v_aff[2]} with nothing written behind N in m_kld / v_kld; the tangent starts from zero in every
 * call (xi = the Adam step itself); only aff[2, 3] (the target's pair) move, aff[0, 1] and -- when aff is NULL -- m_aff / v_aff stay; the
 * pose is Exp(xi) pose in float64 rounded once, its last row set to 0 0 0 1; bias corrections by pow() from the step count. */
int sp_pairs_adam_step(const SpPair* pairs, int n_pairs, int max_N, const float* span_partials, const float* seg_partials,
                       float lr_kld, float lr_pose, float lr_aff, float* state, float* losses, void* stream);

/* Gauss-Newton / Levenberg-Marquardt step from the mode-1 partials: per pair, reduce tiles, eliminate the
 * N diagonal log-depth unknowns (Schur complement onto the 6x6 pose block), solve in fp64, update
 * pose <- Exp(delta)*pose and kld += delta_d.  lm_state: per pair SP_LM_STATE_FLOATS floats {lambda, cost of
 * the last accepted point (init -1), n accepted, n rejected, rejected-last-call flag, last cost seen, the valid points of that
 * evaluation / P, and -- schedules only -- how the pair's last finished phase ended: +iterations = on its cap, -iterations = by
 * its convergence test};
 * lambda adapts on device (cost up -> step undone from the backup, lambda*=lm_up, re-evaluated next call;
 * cost down -> lambda = max(lambda*lm_down, lm_min)).  backup: per pair (16+max_N) floats.  costs: [n_pairs].
 * One call, in full (tests/gn_step_ref.py restates it in float64; tests/test_gpu_gn_step.py holds the device to it):
 *   cost = sum|r| / (3 P) is written to costs and lm_state[5] (valid points / P to [6]) by every call that looks at the pair.
 *   REJECT iff a last accepted cost exists, cost > last * (1 + 1e-6) and the previous call did not reject: pose and log-depths come
 *     back from the backup bit for bit, lambda *= lm_up, [3] += 1, [4] = 1; nothing else moves.
 *   Otherwise a STEP: lambda = max(lambda * lm_down, lm_min) unless the previous call rejected (so the first call lowers it too); the
 *     point is copied to the backup (pose, then the pair's N log-depths: the rest of the slot is never written); the system is damped as
 *     H_pp + lambda diag(H_pp) + 1e-12 I and D (1 + lambda); a segment whose damped D is <= 1e-12 (no valid point) is no unknown: it
 *     stays where it is and does not enter the pose block; every log-depth step is clamped to +-0.5; [1] = cost, [2] += 1, [4] = 0.
 *     When the pose block is not positive definite after the elimination (a failed LDL^T pivot) the pose stays where it is, every
 *     log-depth still takes its own clamped step -b_d / D', and the call counts as an accepted step like any other. */
#define SP_LM_STATE_FLOATS 8
int sp_pairs_gn_step(const SpPair* pairs, int n_pairs, int max_N, const float* span_partials, const float* seg_partials,
                     float lm_up, float lm_down, float lm_min, float* lm_state, float* backup, float* costs, void* stream);

/* Per-pair convergence on the device (the counterpart of the reference's relative-loss early stop, odometery/odometery.py:907-915,
 * for a batch whose pairs need different numbers of iterations).  sp_pairs_gn_step_conv marks done[pair] = 1 -- and leaves the pair
 * at its current point -- when the step that led to the evaluated point was accepted and lowered the cost by less than
 * conv_tol * cost; it returns immediately for pairs already marked, and sp_pairs_cost_opt skips their spans.  done: n_pairs int32,
 * zeroed by the caller (per pyramid level).  conv_tol <= 0 / done == NULL: exactly sp_pairs_gn_step / sp_pairs_cost. */
int sp_pairs_gn_step_conv(const SpPair* pairs, int n_pairs, int max_N, const float* span_partials, const float* seg_partials,
                          float lm_up, float lm_down, float lm_min, float* lm_state, float* backup, float* costs, float conv_tol,
                          int32_t* done, void* stream);

/* RUN DESCRIPTORS (sp_pairs_cost_opt): the pixel words of a wave-span table (granule 64) rebuilt from one 32-byte record per 64-point group instead of
 * read point by point (4 B per point of the cost pass's stream).  A group lies inside one chunk of one segment, its points in
 * row-major order: its points form RUNS of consecutive pixels of one row, and with at most two runs (every segment at least 64
 * pixels wide) lane l of the group decodes as
 *     step = clamp(l + k, 0, 1)          (0 in run 0, 1 in run 1: k = 1 - s1, s1 = first lane of run 1, 64 without one)
 *     col  = base[0] + l + step * d[0],   row = base[1] + step * d[1],   validity bit = bit l of valid
 * (integer-valued floats, exact).  Lanes past the group's last nonzero word (the padding of a segment) continue the last run;
 * they are invalid.  runs > 2: the formula does not hold for that group.  Record n_groups (one past the table) is written too, as
 * that of an all-zero group: the cost pass prepares one trip past the end of a span. */
typedef struct SpRunDesc {
    uint32_t valid[2];           /* bit l of the 64-bit mask: bit 31 of the group's word l */
    float d[2];                  /* run 1 relative to run 0: {c1 - s1 - c0, r1 - r0} ({0, 0} without run 1) */
    float base[2];               /* {col, row} of lane 0 */
    float k;                     /* 1 - s1 */
    int32_t runs;                /* runs among the group's points (1 for an all-zero group) */
} SpRunDesc;
SP_ABI_SIZE(SpRunDesc, 32)

/* descriptors of the n_groups groups of pix[0 .. 64 n_groups) into desc[0 .. n_groups] (n_groups + 1 records); *n_general
 * (device int32, zeroed by the caller) += number of groups with more than two runs.  Build it after the table's validity bits are
 * final (sp_prepare_sample / sp_table_sample_source). */
int sp_run_desc_build(const uint32_t* pix, int n_groups, SpRunDesc* desc, int32_t* n_general, void* stream);

/* A whole coarse-to-fine schedule PER PAIR on the device.  Phase p of the schedule runs on the descriptors `pairs` of one pyramid
 * level (every phase describes the same n_pairs pairs) over the work list (chunks, spans) of that level's point set -- a coarse
 * level may run on a decimated copy of the source points with its own, shorter work list -- with IRLS epsilon irls_eps; a pair
 * moves on to phase p + 1 when an accepted step lowers its cost by less than conv_tol * cost, or after max_iters iterations, and
 * is finished at phase n_phases.  phase[n_pairs] / iters[n_pairs] (int32, zeroed by the caller) hold every pair's position; the
 * host only issues (sp_pairs_schedule_cost, sp_pairs_schedule_gn_step) until min(phase) == n_phases.  Pairs advance
 * independently: one slow pair no longer keeps the others at a coarse level, and finished pairs cost nothing.
 * sp_pairs_schedule_cost runs the Gauss-Newton cost pass over every DISTINCT work list (phases sharing `spans` share the list) in
 * ONE launch -- up to four lists of the same kind (wave spans or workgroup spans), one after the other in block order; otherwise a
 * launch per list; partial buffers of different work lists must not alias.  The struct lives in host memory. */
#define SP_MAX_PHASES 12
/* SP_PHASE_POSE_ONLY: the phase moves the pose alone, the log-depths stay where they are (the solver skips the Schur complement
 * and the depth update; the cost pass is unchanged).  From the reference's own starting distribution (pose off by SE3.Random(sigma =
 * 0.05), depth seeds log(2 + 2 rand), odometery/two_frame_sfm.py:77-81,103-105) a joint Gauss-Newton step lets single segments run
 * away in depth while the pose is still wrong -- the total cost keeps falling, so LM never objects; the reference's Adam moves the
 * pose 10x faster than the depths (lr 1e-2 vs 1e-3, :116-123) and so aligns the pose first.  A pose-only phase at the coarsest
 * level is the Gauss-Newton counterpart (tools/gn_model.py, profiles/r03_sigma05_sweep.txt). */
#define SP_PHASE_POSE_ONLY 1
/* SP_PHASE_WAVE_SPANS: the phase's work list is wave-granular (see SP_COST_WAVE_SPANS). */
#define SP_PHASE_WAVE_SPANS 2
/* SP_PHASE_DEPTH_TABLE: the phase's tables are depth tables (see SP_COST_DEPTH_TABLE); all phases of one schedule alike. */
#define SP_PHASE_DEPTH_TABLE 4
/* SP_PHASE_DEPTH_DAMP(k), k = 0..255: the phase's Gauss-Newton step damps the log-depth block by k / 8 on top of the LM lambda --
 * (H_dd (1 + lambda + k/8)) -- so that the depths follow the pose at a fraction of their Gauss-Newton step, the way the reference's
 * Adam moves them at a tenth of the pose's rate (odometery/two_frame_sfm.py:116-123: lr 1e-3 against 1e-2).  On near-planar scenes
 * (a narrow depth range: the two-fold ambiguity of a plane's homography) the undamped joint step walks into the second solution from
 * the reference's own starts; a damped coarse phase in front of the undamped ones does not (profiles/r05_reference_start.txt). */
#define SP_PHASE_DEPTH_DAMP_SHIFT 8
#define SP_PHASE_DEPTH_DAMP(k) (((k) & 0xff) << SP_PHASE_DEPTH_DAMP_SHIFT)
/* SP_PHASE_ADAM (ABI 13): the phase's update is THE REFERENCE'S OWN OPTIMISER instead of a Gauss-Newton step -- one torch.optim.Adam
 * step (betas 0.9 / 0.999, eps 1e-8, bias correction) on {left pose tangent, log-depths} at the rates SpSchedule.adam_lr_pose /
 * adam_lr_kld (odometery/two_frame_sfm.py:116-123: 1e-2 / 1e-3), pose <- Exp(step) pose.  The gradient is that of the phase's cost pass:
 * b_p and b_d of the IRLS normal equations are sum sign(r) J wherever |r| > irls_eps, i.e. the gradient of the reference's mean |r|
 * (two_frame_sfm.py:201) up to the smoothing inside irls_eps; no Hessian is used, no step is ever rejected.  The phase ends on max_iters
 * (conv_tol is ignored).  Moments: SpSchedule.adam_state, per pair / slot 2 + 2 (max_N + 8) floats laid out like sp_pairs_adam_step's;
 * they persist over consecutive phases (the reference keeps one optimiser over its three pyramid levels, :128-155) and are zeroed whenever
 * a pair (re)starts an attempt.  What it is for: the THIRD attempt of a pair whose two Gauss-Newton attempts failed their verdict
 * (SpSchedule.retry2_entry) -- Gauss-Newton's path from a few of the reference's own starts in ten thousand leads into the second solution
 * of a near-plane's homography under every damping tried, the reference's Adam path from the same starts does not (goldens g20y). */
#define SP_PHASE_ADAM 8
/* SP_PHASE_PREDICTED_EXIT (ABI 13): a pair also leaves the phase right after a step that is PREDICTED to buy less than conv_tol of its cost
 * -- the first-order change of sum |r| along the step, b . delta, which the solver has at hand -- instead of only after the NEXT evaluation
 * has shown that it did: one cost evaluation per phase saved (the all-points polish's is a tenth of a frame pair's work).  Skipped while
 * the LM lambda is above 1e-2 or the phase damps the depth block (a short step is then the damping's doing).  The step is applied. */
#define SP_PHASE_PREDICTED_EXIT 16
typedef struct SpPhase {
    const SpPair* pairs;
    const int32_t* chunks;
    const int32_t* spans;
    float* span_partials;        /* n_spans * SP_GN_PARTIAL_FLOATS */
    float* seg_partials;         /* 4 * n_chunks * SP_GN_SEG_FLOATS */
    int32_t n_spans;             /* 0 = an empty point set: nothing is launched, its pairs pass through the phase */
    int32_t max_iters;
    float irls_eps;
    float conv_tol;
    int32_t flags;               /* SP_PHASE_* */
    int32_t next;                /* the phase a pair moves on to: 0 = the following one (p + 1), k > p = phase k (skips phases p+1..k-1) */
} SpPhase;
SP_ABI_SIZE(SpPhase, 64)
/* entry: the phase a fresh pair starts in.  retry_entry: the phase a pair RESTARTS in -- from its initial pose and log-depths, once --
 * when its verdict at the end of the schedule says it failed (SpVerdict below); -1 = no second attempt.  The phases in front of
 * `entry` belong to the later attempts only: with phases {R0, R1 (next = J), P0, J, ..., polish}, entry = 2 and retry_entry = 0 a
 * first attempt runs P0, J, ..., polish and a second one R0, R1, J, ..., polish.  retry2_entry (ABI 13): where a pair restarts, from
 * its initial values again, when the SECOND attempt fails its verdict too -- -1 = no third attempt; with {A0, A1 (next = J'), R0, ...}
 * and retry2_entry = 0 the third attempt runs A0, A1, J', ..., polish (A* = SP_PHASE_ADAM phases in REFERENCE_START_SCHEDULE). */
typedef struct SpSchedule {
    SpPhase phase[SP_MAX_PHASES];
    int32_t n_phases;
    int32_t entry;
    int32_t retry_entry;
    int32_t retry2_entry;
    float adam_lr_pose, adam_lr_kld;     /* SP_PHASE_ADAM phases */
    float* adam_state;                   /* [pairs or slots][2 + 2 (max_N + 8)], device; NULL when no phase is SP_PHASE_ADAM */
} SpSchedule;
SP_ABI_SIZE(SpSchedule, 800)

/* THE VERDICT of a scheduled run, per pair, on the device.  The reference asserts finiteness every iteration and nothing else
 * (core/dense_optim.py:311,321,340-343); a Gauss-Newton schedule that ends in the wrong basin (about one of the reference's own
 * starts in a thousand, odometery/two_frame_sfm.py:77-84,103-105) would otherwise hand back a wrong pose silently.  The solver
 * workgroup that takes a pair out of its last phase writes
 *   status[pair]  SP_STATUS_* bits; 0 = converged at the first attempt, SP_STATUS_RETRIED alone = converged at the second;
 *   diag[pair * SP_DIAG_FLOATS]  {final cost, max_n |kld_n - kld0_n|, valid points / points of the last evaluated cost,
 *                                 iterations spent in the last phase, attempts made, cost at the first evaluation,
 *                                 median and maximum over the pair's segments of the segment's mean |r| (0 = not judged)}
 * and, when (status & retry_mask) and the schedule has a retry_entry and the pair has made one attempt, puts pose and log-depths
 * back to pose0 / kld0, resets its LM state (lambda = lam0) and restarts it at retry_entry IN THE SAME LAUNCH -- the pair keeps its
 * slot, the resident set stays full.  A pair's verdict depends on the pair alone (no batch statistics): bitwise what it is alone.
 * pose0 / kld0: the initial values, laid out like the batch's own pose / kld arrays (pose_base / kld_base: element 0 of those).
 * THE SMALL PRINT (pinned by tests/test_gpu_schedule_verdict.py against tests/schedule_verdict_ref.py):
 *   - every test is a strict comparison in float32: a quantity EQUAL to its bound is not flagged; a bound <= 0 switches its test off;
 *   - finiteness is tested of pose entries 0..11 (the last row is constant and not looked at), of the pair's N log-depths and of the
 *     final cost; a magnitude above 3e38 counts as non-finite; diag[1] is the maximum over the finite differences only;
 *   - diag[5] is the first evaluated cost of the attempt that is not exactly 0 (a first cost of 0 leaves it for the next evaluation);
 *     cost_ratio is tested only against a first cost > 0;
 *   - a segment's mean |r| is float32(a / (3 c)), a / c = the float64 sums of columns [8] / [9] over its records; the median is the LOWER
 *     median, rank (n_judged - 1) >> 1 of the judged costs ordered by (value, segment index); diag[7] is the maximum over every judged
 *     segment, also when fewer than SP_VERDICT_MIN_SEGMENTS are judged -- there is then no median (diag[6] = 0) and no segment test;
 *   - a restart sets lm_state[0, 1, 4, 7] = {lam0, -1, 0, 0}, iters = 0, diag[5] = 0, attempts[pair] = the attempt's number and zeroes the
 *     slot's Adam moments; lm_state[2, 3] (the iteration counts) run on over all attempts, lm_state[5, 6] keep the last evaluated cost and
 *     valid fraction until the next evaluation; status, the rest of diag, backup and costs are left alone; pose (all 16 entries) and the
 *     pair's N log-depths are bitwise pose0 / kld0;
 *   - with attempts == NULL a pair counts as having made its last attempt: nothing is retried, diag[4] = 1, no SP_STATUS_RETRIED. */
#define SP_STATUS_NONFINITE   1   /* a non-finite pose entry, log-depth or cost */
#define SP_STATUS_LAST_CAP    2   /* the last phase ended on its iteration cap, not by its convergence test */
#define SP_STATUS_DEPTH_RANGE 4   /* some |kld - kld0| > kld_bound: a segment's depth ran away */
#define SP_STATUS_COST        8   /* final cost > cost_bound (absolute), or > cost_ratio * the cost at the first evaluation; the host layer also sets it
                                   * for a final cost far above the batch median (optim/pair_batch.py VERDICT_DEFAULTS['cost_outlier']) */
#define SP_STATUS_VALID       16  /* valid points of the last evaluated cost < valid_min * points */
#define SP_STATUS_SEGMENTS    32  /* (ABI 13) the cost is UNEVEN over the pair's own segments: the worst segment's mean |r| > seg_max_ratio x the median
                                   * segment's, or the pair's cost > seg_mean_ratio x the median segment's -- what the second solution of a near-plane's
                                   * homography looks like from the inside (some segments explained, others not); needs no other pair to compare with */
#define SP_STATUS_RETRIED     0x100   /* the verdict is a later attempt's (second or third) */
#define SP_STATUS_ADAM        0x400   /* ... the third one's: the pair went through the schedule's SP_PHASE_ADAM phases (retry2_entry) */
#define SP_STATUS_UNFINISHED  0x200   /* the run ended (max_rounds) before the pair left its last phase */
#define SP_DIAG_FLOATS 8
typedef struct SpVerdict {
    int32_t* status;             /* [pairs] written when a pair finishes (an attempt that is retried leaves nothing) */
    float* diag;                 /* [pairs * SP_DIAG_FLOATS] */
    int32_t* attempts;           /* [pairs] zeroed by the caller */
    const float* pose0;          /* [pairs * 16] */
    const float* kld0;           /* like the batch's flat log-depth array */
    const float* pose_base;
    const float* kld_base;
    float kld_bound;             /* <= 0: not tested */
    float cost_bound;            /* <= 0: not tested */
    float cost_ratio;            /* <= 0: not tested */
    float valid_min;             /* <= 0: not tested */
    int32_t retry_mask;          /* status bits that send a pair into its next attempt */
    float lam0;                  /* LM damping a later attempt starts with */
    float seg_max_ratio;         /* <= 0: not tested.  Segments with fewer than SP_VERDICT_SEGMENT_POINTS valid points in the last cost pass are not */
    float seg_mean_ratio;        /* judged (of the pair's first SP_VERDICT_SEGMENTS segments); pairs with fewer than SP_VERDICT_MIN_SEGMENTS judged segments are not tested */
    int32_t* evals;              /* [pairs * SP_MAX_PHASES] or NULL, zeroed by the caller: cost evaluations of every pair in every phase (diagnostics:
                                  * bench.py prices a scheduled run's algorithmic bytes with it, roofline_schedule) */
    float seg_product;           /* <= 0: not tested.  (cost / median - 1) x (worst / median) above this: a moderately raised cost TOGETHER WITH a clear
                                  * outlier segment -- neither ratio alone separates such a pair from a converged one with noisy small segments */
    float pad_;
} SpVerdict;
SP_ABI_SIZE(SpVerdict, 104)
#define SP_VERDICT_SEGMENTS 2048
#define SP_VERDICT_SEGMENT_POINTS 64
#define SP_VERDICT_MIN_SEGMENTS 8
int sp_pairs_schedule_cost(const SpSchedule* sched, const int32_t* phase, void* stream);
int sp_pairs_schedule_gn_step(const SpSchedule* sched, int n_pairs, int max_N, float lm_up, float lm_down, float lm_min,
                              float* lm_state, float* backup, float* costs, int32_t* phase, int32_t* iters, const SpVerdict* verdict /* or NULL */,
                              void* stream);

/* The host loop of a scheduled run, natively: issues (sp_pairs_schedule_cost, sp_pairs_schedule_gn_step) up to max_rounds times and,
 * every check_every iterations, polls the pairs' phases (one tiny kernel, a copy of five int32 into flag_host -- PINNED host memory --
 * and a synchronisation of `stream` only) to stop once every pair has finished; work lists whose phases all lie behind the minimum
 * are no longer launched (pairs only move forward).  One foreign call per scheduled run instead of ~100: a
 * Python caller issues nothing per iteration, so several batches can run their schedules from several host threads without
 * contending for the interpreter lock (optim/pair_stream.py), and the launch-bound tail of a schedule runs at the rate of the
 * runtime's launch path.
 * flag_dev / flag_host: EIGHT int32 each (device scratch / pinned host memory).  THE POLL RECORD is the first five:
 *   [0] min(phase) over the pairs (slots)        [1] the queue's head (queue runs; else 0)
 *   [2] 1 when an unfinished pair has an attempt left (verdict runs with a second / third attempt)
 *   [3] how many pairs (slots) are still in a phase       [4] bit p set: phase p holds a pair        [5..7] spare
 * max_rounds: the run ends there whatever the pairs' state (SP_STATUS_UNFINISHED).  Until its first poll -- the first check_every
 * rounds -- this run takes every phase for occupied (the caller set the phases), while sp_pairs_schedule_run_queue takes only the
 * ENTRY phase for occupied (every slot starts there): a slot the caller put into an SP_PHASE_ADAM phase sits those rounds out, and
 * they count towards max_rounds -- as do the rounds a pair that restarts into such a phase waits for the next poll to see it.
 * Returns the number of iterations launched (>= 0), SP_EINVAL, or -(1000 + hipError_t) for a runtime error.  This and
 * sp_pairs_schedule_run_queue (the same host loop) are the entry points that synchronise the host (with `stream` only). */
int sp_pairs_schedule_run(const SpSchedule* sched, int n_pairs, int max_N, float lm_up, float lm_down, float lm_min,
                          float* lm_state, float* backup, float* costs, int32_t* phase, int32_t* iters, int check_every,
                          int max_rounds, int32_t* flag_dev, int32_t* flag_host, const SpVerdict* verdict /* or NULL */, void* stream);

/* SLOT-LEVEL CONTINUOUS BATCHING of a scheduled run.  n_queue pairs are resident (tables, unknowns, descriptors of every phase's
 * level / lattice: qpairs[p][n_queue], and the batch's work lists, which cover all n_queue pairs); n_slots <= n_queue of them are
 * worked on at a time -- the schedule's phase[p].pairs are the SLOT descriptors (slot_pairs[p] = phase[p].pairs, writable, n_slots
 * records, initially copies of the first n_slots pairs'), and lm_state / backup / costs / phase / iters are per slot.  The cost pass
 * is launched over VIRTUAL spans: max_spans[p] per slot (the largest span count of any pair in phase p's work list; a multiple of 4
 * for wave spans); virtual span v belongs to slot v / max_spans[p] and is span  slot descriptor's tile0 + v % max_spans[p]  of the
 * batch's list when that is below the descriptor's n_tiles, nothing otherwise.  So pairs of DIFFERENT padded layouts (ragged
 * segment sets: SAM masks, frontend/process_frame.py:207-250) share the slots, and every pair's partial sums are taken over its own
 * spans in its own order.  The solver launch that finishes a pair files its result under the pair's index (q_costs[pair], q_lm[pair *
 * SP_LM_STATE_FLOATS], the verdict's status / diag; pose and log-depths live in the pair's own storage), takes the next waiting pair
 * from `head` (device int32, initialised to n_slots; one atomic per finished pair), copies that pair's descriptor of every phase over
 * the slot's and restarts the slot at the schedule's entry phase with lambda = lam0.  The resident set stays full until the queue is
 * empty: no launch works on a thinning batch except the very last ones.  Which pair lands in which slot depends on timing; every
 * pair's result does not (pairs never interact; bitwise what the pair gives with all pairs resident).  slot_pair: device [n_slots],
 * initialised 0..n_slots-1.  phase[p].n_spans is ignored (n_slots * max_spans[p] virtual spans are launched).
 * flag_dev / flag_host, max_rounds and everything else: as sp_pairs_schedule_run (the poll record is taken over the slots; before the
 * first poll only the entry phase counts as occupied, see there); pairs still in a slot when the run ends on max_rounds get
 * SP_STATUS_UNFINISHED in verdict->status (when given) and their state as it is. */
typedef struct SpQueue {
    const SpPair* qpairs[SP_MAX_PHASES];
    SpPair* slot_pairs[SP_MAX_PHASES];
    int32_t max_spans[SP_MAX_PHASES];
    int32_t n_queue;
    int32_t pad_;
    int32_t* head;
    int32_t* slot_pair;
    float* q_costs;
    float* q_lm;
    float lam0;
    int32_t pad2_;
    int32_t* active;             /* (ABI 13) device scratch [n_slots] or NULL: the slots that still work on a pair, listed at every poll -- once the queue
                                  * is empty and at most an eighth of the slots are busy, the launches of a round go over those alone (the tail of a run:
                                  * a third attempt iterates 1500 rounds by itself) */
} SpQueue;
SP_ABI_SIZE(SpQueue, 296)
int sp_pairs_schedule_run_queue(const SpSchedule* sched, const SpQueue* queue, int n_slots, int max_N, float lm_up, float lm_down,
                                float lm_min, float* lm_state, float* backup, float* costs, int32_t* phase, int32_t* iters,
                                int check_every, int max_rounds, int32_t* flag_dev, int32_t* flag_host, const SpVerdict* verdict /* or NULL */,
                                void* stream);

/* (ABI 19) sp_pairs_adam_iterate / sp_pairs_gn_iterate are retired: an iteration is sp_pairs_cost[_opt] followed by sp_pairs_adam_step / sp_pairs_gn_step. */

/* ------------------------------------------------------------------------------------------------------
 * Fused SE(3)-Adam optimiser of the reference's driver loops (SURVEY.md section 8(b) "sp_adam_se3_step", 8(f) N1):
 * torch.optim.Adam + lietorch retr()/matrix() + the pose bookkeeping around one cost evaluation, for
 *   odometery/two_frame_sfm.py:116-123,150-207 (persistent tangent, pose = Exp(a) X, no update on the very first
 *   iteration), odometery/odometery.py:300-312,375-407 (tracking: zero-reset tangent, T_supp <- T_supp inv(Exp(d))) and
 *   odometery/odometery.py:576-648,756-915 (windowed mapping: several source keyframes, relative poses
 *   D_trg inv(T_trg) T_src inv(D_src), first keyframe fixed, oldest keyframe's depths frozen when the window is full,
 *   fold-in + renormalise_se3 + tangent reset every iteration, relative-loss early stop).
 *
 * The window is a graph.  NODES = poses; BLOCKS = per-keyframe log-depth vectors; EDGES = photometric terms
 * (source keyframe -> target frame).  Edge e IS pair e of an SpPair array (one array per pyramid level, same kld / pose /
 * aff pointers in all of them): SpPair.kld = its block's kld, SpPair.pose = a 16-float slot and SpPair.aff = a 4-float slot
 * {a_src, b_src, a_trg, b_trg} that sp_window_compose / sp_window_step fill.  One iteration =
 *     sp_pairs_cost(mode 0) over all edges  ->  sp_window_step                                   (3 launches, no host sync)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct SpWindowNode {
    float T[16];         /* kind 0: camera-to-world pose, updated in place by the fold-in; kind 1: the constant group element X */
    float a[6];          /* tangent [tau, phi]: zero between iterations (kind 0) / the persistent parameter (kind 1) */
    float m[6], v[6];    /* Adam moments of the tangent */
    float aff[2];        /* affine brightness (a, b) of this frame */
    float aff_m[2], aff_v[2];
    float lr_pose;       /* 0 = pose not optimised (first keyframe, odometery.py:589-592; source-only frames) */
    float lr_aff;        /* 0 = affine not optimised */
    int32_t kind;        /* 0: edge pose = inv(T_trg) T_src evaluated at zero tangents, T <- T inv(Exp(d)) after every step;
                            1: edge pose = Exp(a) X (two-frame SfM; such a node is only ever a target) */
    int32_t flags;       /* bit 0: renormalise_se3 after every iteration (odometery.py:868,879) */
} SpWindowNode;
SP_ABI_SIZE(SpWindowNode, 176)

typedef struct SpWindowEdge {
    int32_t src_node;    /* pose node of the source keyframe, -1 = identity (two-frame SfM) */
    int32_t trg_node;
    int32_t block;       /* log-depth block of the source keyframe */
    float weight;        /* loss = sum_e weight_e * (abs_loss ? |residual_e| : residual_e) */
} SpWindowEdge;
SP_ABI_SIZE(SpWindowEdge, 16)

typedef struct SpWindowBlock {
    float* kld;          /* [N] -- the SpPair.kld of every edge whose source is this keyframe */
    float* m;            /* [N] Adam moments */
    float* v;
    int32_t N;
    float lr;            /* 0 = frozen (oldest keyframe of a full window, odometery.py:594-603; tracking) */
} SpWindowBlock;
SP_ABI_SIZE(SpWindowBlock, 32)

/* doubles of scratch sp_window_step needs */
int sp_window_scratch_doubles(int n_edges, int max_N);

/* Write every edge's relative pose and affine slot from the current nodes (call once before the first cost pass). */
int sp_window_compose(const SpPair* pairs, const SpWindowEdge* edges, int n_edges, SpWindowNode* nodes, int n_nodes, void* stream);

/* One optimiser step from the mode-0 partials of sp_pairs_cost over `pairs`.  abs_loss: 1 = sum_e w_e |residual_e|
 * (two_frame_sfm.py:201-202), 0 = sum_e w_e residual_e (odometery.py:394,845-850).  skip_first: no parameter update on
 * iteration 0 (two_frame_sfm.py:203).  rel_tol > 0: once |loss - previous loss| / previous loss < rel_tol the window
 * freezes (later calls return without touching anything), like the break at odometery.py:907-915.
 * state: 12 floats, zeroed by the caller {Adam step count, iterations done, previous loss, converged flag, last loss, -,
 *   beta1^t and beta2^t as two doubles in [6..9]}; setting [0] = 0 restarts Adam's bias correction;
 * losses[max_losses]: loss of iteration i (evaluated BEFORE its update) at index i.
 * Pinned call by call (tests/window_adam_step_ref.py restates one call in float64; tests/test_gpu_window_adam_step.py holds the device to it):
 *   gradient   edge e enters with c_e = weight_e (abs_loss: weight_e sign(r_e), sign(0) = 0).  g_left = [g_t ; (A12 - A21, A20 - A02, A01 - A10)],
 *              A = R g_R^T + t g_t^T from the edge's pose slot; kind-0 target += c g_left, source += -c Ad_P^T g_left, kind-1 target += c
 *              <d(Exp(a) X)/da, dr/dP> (float32 dual numbers), affine target += c (d/da, d/db), source -=, block += c (segment sums).
 *   Adam       on the float32 gradient, torch's operation order; only for nodes / blocks that an edge names and whose lr is > 0; the bias
 *              corrections are the running products in state[6..9], restarted (with the moments kept) when state[0] == 0.
 *   poses      kind 0: T <- T Exp(-a) in float64 rounded once whenever a != 0, a <- 0, then renormalise_se3 where flags & 1 -- also for a
 *              node that is fixed or that no edge names; kind 1 keeps X and its tangent.  Every edge's pose slot (and aff slot, unless
 *              SpPair.aff is NULL) is re-composed by every call that is not frozen, the skipped iteration 0 included.
 *   state      [0] += 1 per update, [1] += 1 per call, [4] = loss; [2] is written only when rel_tol > 0; the freeze is decided on this call's
 *              loss AFTER its update went in ([3] = 1; the call itself still updates; iteration 0 never freezes); losses[it] only for it <
 *              max_losses; state[5, 10, 11] are never written; a frozen call writes nothing at all.
 *   Pinned as they are, and questionable: (1) a kind-0 node with a non-zero tangent is folded in even when no edge names it and lr_pose = 0;
 *   (2) under abs_loss an edge with r == 0 gives a zero gradient and still decays the moments of everything it touches, which moves those
 *   parameters; (3) a kind-1 node named as a SOURCE would get the kind-0 source gradient added to its persistent tangent -- it is only ever
 *   a target (above), and nothing tests that case on the device. */
int sp_window_step(const SpPair* pairs, const SpWindowEdge* edges, int n_edges, SpWindowNode* nodes, int n_nodes,
                   const SpWindowBlock* blocks, int n_blocks, int max_N, const float* span_partials, const float* seg_partials,
                   double* scratch, int abs_loss, int skip_first, float rel_tol, float* state, float* losses, int max_losses,
                   void* stream);

/* Gauss-Newton / Levenberg-Marquardt step of the SAME window graph (BASELINE.json north_star: "Gauss-Newton/LM solve on SE(3) (+)
 * log-depth"; the reference's loops it accelerates: odometery/odometery.py:375-407 tracking -- 6 pose + 2 affine unknowns, keyframe
 * depths fixed -- and :756-915 windowed mapping -- K poses + sum N log-depths + affines, first keyframe fixed (:589-592), oldest
 * depths frozen (:594-603), fold-in T <- T inv(Exp(D)) + renormalise_se3 after the step (:861-882)).  One iteration =
 *     sp_pairs_cost(mode 2, irls_eps) over all edges  ->  sp_window_gn_step                       (4 launches, no host sync)
 * Unknowns: the pose tangent of every node with lr_pose > 0, the affine pair of every node with lr_aff > 0 (the reduced camera system,
 * fp64: in LDS as a packed triangle up to 192 scalars -- the reference's own window, config/tum/odom_desk.yaml window_size 5 with two
 * supporting frames per keyframe and two running ones, all poses and affine pairs free (odometery.py:523-575,611-616), is 14 free
 * nodes = 112 -- and through global scratch up to 512 = 64 nodes), the log-depths of every block with lr > 0 (eliminated by a Schur
 * complement, like the per-pair solver; a depth unknown of keyframe k only couples with the frames k is matched against, and only
 * those columns are stored and summed).  No camera unknown at all is allowed (the 'supp' mapping of odometery.py:576-648: only the
 * latest keyframe's depths are free).  flags: SP_WGN_POSE_ONLY -- a pose-only step (all depth blocks treated as frozen);
 * SP_WGN_PREDICTED_EXIT (ABI 13) -- with conv_tol > 0 the window also freezes right after a step that is predicted to buy less than
 * conv_tol of the loss (the first-order change b . delta along the step; lambda <= 1e-2 only), without the evaluation that would
 * confirm it: see SP_PHASE_PREDICTED_EXIT.  SP_WGN_DEPTHS_FIXED (ABI 14) -- the caller's word that NO depth block moves (every
 * SpWindowBlock.lr is 0: frame-to-keyframe tracking); like SP_WGN_POSE_ONLY the Schur-term launch is then left out (its terms are all
 * zero): three launches per iteration instead of four.
 * LM: lambda adapts on the device exactly like sp_pairs_gn_step (loss up -> previous step undone from nodes_backup / kld_backup,
 * lambda *= lm_up, re-evaluated next call; loss down -> lambda = max(lambda lm_down, lm_min)).  A FAILED FACTORISATION (a pivot of the
 * reduced camera system <= 0 at this damping) moves no unknown, neither camera nor log-depth: lambda *= lm_up, state[8] += 1 and the
 * rejected-last flag state[4] = 1, so that the next call solves the same point again without a convergence test and without lowering
 * lambda; state[2] (accepted) and state[3] (rejected) both stay, state[1] takes this call's loss and the backups this point (which is the
 * point the call leaves: a later reject restores it), the loss is recorded and the iteration counted, the edges' slots are re-composed;
 * the predicted exit does not look at such a call.  One call in full: tests/window_gn_step_ref.py restates it in float64,
 * tests/test_gpu_window_gn_step.py holds the device to it.  conv_tol > 0: an accepted step that
 * lowered the loss by less than conv_tol * loss freezes the window (later calls return at once), like the relative-loss break at
 * odometery.py:907-915.
 * n_unknowns: the camera unknowns of the window (6 per node with lr_pose > 0 + 2 per node with lr_aff > 0), which sizes the scratch
 *   and selects the kernel; a window that turns out to have more freezes with state[9] = 1.
 * state: 16 floats {lambda (set by the caller, e.g. 1e-4), loss at the last accepted point (init -1), accepted, rejected,
 *   rejected-last flag, iterations, converged flag, last loss, failed solves, too-many-unknowns flag, ...}; losses[max_losses]: loss of
 *   call i.  scratch: sp_window_gn_scratch_doubles(n_edges, n_blocks, sum_N, max_N, n_unknowns) doubles; nodes_backup: n_nodes nodes;
 *   kld_backup: sum_N floats (blocks in order; sum_N = total log-depths of all blocks). */
#define SP_WGN_POSE_ONLY 1
#define SP_WGN_PREDICTED_EXIT 2
#define SP_WGN_DEPTHS_FIXED 4
int sp_window_gn_scratch_doubles(int n_edges, int n_blocks, int sum_N, int max_N, int n_unknowns);
/* where in the scratch the update kernel leaves 16 time stamps of its phases (100 MHz ticks; diagnostics, tools/window_bench.py) */
int sp_window_gn_profile_offset(int n_edges, int n_blocks, int sum_N, int max_N, int n_unknowns);
int sp_window_gn_step(const SpPair* pairs, const SpWindowEdge* edges, int n_edges, SpWindowNode* nodes, int n_nodes,
                      const SpWindowBlock* blocks, int n_blocks, int sum_N, int max_N, int n_unknowns, const float* span_partials,
                      const float* seg_partials, double* scratch, SpWindowNode* nodes_backup, float* kld_backup, int flags,
                      float lm_up, float lm_down, float lm_min, float conv_tol, float* state, float* losses, int max_losses,
                      void* stream);

/* S WINDOWS PER LAUNCH (ABI 13, config 3's throughput form: S independent sequences side by side, as PairBatch is config 2's).  One window's
 * Gauss-Newton iteration is four small dependent launches that leave the chip empty; here every launch covers all the windows -- the cost
 * pass goes over the S work lists one after the other in block order, the reduce / Schur / update kernels take the window from blockIdx.z
 * (grids sized for the largest window) -- and the host loop polls ALL states with one copy.  windows: host array, one record per window
 * (what sp_window_gn_run takes as arguments); args_dev: device scratch of n_windows * sp_window_gn_multi_bytes() bytes; states_dev / states_host
 * (pinned): n_windows * 16 floats.  The update kernel's instantiation is that of the window with the most camera unknowns.  Per window the
 * arithmetic is sp_window_gn_run's (bitwise: tests/test_gpu_window_gn.py).  With conv_tol > 0 the loop ends when EVERY window froze; a frozen
 * window's launches return at once.  Returns the iterations launched or a negative error. */
typedef struct SpWindowGn {
    const SpPair* pairs;             /* the window's edges as frame pairs, at the pyramid level of this phase */
    const int32_t* chunks;
    const int32_t* spans;
    const SpWindowEdge* edges;
    SpWindowNode* nodes;
    const SpWindowBlock* blocks;
    float* span_partials;
    float* seg_partials;
    double* scratch;                 /* sp_window_gn_scratch_doubles(...) */
    SpWindowNode* nodes_backup;
    float* kld_backup;
    float* state;                    /* 16 floats, as sp_window_gn_step */
    float* losses;
    int32_t n_spans, n_edges, n_nodes, n_blocks, sum_N, max_N, n_unknowns, max_losses;
} SpWindowGn;
SP_ABI_SIZE(SpWindowGn, 136)
int sp_window_gn_multi_bytes(void);
int sp_window_gn_run_multi(const SpWindowGn* windows, int n_windows, float irls_eps, int flags, float lm_up, float lm_down, float lm_min,
                           float conv_tol, int max_iters, int check_every, void* args_dev, float* states_dev, float* states_host, void* stream);

/* Up to max_iters iterations -- sp_pairs_cost(mode 2, irls_eps) over the window's work list + sp_window_gn_step -- as ONE foreign call
 * (the Python loop of optim/window.py run_gn): every check_every iterations the 16-float state is copied to state_host (pinned) and this
 * stream synchronised; with conv_tol > 0 the loop ends once the window froze.  Returns the iterations launched (>= 0), SP_EINVAL, or
 * -(1000 + hipError_t). */
int sp_window_gn_run(const SpPair* pairs, const int32_t* chunks, const int32_t* spans, int n_spans, float irls_eps,
                     const SpWindowEdge* edges, int n_edges, SpWindowNode* nodes, int n_nodes, const SpWindowBlock* blocks, int n_blocks,
                     int sum_N, int max_N, int n_unknowns, float* span_partials, float* seg_partials, double* scratch,
                     SpWindowNode* nodes_backup, float* kld_backup, int flags, float lm_up, float lm_down, float lm_min, float conv_tol,
                     float* state, float* losses, int max_losses, int max_iters, int check_every, float* state_host, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Helpers around the path
 * ---------------------------------------------------------------------------------------------------- */

/* Dense (N,H,W) seeded depths.  log_space = 1: (L + shift_n) * mask  (core/dense_optim.py:38-80
 * infer_depth_seeds);  log_space = 0: exp of that  (core/dense_optim.py:164-174 unproject_kf_to_depths).
 * shift_n = kld[n] - L[n] at the keypoint's pixel; that pixel is float32 0.5 (size - 1) (kp + 1) rounded half to even, per
 * axis.  Outside the masks the product is 0, so the two forms hold exactly 0.0 and exactly 1.0 there.  Every pixel of
 * every segment is written, whatever N*H*W (grid-stride loop over at most 1024 blocks per segment). */
int sp_depth_expand(const uint8_t* masks, const float* logdepth, const float* keypoints, const float* kld, int N,
                    int H, int W, int log_space, float* out, void* stream);

/* core/ops.py:59-96 estimate_depth_diff (mean=False) on table points moved by pose: last-writer-wins z splat
 * at truncated (v,u); ties resolved by highest point index (deterministic, one of the orders the reference's
 * scatter_ may produce).  out: (H,W) zero-initialised by this call.  keys: H*W uint64 scratch.
 * Pinned by tests/test_gpu_segment_depth.py against the float64 statement tests/segment_depth_ref.py:
 *   - the pixel is (trunc v, trunc u), truncation toward ZERO like .long(): u in (-1, 0) lands in column 0 and v in (-1, 0) in
 *     row 0 (floor would drop them); the last row and column are H - 1 and W - 1;
 *   - a point is kept iff z > 1e-6, u and v are finite and the pixel is inside the image; a NaN depth fails z > 1e-6, so a
 *     point with a NaN log-depth vanishes and changes nothing but the pixels it would have won;
 *   - table order is segment by segment, row-major within a segment; the point with the highest table index wins a pixel;
 *   - an untouched pixel is exactly 0; two calls give the same bits. */
int sp_depth_splat(const uint32_t* pix, const float* baseL, const int32_t* seg_off, const float* kp_L,
                   const float* kld, int N, int P, int H, int W, const float* K, const float* pose,
                   unsigned long long* keys, float* out, void* stream);

/* core/ops.py:84-92 estimate_depth_diff(mean=True): scatter_reduce_('mean') at the truncated pixel, WITH the reference's "initial
 * zero counted" semantics (include_self defaults to True): a pixel hit by c points holds sum(z) / (c + 1), an untouched one 0.
 * acc: 12*H*W bytes of scratch (32.32 fixed-point sums + counts: order independent).  No reference caller passes mean=True.
 * Which points are kept and where they land: exactly as sp_depth_splat. */
int sp_depth_splat_mean(const uint32_t* pix, const float* baseL, const int32_t* seg_off, const float* kp_L, const float* kld, int N,
                        int P, int H, int W, const float* K, const float* pose, void* acc, float* out, void* stream);

/* odometery/depth_init.py:10-67 segment_based_depth_reinit.  mode 0 = mean, 1 = median (lower middle for
 * even counts, like torch.median).  est_depth (H,W).  scratch: P floats.  out_kld[N], out_visible[N] u8.
 * Invisible segments receive the (lower) median of the visible segments' values.
 *   - a pixel's estimate is valid iff NOT (est < 1e-6): 5e-7 and 0 are invalid, 2e-6 is valid, and a NaN is VALID (the
 *     reference's ~(est < eps)) -- it makes its segment's result NaN; est_depth is read only;
 *   - a segment's result is the mean, or the LOWER median = the (cnt - 1) / 2-th smallest (0-based; for an even count the lower
 *     of the two middle values, an element of the data, never their average), of log(est) - L over its valid pixels, plus kp_L[n];
 *   - a segment without a valid pixel is flagged invisible and receives the lower median, rank (nvis - 1) / 2, of the nvis
 *     visible segments' results (equal results are ordered by segment index; the value is one of them, bit for bit);
 *   - NO segment visible: every out_kld is 0 and every flag 0 (the reference's torch.median raises on the empty selection). */
int sp_segment_reinit(const uint32_t* pix, const float* baseL, const int32_t* seg_off, const float* kp_L, int N,
                      int P, int H, int W, const float* est_depth, int mode, float* scratch, float* out_kld,
                      uint8_t* out_visible, void* stream);

/* depth_completion/segment_based_completion.py:21-27 render_depth_avg fused with the expansion and the
 * visible-segment filter: per-pixel mean over covering visible segments of exp(L + shift_n)
 * (visible may be NULL = all).  out_depth (H,W), out_invalid (H,W) u8.  acc: 12*H*W bytes of scratch
 * (32.32 fixed-point sums + counts: the accumulation is order-independent, hence reproducible).
 *   - a covering segment counts iff it is visible and its depth d > 1e-6 (a NaN or a vanishing depth is skipped);
 *   - out_depth = sum / (count + 1e-6), the reference's divisor: about 1e-6 below the plain mean for count 1, and 0 / 1e-6 = 0
 *     where nothing counts;
 *   - out_invalid = (count == 0).
 * Two calls, sp_depth_accumulate then sp_depth_average_finish, so that SEGMENT-SHARDED depth completion (BASELINE.json configs[3],
 * SURVEY.md section 8(e)) uses the calls a single GPU uses: every rank accumulates its own segments into acc = {sums[H*W] uint64 (32.32 fixed point), counts[H*W]
 * uint32}, the ranks all_reduce(SUM) the two integer arrays (exact and order independent, so the result is bitwise the
 * single-GPU one; a pixel is invalid iff its summed count is 0, i.e. the OR of the per-rank validity), rank-local finish. */
int sp_depth_accumulate(const uint32_t* pix, const float* baseL, const int32_t* seg_off, const float* kp_L,
                        const float* kld, const uint8_t* visible, int N, int P, int H, int W, void* acc, void* stream);
int sp_depth_average_finish(const void* acc, int H, int W, float* out_depth, uint8_t* out_invalid, void* stream);
/* (ABI 20) retired: sp_depth_average, the wrapper that made the two calls above. */

/* The pose parameter of the reference's drivers, T[b] = Exp(a[b]) * X[b]  (a = [tau, phi] (n,6); X, T (n,4,4)):
 * lietorch's LieGroupParameter.retr().matrix() at odometery/two_frame_sfm.py:83-84, odometery/odometery.py:224-228.
 * grad_T == NULL: forward, writes T.  grad_T != NULL: backward, writes grad_a[b] = (dT/da)^T grad_T[b] (n,6). */
int sp_se3_retract(const float* a, const float* X, int n, float* T, const float* grad_T, float* grad_a, void* stream);

/* lie/lie_algebra.py:41-47 renormalise_se3 on n row-major 4x4 matrices, in place. */
int sp_renormalise_se3(float* T, int n, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Keyframe post-processing: frontend/segment/post_processer.py without cupy.
 * ---------------------------------------------------------------------------------------------------- */

/* post_processer.py:13-36 depth_discontinuity + mask_by_depth_discontinuity: depth = exp(logdepth) (-1 where
 * !valid), filter_size x filter_size max-pool (stride 1, -inf outside the image; filter_size odd, else SP_EINVAL), reflect
 * padding by 1 (index -1 -> 1, n -> n - 2, so H, W >= 2), Scharr/32 gradient magnitude g > threshold.
 * split = valid & !discontinuity (N,H,W) u8; disc (optional) = valid & discontinuity: together they partition valid.
 * scratch: N*H*W floats (the pooled depth).  N <= 65535 (SP_ELIMIT).
 * Pinned: g is a float32 evaluation of the float64 definition and lies within 14 * 2^-24 * max(1, max |pooled| over the
 * pixel's 3x3 window) of it (the count of roundings is derived in tests/post_process_ref.py; measured: 0.12 of that), so
 * the decision equals the float64 one at every pixel whose float64 g is farther than that from the threshold.
 * Non-finite log-depths at valid pixels decide like the reference's max_pool2d + conv2d: the max lets a NaN win (a NaN
 * depth makes every pooled value whose window holds it NaN), and all nine taps of each Scharr filter are multiplied, the
 * zero weights included (0 * inf = NaN); a NaN magnitude is not above the threshold, so such a pixel is no discontinuity
 * and stays in split.  Only a window whose infinite products all carry one sign gives g = inf, a discontinuity.  Values
 * at invalid pixels are never read into the arithmetic. */
int sp_depth_discontinuity(const float* logdepth, const uint8_t* valid, int N, int H, int W, int filter_size,
                           float threshold, float* scratch, uint8_t* split, uint8_t* disc, void* stream);

/* post_processer.py:57-64 connected_components_batch (ndimage.label with the per-slice 4-connectivity structure):
 * labels[i] = 1 + (smallest linear index, over the whole (N,H,W) array, of i's component), 0 for background -- sorting
 * components by label gives scipy's scan-order numbering.  Nothing connects across slices, row ends or slice ends.  The
 * result is exact and the same on every call (the union-find is lock-free, its result is not order-dependent).
 * parent: N*H*W int32 scratch; sizes (optional, N*H*W int32): sizes[root] = pixels of the component, 0 at every other
 * index.  N*H*W <= INT_MAX (SP_ELIMIT). */
int sp_label_components(const uint8_t* fg, int N, int H, int W, int32_t* parent, int32_t* labels, int32_t* sizes,
                        void* stream);

/* Compact list of components {slice, root, size}, one row per root pixel (labels[i] == i + 1), in no particular order,
 * and bg_sizes[n] = |mask_n & !split_n| (the label-0 part post_process_kf forms, post_processer.py:127-133; masks may
 * strictly contain split, and a slice with an empty split is counted like any other).  *n_parts = how many components
 * exist, also when that exceeds cap; then the first cap rows of parts are distinct components, nothing is written
 * behind row cap, and the caller calls again with cap >= *n_parts.  N*H*W <= INT_MAX (SP_ELIMIT). */
int sp_collect_parts(const int32_t* labels, const int32_t* sizes, const uint8_t* masks, const uint8_t* split, int N, int H,
                     int W, int cap, int32_t* parts, int32_t* n_parts, int32_t* bg_sizes, void* stream);

/* Materialise K part masks (K,H,W) u8.  parts[k] = {slice, kind, root}: kind 0 = component `root` of that slice,
 * 1 = mask & !split, 2 = the original mask of the slice (post_processer.py:138-146); kind 0 is ANDed with the mask too, and
 * one root may appear in several parts.  K <= 65535 (SP_ELIMIT). */
int sp_build_part_masks(const uint8_t* masks, const uint8_t* split, const int32_t* labels, int H, int W,
                        const int32_t* parts, int K, uint8_t* out, void* stream);

/* (row, col) of the kth[k]-th set pixel of mask k in raster order, i.e. torch.where(mask)[kth] as used by
 * sample_pts_in_mask (post_processer.py:67-84).  row_off: the row_counts output of sp_mask_count for these masks.
 * 0 <= kth[k] < count of mask k; empty rows in front of, inside and behind the mask are passed over. */
int sp_kth_mask_pixel(const uint8_t* masks, const int32_t* row_off, int K, int H, int W, const int32_t* kth,
                      int32_t* out_rc, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Normal integration (the stage in front of N2): frontend/normals/normals_integration.py:7-28
 * run_tiled_normal_integration as frontend/process_frame.py:78-92 calls it -- per-segment log-depth, right up to one
 * constant per connected component, from surface normals.  The reference's solver is an un-vendored cupy submodule, so
 * the arithmetic is the definition in DESIGN.md §4: with ax = nx (c - cx) + ny (r - cy) fx / fy + nz fx and
 * ay = nx (c - cx) fy / fx + ny (r - cy) + nz fy, every pair of horizontally (vertically) adjacent mask pixels p, q is an
 * edge of weight w = (a_p^2 + a_q^2) / 2 with t = -(a_p n_p + a_q n_q) / 2 (a, n = ax, nx or ay, ny); (L u)_p = sum_e
 * w_e (u_p - u_other), b_q += t, b_p -= t; plain conjugate gradients on L u = b from u = 0, stopped PER SEGMENT once the
 * recursively updated residual has |r_k| <= cg_tol |b|, or after cg_max_iter iterations (|b| = 0: no iteration).
 *
 *   normals (H,W,3) float, camera frame x right / y down / z forward (the sign of a normal does not matter);
 *   K row-major 3x3 (device); masks (N,H,W) u8; boxes_or_null (N,4) int32 {row0, col0, row1, col1} half open, a HINT
 *   (KeyFrame.segment_boxes): no mask pixel lies outside it.  It only narrows the scan -- the solve always works on the
 *   tight box, so results are bitwise the same with and without it, and a segment's result does not depend on the
 *   other segments of the call.  flags: 0 (reserved).
 *   depth (N,H,W) float: exp(u) on the mask (u clamped to +-15, so every mask pixel passes process_frame.py:234's
 *   `> 1e-7`), 0 elsewhere -- every element is written.  info (N,2) float: {iterations used, final recursive |r| / |b|};
 *   iterations = -1 marks a segment whose vectors did not fit the scratch (its depth is 0).
 *   scratch: scratch_floats floats = sp_normal_integration_plan_words(N) + the vector area.  The vector area is at most
 *   N * sp_normal_integration_segment_floats(H, W); the exact need (6 vectors over every segment's padded tight box) is
 *   what sp_normal_integration_plan leaves in plan[0..1] as one int64 (plan: sp_normal_integration_plan_words(N) int32).
 * One workgroup solves one segment (largest first); nothing synchronises the host.
 * ---------------------------------------------------------------------------------------------------- */
int sp_normal_integration_plan_words(int N);
int sp_normal_integration_segment_floats(int H, int W);
int sp_normal_integration_plan(const uint8_t* masks, const int32_t* boxes_or_null, int N, int H, int W, int32_t* plan, void* stream);
int sp_normal_integration(const float* normals, const float* K, const uint8_t* masks, const int32_t* boxes_or_null, int N, int H,
                          int W, int cg_max_iter, float cg_tol, int flags, float* scratch, long long scratch_floats, float* depth,
                          float* info, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Depth completion, the stage after sp_depth_average (BASELINE config 4): depth_completion/fill_in_tools.py:5-7 fill_depth and
 * depth_completion/void.py:7-65 ErrorMetrics / ErrorMetricsDeltas, as the evaluation loop evaluate_void.py:122-146 uses them.
 *
 * sp_depth_fill_nearest: depth (B,H,W) float, invalid (B,H,W) u8 (non-zero = to be filled).  Every invalid pixel (r, c) takes the
 * value of the valid pixel (r', c') of the same image that minimises ((r - r')^2 + (c - c')^2, c', r') lexicographically -- the pixel
 * scipy.ndimage.distance_transform_edt(invalid, return_indices=True) names, ties included; valid pixels keep theirs.  Distances are
 * uint32 squared distances, never floats.  filled (B,H,W) float (not depth itself), index_or_null (B,H,W) int32 = r' W + c',
 * counts (B,2) int32 = {valid pixels, pixels filled}.  An image with no valid pixel is copied through ({0, 0}, index = identity;
 * scipy indexes row -1 there).  workspace: sp_depth_fill_workspace_bytes(B, H, W) bytes.  H, W <= 32767, B <= 65535,
 * B H W < 2^30, else SP_ELIMIT.
 *
 * sp_depth_metrics: estimate, target (B,H,W) float, valid (B,H,W) u8.  out (B,12) double per image, over its valid pixels:
 * {n, rmse, mae, absrel (1000 x the inputs: mm), inv_rmse, inv_mae, inv_absrel (of 1 / (0.001 x the inputs): 1/km), fractions of
 * max(t / e, e / t) below 1.05, 1.10, 1.25, 1.25^2, 1.25^3}.  Per-pixel terms are fp32 with every operation rounded on its own, as
 * numpy forms them; sums are fp64 in a fixed order (two runs agree bitwise); pixels outside valid are never read into a sum
 * (their target may be inf); n = 0 gives NaN.  workspace: sp_depth_metrics_workspace_doubles(B, H, W) doubles.
 * Null pointers and non-positive sizes are SP_EINVAL before any device work.
 * ---------------------------------------------------------------------------------------------------- */
int sp_depth_fill_workspace_bytes(int B, int H, int W);
int sp_depth_fill_nearest(const float* depth, const uint8_t* invalid, int B, int H, int W, void* workspace, float* filled,
                          int32_t* index_or_null, int32_t* counts, void* stream);
int sp_depth_metrics_workspace_doubles(int B, int H, int W);
int sp_depth_metrics(const float* estimate, const float* target, const uint8_t* valid, int B, int H, int W, double* workspace,
                     double* out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * From SAM's raw output to the masks of a keyframe: the tensor code of frontend/segment/mask_generation.py behind the network.
 * Everything runs on the caller's stream without a synchronisation.  Null or aliased pointers and non-positive sizes are SP_EINVAL,
 * sizes beyond the stated limits SP_ELIMIT, both before any device work.  H W < 2^31 and W <= 32767 throughout (the reference's
 * int16 row sums).
 *
 * sp_sam_candidate_stats: logits (M,H,W) float (M = 3 n candidates, M <= 65535), read once.  stats (M,8) int32 per candidate:
 * {#(x > thresh + offset), #(x > thresh - offset), #(x > thresh), left, top, right, bottom, 0} -- the two counts of
 * calculate_stability_score (mask_generation.py:54-56; strict comparisons, NaN false), the size of :71 and the XYXY box of
 * batched_mask_to_box (:93) over x > thresh, zeros for an empty mask.  Integer atomics: bitwise stable.
 *
 * sp_box_nms: batched_nms with one category (mask_generation.py:183-188, :217-222).  boxes (K,4) float XYXY, scores (K) float.
 * Visits in falling score (equal scores: the lower index first; NaN first, as torch.sort), suppresses j when
 * inter / (area_i + area_j - inter) > thr in float32 with area = (x2 - x1)(y2 - y1) and inter = max(x2' - x1', 0) max(y2' - y1', 0)
 * (NaN: false).  keep (K) int64: the kept indices in visiting order, n_keep (1) int32 their number.  K <= 2048.
 *
 * sp_sam_build_masks: masks (K,H,W) u8 0/1 with masks[k] = logits[cand[k]] > thresh (mask_generation.py:67,76), cand (K) int32 in
 * [0, M) (anything else gives an empty mask); coverage_or_null (H,W) u8 = their OR (:192).
 *
 * sp_mask_edges: masks_to_edges / infer_edge_probs (mask_generation.py:291-313) of K masks (K,H,W) u8, optionally seen through a
 * nearest resize to (He,We) (:240-244): row_map (He) / col_map (We) int32 name the source row / column of every coarse one (null: the
 * identity, He = H / We = W).  Scharr / 32 with reflect padding at the coarse border, magnitude, maximum over the masks, with pool a
 * 3x3 maximum on top; edges, edge_probs (He,We) float, edge_probs = clip(1 - 2 edges, 0, 1).  Bitwise the reference's floats.
 * 2 <= He, We <= 32767.
 *
 * sp_sam_cut_masks: cut_masks_by_edges and filter_edge_points (mask_generation.py:254-275).  valid = edge_probs > prob_thresh
 * (null: everywhere); kp_rc_or_null (K,2) int32 (row, col) of every mask's keypoint: mask k is kept when masks[k] & valid is set
 * there (null: every mask is kept; a keypoint outside the image drops its mask).  keep (K) int32: the position of mask k among
 * the kept ones or -1; out_masks_or_null (K,H,W) u8: the kept masks & valid, compacted in order (the rows behind them are not
 * written; null: only keep and the coverage are wanted); final_coverage (H,W) u8 their OR.
 * ---------------------------------------------------------------------------------------------------- */
int sp_sam_candidate_stats(const float* logits, int M, int H, int W, float thresh, float offset, int32_t* stats, void* stream);
int sp_box_nms(const float* boxes, const float* scores, int K, float thr, int64_t* keep, int32_t* n_keep, void* stream);
int sp_sam_build_masks(const float* logits, const int32_t* cand, int K, int M, int H, int W, float thresh, uint8_t* masks,
                       uint8_t* coverage_or_null, void* stream);
int sp_mask_edges(const uint8_t* masks, int K, int H, int W, const int32_t* row_map_or_null, const int32_t* col_map_or_null, int He, int We,
                  float* edges, float* edge_probs, int pool, void* stream);
int sp_sam_cut_masks(const uint8_t* masks, int K, int H, int W, const float* edge_probs_or_null, float prob_thresh, const int32_t* kp_rc_or_null,
                     int32_t* keep, uint8_t* out_masks_or_null, uint8_t* final_coverage, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Frame ingest: raw camera frames already on the device -> KeyFrame-ready images and depth maps, one launch per batch of frames
 * (additive, ABI 18).  The reference does this on the host for EVERY tracked frame (frontend/process_frame.py:257-270
 * process_to_supp_kf; :207-255 process_to_kf for keyframes): cv2.undistort(image, K, d) on the 8-bit BGR frame
 * (data/tum_undistort.py:113; the general form is data/image_transforms.py:36-60 initUndistortRectifyMap + remap), the margin
 * crop [mh:-mh, mw:-mw] and BGR -> RGB (data/tum_undistort.py:86-90,127-130), tool/etc.py image_tt (uint8 / 255 -> float CHW), and
 * frontend/process_frame.py:170-189 _downsample_to_target (bilinear F.interpolate; intrinsics by tool/camera.py:13-22).
 *
 * sp_frame_ingest: raw (B,H,W,3) u8 -> out (B,3,Ho,Wo) float.  With (u, v) a pixel of the full frame,
 *   x = (u - cx) / fx, y = (v - cy) / fy, r2 = x^2 + y^2, kr = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
 *   mx = fx (x kr + 2 p1 x y + p2 (r2 + 2 x^2)) + cx,   my = fy (y kr + p1 (r2 + 2 y^2) + 2 p2 x y) + cy
 * (OpenCV's initUndistortRectifyMap with R = I and newCameraMatrix = K, which is what cv2.undistort uses), U(v, u, c) is the bilinear
 * sample of raw at (mx, my) -- taps floor and floor + 1, a tap outside the frame contributes 0 (BORDER_CONSTANT 0; grid_sample's
 * 'zeros') --, C(i, j) = U(i + top, j + left) for 0 <= i < Hc, 0 <= j < Wc, and out is F.interpolate(C, size=(Ho,Wo), mode='bilinear',
 * align_corners=False): per axis s = max((a + 0.5) Hc / Ho - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, Hc - 1), weight s - i0.
 * (Ho,Wo) == (Hc,Wc) is the identity.  Map and weights are float64; the value is the weighted sum of the integer taps, rounded to float
 * once and DIVIDED by 255.0f, so zero distortion without crop or resize is image_tt bit for bit.  bgr != 0 reverses the channels.
 * cv2.undistort itself returns uint8 from fixed-point coordinates; this keeps the float value (DESIGN.md §4 "Frame ingest").
 *
 * sp_depth_ingest: raw (B,H,W) u16 -> out (B,Ho,Wo) float: d = (float)v * scale in float32 and d > max_depth -> 0
 * (data/tum_undistort.py:16-36 DepthScale, DepthFilter), the same crop (:128), then torch's nearest rule
 * src = min((int)floorf(dst * ((float)in / out)), in - 1) per axis (odometery/odometery.py:152-156); (Ho,Wo) == (Hc,Wc): no resize.
 *
 * cam is read on the host.  A null pointer, out aliasing raw, a non-positive size or a crop that leaves the frame is SP_EINVAL;
 * W > 32767, H W >= 2^31, B > 65535, Ho > 65535, or fx / fy not finite or <= 0 is SP_ELIMIT; both before any device work.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct SpCamera {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;   /* OpenCV's order; absent coefficients are 0 */
} SpCamera;
SP_ABI_SIZE(SpCamera, 96)
int sp_frame_ingest(const uint8_t* raw, int B, int H, int W, const SpCamera* cam, int top, int left, int Hc, int Wc, int Ho, int Wo,
                    int bgr, float* out, void* stream);
int sp_depth_ingest(const uint16_t* raw, int B, int H, int W, float scale, float max_depth, int top, int left, int Hc, int Wc, int Ho,
                    int Wo, float* out, void* stream);

/* odometery/kf_criteria.py:7-21 translation_difference, :23-34 rotation_difference and the depth-validity ratio of
 * odometery/odometery.py:1003-1004, without a host sync.  depth: n floats (the rendered depth of the
 * latest keyframe); poses row-major 4x4.  out[4] = {#(depth > thresh)/n, scale = lower median of the valid depths
 * (torch.median; NaN when none is valid), |t_src - t_trg| / (scale + 1e-6), rotation angle of
 * inv(pose_src) pose_trg in degrees}, from a grid of workgroups (one launch per radix pass; 17 us on a 640 x 480 render):
 * ws = sp_kf_criterion_ws_words() uint32 of scratch, any content. */
/* (ABI 20) retired: sp_kf_criterion, the one-workgroup form (102 us on that render). */
int sp_kf_criterion_ws_words(void);
int sp_kf_criterion_ws(const float* depth, int n, float thresh, const float* pose_src, const float* pose_trg, uint32_t* ws, float* out,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------
 * ONE CALL PER FRAME INDEX of the monocular-odometry chain, for S sequences in lockstep (ABI 14; lockstep ABI 16; one path ABI 17; BASELINE
 * configs[2] as a sequence).  The reference's driver loop (odometery/odometery.py:1018-1075) does, for every frame that is not a keyframe:
 * track_frame against the latest keyframe (:323-449), mapping(mode='supp') -- the latest keyframe's depths against its two running
 * supporting frames (:1038-1042) -- and is_kf (:986-1016: the keyframe's depth rendered in the tracked pose, validity ratio / scaled
 * translation).  Behind Gauss-Newton windows that are built once per keyframe (sp_window_gn_run) the interpreter between those steps -- three
 * dozen small tensor operations, node arrays read back and re-uploaded, a host synchronisation per step -- costs more than the kernels.
 * sp_chain_step_multi (below) runs a frame's stages with ALL state on the device; its argument record, one SpChainStep per sequence:
 * ---------------------------------------------------------------------------------------------------- */
#define SP_CHAIN_LEVELS 4
#define SP_CHAIN_PHASES 6
#define SP_CHAIN_TRACK 1
#define SP_CHAIN_SUPP 2
#define SP_CHAIN_CRITERION 4
typedef struct SpChainPhase {
    int32_t level;                     /* pyramid level (index into SpChainWindow.gn) */
    int32_t max_iters;
    float irls_eps, conv_tol;
} SpChainPhase;
SP_ABI_SIZE(SpChainPhase, 16)
typedef struct SpChainWindow {         /* a built window with its Gauss-Newton schedule */
    SpWindowGn gn[SP_CHAIN_LEVELS];    /* the window at pyramid level l (pairs == NULL: the window has no descriptors there) */
    SpChainPhase phase[SP_CHAIN_PHASES];
    int32_t n_phases;
    int32_t check_every;               /* sp_window_gn_run's */
    int32_t flags;                     /* sp_window_gn_step's (SP_WGN_PREDICTED_EXIT, SP_WGN_DEPTHS_FIXED) */
    float lam0;                        /* LM damping every frame starts from */
    float lm_up, lm_down, lm_min;
    int32_t check_first;               /* > 0: every phase looks at the state after this many iterations for the first time (a window that
                                        * usually converges at once -- the supplementary mapping -- should not run check_every iterations blind) */
    float* state_host;                 /* host: 16 floats, filled by the call */
} SpChainWindow;
SP_ABI_SIZE(SpChainWindow, 680)
typedef struct SpChainTarget {         /* a target node whose frame the step replaces */
    float* packed[SP_CHAIN_LEVELS];    /* the node's packed (H_l, W_l, 3) image at pyramid level l, where the window has that level */
    const float* pose;                 /* 16 floats: the node's new camera-to-world pose */
    const float* aff;                  /* 2 floats, or NULL (no affine compensation) */
    int32_t node;
    int32_t pad_;
} SpChainTarget;
SP_ABI_SIZE(SpChainTarget, 56)
typedef struct SpChainStep {
    int32_t stages;
    int32_t H, W, n_levels;            /* the frame; pyramid levels to build (level 0 = the image itself) */
    const float* image;                /* planar (3,H,W) */
    float* level[SP_CHAIN_LEVELS];     /* planar scratch of levels 1 .. n_levels - 1 ([0] unused) */
    SpChainWindow track;
    SpChainTarget track_target;
    float* out_pose;                   /* 16 floats */
    float* out_aff;                    /* 2 floats or NULL */
    SpChainWindow supp;
    SpChainTarget supp_target[2];      /* the latest keyframe's two running supporting frames, older first */
    int32_t supp_images;               /* bit 0: slot 1 -> slot 0; bit 1: this frame -> slot 1 */
    int32_t kld_n;
    const float* kld_src;
    float* kld_dst;
    /* the keyframe the criterion renders (sp_depth_splat's arguments) */
    const uint32_t* pix; const float* baseL; const int32_t* seg_off; const float* kp_L; const float* kld;
    const float* K; const float* kf_pose;
    int32_t N, P;
    unsigned long long* keys; float* depth_out;
    float* rel_pose;                   /* 16 floats scratch */
    float* crit;                       /* 4 floats */
    uint32_t* crit_ws;                 /* sp_kf_criterion_ws_words() uint32 of scratch */
    float* crit_host;                  /* host: 4 floats, filled by the call */
    float valid_thresh;
    int32_t track_iters, supp_iters;   /* out (host) */
    int32_t pad_;
} SpChainStep;
SP_ABI_SIZE(SpChainStep, 1752)

/* ----------------------------------------------------------------------------------------------------
 * sp_chain_step_multi: the stages named in `stages` for n_steps records at once, one record per sequence (n_steps = 1: one sequence), with
 * ALL state on the device -- poses, affine pairs and depths are read from and written to device buffers the records name -- and the only
 * values that reach the host are the windows' 16-float LM states (the phase loop's polls and the final states) and the 4 criterion floats.
 *   SP_CHAIN_TRACK     : pyramid of `image` packed into the tracker's target buffers (sp_blur_decimate / sp_pack_rgb's arithmetic); the
 *                        target node's pose / affine pair <- track_target.pose / .aff, tangents and moments cleared, edges recomposed; fresh
 *                        LM state; the phases of `track`; out_pose <- renormalise_se3(the node's pose) (lie/lie_algebra.py:41-47), out_aff
 *                        <- its pair
 *   SP_CHAIN_SUPP      : (supp_images bit 0) the packed levels of supp_target[1] move to supp_target[0]; (bit 1) the tracker's packed levels
 *                        are copied into supp_target[1]; both nodes <- their pose / aff; fresh LM state; the phases of `supp`; then
 *                        kld_n floats kld_src -> kld_dst (the mapped depths into the tracker's block)
 *   SP_CHAIN_CRITERION : rel <- inv(out_pose) kf_pose; sp_depth_splat of the keyframe under rel into depth_out; sp_kf_criterion_ws(depth_out,
 *                        out_pose, kf_pose) -> crit (device)
 * Stages run in that order on `stream`.  Every stage covers all records with the same launches -- the frames' pyramids one launch per
 * level, node overwrites / edge composition / LM resets one launch each, the phase loop the round body of sp_window_gn_run_multi (cost pass
 * over all work lists, per-edge reduce, Schur terms, update: window = blockIdx.z), the criterion's splat and select passes with the record on
 * blockIdx.y -- so the launches per call do not grow with n_steps.  The polls are those of sp_window_gn_run with the ones that decide nothing
 * left out: the first after check_first iterations when conv_tol > 0, then every check_every, none after a phase's last iteration; a phase
 * ends once EVERY window froze (st[6]) or at its max_iters.  A frozen window is inert, so per record the result is BITWISE that of the call
 * on that record alone: out_pose, out_aff, the supp window's log-depths and nodes, kld_dst, crit_host, track_iters, supp_iters, and the
 * 16-float states left in each window's state_host.
 * The call is HOMOGENEOUS: every record has the same stages, H, W, n_levels, valid_thresh, and per present stage the same phase list
 * (level, max_iters, irls_eps, conv_tol), check_every, check_first, flags and LM constants (lam0, lm_up, lm_down, lm_min); otherwise
 * -- or for n_steps outside 1 .. 65535 or a null pointer -- SP_EINVAL before anything is launched.
 *   args_dev    : device scratch of n_steps * sp_chain_multi_bytes() bytes (the argument records, one host-to-device copy per call)
 *   states_dev  : device scratch of 36 * n_steps floats, what the device gathers the results into; states_host: pinned host memory of the
 *                 same size that they are copied to -- [16 n] the tracker windows' states, [16 n] the supp windows', [4 n] the criteria
 *                 (one device-to-host copy and one synchronisation of `stream` at the end, plus the phase loop's polls)
 * The records stay in HOST memory.  After the call's one synchronisation the host fills each record's track.state_host / supp.state_host
 * (16 floats each), crit_host (4 floats) and track_iters / supp_iters from states_host.  Returns 0, SP_EINVAL / SP_ELIMIT (before anything
 * is launched), a hipError_t of a failed launch or copy, or the -(1000 + hipError_t) of a phase round (as sp_window_gn_run_multi). */
int sp_chain_multi_bytes(void);
int sp_chain_step_multi(SpChainStep* steps, int n_steps, void* args_dev, float* states_dev, float* states_host, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Sequence results (sp_results.hip): the similarity alignment of trajectories and the world map of keyframes.
 *
 * sp_traj_align: S trajectories in ONE launch, one workgroup each -- what tool/pose_utils.py `align` (:71-133) and `transfer_scale`
 * (:16-48) compute for the translations of pred (the model) against those of gt (the data), accumulated and decomposed in float64:
 *   zero-centred cross-covariance W = sum mz dz^T; rot = U S Vh of svd(W^T) with S = diag(1, 1, -1) when det(U) det(Vh) < 0 (one-sided
 *   Jacobi; the third left vector is taken as u1 x u2, so a rank-2 W -- an exactly planar trajectory -- has its unique answer);
 *   s = dots / norms; trans_scaled = mean(d) - s rot mean(m); trans = mean(d) - rot mean(m); the per-pose errors |s rot m + trans_scaled - d|
 *   and |rot m + trans - d| with their root mean squares (the absolute trajectory error with and without scale); with anchor_rotation
 *   rot_reanchor = R_gt[0] R_pred[0]^T, else the identity.
 *     pred, gt    : (S, n_max, 4, 4) float32, camera-to-world; rows at and beyond lengths[s] are never read
 *     lengths     : (S,) int32 on the device, each 3 .. n_max (the CALLER checks: the entry point sees a device pointer; the kernel
 *                   clamps to 0 .. n_max)
 *     out         : S records
 *     err_scaled, err : (S, n_max) float64 per-pose errors; entries at and beyond lengths[s] are written as 0
 * S in 1 .. 65535, n_max >= 3 (SP_EINVAL), S * n_max * 16 <= INT_MAX (SP_ELIMIT). */
typedef struct SpTrajAlign {
    double rot[9];                     /* row major */
    double trans_scaled[3];
    double trans[3];
    double s;
    double rot_reanchor[9];            /* row major; the identity without anchor_rotation */
    double ate_scaled, ate;            /* root mean square of the per-pose errors with / without scale */
    double dots, norms;                /* s = dots / norms */
    double sigma[3];                   /* singular values of W, descending */
} SpTrajAlign;
SP_ABI_SIZE(SpTrajAlign, 256)
int sp_traj_align(const float* pred, const float* gt, const int32_t* lengths, int S, int n_max, int anchor_rotation, SpTrajAlign* out,
                  double* err_scaled, double* err, void* stream);

/* sp_map_points: the coloured world points of n_kf keyframes in ONE launch (gui/odometery_gui.py:569-575,665-686 get_dense_pcd per window
 * keyframe).  Keyframe k contributes Q_k = ceil(P_k / stride) rows from out_offset on: row o is table point o * stride (table order is the
 * reference's nonzero order, so this is src_pts[::stride]), its camera-frame point p by sp_photo_stats' arithmetic (decode_pix,
 * exp(baseL + (kld[n] - kp_L[n])), backproject).  Without an alignment record the world point is R p + t in float32 fma; with record a it is
 * R' (s p) + t' with R' = a.rot_reanchor R and t' = a.s a.rot t + a.trans_scaled (apply_scale, tool/pose_utils.py:50-68), R' and t'
 * formed in float64 and rounded once.  The colour is image[:, row, col] (a load, no interpolation).  Nothing is filtered.
 *     kfs       : n_kf records on the device; out_offset and first_block are the prefix sums of Q_k and of ceil(Q_k / 256) (the caller's
 *                 host arithmetic: no device value is needed to size the call)
 *     total_blocks, total_rows : the two sums; rows at or beyond total_rows are never written
 *     align     : n_align records on the device, or NULL with n_align 0
 *     points, colours : (total_rows, 3) float32; kf_index, seg_ids : (total_rows,) int32
 * n_kf in 1 .. 65535, stride >= 1, total_blocks >= 1, total_rows in 1 .. 256 * total_blocks (SP_EINVAL). */
typedef struct SpMapKeyframe {
    const uint32_t* pix; const float* baseL; const int32_t* seg_off; const float* kp_L;   /* the keyframe's SegmentTable */
    const float* kld;                  /* N keypoint log-depths */
    const float* image;                /* planar (3, H, W), level 0 */
    const float* K;                    /* 9 floats */
    const float* pose;                 /* 16 floats, camera-to-world */
    int32_t N, P, H, W;
    long long out_offset;              /* first output row */
    int32_t align;                     /* index of an SpTrajAlign record, or -1 */
    int32_t first_block;               /* first workgroup of the launch that works on this keyframe */
} SpMapKeyframe;
SP_ABI_SIZE(SpMapKeyframe, 96)
int sp_map_points(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int stride, const SpTrajAlign* align, int n_align, float* points,
                  float* colours, int32_t* kf_index, int32_t* seg_ids, long long total_rows, void* stream);

/* sp_map_normals (sp_surfel.hip): the surface normal of every row of sp_map_points, in ONE launch, from the keyframes' own tables.  The
 * records, the walk and the argument rules are sp_map_points': the caller passes the very records it built for that call, and row j of
 * normals belongs to row j of points.  image, kld and kp_L are not read: a constant added to log-depth scales the surface about the
 * camera centre, so the normal does not depend on the keypoint log-depth shift.
 *     normals : (total_rows, 3) float32, unit length in the world, facing the keyframe's camera; (0, 0, 0) means "no normal"
 * PRECONDITION on the tables: within a segment's table range seg_off[n] .. (n + 1 < N ? seg_off[n + 1] : P) the words pix & 0x7fffffff
 * (row << 16 | col) are strictly increasing -- row-major order, the reference's nonzero order, what sp_table_fill writes.
 * All arithmetic in float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal), rounded to float32 once.
 *   - Table point i = row * stride lies on pixel (r, c) of pix[i], in segment n; L(k) = float64(baseL[k]).
 *   - Neighbours are looked up at stride 1 in segment n's range only: left / right are i - 1 / i + 1 if inside the range and on
 *     (r, c - 1) / (r, c + 1); up / down are the table points of the range on (r - 1, c) / (r + 1, c) (a binary search each).
 *   - Lu = (L(right) - L(left)) / 2 with both, L(right) - L(i) or L(i) - L(left) with one, 0 with none; Lv likewise from down and up.
 *   - m = (-(fx Lu), -(fy Lv), (1 + (c - cx) Lu) + (r - cy) Lv): fx fy / d^2 times dp/du x dp/dv of p = d ((c - cx) / fx, (r - cy) / fy, 1),
 *     d = exp(L + shift).  n_cam = -m / sqrt((m0 m0 + m1 m1) + m2 m2); m . ray = 1, so n_cam faces the camera.  If a component of m is
 *     not finite the row is (0, 0, 0).
 *   - n_w = R' n_cam, each row as (R'0 n0 + R'1 n1) + R'2 n2; R' is the pose's rotation, or with alignment record a the float64 product
 *     a.rot_reanchor R, each entry as (a0 R0 + a1 R1) + a2 R2, never rounded to float32.  The scale does not enter.
 * No atomics; two runs give the same bits.  Null kfs / normals, and sp_map_points' conditions on n_kf, stride, total_blocks, align /
 * n_align and total_rows: SP_EINVAL. */
int sp_map_normals(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int stride, const SpTrajAlign* align, int n_align, float* normals,
                   long long total_rows, void* stream);

/* sp_keyframe_depths: what each of n_kf keyframes of ONE size claims to see -- its own depth image and segment map, straight from its
 * table (the renderer cannot deliver them: x fx / z + cx does not give back the integer column exactly, and the truncation can land one
 * pixel to the left).
 *     kfs   : the records of an sp_map_points call with stride 1 (first_block = the prefix sum of ceil(P_k / 256), total_blocks their
 *             sum); image, pose, align and out_offset are not read.  Every record must carry the call's H and W (the caller's check:
 *             the records live on the device); a point whose pixel lies outside H x W is skipped, never written
 *     keys  : n_kf H W uint64 of scratch, zeroed by the call
 *     depth : (n_kf,H,W) float32;  seg : (n_kf,H,W) int32, may be NULL
 * Table point i of keyframe k lies on the pixel (row, col) of decode_pix(pix[i]) (col = bits 0..15, row = bits 16..30) and has the
 * float32 depth z = exp(baseL[i] + (kld[n] - kp_L[n])), n its segment -- sp_map_points' own depth, bit for bit (one device function).
 * A point whose z is not a finite float > 0 (NaN, underflow to 0, overflow to inf) is skipped.  The smallest z wins the pixel, equal z
 * goes to the HIGHEST table index (sp_render_views mode 1's key: ~bits(z) << 32 | (i + 1)).  depth = the winner's z, or exactly 0 where
 * no point lies; seg = the winner's segment, or -1.  Integer atomic maxima: two runs give the same bits.
 * Null kfs / keys / depth, n_kf outside 1 .. 65535, total_blocks < 1, H or W <= 0: SP_EINVAL.  n_kf H W >= 2^31: SP_ELIMIT. */
int sp_keyframe_depths(const SpMapKeyframe* kfs, int n_kf, int total_blocks, int H, int W, unsigned long long* keys, float* depth,
                       int32_t* seg, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map views (sp_views.hip): a point set rendered into camera views, and depth images lifted into a point cloud.  Both run on the
 * caller's stream without a synchronisation; argument checks come before any device work.
 *
 * sp_render_views: V views of one point set in ONE call (tool/viz.py:180-190 render_pcd is mode 0 with one identity-pose view).
 *     points   : (Q,3) float32;  colours : (Q,3) float32 (may be NULL when image is)
 *     views    : V records on the device, pose camera-to-world (row major 4x4; the last row is not read)
 *     keys     : V H W uint64 of scratch, zeroed by the call
 *     image    : (V,H,W,3) uint8;  depth : (V,H,W) float32;  index : (V,H,W) int32 -- each may be NULL
 * In float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal):  d = p - t,
 * p_c = ((R0r d0 + R1r d1) + R2r d2) for r = x, y, z (R^T d; a pose that is exactly the identity leaves p_c = p untouched, as render_pcd
 * does), u = x fx / z + cx, v = y fy / z + cy.  A point is kept iff 0 <= u < W and 0 <= v < H (NaN and +-inf fail); its pixel is
 * (trunc v, trunc u).
 *     mode 0 : no test on z (points behind the camera are kept, as the reference keeps them); the kept point with the HIGHEST index
 *              wins the pixel (NumPy's repeated-index assignment)
 *     mode 1 : additionally z > z_min; the kept point with the smallest float32(z) wins, equal float32(z) goes to the highest index
 * index = the winner (or -1); depth = float32(z) of the winner (or exactly 0); image = trunc(colour * 255) per channel from the exact
 * float64 product, clamped to 0 .. 255 (the reference's astype(uint8) wraps), NaN gives 0; an untouched pixel is 0, 0, 0.  Integer
 * atomic maxima: two runs give the same bits.
 * Null points / views / keys (or colours with an image), Q, V, H or W <= 0, mode outside {0, 1}, z_min negative or NaN: SP_EINVAL.
 * Q > 2^31 - 2, V > 65535, V H W >= 2^31: SP_ELIMIT. */
typedef struct SpView {
    float K[9];                        /* row major; fx = K[0], fy = K[4], cx = K[2], cy = K[5] */
    float pose[16];                    /* camera-to-world */
} SpView;
SP_ABI_SIZE(SpView, 100)
int sp_render_views(const float* points, const float* colours, long long Q, const SpView* views, int V, int H, int W, int mode, float z_min,
                    unsigned long long* keys, uint8_t* image, float* depth, int32_t* index, void* stream);

/* sp_render_splats: sp_render_views' depth buffer (mode 1) with a FOOTPRINT per point, so that a map sparser than the view leaves no
 * holes and a near surface hides a far one.  The arguments of sp_render_views without `mode`, plus
 *     radii  : (Q,) float32, the half side of the point's square footprint in world units
 *     max_px : the largest half-width in pixels, 0 .. 16
 * Per (point, view) u, v, z exactly as sp_render_views forms them; then, in float64, ru = (r fx) / z and rv = (r fy) / z.  A half-width
 * that is not >= 0 (a negative or NaN radius, inf / inf) becomes 0; otherwise it is min(., max_px), so an infinite radius gives max_px.
 * The point is kept iff u and v are finite, z > z_min, and the square [u - ru, u + ru] x [v - rv, v + rv] touches the image:
 * u + ru >= 0, u - ru < W, v + rv >= 0, v - rv < H.  It covers the columns max(floor(u - ru), 0) .. min(floor(u + ru), W - 1) and the
 * rows likewise (clamped in float64, then converted): at most 33 x 33 pixels.  A pixel is covered when its cell [c, c + 1) meets the
 * square, NOT when its centre lies inside: a footprint of exactly one source pixel (ru = 0.5) therefore usually covers 2 x 2 pixels
 * (floor(u + 0.5) = floor(u - 0.5) + 1 wherever the two sums are exact), and one of half a pixel 1 or 2 per axis.
 * Every covered pixel is contested with mode 1's key: the smallest float32(z) wins, equal float32(z) goes to the highest index; the
 * depth written is the point's float32(z) on all of its pixels (a splat is flat, fronto-parallel).  With radius 0 the range is the one
 * pixel (trunc v, trunc u) and the call is sp_render_views in mode 1, bit for bit.  Outputs as there; integer maxima: two runs give the
 * same bits.
 * Null points / views / keys / radii (or colours with an image), Q, V, H or W <= 0, z_min negative or NaN, max_px outside 0 .. 16:
 * SP_EINVAL.  Q > 2^31 - 2, V > 65535, V H W >= 2^31: SP_ELIMIT. */
int sp_render_splats(const float* points, const float* colours, long long Q, const SpView* views, int V, int H, int W, float z_min,
                     const float* radii, int max_px, unsigned long long* keys, uint8_t* image, float* depth, int32_t* index, void* stream);

/* sp_render_surfels (sp_views.hip): sp_render_splats' depth buffer with an ORIENTED footprint per point: the depth of every covered
 * pixel is taken on the point's tangent plane, so a slanted surface renders at its true depth.  The arguments, limits and error codes of
 * sp_render_splats, plus
 *     normals : (Q,3) float32 in the frame of the points (sp_map_normals'), required
 *     cull    : 0 (two-sided) or 1 (a surfel seen from behind is dropped)
 * Per (point, view) x, y, z (= p_c), u, v, ru, rv, the keep test and the clipped rectangle r0 .. r1 x c0 .. c1 exactly as sp_render_splats
 * has them (the same device functions: coverage is identical).  Then, in float64, every operation rounded on its own:
 *   - A normal is USABLE iff its three floats are finite and not all zero.  An unusable normal makes the point sp_render_splats' flat
 *     splat: the key of float32(z) on every pixel of the rectangle, nothing more is tested.
 *   - n_c = R^T n, each row as (a + b) + c (an exact identity pose leaves n_c = n, as it leaves p_c = p);  s = (n_c0 x + n_c1 y) + n_c2 z.
 *   - cull = 1: a usable normal with s >= 0 drops the (point, view).  t below does not change with the sign of n.
 *   - Pixel (r, c) of the rectangle: a = ((c + 0.5) - cx) / fx, b = ((r + 0.5) - cy) / fy -- the ray through the pixel's centre (the
 *     renderer truncates: pixel c is [c, c + 1)) --, den = (n_c0 a + n_c1 b) + n_c2, t = s / den; a NaN t becomes z; then if t < z - h,
 *     t = z - h, and if t > z + h, t = z + h, with h = 2 rad, rad = float64(radius) if that is >= 0, else 0 (a disc that reaches the
 *     square's corners has radius sqrt(2) rad and cannot leave that depth range however it is tilted; a grazing plane cannot shoot a
 *     pixel to infinity).  The pixel is contested iff t > z_min and t < inf, with mode 1's key of float32(t): the smallest float32(t)
 *     wins, equal float32(t) goes to the highest index.
 * keys are zeroed by the call; outputs as sp_render_splats (depth = the winner's float32(t)).  Consequences:
 *   - all normals zero (or otherwise unusable): sp_render_splats, bit for bit on every pixel;
 *   - all radii 0 (h = 0, t = z, the one pixel (trunc v, trunc u)): sp_render_views in mode 1, bit for bit on every pixel, for points
 *     of finite z (a point at z = inf with a usable normal fails t < inf; the two other calls keep it).
 * Integer atomic maxima: two runs give the same bits.
 * Null points / views / keys / radii / normals (or colours with an image), Q, V, H or W <= 0, z_min negative or NaN, max_px outside
 * 0 .. 16, cull outside {0, 1}: SP_EINVAL.  Q > 2^31 - 2, V > 65535, V H W >= 2^31: SP_ELIMIT.  Invalid beats too large. */
int sp_render_surfels(const float* points, const float* colours, const float* normals, long long Q, const SpView* views, int V, int H, int W,
                      float z_min, const float* radii, int max_px, int cull, unsigned long long* keys, uint8_t* image, float* depth,
                      int32_t* index, void* stream);

/* sp_map_consistency: every point of a map tested against V depth images -- the other keyframes' own (sp_keyframe_depths), or ground
 * truth -- in ONE launch: does the surface a view claims at the point's pixel agree with the point, does the view look straight
 * through it (a free-space violation), or is the point hidden (no evidence either way)?
 *     points : (Q,3) float32 in the frame the view poses live in;  owner : (Q,) int32 or NULL
 *     views  : V records on the device (as sp_render_views);  view_owner : (V,) int32 or NULL
 *     depth  : (V,H,W) float32
 *     counts : (Q,3) int32, WRITTEN FOR EVERY ROW by the call: the number of views in which the point agrees / is in front / is behind
 * In float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal).  Per pair (point i, view j):
 *   - u, v, z exactly as sp_render_views forms them (the same device function; an exact identity pose leaves the point untouched);
 *   - the pair is SKIPPED if owner and view_owner are both given and owner[i] == view_owner[j] >= 0 (a point is not tested against the
 *     keyframe it came from);
 *   - it is UNSEEN unless 0 <= u < W, 0 <= v < H and z > z_min (NaN and +-inf fail);
 *   - (r, c) = (trunc v, trunc u), zf = float64(float32(z)); the window is the pixels (r + dr, c + dc), |dr|, |dc| <= window, clipped to
 *     the image; a pixel with depth D is VALID iff 0 < D < inf (NaN is not), and then b = float64(tol) D;
 *   - no valid pixel in the window: unseen;
 *   - the pair AGREES if any valid pixel has |zf - D| <= b;
 *   - otherwise it is IN FRONT if every valid pixel has zf < D - b;
 *   - otherwise it is BEHIND: behind every surface, or between surfaces without agreeing with any -- neither is evidence against it.
 * The unseen (and skipped) views of a point are V minus its three counts.  Integer counts: two runs give the same bits.
 * Null points / views / depth / counts, Q, V, H or W <= 0, tol negative, NaN or >= 1, window outside 0 .. 2, z_min negative or NaN:
 * SP_EINVAL.  Q > 2^31 - 2, V > 65535, V H W >= 2^31: SP_ELIMIT.  Invalid beats too large. */
int sp_map_consistency(const float* points, const int32_t* owner, long long Q, const SpView* views, const int32_t* view_owner, int V,
                       const float* depth, int H, int W, float tol, int window, float z_min, int32_t* counts, void* stream);

/* sp_image_metrics: rendered views against real images, in ONE launch.
 *     rendered : (V,H,W,3) uint8 (sp_render_views' / sp_render_splats' image);  index : (V,H,W) int32 (their index)
 *     target   : planar (V,3,H,W) float32, converted by the renderer's own rule: trunc(c * 255) from the exact float64 product, clamped
 *                to 0 .. 255, NaN gives 0
 *     out      : (V,3) int64, zeroed by the call: per view, over the pixels with index >= 0 and their three channels,
 *                n (pixels), sum |a - b|, sum (a - b)^2
 * All integers: exact, independent of the order of the sums.  Null pointers, V, H or W <= 0: SP_EINVAL.  V > 65535 or V H W >= 2^31:
 * SP_ELIMIT. */
int sp_image_metrics(const uint8_t* rendered, const float* target, const int32_t* index, int V, int H, int W, long long* out, void* stream);

/* sp_depth_lift: B depth images into one point cloud (tool/viz.py:30-51 depth_image_lift: Open3D's create_from_depth_image with
 * depth_scale 1, stride 1 and depth_trunc, then transform).
 *     depth : (B,H,W) float32;  K : (B,9) float32;  pose : (B,16) float32 camera-to-world or NULL (the identity)
 *     image : planar (B,3,H,W) float32 or NULL, together with colours
 *     block_counts : sp_depth_lift_blocks(B, H, W) int32 of scratch
 * A pixel is valid iff 0 < d <= depth_trunc (NaN is invalid).  Valid pixels are compacted in row-major order, image after image: row
 * offsets[b] + k is the k-th valid pixel of image b.  Three passes (count per 256-pixel block, scan of the block counts, write); no
 * workgroup waits on another.
 *     points  : (B H W, 3) float32.  In float64 from the float32 inputs, every operation rounded on its own:  x = ((c - cx) d) / fx,
 *               y = ((r - cy) d) / fy, z = d, then per row of the pose ((T0 x + T1 y) + T2 z) + T3; rounded to float32 once, at the end
 *     colours : (B H W, 3) float32 = image[b, :, r, c] (a load);  pixel : (B H W,) int32 = r W + c
 *     counts  : (B,) int32;  offsets : (B + 1,) int64;  rows at or beyond offsets[B] are never written
 * Null required pointers, image without colours (or the reverse), B, H, W <= 0, depth_trunc not > 0: SP_EINVAL.  B > 65535 or
 * B H W >= 2^31: SP_ELIMIT (sp_depth_lift_blocks returns the same codes). */
int sp_depth_lift_blocks(int B, int H, int W);
int sp_depth_lift(const float* depth, const float* K, const float* pose, const float* image, int B, int H, int W, float depth_trunc,
                  int32_t* block_counts, float* points, float* colours, int32_t* pixel, int32_t* counts, long long* offsets, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map fusion (sp_fuse.hip): one averaged point per occupied voxel.  A world map is the concatenation of its keyframes' points, so a
 * surface seen by ten keyframes is stored ten times; sp_map_fuse replaces the points of one voxel by their mean.  Everything runs on
 * the caller's stream without a synchronisation; argument checks come before any device work.
 *     points      : (Q,3) float32;  colours : (Q,3) float32, or NULL together with out_colours
 *     voxel       : the voxel's side, a finite float32 > 0;  ox, oy, oz : the grid's origin o, finite float32
 *     scratch     : sp_map_fuse_scratch_units(Q) units of 64 bytes, aligned to 8 bytes, initialised by the call
 *     out_points, out_colours : (Q,3) float32;  count, first : (Q,) int32 -- CAPACITY buffers (the convention of sp_depth_lift): rows
 *                   at or beyond n_fused[0] are never written
 *     label       : (Q,) int32, WRITTEN FOR EVERY ROW;  n_fused : one int64 on the device
 * The voxel of a point.  In float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal).  Per axis a:
 *     q = (p_a - o_a) / voxel,  g = floor(q).
 * A point is DROPPED (label = -1, it contributes nowhere) unless all three q are finite and all three g lie in -2^20 .. 2^20 - 1; the
 * range is tested on the float64 value, before any conversion to an integer.  The voxel's key is
 *     key = (gx + 2^20) << 42 | (gy + 2^20) << 21 | (gz + 2^20)                              (63 bits).
 * The sub-voxel position of a kept point is f = q - g (float64), s_a = min(trunc(f * 65536), 65535), an integer in 0 .. 65535 (the
 * minimum acts only for -2^-54 < q < 0, where q + 1 rounds to 1).  Its colour per channel is the renderer's 8-bit value: trunc of the
 * exact float64 product c * 255, clamped to 0 .. 255, NaN gives 0 (sp_render_views' device function).
 * Per occupied voxel, over its kept points: n (their number), S_a = sum s_a, C_ch = sum colour8, i0 = their lowest input row.  These
 * are integers: the sums are exact in any order, two runs give the same bits.
 * Output order: voxels in ascending order of i0 -- fused row j is the voxel with the j-th smallest first row.  No sort is involved,
 * and input rows grouped by keyframe give fused rows grouped by keyframe, every voxel under the keyframe that saw it first.
 * Fused row j:  first[j] = i0, count[j] = n, and in float64, each operation rounded on its own, rounded to float32 once at the end:
 *     m = float64(S_a) / float64(n),  c = (m + 0.5) / 65536,  out_points[j][a] = (float64(g) + c) * voxel + o_a;
 *     out_colours[j][ch] = float64(C_ch) / (255 * float64(n)).
 * label[i] = the fused row of point i's voxel (-1 for a dropped point);  n_fused[0] = M, the number of occupied voxels.
 * The fused position is the mean of the members, each quantised to 1 / 65536 of a voxel and placed at the middle of its step: per
 * coordinate it differs from the float64 mean of the members' (p_a - o_a) + o_a by less than voxel * 2^-16.
 * Null points / scratch / out_points / count / first / label / n_fused, colours without out_colours or the reverse, Q <= 0, voxel not
 * finite or not > 0, a non-finite origin: SP_EINVAL.  Q > 2^28 (SP_MAP_FUSE_MAX_POINTS: the table's slot numbers and the scratch size
 * in units stay below 2^31; the 64-bit sums hold 2^28 x 65535 with room to spare): SP_ELIMIT.  Invalid beats too large.
 * sp_map_fuse_scratch_units answers Q <= 0 and Q > 2^28 with the same codes.
 * The table: open addressing with linear probing over S slots of 64 bytes, S the smallest power of two >= 2 Q (load <= 0.5), 64-bit
 * keys claimed by compare-and-swap; then Q slot numbers and ceil(Q / 256) block counts.  Five launches after the table's
 * initialisation (insert, count the first rows per 256-row block, scan, emit, label); no workgroup waits on another and every loop is
 * bounded. */
#define SP_MAP_FUSE_MAX_POINTS (1LL << 28)
int sp_map_fuse_scratch_units(long long Q);
int sp_map_fuse(const float* points, const float* colours, long long Q, float voxel, float ox, float oy, float oz, void* scratch,
                float* out_points, float* out_colours, int32_t* count, int32_t* first, int32_t* label, long long* n_fused, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map distances (sp_nearest.hip): for every point of one cloud the nearest point of another within a radius, and the number of points
 * within it.  The map against a ground-truth cloud gives accuracy, the cloud against the map completion; a cloud against itself its
 * spacing and the neighbour count a radius outlier filter keeps points by.  sp_cloud_grid_build prepares the REFERENCE cloud once,
 * sp_cloud_grid_nearest answers any number of query clouds from it.  Everything runs on the caller's stream without a synchronisation
 * and without an allocation; argument checks come before any device work.
 *     points      : (Q,3) float32, the reference cloud;  queries : (Qa,3) float32
 *     radius      : the search radius, a finite float32 > 0;  ox, oy, oz : the origin o of the ranges below, finite float32
 *     scratch     : sp_cloud_grid_scratch_units(Q) units of 64 bytes, aligned to 16 bytes, initialised by the build.  The query reads
 *                   radius and origin from it: a query cannot be run with a radius other than the build's.  It is given the Q of the
 *                   build; a scratch that was built for another Q answers "none" on every row
 *     skip_self   : 0 or 1.  1: the queries ARE the reference cloud (the caller passes the same cloud twice, Qa == Q) and row i is
 *                   not its own neighbour
 *     index, count : (Qa,) int32;  dist : (Qa,) float32 -- ALL THREE WRITTEN FOR EVERY QUERY ROW
 * In float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal):
 *     r = float64(radius),  r2 = r * r,  cell = r * 1.0009765625                                  (1 + 2^-10; each product rounded once)
 *     per axis a of a point p of either cloud:  q = (p_a - o_a) / cell,  g = floor(q).
 * A point is IN RANGE iff all three q are finite and all three g lie in -2^20 + 1 .. 2^20 - 2; the test is made on the float64 value,
 * before any conversion to an integer.  A reference point out of range (NaN and +-inf among them) is never found as a neighbour; a
 * query out of range gets the "none" answer.
 *     d2(i, j) = (dx dx + dy dy) + dz dz,  dx = float64(a_x) - float64(b_x) and so on, for query a = i and reference b = j.
 * The NEIGHBOURS of query i are the reference rows j in range with d2(i, j) <= r2; with skip_self = 1 the row j == i is left out.
 *     count[i] = their number;
 *     index[i] = the neighbour with the smallest (d2, j) in lexicographic order: on equal distance the lowest row wins;
 *     dist[i]  = float32(sqrt(d2)): the square root in float64, correctly rounded, then rounded to float32;
 *     with no neighbour index[i] = -1, dist[i] = +inf, count[i] = 0.
 * A minimum over (d2, j) and a count do not depend on the order in which candidates are visited: two runs give the same bits.
 * Why the search is local.  The reference rows are binned by (gx, gy, gz) and a query looks into the 27 bins around its own.  Take a
 * query a and an in-range reference row b with computed d2 <= r2.  Per axis the computed dx dx is no larger than the computed sum (a
 * rounded sum of non-negative terms is no smaller than any of them), so |a - b| <= r (1 + 2^-51).  t = p_a - o_a as computed lies
 * within 2^-53 |t| of the exact difference, and |t| / cell < 2^20 + 1 in range; the computed quotient lies within 2^-33 of t / cell.
 * So the two computed quotients differ by at most r (1 + 2^-51) / cell + 2^-31 < 1 - 2^-11 + 2^-31 < 1, because cell exceeds r by
 * the factor 1 + 2^-10.  Two numbers less than 1 apart have floors at most 1 apart: every neighbour lies in one of the 27 bins,
 * whatever the origin, and the bins around an in-range query have indices in -2^20 .. 2^20 - 1, which the 21-bit fields of the key hold.
 * The prepared form: a 64-byte header (r2, cell, origin, table mask, Q); S slots of 16 bytes -- a bin's 64-bit key (sp_map_fuse's),
 * where its members start and how many they are --, S the smallest power of two >= 2 Q, open addressing with linear probing (load <=
 * 0.5); Q records of 16 bytes {x, y, z, row}, the members of one bin side by side; Q slot numbers and ceil(S / 256) block sums.  Five
 * launches after the table's initialisation (count per bin, sum per 256 slots, scan, starts, scatter through an atomic cursor); the
 * query is one launch, one lane per query.  No workgroup waits on another and every loop is bounded.
 * Null points / queries / scratch / index / dist / count, a scratch not aligned to 16 bytes, Q or Qa <= 0, skip_self outside {0, 1},
 * skip_self = 1 with Qa != Q, radius not finite or not > 0, a non-finite origin: SP_EINVAL.  Q > 2^28 (SP_CLOUD_GRID_MAX_POINTS: slot
 * numbers, record places and the scratch size in units stay below 2^31) or Qa > 2^31 - 2: SP_ELIMIT.  Invalid beats too large.
 * sp_cloud_grid_scratch_units answers Q <= 0 and Q > 2^28 with the same codes. */
#define SP_CLOUD_GRID_MAX_POINTS (1LL << 28)
int sp_cloud_grid_scratch_units(long long Q);
int sp_cloud_grid_build(const float* points, long long Q, float radius, float ox, float oy, float oz, void* scratch, void* stream);
int sp_cloud_grid_nearest(const float* queries, long long Qa, long long Q, const void* scratch, int skip_self, int32_t* index, float* dist,
                          int32_t* count, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map neighbourhoods (sp_knn.hip): for every query its k nearest points of a cloud prepared by sp_cloud_grid_build, and a surface
 * normal from such a list.  Normals for a cloud that has none (a lifted depth image, a fused map, a scan), the k distances a
 * statistical outlier filter needs, the lists local descriptors start from.  Everything runs on the caller's stream without a
 * synchronisation and without an allocation; argument checks come before any device work.
 *
 * sp_cloud_grid_knn: one launch, one lane per query.
 *     queries, Qa, Q, scratch, skip_self : as for sp_cloud_grid_nearest (radius and origin are read from the scratch header)
 *     k           : 1 .. SP_CLOUD_KNN_MAX, the length of a list
 *     index       : (Qa,k) int32;  dist : (Qa,k) float32;  count : (Qa,) int32 -- EVERY ENTRY OF ALL THREE WRITTEN FOR EVERY QUERY ROW
 * The NEIGHBOURS of query i are exactly those of sp_cloud_grid_nearest -- the same device function walks them: the range test on the
 * query, the reference rows j in range with the float64 d2(i, j) = (dx dx + dy dy) + dz dz <= r2, row i left out with skip_self = 1.
 *     count[i]           = their number (what sp_cloud_grid_nearest writes);
 *     index[i, 0 .. m-1] = the rows of the m = min(k, count[i]) smallest pairs (d2, j), in ascending lexicographic order of (d2, j): on
 *                          equal distance the lowest row comes first, and a cut that falls inside a tie keeps the lowest rows;
 *     dist[i, n]         = float32(sqrt(d2)) of index[i, n]: the square root in float64, correctly rounded, then rounded to float32;
 *     index[i, m .. k-1] = -1,  dist[i, m .. k-1] = +inf.
 * A query out of range or non-finite, and every query against a scratch built for another Q, gets count 0, all -1 and all +inf.
 * The k smallest members of a set under a total order do not depend on the order in which the members are met: two runs, and two
 * builds whose member order differs, give the same bits.  At k = 1 the three outputs equal sp_cloud_grid_nearest's bit for bit.
 * The list of a lane lives in LDS (entry n of lane l at d2[n][l], row[n][l]: 12 bytes per entry), sorted; the worst entry of a full
 * list and the fill level are kept in registers, so a neighbour that does not make the list costs one float64 compare.  Kernels for
 * list capacities 8, 16 and 32, chosen by k.  No atomics, no workgroup waits on another, every loop is bounded.
 * Null queries / scratch / index / dist / count, a scratch not aligned to 16 bytes, Q or Qa <= 0, k < 1, skip_self outside {0, 1},
 * skip_self = 1 with Qa != Q: SP_EINVAL.  k > SP_CLOUD_KNN_MAX, Q > 2^28, Qa > 2^31 - 2, Qa k > 2^31 - 2: SP_ELIMIT.  Invalid beats too
 * large.
 *
 * sp_cloud_normals: one launch, one lane per query.
 *     points      : (Q,3) float32, the cloud the lists index;  queries : (Qa,3) float32;  index : (Qa,k) int32, k in 1 .. SP_CLOUD_KNN_MAX
 *     toward      : (V,3) float32 viewpoints, or NULL;  owner : (Qa,) int32, the viewpoint of every row, or NULL (then V must be 1)
 *     normals     : (Qa,3) float32;  curvature : (Qa,) float32;  used : (Qa,) int32 -- all written for every row
 * The lane walks its list in list order.  An entry outside 0 .. Q-1 is skipped (the -1 padding, and any list of the caller's stays
 * inside the array), a listed point with a non-finite coordinate is skipped; used[i] is the number of points taken.  In float64 from
 * the float32 inputs, every operation rounded on its own (no fma, no reciprocal), with q the query and p the listed points:
 *     d = p - q  (relative to the query: a cloud far from the origin loses nothing);   S1_a += d_a;   S2_ab += d_a d_b  (six sums)
 *     m_a = S1_a / used,   C_ab = S2_ab / used - m_a m_b                                        (the covariance of the neighbourhood)
 * used < 3: normals and curvature NaN.  Else the eigenvalues l0 <= l1 <= l2 of C and the unit eigenvector n of l0 by cyclic Jacobi:
 * SP_CLOUD_NORMALS_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2); a rotation of the pair (p, q) with C_pq != 0 is
 *     theta = (C_qq - C_pp) / (2 C_pq),  t = sgn(theta) / (|theta| + sqrt(theta theta + 1))  (sgn(0) = 1),  c = 1 / sqrt(t t + 1),  s = t c;
 * l0 is the smallest diagonal entry after the sweeps (on a tie the lowest column), n its column divided by its length.
 *     not l1 > 2^-30 l2  (coincident or collinear points, l2 = 0, a non-finite C):  normals and curvature NaN;
 *     curvature = float32(max(l0, 0) / ((l0 + l1) + l2))                                   (the surface variation, 0 .. 1/3).
 * Orientation.  First the component of n of largest magnitude is made positive (on a tie the lowest axis).  Then, with toward and a
 * viewpoint c = toward[owner[i]] (toward[0] without owner; an owner outside 0 .. V-1 has none):  dot = (n_x e_x + n_y e_y) + n_z e_z
 * with e = c - q, taken of n as the solver left it:  dot < 0: that n is negated;  dot > 0: it is kept, whatever the first rule said;
 * dot = 0 or NaN: the first rule stands.  So the computed n . (c - q) is never negative, and the sign is defined on every row.
 * n is rounded to float32 once, at the end.  A NaN normal is what sp_cloud_register ignores ("a non-finite normal contributes
 * nothing").  Two runs give the same bits: every sum is taken in list order.
 * Null points / queries / index / normals / curvature / used, Q or Qa <= 0, k < 1, toward with V < 1, toward without owner and V != 1:
 * SP_EINVAL.  k > SP_CLOUD_KNN_MAX, Q > 2^28, Qa > 2^31 - 2, Qa k > 2^31 - 2: SP_ELIMIT.  Invalid beats too large. */
#define SP_CLOUD_KNN_MAX 32
#define SP_CLOUD_NORMALS_SWEEPS 8
int sp_cloud_grid_knn(const float* queries, long long Qa, long long Q, const void* scratch, int skip_self, int k, int32_t* index, float* dist,
                      int32_t* count, void* stream);
int sp_cloud_normals(const float* points, long long Q, const float* queries, const int32_t* index, long long Qa, int k, const float* toward,
                     int V, const int32_t* owner, float* normals, float* curvature, int32_t* used, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map registration (sp_register.hip): the similarity x -> s R x + t that moves a QUERY cloud onto a REFERENCE cloud prepared by
 * sp_cloud_grid_build, by Gauss-Newton ICP (iterative closest point) from a start the caller gives.  Everything runs on the caller's
 * stream: no host synchronisation, no allocation, no host read per iteration; argument checks come before any device work.
 *     queries      : (Qa,3) float32;  normals : (Q,3) float32 for residual 1 (the REFERENCE cloud's, one row per grid point), (Qa,3)
 *                    float32 for residual 2 (the QUERY cloud's), NULL allowed for residual 0 (ignored there)
 *     grid_scratch : what sp_cloud_grid_build wrote for the Q reference points (its radius r is the correspondence radius)
 *     residual     : 0 point to point, 1 point to plane (reference normals), 2 plane to point (query normals);  with_scale : 0 or 1
 *     huber        : 0 = every pair weighs 1, > 0 the Huber threshold;  tol : the step length at which the iteration has converged
 *     min_pairs    : fewer pairs than this end the run (SP_CLOUD_REG_FEW);  max_iters : the iterations enqueued
 *     state        : one SpCloudReg on the device.  THE CALLER WRITES rot, trans AND s, the start; the call owns every other field
 *     history      : (max_iters,4) float64 {n, cost, step, status}, one row per enqueued iteration;  index : (Qa,) int32, written for
 *                    every row;  work : sp_cloud_register_work_doubles(Qa) float64 of scratch
 * The rest of the state is zeroed (status = SP_CLOUD_REG_RUNNING), then ONE ITERATION IS TWO LAUNCHES, and all max_iters iterations
 * are enqueued; once the status is no longer RUNNING both passes return after one uniform load.
 * Pass A, one lane per query row i, ceil(Qa / 256) workgroups.  Float64 from the float32 inputs, every operation rounded on its own
 * (no fma, no reciprocal), three-term sums as (x + y) + z.  With R, t, s of the state:
 *     a'_k = s ((R_k0 a_x + R_k1 a_y) + R_k2 a_z) + t_k                                                           (the moved point)
 *     b    = the reference row sp_cloud_grid_nearest finds for the position a' -- the same device function: the range test on a',
 *            the 27 cells, d2 <= r2, the smallest (d2, row) --,  d = a' - b.
 * Unknowns omega (3), v (3), sigma (1: the log of the scale's change; its column J_sigma is 0 with with_scale = 0).  Rows of the residual:
 *     0: three rows r = d;   row k has J_omega = row k of -[a']x = {(0, a'_z, -a'_y), (-a'_z, 0, a'_x), (a'_y, -a'_x, 0)}, J_v = e_k,
 *        J_sigma = a'_k
 *     1: n = normals[row of b];       r = n . d,  J_omega = a' x n,  J_v = n,  J_sigma = n . a'
 *     2: n = R normals[i] (each row (x + y) + z);  r = n . d,  J_omega = b x n,  J_v = n,  J_sigma = n . a'  (the normal turns with the
 *        cloud, which is part of the linearisation: hence b)
 * Dot products as (x + y) + z, a cross product's component as u_y v_z - u_z v_y (two products, one difference).
 *     w = 1;  with huber > 0:  w = min(1, huber / rho),  rho = sqrt((d_x d_x + d_y d_y) + d_z d_z) for residual 0, |r| for 1 and 2;
 *     rho = 0 gives w = 1.
 * A row CONTRIBUTES unless it has no neighbour (a non-finite a' has none: the range test), or the normal it uses or n is non-finite;
 * then index[i] = -1, else the neighbour's row.  Sums over the rows of the residual of the contributing query rows, with wJ_a = w J_a:
 *     H_ab = sum wJ_a J_b (a <= b),   g_a = sum wJ_a r,   cost = sum (w r) r,   n = the contributing query rows (an exact int64).
 * Each workgroup reduces its lanes in a fixed order (a butterfly over the 64 lanes of a wave, then ((w0 + w1) + (w2 + w3))) and writes
 * one record of 40 float64 to work (28 H, 7 g, cost, n as int64, 3 unused).  No floating-point atomics.
 * Pass B, one workgroup: the records summed in a fixed order (25 strided running sums per entry -- record g, g + 25, ... --, then
 * those 25 in order); then
 *     n < min_pairs: status = SP_CLOUD_REG_FEW, no solve, the transform stays bitwise as it was;
 *     a non-finite sum, a pivot of the LDL^T factorisation of H (6 x 6, or 7 x 7 with scale; float64) that is not > 0, or a solution
 *     whose length is not finite: status = SP_CLOUD_REG_DEGENERATE, the transform stays bitwise as it was;
 *     else H delta = -g is solved and the transform moves on the left.  theta2 = (w_x w_x + w_y w_y) + w_z w_z for omega = w:
 *         theta2 < 2^-26 (SP_CLOUD_REG_SMALL_ANGLE2):  A = 1 - theta2 / 6,  B = 0.5 - theta2 / 24   (the next terms are below 2^-58)
 *         else theta = sqrt(theta2),  A = sin(theta) / theta,  h = sin(theta / 2) / (theta / 2),  B = 0.5 h h    (no cancellation)
 *         dR = I + A [w]x + B [w]x [w]x,   e = exp(sigma)
 *         R <- dR R,   t <- e (dR t) + v,   s <- s e
 *     step = sqrt of the sum of delta_k^2 in order;  step <= tol: status = SP_CLOUD_REG_CONVERGED;  else, on the last enqueued
 *     iteration, SP_CLOUD_REG_MAX_ITERS.
 * Pass B stores H, g, delta (0 without a solve), cost, n and step in the state, counts the iteration in state.iterations and writes
 * history[iter] = {n, cost, step, status}.  The rows of history after the stop are {0, 0, 0, status}.
 * The correspondences do not depend on the order in which the build scattered the grid's records (a minimum over (d2, row)) and every
 * sum is taken in a fixed order: TWO RUNS GIVE THE SAME BITS in state, history and index; with the reference rows permuted the state is
 * bitwise the same and index is renamed (where no two candidates tie in d2).  Permuting the QUERY rows reorders the sums: the result
 * agrees within the rounding of the sums only.
 * No workgroup waits on another, nothing spins, every loop is bounded.
 * Null queries / grid_scratch / state / history / index / work, normals missing for residual 1 or 2, residual outside 0 .. 2,
 * with_scale outside {0, 1}, huber or tol negative or non-finite, min_pairs below the number of unknowns (6, or 7 with scale),
 * max_iters < 1, Q or Qa <= 0, a grid_scratch or work not aligned to 16 bytes, state / history not aligned to 8: SP_EINVAL.
 * Q > 2^28, Qa > 2^31 - 2 or max_iters > SP_CLOUD_REG_ITERS_LIMIT (the launches are enqueued up front): SP_ELIMIT.  Invalid beats too
 * large.  sp_cloud_register_work_doubles answers Qa <= 0 and Qa > 2^31 - 2 with the same codes. */
#define SP_CLOUD_REG_RUNNING 0
#define SP_CLOUD_REG_CONVERGED 1
#define SP_CLOUD_REG_MAX_ITERS 2
#define SP_CLOUD_REG_FEW 3
#define SP_CLOUD_REG_DEGENERATE 4
#define SP_CLOUD_REG_ITERS_LIMIT 4096
#define SP_CLOUD_REG_WORK_DOUBLES 40
#define SP_CLOUD_REG_SMALL_ANGLE2 1.490116119384765625e-8 /* 2^-26 */
typedef struct SpCloudReg {
    double rot[9];       /* R, row major */
    double trans[3];     /* t */
    double s;
    double H[28];        /* upper triangle of the 7 x 7 system, row major: (0,0) .. (0,6), (1,1) .. (1,6), ..., (6,6) */
    double g[7];
    double delta[7];     /* omega, v, sigma of the last solve */
    double cost;
    double step;
    long long n;
    int32_t status;      /* SP_CLOUD_REG_* */
    int32_t iterations;  /* the iterations that ran while RUNNING */
    double pad_[5];      /* to a whole number of 64-byte units */
} SpCloudReg;
SP_ABI_SIZE(SpCloudReg, 512)
SP_ABI_ASSERT(sizeof(SpCloudReg) % 64 == 0, "SpCloudReg is padded to a multiple of 64 bytes")
int sp_cloud_register_work_doubles(long long Qa);
int sp_cloud_register(const float* queries, const float* normals, long long Qa, long long Q, const void* grid_scratch, int residual,
                      int with_scale, double huber, double tol, long long min_pairs, int max_iters, SpCloudReg* state, double* history,
                      int32_t* index, double* work, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Map surfaces (sp_tsdf.hip): V depth images fused into one dense signed-distance volume, and its zero level set cut into an indexed
 * triangle mesh.  Everything runs on the caller's stream without a synchronisation; argument checks come before any device work; no
 * floating-point atomics anywhere: two runs give the same bits.
 *
 * sp_tsdf_integrate fuses V depth images into the volume, in place.
 *     depth   : (V,H,W) float32;  images : (V,3,H,W) float32, or NULL together with colour
 *     views   : V SpView records on the device, camera-to-world (the records of sp_render_views)
 *     tsdf, weight : (nz,ny,nx) float32;  colour : (nz,ny,nx,3) float32 -- all three read and updated.  A fresh volume is all zeros;
 *               clearing it is the caller's job, so a second call continues the first
 *     voxel   : the voxel's side;  ox, oy, oz : the origin o;  trunc : the truncation distance;  z_min, depth_max : the depth range
 * Node (ix,iy,iz) sits at its voxel's centre, per axis a
 *     p_a = ((float64(i_a) + 0.5) * voxel) + o_a
 * in float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal), as everywhere in the map kernels.
 * One thread owns one node and walks the views in order v = 0 .. V-1:
 *     d = p - t,  p_c = R^T d  with the operation order of sp_render_views (the same device function);  z = p_c.z;  skip unless z > z_min
 *     u = x fx / z + cx,  v = y fy / z + cy;  col = floor(u + 0.5),  row = floor(v + 0.5): pixel centres are at integers here (the
 *     tables unproject (c - cx) / fx);  skip unless both are finite, 0 <= col < W and 0 <= row < H
 *     D = depth[v,row,col];  skip unless D is finite and 0 < D <= depth_max
 *     sdf = float64(D) - z;  skip if sdf < -trunc;  s = float32(min(1.0, sdf / trunc))
 *     in float32, every operation rounded on its own:  Wn = weight + 1;  tsdf = (tsdf * weight + s) / Wn;  each colour channel likewise
 *     from images[v,ch,row,col], a NaN colour taken as 0;  weight = Wn
 * One call over views 0 .. V-1 therefore leaves the bits of two calls over 0 .. k-1 and k .. V-1.
 * Null depth / views / tsdf / weight, images without colour or the reverse, V, H, W, nx, ny or nz < 1, voxel or trunc not finite or not
 * > 0, z_min negative or NaN, depth_max not > 0 (+inf is allowed), a non-finite origin: SP_EINVAL.  V > 65535, V H W >= 2^31,
 * nx ny nz > 2^30: SP_ELIMIT.  Invalid beats too large.
 *
 * sp_tsdf_mesh cuts the zero level set by marching tetrahedra on the Kuhn split of every cell.
 *     tsdf, weight, colour (or NULL), nx, ny, nz, voxel, ox, oy, oz : the volume, as above
 *     scratch : sp_tsdf_mesh_scratch_bytes(nx, ny, nz) bytes, aligned to 4, initialised by the call.  One int32 per node (the 7-bit mask of
 *               its crossing edges and the number of crossing edges before it in its 256-node block), one per 256 nodes and one per 256
 *               cells, each array rounded up to 64 bytes: at most 4 (nx ny nz) (1 + 2 / 256) + 256 bytes, below 4.1 GiB at the
 *               limit -- the reason the size is a long long
 *     vertices, vertex_colours : (max_vertices,3) float32;  faces : (max_faces,3) int32 -- CAPACITY buffers: rows at or beyond the
 *               capacity are never written.  vertices is NULL iff max_vertices = 0, faces is NULL iff max_faces = 0, vertex_colours is
 *               non-NULL iff colour is given and max_vertices > 0; everything NULL and 0 is the counting call
 *     n_out   : two int64 on the device, always written: the true number of vertices and of faces; the caller compares them with its
 *               capacities.  Should either exceed 2^31 - 1 (indices are int32), no row is written at all
 * A node is VALID iff its weight is >= min_weight and its tsdf is finite, NEGATIVE iff its tsdf is < 0 (an exact 0 is positive).
 * Corner c of a cell has offset bits x = 1, y = 2, z = 4.  Lattice edges run from a node to node + offset for the seven offsets with
 * bits 1 .. 7; the edge id is node_linear * 7 + (bits - 1), node_linear = (iz ny + iy) nx + ix.  An edge CROSSES iff both ends are valid
 * and exactly one is negative.
 * Vertices: one per crossing edge, numbered in ascending edge id (a scan; no sort, no atomics).  With a the lower node and b the upper,
 *     t = f_a / (f_a - f_b)  in float64 from the float32 values;  per axis  p_a + t * (p_b - p_a)  with the node positions above, rounded
 *     to float32 once;  colours the same way from the two nodes' colours.
 * Faces: each of the (nx-1)(ny-1)(nz-1) cells splits into six tetrahedra that share the diagonal 0-7, by corner
 *     0: 0,1,3,7   1: 0,1,5,7   2: 0,2,3,7   3: 0,2,6,7   4: 0,4,5,7   5: 0,4,6,7
 * whose edges are all lattice edges of the seven types, and neighbouring cells agree on their shared face diagonals: the mesh welds
 * without a search.  A tetrahedron emits only if all four nodes are valid: one or three negative nodes give one triangle on the three
 * edges at the lone node, two give a quad on the four crossing edges.  The crossing edges are written as a cycle q0, q1, .. that starts
 * at the smallest edge id and is oriented so that, with every vertex at the MIDPOINT of its edge (exact half-lattice integers),
 * (v1 - v0) x (v2 - v0) has a positive dot product with (centroid of the positive nodes - centroid of the negative nodes): faces look
 * into free space, towards the cameras.  The triangles are (q0,q1,q2) and, for a quad, (q0,q2,q3).  That orientation depends only on
 * (tetrahedron, sign case): a table of 6 x 16 entries, built from this rule at compile time.
 * Faces are ordered by ascending cell linear index ((iz (ny-1) + iy)(nx-1) + ix), then tetrahedron 0 .. 5, then triangle (a scan).
 * A vertex that falls on a node (t = 0 or 1) is kept, so degenerate triangles may occur.
 * Null tsdf / weight / scratch / n_out, a scratch not aligned to 4 bytes, nx, ny or nz < 2, a negative capacity, a buffer that is NULL
 * with a capacity > 0 or the reverse, voxel not finite or not > 0, a non-finite origin, a NaN min_weight: SP_EINVAL.  nx ny nz > 2^30 or
 * a capacity > 2^31 - 1: SP_ELIMIT.  Invalid beats too large.  sp_tsdf_mesh_scratch_bytes answers sizes < 2 and nx ny nz > 2^30 with the
 * same codes.  Three launches count (nodes, cells, one scan of both block arrays), two more write. */
#define SP_TSDF_MAX_NODES (1LL << 30)
int sp_tsdf_integrate(const float* depth, const float* images, const SpView* views, int V, int H, int W, int nx, int ny, int nz, float voxel,
                      float ox, float oy, float oz, float trunc, float z_min, float depth_max, float* tsdf, float* weight, float* colour,
                      void* stream);
long long sp_tsdf_mesh_scratch_bytes(int nx, int ny, int nz);
int sp_tsdf_mesh(const float* tsdf, const float* weight, const float* colour, int nx, int ny, int nz, float voxel, float ox, float oy, float oz,
                 float min_weight, void* scratch, long long max_vertices, long long max_faces, float* vertices, float* vertex_colours,
                 int32_t* faces, long long* n_out, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Surface views (sp_raycast.hip): the volume ray-cast into depth, normal, colour and cell-index images of V cameras -- the surface a
 * sequence saw, or a ground-truth surface, as sp_depth_metrics and sp_image_metrics score it, and the model view a frame-to-model step
 * needs.  ONE launch, one thread per pixel, on the caller's stream without a synchronisation; no atomics, no scratch, nothing zeroed:
 * two runs give the same bits.  Argument checks come before any device work.
 *     tsdf, weight, colour (or NULL), nx, ny, nz, voxel, ox, oy, oz, min_weight : the volume, as sp_tsdf_mesh takes it
 *     views   : V SpView records on the device, camera-to-world
 *     z_start, step, n_steps : the samples of a ray, at camera depths z_k = z_start + k step, k = 0 .. n_steps-1
 *     depth   : (V,H,W) float32;  normals : (V,H,W,3) float32, world frame;  image : (V,H,W,3) uint8;  index : (V,H,W) int32 -- each may be
 *               NULL, at least one must be given, image needs colour.  EVERY GIVEN OUTPUT IS WRITTEN FOR EVERY PIXEL
 * THE RULE.  Float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal).
 * Ray.  Pixel centres are at integers, as in sp_tsdf_integrate:  xr = (col - cx) / fx,  yr = (row - cy) / fy.  The ray is parameterised by
 * camera z, the quantity depth images and the projective sdf of sp_tsdf_integrate use:  q = (xr z, yr z, z), and the world point is
 *     p_a(z) = ((R_a0 q0 + R_a1 q1) + R_a2 q2) + t_a;   an exact identity pose leaves p = q (sp_render_views' convention).
 * Sample S(p).  Per axis  g_a = ((p_a - o_a) / voxel) - 0.5,  i_a = floor(g_a),  f_a = g_a - i_a.  The sample is VALID iff every g_a is
 * finite, 0 <= i_a and i_a + 1 <= n_a - 1 on all three axes, and all eight nodes (ix + dx, iy + dy, iz + dz), dx, dy, dz in {0, 1}, are
 * valid by sp_tsdf_mesh's definition (weight >= min_weight, tsdf finite).  Its value is the trilinear interpolation of the eight tsdf
 * values by lerps a + f (b - a): along x first (four, f = f_x, a at dx = 0), then y (two), then z (one).  C(p), three colour channels, is
 * interpolated in the same way from the same cell.
 * March.  z_k = z_start + float64(k) step,  F_k = S(p(z_k)).  The ray ENDS at the first k whose sample is valid and negative (F_k < 0; an
 * exact 0 is positive, as in the mesh).  It is a HIT iff k >= 1, sample k-1 is valid and F_{k-1} >= 0; otherwise the ray ends without a
 * hit (the surface is seen from behind, or through an unobserved gap).  A ray that never meets a valid negative sample has no hit.
 * On a hit.  t = F_{k-1} / (F_{k-1} - F_k),  z* = t step + z_{k-1};  depth = float32(z*);  index = (iz ny + iy) nx + ix of the lower
 * node of sample k's cell;  per channel c = C_{k-1} + t (C_k - C_{k-1}), rounded to float32 once, and image = trunc(c * 255) from the
 * exact float64 product, clamped to 0 .. 255, NaN gives 0 (sp_render_views' rule and device function).
 * Normal.  With p* = p(z*) and h = voxel:  g_a = S(p* + h e_a) - S(p* - h e_a).  If any of the six samples is invalid all three components
 * are NaN (the depth stands).  Otherwise n = g / sqrt((g0 g0 + g1 g1) + g2 g2), IEEE square root and divisions, rounded to float32 once;
 * a length that is not finite or not > 0 gives NaN.  The tsdf grows towards free space, so n faces the cameras that saw the surface: the
 * orientation of sp_map_normals and of the mesh's faces.
 * No hit.  depth = 0, index = -1, image = 0, 0, 0, normals NaN.
 * A sample outside the box of node centres is invalid by the rule, so the kernel skips the k it can prove invalid (the ray clipped
 * against the box, widened by far more than any rounding, plus a step either side) and runs the rule over the rest: the result is that
 * of marching every k.  The step is fixed; skipping free space by the field's value would change which pair of samples brackets the
 * crossing and is not done.
 * Null tsdf / weight / views, all four outputs NULL, image without colour, nx, ny or nz < 2, V, H or W < 1, voxel or step not finite or
 * not > 0, a non-finite origin, a NaN min_weight, z_start negative or not finite, n_steps < 2: SP_EINVAL.  V > 65535, V H W >= 2^31,
 * nx ny nz > 2^30, n_steps > 2^20 (SP_TSDF_RAYCAST_MAX_STEPS): SP_ELIMIT.  Invalid beats too large. */
#define SP_TSDF_RAYCAST_MAX_STEPS (1 << 20)
int sp_tsdf_raycast(const float* tsdf, const float* weight, const float* colour, int nx, int ny, int nz, float voxel, float ox, float oy, float oz,
                    float min_weight, const SpView* views, int V, int H, int W, float z_start, float step, int n_steps, float* depth,
                    float* normals, uint8_t* image, int32_t* index, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Mesh surfaces (sp_mesh.hip): a triangle list -- sp_tsdf_mesh's, or a ground-truth model's -- as a surface: one record per face, and an
 * area-uniform, seeded cloud with normals sampled from those records.  Everything runs on the caller's stream without a synchronisation;
 * argument checks come before any device work; no floating-point atomics, no float prefix sum, no sort: two runs give the same bits.
 * THE RULE.  Float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal); three-term sums as (x + y) + z.
 *
 * sp_mesh_faces: one record per face, one thread per face.
 *     vertices : (M,3) float32;  faces : (F,3) int32
 *     area     : (F,) float64;  normals : (F,3) float32;  state : (F,) uint8;  cross : (F,3) float64 -- each may be NULL
 *     summary  : SP_MESH_SUMMARY_WORDS = 6 int64 on the device, zeroed and written by the call: the number of faces of state 0, 1, 2, 3, 4
 *                (integer atomics: order-free) and, in word 5, the BITS of the largest area as float64 (a maximum over the bit patterns
 *                of non-negative doubles, which order as the doubles do: order-free too; 0.0 when no face is valid).  The total area is not
 *                part of the contract: a float64 sum has an order, and the caller forms it
 * With (i0, i1, i2) the face's indices and p0, p1, p2 their vertices, the state is the first of these that applies:
 *     1  an index outside [0, M)                   2  two equal indices
 *     3  a non-finite coordinate among the nine    4  zero area: the area below is not > 0, or not finite
 *     0  valid
 *     e1 = p1 - p0,  e2 = p2 - p0  (the differences first);   c = e1 x e2, each component a difference of two products:
 *     c_x = e1_y e2_z - e1_z e2_y,   c_y = e1_z e2_x - e1_x e2_z,   c_z = e1_x e2_y - e1_y e2_x
 *     l = sqrt((c_x c_x + c_y c_y) + c_z c_z)  (IEEE square root);   area = 0.5 l;   normal = c / l per component, rounded to float32 once
 * area, normal and cross (= c) are zeros unless the state is 0.
 * Null vertices / faces / summary, F or M < 1: SP_EINVAL.  F or M > 2^28 (SP_MESH_MAX_FACES): SP_ELIMIT.  Invalid beats too large.
 *
 * sp_mesh_sample: the cloud.  Three launches: a count (one thread per face), one scan workgroup, and -- with a capacity -- a write with
 * ONE THREAD PER OUTPUT ROW, which finds its face by binary search in the integer offsets: a face of 10^6 rows is 10^6 threads.
 *     vertices, M, faces, F : the mesh, as above;  vertex_colours : (M,3) float32 or NULL
 *     area, state : (F,) float64 and uint8, what sp_mesh_faces wrote for this mesh;  face_normals : its normals, or NULL
 *     density  : samples per unit area, finite and > 0;   seed : any 64 bits
 *     scratch  : sp_mesh_sample_scratch_units(F) units of 64 bytes, aligned to 8 bytes, initialised by the call: one int64 per face (the
 *                rows of the faces before it in its 256-face block) and one per 256 faces (the rows before the block), each array a whole
 *                number of units: 2^25 + 2^17 units at the limit, so the size is an int as those of sp_map_fuse and sp_cloud_grid_build are
 *     points, normals, colours : (capacity,3) float32;  face : (capacity,) int32 -- CAPACITY buffers: rows at or beyond the capacity are
 *                never written.  points is NULL iff capacity = 0; normals, colours and face are optional with a capacity and NULL without;
 *                normals needs face_normals, colours needs vertex_colours.  Every output NULL and capacity 0 is the counting call
 *     n_out    : one int64 on the device, always written: the true number of rows.  Should it exceed 2^31 - 1, no row is written
 * mix is the splitmix64 finaliser (x ^= x >> 30, x *= 0xbf58476d1ce4e5b9, x ^= x >> 27, x *= 0x94d049bb133111eb, x ^= x >> 31), all
 * integer arithmetic is modulo 2^64, and  A(x) = mix(x) >> 11  (53 bits),  U(x) = float64(A(x)) * 2^-53  in [0, 1), exact.
 * Face i:  h = seed + 0x9E3779B97F4A7C15 * (i + 1).  Its number of rows is
 *     t = area_i * density, and t = 2^31 unless t < 2^31;   n_i = floor(t + U(h))   (the product and the sum each rounded)
 * and n_i = 0 for a face whose state is not 0 -- or one of whose indices is outside [0, M), whatever its state says: a record of
 * sp_mesh_faces never differs there, the test only keeps a foreign record from reading beyond the vertices.  So |n_i - area_i density| < 1
 * for every face below the clamp (= 1 only where the rounded sum lands on an integer the exact one stays below): stochastic rounding, unbiased.
 * Rows are ordered by (face, k), k = 0 .. n_i - 1: the first row of face i is the exclusive int64 prefix sum of n.  Row k of face i:
 *     a1 = A(h + 1 + 2k),  a2 = A(h + 2 + 2k);  if a1 + a2 > 2^53 (the exact integer sum), both become 2^53 - a;  u = float64(a) * 2^-53:
 *     u1 + u2 > 1 folds the point back into the triangle by u -> 1 - u, exactly, and 1 - u1 - u2 >= 0 afterwards
 *     points, per axis   (p0 + u1 * (p1 - p0)) + u2 * (p2 - p0),  rounded to float32 once;   colours the same from the vertices' colours
 *     normals = face_normals[i];   face = i
 * Null vertices / faces / area / state / scratch / n_out, a scratch not aligned to 8 bytes, F or M < 1, a negative capacity, density not
 * finite or not > 0, points NULL with a capacity > 0 or the reverse, another output with capacity 0, normals without face_normals,
 * colours without vertex_colours: SP_EINVAL.  F or M > 2^28, a capacity > 2^31 - 1: SP_ELIMIT.  Invalid beats too large.
 * sp_mesh_sample_scratch_units answers F < 1 and F > 2^28 with the same codes. */
#define SP_MESH_MAX_FACES (1LL << 28)
#define SP_MESH_SUMMARY_WORDS 6
int sp_mesh_faces(const float* vertices, long long M, const int32_t* faces, long long F, double* area, float* normals, uint8_t* state,
                  double* cross, long long* summary, void* stream);
int sp_mesh_sample_scratch_units(long long F);
int sp_mesh_sample(const float* vertices, const float* vertex_colours, long long M, const int32_t* faces, long long F, const double* area,
                   const float* face_normals, const uint8_t* state, double density, long long seed, void* scratch, long long capacity,
                   float* points, float* normals, float* colours, int32_t* face, long long* n_out, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Mesh views (sp_mesh_render.hip): a triangle mesh rasterised into depth, normal, colour and face-index images of V cameras -- ground-
 * truth depth from a ground-truth model, the views of an extracted or cleaned mesh, and the per-face visibility a benchmark culls by.
 * Runs on the caller's stream without a synchronisation; argument checks come before any device work; 64-bit integer atomic maxima only:
 * two runs give the same bits.
 *     vertices : (M,3) float32;  vertex_colours : (M,3) float32 or NULL;  faces : (F,3) int32
 *     face_normals : (F,3) float32, the normals of sp_mesh_faces for this mesh, or NULL
 *     views    : V SpView records on the device, camera-to-world;  cull : 0 (two-sided) or 1 (only faces seen from their front)
 *     scratch  : sp_mesh_render_scratch_units(F) units of 64 bytes, aligned to 8 bytes, written by the call: for ONE chunk of
 *                SP_MESH_RENDER_VIEW_CHUNK views one int64 per (face, view) padded to 256-face blocks, one per block, and the total
 *                (1 + 2^21 + 2^29 units at the limit: an int, like the sizes of sp_mesh_sample and sp_map_fuse)
 *     keys     : V H W uint64 of scratch, zeroed by the call
 *     depth    : (V,H,W) float32;  normals : (V,H,W,3) float32, world frame;  image : (V,H,W,3) uint8;  index : (V,H,W) int32 -- each may be
 *                NULL, at least one must be given, image needs vertex_colours, normals needs face_normals.  EVERY GIVEN OUTPUT IS WRITTEN
 *                FOR EVERY PIXEL
 * THE RULE.  Float64 from the float32 inputs, every operation rounded on its own (no fma, no reciprocal); three-term sums as (x + y) + z.
 * Face.  A face is USABLE iff its three indices are in [0, M) and distinct and its nine coordinates are finite (states 1 to 3 of
 * sp_mesh_faces, tested again so that a foreign record cannot make the kernel read beyond the vertices).  An unusable face covers nothing.
 * Camera frame.  q_k = R^T (p_k - t), k = 0, 1, 2, exactly as sp_render_views forms p_c (the same device function; an exact identity pose
 * leaves the point untouched).
 * Edge planes.  n_0 = q_1 x q_2,  n_1 = q_2 x q_0,  n_2 = q_0 x q_1,  each component a difference of two products in sp_mesh_faces' order:
 *     (a x b)_x = a_y b_z - a_z b_y,   (a x b)_y = a_z b_x - a_x b_z,   (a x b)_z = a_x b_y - a_y b_x
 * det = (q_0x n_0x + q_0y n_0y) + q_0z n_0z.  A face whose det is 0 or not finite covers nothing in that view.  det < 0 is a face seen
 * from its front, the side its sp_mesh_faces normal points to; cull = 1 drops a face unless det < 0.
 * Pixel.  Pixel centres are at integers, as in sp_tsdf_raycast and sp_tsdf_integrate (the depth image is what those and the depth scores
 * consume):  a = (col - cx) / fx,  b = (row - cy) / fy,  E_k = (n_kx a + n_ky b) + n_kz,  S = (E_0 + E_1) + E_2.  With sigma the sign of
 * det the pixel is COVERED iff sigma E_k >= 0 for k = 0, 1, 2 (a zero of either sign passes, NaN fails), sigma S > 0, and z = det / S (an
 * IEEE division) satisfies z > z_min and z < inf.  The comparison is inclusive on purpose: for an edge shared by two faces the ordered
 * pair (q_i, q_j) of one is (q_j, q_i) of the other, every component of the cross product and with it E negates exactly, so a pixel centre
 * is inside one of the two faces or on the edge of both: no cracks, and no fill-rule table.  The test is homogeneous: a face that crosses
 * the camera plane needs no clipping, and a face behind the camera fails the sign test.
 * Rectangle.  Part of the rule, so that the result does not depend on how an implementation bounds its work.  With z_k = q_kz:
 *   - all three z_k <= z_min: the face covers nothing (every point of it lies at or behind the plane);
 *   - all three z_k > z_min:  (u_k, v_k) = (x fx / z + cx, y fy / z + cy) of q_k, sp_render_views' projection (the same device function).
 *     The face is tested on the columns max(floor(min u), 0) .. min(ceil(max u), W - 1) and the rows max(floor(min v), 0) ..
 *     min(ceil(max v), H - 1), clamped in float64 and then converted; an empty range covers nothing.  Should one of the six numbers not
 *     be finite, the face is tested on the whole image;
 *   - otherwise the face crosses the plane and is tested on the whole image.
 * Contest.  Every covered pixel offers key_nearest(float32(z), face), sp_render_views mode 1's key: the smallest float32(z) wins, equal
 * float32(z) goes to the HIGHEST face index.
 * Resolve.  The winner's values are functions of (face, view, pixel) alone:  depth = float32(z);  index = the face;  normals =
 * face_normals[face], in the world frame and not flipped;  lambda_k = E_k / S (IEEE divisions), and per channel colour = (lambda_0 c_0 +
 * lambda_1 c_1) + lambda_2 c_2 from the three vertices' colours, rounded to float32 once, then sp_render_views' 8-bit rule (trunc(c * 255)
 * clamped to 0 .. 255, NaN gives 0): perspective-correct by construction.  No winner: depth = 0, index = -1, image = 0, 0, 0, normals NaN --
 * sp_tsdf_raycast's no-hit convention.
 * The kernels cut the rectangle into tiles of 64 pixels, one wave per (face, view, tile); the tile's shape is a compile-time choice the
 * result cannot depend on.
 * Null vertices / faces / views / scratch / keys, a scratch or keys not aligned to 8 bytes or another pointer not aligned to 4, all four
 * outputs NULL, image without vertex_colours, normals without face_normals, F, M, V, H or W < 1, z_min negative or NaN, cull outside
 * {0, 1}: SP_EINVAL.  F or M > 2^28 (SP_MESH_MAX_FACES), V > 65535, V H W >= 2^31: SP_ELIMIT.  Invalid beats too large.
 * sp_mesh_render_scratch_units answers F < 1 and F > 2^28 with the same codes. */
#define SP_MESH_RENDER_VIEW_CHUNK 16
int sp_mesh_render_scratch_units(long long F);
int sp_mesh_render(const float* vertices, const float* vertex_colours, long long M, const int32_t* faces, long long F,
                   const float* face_normals, const SpView* views, int V, int H, int W, float z_min, int cull, void* scratch,
                   unsigned long long* keys, float* depth, float* normals, uint8_t* image, int32_t* index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SP_HIP_H */
