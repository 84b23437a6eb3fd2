// sp_chain.hip -- one foreign call per FRAME index of the monocular-odometry chain, for S sequences in lockstep (include/sp_hip.h
// sp_chain_step_multi; reference: odometery/odometery.py:1018-1075 -- track_frame, mapping(mode='supp'), is_kf of a frame that is not a
// keyframe).  One sequence is the call at S = 1.
//
// Nothing new is computed here: the stages are the library's own device functions and launch helpers (the pyramid, edge composition, the
// round body of sp_window_gn_run_multi, sp_depth_splat / sp_kf_criterion_ws's passes) strung together on one stream, every launch covering
// all records (sequence = blockIdx), with small kernels in place of what the Python loop did on the host between them -- overwrite a node's
// pose from a device buffer, reset / re-phase the LM state, read the node back out, inv(A) B of two poses, the slot moves.  Per record the
// arithmetic is that of the record alone: the same device functions on the same values; a window that froze is inert (its update returns
// before it touches anything, its counter stops), so the extra rounds it sits through while others converge change none of its results.
// State stays on the device; the host sees the LM states the phase loop polls and, after the call's one synchronisation, the windows'
// final states and the four floats of the keyframe criterion.
//
// Errors: SP_EINVAL / SP_ELIMIT before anything is launched, a positive hipError_t for a failed launch or copy, and the codes of
// wgn_multi_round unchanged (shared with sp_window_gn_run_multi).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/sp_hip.h"
#include "sp_solve_device.h"

#define SP_CHAIN_STATE 16   // floats of a window's LM state (sp_window_gn_step)

namespace {

struct ChainSeq {                      // per record: what the small kernels of the chain read
    SpWindowNode* t_nodes; const float* t_pose; const float* t_aff; float* out_pose; float* out_aff; float* t_state;
    SpWindowNode* s_nodes; const float* s_pose[2]; const float* s_aff[2]; float* s_state;
    const float* kf_pose; float* rel_pose; const float* crit;
    int32_t t_node, s_node[2], pad_;
};
struct ChainSlotJob { float* a; float* b; const float* t; int64_t n; int32_t bits, pad_; };      // supp_images of one record at one level
struct ChainCopyJob { float* dst; const float* src; int64_t n; };

enum { STAGE_TRACK = 0, STAGE_SUPP = 1 };

// the stage's target nodes (track: one, supp: two; one wave each) <- pose / affine pair from device buffers; tangent and Adam moments
// cleared (optim/window.py set_nodes)
__global__ void k_chain_set_nodes_multi(const ChainSeq* __restrict__ seqs, int stage) {
    const ChainSeq& q = seqs[blockIdx.x];
    const int which = threadIdx.x >> 5, t = threadIdx.x & 31;
    if (which >= (stage == STAGE_TRACK ? 1 : 2)) return;
    SpWindowNode& nd = stage == STAGE_TRACK ? q.t_nodes[q.t_node] : q.s_nodes[q.s_node[which]];
    const float* pose = stage == STAGE_TRACK ? q.t_pose : q.s_pose[which];
    const float* aff = stage == STAGE_TRACK ? q.t_aff : q.s_aff[which];
    if (t < 16) nd.T[t] = pose[t];
    if (t < 6) { nd.a[t] = 0.f; nd.m[t] = 0.f; nd.v[t] = 0.f; }
    if (t < 2) {
        if (aff) nd.aff[t] = aff[t];
        nd.aff_m[t] = 0.f; nd.aff_v[t] = 0.f;
    }
}

// fresh = 1: the state of a new optimisation {lambda, no accepted point, ...}; 0: a new phase of the schedule (optim/window.py
// begin_gn_phase: the accept and convergence tests start afresh, lambda and the iteration count carry over)
__global__ void k_chain_state_multi(const ChainSeq* __restrict__ seqs, int stage, float lam, int fresh) {
    const ChainSeq& q = seqs[blockIdx.x];
    float* st = stage == STAGE_TRACK ? q.t_state : q.s_state;
    const int t = threadIdx.x;
    if (t >= SP_CHAIN_STATE) return;
    if (fresh) st[t] = t == 0 ? lam : (t == 1 ? -1.f : 0.f);
    else if (t == 1) st[t] = -1.f;
    else if (t == 4 || t == 6) st[t] = 0.f;
}

// the tracked node read back out and renormalised (thread 0: the copy, then renormalise_rotation on the copy, as k_renormalise does)
__global__ void k_chain_read_node_multi(const ChainSeq* __restrict__ seqs) {
    const ChainSeq& q = seqs[blockIdx.x];
    if (threadIdx.x != 0) return;
    const SpWindowNode& nd = q.t_nodes[q.t_node];
    for (int t = 0; t < 16; ++t) q.out_pose[t] = nd.T[t];
    if (q.out_aff) { q.out_aff[0] = nd.aff[0]; q.out_aff[1] = nd.aff[1]; }
    renormalise_rotation(q.out_pose);
}

// rel = inv(A) B for rigid A = out_pose, B = kf_pose (lie/lie_algebra.py invertSE3 followed by a matrix product)
__global__ void k_chain_rel_pose_multi(const ChainSeq* __restrict__ seqs) {
    const ChainSeq& q = seqs[blockIdx.x];
    const float* __restrict__ A = q.out_pose;
    const float* __restrict__ B = q.kf_pose;
    const int t = threadIdx.x;
    if (t >= 16) return;
    const int r = t >> 2, c = t & 3;
    float inv[4];                                   // row r of inv(A)
    if (r < 3) {
        inv[0] = A[0 * 4 + r]; inv[1] = A[1 * 4 + r]; inv[2] = A[2 * 4 + r];
        inv[3] = -(inv[0] * A[3] + inv[1] * A[7] + inv[2] * A[11]);
    } else {
        inv[0] = inv[1] = inv[2] = 0.f; inv[3] = 1.f;
    }
    q.rel_pose[t] = inv[0] * B[c] + inv[1] * B[4 + c] + inv[2] * B[8 + c] + inv[3] * B[12 + c];
}

// the supp_images moves of every record and level (job = blockIdx.x): per element first slot 1 -> slot 0, then this frame -> slot 1
__global__ __launch_bounds__(SP_BLOCK) void k_chain_slots_multi(const ChainSlotJob* __restrict__ jobs) {
    const ChainSlotJob& j = jobs[blockIdx.x];
    for (int64_t i = (int64_t)blockIdx.y * SP_BLOCK + threadIdx.x; i < j.n; i += (int64_t)gridDim.y * SP_BLOCK) {
        if (j.bits & 1) j.a[i] = j.b[i];
        if (j.bits & 2) j.b[i] = j.t[i];
    }
}

__global__ __launch_bounds__(SP_BLOCK) void k_chain_copy_multi(const ChainCopyJob* __restrict__ jobs) {
    const ChainCopyJob& j = jobs[blockIdx.x];
    for (int64_t i = (int64_t)blockIdx.y * SP_BLOCK + threadIdx.x; i < j.n; i += (int64_t)gridDim.y * SP_BLOCK) j.dst[i] = j.src[i];
}

// what = 0 / 1: the track / supp windows' 16-float states; 2: the 4 criterion floats
__global__ void k_chain_gather_multi(const ChainSeq* __restrict__ seqs, int n, int what, float* __restrict__ out) {
    const int per = what == 2 ? 4 : SP_CHAIN_STATE;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const ChainSeq& q = seqs[i / per];
    out[i] = (what == 0 ? q.t_state : what == 1 ? q.s_state : q.crit)[i % per];
}

int first_level(const SpChainWindow& w) {
    for (int l = 0; l < SP_CHAIN_LEVELS; ++l) if (w.gn[l].pairs) return l;
    return -1;
}

// byte layout of the device argument area for n records: every array 16-byte aligned
struct ChainLayout {
    size_t img, t_comp, s_comp, seqs, slots, klds, crit, t_args[SP_CHAIN_PHASES], t_lists[SP_CHAIN_PHASES], s_args[SP_CHAIN_PHASES],
        s_lists[SP_CHAIN_PHASES], total;
    explicit ChainLayout(size_t n) {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) / 16 * 16; return at; };
        img = take(sizeof(ChainImgJob) * SP_CHAIN_LEVELS * n);
        t_comp = take(sizeof(ChainComposeJob) * n);
        s_comp = take(sizeof(ChainComposeJob) * n);
        seqs = take(sizeof(ChainSeq) * n);
        slots = take(sizeof(ChainSlotJob) * SP_CHAIN_LEVELS * n);
        klds = take(sizeof(ChainCopyJob) * n);
        crit = take(sizeof(ChainCritJob) * n);
        const size_t wa = (size_t)wgn_multi_args_bytes() * n, wl = sizeof(MultiList) * n;
        for (int p = 0; p < SP_CHAIN_PHASES; ++p) { t_args[p] = take(wa); t_lists[p] = take(wl); }
        for (int p = 0; p < SP_CHAIN_PHASES; ++p) { s_args[p] = take(wa); s_lists[p] = take(wl); }
        total = o;
    }
};

// the schedule and LM constants a stage's windows must share (one phase loop drives them all)
bool same_schedule(const SpChainWindow& a, const SpChainWindow& b) {
    if (a.n_phases != b.n_phases || a.check_every != b.check_every || a.check_first != b.check_first || a.flags != b.flags) return false;
    if (a.lam0 != b.lam0 || a.lm_up != b.lm_up || a.lm_down != b.lm_down || a.lm_min != b.lm_min) return false;
    if (a.n_phases < 0 || a.n_phases > SP_CHAIN_PHASES) return false;
    for (int p = 0; p < a.n_phases; ++p) {
        const SpChainPhase &x = a.phase[p], &y = b.phase[p];
        if (x.level != y.level || x.max_iters != y.max_iters || x.irls_eps != y.irls_eps || x.conv_tol != y.conv_tol) return false;
    }
    return true;
}

// a stage's windows checked, and their per-phase argument records into the staging area
int stage_fill(const SpChainStep* steps, int n, int stage, char* host, const size_t* args_off, const size_t* lists_off, WgnMultiInfo* info) {
    const SpChainWindow& w0 = stage == STAGE_TRACK ? steps[0].track : steps[0].supp;
    if (w0.n_phases < 0 || w0.n_phases > SP_CHAIN_PHASES || w0.check_every <= 0) return SP_EINVAL;
    std::vector<const SpWindowGn*> g(n);
    for (int i = 0; i < n; ++i) {
        const SpChainWindow& w = stage == STAGE_TRACK ? steps[i].track : steps[i].supp;
        if (!same_schedule(w, w0) || !w.state_host || first_level(w) < 0) return SP_EINVAL;
    }
    for (int p = 0; p < w0.n_phases; ++p) {
        const SpChainPhase& ph = w0.phase[p];
        if (ph.level < 0 || ph.level >= SP_CHAIN_LEVELS) return SP_EINVAL;
        for (int i = 0; i < n; ++i) {
            const SpChainWindow& w = stage == STAGE_TRACK ? steps[i].track : steps[i].supp;
            if (!w.gn[ph.level].pairs) return SP_EINVAL;
            g[i] = &w.gn[ph.level];
        }
        if (ph.max_iters <= 0) continue;
        if (int rc = wgn_multi_fill(g.data(), n, w0.flags, w0.lm_up, w0.lm_down, w0.lm_min, ph.conv_tol, true, host + args_off[p],
                                    reinterpret_cast<MultiList*>(host + lists_off[p]), &info[p]))
            return rc;
    }
    return 0;
}

// fresh LM states, then the phases of the stage's schedule over its n windows.  The loop of sp_window_gn_run with the polls that decide
// nothing left out: a look at the states only BETWEEN the iterations of a phase (the last iteration of a phase is followed by the next phase
// whatever the states say); a phase ends once EVERY window froze or at max_iters.  The final states are gathered into the stage's part of
// states_dev; the caller copies them to the host.
int stage_phases(const SpChainWindow& w0, int n, int stage, char* dev, const ChainLayout& L, const WgnMultiInfo* info, float* states_dev,
                 float* states_host, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ChainSeq* seqs = reinterpret_cast<const ChainSeq*>(dev + L.seqs);
    const size_t* args_off = stage == STAGE_TRACK ? L.t_args : L.s_args;
    const size_t* lists_off = stage == STAGE_TRACK ? L.t_lists : L.s_lists;
    float* sd = states_dev + (size_t)stage * SP_CHAIN_STATE * n;
    float* sh = states_host + (size_t)stage * SP_CHAIN_STATE * n;
    hipLaunchKernelGGL(k_chain_state_multi, dim3(n), dim3(64), 0, s, seqs, stage, w0.lam0, 1);
    SP_CHECK_LAUNCH();
    for (int p = 0; p < w0.n_phases; ++p) {
        const SpChainPhase& ph = w0.phase[p];
        if (ph.max_iters <= 0) continue;
        hipLaunchKernelGGL(k_chain_state_multi, dim3(n), dim3(64), 0, s, seqs, stage, 0.f, 0);
        SP_CHECK_LAUNCH();
        int it = 0;
        int look = (w0.check_first > 0 && ph.conv_tol > 0.f) ? w0.check_first : w0.check_every;
        while (it < ph.max_iters) {
            const int k_n = (ph.max_iters - it) < look ? (ph.max_iters - it) : look;
            for (int k = 0; k < k_n; ++k, ++it)
                if (int rc = wgn_multi_round(dev + args_off[p], reinterpret_cast<const MultiList*>(dev + lists_off[p]), n, info[p], w0.flags,
                                             ph.irls_eps, stream))
                    return rc;
            if (it >= ph.max_iters || !(ph.conv_tol > 0.f)) continue;
            hipLaunchKernelGGL(k_chain_gather_multi, dim3((n * SP_CHAIN_STATE + 255) / 256), dim3(256), 0, s, seqs, n, stage, sd);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(sh, sd, sizeof(float) * SP_CHAIN_STATE * n, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return (int)e;
            bool all = true;
            for (int i = 0; i < n && all; ++i) all = static_cast<volatile float*>(sh)[i * SP_CHAIN_STATE + 6] != 0.f;
            if (all) break;
            look = w0.check_every;
        }
    }
    hipLaunchKernelGGL(k_chain_gather_multi, dim3((n * SP_CHAIN_STATE + 255) / 256), dim3(256), 0, s, seqs, n, stage, sd);
    SP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int sp_chain_multi_bytes(void) { return (int)ChainLayout(1).total; }

extern "C" int sp_chain_step_multi(SpChainStep* steps, int n, void* args_dev, float* states_dev, float* states_host, void* stream) {
    // ---- validation: one homogeneous call, every record checked; nothing is launched before it passed
    if (!steps || n < 1 || n > 65535 || !args_dev || !states_dev || !states_host) return SP_EINVAL;
    const SpChainStep& s0 = steps[0];
    const int stages = s0.stages;
    if (stages & ~(SP_CHAIN_TRACK | SP_CHAIN_SUPP | SP_CHAIN_CRITERION)) return SP_EINVAL;
    if (s0.n_levels < 1 || s0.n_levels > SP_CHAIN_LEVELS || s0.H <= 0 || s0.W <= 0) return SP_EINVAL;
    for (int i = 0; i < n; ++i) {
        const SpChainStep& st = steps[i];
        if (st.stages != stages || st.H != s0.H || st.W != s0.W || st.n_levels != s0.n_levels) return SP_EINVAL;
    }
    int Hl[SP_CHAIN_LEVELS], Wl[SP_CHAIN_LEVELS];
    Hl[0] = s0.H; Wl[0] = s0.W;
    for (int l = 1; l < SP_CHAIN_LEVELS; ++l) { Hl[l] = (Hl[l - 1] + 1) / 2; Wl[l] = (Wl[l - 1] + 1) / 2; }
    if ((stages & SP_CHAIN_TRACK) && s0.n_levels > 1 && (s0.H < 2 || s0.W < 2)) return SP_EINVAL;

    const ChainLayout L((size_t)n);
    std::vector<char> host(L.total, 0);
    ChainSeq* seqs = reinterpret_cast<ChainSeq*>(host.data() + L.seqs);
    WgnMultiInfo t_info[SP_CHAIN_PHASES] = {}, s_info[SP_CHAIN_PHASES] = {};
    int max_P = 0;
    if (stages & SP_CHAIN_TRACK) {
        if (int rc = stage_fill(steps, n, STAGE_TRACK, host.data(), L.t_args, L.t_lists, t_info)) return rc;
        ChainImgJob* img = reinterpret_cast<ChainImgJob*>(host.data() + L.img);
        ChainComposeJob* comp = reinterpret_cast<ChainComposeJob*>(host.data() + L.t_comp);
        for (int i = 0; i < n; ++i) {
            const SpChainStep& st = steps[i];
            const SpChainWindow& w = st.track;
            const SpChainTarget& tg = st.track_target;
            const int l0 = first_level(w);
            if (!st.image || !tg.pose || !st.out_pose || tg.node < 0 || tg.node >= w.gn[l0].n_nodes) return SP_EINVAL;
            for (int l = 0; l < st.n_levels; ++l) {
                if (l > 0 && !st.level[l]) return SP_EINVAL;
                const float* in = (l <= 1) ? st.image : st.level[l - 1];          // (level 0 packs the frame, level l blurs level l - 1)
                img[(size_t)l * n + i] = ChainImgJob{in, l == 0 ? nullptr : st.level[l], tg.packed[l]};
            }
            const SpWindowGn& g = w.gn[l0];
            if (!g.pairs || !g.edges || !g.nodes || g.n_edges <= 0 || g.n_nodes <= 0) return SP_EINVAL;
            if (g.n_edges > chain_compose_max_edges()) return SP_ELIMIT;
            comp[i] = ChainComposeJob{g.pairs, g.edges, g.nodes, g.n_edges, g.n_nodes};
            seqs[i].t_nodes = g.nodes; seqs[i].t_node = tg.node; seqs[i].t_pose = tg.pose; seqs[i].t_aff = tg.aff;
            seqs[i].out_pose = st.out_pose; seqs[i].out_aff = st.out_aff; seqs[i].t_state = g.state;
        }
    }
    if (stages & SP_CHAIN_SUPP) {
        if (int rc = stage_fill(steps, n, STAGE_SUPP, host.data(), L.s_args, L.s_lists, s_info)) return rc;
        ChainSlotJob* slots = reinterpret_cast<ChainSlotJob*>(host.data() + L.slots);
        ChainComposeJob* comp = reinterpret_cast<ChainComposeJob*>(host.data() + L.s_comp);
        ChainCopyJob* klds = reinterpret_cast<ChainCopyJob*>(host.data() + L.klds);
        for (int i = 0; i < n; ++i) {
            const SpChainStep& st = steps[i];
            const SpChainWindow& w = st.supp;
            const int l0 = first_level(w);
            const SpWindowGn& g = w.gn[l0];
            const SpChainTarget& a = st.supp_target[0];
            const SpChainTarget& b = st.supp_target[1];
            if (!a.pose || !b.pose || a.node < 0 || b.node < 0 || a.node >= g.n_nodes || b.node >= g.n_nodes) return SP_EINVAL;
            for (int l = 0; l < SP_CHAIN_LEVELS; ++l) {
                ChainSlotJob& j = slots[(size_t)l * n + i];
                j = ChainSlotJob{a.packed[l], b.packed[l], st.track_target.packed[l], 0, 0, 0};
                if (!w.gn[l].pairs) continue;
                if ((st.supp_images & 1) && (!a.packed[l] || !b.packed[l])) return SP_EINVAL;
                if ((st.supp_images & 2) && (!b.packed[l] || !st.track_target.packed[l])) return SP_EINVAL;
                j.n = 3 * (int64_t)Hl[l] * Wl[l];
                j.bits = st.supp_images & 3;
            }
            if (!g.pairs || !g.edges || !g.nodes || g.n_edges <= 0 || g.n_nodes <= 0) return SP_EINVAL;
            if (g.n_edges > chain_compose_max_edges()) return SP_ELIMIT;
            comp[i] = ChainComposeJob{g.pairs, g.edges, g.nodes, g.n_edges, g.n_nodes};
            if (st.kld_n > 0 && (!st.kld_src || !st.kld_dst)) return SP_EINVAL;
            klds[i] = ChainCopyJob{st.kld_dst, st.kld_src, st.kld_n > 0 ? (int64_t)st.kld_n : 0};
            seqs[i].s_nodes = g.nodes; seqs[i].s_state = g.state;
            for (int j = 0; j < 2; ++j) {
                seqs[i].s_node[j] = st.supp_target[j].node; seqs[i].s_pose[j] = st.supp_target[j].pose; seqs[i].s_aff[j] = st.supp_target[j].aff;
            }
        }
    }
    if (stages & SP_CHAIN_CRITERION) {
        ChainCritJob* crit = reinterpret_cast<ChainCritJob*>(host.data() + L.crit);
        for (int i = 0; i < n; ++i) {
            const SpChainStep& st = steps[i];
            if (!st.out_pose || !st.kf_pose || !st.rel_pose || !st.crit || !st.crit_ws || !st.crit_host || !st.depth_out || !st.keys) return SP_EINVAL;
            if (!st.pix || !st.baseL || !st.seg_off || !st.kp_L || !st.kld || !st.K || st.N <= 0 || st.P <= 0) return SP_EINVAL;
            if (st.valid_thresh != s0.valid_thresh || !(st.valid_thresh >= 0.f)) return SP_EINVAL;
            crit[i] = ChainCritJob{st.pix, st.baseL, st.seg_off, st.kp_L, st.kld, st.K, st.rel_pose, st.out_pose, st.kf_pose, st.keys, st.depth_out,
                                   st.crit_ws, st.crit, st.N, st.P};
            seqs[i].out_pose = st.out_pose; seqs[i].kf_pose = st.kf_pose; seqs[i].rel_pose = st.rel_pose; seqs[i].crit = st.crit;
            max_P = st.P > max_P ? st.P : max_P;
        }
    }

    // ---- the records to the device (one copy), then the stages
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* dev = static_cast<char*>(args_dev);
    const ChainSeq* seqs_dev = reinterpret_cast<const ChainSeq*>(dev + L.seqs);
    hipError_t e = hipMemcpyAsync(dev, host.data(), L.total, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return (int)e;

    if (stages & SP_CHAIN_TRACK) {
        if (int rc = chain_pyramid_multi(reinterpret_cast<const ChainImgJob*>(dev + L.img), n, s0.n_levels, s0.H, s0.W, stream)) return rc;
        hipLaunchKernelGGL(k_chain_set_nodes_multi, dim3(n), dim3(64), 0, s, seqs_dev, (int)STAGE_TRACK);
        SP_CHECK_LAUNCH();
        if (int rc = chain_compose_multi(reinterpret_cast<const ChainComposeJob*>(dev + L.t_comp), n, stream)) return rc;
        if (int rc = stage_phases(s0.track, n, STAGE_TRACK, dev, L, t_info, states_dev, states_host, stream)) return rc;
        hipLaunchKernelGGL(k_chain_read_node_multi, dim3(n), dim3(64), 0, s, seqs_dev);
        SP_CHECK_LAUNCH();
    }
    if (stages & SP_CHAIN_SUPP) {
        int64_t max_slot = 0, max_kld = 0;
        for (int l = 0; l < SP_CHAIN_LEVELS; ++l) if (s0.supp.gn[l].pairs) max_slot = std::max<int64_t>(max_slot, 3 * (int64_t)Hl[l] * Wl[l]);
        for (int i = 0; i < n; ++i) max_kld = std::max<int64_t>(max_kld, steps[i].kld_n);
        const unsigned gs = (unsigned)std::min<int64_t>((max_slot + SP_BLOCK - 1) / SP_BLOCK, 256);
        if (gs > 0) {
            hipLaunchKernelGGL(k_chain_slots_multi, dim3(SP_CHAIN_LEVELS * n, gs), dim3(SP_BLOCK), 0, s, reinterpret_cast<const ChainSlotJob*>(dev + L.slots));
            SP_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_chain_set_nodes_multi, dim3(n), dim3(64), 0, s, seqs_dev, (int)STAGE_SUPP);
        SP_CHECK_LAUNCH();
        if (int rc = chain_compose_multi(reinterpret_cast<const ChainComposeJob*>(dev + L.s_comp), n, stream)) return rc;
        if (int rc = stage_phases(s0.supp, n, STAGE_SUPP, dev, L, s_info, states_dev, states_host, stream)) return rc;
        const unsigned gk = (unsigned)std::min<int64_t>((max_kld + SP_BLOCK - 1) / SP_BLOCK, 64);
        if (gk > 0) {
            hipLaunchKernelGGL(k_chain_copy_multi, dim3(n, gk), dim3(SP_BLOCK), 0, s, reinterpret_cast<const ChainCopyJob*>(dev + L.klds));
            SP_CHECK_LAUNCH();
        }
    }
    if (stages & SP_CHAIN_CRITERION) {
        hipLaunchKernelGGL(k_chain_rel_pose_multi, dim3(n), dim3(64), 0, s, seqs_dev);
        SP_CHECK_LAUNCH();
        if (int rc = chain_criterion_multi(reinterpret_cast<const ChainCritJob*>(dev + L.crit), n, max_P, s0.H, s0.W, s0.valid_thresh, stream)) return rc;
        hipLaunchKernelGGL(k_chain_gather_multi, dim3((n * 4 + 255) / 256), dim3(256), 0, s, seqs_dev, n, 2, states_dev + (size_t)2 * SP_CHAIN_STATE * n);
        SP_CHECK_LAUNCH();
    }
    // ---- one copy of what the host reads (the windows' final states, the criteria), one synchronisation
    if (stages) {
        e = hipMemcpyAsync(states_host, states_dev, sizeof(float) * (2 * SP_CHAIN_STATE + 4) * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return (int)e;
    }
    const volatile float* sh = states_host;
    for (int i = 0; i < n; ++i) {
        SpChainStep& st = steps[i];
        if (stages & SP_CHAIN_TRACK) {
            float* dst = static_cast<float*>(st.track.state_host);
            for (int k = 0; k < SP_CHAIN_STATE; ++k) dst[k] = sh[(size_t)i * SP_CHAIN_STATE + k];
            st.track_iters = (int)dst[5];
        }
        if (stages & SP_CHAIN_SUPP) {
            float* dst = static_cast<float*>(st.supp.state_host);
            for (int k = 0; k < SP_CHAIN_STATE; ++k) dst[k] = sh[(size_t)(n + i) * SP_CHAIN_STATE + k];
            st.supp_iters = (int)dst[5];
        }
        if (stages & SP_CHAIN_CRITERION)
            for (int k = 0; k < 4; ++k) st.crit_host[k] = sh[(size_t)2 * SP_CHAIN_STATE * n + 4 * i + k];
    }
    return 0;
}
