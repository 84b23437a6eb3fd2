"""-m gpu: the many-pairs path (sp_pairs_cost + sp_pairs_adam_step / sp_pairs_gn_step) through the C ABI.

* mode-0 partials and the on-device Adam step against the oracle's autograd + torch.optim.Adam loop;
* mode-1 (Gauss-Newton) normal equations against the oracle's finite-difference Jacobian of the reference residual;
* the LM solver: monotone cost over accepted steps, convergence to the synthetic ground truth within
  BASELINE.json's tolerances (pose 1e-4 rad / 1e-4 t at convergence is checked against ground truth, depth 1e-3 rel);
* full-size (640x480x64) properties: agreement with the oracle residual, determinism, replica consistency.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import T, frames_from_golden, npy

pytestmark = pytest.mark.gpu
ADAM_KLD_TOL, ADAM_POSE_TOL = 2.5e-5, 5e-5     # ~5x the measured 4.2e-6 / 9.3e-6 after 12 steps (profiles/r02_parity.txt)


def make_batch(pairs, **kw):
    from super_primitive_amd.optim.pair_batch import PairBatch
    return PairBatch.from_synth(pairs, device="cuda:0", **kw)


def assemble_gn(batch, level=0, eps=1e-3):
    """Host-side reduction of the mode-1 partials (span records + segment records) into per-pair dense (6+N) systems
    (float64)."""
    from super_primitive_amd import _lib
    batch.cost_pass(level, 1, eps)
    torch.cuda.synchronize()
    NV, NS = _lib.SP_GN_PARTIAL_FLOATS, _lib.SP_GN_SEG_FLOATS
    span = npy(batch.partials[: batch.n_spans * NV]).reshape(-1, NV).astype(np.float64)
    span_pair = npy(batch.span_pair)
    segp = npy(batch.seg_partials[: batch.n_seg_records * NS]).reshape(-1, NS).astype(np.float64)
    seg_rec = npy(batch.seg_records)
    out = []
    iu = np.triu_indices(6)
    for m in range(batch.M):
        N = batch.Ns[m]
        H = np.zeros((6 + N, 6 + N))
        b = np.zeros(6 + N)
        p = span[span_pair == m].sum(0)
        Hpp = np.zeros((6, 6))
        Hpp[iu] = p[1:22]
        H[:6, :6] = Hpp + np.triu(Hpp, 1).T
        b[:6] = p[22:28]
        for r in np.nonzero(seg_rec[:, 0] == m)[0]:
            seg = seg_rec[r, 1]
            q = segp[r]
            H[:6, 6 + seg] += q[0:6]
            H[6 + seg, :6] += q[0:6]
            H[6 + seg, 6 + seg] += q[6]
            b[6 + seg] += q[7]
        mine = segp[seg_rec[:, 0] == m]
        out.append(dict(H=H, b=b, cost=p[0] / (3.0 * batch.Ps[m]), n_valid=p[28], seg_abs_sum=mine[:, 8].sum(), seg_valid_sum=mine[:, 9].sum(), abs_sum=p[0]))
    return out


def rot_angle(R):
    R = np.asarray(R, np.float64)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])     # sin(angle) * axis: exact for small angles
    return float(np.arctan2(np.linalg.norm(w), (np.trace(R) - 1) / 2))


@pytest.mark.parametrize("shape,seed", [("grid", 3), ("blobs", 4)])
def test_gn_normal_equations_match_oracle_jacobian(shape, seed):
    from oracle import gn_oracle, photometric_oracle as orc
    from super_primitive_amd import synth
    pairs = [synth.make_pair(48, 64, 6, seed=seed + k, shape=shape, init_sigma=0.01) for k in range(2)]
    batch = make_batch(pairs, levels=(0, 1), tile_points=512)
    got = assemble_gn(batch)
    for m, p in enumerate(pairs):
        src, trg = orc.frames_from_synth(p)
        want = gn_oracle.normal_equations(src, trg, torch.from_numpy(p.kld_init), torch.from_numpy(p.pose_init), eps=1e-3)
        H, b = want["H"].numpy(), want["b"].numpy()
        assert abs(got[m]["n_valid"] - want["n_valid"]) <= 2
        np.testing.assert_allclose(got[m]["cost"], want["cost"], rtol=2e-5)
        # blockwise scaling: the pose block, the coupling and the depth diagonal live on very different scales
        for sl, name in ((np.s_[:6, :6], "H_pp"), (np.s_[:6, 6:], "H_pd"), (np.s_[6:, 6:], "H_dd")):
            scale = np.abs(H[sl]).max()
            assert np.abs(got[m]["H"][sl] - H[sl]).max() <= 3e-3 * scale, name
        assert np.abs(got[m]["b"][:6] - b[:6]).max() <= 3e-3 * np.abs(b[:6]).max()
        assert np.abs(got[m]["b"][6:] - b[6:]).max() <= 3e-3 * np.abs(b[6:]).max()


def test_spans_over_tiny_single_pixel_and_empty_segments():
    """The padded tables and span loops on a VOID-like keyframe: 150 segments, some of one pixel (255 padding points per
    real one), some empty (no chunk at all), most a few hundred pixels, so that one workgroup streams through dozens of
    segments: residual and GN system against the oracle, empty segments untouched by an LM step."""
    from oracle import gn_oracle, photometric_oracle as orc
    from super_primitive_amd import synth
    p = synth.make_pair(60, 88, 150, seed=12, shape="blobs")
    m = p.keypoint_regions
    m &= np.random.default_rng(5).uniform(size=m.shape) < 0.25          # thin the ellipses out: a few hundred pixels each
    for n in range(150):
        m[n, p.meta["kp_rc"][n, 0], p.meta["kp_rc"][n, 1]] = True
    for n in range(0, 150, 7):
        m[n] = False
        m[n, p.meta["kp_rc"][n, 0], p.meta["kp_rc"][n, 1]] = True          # single pixel
    empty = list(range(3, 150, 25))
    for n in empty:
        m[n] = False
    p.logdepth_perseg[~m] = 0
    batch = make_batch([p, p], levels=(0, 1), tile_points=512, span_points=16384)
    assert batch.n_spans < batch.n_chunks / 8 and batch.Ppads[0] > 1.5 * batch.Ps[0]
    got = assemble_gn(batch)
    src, trg = orc.frames_from_synth(p)
    want = gn_oracle.normal_equations(src, trg, torch.from_numpy(p.kld_init), torch.from_numpy(p.pose_init), eps=1e-3)
    H, b = want["H"].numpy(), want["b"].numpy()
    for g in got:
        assert abs(g["n_valid"] - want["n_valid"]) <= 2
        np.testing.assert_allclose(g["cost"], want["cost"], rtol=2e-5)
        for sl, name in ((np.s_[:6, :6], "H_pp"), (np.s_[:6, 6:], "H_pd"), (np.s_[6:, 6:], "H_dd")):
            assert np.abs(g["H"][sl] - H[sl]).max() <= 3e-3 * np.abs(H[sl]).max(), name
        assert np.abs(g["b"] - b).max() <= 3e-3 * np.abs(b).max()
        assert np.all(g["H"][6 + np.array(empty)] == 0) and np.all(g["b"][6 + np.array(empty)] == 0)
    np.testing.assert_allclose(npy(batch.evaluate(0)), [want["cost"]] * 2, rtol=2e-5)
    k0 = torch.cat(batch.klds()).clone()
    for _ in range(3):
        batch.gn_step(0)
    k1 = torch.cat(batch.klds())
    idx = torch.tensor(empty + [150 + e for e in empty], device=k1.device)
    assert torch.equal(k1[idx], k0[idx]) and not torch.equal(k1, k0)


def test_gn_converges_to_ground_truth():
    """Coarse-to-fine LM on rendered pairs: cost drops by > 10x, pose and keypoint depths reach the ground truth."""
    from super_primitive_amd import synth
    pairs = [synth.make_pair(96, 128, 8, seed=40 + k, init_sigma=0.01, overlap=2) for k in range(3)]
    batch = make_batch(pairs, levels=(0, 3))
    c_first = batch.evaluate(0).clone()
    batch.run(12, mode="gn")
    for _ in range(10):
        batch.gn_step(0, irls_eps=1e-4)
    c_last = batch.evaluate(0)
    torch.cuda.synchronize()
    assert bool((c_last < 0.1 * c_first).all()), (c_first.tolist(), c_last.tolist())
    poses = npy(batch.poses())
    klds = [npy(k) for k in batch.klds()]
    for m, p in enumerate(pairs):
        dR = poses[m][:3, :3] @ p.pose_gt[:3, :3].T
        # the global scale of a two-view reconstruction is a gauge freedom: compare after fixing it
        s = np.exp(np.median(klds[m] - p.kld_gt))
        assert rot_angle(dR) < 2e-3, rot_angle(dR)
        assert np.abs(poses[m][:3, 3] / s - p.pose_gt[:3, 3]).max() < 5e-3
        np.testing.assert_allclose(klds[m] - np.log(s), p.kld_gt, atol=5e-3)


def test_gn_reaches_the_minimiser_of_the_reference_cost():
    """The reference has no Gauss-Newton solver, so the LM path is pinned at its fixed point: golden g12 holds the
    minimiser of the REAL reference cost (its own two-frame Adam loop run to convergence, then polished with decayed
    learning rates, oracle/gen_goldens.py).  IRLS with a small epsilon minimises the same L1 cost: it must reach the same
    cost and, modulo the two-view scale gauge, the same pose and log-depths -- measured on MI355X: cost ratio 1.00000,
    2.8e-6 rad, 6.4e-6 t, 5.9e-5 log-depth (north-star bar: 1e-4 rad / 1e-4 t / 1e-3 depth)."""
    from super_primitive_amd.optim.pair_batch import PairBatch
    g = load_golden("g12_converged_sfm")
    src, trg = frames_from_golden(g)
    batch = PairBatch([src], [trg.image], [trg.K], T(g["in_pose_init"])[None].clone(), [T(g["in_kld"]).clone()], levels=(0, 3))
    batch.run(15, mode="gn", polish_iters=40, polish_eps=1e-5)
    cost = float(batch.evaluate(0)[0])
    assert cost <= float(g["final_loss"]) * (1 + 2e-5), (cost, float(g["final_loss"]))
    P, k = npy(batch.poses())[0].astype(np.float64), npy(batch.klds()[0]).astype(np.float64)
    Pr, kr = g["final_pose"].astype(np.float64), g["final_kld"].astype(np.float64)
    s = np.exp(np.mean(k - kr))                                  # scale gauge of a two-view reconstruction
    assert rot_angle(P[:3, :3].T @ Pr[:3, :3]) < 3e-5
    assert np.abs(P[:3, 3] / s - Pr[:3, 3]).max() < 5e-5
    assert np.abs(k - np.log(s) - kr).max() < 3e-4


def test_lm_never_accepts_a_cost_increase():
    from super_primitive_amd import synth
    pairs = [synth.make_pair(60, 80, 6, seed=50 + k, init_sigma=0.03) for k in range(4)]
    batch = make_batch(pairs, levels=(0, 1))
    accepted = []
    for _ in range(25):
        batch.gn_step(0)
        accepted.append(npy(batch.lm_state[:, 1]).copy())
    acc = np.stack(accepted)
    assert np.all(np.diff(acc, axis=0) <= 1e-6 * np.abs(acc[:-1]) + 1e-12), "accepted cost must be non-increasing"
    st = npy(batch.lm_state)
    assert np.all(st[:, 2] > 5)          # steps were accepted
    assert np.all(st[:, 0] > 0)          # lambda stays positive


def test_adam_step_matches_oracle_loop():
    """K reset-tangent Adam steps (odometery.py:394-403 flavour) on device vs autograd + torch.optim.Adam on the oracle."""
    from oracle import photometric_oracle as orc
    from super_primitive_amd import synth
    K = 12
    pairs = [synth.make_pair(48, 64, 6, seed=60 + k, init_sigma=0.01) for k in range(2)]
    batch = make_batch(pairs, levels=(0, 1), tile_points=512)
    losses = []
    for _ in range(K):
        losses.append(npy(batch.adam_step(0, lr_kld=1e-3, lr_pose=1e-2)).copy())
    torch.cuda.synchronize()
    got_pose, got_kld = npy(batch.poses()), [npy(k) for k in batch.klds()]
    for m, p in enumerate(pairs):
        src, trg = orc.frames_from_synth(p)
        kld = torch.nn.Parameter(torch.from_numpy(p.kld_init.copy()))
        delta = torch.nn.Parameter(torch.zeros(1, 6))
        pose = torch.from_numpy(p.pose_init.copy())
        opt = torch.optim.Adam([{"params": [kld], "lr": 1e-3}, {"params": [delta], "lr": 1e-2}], lr=1e-3)
        ref_losses = []
        for _ in range(K):
            out = orc.photometric_cost(src, trg, kld, orc.se3_exp(delta)[0] @ pose)
            loss = out["residual"].abs().mean()
            ref_losses.append(float(loss))
            loss.backward()
            opt.step()
            opt.zero_grad()
            with torch.no_grad():
                pose = orc.se3_exp(delta.detach())[0] @ pose
                delta.data.zero_()
        # Adam's first steps are sign-like (m/sqrt(v) ~ +-1): fp32-noise-level gradient differences on entries
        # near zero are amplified to O(lr) parameter differences, so trajectories are compared at lr scale
        # (SURVEY.md §8(c) "Tolerances"); the first loss values, before any amplification, must agree tightly.
        np.testing.assert_allclose([l[m] for l in losses][:3], ref_losses[:3], rtol=2e-5)
        print(f"adam-step parity pair {m}: loss rel {np.abs(np.array([l[m] for l in losses]) / np.array(ref_losses) - 1).max():.2e} "
              f"kld {np.abs(got_kld[m] - kld.detach().numpy()).max():.2e} pose {np.abs(got_pose[m] - pose.numpy()).max():.2e}")
        np.testing.assert_allclose([l[m] for l in losses], ref_losses, rtol=3e-3)
        np.testing.assert_allclose(got_kld[m], kld.detach().numpy(), atol=ADAM_KLD_TOL)
        np.testing.assert_allclose(got_pose[m], pose.numpy(), atol=ADAM_POSE_TOL)


def test_evaluate_matches_single_pair_api():
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim
    from gpu_util import frames_from_synth
    pairs = [synth.make_pair(60, 80, 6, seed=70 + k, shape="blobs" if k else "grid") for k in range(3)]
    batch = make_batch(pairs, levels=(0, 2))
    for level in (0, 1):
        res = npy(batch.evaluate(level))
        for m, p in enumerate(pairs):
            from super_primitive_amd.image.keyframe import keyframe_pyramid
            src, trg = frames_from_synth(p)
            s_l = keyframe_pyramid(src, 0, 2)[::-1][level]
            t_l = keyframe_pyramid(trg, 0, 2)[::-1][level]
            out = dense_optim.photomeric_cost(s_l, t_l, T(p.kld_init), T(p.pose_init), {"mode": "colour", "collect_stats": 0})
            np.testing.assert_allclose(res[m], npy(out["residual"])[0], rtol=3e-6)


# ---------------------------------------------------------------------------------------------------------
# BASELINE.json full size: 640 x 480, 64 segments
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_size():
    from super_primitive_amd import synth
    pair = synth.make_pair(480, 640, 64, seed=7, overlap=4, init_sigma=0.004)
    batch = make_batch([pair], levels=(0, 3), replicate=3)
    return pair, batch


def test_full_size_residual_matches_oracle(full_size):
    from oracle import photometric_oracle as orc
    pair, batch = full_size
    src, trg = orc.frames_from_synth(pair)
    want = float(orc.photometric_cost(src, trg, torch.from_numpy(pair.kld_init), torch.from_numpy(pair.pose_init))["residual"])
    got = npy(batch.evaluate(0))
    np.testing.assert_allclose(got, want, rtol=2e-5)
    assert got[0] == got[1] == got[2], "replicas of one pair must agree bitwise"


def test_full_size_bitwise_determinism_and_descent(full_size):
    from super_primitive_amd import _lib
    pair, batch = full_size
    n = batch.n_spans * _lib.SP_GN_PARTIAL_FLOATS
    batch.cost_pass(0, 1)
    a, sa = batch.partials[:n].clone(), batch.seg_partials.clone()
    batch.cost_pass(0, 1)
    assert torch.equal(a, batch.partials[:n]) and torch.equal(sa, batch.seg_partials), \
        "two launches on the same inputs must be bitwise identical"
    c0 = batch.evaluate(0).clone()
    batch.reset_lm()
    batch.run(6, mode="gn")
    c1 = batch.evaluate(0)
    assert bool((c1 < 0.5 * c0).all()), (c0.tolist(), c1.tolist())
    poses = npy(batch.poses())
    assert np.array_equal(poses[0], poses[1]) and np.array_equal(poses[1], poses[2])
    klds = [npy(k) for k in batch.klds()]
    s = np.exp(np.median(klds[0] - pair.kld_gt))
    assert rot_angle(poses[0][:3, :3] @ pair.pose_gt[:3, :3].T) < 1e-3
    np.testing.assert_allclose(klds[0] - np.log(s), pair.kld_gt, atol=3e-3)


def test_hipgraph_replay_matches_eager_iterations():
    """The two-launch iteration captured in a hipGraph gives bitwise the same trajectory as eager launches."""
    from super_primitive_amd import synth
    pairs = [synth.make_pair(60, 80, 6, seed=90 + k, init_sigma=0.02) for k in range(3)]
    a = make_batch(pairs, levels=(0, 2))
    b = make_batch(pairs, levels=(0, 2))
    a.run(6, mode="gn")
    b.run(6, mode="gn", use_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(a.pose, b.pose) and torch.equal(a.kld, b.kld)
    assert torch.equal(a.lm_state, b.lm_state)


def test_full_size_segment_permutation_and_tile_size_invariance():
    """Size-independent properties at 640x480x64: relabelling the segments permutes d/dkld and leaves residual and
    d/dpose unchanged (up to fp32 summation order); so does changing the tile size of the work list."""
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.segment_table import table_of
    pair = synth.make_pair(480, 640, 64, seed=8, overlap=4, init_sigma=0.004)
    cfg = {"mode": "colour", "collect_stats": 0}
    perm = np.random.default_rng(0).permutation(64)

    def run(order, tile_points):
        src = KeyFrame(T(pair.src_image), T(pair.K), T(pair.logdepth_perseg[order]), T(pair.keypoints[order]),
                       T(pair.keypoint_regions[order]))
        trg = KeyFrame(T(pair.trg_image), T(pair.K))
        table_of(src, tile_points=tile_points)
        kld, pose = T(pair.kld_init[order], True), T(pair.pose_init, True)
        out = dense_optim.photomeric_cost(src, trg, kld, pose, cfg)
        out["residual"].sum().backward()
        return npy(out["residual"])[0], npy(kld.grad), npy(pose.grad)

    ident = np.arange(64)
    r0, gk0, gp0 = run(ident, 1024)
    r1, gk1, gp1 = run(perm, 1024)
    r2, gk2, gp2 = run(ident, 4096)
    for r, gk, gp, order in ((r1, gk1, gp1, perm), (r2, gk2, gp2, ident)):
        np.testing.assert_allclose(r, r0, rtol=3e-6)
        assert np.abs(gk - gk0[order]).max() <= 1e-4 * np.abs(gk0).max()
        assert np.abs(gp - gp0).max() <= 1e-4 * np.abs(gp0).max()


def test_backward_is_linear_in_the_upstream_gradient():
    """loss = sum_b w_b * residual_b: gradients must be the w-weighted sums of the per-target gradients."""
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim_batch
    from gpu_util import frames_from_synth
    pair = synth.make_pair(60, 80, 6, seed=33)
    other = synth.make_pair(60, 80, 6, seed=33, motion_scale=1.7)
    src, _ = frames_from_synth(pair)
    imgs, Ks = T(np.stack([pair.trg_image, other.trg_image])), T(np.stack([pair.K, pair.K]))
    poses0 = np.stack([pair.pose_init, other.pose_init])
    cfg = {"mode": "colour", "collect_stats": 0}

    def grads(w):
        kld, P = T(pair.kld_init, True), T(poses0, True)
        out = dense_optim_batch.photomeric_cost_batch(src, imgs, Ks, kld, P, cfg)
        (out["residual"] * T(np.asarray(w, np.float32))).sum().backward()
        return npy(kld.grad), npy(P.grad)

    k10, p10 = grads([1, 0])
    k01, p01 = grads([0, 1])
    k, p = grads([0.3, -2.0])
    np.testing.assert_allclose(k, 0.3 * k10 - 2.0 * k01, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(p, 0.3 * p10 - 2.0 * p01, rtol=1e-5, atol=1e-9)
    assert np.all(p10[1] == 0) and np.all(p01[0] == 0)


@pytest.mark.parametrize("mode", ["gn", "adam"])
def test_iterations_on_log_depth_tables_are_bitwise_repeatable(mode):
    """Two batches built from the same pairs run the same iterations (sp_pairs_cost + sp_pairs_*_step): with many pairs of
    uneven size in flight, every partial sum is taken in a fixed order, so costs and state agree bit for bit."""
    from super_primitive_amd import synth
    pairs = [synth.make_pair(60 + 12 * (k % 3), 80 + 8 * (k % 4), 4 + k % 5, seed=100 + k, init_sigma=0.02,
                             shape="blobs" if k % 2 else "grid") for k in range(24)]
    a = make_batch(pairs, levels=(0, 1), tile_points=512, depth_table=False)
    b = make_batch(pairs, levels=(0, 1), tile_points=512, depth_table=False)
    for it in range(15):
        if mode == "gn":
            ca, cb = a.gn_step(0), b.gn_step(0)
        else:
            ca, cb = a.adam_step(0), b.adam_step(0)
        assert torch.equal(ca, cb), it
    torch.cuda.synchronize()
    assert torch.equal(a.pose, b.pose) and torch.equal(a.kld, b.kld)
    if mode == "gn":
        assert torch.equal(a.lm_state, b.lm_state)


def test_results_do_not_depend_on_how_chunks_are_grouped_into_spans():
    """One workgroup per chunk, a few chunks per workgroup, or a whole pair per workgroup: the pair-level sums change
    their summation tree (fp32 noise), the per-segment sums are produced per chunk and wave and must be bitwise equal;
    short chunks exercise a flush in almost every trip, ragged blob segments the padding."""
    from super_primitive_amd import _lib, synth
    pairs = [synth.make_pair(72, 96, 7, seed=150 + k, init_sigma=0.01, shape="blobs" if k else "grid") for k in range(3)]
    want = None
    for span_points in (256, 2048, 1 << 20):
        batch = make_batch(pairs, levels=(0, 1), tile_points=512, span_points=span_points)
        systems = assemble_gn(batch)
        batch.cost_pass(0, 1, 1e-3)
        seg_cols = batch.seg_partials.clone()
        g = batch.evaluate(0).clone()
        if want is None:
            want = (systems, seg_cols, g)
            assert batch.n_spans == batch.n_chunks
            continue
        assert batch.n_spans < batch.n_chunks and batch.n_chunks * 4 == batch.n_seg_records
        # (ABI 13: a segment record is 12 floats -- [0..7] the Gauss-Newton sums, produced per chunk and wave: bitwise; [8], [9] the
        #  record's own sum |r| and valid points, taken as DIFFERENCES of the span's running sums: fp32 noise of the sum |r|, the count exact;
        #  [10], [11] unused)
        NS = _lib.SP_GN_SEG_FLOATS
        sc, sw = seg_cols.reshape(-1, NS), want[1].reshape(-1, NS)
        assert torch.equal(sc[:, :8], sw[:, :8]) and torch.equal(sc[:, 9], sw[:, 9])
        np.testing.assert_allclose(npy(sc[:, 8]), npy(sw[:, 8]), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(npy(g), npy(want[2]), rtol=2e-6)
        for a, b in zip(systems, want[0]):
            # the per-segment cost columns add up to the pair's own sums (what the verdict's within-pair test relies on)
            assert a["seg_valid_sum"] == a["n_valid"] and abs(a["seg_abs_sum"] - a["abs_sum"]) <= 1e-4 * a["abs_sum"]
            scale = np.abs(b["H"]).max()
            assert np.abs(a["H"] - b["H"]).max() <= 2e-6 * scale
            assert np.abs(a["b"] - b["b"]).max() <= 2e-6 * np.abs(b["b"]).max()
    # optimiser trajectories agree to fp32 noise as well
    outs = []
    for span_points in (256, 1 << 20):
        batch = make_batch(pairs, levels=(0, 2), tile_points=1024, span_points=span_points)
        batch.run(8, mode="gn")
        outs.append((npy(batch.poses()), npy(torch.cat(batch.klds()))))
    # (the global scale of a two-view problem is a gauge direction along which fp32 noise drifts freely: compare modulo it)
    np.testing.assert_allclose(outs[0][0][:, :3, :3], outs[1][0][:, :3, :3], atol=2e-5)
    unit = lambda t: t / np.linalg.norm(t, axis=-1, keepdims=True)
    np.testing.assert_allclose(unit(outs[0][0][:, :3, 3]), unit(outs[1][0][:, :3, 3]), atol=2e-4)


def test_per_pair_convergence_skips_finished_pairs_and_keeps_their_result():
    """gn_step(conv_tol > 0): a pair whose accepted step no longer pays is marked done on the device, its spans and its solve
    are skipped from then on (its parameters and cost stay bit-identical), the others continue; with conv_tol = 0 the done
    flags are never consulted."""
    from super_primitive_amd import synth
    easy = synth.make_pair(60, 80, 6, seed=91, init_sigma=0.0005)
    easy.kld_init[:] = easy.kld_gt + 1e-4                      # starts at the optimum: converges at once
    hard = synth.make_pair(60, 80, 6, seed=92, init_sigma=0.01)
    batch = make_batch([easy, hard], levels=(0, 1), tile_points=512)
    done_at = {}
    snap = None
    for it in range(40):
        batch.gn_step(0, conv_tol=1e-3)
        torch.cuda.synchronize()
        d = npy(batch.done)
        for m in (0, 1):
            if d[m] and m not in done_at:
                done_at[m] = it
        if 0 in done_at and snap is None:
            snap = (batch.poses()[0].clone(), batch.klds()[0].clone(), batch.costs()[0].clone())
        if len(done_at) == 2:
            break
    assert 0 in done_at and 1 in done_at and done_at[0] < done_at[1], done_at
    assert torch.equal(batch.poses()[0], snap[0]) and torch.equal(batch.klds()[0], snap[1]) and torch.equal(batch.costs()[0], snap[2])
    # the converged pair sits at the optimum the plain iteration reaches
    ref = make_batch([easy, hard], levels=(0, 1), tile_points=512)
    for _ in range(40):
        ref.gn_step(0)
    np.testing.assert_allclose(npy(batch.evaluate(0)), npy(ref.evaluate(0)), rtol=2e-3)
    p = batch.klds()[1].clone()
    batch.gn_step(0, conv_tol=1e-3)                              # everything done: a no-op
    assert torch.equal(batch.klds()[1], p)


def test_device_side_schedule_walks_every_pair_through_its_own_levels():
    """run_scheduled (sp_pairs_schedule_*): every pair advances through the coarse-to-fine phases on its own -- its result is
    bit-identical to that pair optimised ALONE by run_converging polled every iteration (where the level ends the moment the
    single pair converges), whatever the other pairs of the batch are doing; finished pairs are no longer touched; the
    iteration count is bounded by the slowest pair, not by levels x the slowest pair per level."""
    from super_primitive_amd import synth
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=6, polish_eps=1e-5, polish_tol=1e-4)
    prs = [synth.make_pair(60, 80, 6, seed=93, init_sigma=0.002), synth.make_pair(60, 80, 6, seed=94, init_sigma=0.01),
           synth.make_pair(60, 80, 6, seed=95, init_sigma=0.005)]
    batch = make_batch(prs, levels=(0, 2), tile_points=512)
    launched = batch.run_scheduled(check_every=1, **sch)
    torch.cuda.synchronize()
    n_phases = len(batch.level_ids) + 1
    assert (npy(batch.phase) == n_phases).all() and launched <= n_phases * 12
    solo_iters = []
    for m, pr in enumerate(prs):
        solo = make_batch([pr], levels=(0, 2), tile_points=512)
        its = solo.run_converging(check_every=1, **sch)
        torch.cuda.synchronize()
        solo_iters.append(sum(its))
        assert torch.equal(solo.poses()[0], batch.poses()[m]), m
        assert torch.equal(solo.klds()[0], batch.klds()[m]), m
    assert launched == max(solo_iters), (launched, solo_iters)
    # polled every FOURTH round (a fresh batch): the same per-pair arithmetic, bitwise -- a finished pair's workgroup returns at once -- and the
    # rounds run on to the poll that sees the last pair finished (no SP_PHASE_ADAM phase in this schedule: no work list idles in between)
    every4 = make_batch(prs, levels=(0, 2), tile_points=512)
    launched4 = every4.run_scheduled(check_every=4, **sch)
    torch.cuda.synchronize()
    print(f"\nrounds launched: {launched} polled every round, {launched4} polled every fourth")
    assert torch.equal(every4.pose, batch.pose) and torch.equal(every4.kld, batch.kld)
    assert torch.equal(every4.costs(), batch.costs()) and torch.equal(every4.lm_state[:, :4], batch.lm_state[:, :4])
    assert launched4 == -(-launched // 4) * 4, (launched4, launched)
    # finished: further launches are no-ops
    import ctypes
    from super_primitive_amd import _lib
    before = [k.clone() for k in batch.klds()]
    sched = batch.schedule(**sch)
    _lib.check(batch.lib.sp_pairs_schedule_cost(ctypes.addressof(sched), _lib.ptr(batch.phase), _lib.stream_ptr()), "cost")
    _lib.check(batch.lib.sp_pairs_schedule_gn_step(ctypes.addressof(sched), batch.M, batch.max_N, 8.0, 0.5, 1e-7, _lib.ptr(batch.lm_state),
                                                   _lib.ptr(batch.backup), _lib.ptr(batch._costs), _lib.ptr(batch.phase),
                                                   _lib.ptr(batch.phase_iters), None, _lib.stream_ptr()), "step")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, batch.klds()))


def test_decimated_coarse_levels_have_exact_point_sets_and_the_same_fine_minimiser():
    """PairBatch(point_stride=(1, 2, 4)): the decimated table of a coarse level holds exactly the valid source points on the
    stride lattice, segment by segment, in table order; and run_scheduled over the decimated coarse levels ends -- the finest
    level and the polish use every point -- at the minimiser of the all-points schedule."""
    from parity_util import pose_depth_errors
    from super_primitive_amd import synth
    prs = [synth.make_pair(96, 128, 6, seed=96, init_sigma=0.004), synth.make_pair(96, 128, 9, seed=97, init_sigma=0.006)]
    batch = make_batch(prs, levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4))
    assert sorted(batch.coarse) == [(1, 2), (2, 4)] and batch.coarse[(1, 2)].stride == 2 and batch.coarse[(2, 4)].stride == 4
    pix_full, p_off = npy(batch.pix).view(np.uint32), batch.p_off
    for lay in batch.coarse.values():
        s = lay.stride
        pix = npy(lay.pix).view(np.uint32)
        chunks = npy(lay.chunks)
        assert lay.n_spans == len(npy(lay.spans)) and (chunks[:, 3] % 256 == 0).all()
        for m in range(batch.M):
            full = pix_full[p_off[m]: p_off[m + 1]]
            keep = ((full >> 31) == 1) & ((full & 0xffff) % s == 0) & (((full >> 16) & 0x7fff) % s == 0)
            base = int(chunks[chunks[:, 0] < m, 3].sum())          # chunk starts are relative to the pair's own table
            mine = np.concatenate([pix[base + c[2]: base + c[2] + c[3]] for c in chunks if c[0] == m])
            assert np.array_equal(mine[(mine >> 31) == 1], full[keep])
            assert lay.points[m] >= int(keep.sum())       # points counts every lattice pixel of the masks, valid or not
    # same minimiser as the all-points schedule (both end with full-point phases run to the same tolerances)
    sch = dict(max_iters_per_level=25, conv_tol=1e-4, polish_max=25, polish_eps=1e-5, polish_tol=1e-6)
    launched = batch.run_scheduled(**sch)
    torch.cuda.synchronize()
    ref = make_batch(prs, levels=(0, 3), tile_points=1024)
    ref.run_scheduled(**sch)
    torch.cuda.synchronize()
    assert 0 < launched <= 100
    np.testing.assert_allclose(npy(batch.evaluate(0)), npy(ref.evaluate(0)), rtol=2e-5)
    for m in range(2):
        e = pose_depth_errors(npy(batch.poses()[m]), npy(batch.klds()[m]), npy(ref.poses()[m]), npy(ref.klds()[m]))
        assert e[0] <= 2e-5 and e[1] <= 5e-5 and e[2] <= 5e-4, (m, e)


def test_batched_preparation_equals_the_per_keyframe_tables():
    """PairBatch builds all its tables with the batched sp_prepare_* passes (one launch per pass for the whole batch, one host
    synchronisation); every array must equal, bit for bit, what the per-keyframe path (SegmentTable, blur_decimate,
    source_level, sp_pack_rgb) produces for each pair -- pairs of different image size and segment count, odd sizes
    included -- with zeros in the padding."""
    from super_primitive_amd import synth
    from super_primitive_amd.image import gaussian_pyramid
    from super_primitive_amd.segment_table import SegmentTable, packed_target
    # widths that take each load path of the count / fill passes: 80, 64 (16-byte words), 84 (4-byte words), 131 (bytes),
    # 1040 (wider than the one-load-per-row fast paths)
    prs = [synth.make_pair(60, 80, 6, seed=101), synth.make_pair(97, 131, 9, seed=102), synth.make_pair(48, 64, 1, seed=103),
           synth.make_pair(50, 84, 4, seed=104), synth.make_pair(24, 1040, 2, seed=105)]
    batch = make_batch(prs, levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), extra_tables=[(1, 3)], depth_table=False)     # 3: not a divisor of 4
    assert sorted(batch.coarse) == [(1, 2), (1, 3), (2, 4)]
    # the default DEPTH-TABLE form (SP_COST_DEPTH_TABLE): the same tables with exp(L) in src4.w -- colours bitwise, depths to 2 ulp -- and
    # the same cost / normal equations to the round-off of d = exp(L) exp(shift) against exp(L + shift)
    dt = make_batch(prs, levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), extra_tables=[(1, 3)])
    assert dt.depth_table and not batch.depth_table
    for l in range(3):
        a4, b4 = npy(dt.src4[l].reshape(-1, 4)), npy(batch.src4[l].reshape(-1, 4))
        real = npy(batch.pix).view(np.uint32) != 0
        assert np.array_equal(a4[:, :3], b4[:, :3])
        np.testing.assert_allclose(a4[real, 3], np.exp(b4[real, 3].astype(np.float64)), rtol=3e-7)
    for mode in (0, 1):
        for bt in (dt, batch):
            bt.partials.zero_()             # (a pass writes the columns of its mode only; the buffers come from torch.empty)
            bt.cost_pass(0, mode)
        torch.cuda.synchronize()
        # (IRLS weights 1 / max(|r|, eps) amplify a 2-ulp depth difference where |r| ~ eps: a few sums move by some 1e-4)
        np.testing.assert_allclose(npy(dt.partials), npy(batch.partials), rtol=2e-3, atol=1e-5 * float(np.abs(npy(batch.partials)).max()))
    _check_against_per_keyframe_tables(batch, prs)


def _check_against_per_keyframe_tables(batch, prs, granule=256):
    """every array of the batch's set-up against the per-keyframe path (SegmentTable, blur_decimate, source_level, sp_pack_rgb), bit for bit"""
    from super_primitive_amd.image import gaussian_pyramid
    from super_primitive_amd.segment_table import SegmentTable, packed_target
    dev = batch.device
    for m, pr in enumerate(prs):
        masks, L, kp = T(pr.keypoint_regions).to(dev), T(pr.logdepth_perseg).to(dev), T(pr.keypoints).to(dev)
        tab = SegmentTable(masks, L, kp)
        img_s, img_t, K, kld = T(pr.src_image).to(dev), T(pr.trg_image).to(dev), T(pr.K).to(dev), T(pr.kld_init).to(dev)
        lv_s, lv_t = [img_s], [img_t]
        for _ in range(2):
            lv_s.append(gaussian_pyramid.blur_decimate(lv_s[-1][None])[0])
            lv_t.append(gaussian_pyramid.blur_decimate(lv_t[-1][None])[0])
        src4 = [tab.source_level(lv_s[l], K, kld).clone() for l in range(3)]
        # real points of the padded table: segment n occupies [pos, pos + counts[n])
        pc = (tab.counts + granule - 1) // granule * granule
        pos = np.concatenate(([0], np.cumsum(pc)))[:-1]
        idx = np.concatenate([np.arange(p, p + c) for p, c in zip(pos, tab.counts)])
        lo, hi = batch.p_off[m], batch.p_off[m + 1]
        assert hi - lo == int(pc.sum()) and batch.Ps[m] == tab.P
        pix = npy(batch.pix[lo:hi])
        assert np.array_equal(pix[idx], npy(tab.pix))
        pad = np.ones(hi - lo, bool); pad[idx] = False
        assert not pix[pad].any()
        assert np.array_equal(npy(batch.kp_L[batch.n_off[m]: batch.n_off[m + 1]]), npy(tab.kp_L))
        for l in range(3):
            got = npy(batch.src4[l].reshape(-1, 4)[lo:hi])
            assert np.array_equal(got[idx], npy(src4[l])), (m, l)
            assert not got[pad].any()
            Hl, Wl = lv_t[l].shape[-2:]
            assert batch.level_hw[l][m] == (Hl, Wl)
        # packed targets: compare through the descriptors' offsets
        for l in range(3):
            Hl, Wl = batch.level_hw[l][m]
            off = sum(3 * h * w for h, w in batch.level_hw[l][:m])
            assert np.array_equal(npy(batch.trg4[l][off: off + 3 * Hl * Wl]), npy(packed_target(lv_t[l]).reshape(-1)))
    _check_decimated_tables(batch, prs, granule)


def _check_decimated_tables(batch, prs, granule=256):
    """decimated tables: lattice points of the full table, in order, same validity bits, same source samples -- and, against the
    independent reference (tests/point_table_ref.py), EVERY lattice pixel of the masks in torch.where order at its place in the padded
    layout, the points whose validity bit is clear included, with zeros in the padding"""
    import point_table_ref as ref
    for (level, stride), lay in batch.coarse.items():
        chunks = npy(lay.chunks)
        for m in range(batch.M):
            lo, hi = batch.p_off[m], batch.p_off[m + 1]
            full_pix = npy(batch.pix[lo:hi]).view(np.uint32)
            full_src = npy(batch.src4[level].reshape(-1, 4)[lo:hi])
            real = np.zeros(hi - lo, bool)
            for c in npy(batch.chunks):
                if c[0] == m:
                    real[c[2]: c[2] + c[3]] = True
            on = ((full_pix & 0xffff) % stride == 0) & (((full_pix >> 16) & 0x7fff) % stride == 0) & ((full_pix != 0) | real)
            base = int(chunks[chunks[:, 0] < m, 3].sum())
            mine = np.concatenate([np.arange(base + c[2], base + c[2] + c[3]) for c in chunks if c[0] == m]) if (chunks[:, 0] == m).any() else np.zeros(0, int)
            mpix = npy(lay.pix).view(np.uint32)[mine]
            msrc = npy(lay.src4.reshape(-1, 4))[mine]
            keep_valid = on & ((full_pix >> 31) == 1)
            assert np.array_equal(mpix[(mpix >> 31) == 1], full_pix[keep_valid]), (level, stride, m)
            assert np.array_equal(msrc[(mpix >> 31) == 1], full_src[keep_valid]), (level, stride, m)
            pr = prs[m]
            t = ref.table_ref(pr.keypoint_regions, pr.logdepth_perseg, pr.keypoints, stride)
            pos, pad, total = ref.padded_layout(t["counts"], granule)
            assert len(mine) == total and lay.points[m] == len(t["pix"]), (level, stride, m)
            ref.check_table(t["counts"], mpix[pos], None, None, t, f"level {level} stride {stride} pair {m}")
            assert not mpix[pad].any() and not msrc[pad].view(np.uint32).any(), (level, stride, m)
            t1 = ref.table_ref(pr.keypoint_regions, pr.logdepth_perseg, pr.keypoints, 1)
            pos1 = ref.padded_layout(t1["counts"], granule)[0]
            lattice = ((t1["pix"] & 0xffff) % stride == 0) & ((t1["pix"] >> 16) % stride == 0)
            assert np.array_equal(mpix[pos], full_pix[pos1][lattice]) and np.array_equal(msrc[pos], full_src[pos1][lattice]), (level, stride, m)


def test_fill_pass_on_bit_words_with_every_lattice_stride_and_the_widest_rows():
    """The wave-private fill pass (k_prep_fill_bits) on what the headline batch does not exercise: lattice strides 8 and 16 (one candidate
    pixel per octet, every second octet), rows of 1024 pixels (64 bit words: the widest the path takes, fewer rows per batch), a segment
    that covers whole rows (every octet listed), images taller than a workgroup's 256 rows, and 4 lattices at once: the all-points
    tables equal the per-keyframe tables bit for bit, the decimated ones are their lattice points in order."""
    from super_primitive_amd import synth
    from super_primitive_amd.segment_table import SegmentTable
    prs = [synth.make_pair(48, 1024, 3, seed=201), synth.make_pair(300, 64, 2, seed=202), synth.make_pair(64, 128, 1, seed=203)]
    for strides, extra in (((1, 8, 16), []), ((1, 2, 4), [(0, 8)])):
        batch = make_batch(prs, levels=(0, 3), tile_points=2048, point_stride=strides, extra_tables=extra, depth_table=False, lazy_levels=False)
        dev = batch.device
        for m, pr in enumerate(prs):
            tab = SegmentTable(T(pr.keypoint_regions).to(dev), T(pr.logdepth_perseg).to(dev), T(pr.keypoints).to(dev))
            pc = (tab.counts + 255) // 256 * 256
            pos = np.concatenate(([0], np.cumsum(pc)))[:-1]
            idx = np.concatenate([np.arange(p, p + c) for p, c in zip(pos, tab.counts)])
            lo, hi = batch.p_off[m], batch.p_off[m + 1]
            assert hi - lo == int(pc.sum()) and batch.Ps[m] == tab.P
            pix = npy(batch.pix[lo:hi]).view(np.uint32) & 0x7fffffff
            assert np.array_equal(pix[idx], npy(tab.pix).view(np.uint32) & 0x7fffffff), m
            pad = np.ones(hi - lo, bool); pad[idx] = False
            assert not pix[pad].any()
        _check_decimated_tables(batch, prs)


@pytest.mark.parametrize("optimisers", [1, 3])
def test_pair_stream_overlaps_batches_and_returns_each_batch_s_own_result(optimisers):
    """PairStream: batch k+1 is built on the set-up stream by a producer thread while batch k runs its schedule on an
    optimisation stream; with ``optimisers`` > 1 several batches run their schedules concurrently on their own streams
    (continuous batching: the next batch's bulk fills the tail of the current one).  Every batch's result is bit-identical to the
    same batch built and optimised alone on the default stream -- ragged batches (different pair counts, sizes and segment
    counts), yielded in input order."""
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.pair_batch import PairBatch
    from super_primitive_amd.optim.pair_stream import PairStream
    dev = torch.device("cuda:0")
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=6, polish_eps=1e-5, polish_tol=1e-4)
    groups = [[synth.make_pair(60, 80, 6, seed=111), synth.make_pair(60, 80, 6, seed=112)],
              [synth.make_pair(96, 128, 9, seed=113)],
              [synth.make_pair(60, 80, 6, seed=114), synth.make_pair(48, 64, 4, seed=115), synth.make_pair(60, 80, 6, seed=116)]]

    def inputs(prs):
        t = lambda a: T(a).to(dev)
        return dict(src_frames=[KeyFrame(t(p.src_image), t(p.K), t(p.logdepth_perseg), t(p.keypoints), t(p.keypoint_regions)) for p in prs],
                    trg_images=[t(p.trg_image) for p in prs], trg_Ks=[t(p.K) for p in prs],
                    poses=torch.stack([t(p.pose_init) for p in prs]), klds=[t(p.kld_init) for p in prs])

    items = [inputs(g) for g in groups]
    stream = PairStream(levels=(0, 3), point_stride=(1, 2, 4), schedule=sch, tile_points=1024, optimisers=optimisers)
    items = items * 2 if optimisers > 1 else items
    got = list(stream.run(iter(items)))
    torch.cuda.synchronize()
    assert len(got) == len(items)
    import sys
    interval = sys.getswitchinterval()
    for item, res in zip(items, got):
        poses, klds = res
        ref = PairBatch(item["src_frames"], item["trg_images"], item["trg_Ks"], item["poses"], item["klds"], levels=(0, 3),
                        point_stride=(1, 2, 4), tile_points=1024)
        ref.run_scheduled(**sch)
        torch.cuda.synchronize()
        assert torch.equal(poses, ref.poses())
        assert all(torch.equal(a, b) for a, b in zip(klds, ref.klds()))
        assert torch.equal(res.status, ref.status) and torch.equal(res.attempts, ref.attempts)      # the verdict travels with the results
    # the lowered thread switch interval is handed back at every yield and at the end (reference counted)
    gen = stream.run(iter(items))
    for _ in gen:
        assert sys.getswitchinterval() == interval
    assert sys.getswitchinterval() == interval
    # an error in the producer thread reaches the caller
    bad = dict(items[0]); bad["klds"] = bad["klds"][:1]
    with pytest.raises(AssertionError):
        list(stream.run(iter([bad])))
    # a caller that stops early does not leave the producer blocked
    import time
    gen = stream.run(iter(items * 3))
    next(gen)
    t0 = time.time()
    gen.close()
    assert time.time() - t0 < 10.0


def test_pair_batch_is_freed_by_reference_count_alone():
    """A PairBatch holds ~25 MB of tables per pair: it must go away when the last reference goes (no reference cycle through the
    lazily built level samples / descriptors), otherwise a stream of batches waits for the cyclic collector and the allocator
    runs dry (seen as multi-second stalls of the set-up thread of a PairStream)."""
    import gc
    import weakref
    from super_primitive_amd import synth
    gc.disable()
    try:
        batch = make_batch([synth.make_pair(60, 80, 6, seed=3)], levels=(0, 3), point_stride=(1, 2, 4))
        batch.run_scheduled(max_iters_per_level=3, polish_max=2)
        batch.gn_step(1)                      # a lazily sampled level
        ref = weakref.ref(batch)
        del batch
        assert ref() is None
    finally:
        gc.enable()


@pytest.mark.parametrize("shape,seed", [("grid", 3), ("blobs", 4)])
def test_wave_span_work_list_gives_the_same_sums_and_steps(shape, seed):
    """granule = 64 (SP_COST_WAVE_SPANS: spans belong to single waves, tables padded to multiples of 64, one segment record per
    chunk) against the oracle's Gauss-Newton system and against the 256-granule batch: same cost, same normal equations and
    gradients up to fp32 summation order, same scheduled end state inside half the north-star bar; less padding."""
    from oracle import gn_oracle, photometric_oracle as orc
    from super_primitive_amd import synth
    kw = dict(blob_coverage=1.2) if shape == "blobs" else dict(overlap=1)
    pairs = [synth.make_pair(60, 80, 24, seed=seed + k, shape=shape, init_sigma=0.006, **kw) for k in range(3)]
    a = make_batch(pairs, levels=(0, 2), tile_points=512, point_stride=(1, 2))
    b = make_batch(pairs, levels=(0, 2), tile_points=512, point_stride=(1, 2), granule=64)
    assert b.granule == 64 and b.n_seg_records == b.n_chunks and sum(b.Ppads) < sum(a.Ppads)
    assert all(int(c) % 64 == 0 for c in npy(b.chunks)[:, 3])
    got = assemble_gn(b)
    ref = assemble_gn(a)
    for m, p in enumerate(pairs):
        src, trg = orc.frames_from_synth(p)
        want = gn_oracle.normal_equations(src, trg, torch.from_numpy(p.kld_init), torch.from_numpy(p.pose_init), eps=1e-3)
        H, bb = want["H"].numpy(), want["b"].numpy()
        np.testing.assert_allclose(got[m]["cost"], want["cost"], rtol=2e-5)
        for sl, name in ((np.s_[:6, :6], "H_pp"), (np.s_[:6, 6:], "H_pd"), (np.s_[6:, 6:], "H_dd")):
            assert np.abs(got[m]["H"][sl] - H[sl]).max() <= 3e-3 * np.abs(H[sl]).max(), name
            assert np.abs(got[m]["H"][sl] - ref[m]["H"][sl]).max() <= 2e-5 * np.abs(H[sl]).max(), name      # vs the 256-granule sums
        assert np.abs(got[m]["b"] - bb).max() <= 3e-3 * np.abs(bb).max()
        assert got[m]["n_valid"] == ref[m]["n_valid"]
    # gradient mode: one Adam step moves both batches alike
    np.testing.assert_allclose(npy(b.evaluate(0)), npy(a.evaluate(0)), rtol=2e-6)
    for x in (a, b):
        x.adam_step(0)
    np.testing.assert_allclose(npy(b.pose), npy(a.pose), atol=2e-6)
    np.testing.assert_allclose(npy(b.kld), npy(a.kld), atol=2e-6)
    # the scheduled run (device-side phases on the wave-span work lists of both lattices)
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=8, polish_eps=1e-5, polish_tol=1e-4)
    for x in (a, b):
        x.restore_initial()
        x.run_scheduled(**sch)
    # (the two work lists sum in different orders, so a pair may take one LM iteration more or fewer: the end states agree to the
    #  schedule's own convergence tolerance, compared with the two-view scale gauge removed)
    from parity_util import pose_depth_errors
    for m in range(len(pairs)):
        e = pose_depth_errors(npy(b.poses()[m]), npy(b.klds()[m]), npy(a.poses()[m]), npy(a.klds()[m]))
        assert e[0] <= 5e-5 and e[1] <= 5e-5 and e[2] <= 5e-4, (m, e)
    b.restore_initial()
    b.run_scheduled(**sch)
    again = (b.pose.clone(), b.kld.clone())
    b.restore_initial()
    b.run_scheduled(**sch)
    assert torch.equal(again[0], b.pose) and torch.equal(again[1], b.kld)            # deterministic


@pytest.mark.parametrize("granule", [256, 64])
def test_slot_level_continuous_batching_gives_every_pair_its_own_result(granule):
    """run_scheduled(slots=S) (SpQueue, sp_pairs_schedule_run_queue): 14 resident pairs of one layout, 4 slots -- a
    finished pair's slot goes to the next waiting pair inside the solver launch.  Every pair's pose, log-depths, final cost and
    iteration counts are BITWISE those of the run with all 14 resident (pairs never interact),
    whichever slot it happened to get; the queue is handed out completely; far fewer pair-slots are launched than slots x rounds.
    With 8 slots the last pair to finish iterates alone and 8 x (busy slots) <= slots holds: the one small case whose last rounds are
    launched over the listed slots only (SpQueue.active).  Nothing on the host reports that this branch was taken -- what is asserted is
    that the results are the same bits with it."""
    from super_primitive_amd import synth
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=6, polish_eps=1e-5, polish_tol=1e-4)
    sig = [0.002, 0.012, 0.004, 0.008, 0.001, 0.015, 0.003, 0.006, 0.010, 0.002, 0.007, 0.013, 0.005, 0.009]
    prs = [synth.make_pair(96, 128, 6, seed=120 + i, init_sigma=s, overlap=2) for i, s in enumerate(sig)]
    kw = dict(levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), granule=granule)
    ref = make_batch(prs, **kw)
    n_ref = ref.run_scheduled(check_every=1, **sch)
    torch.cuda.synchronize()
    its_ref = npy(ref.lm_state[:, 2] + ref.lm_state[:, 3])
    assert its_ref.max() > 1.3 * its_ref.min()                 # (the pairs really finish at different times)
    for slots in (4, 5, 8):
        q = make_batch(prs, **kw)
        n_q = q.run_scheduled(check_every=1, slots=slots, **sch)
        torch.cuda.synchronize()
        assert q._queue_stats["head"] >= q.M and sorted(set(npy(q._queue_stats["slot_pair"]).tolist())) != list(range(slots))
        for m in range(q.M):
            assert torch.equal(q.poses()[m], ref.poses()[m]) and torch.equal(q.klds()[m], ref.klds()[m]), (slots, m)
        assert torch.equal(q.costs(), ref.costs()) and torch.equal(q.lm_state[:, :4], ref.lm_state[:, :4])
        # rounds: about (sum of the pairs' iterations) / slots, not (pairs / slots) x the slowest pair
        print(f"\n{q.M} pairs, {slots} slots (granule {granule}): {n_q} rounds launched (all resident: {n_ref}; sum of iterations {int(its_ref.sum())}, / slots = {its_ref.sum() / slots:.1f}, slowest pair {int(its_ref.max())})")
        assert n_q <= its_ref.sum() / slots + its_ref.max() + 2


@pytest.mark.parametrize("granule", [256, 64])
def test_slot_level_continuous_batching_of_ragged_pairs(granule):
    """the slots of run_scheduled(slots=S) take pairs of DIFFERENT padded layouts -- SAM-like blobs of ragged sizes,
    different segment counts, a different image size -- because the cost pass of a queue run goes over virtual spans (as many per slot
    as the largest pair has; a slot's descriptor carries its pair's own span range).  Every pair ends BITWISE where it ends with all
    pairs resident, in whichever slot and order it ran; the verdict arrays are filed per pair."""
    from super_primitive_amd import _lib, synth
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=6, polish_eps=1e-5, polish_tol=1e-4)
    sig = [0.002, 0.012, 0.004, 0.008, 0.001, 0.015, 0.003, 0.006, 0.010, 0.002, 0.007]
    prs = [synth.make_pair(96, 128, 5 + (i % 4) * 3, seed=150 + i, init_sigma=s, shape="blobs", blob_coverage=0.9 + 0.15 * (i % 3)) for i, s in enumerate(sig)]
    prs += [synth.make_pair(72, 96, 7, seed=170, init_sigma=0.005, overlap=2), synth.make_pair(96, 128, 6, seed=171, init_sigma=0.004, overlap=2)]
    kw = dict(levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), granule=granule)
    ref = make_batch(prs, **kw)
    assert not ref._uniform_layout and len(set(ref.Ns)) > 2
    n_ref = ref.run_scheduled(check_every=1, **sch)
    torch.cuda.synchronize()
    its_ref = npy(ref.lm_state[:, 2] + ref.lm_state[:, 3])
    for slots in (1, 3, 5):
        q = make_batch(prs, **kw)
        n_q = q.run_scheduled(check_every=1, slots=slots, **sch)
        torch.cuda.synchronize()
        assert q._queue_stats["head"] >= q.M and q._queue_stats["finished"]
        for m in range(q.M):
            assert torch.equal(q.poses()[m], ref.poses()[m]) and torch.equal(q.klds()[m], ref.klds()[m]), (slots, m)
        assert torch.equal(q.costs(), ref.costs()) and torch.equal(q.lm_state[:, :4], ref.lm_state[:, :4])
        assert torch.equal(q.status, ref.status) and torch.equal(q.diag, ref.diag)
        # (rounds: a phase that ends by its convergence test spends one more evaluation than it counts iterations -- 4 phases per pair)
        assert n_q <= (its_ref.sum() + 4 * q.M) / slots + its_ref.max() + 2
    assert int((ref.status & _lib.SP_STATUS_NONFINITE).sum()) == 0


def test_sam_realistic_masks_through_the_set_up_and_the_slot_queue():
    """SAM-REALISTIC segment sets (``synth.make_pair(shape='sam')``: areas over two decades at this size, masks with
    holes, masks nested inside masks, two-lobed masks split into their components -- what frontend/segment/mask_generation.py:143-312 and
    post_processer.py:160-181 emit; N differs from keyframe to keyframe) through (a) the batched set-up: every table, source sample and
    packed target bitwise the per-keyframe path's; (b) the slot queue on one and on two streams: every pair bitwise where it ends with
    all pairs resident, whatever slot, stream and order it ran in."""
    from super_primitive_amd import _lib, synth
    prs = [synth.make_pair(120, 160, 20, seed=300 + i, init_sigma=0.002 + 0.002 * (i % 4), shape="sam", blob_coverage=1.1) for i in range(9)]
    Ns = [p.N for p in prs]
    areas = np.concatenate([p.keypoint_regions.reshape(p.N, -1).sum(1) for p in prs])
    print(f"\nsam masks: segments per keyframe {Ns}, areas {int(areas.min())} .. {int(areas.max())} px (median {int(np.median(areas))})")
    assert len(set(Ns)) > 2 and areas.max() > 40 * areas.min()
    holes = 0
    for p in prs:                               # at least one ring among them: a mask whose centroid pixel is not in the mask
        for k in range(p.N):
            r, c = np.nonzero(p.keypoint_regions[k])
            holes += int(not p.keypoint_regions[k, int(round(r.mean())), int(round(c.mean()))])
    assert holes >= 1
    batch = make_batch(prs, levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), depth_table=False)
    _check_against_per_keyframe_tables(batch, prs)
    wave = make_batch(prs, levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), depth_table=False, granule=64)
    _check_against_per_keyframe_tables(wave, prs, granule=64)
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=6, polish_eps=1e-5, polish_tol=1e-4)
    kw = dict(levels=(0, 3), tile_points=1024, point_stride=(2, 2, 4), granule=64)
    ref = make_batch(prs, **kw)
    ref.run_scheduled(check_every=1, **sch)
    torch.cuda.synchronize()
    for slots, streams in ((2, 1), (4, 2), (5, 3)):
        q = make_batch(prs, **kw)
        q.run_scheduled(check_every=1, slots=slots, streams=streams, **sch)
        torch.cuda.synchronize()
        assert q._queue_stats["head"] >= q.M and q._queue_stats["finished"]
        for m in range(q.M):
            assert torch.equal(q.poses()[m], ref.poses()[m]) and torch.equal(q.klds()[m], ref.klds()[m]), (slots, streams, m)
        assert torch.equal(q.costs(), ref.costs()) and torch.equal(q.lm_state[:, :4], ref.lm_state[:, :4])
        assert torch.equal(q.status, ref.status) and torch.equal(q.diag, ref.diag)
    from parity_util import pose_depth_errors
    errs = np.array([pose_depth_errors(npy(ref.poses()[m]), npy(ref.klds()[m]), p.pose_gt, p.kld_gt) for m, p in enumerate(prs)])
    st = npy(ref.status)
    print(f"sam masks: end states vs ground truth (worst) {errs.max(0)}, status {[hex(int(v)) for v in st]}")
    assert int((ref.status & _lib.SP_STATUS_NONFINITE).sum()) == 0


def test_scheduled_run_reports_a_verdict_and_retries_what_fails_it():
    """the per-pair verdict of a scheduled run (SpVerdict) and its one second attempt.  Three pairs: one near its
    minimum, one whose start is hopeless (the pose a radian off: the target frame does not see the source's points), and the first again.  (a) Without a second attempt the
    hopeless pair is FLAGGED (``failed()``) and the good ones are not; diag holds the final cost / largest log-depth excursion / valid
    fraction / polish iterations.  (b) A verdict that fails everything (kld_bound tiny) sends every pair through the retry phases once:
    ``attempts`` = 1, SP_STATUS_RETRIED set, and the pair that was fine ends where the retry's phase list brings it -- inside the
    schedule's tolerance of its first result.  (c) The same through the slot queue, bitwise.  (d) A run cut short by its round limit
    marks what it did not finish."""
    from super_primitive_amd import _lib, synth
    from parity_util import pose_depth_errors
    good = synth.make_pair(96, 128, 6, seed=31, init_sigma=0.004, overlap=2)
    bad = synth.make_pair(96, 128, 6, seed=32, init_sigma=0.004, overlap=2)
    bad.pose_init = (synth.se3_exp_np(np.array([0.3, -0.2, 0.1, 0.0, 1.0, 0.0])) @ bad.pose_init.astype(np.float64)).astype(np.float32)
    prs = [good, bad, good]
    kw = dict(levels=(0, 3), tile_points=1024, point_stride=(1, 2, 4), granule=64)
    sch = dict(max_iters_per_level=12, conv_tol=2e-3, polish_max=15, polish_eps=1e-5, polish_tol=1e-4)
    a = make_batch(prs, **kw)
    it, status = a.run_scheduled(return_status=True, **sch)
    st = npy(status)
    assert st[0] == 0 and st[2] == 0 and (st[1] & _lib.SP_STATUS_FAILED) != 0 and not (st[1] & _lib.SP_STATUS_RETRIED), st
    assert npy(a.failed()).tolist() == [False, True, False] and npy(a.attempts).tolist() == [0, 0, 0]
    d = npy(a.diag)
    np.testing.assert_allclose(d[0, 0], float(a.lm_state[0, 5]), rtol=0, atol=0)
    assert 0 < d[0, 1] < 0.5 and 0.8 < d[0, 2] <= 1.0 and 1 <= d[0, 3] <= 15 and d[0, 4] == 1 and d[0, 5] > 0
    first = (a.poses()[0].clone(), a.klds()[0].clone())
    # (b) everything fails a verdict with a tiny depth bound -> everything runs the retry phases once
    b = make_batch(prs, **kw)
    b.run_scheduled(verdict=dict(kld_bound=1e-6), retry_pose_first=((2, 6),), **sch)
    assert npy(b.attempts).tolist() == [1, 1, 1]
    sb = npy(b.status)
    assert all(s & _lib.SP_STATUS_RETRIED for s in sb) and all(s & _lib.SP_STATUS_DEPTH_RANGE for s in sb)
    assert npy(b.diag)[:, 4].tolist() == [2.0, 2.0, 2.0]
    e = pose_depth_errors(npy(b.poses()[0]), npy(b.klds()[0]), npy(first[0]), npy(first[1]))
    assert e[0] <= 5e-5 and e[1] <= 5e-5 and e[2] <= 5e-4, e
    assert torch.equal(b.poses()[0], b.poses()[2]) and torch.equal(b.klds()[0], b.klds()[2])        # same pair, same two attempts
    its_a, its_b = npy(a.lm_state[:, 2] + a.lm_state[:, 3]), npy(b.lm_state[:, 2] + b.lm_state[:, 3])
    assert its_b[0] > its_a[0]                                                                         # (the counts run over both attempts)
    # (c) the same through two slots: bitwise
    c = make_batch(prs, **kw)
    c.run_scheduled(slots=2, verdict=dict(kld_bound=1e-6), retry_pose_first=((2, 6),), **sch)
    assert torch.equal(c.pose, b.pose) and torch.equal(c.kld, b.kld) and torch.equal(c.status, b.status) and torch.equal(c.diag, b.diag)
    assert torch.equal(c.lm_state[:, :4], b.lm_state[:, :4])
    # (c') THREE attempts: a second attempt's pose-only phase, then Adam phases (SP_PHASE_ADAM, on the lattice's fine-grained work list, launched
    #      only while a pair is in them) -- everything fails the tiny depth bound twice and goes through all of it: attempts = 2, RETRIED | ADAM,
    #      and the slot queue on one and two streams gives every pair bitwise the all-resident result
    adam = [dict(level=2, stride=4, max_iters=7, irls_eps=1e-5, conv_tol=0.0, adam=True), dict(level=1, stride=2, max_iters=5, irls_eps=1e-5, conv_tol=0.0, adam=True)]
    e3 = make_batch(prs, **kw)
    e3.run_scheduled(verdict=dict(kld_bound=1e-6), retry_pose_first=((2, 6),), retry2_phases=adam, **sch)
    assert npy(e3.attempts).tolist() == [2, 2, 2] and npy(e3.diag)[:, 4].tolist() == [3.0, 3.0, 3.0]
    assert all((s_ & _lib.SP_STATUS_RETRIED) and (s_ & _lib.SP_STATUS_ADAM) and (s_ & _lib.SP_STATUS_DEPTH_RANGE) for s_ in npy(e3.status))
    assert torch.equal(e3.poses()[0], e3.poses()[2]) and torch.equal(e3.klds()[0], e3.klds()[2])
    assert sorted(e3._fine) == [(1, 2), (2, 4)]
    for slots, streams in ((2, 1), (2, 2), (1, 1)):
        f3 = make_batch(prs, **kw)
        f3.run_scheduled(slots=slots, streams=streams, verdict=dict(kld_bound=1e-6), retry_pose_first=((2, 6),), retry2_phases=adam, **sch)
        assert torch.equal(f3.pose, e3.pose) and torch.equal(f3.kld, e3.kld) and torch.equal(f3.status, e3.status) and torch.equal(f3.diag, e3.diag), (slots, streams)
    # (d) a schedule whose iteration budget is cut by hand: unfinished pairs say so
    dd = make_batch(prs, **kw)
    sched = dd.schedule(**sch)
    v = dd._verdict(sched, None)
    dd.phase.fill_(sched.entry); dd.phase_iters.zero_()
    flag = (torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32).pin_memory())
    import ctypes
    n = dd.lib.sp_pairs_schedule_run(ctypes.addressof(sched), dd.M, dd.max_N, 8.0, 0.5, 1e-7, _lib.ptr(dd.lm_state), _lib.ptr(dd.backup), _lib.ptr(dd._costs),
                                     _lib.ptr(dd.phase), _lib.ptr(dd.phase_iters), 2, 4, _lib.ptr(flag[0]), flag[1].data_ptr(), ctypes.addressof(v), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert n == 4 and all(s == _lib.SP_STATUS_UNFINISHED for s in npy(dd.status))
    #     ... and through two slots, the queue driver's round budget cut to (bound = 1) x (3 pairs / 2 slots, rounded up, + 1) = 3: no pair can
    #     finish; the two in a slot are marked by the library (under the pair's index, through slot_pair), the one still waiting by the host
    dq = make_batch(prs, **kw)
    sched = dq.schedule(**sch)
    v = dq._verdict(sched, None)
    dq._flag = flag
    n = dq._run_queue(sched, 2, 1, 2, 8.0, 0.5, 1e-7, v, ctypes.addressof(v), schedule_kw=sch)
    torch.cuda.synchronize()
    print(f"\nqueue run on its round limit: {n} rounds, status {npy(dq.status).tolist()}, queue {dq._queue_stats}")
    assert n == 3 and npy(dq.status).tolist() == [_lib.SP_STATUS_UNFINISHED] * 3
    assert dq._queue_stats["head"] == 2 and not dq._queue_stats["finished"]
    # (e) a non-finite unknown (the one thing the reference asserts on, core/dense_optim.py:311,321,340-343) is reported for THAT pair only
    ee = make_batch(prs, **kw)
    ee.kld[ee.n_off[2] + 1] = float("nan")
    ee.run_scheduled(**sch)
    se = npy(ee.status)
    assert (se[2] & _lib.SP_STATUS_NONFINITE) != 0 and se[0] == 0 and npy(ee.failed()).tolist() == [False, True, True]
    assert torch.equal(ee.poses()[0], a.poses()[0]) and torch.equal(ee.klds()[0], a.klds()[0])          # (pairs never interact)


def _mask_boxes(masks):
    """(N,4) int32 {row0, col0, row1, col1} (half open) of a bool (N,H,W) mask stack; an empty mask gets an empty box."""
    rows, cols = masks.any(dim=2), masks.any(dim=1)
    H, W = masks.shape[1:]
    first = lambda b: torch.where(b.any(1), b.float().argmax(1), torch.zeros_like(b[:, 0], dtype=torch.long))
    last = lambda b, n: torch.where(b.any(1), n - b.flip(1).float().argmax(1), torch.zeros_like(b[:, 0], dtype=torch.long))
    return torch.stack((first(rows), first(cols), last(rows, H), last(cols, W)), dim=1).to(torch.int32)


@pytest.mark.parametrize("granule", [256, 64])
def test_segment_box_hint_builds_the_same_tables(granule):
    """``KeyFrame.segment_boxes`` -- the (N,4) boxes a SAM-like frontend has anyway
    (frontend/segment/mask_generation.py:93,155-180) -- lets the count pass of the batched set-up read the masks inside the boxes only.
    Every table, every lattice, every sampled level and the work lists are BITWISE what the full scan builds: grid tiles and ragged blobs,
    tight boxes, boxes larger than the mask, boxes reaching over the image (clamped), an empty segment with an inverted box; a keyframe
    off the fast path (width 84) ignores its hint.  A box that cuts its mask -- at the granularity the pass reads the masks with: rows, and
    16-pixel pieces along a row -- loses exactly the pixels outside."""
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.pair_batch import PairBatch
    dev = torch.device("cuda:0")
    prs = [synth.make_pair(96, 128, 6, seed=401, overlap=2), synth.make_pair(96, 128, 9, seed=402, shape="blobs", blob_coverage=1.1),
           synth.make_pair(50, 84, 4, seed=403), synth.make_pair(128, 160, 7, seed=404, shape="blobs", blob_coverage=0.8)]
    prs[1].keypoint_regions[3] = False                      # an empty segment
    t = lambda a: T(a).to(dev)

    def frames(with_boxes, grow=0, cut=False):
        out = []
        for i, p in enumerate(prs):
            kf = KeyFrame(t(p.src_image), t(p.K), t(p.logdepth_perseg), t(p.keypoints), t(p.keypoint_regions))
            if with_boxes:
                b = _mask_boxes(kf.keypoint_regions)
                b[:, :2] -= grow; b[:, 2:] += grow                         # (boxes beyond the image are clamped on the device)
                if i == 1:
                    b[3] = torch.tensor([40, 50, 10, 20], dtype=torch.int32)      # inverted: an empty segment
                if cut and i == 0:
                    b[2, 3] = (b[2, 1] // 16 + 1) * 16                      # segment 2 of pair 0: only up to the next 16-pixel boundary
                    b[2, 2] = b[2, 0] + 5                                   # ... and its first 5 rows
                kf.segment_boxes = b.to(dev)
            out.append(kf)
        return out

    rest = ([t(p.trg_image) for p in prs], [t(p.K) for p in prs], torch.stack([t(p.pose_init) for p in prs]), [t(p.kld_init) for p in prs])
    build = lambda fr: PairBatch(fr, *rest, levels=(0, 3), point_stride=(2, 2, 4), granule=granule, tile_points=1024)
    ref = build(frames(False))
    for grow in (0, 5, 1000):
        got = build(frames(True, grow))
        assert got.Ps == ref.Ps and torch.equal(got.pix, ref.pix) and torch.equal(got.kp_L, ref.kp_L)
        assert torch.equal(got.src4[0], ref.src4[0]) and torch.equal(got.chunks, ref.chunks) and torch.equal(got.spans, ref.spans)
        for key, lay in ref.coarse.items():
            assert torch.equal(got.coarse[key].pix, lay.pix) and torch.equal(got.coarse[key].src4, lay.src4), (grow, key)
    # a box that cuts its mask: exactly the mask pixels outside are gone (compare with the masks cut by hand, no hint)
    cut = build(frames(True, 0, cut=True))
    bx = _mask_boxes(t(prs[0].keypoint_regions))[2]
    hand = frames(False)
    m = hand[0].keypoint_regions.clone(); m[2, :, (int(bx[1]) // 16 + 1) * 16:] = False; m[2, int(bx[0]) + 5:] = False
    hand[0].keypoint_regions = m
    want = build(hand)
    assert cut.Ps[0] < ref.Ps[0] and cut.Ps == want.Ps and torch.equal(cut.pix, want.pix) and torch.equal(cut.src4[0], want.src4[0])
    with pytest.raises(ValueError):
        bad = frames(False)
        bad[0].segment_boxes = torch.zeros(3, 4, dtype=torch.int32, device=dev)
        build(bad)


@pytest.mark.parametrize("granule", [256, 64])
def test_boxed_count_pass_builds_the_same_tables(granule):
    """Round 6 (ABI 15): a batch whose keyframes ALL carry the segment-box hint goes through ``sp_prepare_count_boxed`` -- one workgroup per
    segment, the box's pieces in flight at once, row counts summed by integer adds in LDS -- instead of the row-block pass.  Tables, sampled
    levels and work lists are BITWISE those of the full scan without boxes: grid tiles, ragged blobs, SAM-realistic sets (areas over decades,
    nested masks, holes), boxes tight / grown / reaching over the image, an empty segment with an inverted box, and a keyframe of more than
    1024 rows (its hint is ignored: the whole frame is every segment's box, in passes of 1024 rows)."""
    from super_primitive_amd import _lib, synth
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim import batch_prepare
    from super_primitive_amd.optim.pair_batch import PairBatch
    dev = torch.device("cuda:0")
    prs = [synth.make_pair(96, 128, 6, seed=401, overlap=2), synth.make_pair(96, 128, 9, seed=402, shape="blobs", blob_coverage=1.1),
           synth.make_pair(128, 160, 7, seed=404, shape="blobs", blob_coverage=0.8), synth.make_pair(240, 320, 24, seed=405, shape="sam"),
           synth.make_pair(1104, 32, 3, seed=406)]
    prs[1].keypoint_regions[3] = False                      # an empty segment
    t = lambda a: T(a).to(dev)

    def frames(with_boxes, grow=0):
        out = []
        for i, p in enumerate(prs):
            kf = KeyFrame(t(p.src_image), t(p.K), t(p.logdepth_perseg), t(p.keypoints), t(p.keypoint_regions))
            if with_boxes:
                b = _mask_boxes(kf.keypoint_regions)
                b[:, :2] -= grow; b[:, 2:] += grow
                if i == 1:
                    b[3] = torch.tensor([40, 50, 10, 20], dtype=torch.int32)      # inverted: an empty segment
                kf.segment_boxes = b.to(dev)
            out.append(kf)
        return out

    rest = ([t(p.trg_image) for p in prs], [t(p.K) for p in prs], torch.stack([t(p.pose_init) for p in prs]), [t(p.kld_init) for p in prs])
    calls = []
    lib = _lib.load()
    real = lib.sp_prepare_count_boxed

    class _Spy:                                  # (which entry point the set-up took)
        def __getattr__(self, name):
            if name == "sp_prepare_count_boxed":
                return lambda *a: (calls.append(1), real(*a))[1]
            return getattr(lib, name)

    for stride in ((2, 2, 4), (1, 2, 4)):
        build = lambda fr: PairBatch(fr, *rest, levels=(0, 3), point_stride=stride, granule=granule, tile_points=1024)
        ref = build(frames(False))
        for grow in (0, 5, 1000):
            n0 = len(calls)
            orig = batch_prepare._lib.load
            batch_prepare._lib.load = lambda: _Spy()
            try:
                got = build(frames(True, grow))
            finally:
                batch_prepare._lib.load = orig
            assert len(calls) == n0 + 1, "the boxed count pass was not taken"
            assert got.Ps == ref.Ps and torch.equal(got.pix, ref.pix) and torch.equal(got.kp_L, ref.kp_L)
            bits = lambda x: x.contiguous().view(torch.int32)          # (bit patterns: the tall keyframe's synthetic depths hold NaNs)
            assert torch.equal(bits(got.src4[0]), bits(ref.src4[0])) and torch.equal(got.chunks, ref.chunks) and torch.equal(got.spans, ref.spans)
            for key, lay in ref.coarse.items():
                assert torch.equal(got.coarse[key].pix, lay.pix) and torch.equal(bits(got.coarse[key].src4), bits(lay.src4)), (stride, grow, key)


def test_keyframe_record_of_the_set_up_follows_replaced_and_edited_tensors():
    """The batched set-up finds the device addresses of a keyframe's tensors on the keyframe (optim.batch_prepare.frame_records).  A build
    after one of them was REPLACED reads the new tensor, a build after an IN-PLACE edit reads the edited values -- both equal to a build from
    fresh KeyFrame objects -- and a second build from untouched keyframes equals the first bit for bit."""
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.pair_batch import PairBatch
    dev = torch.device("cuda:0")
    prs = [synth.make_pair(60, 80, 6, seed=301), synth.make_pair(48, 64, 4, seed=302)]
    t = lambda a: T(a).to(dev)
    tens = [dict(img=t(p.src_image), K=t(p.K), L=t(p.logdepth_perseg), kp=t(p.keypoints), m=t(p.keypoint_regions)) for p in prs]
    frames = [KeyFrame(d["img"], d["K"], d["L"], d["kp"], d["m"]) for d in tens]
    rest = ([t(p.trg_image) for p in prs], [t(p.K) for p in prs], torch.stack([t(p.pose_init) for p in prs]), [t(p.kld_init) for p in prs])
    build = lambda fr: PairBatch(fr, *rest, levels=(0, 2), point_stride=(1, 2), depth_table=False)
    a, a2 = build(frames), build(frames)
    assert "_sp_prep" in frames[0].__dict__ and torch.equal(a.src4[0], a2.src4[0]) and torch.equal(a.pix, a2.pix)
    frames[0].logdepth_perseg = tens[0]["L"] + 0.125                 # replaced: the record is dropped and made again
    assert "_sp_prep" not in frames[0].__dict__
    b = build(frames)
    fresh = [KeyFrame(tens[0]["img"], tens[0]["K"], tens[0]["L"] + 0.125, tens[0]["kp"], tens[0]["m"]), KeyFrame(*[tens[1][k] for k in ("img", "K", "L", "kp", "m")])]
    c = build(fresh)
    assert torch.equal(b.src4[0], c.src4[0]) and not torch.equal(b.src4[0], a.src4[0])
    frames[1].logdepth_perseg.mul_(1.5)                               # edited in place: same address, the record stays
    assert "_sp_prep" in frames[1].__dict__
    d, e = build(frames), build([fresh[0], KeyFrame(*[tens[1][k] for k in ("img", "K", "L", "kp", "m")])])
    assert torch.equal(d.src4[0], e.src4[0]) and not torch.equal(d.src4[0], b.src4[0])
