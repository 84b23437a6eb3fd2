"""-m gpu: the Gauss-Newton / LM flavour of the window optimiser (sp_pairs_cost mode 2 + sp_window_gn_step).

* mode 2 of the cost kernel -- the Gauss-Newton sums WITH the affine brightness columns -- against the oracle's float64
  finite-difference Jacobian of the reference residual (pose, per-segment log-depths, target affine pair);
* tracking at BASELINE configs[2] size (224x288x40): 6 pose + 2 affine unknowns reach the reference's converged tracking result
  (golden g17 ``track_polished_*``: its 300 Adam steps + two polish phases) within 1e-4 rad / 1e-4 t in <= 15 LM iterations;
* windowed mapping at that size (3 keyframes = full window, one supporting frame each: 5 free poses, 80 free log-depths, 5 free
  affine pairs; first keyframe and oldest depths fixed) from g17's perturbed estimates: the minimiser of the reference's mapping
  cost (golden g17min: the real ``photomeric_cost_batch`` loop from the ground truth with decaying learning rates until settled)
  inside the north-star bar;
* the loop semantics both share with the reference (fixed / frozen parts untouched, rotations orthonormal after the fold-in +
  renormalisation, monotone accepted losses, a converged window ignores further launches)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import T, npy
from parity_util import rot_angle

pytestmark = pytest.mark.gpu


def test_mode2_normal_equations_with_affine_columns_match_oracle_jacobian():
    from oracle import gn_oracle, photometric_oracle as orc
    from super_primitive_amd import _lib, synth
    from super_primitive_amd.optim.pair_batch import PairBatch
    pairs = [synth.make_pair(48, 64, 6, seed=21 + k, shape=("grid", "blobs")[k], init_sigma=0.01) for k in range(2)]
    batch = PairBatch.from_synth(pairs, levels=(0, 1), tile_points=512, use_affine=True, device="cuda:0", depth_table=False)    # (mode 2 reads log-depth tables)
    aff = np.array([[0.03, -0.02, -0.05, 0.04], [-0.02, 0.01, 0.06, -0.03]], dtype=np.float32)         # {a_s, b_s, a_t, b_t} per pair
    batch.aff.copy_(T(aff))
    NV, NS = _lib.SP_GNA_PARTIAL_FLOATS, _lib.SP_GNA_SEG_FLOATS
    partials = torch.zeros(batch.n_spans * NV, dtype=torch.float32, device=batch.device)
    seg_partials = torch.zeros(batch.n_seg_records * NS, dtype=torch.float32, device=batch.device)
    _lib.check(batch.lib.sp_pairs_cost(_lib.ptr(batch.desc[0]), _lib.ptr(batch.chunks), _lib.ptr(batch.spans), batch.n_spans, 2, 1e-3,
                                       _lib.ptr(partials), _lib.ptr(seg_partials), _lib.stream_ptr()), "sp_pairs_cost")
    torch.cuda.synchronize()
    span = npy(partials).reshape(-1, NV).astype(np.float64)
    segp = npy(seg_partials).reshape(-1, NS).astype(np.float64)
    span_pair, seg_rec = npy(batch.span_pair), npy(batch.seg_records)
    iu = np.triu_indices(6)
    for m, p in enumerate(pairs):
        N = batch.Ns[m]
        s = span[span_pair == m].sum(0)
        H = np.zeros((8 + N, 8 + N))                       # x = [xi(6), kld(N), a_t, b_t]
        b = np.zeros(8 + N)
        Hpp = np.zeros((6, 6)); Hpp[iu] = s[1:22]
        H[:6, :6] = Hpp + np.triu(Hpp, 1).T
        b[:6] = s[22:28]
        A, B = 6 + N, 7 + N
        H[A, A], H[A, B], H[B, A], H[B, B] = s[29], s[30], s[30], s[31]
        b[A], b[B] = s[32], s[33]
        H[:6, A] = H[A, :6] = s[34:40]
        H[:6, B] = H[B, :6] = s[40:46]
        for r in np.nonzero(seg_rec[:, 0] == m)[0]:
            n, q = 6 + seg_rec[r, 1], segp[r]
            H[:6, n] += q[0:6]; H[n, :6] += q[0:6]
            H[n, n] += q[6]; b[n] += q[7]
            H[n, A] += q[8]; H[A, n] += q[8]; H[n, B] += q[9]; H[B, n] += q[9]
        src, trg = orc.frames_from_synth(p)
        want = gn_oracle.normal_equations(src, trg, torch.from_numpy(p.kld_init), torch.from_numpy(p.pose_init), eps=1e-3,
                                          affine=(torch.from_numpy(aff[m, :2]), torch.from_numpy(aff[m, 2:])), with_affine=True)
        Hw, bw = want["H"].numpy(), want["b"].numpy()
        np.testing.assert_allclose(s[0] / (3.0 * batch.Ps[m]), want["cost"], rtol=2e-5)
        blocks = {"H_pp": np.s_[:6, :6], "H_pd": np.s_[:6, 6:A], "H_dd": np.s_[6:A, 6:A], "H_aa": np.s_[A:, A:], "H_pa": np.s_[:6, A:],
                  "H_da": np.s_[6:A, A:]}
        for name, sl in blocks.items():
            assert np.abs(H[sl] - Hw[sl]).max() <= 3e-3 * np.abs(Hw[sl]).max(), (name, m)
        for name, sl in (("b_p", np.s_[:6]), ("b_d", np.s_[6:A]), ("b_a", np.s_[A:])):
            assert np.abs(b[sl] - bw[sl]).max() <= 3e-3 * np.abs(bw[sl]).max(), (name, m)


def _config3(g):
    from test_gpu_fullsize import config3_inputs
    return config3_inputs(g)


def test_config3_tracking_by_gauss_newton_reaches_the_reference_result_in_15_iterations():
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import track_frame_gn
    g = load_golden("g17_config3_tum_shaped")
    frames, est, klds, affs, kfs = _config3(g)
    dev = kfs[0].image.device
    supp = KeyFrame(T(frames[1].image), T(frames[1].K))
    supp_T, aff, losses, its = track_frame_gn(kfs[0], T(frames[0].kld_gt), supp, T(est[1]), T(est[0]), (0, 3),
                                              prev_aff=torch.zeros(2, device=dev), curr_aff=torch.zeros(2, device=dev))
    L = np.array([float(l) for l in losses])
    print("\ntracking losses: " + " ".join(f"{v:.6f}" for v in L))
    print(f"tracking by Gauss-Newton: {its} iterations, loss {L[0]:.6f} -> {L[-1]:.6f}; vs the reference's converged result: "
          f"rot {rot_angle(npy(supp_T), g['track_polished_supp_T']):.2e} rad, t {np.abs(npy(supp_T)[:3, 3] - g['track_polished_supp_T'][:3, 3]).max():.2e}, "
          f"affine {np.abs(npy(aff) - g['track_polished_aff']).max():.2e}")
    assert its <= 15
    assert rot_angle(npy(supp_T), g["track_polished_supp_T"]) <= 1e-4
    np.testing.assert_allclose(npy(supp_T)[:3, 3], g["track_polished_supp_T"][:3, 3], atol=1e-4)
    np.testing.assert_allclose(npy(aff), g["track_polished_aff"], atol=2e-4)
    R = npy(supp_T)[:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
    # the reference's own loss at its converged point (finest level) is what LM ends at
    np.testing.assert_allclose(L[-1], g["track_polished_losses"][-1], rtol=2e-3)


def test_config3_mapping_by_gauss_newton_reaches_the_minimiser_of_the_reference_cost():
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import map_window
    g = load_golden("g17_config3_tum_shaped")
    gm = load_golden("g17min_config3_mapping_minimiser")
    frames, est, klds, affs, kfs = _config3(g)
    klds = [frames[0].kld_gt.copy()] + list(klds[1:])        # the frozen oldest depths are exact in g17min (its docstring); the rest is g17's
    supp = [[(KeyFrame(T(frames[2 * k + 1].image), T(frames[2 * k + 1].K)), T(est[2 * k + 1]), T(affs[2 * k + 1]))] for k in range(3)]
    out = map_window(kfs, [T(est[2 * k]) for k in range(3)], [T(k) for k in klds], [T(affs[2 * k]) for k in range(3)], supp,
                     40, window_size=3, initialised=True, optimiser="gn")
    L = np.array([float(l) for l in out["losses"]])
    poses = np.concatenate([npy(out["kf_poses"]), np.stack([npy(p) for row in out["supp_poses"] for p in row])])
    want = np.concatenate([gm["min_kf_poses"], gm["min_supp_poses"]])
    rot = max(rot_angle(a, b) for a, b in zip(poses, want))
    tt = float(np.abs(poses[:, :3, 3] - want[:, :3, 3]).max())
    dd = float(np.abs(np.expm1(np.stack([npy(k) for k in out["klds"]]).astype(np.float64) - gm["min_klds"])).max())
    print(f"\nmapping by Gauss-Newton: {out['stopped']} iterations ({out['gn']}), loss {L[0]:.7f} -> {L[-1]:.7f} (reference minimiser "
          f"{gm['losses'][-1]:.7f}); vs the minimiser: rot {rot:.2e} rad, t {tt:.2e}, depth {dd:.2e}")
    assert rot <= 1e-4 and tt <= 1e-4 and dd <= 1e-3
    np.testing.assert_allclose(L[-1], gm["losses"][-1], rtol=2e-3)
    assert np.array_equal(npy(out["kf_poses"][0]), est[0])                   # first keyframe fixed (odometery.py:589-592)
    assert np.array_equal(npy(out["klds"][0]), klds[0])                      # full window: oldest depths frozen (:594-603)
    assert np.array_equal(npy(out["affs"][0]), affs[0])
    for P in poses:
        np.testing.assert_allclose(P[:3, :3] @ P[:3, :3].T, np.eye(3), atol=1e-6)
    # LM: a loss above the last accepted one is a rejected evaluation and is followed by the accepted loss again (the step is undone)
    best = np.minimum.accumulate(L)
    assert L[-1] < 0.5 * L[0] and L[-1] <= best[-1] * (1 + 1e-6)
    for i in range(1, len(L) - 1):
        if L[i] > best[i - 1] * (1 + 1e-6):
            np.testing.assert_allclose(L[i + 1], best[i - 1], rtol=1e-5)


def test_window_gn_freezes_when_converged_and_undoes_rejected_steps():
    """LM bookkeeping on a small tracking window: (a) after convergence further launches change nothing; (b) with lm_down = 1
    and a huge initial step (lambda tiny on a far start) a rejected step restores the previous point exactly."""
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.window import KIND_WINDOW, PoseWindow
    pair = synth.make_pair(60, 80, 6, seed=9, init_sigma=0.01, overlap=1)
    t = lambda a: T(np.ascontiguousarray(a))
    kf = KeyFrame(t(pair.src_image), t(pair.K), t(pair.logdepth_perseg), t(pair.keypoints), t(pair.keypoint_regions))
    eye = torch.eye(4, device=kf.image.device)
    supp_T0 = torch.linalg.inv(t(pair.pose_init))            # relative pose inv(T_supp) T_prev = pose_init
    nodes = [dict(T=eye, kind=KIND_WINDOW), dict(T=supp_T0, kind=KIND_WINDOW, lr_pose=1.0, image=t(pair.trg_image), K=t(pair.K))]
    win = PoseWindow([dict(kf=kf, kld=t(pair.kld_gt), lr=0.0, node=0)], nodes, [(0, 1, 1.0, dense_optim.Z_MIN_SINGLE)], (0, 1), max_iters=64)
    n = win.run_gn(0, 30, conv_tol=1e-4)
    assert win.gn_converged() and n < 30
    before = (win.node_poses().clone(), win.gn_iterations())
    for _ in range(3):
        win.gn_step(0, conv_tol=1e-4)
    assert torch.equal(win.node_poses(), before[0]) and win.gn_iterations() == before[1]
    P = npy(torch.linalg.inv(win.node_poses()[1]))
    assert rot_angle(P, pair.pose_gt) < 2e-3
    # (b) the losses of accepted points never increase; a rejected evaluation is followed by the previous loss again
    L = npy(win.gn_losses())
    st = win.gn_stats()
    assert st["accepted"] + st["rejected"] >= len(L) - 1
    for i in range(1, len(L) - 1):
        if L[i] > L[i - 1] * (1 + 1e-6):
            np.testing.assert_allclose(L[i + 1], L[i - 1], rtol=1e-6)


def test_host_copy_of_the_lm_state_is_the_devices_after_every_kind_of_call():
    """The window keeps a pinned copy of its 16-float LM state and flags for when that copy is current; four calls move the device's state:
    ``gn_step``, ``run_gn``, ``PoseWindowBatch.run_gn`` and ``ChainStep.run(TRACK)`` through a ``GnTracker``.  After each of them, and
    whatever came before, ``gn_stats`` / ``gn_iterations`` / ``gn_converged`` report the device's state as read here directly, and ``run_gn``
    counts its iterations from the device's counter (a ``gn_step`` since the last look included).  On the 60 x 80, 6-segment, one-edge
    tracking window of the test above."""
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.chain import TRACK, ChainStep
    from super_primitive_amd.odometery.loops import GnTracker
    from super_primitive_amd.optim.window import KIND_WINDOW, PoseWindow, PoseWindowBatch
    pair = synth.make_pair(60, 80, 6, seed=9, init_sigma=0.01, overlap=1)
    t = lambda a: T(np.ascontiguousarray(a))
    kf = KeyFrame(t(pair.src_image), t(pair.K), t(pair.logdepth_perseg), t(pair.keypoints), t(pair.keypoint_regions))
    frame = KeyFrame(t(pair.trg_image), t(pair.K))
    eye = torch.eye(4, device=kf.image.device)
    supp_T0 = torch.linalg.inv(t(pair.pose_init))

    def build():
        nodes = [dict(T=eye, kind=KIND_WINDOW), dict(T=supp_T0, kind=KIND_WINDOW, lr_pose=1.0, image=frame.image, K=frame.K)]
        return PoseWindow([dict(kf=kf, kld=t(pair.kld_gt), lr=0.0, node=0)], nodes, [(0, 1, 1.0, dense_optim.Z_MIN_SINGLE)], (0, 1), max_iters=64)

    def device_state(win):
        return npy(win._gn_state()['state'])                 # (the device's copy itself, behind the accessors' back)

    def check(win, what):
        st = device_state(win)
        want = dict(lam=float(st[0]), accepted=int(st[2]), rejected=int(st[3]), iterations=int(st[5]), converged=bool(st[6]),
                    failed_solves=int(st[8]), too_many_unknowns=bool(st[9]))
        assert win.gn_iterations() == want["iterations"] and win.gn_converged() == want["converged"], what
        assert win.gn_stats() == want, (what, win.gn_stats(), want)
        return want

    def counted(win, run, what):
        """``run()`` returns the iterations it took: the device's counter after minus before."""
        before = int(device_state(win)[5])
        n = run()
        assert n == check(win, what)["iterations"] - before, what
        return n

    win = build()
    win.gn_step(0, conv_tol=1e-4)                            # the first call of all: nothing has been looked at yet
    assert check(win, "gn_step on a fresh window")["iterations"] == 1
    counted(win, lambda: win.run_gn(0, 2, conv_tol=1e-4), "run_gn after gn_step")      # (the step above moved the counter)
    seen = check(win, "run_gn, looked at twice")
    win.gn_step(0, conv_tol=1e-4)                            # the pinned copy run_gn left is no longer current
    assert check(win, "gn_step after run_gn")["iterations"] == seen["iterations"] + (0 if seen["converged"] else 1)
    win.gn_step(0, conv_tol=1e-4)
    assert counted(win, lambda: win.run_gn(0, 30, conv_tol=1e-4), "run_gn to convergence") < 30 and win.gn_converged()

    two = [build(), build()]
    batch = PoseWindowBatch(two)
    two[1].gn_step(0, conv_tol=1e-4)                         # (one of the two with a step the host has not seen)
    batch.run_gn(0, 2, conv_tol=1e-4)
    assert all(check(w, "batch of two, two rounds")["iterations"] >= 2 for w in two)
    batch.reset_gn()
    batch.run_gn(0, 30, conv_tol=1e-4)
    assert all(check(w, "batch of two to convergence")["converged"] for w in two)

    trk = GnTracker(kf, t(pair.kld_gt), eye, frame, (0, 1))
    chain = ChainStep(2, 60, 80, 1, kf.image.device)
    chain.bind_tracker(trk, kf, False)
    trk.win.gn_step(0, conv_tol=1e-4)                        # (a step the host has not seen, then the call resets and runs the schedule)
    its, _, _ = chain.run(TRACK, i=1, image=frame.image, start_pose=supp_T0)
    st = check(trk.win, "ChainStep.run(TRACK)")
    assert its == st["iterations"] > 0
    torch.cuda.synchronize()


def test_gn_tracker_reuses_one_window_per_keyframe_with_identical_results():
    """GnTracker (one PoseWindow per keyframe; per frame only the target pyramid, two poses and the LM state change) returns
    bitwise what a freshly built window (track_frame_gn) returns, frame after frame, also after the keyframe was updated."""
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import GnTracker, track_frame_gn
    g = load_golden("g17_config3_tum_shaped")
    frames, est, klds, affs, kfs = _config3(g)
    dev = kfs[0].image.device
    z2 = torch.zeros(2, device=dev)
    targets = [KeyFrame(T(frames[i].image), T(frames[i].K)) for i in (1, 2, 1)]
    inits = [T(est[1]), T(est[2]), T(est[1])]
    kld = T(frames[0].kld_gt)
    trk = GnTracker(kfs[0], kld, T(est[0]), targets[0], (0, 3), kf_aff=z2)
    for k, (f, T0) in enumerate(zip(targets, inits)):
        if k == 2:                       # the keyframe moved (as after a mapping pass)
            kld = kld + 0.01
            trk.update_keyframe(kld, T(est[0]), z2)
        a = trk.track(f, T0, z2)
        b = track_frame_gn(kfs[0], kld, f, T0, T(est[0]), (0, 3), prev_aff=z2, curr_aff=z2)
        dT, da = float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())
        if k < 2:
            assert dT == 0.0 and da == 0.0 and a[3] == b[3], (k, dT, da, a[3], b[3])
            assert all(float(x) == float(y) for x, y in zip(a[2], b[2]))
        else:
            # new depths: a fresh window re-samples the source colours at the re-projected pixel (a last-bit matter), the tracker keeps
            # its samples -- the same minimum to fp32 noise
            assert dT <= 2e-6 and da <= 2e-6, (k, dT, da)


# ---------------------------------------------------------------------------------------------------------------------------------
# Round 4: windows at the reference's extent (config/tum/odom_desk.yaml window_size 5, supporting frames with free poses and affine
# pairs), beyond it (the reduced camera system no longer fits LDS), the supplementary mapping, failed factorisations
# ---------------------------------------------------------------------------------------------------------------------------------
def _extent_window(seed, n_kf, n_supp, n_run, exact_first=True, **kw):
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    frames, kfi, si, est, klds, affs = synth.reference_window_inputs(seed, n_kf, n_supp, n_run, **kw)
    if exact_first:
        klds = [frames[kfi[0]].kld_gt.copy()] + list(klds[1:])       # the frozen oldest depths are exact (as in g17min / g22min)
    kfs = [KeyFrame(T(frames[i].image), T(frames[i].K), T(frames[i].logdepth_perseg), T(frames[i].keypoints), T(frames[i].keypoint_regions)) for i in kfi]
    supp = [[(KeyFrame(T(frames[j].image), T(frames[j].K)), T(est[j]), T(affs[j])) for j in row] for row in si]
    return frames, kfi, si, est, klds, affs, kfs, supp


def _window_errors(out, want_kf, want_supp, want_klds):
    poses = np.concatenate([npy(out["kf_poses"]), np.stack([npy(p) for row in out["supp_poses"] for p in row])])
    want = np.concatenate([want_kf, want_supp])
    rot = max(rot_angle(a, b) for a, b in zip(poses, want))
    tt = float(np.abs(poses[:, :3, 3] - want[:, :3, 3]).max())
    dd = float(np.abs(np.expm1(np.stack([npy(k) for k in out["klds"]]).astype(np.float64) - want_klds)).max())
    return rot, tt, dd


def test_reference_extent_window_by_gauss_newton_reaches_the_minimiser_of_the_reference_cost():
    """5 keyframes (a full window: first pose fixed, oldest depths frozen) x 2 supporting frames + the 2 running ones, affine on: 14 free
    nodes = 112 camera unknowns, 28 photometric terms -- the window of config/tum/odom_desk.yaml (window_size 5, supp_every_n 3,
    opt_supporting).  Golden g22min = the minimiser of the REAL reference cost on it (its loop from the ground truth with decaying rates);
    Gauss-Newton must land there from the perturbed estimates.  (Round 3 raised ValueError above 128 unknowns and had no test here.)"""
    from super_primitive_amd.odometery.loops import map_window
    gm = load_golden("g22min_config3_window5_minimiser")
    n_kf, n_supp, n_run = (int(v) for v in gm["window"])
    frames, kfi, si, est, klds, affs, kfs, supp = _extent_window(int(gm["seed"]), n_kf, n_supp, n_run)
    out = map_window(kfs, [T(est[i]) for i in kfi], [T(k) for k in klds], [T(affs[i]) for i in kfi], supp, 40, window_size=5, initialised=True,
                     optimiser="gn", gn_schedule=dict(profile=True))
    L = np.array([float(l) for l in out["losses"]])
    rot, tt, dd = _window_errors(out, gm["min_kf_poses"], gm["min_supp_poses"], gm["min_klds"])
    print(f"\nreference-extent window (112 camera unknowns) by Gauss-Newton: {out['stopped']} iterations ({out['gn']}), loss {L[0]:.7f} -> {L[-1]:.7f} "
          f"(reference minimiser {gm['losses'][-1]:.7f}); vs the minimiser: rot {rot:.2e} rad, t {tt:.2e}, depth {dd:.2e}; update kernel {out['gn_profile']}")
    assert not out["gn"]["too_many_unknowns"] and out["gn"]["failed_solves"] == 0
    assert rot <= 1e-4 and tt <= 1e-4 and dd <= 1e-3
    assert L[-1] <= gm["losses"][-1] * (1 + 2e-3)              # (at or below the loss the reference's own Adam settles at)
    assert np.array_equal(npy(out["kf_poses"][0]), est[0]) and np.array_equal(npy(out["klds"][0]), klds[0]) and np.array_equal(npy(out["affs"][0]), affs[0])


@pytest.mark.parametrize("n_supp,n_y", [(3, 144), (4, 176), (6, 240)])
def test_windows_beyond_the_reference_extent_solve_without_exception(n_supp, n_y):
    """More supporting frames per keyframe than the reference selects: 144 / 176 camera unknowns (packed triangle in LDS, the <192>
    instantiation) and 240 (the reduced system in global scratch).  No golden at these sizes: the end state is compared with the synthetic
    ground truth (the minimiser of g22min's window sits 1e-4 from it) and with the same window solved by the fused Adam schedule."""
    from super_primitive_amd.odometery.loops import map_window
    frames, kfi, si, est, klds, affs, kfs, supp = _extent_window(301, 5, n_supp, 2)
    args = (kfs, [T(est[i]) for i in kfi], [T(k) for k in klds], [T(affs[i]) for i in kfi], supp)
    out = map_window(*args, 40, window_size=5, initialised=True, optimiser="gn")
    assert 8 * (4 + sum(len(r) for r in si)) == n_y
    gt_kf = np.stack([frames[i].T_wc for i in kfi]); gt_supp = np.stack([frames[j].T_wc for row in si for j in row])
    gt_kld = np.stack([frames[i].kld_gt for i in kfi]).astype(np.float64)
    rot, tt, dd = _window_errors(out, gt_kf, gt_supp, gt_kld)
    L = [float(l) for l in out["losses"]]
    print(f"\n{n_y} camera unknowns: {out['stopped']} iterations, loss {L[0]:.6f} -> {L[-1]:.6f}, vs ground truth rot {rot:.2e} t {tt:.2e} depth {dd:.2e}; {out['gn']}")
    assert not out["gn"]["too_many_unknowns"] and out["gn"]["failed_solves"] == 0
    assert L[-1] < 0.1 * L[0] and rot <= 5e-4 and tt <= 1e-3 and dd <= 3e-3


@pytest.mark.parametrize("n_kf,n_supp,n_run,affine,n_y", [(3, 2, 2, True, 64), (4, 4, 1, True, 128), (5, 5, 0, True, 192), (5, 2, 1, False, 78)])
def test_camera_systems_at_the_edges_of_the_factorisation(n_kf, n_supp, n_run, affine, n_y):
    """The update kernel's factorisation keeps the reduced camera system in registers over a 16 x 16 thread grid, one instantiation per
    capacity (64 / 128 / 192 unknowns in LDS) and four pivots per block step: windows whose system FILLS an instantiation (no spare row
    or column) and one whose size is not a multiple of four (13 free poses without affine pairs = 78: a last block of two pivots)."""
    from super_primitive_amd.odometery.loops import map_window
    frames, kfi, si, est, klds, affs, kfs, supp = _extent_window(311, n_kf, n_supp, n_run)
    if not affine:
        supp = [[(kf, pose, None) for kf, pose, _ in row] for row in supp]
    out = map_window(kfs, [T(est[i]) for i in kfi], [T(k) for k in klds], [T(affs[i]) for i in kfi] if affine else None, supp, 40,
                     window_size=n_kf, initialised=True, optimiser="gn")
    assert (8 if affine else 6) * (n_kf - 1 + sum(len(r) for r in si)) == n_y
    gt_kf = np.stack([frames[i].T_wc for i in kfi]); gt_supp = np.stack([frames[j].T_wc for row in si for j in row])
    gt_kld = np.stack([frames[i].kld_gt for i in kfi]).astype(np.float64)
    rot, tt, dd = _window_errors(out, gt_kf, gt_supp, gt_kld)
    L = [float(l) for l in out["losses"]]
    print(f"\n{n_y} camera unknowns: {out['stopped']} iterations, loss {L[0]:.6f} -> {L[-1]:.6f}, vs ground truth rot {rot:.2e} t {tt:.2e} depth {dd:.2e}; {out['gn']}")
    assert not out["gn"]["too_many_unknowns"] and out["gn"]["failed_solves"] == 0
    assert L[-1] < 0.1 * L[0] and rot <= 5e-4 and tt <= 1e-3 and dd <= 3e-3


def test_supplementary_mapping_moves_only_the_latest_keyframes_depths():
    """mode 'supp' (odometery.py:1038-1042; parameter groups :616-619,628-635; connectivity :467-469) against golden g9e (the real
    ``photomeric_cost_batch`` loop, 12 Adam steps): eager and fused engines follow the reference's losses and end depths, nothing but the
    latest keyframe's depths moves; the Gauss-Newton engine (no camera unknown at all: a diagonal solve) ends below Adam's loss."""
    from super_primitive_amd.odometery.loops import map_window
    g = load_golden("g9e_traj_supp")
    seed, n_kf, n_supp, n_run, H, W, N, steps = (int(v) for v in g["cfg"])
    frames, kfi, si, est, klds, affs, kfs, supp = _extent_window(seed, n_kf, n_supp, n_run, exact_first=False, H=H, W=W, N=N)
    assert np.array_equal(np.stack(est), g["in_poses"]) and np.array_equal(np.stack(klds), g["in_klds"])
    args = (kfs, [T(est[i]) for i in kfi], [T(k) for k in klds], [T(affs[i]) for i in kfi], supp)
    for fused in (False, True):
        out = map_window(*args, steps, window_size=5, initialised=True, fused=fused, mode="supp")
        L = np.array([float(l) for l in out["losses"]])
        np.testing.assert_allclose(L, g["supp_losses"], rtol=2e-5)
        np.testing.assert_allclose(np.stack([npy(k) for k in out["klds"]]), g["supp_klds"], atol=2e-5)
        assert all(np.array_equal(npy(out["klds"][k]), klds[k]) for k in range(n_kf - 1))
        np.testing.assert_allclose(npy(out["kf_poses"]), g["supp_kf_poses"], atol=2e-6)
        np.testing.assert_allclose(np.stack([npy(p) for row in out["supp_poses"] for p in row]), g["supp_supp_poses"], atol=2e-6)
        np.testing.assert_allclose(npy(out["affs"]), g["supp_affs"], atol=1e-7)
    out = map_window(*args, steps, window_size=5, initialised=True, optimiser="gn", mode="supp")
    Lg = [float(l) for l in out["losses"]]
    print(f"\nsupplementary mapping: Adam {g['supp_losses'][0]:.6f} -> {g['supp_losses'][-1]:.6f} in {steps} steps; Gauss-Newton {Lg[0]:.6f} -> {Lg[-1]:.6f} in {len(Lg)} ({out['gn']})")
    assert Lg[-1] < g["supp_losses"][-1] and not out["gn"]["too_many_unknowns"]
    assert all(np.array_equal(npy(out["klds"][k]), klds[k]) for k in range(n_kf - 1)) and not np.array_equal(npy(out["klds"][-1]), klds[-1])
    np.testing.assert_allclose(npy(out["kf_poses"]), np.stack([est[i] for i in kfi]), atol=1e-6)


def test_failed_factorisation_is_a_rejected_step_not_a_convergence():
    """a failed Cholesky used to be followed by a false 'converged' (same point, same loss, 0 <= tol).  Force one:
    a negative lambda makes the damped diagonal negative; lm_up < 0 flips it positive for the next solve.  The window must not freeze on
    the failed call, must count it, and must then take an accepted step that lowers the loss."""
    from super_primitive_amd import synth
    from super_primitive_amd.core import dense_optim
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.window import KIND_WINDOW, PoseWindow
    pair = synth.make_pair(60, 80, 6, seed=9, init_sigma=0.01, overlap=1)
    t = lambda a: T(np.ascontiguousarray(a))
    kf = KeyFrame(t(pair.src_image), t(pair.K), t(pair.logdepth_perseg), t(pair.keypoints), t(pair.keypoint_regions))
    eye = torch.eye(4, device=kf.image.device)
    nodes = [dict(T=eye, kind=KIND_WINDOW), dict(T=torch.linalg.inv(t(pair.pose_init)), kind=KIND_WINDOW, lr_pose=1.0, image=t(pair.trg_image), K=t(pair.K))]
    win = PoseWindow([dict(kf=kf, kld=t(pair.kld_gt), lr=0.0, node=0)], nodes, [(0, 1, 1.0, dense_optim.Z_MIN_SINGLE)], (0, 1), max_iters=64)
    win.reset_gn(lam=-3.0)
    P0 = win.node_poses().clone()
    win.gn_step(0, conv_tol=1e-2, lm_up=-1e-4, lm_down=1.0, lm_min=-10.0)               # 1 + lambda < 0: the factorisation fails
    st = win.gn_stats()
    assert st["failed_solves"] == 1 and not st["converged"] and torch.equal(win.node_poses(), P0)
    win.gn_step(0, conv_tol=1e-2, lm_up=-1e-4, lm_down=1.0, lm_min=-10.0)               # same point, lambda = 3e-4 now: NOT a convergence, a step
    st = win.gn_stats()
    assert not st["converged"] and st["failed_solves"] == 1 and not torch.equal(win.node_poses(), P0)
    win.gn_step(0, conv_tol=1e-2, lm_up=8.0, lm_down=1.0)
    L = npy(win.gn_losses())
    assert L[0] == L[1] and L[2] < 0.9 * L[0], L


def test_mono_init_mapping_by_gauss_newton_reaches_the_reference_minimiser():
    """VERDICT r04 item 4(c) / Missing 3: the reference's MONO INITIALISATION mapping (odometery/odometery.py:134-139,578-581,1064-1071,
    config/tum/odom_desk.yaml ``mono_init: True``): two keyframes, UNIT depths, no supporting frames, first pose fixed, all depths free,
    pose rate 1e-2, no early stop.  Golden g23min = that loop through the imported reference functions -- its own 1000 iterations, then
    decaying-rate phases until settled.  The Gauss-Newton window optimiser (``map_window(mode='init', optimiser='gn')``) from the same
    start must reach the settled state inside the north-star bar AFTER REMOVING THE ONE GAUGE of the problem, the monocular scale
    (translations and depths times s, s from the mean log-depth difference)."""
    import os
    import sys
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import map_window
    g = load_golden("g23min_config3_mono_init_minimiser")
    H, W, N = (int(v) for v in g["HWN"])
    # the inputs of oracle/gen_goldens_fullsize.py::mono_init_inputs, regenerated
    rng = np.random.default_rng(int(g["seed"]))
    base = 0.6 * np.array([0.05, -0.02, 0.015, 0.01 * 0.5, -0.015 * 0.5, 0.008 * 0.5])
    twists = [k * base + 0.003 * rng.standard_normal(6) * (k > 0) for k in range(24)]
    seq = synth.make_sequence(H, W, N, [twists[0], twists[int(g["second"])]], keyframe_ids=[0, 1], seed=int(g["seed"]), overlap=1)
    kfs = [KeyFrame(T(f.image), T(f.K), T(f.logdepth_perseg), T(f.keypoints), T(f.keypoint_regions)) for f in seq]
    poses0 = g["start_poses"]
    z = lambda n: torch.zeros(n, device="cuda")
    out = map_window(kfs, [T(p) for p in poses0], [z(N), z(N)], [z(2), z(2)], [[], []], 1000, lr_pose=1e-2, window_size=5, initialised=False,
                     optimiser="gn", mode='init')
    P = npy(out["kf_poses"]).astype(np.float64)
    K = np.stack([npy(k) for k in out["klds"]]).astype(np.float64)

    def gauge_free(poses, klds, ref_klds):
        ls = float(np.mean(ref_klds - klds))
        return (poses[1, :3, 3] - poses[0, :3, 3]) * np.exp(ls), klds + ls

    want_t, want_k = gauge_free(g["min_kf_poses"].astype(np.float64), g["min_klds"].astype(np.float64), g["min_klds"].astype(np.float64))
    got_t, got_k = gauge_free(P, K, g["min_klds"].astype(np.float64))
    rot = rot_angle(P[1], g["min_kf_poses"][1])
    tt = float(np.abs(got_t - want_t).max())
    dd = float(np.abs(np.expm1(got_k - want_k)).max())
    L = np.array([float(l) for l in out["losses"]])
    print(f"\nmono initialisation by Gauss-Newton: {out['stopped']} iterations ({out.get('gn')}), loss {L[0]:.6f} -> {L[-1]:.7f} (reference: after its 1000 "
          f"iterations {g['losses'][999]:.7f}, settled {g['losses'][-1]:.7f}); scale of this run {np.exp(-float(np.mean(K))):.3f}; vs the reference's settled state, "
          f"scale removed: rot {rot:.2e} rad, t {tt:.2e}, depth {dd:.2e}; the reference's settled state vs ground truth {g['err_gt_scale_removed']}")
    assert np.array_equal(npy(out["kf_poses"][0]), poses0[0])               # first keyframe fixed
    assert rot <= 1e-4 and tt <= 1e-4 and dd <= 1e-3


def test_windows_side_by_side_are_bitwise_the_windows_one_at_a_time():
    """``PoseWindowBatch`` (sp_window_gn_run_multi: every launch of a Gauss-Newton iteration covers ALL the windows,
    window = blockIdx.z, the cost pass walks the windows' work lists in one grid) on windows of DIFFERENT extent -- 3 keyframes x 1
    supporting frame (40 camera unknowns), 5 x 2 + 2 running (112), 4 x 1 + 2 (64), affine pairs on, other scenes -- against the same
    windows optimised one at a time (``PoseWindow.run_gn``): poses, affine pairs, log-depths, loss histories and iteration counts of
    every window are BITWISE equal, whichever instantiation of the update kernel the largest window of the batch selects."""
    from super_primitive_amd.odometery.loops import MAP_GN_SCHEDULE, _build_map_window
    from super_primitive_amd.optim.window import PoseWindowBatch
    shapes = [(301, 3, 1, 0), (302, 5, 2, 2), (303, 4, 1, 2), (304, 3, 1, 0), (305, 5, 2, 2)]
    gn = dict(MAP_GN_SCHEDULE)

    def build():
        wins = []
        for seed, n_kf, n_supp, n_run in shapes:
            frames, kfi, si, est, klds, affs, kfs, supp = _extent_window(seed, n_kf, n_supp, n_run, H=96, W=128, N=12)
            win, _, _ = _build_map_window(kfs, [T(est[i]) for i in kfi], [T(k) for k in klds], [T(affs[i]) for i in kfi], supp, 25, 1e-4, n_kf == 5, True, True,
                                          1e-8, 'map', gn)
            wins.append(win)
        return wins

    def phases(run):
        n = run(0, gn['max_iters'], irls_eps=gn['irls_eps'], conv_tol=gn['conv_tol'])
        return n + run(0, gn['polish_max'], irls_eps=gn['polish_eps'], conv_tol=gn['polish_tol'])

    alone = build()
    its = []
    for w in alone:
        w.reset_gn()
        its.append(phases(w.run_gn))
    together = build()
    batch = PoseWindowBatch(together)
    batch.reset_gn()
    rounds = phases(batch.run_gn)
    torch.cuda.synchronize()
    n_y = [w.gn_unknowns for w in together]
    print(f"\n{len(shapes)} windows of {n_y} camera unknowns side by side: {rounds} rounds for the batch; alone {its} iterations")
    assert len(set(n_y)) >= 3 and max(n_y) > 64 > min(n_y)
    for a, b in zip(alone, together):
        assert torch.equal(a.nodes, b.nodes) and torch.equal(a.kld, b.kld)
        assert a.gn_iterations() == b.gn_iterations() and torch.equal(a.gn_losses(), b.gn_losses())
        assert a.gn_converged() == b.gn_converged()
    assert max(its) <= rounds <= max(its) + 2 * 4                 # (the batch runs until its slowest window has been SEEN converged: polled every 4th round)


def test_leaving_out_the_schur_launch_of_a_window_without_free_depths_changes_no_bit():
    """Round 6 (the config-3 chain's per-frame launches): a window whose depth blocks are all fixed -- frame-to-keyframe tracking -- says so in
    ``sp_window_gn_step``'s flags (bit 2, ``PoseWindow.depths_fixed``) and the Schur-term kernel is not launched: its terms are exact zeros,
    so poses, affine pairs, losses and iteration counts are those of the four-launch iteration, bit for bit."""
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import GnTracker
    g = load_golden("g17_config3_tum_shaped")
    frames, est, klds, affs, kfs = _config3(g)
    z2 = torch.zeros(2, device=kfs[0].image.device)
    f = KeyFrame(T(frames[1].image), T(frames[1].K))
    out = {}
    for fixed in (True, False):
        trk = GnTracker(kfs[0], T(frames[0].kld_gt), T(est[0]), f, (0, 3), kf_aff=z2)
        assert trk.win.depths_fixed
        trk.win.depths_fixed = fixed
        res = trk.track(f, T(est[1]), z2)
        out[fixed] = (res[0].clone(), res[1].clone(), torch.stack(res[2]), res[3], trk.win.nodes.clone())
    a, b = out[True], out[False]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and torch.equal(a[4], b[4])


def test_reducing_the_trackers_edge_inside_the_update_kernel_changes_no_bit():
    """Round 6, late: a depth-less window of a few edges (the tracker) has its edges reduced INSIDE ``k_window_gn_update`` instead of in a
    ``k_window_gn_reduce`` launch in front of it, and the per-segment sums -- read by the Schur terms only -- are not made.  Same routine, same
    order of the sums: poses, affine pairs, losses, iteration counts and the whole node array bit for bit those of the separate launch
    (``SP_WGN_NO_INLINE=1``, read by the library per call)."""
    import os
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.loops import GnTracker
    g = load_golden("g17_config3_tum_shaped")
    frames, est, klds, affs, kfs = _config3(g)
    z2 = torch.zeros(2, device=kfs[0].image.device)
    f = KeyFrame(T(frames[1].image), T(frames[1].K))
    out = {}
    try:
        for separate in (False, True):
            if separate:
                os.environ["SP_WGN_NO_INLINE"] = "1"
            else:
                os.environ.pop("SP_WGN_NO_INLINE", None)
            trk = GnTracker(kfs[0], T(frames[0].kld_gt), T(est[0]), f, (0, 3), kf_aff=z2)
            assert trk.win.depths_fixed
            res = trk.track(f, T(est[1]), z2)
            torch.cuda.synchronize()
            out[separate] = (res[0].clone(), res[1].clone(), torch.stack(res[2]), res[3], trk.win.nodes.clone())
    finally:
        os.environ.pop("SP_WGN_NO_INLINE", None)
    a, b = out[False], out[True]
    assert a[3] > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and torch.equal(a[4], b[4])
