"""The float64 yardstick of the depth render, the segment re-init, the depth average and the dense expansion (tests/segment_depth_ref.py)
kept honest without a GPU: against the recorded outputs of the real reference (goldens g6 and g7), and -- for every input the GPU test
(test_gpu_segment_depth.py) uses -- the conditions under which that test may demand what it demands: the taint margin DELTA covers what
float32 can do to a position, it excludes few pixels, the medians are decisive at the comparison tolerance, the thresholds are far from
every value.  Every figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest

import segment_depth_ref as ref
from conftest import load_golden, unpack_masks
from segment_depth_ref import DELTA, EPS, RTOL, TAU

RENDER = [(name, tag) for name in ref.FAMILIES for tag in ("gt", "init", "shift", "behind", "far", "nan")]


def _rel(got, want):
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-300)


# ---- against the real reference's recorded outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("out,L,kld,pose,mean,cap", [("out_half", "in_L_const", "in_kld_const", "in_pose_half", False, 0.02),
                                                     ("out_general", "in_logdepth", "in_kld_gt", "in_pose_gt", False, 0.02),
                                                     ("out_mean_general", "in_logdepth", "in_kld_gt", "in_pose_gt", True, 0.02),
                                                     ("out_mean_far", "in_logdepth", "in_kld_gt", "in_pose_far", True, 0.06)])
def test_render_is_the_reference_s_on_every_untainted_pixel_of_g6(out, L, kld, pose, mean, cap):
    g = load_golden("g6_depth_render")
    t = ref.make_table(unpack_masks(g), g[L], g["in_keypoints"])
    r = ref.splat(t, g["in_K"], g[kld], g[pose], mean=mean)
    ok, want = ~r.taint, g[out]
    print(f"\n{out}: tainted {r.taint.mean():.4f}, worst gap {_rel(want, r.image)[ok].max():.2e}")
    assert r.taint.mean() <= cap
    assert np.array_equal((want != 0)[ok], (r.count > 0)[ok])
    np.testing.assert_allclose(want[ok], r.image[ok], rtol=RTOL, atol=0)


def test_reinit_average_and_expansion_are_the_reference_s_on_g7():
    g = load_golden("g7_segment_stats")
    masks = unpack_masks(g)
    t = ref.make_table(masks, g["in_logdepth"], g["in_keypoints"])
    for mode in ("mean", "median"):
        kld, seen, _ = ref.reinit(t, g["in_sparse_depth"], mode)
        print(f"\ng7 {mode}: worst gap {np.abs(kld - g[f'{mode}_kld']).max():.2e}")
        assert np.array_equal(seen, g[f"{mode}_visible"])
        np.testing.assert_allclose(kld, g[f"{mode}_kld"], rtol=0, atol=5e-7)
    depth, invalid, _ = ref.average(t, g["median_kld"], g["median_visible"])
    assert np.array_equal(invalid, g["avg_invalid"])
    np.testing.assert_allclose(g["avg_depth"], depth, rtol=2e-6, atol=1e-7)
    dense = ref.expand(masks, g["in_logdepth"], g["in_keypoints"], g["median_kld"], log_space=False)
    np.testing.assert_allclose(dense.sum(), float(g["depths_dense_sum"]), rtol=1e-6)
    np.testing.assert_allclose(g["depths_dense"], dense, rtol=2e-3)                    # (the fixture keeps an fp16 copy)


def test_reinit_semantics_on_cases_written_out_by_hand():
    masks = np.zeros((3, 2, 4), bool)
    masks[0, 0, :], masks[1, 1, :3], masks[2, 1, 3] = True, True, True
    L = np.zeros((3, 2, 4), np.float32)
    L[0, 0] = [0.5, 0.0, 0.0, 0.0]
    kp = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0]], np.float32)                 # pixels (0,0), (1,0), (1,3)
    est = np.array([[np.e, 1.0, np.e ** 2, np.e ** 3], [np.nan, 0.0, 5e-7, 0.0]], np.float32)
    t = ref.make_table(masks, L, kp)
    assert t.kp_L.tolist() == [0.5, 0.0, 0.0]
    kld, seen, vals = ref.reinit(t, est, "median")
    assert seen.tolist() == [True, True, False]                                       # the NaN is a valid estimate, as in the reference
    np.testing.assert_allclose(vals[0], [0.0, 0.5, 2.0, 3.0], atol=1e-6)
    np.testing.assert_allclose(kld[0], 0.5 + 0.5, atol=1e-6)                           # LOWER median of four + kp_L
    assert np.isnan(kld[1])                                                           # ... and its segment's result is NaN
    kld, seen, _ = ref.reinit(t, np.where(np.isnan(est), 0, est), "mean")
    assert seen.tolist() == [True, False, False]
    np.testing.assert_allclose(kld, [5.5 / 4 + 0.5] * 3, atol=1e-6)                    # invisible ones: the median of the visible results
    kld, seen, _ = ref.reinit(t, np.zeros((2, 4), np.float32), "median")
    assert not seen.any() and not kld.any()


# ---- the conditions of the GPU test: render ----------------------------------------------------------------------------------------------
def _case(name, tag):
    p = ref.family(name)
    L, kld, pose = ref.render_cases(name)[tag]
    return p, ref.make_table(p.keypoint_regions, L, p.keypoints), kld, pose


@pytest.mark.parametrize("name,tag", RENDER)
def test_taint_margin_covers_float32_and_excludes_few_pixels(name, tag):
    p, t, kld, pose = _case(name, tag)
    r = ref.splat(t, p.K, kld, pose)
    qz32, u32, v32 = ref.positions(t, p.K, kld, pose, np.float32)
    near = (r.qz > EPS) & (r.u > -2) & (r.u < p.W + 1) & (r.v > -2) & (r.v < p.H + 1)        # every point that could reach the image
    du = np.abs(u32 - r.u)[near].max(initial=0.0)
    dv = np.abs(v32 - r.v)[near].max(initial=0.0)
    dz = _rel(qz32.astype(np.float64), r.qz)[near].max(initial=0.0)
    pile = r.count.sum() / max((r.count > 0).sum(), 1)
    print(f"\n{name}/{tag}: {t.P} points, tainted {r.taint.mean():.4f}, float32 gap du {du:.2e} dv {dv:.2e} px, qz {dz:.2e} rel; "
          f"{(r.count > 1).mean():.3f} of the pixels hit more than once, largest pile {r.count.max()}, mean pile {pile:.2f}")
    assert du <= DELTA / 16 and dv <= DELTA / 16
    assert dz <= RTOL / 4
    assert r.taint.mean() <= 0.02
    assert np.array_equal(r.taint, ref.splat(t, p.K, kld, pose, mean=True).taint)
    assert not np.any(np.abs(r.qz - EPS) < 1e-5)                                            # no point near the depth threshold
    if tag == "behind":
        assert not (r.qz > 0).any() and not r.image.any() and pose[2, 3] < -np.exp(t.L + (kld - t.kp_L)[t.seg]).max()
    elif tag == "far":
        assert pile > 3
    elif tag == "shift":
        # points with u or v in (-1, 0) exist, are unambiguous, and truncation puts them in column 0 / row 0
        for a, size in ((r.u, p.W), (r.v, p.H)):
            band = (a > -1 + DELTA) & (a < -DELTA) & (r.pix >= 0) & ~r.ambiguous
            assert band.sum() >= 10
            line = (r.pix[band] % p.W) if a is r.u else (r.pix[band] // p.W)
            assert not line.any()
            assert len(np.unique(r.pix[band][~r.taint.reshape(-1)[r.pix[band]]])) >= 3         # ... on untainted pixels, which the GPU test reads
    elif tag == "nan":
        gone = np.isnan(r.qz)
        clean = ref.splat(_case(name, "init")[1], p.K, kld, pose)
        assert 50 <= gone.sum() and (clean.pix[gone] >= 0).sum() >= 20                       # they vanish, and they were in the image
        assert (gone[clean.winner[clean.winner >= 0]]).sum() >= 5                            # some of them had won their pixel
    if tag in ("gt", "init", "far"):
        assert (r.count > 1).mean() >= 0.15 and r.count.max() >= 5                           # collisions are plentiful


@pytest.mark.parametrize("name,tag", [(n, t) for n, t in RENDER if t in ("gt", "init", "shift")])
def test_winner_can_be_told_from_the_other_candidates_by_value(name, tag):
    """The GPU test decodes the winner by value: that says something where the winner's depth stands apart from every other candidate's."""
    p, t, kld, pose = _case(name, tag)
    r = ref.splat(t, p.K, kld, pose)
    multi = np.nonzero(((r.count > 1) & ~r.taint).reshape(-1))[0]
    decisive = 0
    for px in multi:
        cand = np.nonzero(r.pix == px)[0]
        w = cand.max()
        decisive += bool(np.all(np.abs(r.qz[cand[cand != w]] - r.qz[w]) > 100 * RTOL * r.qz[w]))
    print(f"\n{name}/{tag}: {len(multi)} untainted pixels with a collision, the winner stands apart on {decisive}")
    # (at the ground truth all segments lie on one plane: colliding points have nearly equal depths; away from it they do not)
    assert decisive >= (20 if tag == "gt" else max(0.9 * len(multi), 50))


# ---- the conditions of the GPU test: re-init ---------------------------------------------------------------------------------------------
def _f32_reinit_gap(t, est, vals64):
    """the values log(est) - L + kp_L with every operation rounded to float32, against float64: the margin below TAU"""
    e = est[t.row, t.col]
    valid = ~(e < np.float32(EPS))
    worst = 0.0
    for n in range(t.N):
        s = slice(t.seg_off[n], t.seg_off[n + 1])
        v32 = np.sort(np.log(e[s][valid[s]]) - t.L[s][valid[s]].astype(np.float32))
        assert v32.dtype == np.float32
        if len(v32):
            worst = max(worst, np.abs(v32 - vals64[n]).max())
            assert np.abs(vals64[n]).max() <= 4.0
    return worst


def _assert_decisive(sorted_vals, what, tied=False):
    k = (len(sorted_vals) - 1) // 2
    lo, hi = max(k - 1, 0), min(k + 1, len(sorted_vals) - 1)
    gaps = np.diff(sorted_vals[lo:hi + 1])
    if tied:
        assert (sorted_vals == sorted_vals[k]).sum() > 1, what                               # the tied value is itself the median
    else:
        assert np.all(gaps >= 100 * TAU), f"{what}: gaps {gaps} around the lower median"


@pytest.mark.parametrize("which", ["keyframe", "tie", "rows"])
def test_reinit_inputs_are_what_they_claim_and_their_medians_decisive(which):
    masks, L, kp, est, meta = ref.reinit_rows() if which == "rows" else ref.reinit_keyframe(tie=which == "tie")
    N, H, W = masks.shape
    t = ref.make_table(masks, L, kp)
    px = ref.keypoint_pixels(kp, H, W)
    assert masks[np.arange(N), px[:, 0], px[:, 1]].all()                                     # every keypoint inside its mask
    assert np.array_equal(px, np.rint(0.5 * (np.array([H, W]) - 1) * (kp.astype(np.float64) + 1)))       # ... on an exact pixel centre
    assert t.P % 256 and t.P > 256
    flat = est.reshape(-1)
    assert (flat == 0).any() and (which == "rows" or (flat == np.float32(5e-7)).any())
    for mode in ("mean", "median"):
        kld, seen, vals = ref.reinit(t, est, mode)
        gap = _f32_reinit_gap(t, est, vals)
        print(f"\n{which}/{mode}: valid pixels per segment {[len(v) for v in vals][:12]}, float32 restatement gap {gap:.2e} (tau {TAU:.0e})")
        assert gap <= TAU / 2
        assert seen.sum() % 2 == 0 and (~seen).sum() >= 2                                    # an even number visible, two or more not
        assert np.array_equal(np.nonzero(~seen)[0], meta["invisible"])
        assert np.all(np.abs(kld) <= 4.0)
        if mode == "median":
            for n in np.nonzero(seen)[0]:
                _assert_decisive(vals[n], f"segment {n}", tied=which != "rows" and n == meta["plateau"])
        res = np.sort(kld[seen])
        if which == "tie":
            a, b = meta["tied"]
            k = (len(res) - 1) // 2
            assert kld[a] == kld[b] == res[k] == res[k - 1] and res[k - 2] < res[k] < res[k + 1]      # rank k is the SECOND of the pair
        else:
            _assert_decisive(res, "fill")
    if which == "rows":
        assert N == 300 and len(meta["invisible"]) > 2 and all(len(v) in (0, 6) for v in vals)
        return
    assert (flat == np.float32(2e-6)).sum() == 5
    counts = [len(v) for v in vals]
    assert counts[:8] == [3000, 3001, 257, 256, 1, 0, 600, 600] and counts[9] == 0
    assert vals[6].min() < -0.2 and vals[6].max() > 0.2                                      # both signs
    plateau = vals[7] == vals[7][(600 - 1) // 2]
    assert plateau.sum() == 150 and 0 < np.nonzero(plateau)[0][0] and np.nonzero(plateau)[0][-1] < 599
    assert set(est[masks[9]].tolist()) == {float(np.float32(5e-7))} and not est[masks[5]].any()
    if which == "keyframe":
        e8, L8 = est[masks[8]], L[8][masks[8]]
        e8, L8 = e8[e8 >= 1e-6], L8[e8 >= 1e-6]
        assert counts[8] == 50 and np.all(e8[np.argsort(np.log(e8.astype(np.float64)) - L8)[-5:]] == np.float32(2e-6))       # its five largest values


# ---- the conditions of the GPU test: average and expansion -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_average_and_expansion_inputs(name):
    p = ref.family(name)
    t = ref.make_table(p.keypoint_regions, p.logdepth_perseg, p.keypoints)
    assert t.P % 256 and (p.H * p.W) % 256 and t.P > 256
    f32 = lambda a: np.asarray(a, np.float32)
    for tag, (kld, visible) in ref.average_cases(name).items():
        d = ref.point_depths(t, kld)
        assert not np.any((d > 1e-7) & (d < 1e-5)) and (d <= 1e-7).any()                     # the threshold is far from every depth
        depth, invalid, count = ref.average(t, kld, visible)
        use = p.keypoint_regions if visible is None else p.keypoint_regions & visible[:, None, None]
        only_dropped = use[2] & (use.sum(0) == 1)
        assert only_dropped.sum() >= 10 and invalid[only_dropped].all() and (count > 1).sum() >= 10
        if tag == "mixed":
            assert visible[2] and not visible.all()
        d32 = np.exp(f32(t.L) + (f32(kld) - f32(t.kp_L))[t.seg])
        gap = _rel(d32.astype(np.float64), d)[d > EPS].max()
        print(f"\n{name}/{tag}: {invalid.mean():.3f} invalid, {only_dropped.sum()} pixels under the dropped segment alone, float32 gap of a depth {gap:.2e}")
        assert gap <= RTOL / 4
    for kld in (p.kld_gt, p.kld_init):
        want = ref.expand(p.keypoint_regions, p.logdepth_perseg, p.keypoints, kld, log_space=True)
        px = ref.keypoint_pixels(p.keypoints, p.H, p.W)
        kp_L = p.logdepth_perseg[np.arange(p.N), px[:, 0], px[:, 1]]
        got32 = (p.logdepth_perseg + (f32(kld) - kp_L)[:, None, None]) * p.keypoint_regions
        m = p.keypoint_regions
        gap = _rel(got32.astype(np.float64), want)[m].max()
        print(f"{name}: float32 gap of a seeded log-depth {gap:.2e}")
        assert gap <= RTOL / 4 and np.abs(want[m]).min() > 0.1


def test_large_expansion_input_exceeds_the_grid_cap():
    masks, L, kp, kld = ref.expand_large()
    N, H, W = masks.shape
    assert N == 1 and (H * W + 255) // 256 > 1024 and masks[0].reshape(-1)[1024 * 256:].any() and not masks.all()
    want = ref.expand(masks, L, kp, kld, log_space=True)
    assert np.abs(want[masks]).min() > 0.1
