"""-m gpu: the helpers of ``csrc/sp_aux.hip`` that turn a segment table into a depth image -- ``sp_depth_splat``, ``sp_depth_splat_mean``,
``sp_segment_reinit`` (with its invisible-segment fill), ``sp_depth_accumulate`` / ``sp_depth_average_finish`` and ``sp_depth_expand`` --
through their public wrappers, against the float64 yardstick ``tests/segment_depth_ref.py``.  ``test_segment_depth_ref_host.py`` pins that
yardstick to the real reference's recorded outputs (g6, g7) and shows, for every input used here, the conditions these tests rest on.

Render.  On every pixel that no ambiguous point can reach (``taint``, DELTA = 1e-3 px; the host test bounds what float32 does to a
position by DELTA / 16 and the excluded share by 2 %): the touched set exactly, the value at rtol 2e-6 of the float64 winner (or of
sum / (c + 1)), the winner decoded by value = the highest point index; bitwise the same on a second call.  Cases: the three scenes at
their ground-truth and start poses (piles of 5 to 8 points), a shift that puts a band of points at u, v in (-1, 0) (truncation toward
zero: column 0 / row 0 receive them), everything behind the camera (exactly zero), NaN log-depths (those points vanish, nothing else
moves), a far pose with a mean pile above 3 for the mean form.
Re-init.  A hand-made 48x80 keyframe (segments of 3000 / 3001 / 257 / 256 / 1 / 0 valid pixels, values of both signs, a plateau across
the median rank, estimates of 0, 5e-7 and 2e-6), its form with two equal results at the fill's median rank, 300 single-row segments,
nothing visible.  The median by RANK in the float64 sorted values, #(v < got - tau) <= (cnt - 1) // 2 < #(v <= got + tau); the mean within
tau = 2e-6; the fill by rank among the float64 results, and bitwise one of the device's own visible results.
Average.  visible = None / all / mixed, one segment at log-depth -20 (dropped by d > 1e-6); depth at rtol 2e-6, invalid exactly; two
halves accumulated separately and added through the ``reduce`` hook are bitwise the single call.
Expand.  Both forms at rtol 2e-6 inside the masks, exactly 1.0 / 0.0 outside; one 520x512 segment (more blocks than the grid's cap)."""
import numpy as np
import pytest
import torch

import segment_depth_ref as ref
from gpu_util import T, npy
from segment_depth_ref import RTOL, TAU

pytestmark = pytest.mark.gpu

_K = np.array([[40.0, 0, 20.0], [0, 40.0, 12.0], [0, 0, 1]], np.float32)      # (the re-init, average and expansion read no intrinsics)


def _keyframe(masks, L, keypoints, K=_K):
    from super_primitive_amd.image.keyframe import KeyFrame
    N, H, W = masks.shape
    return KeyFrame(torch.zeros(3, H, W, device="cuda:0"), T(K), T(L), T(keypoints), T(masks))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- render -------------------------------------------------------------------------------------------------------------------------------
_frames = {}


def _render(name, tag, mean):
    """(device image, yardstick) of one case; the keyframe is shared between the cases that render the same log-depths"""
    from super_primitive_amd.core.depth_render import estimate_depth_kf_native
    p = ref.family(name)
    L, kld, pose = ref.render_cases(name)[tag]
    key = (name, "nan" if tag == "nan" else "clean")
    if key not in _frames:
        _frames[key] = (_keyframe(p.keypoint_regions, L, p.keypoints, p.K), ref.make_table(p.keypoint_regions, L, p.keypoints))
    kf, table = _frames[key]
    run = lambda: npy(estimate_depth_kf_native(kf, T(kld), T(pose), mean=mean))
    return run, ref.splat(table, p.K, kld, pose, mean=mean)


def _check_render(got, r, mean, what):
    ok, hit = ~r.taint, r.count > 0
    assert got.shape == r.image.shape and got.dtype == np.float32
    assert np.array_equal((got != 0)[ok], hit[ok]), f"{what}: touched set differs on {((got != 0) != hit)[ok].sum()} untainted pixels"
    sel = ok & hit
    gap = (np.abs(got - r.image)[sel] / r.image[sel]).max(initial=0.0)
    print(f"\n{what}: {sel.sum()} untainted touched pixels, worst gap {gap:.2e} (rtol {RTOL:.0e}), tainted {r.taint.mean():.4f}")
    assert gap <= RTOL, what
    if not mean:
        # which point won, decoded by value: the highest index among the candidates of a pixel whose depth the pixel holds
        kept = np.nonzero(r.pix >= 0)[0]
        match = np.abs(r.qz[kept] - got.reshape(-1)[r.pix[kept]]) <= RTOL * r.qz[kept]
        decoded = np.full(got.size, -1, np.int64)
        np.maximum.at(decoded, r.pix[kept][match], kept[match])
        assert np.array_equal(decoded.reshape(got.shape)[ok], r.winner[ok]), what


@pytest.mark.parametrize("mean", [False, True], ids=["last", "mean"])
@pytest.mark.parametrize("tag", ["gt", "init", "shift", "far"])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_render_on_every_untainted_pixel(name, tag, mean):
    run, r = _render(name, tag, mean)
    got = run()
    _check_render(got, r, mean, f"{name}/{tag}/{'mean' if mean else 'last'}")
    assert np.array_equal(_bits(got), _bits(run()))                         # collisions are resolved by index / integer sums, not by scheduling
    if tag == "shift":                                                      # u, v in (-1, 0) truncate to 0: the first column and row are hit
        ok = ~r.taint
        assert (got[:, 0] != 0)[ok[:, 0]].sum() >= 3 and (got[0, :] != 0)[ok[0, :]].sum() >= 3
        assert np.array_equal((got[:, 0] != 0)[ok[:, 0]], (r.count[:, 0] > 0)[ok[:, 0]])


@pytest.mark.parametrize("mean", [False, True], ids=["last", "mean"])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_render_of_points_behind_the_camera_is_exactly_zero(name, mean):
    run, r = _render(name, "behind", mean)
    got = run()
    assert not r.image.any() and not _bits(got).any()


@pytest.mark.parametrize("mean", [False, True], ids=["last", "mean"])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_render_drops_nan_points_and_moves_nothing_else(name, mean):
    run, r = _render(name, "nan", mean)
    got = run()
    _check_render(got, r, mean, f"{name}/nan/{'mean' if mean else 'last'}")
    run_clean, clean = _render(name, "init", mean)
    got_clean = run_clean()
    gone = np.isnan(r.qz)
    theirs = np.zeros(got.size, bool)                                        # every pixel a vanished point reaches in the clean render
    theirs[clean.pix[gone & (clean.pix >= 0)]] = True
    theirs = theirs.reshape(got.shape) | clean.taint
    assert np.array_equal(_bits(got)[~theirs], _bits(got_clean)[~theirs])
    assert (got != got_clean).sum() >= 5


# ---- re-init ------------------------------------------------------------------------------------------------------------------------------
def _rank_ok(sorted_vals, got, k):
    return (sorted_vals < got - TAU).sum() <= k < (sorted_vals <= got + TAU).sum()


@pytest.mark.parametrize("mode", ["mean", "median"])
@pytest.mark.parametrize("which", ["keyframe", "tie", "rows"])
def test_segment_reinit(which, mode):
    from super_primitive_amd.odometery.depth_init import segment_based_depth_reinit
    masks, L, kp, est, meta = ref.reinit_rows() if which == "rows" else ref.reinit_keyframe(tie=which == "tie")
    t = ref.make_table(masks, L, kp)
    want, seen, vals = ref.reinit(t, est, mode)
    kf = _keyframe(masks, L, kp)
    est_dev = T(est)
    kld, flags = segment_based_depth_reinit(est_dev, kf, mode=mode, return_info=True)
    assert torch.equal(est_dev, T(est))                                     # the estimate is read, not clamped in place
    got, flags = npy(kld), npy(flags)
    assert got.dtype == np.float32 and flags.dtype == np.bool_
    assert np.array_equal(flags, seen)
    worst = 0.0
    for n in np.nonzero(seen)[0]:
        if mode == "mean":
            worst = max(worst, abs(float(got[n]) - want[n]))
            assert abs(float(got[n]) - want[n]) <= TAU, f"segment {n}: {got[n]} against {want[n]}"
        else:
            assert _rank_ok(vals[n], float(got[n]) - t.kp_L[n], (len(vals[n]) - 1) // 2), f"segment {n} ({len(vals[n])} values): {got[n]} against {want[n]}"
            worst = max(worst, abs(float(got[n]) - want[n]))
    print(f"\n{which}/{mode}: worst gap of a visible segment {worst:.2e} (tau {TAU:.0e})")
    # invisible segments: ONE value, the lower median of the visible results -- by rank in float64, and bitwise one of the device's own
    fill = got[~seen]
    assert len(fill) >= 2 and (_bits(fill) == _bits(fill[:1])).all()
    assert _rank_ok(np.sort(want[seen]), float(fill[0]), (seen.sum() - 1) // 2), f"fill {fill[0]} against {want[~seen][0]}"
    assert (_bits(got[seen]) == _bits(fill[:1])).any()
    if which == "tie" and mode == "median":
        a, b = meta["tied"]
        assert _bits(got[a]) == _bits(got[b]) == _bits(fill[0])
    assert np.array_equal(_bits(got), _bits(npy(segment_based_depth_reinit(T(est), kf, mode=mode))))


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_segment_reinit_with_nothing_visible_is_zeros_and_false_flags(mode):
    """(the reference's torch.median raises on the empty selection; the library reports zeros)"""
    from super_primitive_amd.odometery.depth_init import segment_based_depth_reinit
    masks, L, kp, est, _ = ref.reinit_keyframe()
    est = np.where(est < 1e-6, est, np.float32(5e-7)).astype(np.float32)          # zeros stay, everything else below the threshold
    want, seen, _ = ref.reinit(ref.make_table(masks, L, kp), est, mode)
    assert not seen.any() and not want.any()
    kld, flags = segment_based_depth_reinit(T(est), _keyframe(masks, L, kp), mode=mode, return_info=True)
    assert not npy(flags).any() and not _bits(npy(kld)).any()


# ---- average ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["none", "all", "mixed"])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_depth_average(name, tag):
    from super_primitive_amd.depth_completion.segment_based_completion import average_visible_segments
    p = ref.family(name)
    kld, visible = ref.average_cases(name)[tag]
    t = ref.make_table(p.keypoint_regions, p.logdepth_perseg, p.keypoints)
    want, want_invalid, count = ref.average(t, kld, visible)
    kf = _keyframe(p.keypoint_regions, p.logdepth_perseg, p.keypoints, p.K)
    vis = None if visible is None else T(visible)
    depth, invalid = average_visible_segments(kf, T(kld), vis)
    got, got_invalid = npy(depth), npy(invalid)
    assert got_invalid.dtype == np.bool_ and np.array_equal(got_invalid, want_invalid)
    assert not _bits(got[want_invalid]).any()                                # 0 / (0 + 1e-6)
    gap = (np.abs(got - want)[~want_invalid] / want[~want_invalid]).max()
    print(f"\n{name}/{tag}: worst gap {gap:.2e} (rtol {RTOL:.0e}), {want_invalid.mean():.3f} invalid, up to {count.max()} segments on a pixel")
    assert gap <= RTOL
    # two disjoint halves of the segments, accumulated separately and added as integers: bitwise the single call
    every = np.ones(p.N, bool) if visible is None else visible
    first = every & (np.arange(p.N) % 2 == 0)
    held = []
    average_visible_segments(kf, T(kld), T(first), reduce=lambda s, c: held.extend((s.clone(), c.clone())))
    assert held[0].dtype == torch.int64 and held[1].dtype == torch.int32 and held[0].numel() == held[1].numel() == p.H * p.W

    def add(s, c):
        s += held[0]
        c += held[1]
    depth2, invalid2 = average_visible_segments(kf, T(kld), T(every & ~first), reduce=add)
    assert np.array_equal(_bits(npy(depth2)), _bits(got)) and np.array_equal(npy(invalid2), got_invalid)


# ---- expand -------------------------------------------------------------------------------------------------------------------------------
def _check_expand(masks, L, kp, kld, log_space, what):
    from super_primitive_amd.core import dense_optim
    want = ref.expand(masks, L, kp, kld, log_space)
    args = (T(kld), T(kp), T(masks), T(L)) if log_space else (_keyframe(masks, L, kp), T(kld))
    junk = torch.full(masks.shape, float("nan"), device="cuda:0")            # (freed at once: the output is likely to be allocated over it,
    del junk                                                                 #  so a pixel the kernel skips shows a NaN)
    out = dense_optim.infer_depth_seeds(*args) if log_space else dense_optim.unproject_kf_to_depths(*args)
    got = npy(out)
    assert got.shape == masks.shape and got.dtype == np.float32
    assert (got[~masks] == np.float32(0.0 if log_space else 1.0)).all(), what          # (a negative sum times 0 is -0.0, as in the reference)
    gap = (np.abs(got - want)[masks] / np.abs(want[masks])).max()
    print(f"\n{what}: worst gap {gap:.2e} (rtol {RTOL:.0e})")
    assert gap <= RTOL, what


@pytest.mark.parametrize("log_space", [True, False], ids=["log", "exp"])
@pytest.mark.parametrize("name", list(ref.FAMILIES))
def test_depth_expand(name, log_space):
    p = ref.family(name)
    for kld in (p.kld_gt, p.kld_init):
        _check_expand(p.keypoint_regions, p.logdepth_perseg, p.keypoints, kld, log_space, name)


@pytest.mark.parametrize("log_space", [True, False], ids=["log", "exp"])
def test_depth_expand_beyond_the_grid_cap(log_space):
    _check_expand(*ref.expand_large(), log_space, "520x512")
