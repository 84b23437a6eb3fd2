"""-m gpu: every entry point of the keyframe post-processing stage (csrc/sp_frontend.hip, sp_mask_count as its scan) against the
float64 / numpy yardstick of tests/post_process_ref.py on every pixel, and the whole stage against oracle.frontend_oracle.  The inputs are
those of tests/post_process_cases.py, for which test_post_process_ref_host.py proves what is relied on here: the band in which a float32
evaluation may decide a discontinuity the other way (``ambiguous``) holds at most 0.5 % of the valid pixels, and no pixel of the
full-stage cases."""
import functools

import numpy as np
import pytest
import torch

import post_process_cases as C
import post_process_ref as R
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

SP_EINVAL, SP_ELIMIT = -1, -2


def pp_module():
    from super_primitive_amd.frontend.segment import post_processer as pp
    return pp


def lib_and_ptr():
    from super_primitive_amd import _lib
    return _lib.load(), _lib.ptr


def device_disc(case):
    split, disc = pp_module()._discontinuity(T(case["L"]), T(case["valid"]), case["fs"], case["thr"])
    assert split.dtype == torch.bool and disc.dtype == torch.bool
    return npy(split), npy(disc)


# ---- sp_depth_discontinuity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.DISC_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_discontinuity_equals_float64_outside_the_band(shape):
    """filter_size 1, 3, 5, 7 x threshold 0.1, 0.03 x N 1, 3 at one shape, the mask kinds rotating (37 x 53 adds every kind at 3 / 0.1)."""
    cases = C.disc_cases(shape) + (C.all_masks_case() if shape == C.DISC_SHAPES[-1] else [])
    for case in cases:
        d = R.discontinuity_ref(case["L"], case["valid"], case["fs"], case["thr"])
        split, disc = device_disc(case)
        sure = ~d["ambiguous"]
        wrong = int(((disc != d["disc"]) & sure).sum()), int(((split != d["split"]) & sure).sum())
        print(f"{case['name']}: {int(d['ambiguous'].sum())} ambiguous, {int((disc != d['disc']).sum())} decided the other way, wrong {wrong}")
        assert wrong == (0, 0), case["name"]
        assert np.array_equal(split | disc, case["valid"]) and not (split & disc).any(), case["name"]


def test_discontinuity_on_depth_ramps_whose_slope_is_just_beside_the_threshold():
    for case in C.ramp_cases():
        split, disc = device_disc(case)
        assert (disc[:, :, 1:-1] == case["expect"]).all(), case["name"]
        assert not disc[:, :, 0].any() and not disc[:, :, -1].any() and np.array_equal(split, ~disc)


def test_non_finite_depths_decide_like_the_torch_oracle():
    """NaN at a valid interior pixel and at a valid corner, +inf at another pixel, NaN at an invalid one; filter sizes 1 and 3."""
    from oracle import frontend_oracle as fo
    for case in C.nonfinite_cases():
        want_disc, want_split = fo.discontinuity(torch.from_numpy(case["L"]).clone(), torch.from_numpy(case["valid"]), case["fs"], case["thr"])
        split, disc = device_disc(case)
        assert np.array_equal(disc, want_disc.numpy()) and np.array_equal(split, want_split.numpy()), case["name"]


def test_discontinuity_argument_checks():
    lib, ptr = lib_and_ptr()
    L, v = T(np.zeros((1, 4, 4), np.float32)), T(np.ones((1, 4, 4), np.uint8))
    scratch, split, disc = torch.empty_like(L), torch.empty_like(v), torch.empty_like(v)
    call = lambda N, fs: lib.sp_depth_discontinuity(ptr(L), ptr(v), N, 4, 4, fs, 0.1, ptr(scratch), ptr(split), ptr(disc), None)
    for fs in (0, 2, 4, 6, -1, -3):
        assert call(1, fs) == SP_EINVAL, fs
    assert call(1, 3) == 0
    torch.cuda.synchronize()


def test_grid_limits_are_refused_before_any_launch():
    """N (grid.y of sp_depth_discontinuity) and K (grid.y of sp_build_part_masks) of 65536 at 2 x 2, with correctly sized buffers."""
    lib, ptr = lib_and_ptr()
    n = 65536
    L, v = torch.zeros(n, 2, 2, device="cuda"), torch.ones(n, 2, 2, dtype=torch.uint8, device="cuda")
    scratch, split, disc = torch.full_like(L, 7.0), torch.full_like(v, 7), torch.full_like(v, 7)
    assert lib.sp_depth_discontinuity(ptr(L), ptr(v), n, 2, 2, 3, 0.1, ptr(scratch), ptr(split), ptr(disc), None) == SP_ELIMIT
    labels = torch.ones(1, 2, 2, dtype=torch.int32, device="cuda")
    desc = torch.zeros(n, 3, dtype=torch.int32, device="cuda")
    out = torch.full((n, 2, 2), 7, dtype=torch.uint8, device="cuda")
    assert lib.sp_build_part_masks(ptr(v), ptr(v), ptr(labels), 2, 2, ptr(desc), n, ptr(out), None) == SP_ELIMIT
    torch.cuda.synchronize()
    assert bool((scratch == 7).all()) and bool((split == 7).all()) and bool((disc == 7).all()) and bool((out == 7).all())
    assert lib.sp_depth_discontinuity(ptr(L), ptr(v), 65535, 2, 2, 3, 0.1, ptr(scratch), ptr(split), ptr(disc), None) == 0
    assert lib.sp_build_part_masks(ptr(v), ptr(v), ptr(labels), 2, 2, ptr(desc), 65535, ptr(out), None) == 0
    torch.cuda.synchronize()
    assert bool((split[:65535] == 1).all()) and bool((out[:65535] == 1).all()) and bool((out[65535] == 7).all())


# ---- sp_label_components ------------------------------------------------------------------------------------------------------------
def check_labelling(fg, name):
    want_labels, want_sizes = R.label_ref(fg)
    dev_fg = T(fg)
    for run in range(3):
        labels, sizes = pp_module()._label(dev_fg)
        assert np.array_equal(npy(labels), want_labels), (name, run)
        assert np.array_equal(npy(sizes), want_sizes), (name, run)          # sizes[root], and zero off the roots


@pytest.mark.parametrize("name", sorted(C.label_cases()))
def test_labels_and_sizes_are_exact(name):
    check_labelling(C.label_cases()[name], name)


def test_spiral_over_many_workgroups():
    check_labelling(C.big_spiral(), "spiral_257x259")


# ---- sp_collect_parts ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parts_fixture():
    masks, split = C.parts_case()
    labels, sizes = R.label_ref(split)
    return masks, split, labels, sizes, R.collect_parts_ref(labels, sizes, masks, split)


def collect(cap, rows, sentinel=-77):
    lib, ptr = lib_and_ptr()
    masks, split, labels, sizes, _ = parts_fixture()
    N, H, W = masks.shape
    parts = torch.full((rows, 3), sentinel, dtype=torch.int32, device="cuda")
    n_parts = torch.full((1,), sentinel, dtype=torch.int32, device="cuda")
    bg = torch.full((N,), sentinel, dtype=torch.int32, device="cuda")
    d_labels, d_sizes, d_masks, d_split = T(labels), T(sizes), T(masks.view(np.uint8)), T(split.view(np.uint8))
    rc = lib.sp_collect_parts(ptr(d_labels), ptr(d_sizes), ptr(d_masks), ptr(d_split), N, H, W, cap, ptr(parts), ptr(n_parts), ptr(bg), None)
    assert rc == 0
    return npy(parts), int(n_parts.item()), npy(bg)


def test_collect_parts_lists_every_component_once():
    want_parts, want_n, want_bg = parts_fixture()[4]
    parts, n, bg = collect(cap=want_n + 5, rows=want_n + 5)
    assert n == want_n and np.array_equal(bg, want_bg)
    got = [tuple(int(v) for v in row) for row in parts[:n]]
    assert len(set(got)) == n and set(got) == want_parts
    assert (parts[n:] == -77).all()
    parts, n, bg = collect(cap=want_n, rows=want_n + 5)                      # cap == n_parts: everything fits
    assert n == want_n and {tuple(int(v) for v in row) for row in parts[:n]} == want_parts and (parts[n:] == -77).all()


def test_collect_parts_beyond_cap_reports_the_count_and_writes_nothing_past_cap():
    want_parts, want_n, want_bg = parts_fixture()[4]
    for cap in (1, want_n // 2, want_n - 1):
        parts, n, bg = collect(cap=cap, rows=want_n + 5)
        assert n == want_n and np.array_equal(bg, want_bg)
        got = [tuple(int(v) for v in row) for row in parts[:cap]]
        assert len(set(got)) == cap and set(got) <= want_parts, cap
        assert (parts[cap:] == -77).all(), cap


# ---- sp_build_part_masks ------------------------------------------------------------------------------------------------------------
def test_part_masks_of_every_kind():
    lib, ptr = lib_and_ptr()
    masks, split, labels, sizes, (parts, _, _) = parts_fixture()
    N, H, W = masks.shape
    desc = [(n, 0, root) for n, root, _ in sorted(parts)] + [(n, kind, -1) for n in range(N) for kind in (1, 2)]
    desc += desc[:3] + [desc[0]]                                              # one root used by several parts
    desc = np.array(desc, np.int32)
    out = torch.full((len(desc), H, W), 7, dtype=torch.uint8, device="cuda")
    d_masks, d_split, d_labels, d_desc = T(masks.view(np.uint8)), T(split.view(np.uint8)), T(labels), T(desc)
    assert lib.sp_build_part_masks(ptr(d_masks), ptr(d_split), ptr(d_labels), H, W, ptr(d_desc), len(desc), ptr(out), None) == 0
    want = R.part_masks_ref(masks, split, labels, desc)
    assert np.array_equal(npy(out), want.astype(np.uint8))
    for kind in (0, 1, 2):
        assert want[desc[:, 1] == kind].any()


# ---- sp_mask_count and sp_kth_mask_pixel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.kth_masks()))
def test_every_kth_pixel_of_a_mask(name):
    """K copies of one mask with kth = 0 .. count - 1 reproduce np.argwhere; the scan they use equals numpy's."""
    lib, ptr = lib_and_ptr()
    m = C.kth_masks()[name]
    H, W = m.shape
    count = int(m.sum())
    K = max(count, 1)
    stack = np.broadcast_to(m, (K, H, W)).copy()
    m8 = T(stack.view(np.uint8))
    row_counts = torch.full((K * H,), -5, dtype=torch.int32, device="cuda")
    counts = torch.full((K,), -5, dtype=torch.int32, device="cuda")
    seg_off = torch.full((K + 1,), -5, dtype=torch.int32, device="cuda")
    assert lib.sp_mask_count(ptr(m8), K, H, W, ptr(row_counts), ptr(counts), ptr(seg_off), None) == 0
    want = R.mask_count_ref(stack)
    for got, ref in zip((row_counts, counts, seg_off), want):
        assert np.array_equal(npy(got), ref)
    assert count > 0
    kth = T(np.arange(count, dtype=np.int32))
    rc = torch.full((K, 2), -5, dtype=torch.int32, device="cuda")
    assert lib.sp_kth_mask_pixel(ptr(m8), ptr(row_counts), K, H, W, ptr(kth), ptr(rc), None) == 0
    assert np.array_equal(npy(rc), np.argwhere(m))
    assert tuple(npy(rc)[-1]) == tuple(R.kth_pixel_ref(m, count - 1)) and tuple(npy(rc)[0]) == tuple(R.kth_pixel_ref(m, 0))


def test_mask_count_over_different_masks():
    lib, ptr = lib_and_ptr()
    masks, _ = C.parts_case()                        # four different slices, 19 x 23
    K, H, W = masks.shape
    row_counts, counts, seg_off = (torch.full((n,), -5, dtype=torch.int32, device="cuda") for n in (K * H, K, K + 1))
    d_masks = T(masks.view(np.uint8))
    assert lib.sp_mask_count(ptr(d_masks), K, H, W, ptr(row_counts), ptr(counts), ptr(seg_off), None) == 0
    for got, ref in zip((row_counts, counts, seg_off), R.mask_count_ref(masks)):
        assert np.array_equal(npy(got), ref)


# ---- the whole stage ----------------------------------------------------------------------------------------------------------------
def keyframe_of(sc):
    from super_primitive_amd.image.keyframe import KeyFrame
    H, W = sc["masks"].shape[1:]
    return KeyFrame(torch.zeros(3, H, W, device="cuda"), torch.eye(3, device="cuda"), T(sc["L"]), T(sc["keypoints"]), T(sc["masks"]))


def oracle_stage(sc, ratio, seed, split=None):
    from oracle import frontend_oracle as fo
    from oracle import photometric_oracle as orc
    H, W = sc["masks"].shape[1:]
    frame = orc.OracleFrame(torch.zeros(3, H, W), torch.eye(3), torch.from_numpy(sc["L"]), torch.from_numpy(sc["keypoints"]),
                            torch.from_numpy(sc["masks"]))
    torch.manual_seed(seed)
    masks, L, kps = fo.fix_disconnected(frame, ratio, split=None if split is None else torch.from_numpy(split))
    return masks.numpy(), L.numpy(), kps.numpy()


def pixels(kps, H, W):
    return np.round(0.5 * (np.array([H, W]) - 1.0) * (np.asarray(kps, np.float64) + 1)).astype(int)


def assert_same_stage(got_masks, got_L, got_kps, want, H, W):
    want_masks, want_L, want_kps = want
    assert got_masks.shape == want_masks.shape                                # K
    assert np.array_equal(got_masks, want_masks)                              # every pixel of every mask, in the oracle's order
    assert np.array_equal(got_L.view(np.int32), want_L.view(np.int32))        # bitwise
    rc = pixels(got_kps, H, W)
    assert np.array_equal(rc, pixels(want_kps, H, W))
    assert all(got_masks[k, rc[k, 0], rc[k, 1]] for k in range(len(rc)))
    return rc


@pytest.mark.parametrize("ratio", C.STAGE_RATIOS)
def test_whole_stage_equals_the_oracle(ratio):
    """40 x 50: a segment cut in three, label-0 parts kept and first, a segment with one kept part (whole mask, old keypoint), a dropped
    segment, parts of 2 and 3 pixels around keep_ratio 1e-3 (tests/post_process_cases.py: stage_case)."""
    sc = C.stage_case()
    H, W = C.STAGE_HW
    kf = keyframe_of(sc)
    torch.manual_seed(123)
    new = pp_module().kf_fix_disconnected_regions(kf, area_keep_ratio=ratio)
    want = oracle_stage(sc, ratio, 123)
    assert want[0].shape[0] == sc["expected"][ratio]["K"]
    assert_same_stage(npy(new.keypoint_regions), npy(new.logdepth_perseg), npy(new.keypoints), want, H, W)
    assert npy(new.keypoint_regions).sum((1, 2)).tolist() == sc["expected"][ratio]["sizes"]
    whole = [k for k in range(want[0].shape[0]) if any(np.array_equal(want[0][k], m) for m in sc["masks"])]
    assert whole and all(any(np.array_equal(npy(new.keypoints)[k], kp) for kp in sc["keypoints"]) for k in whole)    # the old keypoint, bitwise
    # the input keyframe is untouched
    assert np.array_equal(npy(kf.keypoint_regions), sc["masks"]) and np.array_equal(npy(kf.keypoints), sc["keypoints"])
    assert np.array_equal(npy(kf.logdepth_perseg), sc["L"])


def test_post_process_kf_enlarges_its_part_list_and_still_equals_the_oracle(monkeypatch):
    """More components than the max(1024, 64 N) rows post_process_kf collects at first: the second, larger collection decides."""
    pp = pp_module()
    ns = C.noisy_split_case()
    H, W = ns["masks"].shape[1:]
    calls = []
    check = pp._lib.check
    monkeypatch.setattr(pp._lib, "check", lambda rc, what: (calls.append(what), check(rc, what))[1])
    torch.manual_seed(5)
    masks, L, kps = pp.post_process_kf(keyframe_of(ns), None, keep_ratio=ns["keep_ratio"], _split=T(ns["split"]))
    assert calls.count("sp_collect_parts") == 2
    want = oracle_stage(ns, ns["keep_ratio"], 5, split=ns["split"])
    assert want[0].shape[0] == 8
    assert_same_stage(npy(masks), npy(L), npy(kps), want, H, W)
