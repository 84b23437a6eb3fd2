"""CPU: the yardstick of the keyframe post-processing stage (tests/post_process_ref.py) against the torch oracle, the reference's goldens
and a scipy-free flood fill, and the conditions test_gpu_post_process.py relies on, proved for the very inputs it uses
(tests/post_process_cases.py): the ambiguous band holds at most 0.5 % of the valid pixels of every discontinuity case and nothing in the
full-stage cases."""
import numpy as np
import pytest
import torch

import post_process_cases as C
import post_process_ref as R
from conftest import load_golden
from oracle import frontend_oracle as fo
from oracle import photometric_oracle as orc


def oracle_disc(case):
    disc, split = fo.discontinuity(torch.from_numpy(case["L"]).clone(), torch.from_numpy(case["valid"]), case["fs"], case["thr"])
    return disc.numpy(), split.numpy()


def ambiguous_share(case, d):
    n_valid = int(case["valid"].sum())
    return int(d["ambiguous"].sum()) / max(n_valid, 1)


# ---- the yardstick against the oracle and the goldens -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.DISC_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_discontinuity_ref_matches_the_torch_oracle_and_its_band_is_narrow(shape):
    cases = C.disc_cases(shape) + (C.all_masks_case() if shape == C.DISC_SHAPES[-1] else [])
    for case in cases:
        assert np.abs(case["L"]).max() <= 2
        d = R.discontinuity_ref(case["L"], case["valid"], case["fs"], case["thr"])
        disc, split = oracle_disc(case)
        sure = ~d["ambiguous"]
        assert np.array_equal(disc[sure], d["disc"][sure]) and np.array_equal(split[sure], d["split"][sure]), case["name"]
        share = ambiguous_share(case, d)
        print(f"{case['name']}: ambiguous share {share:.5f}, discontinuities {int(d['disc'].sum())} of {int(case['valid'].sum())} valid")
        assert share <= C.MAX_AMBIGUOUS_SHARE, case["name"]
        assert np.array_equal(d["split"] | d["disc"], case["valid"]) and not (d["split"] & d["disc"]).any()


def test_the_cases_cover_both_sides_of_the_threshold():
    """The comparison is no formality: every filter size and every threshold meets pixels on both sides."""
    seen = {}
    for shape in C.DISC_SHAPES:
        for case in C.disc_cases(shape):
            d = R.discontinuity_ref(case["L"], case["valid"], case["fs"], case["thr"])
            for key in (("fs", case["fs"]), ("thr", case["thr"]), ("shape", shape)):
                n = seen.setdefault(key, [0, 0])
                n[0] += int(d["disc"].sum())
                n[1] += int(d["split"].sum())
    print(seen)
    assert all(n[1] > 0 and (n[0] > 0 or key == ("shape", (2, 2))) for key, n in seen.items()), seen     # 2 x 2: both gradients fold to 0


@pytest.mark.parametrize("tag", ["grid", "blobs"])
def test_yardstick_matches_the_reference_goldens(tag):
    g = load_golden("g10_post_process")
    H, W, N = (int(v) for v in g[f"{tag}_HWN"])
    unpack = lambda a, n: np.unpackbits(a, axis=-1, count=W).astype(bool).reshape(n, H, W)
    masks, L = unpack(g[f"{tag}_masks"], N), g[f"{tag}_L"]
    d = R.discontinuity_ref(L, masks, 3, 0.1)
    sure = ~d["ambiguous"]
    print(f"g10 {tag}: {int(d['ambiguous'].sum())} ambiguous pixels of {int(masks.sum())}")
    assert np.array_equal(d["disc"][sure], unpack(g[f"{tag}_disc"], N)[sure])
    assert np.array_equal(d["split"][sure], unpack(g[f"{tag}_split"], N)[sure])
    labels, sizes = R.label_ref(unpack(g[f"{tag}_split"], N))
    renumbered, n = R.renumber(labels)
    assert n == int(g[f"{tag}_n_labels"]) and np.array_equal(renumbered, g[f"{tag}_labels"])
    assert int(sizes.sum()) == int(unpack(g[f"{tag}_split"], N).sum())


def test_label_ref_matches_a_flood_fill_without_scipy():
    for name, fg in C.label_cases().items():
        labels, sizes = R.label_ref(fg)
        want_labels, want_sizes = R.flood_fill_labels(fg)
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes), name
        assert np.array_equal(labels > 0, fg)
        roots = np.nonzero(sizes)[0]
        assert np.array_equal(labels.reshape(-1)[roots], roots + 1), name


def test_label_shapes_are_what_their_names_say():
    c = C.label_cases()
    n_comp = lambda fg: int((R.label_ref(fg)[1] > 0).sum())
    for name in ("spiral_65x67", "comb_33x41", "serpentine_34x29"):
        labels, sizes = R.label_ref(c[name])
        assert n_comp(c[name]) == 1 and sizes[0] == c[name].sum() and labels.max() == 1, name       # one component, rooted at pixel 0
    assert c["spiral_65x67"].sum() > 65 * 67 // 2 - 70                                               # it fills the slice
    assert n_comp(c["checkerboard_16x18"]) == c["checkerboard_16x18"].sum()
    assert n_comp(c["nested_u_21x40"]) == 10
    assert n_comp(c["full_full_7x9"]) == 2 and n_comp(c["bars_after_full_6x5"]) == 3
    big = C.big_spiral()
    assert n_comp(big) == 1 and big[0, 0, 0] and big.sum() > 257 * 259 // 2 - 300


# ---- analytic pins ------------------------------------------------------------------------------------------------------------------
def test_a_depth_ramp_has_its_slope_as_scharr_magnitude():
    for case in C.ramp_cases():
        d = R.discontinuity_ref(case["L"], case["valid"], case["fs"], case["thr"])
        inner = (slice(None), slice(None), slice(1, -1))
        np.testing.assert_allclose(d["g"][inner], case["slope"], rtol=0, atol=1e-7)
        margin = (np.abs(d["g"] - d["threshold"]) / d["bound"])[inner].min()
        print(f"{case['name']}: {margin:.1f} bands from the threshold")
        assert margin > case["min_bands"]
        assert (d["disc"][inner] == case["expect"]).all() and not d["ambiguous"].any()
        disc, _ = oracle_disc(case)
        assert (disc[inner] == case["expect"]).all()


def test_non_finite_depths_follow_the_torch_oracle():
    """max_pool2d lets a NaN win and conv2d multiplies its zero weights, so a NaN or infinite pooled value anywhere in the 3 x 3 window
    gives a NaN magnitude (no discontinuity) unless every product it enters has the same sign of infinity."""
    for case in C.nonfinite_cases():
        d = R.discontinuity_ref(case["L"], case["valid"], case["fs"], case["thr"])
        disc, split = oracle_disc(case)
        assert np.array_equal(disc, d["disc"]) and np.array_equal(split, d["split"]), case["name"]
        finite = np.isfinite(d["g"]) & case["valid"]
        assert (np.abs(d["g"] - d["threshold"])[finite] > 1000 * d["bound"][finite]).all()       # nothing finite near the threshold
        assert disc[1].any() and np.isnan(d["g"]).any() and np.isinf(d["g"]).any()
        nan_free = case["L"].copy()
        nan_free[~np.isfinite(nan_free)] = 0
        assert (R.discontinuity_ref(nan_free, case["valid"], case["fs"], case["thr"])["disc"] != d["disc"]).any()


# ---- the full stage -----------------------------------------------------------------------------------------------------------------
def stage_frame(sc):
    H, W = sc["masks"].shape[1:]
    return orc.OracleFrame(torch.zeros(3, H, W), torch.eye(3), torch.from_numpy(sc["L"]), torch.from_numpy(sc["keypoints"]),
                           torch.from_numpy(sc["masks"]))


def test_stage_cases_have_an_empty_band_and_the_structure_they_claim():
    sc = C.stage_case()
    d = R.discontinuity_ref(sc["L"], sc["masks"], 3, 0.1)
    print("full stage: ambiguous pixels", int(d["ambiguous"].sum()))
    assert not d["ambiguous"].any()
    disc, split = fo.discontinuity(torch.from_numpy(sc["L"]).clone(), torch.from_numpy(sc["masks"]))
    assert np.array_equal(split.numpy(), d["split"])
    labels, sizes = R.label_ref(d["split"])
    parts, n_parts, bg = R.collect_parts_ref(labels, sizes, sc["masks"], d["split"])
    assert sorted((n, s) for n, _, s in parts) == [(0, 192), (0, 224), (0, 256), (1, 20), (1, 160), (2, 1), (3, 2), (3, 3), (3, 3), (4, 197)]
    assert bg.tolist() == [64, 20, 0, 4, 0]
    for ratio in C.STAGE_RATIOS:
        torch.manual_seed(7)
        masks, L, kps = fo.fix_disconnected(stage_frame(sc), ratio)
        want = sc["expected"][ratio]
        assert masks.shape[0] == want["K"] and masks.sum((1, 2)).tolist() == want["sizes"]
    # at 1e-3 the 2-pixel part of segment 3 sits exactly at the ratio (2 / 2000 > 1e-3 is false in float32) and the 3-pixel parts above it
    assert np.float32(2) / np.float32(2000) == np.float32(1e-3)
    # at 0.05 segment 1 has one kept part: the whole mask and the old keypoint
    torch.manual_seed(7)
    masks, L, kps = fo.fix_disconnected(stage_frame(sc), 0.05)
    assert np.array_equal(masks[3].numpy(), sc["masks"][1]) and np.array_equal(kps[3].numpy(), sc["keypoints"][1])


def test_noisy_split_overflows_the_first_part_list():
    ns = C.noisy_split_case()
    labels, sizes = R.label_ref(ns["split"])
    n_comp = int((sizes > 0).sum())
    assert n_comp > max(1024, 64 * ns["split"].shape[0])
    torch.manual_seed(11)
    masks, L, kps = fo.fix_disconnected(stage_frame(ns), ns["keep_ratio"], split=torch.from_numpy(ns["split"]))
    assert masks.shape[0] == 8          # slice 0: the label-0 part and four blocks; slice 1: its label-0 part and two blocks


def test_select_parts_orders_by_root_whatever_order_the_device_lists_them_in():
    """sp_collect_parts appends in the order its atomics land: _select_parts has to sort.  Fed the stage case's component list reversed
    and shuffled, it must describe the oracle's parts in the oracle's order."""
    from super_primitive_amd.frontend.segment import post_processer as pp
    sc = C.stage_case()
    d = R.discontinuity_ref(sc["L"], sc["masks"], 3, 0.1)
    labels, sizes = R.label_ref(d["split"])
    parts, _, bg = R.collect_parts_ref(labels, sizes, sc["masks"], d["split"])
    rng = np.random.default_rng(0)
    for ratio in C.STAGE_RATIOS:
        torch.manual_seed(7)
        want, _, _ = fo.fix_disconnected(stage_frame(sc), ratio)
        for order in (sorted(parts, reverse=True), [sorted(parts)[i] for i in rng.permutation(len(parts))]):
            chosen, origin = pp._select_parts(5, order, bg, 40 * 50, ratio)
            got = R.part_masks_ref(sc["masks"], d["split"], labels, np.array(chosen))
            assert np.array_equal(got, want.numpy())
            assert [w for _, w in origin] == [bool(np.array_equal(m, sc["masks"][n])) for (n, _), m in zip(origin, got)]


# ---- the small restatements ---------------------------------------------------------------------------------------------------------
def test_small_restatements():
    for name, m in C.kth_masks().items():
        row_counts, counts, seg_off = R.mask_count_ref(np.stack([m, m]))
        H = m.shape[0]
        assert counts.tolist() == [m.sum()] * 2 and seg_off.tolist() == [0, m.sum(), 2 * m.sum()]
        assert row_counts[:H].tolist() == [int(m[:r].sum()) for r in range(H)] and np.array_equal(row_counts[:H], row_counts[H:])
        rows, cols = np.nonzero(m)
        for k in range(int(m.sum())):
            assert tuple(R.kth_pixel_ref(m, k)) == (rows[k], cols[k])
    masks, split = C.parts_case()
    assert (masks & ~split).any() and (split & ~masks).any() and not split[2].any() and masks[2].any()
    labels, sizes = R.label_ref(split)
    parts, n_parts, bg = R.collect_parts_ref(labels, sizes, masks, split)
    assert n_parts == len(parts) == int((sizes > 0).sum()) and sum(s for _, _, s in parts) == split.sum()
    assert bg.tolist() == [(masks[n] & ~split[n]).sum() for n in range(4)] and bg[2] == masks[2].sum() and bg[3] == 0
    root = min(r for n, r, _ in parts if n == 1)
    desc = np.array([[1, 0, root], [1, 1, -1], [1, 2, -1], [1, 0, root]])
    out = R.part_masks_ref(masks, split, labels, desc)
    assert np.array_equal(out[0] | out[1], masks[1]) and not (out[0] & out[1]).any() and np.array_equal(out[2], masks[1])      # the comb is one component
