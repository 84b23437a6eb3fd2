"""SAM mask selection without a GPU: the torch restatement (tests/sam_select_ref.py) against what the real reference returned (golden
g25) and its helpers against brute force, and the host side of the new entry points (header / ctypes table / library, refusals,
host inputs refused, the reference's module path)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import sam_select_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sp_sam_candidate_stats", "sp_box_nms", "sp_sam_build_masks", "sp_mask_edges", "sp_sam_cut_masks")
CASES = [(i, name) for i in range(len(ref.SHAPES)) for name in ref.CONFIGS]


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_sam_select")


@pytest.mark.parametrize("shape_index,name", CASES)
def test_restatement_reproduces_the_references_infer_masks(g25, shape_index, name):
    (H, W), n1, n2, coarse = ref.SHAPES[shape_index]
    sam, keypoints, sampler, want = ref.golden_case(g25, shape_index, name)
    shape = ref.edge_shape_of(name, coarse)
    res = ref.infer_masks(sam, np.zeros((H, W, 3), np.float32), ref.CONFIGS[name], keypoints, n2, edge_probs_shape=shape, sampler=sampler)
    assert sam.at == 2
    ref.assert_same_result(ref.result_arrays(res), want, through_upsample=shape is not None, context=f"{H}x{W} {name}")
    assert want["masks"].shape[0] > 0 and want["masks"].shape[0] < 3 * (n1 + n2)


def test_golden_inputs_are_the_synthetic_sams_and_cover_the_quirks(g25):
    for i, ((H, W), n1, n2, coarse) in enumerate(ref.SHAPES):
        keypoints = ref.golden_keypoints(n1)
        assert np.array_equal(keypoints.numpy(), g25[f"s{i}_keypoints"])
        out = ref.SyntheticSam(H, W, 7)(None, keypoints)
        q = g25[f"s{i}_logits1"]
        assert np.array_equal((out["masks"] * 8).numpy(), q.astype(np.float32))
        assert all((q == v).any() for v in (-8, 0, 8))                        # logits of exactly -1, 0 and +1
        iou = g25[f"s{i}_iou1"]
        assert iou.min() >= 0.82 and iou.max() < 1
        # the planted keypoint 1 survives B's thresholds without a good mask and is given mask 0
        b = ref.smallest_good_mask_batch(out["masks"], out["iou_pred"], 0.88, 0.95, True)
        good = (out["iou_pred"] > 0.88) & (ref.calculate_stability_score(out["masks"], 0.0, 1.0) >= 0.95)
        at = b["keypoints_ids"].tolist().index(1)
        assert not good[1].any() and int(b["masks_ids"][at]) == 0
    assert g25["s0A_masks_ids"].shape[0] > g25["s0B_masks_ids"].shape[0] > g25["s0C_keypoints_ids"].shape[0] > 0


def test_restated_sampler_draws_what_the_reference_drew(g25):
    """Same generator state on the same device: Categorical.sample, then randint_like."""
    for i, name in CASES:
        (H, W), n1, n2, coarse = ref.SHAPES[i]
        c = f"s{i}{name}_"
        coverage = torch.from_numpy(np.unpackbits(g25[c + "coarse_coverage"], axis=-1, count=W).astype(bool))
        torch.manual_seed(100 + i)
        got = ref.active_sample_pos(coverage[None], n2)
        for k in ref.SAMPLER_ARRAYS:
            assert np.array_equal(got[k].numpy(), g25[c + "sampler_" + k]), (i, name, k)


def test_coarse_density_against_float64():
    """A sum of at most 48 cells at these shapes: the bound is 48 * 2^-24 ~ 3e-6; rtol 1e-5."""
    rng = np.random.default_rng(3)
    for H, W in ((96, 128), (37, 53), (64, 80)):
        coverage = rng.random((2, H, W)) < 0.6
        got = ref.coarse_density(torch.from_numpy(coverage)).numpy()
        c = coverage.astype(np.float64)
        c[:, -2:, :] = 1
        Hc, Wc = H // 16, W // 16
        cells = 1.0 - c[:, :Hc * 16, :Wc * 16].reshape(2, Hc, 16, Wc, 16).mean(axis=(2, 4))
        want = cells / (cells.sum(axis=(1, 2), keepdims=True) + 1e-6)
        assert got.shape == (2, 1, Hc, Wc)
        np.testing.assert_allclose(got[:, 0], want, rtol=1e-5)


def test_counts_and_boxes_against_brute_force():
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (5, 7), (3, 130), (37, 53)):
        x = (rng.integers(-16, 17, size=(6, H, W)) / 8).astype(np.float32)
        x[0, 0, 0] = np.nan
        x[1, -1, -1] = np.inf
        x[2] = -3                                                              # empty
        x[3] = 3                                                               # full
        if H > 1:
            x[4] = -3
            x[4, :, W // 2] = 2                                                # one pixel wide
        t = torch.from_numpy(x)
        for thr in (-1.0, 0.0, 1.0):
            assert np.array_equal(ref.threshold_count(t, thr).numpy(), np.count_nonzero(x > thr, axis=(1, 2)))
        score = ref.calculate_stability_score(t, 0.0, 1.0).numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.count_nonzero(x > 1, axis=(1, 2)).astype(np.float32) / np.count_nonzero(x > -1, axis=(1, 2)).astype(np.float32)
        assert np.array_equal(score, want, equal_nan=True)
        assert np.isnan(score[2]) and not (score[2] >= 0.5)                    # 0 / 0 fails >=
        boxes = ref.batched_mask_to_box(t > 0).numpy()
        assert boxes.dtype == np.int64
        for k in range(len(x)):
            rows, cols = np.where(x[k] > 0)
            want = [cols.min(), rows.min(), cols.max(), rows.max()] if len(rows) else [0, 0, 0, 0]
            assert boxes[k].tolist() == want, (H, W, k)
        if H > 1:
            assert int(ref.box_area(torch.from_numpy(boxes))[4]) == 0              # no +1: a one-pixel-wide mask has area 0
            assert float(1 / ref.box_area(torch.from_numpy(boxes))[4]) == float("inf")
    assert ref.batched_mask_to_box(torch.zeros(0, 4, 5, dtype=torch.bool)).shape == (0, 4)


def greedy_nms(boxes, scores, thr):
    """O(K^2) scalar greedy in float32."""
    f = np.float32
    order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))
    area = [f(f(b[2] - b[0]) * f(b[3] - b[1])) for b in boxes]
    keep, dead = [], set()
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, i in enumerate(order):
            if i in dead:
                continue
            keep.append(i)
            for j in order[a + 1:]:
                w = max(f(min(boxes[i][2], boxes[j][2]) - max(boxes[i][0], boxes[j][0])), f(0))
                h = max(f(min(boxes[i][3], boxes[j][3]) - max(boxes[i][1], boxes[j][1])), f(0))
                inter = f(w * h)
                if f(inter / f(f(area[i] + area[j]) - inter)) > f(thr):
                    dead.add(j)
    return keep


def nms_boxes(rng, K):
    """Integer boxes with the corner cases in: identical boxes, zero-area boxes, an empty (all-zero) box, tied scores."""
    x1, y1 = rng.integers(0, 40, K), rng.integers(0, 30, K)
    boxes = np.stack([x1, y1, x1 + rng.integers(0, 25, K), y1 + rng.integers(0, 25, K)], axis=1)
    if K > 8:
        boxes[3] = boxes[1]
        boxes[5, 2] = boxes[5, 0]
        boxes[6] = 0
        boxes[7] = boxes[5]
    return boxes


@pytest.mark.parametrize("K", [0, 1, 2, 9, 60])
def test_nms_against_a_scalar_greedy(K):
    rng = np.random.default_rng(K)
    boxes = nms_boxes(rng, K)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    with np.errstate(divide="ignore"):
        by_area = (1 / area.astype(np.float32)).astype(np.float32)              # ties and +inf
    for scores in (by_area, np.round(rng.random(K), 1).astype(np.float32)):
        for thr in (0.3, 0.7):
            got = ref.batched_nms(torch.from_numpy(boxes).float(), torch.from_numpy(scores), torch.zeros(K, dtype=torch.int64), thr)
            assert got.dtype == torch.int64 and got.tolist() == greedy_nms(boxes.astype(np.float32), scores, thr)
    if K == 2:                                                                  # a threshold of exactly an attained IoU does not suppress
        two = torch.tensor([[0, 0, 4, 4], [0, 0, 4, 2]], dtype=torch.float32)
        s = torch.tensor([2.0, 1.0])
        assert ref.nms(two, s, 0.5).tolist() == [0, 1] and ref.nms(two, s, 0.49).tolist() == [0]


def test_edge_map_is_exact_against_float64():
    rng = np.random.default_rng(2)
    m = rng.random((7, 37, 53)) < 0.5
    p = np.pad(m.astype(np.float64), ((0, 0), (1, 1), (1, 1)), mode="reflect")
    a, d = np.array([3, 10, 3]) / 32, np.array([-1, 0, 1])
    gx = sum(np.outer(a, d)[i, j] * p[:, i:i + 37, j:j + 53] for i in range(3) for j in range(3))
    gy = sum(np.outer(d, a)[i, j] * p[:, i:i + 37, j:j + 53] for i in range(3) for j in range(3))
    want = np.sqrt(gx * gx + gy * gy).max(axis=0).astype(np.float32)
    edges, probs = ref.infer_edge_probs(torch.from_numpy(m))
    assert np.array_equal(edges.numpy(), want)
    assert np.array_equal(probs.numpy(), np.clip(1 - 2 * want, 0, 1))


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for cite in ("mask_generation.py:54-56", "mask_generation.py:183-188", "mask_generation.py:67,76", "mask_generation.py:291-313",
                 "mask_generation.py:254-275"):
        assert cite in header, cite
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name


def test_argument_checks():
    """Everything the entry points refuse is refused before any device work, so this runs without a GPU."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    a, b, c, d, e = (ctypes.c_void_p(256 * k) for k in range(1, 6))             # non-null addresses: never dereferenced
    stats = lib.sp_sam_candidate_stats
    assert stats(None, 3, 8, 8, 0.0, 1.0, b, None) == -1
    assert stats(a, 3, 8, 8, 0.0, 1.0, None, None) == -1
    assert stats(a, 3, 8, 8, 0.0, 1.0, a, None) == -1
    assert stats(a, 0, 8, 8, 0.0, 1.0, b, None) == stats(a, 3, 0, 8, 0.0, 1.0, b, None) == stats(a, 3, 8, -1, 0.0, 1.0, b, None) == -1
    assert stats(a, 3, 8, 32768, 0.0, 1.0, b, None) == -2                       # W <= 32767
    assert stats(a, 3, 70000, 32767, 0.0, 1.0, b, None) == -2                   # H W < 2^31
    assert stats(a, 65536, 8, 8, 0.0, 1.0, b, None) == -2
    nms = lib.sp_box_nms
    assert nms(None, b, 4, 0.5, c, d, None) == nms(a, None, 4, 0.5, c, d, None) == -1
    assert nms(a, b, 4, 0.5, None, d, None) == nms(a, b, 4, 0.5, c, None, None) == -1
    assert nms(a, b, 4, 0.5, a, d, None) == nms(a, b, 4, 0.5, b, d, None) == nms(a, b, 4, 0.5, c, c, None) == -1
    assert nms(a, b, 0, 0.5, c, d, None) == -1
    assert nms(a, b, 2049, 0.5, c, d, None) == -2
    build = lib.sp_sam_build_masks
    assert build(None, b, 2, 6, 8, 8, 0.0, c, d, None) == build(a, None, 2, 6, 8, 8, 0.0, c, d, None) == -1
    assert build(a, b, 2, 6, 8, 8, 0.0, None, d, None) == -1
    assert build(a, b, 2, 6, 8, 8, 0.0, a, d, None) == build(a, b, 2, 6, 8, 8, 0.0, c, c, None) == -1
    assert build(a, b, 0, 6, 8, 8, 0.0, c, d, None) == build(a, b, 2, 0, 8, 8, 0.0, c, d, None) == build(a, b, 2, 6, 8, 0, 0.0, c, d, None) == -1
    assert build(a, b, 2, 6, 8, 40000, 0.0, c, d, None) == -2
    edges = lib.sp_mask_edges
    assert edges(None, 2, 8, 8, None, None, 8, 8, b, c, 0, None) == -1
    assert edges(a, 2, 8, 8, None, None, 8, 8, None, c, 0, None) == edges(a, 2, 8, 8, None, None, 8, 8, b, None, 0, None) == -1
    assert edges(a, 2, 8, 8, None, None, 8, 8, b, b, 0, None) == -1
    assert edges(a, 0, 8, 8, None, None, 8, 8, b, c, 0, None) == edges(a, 2, 8, 8, d, e, 0, 4, b, c, 0, None) == -1
    assert edges(a, 2, 8, 8, None, None, 4, 4, b, c, 0, None) == -1             # another size needs its index tables
    assert edges(a, 2, 8, 8, d, e, 1, 4, b, c, 0, None) == edges(a, 2, 8, 8, d, e, 4, 40000, b, c, 0, None) == -2
    assert edges(a, 2, 8, 40000, d, e, 4, 4, b, c, 0, None) == -2
    cut = lib.sp_sam_cut_masks
    assert cut(None, 2, 8, 8, None, 0.5, None, b, c, d, None) == cut(a, 2, 8, 8, None, 0.5, None, None, c, d, None) == -1
    assert cut(a, 2, 8, 8, None, 0.5, None, b, c, None, None) == -1
    assert cut(a, 2, 8, 8, None, 0.5, None, b, a, d, None) == cut(a, 2, 8, 8, None, 0.5, None, b, c, a, None) == -1
    assert cut(a, 2, 8, 8, None, 0.5, None, b, c, c, None) == -1
    assert cut(a, 0, 8, 8, None, 0.5, None, b, c, d, None) == cut(a, 2, -8, 8, None, 0.5, None, b, c, d, None) == -1
    assert cut(a, 2, 8, 40000, None, 0.5, None, b, c, d, None) == -2


def test_host_inputs_are_refused():
    from super_primitive_amd.frontend import keyframe_assembly
    from super_primitive_amd.frontend.segment import mask_generation as mg
    logits, iou, masks = torch.zeros(2, 3, 8, 8), torch.ones(2, 3), torch.zeros(2, 8, 8, dtype=torch.bool)
    keypoints = torch.zeros(2, 2)
    calls = [lambda: mg.smallest_good_mask_batch(logits, iou), lambda: mg.smallest_good_mask_batch(logits.numpy(), iou.numpy()),
             lambda: mg.candidate_stats(logits[0]), lambda: mg.box_nms(torch.zeros(2, 4), torch.zeros(2), 0.5),
             lambda: mg.active_sample_pos(masks[:1]), lambda: mg.masks_to_edges(masks), lambda: mg.infer_edge_probs(masks),
             lambda: mg.infer_masks(lambda image, kp: {"masks": logits, "iou_pred": iou}, np.zeros((8, 8, 3), np.float32), ref.CONFIG_A,
                                    keypoints=keypoints),
             lambda: keyframe_assembly.keyframe_from_sam(torch.zeros(3, 8, 8), torch.eye(3), torch.zeros(8, 8, 3), None, ref.CONFIG_A, num_pts=2,
                                                         num_pts_active=0, integration_shape=(8, 8))]
    for call in calls:
        with pytest.raises(RuntimeError, match="HIP-only"):
            call()


def test_reference_module_path_resolves_to_the_device_module():
    import super_primitive_amd
    from super_primitive_amd.frontend.segment import mask_generation as ours
    assert "frontend.segment.mask_generation" in super_primitive_amd._REFERENCE_LEAF_MODULES
    saved = dict(sys.modules)
    try:
        super_primitive_amd.install_as_reference_modules()
        import frontend.segment.mask_generation as theirs
        assert theirs is ours
        for name in ("smallest_good_mask_batch", "active_sample_pos", "infer_masks", "masks_to_edges", "infer_edge_probs"):
            assert hasattr(theirs, name), name
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
