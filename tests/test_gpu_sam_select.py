"""-m gpu: SAM mask selection on the device (sp_sam.hip behind frontend/segment/mask_generation.py) against the torch restatement
of tests/sam_select_ref.py on the same device and against what the real reference returned (golden g25).  Every comparison on
integers or bools is exact; the edge maps are bitwise, except behind the bilinear upsample (atol 1e-6)."""

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import T, dev, npy
import sam_select_ref as ref

pytestmark = pytest.mark.gpu


def mg():
    from super_primitive_amd.frontend.segment import mask_generation
    return mask_generation


def quantised_logits(M, H, W, seed):
    """Multiples of 1/8 in [-2, 2]: exactly -1, 0 and +1 occur wherever there are enough pixels."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-16, 17, (M, H, W), generator=g).float() / 8).to(dev())


def check_stats(logits):
    stats = mg().candidate_stats(logits)
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (logits.shape[0], 8)
    for col, t in ((0, 1.0), (1, -1.0), (2, 0.0)):
        assert torch.equal(stats[:, col], ref.threshold_count(logits, t)), f"count of x > {t}"
    assert torch.equal(stats[:, 3:7].long(), ref.batched_mask_to_box(logits > 0))
    assert not bool(stats[:, 7].any())
    return stats


@pytest.mark.parametrize("H,W,M", [(1, 1, 1), (5, 7, 3), (3, 130, 7), (37, 53, 48), (48, 64, 5), (96, 128, 156)])
def test_candidate_stats_against_torch_counts(H, W, M):
    x = quantised_logits(M, H, W, H * W + M)
    check_stats(x)
    # the same values in storage that starts 4 bytes off a 16-byte boundary
    shifted = torch.empty(M * H * W + 1, device=dev())[1:].view(M, H, W)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    shifted.copy_(x)
    assert torch.equal(check_stats(shifted), mg().candidate_stats(x))
    # special maps: all true, all false, one pixel wide, NaN and the infinities
    y = x[:min(M, 6)].clone()
    y[0] = 3
    if len(y) > 1:
        y[1] = -3
    if len(y) > 2:
        y[2] = -3
        y[2, :, W // 2] = 2
    if len(y) > 3:
        y[3].view(-1)[::3] = float("nan")
        y[3].view(-1)[1::5] = float("inf")
        y[3].view(-1)[2::7] = float("-inf")
    stats = check_stats(y)
    assert stats[0, :3].tolist() == [H * W] * 3 and stats[0, 3:7].tolist() == [0, 0, W - 1, H - 1]
    if len(y) > 1:
        assert stats[1].tolist() == [0] * 8
    if len(y) > 2:
        assert stats[2, 2:7].tolist() == [H, W // 2, 0, W // 2, H - 1]


def same_fields(got, want, context=""):
    assert list(got) == list(want), (context, list(got), list(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (context, k, got[k].dtype, got[k].shape, want[k].shape)
        assert torch.equal(got[k], want[k]), (context, k)


@pytest.fixture(scope="module")
def synthetic_round():
    (H, W), n1, _, _ = ref.SHAPES[0]
    return ref.SyntheticSam(H, W, 7)(None, ref.golden_keypoints(n1).to(dev()))


@pytest.mark.parametrize("select_smallest", [True, False])
@pytest.mark.parametrize("iou_thr,stab_thr", [(0.88, 0.95), (0.0, 0.95), (0.88, 0.0), (0.0, 0.0), (1.0, 0.95)])
def test_smallest_good_mask_batch_against_the_restatement(synthetic_round, select_smallest, iou_thr, stab_thr):
    logits, iou = synthetic_round["masks"], synthetic_round["iou_pred"]
    got = mg().smallest_good_mask_batch(logits, iou, iou_thr, stab_thr, select_smallest)
    want = ref.smallest_good_mask_batch(logits, iou, iou_thr, stab_thr, select_smallest)
    same_fields(got, want, (select_smallest, iou_thr, stab_thr))
    H, W = logits.shape[-2:]
    if iou_thr > 0.99:                                                       # everything rejected
        assert tuple(got["masks"].shape) == (0, H, W) and tuple(got["boxes"].shape) == (0, 4) and got["boxes"].dtype == torch.int64
    else:
        assert 0 < got["masks"].shape[0]
    if select_smallest and iou_thr == 0.88 and stab_thr == 0.95:             # the planted keypoint: no good mask, so mask 0
        at = got["keypoints_ids"].tolist().index(1)
        assert int(got["masks_ids"][at]) == 0
        assert got["masks"].shape[0] < logits.shape[0]


def test_an_empty_mask_wins_with_stability_off():
    logits = quantised_logits(6, 12, 20, 9).view(2, 3, 12, 20).clone()
    logits[1, 1] = -0.5                                                      # empty: size 0 is the smallest, its box is zeros
    iou = torch.full((2, 3), 0.9, device=dev())
    got = mg().smallest_good_mask_batch(logits, iou, 0.88, 0.0, True)
    same_fields(got, ref.smallest_good_mask_batch(logits, iou, 0.88, 0.0, True))
    assert got["masks_ids"].tolist()[1] == 1 and got["boxes"][1].tolist() == [0, 0, 0, 0] and not bool(got["masks"][1].any())


def nms_case(K, seed):
    rng = np.random.default_rng(seed)
    x1, y1 = rng.integers(0, 120, K), rng.integers(0, 90, K)
    boxes = np.stack([x1, y1, x1 + rng.integers(0, 40, K), y1 + rng.integers(0, 40, K)], axis=1)
    if K > 8:
        boxes[3] = boxes[1]                                                  # identical boxes
        boxes[5, 2] = boxes[5, 0]                                            # zero area: score +inf, IoU with itself 0 / 0
        boxes[6] = 0                                                         # an empty mask's box
        boxes[7] = boxes[5]
    return torch.from_numpy(boxes).to(dev())


@pytest.mark.parametrize("K", [0, 1, 2, 700, 2048])
def test_box_nms_against_the_restatement(K):
    boxes = nms_case(K, K + 1)
    by_area = 1 / ref.box_area(boxes)                                        # many ties, +inf
    coarse = torch.round(torch.rand(K, generator=torch.Generator().manual_seed(K)) * 20).to(dev()) / 20       # tied scores
    for scores in (by_area, coarse):
        for thr in (0.3, 0.7, 0.8):
            got = mg().box_nms(boxes.float(), scores, thr)
            want = ref.nms(boxes.float(), scores, thr)
            assert got.dtype == torch.int64 and got.tolist() == want.tolist(), (K, thr)      # the order, not only the set
    if K == 2:                                                               # a threshold of exactly an attained IoU does not suppress
        two, s = torch.tensor([[0, 0, 4, 4], [0, 0, 4, 2]], dtype=torch.float32, device=dev()), torch.tensor([2.0, 1.0], device=dev())
        assert mg().box_nms(two, s, 0.5).tolist() == [0, 1] and mg().box_nms(two, s, 0.49).tolist() == [0]
        assert mg().box_nms(two, s.flip(0), 0.49).tolist() == [1]
    if K == 700:
        assert 1 < len(got) < K


def test_box_nms_refuses_more_than_2048_boxes():
    boxes = nms_case(2049, 1).float()
    with pytest.raises(RuntimeError, match="SP_ELIMIT"):
        mg().box_nms(boxes, torch.ones(2049, device=dev()), 0.5)


def blob_masks(K, H, W, seed):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[:H, :W]
    masks = np.stack([((r - rng.uniform(0, H)) / rng.uniform(2, H / 2)) ** 2 + ((c - rng.uniform(0, W)) / rng.uniform(2, W / 2)) ** 2 <= 1
                      for _ in range(K)])
    masks[0, 0, :] = True                                                    # something on the border rows / columns
    masks[-1, :, -1] = True
    return T(masks)


def bitwise_equal(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("K", [1, 52])
@pytest.mark.parametrize("size,coarse", [((96, 128), None), ((96, 128), (48, 64)), ((96, 128), (36, 50)), ((37, 53), (20, 31)), ((37, 53), None)])
def test_edges_bitwise_against_the_restatement(size, coarse, K, pool):
    masks = blob_masks(K, size[0], size[1], K + size[0])
    if coarse is None:
        got = mg().infer_edge_probs(masks, pool_edges=pool)
        want = ref.infer_edge_probs(masks, pool_edges=pool)
        if not pool:
            assert bitwise_equal(mg().masks_to_edges(masks), want[0])
    else:
        got = mg()._edge_maps(masks, coarse, pool)
        want = ref.infer_edge_probs(ref.nearest_resize(masks, coarse), pool_edges=pool)
    assert bitwise_equal(got[0], want[0]), f"edges: {int((got[0] != want[0]).sum())} pixels differ"
    assert bitwise_equal(got[1], want[1]), f"edge_probs: {int((got[1] != want[1]).sum())} pixels differ"
    assert float(want[0].max()) > 0.3 and float(want[1].min()) == 0.0          # not a flat map


@pytest.fixture(scope="module")
def g25():
    return load_golden("g25_sam_select")


@pytest.mark.parametrize("shape_index,name", [(i, name) for i in range(len(ref.SHAPES)) for name in ref.CONFIGS])
def test_infer_masks_reproduces_the_references_results(g25, shape_index, name):
    (H, W), n1, n2, coarse = ref.SHAPES[shape_index]
    sam, keypoints, sampler, want = ref.golden_case(g25, shape_index, name, device=dev())
    shape = ref.edge_shape_of(name, coarse)
    res = mg().infer_masks(sam, torch.zeros(H, W, 3, device=dev()), ref.CONFIGS[name], keypoints=keypoints, num_pts=n1, num_pts_active=n2,
                           edge_probs_shape=shape, sampler=sampler)
    assert sam.at == 2 and list(res) == ["masks", "keypoints", "num_active", "coarse_coverage", "final_coverage", "sampled_masks", "edges",
                                         "edge_probs", "edge_coarse", "edge_probs_coarse"]
    assert isinstance(res["masks"], dict) and res["masks"]["masks"].dtype == torch.bool
    ref.assert_same_result(ref.result_arrays(res), want, through_upsample=shape is not None, context=f"{H}x{W} {name}")


def same_results(got, want, context=""):
    """Two infer_masks results on the same device: everything exact."""
    same_fields(got["masks"], want["masks"], context)
    assert got["num_active"] == want["num_active"], context
    for k in ref.RESULT_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (context, k)
        assert torch.equal(got[k], want[k]), (context, k, int((got[k] != want[k]).sum()))
    for k in ref.SAMPLER_ARRAYS:
        assert torch.equal(got["sampled_masks"][k], want["sampled_masks"][k]), (context, k)


@pytest.mark.parametrize("name", list(ref.CONFIGS))
def test_infer_masks_free_running_against_the_restatement(name):
    """Own keypoints and own draws from the same seed on the same device."""
    (H, W), n1, n2, coarse = ref.SHAPES[0]
    image, shape = torch.zeros(H, W, 3, device=dev()), ref.edge_shape_of(name, coarse)
    torch.manual_seed(5)
    got = mg().infer_masks(ref.SyntheticSam(H, W, 3, 0.3), image, ref.CONFIGS[name], num_pts=n1, num_pts_active=n2, edge_probs_shape=shape)
    torch.manual_seed(5)
    keypoints = torch.rand(n1, 2, device=dev()) * 2 - 1
    want = ref.infer_masks(ref.SyntheticSam(H, W, 3, 0.3), image, ref.CONFIGS[name], keypoints, n2, edge_probs_shape=shape)
    same_results(got, want, name)
    assert not bool(got["coarse_coverage"].all())
    assert 0 < got["masks"]["masks"].shape[0] < 3 * (n1 + n2)


def test_infer_masks_at_working_width():
    """480 x 640 with 64 + 16 keypoints (236 MB of logits), configuration A."""
    H, W, n1, n2 = 480, 640, 64, 16
    image = torch.zeros(H, W, 3, device=dev())
    keypoints = ref.golden_keypoints(n1, seed=2).to(dev())
    torch.manual_seed(8)
    sam = ref.SyntheticSam(H, W, 4)
    got = mg().infer_masks(sam, image, ref.CONFIG_A, keypoints=keypoints, num_pts_active=n2, edge_probs_shape=(240, 320))
    torch.manual_seed(8)
    want = ref.infer_masks(ref.ReplaySam(sam.calls), image, ref.CONFIG_A, keypoints, n2, edge_probs_shape=(240, 320))       # drawn once
    same_results(got, want, "480x640 A")
    assert got["masks"]["masks"].shape[0] > 20


def test_no_survivor_gives_empty_tensors_of_the_right_shape():
    (H, W), n1, n2, coarse = ref.SHAPES[1]
    cfg = dict(ref.CONFIG_B, iou_threshold=1.0)
    res = mg().infer_masks(ref.SyntheticSam(H, W, 3), torch.zeros(H, W, 3, device=dev()), cfg, keypoints=ref.golden_keypoints(n1).to(dev()),
                           num_pts_active=n2, edge_probs_shape=coarse)
    m = res["masks"]
    assert tuple(m["masks"].shape) == (0, H, W) and tuple(m["boxes"].shape) == (0, 4) and tuple(res["keypoints"].shape) == (0, 2)
    assert m["keypoints_ids"].numel() == m["masks_ids"].numel() == m["iou_preds"].numel() == 0 and res["num_active"] == 0
    assert not bool(res["coarse_coverage"].any()) and not bool(res["final_coverage"].any())
    assert tuple(res["edges"].shape) == (H, W) and tuple(res["edge_coarse"].shape) == coarse and not bool(res["edges"].any())


def test_keyframe_from_sam_is_keyframe_from_normals_on_the_restatements_masks():
    from super_primitive_amd import synth
    from super_primitive_amd.frontend.keyframe_assembly import keyframe_from_normals, keyframe_from_sam
    H, W, shape, n1, n2 = 96, 128, (48, 64), 40, 12
    pair = synth.make_pair(H, W, 6, seed=3)
    half = synth.make_pair(shape[0], shape[1], 6, seed=3)
    image, K, normals = T(pair.src_image), T(pair.K), T(synth.plane_normals(half))
    keypoints = ref.golden_keypoints(n1).to(dev())
    torch.manual_seed(21)
    kf = keyframe_from_sam(image, K, normals, ref.SyntheticSam(H, W, 7), ref.CONFIG_A, num_pts=n1, num_pts_active=n2, integration_shape=shape,
                           keypoints=keypoints, cg_max_iter=200, cg_tol=1e-3)
    torch.manual_seed(21)
    want = ref.infer_masks(ref.SyntheticSam(H, W, 7), image.permute(1, 2, 0), ref.CONFIG_A, keypoints, n2, edge_probs_shape=shape)
    masks = ref.nearest_resize(want["masks"]["masks"], shape)
    kf_want = keyframe_from_normals(image, K, normals, masks, want["keypoints"], cg_max_iter=200, cg_tol=1e-3)
    assert kf.num_segments() == kf_want.num_segments() > 10
    for name in ("image", "K", "K_img", "logdepth_perseg", "keypoints", "keypoint_regions", "segment_boxes"):
        a, b = getattr(kf, name), getattr(kf_want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    # with the image brought to another size for the network, the masks come back to the image's size
    torch.manual_seed(21)
    big = keyframe_from_sam(image, K, normals, ref.SyntheticSam(2 * H, 2 * W, 7), ref.CONFIG_A, num_pts=n1, num_pts_active=n2,
                            integration_shape=shape, infer_resolution=(2 * H, 2 * W), keypoints=keypoints, cg_max_iter=200, cg_tol=1e-3)
    assert tuple(big.keypoint_regions.shape[-2:]) == (H, W) and big.num_segments() > 10
