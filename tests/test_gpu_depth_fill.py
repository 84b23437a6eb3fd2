"""-m gpu: the depth fill (sp_depth_fill_nearest) against scipy's distance_transform_edt indices, bit for bit; the depth metrics
(sp_depth_metrics) against the float64-sum restatement and the real reference's values (golden g24); and the two drivers built
on them, DepthCompletion.depth_completion_dense and evaluate_completion.  Yardsticks and inputs: tests/depth_fill_ref.py."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import T, frames_from_synth, npy
import depth_fill_ref as ref

pytestmark = pytest.mark.gpu


def scipy_index_or_identity(invalid):
    return ref.scipy_index(invalid) if not invalid.all() else np.arange(invalid.size, dtype=np.int32).reshape(invalid.shape)


def check_fill(depth, invalid):
    """Both outputs against depth[scipy indices] at every pixel of a (B,H,W) stack; returns the device counts."""
    from super_primitive_amd.depth_completion import fill_in_tools
    filled, counts = fill_in_tools.fill_depth(T(depth), T(invalid), return_counts=True)
    index = fill_in_tools.nearest_valid_index(T(invalid))
    assert filled.dtype == torch.float32 and index.dtype == torch.int32 and filled.shape == index.shape == depth.shape
    filled, index = npy(filled), npy(index)
    for b in range(len(depth)):
        want = scipy_index_or_identity(invalid[b])
        assert np.array_equal(index[b], want), f"image {b}: {(index[b] != want).sum()} indices differ"
        assert np.array_equal(filled[b].view(np.uint32), depth[b].ravel()[want].view(np.uint32)), f"image {b}"
    return npy(counts)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_is_scipys_nearest_pixel_bit_for_bit(shape):
    """Each shape under all four mask patterns, as one batch of four."""
    H, W = shape
    cases = dict(ref.fill_cases())
    invalid = np.stack([cases[f"{p}_{H}x{W}"] for p in ref.PATTERNS])
    depth = np.stack([ref.unique_depth(H, W, 40 + k) for k in range(len(invalid))])
    counts = check_fill(depth, invalid)
    assert np.array_equal(counts[:, 0], (~invalid).sum((1, 2))) and np.array_equal(counts[:, 1], invalid.sum((1, 2)))


def test_fill_of_a_single_image_with_one_valid_pixel():
    from super_primitive_amd.depth_completion import fill_in_tools
    invalid = dict(ref.fill_cases())["one_valid_2x2"]
    depth = ref.unique_depth(2, 2, 3)
    filled = fill_in_tools.fill_depth(T(depth), T(invalid))                   # (H,W) in, (H,W) out
    assert filled.shape == (2, 2) and np.array_equal(npy(filled), np.full((2, 2), depth[1, 0]))
    assert np.array_equal(npy(fill_in_tools.nearest_valid_index(T(invalid))), np.full((2, 2), 2))
    # uint8 masks mean the same as bool ones
    assert np.array_equal(npy(fill_in_tools.fill_depth(T(depth), T(invalid.astype(np.uint8) * 255))), npy(filled))


def test_fill_at_480x640():
    """The working size once: the four patterns as one batch (the blob mask is about half invalid)."""
    invalid = np.stack([ref.invalid_mask(p, 480, 640, 5) for p in ref.PATTERNS])
    depth = np.stack([ref.unique_depth(480, 640, 50 + k) for k in range(len(invalid))])
    check_fill(depth, invalid)


def test_fill_batch_with_an_all_valid_and_an_all_invalid_image():
    H, W = 33, 65
    invalid = np.stack([ref.invalid_mask("holes", H, W, 9), np.zeros((H, W), dtype=bool), np.ones((H, W), dtype=bool)])
    depth = np.stack([ref.unique_depth(H, W, 60 + k) for k in range(3)])
    counts = check_fill(depth, invalid)                                       # the last two: copied through
    n0 = int((~invalid[0]).sum())
    assert counts.tolist() == [[n0, H * W - n0], [H * W, 0], [0, 0]]


# ---- metrics --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def metric_case():
    from super_primitive_amd.depth_completion import void
    estimate, target, valid = ref.metric_scene()
    got = npy(void.depth_metrics(T(estimate), T(target), T(valid)))
    return estimate, target, valid, got


def test_metrics_against_the_float64_sum_restatement():
    """Same float32 terms, float64 sums in another order: at most n 2^-53 = 3.4e-11 for n <= 3.1e5; the tolerance is 1e-9."""
    estimate, target, valid, got = metric_case()
    assert got.shape == (3, 12) and got.dtype == np.float64
    worst = 0.0
    for b in range(2):
        want = ref.metrics(estimate[b], target[b], valid[b])
        worst = max(worst, float(np.abs(got[b] / want - 1).max()))
        np.testing.assert_allclose(got[b], want, rtol=1e-9)
        assert got[b, 0] == valid[b].sum()
    print(f"\ndepth metrics vs float64-sum restatement: {worst:.3g} relative")


def test_metrics_against_the_references_values():
    """The reference averages in float32 (pairwise: about 2^-24 log2 n ~ 1e-6); the tolerance is 1e-5."""
    estimate, target, valid, got = metric_case()
    want = load_golden("g24_depth_fill")["metric_values"]
    worst = float(np.abs(got[:2] / want[:2] - 1).max())
    print(f"\ndepth metrics vs the reference's values: {worst:.3g} relative")
    np.testing.assert_allclose(got[:2], want[:2], rtol=1e-5)


def test_metrics_of_an_empty_mask_are_nan_and_two_runs_agree_bitwise():
    from super_primitive_amd.depth_completion import void
    estimate, target, valid, got = metric_case()
    assert not valid[2].any() and got[2, 0] == 0 and np.isnan(got[2, 1:]).all()
    assert np.isfinite(got[:2]).all()                                         # no inf target leaked into a sum
    again = npy(void.depth_metrics(T(estimate), T(target), T(valid)))
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    # an image's values do not depend on the batch it is scored in
    alone = npy(void.depth_metrics(T(estimate[1]), T(target[1]), T(valid[1])))
    assert np.array_equal(alone[0].view(np.uint64), got[1].view(np.uint64))


def test_metric_classes_keep_the_references_attributes_and_average_on_the_device():
    from super_primitive_amd.depth_completion import void
    estimate, target, valid, got = metric_case()
    avg, avg_d = void.ErrorMetricsAverager(), void.ErrorMetricsDeltasAverager()
    for b in range(2):
        m, d = void.ErrorMetrics(), void.ErrorMetricsDeltas()
        m.compute(T(estimate[b]), T(target[b]), T(valid[b]))
        d.compute(T(estimate[b]), T(target[b]), T(valid[b]))
        assert m._values.is_cuda and m._host is None                          # nothing read yet
        assert [m.rmse, m.mae, m.absrel, m.inv_rmse, m.inv_mae, m.inv_absrel] == got[b, 1:7].tolist()
        assert [d.delta105, d.delta110, d.delta1, d.delta2, d.delta3] == got[b, 7:].tolist() and d.delta0 == d.delta110
        avg.accumulate(m)
        avg_d.accumulate(d)
    assert avg.total_count == 2 and avg._values.is_cuda
    assert avg.rmse_avg == got[0, 1] + got[1, 1]                              # a running sum until average()
    avg.average()
    avg_d.average()
    assert avg.rmse_avg == (got[0, 1] + got[1, 1]) / 2 and avg.inv_absrel_avg == (got[0, 6] + got[1, 6]) / 2
    assert avg_d.delta1_avg == (got[0, 9] + got[1, 9]) / 2 and avg_d.mae_avg == avg.mae_avg


# ---- drivers --------------------------------------------------------------------------------------------------------
class Front:
    """The stand-in frontend of tests/test_gpu_drivers.py: a synthetic keyframe per image -- here with holes in its masks, so that
    the completion leaves pixels to fill."""
    config = {"sam_params": {"nms": True, "select_smallest": True}}

    def __init__(self):
        self.frames = {}

    def add(self, pair, seed):
        rng = np.random.default_rng(seed)
        hole = rng.uniform(size=pair.depth.shape) < 0.03
        hole[[0, -1], :] = True
        hole[:, [0, -1]] = True
        hole[10:16, 30:50] = True
        kp = np.asarray(pair.meta["kp_rc"]).astype(int)
        hole[kp[:, 0], kp[:, 1]] = False
        pair.keypoint_regions = pair.keypoint_regions & ~hole
        src, _ = frames_from_synth(pair)
        self.frames[id(src.image)] = src
        return src

    def process_to_kf(self, image, K, keypoints=None):
        return self.frames[id(image)]


def synth_sample(front, seed):
    from super_primitive_amd import synth
    pair = synth.make_pair(60, 80, 12, seed=seed, overlap=2)
    src = front.add(pair, seed)
    rng = np.random.default_rng(seed)
    sparse = np.where(rng.uniform(size=pair.depth.shape) < 0.05, pair.depth, 0.0).astype(np.float32)
    return src, pair, sparse


def test_depth_completion_dense_fills_what_the_completion_leaves():
    from super_primitive_amd.depth_completion.segment_based_completion import DepthCompletion
    front = Front()
    src, pair, sparse = synth_sample(front, 81)
    dc = DepthCompletion(front_processor=front, config={})
    filled, depth, invalid = dc.depth_completion_dense(src.image, src.K, torch.from_numpy(sparse))
    assert filled.is_cuda and depth.is_cuda and invalid.is_cuda and filled.shape == depth.shape == invalid.shape == (60, 80)
    want_depth, want_invalid = dc.depth_completion(src.image, src.K, torch.from_numpy(sparse))
    filled, depth, invalid = npy(filled), npy(depth), npy(invalid)
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)) and np.array_equal(invalid, want_invalid)
    assert 0.05 < invalid.mean() < 0.15                                       # holes to fill (3 % + border + a block = 11 %), no rerun
    assert np.array_equal(filled[~invalid].view(np.uint32), depth[~invalid].view(np.uint32))
    assert not (filled < 1e-6).any()
    assert np.array_equal(filled.view(np.uint32), ref.scipy_fill(depth, invalid).view(np.uint32))
    np.testing.assert_allclose(filled, pair.depth, rtol=5e-2)                 # a neighbour's depth on a smooth plane


def test_evaluate_completion_is_the_restated_loop():
    """evaluate_void.py:87-160 over three samples: both scoreboards at the metric tolerance against the float64-sum restatement
    (1e-9, see above) and the validity rates."""
    from super_primitive_amd.depth_completion.evaluate import evaluate_completion
    from super_primitive_amd.depth_completion.segment_based_completion import DepthCompletion
    front = Front()
    dc = DepthCompletion(front_processor=front, config={})
    min_depth, max_depth = 0.2, 3.4                                           # the scenes reach 3.6 - 3.9: the mask cuts pixels away
    samples, want_filled, want_partial, want_rates = [], [], [], []
    for seed in (81, 82, 83):
        src, pair, sparse = synth_sample(front, seed)
        target = pair.depth.astype(np.float32).copy()
        samples.append((src.image, src.K, torch.from_numpy(sparse), target))
        depth, invalid = dc.depth_completion(src.image, src.K, torch.from_numpy(sparse))
        mask = (target < max_depth) & (target > min_depth)
        assert 0 < mask.sum() < mask.size
        target = np.where(mask, target, np.float32(np.inf))
        want_filled.append(ref.metrics(ref.scipy_fill(depth, invalid), target, mask))
        want_partial.append(ref.metrics(depth, target, mask & (depth > 1e-6)))
        want_rates.append((depth > 1e-6).sum() / depth.size)
    scores = evaluate_completion(dc, samples, min_depth, max_depth)
    assert scores.filled.total_count == scores.partial.total_count == 3
    names = ("rmse", "mae", "absrel", "inv_rmse", "inv_mae", "inv_absrel", "delta105", "delta110", "delta1", "delta2", "delta3")
    for board, want in ((scores.filled, want_filled), (scores.partial, want_partial)):
        want = np.mean(want, axis=0)[1:]
        got = np.array([getattr(board, n + "_avg") for n in names])
        np.testing.assert_allclose(got, want, rtol=1e-9)
    np.testing.assert_allclose(scores.validity_rates, want_rates, rtol=1e-12)
    assert scores.filled.rmse_avg != scores.partial.rmse_avg
