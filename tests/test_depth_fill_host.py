"""Depth fill and depth metrics without a GPU: the numpy restatement of the fill rule (tests/depth_fill_ref.py) against scipy and
against what the real reference returned (golden g24), and the host side of the new entry points (header / ctypes table /
library, refusals and size queries, host inputs refused, the reference's module paths)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
import depth_fill_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sp_depth_fill_workspace_bytes", "sp_depth_fill_nearest", "sp_depth_metrics_workspace_doubles", "sp_depth_metrics")


def test_restated_rule_is_scipys_choice_on_every_small_case():
    ties = pixels = 0
    for name, invalid in ref.fill_cases():
        got, want = ref.nearest_valid_index(invalid), ref.scipy_index(invalid)
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} pixels differ"
        assert not invalid.ravel()[got.ravel()].any(), name                   # every source is a valid pixel
        assert np.array_equal(got[~invalid], np.arange(invalid.size).reshape(invalid.shape)[~invalid]), name
        pixels += invalid.size
    print(f"{pixels} pixels over {len(ref.fill_cases())} masks: 0 differences to scipy")


@pytest.mark.parametrize("pattern", ref.PATTERNS)
def test_restated_rule_is_scipys_choice_at_480x640(pattern):
    invalid = ref.invalid_mask(pattern, 480, 640, 5)
    assert np.array_equal(ref.nearest_valid_index(invalid), ref.scipy_index(invalid))


def test_restated_rule_copies_an_image_without_a_valid_pixel_through():
    assert np.array_equal(ref.nearest_valid_index(np.ones((5, 9), dtype=bool)), np.arange(45).reshape(5, 9))
    assert np.array_equal(ref.nearest_valid_index(np.zeros((5, 9), dtype=bool)), np.arange(45).reshape(5, 9))


def test_restated_rule_reproduces_the_references_fill_depth():
    g = load_golden("g24_depth_fill")
    names = [str(n) for n in g["fill_names"]]
    assert names == [name for name, _ in ref.fill_cases()]
    for k, (name, invalid) in enumerate(ref.fill_cases()):
        H, W = (int(v) for v in g[f"fill{k}_shape"])
        stored = np.unpackbits(g[f"fill{k}_invalid"], axis=-1, count=W).astype(bool)
        assert np.array_equal(stored, invalid), name                          # the generators still make the golden's inputs
        depth = g[f"fill{k}_depth"]
        assert np.array_equal(depth, ref.unique_depth(H, W, 1000 + k)) and np.unique(depth).size == H * W
        got = depth.ravel()[ref.nearest_valid_index(invalid)]
        assert np.array_equal(got, g[f"fill{k}_filled"]), name


def test_restated_metrics_reproduce_the_references_values():
    """float32 pairwise means (the reference) against float64 sums of the same float32 terms: the pairwise error is bounded by about
    2^-24 log2 n ~ 1e-6; the tolerance is 1e-5 (measured 8.5e-8)."""
    g = load_golden("g24_depth_fill")
    estimate, target, valid = ref.metric_scene()
    assert np.array_equal(estimate, g["metric_estimate"]) and np.array_equal(target, g["metric_target"])
    assert np.array_equal(valid, np.unpackbits(g["metric_valid"], axis=-1, count=valid.shape[-1]).astype(bool))
    assert np.isinf(target[~valid]).all()
    for b in range(len(valid)):
        got, want = ref.metrics(estimate[b], target[b], valid[b]), g["metric_values"][b]
        if valid[b].any():
            np.testing.assert_allclose(got, want, rtol=1e-5)
        else:
            assert got[0] == want[0] == 0 and np.isnan(got[1:]).all() and np.isnan(want[1:]).all()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for cite in ("depth_completion/fill_in_tools.py:5-7", "depth_completion/void.py:7-65", "evaluate_void.py:122-146"):
        assert cite in header, cite
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name


def test_size_queries_and_argument_checks():
    """Everything the entry points refuse is refused before any device work, so this runs without a GPU."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    assert lib.sp_depth_fill_workspace_bytes(1, 480, 640) >= 2 * 480 * 640           # one int16 row offset per pixel
    assert lib.sp_depth_fill_workspace_bytes(64, 480, 640) >= 64 * 2 * 480 * 640
    assert lib.sp_depth_fill_workspace_bytes(1, 1, 7) >= 14
    assert lib.sp_depth_metrics_workspace_doubles(3, 33, 65) >= 3 * 12
    assert lib.sp_depth_metrics_workspace_doubles(1, 480, 640) * 8 < 480 * 640       # partial sums, not a per-pixel array
    for query in (lib.sp_depth_fill_workspace_bytes, lib.sp_depth_metrics_workspace_doubles):
        assert query(0, 8, 8) == query(1, 0, 8) == query(1, 8, -1) == -1
        assert query(1, 32768, 8) == query(1, 8, 32768) == query(70000, 8, 8) == query(4, 32767, 32767) == -2
        assert query(1, 32767, 32767) > 0
    one = ctypes.c_void_p(16)                                                        # any non-null address: never dereferenced
    other = ctypes.c_void_p(32)
    fill, score = lib.sp_depth_fill_nearest, lib.sp_depth_metrics
    assert fill(None, one, 1, 8, 8, one, other, None, one, None) == -1
    assert fill(one, None, 1, 8, 8, one, other, None, one, None) == -1
    assert fill(one, one, 1, 8, 8, None, other, None, one, None) == -1
    assert fill(one, one, 1, 8, 8, one, None, None, one, None) == -1
    assert fill(one, one, 1, 8, 8, one, other, None, None, None) == -1
    assert fill(one, one, 1, 8, 8, one, one, None, one, None) == -1                  # filled must not be depth itself
    assert fill(one, one, 0, 8, 8, one, other, None, one, None) == -1
    assert fill(one, one, 1, -3, 8, one, other, None, one, None) == -1
    assert fill(one, one, 1, 8, 40000, one, other, None, one, None) == -2
    assert score(None, one, one, 1, 8, 8, one, one, None) == -1
    assert score(one, None, one, 1, 8, 8, one, one, None) == -1
    assert score(one, one, None, 1, 8, 8, one, one, None) == -1
    assert score(one, one, one, 1, 8, 8, None, one, None) == -1
    assert score(one, one, one, 1, 8, 8, one, None, None) == -1
    assert score(one, one, one, 1, 8, 0, one, one, None) == -1
    assert score(one, one, one, 1, 40000, 8, one, one, None) == -2


def test_host_inputs_are_refused():
    from super_primitive_amd.depth_completion import fill_in_tools, void
    depth, invalid = torch.ones(4, 6), torch.zeros(4, 6, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="HIP-only"):
        fill_in_tools.fill_depth(depth, invalid)
    with pytest.raises(RuntimeError, match="HIP-only"):
        fill_in_tools.fill_depth(depth.numpy(), invalid.numpy())
    with pytest.raises(RuntimeError, match="HIP-only"):
        fill_in_tools.nearest_valid_index(invalid)
    with pytest.raises(RuntimeError, match="HIP-only"):
        fill_in_tools.nearest_valid_index(invalid.numpy())
    with pytest.raises(RuntimeError, match="HIP-only"):
        void.ErrorMetrics().compute(depth, depth, ~invalid)
    with pytest.raises(RuntimeError, match="HIP-only"):
        void.ErrorMetricsDeltas().compute(depth.numpy(), depth.numpy(), ~invalid.numpy())
    assert not hasattr(fill_in_tools, "fill_single_griddata")


def test_metric_objects_before_compute_read_as_the_references_initial_values():
    from super_primitive_amd.depth_completion import void
    m = void.ErrorMetricsDeltas()
    assert all(getattr(m, n) == np.inf for n in ("rmse", "mae", "absrel", "inv_rmse", "inv_mae", "inv_absrel"))
    assert (m.delta0, m.delta1, m.delta2, m.delta3) == (0, 0, 0, 0)
    for avg in (void.ErrorMetricsAverager(), void.ErrorMetricsDeltasAverager()):
        assert avg.total_count == 0 and avg.rmse_avg == 0 and avg.inv_absrel_avg == 0
        with pytest.raises(ZeroDivisionError):
            avg.average()
    assert void.ErrorMetricsDeltasAverager().delta105_avg == 0
    with pytest.raises(AssertionError):
        void.ErrorMetricsDeltasAverager().accumulate(void.ErrorMetrics())


def test_reference_module_paths_resolve_to_the_device_modules():
    import super_primitive_amd
    from super_primitive_amd.depth_completion import evaluate, fill_in_tools, void
    saved = dict(sys.modules)
    try:
        super_primitive_amd.install_as_reference_modules()
        import depth_completion.fill_in_tools as theirs_fill
        import depth_completion.void as metrics
        import depth_completion.evaluate as theirs_eval
        assert theirs_fill is fill_in_tools and metrics is void and theirs_eval is evaluate
        for name in ("ErrorMetrics", "ErrorMetricsDeltas", "ErrorMetricsAverager", "ErrorMetricsDeltasAverager"):
            assert hasattr(metrics, name), name
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)
