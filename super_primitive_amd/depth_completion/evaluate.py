"""The scoring loop of the reference's ``evaluate_void.py:87-160`` over samples already in memory.

Per sample: the target's evaluation mask (``:113-116``), the completion with its fill (``:122-125``, nearest-valid fill in place
of griddata + nearest: DESIGN.md §8), the filled map scored over the mask and the partial map over ``mask & depth > 1e-6``
(``:138-155``), the validity rate (``:158``).  Every score stays on the device; the host reads once, after the last sample."""
from __future__ import annotations

import numpy as np
import torch

from . import void


class CompletionScores:
    """``filled`` / ``partial``: averaged ``ErrorMetricsDeltasAverager`` (the reference's two tables, plus the delta columns);
    ``validity_rates``: float64 array, one per sample."""

    def __init__(self, filled, partial, validity_rates):
        self.filled, self.partial, self.validity_rates = filled, partial, validity_rates


def evaluate_completion(dc, samples, min_depth=0.2, max_depth=5.0):
    """``dc``: a ``DepthCompletion``; ``samples``: iterable of ``(image, K, sparse_depth, target_depth)`` with ``sparse_depth`` what
    ``depth_completion`` takes and ``target_depth`` an (H,W) float tensor or array (<= 0 where there is no ground truth)."""
    filled_avg, partial_avg = void.ErrorMetricsDeltasAverager(), void.ErrorMetricsDeltasAverager()
    rates = []
    for image, K, sparse, target in samples:
        filled, depth, invalid = dc.depth_completion_dense(image, K, sparse)
        target = torch.as_tensor(target).to(device=depth.device, dtype=torch.float32)
        mask = target < max_depth
        if min_depth is not None:
            mask &= target > min_depth
        target = torch.where(mask, target, torch.full_like(target, float("inf")))
        covered = depth > 1e-6
        for avg, estimate, valid in ((filled_avg, filled, mask), (partial_avg, depth, covered & mask)):
            err = void.ErrorMetricsDeltas()
            err.compute(estimate, target, valid)
            avg.accumulate(err)
        rates.append(covered.sum().double() / covered.numel())
    if not rates:
        raise ValueError("evaluate_completion needs at least one sample")
    filled_avg.average()
    partial_avg.average()
    host = torch.cat([filled_avg._values, partial_avg._values, torch.stack(rates)]).tolist()      # the one host read
    k = len(void._COLUMNS)
    filled_avg._host, partial_avg._host = host[:k], host[k:2 * k]
    return CompletionScores(filled_avg, partial_avg, np.asarray(host[2 * k:], dtype=np.float64))
