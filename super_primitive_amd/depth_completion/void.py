"""VOID error metrics on the device -- the reference's ``depth_completion/void.py`` classes and attribute names.

``compute(estimate, target, valid)`` is one native call (``sp_depth_metrics``): per-pixel terms in fp32 exactly as numpy forms
them (``void.py:7-43,52-65``), summed in fp64 in a fixed order.  The twelve values of an image stay on the device until an
attribute is first read; the averagers add device tensors, so a scoring loop reads the host once, at its end."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib

# columns of sp_depth_metrics' output (include/sp_hip.h)
_COLUMNS = ("n", "rmse", "mae", "absrel", "inv_rmse", "inv_mae", "inv_absrel", "delta105", "delta110", "delta1", "delta2", "delta3")
_COL = {name: k for k, name in enumerate(_COLUMNS)}
_COL["delta0"] = _COL["delta110"]                 # void.py:34 a0 is a10


def depth_metrics(estimate, target, valid):
    """(B,12) float64 device tensor ``{n, rmse, mae, absrel, inv_rmse, inv_mae, inv_absrel, fractions below 1.05, 1.10, 1.25,
    1.25^2, 1.25^3}`` of (B,H,W) (or (H,W): B = 1) cuda tensors; pixels outside ``valid`` are never read into a sum."""
    for t in (estimate, target, valid):
        if not torch.is_tensor(t):
            raise RuntimeError("super_primitive_amd: the depth metrics are HIP-only; got a host array. Pass cuda tensors (no CPU fallback exists).")
    _lib.require_device(estimate, target, valid)
    lib = _lib.load()
    if not (tuple(estimate.shape) == tuple(target.shape) == tuple(valid.shape)) or valid.dim() not in (2, 3):
        raise ValueError(f"estimate {tuple(estimate.shape)}, target {tuple(target.shape)} and valid {tuple(valid.shape)} must share one (H,W) or (B,H,W) shape")
    H, W = valid.shape[-2:]
    B = valid.numel() // (H * W) if H * W else 0
    dev = valid.device
    e = estimate.detach().to(torch.float32).contiguous()
    t = target.detach().to(torch.float32).contiguous()
    v = valid.detach()
    v = (v if v.dtype == torch.bool else v != 0).contiguous().view(torch.uint8)
    n = lib.sp_depth_metrics_workspace_doubles(B, H, W)
    _lib.check(min(n, 0), "sp_depth_metrics_workspace_doubles")
    workspace = torch.empty(n, dtype=torch.float64, device=dev)
    out = torch.empty(B, len(_COLUMNS), dtype=torch.float64, device=dev)
    _lib.check(lib.sp_depth_metrics(_lib.ptr(e), _lib.ptr(t), _lib.ptr(v), B, H, W, _lib.ptr(workspace), _lib.ptr(out), _lib.stream_ptr()),
               "sp_depth_metrics")
    return out


class _DeviceValues:
    """Twelve doubles on the device, read to the host once, on the first attribute that needs them."""
    _values = None          # (12,) float64 device tensor
    _host = None

    def _read(self, name, default):
        if self._values is None:
            return default
        if self._host is None:
            self._host = self._values.tolist()
        return self._host[_COL[name]]


def _metric(name, default):
    return property(lambda self: self._read(name, default))


class ErrorMetrics(_DeviceValues):
    """void.py:46-65.  Before ``compute`` every metric reads as the reference's worst value, inf."""
    rmse, mae, absrel = _metric("rmse", np.inf), _metric("mae", np.inf), _metric("absrel", np.inf)
    inv_rmse, inv_mae, inv_absrel = _metric("inv_rmse", np.inf), _metric("inv_mae", np.inf), _metric("inv_absrel", np.inf)

    def compute(self, estimate, target, valid):
        values = depth_metrics(estimate, target, valid)
        if len(values) != 1:
            raise ValueError("compute scores one (H,W) image; depth_metrics takes a batch")
        self._values, self._host = values[0], None


class ErrorMetricsDeltas(ErrorMetrics):
    """void.py:67-97: the same six and the fractions of max(t / e, e / t) below 1.10, 1.25, 1.25^2, 1.25^3, 1.05, 1.10."""
    delta0, delta1, delta2, delta3 = _metric("delta0", 0), _metric("delta1", 0), _metric("delta2", 0), _metric("delta3", 0)
    delta105, delta110 = _metric("delta105", 0), _metric("delta110", 0)


class _Averager(_DeviceValues):
    _accepts = ErrorMetrics

    def __init__(self):
        self.total_count = 0

    def accumulate(self, error_metrics):
        assert isinstance(error_metrics, self._accepts)
        if error_metrics._values is None:
            raise RuntimeError("accumulate() needs metrics that compute() has filled")
        self._values = error_metrics._values.clone() if self._values is None else self._values + error_metrics._values
        self._host = None
        self.total_count += 1

    def average(self):
        if self._values is None:
            raise ZeroDivisionError("average() of no metrics")
        self._values, self._host = self._values / self.total_count, None


def _average(name):
    return property(lambda self: self._read(name, 0))


class ErrorMetricsAverager(_Averager):
    """void.py:100-129: ``*_avg`` hold running sums until ``average()`` divides them by ``total_count``."""
    rmse_avg, mae_avg, absrel_avg = _average("rmse"), _average("mae"), _average("absrel")
    inv_rmse_avg, inv_mae_avg, inv_absrel_avg = _average("inv_rmse"), _average("inv_mae"), _average("inv_absrel")


class ErrorMetricsDeltasAverager(ErrorMetricsAverager):
    """void.py:134-182."""
    _accepts = ErrorMetricsDeltas
    delta0_avg, delta1_avg, delta2_avg, delta3_avg = _average("delta0"), _average("delta1"), _average("delta2"), _average("delta3")
    delta105_avg, delta110_avg = _average("delta105"), _average("delta110")
