"""Per-segment depth from surface normals -- the reference's ``frontend/normals/normals_integration.py`` API without cupy.

The reference hands normals, intrinsics and the (N,H,W) mask stack to ``normal_integration_batch_cupy``, a batched
conjugate-gradient solver of a submodule its tree does not carry.  Here the same stage runs in one native call
(``sp_normal_integration``): one workgroup per segment builds the masked stencil of the segment's tight box and runs its
CG to the segment's own stopping point.  The arithmetic is the definition in DESIGN.md §4 "Normal integration"; the
result is right up to one constant per connected component of a mask (zero-mean ``log depth`` on each), which
``kf_fix_disconnected_regions`` and the keypoint log-depths absorb afterwards.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib


def _u8(mask):
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    return (mask > 0).contiguous().view(torch.uint8)


def _device_K(K, device):
    K = torch.as_tensor(np.asarray(K, dtype=np.float32)) if not torch.is_tensor(K) else K
    return K.detach().to(device=device, dtype=torch.float32).reshape(3, 3).contiguous()


def integrate_normals(normals, K, masks, *, boxes=None, cg_max_iter=1000, cg_tol=1e-3, return_info=False):
    """(N,H,W) float32 depth ``exp(u)`` on every mask, 0 elsewhere, from ``normals`` (H,W,3) and ``masks`` (N,H,W).

    ``boxes``: optional (N,4) int32 ``{row0, col0, row1, col1}`` hint (``KeyFrame.segment_boxes``); results do not depend on it.
    ``return_info``: also the (N,2) float32 ``{iterations used, final recursive |r| / |b|}`` of every segment."""
    _lib.require_device(normals, masks, boxes)
    lib = _lib.load()
    dev = masks.device
    N, H, W = masks.shape
    if tuple(normals.shape) != (H, W, 3):
        raise ValueError(f"normals must be (H,W,3) = ({H},{W},3), got {tuple(normals.shape)}")
    nrm = normals.detach().to(device=dev, dtype=torch.float32).contiguous()
    Kd = _device_K(K, dev)
    m8 = _u8(masks.detach())
    bx = None if boxes is None else boxes.detach().to(device=dev, dtype=torch.int32).contiguous()
    depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    info = torch.empty(N, 2, dtype=torch.float32, device=dev)
    if N == 0:
        return (depth, info) if return_info else depth
    stream = _lib.stream_ptr()
    # size the vectors by the segments' tight boxes (one 8-byte read-back) instead of N full frames
    words = lib.sp_normal_integration_plan_words(N)
    _lib.check(min(words, 0), "sp_normal_integration_plan_words")
    plan = torch.empty(words, dtype=torch.int32, device=dev)
    _lib.check(lib.sp_normal_integration_plan(_lib.ptr(m8), _lib.ptr(bx), N, H, W, _lib.ptr(plan), stream), "sp_normal_integration_plan")
    n_floats = words + int(plan[:2].view(torch.int64).item())
    scratch = torch.empty(n_floats, dtype=torch.float32, device=dev)
    _lib.check(lib.sp_normal_integration(_lib.ptr(nrm), _lib.ptr(Kd), _lib.ptr(m8), _lib.ptr(bx), N, H, W, int(cg_max_iter), float(cg_tol),
                                         0, _lib.ptr(scratch), n_floats, _lib.ptr(depth), _lib.ptr(info), stream), "sp_normal_integration")
    return (depth, info) if return_info else depth


def run_tiled_normal_integration(normals, intrinsics, mask, down_scale=1, cg_max_iter=1000, cg_tol=1e-3):
    """normals_integration.py:7-28: rows / columns ``::down_scale`` of normals and masks, ``fx, fy, cx, cy`` divided by it
    (tool/camera.py instrinsic_scaled_K), the integrated depth expanded into a float (N,h,w) stack that is 0 off the masks."""
    _lib.require_device(normals, mask)
    K = _device_K(intrinsics, mask.device).clone()
    s = int(down_scale)
    K[:2] = K[:2] / s
    normals = normals[::s, ::s]
    mask = mask[:, ::s, ::s]
    return integrate_normals(normals, K, mask > 0 if mask.dtype != torch.bool else mask, cg_max_iter=cg_max_iter, cg_tol=cg_tol)
