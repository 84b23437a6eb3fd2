"""Fill uncovered depth pixels from their nearest covered ones -- the reference's ``depth_completion/fill_in_tools.py`` API.

``fill_depth`` (``:5-7``) is ``depth[distance_transform_edt(invalid, return_indices=True)]``.  Here it is one native call
(``sp_depth_fill_nearest``) that names the same source pixel as scipy for every pixel, ties included: the valid pixel that
minimises ``(d^2, column, row)`` (DESIGN.md §4 "Depth fill").  ``fill_single_griddata`` (``:9-21``) is not provided: its first
stage is a Qhull Delaunay triangulation of lattice points, and which triangles Qhull picks among co-circular pixels is not a
definition."""
from __future__ import annotations

import torch

from .. import _lib


def _fill(depth, invalid_mask, want_index):
    for t in (depth, invalid_mask):
        if t is not None and not torch.is_tensor(t):
            raise RuntimeError("super_primitive_amd: the depth fill is HIP-only; got a host array. Pass cuda tensors (no CPU fallback exists).")
    _lib.require_device(depth, invalid_mask)
    lib = _lib.load()
    single = invalid_mask.dim() == 2
    inv = invalid_mask.detach()
    inv = (inv if inv.dtype == torch.bool else inv != 0).contiguous().view(torch.uint8)
    if single:
        inv = inv[None]
    if inv.dim() != 3:
        raise ValueError(f"invalid_mask must be (H,W) or (B,H,W), got {tuple(invalid_mask.shape)}")
    B, H, W = inv.shape
    dev = inv.device
    if depth is None:
        d = torch.zeros(B, H, W, dtype=torch.float32, device=dev)
    else:
        if tuple(depth.shape) != tuple(invalid_mask.shape):
            raise ValueError(f"depth {tuple(depth.shape)} and invalid_mask {tuple(invalid_mask.shape)} differ in shape")
        d = depth.detach().to(torch.float32).contiguous().view(B, H, W)
    n_bytes = lib.sp_depth_fill_workspace_bytes(B, H, W)
    _lib.check(min(n_bytes, 0), "sp_depth_fill_workspace_bytes")
    workspace = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    filled = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    index = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_index else None
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    _lib.check(lib.sp_depth_fill_nearest(_lib.ptr(d), _lib.ptr(inv), B, H, W, _lib.ptr(workspace), _lib.ptr(filled), _lib.ptr(index),
                                         _lib.ptr(counts), _lib.stream_ptr()), "sp_depth_fill_nearest")
    if single:
        filled, counts = filled[0], counts[0]
        index = None if index is None else index[0]
    return filled, index, counts


def fill_depth(depth, invalid_mask, return_counts=False):
    """``depth`` with every pixel of ``invalid_mask`` replaced by its nearest valid pixel's value; (H,W) or (B,H,W) cuda tensors.
    An image without a valid pixel comes back unchanged.  ``return_counts``: also the int32 ``{valid pixels, pixels filled}`` of
    every image ((2,) or (B,2), on the device)."""
    filled, _, counts = _fill(depth, invalid_mask, False)
    return (filled, counts) if return_counts else filled


def nearest_valid_index(invalid_mask):
    """int32 flat index ``r' * W + c'`` of the pixel ``fill_depth`` copies from, for every pixel; valid pixels name themselves."""
    return _fill(None, invalid_mask, True)[1]
