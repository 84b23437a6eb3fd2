"""A keyframe from masks and normals: the network-free part of the reference's ``FrontProcessorNew.process_to_kf``
(``frontend/process_frame.py:78-92,231-250``), and -- ``keyframe_from_sam`` -- of its ``infer_masks`` / ``preprocess`` (``:94-154``) in front
of it.  The SAM network and the normals network stay out of scope; with their raw outputs at hand, this is what a ``to_keyframe``
callback of ``run_sequence`` or ``DepthCompletion``'s ``front_processor`` is built from.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib
from ..image.keyframe import KeyFrame, put_keypoints_back
from ..optim.batch_prepare import segment_boxes_of
from .normals.normals_integration import _device_K, integrate_normals
from .segment.mask_generation import infer_masks
from .segment.post_processer import kf_fix_disconnected_regions
from ..tool.point_utils import img_to_np


def keyframe_from_normals(image, K, normals, masks, keypoints, *, cg_max_iter=1000, cg_tol=1e-3, split_disconnected=True,
                          depth_disc_params=None):
    """``KeyFrame`` of ``image`` (C,H,W) with intrinsics ``K`` from ``normals`` (h,w,3), ``masks`` (N,h,w) and normalised (row, col)
    ``keypoints`` (N,2).  (h,w) is the integration size; when it differs from (H,W) the intrinsics are scaled to it for the
    integration and the integrated depth is brought to (H,W) by nearest resize, as process_frame.py:132-134,231-233 do.

    process_frame.py:234-250: ``masks = depth > 1e-7``, ``put_keypoints_back``, ``log``, ``KeyFrame``, then -- with
    ``split_disconnected`` -- ``kf_fix_disconnected_regions`` (``depth_disc_params``: its ``filter_size``, ``depth_threshold``,
    ``area_keep_ratio``).  ``segment_boxes`` of the result is filled in."""
    with torch.no_grad():
        H, W = image.shape[-2:]
        h, w = masks.shape[-2:]
        dev = masks.device
        K_kf = _device_K(K, dev)
        K_geom = K_kf.clone()
        K_geom[0] = K_geom[0] * (w / W)
        K_geom[1] = K_geom[1] * (h / H)
        depth = integrate_normals(normals, K_geom, masks, cg_max_iter=cg_max_iter, cg_tol=cg_tol)
        if (h, w) != (H, W):
            depth = F.interpolate(depth[:, None], size=(H, W), mode='nearest')[:, 0]
        regions = depth > 1e-7
        keypoints, regions, depth = put_keypoints_back(keypoints.to(dev), regions, depth)
        logdepth = torch.where(regions, torch.log(depth.clamp_min(1e-30)), torch.zeros_like(depth))
        kf = KeyFrame(image, K=K_kf, logdepth_perseg=logdepth, keypoints=keypoints, keypoint_regions=regions)
        if split_disconnected:
            kf = kf_fix_disconnected_regions(kf, **(depth_disc_params or {}))
        kf.segment_boxes = segment_boxes_of(kf.keypoint_regions)
    return kf


def _nearest_masks(masks, size):
    return masks if tuple(masks.shape[-2:]) == tuple(size) else F.interpolate(masks.float()[:, None], size=tuple(size), mode='nearest')[:, 0] > 0.5


def keyframe_from_sam(image, K, normals, sam_model, sam_config, *, num_pts, num_pts_active, integration_shape, infer_resolution=None,
                      keypoints=None, **keyframe_from_normals_kwargs):
    """``KeyFrame`` of ``image`` (3,H,W) from SAM's raw outputs and ``normals`` (h,w,3), (h,w) = ``integration_shape``: the
    network-free part of process_frame.py:94-154.  The image is brought to ``infer_resolution`` (bilinear) for ``sam_model`` when one
    is given, ``infer_masks`` runs there with ``edge_probs_shape=integration_shape``, its masks come back to (H,W) and go on to
    ``integration_shape`` by nearest resize, and ``keyframe_from_normals`` does the rest (it takes the remaining keyword arguments).
    ``sam_model``: a SamPredictor-like object (it is handed the image as (H,W,3) uint8 on the host, as the reference hands it) or a
    callable ``(image (H,W,3) device tensor, keypoints) -> {'masks', 'iou_pred'}``."""
    _lib.require_device(image, normals, keypoints)
    with torch.no_grad():
        H, W = image.shape[-2:]
        sam_image = image if infer_resolution is None else F.interpolate(image[None], size=tuple(infer_resolution), mode='bilinear')[0]
        sam_image = img_to_np(sam_image) if hasattr(sam_model, "predict_torch") else sam_image.permute(1, 2, 0)
        found = infer_masks(sam_model, sam_image, sam_config, keypoints=keypoints, num_pts=num_pts, num_pts_active=num_pts_active,
                            edge_probs_shape=tuple(integration_shape), device=image.device)
        masks = found['masks']['masks']
        if masks.shape[0] == 0:
            raise ValueError("keyframe_from_sam: no mask survived the selection")
        masks = _nearest_masks(_nearest_masks(masks, (H, W)), integration_shape)
    return keyframe_from_normals(image, K, normals, masks, found['keypoints'], **keyframe_from_normals_kwargs)
