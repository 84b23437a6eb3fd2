"""From SAM's raw output to the ``(masks, keypoints)`` of a keyframe -- the reference's ``frontend/segment/mask_generation.py`` API.

The network stays the caller's (``sam_model``); everything behind it runs on the device: one pass over the 3n logit maps for
the stability counts, sizes and boxes (``sp_sam_candidate_stats``), the rules on the (n,3) tables as torch ops on device tensors,
greedy box NMS (``sp_box_nms``), the masks of the survivors only (``sp_sam_build_masks``), the edge map (``sp_mask_edges``) and the
cut / keypoint filter (``sp_sam_cut_masks``).  The semantics -- the helpers of ``segment_anything.utils.amg`` and ``torchvision.ops``
included -- are written out in DESIGN.md §4 "SAM mask selection".  One host read per data-dependent size: the survivors of the
thresholds, of NMS and of the keypoint filter."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ... import _lib
from ...tool import point_utils

_MASK_THRESH = 0.0           # model_mask_thresh (mask_generation.py:27)
_STABILITY_OFFSET = 1.0      # stability_score_offset (:26)
_NO_GOOD_MASK = 1000000      # the size a mask that failed a test is given (:73)


def _device_tensors(*tensors):
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise RuntimeError("super_primitive_amd: the SAM mask selection is HIP-only; got a host array. Pass cuda tensors (no CPU fallback exists).")
    _lib.require_device(*tensors)


def candidate_stats(logits, thresh=_MASK_THRESH, offset=_STABILITY_OFFSET):
    """(M,8) int32 of (M,H,W) float logits: ``#(x > thresh+offset), #(x > thresh-offset), #(x > thresh), left, top, right, bottom, 0``
    (the box is over ``x > thresh``; zeros when empty).  One read of the logits."""
    _device_tensors(logits)
    if logits.dim() != 3:
        raise ValueError(f"logits must be (M,H,W), got {tuple(logits.shape)}")
    x = logits.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    M, H, W = x.shape
    stats = torch.empty(M, 8, dtype=torch.int32, device=x.device)
    if M:
        _lib.check(_lib.load().sp_sam_candidate_stats(_lib.ptr(x), M, H, W, thresh, offset, _lib.ptr(stats), _lib.stream_ptr()),
                   "sp_sam_candidate_stats")
    return stats


def box_nms(boxes, scores, iou_threshold):
    """``batched_nms`` with one category: the kept indices (int64) in visiting order; equal scores visit the lower index first."""
    _device_tensors(boxes, scores)
    K = boxes.shape[0]
    keep = torch.empty(K, dtype=torch.int64, device=boxes.device)
    if K == 0:
        return keep
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    n_keep = torch.empty(1, dtype=torch.int32, device=boxes.device)
    _lib.check(_lib.load().sp_box_nms(_lib.ptr(b), _lib.ptr(s), K, float(iou_threshold), _lib.ptr(keep), _lib.ptr(n_keep), _lib.stream_ptr()),
               "sp_box_nms")
    return keep[:int(n_keep.item())]


def _build_masks(logits, cand, want_coverage):
    """bool (K,H,W) masks ``logits[cand] > 0`` of (M,H,W) logits and, asked for, their OR (H,W)."""
    M, H, W = logits.shape
    K = cand.shape[0]
    dev = logits.device
    masks = torch.empty(K, H, W, dtype=torch.uint8, device=dev)
    coverage = None
    if want_coverage:
        coverage = torch.empty(H, W, dtype=torch.uint8, device=dev) if K else torch.zeros(H, W, dtype=torch.uint8, device=dev)
    if K:
        c = cand.to(torch.int32).contiguous()
        _lib.check(_lib.load().sp_sam_build_masks(_lib.ptr(logits), _lib.ptr(c), K, M, H, W, _MASK_THRESH, _lib.ptr(masks), _lib.ptr(coverage),
                                                  _lib.stream_ptr()), "sp_sam_build_masks")
    return masks.view(torch.bool), None if coverage is None else coverage.view(torch.bool)


def _flat_logits(masks):
    if masks.dim() != 4 or masks.shape[1] != 3:
        raise ValueError(f"masks must be (n,3,H,W) logits, got {tuple(masks.shape)}")
    x = masks.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    return x.view(-1, x.shape[2], x.shape[3])


def _select(logits, iou_pred, iou_threshold, stability_score_thresh, select_smallest):
    """The rules of smallest_good_mask_batch on the (n,3) tables: which candidates survive (``cand``, indices into the 3n maps), with
    their fields -- everything but the masks themselves."""
    n = logits.shape[0] // 3
    stats = candidate_stats(logits).view(n, 3, 8)
    tests = []
    if iou_threshold > 0:
        tests.append(iou_pred > iou_threshold)
    if stability_score_thresh > 0:
        tests.append(stats[..., 0].float() / stats[..., 1].float() >= stability_score_thresh)      # 0 / 0 = NaN fails
    dev = logits.device
    if select_smallest:
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        good = torch.ones(n, 3, dtype=torch.bool, device=dev)
        for ok in tests:                                    # a keypoint survives a test when any of its masks passes it
            alive &= ok.any(dim=1)
            good &= ok
        size = torch.where(good, stats[..., 2], torch.full_like(stats[..., 2], _NO_GOOD_MASK))
        s0, s1, s2 = size.unbind(dim=1)
        first_min = torch.where((s0 <= s1) & (s0 <= s2), 0, torch.where(s1 <= s2, 1, 2))
        keypoints_ids = alive.nonzero()[:, 0]               # host read: the survivors of the thresholds
        masks_ids = first_min[keypoints_ids]
        cand = keypoints_ids * 3 + masks_ids
        out = {"iou_preds": iou_pred.reshape(-1)[cand], "keypoints_ids": keypoints_ids, "masks_ids": masks_ids}
    else:
        ok = torch.ones(n, 3, dtype=torch.bool, device=dev)
        for t in tests:
            ok &= t
        cand = ok.reshape(-1).nonzero()[:, 0]
        out = {"iou_preds": iou_pred.reshape(-1)[cand], "keypoints_ids": torch.div(cand, 3, rounding_mode="floor")}
    out["boxes"] = stats.view(-1, 8)[cand, 3:7].long()
    return cand, out


def _with_masks(masks, fields):
    out = {"masks": masks}
    out.update(fields)
    return out


def smallest_good_mask_batch(masks, iou_pred, iou_threshold=0.88, stability_score_thresh=0.95, select_smallest=True):
    """``masks`` (n,3,H,W) float logits, ``iou_pred`` (n,3).  A threshold ``<= 0`` switches its test off.  With ``select_smallest`` one
    mask per surviving keypoint -- the smallest that passed both tests, mask 0 when none did -- else every candidate that passed.
    Returns ``masks`` (K,H,W) bool, ``iou_preds``, ``keypoints_ids``, ``masks_ids`` (only with ``select_smallest``), ``boxes`` (K,4) XYXY."""
    _device_tensors(masks, iou_pred)
    with torch.no_grad():
        logits = _flat_logits(masks)
        cand, fields = _select(logits, iou_pred, iou_threshold, stability_score_thresh, select_smallest)
        return _with_masks(_build_masks(logits, cand, False)[0], fields)


def active_sample_pos(coverage_mask, num_samples=100, fine_noise=True):
    """``num_samples`` keypoints per image of ``coverage_mask`` (B,H,W) bool, drawn where 16x16 cells are least covered (the lowest two
    rows count as covered), then jittered inside the cell.  Consumes the generator as the reference does: ``Categorical.sample``,
    then ``randint_like``."""
    _device_tensors(coverage_mask)
    B, H, W = coverage_mask.shape
    cell = 16
    with torch.no_grad():
        covered = coverage_mask.clone()
        covered[:, -2:, :] = 1
        coarse = F.avg_pool2d(covered.float()[:, None], cell, stride=cell)
        Hc, Wc = coarse.shape[2:]
        density = 1.0 - coarse
        density = density / (density.sum(dim=(2, 3), keepdim=True) + 1e-6)
        flat = torch.distributions.Categorical(probs=density.view(B, -1)).sample((num_samples,)).view(num_samples, B)
        coarse_indices = torch.stack([flat // Wc, flat % Wc], dim=2).permute(1, 0, 2).reshape(B, num_samples, 2)
        coords = point_utils.normalise_coordinates(coarse_indices, (Hc, Wc))
        if fine_noise:
            jitter = torch.randint_like(coords, high=cell // 2, device=coverage_mask.device)
            coords = (coords + (point_utils.normalise_coordinates(jitter, (H, W)) + 1)).clamp(-1, 1)
        sample_indices = point_utils.denormalise_coordinates(coords, (H, W)).reshape(B, num_samples, 2)
    return {"coarse_density": density, "coarse_indices": coarse_indices, "sample_indices": sample_indices,
            "normalised_coords": coords.reshape(B, num_samples, 2)}


def _nearest_source_index(n_out, n_in, device):
    """The source index of every output index of a nearest resize, torch's rule: ``min(floor(i * float32(n_in / n_out)), n_in - 1)``."""
    if n_out == n_in:
        return None
    scale = torch.tensor(float(n_in), dtype=torch.float32, device=device) / n_out
    index = torch.floor(torch.arange(n_out, dtype=torch.float32, device=device) * scale)
    return index.clamp_(max=n_in - 1).to(torch.int32)


def _edge_maps(masks, shape, pool_edges):
    """edges, edge_probs (He,We) of bool masks (K,H,W) seen through a nearest resize to ``shape`` (None: as they are)."""
    K, H, W = masks.shape
    He, We = (H, W) if shape is None else (int(shape[0]), int(shape[1]))
    dev = masks.device
    if K == 0:                                              # no mask, no edge
        return torch.zeros(He, We, device=dev), torch.ones(He, We, device=dev)
    m = masks.detach()
    m = (m if m.dtype == torch.bool else m != 0).contiguous().view(torch.uint8)
    rows, cols = _nearest_source_index(He, H, dev), _nearest_source_index(We, W, dev)
    edges = torch.empty(He, We, dtype=torch.float32, device=dev)
    edge_probs = torch.empty(He, We, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().sp_mask_edges(_lib.ptr(m), K, H, W, _lib.ptr(rows), _lib.ptr(cols), He, We, _lib.ptr(edges), _lib.ptr(edge_probs),
                                         1 if pool_edges else 0, _lib.stream_ptr()), "sp_mask_edges")
    return edges, edge_probs


def masks_to_edges(masks):
    """Scharr/32 gradient magnitude (reflect padding) of every mask of (K,H,W), maximum over the masks."""
    _device_tensors(masks)
    return _edge_maps(masks, None, False)[0]


def infer_edge_probs(masks, pool_edges=False):
    """``edges`` (with ``pool_edges`` under a 3x3 maximum) and ``edge_probs = clip(1 - 2 edges, 0, 1)``."""
    _device_tensors(masks)
    return _edge_maps(masks, None, pool_edges)


def _run_sam(sam_model, image, keypoints):
    """The raw output of the network for normalised (row, col) ``keypoints``: a SamPredictor-like object is driven the way
    frontend/segment/sam_tools.py:20-45 drives it, anything else is called as ``sam_model(image, keypoints)``."""
    if hasattr(sam_model, "predict_torch"):
        sam_model.set_image(image)
        H, W = image.shape[:2]
        size = sam_model.transform.get_preprocess_shape(H, W, sam_model.transform.target_length)
        points = point_utils.denormalise_coordinates(keypoints, size).flip(-1)
        labels = torch.ones((keypoints.shape[0], 1), dtype=torch.int64, device=keypoints.device)
        masks, iou_pred, _ = sam_model.predict_torch(points[:, None], labels, multimask_output=True, return_logits=True)
        out = {"masks": masks, "iou_pred": iou_pred}
    else:
        out = sam_model(image, keypoints)
    _device_tensors(out["masks"], out["iou_pred"])
    return out


def _filter(fields, index):
    return {k: v[index] for k, v in fields.items()}


def _round(sam_model, image, keypoints, cfg, want_coverage):
    """One round of prompts: thresholds, optional NMS, then the masks of what is left (and their OR)."""
    raw = _run_sam(sam_model, image, keypoints)
    logits = _flat_logits(raw["masks"])
    cand, fields = _select(logits, raw["iou_pred"], cfg["iou_threshold"], cfg["stability_threshold"], cfg["select_smallest"])
    kept_keypoints = keypoints[fields["keypoints_ids"]]
    if cfg["nms"] and cand.shape[0]:
        boxes = fields["boxes"]
        scores = 1 / ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) if cfg["filter_by_box_size"] else fields["iou_preds"]
        keep = box_nms(boxes.float(), scores, cfg["box_nms_thresh"])      # host read: the survivors of NMS
        cand, fields, kept_keypoints = cand[keep], _filter(fields, keep), kept_keypoints[keep]
    masks, coverage = _build_masks(logits, cand, want_coverage)
    return _with_masks(masks, fields), kept_keypoints, coverage


def infer_masks(sam_model, image, sam_config, keypoints=None, num_pts=300, num_pts_active=50, edge_probs_shape=None, device=None, *,
                sampler=None):
    """Two rounds of SAM prompts (the given or random keypoints, then ``num_pts_active`` drawn where the first round left the image
    uncovered), each with its thresholds and NMS; then the edge map, the optional cut by it and the keypoint filter.  Returns the
    reference's ten keys; ``result['masks']`` is a dict of tensors.  ``sampler(coverage[None], num_pts_active)`` defaults to
    ``active_sample_pos``."""
    H, W = image.shape[:2]
    if torch.is_tensor(image):
        _lib.require_device(image)
    _device_tensors(keypoints)
    cfg = sam_config
    sampler = active_sample_pos if sampler is None else sampler
    with torch.no_grad():
        if keypoints is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
            keypoints = torch.rand(num_pts, 2, device=dev) * 2 - 1
        fields, keypoints_final, coverage = _round(sam_model, image, keypoints, cfg, True)
        sampled, num_added = None, 0
        if num_pts_active > 0:
            sampled = sampler(coverage[None], num_pts_active)
            more, keypoints_more, _ = _round(sam_model, image, sampled["normalised_coords"][0], cfg, False)
            num_added = keypoints_more.shape[0]
            keypoints_final = torch.cat([keypoints_final, keypoints_more], dim=0)
            fields = {k: torch.cat([v, more[k]], dim=0) for k, v in fields.items()}
        masks = fields["masks"]
        K = masks.shape[0]
        dev = masks.device

        edges_coarse, probs_coarse = _edge_maps(masks, edge_probs_shape, False)
        if edge_probs_shape is None:
            edges, edge_probs = edges_coarse, probs_coarse
        else:
            edges = F.interpolate(edges_coarse[None, None], size=(H, W), mode="bilinear", align_corners=True)[0, 0]
            edge_probs = F.interpolate(probs_coarse[None, None], size=(H, W), mode="bilinear", align_corners=True)[0, 0]

        cut, by_keypoint = bool(cfg["cut_masks_by_edges"]), bool(cfg["filter_edge_points"])
        final_coverage = torch.zeros(H, W, dtype=torch.bool, device=dev)
        if K:
            m8 = masks.view(torch.uint8)
            kp_rc = point_utils.denormalise_coordinates(keypoints_final, (H, W)).to(torch.int32).contiguous() if by_keypoint else None
            slot = torch.empty(K, dtype=torch.int32, device=dev)
            out = torch.empty_like(m8) if cut or by_keypoint else None
            probs = edge_probs.contiguous() if cut else None
            _lib.check(_lib.load().sp_sam_cut_masks(_lib.ptr(m8), K, H, W, _lib.ptr(probs), float(cfg["edge_probs_threshold"]), _lib.ptr(kp_rc),
                                                    _lib.ptr(slot), _lib.ptr(out), _lib.ptr(final_coverage.view(torch.uint8)),
                                                    _lib.stream_ptr()), "sp_sam_cut_masks")
            if by_keypoint:
                kept = (slot >= 0).nonzero()[:, 0]          # host read: the survivors of the keypoint filter
                fields = _filter(fields, kept)
                fields["masks"] = out[:kept.shape[0]].view(torch.bool)
                keypoints_final = keypoints_final[kept]
            elif cut:
                fields["masks"] = out.view(torch.bool)
    return {"masks": fields, "keypoints": keypoints_final, "num_active": num_added, "coarse_coverage": coverage,
            "final_coverage": final_coverage, "sampled_masks": sampled, "edges": edges, "edge_probs": edge_probs,
            "edge_coarse": edges_coarse, "edge_probs_coarse": probs_coarse}
